"""The material step on the adversarial cases of tests/bsdf_cases.py (CPU): the oracle against the float64 restatement of the reference's
formulas, and the oracle against the reference's own kernels (oracle/_ref, `ref` marker) on every case.

Printed: decided / undecided counts per (BSDF, case group).  A case is decided when fp32 can still be held to float64 there (the classifier
in bsdf_cases.py); the undecided ones are mostly the crafted ones: draws one ulp from the Fresnel threshold, exactly grazing directions,
lobes too sharp for fp32 (Ns >= 1e5) and values past the fp32 range."""
import functools
import numpy as np
import pytest
import bsdf_cases as bc
import common
from common import COL
from fluctus_amd import driver
from oracle.binding import OracleContext, ref_available

# the least decided share per case group (every BSDF type): what the classifier decides today, with room; the 'fresnel' group is one ulp
# from the threshold by construction (parity only)
MIN_DECIDED = {"material": 0.6, "geometry": 0.35, "draws": 0.45, "uv": 0.95, "random": 0.6, "fresnel": 0.0}


@functools.lru_cache(maxsize=1)
def cases():
    cs = bc.CaseSet()
    return cs, bc.Verdict(cs.restatement(), cs.case)


def run(ctx_cls, cs, separate=True, **kw):
    d = cs.scene()
    c = ctx_cls(cs.n, **kw)
    try:
        c.upload_scene(d)
        c.set_params(bc.params(d, separate))
        driver.reset_renderer(c)
        bc.load(c, cs, bc.queues_of(cs, separate=separate))
        c.wf_materials()
        cnt = np.array(c.get_counters(), copy=True)
        ext = c.queue_read(common.Q.EXTENSION)[:int(cnt[common.Q.EXTENSION])].copy()
        return c.state_export().copy(), cnt, ext
    finally:
        c.close()


def test_counts_printed_and_decided_share():
    cs, v = cases()
    lines, short = [], []
    for t in bc.TYPES:
        for g in MIN_DECIDED:
            m = (cs.type == t) & (cs.group == g)
            if not m.any():
                continue
            nd = int(v.decided[m].sum())
            lines.append(f"{bc.TYPE_NAMES[t]:>10} {g:>9}: {nd:5d} decided {int(m.sum()) - nd:5d} undecided")
            if nd < MIN_DECIDED[g] * m.sum():
                short.append(lines[-1])
    print("\n" + "\n".join(lines) + f"\n     total: {int(v.decided.sum())} decided of {cs.n}")
    assert not short, "decided share below the minimum: " + "; ".join(short)
    assert set(np.unique(cs.group)) == set(MIN_DECIDED)


def test_seed_helpers():
    s = np.arange(0, 2 ** 32, 2 ** 32 // 4099, dtype=np.uint64)
    assert np.array_equal(bc.unhash_u32(bc.hash_u32(s)), s)
    from oracle.binding import lib
    L = lib()
    for x in (0, 1, 61, 0xFFFFFFFF, 0x12345678):
        assert L.orc_hash(x) == int(bc.hash_u32(np.array([x], np.uint64))[0])
    for k in (1, 2, 3):
        for val in (0.0, 1.0, 0.5, float(np.nextafter(np.float32(0.5), np.float32(1)))):
            s = np.array([bc.seed_for_draw(k, val)], np.uint64)
            for _ in range(k):
                r, s = bc.rand01(s)
            assert r[0] == val


def test_texel_coordinates_in_bounds():
    """The uv cases' texel math (the restatement of csrc/flx_shading.h texel_coord) stays in bounds, its int conversions are defined, and
    the chosen wrap holds: unsigned modulo through 2^32 for floor < 0, floor modulo 2^32 past 2^31, coordinate 0 for inf / NaN."""
    cs, _ = cases()
    for k, (w, h) in enumerate(bc.TEX_SIZES):
        for n in (w, h):
            x = (cs.case.uv.astype(np.float32) * np.float32(n)).reshape(-1)
            c = bc.texel_coord(x, n)
            assert ((c >= 0) & (c < n)).all()
    assert bc.texel_coord(np.float32(-0.9), 3) == 0                  # (uint)(-1) % 3 = 0, not the signed 2
    assert bc.texel_coord(np.float32(-0.9), 16) == 15
    assert bc.texel_coord(np.float32(-2.5), 5) == (2 ** 32 - 3) % 5
    assert bc.texel_coord(np.float32(3e9), 3) == 0 and bc.texel_coord(np.float32(2.0 ** 31 + 256), 4096) == 256
    for x in (np.inf, -np.inf, np.nan, 1e30):
        assert bc.texel_coord(np.float32(x), 7) == 0


def test_oracle_seed_stream_and_float64():
    """Every case: the seed stream as the restatement's (exact), lastSpecular, lastT = T in; decided cases within the derived tolerance of
    float64.  Separate queues and the single queue give the same state."""
    cs, v = cases()
    st, cnt, ext = run(OracleContext, cs, threads=8)
    u = st.view(np.uint32)
    assert np.array_equal(u[COL.SEED, :cs.n], v.seed), "seed stream differs from the restatement"
    assert np.array_equal(u[COL.LAST_SPECULAR, :cs.n], v.singular)
    assert np.array_equal(st[COL.LAST_T:COL.LAST_T + 3, :cs.n].T, cs.case.T.astype(np.float32))
    assert cnt[common.Q.EXTENSION] == cs.n and np.array_equal(np.sort(ext), np.arange(cs.n))
    fails = v.check(st)
    assert not fails, "; ".join(fails)
    st1, cnt1, ext1 = run(OracleContext, cs, separate=False, threads=8)
    assert not common.state_diff(st1[:, :cs.n], st[:, :cs.n], 0.0, 0.0)
    assert np.array_equal(ext1, np.arange(cs.n))


@pytest.mark.ref
@pytest.mark.skipif(not ref_available(), reason="oracle/_ref not built (needs /root/reference)")
def test_oracle_vs_reference_kernels():
    """Every case through the reference's own wf_mat_*.cl kernels: integers exact, decided floats within the derived tolerance of the
    oracle, the larger undecided gaps printed.  pdfW is masked where the reference leaves it undefined (glossy's rejected sample, T = 0)."""
    from oracle.binding import RefContext
    cs, v = cases()
    so, co, eo = run(OracleContext, cs, threads=8)
    sr, cr, er = run(RefContext, cs)
    assert np.array_equal(co, cr)
    assert np.array_equal(np.sort(eo), np.sort(er))
    n = cs.n
    for c in common.INT_COLS:
        bad = so.view(np.uint32)[c, :n] != sr.view(np.uint32)[c, :n]
        assert not bad.any(), f"{common.colname(c)}: {int(bad.sum())} cases differ, first {int(np.argmax(bad))}"
    rejected = (so[COL.T:COL.T + 3, :n] == 0).all(0) & (cs.type == bc.BXDF.GLOSSY)
    gaps = []
    for k, (col, w) in bc.OUTPUTS.items():
        a, b = so[col:col + w, :n].T.astype(np.float64), sr[col:col + w, :n].T.astype(np.float64)
        with np.errstate(all="ignore"):
            ok = (np.abs(a - b) <= v.tol[k]).all(1) | ((a == b) | (np.isnan(a) & np.isnan(b))).all(1)
        if k == "lastPdfW":
            ok |= rejected
        bad = ~ok & v.decided
        assert not bad.any(), f"{k}: {int(bad.sum())} decided cases differ from the reference, first {int(np.argmax(bad))}: " \
                              f"{a[np.argmax(bad)]} vs {b[np.argmax(bad)]}"
        with np.errstate(all="ignore"):
            rel = np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-30), axis=1)
        for i in np.nonzero(~ok & ~v.decided & (rel > 1e-3))[0][:3]:
            gaps.append(f"{k} case {i} ({bc.TYPE_NAMES[int(cs.type[i])]}, {cs.group[i]}, {cs.label[i]}): {a[i]} vs {b[i]}")
    print("\nundecided cases with a gap above 1e-3 relative to the reference:\n  " + ("\n  ".join(gaps) if gaps else "none"))
