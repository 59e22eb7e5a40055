"""The material step on the device, on the adversarial cases of tests/bsdf_cases.py: bit-exact with the oracle on every case (undecided
included) in state, counters and the extension queue, and within the derived tolerance of the float64 restatement on the decided cases.

Routes:
  separate      k_material<USE_DIFFUSE> on the diffuse queue, then k_material_rest on the other four (wfSeparateQueues 1)
  single        k_material<USE_ALL> on one queue (wfSeparateQueues 0)
  microkernel   k_mk_sample_bsdf on the same hits (sampleExpl off: nothing traced), device vs oracle
  fused         the all-types fused logic + material pass (fuse_set 31) with regroup 0 and 1, from pre-logic states carrying the crafted hits;
                the float64 check takes its inputs from the oracle's logic step run on its own
Queue fill: every material queue with 0, 1, 63, 64 and 65 paths, all-one-type and alternating-type batches; numTasks (the case count plus
37) is not a multiple of 64."""
import numpy as np
import pytest
import bsdf_cases as bc
import common
from common import COL, Q
from fluctus_amd import driver

pytestmark = pytest.mark.gpu
EXTRA = 37
_CACHE = {}


def cases():
    if "cs" not in _CACHE:
        cs = bc.CaseSet()
        _CACHE["cs"] = cs, bc.Verdict(cs.restatement(), cs.case)
    return _CACHE["cs"]


def _pair(cs, separate=True, **params):
    from fluctus_amd.device import HipContext
    from oracle.binding import OracleContext
    d = cs.scene()
    p = bc.params(d, separate)
    for k, v in params.items():
        p[k] = v
    g, o = HipContext(cs.n + EXTRA), OracleContext(cs.n + EXTRA, threads=8)
    for c in (g, o):
        c.upload_scene(d)
        c.set_params(p)
        driver.reset_renderer(c)
    return g, o


def _compare(g, o, what, ext_sorted=False):
    cg, co = g.get_counters(), o.get_counters()
    g.finish()                                      # (the device's counters arrive with the stream)
    cg, co = np.array(cg, copy=True), np.array(co, copy=True)
    assert (cg == co).all(), f"{what}: counters {cg} vs {co}"
    for q in range(Q.NUM):
        n = int(co[q])
        qa, qb = g.queue_read(q)[:n], o.queue_read(q)[:n]
        if q == Q.EXTENSION and ext_sorted:
            # the fused pass lists the continuing paths in path-id order (tests/test_gpu_parity.py _compare)
            assert np.array_equal(np.sort(qa), np.sort(qb)), f"{what}: extension queue holds different paths"
            assert (np.diff(qa.astype(np.int64)) > 0).all(), f"{what}: extension queue not in path-id order"
        else:
            assert np.array_equal(qa, qb), f"{what}: queue {q} differs"
    sg, so = g.state_export(), o.state_export()
    fails = common.state_diff(sg, so, 0.0, 0.0)
    assert not fails, f"{what}: " + "; ".join(fails[:5])
    return sg


def _fill_batches(cs, rng):
    """(label, path ids, separate): every material queue with 0 / 1 / 63 / 64 / 65 paths, all-one-type and alternating-type batches."""
    out = []
    by_q = {q: rng.permutation(np.nonzero(np.isin(cs.type, [t for t, qq in bc.QUEUE_OF.items() if qq == q]))[0])
            for q in sorted(set(bc.QUEUE_OF.values()))}
    for fill in (0, 1, 63, 64, 65):
        out.append((f"fill {fill}", np.sort(np.concatenate([ids[:fill] for ids in by_q.values()])), True))
    for q, ids in by_q.items():
        out.append((f"only queue {q}", np.sort(ids[:65]), True))
    alt = np.stack([ids[:130] for ids in by_q.values()], 1).reshape(-1)           # types alternating in path-id order
    out.append(("alternating", alt, True))
    out.append(("alternating single", alt, False))
    return out


@pytest.mark.parametrize("separate", [1, 0])
def test_material_kernels_vs_oracle_and_float64(separate):
    cs, v = cases()
    g, o = _pair(cs, bool(separate))
    try:
        for c in (g, o):
            bc.load(c, cs, bc.queues_of(cs, separate=bool(separate)))
            c.wf_materials()
        st = _compare(g, o, f"all cases, separate {separate}")
        assert np.array_equal(st.view(np.uint32)[COL.SEED, :cs.n], v.seed)
        fails = v.check(st)
        assert not fails, "; ".join(fails)
        # queue fills: the paths outside the batch keep their state on both sides
        for label, ids, sep in _fill_batches(cs, np.random.RandomState(5)):
            if bool(sep) != bool(separate) and label != "alternating single":
                continue
            if label == "alternating single" and separate:
                continue
            for c in (g, o):
                bc.load(c, cs, bc.queues_of(cs, order=ids, separate=bool(separate)))
                c.wf_materials()
            st = _compare(g, o, f"{label}, separate {separate}")
            m = np.zeros(cs.n, bool)
            m[ids] = True
            fails = v.check(st, mask=m)
            assert not fails, f"{label}: " + "; ".join(fails)
    finally:
        g.close()
        o.close()


def test_microkernel_sample_bsdf_vs_oracle():
    """k_mk_sample_bsdf on the crafted hits: the microkernel decides the face itself (dot(N, dir) > 0 flips N), so a back-face case carries
    its normal turned away; nothing is traced (sampleExpl 0)."""
    cs, _ = cases()
    n = cs.n
    g, o = _pair(cs, True, sampleExpl=0, useRoulette=0)
    try:
        p = bc.params(cs.scene())
        p["sampleExpl"], p["useRoulette"], p["width"], p["height"] = 0, 0, 128, (n + EXTRA + 127) // 128
        for c in (g, o):
            c.set_params(p)
            c.mk_reset()
            st = bc.state_of(cs, c.state_export())
            st[COL.N:COL.N + 3, :n] *= np.where(cs.case.backface, -1.0, 1.0)[None, :].astype(np.float32)
            st.view(np.int32)[COL.PHASE, :n] = 1                              # MK_SAMPLE_BSDF
            st.view(np.int32)[COL.PHASE, n:] = 4                              # the padding paths: splat (left alone)
            st.view(np.int32)[COL.HIT_I, :n] = np.arange(n) % cs.scene().tris.size
            c.state_import(st)
            c.mk_sample_bsdf()
        g.finish()
        fails = common.state_diff(g.state_export(), o.state_export(), 0.0, 0.0)
        assert not fails, "; ".join(fails[:5])
        assert np.array_equal(g.mk_stats(), o.mk_stats())
    finally:
        g.close()
        o.close()


@pytest.mark.parametrize("regroup", [0, 1])
def test_fused_all_types_pass_vs_oracle_and_float64(regroup):
    """Pre-logic states whose hit records are the crafted cases (P, N, uv, matId, hit index on a triangle of the scene); logic + materials
    back to back run as the fused all-types pass.  Float64 inputs: the oracle's logic step run on its own."""
    from oracle.binding import OracleContext
    cs, _ = cases()
    n = cs.n
    g, o = _pair(cs, True, maxBounces=8)
    o2 = OracleContext(n + EXTRA, threads=8)
    try:
        d = cs.scene()
        p = bc.params(d, True)
        p["maxBounces"] = 8
        o2.upload_scene(d); o2.set_params(p); driver.reset_renderer(o2)
        g.set_option("fuse", 1)
        g.set_option("fuse_set", 31)
        g.set_option("ext_order", 1)
        g.set_option("regroup", regroup)
        assert g.get_option("regroup") == regroup
        rng = np.random.RandomState(9)
        batches = [("all", np.arange(n)), ("alternating", np.stack([rng.permutation(np.nonzero(cs.type == t)[0])[:100] for t in bc.TYPES], 1).reshape(-1)),
                   ("one type", np.nonzero(cs.type == bc.BXDF.GLOSSY)[0][:65])]
        for label, ids in batches:
            st = bc.state_of(cs, o.state_export())
            keep = np.zeros(st.shape[1], bool)
            keep[ids] = True
            st.view(np.int32)[COL.HIT_I, :n] = np.arange(n) % d.tris.size
            st[COL.HIT_T, :n] = 1.0
            st.view(np.int32)[COL.HIT_I, ~keep] = -1                           # the others miss (and regenerate)
            st.view(np.int32)[COL.AREA_LIGHT_HIT, :] = 0
            st.view(np.uint32)[COL.PATH_LEN, :] = 1
            st.view(np.uint32)[COL.LAST_SPECULAR, :] = 1
            for c in (g, o, o2):
                c.state_import(st)
                c.clear_queues()
            g.profile_enable(1); g.profile_reset()
            for c in (g, o):
                c.wf_logic(False)
                c.wf_materials()
            st = _compare(g, o, f"fused regroup {regroup} {label}", ext_sorted=True)
            prof = g.profile_get(); g.profile_enable(0)
            assert prof["logic_fused"][1] == 1 and prof["logic"][1] == 0, prof
            # float64: the inputs of the material step as the oracle's logic leaves them
            o2.wf_logic(False)
            s2, cnt2 = o2.state_export(), np.array(o2.get_counters(), copy=True)
            q = np.concatenate([o2.queue_read(k)[:int(cnt2[k])] for k in (Q.DIFFUSE, Q.GLOSSY, Q.GGX_REFL, Q.GGX_REFR, Q.DELTA)]).astype(np.int64)
            assert q.size > 0.5 * ids.size
            u2 = s2.view(np.uint32)
            case = bc.Case(P=s2[COL.P:COL.P + 3, q].T.astype(np.float64), N=s2[COL.N:COL.N + 3, q].T.astype(np.float64),
                           uv=s2[COL.UV:COL.UV + 2, q].T.astype(np.float64), dir=s2[COL.DIR:COL.DIR + 3, q].T.astype(np.float64),
                           L=s2[COL.SHADOW_DIR:COL.SHADOW_DIR + 3, q].T.astype(np.float64), T=s2[COL.T:COL.T + 3, q].T.astype(np.float64),
                           seed=u2[COL.SEED, q].astype(np.uint64), backface=u2[COL.BACKFACE, q] != 0, mat=u2[COL.MAT_ID, q].astype(np.int64))
            v = bc.Verdict(cs.restatement(), case)
            fails = v.check(st[:, q])
            assert not fails, f"fused regroup {regroup} {label}: " + "; ".join(fails)
            assert v.decided.sum() > 0.3 * q.size
            for c in (g, o):
                c.clear_queues()
    finally:
        g.close()
        o.close()
        o2.close()

