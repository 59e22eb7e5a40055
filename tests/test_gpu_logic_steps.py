"""The five shipped instances of k_logic (csrc/logic.hip) and the plain all-types one, path by path, on the crafted cases of
tests/logic_step_cases.py: the logic-owned columns, the framebuffer pixel and the queue membership of every decided case against the float64
restatement within the tolerance derived per case (bit-identical to the input where the restatement changes nothing), and everything --
undecided cases included -- bit-identical to the oracle run in lockstep.

  A. committed records: k_logic<0> (fuse 0), k_logic<USE_DIFFUSE, false> and k_logic<USE_ALL, false> (logic, genRays, materials back to back
     under extend_tree 2, fuse_set 1 and 31), three light configurations x three sampling modes each.
  B. the RAW chain, the shipped path: rays traced by the persistent 4-wide kernel (extend_tree 4), whose RAW hit records the fused pass
     commits itself: k_logic<USE_ALL, true> (regroup 0), k_logic<USE_ALL, true, true> (regroup 1, a packing of a multiple of 256 paths padded
     with inert ones) and k_logic<USE_DIFFUSE, true> on the all-diffuse scene.  Terminating paths are regenerated in the same chain, so their
     pixel speaks for them; of the regenerated paths only the count and the pixel words are checked.
Columns the material step rewrites (T, seed, the extension ray, lastBsdf ...) are tests/bsdf_cases.py's business: here they are compared with
the oracle only."""
import numpy as np
import pytest
import common
import logic_step_cases as LC
from common import COL, Q
from fluctus_amd import driver

pytestmark = pytest.mark.gpu
_CACHE = {}
INSTANCES = {"plain": dict(fuse=0), "diffuse": dict(fuse=1, fuse_set=1), "all": dict(fuse=1, fuse_set=31)}
HIT_COLS = [COL.P, COL.P + 1, COL.P + 2, COL.N, COL.N + 1, COL.N + 2, COL.UV, COL.UV + 1, COL.HIT_T, COL.HIT_I, COL.AREA_LIGHT_HIT, COL.MAT_ID]


def contexts(key, d, env, n, **options):
    """a device context and an oracle context on the same scene, cached per module"""
    if key not in _CACHE:
        from fluctus_amd.device import HipContext
        from oracle.binding import OracleContext
        g, o = HipContext(n), OracleContext(n, threads=8)
        for k, v in options.items():
            g.set_option(k, v)
        for ctx in (g, o):
            ctx.upload_scene(d)
            ctx.upload_envmap(env)
        _CACHE[key] = g, o
    return _CACHE[key]


def same_as_oracle(a, b, what, fused, skip=None):
    """a, b: snapshots of the device and the oracle.  skip: paths whose nearest hit is a tie the two traversals break differently"""
    (sa, pa, ca, qa), (sb, pb, cb, qb) = a, b
    keep = np.ones(sa.shape[1], bool)
    if skip is not None and skip.size:
        keep[skip] = False
    else:
        assert np.array_equal(ca, cb), f"{what}: counters {ca} vs {cb}"
    for qi in range(Q.NUM):
        x, y = qa[qi][:int(ca[qi])], qb[qi][:int(cb[qi])]
        x, y = x[keep[x]], y[keep[y]]
        if qi == Q.EXTENSION and fused:
            # the fused pass lists the continuing paths by path id where the material kernels append one segment per queue: the same set
            assert np.array_equal(np.sort(x), np.sort(y)), f"{what}: the extension queue holds different paths"
        else:
            assert np.array_equal(x, y), f"{what}: queue {qi} differs"
    fails = common.state_diff(sa, sb, 0.0, 0.0, mask=keep)
    assert not fails, f"{what}: " + "; ".join(fails[:5])
    n = sa.shape[1]
    assert np.array_equal(pa.view(np.uint32)[:n][keep], pb.view(np.uint32)[:n][keep]), f"{what}: the framebuffer differs"


# ---- A. committed records
def logic_step(ctx, st, chained):
    ctx.state_import(st)
    ctx.clear_queues()
    ctx.wf_logic(False)
    if chained:
        ctx.wf_raygen()
        ctx.wf_materials()


@pytest.mark.parametrize("cfg", list(LC.CONFIGS))
@pytest.mark.parametrize("inst", list(INSTANCES))
def test_committed_records(inst, cfg):
    S, c = LC.scene(), LC.cases(cfg)
    n = c.n + LC.EXTRA
    assert n % 64 and n % 256
    g, o = contexts(("A", cfg), S.d, S.env(cfg), n, extend_tree=2)
    opt = INSTANCES[inst]
    chained = bool(opt["fuse"])
    g.set_option("fuse", opt["fuse"])
    if chained:
        g.set_option("fuse_set", opt["fuse_set"])
    for mode in LC.MODES:
        v = LC.verdict(cfg, mode)
        p = S.params(n, cfg, mode)
        assert int(p["width"]) * int(p["height"]) >= n
        for ctx in (g, o):
            ctx.set_params(p)
            driver.reset_renderer(ctx)
        st = c.state(o.state_export().copy())
        g.profile_enable(1); g.profile_reset()
        for ctx in (g, o):
            logic_step(ctx, st, chained)
        a, b = LC.snapshot(g), LC.snapshot(o)
        prof = g.profile_get(); g.profile_enable(0)
        what = f"{inst}, {cfg}, sampleExpl {mode[0]} sampleImpl {mode[1]}"
        if chained:
            assert prof["logic_fused"][1] == 1 and prof["logic"][1] == 0 and g.get_option("fuse_set_now") == opt["fuse_set"], (what, prof)
        else:
            assert prof["logic"][1] == 1 and prof["logic_fused"][1] == 0, (what, prof)
        same_as_oracle(a, b, what, chained)
        worst, label = LC.check(v, c, st, a[0], a[1], a[2], a[3], what, chained=chained)
        if chained:
            LC.check_regenerated(v, c, a[0], a[2], a[3], n, int(p["width"]) * int(p["height"]), what)
        print(f"{what}: largest error / tolerance {worst:.3f} ({label}); {int(v.decided.sum())} of {c.n} decided")
        if LC.CONFIGS[cfg]["useEnvMap"] and mode == (1, 1) and not chained:
            # the named quirk (logic_step_cases' docstring): the oracle's bits (same_as_oracle above), finite and negative
            q = np.nonzero((c.label == "-y pole") & v.info["mis_env"])[0]
            ei = a[0][COL.EI:COL.EI + 3, q]
            assert q.size == 3 and np.isfinite(ei).all() and (ei < 0).all(), f"{what}: the -y pole with a MIS weight: {ei.T.tolist()}"
        if LC.CONFIGS[cfg]["useEnvMap"] and mode == (1, 1):
            q = np.nonzero((c.label == "-y pole") & v.info["mis_env"])[0]
            assert np.isfinite(a[1][q, :3]).all() and (a[1][q, :3] < 0).all() and (a[1][q, 3] == 1).all(), f"{what}: the -y pole's pixels"


# ---- B. the RAW chain
RAW_INSTANCES = {"all": dict(all_diffuse=False, pad_to=None, fuse_set=31, regroup=0),
                 "all, regrouped": dict(all_diffuse=False, pad_to=256, fuse_set=31, regroup=1),
                 "diffuse": dict(all_diffuse=True, pad_to=None, fuse_set=1, regroup=0)}


@pytest.mark.parametrize("inst", list(RAW_INSTANCES))
def test_raw_chain(inst):
    opt = RAW_INSTANCES[inst]
    S, c = LC.scene(opt["all_diffuse"]), LC.ray_cases(opt["all_diffuse"], opt["pad_to"])
    n = c.n_tasks
    assert (n % 256 == 0) == (opt["pad_to"] == 256)
    g, o = contexts(("B", inst), S.d, S.env("both"), n)
    g.set_option("fuse_set", opt["fuse_set"])
    g.set_option("regroup", opt["regroup"])
    assert g.get_option("extend_tree") == 4 and g.get_option("fuse") == 1 and g.get_option("refill_extend") > 0, "the defaults: the persistent 4-wide kernel, fused"
    for mode in LC.MODES:
        v = LC.ray_verdict(opt["all_diffuse"], opt["pad_to"], mode)
        p = S.params(n, "both", mode, quad=c.quad)
        npix = int(p["width"]) * int(p["height"])
        assert npix >= n
        what = f"RAW {inst}, sampleExpl {mode[0]} sampleImpl {mode[1]}"
        for ctx in (g, o):
            ctx.set_params(p)
            driver.reset_renderer(ctx)
        # the device's nearest hits, looked at once (the look commits the RAW records): where they differ from the oracle's it is a tie
        # (tests/test_gpu_wide.py _extend_flips' rule), and the float64 nearest hit is the traversal's on the robust rays
        for ctx in (g, o):
            st = LC.load_rays(ctx, c)
            ctx.wf_extend()
        g.finish()
        sg, so = g.state_export(), o.state_export()
        ig, io = sg.view(np.int32), so.view(np.int32)
        flip = ig[COL.HIT_I] != io[COL.HIT_I]
        for col in HIT_COLS:
            assert np.array_equal(ig[col][~flip], io[col][~flip]), f"{what}: column {common.colname(col)} differs on rays whose hit index agrees"
        if flip.any():
            assert (ig[COL.HIT_I][flip] >= 0).all() and (io[COL.HIT_I][flip] >= 0).all(), f"{what}: a flip between hit and miss"
            assert np.allclose(sg[COL.HIT_T][flip], so[COL.HIT_T][flip], rtol=1e-5, atol=1e-6), f"{what}: flipped rays differ in t by more than a rounding tie"
        assert not flip[c.index][c.robust].any(), f"{what}: a flip on a robust ray"
        on = c.robust & ~(c.quad_wins & bool(mode[1]))
        assert np.array_equal(ig[COL.HIT_I][c.index][on], c.hit[on]), f"{what}: the float64 nearest hit is the traversal's on the robust rays"
        flipped = np.nonzero(flip)[0]
        # the chain itself
        LC.load_rays(g, c)
        g.profile_enable(1); g.profile_reset()
        g.wf_extend()
        assert g.get_option("phase") & 8, f"{what}: the extension kernel left RAW hit records"
        for ctx in (g, o):                     # the loop's order: the queues are cleared behind the traversal (the extension queue is full), then the next pass
            ctx.clear_queues()
            ctx.wf_logic(False); ctx.wf_raygen(); ctx.wf_materials()
        a, b = LC.snapshot(g), LC.snapshot(o)
        prof = g.profile_get(); g.profile_enable(0)
        assert prof["logic_fused"][1] == 1 and prof["logic"][1] == 0, (what, prof)
        assert g.get_option("fuse_set_now") == opt["fuse_set"] and g.get_option("regroup") == opt["regroup"] and not g.get_option("phase") & 8, what
        same_as_oracle(a, b, what, True, skip=flipped)
        worst, label = LC.check(v, c, st, a[0], a[1], a[2], a[3], what, chained=True, index=c.index)
        cnt = LC.check_regenerated(v, c, a[0], a[2], a[3], n, npix, what)
        print(f"{what}: largest error / tolerance {worst:.3f} ({label}); {int(v.decided.sum())} of {c.n} decided, {flipped.size} ties, {cnt} paths regenerated")
