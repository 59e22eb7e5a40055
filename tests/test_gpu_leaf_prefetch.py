"""The leaf visit of the 4-wide traversal (csrc/flx_trace4.h: wide_leaf_visit) fetches a leaf's first triangle together with its header,
before the box test.  The read must stay inside the leaf array for every block a ray can stand on -- the last one and the dummy leaf of
unused child slots included -- and change nothing a ray computes.

Scenes: the stored teapot (tests/golden/teapot_wf.npz with the reference's own SBVH: the smallest stored scene whose wide tree has leaves
of 1, 2 and 3+ triangles and unused child slots), and one triangle (the root IS a leaf block, the last of the array).  4096 rays = 64
blocks: the adversarial sets of tests/traversal_cases.py plus rays that miss every leaf box, rays that pass a leaf box just outside one of
its corners (inside the quantised box, outside the exact one: the box test fails AFTER the fetch), axis-parallel rays, rays with a zero
direction component and origins beyond 2^26.  Every 4-wide kernel traces them:
  any hit       persistent k_trace4r, thread-per-ray k_shadow4, its counting instance and the budgeted k_shadow4s -- each bit-identical
                to the binary tree (shadow_tree 2)
  closest hit   persistent k_trace4r, thread-per-ray k_extend4 and its counting instance -- their hit records bit-identical to each other,
                and equal to the binary tree's (extend_tree 2) under test_gpu_wide's tie rule: identical records where the hit index
                agrees, otherwise both hit at the same t."""
import os
import numpy as np
import pytest
import common
import traversal_cases as tc
import test_gpu_wide
import test_wide_emulation
from common import COL
from fluctus_amd import host, wire, driver

pytestmark = pytest.mark.gpu
N = 4096
REFILL = 16 | (32 << 8)


def _teapot():
    z = np.load(os.path.join(common.GOLDEN, "teapot_wf.npz"))
    d = host.SceneData()
    d.tris = z["tris"].view(wire.TRIANGLE).reshape(-1); d.nodes = z["nodes"].view(wire.NODE).reshape(-1); d.indices = z["indices"]
    d.materials = z["materials"].view(wire.MATERIAL).reshape(-1)
    d.texdesc = np.zeros(0, wire.TEXDESC); d.texdata = np.zeros(0, np.uint8)
    return d


def _one_triangle():
    d = tc.make_scene(np.array([[[-1.0, -0.5, 0.25], [1.5, -0.25, 0.0], [0.25, 1.25, -0.5]]]))
    host.build_bvh(d, "sbvh")
    assert d.nodes.size == 1
    return d


def _rays(d, seed):
    """exactly N rays: (orig, dir, tmax), and where the corner-grazing ones sit"""
    P, leaves = tc.tri_points(d), tc.Leaves(d)
    rng = np.random.RandomState(seed)
    lo, hi = P.reshape(-1, 3).min(0), P.reshape(-1, 3).max(0)
    cen, ext = 0.5 * (lo + hi), float(np.linalg.norm(hi - lo))
    sets = list(tc.all_rays(P, leaves, n=256, seed=seed).values())
    m = 320
    # miss every leaf box: from outside the scene's box, away from it, and past it at a distance
    o = cen + rng.normal(size=(m, 3)) * 3.0 * ext
    away = (o - cen) / np.linalg.norm(o - cen, axis=1, keepdims=True)
    dd = np.where(rng.rand(m, 1) < 0.5, away, np.cross(away, rng.normal(size=(m, 3))))
    sets.append((o, dd, np.full(m, 100.0 * ext)))
    # past a leaf box just outside one of its corners, along a direction that keeps the corner's other two coordinates
    lf = rng.randint(0, leaves.lo.shape[0], m)
    size = np.maximum(leaves.hi[lf] - leaves.lo[lf], 1e-6 * ext)
    corner = np.where(rng.rand(m, 3) < 0.5, leaves.lo[lf] - size * 10.0 ** rng.uniform(-6, -2, (m, 1)), leaves.hi[lf] + size * 10.0 ** rng.uniform(-6, -2, (m, 1)))
    dd = rng.normal(size=(m, 3)); dd /= np.linalg.norm(dd, axis=1, keepdims=True)
    sets.append((corner - dd * rng.uniform(0.5, 2.0, (m, 1)) * ext, dd, np.full(m, 8.0 * ext)))
    graze = slice(sum(x[0].shape[0] for x in sets[:-1]), sum(x[0].shape[0] for x in sets))
    # axis-parallel through leaf boxes (two exactly-zero components), either way
    lf = rng.randint(0, leaves.lo.shape[0], m)
    through = leaves.lo[lf] + rng.uniform(0.0, 1.0, (m, 3)) * (leaves.hi[lf] - leaves.lo[lf])
    dd = np.zeros((m, 3)); dd[np.arange(m), rng.randint(0, 3, m)] = np.where(rng.rand(m) < 0.5, 1.0, -1.0)
    sets.append((through - dd * 2.0 * ext, dd, np.full(m, 8.0 * ext)))
    # beyond 2^26, aimed at the scene
    fd = rng.normal(size=(m, 3)); fd /= np.linalg.norm(fd, axis=1, keepdims=True)
    o = cen + fd * 1.5 * tc.FAR_ORIGIN
    tg = cen + rng.normal(size=(m, 3)) * 0.2 * ext
    sets.append((o, (tg - o) / np.linalg.norm(tg - o, axis=1, keepdims=True), np.full(m, 4.0 * tc.FAR_ORIGIN)))
    orig = np.concatenate([s[0] for s in sets]).astype(np.float32); dirs = np.concatenate([s[1] for s in sets]).astype(np.float32)
    tmax = np.concatenate([s[2] for s in sets]).astype(np.float32)
    assert orig.shape[0] <= N
    k = N - orig.shape[0]                                   # the rest: random rays through the scene's box
    o = rng.uniform(lo - 0.25 * ext, hi + 0.25 * ext, (k, 3)); dd = rng.normal(size=(k, 3))
    orig = np.concatenate([orig, o.astype(np.float32)]); dirs = np.concatenate([dirs, (dd / np.linalg.norm(dd, axis=1, keepdims=True)).astype(np.float32)])
    tmax = np.concatenate([tmax, np.full(k, 4.0 * ext, np.float32)])
    assert np.isfinite(orig).all() and np.isfinite(dirs).all() and (np.abs(dirs).max(1) > 0).all()
    assert ((dirs == 0).sum(1) == 2).sum() >= m and ((dirs == 0).sum(1) == 1).any() and (np.abs(orig).max(1) > tc.FAR_ORIGIN).sum() >= m
    return (orig, dirs, tmax), graze


def _emulation_lib():
    import ctypes
    import conftest
    L = ctypes.CDLL(conftest.build_wide_analysis())
    L.fh_analysis_last_error.restype = ctypes.c_char_p
    return L


def _ctx(d):
    from fluctus_amd.device import HipContext
    g = HipContext(N)
    g.upload_scene(d); g.set_params(tc.params(d, 1)); driver.reset_renderer(g)
    return g


def _trace(g, base, rays, opts, shadow):
    """One launch from the SAME path state every time (the commit of a closest hit counts the path's length up and keeps flags of the record
    it replaces: a state carried from one launch into the next would differ by that alone)."""
    for k, v in dict({"extend_tree": 4, "shadow_tree": 4, "refill_extend": REFILL, "refill_shadow": 0, "shadow_split": 0}, **opts).items():
        if k != "stats":
            g.set_option(k, v)
    g.trace_stats_enable(bool(opts.get("stats")))
    g.state_import(base)
    tc.load_rays(g, *rays)
    if shadow:
        g.wf_shadow()
    else:
        g.wf_extend()
    g.finish()
    st = g.state_export()
    g.trace_stats_enable(False)
    return st.view(np.uint32)


@pytest.mark.parametrize("scene", ["teapot", "one_triangle"])
def test_every_wide_kernel_with_the_first_triangle_fetched_early(scene):
    d = _teapot() if scene == "teapot" else _one_triangle()
    g = _ctx(d)
    try:
        leafdata, wnodes = g.tree_read(4), g.tree_read(3)
        count = leafdata[:, 3].view(np.int32)
        if scene == "teapot":
            npr = d.nodes["nPrims"][d.nodes["nPrims"] > 0]
            assert (npr == 1).any() and (npr == 2).any() and (npr >= 3).any()
            assert (wnodes[:, 6:10] == 0x80000000).any(), "no unused child slot in the wide tree"
        # the dummy leaf at offset 0 and the LAST block of the array both hold a whole triangle behind their header
        assert count[0] == 1 and leafdata.shape[0] >= 5
        last = 5
        while last + 2 + 3 * count[last] < leafdata.shape[0]:
            last += 2 + 3 * count[last]
        assert count[last] >= 1 and last + 2 + 3 * count[last] == leafdata.shape[0]
        rays, graze = _rays(d, 3)
        # the grazing rays do what they are for: the host emulation of the device's traversal (tests/wide_analysis.cpp, the product's own tree builder)
        # sees leaf visits whose exact box test fails after the quantised node test let the ray in -- the visits that fetch a triangle for nothing
        _, em = test_wide_emulation._emulate(_emulation_lib(), d, d.nodes, tc.emulation_rays(rays[0][graze], rays[1][graze], np.full(graze.stop - graze.start, tc.FLT_MAX, np.float32)), 0)
        assert em[1] > 0 and em[2] > 0 and em[1] - em[2] >= 16, f"{scene}: only {int(em[1] - em[2])} of {int(em[1])} leaf visits of the grazing rays fail the box test"
        base = g.state_export()
        q = np.arange(N)
        # any hit
        ref = _trace(g, base, rays, {"shadow_tree": 2}, True)[COL.SHADOW_BLOCKED][q]
        assert ref.any() and not ref.all()
        for name, opts in (("k_trace4r any-hit", {"refill_shadow": REFILL}), ("k_shadow4", {}), ("k_shadow4 counting", {"stats": 1}), ("k_shadow4s", {"shadow_split": 8})):
            got = _trace(g, base, rays, opts, True)[COL.SHADOW_BLOCKED][q]
            assert np.array_equal(got, ref), f"{scene}: {name}: shadowRayBlocked differs from the binary tree on {int((got != ref).sum())} rays"
        # closest hit
        rec = {name: _trace(g, base, rays, opts, False)[test_gpu_wide.HIT_COLS][:, q]
               for name, opts in (("k_trace4r", {}), ("k_extend4", {"refill_extend": 0}), ("k_extend4 counting", {"refill_extend": 0, "stats": 1}))}
        for name in ("k_extend4", "k_extend4 counting"):
            ne = rec[name] != rec["k_trace4r"]
            assert not ne.any(), (f"{scene}: hit records of {name} and k_trace4r differ on {int(ne.any(axis=0).sum())} rays, columns "
                                  f"{[common.colname(c) for c, x in zip(test_gpu_wide.HIT_COLS, ne.any(axis=1)) if x]}")
        wide = rec["k_trace4r"]
        binary = _trace(g, base, rays, {"extend_tree": 2}, False)[test_gpu_wide.HIT_COLS][:, q]
        ci, ct = test_gpu_wide.HIT_COLS.index(COL.HIT_I), test_gpu_wide.HIT_COLS.index(COL.HIT_T)
        assert (wide[ci].view(np.int32) >= 0).any()
        flip = wide[ci] != binary[ci]
        assert np.array_equal(wide[:, ~flip], binary[:, ~flip]), f"{scene}: hit records differ from the binary tree's on rays whose hit index agrees"
        if flip.any():
            assert (wide[ci][flip].view(np.int32) >= 0).all() and (binary[ci][flip].view(np.int32) >= 0).all(), f"{scene}: a flip between hit and miss"
            assert np.allclose(wide[ct][flip].view(np.float32), binary[ct][flip].view(np.float32), rtol=1e-5, atol=1e-6), f"{scene}: a flip that is not a tie in t"
    finally:
        g.close()
