"""flx_tree_cost on the device (csrc/tree_cost.hip, csrc/flx_tree_cost.h) against tests/tree_cost_reference.py.

  (a)  the eight sums against the float64 restatement over the SAME context's tree_read arrays, fresh and after every deformation of
       tests/refit_cases.py; the +-2^61 room and the room at 1e5 for the fp64 range; the one-leaf scene (synthetic binary root, the wide root a
       leaf block); a 60 000-triangle kitchen: hundreds of blocks and record counts that are no multiple of the block, so the slab pass and the
       tails are exercised
  (b)  the binary sums against the host node array of host.refit_bvh, independent of the device layout.  The one-leaf scene is left out of this
       leg: the device's synthetic root tests the only leaf's box in both halves and counts both (tree_cost_reference's docstring)
  TOLERANCE  relative 1e-9 per sum, derived, not measured: every term is positive and carries a few fp64 roundings, so a sum of n <= 1e7 terms in
       ANY order errs by at most about n 2^-53 ~ 1e-9 relative
  reproducible  two calls and a second context agree bit for bit; sah / identity is bit-equal before and after the update
  quiet  a running wavefront render with the call at every position of an iteration: counters, exported state, pixels as without it
  errors no scene; a null out8
"""
import ctypes as C
import numpy as np
import pytest
import traversal_cases as tc
import common
import refit_cases as rc
import tree_cost_reference as ref
from fluctus_amd import host, driver

pytestmark = pytest.mark.gpu
RTOL = 1e-9


def _ctx(n=256):
    from fluctus_amd.device import HipContext
    return HipContext(n)


def _close(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        print(f"{what}[{k}]: device {g!r} reference {w!r} rel {abs(g - w) / max(abs(w), 1e-300):.3g}")
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.isfinite(g) and abs(g - w) <= RTOL * abs(w), f"{what}: sum {k} is {g!r}, the reference says {w!r}"


def _check(g, what, nodes=None):
    """the context's sums against (a) on its own arrays and, with nodes, its binary sums against (b)"""
    b, w = g.tree_cost()
    rb, rw = ref.device_sums(g.tree_read(0), g.tree_read(1), g.tree_read(3), g.tree_read(4))
    _close(b, rb, what + "/binary")
    _close(w, rw, what + "/wide")
    assert b[0] > 0 and w[0] > 0
    if nodes is not None:
        _close(b, ref.host_sums(nodes), what + "/binary vs host nodes")
    return b, w


@pytest.mark.parametrize("name", rc.CASES + ["flat_walls-2^61"])
@pytest.mark.parametrize("builder", rc.BUILDERS)
def test_sums_match_the_reference_fresh_and_after_every_deformation(name, builder):
    P = rc.SCENES[name]
    d = rc.built(P, builder)
    g = _ctx()
    try:
        g.upload_scene(d)
        fresh = _check(g, f"{name}/{builder}/fresh")
        for kind in rc.DEFORMS if name != "flat_walls-2^61" else ("identity",):      # (the deformations of the far room leave +-2^62)
            r = rc.refitted(d, rc.deform(P, kind))
            g.update_triangles(r)
            got = _check(g, f"{name}/{builder}/{kind}", r.nodes)
            if builder == "sah" and kind == "identity":
                assert got == fresh, "a sah tree refitted in place has the fresh tree's boxes: the sums are bit-equal"
    finally:
        g.close()


def test_one_leaf_scene_synthetic_root_and_leaf_root():
    P, d = rc.two_triangle_scene()
    g = _ctx()
    try:
        g.upload_scene(d)
        b, w = _check(g, "two_triangles/fresh")
        assert b[2] == 2.0 * b[0] and b[3] == 2.0 * b[2] and b[1] == b[0], "both halves of the synthetic root count"
        assert w[1] == 0.0 and w[0] == w[2] and w[3] == 2.0 * w[0], "the wide root is the leaf block"
        g.update_triangles(rc.refitted(d, P * 1.5 + 1024.0))
        b2, w2 = _check(g, "two_triangles/moved")
        assert b2[0] > b[0]
    finally:
        g.close()


@pytest.fixture(scope="module")
def kitchen():
    d = host.generate_scene("kitchen", 60000, 42)
    return host.build_bvh(d, "sbvh")


def test_kitchen_many_blocks_tails_and_reproducibility(kitchen):
    d = kitchen
    g, h = _ctx(), _ctx()
    try:
        g.upload_scene(d)
        info = g.scene_info()
        nrec, nwide = int((d.nodes["nPrims"] == 0).sum()), info["wide_nodes"]
        assert -(-nrec // 256) + -(-nwide // 256) > 100 and nwide > 256, "the scene no longer fills a hundred blocks"
        assert nrec % 256 and nwide % 256, "a record count is a multiple of the block: the tails are not exercised"
        first = _check(g, "kitchen/fresh")
        assert g.tree_cost() == first, "two calls differ"
        h.upload_scene(d)
        assert h.tree_cost() == first, "a second context differs"
        # a sine field of 2 % of the extent, as scripts/bench_refit.py deforms
        P = tc.tri_points(d)
        lo, hi = P.min((0, 1)), P.max((0, 1))
        ext = float((hi - lo).max())
        u = (P - lo) / ext
        P2 = P + 0.02 * ext * np.stack([np.sin(5.0 * u[..., 1] + 1.0), np.sin(4.0 * u[..., 2] + 2.0), np.sin(6.0 * u[..., 0] + 3.0)], -1)
        m = host.SceneData()
        m.__dict__.update(d.__dict__)
        m.tris, m.nodes = d.tris.copy(), d.nodes.copy()
        for i, v in enumerate(("v0", "v1", "v2")):
            for j, k in enumerate("xyz"):
                m.tris[v]["p"][k] = np.float32(P2[:, i, j])
        host.refit_bvh(m)
        g.update_triangles(m); h.update_triangles(m)
        moved = _check(g, "kitchen/sine 2 %", m.nodes)
        assert h.tree_cost() == moved and g.tree_cost() == moved
        from fluctus_amd.device import tree_cost_value
        ratio = tree_cost_value(moved[1]) / tree_cost_value(first[1])
        print(f"kitchen 60k, sine 2 %: wide cost ratio refit / fresh {ratio:.4f}")
        assert ratio > 1.0
    finally:
        g.close(); h.close()


def test_tree_cost_leaves_the_run_alone():
    """two contexts run the same wavefront chain, one with flx_tree_cost at every position of an iteration: counters and the exported state are
    identical bit for bit; the framebuffer is a sum of float atomics in an order the device does not define: identical sample counts and
    common.fb_close's bound, as test_gbuffer_leaves_the_run_alone compares"""
    W, H = 64, 48
    d = common.mixed_material_scene()
    p = common.scene_params(d, W, H, maxBounces=4, wfSeparateQueues=1)
    a, b = _ctx(W * H), _ctx(W * H)
    try:
        for g in (a, b):
            g.set_option("extend_tree", 2)
            g.upload_scene(d); g.set_params(p); driver.reset_renderer(g)
        want = None
        for it in range(6):
            cnts = []
            for g, probe in ((a, False), (b, True)):
                steps = [lambda: g.wf_logic(False), g.wf_raygen, g.wf_materials, g.wf_extend, g.wf_shadow, g.clear_queues]
                cnt = None
                for k, s in enumerate(steps):
                    if probe:
                        got = g.tree_cost()
                        want = want or got
                        assert got == want
                    s()
                    if k == 2:
                        cnt = g.get_counters()
                g.finish()
                cnt = np.array(cnt, copy=True)
                g.pixel_index_update(W * H, int(cnt[0]))
                cnts.append(cnt)
            assert np.array_equal(cnts[0], cnts[1]), (it, cnts)
        assert not common.state_diff(a.state_export(), b.state_export(), 0.0, 0.0)
        pa, pb = a.read_pixels(0), b.read_pixels(0)
        assert pa[:, 3].sum() > 0 and np.array_equal(pa[:, 3], pb[:, 3]) and common.fb_close(pa, pb)
    finally:
        a.close(); b.close()


def test_error_paths():
    g = _ctx()
    try:
        with pytest.raises(RuntimeError, match="flx_tree_cost: upload a scene first"):
            g.tree_cost()
        g.upload_scene(rc.built(rc.SCENES["flat_walls-o0"], "sbvh"))
        assert g.L.flx_tree_cost(g.h, None) != 0
        assert b"flx_tree_cost: null out8" in g.L.flx_last_error(g.h)
        g.tree_cost()                                                        # and a good call still goes through
    finally:
        g.close()
