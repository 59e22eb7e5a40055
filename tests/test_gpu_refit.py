"""flx_update_triangles on the device: both traversal trees refitted over the uploaded topology (csrc/refit.hip, csrc/flx_refit.h).

Trees are built on positions P, uploaded, and moved to P' by HipContext.update_triangles (tests/refit_cases.py: identity, smooth, scramble; a
one-leaf scene; the flat room at +-2^61).  The reference is host.refit_bvh's node array over P' -- uploaded into the oracle, and into a fresh
HipContext for everything that is compared byte for byte.
  parity      the comparison of test_gpu_traversal_edges.test_kernels_vs_oracle_and_brute_force (variants default / refill / binary, env 1 / 0,
              float64 brute force over P'): binary closest hit and every any-hit bit-identical to the oracle, 4-wide closest hit without a flip on
              decided rays and with ties only on the others.  The same comparison with a FRESH upload of the refit nodes runs first: it is the
              code as it was, so a failure after it points at the refit and not at the rays.
  invariants  flx_tree_read's five arrays: boxes, .w words, positions, shading records, child refs, inverted unused slots, planes that contain
              the child's exact box in rational arithmetic, scales at most 2 x the host quantiser's (a quality cap: both grids are valid where the
              first guess of the exponent differs; the count of differing nodes is printed)
  no history  P -> P' -> P equals P -> P on all five arrays; updating twice changes nothing
  render      64 x 64, four wavefront iterations with extend_tree 2, and the microkernel integrator for 2 spp, with normals / uvs / matId changed
              too: "upload P, update to P'" equals "upload P' with the refit nodes" bit for bit
  boundary    deferred launches run on the old scene first; the adaptive list and the reprojection history are dropped; a device source equals
              the host source; refused calls leave the old scene rendering as before
"""
import numpy as np
import pytest
import traversal_cases as tc
import common
import test_gpu_wide
import refit_cases as rc
from common import COL
from fluctus_amd import host, driver
from test_gpu_traversal_edges import VARIANTS, _rays_and_witness

pytestmark = pytest.mark.gpu
PARITY = [(n, "sbvh", k) for n in rc.CASES for k in rc.DEFORMS] + [("spatial_splits-o0", "sah", k) for k in rc.DEFORMS] + [("flat_walls-2^61", "sbvh", "identity")]
N_RAYS = 1024


def _ctx(n):
    from fluctus_amd.device import HipContext
    return HipContext(n)


def _compare(g, o, d, orig, dirs, tmax, gen, names, v, what0):
    """test_kernels_vs_oracle_and_brute_force's body for contexts that already hold their scene (g: HipContext, o: the oracle on tree d)"""
    n = orig.shape[0]
    dec, P = v["ext_decided"], tc.tri_points(d)
    launched = []
    for env in (1, 0):
        p = tc.params(d, env)
        for c in (g, o):
            c.set_params(p); driver.reset_renderer(c)
        assert g.scene_info()["nested"] == 1
        for var, opts in VARIANTS.items():
            for k in ("extend_tree", "shadow_tree"):
                g.set_option(k, opts.get(k, 4))
            g.set_option("refill_extend", opts.get("refill_extend", 16 | (32 << 8)))
            g.set_option("refill_shadow", opts.get("refill_shadow", -1))
            what = f"{what0}/env{env}/{var}"
            tc.load_rays(o, orig, dirs, tmax, np.nonzero(dec)[0])
            common.sync(g, o)
            _, flips = test_gpu_wide._extend_flips(g, o, what)
            assert flips == 0, f"{what}: {flips} decided rays flip against the oracle"
            hg, _ = tc.hits(g, n)
            ho, _ = tc.hits(o, n)
            tc.load_rays(o, orig, dirs, tmax, np.nonzero(~dec)[0])
            common.sync(g, o)
            g.wf_extend(); o.wf_extend(); g.finish()
            hu, _ = tc.hits(g, n)
            ou, _ = tc.hits(o, n)
            hg, ho = np.where(dec, hg, hu), np.where(dec, ho, ou)
            assert np.array_equal(hg >= 0, ho >= 0), f"{what}: hit / miss differs from the oracle on {int(((hg >= 0) != (ho >= 0)).sum())} rays"
            flip = hg != ho
            if var == "binary":
                assert not flip.any(), f"{what}: the binary kernel's closest hit differs from the oracle's on {int(flip.sum())} rays"
            if flip.any():
                (ta, ea), (tb, eb) = tc.pair_t(P, orig[flip], dirs[flip], hg[flip]), tc.pair_t(P, orig[flip], dirs[flip], ho[flip])
                wide = ~(np.abs(ta - tb) <= 1e-5 * np.abs(tb) + 1e-6 + ea + eb)
                assert not wide.any(), f"{what}: a closest-hit flip that is not a tie in t: {ta[wide][:4]} vs {tb[wide][:4]}"
            bad = dec & (hg != ho)
            assert not bad.any(), f"{what}: {int(bad.sum())} decided rays flip against the oracle (generators {sorted({names[i] for i in gen[bad]})})"
            bad = dec & (hg != v["closest"])
            assert not bad.any(), f"{what}: {int(bad.sum())} decided closest hits differ from the brute force"
            tc.load_rays(o, orig, dirs, tmax)
            common.sync(g, o)
            g.wf_shadow(); o.wf_shadow(); g.finish()
            _, bg = tc.hits(g, n)
            _, bo = tc.hits(o, n)
            assert np.array_equal(bg, bo), f"{what}: shadowRayBlocked differs from the oracle on {int((bg != bo).sum())} of {n} rays"
            bad = v["sh_decided"] & (bg != v["blocked"])
            assert not bad.any(), f"{what}: {int(bad.sum())} decided shadow rays differ from the brute force"
            launched.append((env, var))
    assert len(launched) == 2 * len(VARIANTS)


def _case(name, builder, kind):
    if name == "two_triangles":
        P, d = rc.two_triangle_scene()
    else:
        P = rc.SCENES[name]
        d = rc.built(P, builder)
    P2 = rc.deform(P, kind) if name != "two_triangles" else P * 1.5 + 1024.0
    return d, rc.refitted(d, P2)


def _parity(name, builder, kind):
    from oracle.binding import OracleContext
    d, r = _case(name, builder, kind)
    orig, dirs, tmax, gen, names = _rays_and_witness(r)
    v = tc.BruteForce(tc.tri_points(r), orig, dirs, tmax).verdict(r)
    assert not v["uncovered"], f"robust hits outside every leaf box of their triangle: {v['uncovered'][:3]}"
    n = orig.shape[0]
    g, o = _ctx(n), OracleContext(n, threads=16)
    try:
        o.upload_scene(r)
        g.upload_scene(r)                                   # precondition: today's code on the refit nodes
        _compare(g, o, r, orig, dirs, tmax, gen, names, v, f"{name}/{builder}/{kind}/fresh")
        g.upload_scene(d)
        g.update_triangles(r)
        _compare(g, o, r, orig, dirs, tmax, gen, names, v, f"{name}/{builder}/{kind}/refit")
    finally:
        g.close()
        o.close()


@pytest.mark.parametrize("name,builder,kind", PARITY)
def test_refit_parity_with_oracle_and_brute_force(name, builder, kind):
    _parity(name, builder, kind)


def test_refit_parity_one_leaf_scene():
    _parity("two_triangles", "sbvh", "move")


# ---------------------------------------------------------------------------------------------------------------------------------
def _arrays(g):
    return [g.tree_read(w) for w in range(5)]


def _f(a):
    return a.view(np.float32)


def _positions(r):
    return np.float32(tc.tri_points(r))                     # (T, 3, 3): exactly the fp32 vertices


def _check_invariants(before, after, r, fresh_shade):
    bn, tr, sh, wn, wl = after
    nd, P32 = r.nodes, _positions(r)
    # BNode boxes = host.refit_bvh's, through the record numbering (record 0 = node 0; an inner child's record is the parent's ref)
    if nd["nPrims"][0] == 0:
        todo = [(0, 0)]
        while todo:
            i, rec = todo.pop()
            b = bn[rec]
            for (ch, box, ref) in ((i + 1, b[0:6], b[12]), (int(nd["iStartOrRight"][i]), b[6:12], b[13])):
                mn, mx = rc.node_box(nd, ch)
                assert np.array_equal(box, np.concatenate([rc.bits(mn), rc.bits(mx)])), f"record {rec}: box of node {ch}"
                if nd["nPrims"][ch]:
                    assert ref == rc.LEAF_BIT | int(nd["iStartOrRight"][ch])
                else:
                    todo.append((ch, int(ref)))
    else:
        mn, mx = rc.node_box(nd, 0)
        assert np.array_equal(bn[0][0:6], np.concatenate([rc.bits(mn), rc.bits(mx)])) and np.array_equal(bn[0][6:12], bn[0][0:6])
    assert np.array_equal(bn[:, 12:], before[0][:, 12:])
    # TriRec: .w words as uploaded, positions = P'
    t0, t1 = before[1].reshape(-1, 3, 4), tr.reshape(-1, 3, 4)
    assert np.array_equal(t0[:, :, 3], t1[:, :, 3])
    assert np.array_equal(t1[:, 0, 3], r.indices)
    assert np.array_equal(t1[:, :, :3], rc.bits(P32[r.indices]))
    # wide leaf data: .w words as uploaded, positions = P', header = the union of the block's triangles
    assert np.array_equal(before[4][:, 3], wl[:, 3])
    off, leaf_box = 5, {}
    while off < wl.shape[0]:
        cnt = int(wl[off, 3])
        blk = wl[off + 2:off + 2 + 3 * cnt].reshape(cnt, 3, 4)
        assert np.array_equal(blk[:, :, :3], rc.bits(P32[blk[:, 0, 3]]))
        pts = _f(np.ascontiguousarray(blk[:, :, :3])).reshape(-1, 3)
        assert np.array_equal(wl[off, :3], rc.bits(rc.fold_min(pts))) and np.array_equal(wl[off + 1, :3], rc.bits(rc.fold_max(pts)))
        leaf_box[off] = (_f(wl[off, :3].copy()), _f(wl[off + 1, :3].copy()))
        off += 2 + 3 * cnt
    assert off == wl.shape[0] and len(leaf_box) == int((nd["nPrims"] > 0).sum())
    assert sh.tobytes() == fresh_shade.tobytes()
    # WNodes: refs as uploaded; bottom-up (children are numbered after their parent) the exact boxes, then the grid of every node
    assert np.array_equal(wn[:, 6:10], before[3][:, 6:10])
    differ = 0
    if nd["nPrims"][0] == 0:
        exact = {}
        for wi in range(wn.shape[0] - 1, -1, -1):
            w = wn[wi]
            o, s, qlo, qhi = _f(w[0:3].copy()), _f(w[3:6].copy()), w[10:13], w[13:16]
            cmin, cmax = [], []
            for k in range(4):
                ref = int(w[6 + k])
                if ref == rc.LEAF_BIT:
                    for a in range(3):
                        assert (int(qlo[a]) >> (8 * k)) & 255 == 255 and (int(qhi[a]) >> (8 * k)) & 255 == 0, f"wide node {wi}: unused slot {k} not inverted"
                    continue
                assert len(cmin) == k
                mn, mx = leaf_box[ref & 0x7FFFFFFF] if ref & rc.LEAF_BIT else exact[ref]
                cmin.append(mn); cmax.append(mx)
            cmin, cmax = np.stack(cmin), np.stack(cmax)
            exact[wi] = (rc.fold_min(cmin), rc.fold_max(cmax))
            assert rc.planes_contain(o, s, qlo, qhi, cmin, cmax), f"wide node {wi}: a quantised plane cuts into a child's exact box"
            ho, hs, hqlo, hqhi = host.wide_quantise(cmin, cmax)
            assert np.array_equal(rc.bits(o), rc.bits(ho))
            e = np.log2(s.astype(np.float64))
            assert (e == np.round(e)).all() and (e >= -108).all()
            assert (s <= 2.0 * hs).all(), f"wide node {wi}: scale {s} above twice the host quantiser's {hs}"
            differ += int(not (np.array_equal(s, hs) and np.array_equal(qlo, hqlo) and np.array_equal(qhi, hqhi)))
        mn, mx = rc.node_box(nd, 0)
        assert np.array_equal(exact[0][0], mn) and np.array_equal(exact[0][1], mx)
    return differ


@pytest.mark.parametrize("name,builder,kind", [(n, "sbvh", k) for n in ("spatial_splits-o0", "flat_walls-o1e5") for k in rc.DEFORMS] +
                         [("mixed_scale-o0", "sah", "smooth"), ("flat_walls-2^61", "sbvh", "identity"), ("two_triangles", "sbvh", "move")])
def test_refit_tree_invariants_and_no_history(name, builder, kind):
    d, r = _case(name, builder, kind)
    r = rc.with_shading(r)
    g, f = _ctx(256), _ctx(256)
    try:
        g.upload_scene(d)
        before = _arrays(g)
        g.update_triangles(r)
        after = _arrays(g)
        f.upload_scene(r)
        differ = _check_invariants(before, after, r, f.tree_read(2))
        print(f"{name}/{builder}/{kind}: {differ} of {after[3].shape[0]} wide nodes quantised differently from the host quantiser")
        # updating twice changes nothing; P -> P' -> P equals P -> P
        g.update_triangles(r)
        for a, b in zip(after, _arrays(g)):
            assert a.tobytes() == b.tobytes()
        g.update_triangles(d)
        back = _arrays(g)
        f.upload_scene(d); f.update_triangles(d)
        for w, (a, b) in enumerate(zip(back, _arrays(f))):
            assert a.tobytes() == b.tobytes(), f"array {w} remembers the detour"
    finally:
        g.close(); f.close()


# ---------------------------------------------------------------------------------------------------------------------------------
def _render_pair():
    """(scene built on P, the same topology refitted to P' with normals, uvs and material ids changed too)"""
    d = common.mixed_material_scene()
    P = tc.tri_points(d)
    m = rc.with_shading(d, nmat=d.materials.size)
    m.nodes = d.nodes.copy()
    P2 = np.float32(rc.deform(P, "smooth") * np.array([1.0, 0.35, 1.0]))
    for i, v in enumerate(("v0", "v1", "v2")):
        for j, k in enumerate("xyz"):
            m.tris[v]["p"][k] = P2[:, i, j]
    return d, host.refit_bvh(m)


@pytest.mark.parametrize("integrator", ["wavefront", "microkernel"])
def test_refit_render_equals_fresh_upload_bit_for_bit(integrator):
    d, r = _render_pair()
    W = H = 64
    p = common.scene_params(r, W, H, maxBounces=4, wfSeparateQueues=1)
    a, b = _ctx(W * H), _ctx(W * H)
    try:
        a.upload_scene(d); a.update_triangles(r)
        b.upload_scene(r)
        for k in ("fuse_set", "ext_order", "regroup"):       # the update keeps what the upload of P chose; the fresh upload of P' gets the same
            b.set_option(k, a.get_option(k))
        for c in (a, b):
            c.set_option("extend_tree", 2)
            c.set_params(p)
            if integrator == "wavefront":
                driver.reset_renderer(c)
                for _ in range(4):
                    driver.benchmark_iteration(c, W * H)
            else:
                driver.render_single(c, p, 2)
        pa, pb = a.read_pixels(0), b.read_pixels(0)
        assert pa[:, 3].sum() > 0
        assert pa.tobytes() == pb.tobytes(), f"{int((pa != pb).any(1).sum())} pixels differ"
        assert not common.state_diff(a.state_export(), b.state_export(), 0.0, 0.0)
    finally:
        a.close(); b.close()


def test_update_launches_deferred_work_on_the_old_scene_first():
    d, r = _render_pair()
    W = H = 64
    p = common.scene_params(d, W, H, maxBounces=4, wfSeparateQueues=1)
    ctxs = [_ctx(W * H), _ctx(W * H)]
    try:
        for fuse, c in enumerate(ctxs):
            c.set_option("fuse", fuse); c.set_option("extend_tree", 2)
            c.upload_scene(d); c.set_params(p); driver.reset_renderer(c)
            for _ in range(2):
                driver.benchmark_iteration(c, W * H)
            c.wf_logic(False)
            if fuse:
                assert c.get_option("phase") & 7 == 1, "flx_wf_logic was not deferred: the test does not reach the boundary"
            c.update_triangles(r)
            assert c.get_option("phase") & 7 == 0
            c.wf_raygen(); c.wf_materials(); c.wf_extend(); c.wf_shadow(); c.clear_queues(); c.finish()
        assert not common.state_diff(ctxs[1].state_export(), ctxs[0].state_export(), 0.0, 0.0)
        # (the fused pass splats in another order than the separate kernels: float atomics, common.fb_close's bound)
        assert common.fb_close(ctxs[1].read_pixels(0), ctxs[0].read_pixels(0))
    finally:
        for c in ctxs:
            c.close()


def test_update_drops_the_adaptive_list_and_the_reprojection_history():
    d, r = _render_pair()
    W = H = 32
    g = _ctx(W * H)
    try:
        g.set_option("moments", 1)
        g.upload_scene(d); g.set_params(common.scene_params(d, W, H)); g.mk_reset()
        g.mk_active_write([0, 5, 9])
        assert g.mk_active_read()[0].tolist() == [0, 5, 9]
        g.gbuffer(); g.history_capture(); g.gbuffer()
        g.reproject()
        g.update_triangles(r)
        with pytest.raises(RuntimeError, match="no list of active pixels"):
            g.mk_active_read()
        with pytest.raises(RuntimeError, match="flx_reproject"):
            g.reproject()
        g.gbuffer()
        with pytest.raises(RuntimeError, match="no captured history"):
            g.reproject()
        g.history_capture(); g.gbuffer()
        g.reproject(); g.finish()
    finally:
        g.close()


def test_device_source_equals_host_source():
    import torch
    d, r = _render_pair()
    a, b = _ctx(256), _ctx(256)
    try:
        a.upload_scene(d); a.update_triangles(r)
        t = torch.from_numpy(np.frombuffer(r.tris.tobytes(), np.uint8).copy()).cuda()
        b.upload_scene(d); b.update_triangles(t, on_device=True)
        for x, y in zip(_arrays(a), _arrays(b)):
            assert x.tobytes() == y.tobytes()
    finally:
        a.close(); b.close()


def test_refused_updates_leave_the_old_scene_rendering_as_before():
    good = rc.built(rc.SCENES["flat_walls-o0"], "sbvh")
    orig, dirs, tmax, _, _ = _rays_and_witness(good)
    n = orig.shape[0]

    def bad_copy(edit):
        m = rc.moved(good, tc.tri_points(good))
        edit(m.tris)
        return m

    def nan(t): t["v1"]["p"]["y"][7] = np.nan
    def inf(t): t["v2"]["p"]["x"][0] = np.inf
    def far(t): t["v0"]["p"]["z"][t.size - 1] = -2.0 ** 63
    def mat(t): t["matId"][3] = good.materials.size
    def neg(t): t["matId"][3] = -1
    refusals = [(bad_copy(nan), "NaN or infinite"), (bad_copy(inf), "NaN or infinite"), (bad_copy(far), r"beyond \+-2\^62"),
                (bad_copy(mat), "material id out of range"), (bad_copy(neg), "material id out of range"), (good.tris[:-1], "triangle count differs")]
    g = _ctx(n)
    try:
        with pytest.raises(RuntimeError, match="upload a scene first"):
            g.update_triangles(good)
        g.upload_scene(good); g.set_params(tc.params(good, 0)); driver.reset_renderer(g)

        def trace():
            tc.load_rays(g, orig, dirs, tmax)
            g.wf_extend(); g.wf_shadow(); g.finish()
            st = g.state_export()
            return st[[COL.HIT_I, COL.HIT_T, COL.SHADOW_BLOCKED], :n].tobytes(), [a.tobytes() for a in _arrays(g)]

        ref = trace()
        assert g.state_export().view(np.int32)[COL.HIT_I][:n].max() >= 0
        for m, msg in refusals:
            with pytest.raises(RuntimeError, match=msg):
                g.update_triangles(m)
            assert trace() == ref, f"after the refusal '{msg}' the context no longer renders the old scene"
        g.update_triangles(good)                             # and a good call still goes through
        g.finish()
    finally:
        g.close()
