"""flx_update_triangles_subset on the device: a listed subset of the triangles moves, only what hangs above it is rewritten (csrc/refit.hip,
DESIGN.md 4.10.2).

Trees are built on positions P and uploaded; the standard subset S of tests/refit_subset_cases.py (every eighth triangle, moved by an eighth of the
extent) goes in through HipContext.update_triangles_subset.  The reference is host.refit_bvh_subset's node array.
  tree bytes  flx_tree_read's five arrays: every record without a listed triangle below it equals its pre-call BYTES (the property a call that
              forwards to the full refit fails), .w words and child refs as uploaded, shading records of a fresh upload, BNode boxes =
              host.refit_bvh_subset's through the record numbering, dirty leaf headers = the folded union of their triangles, dirty WNodes pass
              test_gpu_refit's wide checks (planes contain the children's exact boxes in rational arithmetic, origins equal, power-of-two scales
              at most 2 x the host quantiser's, unused slots inverted)
  algebra     every index listed = update_triangles; two disjoint calls = one; a repeated call changes nothing; two contexts agree; on the
              unclipped cases arrays 0, 1, 2, 4 equal the full update's (array 3 may keep the upload's host-quantised grid on clean nodes)
  modes       subset, full, subset in one context = full, subset, checked against host.refit_bvh + host.refit_bvh_subset; the full update again =
              "upload, full update"; device and host sources mixed (one context's stamps, epoch, staging buffers and triangle copy serve both calls)
  parity      test_gpu_refit._compare against the oracle on host.refit_bvh_subset's nodes and the float64 brute force, fresh upload first
  render      "upload, subset update" = "upload of the result with the subset-refit nodes", bit for bit, both integrators
  cost        the binary figure of flx_tree_cost after the subset update is strictly below the full update's
  clamp       the read-only option "wide_far" follows the whole resulting triangle set, up and down again
  boundary    deferred launches run on the old scene first; the adaptive list and the reprojection history are dropped; a device source equals
              a host source; nothing listed changes nothing; every refusal names its cause and leaves trees and render as they were
  Tracer      update_geometry_subset against a HipContext driven by hand, and under the Blocking and Background rebuild policies
"""
import copy
import math
import numpy as np
import pytest
import traversal_cases as tc
import common
import refit_cases as rc
import refit_subset_cases as sc
import test_gpu_refit as tgr
import test_gpu_rebuild as tgb
from common import COL
from fluctus_amd import host, driver
from fluctus_amd.device import tree_cost_value
from test_gpu_traversal_edges import _rays_and_witness

pytestmark = pytest.mark.gpu
_ctx, _arrays, _f = tgr._ctx, tgr._arrays, tgr._f


def _case(name, builder, shading=True):
    """(tree d on P, index list, scene r = d's topology with the subset moved (and re-shaded) and host.refit_bvh_subset's nodes)"""
    d = sc.built(name, builder)
    idx, P2 = sc.S(name)
    m = rc.moved(d, P2)
    if shading:
        m = sc.with_shading_on(m, idx)
    return d, idx, host.refit_bvh_subset(m, idx)


def _same(a, b, what):
    for w, (x, y) in enumerate(zip(a, b)):
        assert x.tobytes() == y.tobytes(), f"{what}: tree array {w} differs"


# ---------------------------------------------------------------------------------------------------------------------------------
def _check_subset(before, after, d, r, idx, fresh_shade):
    """test_gpu_refit._check_invariants for a subset update: what is dirty holds the refit's values, everything else its pre-call bytes"""
    bn, tr, sh, wn, wl = after
    nd, P32 = r.nodes, tgr._positions(r)
    moved = np.zeros(d.tris.size, bool); moved[idx] = True
    dirty = sc.dirty_sets(d, idx)
    # BNode boxes = host.refit_bvh_subset's, through the record numbering; records with two clean halves on their pre-call bytes
    touched = np.zeros(bn.shape[0], bool)
    if nd["nPrims"][0] == 0:
        todo = [(0, 0)]
        while todo:
            i, rec = todo.pop()
            b = bn[rec]
            for (ch, box, ref) in ((i + 1, b[0:6], b[12]), (int(nd["iStartOrRight"][i]), b[6:12], b[13])):
                mn, mx = rc.node_box(nd, ch)
                assert np.array_equal(box, np.concatenate([rc.bits(mn), rc.bits(mx)])), f"record {rec}: box of node {ch}"
                touched[rec] |= dirty[ch]
                if nd["nPrims"][ch]:
                    assert ref == rc.LEAF_BIT | int(nd["iStartOrRight"][ch])
                else:
                    todo.append((ch, int(ref)))
    else:
        mn, mx = rc.node_box(nd, 0)
        assert np.array_equal(bn[0][0:6], np.concatenate([rc.bits(mn), rc.bits(mx)])) and np.array_equal(bn[0][6:12], bn[0][0:6])
        touched[0] = dirty[0]
    assert bn[~touched].tobytes() == before[0][~touched].tobytes(), "a BNode record with two clean halves was rewritten"
    assert np.array_equal(bn[:, 12:], before[0][:, 12:])
    # TriRec: .w words as uploaded, listed triangles at their new positions, every other record on its pre-call bytes
    t0, t1 = before[1].reshape(-1, 3, 4), tr.reshape(-1, 3, 4)
    assert np.array_equal(t0[:, :, 3], t1[:, :, 3])
    assert np.array_equal(t1[:, 0, 3], r.indices)
    assert np.array_equal(t1[:, :, :3], rc.bits(P32[r.indices]))
    keep = ~moved[r.indices]
    assert t1[keep].tobytes() == t0[keep].tobytes(), "the TriRec of an unlisted triangle was rewritten"
    assert moved[r.indices].sum() >= idx.size
    # wide leaf data: .w words as uploaded; a block with a listed triangle: positions and the folded union; every other block on its bytes
    assert np.array_equal(before[4][:, 3], wl[:, 3])
    assert wl[:5].tobytes() == before[4][:5].tobytes()
    off, leaf_box, leaf_dirty = 5, {}, {}
    while off < wl.shape[0]:
        cnt = int(wl[off, 3])
        blk = wl[off + 2:off + 2 + 3 * cnt].reshape(cnt, 3, 4)
        leaf_dirty[off] = bool(moved[blk[:, 0, 3]].any())
        if leaf_dirty[off]:
            assert np.array_equal(blk[:, :, :3], rc.bits(P32[blk[:, 0, 3]]))
            pts = _f(np.ascontiguousarray(blk[:, :, :3])).reshape(-1, 3)
            assert np.array_equal(wl[off, :3], rc.bits(rc.fold_min(pts))) and np.array_equal(wl[off + 1, :3], rc.bits(rc.fold_max(pts)))
        else:
            assert wl[off:off + 2 + 3 * cnt].tobytes() == before[4][off:off + 2 + 3 * cnt].tobytes(), f"clean leaf block {off} was rewritten"
        leaf_box[off] = (_f(wl[off, :3].copy()), _f(wl[off + 1, :3].copy()))
        off += 2 + 3 * cnt
    assert off == wl.shape[0] and len(leaf_box) == int((nd["nPrims"] > 0).sum())
    assert sum(leaf_dirty.values()) == int((dirty & (nd["nPrims"] > 0)).sum())
    assert sh.tobytes() == fresh_shade.tobytes()
    # WNodes: refs as uploaded; bottom-up (children are numbered after their parent) the exact boxes -- the builders' inner boxes are the unions of
    # their children (asserted at the root), so the exact box of a clean node follows from its children too -- a node without a dirty child on its
    # pre-call bytes, every other node through test_gpu_refit's wide checks
    assert np.array_equal(wn[:, 6:10], before[3][:, 6:10])
    n_dirty = differ = 0
    if nd["nPrims"][0] == 0:
        exact, wdirty = {}, {}
        for wi in range(wn.shape[0] - 1, -1, -1):
            w = wn[wi]
            o, s, qlo, qhi = _f(w[0:3].copy()), _f(w[3:6].copy()), w[10:13], w[13:16]
            cmin, cmax, wdirty[wi] = [], [], False
            for k in range(4):
                ref = int(w[6 + k])
                if ref == rc.LEAF_BIT:
                    for a in range(3):
                        assert (int(qlo[a]) >> (8 * k)) & 255 == 255 and (int(qhi[a]) >> (8 * k)) & 255 == 0, f"wide node {wi}: unused slot {k} not inverted"
                    continue
                assert len(cmin) == k
                mn, mx = leaf_box[ref & 0x7FFFFFFF] if ref & rc.LEAF_BIT else exact[ref]
                wdirty[wi] |= leaf_dirty[ref & 0x7FFFFFFF] if ref & rc.LEAF_BIT else wdirty[ref]
                cmin.append(mn); cmax.append(mx)
            cmin, cmax = np.stack(cmin), np.stack(cmax)
            exact[wi] = (rc.fold_min(cmin), rc.fold_max(cmax))
            assert rc.planes_contain(o, s, qlo, qhi, cmin, cmax), f"wide node {wi}: a quantised plane cuts into a child's exact box"
            if not wdirty[wi]:
                assert w.tobytes() == before[3][wi].tobytes(), f"wide node {wi} has no dirty child and was rewritten"
                continue
            n_dirty += 1
            ho, hs, hqlo, hqhi = host.wide_quantise(cmin, cmax)
            assert np.array_equal(rc.bits(o), rc.bits(ho))
            e = np.log2(s.astype(np.float64))
            assert (e == np.round(e)).all() and (e >= -108).all()
            assert (s <= 2.0 * hs).all(), f"wide node {wi}: scale {s} above twice the host quantiser's {hs}"
            differ += int(not (np.array_equal(s, hs) and np.array_equal(qlo, hqlo) and np.array_equal(qhi, hqhi)))
        mn, mx = rc.node_box(nd, 0)
        assert np.array_equal(exact[0][0], mn) and np.array_equal(exact[0][1], mx)
        assert wdirty[0] and n_dirty < wn.shape[0]
    return int(touched.sum()), n_dirty, differ


@pytest.mark.parametrize("name,builder", sc.CASES)
def test_subset_tree_bytes(name, builder):
    d, idx, r = _case(name, builder)
    g, f = _ctx(256), _ctx(256)
    try:
        g.upload_scene(d)
        before = _arrays(g)
        g.update_triangles_subset(r.tris[idx], idx)
        after = _arrays(g)
        f.upload_scene(r)
        nb, nw, differ = _check_subset(before, after, d, r, idx, f.tree_read(2))
        print(f"{name}/{builder}: {nb} of {after[0].shape[0]} BNode records and {nw} of {after[3].shape[0]} wide nodes rewritten, "
              f"{differ} of them quantised differently from the host quantiser")
        assert 0 < nb < after[0].shape[0]
    finally:
        g.close(); f.close()


@pytest.mark.parametrize("name,builder", sc.CASES)
def test_subset_algebra_on_the_device(name, builder):
    d, idx, r = _case(name, builder)
    every = np.arange(d.tris.size, dtype=np.uint32)
    a, b, c = _ctx(256), _ctx(256), _ctx(256)
    try:
        # every index listed = update_triangles with the same triangles
        a.upload_scene(d); a.update_triangles_subset(r.tris, every)
        b.upload_scene(d); b.update_triangles(r.tris)
        _same(_arrays(a), _arrays(b), "all indices vs update_triangles")
        full = _arrays(b)
        # one call; repeated; two disjoint calls; a second context with the same sequence
        a.upload_scene(d); a.update_triangles_subset(r.tris[idx], idx)
        once = _arrays(a)
        a.update_triangles_subset(r.tris[idx], idx)
        _same(_arrays(a), once, "a repeated call")
        h0, h1 = idx[::2], idx[1::2]
        b.upload_scene(d); b.update_triangles_subset(r.tris[h0], h0); b.update_triangles_subset(r.tris[h1], h1)
        _same(_arrays(b), once, "two disjoint calls vs one")
        c.upload_scene(d); c.update_triangles_subset(r.tris[h0], h0); c.update_triangles_subset(r.tris[h1], h1)
        _same(_arrays(c), _arrays(b), "two contexts, one sequence")
        if (name, builder) in sc.UNCLIPPED:
            for w in (0, 1, 2, 4):
                assert once[w].tobytes() == full[w].tobytes(), f"unclipped case: array {w} differs from the full update's"
            print(f"{name}/{builder}: {int((once[3] != full[3]).any(1).sum())} of {once[3].shape[0]} wide nodes keep a grid other than the full update's")
        else:
            assert once[0].tobytes() != full[0].tobytes(), "a clipped case equals the full update: the call forwards to it"
    finally:
        a.close(); b.close(); c.close()


def test_full_and_subset_updates_interleaved_in_one_context():
    """The two calls are two modes over one context's stamps, epoch, staging buffers and device copy of the triangles: in either order they leave
    what the host's BVH::refit / BVH::refitSubset leave, and a full update leaves no history behind, of stamps either."""
    import torch
    name = "spatial_splits-o0"                               # clipped leaves: a subset result differs from a full one
    d = sc.built(name, "sbvh")
    P = rc.SCENES[name]
    idx, P2 = sc.S(name)
    h0, h1 = idx[::2], idx[1::2]
    first = rc.moved(d, P2).tris[h0]
    PT = rc.deform(P, "smooth")
    rT = host.refit_bvh(rc.with_shading(rc.moved(d, PT)))    # T: every triangle moved and re-shaded
    PF = sc.translated(PT, h1, sc.standard_shift(P))         # then h1 moved again, by the standard shift, and re-shaded with other draws
    m = copy.copy(rT)
    m.tris, m.nodes = rT.tris.copy(), rT.nodes.copy()
    m.tris[h1] = sc.with_shading_on(rc.moved(rT, PF), h1, seed=7).tris[h1]
    r = host.refit_bvh_subset(m, h1)
    a, b, f = _ctx(256), _ctx(256), _ctx(256)
    try:
        # A: upload, subset(h0) from a device source, full(T) and subset(h1) from host sources (the staging buffers are shared)
        a.upload_scene(d)
        t = torch.from_numpy(np.frombuffer(first.tobytes(), np.uint8).copy()).cuda()
        i = torch.from_numpy(h0.astype(np.int32)).cuda()
        a.update_triangles_subset(t, i, on_device=True)
        a.update_triangles(rT.tris)
        before = _arrays(a)
        a.update_triangles_subset(r.tris[h1], h1)
        after = _arrays(a)
        # B: upload, full(T), the same last call
        b.upload_scene(d); b.update_triangles(rT.tris); b.update_triangles_subset(r.tris[h1], h1)
        _same(after, _arrays(b), "subset, full, subset vs full, subset")
        f.upload_scene(r)
        nb, nw, _ = _check_subset(before, after, d, r, h1, f.tree_read(2))
        assert 0 < nb < after[0].shape[0] and 0 < nw
        # the full call again, on what the subset call left: exactly "upload, full(final triangle set)"
        a.update_triangles(r.tris)
        f.upload_scene(d); f.update_triangles(r.tris)
        _same(_arrays(a), _arrays(f), "full after subset vs upload, full")
    finally:
        a.close(); b.close(); f.close()


# ---------------------------------------------------------------------------------------------------------------------------------
def _parity(d, idx, r, what):
    from oracle.binding import OracleContext
    orig, dirs, tmax, gen, names = _rays_and_witness(r)
    v = tc.BruteForce(tc.tri_points(r), orig, dirs, tmax).verdict(r)
    assert not v["uncovered"], f"robust hits outside every leaf box of their triangle: {v['uncovered'][:3]}"
    n = orig.shape[0]
    g, o = _ctx(n), OracleContext(n, threads=16)
    try:
        o.upload_scene(r)
        g.upload_scene(r)                                   # precondition: today's code on the subset-refit nodes
        tgr._compare(g, o, r, orig, dirs, tmax, gen, names, v, f"{what}/fresh")
        g.upload_scene(d)
        g.update_triangles_subset(r.tris[idx], idx)
        tgr._compare(g, o, r, orig, dirs, tmax, gen, names, v, f"{what}/subset")
    finally:
        g.close()
        o.close()


@pytest.mark.parametrize("name,builder", sc.CASES + [("spatial_splits-o1e5", "sbvh")])
def test_subset_parity_with_oracle_and_brute_force(name, builder):
    d, idx, r = _case(name, builder, shading=False)
    _parity(d, idx, r, f"{name}/{builder}")


def test_subset_parity_one_leaf_scene():
    P, d = rc.two_triangle_scene()
    idx = np.array([1], np.uint32)
    # (each vertex stays the box's extreme on exactly one axis side: refit_cases.two_triangle_scene)
    r = host.refit_bvh_subset(rc.moved(d, sc.translated(P, idx, (409.6, 409.6, -409.6))), idx)
    _parity(d, idx, r, "two_triangles")


# ---------------------------------------------------------------------------------------------------------------------------------
def _render_case():
    """test_gpu_refit._render_pair with a third of its triangles moved and re-shaded: (d, index list, the result with the subset-refit nodes)"""
    d, full = tgr._render_pair()
    idx = np.arange(0, d.tris.size, 3, dtype=np.uint32)
    m = copy.copy(d)
    m.tris = d.tris.copy()
    m.tris[idx] = full.tris[idx]
    m.nodes = d.nodes.copy()
    return d, idx, host.refit_bvh_subset(m, idx)


@pytest.mark.parametrize("integrator", ["wavefront", "microkernel"])
def test_subset_render_equals_fresh_upload_bit_for_bit(integrator):
    d, idx, r = _render_case()
    W = H = 64
    p = common.scene_params(r, W, H, maxBounces=4, wfSeparateQueues=1)
    a, b = _ctx(W * H), _ctx(W * H)
    try:
        a.upload_scene(d); a.update_triangles_subset(r.tris[idx], idx)
        b.upload_scene(r)
        for k in ("fuse_set", "ext_order", "regroup"):       # the update keeps what the upload of P chose; the fresh upload of the result gets the same
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


def test_subset_cost_is_below_the_full_updates():
    d, idx, r = _case("spatial_splits-o0", "sbvh")
    ctxs = [_ctx(256) for _ in range(4)]
    try:
        for c in ctxs:
            c.upload_scene(d)
        fresh = ctxs[0].tree_cost()
        for c in ctxs[:2]:
            c.update_triangles_subset(r.tris[idx], idx)
        for c in ctxs[2:]:
            c.update_triangles(r.tris)
        sub, sub2, full, full2 = (c.tree_cost() for c in ctxs)
        vb = [tree_cost_value(x[0]) for x in (fresh, sub, full)]
        vw = [tree_cost_value(x[1]) for x in (fresh, sub, full)]
        print(f"binary tree cost: fresh {vb[0]:.3f}, subset update {vb[1]:.3f}, full update {vb[2]:.3f}")
        print(f"4-wide tree cost: fresh {vw[0]:.3f}, subset update {vw[1]:.3f}, full update {vw[2]:.3f}")
        assert vb[1] < vb[2], "the subset update's binary tree costs no less than the full update's: the clipped leaves were not kept"
        assert sub == sub2 and full == full2
        _same(_arrays(ctxs[0]), _arrays(ctxs[1]), "subset update, second context")
        _same(_arrays(ctxs[2]), _arrays(ctxs[3]), "full update, second context")
    finally:
        for c in ctxs:
            c.close()


def test_wide_far_follows_the_whole_resulting_set():
    name = "flat_walls-o0"
    P = rc.SCENES[name]
    d = rc.built(P, "sbvh")
    idx = np.arange(300, 350, dtype=np.uint32)                 # the table: its box and the second top (traversal_cases.flat_walls)
    assert P.shape[0] == 356 and (np.abs(P[idx] - (-0.25, 0.5, 0.0)) <= (0.75, 0.5, 0.5)).all() and np.abs(P).max() < 2.0 ** 26
    far = host.refit_bvh_subset(rc.moved(d, sc.translated(P, idx, (2.0 ** 40, 0.0, 0.0))), idx)
    back = host.refit_bvh_subset(rc.moved(far, P), idx)
    from oracle.binding import OracleContext
    rays = {k: _rays_and_witness(s) for k, s in (("far", far), ("back", back))}
    n = rays["far"][0].shape[0]
    assert rays["back"][0].shape[0] == n
    g, o = _ctx(n), OracleContext(n, threads=16)
    try:
        g.upload_scene(d)
        assert g.get_option("wide_far") == 0
        with pytest.raises(RuntimeError, match="unknown option"):
            g.set_option("wide_far", 1)
        for k, s, want in (("far", far, 1), ("back", back, 0)):
            g.update_triangles_subset(s.tris[idx], idx)
            assert g.get_option("wide_far") == want, f"{k}: the clamp does not follow the resulting triangle set"
            orig, dirs, tmax, gen, names = rays[k]
            v = tc.BruteForce(tc.tri_points(s), orig, dirs, tmax).verdict(s)
            assert not v["uncovered"]
            o.upload_scene(s)
            tgr._compare(g, o, s, orig, dirs, tmax, gen, names, v, f"{name}/table {k}")
            assert g.get_option("wide_far") == want
    finally:
        g.close(); o.close()


# ---------------------------------------------------------------------------------------------------------------------------------
def test_subset_update_launches_deferred_work_on_the_old_scene_first():
    d, idx, r = _render_case()
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
            c.update_triangles_subset(r.tris[idx], idx)
            assert c.get_option("phase") & 7 == 0
            c.wf_raygen(); c.wf_materials(); c.wf_extend(); c.wf_shadow(); c.clear_queues(); c.finish()
        assert not common.state_diff(ctxs[1].state_export(), ctxs[0].state_export(), 0.0, 0.0)
        # (the fused pass splats in another order than the separate kernels: float atomics, common.fb_close's bound)
        assert common.fb_close(ctxs[1].read_pixels(0), ctxs[0].read_pixels(0))
    finally:
        for c in ctxs:
            c.close()


def test_subset_update_drops_the_adaptive_list_and_the_reprojection_history():
    d, idx, r = _render_case()
    W = H = 32
    g = _ctx(W * H)
    try:
        g.set_option("moments", 1)
        g.upload_scene(d); g.set_params(common.scene_params(d, W, H)); g.mk_reset()
        g.mk_active_write([0, 5, 9])
        assert g.mk_active_read()[0].tolist() == [0, 5, 9]
        g.gbuffer(); g.history_capture(); g.gbuffer()
        g.reproject()
        g.update_triangles_subset(r.tris[idx], idx)
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


def test_subset_device_source_equals_host_source_and_nothing_listed_changes_nothing():
    import torch
    d, idx, r = _render_case()
    a, b = _ctx(256), _ctx(256)
    try:
        a.upload_scene(d)
        before = _arrays(a)
        a.update_triangles_subset(r.tris[:0], idx[:0])
        _same(_arrays(a), before, "count == 0")
        a.update_triangles_subset(r.tris[idx], idx)
        t = torch.from_numpy(np.frombuffer(r.tris[idx].tobytes(), np.uint8).copy()).cuda()
        i = torch.from_numpy(idx.astype(np.int32)).cuda()
        b.upload_scene(d); b.update_triangles_subset(t, i, on_device=True)
        _same(_arrays(a), _arrays(b), "device source vs host source")
        after = _arrays(a)
        a.update_triangles_subset(r.tris[:0], idx[:0])
        b.update_triangles_subset(t[:0], i[:0], on_device=True)
        _same(_arrays(a), after, "count == 0 after an update")
        _same(_arrays(b), after, "count == 0 from a device source")
    finally:
        a.close(); b.close()


def test_refused_subset_updates_leave_trees_and_render_as_before():
    good = rc.built(rc.SCENES["flat_walls-o0"], "sbvh")
    idx, P2 = sc.S("flat_walls-o0")
    new = rc.moved(good, P2).tris[idx]
    W = H = 64
    p = common.scene_params(good, W, H, maxBounces=4, wfSeparateQueues=1)
    from fluctus_amd import wire
    wire.look_at(p, (0.0, 1.5, 1.8), (0.0, 0.5, 0.0))        # inside the room, as the area light is

    def edited(edit):
        t = new.copy()
        edit(t)
        return t

    def nan(t): t["v1"]["p"]["y"][7] = np.nan
    def inf(t): t["v2"]["p"]["x"][0] = np.inf
    def far(t): t["v0"]["p"]["z"][t.size - 1] = -2.0 ** 63
    def mat(t): t["matId"][3] = good.materials.size
    def neg(t): t["matId"][3] = -1
    swapped, dup, out = idx.copy(), idx.copy(), idx.copy()
    swapped[[2, 3]] = swapped[[3, 2]]
    dup[5] = dup[4]
    out[-1] = good.tris.size
    every = np.arange(good.tris.size + 1, dtype=np.uint32)
    refusals = [(edited(nan), idx, "NaN or infinite"), (edited(inf), idx, "NaN or infinite"), (edited(far), idx, r"beyond \+-2\^62"),
                (edited(mat), idx, "material id out of range"), (edited(neg), idx, "material id out of range"),
                (new, swapped, "not strictly ascending"), (new, dup, "not strictly ascending"), (new, out, "index out of range"),
                (np.zeros(every.size, new.dtype), every, "more triangles listed than the uploaded scene has")]
    g = _ctx(W * H)
    try:
        with pytest.raises(RuntimeError, match="upload a scene first"):
            g.update_triangles_subset(new, idx)
        g.upload_scene(good); g.set_params(p)
        g.set_option("extend_tree", 2)

        def look():
            driver.render_single(g, p, 2)                    # the microkernel integrator: every pixel takes its two samples, whatever it hits
            return g.read_pixels(0).tobytes(), [a.tobytes() for a in _arrays(g)], g.get_option("wide_far")

        ref = look()
        px = np.frombuffer(ref[0], np.float32).reshape(-1, 4)
        assert (px[:, 3] == 2.0).all() and px[:, :3].sum() > 0
        for t, i, msg in refusals:
            with pytest.raises(RuntimeError, match=msg):
                g.update_triangles_subset(t, i)
            assert look() == ref, f"after the refusal '{msg}' the context no longer renders the old scene"
        import ctypes as C
        for args in ((None, C.c_void_p(idx.ctypes.data)), (C.c_void_p(new.ctypes.data), None)):
            assert g.L.flx_update_triangles_subset(g.h, args[0], args[1], C.c_size_t(idx.size), 0) != 0
            assert "null triangles or indices" in g.L.flx_last_error(g.h).decode()
        assert look() == ref
        g.update_triangles_subset(new, idx)                  # and a good call still goes through
        g.finish()
        assert look()[1] != ref[1]
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# Tracer (tests/test_gpu_rebuild.py's scene and idiom)
poses = tgb.poses


def _drawer(tris):
    """a compact part of the kitchen: the 2 % of the triangles whose centroid lies nearest (Chebyshev) the median centroid; (indices, extent)"""
    P = np.stack([np.stack([tris[v]["p"][k] for k in "xyz"], -1) for v in ("v0", "v1", "v2")], 1).astype(np.float64)
    c = P.mean(1)
    dist = np.abs(c - np.median(c, 0)).max(1)
    idx = np.nonzero(dist <= np.quantile(dist, 0.02))[0].astype(np.uint32)
    assert 8 <= idx.size < P.shape[0] // 4, idx.size
    return idx, float((P.max((0, 1)) - P.min((0, 1))).max())


def _shifted(tris, idx, dx):
    t = tris[idx].copy()
    for v in ("v0", "v1", "v2"):
        t[v]["p"]["x"] = np.float32(t[v]["p"]["x"] + np.float32(dx))
    return t


def _mirrored(tris, stride=8):
    """every `stride`-th triangle translated so that its centroid lands on the mirror image through the scene's centre: the root box hardly moves,
    every box above a listed triangle spans the room"""
    P = np.stack([np.stack([tris[v]["p"][k] for k in "xyz"], -1) for v in ("v0", "v1", "v2")], 1).astype(np.float64)
    idx = np.arange(0, tris.size, stride, dtype=np.uint32)
    shift = (P.min((0, 1)) + P.max((0, 1))) - 2.0 * P[idx].mean(1)
    t = tris[idx].copy()
    for v in ("v0", "v1", "v2"):
        for j, k in enumerate("xyz"):
            t[v]["p"][k] = np.float32(t[v]["p"][k] + shift[:, j])
    return t, idx


def _by_hand(built_for, calls, full=None):
    """a fresh context: upload(build_bvh(built_for)) [+ update_triangles(full)] + update_triangles_subset for every (tris, idx) of calls"""
    g = _ctx(256)
    try:
        d = copy.copy(built_for)
        host.build_bvh(d, "sbvh")
        g.upload_scene(d)
        if full is not None:
            g.update_triangles(full)
        for t, i in calls:
            g.update_triangles_subset(t, i)
        return [g.tree_read(w).tobytes() for w in range(5)]
    finally:
        g.close()


def test_tracer_subset_update_equals_a_context_driven_by_hand(poses):
    t = tgb._tracer()
    try:
        idx, ext = _drawer(poses["P0"].tris)
        m1 = _shifted(poses["P0"].tris, idx, 0.02 * ext)
        t.update_geometry_subset(m1, idx)
        tgb._same(tgb._trees(t), _by_hand(poses["P0"], [(m1, idx)]), "one subset move")
        want = poses["P0"].tris.copy(); want[idx] = m1
        assert t.triangles().tobytes() == want.tobytes()
        assert t.rebuild_count == 0 and not t.rebuild_pending and math.isnan(t.last_cost_ratio)
        m2 = _shifted(m1, np.arange(idx.size), 0.02 * ext)
        t.update_geometry_subset(m2, idx)
        tgb._same(tgb._trees(t), _by_hand(poses["P0"], [(m1, idx), (m2, idx)]), "two subset moves")
        with pytest.raises(RuntimeError, match="not strictly ascending"):
            t.update_geometry_subset(m2, idx[::-1])
        tgb._same(tgb._trees(t), _by_hand(poses["P0"], [(m1, idx), (m2, idx)]), "after a refused move")
        want[idx] = m2
        assert t.triangles().tobytes() == want.tobytes()
        t.render_single(2)
        assert t.read_pixels(0)[:, 3].min() == 2.0
    finally:
        t.close()


def test_tracer_blocking_policy_rebuilds_on_a_subset_move_past_the_threshold(poses):
    t = tgb._tracer()
    try:
        far, idx = _mirrored(poses["P0"].tris)
        t.set_rebuild_policy("blocking", 1.0 + 1e-9)
        t.update_geometry_subset(far, idx)
        assert t.rebuild_count == 1 and not t.rebuild_pending and t.last_cost_ratio == 1.0
        now = copy.copy(poses["P0"]); now.tris = poses["P0"].tris.copy(); now.tris[idx] = far
        assert t.triangles().tobytes() == now.tris.tobytes()
        tgb._same(tgb._trees(t), tgb._fresh(now), "blocking / subset move")
    finally:
        t.close()


def test_tracer_background_job_adopted_after_a_later_subset_move(poses):
    t = tgb._tracer()
    try:
        far, idx = _mirrored(poses["P0"].tris)
        ext = _drawer(poses["P0"].tris)[1]
        t.hold_rebuild(True)
        t.set_rebuild_policy("background", 1.0 + 1e-9)
        t.update_geometry_subset(far, idx)
        print(f"cost ratio after the subset move: {t.last_cost_ratio:.4f}")
        assert t.last_cost_ratio > 1.0 + 1e-9 and t.rebuild_pending and t.rebuild_count == 0
        snap = copy.copy(poses["P0"]); snap.tris = poses["P0"].tris.copy(); snap.tris[idx] = far
        farther = _shifted(far, np.arange(idx.size), 0.02 * ext)
        t.update_geometry_subset(farther, idx)               # a later subset move while the job is in flight: only refits
        assert t.rebuild_pending and t.rebuild_count == 0
        tgb._same(tgb._trees(t), _by_hand(poses["P0"], [(far, idx), (farther, idx)]), "background / in flight")
        t.wait_for_rebuild()
        t.update()                                           # adopted here: the fresh build, then a FULL refit to the current triangles
        assert t.rebuild_count == 1 and not t.rebuild_pending
        cur = snap.tris.copy(); cur[idx] = farther
        assert t.triangles().tobytes() == cur.tobytes()
        tgb._same(tgb._trees(t), tgb._fresh(snap, cur), "background / adopted")
    finally:
        t.close()
