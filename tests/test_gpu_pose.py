"""flx_objects_define / flx_objects_pose on the device: objects over the uploaded triangles moved by a matrix each; their triangles are produced on
the GPU from the rest pose kept there (csrc/pose.hip, csrc/flx_pose.h) and handed to the subset refit as a device source.

The reference of everything here is the code as it was: context B gets `update_triangles_subset(host.pose_triangles(...), members of the listed
objects)` -- the same arithmetic on the CPU (tests/test_pose.py pins it against a numpy restatement), through the host source of the parent's call.
  equivalence  every case x object map x transform: all five flx_tree_read arrays byte-equal, "wide_far" equal, all eight flx_tree_cost numbers equal
  algebra      X then Y = Y; two objects in one call = in two calls; twenty rotations then identity = one identity pose (no drift); an empty
               object or an empty list changes no byte; an unlisted object keeps its pose; two contexts agree
  compaction   the gridded scene (tests/pose_cases.py: seven blocks of members, runs that begin and end inside a wave, whole unlisted waves between):
               flx_objects_read = numpy's compaction; both / the first / the second object listed = context B, for the runs and the interleaved map
  render       "upload, define, pose" = "upload, subset update with host-posed triangles": framebuffer and state bit for bit, both integrators
  boundary     a deferred flx_wf_logic runs on the old scene first; the adaptive list and the reprojection history are dropped; every refusal names
               its cause and leaves trees, render and a following valid pose as they were; an upload drops the definition, a second one replaces it
  Tracer       pose_objects against a HipContext driven by hand; under the Blocking and Background rebuild policies; define_objects() from an OBJ
"""
import copy
import numpy as np
import pytest
import common
import refit_cases as rc
import refit_subset_cases as sc
import pose_cases as pc
import test_gpu_refit as tgr
import test_gpu_rebuild as tgb
from fluctus_amd import host, driver, wire

pytestmark = pytest.mark.gpu
_ctx, _arrays = tgr._ctx, tgr._arrays
NO = pc.NO_OBJECT


def _look(g):
    """(the five arrays' bytes, wide_far, the eight cost numbers)"""
    return [a.tobytes() for a in _arrays(g)], g.get_option("wide_far"), g.tree_cost()


def _same(a, b, what):
    for w, (x, y) in enumerate(zip(a[0], b[0])):
        assert x == y, f"{what}: tree array {w} differs"
    assert a[1] == b[1], f"{what}: wide_far {a[1]} vs {b[1]}"
    assert a[2] == b[2], f"{what}: tree cost {a[2]} vs {b[2]}"


def _by_subset(g, rest, omap, ids, xfs):
    """the parent's path: the listed objects' members posed on the host, in through update_triangles_subset's host source"""
    idx, t = pc.posed(rest, omap, ids, xfs)
    g.update_triangles_subset(t, idx)
    return idx


def _xfs(T, tname, count):
    """the transform of the object at list position k: the named one, then the following ones -- every listed object moves differently"""
    i = pc.TRANSFORM_NAMES.index(tname)
    return np.stack([T[pc.TRANSFORM_NAMES[(i + k) % len(pc.TRANSFORM_NAMES)]] for k in range(count)]) if count else np.zeros((0, 3, 4), np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,builder", pc.CASES)
@pytest.mark.parametrize("kind", pc.MAP_NAMES)
def test_pose_equals_subset_update_with_host_posed_triangles(name, builder, kind):
    d = pc.case(name, builder)
    T = pc.transforms(rc.SCENES[name])
    omap, nobj, ids = pc.object_map(kind, d.tris.size)
    a, b = _ctx(256), _ctx(256)
    try:
        for tname in pc.TRANSFORM_NAMES:
            xfs = _xfs(T, tname, len(ids))
            a.upload_scene(d); a.objects_define(d.tris, omap, nobj)
            fresh = [x.tobytes() for x in _arrays(a)]
            a.objects_pose(ids, xfs)
            b.upload_scene(d)
            idx = _by_subset(b, d.tris, omap, ids, xfs)
            assert idx.size == int((omap != NO).sum())
            la, lb = _look(a), _look(b)
            _same(la, lb, f"{name}/{kind}/{tname}")
            if tname != "identity":
                assert la[0][1] != fresh[1], f"{name}/{kind}/{tname}: the pose moved nothing"
    finally:
        a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------------------------
def test_pose_algebra():
    name, builder = "spatial_splits-o0", "sbvh"
    d = pc.case(name, builder)
    T = pc.transforms(rc.SCENES[name])
    omap, nobj, _ = pc.object_map("interleaved", d.tris.size)
    X, Y, Z = T["rotation"], T["shear"], T["translation"]
    a, b = _ctx(256), _ctx(256)

    def start(g, m=omap, n=nobj):
        g.upload_scene(d); g.objects_define(d.tris, m, n)

    try:
        # X then Y = Y alone: a pose is absolute, and it is the same dirty set
        start(a); a.objects_pose([0], [X]); a.objects_pose([0], [Y])
        start(b); b.objects_pose([0], [Y])
        _same(_look(a), _look(b), "X then Y vs Y")
        # two objects in one call = the same two in two calls
        start(a); a.objects_pose([0, 1], [X, Y])
        start(b); b.objects_pose([1], [Y]); b.objects_pose([0], [X])
        both = _look(a)
        _same(both, _look(b), "one call vs two")
        # an unlisted object keeps its last pose
        a.objects_pose([0], [Z])
        start(b); b.objects_pose([0, 1], [Z, Y])
        _same(_look(a), _look(b), "object 1 not listed in the second call")
        # a second context, the same sequence
        start(b); b.objects_pose([0, 1], [X, Y]); b.objects_pose([0], [Z])
        _same(_look(a), _look(b), "two contexts, one sequence")
        # twenty successive rotations, then identity = one identity pose: nothing drifts
        start(a)
        for k in range(20):
            a.objects_pose([0, 1], [pc.about(pc.rotation((1.0, 2.0, 3.0), 0.3 * (k + 1)), (0.1, -0.2, 0.3))] * 2)
        a.objects_pose([0, 1], [pc.IDENTITY] * 2)
        start(b); b.objects_pose([0, 1], [pc.IDENTITY] * 2)
        _same(_look(a), _look(b), "twenty rotations then identity vs identity")
        # ... which gives back the rest triangles (unit normals: bit for bit), not the clipped leaves the first pose unclipped
        b.upload_scene(d)
        fresh = _look(b)
        assert _look(a)[0][2] == fresh[0][2] and _look(a)[0][1] == fresh[0][1], "identity does not restore the shading and triangle records"
        assert _look(a)[0][0] != fresh[0][0], "no SBVH leaf was unclipped: the case does not show what identity does not restore"
        # nothing listed, or only an object without a triangle: no byte changes
        m2, n2, _ = pc.object_map("single_and_empty", d.tris.size)
        start(a, m2, n2); a.objects_pose([0, 2], [X, Y])
        before = _look(a)
        a.objects_pose([], np.zeros((0, 3, 4), np.float32))
        _same(_look(a), before, "count == 0")
        a.objects_pose([1], [Z])
        _same(_look(a), before, "only an empty object listed")
    finally:
        a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["runs", "interleaved"])
def test_compaction_on_the_gridded_scene(kind):
    d = pc.grid_case()
    P = pc.grid_positions()
    T = pc.transforms(P)
    omap, nobj = pc.grid_map(d.tris.size) if kind == "runs" else pc.object_map("interleaved", d.tris.size)[:2]
    members = np.nonzero(omap != NO)[0].astype(np.uint32)
    assert d.tris.size >= 1500 and members.size > 4 * 256
    if kind == "runs":                                       # the shapes the count, scan and scatter can go wrong at (pose_cases.grid_map)
        first = np.nonzero(omap[members] == 0)[0]
        runs = np.split(first, np.nonzero(np.diff(first) > 1)[0] + 1)
        assert len(runs) == 2 and all(r[0] % 64 and (r[-1] + 1) % 64 for r in runs) and runs[1][0] - runs[0][-1] - 1 > 64
    a, b = _ctx(256), _ctx(256)
    try:
        a.upload_scene(d); a.objects_define(d.tris, omap, nobj)
        counts, got = a.objects_read()
        assert counts.tolist() == [int((omap == o).sum()) for o in range(nobj)]
        assert np.array_equal(got, members)
        for ids in ([0, 1], [0], [1]):
            xfs = _xfs(T, "rotation", len(ids))
            a.upload_scene(d); a.objects_define(d.tris, omap, nobj); a.objects_pose(ids, xfs)
            b.upload_scene(d)
            idx = _by_subset(b, d.tris, omap, ids, xfs)      # (ascending, or the subset refit had refused the device's list as it would this one)
            assert (np.diff(idx.astype(np.int64)) > 0).all()
            _same(_look(a), _look(b), f"grid/{kind}/objects {ids}")
    finally:
        a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------------------------
def _render_case():
    """test_gpu_refit's render scene, its triangles in three interleaved classes: two objects and the rest; (scene, map, ids, transforms)"""
    d = common.mixed_material_scene()
    omap, nobj, ids = pc.object_map("interleaved", d.tris.size)
    ctr = (0.0, 0.5, 0.0)
    xfs = np.stack([pc.about(pc.rotation((0.2, 1.0, 0.1), 0.5) * 0.8, ctr), pc.about(np.diag([-1.0, 1.0, 1.0]), ctr) + pc.affine(np.zeros((3, 3)), (0.1, 0.05, 0.0))])
    return d, omap, nobj, ids, xfs


@pytest.mark.parametrize("integrator", ["wavefront", "microkernel"])
def test_pose_render_equals_subset_update_bit_for_bit(integrator):
    d, omap, nobj, ids, xfs = _render_case()
    W, H = 64, 48
    p = common.scene_params(d, W, H, maxBounces=4, wfSeparateQueues=1)
    a, b = _ctx(W * H), _ctx(W * H)
    try:
        a.upload_scene(d); a.objects_define(d.tris, omap, nobj); a.objects_pose(ids, xfs)
        b.upload_scene(d); _by_subset(b, d.tris, omap, ids, xfs)
        for c in (a, b):
            c.set_option("extend_tree", 2)
            c.set_params(p)
            if integrator == "wavefront":
                driver.reset_renderer(c)
                for _ in range(3):
                    driver.benchmark_iteration(c, W * H)
            else:
                driver.render_single(c, p, 2)
        pa, pb = a.read_pixels(0), b.read_pixels(0)
        assert pa[:, 3].sum() > 0 and pa[:, :3].sum() > 0
        assert pa.tobytes() == pb.tobytes(), f"{int((pa != pb).any(1).sum())} pixels differ"
        assert not common.state_diff(a.state_export(), b.state_export(), 0.0, 0.0)
        b.upload_scene(d); b.set_params(p)                   # and the pose shows: the unposed scene renders another image
        if integrator == "microkernel":
            driver.render_single(b, p, 2)
            assert b.read_pixels(0).tobytes() != pa.tobytes()
    finally:
        a.close(); b.close()


def test_pose_launches_deferred_work_on_the_old_scene_first():
    d, omap, nobj, ids, xfs = _render_case()
    W, H = 64, 48
    p = common.scene_params(d, W, H, maxBounces=4, wfSeparateQueues=1)
    ctxs = [_ctx(W * H), _ctx(W * H)]
    try:
        for fuse, c in enumerate(ctxs):
            c.set_option("fuse", fuse); c.set_option("extend_tree", 2)
            c.upload_scene(d); c.objects_define(d.tris, omap, nobj); c.set_params(p); driver.reset_renderer(c)
            for _ in range(2):
                driver.benchmark_iteration(c, W * H)
            c.wf_logic(False)
            if fuse:
                assert c.get_option("phase") & 7 == 1, "flx_wf_logic was not deferred: the test does not reach the boundary"
            c.objects_pose(ids, xfs)
            assert c.get_option("phase") & 7 == 0
            c.wf_raygen(); c.wf_materials(); c.wf_extend(); c.wf_shadow(); c.clear_queues(); c.finish()
        assert not common.state_diff(ctxs[1].state_export(), ctxs[0].state_export(), 0.0, 0.0)
        # (the fused pass splats in another order than the separate kernels: float atomics, common.fb_close's bound)
        assert common.fb_close(ctxs[1].read_pixels(0), ctxs[0].read_pixels(0))
    finally:
        for c in ctxs:
            c.close()


def test_pose_drops_the_adaptive_list_and_the_reprojection_history():
    d, omap, nobj, ids, xfs = _render_case()
    W = H = 32
    g = _ctx(W * H)
    try:
        g.set_option("moments", 1)
        g.upload_scene(d); g.objects_define(d.tris, omap, nobj); g.set_params(common.scene_params(d, W, H)); g.mk_reset()
        g.mk_active_write([0, 5, 9])
        assert g.mk_active_read()[0].tolist() == [0, 5, 9]
        g.gbuffer(); g.history_capture(); g.gbuffer()
        g.reproject()
        g.objects_pose(ids, xfs)
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


def test_refused_calls_leave_trees_render_and_later_poses_as_they_were():
    good = pc.shaded(rc.built(rc.SCENES["flat_walls-o0"], "sbvh"))
    T = pc.transforms(rc.SCENES["flat_walls-o0"])
    omap, nobj, _ = pc.object_map("single_and_empty", good.tris.size)
    W, H = 64, 48
    p = common.scene_params(good, W, H, maxBounces=4, wfSeparateQueues=1)
    wire.look_at(p, (0.0, 1.5, 1.8), (0.0, 0.5, 0.0))        # inside the room, as the area light is
    X, Y = T["rotation"], T["translation"]

    def edited(i, v):
        m = X.copy(); m.flat[i] = v
        return m

    singular = pc.affine(np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 1.0, 0.0]]))
    refusals = [([2, 0], [X, Y], "not strictly ascending"), ([0, 0], [X, Y], "not strictly ascending"), ([0, 3], [X, Y], "object id out of range"),
                ([0, 1, 2, 3], [X] * 4, "more objects listed than are defined"),
                ([0, 2], [X, edited(5, np.nan)], "NaN or infinite entry"), ([0, 2], [edited(3, np.inf), Y], "NaN or infinite entry"),
                ([2], [singular], "zero or non-finite determinant"), ([2], [pc.affine(np.zeros((3, 3)))], "zero or non-finite determinant"),
                ([0, 2], [X, pc.affine(None, (0.0, -2.0 ** 63, 0.0))], r"beyond \+-2\^62"),
                ([2], [pc.affine(np.diag([2.0 ** 127, 1.0, 2.0 ** -120]))], "NaN or infinite vertex")]
    g, f = _ctx(W * H), _ctx(W * H)
    try:
        with pytest.raises(RuntimeError, match="flx_objects_pose: upload a scene first"):
            g.objects_pose([0], [X])
        with pytest.raises(RuntimeError, match="flx_objects_define: upload a scene first"):
            g.objects_define(good.tris, omap, nobj)
        g.upload_scene(good); g.set_params(p); g.set_option("extend_tree", 2)
        with pytest.raises(RuntimeError, match="flx_objects_pose: no objects are defined"):
            g.objects_pose([0], [X])
        with pytest.raises(RuntimeError, match="flx_objects_read: no objects are defined"):
            g.objects_read()
        g.objects_define(good.tris, omap, nobj)
        g.objects_pose([2], [Y])                             # a pose is in place: a refusal must leave it, not the rest pose

        def look():
            driver.render_single(g, p, 2)                    # the microkernel integrator: every pixel takes its two samples, whatever it hits
            return g.read_pixels(0).tobytes(), [a.tobytes() for a in _arrays(g)], g.get_option("wide_far"), [a.tobytes() for a in g.objects_read()]

        ref = look()
        px = np.frombuffer(ref[0], np.float32).reshape(-1, 4)
        assert (px[:, 3] == 2.0).all() and px[:, :3].sum() > 0
        for ids, xfs, msg in refusals:
            with pytest.raises(RuntimeError, match="flx_objects_pose: .*" + msg):
                g.objects_pose(ids, xfs)
            assert look() == ref, f"after the refusal '{msg}' the context no longer renders the scene as posed before"
        # a refused definition keeps the one in place
        bad = omap.copy(); bad[11] = nobj
        for args, msg in (((good.tris[:-1], omap[:-1], nobj), "triangle count differs"), ((good.tris, bad, nobj), "triangle 11 has an object id")):
            with pytest.raises(RuntimeError, match="flx_objects_define: .*" + msg):
                g.objects_define(*args)
            assert look() == ref
        import ctypes as C
        assert g.L.flx_objects_define(g.h, None, C.c_size_t(good.tris.size), C.c_void_p(omap.ctypes.data), C.c_uint32(nobj)) != 0
        assert "null triangles or object ids" in g.L.flx_last_error(g.h).decode()
        assert g.L.flx_objects_pose(g.h, None, None, C.c_uint32(1)) != 0
        assert "null object ids or transforms" in g.L.flx_last_error(g.h).decode()
        assert look() == ref
        # ... and a following valid pose gives what it gives in a context that met no refusal
        g.objects_pose([0], [X])
        f.upload_scene(good); f.objects_define(good.tris, omap, nobj); f.objects_pose([2], [Y]); f.objects_pose([0], [X])
        _same(_look(g), _look(f), "a valid pose after the refusals")
        assert look()[1] != ref[1]
    finally:
        g.close(); f.close()


def test_upload_drops_the_definition_and_a_second_one_replaces_the_first():
    name, builder = "mixed_scale-o0", "sbvh"
    d = pc.case(name, builder)
    T = pc.transforms(rc.SCENES[name])
    m1, n1, _ = pc.object_map("interleaved", d.tris.size)
    m2, n2, _ = pc.object_map("single_and_empty", d.tris.size)
    a, b = _ctx(256), _ctx(256)
    try:
        a.upload_scene(d)
        fresh = [x.tobytes() for x in _arrays(a)]
        a.objects_define(d.tris, m1, n1)
        assert [x.tobytes() for x in _arrays(a)] == fresh, "defining objects changed a tree"
        a.objects_pose([1], [T["shear"]])
        a.objects_define(d.tris, m2, n2)                     # replaces: object 0 is now one triangle; the pose object 1 of the first map took stays
        counts, members = a.objects_read()
        assert counts.tolist() == [1, 0, d.tris.size - d.tris.size // 2] and np.array_equal(members, np.nonzero(m2 != NO)[0])
        a.objects_pose([0], [T["rotation"]])
        b.upload_scene(d); _by_subset(b, d.tris, m1, [1], [T["shear"]]); _by_subset(b, d.tris, m2, [0], [T["rotation"]])
        _same(_look(a), _look(b), "second definition")
        with pytest.raises(RuntimeError, match="object id out of range"):
            a.objects_pose([3], [T["shear"]])
        a.objects_define(None, None, 0)                      # nobjects == 0 drops it
        with pytest.raises(RuntimeError, match="no objects are defined"):
            a.objects_pose([0], [T["shear"]])
        a.objects_define(d.tris, m1, n1)
        a.upload_scene(d)                                    # and so does an upload
        with pytest.raises(RuntimeError, match="no objects are defined"):
            a.objects_pose([0], [T["shear"]])
        assert [x.tobytes() for x in _arrays(a)] == fresh
    finally:
        a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# Tracer (tests/test_gpu_rebuild.py's scene and idiom)
poses = tgb.poses


def _tracer_objects(tris):
    """two objects over the kitchen: every eighth triangle from 0 and from 4; (map, nobjects, centre, extent)"""
    o = np.full(tris.size, NO, np.uint32)
    o[0::8] = 0; o[4::8] = 1
    P = np.stack([np.stack([tris[v]["p"][k] for k in "xyz"], -1) for v in pc.VERTS], 1).astype(np.float64)
    return o, 2, 0.5 * (P.min((0, 1)) + P.max((0, 1))), sc.extent(P)


def _by_hand(built_for, rest, omap, nobj, calls, full=None):
    """a fresh context: upload(build_bvh(built_for)) [+ update_triangles(full)] + objects_define(rest) + objects_pose for every (ids, xforms)"""
    g = _ctx(256)
    try:
        d = copy.copy(built_for)
        host.build_bvh(d, "sbvh")
        g.upload_scene(d)
        if full is not None:
            g.update_triangles(full)
        g.objects_define(rest, omap, nobj)
        for ids, xfs in calls:
            g.objects_pose(ids, xfs)
        return [g.tree_read(w).tobytes() for w in range(5)]
    finally:
        g.close()


def _posed_scene(base, rest, omap, calls):
    """a copy of scene `base` whose triangles are base's with every call's members replaced by their pose from `rest`"""
    m = copy.copy(base); m.tris = base.tris.copy()
    for ids, xfs in calls:
        idx, t = pc.posed(rest, omap, ids, xfs)
        m.tris[idx] = t
    return m


def test_tracer_pose_equals_a_context_driven_by_hand(poses):
    t = tgb._tracer()
    try:
        rest = poses["P0"].tris
        omap, nobj, ctr, ext = _tracer_objects(rest)
        with pytest.raises(RuntimeError, match="no objects are defined"):
            t.pose_objects([0], [pc.IDENTITY])
        assert t.define_objects(omap, nobj) == 2
        c1 = ([0, 1], np.stack([pc.about(pc.rotation((0.0, 1.0, 0.0), 0.3), ctr), pc.affine(None, (0.02 * ext, 0.0, 0.0))]))
        c2 = ([1], np.stack([pc.affine(None, (0.0, 2.0 * ext, 0.0))]))
        t.pose_objects(*c1)
        tgb._same(tgb._trees(t), _by_hand(poses["P0"], rest, omap, nobj, [c1]), "one pose")
        assert t.triangles().tobytes() == _posed_scene(poses["P0"], rest, omap, [c1]).tris.tobytes()
        t.pose_objects(*c2)                                  # object 1 leaves the room: the root box, and worldRadius with it, follow the host tree
        tgb._same(tgb._trees(t), _by_hand(poses["P0"], rest, omap, nobj, [c1, c2]), "two poses")
        now = _posed_scene(poses["P0"], rest, omap, [c1, c2])
        assert t.triangles().tobytes() == now.tris.tobytes()
        h = copy.copy(poses["P0"]); host.build_bvh(h, "sbvh")
        r0 = h.world_radius
        h.tris = now.tris
        host.refit_bvh_subset(h, np.nonzero(omap != NO)[0])
        assert float(t.params["worldRadius"]) == np.float32(h.world_radius) and h.world_radius > 1.5 * r0
        with pytest.raises(RuntimeError, match="not strictly ascending"):
            t.pose_objects([1, 0], np.stack([pc.IDENTITY, pc.IDENTITY]))
        tgb._same(tgb._trees(t), _by_hand(poses["P0"], rest, omap, nobj, [c1, c2]), "after a refused pose")
        assert t.triangles().tobytes() == now.tris.tobytes()
        t.render_single(2)
        assert t.read_pixels(0)[:, 3].min() == 2.0
    finally:
        t.close()


def _far_pose(ctr, ext):
    """both objects mirrored through the scene's centre and pushed apart: every box above a member spans the room"""
    return ([0, 1], np.stack([pc.about(-np.eye(3), ctr), pc.about(np.diag([-1.0, 1.0, -1.0]), ctr)]))


def test_tracer_blocking_policy_rebuilds_on_a_pose_and_keeps_the_objects(poses):
    t = tgb._tracer()
    try:
        rest = poses["P0"].tris
        omap, nobj, ctr, ext = _tracer_objects(rest)
        t.define_objects(omap, nobj)
        t.set_rebuild_policy("blocking", 1.0 + 1e-9)
        far = _far_pose(ctr, ext)
        t.pose_objects(*far)
        assert t.rebuild_count == 1 and not t.rebuild_pending and t.last_cost_ratio == 1.0
        now = _posed_scene(poses["P0"], rest, omap, [far])
        assert t.triangles().tobytes() == now.tris.tobytes()
        tgb._same(tgb._trees(t), tgb._fresh(now), "blocking / pose")
        # the objects survive the swap, with their REST pose: a further (small) pose only refits the rebuilt topology
        t.set_rebuild_policy("blocking", 1e6)
        nxt = ([0], np.stack([pc.about(-np.eye(3), ctr) + pc.affine(np.zeros((3, 3)), (0.01 * ext, 0.0, 0.0))]))
        t.pose_objects(*nxt)
        assert t.rebuild_count == 1
        tgb._same(tgb._trees(t), _by_hand(now, rest, omap, nobj, [nxt]), "blocking / a pose after the swap")
        assert t.triangles().tobytes() == _posed_scene(now, rest, omap, [nxt]).tris.tobytes()
    finally:
        t.close()


def test_tracer_background_job_adopted_after_a_later_pose(poses):
    t = tgb._tracer()
    try:
        rest = poses["P0"].tris
        omap, nobj, ctr, ext = _tracer_objects(rest)
        t.define_objects(omap, nobj)
        t.hold_rebuild(True)
        t.set_rebuild_policy("background", 1.0 + 1e-9)
        far = _far_pose(ctr, ext)
        t.pose_objects(*far)
        print(f"cost ratio after the pose: {t.last_cost_ratio:.4f}")
        assert t.last_cost_ratio > 1.0 + 1e-9 and t.rebuild_pending and t.rebuild_count == 0
        snap = _posed_scene(poses["P0"], rest, omap, [far])
        later = ([1], np.stack([pc.about(np.diag([-1.0, 1.0, -1.0]), ctr) + pc.affine(np.zeros((3, 3)), (0.0, 0.02 * ext, 0.0))]))
        t.pose_objects(*later)                               # while the job is in flight: only refits
        assert t.rebuild_pending and t.rebuild_count == 0
        tgb._same(tgb._trees(t), _by_hand(poses["P0"], rest, omap, nobj, [far, later]), "background / in flight")
        t.wait_for_rebuild()
        t.update()                                           # adopted here: the fresh build, then a FULL refit to the pose of this moment
        assert t.rebuild_count == 1 and not t.rebuild_pending
        cur = _posed_scene(snap, rest, omap, [later])
        assert t.triangles().tobytes() == cur.tris.tobytes()
        tgb._same(tgb._trees(t), tgb._fresh(snap, cur.tris), "background / adopted")
        t.set_rebuild_policy("off")
        nxt = ([0], np.stack([pc.affine(None, (0.01 * ext, 0.0, 0.0))]))
        t.pose_objects(*nxt)                                 # the objects are still defined, over the rest pose
        tgb._same(tgb._trees(t), _by_hand(snap, rest, omap, nobj, [nxt], full=cur.tris), "background / a pose after the swap")
    finally:
        t.close()


def test_tracer_defines_the_objects_of_an_obj_file(tmp_path):
    from fluctus_amd.tracer import Tracer
    sheets = {"floor": pc.grid_positions()[:200], "lid": pc.grid_positions()[200:320] + (0.0, 1.0, 0.0)}
    lines, nv = [], 0
    for nm, P in sheets.items():
        lines.append(f"o {nm}")
        for tri in P:
            lines += ["v %.6f %.6f %.6f" % tuple(v) for v in tri] + [f"f {nv + 1} {nv + 2} {nv + 3}"]
            nv += 3
    path = tmp_path / "two.obj"
    path.write_text("\n".join(lines) + "\n")
    d = host.load_scene(str(path))
    assert d.object_names == ["floor", "lid"] and d.object_of_triangle.tolist() == [0] * 200 + [1] * 120
    W, H = 32, 24
    t = Tracer(W, H, 0, W * H)
    try:
        t.init(W, H, str(path))
        assert t.triangles().tobytes() == d.tris.tobytes()
        assert t.define_objects() == 2
        X = pc.about(pc.rotation((0.0, 1.0, 0.0), 0.4), (0.0, 1.0, 0.0))
        t.pose_objects([1], [X])
        want = d.tris.copy()
        want[200:] = host.pose_triangles(d.tris[200:], X)
        assert t.triangles().tobytes() == want.tobytes()
        tgb._same(tgb._trees(t), _by_hand(d, d.tris, d.object_of_triangle, 2, [([1], np.stack([X]))]), "OBJ objects")
    finally:
        t.close()
