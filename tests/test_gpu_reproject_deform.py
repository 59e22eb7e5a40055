"""Option "deform_history" on the device: flx_reproject across per-triangle moves bit for bit against
tests/reproject_deform_cpu.cpp through the write hooks, the barycentric plane of flx_gbuffer, the lazy snapshot of the positions at the capture,
the boundary (tests/feature_state_deform_cases.py through the C ABI), the neutrality of the option (nothing moved, the option off, a running
wavefront chain) and the end-to-end quality with exact sample counts.

Measured on an MI355X: see test_quality_end_to_end_exact_spp's docstring and DESIGN.md 4.3.6."""
import types
import numpy as np
import pytest
import common
import pose_cases as pc
import reproject_reference as R
import reproject_deform_reference as D
import feature_state_deform_cases as fs
import test_reproject_deform as trd
from fluctus_amd import driver, wire

pytestmark = pytest.mark.gpu
NOBARY = trd.NOBARY


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return D.build_cpu(tmp_path_factory.mktemp("reproject_deform_gpu"))


def _ctx(d, p, n, **opts):
    from fluctus_amd.device import HipContext
    g = HipContext(n)
    for k, v in opts.items():
        g.set_option(k, v)
    g.upload_scene(d)
    g.set_params(p)
    return g


def _same_u32(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def positions(tris):
    """(n, 3, 3) float32: the three positions of every wire triangle"""
    return np.stack([np.stack([tris[v]["p"][k] for k in "xyz"], 1) for v in ("v0", "v1", "v2")], 1).astype(np.float32)


def with_positions(tris, idx, P):
    """a copy of the wire triangles with the positions of triangles idx replaced by P (len(idx), 3, 3)"""
    t = tris.copy()
    P = np.asarray(P, np.float32)
    for j, v in enumerate(("v0", "v1", "v2")):
        for k, c in enumerate("xyz"):
            col = t[v]["p"][c]; col[idx] = P[:, j, k]
    return t


def bent(tris, sel, a):
    """the selected triangles bent by the smooth non-affine field x += a (y - y0)^2, y0 their lowest vertex"""
    P = positions(tris)[sel].astype(np.float64)
    y0 = P[:, :, 1].min()
    P[:, :, 0] += a * (P[:, :, 1] - y0) ** 2
    return with_positions(tris, np.nonzero(sel)[0], P)


# ---------------------------------------------------------------------------------------------------------------------------------
def test_option_and_hooks():
    W, H = 16, 12
    d = common.mixed_material_scene()
    g = _ctx(d, common.scene_params(d, W, H), W * H)
    assert g.get_option("deform_history") == 0
    with pytest.raises(RuntimeError, match="unknown option"):
        g.set_option("deform_history", 2)
    g.gbuffer()
    with pytest.raises(RuntimeError, match="no barycentric plane"):
        g.gbuffer_bary_read(0)
    with pytest.raises(RuntimeError, match="deform_history"):
        g.gbuffer_bary_write(0, np.zeros((W * H, 2), np.float32))
    with pytest.raises(RuntimeError, match="no snapshot"):
        g.deform_read(d.tris.size)
    g.set_option("motion_history", 1)
    with pytest.raises(RuntimeError, match="motion_history"):
        g.set_option("deform_history", 1)
    g.set_option("motion_history", 0); g.set_option("deform_history", 1)
    with pytest.raises(RuntimeError, match="deform_history"):
        g.set_option("motion_history", 1)
    assert g.get_option("deform_history") == 1 and g.get_option("motion_history") == 0
    g.gbuffer()
    plane = g.gbuffer_bary_read(0)
    gb, cam = g.gbuffer_read(0)
    idx, al = gb[:, 3].copy().view(np.int32), g.params["areaLight"]["N"]
    light = (idx == 0) & (gb[:, 4] == al["x"]) & (gb[:, 5] == al["y"]) & (gb[:, 6] == al["z"])      # the implicit quad: a hit that names no triangle
    tri = (idx >= 0) & ~light
    assert (plane[tri] >= 0).all() and (plane[tri].sum(1) <= 1.0 + 1e-5).all() and (plane[~tri] == NOBARY).all() and tri.any() and not tri.all()
    g.gbuffer_write(0, gb, cam)                              # a written G-buffer names no triangle ...
    assert (g.gbuffer_bary_read(0) == NOBARY).all()
    b = np.random.default_rng(1).uniform(0, 0.5, (W * H, 2)).astype(np.float32)
    g.gbuffer_bary_write(0, b)                               # ... until the barycentrics are written behind it
    assert np.array_equal(g.gbuffer_bary_read(0), b)
    with pytest.raises(RuntimeError, match="slot must be"):
        g.gbuffer_bary_write(2, b)
    g.history_capture()                                      # the plane goes with its slot
    assert np.array_equal(g.gbuffer_bary_read(1), b)
    with pytest.raises(RuntimeError, match="no barycentric plane"):
        g.gbuffer_bary_read(0)
    g.set_option("deform_history", 0)                        # off: the planes are nobody's
    with pytest.raises(RuntimeError, match="no barycentric plane"):
        g.gbuffer_bary_read(1)
    g.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# scene triangles that stand in for the analytic ones: [rectangle a, b (moved; a is triangle 0, the index the light quad is stored with), wall a, b
# (unmoved), second rectangle a (unmoved), b (moved: a seam inside one rectangle), sliver a, b (b degenerate at the capture)]
STAND_INS = np.array([0, 1, 300, 17, 40, 41, 400, 401])


def _adversarial(exe, d, W, H, moments):
    """the CPU tests' wall and rectangles under two cameras, laid over eight triangles of the uploaded scene: a moved rectangle, the unmoved wall, a
    rectangle with a moved and an unmoved half, a triangle degenerate at the capture, light-quad pixels (hit index 0, the sentinel), hit indices
    beyond the triangle count, NaN / inf / empty history taps, a turned normal, a non-finite current position and non-finite barycentrics"""
    ca, cb = R.camera((0.0, 0.0, 4.0), (0.0, 0.0, 0.0)), R.camera((0.3, 0.1, 3.8), (0.1, 0.0, 0.0), 55.0)
    X, Y = trd.X, trd.Y
    wall = D.tri_quad((0.0, 0.0, 0.0), X, Y, 2.0, 50.0)                              # narrow: misses left and right of it
    q1 = D.tri_quad((-0.9, -0.4, 0.8), X, Y, 0.4, 0.3)
    sl = D.tri_quad((-0.8, 0.7, 0.6), X, Y, 0.35, 0.3)
    light = D.tri_quad((1.0, 0.8, 1.0), X, Y, 0.3, 0.3)
    s = trd.px_step(H, dist=3.0) if H > 1 else 0.05
    q1n = q1.copy(); q1n[1] += (0.4 * s, 0.0, 0.0)
    slc = sl.copy(); slc[1, 2] = 0.5 * (slc[1, 0] + slc[1, 1])
    cap = np.concatenate([trd.QUAD, wall, q1, slc, light])
    now = np.concatenate([trd.shifted(trd.QUAD, 1.7 * s, -0.8 * s), wall, q1n, sl, light])
    c = trd.Case(exe, W, H, ca, cb, cap, now, seed=W + H, moments=moments)
    # analytic triangle k -> scene triangle; the light's two triangles -> hit index 0 with the sentinel
    ntris = d.tris.size
    for g, bary in ((c.prev, c.pbary), (c.cur, c.cbary)):
        k = g[:, 3].copy().view(np.int32)
        lit = k >= 8
        bary[lit] = NOBARY
        g[:, 3] = np.where(k < 0, k, np.where(lit, 0, STAND_INS[np.clip(k, 0, 7)])).astype(np.int32).view(np.float32)
    tA, tB = with_positions(d.tris, STAND_INS, c.cap[:8]), with_positions(d.tris, STAND_INS, c.now[:8])
    c.cap, c.now = positions(tA), positions(tB)
    rng = np.random.default_rng(W + H + 1)
    N, k = W * H, max(1, W * H // 40)
    c.hist[rng.choice(N, k), 0] = np.nan; c.hist[rng.choice(N, k), 1] = np.inf; c.hist[rng.choice(N, k), 3] = 0.0
    if moments:
        c.mom[rng.choice(N, k), 3] = 0.0; c.mom[rng.choice(N, k), 0] = np.nan
    c.prev[rng.choice(N, k), 4:7] = (0.6, 0.0, 0.8)
    c.cur[rng.choice(N, k), 0] = np.nan
    c.cbary[rng.choice(N, k), 0] = np.nan; c.cbary[rng.choice(N, k), 1] = np.inf
    if N > 1:
        for g in (c.prev, c.cur):                            # hit indices that name no triangle of this scene
            sel = rng.choice(N, k)
            g[sel, 3] = np.where(g[sel, 3].copy().view(np.int32) >= 0, np.int32(ntris + 5), np.int32(-1)).astype(np.int32).view(np.float32)
    c.ps, c.cs = c.prev[:, 3].copy().view(np.int32), c.cur[:, 3].copy().view(np.int32)
    return c, tA, tB


@pytest.mark.parametrize("moments", [1, 0])
@pytest.mark.parametrize("W,H", [(1, 1), (17, 13), (64, 48)])
def test_reproject_deform_bit_identical_to_cpu(exe, W, H, moments):
    d = common.simple_scene()
    g = _ctx(d, common.scene_params(d, W, H), 4096, moments=moments, deform_history=1)
    c, tA, tB = _adversarial(exe, d, W, H, bool(moments))
    g.update_triangles(tA)
    g.write_pixels(0, c.hist)
    if moments:
        g.write_pixels(7, c.mom)
    g.gbuffer_write(0, c.prev, c.cam_a); g.gbuffer_bary_write(0, c.pbary)
    g.history_capture()
    g.update_triangles(tB)                                   # snapshots A, keeps the capture
    g.gbuffer_write(0, c.cur, c.cam_b); g.gbuffer_bary_write(0, c.cbary)
    g.mk_reset()
    for kw in ({}, dict(max_history=5.0, plane_tolerance_px=0.5, normal_cos=0.5, min_weight=0.3)):
        g.reproject(**kw); g.finish()
        cpx, cmom, _, _ = c.run(check=False, **kw)
        px = g.read_pixels(0)
        assert _same_u32(px, cpx), int((px.view(np.uint32) != cpx.view(np.uint32)).any(1).sum())
        if moments:
            assert _same_u32(g.read_pixels(7), cmom)
    snap, moved = g.deform_read(d.tris.size)
    assert _same_u32(snap, c.cap) and np.array_equal(moved, c.moved)
    assert sorted(np.nonzero(moved)[0].tolist()) == [0, 1, 41, 401]
    if W * H > 1:
        assert (px[c.cs == 1, 3] > 0).any() and (px[c.cs == 300, 3] > 0).any() and (px[c.cs == 40, 3] > 0).any()
        assert not px[(c.cs == 401) & np.isfinite(c.cbary).all(1) & (c.cbary[:, 0] != NOBARY)].any()
    g.close()


# ---------------------------------------------------------------------------------------------------------------------------------
def _light_view(d, W, H):
    """a camera that sees the spheres, the ground and the area light's quad (x = 1.6, facing -x)"""
    p = common.scene_params(d, W, H, useAreaLight=1)
    wire.look_at(p, (-1.5, 1.2, 2.5), (0.8, 0.9, 0.0))
    return p


def _bary_error(gb, plane, P, fov, H):
    """per triangle-hit pixel: |bary(u, v, p0, p1, p2) - G0's P| in float64, in units of the pixel footprint at the hit (t * 2 tan(fov / 2) / H)"""
    idx = gb[:, 3].copy().view(np.int32)
    on = (idx >= 0) & (plane[:, 0] != NOBARY)
    u, v = plane[on, 0].astype(np.float64)[:, None], plane[on, 1].astype(np.float64)[:, None]
    p = P[idx[on]].astype(np.float64)
    at = (1.0 - u - v) * p[:, 0] + u * p[:, 1] + v * p[:, 2]
    foot = gb[on, 7].astype(np.float64) * 2.0 * np.tan(np.radians(float(fov)) / 2.0) / H
    return np.linalg.norm(at - gb[on, :3].astype(np.float64), axis=1) / foot, on


@pytest.mark.parametrize("tree", [2, 4])
@pytest.mark.parametrize("tasks", [64 * 48, 320])
def test_gbuffer_bary_plane(tree, tasks):
    """G0 / G1 byte-equal to the option off; the sentinel exactly on misses and on the area light's pixels; in float64 bary(u, v, p0, p1, p2)
    lies within 0.01 pixel footprints of G0's P (a condition from the use: two orders under the plane tolerance of 2 pixels; the float64
    brute force meets it on this scene, tests/test_reproject_deform.py); 320 paths for 3072 pixels: the striding loop"""
    W, H = 64, 48
    d = common.mixed_material_scene()
    p = _light_view(d, W, H)
    off, on = _ctx(d, p, tasks, extend_tree=tree), _ctx(d, p, tasks, extend_tree=tree, deform_history=1)
    for g in (off, on):
        g.gbuffer(); g.finish()
    ga, gb = off.gbuffer_read(0)[0], on.gbuffer_read(0)[0]
    assert _same_u32(ga, gb)
    plane = on.gbuffer_bary_read(0)
    idx = gb[:, 3].copy().view(np.int32)
    al = p["areaLight"]["N"]
    light = (idx == 0) & (gb[:, 4] == al["x"]) & (gb[:, 5] == al["y"]) & (gb[:, 6] == al["z"])
    miss = idx < 0
    assert light.sum() > 10 and miss.any()
    none = (plane[:, 0] == NOBARY) & (plane[:, 1] == NOBARY)
    assert np.array_equal(none, light | miss)
    tri = ~none
    assert (plane[tri] >= 0).all() and (plane[tri].sum(1) <= 1.0 + 1e-5).all()
    err, on_tri = _bary_error(gb, plane, positions(d.tris), p["camera"]["fov"], H)
    print(f"tree {tree}, {tasks} paths: {int(light.sum())} area-light pixels, {int(miss.sum())} misses, {int(tri.sum())} triangle pixels; "
          f"|bary(u, v) - P| at most {err.max():.2e} pixel footprints")
    assert np.array_equal(on_tri, tri) and err.max() <= 0.01
    with pytest.raises(RuntimeError, match="no barycentric plane"):
        off.gbuffer_bary_read(0)
    off.close(); on.close()


# ---------------------------------------------------------------------------------------------------------------------------------
def _history(g, W, H, seed=5):
    """a known accumulation, its G-buffer and the capture"""
    hist, mom = R.random_history(W * H, seed)
    g.write_pixels(0, hist)
    if g.get_option("moments"):
        g.write_pixels(7, mom)
    g.gbuffer(); g.history_capture()
    return hist


def _shapes(d):
    """three shapes of mixed_material_scene: A as uploaded, B with the first sphere bent, C with the first sphere bent further and the second bent too"""
    m = d.tris["matId"]
    A = d.tris.copy()
    B = bent(A, m == 3, 0.3)
    C = bent(bent(A, m == 3, 0.5), m == 4, -0.2)
    return A, B, C


@pytest.mark.parametrize("how", ["full", "subset", "device", "pose"])
def test_snapshot_is_taken_once_per_capture_and_before_the_move(how):
    """capture under A, update A -> B, update B -> C: flx_deform_read returns A's positions (the first move copied them aside before the refit
    overwrote them, the second kept that copy) and flags exactly the triangles whose positions differ between A and C; through the full update,
    the subset update, a device source and flx_objects_pose; after the next capture the next move snapshots again"""
    import torch
    W, H = 32, 24
    d = common.mixed_material_scene()
    g = _ctx(d, common.scene_params(d, W, H), W * H, deform_history=1)
    A, B, C = _shapes(d)
    n = A.size
    if how == "pose":
        m = d.tris["matId"].astype(np.int64)
        omap = np.where(m >= 3, m - 3, 0xFFFFFFFF).astype(np.uint32)
        g.objects_define(A, omap, 6)
        XB, XC = pc.affine(None, (0.1, 0.0, 0.0)), pc.affine(None, (0.2, 0.05, 0.0))
        from fluctus_amd import host
        B = A.copy(); B[omap == 0] = host.pose_triangles(A[omap == 0], XB)
        C = B.copy(); C[omap == 0] = host.pose_triangles(A[omap == 0], XC); C[omap == 1] = host.pose_triangles(A[omap == 1], XB)
    hist = _history(g, W, H)
    with pytest.raises(RuntimeError, match="no snapshot"):
        g.deform_read(n)
    def move(T, prev):
        ch = np.nonzero((positions(T).view(np.uint32) != positions(prev).view(np.uint32)).any((1, 2)))[0].astype(np.uint32)
        if how == "full":
            g.update_triangles(T)
        elif how == "subset":
            g.update_triangles_subset(T[ch], ch)
        elif how == "device":
            g.update_triangles(torch.from_numpy(np.frombuffer(T.tobytes(), np.uint8).copy()).cuda(), on_device=True)
        elif T is B:
            g.objects_pose([0], [XB])
        else:
            g.objects_pose([0, 1], [XC, XB])
    move(B, A)
    snap, moved = g.deform_read(n)
    assert _same_u32(snap, positions(A)) and np.array_equal(moved, D.moved_flags(positions(B), positions(A))) and moved.any() and not moved.all()
    move(C, B)
    snap, moved = g.deform_read(n)
    assert _same_u32(snap, positions(A)), "the second move overwrote the snapshot"
    assert np.array_equal(moved, D.moved_flags(positions(C), positions(A)))
    assert _same_u32(g.read_pixels(0), hist)                 # the moves touched no framebuffer
    g.gbuffer(); g.mk_reset(); g.reproject(); g.finish()
    assert (g.read_pixels(0)[:, 3] > 0).mean() > 0.5
    g.history_capture()                                      # the next capture: the snapshot is of the past
    with pytest.raises(RuntimeError, match="no snapshot"):
        g.deform_read(n)
    if how != "pose":
        move(A, C)
        snap, moved = g.deform_read(n)
        assert _same_u32(snap, positions(C)) and np.array_equal(moved, D.moved_flags(positions(A), positions(C)))
    g.close()


def test_refused_update_leaves_no_snapshot_and_keeps_the_history():
    W, H = 32, 24
    d = common.mixed_material_scene()
    g = _ctx(d, common.scene_params(d, W, H), W * H, deform_history=1)
    A, B, _ = _shapes(d)
    hist = _history(g, W, H)
    bad = B.copy(); bad["v1"]["p"]["y"][7] = np.nan
    with pytest.raises(RuntimeError, match="NaN or infinite"):
        g.update_triangles(bad)
    with pytest.raises(RuntimeError, match="not strictly ascending"):
        g.update_triangles_subset(B[:2], np.array([1, 0], np.uint32))
    with pytest.raises(RuntimeError, match="no snapshot"):
        g.deform_read(A.size)
    g.gbuffer(); g.mk_reset(); g.reproject(); g.finish()     # the history is there, and nothing moved: the identity
    got = g.read_pixels(0)
    hit = g.gbuffer_read(0)[0][:, 3].copy().view(np.int32) >= 0
    # (the fp32 projection lands within 1e-4 pixel of the pixel's own centre, so a neighbour's count of 1 .. 40 enters with a weight below 1e-4: 4e-3)
    assert np.allclose(got[hit, 3], np.minimum(hist[hit, 3], 32.0), rtol=4e-3) and not got[~hit].any()
    g.close()


# ---------------------------------------------------------------------------------------------------------------------------------
class Run:
    """tests/feature_state_deform_cases.py through the C ABI, the flags read off the refusals as tests/test_gpu_feature_state.py reads its own"""
    def __init__(self, d):
        from fluctus_amd.device import HipContext
        self.d, self.g = d, HipContext(256)
        self.g.upload_scene(d)
        self.size(fs.W0, fs.H0)
        self.bad = d.tris.copy(); self.bad["v0"]["p"]["x"][3] = np.nan

    def size(self, W, H):
        self.p = common.scene_params(self.d, W, H)
        self.g.set_params(self.p)
        self.blank = np.zeros((W * H, 8), np.float32)
        self.blank[:, 3] = np.array([-1], np.int32).view(np.float32)[0]          # every pixel a miss

    def event(self, e):
        g, d, k = self.g, self.d, e[0]
        if k == "refused":
            with pytest.raises(RuntimeError, match=e[2]):
                self.event(e[1])
        elif k == "opt": g.set_option(e[1], e[2])
        elif k == "define":
            m = d.tris["matId"].astype(np.int64)
            g.objects_define(d.tris, np.where((m >= 3) & (m < 3 + e[1]), m - 3, 0xFFFFFFFF).astype(np.uint32), e[1])
        elif k == "pose": g.objects_pose([0], [pc.affine(None, (0.1, 0.0, 0.0))])
        elif k == "gbuffer": g.gbuffer()
        elif k == "capture": g.history_capture()
        elif k == "gb_write": g.gbuffer_write(e[1], self.blank, self.p["camera"])
        elif k == "bary_write": g.gbuffer_bary_write(e[1], np.full((self.blank.shape[0], 2), NOBARY, np.float32))
        elif k == "reproject": g.reproject(); g.finish()
        elif k == "upload": g.upload_scene(d)
        elif k == "update": g.update_triangles(d.tris)
        elif k == "update_nan": g.update_triangles(self.bad)
        elif k == "subset": g.update_triangles_subset(d.tris[:e[1]], np.arange(e[1], dtype=np.uint32))
        elif k == "resize": self.size(e[1], e[2])
        else: raise ValueError(e)

    def flags(self):
        """(T0, T1, B0, B1, H, S).  H last, it changes the state: a snapshot stands on a history; without one the option goes off (which then
        keeps the history), both slots are written and flx_reproject is refused for the want of a history or runs"""
        g = self.g
        def refuses(call, message):
            try:
                call()
            except RuntimeError as err:
                assert message in str(err), str(err)
                return True
            return False
        T = [int(not refuses(lambda: g.gbuffer_read(s), "the slot holds no G-buffer")) for s in (0, 1)]
        B = [int(not refuses(lambda: g.gbuffer_bary_read(s), "no barycentric plane")) for s in (0, 1)]
        S = int(not refuses(lambda: g.deform_read(self.d.tris.size), "no snapshot"))
        if S:
            return (T[0], T[1], B[0], B[1], 1, 1)
        g.set_option("deform_history", 0); g.set_option("motion_history", 0)
        for s in (0, 1):
            g.gbuffer_write(s, self.blank, self.p["camera"])
        Hh = int(not refuses(g.reproject, "no captured history"))
        g.finish()
        return (T[0], T[1], B[0], B[1], Hh, 0)


@pytest.fixture(scope="module")
def scene():
    d = common.mixed_material_scene()
    d.tris.setflags(write=False)
    return d


@pytest.mark.parametrize("case", fs.CASES, ids=[c["name"] for c in fs.CASES])
def test_boundary_sequence(scene, case):
    r = Run(scene)
    try:
        for e in case["events"]:
            r.event(e)
        got = r.flags()
    finally:
        r.g.close()
    assert got == case["expect"], (case["name"], got)


# ---------------------------------------------------------------------------------------------------------------------------------
def test_nothing_moved_equals_the_option_off_and_off_an_update_drops_the_history():
    """(a) the option on and no move: flx_reproject is k_reproject's call; (b) the option on and a move that changed no bit: the snapshot exists,
    k_moved_flags finds nothing, and k_reproject_deform's framebuffer and moments are byte-equal to the option off -- the property that pins the
    design, on the device; (c) the option off: an update drops the history, exactly as before"""
    W, H = 48, 36
    d = common.mixed_material_scene()
    p = common.scene_params(d, W, H)
    pb = common.scene_params(d, W, H)
    wire.look_at(pb, (0.12, 1.65, 3.15), (0.03, 0.5, 0.0))
    on, off = _ctx(d, p, W * H, moments=1, deform_history=1), _ctx(d, p, W * H, moments=1)
    for g in (on, off):
        g.update_triangles(d.tris)                           # both render over refitted trees
        _history(g, W, H)
    for g in (on, off):
        g.set_params(pb); g.gbuffer(); g.mk_reset(); g.reproject(); g.finish()
    a0, a7 = off.read_pixels(0), off.read_pixels(7)
    assert _same_u32(on.read_pixels(0), a0) and _same_u32(on.read_pixels(7), a7) and (a0[:, 3] > 0).mean() > 0.5
    for g in (on, off):
        g.set_params(p); _history(g, W, H)
    on.update_triangles(d.tris)                              # the same bytes: a move that moved nothing
    assert not on.deform_read(d.tris.size)[1].any()
    for g in (on, off):
        g.set_params(pb); g.gbuffer(); g.mk_reset(); g.reproject(); g.finish()
    b0 = off.read_pixels(0)
    assert _same_u32(on.read_pixels(0), b0) and _same_u32(on.read_pixels(7), off.read_pixels(7)) and (b0[:, 3] > 0).mean() > 0.5
    _history(off, W, H)
    off.update_triangles(d.tris); off.gbuffer(); off.mk_reset()
    with pytest.raises(RuntimeError, match="no captured history"):
        off.reproject()
    on.close(); off.close()


def test_new_calls_leave_the_run_alone():
    """test_gbuffer_leaves_the_run_alone with the option on: flx_gbuffer (writing the plane) and the plane's read hook at every position of an
    iteration leave counters and exported state bit for bit, the framebuffer within common.fb_close (float atomics)"""
    W, H = 64, 48
    d = common.mixed_material_scene()
    p = common.scene_params(d, W, H, maxBounces=4, wfSeparateQueues=1)
    a, b = _ctx(d, p, W * H, extend_tree=2), _ctx(d, p, W * H, extend_tree=2, deform_history=1)
    for g in (a, b):
        driver.reset_renderer(g)
    for it in range(4):
        cnts = []
        for g, probe in ((a, False), (b, True)):
            steps = [lambda: g.wf_logic(False), g.wf_raygen, g.wf_materials, g.wf_extend, g.wf_shadow, g.clear_queues]
            cnt = None
            for k, s in enumerate(steps):
                if probe:
                    g.gbuffer(); g.gbuffer_bary_read(0)
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
    assert np.array_equal(pa[:, 3], pb[:, 3]) and common.fb_close(pa, pb)
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------------------------
def test_quality_end_to_end_exact_spp():
    """mixed_material_scene 80 x 60, microkernel integrator through the C ABI, useRoulette 0.  Shape A: the diffuse sphere in front of the row;
    shape B: that sphere bent by x += a (y - y0)^2, its top displaced by 0.15 = about 3 pixels (DESIGN.md 4.3.4's size of move), a field no
    matrix describes.  32 spp under A, then gbuffer, capture, flx_update_triangles(B), gbuffer, reset, reproject + 1 spp (T) against reset + 1
    spp (R); truth 512 spp under B.  On the sphere's surface pixels that received history RMSE(T) / RMSE(R) < 0.5 (DESIGN.md 4.3.3's bar; the
    ideal is 1 / sqrt(33) = 0.174); the pixels without history equal R bit for bit.
    Measured on an MI355X: ratio 0.361 on 136 pixels, 100 % of the sphere's 136 surface pixels with history (printed below)."""
    W, H = 80, 60
    d = common.mixed_material_scene()
    p = common.scene_params(d, W, H, maxBounces=4, useAreaLight=1, useRoulette=0)
    sphere = d.tris["matId"] == 3
    PA = positions(d.tris)[sphere].astype(np.float64); PA[:, :, 2] += 1.2
    A = with_positions(d.tris, np.nonzero(sphere)[0], PA)
    height = float(PA[:, :, 1].max() - PA[:, :, 1].min())
    B = bent(A, sphere, 0.15 / height ** 2)

    def ctx(T, **o):
        g = _ctx(d, p, W * H, **o)
        g.update_triangles(T)
        return g

    truth = ctx(B, denoiser=1)
    driver.render_single(truth, p, 512)
    hi, hialb = truth.read_pixels(0), truth.read_pixels(4)
    surf = hialb[:, 3] == hi[:, 3]
    ref = hi[:, :3] / hi[:, 3:4]

    t = ctx(A, deform_history=1)
    driver.render_single(t, p, 32)
    t.gbuffer(); t.history_capture()
    t.update_triangles(B)
    t.gbuffer(); t.mk_reset(); t.reproject(); t.finish()
    n1 = t.read_pixels(0)[:, 3].copy()
    idx = t.gbuffer_read(0)[0][:, 3].copy().view(np.int32)
    obj = (idx >= 0) & sphere[np.clip(idx, 0, None)] & (t.gbuffer_bary_read(0)[:, 0] != NOBARY)
    driver.render_single_pass(t, p["maxBounces"]); t.finish()
    T = t.read_pixels(0)

    r = ctx(B)
    r.mk_reset(); driver.render_single_pass(r, p["maxBounces"]); r.finish()
    Rr = r.read_pixels(0)

    got = n1 > 0
    assert R.same(T[~got], Rr[~got]), "pixels without history differ from the plain restart"
    assert np.allclose(T[got, 3], n1[got] + 1.0)
    sel = got & surf & obj
    share = float(sel.sum() / max(1, (surf & obj).sum()))
    eT = np.sqrt((((T[sel, :3] / T[sel, 3:4]) - ref[sel]) ** 2).mean())
    eR = np.sqrt((((Rr[sel, :3] / Rr[sel, 3:4]) - ref[sel]) ** 2).mean())
    print(f"deform reprojection quality: RMSE(T) {eT:.4f} / RMSE(R) {eR:.4f} = {eT / eR:.3f} on {int(sel.sum())} pixels of the bent sphere; "
          f"{100 * share:.1f} % of its {int((surf & obj).sum())} surface pixels received history; mean n' {n1[sel].mean():.1f}; "
          f"{100 * float((got & surf).sum() / surf.sum()):.1f} % of all {int(surf.sum())} surface pixels received history")
    assert sel.sum() >= 20, int(sel.sum())
    assert eT / eR < 0.5, eT / eR
    for g in (truth, t, r):
        g.close()


# ---------------------------------------------------------------------------------------------------------------------------------
def _tracer(W, H, devices=0):
    from fluctus_amd.tracer import Tracer
    t = Tracer(W, H, devices, W * H)
    t.init(W, H, "proc:kitchen:3000:7")
    return t


def _slid(tris, sel, dx):
    out = tris.copy()
    for v in ("v0", "v1", "v2"):
        col = out[v]["p"]["x"]; col[sel] += np.float32(dx)
    return out


def test_tracer_update_geometry_keeps_the_history_and_the_filter_schedule():
    """kitchen stand-in 64 x 48, the variance-guided denoiser on: ten frames, updateGeometry(all) with every triangle slid by 0.03, one frame --
    under setDeformReprojection most pixels carry more than the restart's samples and the filter schedule continues (frame 10 since the last
    discarded history: which = 6 exists), without the switch the move restarted both; then the same through updateGeometry(indices, tris) with
    half of the triangles slid back.  Measured on an MI355X: 95.7 % and 98.9 % of the pixels kept history (printed below)"""
    W, H = 64, 48
    on, off = _tracer(W, H), _tracer(W, H)
    for t in (on, off):
        t.set_temporal_reprojection(True)
        t.set_denoiser(True); t.set_denoiser_mode("variance"); t.set_denoiser_strength(1.0)
    on.set_deform_reprojection(True)
    assert on.deform_reprojection and not off.deform_reprojection
    for t in (on, off):
        for _ in range(10):
            t.update()
        t.update_geometry(_slid(t.triangles(), slice(None), 0.03))
        t.update()
    pon, poff = on.read_pixels(0), off.read_pixels(0)
    more = pon[:, 3] > poff[:, 3] + 1.0
    print(f"tracer, updateGeometry(all): {100 * more.mean():.1f} % of the pixels kept history across the move; median count {np.median(pon[:, 3]):.1f} against {np.median(poff[:, 3]):.1f}")
    assert more.mean() > 0.5 and (pon[:, 3] > 1.0).mean() > 0.5
    out = on.read_pixels(6)                                  # frame 10 since the last discarded history: the filter ran
    assert np.isfinite(out).all() and out[:, :3].any()
    with pytest.raises(RuntimeError, match="which = 6"):
        off.read_pixels(6)                                   # without the switch the move restarted the schedule
    for t in (on, off):
        for _ in range(3):
            t.update()
        n = t.triangles().size
        idx = np.arange(0, n // 2, dtype=np.uint32)
        t.update_geometry_subset(_slid(t.triangles(), slice(None), -0.03)[idx], idx)
        t.update()
    pon, poff = on.read_pixels(0), off.read_pixels(0)
    more = pon[:, 3] > poff[:, 3] + 1.0
    print(f"tracer, updateGeometry(indices, tris): {100 * more.mean():.1f} % of the pixels kept history across the move")
    assert more.mean() > 0.5
    # a refused update after the capture leaves the next frame to re-trace and reproject: nothing moved, the history is still there
    for _ in range(3):
        on.update()
    bad = on.triangles().copy(); bad["v0"]["p"]["x"][5] = np.nan
    with pytest.raises(RuntimeError, match="NaN or infinite"):
        on.update_geometry(bad)
    on.update()
    assert (on.read_pixels(0)[:, 3] > 2.0).mean() > 0.5
    on.close(); off.close()


def test_tracer_two_moves_and_a_camera_change_in_one_frame_share_one_capture():
    """kitchen stand-in 32 x 24: ten frames, then within ONE frame updateGeometry(all) sliding every triangle by 0.03, updateGeometry(indices,
    tris) sliding half of them by a further 0.03 and a camera nudge, then one update().  A second flx_history_capture in that frame would hand
    an untraced slot over, which the device refuses: the frame completing is the pin for "at most one capture per frame, shared with a pending
    camera change".  And the history survived: most pixels carry more than the restarted Tracer's samples (the neighbouring test's bound).
    Measured on an MI355X: 94.0 % of the pixels kept history (printed below)"""
    W, H = 32, 24
    on, off = _tracer(W, H), _tracer(W, H)
    for t in (on, off):
        t.set_temporal_reprojection(True)
    on.set_deform_reprojection(True)
    for t in (on, off):
        for _ in range(10):
            t.update()
        t.update_geometry(_slid(t.triangles(), slice(None), 0.03))
        idx = np.arange(0, t.triangles().size // 2, dtype=np.uint32)
        t.update_geometry_subset(_slid(t.triangles(), slice(None), 0.03)[idx], idx)
        p = t.params.copy(); p["camera"]["pos"]["x"] += 0.02; t.params = p
        t.update()
    pon, poff = on.read_pixels(0), off.read_pixels(0)
    more = pon[:, 3] > poff[:, 3] + 1.0
    print(f"tracer, two moves and a camera change in one frame: {100 * more.mean():.1f} % of the pixels kept history; "
          f"median count {np.median(pon[:, 3]):.1f} against {np.median(poff[:, 3]):.1f}")
    assert more.mean() > 0.5
    on.close(); off.close()


def test_tracer_switch_throws_in_its_three_cases():
    t = _tracer(32, 24)
    with pytest.raises(RuntimeError, match="setTemporalReprojection"):
        t.set_deform_reprojection(True)
    t.set_temporal_reprojection(True); t.set_motion_reprojection(True)
    with pytest.raises(RuntimeError, match="setMotionReprojection"):
        t.set_deform_reprojection(True)
    t.set_motion_reprojection(False); t.set_deform_reprojection(True)
    with pytest.raises(RuntimeError, match="setDeformReprojection"):
        t.set_motion_reprojection(True)
    t.set_temporal_reprojection(False)
    assert not t.deform_reprojection
    t.close()
    m = _tracer(32, 24, [0, 0])
    with pytest.raises(RuntimeError, match="single-GPU"):
        m.set_deform_reprojection(True)
    m.set_deform_reprojection(False)
    m.close()
