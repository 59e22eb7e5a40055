"""Option "motion_history" on the device: the object plane of flx_gbuffer, flx_reproject across flx_objects_pose bit for bit
against tests/reproject_motion_cpu.cpp through the write hooks, the boundary (what keeps and what drops the history), the isolation from a
running wavefront chain, the end-to-end quality with exact sample counts, and the Tracer switch.

Measured on an MI355X: see test_quality_end_to_end_exact_spp's docstring and DESIGN.md 4.3.4."""
import numpy as np
import pytest
import common
import pose_cases as pc
import reproject_reference as R
import reproject_motion_reference as M
import test_reproject_motion as trm
from fluctus_amd import driver, wire

pytestmark = pytest.mark.gpu
NO = M.NO_OBJECT
GROUND = 288                    # mixed_material_scene / simple_scene: the ground's triangles come first, the spheres (120 each) follow


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return M.build_cpu(tmp_path_factory.mktemp("reproject_motion_gpu"))


def _ctx(d, p, n, **opts):
    from fluctus_amd.device import HipContext
    g = HipContext(n)
    for k, v in opts.items():
        g.set_option(k, v)
    g.upload_scene(d)
    g.set_params(p)
    return g


def _spheres(d, ground_too=False):
    """mixed_material_scene's six spheres as objects 0..5 (matId 3 + k); ground_too: the ground's first two triangles join object 0, so that
    triangle 0 -- the hit index the area light's quad is stored with -- belongs to an object"""
    o = np.full(d.tris.size, NO, np.uint32)
    m = d.tris["matId"].astype(np.int64)
    o[m >= 3] = (m[m >= 3] - 3).astype(np.uint32)
    if ground_too:
        o[:2] = 0
    return o, 6


def _same_u32(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------------------
def test_option_and_hooks():
    W, H = 16, 12
    d = common.mixed_material_scene()
    omap, nobj = _spheres(d)
    g = _ctx(d, common.scene_params(d, W, H), W * H)
    assert g.get_option("motion_history") == 0
    with pytest.raises(RuntimeError, match="unknown option"):
        g.set_option("motion_history", 2)
    g.gbuffer()
    with pytest.raises(RuntimeError, match="no object plane"):
        g.gbuffer_objects_read(0)
    with pytest.raises(RuntimeError, match="motion_history"):
        g.gbuffer_objects_write(0, np.zeros(W * H, np.uint32))
    g.set_option("motion_history", 1)
    assert g.get_option("motion_history") == 1
    g.gbuffer()                                              # no objects are defined: still no plane
    with pytest.raises(RuntimeError, match="no object plane"):
        g.gbuffer_objects_read(0)
    g.objects_define(d.tris, omap, nobj)
    g.gbuffer()
    plane = g.gbuffer_objects_read(0)
    assert ((plane < nobj) | (plane == NO)).all() and (plane < nobj).any()
    gb, cam = g.gbuffer_read(0)
    g.gbuffer_write(0, gb, cam)                              # a written G-buffer shows no object ...
    assert (g.gbuffer_objects_read(0) == NO).all()
    ids = (np.arange(W * H) % 5).astype(np.uint32)
    g.gbuffer_objects_write(0, ids)                          # ... until the objects are written behind it
    assert np.array_equal(g.gbuffer_objects_read(0), ids)
    with pytest.raises(RuntimeError, match="slot must be"):
        g.gbuffer_objects_write(2, ids)
    g.history_capture()                                      # the plane goes with its slot
    assert np.array_equal(g.gbuffer_objects_read(1), ids)
    with pytest.raises(RuntimeError, match="no object plane"):
        g.gbuffer_objects_read(0)
    with pytest.raises(RuntimeError, match="no G-buffer of the current size"):
        g.gbuffer_objects_write(0, ids)
    g.set_option("motion_history", 0)                        # off: the planes are nobody's
    with pytest.raises(RuntimeError, match="no object plane"):
        g.gbuffer_objects_read(1)
    g.close()


# ---------------------------------------------------------------------------------------------------------------------------------
def _adversarial(exe, W, H, moments):
    """the CPU tests' wall and rectangles under two cameras: object 0 turns and shifts (posed before the capture: its pose is known), object 1
    is posed for the first time after the capture (no history), object 2 is never posed, object 3 has no pixel; the wall and a second rectangle
    belong to no object.  NaN / inf / empty history taps, a turned normal and a non-finite current position as in test_gpu_reproject.py."""
    ca, cb = R.camera((0.0, 0.0, 4.0), (0.0, 0.0, 0.0)), R.camera((0.3, 0.1, 3.8), (0.1, 0.0, 0.0), 55.0)
    wall = R.quad((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 3.0, 50.0)          # narrow: misses left and right of it
    q1 = R.quad((-0.9, -0.4, 0.8), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 0.4, 0.3)
    q2 = R.quad((-0.8, 0.7, 0.6), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 0.35, 0.3)
    light = R.quad((1.0, 0.8, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 0.3, 0.3)
    Xa = M.rotate((0, 1, 0), -8.0, trm.QUAD["c"])
    Xb = M.rotate((0, 1, 0), 10.0, trm.QUAD["c"]); Xb[:, 3] += (0.1, -0.05, 0.05)
    x_cap, x_now = [Xa, None, None, None], [Xb, M.translate(0.1, 0.05), None, None]
    c = trm.Case(exe, W, H, ca, cb, [wall, trm.QUAD, q1, q2, light], [NO, 0, 1, 2, NO], x_cap, x_now, seed=W + H, moments=moments)
    rng = np.random.default_rng(W + H + 1)
    N, k = W * H, max(1, W * H // 40)
    c.hist[rng.choice(N, k), 0] = np.nan; c.hist[rng.choice(N, k), 1] = np.inf; c.hist[rng.choice(N, k), 3] = 0.0
    if moments:
        c.mom[rng.choice(N, k), 3] = 0.0; c.mom[rng.choice(N, k), 0] = np.nan
    c.prev[rng.choice(N, k), 4:7] = (0.6, 0.0, 0.8)
    c.cur[rng.choice(N, k), 0] = np.nan
    c.cobj[rng.choice(N, k)] = 77                            # an id beyond the table reads as no object
    return c, x_cap, x_now


@pytest.mark.parametrize("moments", [1, 0])
@pytest.mark.parametrize("W,H", [(1, 1), (17, 13), (64, 48)])
def test_reproject_motion_bit_identical_to_cpu(exe, W, H, moments):
    d = common.simple_scene()
    g = _ctx(d, common.scene_params(d, W, H), 4096, moments=moments, motion_history=1)
    omap = np.full(d.tris.size, NO, np.uint32)
    omap[GROUND:GROUND + 40] = 0; omap[GROUND + 40:GROUND + 80] = 1; omap[GROUND + 80:] = 2      # (object 3: no triangle)
    g.objects_define(d.tris, omap, 4)
    c, x_cap, x_now = _adversarial(exe, W, H, bool(moments))
    assert c.any and c.table[0, 3].tolist() == [1, 0, 0, 0] and c.table[1, 3].tolist() == [1, 1, 0, 0] and not c.table[2:, 3].any()
    g.objects_pose([0], [x_cap[0]])
    g.write_pixels(0, c.hist)
    if moments:
        g.write_pixels(7, c.mom)
    g.gbuffer_write(0, c.prev, c.cam_a); g.gbuffer_objects_write(0, c.pobj)
    g.history_capture()
    g.objects_pose([0, 1], [x_now[0], x_now[1]])             # keeps the capture
    g.gbuffer_write(0, c.cur, c.cam_b); g.gbuffer_objects_write(0, c.cobj)
    g.mk_reset()
    for kw in ({}, dict(max_history=5.0, plane_tolerance_px=0.5, normal_cos=0.5, min_weight=0.3)):
        g.reproject(**kw); g.finish()
        cpx, cmom, _, _ = c.run(check=False, **kw)
        px = g.read_pixels(0)
        assert _same_u32(px, cpx), int((px.view(np.uint32) != cpx.view(np.uint32)).any(1).sum())
        if moments:
            assert _same_u32(g.read_pixels(7), cmom)
    if W * H > 1:
        moved = (c.cobj == 0) & (c.cs == 1)
        assert (px[moved, 3] > 0).any() and not px[(c.cobj == 1) & (c.cs == 2)].any() and (px[c.cs == 0, 3] > 0).any()
    g.close()


# ---------------------------------------------------------------------------------------------------------------------------------
def _light_view(d, W, H):
    """a camera that sees the spheres, the ground and the area light's quad (x = 1.6, facing -x)"""
    p = common.scene_params(d, W, H, useAreaLight=1)
    wire.look_at(p, (-1.5, 1.2, 2.5), (0.8, 0.9, 0.0))
    return p


@pytest.mark.parametrize("tasks", [64 * 48, 320])
def test_gbuffer_object_plane(tasks):
    """G0 / G1 byte-equal to the option off; the plane is object_of_triangle[hit index], FLX_NO_OBJECT on misses and on the area light's pixels
    (whose hit index 0 is a member's here); 320 paths for 3072 pixels: the striding loop"""
    W, H = 64, 48
    d = common.mixed_material_scene()
    omap, nobj = _spheres(d, ground_too=True)
    p = _light_view(d, W, H)
    off, on = _ctx(d, p, tasks, extend_tree=2), _ctx(d, p, tasks, extend_tree=2, motion_history=1)
    on.objects_define(d.tris, omap, nobj); off.objects_define(d.tris, omap, nobj)
    for g in (off, on):
        g.gbuffer(); g.finish()
    ga, gb = off.gbuffer_read(0)[0], on.gbuffer_read(0)[0]
    assert _same_u32(ga, gb)
    plane = on.gbuffer_objects_read(0)
    idx = gb[:, 3].copy().view(np.int32)
    al = p["areaLight"]["N"]
    light = (idx == 0) & (gb[:, 4] == al["x"]) & (gb[:, 5] == al["y"]) & (gb[:, 6] == al["z"])
    miss = idx < 0
    print(f"{int(light.sum())} area-light pixels, {int(miss.sum())} misses, {int((plane != NO).sum())} object pixels")
    assert light.sum() > 10 and miss.any()
    assert (plane[light] == NO).all() and (plane[miss] == NO).all()
    tri = ~light & ~miss
    assert np.array_equal(plane[tri], omap[idx[tri]])
    assert len(set(plane[tri].tolist())) >= 3                # the ground (no object) and several spheres
    with pytest.raises(RuntimeError, match="no object plane"):
        off.gbuffer_objects_read(0)
    off.close(); on.close()


def test_new_calls_leave_the_run_alone():
    """test_gbuffer_leaves_the_run_alone with the option on and objects defined: flx_gbuffer (writing the plane) and the plane's read hook at
    every position of an iteration leave counters and exported state bit for bit, the framebuffer within common.fb_close (float atomics)"""
    W, H = 64, 48
    d = common.mixed_material_scene()
    omap, nobj = _spheres(d)
    p = common.scene_params(d, W, H, maxBounces=4, wfSeparateQueues=1)
    a, b = _ctx(d, p, W * H, extend_tree=2), _ctx(d, p, W * H, extend_tree=2, motion_history=1)
    for g in (a, b):
        g.objects_define(d.tris, omap, nobj)
        driver.reset_renderer(g)
    for it in range(4):
        cnts = []
        for g, probe in ((a, False), (b, True)):
            steps = [lambda: g.wf_logic(False), g.wf_raygen, g.wf_materials, g.wf_extend, g.wf_shadow, g.clear_queues]
            cnt = None
            for k, s in enumerate(steps):
                if probe:
                    g.gbuffer(); g.gbuffer_objects_read(0)
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
POSE_A = np.stack([pc.affine(None, (0.0, 0.05 * k, 0.0)) for k in range(6)])
POSE_B = POSE_A.copy(); POSE_B[0, 0, 3] += 0.2; POSE_B[3, 2, 3] -= 0.15


def _history(g, d, W, H, seed=5):
    """a known accumulation under pose A, its G-buffer and the capture"""
    hist, mom = R.random_history(W * H, seed)
    g.write_pixels(0, hist)
    if g.get_option("moments"):
        g.write_pixels(7, mom)
    g.gbuffer(); g.history_capture()
    return hist


def _start(motion, W=48, H=36, **opts):
    d = common.mixed_material_scene()
    omap, nobj = _spheres(d)
    g = _ctx(d, common.scene_params(d, W, H), W * H, motion_history=motion, **opts)
    g.objects_define(d.tris, omap, nobj)
    g.objects_pose(np.arange(6), POSE_A)
    return g, d, omap, nobj


def test_boundary_what_keeps_and_what_drops_the_history():
    W, H = 48, 36
    on, d, omap, nobj = _start(1)
    off = _start(0)[0]
    # the option off: a pose drops the history, exactly as before
    _history(off, d, W, H)
    off.objects_pose(np.arange(6), POSE_B); off.gbuffer(); off.mk_reset()
    with pytest.raises(RuntimeError, match="no captured history"):
        off.reproject()
    # on: the pose keeps it; the current slot alone is gone
    hist = _history(on, d, W, H)
    on.objects_pose(np.arange(6), POSE_B)
    with pytest.raises(RuntimeError, match="no G-buffer has been traced for the current camera"):
        on.reproject()
    assert _same_u32(on.read_pixels(0), hist)
    on.gbuffer(); on.mk_reset(); on.reproject(); on.finish()
    got = on.read_pixels(0)
    assert (got[:, 3] > 0).any() and not _same_u32(got, hist)
    # per-triangle updates drop it with the option on: nobody knows where those triangles were
    tris = d.tris.copy()
    for call in (lambda: on.update_triangles(tris), lambda: on.update_triangles_subset(tris[:4], np.arange(4, dtype=np.uint32))):
        on.objects_pose(np.arange(6), POSE_A)
        _history(on, d, W, H)
        call()
        on.gbuffer(); on.mk_reset()
        with pytest.raises(RuntimeError, match="no captured history"):
            on.reproject()
    # a pose with nothing captured, then upload and a new definition
    on.objects_pose(np.arange(6), POSE_A)
    _history(on, d, W, H)
    on.objects_define(d.tris, omap, nobj); on.gbuffer()
    with pytest.raises(RuntimeError, match="no captured history"):
        on.reproject()
    on.objects_pose(np.arange(6), POSE_A)
    _history(on, d, W, H)
    on.upload_scene(d); on.gbuffer()
    with pytest.raises(RuntimeError, match="no captured history"):
        on.reproject()
    # the option switched off between the pose and the reprojection: refused, never a reprojection that ignores the move
    on.objects_define(d.tris, omap, nobj); on.objects_pose(np.arange(6), POSE_A)
    _history(on, d, W, H)
    on.objects_pose(np.arange(6), POSE_B)
    on.set_option("motion_history", 0); on.gbuffer()
    with pytest.raises(RuntimeError, match="objects were posed since the capture"):
        on.reproject()
    on.close(); off.close()


def test_refused_pose_leaves_history_and_poses_and_nothing_moved_equals_the_option_off():
    """the option on with every object posed by the bytes it already has, and a refused pose in between: flx_reproject is k_reproject's call,
    the framebuffer and the moments byte-equal to a context with the option off"""
    W, H = 48, 36
    on, d, _, _ = _start(1, moments=1)
    off = _start(0, moments=1)[0]
    pb = common.scene_params(d, W, H)
    wire.look_at(pb, (0.12, 1.65, 3.15), (0.03, 0.5, 0.0))
    for g in (on, off):
        _history(g, d, W, H)
    bad = POSE_B.copy(); bad[2, 1, 1] = np.nan
    with pytest.raises(RuntimeError, match="NaN or infinite"):
        on.objects_pose(np.arange(6), bad)
    with pytest.raises(RuntimeError, match="not strictly ascending"):
        on.objects_pose([1, 0], POSE_B[:2])
    on.objects_pose(np.arange(6), POSE_A)                    # the same bytes: nothing moved
    _history(on, d, W, H)                                    # (the pose re-traced nothing: capture again on both)
    _history(off, d, W, H)
    for g in (on, off):
        g.set_params(pb); g.gbuffer(); g.mk_reset(); g.reproject(); g.finish()
    assert _same_u32(on.read_pixels(0), off.read_pixels(0)) and _same_u32(on.read_pixels(7), off.read_pixels(7))
    assert (on.read_pixels(0)[:, 3] > 0).mean() > 0.5
    # the refused poses above left X_now alone: after a capture, a refusal, and a camera move the call is still k_reproject's
    _history(on, d, W, H); _history(off, d, W, H)
    with pytest.raises(RuntimeError, match="NaN or infinite"):
        on.objects_pose(np.arange(6), bad)
    for g in (on, off):
        g.set_params(common.scene_params(d, W, H)); g.gbuffer(); g.mk_reset(); g.reproject(); g.finish()
    assert _same_u32(on.read_pixels(0), off.read_pixels(0))
    on.close(); off.close()


# ---------------------------------------------------------------------------------------------------------------------------------
def test_quality_end_to_end_exact_spp():
    """mixed_material_scene 80 x 60, microkernel integrator through the C ABI, useRoulette 0: 32 spp under pose A, then gbuffer, capture, pose B
    (the diffuse sphere, object 0, slides 0.15 = about 3 pixels), gbuffer, reset, reproject + 1 spp (T) against reset + 1 spp (R); truth 512 spp
    under pose B.  On the moved object's surface pixels that received history RMSE(T) / RMSE(R) < 0.5 (DESIGN.md 4.3.3's bar); the pixels without
    history equal R bit for bit.  Measured on an MI355X: ratio 0.227 on 135 pixels, 95.7 % of the object's 141 surface pixels with history
    (printed below)."""
    W, H = 80, 60
    d = common.mixed_material_scene()
    omap, nobj = _spheres(d)
    p = common.scene_params(d, W, H, maxBounces=4, useAreaLight=1, useRoulette=0)
    A = np.stack([pc.IDENTITY] * 6)
    A[0, 2, 3] = 1.2                                         # at rest the diffuse sphere stands behind the glossy one: pose A puts it in front of the row
    B = A.copy(); B[0, 0, 3] = 0.15

    def ctx(**o):
        g = _ctx(d, p, W * H, **o)
        g.objects_define(d.tris, omap, nobj)
        return g

    truth = ctx(denoiser=1)
    truth.objects_pose(np.arange(6), B)
    driver.render_single(truth, p, 512)
    hi, hialb = truth.read_pixels(0), truth.read_pixels(4)
    surf = hialb[:, 3] == hi[:, 3]
    ref = hi[:, :3] / hi[:, 3:4]

    t = ctx(motion_history=1)
    t.objects_pose(np.arange(6), A)
    driver.render_single(t, p, 32)
    t.gbuffer(); t.history_capture()
    t.objects_pose([0], B[:1])
    t.gbuffer(); t.mk_reset(); t.reproject(); t.finish()
    n1 = t.read_pixels(0)[:, 3].copy()
    obj = t.gbuffer_objects_read(0) == 0
    driver.render_single_pass(t, p["maxBounces"]); t.finish()
    T = t.read_pixels(0)

    r = ctx()
    r.objects_pose(np.arange(6), B)
    r.mk_reset(); driver.render_single_pass(r, p["maxBounces"]); r.finish()
    Rr = r.read_pixels(0)

    got = n1 > 0
    assert R.same(T[~got], Rr[~got]), "pixels without history differ from the plain restart"
    assert np.allclose(T[got, 3], n1[got] + 1.0)
    sel = got & surf & obj
    share = float(sel.sum() / max(1, (surf & obj).sum()))
    eT = np.sqrt((((T[sel, :3] / T[sel, 3:4]) - ref[sel]) ** 2).mean())
    eR = np.sqrt((((Rr[sel, :3] / Rr[sel, 3:4]) - ref[sel]) ** 2).mean())
    print(f"motion reprojection quality: RMSE(T) {eT:.4f} / RMSE(R) {eR:.4f} = {eT / eR:.3f} on {int(sel.sum())} pixels of the moved object; "
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


def _whole_scene(t):
    """one object of every triangle: each surface pixel is the object's"""
    return np.zeros(t.triangles().size, np.uint32), 1


SHIFT_A, SHIFT_B = [pc.affine(None, (0.0, 0.0, 0.0))], [pc.affine(None, (0.03, 0.0, 0.0))]


def test_tracer_pose_keeps_the_history_and_the_filter_schedule():
    W, H = 64, 48
    on, off = _tracer(W, H), _tracer(W, H)
    for t in (on, off):
        t.set_temporal_reprojection(True)
        t.set_denoiser(True); t.set_denoiser_mode("variance"); t.set_denoiser_strength(1.0)
    on.set_motion_reprojection(True)
    assert on.motion_reprojection and not off.motion_reprojection
    for t in (on, off):
        t.define_objects(*_whole_scene(t))
        t.pose_objects([0], SHIFT_A)
        for _ in range(10):
            t.update()
        t.pose_objects([0], SHIFT_B)
        t.update()
    pon, poff = on.read_pixels(0), off.read_pixels(0)
    more = pon[:, 3] > poff[:, 3] + 1.0
    print(f"tracer: {100 * more.mean():.1f} % of the pixels kept history across the pose; median count {np.median(pon[:, 3]):.1f} against {np.median(poff[:, 3]):.1f}")
    assert more.mean() > 0.5 and (pon[:, 3] > 1.0).mean() > 0.5
    out = on.read_pixels(6)                                  # frame 10 since the last discarded history: the filter ran
    assert np.isfinite(out).all() and out[:, :3].any()
    with pytest.raises(RuntimeError, match="which = 6"):
        off.read_pixels(6)                                   # without motion reprojection the pose restarted the schedule
    # updateGeometry restarts with the switch on: the frame is the other Tracer's
    for t in (on, off):
        for _ in range(3):
            t.update()
        t.update_geometry(t.triangles())
        t.update()
    pon, poff = on.read_pixels(0), off.read_pixels(0)
    assert np.array_equal(pon[:, 3], poff[:, 3]) and common.fb_close(pon, poff)
    # a camera change pending in the same frame shares the one capture (updateGeometry made the object's pose unknown: pose it, render, then move)
    on.pose_objects([0], SHIFT_B)
    for _ in range(10):
        on.update()
    on.pose_objects([0], SHIFT_A)
    p = on.params.copy(); p["camera"]["pos"]["x"] += 0.02; on.params = p
    on.update()
    assert (on.read_pixels(0)[:, 3] > poff[:, 3] + 1.0).mean() > 0.5
    on.close(); off.close()


def test_tracer_switch_throws_without_temporal_reprojection_and_on_several_ranks():
    t = _tracer(32, 24)
    with pytest.raises(RuntimeError, match="setTemporalReprojection"):
        t.set_motion_reprojection(True)
    t.set_temporal_reprojection(True); t.set_motion_reprojection(True)
    t.set_temporal_reprojection(False)
    assert not t.motion_reprojection
    t.close()
    m = _tracer(32, 24, [0, 0])
    with pytest.raises(RuntimeError, match="single-GPU"):
        m.set_motion_reprojection(True)
    m.set_motion_reprojection(False)
    m.close()
