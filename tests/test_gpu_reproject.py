"""flx_gbuffer / flx_history_capture / flx_reproject on the device: the G-buffer against the extension kernel and the float64
brute force, the calls' isolation from a running wavefront chain, flx_reproject bit for bit against tests/reproject_cpu.cpp, the error paths,
the end-to-end quality with exact sample counts, and the Tracer switch.

Measured on an MI355X (quality test, mixed_material_scene 80 x 60, 32 spp history, 1 new sample, 512 spp truth): see the test's docstring."""
import numpy as np
import pytest
import common
import traversal_cases as tc
import reproject_reference as R
from common import COL
from fluctus_amd import host, driver, wire

pytestmark = pytest.mark.gpu
SCENES = dict(tc.scene_cases())


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return R.build_cpu(tmp_path_factory.mktemp("reproject_gpu"))


def _ctx(d, p, n, **opts):
    from fluctus_amd.device import HipContext
    g = HipContext(n)
    for k, v in opts.items():
        g.set_option(k, v)
    g.upload_scene(d)
    g.set_params(p)
    return g


def _scene_and_params(name, W, H):
    if name == "mixed_material":
        d = common.mixed_material_scene()
        return d, common.scene_params(d, W, H)
    d = tc.make_scene(SCENES[name])
    host.build_bvh(d, "sbvh")
    P = tc.tri_points(d)
    lo, hi = P.min((0, 1)), P.max((0, 1))
    c, ext = 0.5 * (lo + hi), float((hi - lo).max())
    p = tc.params(d, False)
    p["width"], p["height"] = W, H
    wire.look_at(p, c + np.array([0.3, 0.4, 1.2]) * ext, c)
    return d, p


@pytest.mark.parametrize("name", list(SCENES) + ["mixed_material"])
def test_gbuffer_equals_the_extension_kernel(exe, name):
    """the centre rays of the CPU counterpart through flx_wf_extend under extend_tree 2: hit index and t equal flx_gbuffer's bit for bit; the
    default tree differs at most on exact ties (budget 1e-5 of the rays); hit / miss and t agree with the float64 brute force where it decides"""
    W, H = 40, 28
    n = W * H
    d, p = _scene_and_params(name, W, H)
    g = _ctx(d, p, n, extend_tree=2)
    g.gbuffer(); g.finish()
    gb, cam = g.gbuffer_read(0)
    assert cam.tobytes() == np.asarray(p["camera"]).tobytes()
    dirs = R.centre_rays(exe, W, H, p["camera"])
    orig = np.repeat(np.array([[p["camera"]["pos"][k] for k in "xyz"]], np.float32), n, 0)
    tc.load_rays(g, orig, dirs, np.full(n, 3.0e38, np.float32))
    g.wf_extend(); g.finish()
    st = g.state_export()
    hi_, ht = st.view(np.int32)[COL.HIT_I][:n], st[COL.HIT_T][:n]
    gi, gt = gb[:, 3].copy().view(np.int32), gb[:, 7]
    assert np.array_equal(gi, hi_), int((gi != hi_).sum())
    hit = gi >= 0
    assert np.array_equal(gt[hit].view(np.uint32), ht[hit].view(np.uint32))
    assert (gt[~hit] == -1).all() and not gb[~hit][:, [0, 1, 2, 4, 5, 6]].any()
    assert np.array_equal(gb[hit, :3].view(np.uint32), np.ascontiguousarray(st[COL.P:COL.P + 3, :n].T[hit]).view(np.uint32))
    nn = np.linalg.norm(gb[hit, 4:7].astype(np.float64), axis=1)
    assert np.allclose(nn, 1.0, atol=1e-5) and ((gb[hit, 4:7] * dirs[hit]).sum(1) <= 1e-6).all()      # unit, facing the ray origin
    # the default tree
    g4 = _ctx(d, p, n)
    g4.gbuffer(); g4.finish()
    gb4, _ = g4.gbuffer_read(0)
    flip = gb4[:, 3].copy().view(np.int32) != gi
    assert flip.sum() <= int(1e-5 * n), f"{int(flip.sum())} of {n} hit indices differ between the trees"
    assert np.array_equal(gb4[~flip, 7].view(np.uint32), gt[~flip].view(np.uint32))
    # the brute force (geometry only: the mixed scene's implicit light quad is not its business)
    if name != "mixed_material":
        bf = tc.BruteForce(tc.tri_points(d), orig, dirs, np.full(n, 3.0e38, np.float32))
        v = bf.verdict(d)
        dec = v["ext_decided"]
        assert not (dec & (gi != v["closest"])).any()
        dh = dec & hit
        assert np.allclose(gt[dh], bf.t_closest[dh], rtol=1e-4)


def test_gbuffer_strides_when_the_image_exceeds_the_path_count():
    W, H = 64, 48
    d = common.mixed_material_scene()
    p = common.scene_params(d, W, H)
    a, b = _ctx(d, p, W * H, extend_tree=2), _ctx(d, p, 320, extend_tree=2)
    for g in (a, b):
        g.gbuffer(); g.finish()
    assert R.same(a.gbuffer_read(0)[0], b.gbuffer_read(0)[0])


def test_gbuffer_leaves_the_run_alone():
    """two contexts run the same wavefront chain, one with flx_gbuffer at every position of an iteration: the counters and the full exported
    state are identical bit for bit.  The framebuffer is a sum of float atomics whose order the device does not define (the probing context
    also runs the separate kernels where the other fuses): its sample counts are identical and its sums equal up to the order of addition,
    common.fb_close's bound of (N - 1) 2^-24 relative, the project's comparison for every framebuffer"""
    W, H = 64, 48
    d = common.mixed_material_scene()
    p = common.scene_params(d, W, H, maxBounces=4, wfSeparateQueues=1)
    a, b = _ctx(d, p, W * H, extend_tree=2), _ctx(d, p, W * H, extend_tree=2)
    for g in (a, b):
        driver.reset_renderer(g)
    for it in range(6):
        cnts = []
        for g, probe in ((a, False), (b, True)):
            steps = [lambda: g.wf_logic(False), g.wf_raygen, g.wf_materials, g.wf_extend, g.wf_shadow, g.clear_queues]
            cnt = None
            for k, s in enumerate(steps):
                if probe:
                    g.gbuffer()
                s()
                if k == 2:
                    cnt = g.get_counters()
            if probe:
                g.gbuffer()
            g.finish()
            cnt = np.array(cnt, copy=True)
            g.pixel_index_update(W * H, int(cnt[0]))
            cnts.append(cnt)
        assert np.array_equal(cnts[0], cnts[1]), (it, cnts)
    assert not common.state_diff(a.state_export(), b.state_export(), 0.0, 0.0)
    pa, pb = a.read_pixels(0), b.read_pixels(0)
    assert np.array_equal(pa[:, 3], pb[:, 3]) and common.fb_close(pa, pb)


def _adversarial(W, H, seed, moments):
    ca, cb = R.camera((0.0, 0.0, 4.0), (0.0, 0.0, 0.0)), R.camera((0.45, 0.1, 3.8), (0.1, 0.0, 0.0), 55.0)
    wall = R.quad((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 3.0, 50.0)          # narrow: misses left and right of it
    quad = R.quad((0.3, 0.1, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 0.5, 0.4)
    prev, cur = R.synth_gbuffer(ca, W, H, [wall, quad]), R.synth_gbuffer(cb, W, H, [wall, quad])
    hist, mom = R.random_history(W * H, seed, True)
    rng = np.random.default_rng(seed + 1)
    N, k = W * H, max(1, W * H // 40)
    hist[rng.choice(N, k), 0] = np.nan; hist[rng.choice(N, k), 1] = np.inf; hist[rng.choice(N, k), 2] = -np.inf
    hist[rng.choice(N, k), 3] = 0.0; hist[rng.choice(N, k), 3] = np.inf
    mom[rng.choice(N, k), 3] = 0.0; mom[rng.choice(N, k), 1] = np.inf; mom[rng.choice(N, k), 0] = np.nan
    prev[rng.choice(N, k), 4:7] = (0.6, 0.0, 0.8)                                          # a turned normal at the same position
    cur[rng.choice(N, k), 0] = np.nan                                                      # a non-finite current position
    return ca, cb, prev, cur, hist, (mom if moments else None)


@pytest.mark.parametrize("moments", [1, 0])
@pytest.mark.parametrize("W,H", [(1, 1), (7, 5), (33, 17), (200, 120), (1920, 1080)])
def test_reproject_bit_identical_to_cpu(exe, W, H, moments):
    d = common.simple_scene()
    p = common.scene_params(d, W, H)
    g = _ctx(d, p, 4096, moments=moments)
    ca, cb, prev, cur, hist, mom = _adversarial(W, H, W + H, moments)
    g.write_pixels(0, hist)
    if moments:
        g.write_pixels(7, mom)
    g.gbuffer_write(0, prev, ca)
    g.history_capture()
    g.gbuffer_write(0, cur, cb)
    assert R.same(g.gbuffer_read(1)[0], prev) and g.gbuffer_read(1)[1].tobytes() == ca.tobytes()
    g.mk_reset()
    for kw in ({}, dict(max_history=5.0, plane_tolerance_px=0.5, normal_cos=0.5, min_weight=0.3)):
        g.reproject(**kw); g.finish()
        cpx, cmom, _, _ = R.run_cpu(exe, W, H, cur, prev, ca, float(cb["fov"]), hist, mom, **kw)
        px = g.read_pixels(0)
        assert R.same(px, cpx), int((px.view(np.uint32) != cpx.view(np.uint32)).any(1).sum())
        if moments:
            assert R.same(g.read_pixels(7), cmom)
        assert (px[:, 3] > 0).any() and (px[:, 3] == 0).any() or W * H == 1


def test_order_and_error_paths():
    W, H = 32, 16
    d = common.simple_scene()
    p = common.scene_params(d, W, H)
    g = _ctx(d, p, W * H, moments=1)
    px = R.random_history(W * H, 1)[0]
    g.write_pixels(0, px)

    def fails(fn, match, *a, **kw):
        with pytest.raises(RuntimeError, match=match):
            fn(*a, **kw)
        assert R.same(g.read_pixels(0), px), "a failed call changed the accumulation"

    fails(g.reproject, "no captured history")
    fails(g.history_capture, "no G-buffer")
    g.gbuffer()
    fails(g.reproject, "no captured history")
    g.history_capture()
    fails(g.reproject, "no G-buffer has been traced for the current camera")
    fails(g.history_capture, "no G-buffer")                      # the current slot was handed over
    g.gbuffer()
    for bad in (dict(max_history=0.5), dict(max_history=np.inf), dict(plane_tolerance_px=0.0), dict(plane_tolerance_px=np.nan), dict(normal_cos=1.5),
                dict(normal_cos=np.nan), dict(min_weight=0.0), dict(min_weight=1.5)):
        fails(g.reproject, "parameters must be", **bad)
    with pytest.raises(TypeError):
        g.reproject(sigma=1.0)
    g.reproject(); g.finish()                                      # and the valid sequence works
    assert not R.same(g.read_pixels(0), px)
    # a change of shape at the same pixel count between capture and reproject: the framebuffers, the slots and the history stay, the sizes differ
    g.write_pixels(0, px); g.gbuffer(); g.history_capture()
    g.set_params(common.scene_params(d, H, W))
    assert R.same(g.read_pixels(0), px)
    g.gbuffer()
    fails(g.reproject, "image size changed")
    g.set_params(p)                                                # the current slot still has the other shape
    fails(g.history_capture, "image size differs")
    fails(g.reproject, "image size changed")
    g.gbuffer(); g.reproject(); g.finish()
    assert not R.same(g.read_pixels(0), px)
    # a change of the pixel count: the slots and the history go with the framebuffers
    g.write_pixels(0, px); g.gbuffer(); g.history_capture()
    g.set_params(common.scene_params(d, W + 8, H))
    g.gbuffer()
    with pytest.raises(RuntimeError, match="no captured history"):
        g.reproject()
    # a partitioned context
    g.set_params(p)
    g.set_partition(0, 2)
    for fn in (g.gbuffer, g.history_capture, g.reproject):
        with pytest.raises(RuntimeError, match="partitioned"):
            fn()
    g.set_partition(0, 1)
    g.gbuffer(); g.history_capture(); g.gbuffer(); g.reproject(); g.finish()


def test_quality_end_to_end_exact_spp():
    """mixed_material_scene 80 x 60, microkernel integrator through the C ABI, useRoulette 0: 32 spp under camera A reprojected into camera B
    (a small translation + rotation) + 1 spp (T) against reset + 1 spp (R), truth 512 spp under B.  On the surface pixels that received
    history RMSE(T) / RMSE(R) <= 0.5 (ideal for view-independent radiance 1 / sqrt(33) = 0.17); the pixels without history equal R bit for
    bit; >= 80 % of the surface pixels receive history.  Measured on an MI355X: ratio 0.228, 99.8 % of the 2 218 surface pixels with history (printed below)."""
    W, H = 80, 60
    d = common.mixed_material_scene()
    kw = dict(maxBounces=4, useAreaLight=1, useRoulette=0)
    pa = common.scene_params(d, W, H, **kw)
    pb = common.scene_params(d, W, H, **kw)
    wire.look_at(pb, (0.12, 1.65, 3.15), (0.03, 0.5, 0.0))
    truth = _ctx(d, pb, W * H, denoiser=1)
    driver.render_single(truth, pb, 512)
    hi, hialb = truth.read_pixels(0), truth.read_pixels(4)
    surf = hialb[:, 3] == hi[:, 3]
    ref = hi[:, :3] / hi[:, 3:4]

    t = _ctx(d, pa, W * H)
    driver.render_single(t, pa, 32)
    t.gbuffer(); t.history_capture()
    t.set_params(pb); t.gbuffer(); t.mk_reset(); t.reproject(); t.finish()
    n1 = t.read_pixels(0)[:, 3].copy()
    driver.render_single_pass(t, pb["maxBounces"]); t.finish()
    T = t.read_pixels(0)

    r = _ctx(d, pb, W * H)
    r.mk_reset(); driver.render_single_pass(r, pb["maxBounces"]); r.finish()
    Rr = r.read_pixels(0)

    got = n1 > 0
    assert R.same(T[~got], Rr[~got]), "pixels without history differ from the plain restart"
    assert np.allclose(T[got, 3], n1[got] + 1.0)
    share = float((got & surf).sum() / surf.sum())
    sel = got & surf
    eT = np.sqrt((((T[sel, :3] / T[sel, 3:4]) - ref[sel]) ** 2).mean())
    eR = np.sqrt((((Rr[sel, :3] / Rr[sel, 3:4]) - ref[sel]) ** 2).mean())
    print(f"reprojection quality: RMSE(T) {eT:.4f} / RMSE(R) {eR:.4f} = {eT / eR:.3f} on {int(sel.sum())} pixels; "
          f"{100 * share:.1f} % of the {int(surf.sum())} surface pixels received history; mean n' {n1[got].mean():.1f}")
    assert share >= 0.8, share
    assert eT / eR <= 0.5, eT / eR


def _move(t, dx):
    p = t.params.copy()
    p["camera"]["pos"]["x"] += dx
    t.params = p


def _tracer(W, H, devices=0):
    from fluctus_amd.tracer import Tracer
    t = Tracer(W, H, devices, W * H)
    t.init(W, H, "proc:kitchen:3000:7")
    return t


def test_tracer_off_is_unchanged_and_on_keeps_the_history():
    W, H = 64, 48
    a, b, c = _tracer(W, H), _tracer(W, H), _tracer(W, H)
    b.set_temporal_reprojection(True); b.set_temporal_reprojection(False)
    c.set_temporal_reprojection(True); c.set_max_history(16)
    assert c.temporal_reprojection and not b.temporal_reprojection and not a.temporal_reprojection
    for t in (a, b, c):
        for _ in range(6):
            t.update()
    # nothing changes before a move (two Tracers agree up to the order of their float atomics: common.fb_close)
    assert common.fb_close(a.read_pixels(0), b.read_pixels(0)) and common.fb_close(a.read_pixels(0), c.read_pixels(0))
    for t in (a, b, c):
        _move(t, 0.03)
        t.update()
    pa, pb, pc = a.read_pixels(0), b.read_pixels(0), c.read_pixels(0)
    assert common.fb_close(pa, pb)
    more = pc[:, 3] > pa[:, 3] + 1.0
    print(f"tracer: {100 * more.mean():.1f} % of the pixels kept history; median count {np.median(pc[:, 3]):.1f} against {np.median(pa[:, 3]):.1f}")
    assert more.mean() > 0.8 and pc[:, 3].max() <= 16.0 + pa[:, 3].max() + 1e-3
    with pytest.raises(RuntimeError, match="setMaxHistory"):
        c.set_max_history(0.5)


def _detour(t):
    """frames on the wavefront integrator, a camera move consumed on the microkernel integrator, frames on the wavefront integrator again,
    one more move -> the accumulation of the frame after that move"""
    for _ in range(4):
        t.update()
    t.toggle_renderer()
    _move(t, 0.2)
    t.update()
    t.toggle_renderer()
    for _ in range(3):
        t.update()
    _move(t, 0.03)
    t.update()
    return t.read_pixels(0)


def test_tracer_drops_the_history_of_another_camera():
    """a move consumed by the microkernel branch traces no G-buffer: the G-buffer the wavefront branch left belongs to another camera, and the
    next move on the wavefront branch must not reproject through it -- the frame equals what a Tracer without reprojection renders.  Without the
    detour the same last move does keep its history"""
    W, H = 64, 48
    on, off, straight = _tracer(W, H), _tracer(W, H), _tracer(W, H)
    on.set_temporal_reprojection(True); straight.set_temporal_reprojection(True)
    pon, poff = _detour(on), _detour(off)
    assert np.array_equal(pon[:, 3], poff[:, 3]) and common.fb_close(pon, poff), float(np.abs(pon[:, 3] - poff[:, 3]).max())
    for _ in range(4):
        straight.update()
    _move(straight, 0.03)
    straight.update()
    assert (straight.read_pixels(0)[:, 3] > poff[:, 3]).mean() > 0.5       # the control: most pixels carry more than the restart's samples


def test_tracer_drops_the_history_when_more_than_the_camera_changed():
    """a re-coloured area light is a parameter update too: the radiance kept under the old light would be stale, so the history is discarded and
    the frame is the default path's; the camera move after it keeps the (new) history again"""
    W, H = 64, 48
    on, off = _tracer(W, H), _tracer(W, H)
    on.set_temporal_reprojection(True)
    for t in (on, off):
        for _ in range(4):
            t.update()
        p = t.params.copy()
        p["areaLight"]["E"]["x"] *= 0.25
        t.params = p
        t.update()
    pon, poff = on.read_pixels(0), off.read_pixels(0)
    assert np.array_equal(pon[:, 3], poff[:, 3]) and common.fb_close(pon, poff)
    for t in (on, off):
        for _ in range(4):
            t.update()
        _move(t, 0.03)
        t.update()
    assert (on.read_pixels(0)[:, 3] > off.read_pixels(0)[:, 3]).mean() > 0.5   # most pixels carry more than the restart's samples


def test_tracer_filter_runs_on_the_frame_after_a_move():
    W, H = 64, 48
    on, off = _tracer(W, H), _tracer(W, H)
    on.set_temporal_reprojection(True)
    for t in (on, off):
        t.set_denoiser(True); t.set_denoiser_mode("variance"); t.set_denoiser_strength(1.0)
        for _ in range(10):
            t.update()
        with pytest.raises(RuntimeError, match="which = 6"):
            t.read_pixels(6)                                      # frames 0..9: the filter has not run yet
        _move(t, 0.03)
        t.update()
    out = on.read_pixels(6)                                       # frame 10 since the last discarded history: it ran
    assert np.isfinite(out).all() and out[:, :3].any()
    assert (on.read_pixels(7)[:, 3] > 2.0).mean() > 0.5           # ... with reprojected moments under it
    with pytest.raises(RuntimeError, match="which = 6"):
        off.read_pixels(6)                                        # without reprojection the move restarted the schedule


def test_tracer_multi_rank_throws():
    t = _tracer(32, 24, [0, 0])
    with pytest.raises(RuntimeError, match="single-GPU"):
        t.set_temporal_reprojection(True)
    t.set_temporal_reprojection(False)
