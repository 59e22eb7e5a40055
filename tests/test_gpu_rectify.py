"""flx_history_mark / flx_history_rectify on the device: bit identity with tests/rectify_cpu.cpp, the order and error paths, the
calls' isolation from a running wavefront chain, flx_reproject unchanged by a mark behind it, and the end-to-end quality with exact sample
counts.  (Which call drops the mark: tests/test_gpu_feature_state_rectify.py, the table of tests/feature_state_rectify_cases.py.)

Measured on an MI355X: see the docstrings of test_quality_end_to_end_exact_spp and of the Tracer tests."""
import numpy as np
import pytest
import common
import pose_cases as pc
import rectify_cases as K
import rectify_reference as RC
from fluctus_amd import driver

pytestmark = pytest.mark.gpu
NO = 0xFFFFFFFF
NONDEFAULT = dict(radius=2, gamma=1.5, sensitivity=0.7, lum_floor=0.2, min_pixels=3, plane_tolerance_px=0.5, normal_cos=0.5)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return RC.build_cpu(tmp_path_factory.mktemp("rectify_gpu"))


def _ctx(d, p, n, **opts):
    from fluctus_amd.device import HipContext
    g = HipContext(n)
    for k, v in opts.items():
        g.set_option(k, v)
    g.upload_scene(d)
    g.set_params(p)
    return g


def _load(g, s, moments):
    """the adversarial state as a render would have left it: the history, the G-buffer, the mark, then the accumulation with the new samples"""
    g.write_pixels(0, s["S"])
    if moments:
        g.write_pixels(7, s["SM"])
    g.gbuffer_write(0, s["cur"], K.CAM)
    g.history_mark()
    g.write_pixels(0, s["A"])
    if moments:
        g.write_pixels(7, s["M"])


@pytest.mark.parametrize("moments", [1, 0])
@pytest.mark.parametrize("W,H", [(1, 1), (7, 5), (33, 17), (49, 35)])
def test_rectify_bit_identical_to_cpu(exe, W, H, moments):
    """the lambda plane, which = 0, which = 7 and the mark read back, against the counterpart: defaults, non-default parameters, and r = 4
    (at 49 x 35 the halo of the middle tile reaches across three tiles in x and in y)"""
    d = common.simple_scene()
    g = _ctx(d, common.scene_params(d, W, H), 4096, moments=moments)
    s = K.scene(W, H, W + H, moments=bool(moments))
    some = 0
    for kw in ({}, NONDEFAULT, dict(radius=4, min_pixels=20), dict(radius=1, min_pixels=1, sensitivity=0.4)):
        _load(g, s, moments)
        mark, mmom, lam = g.history_mark_read(moments=bool(moments))
        assert RC.same(mark, s["S"]) and not lam.any() and (not moments or RC.same(mmom, s["SM"]))
        g.history_rectify(**kw); g.finish()
        cpu = RC.run_cpu(exe, W, H, s["cur"], s["A"], s["S"], K.FOV, s["M"], s["SM"], **kw)
        mark, mmom, lam = g.history_mark_read(moments=bool(moments))
        assert RC.same(lam, cpu["lam"]), int((lam.view(np.uint32) != cpu["lam"].view(np.uint32)).sum())
        assert RC.same(g.read_pixels(0), cpu["A"]) and RC.same(mark, cpu["S"])
        if moments:
            assert RC.same(g.read_pixels(7), cpu["M"]) and RC.same(mmom, cpu["SM"])
        some += int((lam > 0).sum())
    assert some or W * H < 50
    g.close()


def test_moments_on_at_the_mark_only_and_now_only(exe):
    W, H = 33, 17
    d = common.simple_scene()
    s = K.scene(W, H, 3)
    cpu = RC.run_cpu(exe, W, H, s["cur"], s["A"], s["S"], K.FOV)
    # on at the mark, off now: which = 7 is gone, the mark's moments stay as they were
    g = _ctx(d, common.scene_params(d, W, H), 4096, moments=1)
    _load(g, s, 1)
    g.set_option("moments", 0)
    g.history_rectify(); g.finish()
    mark, mmom, lam = g.history_mark_read(moments=True)
    assert RC.same(lam, cpu["lam"]) and RC.same(g.read_pixels(0), cpu["A"]) and RC.same(mark, cpu["S"]) and RC.same(mmom, s["SM"])
    g.close()
    # off at the mark, on now: which = 7 stays as it was
    g = _ctx(d, common.scene_params(d, W, H), 4096)
    _load(g, s, 0)
    g.set_option("moments", 1)
    g.write_pixels(7, s["M"])
    g.history_rectify(); g.finish()
    assert RC.same(g.read_pixels(7), s["M"]) and RC.same(g.read_pixels(0), cpu["A"])
    with pytest.raises(RuntimeError, match="holds no moments"):
        g.history_mark_read(moments=True)
    g.close()


def test_order_and_error_paths():
    W, H = 32, 16
    d = common.simple_scene()
    p = common.scene_params(d, W, H)
    g = _ctx(d, p, W * H, moments=1)
    s = K.scene(W, H, 1)
    g.write_pixels(0, s["A"])
    state = {"mark": None}

    def fails(fn, match, *a, **kw):
        with pytest.raises(RuntimeError, match=match):
            fn(*a, **kw)
        assert RC.same(g.read_pixels(0), s["A"]), "a refused call changed the accumulation"
        if state["mark"] is not None:
            m, mm, lam = g.history_mark_read(moments=True)
            assert RC.same(m, state["mark"][0]) and RC.same(mm, state["mark"][1]) and RC.same(lam, state["mark"][2]), "a refused call changed the mark"

    fails(g.history_rectify, "no mark")
    fails(g.history_mark, "no G-buffer")
    fails(g.history_mark_read, "no mark")
    g.gbuffer()
    fails(g.history_rectify, "no mark")
    g.write_pixels(0, s["S"]); g.write_pixels(7, s["SM"])
    g.history_mark()
    g.write_pixels(0, s["A"]); g.write_pixels(7, s["M"])
    state["mark"] = g.history_mark_read(moments=True)
    assert RC.same(state["mark"][0], s["S"])
    for bad in (dict(radius=0), dict(radius=5), dict(gamma=-1.0), dict(gamma=np.inf), dict(gamma=np.nan), dict(sensitivity=0.0), dict(sensitivity=np.inf),
                dict(sensitivity=np.nan), dict(lum_floor=-0.1), dict(lum_floor=np.inf), dict(min_pixels=0), dict(min_pixels=50), dict(radius=1, min_pixels=10),
                dict(plane_tolerance_px=0.0), dict(plane_tolerance_px=np.nan), dict(normal_cos=1.5), dict(normal_cos=-1.5), dict(normal_cos=np.nan)):
        fails(g.history_rectify, "parameters must be", **bad)
    with pytest.raises(TypeError):
        g.history_rectify(sigma=1.0)
    g.history_rectify(radius=4, min_pixels=81, gamma=0.0, lum_floor=0.0, normal_cos=-1.0); g.finish()      # the corners of what is allowed
    # the calls that drop the mark: each followed by the refusal (the whole table: tests/test_gpu_feature_state_rectify.py)
    state["mark"] = None

    def again():
        g.set_partition(0, 1); g.set_params(p); g.write_pixels(0, s["A"]); g.gbuffer(); g.history_mark()

    for drop in (g.mk_reset, g.wf_reset, lambda: g.set_params(common.scene_params(d, H, W)), lambda: g.set_params(common.scene_params(d, W + 8, H)),
                 lambda: g.set_partition(0, 1), g.history_capture, lambda: g.update_triangles(d.tris),
                 lambda: g.update_triangles_subset(d.tris[:2], np.arange(2, dtype=np.uint32)), lambda: g.upload_scene(d)):
        again()
        g.history_rectify()
        drop()
        with pytest.raises(RuntimeError, match="no mark"):
            g.history_rectify()
        with pytest.raises(RuntimeError, match="no mark"):
            g.history_mark_read()
    # flx_write_pixels keeps it, and so does tracing the G-buffer again
    again()
    g.write_pixels(0, s["S"]); g.gbuffer(); g.history_rectify(); g.finish()
    # a partitioned context
    g.set_partition(0, 2)
    for fn in (g.history_mark, g.history_rectify, g.history_mark_read):
        with pytest.raises(RuntimeError, match="partitioned"):
            fn()
    g.set_partition(0, 1)
    g.gbuffer(); g.history_mark(); g.history_rectify(); g.finish()
    g.close()


def test_mark_and_rectify_leave_the_run_alone():
    """test_gbuffer_leaves_the_run_alone's pattern: two contexts run the same wavefront chain, one with flx_history_mark / flx_history_rectify at
    every position of an iteration: the counters and the full exported state are identical bit for bit.  The framebuffer is theirs to change, and
    only as they say: a mark leaves which = 0 / 7 bit for bit, a rectify changes only the pixels whose lambda is > 0."""
    W, H = 64, 48
    d = common.mixed_material_scene()
    p = common.scene_params(d, W, H, maxBounces=4, wfSeparateQueues=1)
    a, b = _ctx(d, p, W * H, extend_tree=2, moments=1), _ctx(d, p, W * H, extend_tree=2, moments=1)
    for g in (a, b):
        driver.reset_renderer(g)
    b.gbuffer()
    for it in range(6):
        cnts = []
        for g, probe in ((a, False), (b, True)):
            steps = [lambda: g.wf_logic(False), g.wf_raygen, g.wf_materials, g.wf_extend, g.wf_shadow, g.clear_queues]
            cnt = None
            for k, s in enumerate(steps):
                if probe:
                    (g.history_mark if (k + it) % 2 == 0 or it == 0 and k == 0 else g.history_rectify)()
                s()
                if k == 2:
                    cnt = g.get_counters()
            if probe:
                g.history_rectify(gamma=0.5)
            g.finish()
            cnt = np.array(cnt, copy=True)
            g.pixel_index_update(W * H, int(cnt[0]))
            cnts.append(cnt)
        assert np.array_equal(cnts[0], cnts[1]), (it, cnts)
    assert not common.state_diff(a.state_export(), b.state_export(), 0.0, 0.0)
    # what the two calls do to the framebuffer, on the render b has arrived at
    px, mo = b.read_pixels(0), b.read_pixels(7)
    b.history_mark(); b.finish()
    assert RC.same(b.read_pixels(0), px) and RC.same(b.read_pixels(7), mo)
    mark, mmom, lam = b.history_mark_read(moments=True)
    assert RC.same(mark, px) and RC.same(mmom, mo) and not lam.any()
    new = px.copy(); new[:, :3] *= 1.5; new[:, 3] += 4.0                # as if four samples had come in, much brighter than the history
    b.write_pixels(0, new)
    b.history_rectify(); b.finish()
    px2, mo2 = b.read_pixels(0), b.read_pixels(7)
    lam = b.history_mark_read()[2]
    w = lam > 0
    assert w.any() and not w.all()
    assert RC.same(px2[~w], new[~w]) and RC.same(mo2[~w], mo[~w])
    assert (px2[w, 3] < new[w, 3]).all() and (mo2[w, 3] < mo[w, 3]).all()
    a.close(); b.close()


def test_reproject_followed_by_a_mark_is_unchanged():
    """flx_reproject's result with and without a flx_history_mark behind it: the same bits, which = 0 and which = 7"""
    import test_gpu_reproject as tgr
    W, H = 33, 17
    d = common.simple_scene()
    ca, cb, prev, cur, hist, mom = tgr._adversarial(W, H, 9, 1)
    out = []
    for with_mark in (False, True):
        g = _ctx(d, common.scene_params(d, W, H), 4096, moments=1)
        g.write_pixels(0, hist); g.write_pixels(7, mom)
        g.gbuffer_write(0, prev, ca); g.history_capture(); g.gbuffer_write(0, cur, cb)
        g.mk_reset(); g.reproject()
        if with_mark:
            g.history_mark()
        g.finish()
        out.append((g.read_pixels(0), g.read_pixels(7)))
        if with_mark:
            mark, mmom, _ = g.history_mark_read(moments=True)
            assert RC.same(mark, out[-1][0]) and RC.same(mmom, out[-1][1])
        g.close()
    assert RC.same(out[0][0], out[1][0]) and RC.same(out[0][1], out[1][1])


def _lum(rgb):
    return rgb @ np.array([0.2126, 0.7152, 0.0722])


def test_quality_end_to_end_exact_spp():
    """mixed_material_scene 80 x 60, microkernel integrator through the C ABI, useRoulette 0, the six spheres as objects, "motion_history" on:
    32 spp under pose A; gbuffer, capture, pose B (the diffuse sphere slides 0.5), gbuffer, reset, reproject, mark; 4 passes (this is P);
    rectify with the defaults (this is T); R: reset + 4 passes; truths: 512 spp under A and under B.  The CHANGED set: ground pixels outside the
    moved object (in both poses) whose two truths differ by more than 25 % of the larger luminance -- the shadow that left and the shadow that
    arrived; at least 30 of them.  On it RMSE(T) < RMSE(P).  On the other surface pixels with history (the moved object's left out)
    RMSE(T) <= 1.1 RMSE(P) -- the bound a retained history share of 0.9 implies, 1 / sqrt(0.9) = 1.05, with margin for the set's edge -- and
    RMSE(T) < RMSE(R).  Measured on an MI355X (printed below): 443 changed pixels, RMSE(T) 0.4867 against RMSE(P) 0.5274 on them
    (mean lambda 0.29); on the 1 544 unchanged ones RMSE(T) 0.5399, RMSE(P) 0.5400, RMSE(R) 1.4595 (mean lambda 0.003); retained share
    sum S'.w / sum S.w = 0.9448.  The defaults met both bars at the first run: no sweep of gamma."""
    W, H = 80, 60
    d = common.mixed_material_scene()
    m = d.tris["matId"].astype(np.int64)
    omap = np.full(d.tris.size, NO, np.uint32); omap[m >= 3] = (m[m >= 3] - 3).astype(np.uint32)
    p = common.scene_params(d, W, H, maxBounces=4, useAreaLight=1, useRoulette=0)
    A = np.stack([pc.IDENTITY] * 6)
    A[0, 2, 3] = 1.2                                         # pose A puts the diffuse sphere in front of the row
    B = A.copy(); B[0, 0, 3] = 0.5

    def ctx(**o):
        g = _ctx(d, p, W * H, **o)
        g.objects_define(d.tris, omap, 6)
        return g

    truths = []
    for pose in (A, B):
        g = ctx(denoiser=1)
        g.objects_pose(np.arange(6), pose)
        driver.render_single(g, p, 512)
        hi, alb = g.read_pixels(0), g.read_pixels(4)
        truths.append((hi[:, :3] / hi[:, 3:4], alb[:, 3] == hi[:, 3]))
        g.close()
    (refA, _), (refB, surf) = truths

    t = ctx(motion_history=1)
    t.objects_pose(np.arange(6), A)
    driver.render_single(t, p, 32)
    t.gbuffer(); t.history_capture()
    t.objects_pose([0], B[:1])
    t.gbuffer(); t.mk_reset(); t.reproject(); t.history_mark(); t.finish()
    n1 = t.read_pixels(0)[:, 3].copy()
    gA, gB = t.gbuffer_read(1)[0], t.gbuffer_read(0)[0]
    oA, oB = t.gbuffer_objects_read(1), t.gbuffer_objects_read(0)
    for _ in range(4):
        driver.render_single_pass(t, p["maxBounces"])
    t.finish()
    P = t.read_pixels(0)
    S0 = t.history_mark_read()[0]
    t.history_rectify(); t.finish()
    T = t.read_pixels(0)
    S1, _, lam = t.history_mark_read()
    t.close()

    r = ctx()
    r.objects_pose(np.arange(6), B)
    r.mk_reset()
    for _ in range(4):
        driver.render_single_pass(r, p["maxBounces"])
    r.finish()
    Rr = r.read_pixels(0)
    r.close()

    def on_ground(gb):                                       # the ground grid carries the materials 1 and 2
        i = gb[:, 3].copy().view(np.int32)
        return (i >= 0) & np.isin(m[np.clip(i, 0, m.size - 1)], (1, 2))

    ground = on_ground(gA) & on_ground(gB) & (oA == NO) & (oB == NO)
    la, lb = _lum(refA.astype(np.float64)), _lum(refB.astype(np.float64))
    differ = np.abs(la - lb) > 0.25 * np.maximum(la, lb)
    got = n1 > 0
    changed = ground & differ & surf & got
    unchanged = surf & got & ~differ & (oA != 0) & (oB != 0)

    def rmse(px, sel):
        return float(np.sqrt((((px[sel, :3] / px[sel, 3:4]) - refB[sel]) ** 2).mean()))

    share = float(S1[:, 3].sum() / S0[:, 3].sum())
    fig = dict(changed=int(changed.sum()), unchanged=int(unchanged.sum()), T_changed=rmse(T, changed), P_changed=rmse(P, changed),
               T_unchanged=rmse(T, unchanged), P_unchanged=rmse(P, unchanged), R_unchanged=rmse(Rr, unchanged), retained=share,
               lam_changed=float(lam[changed].mean()), lam_unchanged=float(lam[unchanged].mean()))
    print("rectification quality: " + ", ".join(f"{k} {v:.4f}" if isinstance(v, float) else f"{k} {v}" for k, v in fig.items()))
    assert changed.sum() >= 30, int(changed.sum())
    assert fig["T_changed"] < fig["P_changed"], fig
    assert fig["T_unchanged"] <= 1.1 * fig["P_unchanged"], fig
    assert fig["T_unchanged"] < fig["R_unchanged"], fig


# ---------------------------------------------------------------------------------------------------------------------------------
def _tracer(W, H, devices=0):
    from fluctus_amd.tracer import Tracer
    t = Tracer(W, H, devices, W * H)
    t.init(W, H, "proc:kitchen:3000:7")
    return t


def _move(t, dx):
    p = t.params.copy()
    p["camera"]["pos"]["x"] += dx
    t.params = p


def _dim(t, k):
    p = t.params.copy()
    for c in "xyz":
        p["areaLight"]["E"][c] *= k
    t.params = p


def test_tracer_switch_off_is_unchanged():
    """a Tracer whose switch was on and is off again renders what one that never had it renders, through a camera move, the frames where a
    rectify would have fired, and a changed light (which discards again): exact sample counts, sums within common.fb_close (two Tracers
    differ in the order of their float atomics)"""
    W, H = 64, 48
    a, b = _tracer(W, H), _tracer(W, H)
    for t in (a, b):
        t.set_temporal_reprojection(True)
    b.set_history_rectification(True); b.set_rectify_delay(3); b.set_history_rectification(False)
    assert not a.history_rectification and not b.history_rectification
    for t in (a, b):
        for _ in range(5):
            t.update()
        _move(t, 0.03)
        for _ in range(5):
            t.update()
        _dim(t, 0.25)
        for _ in range(2):
            t.update()
    pa, pb = a.read_pixels(0), b.read_pixels(0)
    assert np.array_equal(pa[:, 3], pb[:, 3]) and common.fb_close(pa, pb)
    assert b.rectify_info()[1] == 0
    a.close(); b.close()


def test_tracer_dimmed_light_keeps_a_history_and_the_rectify_frame_sheds_it():
    """switch on, the area light dimmed to a quarter: the frame after the change keeps a history (mean sample count above the restart's, which a
    Tracer without the switch renders), and the frame that runs the rectify sheds it (the mean count falls below the previous frame's, although
    that frame added a sample).  The means are over ALL pixels: the Tracer shows no G-buffer to pick the surface pixels by, and a pixel that
    misses the scene carries the restart's count in both Tracers, so it dilutes the difference and never makes it.  Measured on an MI355X:
    3.86 samples per pixel against the restart's 1.01; 7.24 on the frame before the rectify, 5.83 on its frame; retained share 0.597."""
    W, H = 64, 48
    on, off = _tracer(W, H), _tracer(W, H)
    for t in (on, off):
        t.set_temporal_reprojection(True)
    on.set_history_rectification(True)
    delay = on.rectify_delay
    assert on.history_rectification and delay == 2 * int(on.params["maxBounces"]) + 2
    for t in (on, off):
        for _ in range(12):
            t.update()
        _dim(t, 0.25)
        t.update()
    pon, poff = on.read_pixels(0), off.read_pixels(0)
    surf = np.ones(W * H, bool)
    kept, restart = float(pon[surf, 3].mean()), float(poff[surf, 3].mean())
    assert kept > restart + 1.0, (kept, restart)
    means = [kept]
    for _ in range(delay - 1):
        assert on.rectify_info()[1] == 0
        on.update()
        means.append(float(on.read_pixels(0)[surf, 3].mean()))
    share, count = on.rectify_info()
    print(f"tracer, light dimmed to a quarter: mean count on {int(surf.sum())} pixels {kept:.2f} against the restart's {restart:.2f}; "
          f"per frame until the rectify {[round(v, 2) for v in means]}; retained share of the mark {share:.3f}")
    assert count == 1 and means[-1] < means[-2], means
    on.update()
    assert on.rectify_info()[1] == 1                          # once
    on.close(); off.close()


def test_tracer_camera_nudge_keeps_most_of_the_history():
    """switch on, a camera nudge only: nothing changed but the view, so the rectify at the default delay must keep the history -- the retained
    share of the mark's sample count is >= 0.8.  Measured on an MI355X (printed below): 0.9996 at the default delay of 22
    frames (maxBounces 10), so the delay was not lengthened."""
    W, H = 64, 48
    t = _tracer(W, H)
    t.set_temporal_reprojection(True); t.set_history_rectification(True)
    t.rectify_info(measure=True)
    for _ in range(12):
        t.update()
    _move(t, 0.03)
    for _ in range(t.rectify_delay):
        t.update()
    share, count = t.rectify_info()
    print(f"tracer, camera nudge: retained share {share:.4f} at the rectify frame (delay {t.rectify_delay} frames)")
    assert count == 1
    assert share >= 0.8, share
    t.close()


def test_tracer_switch_throws_without_temporal_reprojection_and_on_several_ranks():
    t = _tracer(32, 24)
    with pytest.raises(RuntimeError, match="setTemporalReprojection"):
        t.set_history_rectification(True)
    t.set_temporal_reprojection(True); t.set_history_rectification(True)
    with pytest.raises(RuntimeError, match="setRectifyDelay"):
        t.set_rectify_delay(-1)
    t.set_rectify_delay(5)
    assert t.rectify_delay == 5
    t.set_rectify_delay(0)
    assert t.rectify_delay == 2 * int(t.params["maxBounces"]) + 2
    t.set_temporal_reprojection(False)
    assert not t.history_rectification
    t.close()
    m = _tracer(32, 24, [0, 0])
    with pytest.raises(RuntimeError, match="single-GPU"):
        m.set_history_rectification(True)
    m.set_history_rectification(False)
    m.close()
