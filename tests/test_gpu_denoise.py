"""flx_denoise on the MI355X: bit-identical to the CPU counterpart (tests/denoise_cpu.cpp, the same header) on adversarial
inputs and on the device's own renders, the identity and preview contracts, ordering behind deferred launches, the errors, and the
Tracer's strength control."""
import numpy as np
import pytest
import common
import denoise_reference as R
from fluctus_amd import host, wire, driver

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return R.build_cpu(tmp_path_factory.mktemp("denoise_cpu_gpu"))


@pytest.fixture(scope="module")
def scene():
    return common.simple_scene()


def _ctx(d, W, H, denoiser=1, **kw):
    from fluctus_amd.device import HipContext
    g = HipContext(max(W * H, 64))
    if denoiser:
        g.set_option("denoiser", 1)
    g.upload_scene(d)
    g.set_params(common.scene_params(d, W, H, **kw))
    return g


def _tm(p):
    """the post-process parameters of a context's or Tracer's RenderParams, for the counterpart's preview"""
    return dict(exposure=float(p["exposure"]), tm_operator=int(p["tmOperator"]))


def _same(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _adversarial(W, H, seed):
    px, alb, nrm = R.random_inputs(W, H, seed)
    N = W * H
    rng = np.random.default_rng(seed + 100)
    k = max(1, N // 50)
    for col, vals in ((3, [0.0]), (0, [np.nan]), (1, [np.inf, -np.inf])):
        idx = rng.choice(N, k, replace=True)
        px[idx, col] = rng.choice(vals, k)
    alb[rng.choice(N, k), :3] = 0.0                      # zero albedo (floored)
    nrm[rng.choice(N, k), :4] = 0.0                      # zero normals
    alb[rng.choice(N, k), 3] = 0.0                       # unresolved accumulators (w <= 1: as is)
    return px, alb, nrm


def _device_denoise(g, px, alb, nrm, **kw):
    g.write_pixels(0, px); g.write_pixels(4, alb); g.write_pixels(5, nrm)
    g.denoise(**kw)
    g.finish()
    return g.read_pixels(6), g.read_pixels(1)


CASES = [(1, 1, 5, 0.0), (1, 37, 3, 0.5), (53, 1, 8, 0.0), (333, 217, 5, 0.0), (333, 217, 0, 0.0), (333, 217, 2, 1.0),
         (333, 217, 8, -0.5), (333, 217, 6, 7.0), (333, 217, 1, 0.5), (333, 217, 4, 0.0), (1920, 1080, 5, 0.0)]


@pytest.mark.parametrize("W,H,K,blend", CASES)
def test_bit_identical_to_cpu_adversarial(exe, scene, W, H, K, blend):
    g = _ctx(scene, W, H)
    px, alb, nrm = _adversarial(W, H, W + H + K)
    out, prev = _device_denoise(g, px, alb, nrm, iterations=K, blend=blend)
    cout, cprev = R.run_cpu(exe, px, alb, nrm, W, H, iterations=K, blend=blend, **_tm(g.params))
    assert _same(out, cout), int((out.view(np.uint32) != cout.view(np.uint32)).any(1).sum())
    assert _same(prev, cprev)


def test_bit_identical_other_sigmas_and_tonemaps(exe, scene):
    W, H = 200, 120
    for tm, sig in ((1, dict(sigma_color=0.25, sigma_normal=2.0, sigma_albedo=1e-3)), (2, dict(sigma_color=1e20, sigma_normal=1e-20, sigma_albedo=5.0))):
        g = _ctx(scene, W, H, tmOperator=tm, exposure=1.7)
        px, alb, nrm = _adversarial(W, H, tm)
        out, prev = _device_denoise(g, px, alb, nrm, iterations=5, **sig)
        cout, cprev = R.run_cpu(exe, px, alb, nrm, W, H, iterations=5, **_tm(g.params), **sig)
        assert _same(out, cout) and _same(prev, cprev), tm


def _mk_render(d, W, H, spp, env=None):
    from fluctus_amd.device import HipContext
    g = HipContext(W * H)
    g.set_option("denoiser", 1)
    g.upload_scene(d)
    if env is not None:
        g.upload_envmap(env)
    p = common.scene_params(d, W, H, maxBounces=4, useAreaLight=1, useEnvMap=int(env is not None))
    g.set_params(p)
    driver.render_single(g, p, spp)
    return g


def _wf_render(d, W, H, iters, env=None):
    from fluctus_amd.device import HipContext
    g = HipContext(W * H)
    g.set_option("extend_tree", 2)
    g.set_option("denoiser", 1)
    g.upload_scene(d)
    if env is not None:
        g.upload_envmap(env)
    g.set_params(common.scene_params(d, W, H, maxBounces=4, useAreaLight=1, useEnvMap=int(env is not None), wfSeparateQueues=1))
    driver.reset_renderer(g)
    for _ in range(iters):
        driver.benchmark_iteration(g, W * H)
    return g


@pytest.mark.parametrize("kind", ["microkernel", "wavefront", "egyptcat"])
def test_bit_identical_to_cpu_on_device_renders(exe, kind):
    W, H = 96, 72
    if kind == "microkernel":
        g = _mk_render(common.mixed_material_scene(), W, H, 4, env=host.synthetic_sky(64, 32))
    elif kind == "wavefront":
        g = _wf_render(common.mixed_material_scene(), W, H, 10, env=host.synthetic_sky(64, 32))
    else:
        g = _mk_render(common.egyptcat_scene(), W, H, 2)
    px, alb, nrm = g.read_pixels(0), g.read_pixels(4), g.read_pixels(5)
    for kw in (dict(), dict(iterations=8, blend=0.3)):
        g.denoise(**kw); g.finish()
        cout, cprev = R.run_cpu(exe, px, alb, nrm, W, H, **kw, **_tm(g.params))
        assert _same(g.read_pixels(6), cout) and _same(g.read_pixels(1), cprev), (kind, kw)
    assert _same(g.read_pixels(0), px)                    # the accumulation is not touched


@pytest.mark.parametrize("kw", [dict(blend=1.0), dict(iterations=0), dict(blend=2.5, iterations=3)])
def test_identity_preview_equals_postprocess(scene, kw):
    W, H = 120, 90
    g = _ctx(scene, W, H, tmOperator=2)
    px, alb, nrm = _adversarial(W, H, 3)
    g.write_pixels(0, px); g.write_pixels(4, alb); g.write_pixels(5, nrm)
    g.postprocess(); g.finish()
    want = g.read_pixels(1)
    g.denoise(**kw); g.finish()
    assert _same(g.read_pixels(1), want)


def test_preview_is_postprocess_of_denoised(scene):
    W, H = 150, 100
    g, h = _ctx(scene, W, H, tmOperator=1, exposure=0.8), _ctx(scene, W, H, tmOperator=1, exposure=0.8)
    px, alb, nrm = _adversarial(W, H, 4)
    out, prev = _device_denoise(g, px, alb, nrm, iterations=5, blend=0.2)
    h.write_pixels(0, out)
    h.postprocess(); h.finish()
    assert _same(prev, h.read_pixels(1))


def test_ordering_behind_deferred_logic():
    """fuse on: logic -> raygen -> materials -> extend -> shadow -> denoise with no finish between gives the flushed sequence's result"""
    d = common.mixed_material_scene()
    W, H = 64, 48
    gs = [_wf_render(d, W, H, 3) for _ in range(2)]
    for i, g in enumerate(gs):
        g.wf_logic(False); g.wf_raygen(); g.wf_materials(); g.wf_extend(); g.wf_shadow(); g.wf_logic(False)
        if i == 1:
            g.finish()
        g.denoise()
        g.finish()
    for which in (0, 4, 5, 6, 1):
        assert _same(gs[0].read_pixels(which), gs[1].read_pixels(which)), which


def test_errors(scene):
    W, H = 32, 16
    g = _ctx(scene, W, H, denoiser=0)
    with pytest.raises(RuntimeError, match="denoiser"):
        g.denoise()
    with pytest.raises(RuntimeError, match="denoiser"):
        g.read_pixels(6)
    g = _ctx(scene, W, H)
    with pytest.raises(RuntimeError, match="flx_denoise"):
        g.read_pixels(6)                                  # before any flx_denoise
    for bad in (dict(iterations=-1), dict(iterations=9)):
        with pytest.raises(RuntimeError, match="iterations must be 0..8"):
            g.denoise(**bad)
    for bad in (dict(sigma_color=0.0), dict(sigma_normal=-1.0), dict(sigma_albedo=float("nan")), dict(sigma_color=float("inf"))):
        with pytest.raises(RuntimeError, match="finite and > 0"):
            g.denoise(**bad)
    with pytest.raises(RuntimeError, match="which must be 0, 4 or 5"):
        g.write_pixels(1, np.zeros((W * H, 4), np.float32))
    g.denoise(); g.finish()
    assert g.read_pixels(6).shape == (W * H, 4)
    g.set_option("denoiser", 0)                           # the option off frees which = 6 with the feature buffers
    with pytest.raises(RuntimeError, match="denoiser"):
        g.read_pixels(6)
    g.set_option("denoiser", 1)
    g.set_partition(0, 2)
    with pytest.raises(RuntimeError, match="partitioned"):
        g.denoise()


def _tracer(W=64, H=48):
    from fluctus_amd.tracer import Tracer
    t = Tracer(W, H, 0, 4096)
    t.set_option("extend_tree", 2)
    t.init(W, H, "proc:kitchen:3000:7")
    p = t.params
    wire.look_at(p, (0.0, 1.2, 2.6), (0.0, 0.2, 0.0))
    p["maxBounces"] = 3
    t.params = p
    return t


def test_tracer_strength_zero_changes_nothing():
    a, b = _tracer(), _tracer()
    for t in (a, b):
        t.toggle_renderer()                               # the microkernel integrator: one thread per pixel, no float atomics -> exact
        t.set_denoiser(True)
    a.set_denoiser_strength(0.0)
    for _ in range(21):
        a.update(); b.update()
    for which in (0, 1, 2, 3, 4, 5):
        assert _same(a.read_pixels(which), b.read_pixels(which)), which
    with pytest.raises(RuntimeError, match="flx_denoise"):
        a.read_pixels(6)                                  # never denoised


def test_tracer_strength_one_denoises_at_10_and_20(exe):
    t = _tracer()
    W, H = 64, 48
    t.set_denoiser(True)
    t.set_denoiser_strength(1.0)
    hits = []
    for it in range(22):
        t.update()
        px, alb, nrm = t.read_pixels(0), t.read_pixels(4), t.read_pixels(5)
        _, plain = R.run_cpu(exe, px, alb, nrm, W, H, iterations=0, **_tm(t.params))
        prev = t.read_pixels(1)
        if not _same(prev, plain):
            _, den = R.run_cpu(exe, px, alb, nrm, W, H, blend=0.0, **_tm(t.params))
            assert _same(prev, den), it
            hits.append(it)
    assert hits == [10, 20], hits


def test_tracer_render_single_denoise(exe):
    from fluctus_amd.tracer import Tracer
    W, H = 64, 48
    t = Tracer(W, H, 0, W * H)
    t.init(W, H, "proc:kitchen:3000:7")
    t.set_denoiser_strength(0.75)
    t.render_single(4, denoise=True)
    px, alb, nrm = t.read_pixels(0), t.read_pixels(4), t.read_pixels(5)
    out, prev = R.run_cpu(exe, px, alb, nrm, W, H, blend=0.25, **_tm(t.params))
    assert _same(t.read_pixels(6), out) and _same(t.read_pixels(1), prev)


def test_quality_on_device_renders(exe):
    d = common.mixed_material_scene()
    W, H = 80, 60
    env = host.synthetic_sky(64, 32)
    lo, hi = _mk_render(d, W, H, 4, env=env), _mk_render(d, W, H, 512, env=env)
    h = hi.read_pixels(0); hic = h[:, :3] / h[:, 3:4]
    px = lo.read_pixels(0)
    lo.denoise(); lo.finish()
    out = lo.read_pixels(6)
    ratio = R.rmse(out, hic) / R.rmse(px[:, :3] / px[:, 3:4], hic)
    med = np.median(np.abs(out[:, :3] - hic)) / np.median(np.abs(px[:, :3] / px[:, 3:4] - hic))
    print(f"device microkernel 4 spp vs 512 spp: RMSE ratio {ratio:.3f}, median-abs-error ratio {med:.3f}")
    assert ratio <= 1.0 and med <= 1.0, (ratio, med)
