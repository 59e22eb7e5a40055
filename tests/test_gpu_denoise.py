"""flx_denoise on the MI355X: bit-identical to the CPU counterpart (tests/denoise_cpu.cpp, the same header) on adversarial
inputs and on the device's own renders, the identity and preview contracts, ordering behind deferred launches, the errors, and the
Tracer's strength control."""
import numpy as np
import pytest
import common
import denoise_reference as R
from fluctus_amd import host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return R.build_cpu(tmp_path_factory.mktemp("denoise_cpu_gpu"))


@pytest.fixture(scope="module")
def scene():
    return common.simple_scene()


CASES = [(1, 1, 5, 0.0), (1, 37, 3, 0.5), (53, 1, 8, 0.0), (333, 217, 5, 0.0), (333, 217, 0, 0.0), (333, 217, 2, 1.0),
         (333, 217, 8, -0.5), (333, 217, 6, 7.0), (333, 217, 1, 0.5), (333, 217, 4, 0.0), (1920, 1080, 5, 0.0)]


@pytest.mark.parametrize("W,H,K,blend", CASES)
def test_bit_identical_to_cpu_adversarial(exe, scene, W, H, K, blend):
    R.check_device_vs_cpu_adversarial(exe, scene, W, H, K, blend)


def test_bit_identical_other_sigmas_and_tonemaps(exe, scene):
    R.check_device_vs_cpu_sigmas(exe, scene, ((1, dict(sigma_color=0.25, sigma_normal=2.0, sigma_albedo=1e-3)),
                                              (2, dict(sigma_color=1e20, sigma_normal=1e-20, sigma_albedo=5.0))))


@pytest.mark.parametrize("kind", ["microkernel", "wavefront", "egyptcat"])
def test_bit_identical_to_cpu_on_device_renders(exe, kind):
    R.check_device_vs_cpu_on_render(exe, kind)


@pytest.mark.parametrize("kw", [dict(blend=1.0), dict(iterations=0), dict(blend=2.5, iterations=3)])
def test_identity_preview_equals_postprocess(scene, kw):
    W, H = 120, 90
    g = R.ctx(scene, W, H, tmOperator=2)
    px, alb, nrm = R.adversarial(W, H, 3)
    g.write_pixels(0, px); g.write_pixels(4, alb); g.write_pixels(5, nrm)
    g.postprocess(); g.finish()
    want = g.read_pixels(1)
    g.denoise(**kw); g.finish()
    assert R.same(g.read_pixels(1), want)


def test_preview_is_postprocess_of_denoised(scene):
    W, H = 150, 100
    g, h = R.ctx(scene, W, H, tmOperator=1, exposure=0.8), R.ctx(scene, W, H, tmOperator=1, exposure=0.8)
    px, alb, nrm = R.adversarial(W, H, 4)
    out, prev = R.device_denoise(g, px, alb, nrm, iterations=5, blend=0.2)
    h.write_pixels(0, out)
    h.postprocess(); h.finish()
    assert R.same(prev, h.read_pixels(1))


def test_ordering_behind_deferred_logic():
    """fuse on: logic -> raygen -> materials -> extend -> shadow -> denoise with no finish between gives the flushed sequence's result"""
    d = common.mixed_material_scene()
    W, H = 64, 48
    gs = [R.wf_render(d, W, H, 3) for _ in range(2)]
    for i, g in enumerate(gs):
        g.wf_logic(False); g.wf_raygen(); g.wf_materials(); g.wf_extend(); g.wf_shadow(); g.wf_logic(False)
        if i == 1:
            g.finish()
        g.denoise()
        g.finish()
    for which in (0, 4, 5, 6, 1):
        assert R.same(gs[0].read_pixels(which), gs[1].read_pixels(which)), which


def test_errors(scene):
    W, H = 32, 16
    g = R.ctx(scene, W, H, denoiser=0)
    with pytest.raises(RuntimeError, match="denoiser"):
        g.denoise()
    with pytest.raises(RuntimeError, match="denoiser"):
        g.read_pixels(6)
    g = R.ctx(scene, W, H)
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


def test_tracer_strength_zero_changes_nothing():
    a, b = R.tracer(), R.tracer()
    for t in (a, b):
        t.toggle_renderer()                               # the microkernel integrator: one thread per pixel, no float atomics -> exact
        t.set_denoiser(True)
    a.set_denoiser_strength(0.0)
    for _ in range(21):
        a.update(); b.update()
    for which in (0, 1, 2, 3, 4, 5):
        assert R.same(a.read_pixels(which), b.read_pixels(which)), which
    with pytest.raises(RuntimeError, match="flx_denoise"):
        a.read_pixels(6)                                  # never denoised


def test_tracer_strength_one_denoises_at_10_and_20(exe):
    t = R.tracer()
    W, H = 64, 48
    t.set_denoiser(True)
    t.set_denoiser_strength(1.0)
    hits = []
    for it in range(22):
        t.update()
        px, alb, nrm = t.read_pixels(0), t.read_pixels(4), t.read_pixels(5)
        _, plain = R.run_cpu(exe, px, alb, nrm, W, H, iterations=0, **R.tm(t.params))
        prev = t.read_pixels(1)
        if not R.same(prev, plain):
            _, den = R.run_cpu(exe, px, alb, nrm, W, H, blend=0.0, **R.tm(t.params))
            assert R.same(prev, den), it
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
    out, prev = R.run_cpu(exe, px, alb, nrm, W, H, blend=0.25, **R.tm(t.params))
    assert R.same(t.read_pixels(6), out) and R.same(t.read_pixels(1), prev)


def test_quality_on_device_renders(exe):
    d = common.mixed_material_scene()
    W, H = 80, 60
    env = host.synthetic_sky(64, 32)
    lo, hi = R.mk_render(d, W, H, 4, env=env), R.mk_render(d, W, H, 512, env=env)
    h = hi.read_pixels(0); hic = h[:, :3] / h[:, 3:4]
    px = lo.read_pixels(0)
    lo.denoise(); lo.finish()
    out = lo.read_pixels(6)
    ratio = R.rmse(out, hic) / R.rmse(px[:, :3] / px[:, 3:4], hic)
    med = np.median(np.abs(out[:, :3] - hic)) / np.median(np.abs(px[:, :3] / px[:, 3:4] - hic))
    print(f"device microkernel 4 spp vs 512 spp: RMSE ratio {ratio:.3f}, median-abs-error ratio {med:.3f}")
    assert ratio <= 1.0 and med <= 1.0, (ratio, med)
