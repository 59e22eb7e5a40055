"""The guided a-trous denoiser on the CPU: the CPU counterpart of the kernels (tests/denoise_cpu.cpp, which runs
fluctus_amd/csrc/flx_denoise.h) against the float64 restatement (tests/denoise_reference.py), its edge semantics, and its quality on
oracle renders.  tests/test_gpu_denoise.py holds the device to the counterpart bit for bit."""
import numpy as np
import pytest
import common
import denoise_reference as R
from fluctus_amd import host, driver


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return R.build_cpu(tmp_path_factory.mktemp("denoise_cpu"))


def _check64(exe, px, alb, nrm, W, H, **kw):
    got, _ = R.run_cpu(exe, px, alb, nrm, W, H, **kw)
    P = dict(R.DEFAULTS, **kw)
    ref = R.denoise64(px, alb, nrm, W, H, **P)
    valid = R.prepare64(px, alb, nrm)[4]
    worst = R.close_to_reference(got, ref, valid)
    return got, ref, valid, worst


@pytest.mark.parametrize("W,H,K,blend,seed", [(64, 48, 5, 0.0, 1), (33, 71, 1, 0.0, 2), (40, 40, 3, 0.5, 3), (96, 20, 8, 0.0, 4),
                                              (17, 9, 5, -0.3, 5), (333, 217, 5, 0.0, 6)])
def test_counterpart_vs_float64_random(exe, W, H, K, blend, seed):
    px, alb, nrm = R.random_inputs(W, H, seed)
    got, ref, valid, worst = _check64(exe, px, alb, nrm, W, H, iterations=K, blend=blend, sigma_color=2.0)
    print(f"{W}x{H} K={K}: worst error / (1e-4 |ref| + 1e-6) = {worst:.3g}")
    assert valid.all() and worst <= 1.0, worst
    assert np.array_equal(got[:, 3], np.ones(W * H, np.float32))


def _oracle_render(d, p, spp=None, iterations=None, env=None):
    from oracle.binding import OracleContext
    W, H = int(p["width"]), int(p["height"])
    o = OracleContext(W * H, threads=8)
    o.set_option("denoiser", 1)
    o.upload_scene(d)
    if env is not None:
        o.upload_envmap(env)
    o.set_params(p)
    if spp is not None:
        driver.render_single(o, p, spp)
    else:
        driver.reset_renderer(o)
        for _ in range(iterations):
            driver.benchmark_iteration(o, W * H)
    return o.read_pixels(0), o.read_pixels(4), o.read_pixels(5)


@pytest.fixture(scope="module")
def renders():
    d = common.mixed_material_scene()
    W, H = 80, 60
    p = common.scene_params(d, W, H, maxBounces=4, useAreaLight=1, useEnvMap=1)
    env = host.synthetic_sky(64, 32)
    return dict(W=W, H=H, mk4=_oracle_render(d, p, spp=4, env=env), mk_hi=_oracle_render(d, p, spp=512, env=env),
                wf10=_oracle_render(d, p, iterations=10, env=env))


@pytest.mark.parametrize("which", ["mk4", "wf10"])
@pytest.mark.parametrize("K,blend", [(5, 0.0), (8, 0.25)])
def test_counterpart_vs_float64_oracle_render(exe, renders, which, K, blend):
    W, H = renders["W"], renders["H"]
    got, ref, valid, worst = _check64(exe, *renders[which], W, H, iterations=K, blend=blend)
    print(f"{which} K={K}: valid {valid.mean():.3f}, worst error / (1e-4 |ref| + 1e-6) = {worst:.3g}")
    assert valid.sum() > 0.5 * W * H and worst <= 1.0, worst


@pytest.mark.parametrize("kw", [dict(iterations=0), dict(blend=1.0), dict(blend=3.0, iterations=8)])
def test_identity_is_exact(exe, kw):
    W, H = 37, 23
    px, alb, nrm = R.random_inputs(W, H, 11)
    px[5] = (1.0, 2.0, 3.0, 0.0)                        # no samples: passed through
    alb[6] = (np.inf, 0.0, 0.0, 1.0)                    # non-finite guide: passed through
    out, prev = R.run_cpu(exe, px, alb, nrm, W, H, **kw)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = px[:, :3] / px[:, 3:4]
    keep = np.ones(W * H, bool); keep[[5, 6]] = False
    assert np.array_equal(out[keep, :3].view(np.uint32), c[keep].view(np.uint32))
    assert np.array_equal(out[~keep].view(np.uint32), px[~keep].view(np.uint32))


def test_constant_image_stays_constant(exe):
    W, H = 50, 30
    px = np.tile(np.array([0.3, 0.6, 0.9, 1.0], np.float32) * 8, (W * H, 1)); px[:, 3] = 8
    alb = np.tile(np.array([0.5, 0.4, 0.3, 1.0], np.float32), (W * H, 1))
    nrm = np.tile(np.array([0.0, 0.0, 1.0, 1.0], np.float32), (W * H, 1))
    out, _ = R.run_cpu(exe, px, alb, nrm, W, H, iterations=8)
    c = px[0, :3] / px[0, 3]
    assert np.allclose(out[:, :3], c, rtol=4 * np.finfo(np.float32).eps, atol=0), np.abs(out[:, :3] - c).max()


def test_half_planes_stay_apart(exe):
    W, H = 64, 48
    rng = np.random.default_rng(5)
    left = (np.arange(W * H) % W) < W // 2
    px = np.zeros((W * H, 4), np.float32); px[:, 3] = 4
    base = np.where(left[:, None], 0.2, 1.5)
    px[:, :3] = (base + 0.1 * rng.normal(size=(W * H, 3))) * 4
    alb = np.tile(np.array([0.6, 0.6, 0.6, 1.0], np.float32), (W * H, 1))
    nrm = np.zeros((W * H, 4), np.float32); nrm[:, 3] = 1
    nrm[left, 0] = 1.0; nrm[~left, 2] = 1.0
    out, _ = R.run_cpu(exe, px, alb, nrm, W, H)
    mL, mR = out[left, :3].mean(), out[~left, :3].mean()
    assert abs(mL - 0.2) <= 0.02 * (1.5 - 0.2) and abs(mR - 1.5) <= 0.02 * (1.5 - 0.2), (mL, mR)
    assert out[left, :3].std() < 0.5 * (px[left, :3] / 4).std()           # and it did filter


def test_albedo_checker_keeps_contrast(exe):
    W, H = 64, 64
    rng = np.random.default_rng(6)
    x, y = np.arange(W * H) % W, np.arange(W * H) // W
    dark = ((x // 8 + y // 8) % 2) == 0
    a = np.where(dark, 0.1, 0.8).astype(np.float32)
    alb = np.zeros((W * H, 4), np.float32); alb[:, :3] = a[:, None]; alb[:, 3] = 1
    nrm = np.tile(np.array([0.0, 1.0, 0.0, 1.0], np.float32), (W * H, 1))
    px = np.zeros((W * H, 4), np.float32); px[:, 3] = 4
    px[:, :3] = (a[:, None] * (1.0 + 0.3 * rng.normal(size=(W * H, 3)))) * 4       # flat lighting x albedo, noisy
    out, _ = R.run_cpu(exe, px, alb, nrm, W, H)
    ratio_in = (px[~dark, :3] / 4).mean() / (px[dark, :3] / 4).mean()
    ratio_out = out[~dark, :3].mean() / out[dark, :3].mean()
    assert abs(ratio_out / ratio_in - 1.0) < 0.02, (ratio_in, ratio_out)


def test_invalid_pixels_pass_through_and_do_not_contaminate(exe):
    W, H = 40, 30
    px, alb, nrm = R.random_inputs(W, H, 7)
    bad = {3: "count0", 50: "nan", 51: "inf", 200: "albedo_inf", 201: "normal_nan", 640: "neg_count"}
    px[3, 3] = 0.0
    px[50, 0] = np.nan
    px[51, 1] = np.inf
    alb[200, 2] = np.inf
    nrm[201, 0] = np.nan
    px[640, 3] = -1.0
    alb[300, :3] = 0.0                                  # zero albedo: floored, a valid pixel
    out, prev = R.run_cpu(exe, px, alb, nrm, W, H, iterations=6)
    idx = np.array(sorted(bad))
    assert np.array_equal(out[idx].view(np.uint32), px[idx].view(np.uint32))
    others = np.setdiff1d(np.arange(W * H), idx)
    assert np.isfinite(out[others]).all() and np.isfinite(prev[others]).all()
    got, ref, valid, worst = _check64(exe, px, alb, nrm, W, H, iterations=6)
    assert not valid[idx].any() and valid[others].all() and worst <= 1.0, worst


@pytest.mark.parametrize("W,H", [(1, 1), (1, 37), (53, 1), (333, 217)])
def test_image_sizes(exe, W, H):
    px, alb, nrm = R.random_inputs(W, H, W * 1000 + H)
    for K in (1, 5, 8):
        got, ref, valid, worst = _check64(exe, px, alb, nrm, W, H, iterations=K)
        assert worst <= 1.0 and np.isfinite(got).all(), (K, worst)


def test_quality_synthetic_noise(exe):
    """Estimator-like noise on a scene with albedo texture and two surfaces: the filter halves the error (and more)."""
    W, H = 96, 64
    rng = np.random.default_rng(8)
    x, y = np.arange(W * H) % W, np.arange(W * H) // W
    wall = y < H // 2
    a = np.where(((x // 6 + y // 6) % 2) == 0, 0.25, 0.75)[:, None] * np.array([1.0, 0.8, 0.6])
    light = np.where(wall, 1.0, 0.4)[:, None] * (1.0 + 0.5 * x[:, None] / W)
    clean = (a * light).astype(np.float32)
    spp = 4
    px = np.zeros((W * H, 4), np.float32); px[:, 3] = spp
    px[:, :3] = (clean * rng.gamma(4.0, 0.25, (W * H, 3))) * spp            # mean-preserving, sample-mean-like noise
    alb = np.zeros((W * H, 4), np.float32); alb[:, :3] = a * spp; alb[:, 3] = spp
    nrm = np.zeros((W * H, 4), np.float32); nrm[:, 3] = spp
    nrm[wall, 2] = spp; nrm[~wall, 1] = spp
    out, _ = R.run_cpu(exe, px, alb, nrm, W, H)
    ratio = R.rmse(out, clean) / R.rmse(px[:, :3] / spp, clean)
    print(f"synthetic: RMSE(denoised) / RMSE(noisy) = {ratio:.3f}")
    assert ratio <= 0.5, ratio


def test_quality_oracle_renders(exe, renders):
    """mixed_material_scene at 80 x 60: 4 spp (microkernel) and 10 wavefront iterations against 512 spp.  The ratios are printed and
    recorded in DESIGN.md 4.3.1; the scene's error is dominated by heavy-tailed samples (caustics through the dielectrics, the directly
    visible area light) that a colour-stopped filter keeps by design, so the bar here is that denoising never adds error."""
    hi = renders["mk_hi"][0]
    hic = hi[:, :3] / hi[:, 3:4]
    for which in ("mk4", "wf10"):
        px = renders[which][0]
        cov = px[:, 3] > 0
        noisy = np.where(cov[:, None], px[:, :3] / np.maximum(px[:, 3:4], 1e-30), 0.0)
        out, _ = R.run_cpu(exe, *renders[which], renders["W"], renders["H"])
        ratio = R.rmse(out[cov], hic[cov]) / R.rmse(noisy[cov], hic[cov])
        med = np.median(np.abs(out[cov, :3] - hic[cov])) / np.median(np.abs(noisy[cov] - hic[cov]))
        print(f"{which}: RMSE ratio {ratio:.3f}, median-abs-error ratio {med:.3f}")
        assert ratio <= 1.0 and med <= 1.0, (which, ratio, med)
