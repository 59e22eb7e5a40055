"""The variance-guided a-trous denoiser on the CPU: the CPU counterpart of the kernels (tests/denoise_cpu.cpp, which runs
fluctus_amd/csrc/flx_denoise_vg.h) against the float64 restatement (tests/denoise_vg_reference.py), its edge semantics, and its quality on
heavy-tailed noise, where the guided filter (flx_denoise) fails.  tests/test_gpu_denoise_variance.py holds the device to the counterpart bit
for bit and checks the moments the integrators accumulate."""
import numpy as np
import pytest
import denoise_reference as R
import denoise_vg_reference as V


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return R.build_cpu(tmp_path_factory.mktemp("denoise_cpu"))


def _check64(exe, px, alb, nrm, mom, W, H, **kw):
    got, _, var = R.run_cpu(exe, px, alb, nrm, W, H, mom=mom, with_variance=True, **kw)
    P = dict(R.VG_DEFAULTS, **kw)
    ref = V.denoise_vg64(px, alb, nrm, mom, W, H, **P)
    var64, _, guided, scale = V.initial_variance64(px, alb, nrm, mom, W, H, P["sigma_normal"], P["sigma_albedo"], with_scale=True)
    valid = R.prepare64(px, alb, nrm)[4]
    worst = R.close_to_reference(got, ref, valid)
    # the initial variance: 1e-4 relative, plus float32 cancellation of its two terms (a few ulp of their magnitude)
    tol = 1e-4 * np.abs(var64[guided]) + 1e-6 * np.minimum(scale[guided], 1e30) + 1e-30
    vworst = float((np.abs(var[guided] - var64[guided]) / tol).max()) if guided.any() else 0.0
    return got, ref, valid, worst, vworst


def _edge_inputs(W, H, seed):
    """consistent random moments, then n = 0 / 1 / 2, a non-finite or overflowing sum of squares, a count that disagrees with the colour's,
    and zero albedo on a few pixels each.  (Moments whose variance clamps to 0 next to pixels of nearly equal luminance are left to the
    bit-exact tests: there the luminance stop divides by FLX_VG_EPS, and float32 and float64 rounding decide different weights.)"""
    px, alb, nrm, mom = V.random_inputs(W, H, seed)
    N = W * H
    rng = np.random.default_rng(seed + 1)
    k = max(1, N // 20)
    for n in (0, 1, 2):
        idx = rng.choice(N, k, replace=False)
        if n:
            px[idx], mom[idx] = V.accumulate(rng.gamma(0.7, 1.0, (k, n, 3)).astype(np.float32))
        else:
            mom[idx] = 0.0
    mom[rng.choice(N, k), 1] = np.inf                              # sum l^2 overflowed on a firefly
    mom[rng.choice(N, k), 0] = 3e38                                # (S1 / n)^2 overflows float32
    mom[rng.choice(N, k), 3] = 7.0                                 # the moments' count disagrees with pixels.w (flx_write_pixels)
    alb[rng.choice(N, k), :3] = 0.0                                # zero albedo: floored
    alb[rng.choice(N, k), 3] = 0.0                                 # no surface hit: not guided
    return px, alb, nrm, mom


@pytest.mark.parametrize("W,H", [(1, 1), (1, 37), (53, 1), (333, 217)])
def test_counterpart_vs_float64_sizes(exe, W, H):
    px, alb, nrm, mom = V.random_inputs(W, H, W * 1000 + H)
    for K in (0, 1, 2, 5, 8):
        got, ref, valid, worst, vworst = _check64(exe, px, alb, nrm, mom, W, H, iterations=K)
        print(f"{W}x{H} K={K}: worst {worst:.3g}, initial variance worst {vworst:.3g}")
        assert valid.all() and worst <= 1.0 and vworst <= 1.0 and np.isfinite(got).all(), (K, worst, vworst)


@pytest.mark.parametrize("K", range(0, 9))
@pytest.mark.parametrize("blend", [0.0, 0.4, -0.5, 1.7])
def test_counterpart_vs_float64_iterations_blend_edges(exe, K, blend):
    W, H = 47, 31
    px, alb, nrm, mom = _edge_inputs(W, H, 10 + K)
    got, ref, valid, worst, vworst = _check64(exe, px, alb, nrm, mom, W, H, iterations=K, blend=blend, sigma_luminance=3.0)
    assert valid.all() and worst <= 1.0 and vworst <= 1.0, (worst, vworst)


def test_initial_variance_cases(exe):
    """the per-pixel estimate is the variance of the MEAN (/ n), demodulated by l(a')^2; n < 2 and non-finite sums fall back to the guided
    3 x 3 spread of the neighbours' demodulated luminance; the moments' own n counts"""
    W, H = 5, 4
    N = W * H
    px = np.zeros((N, 4), np.float32); px[:, :3] = 0.5 * 4; px[:, 3] = 4
    alb = np.tile(np.array([0.5, 0.5, 0.5, 1.0], np.float32), (N, 1))
    nrm = np.tile(np.array([0.0, 0.0, 1.0, 1.0], np.float32), (N, 1))
    px[7, :3] = 0.9 * 4                                            # one neighbour of a different brightness
    mom = np.zeros((N, 4), np.float32)
    mom[:, 0], mom[:, 1], mom[:, 3] = 2.0, 1.5, 4.0                 # l = 0.5 +- 0.5: sample variance 1.5/4 - 0.25 = 0.125
    mom[2] = (0.5, 0.25, 0.0, 1.0)                                  # n = 1: fallback
    mom[12] = (1.0, np.inf, 0.0, 2.0)                               # non-finite: fallback
    mom[13] = (2.0, 1.5, 0.0, 8.0)                                  # n disagrees with pixels.w: the moments' own n
    _, _, var = R.run_cpu(exe, px, alb, nrm, W, H, mom=mom, iterations=1, with_variance=True)
    var64, per, _ = V.initial_variance64(px, alb, nrm, mom, W, H, 0.3, 0.1)
    assert np.allclose(var, var64, rtol=1e-5, atol=0)
    la = 0.5
    assert np.isclose(var[0], 0.125 / 4 / la ** 2, rtol=1e-6)       # variance of the mean of 4 samples, in demodulated units
    m1, m2 = 2.0 / 8, 1.5 / 8
    assert np.isclose(var[13], (m2 - m1 * m1) / 8 / la ** 2, rtol=1e-6)
    assert not per[2] and not per[12] and per[0] and per[13]
    e = np.full(N, 1.0); e[7] = 1.8                                 # demodulated luminance: c / a' = 1, pixel 7 = 1.8
    nb = [1, 2, 3, 6, 7, 8]                                        # pixel 2 at (2, 0): its valid 3 x 3 neighbours
    want = e[nb].var()
    assert np.isclose(var[2], want, rtol=1e-5), (var[2], want)


@pytest.mark.parametrize("kw", [dict(iterations=0), dict(blend=1.0), dict(blend=3.0, iterations=8)])
def test_identity_is_exact(exe, kw):
    W, H = 37, 23
    px, alb, nrm, mom = _edge_inputs(W, H, 11)
    px[5] = (1.0, 2.0, 3.0, 0.0)                        # no samples: passed through
    alb[6] = (np.inf, 0.0, 0.0, 1.0)                    # non-finite guide: passed through
    out, _ = R.run_cpu(exe, px, alb, nrm, W, H, mom=mom, **kw)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = px[:, :3] / px[:, 3:4]
    keep = np.ones(W * H, bool); keep[[5, 6]] = False
    assert np.array_equal(out[keep, :3].view(np.uint32), c[keep].view(np.uint32))
    assert np.array_equal(out[~keep].view(np.uint32), px[~keep].view(np.uint32))


def test_invalid_pixels_pass_through_and_do_not_contaminate(exe):
    W, H = 40, 30
    px, alb, nrm, mom = V.random_inputs(W, H, 7)
    bad = [3, 50, 51, 200, 201, 640]
    px[3, 3] = 0.0; px[50, 0] = np.nan; px[51, 1] = np.inf; alb[200, 2] = np.inf; nrm[201, 0] = np.nan; px[640, 3] = -1.0
    mom[bad, 0] = 1e30                                  # their moments would dominate any neighbour's variance
    out, prev = R.run_cpu(exe, px, alb, nrm, W, H, mom=mom, iterations=6)
    idx = np.array(sorted(bad))
    assert np.array_equal(out[idx].view(np.uint32), px[idx].view(np.uint32))
    others = np.setdiff1d(np.arange(W * H), idx)
    assert np.isfinite(out[others]).all() and np.isfinite(prev[others]).all()
    got, ref, valid, worst, _ = _check64(exe, px, alb, nrm, mom, W, H, iterations=6)
    assert not valid[idx].any() and valid[others].all() and worst <= 1.0, worst
    # other values on the (still invalid) bad pixels give the same output everywhere else: they are never neighbours
    px2, mom2 = px.copy(), mom.copy()
    px2[3, :3] = 99.0; px2[50, 1:3] = 55.0; px2[51, 0] = 77.0; px2[640, :3] = -5.0; mom2[bad] = (0.0, 0.0, 0.0, 0.0)
    out2, _ = R.run_cpu(exe, px2, alb, nrm, W, H, mom=mom2, iterations=6)
    assert np.array_equal(out[others].view(np.uint32), out2[others].view(np.uint32))


def test_unguided_pixels_return_c_and_are_never_neighbours(exe):
    """a valid pixel whose albedo accumulator counted no surface hit (it saw the light or the environment directly) comes back as c, bit for
    bit, and its value never reaches a neighbour"""
    W, H = 40, 30
    px, alb, nrm, mom = V.random_inputs(W, H, 17)
    ung = np.zeros(W * H, bool); ung[[5, 6, 7, 45, 46, 47, 85, 86, 87, 300]] = True
    alb[ung] = (0.1, 0.1, 0.1, 0.0)                                # the resets' placeholder, count 0
    px[ung, :3] = 500.0 * px[ung, 3:4]                              # a bright light
    out, _ = R.run_cpu(exe, px, alb, nrm, W, H, mom=mom, iterations=5)
    c = px[:, :3] / px[:, 3:4]
    assert np.array_equal(out[ung, :3].view(np.uint32), c[ung].view(np.uint32)) and (out[ung, 3] == 1.0).all()
    px2 = px.copy(); px2[ung, :3] = 0.5 * px2[ung, 3:4]
    out2, _ = R.run_cpu(exe, px2, alb, nrm, W, H, mom=mom, iterations=5)
    assert np.array_equal(out[~ung].view(np.uint32), out2[~ung].view(np.uint32))
    got, ref, valid, worst, _ = _check64(exe, px, alb, nrm, mom, W, H, iterations=5)
    assert valid.all() and worst <= 1.0, worst


def test_constant_image_zero_variance_stays_constant(exe):
    W, H = 50, 30
    px = np.tile(np.array([0.3, 0.6, 0.9, 1.0], np.float32) * 8, (W * H, 1)); px[:, 3] = 8
    alb = np.tile(np.array([0.5, 0.4, 0.3, 1.0], np.float32), (W * H, 1))
    nrm = np.tile(np.array([0.0, 0.0, 1.0, 1.0], np.float32), (W * H, 1))
    l = V.lum32(np.array([[0.3, 0.6, 0.9]], np.float32))[0]
    mom = np.tile(np.array([8 * l, 8 * l * l, 0.0, 8.0], np.float32), (W * H, 1))
    out, _, var = R.run_cpu(exe, px, alb, nrm, W, H, mom=mom, iterations=8, with_variance=True)
    c = px[0, :3] / px[0, 3]
    assert var.max() < 1e-12
    assert np.allclose(out[:, :3], c, rtol=4 * np.finfo(np.float32).eps, atol=0), np.abs(out[:, :3] - c).max()


def test_half_planes_stay_apart(exe):
    W, H = 64, 48
    rng = np.random.default_rng(5)
    left = (np.arange(W * H) % W) < W // 2
    base = np.where(left[:, None], 0.2, 1.5)
    px, mom = V.accumulate((base[:, None, :] * (1.0 + 0.2 * rng.normal(size=(W * H, 4, 3)))).astype(np.float32))
    alb = np.tile(np.array([0.6, 0.6, 0.6, 1.0], np.float32), (W * H, 1))
    nrm = np.zeros((W * H, 4), np.float32); nrm[:, 3] = 1
    nrm[left, 0] = 1.0; nrm[~left, 2] = 1.0
    out, _ = R.run_cpu(exe, px, alb, nrm, W, H, mom=mom)
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
    px, mom = V.accumulate((a[:, None, None] * (1.0 + 0.3 * rng.normal(size=(W * H, 4, 3)))).astype(np.float32))
    out, _ = R.run_cpu(exe, px, alb, nrm, W, H, mom=mom)
    ratio_in = (px[~dark, :3] / 4).mean() / (px[dark, :3] / 4).mean()
    ratio_out = out[~dark, :3].mean() / out[dark, :3].mean()
    assert abs(ratio_out / ratio_in - 1.0) < 0.02, (ratio_in, ratio_out)


def test_quality_heavy_tailed(exe):
    """4 spp with a mean-1 multiplier that is 40 with probability 1 %: the guided filter keeps the outliers (ratio > 0.8), the
    variance-guided filter spreads them (ratio <= 0.5)"""
    W, H = 96, 64
    px, alb, nrm, mom, clean = V.heavy_tailed(W, H, 8)
    noisy = px[:, :3] / px[:, 3:4]
    g, _ = R.run_cpu(exe, px, alb, nrm, W, H)
    v, _ = R.run_cpu(exe, px, alb, nrm, W, H, mom=mom)
    rg = R.rmse(g, clean) / R.rmse(noisy, clean)
    rv = R.rmse(v, clean) / R.rmse(noisy, clean)
    print(f"heavy-tailed 4 spp: RMSE ratio guided {rg:.3f}, variance-guided {rv:.3f}")
    assert rg > 0.8, rg
    assert rv <= 0.5, rv


def test_sigma_luminance_sweep(exe):
    """the sweep behind FLX_VG_DEFAULT_SIGMA_LUMINANCE: RMSE ratio and texture contrast on the heavy-tailed input"""
    W, H = 96, 64
    px, alb, nrm, mom, clean = V.heavy_tailed(W, H, 9)
    noisy = px[:, :3] / px[:, 3:4]
    rows = []
    for sl in (0.5, 1.0, 2.0, 4.0, 8.0, 16.0):
        v, _ = R.run_cpu(exe, px, alb, nrm, W, H, mom=mom, sigma_luminance=sl)
        rows.append((sl, R.rmse(v, clean) / R.rmse(noisy, clean)))
        print(f"sigma_l {sl:5.1f}: RMSE ratio {rows[-1][1]:.3f}")
    best = dict(rows)
    assert best[4.0] <= 0.5 and best[4.0] < best[0.5]
