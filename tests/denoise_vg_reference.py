"""The variance-guided a-trous denoiser (fluctus_amd/csrc/flx_denoise_vg.h) restated formula by formula in numpy float64,
the luminance moments the integrators accumulate (option "moments", which = 7), and the inputs of the variance-guided tests.  The CPU
counterpart (tests/denoise_cpu.cpp) is run by denoise_reference.run_cpu with mom=.

The device and the CPU counterpart share one header, so comparing them proves the kernels run the header; comparing the counterpart with
this restatement proves the header computes what DESIGN.md says."""
import numpy as np
import denoise_reference as R

FLT_MAX = float(np.finfo(np.float32).max)
VAR_MAX = 1e30                  # FLX_VG_VAR_MAX
EPS = 1e-10                     # FLX_VG_EPS
EXP_CUT = 87.0                  # FLX_DN_EXP_CUT
LUM_W = (0.2126, 0.7152, 0.0722)
G3 = np.array([0.25, 0.5, 0.25])


def lum32(rgb):
    """flx_lum in float32, in the header's order (no FMA): what the integrators splat"""
    rgb = np.asarray(rgb, np.float32).reshape(-1, rgb.shape[-1] if hasattr(rgb, "shape") else 3)
    w = [np.float32(x) for x in LUM_W]
    return (w[0] * rgb[:, 0] + w[1] * rgb[:, 1]) + w[2] * rgb[:, 2]


def lum64(rgb):
    rgb = np.asarray(rgb, np.float64)
    return LUM_W[0] * rgb[..., 0] + LUM_W[1] * rgb[..., 1] + LUM_W[2] * rgb[..., 2]


def _cap(v):
    return np.where(np.isnan(v), VAR_MAX, np.clip(v, 0.0, VAR_MAX))


def _fin32(x):
    """finite as a float32 would be"""
    return np.abs(x) <= FLT_MAX


def _pairs(H, W, oy, ox):
    """(centre slices, neighbour slices) for the offset (oy, ox), or None when no centre has that neighbour inside the image"""
    ys, yd = slice(max(0, oy), H + min(0, oy)), slice(max(0, -oy), H - max(0, oy))
    xs, xd = slice(max(0, ox), W + min(0, ox)), slice(max(0, -ox), W - max(0, ox))
    if ys.start >= ys.stop or xs.start >= xs.stop:
        return None
    return (yd, xd), (ys, xs)


def initial_variance64(px, alb, nrm, mom, W, H, sigma_normal, sigma_albedo, with_scale=False):
    """-> (var (N,), per_pixel (N,) bool, valid (N,)): the initial variance of flx_denoise_vg.h in float64; `valid` is the header's (guided:
    the albedo accumulator counted a surface hit), other pixels 0.
    with_scale: also the magnitude of the two terms whose difference is the variance (mean of l^2 in the same units) -- float32 cancellation
    makes the counterpart's error proportional to it, not to the variance"""
    c, e, n, a, valid = R.prepare64(px, alb, nrm)
    valid = valid & (np.asarray(alb, np.float64).reshape(-1, 4)[:, 3] > 0.0)
    mom = np.asarray(mom, np.float64).reshape(-1, 4)
    m = mom[:, 3]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m1, m2 = mom[:, 0] / m, mom[:, 1] / m
        sq = m1 * m1
        per = (m >= 2.0) & _fin32(m) & _fin32(m1) & _fin32(m2) & _fin32(sq)
        la = lum64(a)
        vp = np.maximum(m2 - sq, 0.0) / m / (la * la)
    e, n, a = (np.where(valid[:, None], x, 0.0) for x in (e, n, a))
    L = lum64(e).reshape(H, W)
    Nn, A, V = n.reshape(H, W, 3), a.reshape(H, W, 3), valid.reshape(H, W).astype(np.float64)
    i_n, i_a = 1.0 / sigma_normal ** 2, 1.0 / sigma_albedo ** 2
    s0, s1, s2 = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W))
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            pr = _pairs(H, W, dy, dx)
            if pr is None:
                continue
            d, s = pr
            q = ((Nn[d] - Nn[s]) ** 2).sum(-1) * i_n + ((A[d] - A[s]) ** 2).sum(-1) * i_a
            u = np.where(q < EXP_CUT, np.exp(-q), 0.0) * V[s]
            s0[d] += u; s1[d] += u * L[s]; s2[d] += u * L[s] ** 2
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = s1 / s0
        vs = np.maximum(s2 / s0 - mean * mean, 0.0).reshape(-1)
    var = np.where(per, vp, vs)
    var = np.where(valid, _cap(var), 0.0)
    if with_scale:
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            scale = np.where(per, np.abs(m2) / m / (la * la), (s2 / s0).reshape(-1))
        return var, per & valid, valid, np.where(valid, scale, 0.0)
    return var, per & valid, valid


def denoise_vg64(px, alb, nrm, mom, W, H, iterations, sigma_luminance, sigma_normal, sigma_albedo, blend):
    """which = 6 of flx_denoise_variance_guided in float64: (N, 4).  Valid pixels (rgb, 1), invalid ones the raw accumulation; valid pixels
    that are not guided (no surface hit) are c."""
    px = np.asarray(px, np.float64).reshape(-1, 4)
    c, e, n, a, valid0 = R.prepare64(px, alb, nrm)
    valid = valid0 & (np.asarray(alb, np.float64).reshape(-1, 4)[:, 3] > 0.0)
    blend = min(max(float(blend), 0.0), 1.0)
    out = px.copy()
    out[valid0, :3] = c[valid0]; out[valid0, 3] = 1.0
    if blend == 1.0 or iterations == 0:
        return out
    var, _, _ = initial_variance64(px, alb, nrm, mom, W, H, sigma_normal, sigma_albedo)
    e, n, a = (np.where(valid[:, None], x, 0.0) for x in (e, n, a))
    E, Nn, A = e.reshape(H, W, 3), n.reshape(H, W, 3), a.reshape(H, W, 3)
    V, Var = valid.reshape(H, W).astype(np.float64), var.reshape(H, W)
    i_n, i_a = 1.0 / sigma_normal ** 2, 1.0 / sigma_albedo ** 2
    for k in range(iterations):
        s = 2 ** k
        gacc, gws = np.zeros((H, W)), np.zeros((H, W))
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                pr = _pairs(H, W, dy, dx)
                if pr is None:
                    continue
                d, sl = pr
                g = G3[dx + 1] * G3[dy + 1] * V[sl]
                gacc[d] += g * Var[sl]; gws[d] += g
        with np.errstate(invalid="ignore", divide="ignore"):
            gv = np.minimum(gacc / gws, Var)                  # clamped by the centre's own variance
        den = sigma_luminance * np.sqrt(np.where(V > 0, gv, 0.0)) + EPS
        L = lum64(E)
        acc, ws, vs = np.zeros_like(E), np.zeros((H, W)), np.zeros((H, W))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                pr = _pairs(H, W, dy * s, dx * s)
                if pr is None:
                    continue
                d, sl = pr
                q = (np.abs(L[d] - L[sl]) / den[d] + ((Nn[d] - Nn[sl]) ** 2).sum(-1) * i_n + ((A[d] - A[sl]) ** 2).sum(-1) * i_a)
                w = R.H5[dx + 2] * R.H5[dy + 2] * np.where(q < EXP_CUT, np.exp(-q), 0.0) * V[sl]
                acc[d] += w[..., None] * E[sl]; ws[d] += w; vs[d] += w * w * Var[sl]
        with np.errstate(invalid="ignore", divide="ignore"):
            E = np.where(V[..., None] > 0, acc / ws[..., None], E)
            Var = np.where(V > 0, _cap(vs / (ws * ws)), 0.0)
    d = E.reshape(-1, 3) * a
    out[valid, :3] = blend * c[valid] + (1.0 - blend) * d[valid]
    out[valid, 3] = 1.0
    return out


# ---- inputs
def accumulate(samples):
    """per-pixel samples (N, spp, 3) float32 -> (pixels (N, 4), moments (N, 4)) summed in float32 in sample order, as a splat does"""
    samples = np.asarray(samples, np.float32)
    N, spp = samples.shape[:2]
    px = np.zeros((N, 4), np.float32); mom = np.zeros((N, 4), np.float32)
    for s in range(spp):
        e = samples[:, s]
        l = lum32(e)
        px[:, :3] += e; px[:, 3] += np.float32(1.0)
        mom[:, 0] += l; mom[:, 1] += l * l; mom[:, 3] += np.float32(1.0)
    return px, mom


def random_inputs(W, H, seed, spp=4):
    """random accumulations with consistent moments: `spp` gamma samples per pixel, albedo and normal accumulators as the integrators
    leave them"""
    _, alb, nrm = R.random_inputs(W, H, seed, spp)
    rng = np.random.default_rng(seed + 7)
    px, mom = accumulate(rng.gamma(0.7, 1.0, (W * H, spp, 3)).astype(np.float32))
    return px, alb, nrm, mom


def heavy_tailed(W, H, seed, spp=4, p_out=0.01, big=40.0):
    """a textured two-surface scene (tests/test_denoise.py's synthetic quality case) rendered with a mean-1 per-sample multiplier that is
    `big` with probability p_out and (1 - p_out big) / (1 - p_out) otherwise: rare, large outliers like caustics and visible lights.
    -> (pixels, albedo, normal, moments, clean)"""
    rng = np.random.default_rng(seed)
    N = W * H
    x, y = np.arange(N) % W, np.arange(N) // W
    wall = y < H // 2
    a = np.where(((x // 6 + y // 6) % 2) == 0, 0.25, 0.75)[:, None] * np.array([1.0, 0.8, 0.6])
    light = np.where(wall, 1.0, 0.4)[:, None] * (1.0 + 0.5 * x[:, None] / W)
    clean = (a * light).astype(np.float32)
    lo = (1.0 - p_out * big) / (1.0 - p_out)
    mult = np.where(rng.random((N, spp, 1)) < p_out, big, lo) * rng.gamma(8.0, 1.0 / 8.0, (N, spp, 1))
    px, mom = accumulate((clean[:, None, :] * mult).astype(np.float32))
    alb = np.zeros((N, 4), np.float32); alb[:, :3] = a * spp; alb[:, 3] = spp
    nrm = np.zeros((N, 4), np.float32); nrm[:, 3] = spp
    nrm[wall, 2] = spp; nrm[~wall, 1] = spp
    return px, alb, nrm, mom, clean
