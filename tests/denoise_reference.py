"""The guided a-trous denoiser (fluctus_amd/csrc/flx_denoise.h) restated formula by formula in numpy float64, and the
helpers the denoiser tests of both filters share: building and running the CPU counterpart (tests/denoise_cpu.cpp), inputs, error measures,
and the device side of the GPU tests.

The device and the CPU counterpart share one header, so comparing them proves the kernels run the header; comparing the counterpart with
this restatement proves the header computes what DESIGN.md says."""
import os
import subprocess
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS_ALBEDO = 1e-3
H5 = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
DEFAULTS = dict(iterations=5, sigma_color=2.0, sigma_normal=0.3, sigma_albedo=0.1, blend=0.0)     # = FLX_DN_DEFAULT_*
VG_DEFAULTS = dict(iterations=5, sigma_luminance=4.0, sigma_normal=0.3, sigma_albedo=0.1, blend=0.0)  # = FLX_VG_DEFAULT_*


def _resolve(g):
    """guide accumulator -> guide (k_postprocess: w > 1 ? sum / w : as is)"""
    w = g[:, 3:4]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return np.where(w > 1.0, g[:, :3] / np.where(w > 1.0, w, 1.0), g[:, :3])


def prepare64(px, alb, nrm):
    """-> colour c, demodulated e, normal n, floored albedo a', valid (all float64, flat pixel order)"""
    px, alb, nrm = (np.asarray(x, np.float64).reshape(-1, 4) for x in (px, alb, nrm))
    n = _resolve(nrm)
    a = np.fmax(_resolve(alb), EPS_ALBEDO)                     # fmax: a NaN albedo floors to eps, as fmaxf_ does
    count = px[:, 3:4]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        c = np.where(count > 0.0, px[:, :3] / np.where(count > 0.0, count, 1.0), 0.0)
        e = c / a
    valid = (count[:, 0] > 0.0) & np.isfinite(e).all(1) & np.isfinite(a).all(1) & np.isfinite(n).all(1)
    return c, e, n, a, valid


def denoise64(px, alb, nrm, W, H, iterations, sigma_color, sigma_normal, sigma_albedo, blend):
    """which = 6 of flx_denoise in float64: (N, 4).  Valid pixels (rgb, 1), invalid ones the raw accumulation."""
    px = np.asarray(px, np.float64).reshape(-1, 4)
    c, e, n, a, valid = prepare64(px, alb, nrm)
    blend = min(max(float(blend), 0.0), 1.0)
    out = px.copy()
    if blend == 1.0 or iterations == 0:
        out[valid, :3] = c[valid]; out[valid, 3] = 1.0
        return out
    # an invalid pixel is never a neighbour: its weight is 0, and its (possibly non-finite) values must not reach the sums as 0 * inf
    e, n, a = (np.where(valid[:, None], x, 0.0) for x in (e, n, a))
    E, Nn, A, V = (x.reshape(H, W, -1) for x in (e, n, a, valid.astype(np.float64)))
    i_n, i_a = 1.0 / sigma_normal ** 2, 1.0 / sigma_albedo ** 2
    for k in range(iterations):
        s = 2 ** k
        ic = 1.0 / (sigma_color * 2.0 ** -k) ** 2
        acc = np.zeros_like(E); ws = np.zeros((H, W, 1))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = dy * s, dx * s
                # neighbour j of every centre i = (y, x): (y + oy, x + ox), where inside the image
                ys, yd = slice(max(0, oy), H + min(0, oy)), slice(max(0, -oy), H - max(0, oy))
                xs, xd = slice(max(0, ox), W + min(0, ox)), slice(max(0, -ox), W - max(0, ox))
                if ys.start >= ys.stop or xs.start >= xs.stop:
                    continue
                Ej, Nj, Aj, Vj = E[ys, xs], Nn[ys, xs], A[ys, xs], V[ys, xs]
                q = (((E[yd, xd] - Ej) ** 2).sum(-1, keepdims=True) * ic + ((Nn[yd, xd] - Nj) ** 2).sum(-1, keepdims=True) * i_n
                     + ((A[yd, xd] - Aj) ** 2).sum(-1, keepdims=True) * i_a)
                w = H5[dx + 2] * H5[dy + 2] * np.exp(-q) * Vj
                acc[yd, xd] += w * Ej
                ws[yd, xd] += w
        with np.errstate(invalid="ignore", divide="ignore"):
            E = np.where(V > 0, acc / ws, E)
    d = E.reshape(-1, 3) * a
    out[valid, :3] = blend * c[valid] + (1.0 - blend) * d[valid]
    out[valid, 3] = 1.0
    return out


# ---- the CPU counterpart
def build_cpu(outdir):
    """g++ -O2 -ffp-contract=off tests/denoise_cpu.cpp -> <outdir>/denoise_cpu.  A failed compile raises."""
    exe = os.path.join(str(outdir), "denoise_cpu")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "denoise_cpu.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, "denoise_cpu.cpp does not compile:\n" + r.stdout
    return exe


def run_cpu(exe, px, alb, nrm, W, H, mom=None, iterations=None, sigma_color=None, sigma_luminance=None, sigma_normal=None, sigma_albedo=None,
            blend=None, exposure=1.0, tm_operator=0, with_variance=False):
    """-> (which = 6, preview) of the counterpart, float32 (W*H, 4) each [, initial variance (W*H,) with with_variance].  mom (the moments,
    which = 7) selects the variance-guided filter, whose sigma is sigma_luminance; the guided filter's is sigma_color.  None = the library's
    default."""
    vg = mom is not None
    assert (sigma_color if vg else sigma_luminance) is None and (vg or not with_variance), "the other filter's parameter"
    P = dict(VG_DEFAULTS if vg else DEFAULTS)
    for k, v in dict(iterations=iterations, sigma_color=sigma_color, sigma_luminance=sigma_luminance, sigma_normal=sigma_normal,
                     sigma_albedo=sigma_albedo, blend=blend).items():
        if v is not None:
            P[k] = v
    d = os.path.dirname(exe)
    fin, fout = os.path.join(d, "dn_in.bin"), os.path.join(d, "dn_out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([W, H, P["iterations"], int(vg)], np.int32).tobytes())
        sigma = P["sigma_luminance"] if vg else P["sigma_color"]
        f.write(np.array([sigma, P["sigma_normal"], P["sigma_albedo"], P["blend"], exposure], np.float32).tobytes())
        f.write(np.array([tm_operator], np.uint32).tobytes())
        for a in (px, alb, nrm) + ((mom,) if vg else ()):
            a = np.ascontiguousarray(a, np.float32).reshape(-1, 4)
            assert a.shape[0] == W * H
            f.write(a.tobytes())
    r = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    raw = np.fromfile(fout, np.float32)
    o = raw[:W * H * 8].reshape(2, W * H, 4)
    if with_variance:
        return o[0].copy(), o[1].copy(), raw[W * H * 8:].copy()
    return o[0].copy(), o[1].copy()


# ---- inputs and measures
def random_inputs(W, H, seed, spp=4):
    """random accumulations: radiance sums of `spp` samples, albedo and normal accumulators as the integrators leave them"""
    rng = np.random.default_rng(seed)
    N = W * H
    px = np.zeros((N, 4), np.float32)
    px[:, 3] = spp
    px[:, :3] = rng.gamma(0.7, 1.0, (N, 3)) * spp
    alb = np.zeros((N, 4), np.float32)
    alb[:, :3] = rng.uniform(0.0, 1.0, (N, 3)) * spp; alb[:, 3] = spp
    nrm = np.zeros((N, 4), np.float32)
    v = rng.normal(size=(N, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)
    nrm[:, :3] = v * spp; nrm[:, 3] = spp
    return px, alb, nrm


def close_to_reference(got, ref, valid, rtol=1e-4, atol=1e-6):
    """worst |got - ref| / (rtol |ref| + atol) over the valid pixels' rgb: <= 1 passes"""
    g, r = np.asarray(got, np.float64)[valid, :3], np.asarray(ref, np.float64)[valid, :3]
    if not g.size:
        return 0.0
    return float((np.abs(g - r) / (rtol * np.abs(r) + atol)).max())


def rmse(a, b):
    a, b = np.asarray(a, np.float64)[:, :3], np.asarray(b, np.float64)[:, :3]
    return float(np.sqrt(((a - b) ** 2).mean()))


# ---- the device side of the GPU tests (tests/test_gpu_denoise.py, tests/test_gpu_denoise_variance.py)
def same(a, b):
    """bit for bit"""
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def tm(p):
    """the post-process parameters of a context's or Tracer's RenderParams, for the counterpart's preview"""
    return dict(exposure=float(p["exposure"]), tm_operator=int(p["tmOperator"]))


def ctx(d, W, H, n=None, denoiser=1, moments=0, env=None, **kw):
    """a context on scene d with the denoiser's options, params for W x H (kw: scene_params overrides)"""
    import common
    from fluctus_amd.device import HipContext
    g = HipContext(n or max(W * H, 64))
    if denoiser:
        g.set_option("denoiser", 1)
    if moments:
        g.set_option("moments", 1)
    g.upload_scene(d)
    if env is not None:
        g.upload_envmap(env)
    g.set_params(common.scene_params(d, W, H, **kw))
    return g


def mk_render(d, W, H, spp, env=None, moments=0):
    """a microkernel render of `spp` samples per pixel"""
    import common
    from fluctus_amd import driver
    kw = dict(maxBounces=4, useAreaLight=1, useEnvMap=int(env is not None))
    g = ctx(d, W, H, n=W * H, moments=moments, env=env, **kw)
    driver.render_single(g, common.scene_params(d, W, H, **kw), spp)
    return g


def wf_render(d, W, H, iters, env=None, moments=0):
    """`iters` wavefront iterations (extend_tree 2, separate queues)"""
    from fluctus_amd import driver
    g = ctx(d, W, H, n=W * H, moments=moments, env=env, maxBounces=4, useAreaLight=1, useEnvMap=int(env is not None), wfSeparateQueues=1)
    g.set_option("extend_tree", 2)
    driver.reset_renderer(g)
    for _ in range(iters):
        driver.benchmark_iteration(g, W * H)
    return g


def adversarial(W, H, seed, moments=False):
    """random inputs with zero counts, NaN, +-inf, zero albedo and normals, unresolved accumulators; with moments also n < 2, n disagreeing
    with pixels.w, a non-finite sum of squares, an overflowing sum and zero variance.  -> (px, alb, nrm[, mom])"""
    if moments:
        import denoise_vg_reference as V
        px, alb, nrm, mom = V.random_inputs(W, H, seed)
    else:
        px, alb, nrm = random_inputs(W, H, seed)
    N = W * H
    rng = np.random.default_rng(seed + 100)
    k = max(1, N // 50)
    for col, vals in ((3, [0.0]), (0, [np.nan]), (1, [np.inf, -np.inf])):
        idx = rng.choice(N, k, replace=True)
        px[idx, col] = rng.choice(vals, k)
    alb[rng.choice(N, k), :3] = 0.0                      # zero albedo (floored)
    nrm[rng.choice(N, k), :4] = 0.0                      # zero normals
    alb[rng.choice(N, k), 3] = 0.0                       # unresolved accumulators (w <= 1: as is)
    if not moments:
        return px, alb, nrm
    mom[rng.choice(N, k), 3] = rng.choice([0.0, 1.0, 2.0, 9.0], k)      # n < 2 (fallback), n disagreeing with pixels.w
    mom[rng.choice(N, k), 1] = np.inf                                   # a non-finite sum of squares
    mom[rng.choice(N, k), 0] = 3e38
    mom[rng.choice(N, k), :2] = 0.0                                     # zero variance
    return px, alb, nrm, mom


def device_denoise(g, px, alb, nrm, mom=None, **kw):
    """write the inputs, run flx_denoise (or flx_denoise_variance_guided with mom) -> (which = 6, preview)"""
    g.write_pixels(0, px); g.write_pixels(4, alb); g.write_pixels(5, nrm)
    if mom is None:
        g.denoise(**kw)
    else:
        g.write_pixels(7, mom)
        assert same(g.read_pixels(7), mom)
        g.denoise_variance_guided(**kw)
    g.finish()
    return g.read_pixels(6), g.read_pixels(1)


def check_device_vs_cpu_adversarial(exe, d, W, H, K, blend, moments=False):
    g = ctx(d, W, H, moments=int(moments))
    ins = adversarial(W, H, W + H + K, moments)
    mom = ins[3] if moments else None
    out, prev = device_denoise(g, *ins[:3], mom=mom, iterations=K, blend=blend)
    cout, cprev = run_cpu(exe, *ins[:3], W, H, mom=mom, iterations=K, blend=blend, **tm(g.params))
    assert same(out, cout), int((out.view(np.uint32) != cout.view(np.uint32)).any(1).sum())
    assert same(prev, cprev)


def check_device_vs_cpu_sigmas(exe, d, sigmas, moments=False):
    """200 x 120, K = 5, for each (tmOperator, sigmas) of `sigmas` at exposure 1.7"""
    W, H = 200, 120
    for tmo, sig in sigmas:
        g = ctx(d, W, H, moments=int(moments), tmOperator=tmo, exposure=1.7)
        ins = adversarial(W, H, tmo, moments)
        mom = ins[3] if moments else None
        out, prev = device_denoise(g, *ins[:3], mom=mom, iterations=5, **sig)
        cout, cprev = run_cpu(exe, *ins[:3], W, H, mom=mom, iterations=5, **tm(g.params), **sig)
        assert same(out, cout) and same(prev, cprev), tmo


def check_device_vs_cpu_on_render(exe, kind, moments=False):
    """96 x 72 renders of the device itself: microkernel 4 spp and 10 wavefront iterations of mixed_material_scene under a sky, egyptcat
    2 spp; the default call and K = 8, blend 0.3.  The inputs are not touched."""
    import common
    from fluctus_amd import host
    W, H = 96, 72
    if kind == "microkernel":
        g = mk_render(common.mixed_material_scene(), W, H, 4, env=host.synthetic_sky(64, 32), moments=int(moments))
    elif kind == "wavefront":
        g = wf_render(common.mixed_material_scene(), W, H, 10, env=host.synthetic_sky(64, 32), moments=int(moments))
    else:
        g = mk_render(common.egyptcat_scene(), W, H, 2, moments=int(moments))
    px, alb, nrm = g.read_pixels(0), g.read_pixels(4), g.read_pixels(5)
    mom = g.read_pixels(7) if moments else None
    call = g.denoise_variance_guided if moments else g.denoise
    for kw in (dict(), dict(iterations=8, blend=0.3)):
        call(**kw); g.finish()
        cout, cprev = run_cpu(exe, px, alb, nrm, W, H, mom=mom, **kw, **tm(g.params))
        assert same(g.read_pixels(6), cout) and same(g.read_pixels(1), cprev), (kind, kw)
    assert same(g.read_pixels(0), px) and (mom is None or same(g.read_pixels(7), mom))


def tracer(W=64, H=48):
    """a Tracer on the procedural kitchen, extend_tree 2, 3 bounces"""
    from fluctus_amd import wire
    from fluctus_amd.tracer import Tracer
    t = Tracer(W, H, 0, 4096)
    t.set_option("extend_tree", 2)
    t.init(W, H, "proc:kitchen:3000:7")
    p = t.params
    wire.look_at(p, (0.0, 1.2, 2.6), (0.0, 0.2, 0.0))
    p["maxBounces"] = 3
    t.params = p
    return t
