"""The stopping rule of the adaptive microkernel render (fluctus_amd/csrc/flx_adaptive.h) restated in float64 with numpy, the
driver of its CPU counterpart (tests/adaptive_cpu.cpp), and the adaptive render SIMULATED from a stack of per-sample images: the integrator is
deterministic per pixel, so the n-th sample of a pixel is the same whatever the other pixels do, and the whole adaptive run is a pure function of
the stack."""
import os
import subprocess
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = dict(threshold=0.05, min_samples=4, max_samples=32, lum_floor=0.01, dilate=1)
OWN, ACTIVE, DONE, CONVERGED = 1, 2, 4, 8
FLT_MAX = float(np.finfo(np.float32).max)
R_RTOL, R_ATOL = 1e-5, 1e-7          # the counterpart's r against float64


def build_cpu(outdir, source=None):
    """g++ -O2 -ffp-contract=off tests/adaptive_cpu.cpp -> <outdir>/adaptive_cpu.  A failed compile raises."""
    exe = os.path.join(str(outdir), "adaptive_cpu")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", source or os.path.join(ROOT, "tests", "adaptive_cpu.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, "adaptive_cpu.cpp does not compile:\n" + r.stdout
    return exe


def run_cpu(exe, W, H, mom, **params):
    """the counterpart -> (flags uint8 (N,), r float32 (N,), list uint32 (count,))"""
    P = dict(DEFAULTS, **params)
    d = os.path.dirname(exe)
    fin, fout = os.path.join(d, "ad_in.bin"), os.path.join(d, "ad_out.bin")
    N = W * H
    mom = np.ascontiguousarray(mom, np.float32).reshape(-1, 4)
    assert mom.shape[0] == N
    with open(fin, "wb") as f:
        f.write(np.array([W, H], np.int32).tobytes())
        f.write(np.array([P["threshold"]], np.float32).tobytes())
        f.write(np.array([P["min_samples"], P["max_samples"]], np.uint32).tobytes())
        f.write(np.array([P["lum_floor"]], np.float32).tobytes())
        f.write(np.array([P["dilate"]], np.uint32).tobytes())
        f.write(mom.tobytes())
    r = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    raw = np.fromfile(fout, np.uint8)
    flags = raw[:N].copy()
    rr = raw[N:5 * N].view(np.float32).copy()
    count = int(raw[5 * N:5 * N + 4].view(np.uint32)[0])
    lst = raw[5 * N + 4:].view(np.uint32).copy()
    assert lst.size == count
    return flags, rr, lst


def rel_error64(mom, lum_floor):
    """(r, exists) in float64 from float32 moments; r = inf where it does not exist"""
    m = np.asarray(mom, np.float32).reshape(-1, 4).astype(np.float64)
    s1, s2, n = m[:, 0], m[:, 1], m[:, 3]
    ok = np.isfinite(s1) & np.isfinite(s2) & np.isfinite(n) & (n > 0)
    with np.errstate(all="ignore"):
        mu = s1 / n
        m2 = s2 / n
        ok &= (np.abs(mu) <= FLT_MAX) & (np.abs(m2) <= FLT_MAX) & (mu * mu <= FLT_MAX)      # the float32 rule's finiteness tests
        den = mu + float(np.float32(lum_floor))
        ok &= den > 0
        v = np.maximum(m2 - mu * mu, 0.0) / n
        r = np.sqrt(v) / den
    ok &= ~np.isnan(r)
    return np.where(ok, r, np.inf), ok


def reference(W, H, mom, **params):
    """float64 restatement -> (flags, r64, list, near): `near` marks the pixels whose r is within the tolerance of the threshold -- their own
    flags, and through the dilation their neighbours', may legitimately differ from a float32 evaluation"""
    P = dict(DEFAULTS, **params)
    thr = float(np.float32(P["threshold"]))
    m = np.asarray(mom, np.float32).reshape(-1, 4)
    n = m[:, 3].astype(np.float64)
    r, ok = rel_error64(m, P["lum_floor"])
    done = n >= P["max_samples"]                      # NaN: False
    conv = ok & (n >= P["min_samples"]) & (n >= 2) & (r <= thr)
    own = ~done & ~conv
    near = ok & (np.abs(r - thr) <= R_RTOL * np.abs(r) + R_ATOL) & (n >= P["min_samples"]) & (n >= 2) & ~done
    act = own.copy()
    nearAct = near.copy()
    if P["dilate"]:
        o2 = np.pad(own.reshape(H, W), 1)
        n2 = np.pad(near.reshape(H, W), 1)
        anyOwn = np.zeros((H, W), bool)
        anyNear = np.zeros((H, W), bool)
        for dy in range(3):
            for dx in range(3):
                anyOwn |= o2[dy:dy + H, dx:dx + W]
                anyNear |= n2[dy:dy + H, dx:dx + W]
        act = ~done & (own | anyOwn.reshape(-1))
        nearAct = anyNear.reshape(-1)
    flags = (own * OWN + act * ACTIVE + done * DONE + conv * CONVERGED).astype(np.uint8)
    return flags, r, np.flatnonzero(act).astype(np.uint32), near, nearAct


def compare(cpu, ref, max_excluded=0.005):
    """counterpart (flags, r, list) against reference(...): r within the tolerance wherever both have one; own / done / converged equal outside
    `near`, active and the list equal outside the dilated `near`.  -> (worst r error in units of the tolerance, share of pixels left out)"""
    cf, cr, cl = cpu
    rf, rr, rl, near, nearAct = ref
    have = np.isfinite(rr)
    assert not (have ^ (cr < np.float32(FLT_MAX)))[~near].any(), "the two sides disagree on where r exists"
    both = have & (cr < np.float32(FLT_MAX))
    err = np.abs(cr[both].astype(np.float64) - rr[both]) / (R_RTOL * np.abs(rr[both]) + R_ATOL)
    worst = float(err.max()) if err.size else 0.0
    own_bits = OWN | DONE | CONVERGED
    assert np.array_equal((cf & own_bits)[~near], (rf & own_bits)[~near]), "own / done / converged differ away from the threshold"
    assert np.array_equal((cf & ACTIVE)[~nearAct], (rf & ACTIVE)[~nearAct]), "active differs away from the threshold"
    # the list: ascending, exactly the counterpart's active pixels, and equal to the reference's outside the excluded pixels
    assert np.array_equal(cl, np.flatnonzero(cf & ACTIVE).astype(np.uint32)), "the list is not the ascending list of the active pixels"
    keep = ~nearAct
    assert np.array_equal(cl[keep[cl]], rl[keep[rl]]), "the lists differ away from the threshold"
    share = float(nearAct.mean())
    assert share <= max_excluded, f"{100 * share:.3f} % of the pixels are within the tolerance of the threshold (cap {100 * max_excluded} %)"
    return worst, share


def lum32(rgb):
    """flx_lum in float32, in the header's order (no FMA): what the integrators splat"""
    rgb = np.asarray(rgb, np.float32)
    return (np.float32(0.2126) * rgb[..., 0] + np.float32(0.7152) * rgb[..., 1]) + np.float32(0.0722) * rgb[..., 2]


def per_sample_stack(ctx, params, S, keep=True):
    """S uniform microkernel passes on `ctx` (the oracle or the device; scene and environment uploaded): the radiance every pass splats, read from
    the path state just before the splat (roulette off: every path has terminated by then), and the accumulation after every pass.
    -> (samples (S, N, 3), accumulations (S, N, 4)) float32; keep=False: (None, the last accumulation)"""
    from fluctus_amd.wire import COL
    p = params.copy()
    p["useRoulette"] = 0
    ctx.set_params(p)
    ctx.mk_reset()
    N = int(p["width"]) * int(p["height"])
    smp, acc = (np.zeros((S, N, 3), np.float32), np.zeros((S, N, 4), np.float32)) if keep else (None, None)
    for s in range(S):
        ctx.mk_raygen()
        for _ in range(int(p["maxBounces"]) + 1):
            ctx.mk_next_vertex()
            ctx.mk_sample_bsdf()
        if keep:
            smp[s] = ctx.state_export()[COL.EI:COL.EI + 3, :N].T
        ctx.mk_splat()
        if keep:
            acc[s] = ctx.read_pixels(0)
    ctx.finish()
    return (smp, acc) if keep else (None, ctx.read_pixels(0))


def simulate(exe, W, H, samples, min_spp, max_spp, classify=None, **params):
    """The adaptive render from per-sample radiance `samples` (S >= max_spp, N, 3) float32: sample k of pixel p is samples[k, p] whenever it is
    taken -- exactly what the device does (float32 sums in sample order, flx_mk_splat's arithmetic).
    -> (pixels (N, 4), moments (N, 4), history: list of (active count, list) per pass)"""
    N = W * H
    samples = np.asarray(samples, np.float32)
    px, mom = np.zeros((N, 4), np.float32), np.zeros((N, 4), np.float32)
    taken = np.zeros(N, np.int64)
    hist = []
    for s in range(max_spp):
        if s >= min_spp:
            if classify is not None:
                lst = classify(mom)
            else:
                lst = run_cpu(exe, W, H, mom, min_samples=min_spp, max_samples=max_spp, **params)[2]
            if lst.size == 0:
                break
        else:
            lst = np.arange(N, dtype=np.uint32)
        e = samples[taken[lst], lst]
        l = lum32(e)
        px[lst, :3] += e
        px[lst, 3] += np.float32(1)
        mom[lst, 0] += l
        mom[lst, 1] += l * l
        mom[lst, 3] += np.float32(1)
        taken[lst] += 1
        hist.append((int(lst.size), lst))
    return px, mom, hist


def quality(px, truth, lum_floor=0.01):
    """(the metric the stopping rule controls: mean of (x - truth)^2 / (truth + lum_floor)^2 on luminance, plain RMSE on luminance), float64"""
    x = lum32(px[:, :3] / np.maximum(px[:, 3:4], 1)).astype(np.float64)
    t = lum32(truth[:, :3] / np.maximum(truth[:, 3:4], 1)).astype(np.float64)
    return float(np.mean((x - t) ** 2 / (t + lum_floor) ** 2)), float(np.sqrt(np.mean((x - t) ** 2)))
