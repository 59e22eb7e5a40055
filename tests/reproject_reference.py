"""flx_reproject restated in float64 from its definition, synthetic G-buffers, and the CPU counterpart's driver.

reference() is written from the definition's text, not from csrc/flx_reproject.h: per new pixel with a surface in the current G-buffer,
v = P - pos_prev, z = v . dir_prev (no history unless z > 0 and finite); screen coordinates v . right / z and v . up / z, divided by
tan(fov_prev / 2) (x also by the aspect W / H), through NDC to continuous pixel coordinates, minus the 0.5 of the pixel centre (the camera
frame is taken as orthonormal).  Four bilinear taps at floor(xf), floor(yf); a tap counts iff it is inside the image, its previous hit index
is >= 0, its history count is > 0 with finite rgb and count, |(P_tap - P) . N| <= plane_tolerance_px t 2 tan(fov_cur / 2) / H and
Ng_tap . N >= normal_cos.  Sum of the counted weights < min_weight: zeros.  Otherwise, weights renormalised: c = sum w rgb / n,
nbar = sum w n, n' = min(nbar, max_history), pixel (c n', n').  Moments: the same taps on (sum l / n_m, sum l^2 / n_m); a counted tap whose
n_m is <= 0 or whose sums are not finite is left out and the moments' weights renormalise over the rest (none left: zeros); output
(m1 n', m2 n', 0, n')."""
import os
import subprocess
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = dict(max_history=32.0, plane_tolerance_px=2.0, normal_cos=0.9, min_weight=0.01)
CAMERA = np.dtype([("pos", "<f4", 4), ("dir", "<f4", 4), ("up", "<f4", 4), ("right", "<f4", 4), ("fov", "<f4"), ("apertureSize", "<f4"),
                   ("focalDist", "<f4"), ("_pad", "<f4")])
assert CAMERA.itemsize == 80
# a tap whose bilinear weight is below this lies within rounding of floor()'s integer boundary at the sizes tested (|xf| < 2048: one ulp of xf is
# 1.2e-4 and it comes from ~6 operations): whether it is a tap at all is decided by rounding, and it carries no weight either way
WEIGHT_EPS = 1e-3


def camera(pos, target, fov=60.0, up=(0.0, 1.0, 0.0), focal=0.5):
    """an orthonormal camera record (float32 values, as the library receives them)"""
    pos = np.asarray(pos, np.float64)
    d = np.asarray(target, np.float64) - pos
    d /= np.linalg.norm(d)
    r = np.cross(d, np.asarray(up, np.float64)); r /= np.linalg.norm(r)
    u = np.cross(r, d)
    c = np.zeros((), CAMERA)
    c["pos"][:3], c["dir"][:3], c["up"][:3], c["right"][:3] = pos, d, u, r
    c["fov"], c["focalDist"] = fov, focal
    return c


def _cam64(c):
    return {k: np.asarray(c[k], np.float64)[:3] for k in ("pos", "dir", "up", "right")}, float(c["fov"])


def quad(centre, u, v, hu, hv):
    """a rectangle: centre, unit axes u and v, half extents"""
    return dict(c=np.asarray(centre, np.float64), u=np.asarray(u, np.float64), v=np.asarray(v, np.float64), hu=float(hu), hv=float(hv))


def synth_gbuffer(cam, W, H, surfaces):
    """(W*H, 8) float32 G-buffer of the surfaces (quad()s; index = position in the list) seen through the pixel centres, analytically in float64"""
    f, fov = _cam64(cam)
    x = (np.arange(W * H) % W + 0.5) / W * 2.0 - 1.0
    y = (np.arange(W * H) // W + 0.5) / H * 2.0 - 1.0
    s = np.tan(np.radians(fov) / 2.0)
    d = f["dir"][None] + f["right"][None] * (x * W / H * s)[:, None] + f["up"][None] * (y * s)[:, None]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    best = np.full(W * H, np.inf); idx = np.full(W * H, -1, np.int32); ng = np.zeros((W * H, 3))
    for i, q in enumerate(surfaces):
        n = np.cross(q["u"], q["v"])
        den = d @ n
        with np.errstate(all="ignore"):
            t = ((q["c"] - f["pos"]) @ n) / den
        p = f["pos"][None] + t[:, None] * d - q["c"][None]
        hit = (np.abs(den) > 1e-12) & (t > 1e-9) & (np.abs(p @ q["u"]) <= q["hu"]) & (np.abs(p @ q["v"]) <= q["hv"]) & (t < best)
        best[hit] = t[hit]; idx[hit] = i
        ng[hit] = np.where(den[hit, None] > 0, -n[None], n[None])
    g = np.zeros((W * H, 8), np.float32)
    h = idx >= 0
    g[h, :3] = (f["pos"][None] + best[h, None] * d[h])
    g[:, 3] = idx.view(np.float32)
    g[h, 4:7] = ng[h]
    g[:, 7] = np.where(h, best, -1.0)
    return g


def random_history(N, seed, moments=True, lo=1, hi=40):
    """(history, moments): counts in lo..hi, radiance sums, consistent luminance moments"""
    rng = np.random.default_rng(seed)
    n = rng.integers(lo, hi + 1, N).astype(np.float64)
    px = np.zeros((N, 4), np.float32)
    px[:, :3] = rng.uniform(0.5, 1.5, (N, 3)) * n[:, None]; px[:, 3] = n
    mom = np.zeros((N, 4), np.float32)
    m1 = rng.uniform(0.5, 1.5, N)
    mom[:, 0] = m1 * n; mom[:, 1] = (m1 * m1 + rng.uniform(0.0, 0.5, N)) * n; mom[:, 3] = n
    return px, (mom if moments else None)


def reference(W, H, cur, prev, cam_prev, fov_cur, hist, mom=None, **params):
    """float64 -> (pixels (N, 4), moments (N, 4), taps (N, 4) int64 previous-view pixel of each counted tap or -1, weights (N, 4))"""
    P_ = dict(DEFAULTS, **params)
    N = W * H
    f, fovp = _cam64(cam_prev)
    cur = np.asarray(cur, np.float32).reshape(N, 8); prev = np.asarray(prev, np.float32).reshape(N, 8)
    ci = cur[:, 3].copy().view(np.int32); pi = prev[:, 3].copy().view(np.int32)
    c64, p64 = cur.astype(np.float64), prev.astype(np.float64)
    h64 = np.asarray(hist, np.float32).reshape(N, 4).astype(np.float64)
    out = np.zeros((N, 4)); outm = np.zeros((N, 4)); taps = np.full((N, 4), -1, np.int64); wts = np.zeros((N, 4))
    with np.errstate(all="ignore"):
        P, Nn, t = c64[:, :3], c64[:, 4:7], c64[:, 7]
        v = P - f["pos"][None]
        z = v @ f["dir"]
        ok = (ci >= 0) & (z > 0) & np.isfinite(z)
        sp = np.tan(np.radians(fovp) / 2.0)
        xf = ((v @ f["right"]) / z / sp / (W / H) + 1.0) / 2.0 * W - 0.5
        yf = ((v @ f["up"]) / z / sp + 1.0) / 2.0 * H - 0.5
        ok &= np.isfinite(xf) & np.isfinite(yf)
        x0 = np.floor(np.where(ok, xf, 0.0)); y0 = np.floor(np.where(ok, yf, 0.0))
        fx, fy = xf - x0, yf - y0
        tol = P_["plane_tolerance_px"] * t * 2.0 * np.tan(np.radians(float(fov_cur)) / 2.0) / H
        cnt = np.zeros((N, 4), bool); b = np.zeros((N, 4)); J = np.zeros((N, 4), np.int64)
        for k in range(4):
            xj, yj = x0 + (k & 1), y0 + (k >> 1)
            ins = ok & (xj >= 0) & (xj < W) & (yj >= 0) & (yj < H)
            j = np.where(ins, yj * W + xj, 0).astype(np.int64)
            hj = h64[j]
            good = ins & (pi[j] >= 0) & (hj[:, 3] > 0) & np.isfinite(hj).all(1)
            good &= np.abs(((p64[j, :3] - P) * Nn).sum(1)) <= tol
            good &= (p64[j, 4:7] * Nn).sum(1) >= P_["normal_cos"]
            cnt[:, k] = good; J[:, k] = j
            b[:, k] = np.where(k & 1, fx, 1.0 - fx) * np.where(k >> 1, fy, 1.0 - fy)
        S = (b * cnt).sum(1)
        have = cnt.any(1) & (S >= P_["min_weight"])
        w = np.where(cnt & have[:, None], b / S[:, None], 0.0)
        hJ = h64[J]
        c = (w[:, :, None] * np.where(cnt[:, :, None], hJ[:, :, :3] / hJ[:, :, 3:4], 0.0)).sum(1)
        nbar = (w * np.where(cnt, hJ[:, :, 3], 0.0)).sum(1)
        n = np.minimum(nbar, P_["max_history"])
        out[have, :3] = (c * n[:, None])[have]; out[have, 3] = n[have]
        taps[cnt & have[:, None]] = J[cnt & have[:, None]]
        wts = np.where(cnt & have[:, None], b, 0.0)
        if mom is not None:
            m64 = np.asarray(mom, np.float32).reshape(N, 4).astype(np.float64)[J]
            mc = cnt & have[:, None] & (m64[:, :, 3] > 0) & np.isfinite(m64[:, :, 3]) & np.isfinite(m64[:, :, 0]) & np.isfinite(m64[:, :, 1])
            Sm = (b * mc).sum(1)
            hm = mc.any(1) & (Sm > 0)
            wm = np.where(mc & hm[:, None], b / Sm[:, None], 0.0)
            m1 = (wm * np.where(mc, m64[:, :, 0] / m64[:, :, 3], 0.0)).sum(1)
            m2 = (wm * np.where(mc, m64[:, :, 1] / m64[:, :, 3], 0.0)).sum(1)
            outm[hm, 0] = (m1 * n)[hm]; outm[hm, 1] = (m2 * n)[hm]; outm[hm, 3] = n[hm]
    return out, outm, taps, wts


def build_cpu(outdir):
    """g++ -O2 -ffp-contract=off tests/reproject_cpu.cpp -> <outdir>/reproject_cpu.  A failed compile raises."""
    exe = os.path.join(str(outdir), "reproject_cpu")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "reproject_cpu.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, "reproject_cpu.cpp does not compile:\n" + r.stdout
    return exe


def run_cpu(exe, W, H, cur, prev, cam_prev, fov_cur, hist, mom=None, **params):
    """the counterpart -> (pixels, moments, taps int32 (N, 4), weights (N, 4)), float32"""
    P_ = dict(DEFAULTS, **params)
    d = os.path.dirname(exe)
    fin, fout = os.path.join(d, "rp_in.bin"), os.path.join(d, "rp_out.bin")
    N = W * H
    with open(fin, "wb") as f:
        f.write(np.array([W, H, int(mom is not None)], np.int32).tobytes())
        f.write(np.array([P_["max_history"], P_["plane_tolerance_px"], P_["normal_cos"], P_["min_weight"]], np.float32).tobytes())
        f.write(np.asarray(cam_prev).tobytes()[:80])
        f.write(np.array([fov_cur], np.float32).tobytes())
        for a, k in ((cur, 8), (prev, 8), (hist, 4)) + (((mom, 4),) if mom is not None else ()):
            a = np.ascontiguousarray(a, np.float32).reshape(-1, k)
            assert a.shape[0] == N
            f.write(a.tobytes())
    r = subprocess.run([exe, "reproject", fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    raw = np.fromfile(fout, np.float32)
    px, mo = raw[:N * 4].reshape(N, 4).copy(), raw[N * 4:N * 8].reshape(N, 4).copy()
    taps = raw[N * 8:N * 12].view(np.int32).reshape(N, 4).copy()
    return px, mo, taps, raw[N * 12:].reshape(N, 4).copy()


def centre_rays(exe, W, H, cam):
    """(W*H, 3) float32 directions of the un-jittered pixel-centre rays, bit for bit what flx_gbuffer traces (origin: cam["pos"])"""
    d = os.path.dirname(exe)
    fin, fout = os.path.join(d, "rays_in.bin"), os.path.join(d, "rays_out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([W, H], np.int32).tobytes())
        f.write(np.asarray(cam).tobytes()[:80])
    r = subprocess.run([exe, "rays", fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return np.fromfile(fout, np.float32).reshape(W * H, 3)


def tap_sets(taps, wts):
    """per pixel, the sorted tuple of counted taps that carry weight (WEIGHT_EPS), for the agreement check"""
    sig = (np.asarray(taps) >= 0) & (np.asarray(wts) > WEIGHT_EPS)
    t = np.where(sig, taps, -1).astype(np.int64)
    return np.sort(t, axis=1)


def compare(cpu, ref, rtol=1e-4, atol=1e-6):
    """cpu, ref = (pixels, moments, taps, weights).  -> (worst error in tolerance units over the agreeing pixels, share of pixels excluded because
    the two disagree on the counted taps, number of agreeing pixels).  c, n' and the moments are compared (c = rgb / n')."""
    agree = (tap_sets(cpu[2], cpu[3]) == tap_sets(ref[2], ref[3])).all(1)
    def cols(px, mo):
        px, mo = np.asarray(px, np.float64), np.asarray(mo, np.float64)
        with np.errstate(all="ignore"):
            c = np.where(px[:, 3:4] > 0, px[:, :3] / px[:, 3:4], 0.0)
        return np.concatenate([c, px[:, 3:4], mo], 1)
    a, b = cols(cpu[0], cpu[1])[agree], cols(ref[0], ref[1])[agree]
    worst = float((np.abs(a - b) / (rtol * np.abs(b) + atol)).max()) if a.size else 0.0
    return worst, float(1.0 - agree.mean()), int(agree.sum())


def same(a, b):
    """bit for bit"""
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))
