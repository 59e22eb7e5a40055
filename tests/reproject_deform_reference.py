"""flx_reproject with option "deform_history"  restated in float64 from its definition, analytic G-buffers of triangles with
their barycentrics, and the CPU counterpart's driver (tests/reproject_deform_cpu.cpp).

reference() is written from the definition's text, not from csrc/flx_reproject_deform.h.  moved(i): any of triangle i's nine position words now
differs bitwise from the word at the capture.  Per new pixel with a surface (hit index i >= 0) and barycentric record (u, v): the record names no
triangle when it is (-1, -1) or i is not below the triangle count, and such a pixel is unmoved; unmoved: P' = P, N' = N; moved:
P' = (1 - u - v) q0 + u q1 + v q2 over the positions at the capture, N' = s (q1 - q0) x (q2 - q0) / |.|, s = -1 when the unit normal of the
triangle now, (p1 - p0) x (p2 - p0) / |.|, has a negative dot product with N, else +1.  Then reproject_reference's text with P', N' for P, N and
one more condition on a tap: the tap's own record (its hit index in the previous G-buffer, its barycentric record) is moved exactly when the pixel
is."""
import os
import subprocess
import numpy as np
import reproject_reference as R

ROOT = R.ROOT
NO_BARY = -1.0


def tri_quad(centre, u, v, hu, hv):
    """a rectangle as two triangles (2, 3, 3) float64: (c - u - v, c + u - v, c + u + v), (c - u - v, c + u + v, c - u + v); normal u x v"""
    c, u, v = np.asarray(centre, np.float64), np.asarray(u, np.float64) * hu, np.asarray(v, np.float64) * hv
    a, b, d, e = c - u - v, c + u - v, c + u + v, c - u + v
    return np.array([[a, b, d], [a, d, e]])


def synth(cam, W, H, tris):
    """the triangles (n, 3, 3) seen through the pixel centres, analytically in float64 -> ((W*H, 8) float32 G-buffer, (W*H, 2) float32 barycentrics:
    (-1, -1) on a miss).  Both sides of a triangle are seen; the normal faces the camera.  A degenerate triangle is never hit."""
    tris = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    f, fov = R._cam64(cam)
    x = (np.arange(W * H) % W + 0.5) / W * 2.0 - 1.0
    y = (np.arange(W * H) // W + 0.5) / H * 2.0 - 1.0
    s = np.tan(np.radians(fov) / 2.0)
    d = f["dir"][None] + f["right"][None] * (x * W / H * s)[:, None] + f["up"][None] * (y * s)[:, None]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    N = W * H
    best = np.full(N, np.inf); idx = np.full(N, -1, np.int32); ng = np.zeros((N, 3)); uv = np.full((N, 2), NO_BARY)
    for i, (p0, p1, p2) in enumerate(tris):
        e1, e2 = p1 - p0, p2 - p0
        n = np.cross(e1, e2)
        if not n.any():
            continue
        with np.errstate(all="ignore"):
            pv = np.cross(d, e2[None])
            det = pv @ e1
            tv = f["pos"] - p0
            u = (pv @ tv) / det
            qv = np.cross(tv, e1)
            v = (d @ qv) / det
            t = (qv @ e2) / det
        hit = (np.abs(det) > 1e-14) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 1e-9) & (t < best)
        best[hit] = t[hit]; idx[hit] = i
        nn = n / np.linalg.norm(n)
        ng[hit] = np.where((d[hit] @ nn)[:, None] > 0, -nn[None], nn[None])
        uv[hit, 0] = u[hit]; uv[hit, 1] = v[hit]
    g = np.zeros((N, 8), np.float32)
    h = idx >= 0
    g[h, :3] = f["pos"][None] + best[h, None] * d[h]
    g[:, 3] = idx.view(np.float32)
    g[h, 4:7] = ng[h]
    g[:, 7] = np.where(h, best, -1.0)
    return g, uv.astype(np.float32)


def moved_flags(now, cap):
    a, b = np.ascontiguousarray(now, np.float32).reshape(-1, 9), np.ascontiguousarray(cap, np.float32).reshape(-1, 9)
    return (a.view(np.uint32) != b.view(np.uint32)).any(1)


def reference(W, H, cur, prev, cam_prev, fov_cur, hist, mom, cur_bary, prev_bary, now, cap, **params):
    """float64 -> (pixels (N, 4), moments (N, 4), taps (N, 4) int64 or -1, weights (N, 4)).  now / cap: (ntris, 3, 3) float32"""
    P_ = dict(R.DEFAULTS, **params)
    N = W * H
    f, fovp = R._cam64(cam_prev)
    now32, cap32 = np.ascontiguousarray(now, np.float32).reshape(-1, 3, 3), np.ascontiguousarray(cap, np.float32).reshape(-1, 3, 3)
    ntris = now32.shape[0]
    mvtri = np.concatenate([moved_flags(now32, cap32), [False]])          # the last: no triangle
    p64, q64 = np.concatenate([now32.astype(np.float64), np.zeros((1, 3, 3))]), np.concatenate([cap32.astype(np.float64), np.zeros((1, 3, 3))])
    cur = np.asarray(cur, np.float32).reshape(N, 8); prev = np.asarray(prev, np.float32).reshape(N, 8)
    ci = cur[:, 3].copy().view(np.int32); pi = prev[:, 3].copy().view(np.int32)
    cb, pb = np.asarray(cur_bary, np.float32).reshape(N, 2), np.asarray(prev_bary, np.float32).reshape(N, 2)
    def tri_of(i, b):
        none = ((b[:, 0] == NO_BARY) & (b[:, 1] == NO_BARY)) | (i < 0) | (i >= ntris)
        return np.where(none, ntris, i).astype(np.int64)
    ct, pt = tri_of(ci, cb), tri_of(pi, pb)
    mv, mvprev = mvtri[ct], mvtri[pt]
    c64, pv64 = cur.astype(np.float64), prev.astype(np.float64)
    h64 = np.asarray(hist, np.float32).reshape(N, 4).astype(np.float64)
    out = np.zeros((N, 4)); outm = np.zeros((N, 4)); taps = np.full((N, 4), -1, np.int64)
    with np.errstate(all="ignore"):
        P, Nn, t = c64[:, :3].copy(), c64[:, 4:7].copy(), c64[:, 7]
        u, v = cb[:, 0].astype(np.float64)[:, None], cb[:, 1].astype(np.float64)[:, None]
        q, p = q64[ct], p64[ct]
        Pm = (1.0 - u - v) * q[:, 0] + u * q[:, 1] + v * q[:, 2]
        nnow = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        nnow = nnow / np.sqrt((nnow * nnow).sum(1))[:, None]
        sgn = np.where((nnow * Nn).sum(1) < 0, -1.0, 1.0)[:, None]
        ncap = np.cross(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0])
        Nm = sgn * ncap / np.sqrt((ncap * ncap).sum(1))[:, None]
        P[mv] = Pm[mv]; Nn[mv] = Nm[mv]
        w_ = P - f["pos"][None]
        z = w_ @ f["dir"]
        ok = (ci >= 0) & (z > 0) & np.isfinite(z)
        sp = np.tan(np.radians(fovp) / 2.0)
        xf = ((w_ @ f["right"]) / z / sp / (W / H) + 1.0) / 2.0 * W - 0.5
        yf = ((w_ @ f["up"]) / z / sp + 1.0) / 2.0 * H - 0.5
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
            good &= mvprev[j] == mv
            good &= np.abs(((pv64[j, :3] - P) * Nn).sum(1)) <= tol
            good &= (pv64[j, 4:7] * Nn).sum(1) >= P_["normal_cos"]
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


def build_cpu(outdir, sanitize=False):
    """g++ -O2 -ffp-contract=off tests/reproject_deform_cpu.cpp -> <outdir>/reproject_deform_cpu.  A failed compile raises."""
    exe = os.path.join(str(outdir), "reproject_deform_cpu")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off"] + (["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []) + \
          [os.path.join(ROOT, "tests", "reproject_deform_cpu.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, "reproject_deform_cpu.cpp does not compile:\n" + r.stdout
    return exe


def run_cpu(exe, W, H, cur, prev, cam_prev, fov_cur, hist, mom, cur_bary, prev_bary, now, cap, **params):
    """the counterpart -> (pixels, moments, taps int32 (N, 4), weights (N, 4)) float32, moved (ntris,) bool"""
    P_ = dict(R.DEFAULTS, **params)
    d = os.path.dirname(exe)
    fin, fout = os.path.join(d, "rd_in.bin"), os.path.join(d, "rd_out.bin")
    N = W * H
    now, cap = np.ascontiguousarray(now, np.float32).reshape(-1, 9), np.ascontiguousarray(cap, np.float32).reshape(-1, 9)
    assert now.shape == cap.shape
    with open(fin, "wb") as f:
        f.write(np.array([W, H, int(mom is not None), now.shape[0]], np.int32).tobytes())
        f.write(np.array([P_["max_history"], P_["plane_tolerance_px"], P_["normal_cos"], P_["min_weight"]], np.float32).tobytes())
        f.write(np.asarray(cam_prev).tobytes()[:80])
        f.write(np.array([fov_cur], np.float32).tobytes())
        for a, k in ((cur, 8), (prev, 8), (hist, 4)) + (((mom, 4),) if mom is not None else ()) + ((cur_bary, 2), (prev_bary, 2)):
            a = np.ascontiguousarray(a, np.float32).reshape(-1, k)
            assert a.shape[0] == N
            f.write(a.tobytes())
        f.write(now.tobytes()); f.write(cap.tobytes())
    r = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    raw = np.fromfile(fout, np.float32)
    px, mo = raw[:N * 4].reshape(N, 4).copy(), raw[N * 4:N * 8].reshape(N, 4).copy()
    taps = raw[N * 8:N * 12].view(np.int32).reshape(N, 4).copy()
    return (px, mo, taps, raw[N * 12:N * 16].reshape(N, 4).copy()), raw[N * 16:].view(np.int32).astype(bool)
