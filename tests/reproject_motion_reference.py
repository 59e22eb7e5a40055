"""flx_reproject with option "motion_history"  restated in float64 from its definition, posed analytic surfaces, and the CPU
counterpart's driver (tests/reproject_motion_cpu.cpp).

reference() is written from the definition's text, not from csrc/flx_reproject_motion.h.  It takes the fp32 per-object table as input, so the
rounding of the inverse is not part of the comparison.  Per new pixel with a surface and object id o (>= nobjects reads as NO_OBJECT):
no object or moved[o] == 0: P' = P, N' = N; no_history[o]: zeros; otherwise P' = D P (affine), N' = s cof(D) N / |.|, s = -1 unless det > 0.
Then reproject_reference's text with P', N' for P, N and one more condition on a tap: its object id o_j equals o, or neither o nor o_j moved."""
import os
import subprocess
import numpy as np
import reproject_reference as R

ROOT = R.ROOT
NO_OBJECT = 0xFFFFFFFF
IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)


def translate(x, y=0.0, z=0.0):
    X = IDENTITY.copy(); X[:, 3] = (x, y, z)
    return X


def rotate(axis, degrees, about=(0.0, 0.0, 0.0)):
    """rotation about the line through `about` along `axis`, as a float32 3 x 4 matrix"""
    a = np.asarray(axis, np.float64); a /= np.linalg.norm(a)
    th = np.radians(degrees)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    M = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    c = np.asarray(about, np.float64)
    return np.concatenate([M, (c - M @ c)[:, None]], 1).astype(np.float32)


def scale(sx, sy, sz, about=(0.0, 0.0, 0.0)):
    M = np.diag([sx, sy, sz]).astype(np.float64)
    c = np.asarray(about, np.float64)
    return np.concatenate([M, (c - M @ c)[:, None]], 1).astype(np.float32)


def posed(q, X):
    """the quad q under the 3 x 4 transform X (float64 arithmetic on the float32 entries).  X's linear part must keep u and v orthogonal
    (a rotation, a mirror, a scale along the quad's own axes)."""
    X = np.asarray(X, np.float32).astype(np.float64).reshape(3, 4)
    M, t = X[:, :3], X[:, 3]
    u, v = M @ q["u"], M @ q["v"]
    lu, lv = np.linalg.norm(u), np.linalg.norm(v)
    assert abs(u @ v) < 1e-9 * lu * lv
    return R.quad(M @ q["c"] + t, u / lu, v / lv, q["hu"] * lu, q["hv"] * lv)


def object_plane(g, object_of_surface):
    """the object id of every pixel of a synthetic G-buffer: object_of_surface[hit index], NO_OBJECT on a miss"""
    idx = np.asarray(g, np.float32).reshape(-1, 8)[:, 3].copy().view(np.int32)
    m = np.asarray(object_of_surface, np.uint32)
    return np.where(idx >= 0, m[np.maximum(idx, 0)], np.uint32(NO_OBJECT)).astype(np.uint32)


def reference(W, H, cur, prev, cam_prev, fov_cur, hist, mom, cur_obj, prev_obj, table, **params):
    """float64 -> (pixels (N, 4), moments (N, 4), taps (N, 4) int64 or -1, weights (N, 4)).  table: (nobjects, 4, 4) float32"""
    P_ = dict(R.DEFAULTS, **params)
    N = W * H
    f, fovp = R._cam64(cam_prev)
    table = np.asarray(table, np.float32).reshape(-1, 4, 4).astype(np.float64)
    nobj = table.shape[0]
    tab = np.concatenate([table, np.zeros((1, 4, 4))])                  # the last row: NO_OBJECT (never moved, D unused)
    tab[nobj, :3, :3] = np.eye(3)
    def ids(o):
        o = np.asarray(o, np.uint32).astype(np.int64)
        return np.where(o < nobj, o, nobj)
    o, oprev = ids(cur_obj), ids(prev_obj)
    moved, nohist = tab[:, 3, 0] != 0, tab[:, 3, 1] != 0
    cur = np.asarray(cur, np.float32).reshape(N, 8); prev = np.asarray(prev, np.float32).reshape(N, 8)
    ci = cur[:, 3].copy().view(np.int32); pi = prev[:, 3].copy().view(np.int32)
    c64, p64 = cur.astype(np.float64), prev.astype(np.float64)
    h64 = np.asarray(hist, np.float32).reshape(N, 4).astype(np.float64)
    out = np.zeros((N, 4)); outm = np.zeros((N, 4)); taps = np.full((N, 4), -1, np.int64)
    with np.errstate(all="ignore"):
        P, Nn, t = c64[:, :3].copy(), c64[:, 4:7].copy(), c64[:, 7]
        mv = moved[o] & ~nohist[o]
        D = tab[o]
        Pm = np.einsum("nij,nj->ni", D[:, :3, :3], P) + D[:, :3, 3]
        M = D[:, :3, :3]
        cof = np.stack([np.cross(M[:, 1], M[:, 2]), np.cross(M[:, 2], M[:, 0]), np.cross(M[:, 0], M[:, 1])], 1)
        det = (M[:, 0] * cof[:, 0]).sum(1)
        u = np.einsum("nij,nj->ni", cof, Nn) * np.where(det > 0, 1.0, -1.0)[:, None]
        Nm = u / np.sqrt((u * u).sum(1))[:, None]
        P[mv] = Pm[mv]; Nn[mv] = Nm[mv]
        v = P - f["pos"][None]
        z = v @ f["dir"]
        ok = (ci >= 0) & ~nohist[o] & (z > 0) & np.isfinite(z)
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
            good &= (oprev[j] == o) | ~(moved[o] | moved[oprev[j]])
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
    """g++ -O2 -ffp-contract=off tests/reproject_motion_cpu.cpp -> <outdir>/reproject_motion_cpu.  A failed compile raises."""
    exe = os.path.join(str(outdir), "reproject_motion_cpu")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "reproject_motion_cpu.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, "reproject_motion_cpu.cpp does not compile:\n" + r.stdout
    return exe


def make_table(exe, x_cap, known_cap, x_now, known_now):
    """the header's rm_make_table -> ((nobjects, 4, 4) float32, any)"""
    xc, xn = np.ascontiguousarray(x_cap, np.float32).reshape(-1, 12), np.ascontiguousarray(x_now, np.float32).reshape(-1, 12)
    n = xc.shape[0]
    assert xn.shape[0] == n and len(known_cap) == n and len(known_now) == n
    d = os.path.dirname(exe)
    fin, fout = os.path.join(d, "rm_tab_in.bin"), os.path.join(d, "rm_tab_out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([n], np.int32).tobytes())
        f.write(xc.tobytes()); f.write(np.asarray(known_cap, np.int32).tobytes())
        f.write(xn.tobytes()); f.write(np.asarray(known_now, np.int32).tobytes())
    r = subprocess.run([exe, "table", fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    raw = np.fromfile(fout, np.float32)
    return raw[:n * 16].reshape(n, 4, 4).copy(), bool(raw[n * 16:].view(np.int32)[0])


def run_cpu(exe, W, H, cur, prev, cam_prev, fov_cur, hist, mom, cur_obj, prev_obj, table, **params):
    """the counterpart -> (pixels, moments, taps int32 (N, 4), weights (N, 4)), float32"""
    P_ = dict(R.DEFAULTS, **params)
    d = os.path.dirname(exe)
    fin, fout = os.path.join(d, "rm_in.bin"), os.path.join(d, "rm_out.bin")
    N = W * H
    table = np.ascontiguousarray(table, np.float32).reshape(-1, 16)
    with open(fin, "wb") as f:
        f.write(np.array([W, H, int(mom is not None), table.shape[0]], np.int32).tobytes())
        f.write(np.array([P_["max_history"], P_["plane_tolerance_px"], P_["normal_cos"], P_["min_weight"]], np.float32).tobytes())
        f.write(np.asarray(cam_prev).tobytes()[:80])
        f.write(np.array([fov_cur], np.float32).tobytes())
        for a, k in ((cur, 8), (prev, 8), (hist, 4)) + (((mom, 4),) if mom is not None else ()):
            a = np.ascontiguousarray(a, np.float32).reshape(-1, k)
            assert a.shape[0] == N
            f.write(a.tobytes())
        for o in (cur_obj, prev_obj):
            o = np.ascontiguousarray(o, np.uint32)
            assert o.size == N
            f.write(o.tobytes())
        f.write(table.tobytes())
    r = subprocess.run([exe, "reproject", fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    raw = np.fromfile(fout, np.float32)
    px, mo = raw[:N * 4].reshape(N, 4).copy(), raw[N * 4:N * 8].reshape(N, 4).copy()
    taps = raw[N * 8:N * 12].view(np.int32).reshape(N, 4).copy()
    return px, mo, taps, raw[N * 12:].reshape(N, 4).copy()
