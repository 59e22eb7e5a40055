"""flx_history_rectify restated in float64 from its definition, and the CPU counterpart's driver.

reference() is written from the definition's text, not from csrc/flx_rectify.h.  Per pixel q, from the accumulation A = (rgb sum, count), its
marked copy S and the current G-buffer (G0 = (P, hit index), G1 = (N, t)), with lum = 0.2126 r + 0.7152 g + 0.0722 b:
n = A.w - S.w, a = lum(A.rgb - S.rgb) / n, h = lum(S.rgb) / S.w, x = a - h; q is usable iff its hit index is >= 0, S.w > 0, n >= 0.5 and all
of these are finite.  Per centre p with a surface, S.w > 0 and finite A and S: the taps are the usable pixels of the (2 r + 1)^2 window inside
the image with |(P_q - P_p) . N_p| <= plane_tolerance_px t_p 2 tan(fov / 2) / H and N_q . N_p >= normal_cos; over them N = their number,
K = sum n, d = sum n x / K, v = max(0, sum n x^2 / K - d^2), se = sqrt(v / N), e = max(0, |d| - gamma se),
lambda = min(1, sensitivity e / (max(sum n a / K, sum n h / K) + lum_floor)); N < min_pixels: 0.  Where lambda > 0: A' = A - lambda S,
S' = S (1 - lambda), and the same for the moments (M, SM) when both exist."""
import os
import subprocess
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = dict(radius=3, gamma=3.0, sensitivity=2.0, lum_floor=0.01, min_pixels=8, plane_tolerance_px=2.0, normal_cos=0.9)
LUM = np.array([0.2126, 0.7152, 0.0722])


def reference(W, H, cur, A, S, fov, M=None, SM=None, **params):
    """float64 -> dict(A, S, M, SM (None where absent), lam (N,), counted (N,) int, taps (N,) uint32 checksum as tests/rectify_cpu.cpp,
    margin (N,): |d| - gamma se where the window was evaluated, nan elsewhere)"""
    P_ = dict(DEFAULTS, **params)
    r, N = int(P_["radius"]), W * H
    cur = np.asarray(cur, np.float32).reshape(N, 8)
    hit = (cur[:, 3].copy().view(np.int32) >= 0).reshape(H, W)
    c64 = cur.astype(np.float64).reshape(H, W, 8)
    A64 = np.asarray(A, np.float32).reshape(N, 4).astype(np.float64).reshape(H, W, 4)
    S64 = np.asarray(S, np.float32).reshape(N, 4).astype(np.float64).reshape(H, W, 4)
    with np.errstate(all="ignore"):
        n = A64[..., 3] - S64[..., 3]
        a = ((A64[..., :3] - S64[..., :3]) @ LUM) / n
        h = (S64[..., :3] @ LUM) / S64[..., 3]
        x = a - h
        ok = hit & (S64[..., 3] > 0) & (n >= 0.5) & np.isfinite(S64[..., 3]) & np.isfinite(n) & np.isfinite(a) & np.isfinite(h) & np.isfinite(x)
        centre = hit & (S64[..., 3] > 0) & np.isfinite(S64).all(-1) & np.isfinite(A64).all(-1)
        Pp, Np, tp = c64[..., :3], c64[..., 4:7], c64[..., 7]
        tol = P_["plane_tolerance_px"] * tp * 2.0 * np.tan(np.radians(float(fov)) / 2.0) / H
        pad = lambda v, fill: np.pad(v, [(r, r), (r, r)] + [(0, 0)] * (v.ndim - 2), constant_values=fill)
        okp, np_, ap, hp, xp = pad(ok, False), pad(np.where(ok, n, 0.0), 0.0), pad(np.where(ok, a, 0.0), 0.0), pad(np.where(ok, h, 0.0), 0.0), pad(np.where(ok, x, 0.0), 0.0)
        Pq, Nq = pad(c64[..., :3], 0.0), pad(c64[..., 4:7], 0.0)
        cnt = np.zeros((H, W), np.int64); taps = np.zeros((H, W), np.uint64)
        K = np.zeros((H, W)); snx = np.zeros((H, W)); snx2 = np.zeros((H, W)); sna = np.zeros((H, W)); snh = np.zeros((H, W))
        k = 0
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                sl = (slice(r + dy, r + dy + H), slice(r + dx, r + dx + W))
                good = centre & okp[sl]
                good &= np.abs(((Pq[sl] - Pp) * Np).sum(-1)) <= tol
                good &= (Nq[sl] * Np).sum(-1) >= P_["normal_cos"]
                g = good.astype(np.float64)
                cnt += good; taps += np.where(good, (k + 1) * (k + 1), 0).astype(np.uint64)
                K += g * np_[sl]; snx += g * np_[sl] * xp[sl]; snx2 += g * np_[sl] * xp[sl] ** 2; sna += g * np_[sl] * ap[sl]; snh += g * np_[sl] * hp[sl]
                k += 1
        run = (cnt >= int(P_["min_pixels"])) & (K > 0)
        d = snx / K
        v = np.maximum(0.0, snx2 / K - d * d)
        se = np.sqrt(v / cnt)
        margin = np.where(run, np.abs(d) - P_["gamma"] * se, np.nan)
        e = np.maximum(0.0, margin)
        lam = np.minimum(1.0, P_["sensitivity"] * e / (np.maximum(sna / K, snh / K) + P_["lum_floor"]))
        lam = np.where(run & (lam > 0), lam, 0.0)
    out = dict(lam=lam.reshape(N), counted=cnt.reshape(N), taps=(taps.reshape(N) & 0xFFFFFFFF).astype(np.uint32), margin=margin.reshape(N))
    L, w = lam.reshape(N, 1), lam.reshape(N) > 0
    A0, S0 = A64.reshape(N, 4), S64.reshape(N, 4)
    with np.errstate(all="ignore"):
        out["A"] = np.where(w[:, None], A0 - L * S0, A0); out["S"] = np.where(w[:, None], S0 * (1.0 - L), S0)
    both = M is not None and SM is not None
    for key, arr in (("M", M), ("SM", SM)):
        out[key] = None if arr is None else np.asarray(arr, np.float32).reshape(N, 4).astype(np.float64)
    if both:
        M0, SM0 = out["M"], out["SM"]
        with np.errstate(all="ignore"):
            out["M"] = np.where(w[:, None], M0 - L * SM0, M0); out["SM"] = np.where(w[:, None], SM0 * (1.0 - L), SM0)
    return out


def build_cpu(outdir):
    """g++ -O2 -ffp-contract=off tests/rectify_cpu.cpp -> <outdir>/rectify_cpu.  A failed compile raises."""
    exe = os.path.join(str(outdir), "rectify_cpu")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "rectify_cpu.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, "rectify_cpu.cpp does not compile:\n" + r.stdout
    return exe


def run_cpu(exe, W, H, cur, A, S, fov, M=None, SM=None, expect_refused=False, **params):
    """the counterpart -> the same dict as reference(), float32 (margin absent)"""
    P_ = dict(DEFAULTS, **params)
    d = os.path.dirname(exe)
    fin, fout = os.path.join(d, "rc_in.bin"), os.path.join(d, "rc_out.bin")
    N = W * H
    with open(fin, "wb") as f:
        f.write(np.array([W, H, int(M is not None) | 2 * int(SM is not None), P_["radius"], P_["min_pixels"]], np.int32).tobytes())
        f.write(np.array([P_["gamma"], P_["sensitivity"], P_["lum_floor"], P_["plane_tolerance_px"], P_["normal_cos"], fov], np.float32).tobytes())
        for arr, k in ((cur, 8), (A, 4), (S, 4)) + (((M, 4),) if M is not None else ()) + (((SM, 4),) if SM is not None else ()):
            arr = np.ascontiguousarray(arr, np.float32).reshape(-1, k)
            assert arr.shape[0] == N
            f.write(arr.tobytes())
    r = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if expect_refused:
        assert r.returncode == 3, (r.returncode, r.stdout)
        return None
    assert r.returncode == 0, r.stdout
    raw = np.fromfile(fout, np.float32)
    q = [raw[i * N * 4:(i + 1) * N * 4].reshape(N, 4).copy() for i in range(4)]
    tail = raw[16 * N:]
    return dict(A=q[0], S=q[1], M=q[2] if M is not None else None, SM=q[3] if SM is not None else None, lam=tail[:N].copy(),
                counted=tail[N:2 * N].view(np.int32).copy(), taps=tail[2 * N:3 * N].view(np.uint32).copy())


def compare(cpu, ref, S, SM=None, rtol=1e-4, atol=1e-6):
    """-> (worst error in tolerance units over the agreeing pixels, share of pixels excluded because the two disagree on the counted taps or on
    which side of e > 0 they stand).  lambda and A': rtol relative + atol absolute.  S' = S (1 - lambda), and M' / SM' likewise, carry lambda's
    own allowance times the marked value on top -- 1 - lambda cancels as lambda nears 1, so an error of lambda inside ITS tolerance is an
    ABSOLUTE error of |S| (rtol lambda + atol) in S', whatever is left of S'.  S / SM: the marked inputs."""
    agree = (cpu["counted"] == ref["counted"]) & (cpu["taps"] == ref["taps"]) & ((cpu["lam"] > 0) == (ref["lam"] > 0))
    lam_tol = (rtol * np.abs(ref["lam"]) + atol)[agree, None]
    marks = dict(S=S, M=SM, SM=SM)
    worst = 0.0
    for key in ("lam", "A", "S", "M", "SM"):
        if ref[key] is None:
            continue
        a, b = np.asarray(cpu[key], np.float64)[agree], np.asarray(ref[key], np.float64)[agree]
        tol = rtol * np.abs(b) + atol
        if marks.get(key) is not None:
            with np.errstate(all="ignore"):
                tol = tol + np.abs(np.asarray(marks[key], np.float64))[agree] * lam_tol
        fin = np.isfinite(b)
        assert np.array_equal(np.isfinite(a), fin)
        if fin.any():
            worst = max(worst, float((np.abs(a[fin] - b[fin]) / tol[fin]).max()))
    return worst, float(1.0 - agree.mean())


def same(a, b):
    """bit for bit"""
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))
