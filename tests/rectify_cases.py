"""Analytic inputs of the history-rectification tests, shared by tests/test_rectify.py (CPU counterpart against the float64
restatement) and tests/test_gpu_rectify.py (device against the counterpart).

scene(): a camera in front of a wall (index 0) with a rectangle (index 1) one unit in front of it, G-buffer analytic in float64
(reproject_reference.synth_gbuffer).  The history S is `spp` samples of a static per-pixel texture in [0.5, 1.5] (grey-ish rgb); the new samples
(1..4 per pixel) have the texture's mean times (1 + s_q u_q), s_q a checkerboard of +-1 and u_q in [0.1, 0.2] -- real noise, so the variance is
far above fp32 rounding, but balanced, so that on the unchanged surface |d| stays far below gamma se -- times `factor` on the rectangle (the
radiance there changed) and 1 on the wall.  No window mixes the two surfaces, and at the default gamma e > 0 is decided far from the threshold;
with a small gamma or window some of the wall's windows come close to it, which tests/test_rectify.py counts against its cap."""
import numpy as np
import reproject_reference as R

CAM = R.camera((0.0, 0.0, 4.0), (0.0, 0.0, 0.0))
FOV = float(CAM["fov"])


def gbuffer(W, H, wide=False, rect=True):
    # (the view is 2.31 W / H half-wide at the wall: the narrow wall leaves misses left and right of it, the wide one reaches all four edges)
    wall = R.quad((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 50.0 if wide else 1.8 * W / H, 50.0)
    front = R.quad((0.3, 0.1, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 0.9, 0.7)
    return R.synth_gbuffer(CAM, W, H, [wall, front] if rect else [wall])


def scene(W, H, seed, factor=0.3, spp=32, wide=False, adversarial=True, moments=True, rect=True):
    """-> dict(cur, A, S, M, SM, idx): float32 arrays as the library holds them; idx = the hit index per pixel"""
    rng = np.random.default_rng(seed)
    N = W * H
    cur = gbuffer(W, H, wide, rect)
    idx = cur[:, 3].copy().view(np.int32)
    tex = rng.uniform(0.5, 1.5, N)
    tint = rng.uniform(0.9, 1.1, (N, 3))
    S = np.zeros((N, 4)); S[:, :3] = tex[:, None] * tint * spp; S[:, 3] = spp
    n = rng.integers(1, 5, N).astype(np.float64)
    sign = np.where((np.arange(N) % W + np.arange(N) // W) % 2 == 0, 1.0, -1.0)
    mean = tex * (1.0 + sign * rng.uniform(0.1, 0.2, N)) * np.where(idx == 1, factor, 1.0)
    A = S.copy(); A[:, :3] += (mean * n)[:, None] * tint; A[:, 3] += n
    lumS = S[:, :3] @ np.array([0.2126, 0.7152, 0.0722]) / spp
    SM = np.stack([lumS * spp, (lumS ** 2 + 0.05) * spp, np.zeros(N), np.full(N, float(spp))], 1)
    M = SM.copy(); M[:, 0] += mean * n; M[:, 1] += mean * mean * n; M[:, 3] += n
    A, S, M, SM = (np.ascontiguousarray(v, np.float32) for v in (A, S, M, SM))
    if adversarial:
        k = max(1, N // 40)
        pick = lambda: rng.choice(N, k)
        j = pick(); A[j] = S[j]                                # no new sample: the pixel is no tap, its own window still decides
        A[pick(), 0] = np.nan; A[pick(), 1] = np.inf; S[pick(), 2] = -np.inf; S[pick(), 0] = np.nan
        j = pick(); S[j, 3] = 0.0
        j = pick(); A[j, 3] = np.inf
        j = pick(); S[j, 3] = np.inf
        M[pick(), 0] = np.nan; SM[pick(), 1] = np.inf
        cur[pick(), 4:7] = (0.6, 0.0, 0.8)                     # a turned normal at the same position
        cur[pick(), 0] = np.nan                                # a non-finite position
    return dict(cur=cur, A=A, S=S, M=M if moments else None, SM=SM if moments else None, idx=idx)


def same_surface_count(W, H, idx, r):
    """per pixel, how many pixels of its window (inside the image) show the same surface: the most taps it can count"""
    g = idx.reshape(H, W)
    p = np.pad(g, r, constant_values=-2)
    out = np.zeros((H, W), np.int64)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            out += (p[r + dy:r + dy + H, r + dx:r + dx + W] == g) & (g >= 0)
    return out.reshape(-1)


def statistical(seed, W=64, H=48, spp=32, drop=0.3):
    """the prototype's plane: a history of `spp` samples of mean 1, new samples uniform in [0, 2 mean] (one per pixel), the right half's mean
    dropped to `drop`, a fifth of the pixels without a new sample"""
    rng = np.random.default_rng(seed)
    N = W * H
    cur = R.synth_gbuffer(CAM, W, H, [R.quad((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 50.0, 50.0)])
    right = (np.arange(N) % W) >= W // 2
    S = np.zeros((N, 4)); S[:, :3] = spp; S[:, 3] = spp
    new = rng.uniform(0.0, 2.0, N) * np.where(right, drop, 1.0)
    has = rng.uniform(0.0, 1.0, N) >= 0.2
    A = S.copy(); A[has, :3] += new[has, None]; A[has, 3] += 1.0
    return dict(cur=cur, A=np.ascontiguousarray(A, np.float32), S=np.ascontiguousarray(S, np.float32), right=right)
