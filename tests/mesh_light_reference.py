"""The arithmetic of the emissive-triangle lights (csrc/flx_mesh_light.h) restated in numpy, written from the definitions and
not from the header.

WHAT IS EXACT AND WHAT IS FLOAT64.  The weight w = 0.5 |(p1 - p0) x (p2 - p0)| luminance(Ke) is DEFINED in fp32 (the host and the device must
agree on it bit for bit, and its cross product cancels: no fp64 value is "within an ulp" of it for a thin triangle).  weights32 restates that
definition in np.float32 operations, one rounding each, in the order of flx_math.h (x x + y y + z z left to right; cross as a.y b.z - a.z b.y);
weights64 is the same in float64, for the tests that bound the fp32 value.  Everything AFTER the weights -- prefix sums, the division by the
total, the barycentric point -- is restated in float64 from those fp32 inputs: the code's fp64 sums differ from the exact ones by ~1e-16
relative, so its cdf is within one fp32 ulp of the rounded float64 value.
"""
import numpy as np

F = np.float32
NONE = 0xFFFFFFFF
VERTS = ("v0", "v1", "v2")


def positions(tris, dtype=np.float64):
    """(T, 3 vertices, 3) positions"""
    return np.stack([np.stack([tris[v]["p"][k] for k in "xyz"], -1) for v in VERTS], 1).astype(dtype)


def ke_of(d):
    """(T, 3) the Ke of every triangle's material"""
    m = d.materials[d.tris["matId"]]
    return np.stack([m["Ke"][k] for k in "xyz"], -1)


def lights(d):
    """ascending indices of the triangles whose material has a Ke component > 0"""
    return np.nonzero((ke_of(d) > 0).any(-1))[0].astype(np.uint32)


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], -1)


def _weights(P, ke, T):
    c = _cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    area = T(0.5) * np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
    lum = (T(F(0.212671)) * ke[:, 0] + T(F(0.715160)) * ke[:, 1]) + T(F(0.072169)) * ke[:, 2]
    w = area * lum
    assert w.dtype == T
    with np.errstate(invalid="ignore"):
        return np.where((w > 0) & np.isfinite(w), w, T(0.0)), area


def weights32(d, idx):
    return _weights(positions(d.tris[idx], F), ke_of(d)[idx].astype(F), F)


def weights64(d, idx):
    return _weights(positions(d.tris[idx]), ke_of(d)[idx].astype(np.float64), np.float64)


def table(d):
    """(tris, cdf as float32(float64 value), total) from the fp32 weights; the last light with a weight has cdf 1; no weight at all: empty"""
    idx = lights(d)
    w, _ = weights32(d, idx)
    total = float(np.sum(w.astype(np.float64)))
    if not total > 0.0:
        return np.zeros(0, np.uint32), np.zeros(0, F), 0.0
    cdf = (np.cumsum(w.astype(np.float64)) / total).astype(F)
    cdf[np.nonzero(w > 0)[0][-1]:] = F(1.0)
    return idx, cdf, total


def pick(cdf, pk, r):
    """the first k with cdf[k] > r, clamped to the last light with pick > 0"""
    last = np.nonzero(np.asarray(pk) > 0)[0][-1]
    return np.minimum(np.searchsorted(cdf, np.asarray(r, F), side="right"), last).astype(np.uint32)


def sample64(P, r1, r2):
    """float64: P (n, 3, 3) -> (points (n, 3), barycentric coefficients (n, 3)) for s = sqrt(r1): (1 - s) p0 + s (1 - r2) p1 + s r2 p2"""
    r1, r2 = np.asarray(r1, F).astype(np.float64), np.asarray(r2, F).astype(np.float64)
    s = np.sqrt(r1)
    b = np.stack([1.0 - s, s * (1.0 - r2), s * r2], -1)
    return (b[:, :, None] * P.astype(np.float64)).sum(1), b


def edge_randoms(n, seed):
    """n (r1, r2) pairs in [0, 1): random ones behind every combination of 0, the largest float below 1 and two ordinary values"""
    below1 = np.nextafter(F(1.0), F(0.0))
    e = np.array([0.0, below1, 0.25, 0.7], F)
    g = np.stack(np.meshgrid(e, e), -1).reshape(-1, 2)
    rng = np.random.RandomState(seed)
    r = rng.random_sample((n, 2)).astype(F)
    r[r >= 1.0] = below1
    r[:g.shape[0]] = g
    return r


def ulp_diff(a, b):
    """distance in fp32 ulps between two arrays of non-negative finite floats"""
    return np.abs(np.asarray(a, F).view(np.int32).astype(np.int64) - np.asarray(b, F).view(np.int32).astype(np.int64))


# ---- the statistical comparison of two renders (tests 4 and 5 of tests/test_gpu_mesh_lights.py)
def lum(rgb):
    return 0.2126 * rgb[..., 0] + 0.7152 * rgb[..., 1] + 0.0722 * rgb[..., 2]


def tile_stats(px, mom, W, H, tile=8):
    """per tile: (mean luminance of the tile, variance of that mean) from the accumulation (rgb sum, n) and the moments (sum l, sum l^2, _, n):
    the pixel mean is S1 / n with variance (S2 / n - mean^2) / n; the tile mean averages its npx pixel means, so its variance is sum(var_px) / npx^2"""
    mom = np.asarray(mom, np.float64).reshape(H, W, 4)
    n = np.maximum(mom[..., 3], 1.0)
    mean = mom[..., 0] / n
    var = np.maximum(mom[..., 1] / n - mean * mean, 0.0) / n
    ty, tx = H // tile, W // tile
    tm = mean[:ty * tile, :tx * tile].reshape(ty, tile, tx, tile)
    tv = var[:ty * tile, :tx * tile].reshape(ty, tile, tx, tile)
    npx = tile * tile
    return tm.mean((1, 3)), tv.sum((1, 3)) / npx ** 2


def tile_z(a, b, W, H):
    """|A - B| / SE per tile, SE^2 the sum of the two tile-mean variances; a, b = (pixels, moments)"""
    ma, va = tile_stats(a[0], a[1], W, H)
    mb, vb = tile_stats(b[0], b[1], W, H)
    se = np.sqrt(va + vb)
    with np.errstate(invalid="ignore", divide="ignore"):
        z = np.where(se > 0, np.abs(ma - mb) / se, np.where(ma == mb, 0.0, np.inf))
    return z, ma, mb
