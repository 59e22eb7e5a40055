"""Scenes, deformations and numpy restatements shared by tests/test_refit.py (CPU) and tests/test_gpu_refit.py.

A case is a scene family of tests/traversal_cases.py with the tree built on positions P, then moved to P' by
  identity   P' = P              (SBVH: clipped leaves become unclipped; flat_walls: zero-extent boxes)
  smooth     P + 0.3 * extent * a sine field of the position
  scramble   every triangle translated by its own random vector of up to the scene extent (the topology is then worthless)
"""
from fractions import Fraction
import copy
import numpy as np
import traversal_cases as tc
from fluctus_amd import host

SCENES = dict(tc.scene_cases())
CASES = ["flat_walls-o0", "mixed_scale-o0", "spatial_splits-o0", "flat_walls-o1e5"]
BUILDERS = ("sbvh", "sah")
DEFORMS = ("identity", "smooth", "scramble")
LEAF_BIT = 0x80000000


def deform(P, kind, seed=3):
    P = np.asarray(P, np.float64)
    if kind == "identity":
        return P.copy()
    lo, hi = P.min((0, 1)), P.max((0, 1))
    ext = float((hi - lo).max())
    if kind == "smooth":
        u = (P - lo) / ext
        f = np.stack([np.sin(5.0 * u[..., 1] + 1.0), np.sin(4.0 * u[..., 2] + 2.0), np.sin(6.0 * u[..., 0] + 3.0)], -1)
        return P + 0.3 * ext * f
    if kind == "scramble":
        rng = np.random.RandomState(seed)
        return P + rng.uniform(-ext, ext, (P.shape[0], 1, 3))
    raise ValueError(kind)


def built(P, builder):
    d = tc.make_scene(P)
    host.build_bvh(d, builder)
    return d


def moved(d, P2):
    """d's tree (nodes, indices: shared topology) over the triangles of positions P2; the nodes are a copy, still holding d's boxes"""
    m = tc.make_scene(P2)
    m.nodes, m.indices, m.world_radius = d.nodes.copy(), d.indices, d.world_radius
    return m


def refitted(d, P2):
    return host.refit_bvh(moved(d, P2))


def fold_min(vals):
    """first-of-equals fold (Box::expand, flx_refit.h: rf_min) along axis 0 -- unlike np.min it fixes the sign of a zero"""
    acc = vals[0].copy()
    for v in vals[1:]:
        acc = np.where(v < acc, v, acc)
    return acc


def fold_max(vals):
    acc = vals[0].copy()
    for v in vals[1:]:
        acc = np.where(v > acc, v, acc)
    return acc


def tri_bounds_union(d, slots):
    """fp32 union of the full bounds of the triangles in index-list slots `slots`, vertices folded in order v0 v1 v2"""
    pts = []
    for s in slots:
        t = d.tris[d.indices[s]]
        for v in ("v0", "v1", "v2"):
            pts.append(np.array([t[v]["p"][k] for k in "xyz"], np.float32))
    pts = np.stack(pts)
    return fold_min(pts), fold_max(pts)


def node_box(nd, i):
    return (np.array([nd["bmin"][k][i] for k in "xyz"], np.float32), np.array([nd["bmax"][k][i] for k in "xyz"], np.float32))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_refit_boxes(d):
    """every leaf box of d.nodes is the union of its triangles' bounds, every inner box the union of its two children, bit for bit"""
    nd = d.nodes
    for i in range(nd.size):
        mn, mx = node_box(nd, i)
        if nd["nPrims"][i]:
            s0 = int(nd["iStartOrRight"][i])
            emn, emx = tri_bounds_union(d, range(s0, s0 + int(nd["nPrims"][i])))
        else:
            (lmn, lmx), (rmn, rmx) = node_box(nd, i + 1), node_box(nd, int(nd["iStartOrRight"][i]))
            emn, emx = fold_min(np.stack([lmn, rmn])), fold_max(np.stack([lmx, rmx]))
        assert np.array_equal(bits(mn), bits(emn)) and np.array_equal(bits(mx), bits(emx)), f"node {i}: {mn} {mx} vs {emn} {emx}"


def planes_contain(o, s, qlo, qhi, cmin, cmax):
    """in exact rational arithmetic: o + qlo s <= child min and o + qhi s >= child max on every axis of every child (cmin, cmax: (ns, 3))"""
    for a in range(3):
        fo, fs = Fraction(float(o[a])), Fraction(float(s[a]))
        for k in range(cmin.shape[0]):
            ql, qh = (int(qlo[a]) >> (8 * k)) & 255, (int(qhi[a]) >> (8 * k)) & 255
            if fo + ql * fs > Fraction(float(cmin[k, a])) or fo + qh * fs < Fraction(float(cmax[k, a])):
                return False
    return True


def two_triangle_scene():
    """one leaf: ninner == 0, the binary root is synthetic and the wide root a leaf ref.
    WHY THIS SHAPE.  When the root is a leaf the reference (and the oracle) test NO box at all (src/bvh.cl:234-310 starts on the triangles),
    while the device tests the leaf's box as it does for every other leaf (binary kernels: the synthetic root's two halves).  Where the slab's
    rounding decides -- a ray through an edge of the box, or a ray from 2^26 away, where one ulp of t (8 units) exceeds a small box -- the
    device misses what the oracle hits.  Measured with a FRESH upload, no refit involved, both the 4-wide and the binary kernels: 75 of 6370
    rays of traversal_cases on a unit-sized pair with an edge on the box's edge, 37 (all from the far-origin generator) on a unit-sized pair
    without one.  That is the code as it stands for one-leaf scenes; the traversal kernels are out of this change's reach.  So the pair is
    4096 units across (the far rays aim at its centroids, thousands of ulps inside the box) and each of the six vertices is the box's extreme
    on exactly ONE axis side (no vertex or edge of a triangle on an edge of the box): the slab then passes with room for every ray that can hit."""
    a, b, c = (0.0, 0.4, 0.5), (1.0, 0.6, 0.45), (0.5, 0.0, 0.55)
    d, e, f = (0.45, 1.0, 0.4), (0.4, 0.55, 0.0), (0.6, 0.5, 1.0)
    P = np.array([[a, c, f], [b, d, e]], np.float64) * 4096.0
    d = built(P, "sbvh")
    assert d.nodes.size == 1 and d.nodes["nPrims"][0] == 2
    return P, d


def with_shading(d, seed=5, nmat=None):
    """a copy of d whose normals, uvs and (with nmat) material ids are replaced by random ones: what a shade pass must carry over"""
    m = copy.copy(d)
    m.tris = d.tris.copy()
    rng = np.random.RandomState(seed)
    for v in ("v0", "v1", "v2"):
        n = rng.normal(size=(m.tris.size, 3)); n /= np.linalg.norm(n, axis=1, keepdims=True)
        for j, k in enumerate("xyz"):
            m.tris[v]["n"][k] = n[:, j]
        m.tris[v]["t"]["x"], m.tris[v]["t"]["y"] = rng.rand(m.tris.size), rng.rand(m.tris.size)
    if nmat:
        m.tris["matId"] = rng.randint(0, nmat, m.tris.size)
    return m
