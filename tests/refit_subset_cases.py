"""Subsets, scenes and the numpy restatement shared by tests/test_refit_subset.py (CPU) and tests/test_gpu_refit_subset.py.

A case is a scene family of tests/traversal_cases.py with the tree built on positions P; the STANDARD SUBSET S(name) -- every eighth triangle,
from index 40 for the spatial_splits family (the first 40 are the room: the long slivers the SBVH clips start behind them) and from 0 for the
others -- is translated by 0.125 x the scene extent along x.  `refit_subset` restates BVH::refitSubset (host.refit_bvh_subset) in numpy: a leaf
holding a listed triangle gets the union of the full bounds of its triangles, an inner node with a changed child the union of its two children,
every other node keeps its bytes.
"""
import copy
import numpy as np
import traversal_cases as tc
import refit_cases as rc

CASES = [("spatial_splits-o0", "sbvh"), ("mixed_scale-o0", "sbvh"), ("flat_walls-o1e5", "sbvh"), ("spatial_splits-o0", "sah")]
UNCLIPPED = [("flat_walls-o1e5", "sbvh"), ("spatial_splits-o0", "sah")]      # no leaf is clipped: the subset result is the full refit's


def extent(P):
    P = np.asarray(P, np.float64)
    return float((P.max((0, 1)) - P.min((0, 1))).max())


def subset_indices(name, ntris):
    return np.arange(40 if name.startswith("spatial_splits") else 0, ntris, 8, dtype=np.uint32)


def translated(P, idx, shift):
    P2 = np.asarray(P, np.float64).copy()
    P2[idx] += np.asarray(shift, np.float64)
    return P2


def standard_shift(P):
    return np.array([0.125 * extent(P), 0.0, 0.0])


def S(name, P=None):
    """(indices, positions with the subset moved) of the standard subset"""
    P = rc.SCENES[name] if P is None else P
    idx = subset_indices(name, P.shape[0])
    return idx, translated(P, idx, standard_shift(P))


_BUILT = {}


def built(name, builder):
    """the case's tree on its rest positions: built once, shared, never modified (every user copies what it changes)"""
    if (name, builder) not in _BUILT:
        _BUILT[name, builder] = rc.built(rc.SCENES[name], builder)
    return _BUILT[name, builder]


def moved_scene(d, P2):
    """rc.moved: d's topology and (still) d's boxes over the triangles at P2"""
    return rc.moved(d, P2)


def with_shading_on(m, idx, seed=5, nmat=None):
    """a copy of m whose triangles `idx` carry the normals, uvs (and material ids) rc.with_shading draws; all others keep theirs"""
    s = rc.with_shading(m, seed, nmat)
    out = copy.copy(m)
    out.tris = m.tris.copy()
    out.tris[idx] = s.tris[idx]
    return out


def dirty_sets(d, idx):
    """(per node: holds a listed triangle below it, the leaf nodes among them) over d's topology"""
    nd = d.nodes
    moved = np.zeros(d.tris.size, bool); moved[np.asarray(idx, np.int64)] = True
    dirty = np.zeros(nd.size, bool)
    for i in range(nd.size - 1, -1, -1):
        if nd["nPrims"][i]:
            s0 = int(nd["iStartOrRight"][i])
            dirty[i] = moved[d.indices[s0:s0 + int(nd["nPrims"][i])]].any()
        else:
            dirty[i] = dirty[i + 1] or dirty[int(nd["iStartOrRight"][i])]
    return dirty


def refit_subset(m, idx):
    """the restatement: (new node array, dirty flags) for m.nodes / m.indices over m.tris (the moved triangles in place), `idx` listed"""
    nd = m.nodes.copy()
    dirty = dirty_sets(m, idx)
    for i in range(nd.size - 1, -1, -1):
        if not dirty[i]:
            continue
        if nd["nPrims"][i]:
            s0 = int(nd["iStartOrRight"][i])
            mn, mx = rc.tri_bounds_union(m, range(s0, s0 + int(nd["nPrims"][i])))
        else:
            (lmn, lmx), (rmn, rmx) = rc.node_box(nd, i + 1), rc.node_box(nd, int(nd["iStartOrRight"][i]))
            mn, mx = rc.fold_min(np.stack([lmn, rmn])), rc.fold_max(np.stack([lmx, rmx]))
        for j, k in enumerate("xyz"):
            nd["bmin"][k][i], nd["bmax"][k][i] = mn[j], mx[j]
    return nd, dirty


def clipped_leaves(d):
    """leaf nodes of d whose box lies strictly inside the full bounds of their triangles on some axis side"""
    nd = d.nodes
    out = []
    for i in np.nonzero(nd["nPrims"] > 0)[0]:
        s0 = int(nd["iStartOrRight"][i])
        fmn, fmx = rc.tri_bounds_union(d, range(s0, s0 + int(nd["nPrims"][i])))
        mn, mx = rc.node_box(nd, i)
        if (mn > fmn).any() or (mx < fmx).any():
            out.append(int(i))
    return out


def subset_refitted(d, idx, P2):
    """host.refit_bvh_subset of d's tree with triangles `idx` moved to P2[idx]"""
    from fluctus_amd import host
    return host.refit_bvh_subset(moved_scene(d, P2), idx)


def surface_area_sum(nd):
    """sum over the nodes of area x (count or 1) / root area: the plain figure the clipped-leaf argument is made with"""
    e = [nd["bmax"][k].astype(np.float64) - nd["bmin"][k] for k in "xyz"]
    a = e[0] * e[1] + e[1] * e[2] + e[2] * e[0]
    return float((a * np.maximum(nd["nPrims"], 1)).sum() / a[0])
