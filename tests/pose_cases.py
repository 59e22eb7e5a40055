"""Transforms, object maps, scenes and the numpy restatements shared by tests/test_pose.py (CPU) and tests/test_gpu_pose.py.

THE RESTATEMENT (pose32) is written from the definition of the pose, not from csrc/flx_pose.h: for a 3 x 4 row-major affine X = [M | t], all in
np.float32 operations in this order,
  position  p'.x = ((m00 p.x + m01 p.y) + m02 p.z) + t.x, likewise y and z
  normal    u = s (C n) row by row as above, C[i][j] = M[i+1][j+1] M[i+2][j+2] - M[i+1][j+2] M[i+2][j+1] (indices mod 3: the cofactor matrix),
            det = (m00 C00 + m01 C01) + m02 C02, s = +1 when det > 0 else -1, then n' = u / sqrt((u.x u.x + u.y u.y) + u.z u.z)
  copied    every .w word, the texcoords, matId and the pad words
pose64 is the same in float64 (from the fp32 matrix entries, exactly converted).
"""
import copy
import numpy as np
import traversal_cases as tc
import refit_cases as rc
import refit_subset_cases as sc

NO_OBJECT = 0xFFFFFFFF
F = np.float32
VERTS = ("v0", "v1", "v2")
CASES = [("spatial_splits-o0", "sbvh"), ("mixed_scale-o0", "sbvh"), ("flat_walls-o1e5", "sbvh")]


# ---------------------------------------------------------------------------------------------------------------------------------
def _cofactors(m):
    c = np.zeros((3, 3), m.dtype)
    for i in range(3):
        for j in range(3):
            c[i, j] = m[(i + 1) % 3, (j + 1) % 3] * m[(i + 2) % 3, (j + 2) % 3] - m[(i + 1) % 3, (j + 2) % 3] * m[(i + 2) % 3, (j + 1) % 3]
    det = (m[0, 0] * c[0, 0] + m[0, 1] * c[0, 1]) + m[0, 2] * c[0, 2]
    return c, det, m.dtype.type(1.0 if det > 0 else -1.0)


def _xyz(a):
    return [a[k].copy() for k in "xyz"]


def pose32(tris, X):
    """the float32 restatement: a new wire.TRIANGLE array"""
    X = np.asarray(X, F).reshape(3, 4)
    m, t = X[:, :3], X[:, 3]
    c, _, s = _cofactors(m)
    out = tris.copy()
    with np.errstate(all="ignore"):
        for v in VERTS:
            p, n = _xyz(tris[v]["p"]), _xyz(tris[v]["n"])
            u = []
            for r, k in enumerate("xyz"):
                out[v]["p"][k] = ((m[r, 0] * p[0] + m[r, 1] * p[1]) + m[r, 2] * p[2]) + t[r]
                u.append(s * ((c[r, 0] * n[0] + c[r, 1] * n[1]) + c[r, 2] * n[2]))
            ln = np.sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2])
            assert ln.dtype == F and out[v]["p"]["x"].dtype == F
            for r, k in enumerate("xyz"):
                out[v]["n"][k] = u[r] / ln
    return out


def pose64(tris, X):
    """float64: (positions (T, 3, 3), unit normals (T, 3, 3), sum of |terms| per position component (T, 3, 3): what one fp32 ulp is measured at)"""
    X = np.asarray(X, F).reshape(3, 4).astype(np.float64)
    m, t = X[:, :3], X[:, 3]
    c, _, s = _cofactors(m)
    P = np.stack([np.stack(_xyz(tris[v]["p"]), -1) for v in VERTS], 1).astype(np.float64)
    N = np.stack([np.stack(_xyz(tris[v]["n"]), -1) for v in VERTS], 1).astype(np.float64)
    P2 = P @ m.T + t
    mag = np.abs(P) @ np.abs(m).T + np.abs(t)
    with np.errstate(all="ignore"):
        U = s * (N @ c.T)
        U = U / np.linalg.norm(U, axis=-1, keepdims=True)
    return P2, U, mag


# ---------------------------------------------------------------------------------------------------------------------------------
def rotation(axis, angle):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def affine(M=None, t=(0.0, 0.0, 0.0)):
    X = np.zeros((3, 4), F)
    X[:, :3] = np.eye(3) if M is None else M
    X[:, 3] = t
    return X


def about(M, centre):
    """x -> centre + M (x - centre)"""
    c = np.asarray(centre, np.float64)
    return affine(M, c - np.asarray(M, np.float64) @ c)


IDENTITY = affine()
TRANSFORM_NAMES = ("identity", "translation", "rotation", "scale", "mirror", "shear")


def transforms(P):
    """the six transforms for a scene of positions P: linear parts act about the scene's centre, so that the posed objects stay near the scene"""
    P = np.asarray(P, np.float64)
    ext, ctr = sc.extent(P), 0.5 * (P.min((0, 1)) + P.max((0, 1)))
    return {"identity": IDENTITY.copy(),
            "translation": affine(None, (0.125 * ext, 0.0, 0.0)),
            "rotation": about(rotation((1.0, 2.0, 3.0), 0.7), ctr),
            "scale": about(np.diag([2.0, 0.5, 3.0]), ctr),
            "mirror": about(np.diag([-1.0, 1.0, 1.0]), ctr),
            "shear": about(np.array([[1.0, 0.4, 0.0], [0.0, 1.0, -0.3], [0.2, 0.0, 1.0]]), ctr)}


# ---------------------------------------------------------------------------------------------------------------------------------
MAP_NAMES = ("interleaved", "single_and_empty", "all")


def object_map(kind, ntris):
    """(object_of_triangle, nobjects, the ids a test lists by default)"""
    i = np.arange(ntris)
    if kind == "interleaved":                                # i % 3, class 2 belongs to no object
        o = (i % 3).astype(np.uint32); o[i % 3 == 2] = NO_OBJECT
        return o, 2, [0, 1]
    if kind == "single_and_empty":                           # object 0: one member; object 1: none; object 2: the upper half
        o = np.full(ntris, NO_OBJECT, np.uint32); o[7] = 0; o[ntris // 2:] = 2
        return o, 3, [0, 1, 2]
    if kind == "all":
        return np.zeros(ntris, np.uint32), 1, [0]
    raise ValueError(kind)


def members_of(object_of, ids):
    """ascending triangle indices of the listed objects, and for each the position of its object in the list"""
    slot = {int(o): k for k, o in enumerate(np.asarray(ids).reshape(-1))}
    s = np.array([slot.get(int(o), -1) for o in np.asarray(object_of, np.uint32)], np.int64)
    idx = np.nonzero(s >= 0)[0].astype(np.uint32)
    return idx, s[idx]


def posed(rest_tris, object_of, ids, xforms, pose=None):
    """(indices, triangles): what a pose call hands to the subset refit -- the listed objects' members, ascending, each posed from rest_tris by its
    object's transform with `pose` (default: host.pose_triangles)"""
    if pose is None:
        from fluctus_amd import host
        pose = host.pose_triangles
    idx, slot = members_of(object_of, ids)
    out = rest_tris[idx].copy()
    xforms = np.asarray(xforms, F).reshape(-1, 3, 4)
    for k in range(xforms.shape[0]):
        sel = slot == k
        if sel.any():
            out[sel] = pose(rest_tris[idx[sel]], xforms[k])
    return idx, out


# ---------------------------------------------------------------------------------------------------------------------------------
def unit_normals(n, seed):
    """(n, 3) float32 vectors whose fp32 length, evaluated as the pose evaluates it, is 1 to the last bit: sqrt((x x + y y) + z z) == 1"""
    rng = np.random.RandomState(seed)
    out = np.zeros((n, 3), F)
    todo = np.arange(n)
    while todo.size:
        v = rng.normal(size=(todo.size, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)
        v = v.astype(F)
        ok = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]) == F(1.0)
        out[todo[ok]] = v[ok]
        todo = todo[~ok]
    return out


def shaded(d, seed=9, nmat=None):
    """a copy of d with unit normals (unit_normals), random uvs, and marked spare words: every .w, the texcoords' z and the pad carry bit patterns a
    pose must copy untouched"""
    m = copy.copy(d)
    m.tris = d.tris.copy()
    rng = np.random.RandomState(seed)
    T = m.tris.size
    for v in VERTS:
        n = unit_normals(T, rng.randint(1 << 30))
        for j, k in enumerate("xyz"):
            m.tris[v]["n"][k] = n[:, j]
        m.tris[v]["t"]["x"], m.tris[v]["t"]["y"] = rng.rand(T), rng.rand(T)
        m.tris[v]["t"]["z"] = rng.rand(T)
        for f in "pnt":
            m.tris[v][f]["w"] = rng.randint(1, 1 << 22, T).astype(np.uint32).view(F)
    m.tris["_pad"] = rng.randint(1, 1 << 30, (T, 3))
    if nmat:
        m.tris["matId"] = rng.randint(0, nmat, T)
    return m


_BUILT = {}


def case(name, builder):
    """the case's tree on its rest positions with `shaded` triangles: built once, shared, never modified"""
    if (name, builder) not in _BUILT:
        _BUILT[name, builder] = shaded(sc.built(name, builder))
    return _BUILT[name, builder]


# ---------------------------------------------------------------------------------------------------------------------------------
GRID_N = 28                                                  # 28 x 28 quads = 1568 triangles


def grid_positions():
    """a gently curved sheet of 2 x 28 x 28 triangles (traversal_cases._grid, lifted by a sine so that no box is flat)"""
    P = np.array(tc._grid((-2.0, 0.0, -2.0), (4.0, 0.0, 0.0), (0.0, 0.0, 4.0), GRID_N, GRID_N), np.float64)
    P[..., 1] = 0.3 * np.sin(1.7 * P[..., 0]) * np.cos(1.3 * P[..., 2])
    return P


def grid_map(ntris):
    """two objects in runs: 1550 members from triangle 10 on (seven blocks of 256).  Object 0's members are members 27 .. 289 and 490 .. 1326: both runs
    begin and end in the middle of a wave; between them lie 200 consecutive members of object 1, more than three whole waves that are not listed
    when object 0 alone is"""
    o = np.full(ntris, NO_OBJECT, np.uint32)
    o[10:37] = 1; o[37:300] = 0; o[300:500] = 1; o[500:1337] = 0; o[1337:1560] = 1
    return o, 2


_GRID = []


def grid_case():
    if not _GRID:
        _GRID.append(shaded(rc.built(grid_positions(), "sbvh")))
    return _GRID[0]
