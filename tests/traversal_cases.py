"""Adversarial scenes and rays for the traversal kernels, and a float64 brute-force witness that does not use the tree.

Every other traversal test compares two traversals of the same node array (device / emulation / oracle / reference kernels).  Here the
question is the one a loop over all triangles answers: "is this the closest triangle?", asked where the fp32 arithmetic of the reference
can still decide it (the classifier below) and on inputs chosen for the edges of flx_trace4.h's error analysis, not for realism.

  BruteForce      every ray against every triangle, the reference's Moller-Trumbore (src/intersect.cl:62-93, csrc/flx_trace.h:42-62)
                  restated in float64, plus an fp32 error estimate per ray / triangle pair -> robust hit / robust miss / ambiguous.
  Verdict         per builder: a ray is DECIDED when the float64 answer binds the fp32 traversal of that tree (closest hit: one robust
                  nearest hit, no ambiguous or robust rival near it, its hit point inside a leaf box that references the triangle;
                  any hit: a robust occluder inside such a leaf box, or nothing robust or ambiguous below tMax).
  scenes / rays   wire-format generators (numpy).  Used by tests/test_traversal_edges.py (CPU) and tests/test_gpu_traversal_edges.py.
"""
import numpy as np
from fluctus_amd import host, wire
from common import COL, Q

# ---- the classifier's margins, in one place -------------------------------------------------------------------------------------
EPS_B = 1e-5                  # barycentric margin (floor; the fp32 error estimate of u, v widens it per pair)
EPS_T = 1e-5                  # relative gap in t between the closest robust hit and any rival, and between an occluder and tMax
EPS_D = 1e-5                  # relative margin of |det| around the Moller-Trumbore cut-off
EPS_P = 1e-6                  # leaf-box margin of a hit point, relative to the scene extent (plus the fp32 resolution at the point)
K_ERR = 16.0 * 2.0 ** -24     # fp32 evaluation error of one dot / cross product chain, with room to spare
DET_CUT = float(np.float32(1e-12))              # the cut-off as the kernels compare it (an fp32 constant)
FLT_MAX = float(np.finfo(np.float32).max)
FAR_ORIGIN = 67108864.0                         # 2^26: flx_trace4.h WRay::setup's per-ray `far` branch, api_upload.hip's wideClamp choice
COORD_MAX = 4.611686e18                         # 2^62: FLX_WIDE_COORD_MAX (csrc/flx_wide.h)
BUILDERS = ("sbvh", "sah", "binned")


# ---------------------------------------------------------------------------------------------------------------------------------
# scenes
def tri_points(d):
    """(T, 3 vertices, 3) float64 -- exactly the fp32 vertex positions."""
    return np.stack([np.stack([d.tris[v]["p"][k] for k in "xyz"], 1) for v in ("v0", "v1", "v2")], 1).astype(np.float64)


def make_scene(P):
    """SceneData from (T, 3, 3) vertex positions (rounded to fp32): face normals, one diffuse material, no textures, no tree."""
    import common
    P = np.asarray(P, np.float64)
    P32 = P.astype(np.float32)
    n = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-300)
    t = np.zeros(P.shape[0], wire.TRIANGLE)
    for i, v in enumerate(("v0", "v1", "v2")):
        for j, k in enumerate("xyz"):
            t[v]["p"][k] = P32[:, i, j]
            t[v]["n"][k] = n[:, j]
    d = host.SceneData()
    d.tris = t
    d.materials = np.array([common.default_material()], wire.MATERIAL)
    d.texdesc = np.zeros(0, wire.TEXDESC)
    d.texdata = np.zeros(0, np.uint8)
    return d


def _quad(c, u, v):
    """Two triangles of the parallelogram c, c + u, c + u + v, c + v (sharing the diagonal c -- c + u + v)."""
    c, u, v = (np.asarray(a, np.float64) for a in (c, u, v))
    return [[c, c + u, c + u + v], [c, c + u + v, c + v]]


def _grid(c, u, v, nu, nv):
    out = []
    for j in range(nv):
        for i in range(nu):
            out += _quad(np.asarray(c, float) + np.asarray(u, float) * i / nu + np.asarray(v, float) * j / nv,
                         np.asarray(u, float) / nu, np.asarray(v, float) / nv)
    return out


def _box(lo, hi, n=1):
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    e = hi - lo
    X, Y, Z = np.array([e[0], 0, 0]), np.array([0, e[1], 0]), np.array([0, 0, e[2]])
    out = []
    out += _grid(lo, X, Z, n, n) + _grid(lo + Y, X, Z, n, n)            # bottom, top
    out += _grid(lo, X, Y, n, n) + _grid(lo + Z, X, Y, n, n)            # front, back
    out += _grid(lo, Z, Y, n, n) + _grid(lo + X, Z, Y, n, n)            # left, right
    return out


def flat_walls():
    """An axis-aligned room [-2, 2] x [0, 3] x [-2, 2]: floor in two halves gridded 4 x 8 and 3 x 6 (T-junctions along x = 0), walls
    gridded in rows 0.75 high (y = 1 is inside a row), a ceiling, a table (a box, and a second coplanar top quad stacked on it), a shelf
    of three coplanar quads that share edges.  Every leaf and node box is flat on some axis."""
    T = []
    T += _grid((-2, 0, -2), (2, 0, 0), (0, 0, 4), 4, 8) + _grid((0, 0, -2), (2, 0, 0), (0, 0, 4), 3, 6)
    T += _grid((-2, 3, -2), (4, 0, 0), (0, 0, 4), 4, 4)
    T += _grid((-2, 0, -2), (4, 0, 0), (0, 3, 0), 6, 4) + _grid((-2, 0, 2), (4, 0, 0), (0, 3, 0), 5, 4)
    T += _grid((-2, 0, -2), (0, 0, 4), (0, 3, 0), 6, 4) + _grid((2, 0, -2), (0, 0, 4), (0, 3, 0), 4, 4)
    T += _box((-1.0, 0.0, -0.5), (0.5, 1.0, 0.5), 2)
    T += _quad((-1.0, 1.0, -0.5), (0.75, 0, 0), (0, 0, 1.0))              # a second top, coplanar with the table's, half as wide
    for k in range(3):
        T += _quad((0.8 + 0.4 * k, 2.0, -1.9), (0.4, 0, 0), (0, 0, 0.5))  # shelf: three quads sharing edges, a flat node
    return np.array(T)


def mixed_scale(seed=5):
    """One triangle ~1e4 times larger than its neighbours, clusters of tiny triangles and of slivers next to it."""
    rng = np.random.RandomState(seed)
    T = [[(-2, 0, -2), (2, 0, -2), (-2, 0, 2)]]                             # the big one, 4 units
    for c in rng.uniform(-1.5, 1.5, size=(6, 3)) * (1, 0, 1) + (0, 0.3, 0):
        for _ in range(24):                                                 # tiny: ~4e-4
            p = c + rng.uniform(-2e-3, 2e-3, 3)
            T.append([p, p + rng.uniform(-4e-4, 4e-4, 3), p + rng.uniform(-4e-4, 4e-4, 3)])
    for k in range(48):                                                     # slivers: 1 long, ~1e-4 wide
        p = np.array([-1.0 + 2.0 * k / 48, 0.5 + 0.01 * (k % 5), 1.0])
        a = rng.uniform(0, np.pi)
        u = np.array([np.cos(a), 0.0, np.sin(a)])
        T.append([p, p + u, p + u * 0.5 + (0, 1e-4, 0)])
    return np.array(T, np.float64)


def spatial_split_scene(seed=7):
    """Long thin triangles that straddle the scene (SBVH makes spatial splits) over a field of small ones."""
    rng = np.random.RandomState(seed)
    T = []
    for k in range(40):
        a = rng.uniform(-2, 2, 3); b = -a + rng.uniform(-0.2, 0.2, 3)
        w = rng.normal(size=3); w *= 0.02 / np.linalg.norm(w)
        T.append([a, b, b + w])
    for c in rng.uniform(-2, 2, size=(300, 3)):
        T.append([c, c + rng.uniform(-0.12, 0.12, 3), c + rng.uniform(-0.12, 0.12, 3)])
    return np.array(T, np.float64)


# family: (generator, size of its smallest feature)
FAMILIES = {"flat_walls": (flat_walls, 0.25), "mixed_scale": (mixed_scale, 4e-4), "spatial_splits": (spatial_split_scene, 0.05)}
# (name, scale, offset): translations 0, 1e3, 1e5 and one past 2^26 -- with the geometry scaled up, where needed, so that the smallest
# feature still spans ~1000 ulps -- and copies scaled by 1e-3 / 1e3
TRANSFORMS = [("o0", 1.0, 0.0), ("o1e3", 1.0, 1e3), ("o1e5", 1.0, 1e5), ("o1e8", 1.0, 1e8), ("s1e-3", 1e-3, 0.0), ("s1e3", 1e3, 0.0)]


def scene_cases():
    """[(name, (T, 3, 3) positions)]: every family under every transform, and the flat room blown up to a root box of ~+-2^61."""
    out = []
    for fam, (fn, finest) in FAMILIES.items():
        P = fn()
        for tn, s, o in TRANSFORMS:
            s = max(s, 1000.0 * o * 2.0 ** -23 / finest)
            out.append((f"{fam}-{tn}", (P * s + np.array([o, 0.5 * o, -o]))))
    out.append(("flat_walls-2^61", flat_walls() * (2.0 ** 61 / 3.0)))
    return out


def beyond_bound_scene():
    """The flat room with its root box reaching past +-2^62: flx_upload_scene and the wide-tree build must refuse it."""
    return flat_walls() * (2.0 ** 63 / 3.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# the tree's leaves
class Leaves:
    """Leaf boxes of a binary node array and, per triangle, the leaves that reference it."""

    def __init__(self, d):
        nd = d.nodes
        leaf = np.nonzero(nd["nPrims"] > 0)[0]
        self.lo = np.stack([nd["bmin"][k][leaf] for k in "xyz"], 1).astype(np.float64)
        self.hi = np.stack([nd["bmax"][k][leaf] for k in "xyz"], 1).astype(np.float64)
        self.node = leaf
        owner = np.repeat(np.arange(leaf.size), nd["nPrims"][leaf].astype(np.int64))
        start = nd["iStartOrRight"][leaf].astype(np.int64)
        slot = np.concatenate([np.arange(s, s + c) for s, c in zip(start, nd["nPrims"][leaf].astype(np.int64))])
        tri = d.indices[slot].astype(np.int64)
        order = np.argsort(tri, kind="stable")
        tri, owner = tri[order], owner[order]
        cnt = np.bincount(tri, minlength=d.tris.size)
        self.maxdup = int(cnt.max())
        self.of_tri = np.full((d.tris.size, self.maxdup), -1, np.int64)
        first = np.concatenate([[0], np.cumsum(cnt)[:-1]])
        self.of_tri[tri, np.arange(tri.size) - first[tri]] = owner
        self.count = cnt


def leaf_check(leaves, tri, p, tol, crossing):
    """Per (ray, triangle) pair with float64 hit point p (absolute coordinates) and margin tol:
      ok       some leaf referencing tri holds p at least tol inside on every axis, except on at most one axis that the ray crosses
               (fp32 1/d finite: the slab's two planes are then ordered and a hit point on that face is reached), where it may lie on
               the face (within tol);
      covered  p lies within tol of some leaf box referencing tri (else: a builder bug);
      face0    no leaf is ok, and p lies within tol of a face whose axis the ray does not cross (d = +-0 or 1/d overflows): the
               reference's slab evaluates (b - o) * inf there, which is where its semantics decide."""
    L = leaves.of_tri[tri]                                  # (n, maxdup)
    valid = L >= 0
    Lc = np.where(valid, L, 0)
    lo, hi = leaves.lo[Lc], leaves.hi[Lc]                   # (n, maxdup, 3)
    pp = p[:, None, :]
    margin = np.minimum(pp - lo, hi - pp)
    t = tol[:, None, None]
    bad = margin < t
    nbad = bad.sum(2)
    cr = crossing[:, None, :]
    one_ok = (nbad == 1) & (bad & cr & (margin >= -t)).any(2)
    ok = ((nbad == 0) | one_ok) & valid
    out = np.maximum(np.maximum(lo - pp, pp - hi), 0.0).max(2)
    covered = ((out <= tol[:, None]) & valid).any(1)
    face0 = ((np.abs(margin) <= t) & ~cr).any(2) & valid
    ok_any = ok.any(1)
    return ok_any, covered, face0.any(1) & ~ok_any


# ---------------------------------------------------------------------------------------------------------------------------------
# the float64 witness
def _cabs(a, b):
    """|a| x |b| with every product added: the componentwise bound of a cross product's rounding."""
    a, b = np.abs(a), np.abs(b)
    return np.stack([a[:, 1] * b[:, 2] + a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] + a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0]], 1)


class BruteForce:
    """All rays x all triangles in float64 with the reference's semantics: Moller-Trumbore with |det| < 1e-12 rejecting, inclusive u, v,
    u + v bounds; closest hit needs t > 0 (MT's t >= 0 and the traversal's t > 0), any hit 0 < t < tMax.  Each pair is classified
    robust hit / robust miss / ambiguous against an fp32 error estimate; the tree enters only in verdict()."""

    def __init__(self, P, orig, dirs, tmax, chunk_pairs=1 << 18):
        P = np.asarray(P, np.float64)
        self.ntri = P.shape[0]
        self.extent = float((P.max((0, 1)) - P.min((0, 1))).max())
        c = np.float32(0.5 * (P.min((0, 1)) + P.max((0, 1)))).astype(np.float64)     # fp32 centre: every shift below is exact
        self.c = c
        p0, p1, p2 = P[:, 0] - c, P[:, 1] - c, P[:, 2] - c
        s1, s2 = p1 - p0, p2 - p0
        n = np.cross(s1, s2)
        c1p, c2 = np.cross(p0, s1), np.cross(s2, p0)
        k = (s2 * c1p).sum(1)
        S1, S2 = np.linalg.norm(s1, axis=1), np.linalg.norm(s2, axis=1)
        cab = _cabs(s1, s2)
        pp = (p0 * p0).sum(1)
        o = np.asarray(orig, np.float32).astype(np.float64)
        dd = np.asarray(dirs, np.float32).astype(np.float64)
        tm = np.asarray(tmax, np.float32).astype(np.float64)
        self.orig_abs, self.dir, self.tmax = o, dd, tm
        o = o - c
        nr = o.shape[0]
        self.closest = np.full(nr, -1, np.int64)
        self.t_closest = np.full(nr, np.inf)
        self.closest_clear = np.zeros(nr, bool)       # no ambiguous triangle and no rival robust hit near the closest robust hit
        self.reason = np.zeros(nr, np.int8)           # 0 clear, 1 ambiguous triangle, 2 robust rival within eps_t
        self.shadow_clear = np.zeros(nr, bool)        # nothing robust or ambiguous below tMax (1 + eps_t)
        self.shadow_hit_any = np.zeros(nr, bool)      # float64: some triangle with 0 < t < tMax
        occ_r, occ_t, occ_tri = [], [], []            # robust occluders below tMax (1 - eps_t)
        self.n_amb = np.zeros(nr, np.int64)
        step = max(1, chunk_pairs // max(1, self.ntri))
        for a in range(0, nr, step):
            b = min(nr, a + step)
            O, D = o[a:b], dd[a:b]
            M = np.cross(O, D)
            Dn = np.linalg.norm(D, axis=1)[:, None]
            with np.errstate(all="ignore"):
                DET = -(D @ n.T)
                U = (M @ s2.T - D @ c2.T) / DET
                V = (-(M @ s1.T) - D @ c1p.T) / DET
                T = (O @ n.T - k) / DET
                B = np.sqrt(np.maximum((O * O).sum(1)[:, None] + pp[None, :] - 2.0 * (O @ p0.T), 0.0))
                aD = np.abs(DET)
                dDet = K_ERR * (np.abs(D) @ cab.T)
                dU = K_ERR * Dn * S2 * (B + S1) / aD + np.abs(U) * dDet / aD
                dV = K_ERR * Dn * S1 * (B + S2) / aD + np.abs(V) * dDet / aD
                dT = K_ERR * S1 * S2 * (B + np.abs(T) * Dn) / aD + np.abs(T) * dDet / aD
                mb = np.maximum(EPS_B, dU + dV + K_ERR)
                W = 1.0 - U - V
                # fp32 overflow or underflow inside Moller-Trumbore (coordinates past ~2^42: |tvec| |s1| |s2| > FLT_MAX): the reference's
                # answer is its rounding, not the geometry's -- neither a robust hit nor a robust miss
                big = np.maximum(np.maximum(B * S1 * S2, Dn * S1 * S2), np.maximum(B * Dn * S2, B * Dn * S1))
                faithful = (big < 1e36) & (Dn * S1 * S2 > 1e-30)
                det_in = aD > DET_CUT * (1.0 + EPS_D) + dDet
                det_out = aD < DET_CUT * (1.0 - EPS_D) - dDet
                hit = faithful & det_in & (U > mb) & (V > mb) & (W > mb) & (T > 2.0 * dT)
                miss = faithful & (det_out | (U < -mb) | (U > 1.0 + mb) | (V < -mb) | (W < -mb) | (T < -dT))
                amb = ~hit & ~miss
                Th = np.where(hit, T, np.inf)
                j = np.argmin(Th, 1)
                r = np.arange(b - a)
                ts = Th[r, j]
                dts = np.where(np.isfinite(ts), dT[r, j], 0.0)
                lim = ts * (1.0 + EPS_T) + dts
                lo = np.where(np.isnan(T) | ~np.isfinite(T), -np.inf, T - dT)
                amb_near = (amb & (lo < lim[:, None])).any(1)
                rival = hit & (lo < lim[:, None])
                rival[r, j] = False
                rival = rival.any(1)
                tmr = tm[a:b]
                self.closest[a:b] = np.where(np.isfinite(ts), j, -1)
                self.t_closest[a:b] = ts
                self.closest_clear[a:b] = ~amb_near & ~rival
                self.reason[a:b] = np.where(amb_near, 1, np.where(rival, 2, 0))
                self.shadow_clear[a:b] = ~((hit | amb) & (lo < (tmr * (1.0 + EPS_T))[:, None])).any(1)
                exact = (aD >= DET_CUT) & (U >= 0) & (U <= 1) & (V >= 0) & (U + V <= 1) & (T > 0) & (T < tmr[:, None])
                self.shadow_hit_any[a:b] = exact.any(1)
                occ = hit & (T + dT < (tmr * (1.0 - EPS_T))[:, None])
                rr, tt = np.nonzero(occ)
                occ_r.append(rr + a); occ_tri.append(tt); occ_t.append(T[rr, tt])
                self.n_amb[a:b] = amb.sum(1)
        self.occ_r, self.occ_tri, self.occ_t = np.concatenate(occ_r), np.concatenate(occ_tri), np.concatenate(occ_t)
        with np.errstate(all="ignore"):
            inv = np.float32(1.0) / np.asarray(dirs, np.float32)
        self.crossing = np.isfinite(inv)              # axes the reference's slab can resolve (fp32 1/d finite)

    def _tol(self, rays, p):
        """Leaf-box margin: eps_p of the scene extent plus the fp32 resolution of the slab's (b - o) and of the hit point itself."""
        mag = np.abs(self.orig_abs[rays]).max(1) + np.abs(p).max(1)
        return EPS_P * self.extent + 2.0 * K_ERR * mag

    def verdict(self, d):
        """Per ray, for the tree in d: closest-hit and any-hit decisions, and the builder-coverage failures of robust hits."""
        lv = Leaves(d)
        nr = self.closest.size
        v = dict(closest=self.closest.copy(), ext_decided=np.zeros(nr, bool), sh_decided=np.zeros(nr, bool), blocked=np.zeros(nr, bool),
                 ext_face0=np.zeros(nr, bool), sh_face0=np.zeros(nr, bool), uncovered=[])
        h = np.nonzero(self.closest >= 0)[0]
        p = self.orig_abs[h] + self.t_closest[h, None] * self.dir[h]
        ok, cov, f0 = leaf_check(lv, self.closest[h], p, self._tol(h, p), self.crossing[h])
        v["ext_decided"][:] = self.closest_clear
        v["ext_decided"][h] &= ok
        v["ext_face0"][h] = f0 & self.closest_clear[h]
        for i in np.nonzero(~cov)[0][:8]:
            v["uncovered"].append((int(h[i]), int(self.closest[h[i]]), p[i].tolist(), lv.node[lv.of_tri[self.closest[h[i]]]].tolist()))
        # any hit: a robust occluder inside one of its leaves, or nothing robust / ambiguous below tMax
        r = self.occ_r
        if r.size:
            p = self.orig_abs[r] + self.occ_t[:, None] * self.dir[r]
            ok, cov, f0 = leaf_check(lv, self.occ_tri, p, self._tol(r, p), self.crossing[r])
            okr = np.zeros(nr, bool); okr[r[ok]] = True
            f0r = np.zeros(nr, bool); f0r[r[f0]] = True
            anyocc = np.zeros(nr, bool); anyocc[r] = True
            for i in np.nonzero(~cov)[0][:8]:
                v["uncovered"].append((int(r[i]), int(self.occ_tri[i]), p[i].tolist(), lv.node[lv.of_tri[self.occ_tri[i]]].tolist()))
        else:
            okr = f0r = anyocc = np.zeros(nr, bool)
        v["blocked"] = okr
        v["sh_decided"] = okr | (self.shadow_clear & ~anyocc)
        v["sh_face0"] = f0r & ~okr & ~v["sh_decided"]
        return v


# ---------------------------------------------------------------------------------------------------------------------------------
# rays: (orig, dir, tmax) fp32 arrays, per generator
def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _ulp(a, k):
    a = _f32(a)
    with np.errstate(over="ignore"):
        return np.nextafter(a, np.float32(np.inf) if k > 0 else np.float32(-np.inf)).astype(np.float32)


def _default_tmax(rng, n, extent, dirs):
    dn = np.linalg.norm(np.asarray(dirs, np.float64), axis=1)
    f = np.where(rng.rand(n) < 0.5, 4.0, rng.uniform(0.05, 1.0, n))
    with np.errstate(all="ignore"):
        t = f * 2.0 * extent / np.maximum(dn, 1e-30)
    return _f32(np.minimum(t, 1e30))


def ray_sets(P, leaves, n=1024, seed=11):
    """{generator: (orig, dir, tmax)} for the scene with positions P and (sbvh) leaves; ~n rays per generator."""
    rng = np.random.RandomState(seed)
    P = np.asarray(P, np.float64)
    lo, hi = P.min((0, 1)), P.max((0, 1))
    ext = float((hi - lo).max())
    cen = 0.5 * (lo + hi)
    P32 = P.astype(np.float32).astype(np.float64)
    cent = P32.mean(1)
    area = 0.5 * np.linalg.norm(np.cross(P32[:, 1] - P32[:, 0], P32[:, 2] - P32[:, 0]), axis=1)
    big = np.argsort(-area)[:max(8, P.shape[0] // 8)]
    out = {}

    def pick(m):
        return rng.randint(0, P.shape[0], m)

    # -- exactly-zero direction components, rays in the plane of flat boxes / quads, and the same rays 1 ulp off the plane
    o, dvec = [], []
    m = n // 8
    for axis in range(3):
        # one zero component: origin in the plane of a triangle whose normal is this axis (a flat box), direction in that plane
        flat = np.nonzero((np.ptp(P32[:, :, axis], 1) == 0) & (P32[:, 0, axis] > lo[axis]) & (P32[:, 0, axis] < hi[axis]))[0]
        src = flat if flat.size else pick(16)
        t = src[rng.randint(0, src.size, m)]
        bc = rng.dirichlet((1, 1, 1), m)
        org = (bc[:, :, None] * P32[t]).sum(1)
        org[:, axis] = P32[t, 0, axis]
        dd = rng.normal(size=(m, 3)); dd[:, axis] = np.where(rng.rand(m) < 0.5, 0.0, -0.0)
        o.append(org); dvec.append(dd)
        # two zero components: axis-parallel rays from outside onto the scene; a quarter of the origins on leaf-box faces
        q = rng.uniform(lo, hi, (m, 3))
        onf = rng.rand(m) < 0.25
        lf = rng.randint(0, leaves.lo.shape[0], m)
        for b in range(3):
            if b != axis:
                q[onf, b] = np.where(rng.rand(onf.sum()) < 0.5, leaves.lo[lf[onf], b], leaves.hi[lf[onf], b])
        sgn = np.where(rng.rand(m) < 0.5, 1.0, -1.0)
        q[:, axis] = np.where(sgn > 0, lo[axis] - 0.1 * ext, hi[axis] + 0.1 * ext)
        dd = np.zeros((m, 3)); dd[:, axis] = sgn
        for b in range(3):
            if b != axis:
                dd[:, b] = np.where(rng.rand(m) < 0.5, 0.0, -0.0)
        o.append(q); dvec.append(dd)
    o, dvec = _f32(np.concatenate(o)), _f32(np.concatenate(dvec))
    # the in-plane rays again, origin 1 ulp above and below the plane
    k = o.shape[0] // 8
    sel = rng.choice(o.shape[0], k, replace=False)
    up, dn = o[sel].copy(), o[sel].copy()
    zc = (dvec[sel] == 0)
    up[zc] = _ulp(up[zc], 1); dn[zc] = _ulp(dn[zc], -1)
    o = np.concatenate([o, up, dn]); dvec = np.concatenate([dvec, dvec[sel], dvec[sel]])
    out["zero_dir"] = (o, dvec, _default_tmax(rng, o.shape[0], ext, dvec))

    # -- aimed at shared edges and shared vertices: exactly, and 2e-5 ... 0.1 of the way to a triangle's centroid, to either side
    m = n // 7
    t = pick(m)
    e = rng.randint(0, 3, m)
    a, b = P32[t, e], P32[t, (e + 1) % 3]
    s = rng.uniform(0.1, 0.9, m)
    tgt = a + s[:, None] * (b - a)
    tgt = np.concatenate([tgt, P32[t, e]])                                     # + the vertices themselves
    tc = np.concatenate([t, t])
    off = rng.choice([0.0, 2e-5, -2e-5, 1e-4, -1e-4, 1e-3, -1e-3, 1e-2, -1e-2, 0.1], tgt.shape[0])
    inward = cent[tc] - tgt
    tgt = tgt + off[:, None] * inward
    src = cen + rng.normal(size=tgt.shape) * ext
    dd = tgt - src
    out["edges"] = (_f32(src), _f32(dd / np.linalg.norm(dd, axis=1, keepdims=True)), _f32(np.full(tgt.shape[0], 4.0 * ext)))

    # -- grazing rays: (a) 1e-1 ... 1e-4 rad off the plane of their target triangle, origin close to it; (b) |det| near the 1e-12 cut-off:
    #    unnormalised directions scaled so that det = f * 1e-12 at a steep angle (the cut-off compares |det|, which scales with |d|)
    m = n // 2
    t = big[rng.randint(0, big.size, 2 * m)]
    s1, s2 = P32[t, 1] - P32[t, 0], P32[t, 2] - P32[t, 0]
    nn = np.cross(s1, s2)
    nl = np.linalg.norm(nn, axis=1)
    nh = nn / nl[:, None]
    w = np.cross(nh, rng.normal(size=(2 * m, 3))); w /= np.linalg.norm(w, axis=1, keepdims=True)
    ang = 10.0 ** rng.uniform(-4, -1, 2 * m)
    side = np.where(rng.rand(2 * m) < 0.5, 1.0, -1.0)
    dd = np.where((np.arange(2 * m) < m)[:, None], w * np.cos(ang)[:, None] + (side * np.sin(ang))[:, None] * nh,
                  -side[:, None] * (nh + 0.3 * w))
    f = rng.choice([0.25, 0.5, 0.8, 1.25, 2.0, 4.0], 2 * m)
    det1 = np.abs((dd * nn).sum(1))
    scl = np.where(np.arange(2 * m) < m, 1.0, f * 1e-12 / det1)
    L = 2.0 * np.sqrt(area[t] + 1e-300)
    with np.errstate(all="ignore"):
        dn = np.linalg.norm(dd * scl[:, None], axis=1)
        scl = np.where((dn > 1e-30) & (4.0 * L / dn < 1e37), scl, 1.0)      # out of fp32 reach (the 2^61 scene): a plain steep ray
    dd = _f32(dd * scl[:, None])
    dn = np.linalg.norm(dd.astype(np.float64), axis=1)
    org = cent[t] - (L / dn)[:, None] * dd.astype(np.float64)
    out["grazing"] = (_f32(org), dd, _f32(4.0 * L / dn))

    # -- origins on leaf-box faces, inside leaf boxes, and beyond 2^26 with the scene near the origin (the per-ray `far` branch)
    m = n // 3
    lf = rng.randint(0, leaves.lo.shape[0], m)
    fo = rng.uniform(leaves.lo[lf], leaves.hi[lf])
    ax = rng.randint(0, 3, m)
    fo[np.arange(m), ax] = np.where(rng.rand(m) < 0.5, leaves.lo[lf, ax], leaves.hi[lf, ax])
    io = leaves.lo[lf] + rng.uniform(0.1, 0.9, (m, 3)) * (leaves.hi[lf] - leaves.lo[lf])
    far_t = big[rng.randint(0, big.size, m)]
    fdir = rng.normal(size=(m, 3)); fdir /= np.linalg.norm(fdir, axis=1, keepdims=True)
    farr = cent[far_t] + fdir * 1.5 * FAR_ORIGIN
    org = np.concatenate([fo, io, farr])
    tg = np.concatenate([cent[pick(2 * m)], cent[far_t]])
    dd = tg - org
    dd /= np.linalg.norm(dd, axis=1, keepdims=True)
    dd[:m] = np.where(rng.rand(m, 1) < 0.5, dd[:m], rng.normal(size=(m, 3)))
    out["origins"] = (_f32(org), _f32(dd), _f32(np.full(org.shape[0], 4.0 * (ext + 2.0 * FAR_ORIGIN))))

    # -- shadow rays ending on an occluder: tMax = its float64 distance, and 1 ulp either side (filled in by shadow_ulp_tmax)
    m = n // 3
    t = pick(m)
    tg = (rng.dirichlet((2, 2, 2), m)[:, :, None] * P32[t]).sum(1)
    org = cen + rng.normal(size=(m, 3)) * ext
    dd = tg - org
    out["shadow_ulp"] = (_f32(np.concatenate([org] * 3)), _f32(np.concatenate([dd] * 3)), None)

    # -- subnormal direction components (1 / d overflows) and unnormalised directions
    m = n // 2
    org = cen + rng.normal(size=(m, 3)) * ext
    dd = cent[pick(m)] - org
    ax = rng.randint(0, 3, m)
    sub = rng.choice([1e-40, -1e-40, 1e-45, -1e-45, 3e-39], m)
    dd[np.arange(m), ax] = sub
    scale = 10.0 ** rng.uniform(-3, 3, m)
    org2 = cen + rng.normal(size=(m, 3)) * ext
    dd2 = (cent[pick(m)] - org2) * scale[:, None]
    org, dd = np.concatenate([org, org2]), np.concatenate([dd, dd2])
    out["subnormal"] = (_f32(org), _f32(dd), _default_tmax(rng, 2 * m, ext, dd))

    # -- control: uniformly random rays through the scene's box
    m = n
    org = rng.uniform(lo - 0.25 * ext, hi + 0.25 * ext, (m, 3))
    dd = rng.normal(size=(m, 3))
    out["random"] = (_f32(org), _f32(dd / np.linalg.norm(dd, axis=1, keepdims=True)), _default_tmax(rng, m, ext, dd))
    return out


def shadow_ulp_tmax(P, orig, dirs):
    """tMax for the shadow_ulp rays: the float64 distance to their closest triangle rounded to fp32, then -1 ulp and +1 ulp (thirds)."""
    bf = BruteForce(P, orig, dirs, np.full(orig.shape[0], FLT_MAX, np.float32))
    t = np.where(np.isfinite(bf.t_closest), bf.t_closest, FLT_MAX).astype(np.float32)
    m = orig.shape[0] // 3
    t[m:2 * m] = _ulp(t[m:2 * m], -1)
    t[2 * m:] = _ulp(t[2 * m:], 1)
    return np.where(np.isfinite(t), t, np.float32(FLT_MAX)).astype(np.float32)


def all_rays(P, leaves, n=1024, seed=11):
    """ray_sets() with the shadow_ulp tMax filled in; every (orig, dir) finite."""
    rs = ray_sets(P, leaves, n, seed)
    o, d, _ = rs["shadow_ulp"]
    rs["shadow_ulp"] = (o, d, shadow_ulp_tmax(P, o, d))
    for k, (o, d, t) in rs.items():
        assert np.isfinite(o).all() and np.isfinite(d).all() and np.isfinite(t).all() and (t > 0).all(), k
        assert (np.abs(d).max(1) > 0).all(), k
    return rs


# ---------------------------------------------------------------------------------------------------------------------------------
# loading crafted rays into a context (OracleContext or HipContext)
def params(d, env):
    p = wire.default_params(32, 32, d.world_radius, d.tris.size)
    p["useAreaLight"], p["useEnvMap"] = 0, int(env)
    return p


def load_rays(ctx, orig, dirs, tmax, queue=None):
    """The rays become extension queue entries (orig, dir) and shadow queue entries (shadowOrig, shadowDir, shadowRayLen), one path each
    (queue: the paths to enqueue, default all)."""
    n = orig.shape[0]
    st = ctx.state_export()
    assert st.shape[1] >= n
    st[COL.ORIG:COL.ORIG + 3, :n] = orig.T
    st[COL.DIR:COL.DIR + 3, :n] = dirs.T
    st[COL.SHADOW_ORIG:COL.SHADOW_ORIG + 3, :n] = orig.T
    st[COL.SHADOW_DIR:COL.SHADOW_DIR + 3, :n] = dirs.T
    st[COL.SHADOW_LEN, :n] = tmax
    ctx.state_import(st)
    q = np.arange(n, dtype=np.uint32) if queue is None else np.asarray(queue, np.uint32)
    ctx.queue_write(Q.EXTENSION, q)
    ctx.queue_write(Q.SHADOW, q)
    cnt = np.array(ctx.get_counters(), copy=True)
    if hasattr(ctx, "finish"):
        ctx.finish()
    cnt = np.array(cnt, copy=True)
    cnt[Q.EXTENSION] = q.size
    cnt[Q.SHADOW] = q.size
    ctx.set_counters(cnt)


def hits(ctx, n):
    st = ctx.state_export()
    return st.view(np.int32)[COL.HIT_I][:n].copy(), st.view(np.uint32)[COL.SHADOW_BLOCKED][:n] != 0


def pair_t(P, orig, dirs, tri):
    """Float64 ray parameter of each ray's plane crossing with triangle tri[i] (Moller-Trumbore's t, no inside test), and BruteForce's
    estimate of the error of its fp32 evaluation."""
    P = np.asarray(P, np.float64)[tri]
    o, d = np.asarray(orig, np.float64), np.asarray(dirs, np.float64)
    s1, s2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    n = np.cross(s1, s2)
    S1, S2, B, Dn = (np.linalg.norm(a, axis=1) for a in (s1, s2, o - P[:, 0], d))
    with np.errstate(all="ignore"):
        det = np.abs((d * n).sum(1))
        t = ((P[:, 0] - o) * n).sum(1) / (d * n).sum(1)
        return t, K_ERR * S1 * S2 * (B + np.abs(t) * Dn) / det + np.abs(t) * K_ERR * Dn * S1 * S2 / det


def emulation_rays(orig, dirs, tmax):
    """tests/wide_analysis.cpp's ray layout: n x 8 floats {orig.xyz, tmax, dir.xyz, unused}."""
    r = np.zeros((orig.shape[0], 8), np.float32)
    r[:, 0:3] = orig; r[:, 3] = tmax; r[:, 4:7] = dirs
    return r
