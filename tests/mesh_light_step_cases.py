"""Crafted paths for the MESH instances of mk_next_vertex and mk_sample_bsdf (csrc/microkernel.hip) and a float64 restatement of what each
path must add to Ei, written from DESIGN.md 4.2.2 and not from the kernels; the closed form of a lamp over a floor.

  StepScene     MC.lamp_field(steps=...): the field of 259 lamps plus the named arrangements (a pick that rounds to 0 beside a dominant
                light, a lamp seen from its back, one half behind a plate, one before another, one behind a veil past 0.995 |L|, a triangle
                that gains its emission after the upload, a receiver of every BSDF type), its table from the host (the device's is pinned to
                those bytes by tests/test_gpu_mesh_lights.py) and the float64 geometry of every triangle.
  implicit_*    paths entering mk_next_vertex: rays aimed at interior points of chosen triangles; the nearest hit is
                traversal_cases.BruteForce's, the contribution T w Ke with the MIS weight of 4.2.2.
  sampled_*     paths entering mk_sample_bsdf on crafted hit records: the three draws in exact uint32, MR.pick, MR.sample64, the float64
                any-hit over [0, 0.995 |L|], (f, pdf) toward L from bsdf_cases.Restatement.
  classify      bsdf_cases' method and constants: JITTER re-evaluations with every fp32-computed intermediate moved by ULPS ulp; a case is
                DECIDED when no branch flips (nearest triangle and occlusion: BruteForce's robust verdicts), nothing leaves the fp32 range
                and the output spreads by at most MAX_SPREAD of its scale; its tolerance is TOL_SPREAD spread + TOL_FLOOR 2^-24 scale.
  lamp_floor_*  one black emissive triangle over a diffuse floor: Lambert's edge sum for the irradiance of a uniformly emitting polygon.
"""
import copy
import functools
import numpy as np
import bsdf_cases as bc
import mesh_light_cases as MC
import mesh_light_reference as MR
import traversal_cases as tc
from common import COL
from fluctus_amd import host, wire

F = np.float32
BELOW1 = np.nextafter(F(1.0), F(0.0))
EXTRA = 37                                       # numTasks = cases + 37: not a multiple of 64
MODES = [(1, 1), (1, 0), (0, 1)]                 # (sampleExpl, sampleImpl)
PH_NEXT_VERTEX, PH_SAMPLE_BSDF, PH_SPLAT = 0, 1, 4
NONSINGULAR = (bc.BXDF.DIFFUSE, bc.BXDF.GLOSSY, bc.BXDF.GGX_ROUGH_REFLECTION, bc.BXDF.GGX_ROUGH_DIELECTRIC)
EPS_SURF = bc.F32(1e-3)                          # orig = P - 1e-3 dir
SHORT = bc.F32(0.995)                            # the shadow ray stops at 0.995 |L|
UNDECIDED_CAP = 0.03


def f32(a):
    """fp32 values held in float64"""
    return np.asarray(a, np.float64).astype(F).astype(np.float64)


def _dot(a, b):
    return (a * b).sum(-1)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


class NoTextures:
    desc = np.zeros(0, wire.TEXDESC)

    def fetch(self, idx, uv):
        return np.full((uv.shape[0], 3), np.nan)


# ---------------------------------------------------------------------------------------------------------------------------------
# the scene
class StepScene:
    def __init__(self):
        self.names = {}
        self.d0, _, self.lamps = MC.lamp_field(steps=self.names)           # as uploaded
        self.d1 = copy.copy(self.d0)                                        # after update_triangles: one triangle has gained an emissive matId
        self.d1.tris = self.d0.tris.copy()
        self.gains = self.names["gains"][0]
        self.d1.tris["matId"][self.gains] = 1
        self.P = MR.positions(self.d1.tris)
        self.cross = np.cross(self.P[:, 1] - self.P[:, 0], self.P[:, 2] - self.P[:, 0])
        self.mat = self.d1.tris["matId"].astype(np.int64)
        self.ke = MR.ke_of(self.d1).astype(np.float64)
        self.rs = bc.Restatement(self.d1.materials, NoTextures())
        self.type = self.d1.materials["type"].astype(np.int64)
        self.table = host.mesh_light_table(self.d0)
        assert np.array_equal(self.table[0], self.lamps)

    def listed(self, tri, tab):
        """the light record of every triangle (-1: not in the list)"""
        tris = tab[0]
        k = np.searchsorted(tris, tri)
        k = np.minimum(k, tris.size - 1)
        return np.where(tris[k] == tri, k, -1)

    def quad_light(self):
        """the parametric quad, 0.2 below the lamp 'quad_lamp' and larger than it"""
        return dict(pos=(5.7, 1.5, 0.0), N=(0.0, -1.0, 0.0), right=(1.0, 0.0, 0.0), up=(0.0, 0.0, 1.0), size=(0.3, 0.3), E=(7.0, 6.0, 5.0))

    def params(self, n, mode, **kw):
        w = 128
        p = wire.default_params(w, (n + EXTRA + w - 1) // w, self.d0.world_radius, self.d0.tris.size)
        q = self.quad_light()
        al = p["areaLight"]
        for k in ("pos", "N", "right", "up", "E"):
            al[k]["x"], al[k]["y"], al[k]["z"] = q[k]
        al["size"] = q["size"]
        p["useEnvMap"], p["useAreaLight"], p["useRoulette"], p["maxBounces"] = 0, 0, 0, 8
        p["sampleExpl"], p["sampleImpl"] = mode
        for k, v in kw.items():
            p[k] = v
        return p


@functools.lru_cache(None)
def step_scene():
    return StepScene()


# ---------------------------------------------------------------------------------------------------------------------------------
# the classifier (bsdf_cases.Verdict's method on one (n, 3) output)
class Verdict:
    def __init__(self, fn, n, robust, seed=77):
        """fn(E) -> dict(out (n, 3) = prior + dEi, delta (n, 3), ...); robust: cases whose float64 hits bind the fp32 traversal"""
        with np.errstate(all="ignore"):
            E0 = bc.Eval(n)
            self.nom = fn(E0)
            rng = np.random.RandomState(seed)
            runs = []
            for _ in range(bc.JITTER):
                E = bc.Eval(n, rng)
                runs.append((fn(E), E))
            flip = E0.bad.copy() | ~np.asarray(robust, bool)
            for o, E in runs:
                flip |= E.bad
                assert len(E.branches) == len(E0.branches)
                for (i0, b0), (_, b1) in zip(E0.branches, E.branches):
                    flip[i0] |= b0 != b1
            out = self.nom["out"]
            spr = np.max([np.abs(o["out"] - out) for o, _ in runs], axis=0)
            scale = np.max(np.abs(out), axis=1, keepdims=True)
            finite = np.isfinite(out).all(1) & np.isfinite(spr).all(1)
            self.spread_rel = spr.max(1) / np.where(scale[:, 0] > 0, scale[:, 0], 1.0)
            self.tol = bc.TOL_SPREAD * spr + bc.TOL_FLOOR * 2.0 ** -24 * scale
            self.decided = ~flip & finite & (spr.max(1) <= bc.MAX_SPREAD * scale[:, 0])
        self.out, self.delta = out, self.nom["delta"]
        self.silent = self.decided & (self.delta == 0.0).all(1)             # the restatement says: Ei keeps its bits

    def ratio(self, got):
        """|got - out| / tol per case (the largest of the three components); meaningful on the decided cases"""
        with np.errstate(all="ignore"):
            err = np.abs(np.asarray(got, np.float64) - self.out)
            return np.where(err == 0.0, 0.0, err / self.tol).max(1)


def undecided_share(v, group):
    """{group: share of undecided cases}"""
    return {g: float((~v.decided[group == g]).mean()) for g in np.unique(group)}


# ---------------------------------------------------------------------------------------------------------------------------------
# A. the implicit hit
class ImplicitCases:
    """paths entering mk_next_vertex.  Arrays of length n: orig, dir (fp32 in float64), T, Ei (prior), lastPdfW, lastSpecular, len_before,
    target (the triangle aimed at), group, label.  `named`: the cases that must be decided."""

    def __init__(self, S, seed=21):
        rng = np.random.RandomState(seed)
        nm = S.names
        rows = []
        # lastPdfW: the three magnitudes, and exact values of a preceding BSDF sample (the diffuse and the glossy sampler of bsdf_cases)
        cs = bc.CaseSet()
        sel = np.nonzero((cs.group == "random") & np.isin(cs.type, NONSINGULAR))[0][:64]
        with np.errstate(all="ignore"):
            sampled, _, _ = cs.restatement().run(bc.Case(**{k: getattr(cs.case, k)[sel] for k in bc.Case.FIELDS}), bc.Eval(sel.size))
        sampled = f32(sampled["lastPdfW"][:, 0])
        sampled = sampled[np.isfinite(sampled) & (sampled > 1e-3) & (sampled < 1e3)]
        assert sampled.size >= 16
        PDFS = [1.0, 1e-6, 1e6]
        COS = [1.0, 0.7, 0.3, 0.1, 1e-2, 1e-3]

        def add(group, label, target, cos=None, side=1, lb=None, spec=None, pdf=None, zero_T=False, named=False):
            p = S.P[target]
            b = rng.dirichlet((1.0, 1.0, 1.0)) * 0.55 + 0.15                       # barycentrics >= 0.15: well inside
            X = b @ p
            n = _unit(S.cross[target])
            tng = _unit(p[1] - p[0]) * np.cos(a := rng.uniform(0, 2 * np.pi)) + np.cross(n, _unit(p[1] - p[0])) * np.sin(a)
            c = float(rng.choice(COS)) if cos is None else cos
            dist = rng.uniform(0.4, 1.5)
            o = X + dist * (side * c * n + np.sqrt(1.0 - c * c) * tng)
            o32 = f32(o)
            rows.append(dict(orig=o32, dir=f32(_unit(X - o32)), T=np.zeros(3) if zero_T else rng.uniform(0.2, 1.0, 3), Ei=rng.uniform(0.05, 1.0, 3),
                             lastPdfW=float(rng.choice(PDFS + [float(rng.choice(sampled))] * 3)) if pdf is None else pdf,
                             lastSpecular=int(rng.randint(2)) if spec is None else spec, len_before=int(rng.choice([0, 1, 3])) if lb is None else lb,
                             target=target, group=group, label=label, named=named, cos=c))

        def sweep(group, label, target, side=1, named=True):
            """the full grid of the path's own state on one target, at one ordinary incidence"""
            for lb in (0, 1, 3):
                for spec in (0, 1):
                    for pdf in PDFS + [float(sampled[0]), float(sampled[1])]:
                        add(group, label, target, cos=0.7, side=side, lb=lb, spec=spec, pdf=pdf, named=named)
            add(group, label + " T=0", target, cos=0.7, side=side, lb=1, spec=0, pdf=1.0, zero_T=True, named=named)

        k255, k256 = int(S.lamps[MC.SCAN_BLOCK - 1]), int(S.lamps[MC.SCAN_BLOCK])
        sweep("named", "light 0", int(S.lamps[0]))
        sweep("named", "light 255", k255)
        sweep("named", "light 256", k256)
        sweep("named", "pick = 0", nm["tiny"][0])
        sweep("named", "dominant", nm["dominant"][0])
        sweep("named", "last light", nm["last"][0])
        sweep("named", "back of a lamp", nm["back"][0], side=-1)
        sweep("named", "gains emission", S.gains)
        sweep("named", "lamp before a lamp", nm["front"][1])
        sweep("named", "plate before a lamp", nm["half_plate"][0])
        sweep("named", "no light", nm["receiver0"][0])
        # incidence from the normal down to cos = 1e-3, both sides, on large and small lamps
        for target in (nm["dominant"][1], nm["behind"][0], k255, k256):
            for c in COS:
                for side in (1, -1):
                    for lb, spec in ((1, 0), (3, 0), (0, 1)):
                        add("incidence", f"cos {c:g}", target, cos=c, side=side, lb=lb, spec=spec)
        # the lamps hidden from below (the ray meets what is before them), seen from below
        for name in ("half", "behind", "veiled", "quad_lamp"):
            for t in nm[name]:
                for _ in range(12):
                    add("hidden", name, t, cos=float(rng.uniform(0.5, 1.0)), side=1)
        # every kind of triangle at random: field lamps either side of the seam, Ke = 0 materials, the floor, the extras
        every = np.arange(S.P.shape[0])
        for target in rng.choice(every, 700):
            add("random", "random", int(target), side=int(rng.choice([1, -1])))
        self.n = len(rows)
        for k in ("orig", "dir", "T", "Ei"):
            setattr(self, k, f32([r[k] for r in rows]))
        self.lastPdfW = f32([r["lastPdfW"] for r in rows])
        for k in ("lastSpecular", "len_before", "target"):
            setattr(self, k, np.array([r[k] for r in rows], np.int64))
        self.group, self.label = np.array([r["group"] for r in rows]), np.array([r["label"] for r in rows])
        self.named = np.array([r["named"] for r in rows], bool)
        self.cos = np.array([r["cos"] for r in rows])
        # the float64 nearest hit of every ray, and whether it binds the fp32 traversal
        bf = tc.BruteForce(S.P, self.orig, self.dir, np.full(self.n, tc.FLT_MAX, F))
        v = bf.verdict(S.d0)
        self.hit, self.t_hit, self.robust = bf.closest, bf.t_closest, v["ext_decided"]
        # the parametric quad of the sub-case: wins where the ray meets it from its front before the triangle (margins: 1e-4 of its size)
        q = S.quad_light()
        qn, qp = np.array(q["N"]), np.array(q["pos"])
        den = _dot(self.dir, qn)
        with np.errstate(all="ignore"):
            tq = _dot(qp - self.orig, qn) / den
            X = self.orig + tq[:, None] * self.dir - qp
            a, b = np.abs(_dot(X, np.array(q["right"]))) / q["size"][0], np.abs(_dot(X, np.array(q["up"]))) / q["size"][1]
            inside, outside = (a < 1 - 1e-4) & (b < 1 - 1e-4), (a > 1 + 1e-4) | (b > 1 + 1e-4)
            front = den < -1e-6
            before = (tq > 1e-6) & (tq < np.where(self.hit >= 0, self.t_hit, np.inf) * (1 - 1e-5))
            self.quad_wins = front & before & inside
            self.quad_clear = self.quad_wins | (den > 1e-6) | outside | (tq < -1e-6) | (tq > np.where(self.hit >= 0, self.t_hit, np.inf) * (1 + 1e-5))

    def state(self, st):
        """write the paths into a reference-layout state (64, >= n) in place: phase MK_RT_NEXT_VERTEX; the padding paths wait for the splat"""
        n, u = self.n, st.view(np.uint32)
        assert st.shape[1] >= n + EXTRA
        st[COL.ORIG:COL.ORIG + 3, :n] = self.orig.T
        st[COL.DIR:COL.DIR + 3, :n] = self.dir.T
        st[COL.T:COL.T + 3, :n] = self.T.T
        st[COL.EI:COL.EI + 3, :n] = self.Ei.T
        st[COL.LAST_PDF_W, :n] = self.lastPdfW
        u[COL.LAST_SPECULAR, :n] = self.lastSpecular
        u[COL.PATH_LEN, :n] = self.len_before
        u[COL.SEED, :n] = np.arange(n) * 2654435761 % 2 ** 32
        u[COL.PHASE, :n] = PH_NEXT_VERTEX
        u[COL.PHASE, n:] = PH_SPLAT
        return st


def implicit_restatement(S, c, tab, mode, quad=False):
    """fn(E) of Verdict for the cases c under (sampleExpl, sampleImpl) = mode; quad: the parametric quad is on and wins where c.quad_wins"""
    expl, impl = mode
    _, _, pick, _ = tab
    pickable = bool((np.asarray(pick) > 0).any())
    n = c.n
    hit = c.hit >= 0
    tri = np.where(hit, c.hit, 0)
    k = S.listed(tri, tab)
    ke = S.ke[tri]
    emissive = hit & (ke > 0).any(1)
    len_after = c.len_before + 1
    counted = (len_after == 1) | bool(impl)
    P3 = S.P[tri]

    def fn(E):
        E.idx = np.arange(n)
        dirj = E.j(c.dir)
        cr = E.j(np.cross(E.j(P3[:, 1] - P3[:, 0]), E.j(P3[:, 2] - P3[:, 0])))
        ng = E.normalize(cr)
        side = E.br((_dot(ng, dirj) < 0.0) & emissive)
        contrib = emissive & side & counted
        if quad:
            contrib = contrib & ~c.quad_wins
        mis = contrib & bool(expl) & (len_after > 1) & (c.lastSpecular == 0) & pickable & (k >= 0)
        area = E.j(0.5 * np.sqrt(_dot(cr, cr)))
        pdfA = E.j(np.asarray(pick, np.float64)[np.maximum(k, 0)] / area)
        t = E.j(_dot(E.j(P3[:, 0] - c.orig), cr) / _dot(dirj, cr))             # the plane's t: the nominal value is the float64 hit's
        X = E.j(c.orig + E.j(t[:, None] * dirj))
        d = E.j(np.sqrt(_dot(X - c.orig, X - c.orig)))
        cos = _dot(E.normalize(-dirj), ng)
        pdfW = E.j(pdfA * E.j(d * d) / np.abs(cos))
        w = np.where(mis, E.j(c.lastPdfW / E.j(c.lastPdfW + pdfW)), 1.0)
        E.chk(np.where(mis, pdfW, 1.0))
        delta = np.where(contrib[:, None], E.j(E.j(c.T * w[:, None]) * ke), 0.0)
        return dict(out=c.Ei + delta, delta=delta, contrib=contrib, mis=mis, w=w)
    return fn


def implicit_verdict(S, c, tab, mode, quad=False):
    robust = c.robust & (c.quad_clear if quad else True)
    v = Verdict(implicit_restatement(S, c, tab, mode, quad), c.n, robust)
    if not quad:
        assert np.allclose(np.where(c.hit >= 0, c.t_hit, 0.0), np.where(c.hit >= 0, _plane_t(S, c), 0.0), rtol=1e-9, atol=1e-12)
    return v


def _plane_t(S, c):
    tri = np.maximum(c.hit, 0)
    return _dot(S.P[tri, 0] - c.orig, S.cross[tri]) / _dot(c.dir, S.cross[tri])


# ---------------------------------------------------------------------------------------------------------------------------------
# B. the sampled light
def advance(seed, draws):
    s = np.asarray(seed, np.uint64)
    for _ in range(draws):
        s = bc.hash_u32(s)
    return s.astype(np.uint32)


def draw_of(h):
    """the draw of a hashed seed h, as rand01 makes it"""
    return F(np.uint32(h)) * F(2.0 ** -32)


def reachable(v, below=False):
    """the smallest draw >= v that a seed can give, or (below) the largest < v: a draw is (float)h 2^-32 for an integer h, so an fp32 under
    2^-9 is in general no draw, and above 2^-8 the neighbouring draw is the neighbouring float"""
    v = F(v)
    h = float(v) * 2.0 ** 32
    if not below:
        r = draw_of(min(int(np.ceil(h)), 0xFFFFFFFF))
        assert r >= v and (r == v or h != int(h))
        return r
    cands = [draw_of(max(int(np.ceil(h)) - 1, 0)), draw_of(int(float(np.nextafter(v, F(0.0))) * 2.0 ** 32))]
    r = max(c for c in cands if c < v)
    assert r >= np.nextafter(v, F(0.0)) or v - r <= F(2.0 ** -32)
    return r


class SampledCases:
    """paths entering mk_sample_bsdf with a crafted hit record: P on a receiver, the state's normal N (turned away on a back-face case: the
    kernel turns it toward the ray), dir, the receiver's material and triangle, T, the prior Ei and a seed chosen for its draws."""

    def __init__(self, S, tab, seed=22):
        rng = np.random.RandomState(seed)
        nm = S.names
        tris, cdf, pick, _ = tab
        n_l = tris.size
        lastpick = int(np.nonzero(pick > 0)[0][-1])
        rows = []
        UP = np.array([0.0, 1.0, 0.0])

        def receiver_point(j):
            """a point well inside receiver j (the quad of BSDF type j beside the floor; -1: the floor under the field)"""
            if j < 0:
                return np.array([rng.uniform(-1.8, 1.8), 0.0, rng.uniform(-1.8, 1.8)]), 0, 0
            t = nm[f"receiver{j}"][int(rng.randint(2))]
            b = rng.dirichlet((1.0, 1.0, 1.0)) * 0.7 + 0.1
            return b @ S.P[t], t, int(S.mat[t])

        def add(group, label, j, seed, N=UP, back=False, cos=None, zero_T=False, named=False):
            P, t, m = receiver_point(j)
            N = _unit(N(P) if callable(N) else N)
            c = float(rng.uniform(0.2, 1.0)) if cos is None else cos
            while True:                                                           # the ray arrives from above the receiver's plane and before N
                d = -(c * N + np.sqrt(1.0 - c * c) * _unit(np.cross(N, rng.normal(size=3))))
                if d[1] < -0.05:
                    break
            rows.append(dict(P=f32(P), N=f32(-N if back else N), dir=f32(d), mat=m, hitI=t, T=np.zeros(3) if zero_T else rng.uniform(0.2, 1.0, 3),
                             Ei=rng.uniform(0.01, 0.2, 3), seed=int(seed), group=group, label=label, named=named, back=back))

        def r0_in(k, u=None):
            """an fp32 r0 that picks light k: inside [cdf[k - 1], cdf[k])"""
            lo = float(cdf[k - 1]) if k else 0.0
            v = F(lo + (rng.uniform(0.05, 0.95) if u is None else u) * float(pick[k]))
            assert MR.pick(cdf, pick, v) == k
            return v

        def rnd():
            return int(rng.randint(0, 2 ** 32, dtype=np.uint64))
        k_of = {name: [int(np.searchsorted(tris, t)) for t in nm[name]] for name in ("back", "half", "front", "behind", "veiled", "quad_lamp", "tiny", "dominant", "last")}
        self.k_of = k_of
        # the pick's edges
        edges = [("r0 = 0", F(0.0)), ("r0 = 1", F(1.0)), ("r0 = 1 - ulp", F(1.0))]
        for k in (0, MC.SCAN_BLOCK - 1, MC.SCAN_BLOCK, n_l - 1):
            edges += [(f"r0 = cdf[{k}]", cdf[k]), (f"r0 = cdf[{k}] - ulp", cdf[k])]
        kt = k_of["tiny"][0]
        assert pick[kt] == 0 and pick[kt + 1] > 0 and pick[n_l - 1] == 0 and lastpick == k_of["dominant"][1]
        edges += [("r0 = cdf[pick = 0]", cdf[kt]), ("r0 = cdf[pick = 0] - ulp", cdf[kt])]
        self.edge_r0 = {}
        for label, v in edges:
            r = reachable(v, below=label.endswith("- ulp"))
            self.edge_r0[label] = r
            for j in (0, 1, 2, 3):
                add("pick edges", label, j, bc.seed_for_draw(1, r), named=True)
        # r1 and r2 at 0 and at the largest float below 1, on lights of every size
        for draw, name in ((2, "r1"), (3, "r2")):
            for v, vl in ((F(0.0), "0"), (BELOW1, "below 1")):
                for j in (0, 1, 2, 3, -1):
                    for _ in range(6):
                        add("r1 r2 edges", f"{name} = {vl}", j, bc.seed_for_draw(draw, v), named=(j >= 0))
        # the arrangements, each from every non-singular receiver
        for name in ("back", "half", "front", "behind", "veiled", "quad_lamp", "dominant"):
            for k in k_of[name]:
                for j in (0, 1, 2, 3):
                    for _ in range(8):
                        add("arrangements", name, j, bc.seed_for_draw(1, r0_in(k)))
        # L below the receiver's horizon: the state's normal leans 50 -- 80 degrees over, the lights stay above the geometry
        for _ in range(80):
            a, ph = np.radians(rng.uniform(50.0, 80.0)), rng.uniform(0, 2 * np.pi)
            add("horizon", "leaning normal", int(rng.randint(4)), rnd(), N=(np.sin(a) * np.cos(ph), np.cos(a), np.sin(a) * np.sin(ph)))
        centre = S.P[nm["dominant"]].mean((0, 1))
        for i in range(80):                                                       # ... away from the dominant light, which is the one picked

            def away(P, a=np.radians(rng.uniform(60.0, 80.0))):
                h = _unit((P - centre) * (1.0, 0.0, 1.0))
                return np.sin(a) * h + np.cos(a) * UP
            add("horizon", "leaning away", 1 + i % 3, bc.seed_for_draw(1, r0_in(k_of["dominant"][i % 2])), N=away)
        # a back-face receiver: the normal arrives turned away from the ray
        for _ in range(120):
            add("back face", "back face", int(rng.randint(4)), rnd(), back=True)
        for j in (0, 1, 2, 3):
            add("back face", "back face, dominant", j, bc.seed_for_draw(1, r0_in(k_of["dominant"][0])), back=True, named=True)
            add("T = 0", "T = 0", j, bc.seed_for_draw(1, r0_in(k_of["dominant"][0])), zero_T=True, named=True)
        # the field's own lamps, either side of the seam, from the floor under them
        for k in list(range(0, n_l, 7)) + [MC.SCAN_BLOCK - 2, MC.SCAN_BLOCK - 1, MC.SCAN_BLOCK, MC.SCAN_BLOCK + 1]:
            if pick[k] > 0:
                for _ in range(4):
                    add("field", "field", -1, bc.seed_for_draw(1, r0_in(k)))
        for _ in range(300):
            add("random", "random", int(rng.randint(-1, 4)), rnd())
        # singular receivers: no draw, no ray
        for j in (4, 5):
            for _ in range(40):
                add("singular", "singular", j, rnd())
        self.n = len(rows)
        for k in ("P", "N", "dir", "T", "Ei"):
            setattr(self, k, f32([r[k] for r in rows]))
        for k in ("mat", "hitI"):
            setattr(self, k, np.array([r[k] for r in rows], np.int64))
        self.seed = np.array([r["seed"] for r in rows], np.uint64)
        self.group, self.label = np.array([r["group"] for r in rows]), np.array([r["label"] for r in rows])
        self.named = np.array([r["named"] for r in rows], bool)
        self.back = np.array([r["back"] for r in rows], bool)
        self.uv = np.tile(f32([0.25, 0.75]), (self.n, 1))
        self.singular = ~np.isin(S.type[self.mat], NONSINGULAR)
        assert np.array_equal(self.back, _dot(self.N, self.dir) > 0)

    def state(self, st, seed=None):
        n, u = self.n, st.view(np.uint32)
        assert st.shape[1] >= n + EXTRA
        st[COL.P:COL.P + 3, :n] = self.P.T
        st[COL.N:COL.N + 3, :n] = self.N.T
        st[COL.UV:COL.UV + 2, :n] = self.uv.T
        st[COL.DIR:COL.DIR + 3, :n] = self.dir.T
        st[COL.T:COL.T + 3, :n] = self.T.T
        st[COL.EI:COL.EI + 3, :n] = self.Ei.T
        st[COL.HIT_T, :n] = 1.0
        st[COL.LAST_PDF_W, :n] = 1.0
        u[COL.SEED, :n] = (self.seed if seed is None else seed).astype(np.uint32)
        u[COL.MAT_ID, :n] = self.mat
        u[COL.HIT_I, :n] = self.hitI
        u[COL.AREA_LIGHT_HIT, :n] = 0
        u[COL.PATH_LEN, :n] = 1
        u[COL.LAST_SPECULAR, :n] = 0
        u[COL.FIRST_DIFFUSE, :n] = 0
        u[COL.PHASE, :n] = PH_SAMPLE_BSDF
        u[COL.PHASE, n:] = PH_SPLAT
        return st


class SampledGeometry:
    """what does not depend on the mode: the draws, the light, the point, the shadow ray and its float64 any-hit.  first: how many draws of
    the stream other lights consume before the mesh lights' three."""

    def __init__(self, S, c, tab, first=0):
        tris, cdf, pick, _ = tab
        s = advance(c.seed, first).astype(np.uint64)
        self.r0, s = bc.rand01(s)
        self.r1, s = bc.rand01(s)
        self.r2, s = bc.rand01(s)
        self.k = MR.pick(cdf, pick, self.r0).astype(np.int64)
        self.tri = tris[self.k].astype(np.int64)
        self.point, _ = MR.sample64(S.P[self.tri], self.r1, self.r2)
        self.orig = c.P - EPS_SURF * c.dir
        L = self.point - self.orig
        self.lenL = np.sqrt(_dot(L, L))
        self.L = L / self.lenL[:, None]
        bf = tc.BruteForce(S.P, self.orig, self.L, SHORT * self.lenL)
        v = bf.verdict(S.d0)
        self.occluded, self.robust = v["blocked"], v["sh_decided"] | c.singular
        assert not (self.occluded & ~bf.shadow_hit_any).any()


def sampled_restatement(S, c, tab, g, mode):
    expl, impl = mode
    tris, cdf, pick, _ = tab
    n = c.n
    active = bool(expl) & ~c.singular
    P3 = S.P[g.tri]
    ke = S.ke[g.tri]
    pk = np.asarray(pick, np.float64)[g.k]
    Nn = np.where(c.back[:, None], -c.N, c.N)

    def fn(E):
        E.idx = np.arange(n)
        dirj = E.j(c.dir)
        point = E.j(g.point)
        orig = E.j(c.P - E.j(EPS_SURF * dirj))
        L = E.j(point - orig)
        lenL = E.j(np.sqrt(_dot(L, L)))
        Ln = E.normalize(L)
        cr = E.j(np.cross(E.j(P3[:, 1] - P3[:, 0]), E.j(P3[:, 2] - P3[:, 0])))
        ng = E.normalize(cr)
        cosLight = np.fmax(_dot(ng, -Ln), 0.0)
        lit = E.br(active & ~g.occluded & (cosLight > 0.0))
        Nj = E.j(Nn)
        above = E.br(lit & (_dot(Ln, Nj) > 0.0))
        cosTh = np.fmax(_dot(Ln, Nj), 0.0)
        f, bpdf = np.zeros((n, 3)), np.zeros(n)
        for t in NONSINGULAR:
            idx = np.nonzero((S.type[c.mat] == t) & active & ~g.occluded)[0]
            if not idx.size:
                continue
            E.idx = idx
            cc = bc.Case(P=c.P[idx], N=Nj[idx], uv=c.uv[idx], dir=dirj[idx], L=Ln[idx], T=c.T[idx], seed=c.seed[idx], backface=c.back[idx], mat=c.mat[idx])
            with E.only(lit[idx]):                                                # (an unlit path's BSDF decides nothing)
                ff, pp = getattr(S.rs, S.rs.FN[t])(E, cc, S.rs._mat_arrays(E, cc.mat), dirj[idx], Ln[idx], c.seed[idx].astype(np.uint64))[:2]
            f[idx], bpdf[idx] = ff * np.ones((1, 3)), np.fmax(0.0, pp)
        E.idx = np.arange(n)
        area = E.j(0.5 * np.sqrt(_dot(cr, cr)))
        pdfA = E.j(pk / area)
        pdfW = E.j(pdfA * E.j(lenL * lenL) / np.where(cosLight > 0, cosLight, 1.0))
        E.chk(np.where(lit, pdfW, 1.0))
        weight = E.j(pdfW / E.j(pdfW + bpdf)) if impl else np.ones(n)
        delta = np.where(lit[:, None], E.j(f * c.T * ke * (weight * cosTh / pdfW)[:, None]), 0.0)
        return dict(out=c.Ei + delta, delta=delta, lit=lit, above=above, cosLight=cosLight, weight=weight)
    return fn


def sampled_verdict(S, c, tab, g, mode):
    return Verdict(sampled_restatement(S, c, tab, g, mode), c.n, g.robust | (not mode[0]))


# ---------------------------------------------------------------------------------------------------------------------------------
# the closed form: one black emissive triangle over a diffuse floor
LF_W, LF_H = 48, 32
LF_KD, LF_KE = 0.8, 3.0
LF_LAMP = np.array([[-2.0, 0.75, -1.5], [2.0, 0.75, -1.5], [0.0, 0.75, 2.0]])      # (p1 - p0) x (p2 - p0) points down
LF_CAMERA = dict(pos=(0.0, 0.5, 0.0), target=(0.0, 0.0, 0.0), up=(0.0, 0.0, -1.0), fov=60.0)
LF_SUBPIXEL_REL = 1e-5                            # how far the truth of a tile may still move between a 4 x 4 and an 8 x 8 sub-pixel grid
LF_ALBEDO = LF_KD ** 2.2                          # the diffuse BSDF's albedo is pow(Kd, 2.2) (bsdf_cases.Restatement._albedo)


def lamp_floor_scene():
    mats = [common_diffuse(LF_KD), MC.emissive((LF_KE,) * 3)]
    tris = MC.quad((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), 2.0, 2.0, 0, (0.0, 1.0, 0.0)) + [MC.tri(*LF_LAMP, 1)]
    assert np.cross(LF_LAMP[1] - LF_LAMP[0], LF_LAMP[2] - LF_LAMP[0])[1] < 0
    return MC.scene(tris, mats)


def common_diffuse(kd):
    import common
    return common.make_material(bc.BXDF.DIFFUSE, kd=(kd,) * 3, ks=(0.0, 0.0, 0.0))


def lamp_floor_params(d, mode):
    p = wire.default_params(LF_W, LF_H, d.world_radius, d.tris.size)
    wire.look_at(p, LF_CAMERA["pos"], LF_CAMERA["target"], fov=LF_CAMERA["fov"], up=LF_CAMERA["up"])
    p["camera"]["apertureSize"] = 0.0
    p["useEnvMap"], p["useAreaLight"], p["useRoulette"], p["maxBounces"] = 0, 0, 0, 1
    p["sampleExpl"], p["sampleImpl"] = mode
    return p


def polygon_irradiance(x, n, verts):
    """Lambert's edge sum: the irradiance at x (normal n) from a polygon of unit radiance seen in full, E = 1/2 |sum_i theta_i (gamma_i . n)|
    with theta_i the angle between the directions to vertices i and i + 1 and gamma_i the unit normal of the plane through x and that edge"""
    x = np.asarray(x, np.float64)
    v = _unit(np.asarray(verts, np.float64)[None, :, :] - x[:, None, :])
    w = np.roll(v, -1, axis=1)
    theta = np.arccos(np.clip(_dot(v, w), -1.0, 1.0))
    gamma = _unit(np.cross(v, w))
    return 0.5 * np.abs((theta * _dot(gamma, np.asarray(n, np.float64))).sum(1))


def quadrature_irradiance(x, n, tri, m=96):
    """the same by Gauss-Legendre quadrature (m x m nodes) of cos cos' / d^2 over the triangle y = (1 - s) p0 + s (1 - b) p1 + s b p2,
    dA = 2 area s ds db: the integrand is smooth, the lamp being 0.75 above the floor"""
    p0, p1, p2 = np.asarray(tri, np.float64)
    u, wu = np.polynomial.legendre.leggauss(m)
    u, wu = 0.5 * (u + 1.0), 0.5 * wu
    s, b = (a.ravel() for a in np.meshgrid(u, u, indexing="ij"))
    wgt = (wu[:, None] * wu[None, :]).ravel() * s
    y = (1 - s)[:, None] * p0 + (s * (1 - b))[:, None] * p1 + (s * b)[:, None] * p2
    ng = _unit(np.cross(p1 - p0, p2 - p0))
    area = 0.5 * np.linalg.norm(np.cross(p1 - p0, p2 - p0))
    out = np.zeros(len(x))
    for i, xi in enumerate(np.asarray(x, np.float64)):
        d = y - xi
        r2 = _dot(d, d)
        out[i] = 2.0 * area * np.sum(wgt * np.maximum(_dot(d, n), 0.0) * np.maximum(-_dot(d, ng), 0.0) / (r2 * r2))
    return out


def lamp_floor_truth(p, s):
    """(H, W) luminance each pixel converges to: albedo / pi * Ke * E(x) averaged over s x s sub-pixel positions of the reference's camera
    (x / width and y / height to [-1, 1], times tan(fov / 2), x by the aspect too; the ray from the eye through pos + right X + up Y + dir)"""
    cam = p["camera"]
    v = lambda k: np.array([cam[k]["x"], cam[k]["y"], cam[k]["z"]], np.float64)
    W, H = int(p["width"]), int(p["height"])
    sub = (np.arange(s) + 0.5) / s
    px = (np.arange(W)[:, None] + sub[None, :]).ravel() / W
    py = (np.arange(H)[:, None] + sub[None, :]).ravel() / H
    sc = np.tan(0.5 * float(cam["fov"]) * np.pi / 180.0)
    X, Y = np.meshgrid((2 * px - 1) * (W / H) * sc, (2 * py - 1) * sc)
    d = v("right")[None, None] * X[..., None] + v("up")[None, None] * Y[..., None] + v("dir")[None, None]
    t = -v("pos")[1] / d[..., 1]                                   # the floor is y = 0
    assert (t > 0).all()
    x = v("pos") + t[..., None] * d
    assert (np.abs(x[..., 0]) < 1.9).all() and (np.abs(x[..., 2]) < 1.9).all(), "the camera sees only the floor"
    E = polygon_irradiance(x.reshape(-1, 3), (0.0, 1.0, 0.0), LF_LAMP).reshape(x.shape[:2])
    return (LF_ALBEDO / np.pi * LF_KE * E).reshape(H, s, W, s).mean((1, 3))


def tile_means(img, tile=8):
    H, W = img.shape
    return img.reshape(H // tile, tile, W // tile, tile).mean((1, 3))
