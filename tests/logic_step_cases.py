"""Crafted paths for the logic step (csrc/logic.hip k_logic, oracle/wf_oracle.cpp) and a float64 restatement of what the reference's kernel
does with each of them, written from the reference's src/wf_logic.cl:14-314 and src/env_map.cl:14-107 (utils.cl:149-182 tangentSpaceNormal,
:197-200 pdfAtoW, :226-234 sampleAreaLight, :237-240 luminance) and not from logic.hip.

  LogicScene    a few hundred triangles with per-vertex normals and uvs (common.small_mesh_scene), the six BSDF types plus normal-mapped
                materials on bsdf_cases' 3 x 5 texture, one triangle whose uv determinant is exactly 0, a parametric quad, and two
                environment maps built in memory (16 x 8 and 12 x 5: a dominant texel, black texels, random pole rows).
  CONFIGS       what a run fixes for all of its paths: which lights are on, the map, envMapStrength, roulette.  Every case set is built
                per configuration (the seeds are chosen for its draw order) and run in the three sampling modes.
  Cases         committed hit records and path state, one path per pixel (pixelIndex = path id): the groups termination, miss, quad hit,
                consume, NEE environment, NEE quad, normal map, and a random fill of each.  A `named` case must be decided; the named cases
                of the groups that are not about a light sample sit on a mirror, so that no sample's cosine rides along.
  RayCases      the RAW chain: rays aimed at interior points of triangles, at smooth-normal vertices, at the quad (nothing before it, the
                ground before it, a sphere behind it) and at the sky; the float64 nearest hit is traversal_cases.BruteForce's on its robust
                rays, the commit (P = o + t d, barycentric normal and uv, matId, the implicit quad) is restated with Moller-Trumbore's
                operations under the same jitter, and the logic step of `restatement` follows.  One packing has cases + 37 paths, the other
                is padded with inert paths (T = 0, pathLen 0) to a multiple of 256 for the regrouped instance.
  restatement   wf_logic.cl line by line in float64.  The draws are exact uint32 (bsdf_cases.rand01).  Integer decisions the kernel takes on
                fp32 values it can form exactly are restated in fp32: the alias index floor(r w h) and its clamp, r - i < prob[i], the
                light choice, the roulette comparison against a clamped contProb, the normal map's texel (bsdf_cases.texel_coord).  The
                pdf texel floor(u w) of envMapPdf is taken on a u that comes out of atan2 / acos: it is a branch under the classifier's
                jitter.  The bilinear lookup (OpenCL 1.2 s8.2, the sampler of env_map.cl:10) is continuous in (u, v) across texel borders,
                so its floor is no branch: either side gives the same value.
  Verdict       bsdf_cases' classifier and constants (JITTER, ULPS, MAX_SPREAD, TOL_SPREAD, TOL_FLOOR) over every logic-owned float
                output, mesh_light_step_cases.UNDECIDED_CAP per group.
  check         the assertions of the GPU test on one run (state out, framebuffer, counters, queues); tests/test_logic_steps.py makes them
                on the oracle first.  No constant had to move: the oracle's largest error / tolerance is 0.11 on the committed records and
                0.17 behind the commit (the device's figures are the same: its bits are the oracle's).

Divergences the restatement found (oracle and device both off float64 on decided cases; DESIGN.md 'atan2f_'): misses along +-y and toward
(-0, 0, 1) looked up another column of the map -- include/flx_math.h atan2f_ returned 0 for atan2(+-0, -0) and +pi for atan2(-0, x < 0) where
OpenCL's atan2 (env_map.cl:19) gives +-pi and -pi.  Fixed in flx_math.h; the miss group's axis cases and test_atan2_at_the_signed_zeros stay.
The quad is intersected only with sampleImpl on (wf_extrays.cl:29): a first draft of the commit missed that -- a restatement error.

Named quirk: a miss toward exactly (0, -1, 0) with MIS on.  acos(-1) / pi is 1.0f and sin(1.0f pi_f) is -8.74e-8, so the sinTh == 0 guard of
envMapPdf does not fire and the pdf is a huge NEGATIVE number: Ei comes back negative.  The reference's arithmetic, kept for parity
(DESIGN.md, next to the texel-wrap note); the classifier leaves the case undecided (sin crosses zero under the jitter) and the tests pin it
to the oracle's bits.
"""
import functools
import numpy as np
import bsdf_cases as bc
import common
from common import COL, Q
from mesh_light_step_cases import UNDECIDED_CAP, EXTRA, MODES, BELOW1, f32, draw_of       # (the cap and the modes: for the tests, through this module)
from fluctus_amd import host, wire

F = np.float32
PI, TWO_PI = bc.PI, bc.TWO_PI
EPS_SURF = bc.F32(1e-3)                          # orig = P - 1e-3 dir (wf_logic.cl:184)
SHORT = bc.F32(0.995)                            # the quad's shadow ray stops at 0.995 |L| (:272)
LUM = (bc.F32(0.212671), bc.F32(0.715160), bc.F32(0.072169))
CONT_LO, CONT_HI = bc.F32(0.01), 0.5
NONSINGULAR = (bc.BXDF.DIFFUSE, bc.BXDF.GLOSSY, bc.BXDF.GGX_ROUGH_REFLECTION, bc.BXDF.GGX_ROUGH_DIELECTRIC)
MAX_BOUNCES = 4
LIST_OF = {bc.BXDF.DIFFUSE: Q.DIFFUSE, bc.BXDF.GLOSSY: Q.GLOSSY, bc.BXDF.GGX_ROUGH_REFLECTION: Q.GGX_REFL,
           bc.BXDF.GGX_ROUGH_DIELECTRIC: Q.GGX_REFR, bc.BXDF.IDEAL_REFLECTION: Q.DELTA, bc.BXDF.IDEAL_DIELECTRIC: Q.DELTA}
CONFIGS = {"both": dict(useEnvMap=1, useAreaLight=1, envMapStrength=1.5, useRoulette=1, env=0),
           "env": dict(useEnvMap=1, useAreaLight=0, envMapStrength=1.0, useRoulette=0, env=1),
           "quad": dict(useEnvMap=0, useAreaLight=1, envMapStrength=1.0, useRoulette=1, env=0)}
QUAD = dict(pos=(0.25, 2.5, 0.125), N=(0.0, -1.0, 0.0), right=(1.0, 0.0, 0.0), up=(0.0, 0.0, 1.0), size=(0.5, 0.25), E=(7.0, 6.0, 5.0))
# the logic-owned float columns of the reference layout
RAW_OUT = {"P": (COL.P, 3), "uv": (COL.UV, 2), "hitT": (COL.HIT_T, 1)}          # what the commit of a RAW hit record adds (continuing paths)
FLOAT_OUT = {"Ei": (COL.EI, 3), "T": (COL.T, 3), "N": (COL.N, 3), "shadowOrig": (COL.SHADOW_ORIG, 3), "shadowDir": (COL.SHADOW_DIR, 3),
             "shadowRayLen": (COL.SHADOW_LEN, 1), "lastPdfDirect": (COL.LAST_PDF_DIRECT, 1), "lastEmission": (COL.LAST_EMISSION, 3),
             "lastCosTh": (COL.LAST_COS_TH, 1), "lastLightPickProb": (COL.LAST_PICK_PROB, 1)}
SAMPLE_OUT = ("shadowOrig", "shadowDir", "shadowRayLen", "lastPdfDirect", "lastEmission", "lastCosTh", "lastLightPickProb")


def _dot(a, b):
    return (a * b).sum(-1)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


# ---------------------------------------------------------------------------------------------------------------------------------
# the scene
def _env_rgb(w, h, seed):
    """a dominant texel, black texels (also in the pole rows), both pole rows non-uniform"""
    rng = np.random.RandomState(seed)
    img = rng.uniform(0.05, 1.0, (h, w, 3))
    img[h // 2 - 1, w // 3] = (400.0, 300.0, 200.0)
    black = [(0, 1), (h - 1, w - 2), (h // 2, 0), (h // 2, w - 1), (1, w // 2), (1, w // 2 + 1)]
    for j, i in black:
        img[j, i] = 0.0
    return img.astype(F), (h // 2 - 1) * w + w // 3, [j * w + i for j, i in black]


class LogicScene:
    def __init__(self, all_diffuse=False):
        d = common.small_mesh_scene(n=4, mats=9)
        self.FLAT = 5                                                    # a triangle whose three uvs are equal: determinant exactly 0
        for v in ("v1", "v2"):
            d.tris[v]["t"][self.FLAT] = d.tris["v0"]["t"][self.FLAT]
        mk = common.make_material
        B = bc.BXDF
        mats = [mk(B.DIFFUSE, kd=(0.64, 0.64, 0.64)), mk(B.DIFFUSE, kd=(0.7, 0.3, 0.2), map_kd=0),
                mk(B.GLOSSY, kd=(0.2, 0.5, 0.7), ks=(0.3, 0.3, 0.3), ns=300.0, ni=1.5, map_n=1), mk(B.DIFFUSE, kd=(0.5, 0.5, 0.5)),
                mk(B.GLOSSY, kd=(0.6, 0.2, 0.2), ks=(0.4, 0.4, 0.4), ns=80.0, ni=1.5), mk(B.GGX_ROUGH_REFLECTION, ks=(0.9, 0.8, 0.5), ns=60.0, ni=1.5),
                mk(B.IDEAL_REFLECTION, ks=(0.9, 0.9, 0.9)), mk(B.GGX_ROUGH_DIELECTRIC, ks=(0.95, 0.95, 0.95), ns=400.0, ni=1.5),
                mk(B.IDEAL_DIELECTRIC, ks=(0.9, 0.95, 1.0), ni=1.5), mk(B.DIFFUSE, kd=(0.4, 0.6, 0.5), map_n=1),
                mk(B.IDEAL_REFLECTION, ks=(0.8, 0.8, 0.8), map_n=1)]
        d.materials = np.array(mats, wire.MATERIAL)
        if all_diffuse:                                                  # the same surfaces, every one of them diffuse (textures and normal maps stay)
            d.materials["type"] = B.DIFFUSE
        self.MAPPED = (2, 9, 10)
        self.tex = bc.Textures(bc.TEX_SIZES)
        d.texdesc, d.texdata = self.tex.desc, self.tex.data
        host.build_bvh(d, "sbvh")
        self.d = d
        self.type = d.materials["type"].astype(np.int64)
        self.mapN = d.materials["map_N"].astype(np.int64)
        t = d.tris
        xyz = lambda a: np.stack([a["x"], a["y"], a["z"]], -1).astype(np.float64)
        self.P = np.stack([xyz(t[v]["p"]) for v in ("v0", "v1", "v2")], 1)
        self.Nv = np.stack([xyz(t[v]["n"]) for v in ("v0", "v1", "v2")], 1)
        self.UV = np.stack([np.stack([t[v]["t"]["x"], t[v]["t"]["y"]], -1).astype(np.float64) for v in ("v0", "v1", "v2")], 1)
        self.envs, self.dominant, self.black = [], [], []
        for (w, h), seed in (((16, 8), 5), ((12, 5), 6)):
            rgb, dom, black = _env_rgb(w, h, seed)
            self.envs.append(host.envmap_from_rgb(w, h, rgb))
            self.dominant.append(dom)
            self.black.append(black)

    def params(self, num_tasks, cfg, mode, quad=None, d=None, **kw):
        w = 128
        quad, d = quad or QUAD, d or self.d
        p = wire.default_params(w, (num_tasks + w - 1) // w, d.world_radius, d.tris.size)
        al = p["areaLight"]
        for k in ("pos", "N", "right", "up", "E"):
            al[k]["x"], al[k]["y"], al[k]["z"] = quad[k]
        al["size"] = quad["size"]
        c = CONFIGS[cfg]
        for k in ("useEnvMap", "useAreaLight", "envMapStrength", "useRoulette"):
            p[k] = c[k]
        p["maxBounces"], p["wfSeparateQueues"] = MAX_BOUNCES, 1
        p["sampleExpl"], p["sampleImpl"] = mode
        for k, v in kw.items():
            p[k] = v
        return p

    def env(self, cfg):
        return self.envs[CONFIGS[cfg]["env"]]


@functools.lru_cache(None)
def scene(all_diffuse=False):
    return LogicScene(all_diffuse)


# ---------------------------------------------------------------------------------------------------------------------------------
# seeds
def draws_of(seed, k):
    """the first k draws of a seed (float64 holding the fp32 draws)"""
    s = np.asarray([seed], np.uint64)
    out = []
    for _ in range(k):
        r, s = bc.rand01(s)
        out.append(float(r[0]))
    return out


def seed_with(k, value, ok=lambda dr: True):
    """a seed whose k-th draw is exactly the fp32 `value` and whose draws satisfy ok(draws): the hashes that round to `value` are tried in turn"""
    value = F(value)
    centre = min(int(round(float(value) * 2.0 ** 32)), 0xFFFFFFFF)
    for delta in range(0, 400):
        for h in {centre + delta, centre - delta}:
            if not 0 <= h <= 0xFFFFFFFF or draw_of(h) != value:
                continue
            s = np.array([h], np.uint64)
            for _ in range(k):
                s = bc.unhash_u32(s)
            if ok(draws_of(int(s[0]), k)):
                return int(s[0])
    return None


def alias_step(env, rnd):
    """sampleEnvMapAlias' integer part in fp32 (env_map.cl:71-74): (slot i, took the slot itself, the texel)"""
    rnd = np.asarray(rnd, np.float64).astype(F)
    n = env.w * env.h
    r = (rnd * F(env.w)) * F(env.h)
    i = np.minimum(np.floor(r).astype(np.int64), n - 1)
    own = (r - i.astype(F)) < np.asarray(env.prob, F)[i]
    return i, own, np.where(own, i, np.asarray(env.alias, np.int64)[i])


def alias_edge(env, i):
    """the two draws nearest to the threshold of slot i that a seed can give: (largest that still takes the slot, smallest that takes its alias)"""
    n = env.w * env.h
    centre = int((i + float(env.prob[i])) / n * 2.0 ** 32)
    hs = np.clip(centre + np.arange(-200000, 200000, dtype=np.int64), 0, 0xFFFFFFFF)
    rnd = hs.astype(F).astype(np.float64) * 2.0 ** -32
    slot, own, _ = alias_step(env, rnd)
    inside = slot == i
    a, b = rnd[inside & own], rnd[inside & ~own]
    assert a.size and b.size and a.max() < b.min()
    return F(a.max()), F(b.min())


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases
FIELDS3 = ("orig", "dir", "T", "Ei", "P", "N", "lastBsdf", "lastT", "lastEmission", "shadowOrig", "shadowDir")
FIELDS1 = ("lastPdfW", "pick", "hitT", "lastCosTh", "lastPdfDirect", "lastPdfImplicit", "shadowRayLen")
FIELDSI = ("pathLen", "lastSpecular", "hitI", "mat", "alh", "blocked")


class Cases:
    """paths entering the logic step under one configuration.  Arrays of length n (fp32 values in float64, integers in int64, seeds in
    uint64); group, label, named (must be decided)."""

    quad = QUAD

    def __init__(self, S, cfg, seed=31):
        self.cfg = cfg
        C = CONFIGS[cfg]
        env = S.env(cfg)
        rng = np.random.RandomState(seed)
        rows = []
        both = C["useEnvMap"] and C["useAreaLight"]
        ntri = S.d.tris.size
        qpos, qn = np.array(QUAD["pos"]), np.array(QUAD["N"])

        def rnd_seed():
            return int(rng.randint(0, 2 ** 32, dtype=np.uint64))

        def unit():
            return _unit(rng.normal(size=3))

        def add(group, label, named=False, **kw):
            tri = int(kw.pop("tri", rng.randint(ntri)))
            b = rng.dirichlet((1.0, 1.0, 1.0)) * 0.7 + 0.1
            P = b @ S.P[tri]
            N = _unit(b @ S.Nv[tri])
            d = kw.get("dir")
            if d is None:
                c = rng.uniform(0.2, 1.0)
                d = -(c * N + np.sqrt(1 - c * c) * _unit(np.cross(N, rng.normal(size=3))))
            P = np.asarray(kw.get("P", P), np.float64)
            dist = kw.pop("dist", rng.uniform(0.4, 2.0))
            r = dict(orig=P - dist * np.asarray(d), dir=d, T=rng.uniform(0.2, 1.0, 3), Ei=np.zeros(3), P=P, N=N, uv=b @ S.UV[tri],
                     lastBsdf=rng.uniform(0.0, 1.0, 3), lastT=rng.uniform(0.1, 1.0, 3), lastEmission=rng.uniform(0.0, 5.0, 3),
                     shadowOrig=rng.uniform(-1, 1, 3), shadowDir=unit(), lastPdfW=float(rng.choice([1.0, 0.05, 3.0, 40.0])), pick=1.0, hitT=dist,
                     lastCosTh=rng.uniform(0.1, 1.0), lastPdfDirect=rng.uniform(0.05, 4.0), lastPdfImplicit=rng.uniform(0.05, 4.0),
                     shadowRayLen=rng.uniform(0.5, 3.0), pathLen=1, lastSpecular=0, hitI=tri, mat=int(rng.choice([0, 3, 4, 5, 7])), alh=0, blocked=1,
                     seed=rnd_seed(), group=group, label=label, named=named)
            if named and group in ("termination", "consume", "quad hit"):        # a named case of these groups sits on a mirror: no light sample
                r["mat"] = 6                                                     # rides along, its subject alone decides it
            for k, v in kw.items():
                assert k in r, k
                r[k] = v
            rows.append(r)

        # ---- termination
        g = "termination"
        for ln in (MAX_BOUNCES, MAX_BOUNCES + 1, MAX_BOUNCES + 3):
            for _ in range(6):
                add(g, f"pathLen {ln}", named=True, pathLen=ln, T=np.full(3, 0.9))
        # roulette: luminance below 0.01, inside (0.01, 0.5), above 0.5; the draw one ulp either side of a CLAMPED contProb (exact in fp32)
        for lum, lb in ((0.004, "lum < 0.01"), (0.2, "lum inside"), (0.8, "lum > 0.5")):
            for _ in range(12):
                add(g, f"roulette, {lb}", named=True, pathLen=MAX_BOUNCES + 1, T=np.full(3, lum) * rng.uniform(0.9, 1.1))
        for cp, lum, lb in ((CONT_LO, 0.003, "0.01"), (CONT_HI, 0.9, "0.5")):
            for v, side in ((F(cp), "at"), (np.nextafter(F(cp), F(1)), "above"), (np.nextafter(F(cp), F(0)), "below")):
                s = seed_with(1, v)
                assert s is not None
                for mat in (0, 4, 6):
                    add(g, f"roulette draw {side} contProb {lb}", named=(mat == 6), pathLen=MAX_BOUNCES + 1, T=np.full(3, lum), seed=s, mat=mat)
        for _ in range(6):
            add(g, "T = 0", named=True, T=np.zeros(3))
            add(g, "lastPdfW = 0", named=True, lastPdfW=0.0)
            add(g, "pathLen 0 terminator", named=True, pathLen=0, T=np.zeros(3), Ei=rng.uniform(0.1, 1.0, 3))
            add(g, "pathLen 0 miss", named=True, pathLen=0, hitI=-1, mat=-1, dir=unit())
            add(g, "T = 0 with a light sample to consume", named=True, T=np.zeros(3), blocked=0)
        for _ in range(60):
            add(g, "random", pathLen=int(rng.randint(0, MAX_BOUNCES + 3)), T=rng.uniform(0.0, 1.0, 3) * float(rng.choice([1.0, 0.02])))

        # ---- miss
        g = "miss"
        axes = [("+y pole", (0, 1, 0)), ("+x", (1, 0, 0)), ("-x", (-1, 0, 0)), ("-z", (0, 0, -1)), ("(+0,0,1)", (0.0, 0, 1)), ("(-0,0,1)", (-0.0, 0, 1)),
                ("(1e-8,0,1)", (1e-8, 0, 1)), ("(-1e-8,0,1)", (-1e-8, 0, 1)), ("zero vector", (0, 0, 0)), ("unnormalised", (0.6, 2.0, -1.1)),
                ("unnormalised tiny", (3e-4, -1e-4, 2e-4))]

        def miss(label, d, named=False, **kw):
            add(g, label, named=named, hitI=-1, mat=-1, dir=np.asarray(d, np.float64), **kw)
        plain = [dict(pathLen=1), dict(pathLen=2, lastSpecular=1)]               # no MIS weight: the lookup alone
        weighted = [dict(pathLen=2), dict(pathLen=2, pick=0.5), dict(pathLen=3, pick=0.5, lastPdfW=0.05)]
        state_sweep = plain + weighted
        # (an axis direction lies on a texel border of both maps: with a MIS weight its pdf texel is fp32's to choose -- undecided by nature,
        #  and still held to the oracle bit for bit)
        for lb, d in axes:
            for kw in plain + weighted[:2]:
                miss(lb, d, **kw)
        for kw in state_sweep:
            miss("-y pole", (0, -1, 0), **kw)                                   # the named quirk: see the module docstring
        for e in S.envs:                                                        # texel centres and texel edges of both maps
            for k in range(24):
                i, j = int(rng.randint(e.w)), int(rng.randint(e.h))
                for lb, (u, v) in (("texel centre", ((i + 0.5) / e.w, (j + 0.5) / e.h)), ("texel edge", (i / e.w, (j + 0.5) / e.h)),
                                   ("texel corner", (i / e.w, max(j, 1) / e.h))):
                    ph, th = v * np.pi, (u * 2 - 1) * np.pi
                    sweep = state_sweep if lb == "texel centre" or k < 2 else plain
                    miss(lb, (np.sin(ph) * np.sin(th), np.cos(ph), -np.sin(ph) * np.cos(th)), **sweep[int(rng.randint(len(sweep)))])
        for _ in range(1500):
            miss("random", unit(), **state_sweep[int(rng.randint(len(state_sweep)))])
        for _ in range(40):
            miss("random, prior Ei", unit(), pathLen=2, Ei=rng.uniform(0.05, 1.0, 3))

        # ---- quad hit: the hit record of a ray that met the parametric quad (P on it, N its normal, areaLightHit 1)
        g = "quad hit"
        for lb, cos, dist in (("near", 0.9, 0.05), ("far", 0.8, 40.0), ("grazing", 1e-3, 1.0), ("normal incidence", 1.0, 1.0), ("ordinary", 0.5, 1.5)):
            for kw in state_sweep:
                for _ in range(3):
                    X = qpos + rng.uniform(-0.9, 0.9) * QUAD["size"][0] * np.array(QUAD["right"]) + rng.uniform(-0.9, 0.9) * QUAD["size"][1] * np.array(QUAD["up"])
                    t = _unit(np.cross(qn, rng.normal(size=3)))
                    d = -(cos * qn + np.sqrt(max(0.0, 1 - cos * cos)) * t)
                    add(g, lb, named=(lb != "grazing"), alh=1, hitI=0, P=X, N=qn, dir=d, dist=dist, **kw)

        # ---- consume: the previous vertex' light sample, on continuing and on terminating paths
        g = "consume"
        for _ in range(200):
            add(g, "swept", named=True, blocked=0, pick=float(rng.choice([1.0, 0.5])), lastPdfDirect=float(10 ** rng.uniform(-3, 3)),
                lastPdfImplicit=float(10 ** rng.uniform(-3, 3)), lastEmission=rng.uniform(0.0, 300.0, 3))
        for _ in range(12):
            add(g, "lastCosTh = 0", named=True, blocked=0, lastCosTh=0.0)
            add(g, "lastBsdf = 0", named=True, blocked=0, lastBsdf=np.zeros(3))
            add(g, "lastPdfImplicit = 0", named=True, blocked=0, lastPdfImplicit=0.0)
            add(g, "on a miss", blocked=0, hitI=-1, mat=-1, dir=unit(), pathLen=2)
            add(g, "on the last bounce", named=True, blocked=0, pathLen=MAX_BOUNCES + 1, T=np.full(3, 0.9))
        for _ in range(60):
            add(g, "prior Ei", named=True, blocked=0, Ei=rng.uniform(0.05, 2.0, 3))

        # ---- NEE, environment
        g = "nee env"
        if C["useEnvMap"]:
            n_tex = env.w * env.h
            k_pick = 2
            is_env = (lambda dr: dr[0] < 0.5) if both else (lambda dr: dr[0] < 1.0)
            prob = np.asarray(env.prob, np.float64)
            part = [i for i in range(n_tex) if 0.05 < prob[i] < 0.95][:3]
            to_dom = [i for i in range(n_tex) if env.alias[i] == S.dominant[CONFIGS[cfg]["env"]] and prob[i] < 0.9][:2]
            black = [i for i in S.black[CONFIGS[cfg]["env"]]]
            assert len(part) == 3 and to_dom and all(prob[i] == 0 for i in black)
            picks = [("pick draw = 0", F(0.0)), ("pick draw = 1 - ulp (index clamp)", BELOW1), ("pick draw = 1 (index clamp)", F(1.0))]
            for i in part:
                lo, hi = alias_edge(env, i)
                picks += [(f"slot {i}: below prob", lo), (f"slot {i}: at prob", hi)]
            for i in to_dom:
                picks.append((f"slot {i}: alias is the dominant texel", F((i + 0.5 * (1 + prob[i])) / n_tex)))
            picks.append(("the dominant texel's own slot", F((S.dominant[CONFIGS[cfg]["env"]] + 1e-3) / n_tex)))
            for i in black:
                picks.append((f"slot {i}: black, aliased", F((i + 0.5) / n_tex)))
            self.picks = {}
            for lb, v in picks:
                s = seed_with(k_pick, v, is_env)
                if s is None:                                                    # (no seed gives this draw behind an environment choice: the other configuration has it)
                    continue
                self.picks[lb] = F(v)
                for mat in (0, 4, 5, 7):
                    add(g, lb, named=True, seed=s, mat=mat)
            if not both:
                assert all(lb in self.picks for lb, _ in picks), "with the map alone every pick draw is reachable"
                s = seed_with(1, F(1.0))
                for mat in (0, 4):
                    add(g, "choice draw = 1: no light at all", named=True, seed=s, mat=mat, blocked=0)
            for _ in range(40):
                add(g, "back face", mat=int(rng.choice([0, 4, 5, 7])))               # the state's normal arrives turned away from the ray
                rows[-1]["N"] = -rows[-1]["N"]
            for _ in range(300):
                add(g, "random", mat=int(rng.choice([0, 3, 4, 5, 7])))
            for mat in (6, 8):
                for _ in range(20):
                    add(g, "singular receiver", named=True, mat=mat)

        # ---- NEE, quad
        g = "nee quad"
        if C["useAreaLight"]:
            is_quad = (lambda dr: dr[0] >= 0.5) if both else (lambda dr: True)
            self.quad_draws = {}
            for k, name in ((2, "r1"), (3, "r2")):
                for v, vl in ((F(0.0), "0"), (F(1.0), "1"), (BELOW1, "1 - ulp")):
                    s = seed_with(k, v, is_quad)
                    if s is None:
                        continue
                    self.quad_draws[f"{name} draw = {vl}"] = (k, v)
                    for mat in (0, 4, 5, 7):
                        add(g, f"{name} draw = {vl}", named=True, seed=s, mat=mat, tri=int(rng.randint(128)))
            if both:
                for v, vl in ((F(0.5), "0.5"), (np.nextafter(F(0.5), F(0)), "0.5 - ulp"), (np.nextafter(F(0.5), F(1)), "0.5 + ulp")):
                    s = seed_with(1, v)
                    for mat in (0, 4, 5, 7):
                        add(g, f"choice draw = {vl}", named=True, seed=s, mat=mat, tri=int(rng.randint(128)))
            for _ in range(40):                                                  # above the quad's plane: cosLight <= 0, shadowRayBlocked set
                P = qpos + np.array([rng.uniform(-1, 1), rng.uniform(0.05, 1.0), rng.uniform(-1, 1)])
                add(g, "behind the quad", P=P, blocked=0, seed=seed_with(1, F(rng.uniform(0.5, 1.0))))
            for _ in range(40):                                                  # nearly in the quad's plane, below it
                P = qpos + np.array([rng.uniform(-2, 2), -10 ** rng.uniform(-5, -2), rng.uniform(-2, 2)])
                add(g, "nearly in the quad's plane", P=P, seed=seed_with(1, F(rng.uniform(0.5, 1.0))))
            for _ in range(300):
                add(g, "random", tri=int(rng.randint(128)), seed=seed_with(1, F(rng.uniform(0.5, 1.0))) if both else rnd_seed())

        # ---- normal map
        g = "normal map"
        uvs = [u for u in bc.UV_SWEEP if np.isfinite(u)]
        for mat in S.MAPPED:
            for u in uvs:
                for uv in ((u, 0.5), (0.5, u), (u, u)):
                    add(g, f"uv sweep, material {mat}", named=(mat == 10 and abs(u) <= 1.0), mat=mat, uv=np.array(uv))
            for _ in range(12):
                add(g, "uv determinant 0", named=(mat == 10), mat=mat, tri=S.FLAT)
            for _ in range(60):                                                   # grazing arrivals: the turned normal decides the face
                add(g, "turned normal against the ray", mat=mat)
                r = rows[-1]
                t = _unit(np.cross(r["N"], rng.normal(size=3)))
                c = rng.uniform(-0.3, 0.3)
                r["dir"] = -(c * r["N"] + np.sqrt(1 - c * c) * t)
                r["orig"] = r["P"] - r["hitT"] * r["dir"]
        # back faces: the state's normal arrives turned away from the ray (every group's random fill has front faces only)
        for _ in range(80):
            add("back face", "back face", mat=int(rng.choice([0, 4, 5, 7, 6, 2, 9])))
            rows[-1]["N"] = -rows[-1]["N"]

        self.n = len(rows)
        for k in FIELDS3:
            setattr(self, k, f32([r[k] for r in rows]))
        self.uv = f32([r["uv"] for r in rows])
        for k in FIELDS1:
            setattr(self, k, f32([r[k] for r in rows]))
        for k in FIELDSI:
            setattr(self, k, np.array([r[k] for r in rows], np.int64))
        self.seed = np.array([r["seed"] for r in rows], np.uint64)
        self.group, self.label = np.array([r["group"] for r in rows]), np.array([r["label"] for r in rows])
        self.named = np.array([r["named"] for r in rows], bool)

    def state(self, st):
        """write the paths into a reference-layout state (64, >= n + EXTRA) in place; the others become inert (T = 0, pathLen 0: they
        terminate and add nothing)"""
        n, u = self.n, st.view(np.uint32)
        assert st.shape[1] >= n + EXTRA
        for k, col in (("orig", COL.ORIG), ("dir", COL.DIR), ("T", COL.T), ("Ei", COL.EI), ("P", COL.P), ("N", COL.N), ("lastBsdf", COL.LAST_BSDF),
                       ("lastT", COL.LAST_T), ("lastEmission", COL.LAST_EMISSION), ("shadowOrig", COL.SHADOW_ORIG), ("shadowDir", COL.SHADOW_DIR)):
            st[col:col + 3, :n] = getattr(self, k).T
        st[COL.UV:COL.UV + 2, :n] = self.uv.T
        for k, col in (("lastPdfW", COL.LAST_PDF_W), ("pick", COL.LAST_PICK_PROB), ("hitT", COL.HIT_T), ("lastCosTh", COL.LAST_COS_TH),
                       ("lastPdfDirect", COL.LAST_PDF_DIRECT), ("lastPdfImplicit", COL.LAST_PDF_IMPLICIT), ("shadowRayLen", COL.SHADOW_LEN)):
            st[col, :n] = getattr(self, k)
        i = st.view(np.int32)
        for k, col in (("pathLen", COL.PATH_LEN), ("lastSpecular", COL.LAST_SPECULAR), ("hitI", COL.HIT_I), ("mat", COL.MAT_ID), ("alh", COL.AREA_LIGHT_HIT),
                       ("blocked", COL.SHADOW_BLOCKED)):
            i[col, :n] = getattr(self, k)
        u[COL.SEED, :n] = self.seed.astype(np.uint32)
        u[COL.BACKFACE, :n] = 0
        u[COL.FIRST_DIFFUSE, :] = 0
        st[COL.T:COL.T + 3, n:] = 0.0
        st[COL.EI:COL.EI + 3, n:] = 0.0
        u[COL.PATH_LEN, n:] = 0
        u[COL.SHADOW_BLOCKED, n:] = 1
        u[COL.PIXEL_INDEX, :] = np.arange(st.shape[1])
        return st


@functools.lru_cache(None)
def cases(cfg):
    return Cases(scene(), cfg)


# ---------------------------------------------------------------------------------------------------------------------------------
# B. rays: paths entering the extension kernel, whose RAW hit records the fused pass commits itself
QUAD_LOW = dict(QUAD, pos=(0.25, 0.4375, 0.125))          # between the ground and the spheres: triangles before it and behind it


class Hit:
    """the committed hit record of every path (and the path's other inputs), as one evaluation of the commit leaves it"""


def _mt(E, o, d, p0, p1, p2):
    """intersectTriangle (src/intersect.cl:64-93) without its tests: (t, u, v)"""
    s1, s2 = E.j(p1 - p0), E.j(p2 - p0)
    pvec = E.j(np.cross(d, s2))
    iDet = E.j(1.0 / E.j(_dot(s1, pvec)))
    tvec = E.j(o - p0)
    qvec = E.j(np.cross(tvec, s1))
    return E.j(E.j(_dot(s2, qvec)) * iDet), E.j(E.j(_dot(tvec, pvec)) * iDet), E.j(E.j(_dot(d, qvec)) * iDet)


class RayCases:
    """rays aimed from crafted origins at interior points of chosen triangles, at the neighbourhood of smooth-normal vertices, at the quad
    (with nothing before it, with the ground before it, with a sphere behind it) and at the sky.  The float64 nearest hit is
    traversal_cases.BruteForce's; a ray it does not call robust is undecided."""
    quad = QUAD_LOW
    cfg = "both"

    def __init__(self, S, seed=41, pad_to=None):
        import traversal_cases as tc
        rng = np.random.RandomState(seed)
        rows = []
        qpos, qr, qu = (np.array(self.quad[k]) for k in ("pos", "right", "up"))
        sx, sy = self.quad["size"]
        ntri = S.d.tris.size
        cross = np.cross(S.P[:, 1] - S.P[:, 0], S.P[:, 2] - S.P[:, 0])

        def add(group, o, X):
            o32 = f32(o)
            rows.append(dict(orig=o32, dir=f32(_unit(X - o32)), group=group))

        def toward(group, tri, b, side=None):
            X = b @ S.P[tri]
            nrm = _unit(cross[tri])
            t0 = _unit(S.P[tri, 1] - S.P[tri, 0])
            a, c = rng.uniform(0, 2 * np.pi), float(rng.choice([1.0, 0.7, 0.3, 0.1]))
            tng = t0 * np.cos(a) + np.cross(nrm, t0) * np.sin(a)
            sd = int(rng.choice([1, -1])) if side is None else side
            add(group, X + rng.uniform(0.3, 1.5) * (sd * c * nrm + np.sqrt(1 - c * c) * tng), X)
        for _ in range(900):
            toward("interior", int(rng.randint(ntri)), rng.dirichlet((1.0, 1.0, 1.0)) * 0.55 + 0.15)
        for _ in range(250):
            toward("vertex", int(rng.randint(128, ntri)), rng.permutation([0.9, 0.05, 0.05]))
        on_quad = lambda: qpos + rng.uniform(-0.9, 0.9) * sx * qr + rng.uniform(-0.9, 0.9) * sy * qu
        for _ in range(200):                                                  # from between the ground and the quad
            add("quad", np.array([rng.uniform(-1.5, 1.5), rng.uniform(0.03, 0.4), rng.uniform(-1.0, 1.0)]), on_quad())
        for _ in range(60):                                                   # from under the ground: the ground is met first
            add("ground before the quad", np.array([rng.uniform(-1.0, 1.0), rng.uniform(-0.6, -0.05), rng.uniform(-0.6, 0.6)]), on_quad())
        for _ in range(80):                                                   # through the quad at the sphere above it
            X = on_quad()
            o = np.array([X[0] + rng.uniform(-0.05, 0.05), 0.2, X[2] + rng.uniform(-0.05, 0.05)])
            add("sphere behind the quad", o, o + (X - o) * 3.0)
        for _ in range(200):
            o = np.array([rng.uniform(-1.5, 1.5), 1.5, rng.uniform(-1.0, 1.0)])
            add("sky", o, o + _unit(rng.normal(size=3)) * np.array([1.0, 0.0, 1.0]) + np.array([0.0, rng.uniform(0.02, 1.0), 0.0]))
        n = self.n = len(rows)
        self.orig, self.dir = f32([r["orig"] for r in rows]), f32([r["dir"] for r in rows])
        self.group = np.array([r["group"] for r in rows])
        self.label = self.group
        self.named = np.zeros(n, bool)
        # the path's own state
        self.len_before = rng.choice([0, 1, 2, MAX_BOUNCES, MAX_BOUNCES + 1], n, p=[0.3, 0.3, 0.2, 0.1, 0.1]).astype(np.int64)
        self.T, self.Ei = f32(rng.uniform(0.2, 1.0, (n, 3))), np.zeros((n, 3))
        self.lastPdfW = f32(rng.choice([1.0, 0.05, 3.0, 40.0], n))
        self.pick = f32(rng.choice([1.0, 0.5], n))
        self.lastSpecular = rng.randint(0, 2, n).astype(np.int64)
        self.blocked = (rng.uniform(size=n) > 0.3).astype(np.int64)
        self.lastBsdf, self.lastT, self.lastEmission = f32(rng.uniform(0, 1, (n, 3))), f32(rng.uniform(0.1, 1, (n, 3))), f32(rng.uniform(0, 5, (n, 3)))
        self.lastCosTh, self.lastPdfDirect, self.lastPdfImplicit = (f32(rng.uniform(0.05, 4.0, n)) for _ in range(3))
        self.shadowOrig, self.shadowDir, self.shadowRayLen = f32(rng.uniform(-1, 1, (n, 3))), f32(_unit(rng.normal(size=(n, 3)))), f32(rng.uniform(0.5, 3.0, n))
        self.seed = rng.randint(0, 2 ** 32, n, dtype=np.uint64)
        # where each path sits: in order, or spread over a packing padded with inert paths to a multiple of 256
        self.n_tasks = n + EXTRA if pad_to is None else (n + EXTRA + pad_to - 1) // pad_to * pad_to
        self.index = np.arange(n) if pad_to is None else np.sort(rng.permutation(self.n_tasks)[:n])
        # the float64 nearest hit
        bf = tc.BruteForce(S.P, self.orig, self.dir, np.full(n, tc.FLT_MAX, F))
        self.hit, self.t_hit, robust = bf.closest, bf.t_closest, bf.verdict(S.d)["ext_decided"]
        qn = np.array(self.quad["N"])
        den = _dot(self.dir, qn)
        with np.errstate(all="ignore"):
            tq = _dot(qpos - self.orig, qn) / den
            X = self.orig + tq[:, None] * self.dir - qpos
            a, b = np.abs(_dot(X, qr)) / sx, np.abs(_dot(X, qu)) / sy
            diag = np.abs(_dot(X, qr) / sx - _dot(X, qu) / sy)                # the seam of the quad's two triangles (tl - br)
            inside, outside = (a < 1 - 1e-4) & (b < 1 - 1e-4) & (diag > 1e-4), (a > 1 + 1e-4) | (b > 1 + 1e-4)
            t_tri = np.where(self.hit >= 0, self.t_hit, np.inf)
            self.quad_wins = (den < -1e-6) & (tq > 1e-6) & (tq < t_tri * (1 - 1e-5)) & inside
            quad_clear = self.quad_wins | (den > 1e-6) | outside | (tq < -1e-6) | (tq > t_tri * (1 + 1e-5))
            self.first = _dot(X, qr) / sx > _dot(X, qu) / sy                  # which of the quad's two triangles holds the point
        self.robust = robust & quad_clear
        self.S = S

    def commit(self, E, q, sx, sy, quad_on):
        """traceExtension's commit (src/wf_extrays.cl:22-35, src/bvh.cl:271-279, src/intersect.cl:124-155): the nearest triangle's P, barycentric
        normal and uv, then the implicit quad (only with sampleImpl and useAreaLight, wf_extrays.cl:29), pathLen + 1"""
        S, n = self.S, self.n
        E.bad |= ~self.robust
        h = Hit()
        for k in FIELDS3 + FIELDS1 + ("seed", "lastSpecular", "blocked", "quad"):
            if hasattr(self, k):
                setattr(h, k, getattr(self, k))
        tri = np.maximum(self.hit, 0)
        P3 = S.P[tri]
        t, u, v = _mt(E, self.orig, self.dir, P3[:, 0], P3[:, 1], P3[:, 2])
        lerp = lambda a: E.j(E.j(E.j(1.0 - u - v)[:, None] * a[:, 0]) + E.j(u[:, None] * a[:, 1]) + E.j(v[:, None] * a[:, 2]))
        got = self.hit >= 0
        N = np.where(got[:, None], E.normalize(lerp(S.Nv[tri])), 0.0)
        uv = np.where(got[:, None], lerp(S.UV[tri]), 0.0)
        # the quad's two triangles: (tl, bl, br) and (tl, br, tr)
        c = lambda a, b: q["pos"] + a * sx * q["right"] + b * sy * q["up"]
        tl, tr, bl, br = c(1, 1), c(-1, 1), c(1, -1), c(-1, -1)
        ones = np.ones((n, 1))
        t1 = _mt(E, self.orig, self.dir, tl * ones, bl * ones, br * ones)[0]
        t2 = _mt(E, self.orig, self.dir, tl * ones, br * ones, tr * ones)[0]
        tq = np.where(self.first, t1, t2)
        w = self.quad_wins & quad_on
        t = np.where(w, tq, np.where(got, t, float(np.finfo(F).max)))             # EMPTY_HIT(FLT_MAX), wf_extrays.cl:27
        h.P = np.where((w | got)[:, None], E.j(self.orig + E.j(t[:, None] * self.dir)), 0.0)
        h.N = np.where(w[:, None], q["N"], N)
        h.uv, h.hitT = uv, t
        h.hitI = np.where(w, 0, self.hit)
        h.mat = np.where(w, 0, np.where(got, S.d.tris["matId"].astype(np.int64)[tri], -1))
        h.alh = w.astype(np.int64)
        h.pathLen = self.len_before + 1
        return h

    def state(self, st):
        """the paths, before the extension kernel traces them, in a reference-layout state; every other path becomes inert"""
        at, u = self.index, st.view(np.uint32)
        assert st.shape[1] == self.n_tasks
        st[COL.T:COL.T + 3, :] = 0.0
        st[COL.EI:COL.EI + 3, :] = 0.0
        u[COL.PATH_LEN, :] = 0
        u[COL.SHADOW_BLOCKED, :] = 1
        u[COL.FIRST_DIFFUSE, :] = 0
        u[COL.BACKFACE, :] = 0
        st.view(np.int32)[COL.HIT_I, :] = -1
        for k, col in (("orig", COL.ORIG), ("dir", COL.DIR), ("T", COL.T), ("Ei", COL.EI), ("lastBsdf", COL.LAST_BSDF), ("lastT", COL.LAST_T),
                       ("lastEmission", COL.LAST_EMISSION), ("shadowOrig", COL.SHADOW_ORIG), ("shadowDir", COL.SHADOW_DIR)):
            st[col:col + 3, at] = getattr(self, k).T
        for k, col in (("lastPdfW", COL.LAST_PDF_W), ("pick", COL.LAST_PICK_PROB), ("lastCosTh", COL.LAST_COS_TH), ("lastPdfDirect", COL.LAST_PDF_DIRECT),
                       ("lastPdfImplicit", COL.LAST_PDF_IMPLICIT), ("shadowRayLen", COL.SHADOW_LEN)):
            st[col, at] = getattr(self, k)
        for k, col in (("len_before", COL.PATH_LEN), ("lastSpecular", COL.LAST_SPECULAR), ("blocked", COL.SHADOW_BLOCKED)):
            u[col, at] = getattr(self, k)
        u[COL.SEED, at] = self.seed.astype(np.uint32)
        u[COL.PIXEL_INDEX, :] = np.arange(st.shape[1])
        return st


@functools.lru_cache(None)
def ray_cases(all_diffuse=False, pad_to=None):
    return RayCases(scene(all_diffuse), pad_to=pad_to)


@functools.lru_cache(None)
def ray_verdict(all_diffuse, pad_to, mode):
    c = ray_cases(all_diffuse, pad_to)
    return Verdict(restatement(scene(all_diffuse), c, mode), c.n)


def load_rays(ctx, c):
    """import the rays' paths and enqueue exactly them for the extension kernel; returns the state before"""
    st = c.state(ctx.state_export().copy())
    ctx.state_import(st)
    ctx.clear_queues()
    ctx.queue_write(Q.EXTENSION, c.index.astype(np.uint32))
    cnt = np.array(ctx.get_counters(), copy=True)
    if hasattr(ctx, "finish"):
        ctx.finish()
    cnt = np.array(cnt, copy=True)
    cnt[:] = 0
    cnt[Q.EXTENSION] = c.n
    ctx.set_counters(cnt)
    return st


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatement
def _br_int(E, k, m):
    """an integer decision taken on a jittered value: a branch of the cases in m"""
    E.branches.append((E.idx, np.where(m, np.asarray(k, np.int64), 0)))


def _direction_to_uv(E, d):
    """env_map.cl:14-24"""
    zero = (d == 0).all(1)
    with np.errstate(all="ignore"):
        at = E.j(np.arctan2(d[:, 0], -d[:, 2]))
        u = E.j(1.0 + E.j(at / PI)) * 0.5
        ln = E.j(np.sqrt(_dot(d, d)))
        E.chk(np.where(zero, 1.0, ln))
        r = np.clip(E.j(d[:, 1] / np.where(zero, 1.0, ln)), -1.0, 1.0)
        v = E.j(E.j(np.arccos(r)) / PI)
    return np.where(zero, 0.0, u), np.where(zero, 0.0, v)


def _env_lookup(E, env, u, v):
    """read_imagef with samplerFloat (env_map.cl:10, :39-43): normalised coordinates, clamp to edge, linear -- OpenCL 1.2 s8.2"""
    w, h = env.w, env.h
    rgb = np.asarray(env.rgb, np.float64).reshape(h, w, 3)
    fu, fv = E.j(E.j(u * w) - 0.5), E.j(E.j(v * h) - 0.5)
    i0, j0 = np.floor(fu), np.floor(fv)
    a, b = (fu - i0)[:, None], (fv - j0)[:, None]
    ci = lambda x: np.clip(x, 0, w - 1).astype(np.int64)
    cj = lambda x: np.clip(x, 0, h - 1).astype(np.int64)
    t = lambda j, i: rgb[cj(j), ci(i)]
    return E.j((1 - a) * (1 - b) * t(j0, i0) + a * (1 - b) * t(j0, i0 + 1) + (1 - a) * b * t(j0 + 1, i0) + a * b * t(j0 + 1, i0 + 1))


def _env_pdf(E, env, u, v, m):
    """envMapPdf (env_map.cl:95-107) for the cases in m"""
    w, h = env.w, env.h
    pdf = np.asarray(env.pdf, np.float64)
    sinTh = E.j(np.sin(E.j(v * PI)))
    z = E.br(m & (sinTh == 0.0))
    iu, iv = np.minimum(np.floor(E.j(u * w)), w - 1), np.minimum(np.floor(E.j(v * h)), h - 1)
    _br_int(E, iu, m)
    _br_int(E, iv, m)
    idx = np.clip(iv * w + iu, 0, w * h - 1).astype(np.int64)
    with np.errstate(all="ignore"):
        r = E.j(pdf[idx] / (TWO_PI * PI * np.where(z, 1.0, sinTh)))
    return np.where(z, 0.0, r)


def restatement(S, c, mode):
    """fn(E) of Verdict: the logic step of the cases c under (sampleExpl, sampleImpl) = mode"""
    expl, impl = mode
    C = CONFIGS[c.cfg]
    env = S.env(c.cfg)
    n = c.n
    useEnv, useArea, strength, roulette = bool(C["useEnvMap"]), bool(C["useAreaLight"]), float(F(C["envMapStrength"])), bool(C["useRoulette"])
    envMapProb = C["useEnvMap"] / max(1, C["useEnvMap"] + C["useAreaLight"])
    sx, sy = float(F(c.quad["size"][0])), float(F(c.quad["size"][1]))
    q = {k: np.asarray(c.quad[k], np.float64) for k in ("pos", "N", "right", "up", "E")}
    world_radius = float(F(S.d.world_radius))
    all_n = np.arange(n)
    inputs = c

    def fn(E):
        E.idx = all_n
        out = {k: None for k in FLOAT_OUT}
        with np.errstate(all="ignore"):
            c = inputs.commit(E, q, sx, sy, bool(impl) and useArea) if hasattr(inputs, "commit") else inputs     # RAW hit records: the commit comes first
            mat = np.where(c.mat >= 0, c.mat, 0)
            mtype, mapN = S.type[mat], S.mapN[mat]
            tri = np.where(c.hitI >= 0, c.hitI, 0)
            # ---- russian roulette, :60-69
            seed = c.seed.copy()
            T = c.T.copy()
            term = c.pathLen >= MAX_BOUNCES + 1
            roul = term & roulette
            contProb = np.clip(E.j(LUM[0] * T[:, 0] + LUM[1] * T[:, 1] + LUM[2] * T[:, 2]), CONT_LO, CONT_HI)
            r, s1 = bc.rand01(seed)
            stop = E.br(roul & (r > contProb))
            term = np.where(roul, stop, term)
            T = np.where(roul[:, None], E.j(T / contProb[:, None]), T)
            seed = np.where(roul, s1, seed)
            # ---- :72-73
            term = term | (T == 0).all(1) | (c.lastPdfW == 0)
            Ei = c.Ei.copy()
            # ---- implicit environment sample, :84-107
            miss = (c.hitI < 0) & ~term
            u, v = _direction_to_uv(E, c.dir)
            bg = np.zeros((n, 3))
            if useEnv:
                see = miss & ((c.pathLen == 1) | bool(impl))
                bg = np.where(see[:, None], E.j(_env_lookup(E, env, u, v) * strength), 0.0)
            mis_env = miss & bool(impl) & bool(expl) & useEnv & (c.pathLen > 1) & (c.lastSpecular == 0)
            pdfE = _env_pdf(E, env, u, v, mis_env)
            a = E.j(c.lastPdfW * c.pick)
            w_env = np.where(mis_env, E.j(a / E.j(a + pdfE)), 1.0)
            E.chk(np.where(mis_env & (pdfE != 0), pdfE, 1.0))
            add_env = E.j(E.j(w_env[:, None] * T) * bg)
            Ei = np.where(miss[:, None], E.j(Ei + add_env), Ei)
            # ---- implicit area-light sample, :111-131
            quad = useArea & (c.alh != 0) & ~term & ~miss
            mis_q = quad & bool(expl) & (c.pathLen > 1) & (c.lastSpecular == 0)
            pdfA = E.j(1.0 / E.j(4.0 * sx * sy))
            dist = E.j(np.sqrt(_dot(c.P - c.orig, c.P - c.orig)))
            cosq = _dot(E.normalize(-c.dir), c.N)
            pdfWq = E.j(E.j(pdfA * E.j(dist * dist)) / np.abs(np.where(mis_q, cosq, 1.0)))
            E.chk(np.where(mis_q, pdfWq, 1.0))
            w_q = np.where(mis_q, E.j(c.lastPdfW / E.j(c.lastPdfW + E.j(pdfWq * c.pick))), 1.0)
            Ei = np.where(quad[:, None], E.j(Ei + E.j(E.j(T * w_q[:, None]) * q["E"])), Ei)
            term = term | miss | quad
            # ---- consume the light sample of the previous vertex, :135-156
            cons = c.blocked == 0
            b = E.j(c.lastPdfDirect * c.pick)
            w_c = E.j(b / E.j(b + c.lastPdfImplicit)) if impl else np.ones(n)
            contrib = E.j(E.j(E.j(E.j(E.j(c.lastBsdf * c.lastT) * c.lastEmission) * w_c[:, None]) * c.lastCosTh[:, None]) / E.j(c.pick * c.lastPdfDirect)[:, None])
            E.chk(np.where(cons[:, None], contrib, 0.0))
            Ei = np.where(cons[:, None], E.j(Ei + contrib), Ei)
            # ---- the hit: tangent-space normal (utils.cl:149-182), the back-face turn, the shadow origin, :180-184
            cont = ~term
            mapped = cont & (mapN != -1)
            tex = E.j(2.0 * E.j(np.where(mapped[:, None], S.tex.fetch(np.where(mapped, mapN, -1), c.uv), 0.0)) - 1.0)
            P3, U3 = S.P[tri], S.UV[tri]
            e1, e2 = P3[:, 1] - P3[:, 0], P3[:, 2] - P3[:, 0]
            t1, t2 = f32(U3[:, 1] - U3[:, 0]), f32(U3[:, 2] - U3[:, 0])
            det = E.j(t1[:, 0] * t2[:, 1] - t1[:, 1] * t2[:, 0])
            turn = E.br(mapped & (det != 0.0))
            inv = 1.0 / np.where(det != 0, det, 1.0)
            Tt = E.normalize(E.j(inv[:, None] * E.j(e1 * t2[:, 1:2] - e2 * t1[:, 1:2])))
            Bt = E.normalize(E.j(inv[:, None] * E.j(e2 * t1[:, 0:1] - e1 * t2[:, 0:1])))
            Nm = E.normalize(E.j(Tt * tex[:, 0:1] + Bt * tex[:, 1:2] + c.N * tex[:, 2:3]))
            N = np.where(turn[:, None], Nm, c.N)
            back = E.br(cont & (_dot(N, c.dir) > 0.0))
            N = np.where(back[:, None], -N, N)
            orig = E.j(c.P - E.j(EPS_SURF * c.dir))
            # ---- next event estimation, :217-302
            nee = cont & bool(expl) & np.isin(mtype, NONSINGULAR)
            r0, s1 = bc.rand01(seed)
            pickEnv = nee & (r0 < envMapProb)
            pickQuad = nee & ~(r0 < envMapProb) & useArea
            r1, s2 = bc.rand01(s1)
            r2, s3 = bc.rand01(s2)
            seed = np.where(pickEnv, s2, np.where(pickQuad, s3, np.where(nee, s1, seed)))
            # environment (env_map.cl:65-92)
            slot, own, texel = alias_step(env, r1)
            ui, vi = texel % env.w, texel // env.w
            ue, ve = E.j((ui + 0.5) / env.w), E.j((vi + 0.5) / env.h)
            sPh, cPh = E.sincos(ve * PI)
            sTh, cTh = E.sincos(E.j(E.j(ue * 2.0 - 1.0) * PI))
            Le = E.normalize(E.j(np.stack([sPh * sTh, cPh, -sPh * cTh], 1)))
            sinV = E.j(np.sin(E.j(PI * ve)))
            pdfWe = np.where(sinV != 0, E.j(np.asarray(env.pdf, np.float64)[texel] / E.j(2.0 * PI * PI * np.where(sinV != 0, sinV, 1.0))), 0.0)
            u2, v2 = _direction_to_uv(E, Le)
            Lie = E.j(_env_lookup(E, env, u2, v2) * strength)
            # quad (utils.cl:226-234)
            posL = q["pos"] + E.j(E.j(E.j(2.0 * r1 - 1.0) * sx)[:, None] * q["right"]) + E.j(E.j(E.j(2.0 * r2 - 1.0) * sy)[:, None] * q["up"])
            Lq = E.j(E.j(posL) - orig)
            lenq = E.j(E.j(np.sqrt(_dot(Lq, Lq))) * SHORT)
            Lq = E.normalize(Lq)
            cosLight = np.fmax(_dot(q["N"], -Lq), 0.0)
            lit = E.br(pickQuad & (cosLight > 0.0))
            pdfWq2 = E.j(E.j(pdfA * E.j(lenq * lenq)) / np.where(lit, cosLight, 1.0))
            E.chk(np.where(lit, pdfWq2, 1.0))
            have = pickEnv | lit
            L = np.where(pickEnv[:, None], Le, Lq)
            cosTh = np.fmax(0.0, _dot(L, N))
            E.br(have & (_dot(L, N) > 0.0))
            new = {"shadowOrig": orig, "shadowDir": L, "shadowRayLen": np.where(pickEnv, 2.0 * world_radius, lenq)[:, None],
                   "lastPdfDirect": np.where(pickEnv, pdfWe, pdfWq2)[:, None], "lastEmission": np.where(pickEnv[:, None], Lie, q["E"]),
                   "lastCosTh": cosTh[:, None], "lastLightPickProb": np.where(pickEnv, envMapProb, 1.0 - envMapProb)[:, None]}
            old = {"shadowOrig": c.shadowOrig, "shadowDir": c.shadowDir, "shadowRayLen": c.shadowRayLen[:, None], "lastPdfDirect": c.lastPdfDirect[:, None],
                   "lastEmission": c.lastEmission, "lastCosTh": c.lastCosTh[:, None], "lastLightPickProb": c.pick[:, None]}
            for k in SAMPLE_OUT:
                out[k] = np.where(have[:, None], new[k], old[k])
            out["Ei"], out["T"] = Ei, T
            out["N"] = np.where(cont[:, None], N, c.N)
            if c is not inputs:
                out["P"], out["uv"], out["hitT"] = c.P, c.uv, c.hitT[:, None]
        changed = {k: have for k in SAMPLE_OUT}
        changed["Ei"] = (out["Ei"] != c.Ei).any(1) | (miss & (add_env != 0).any(1)) | quad | (cons & (contrib != 0).any(1))
        changed["T"] = roul
        changed["N"] = cont & (turn | back)
        if c is not inputs:
            changed.update({k: np.ones(n, bool) for k in ("P", "uv", "hitT", "N")})          # the commit writes the record of every traced path
        exact = dict(hitI=c.hitI, mat=c.mat, alh=c.alh, pathLen=c.pathLen, seed=seed.astype(np.uint32), terminate=term, splat=term & (c.pathLen > 0), shadow=have,
                     blocked=np.where(pickQuad & ~lit, 1, c.blocked), backface=np.where(cont, back, False), cont=cont,
                     list=np.where(cont, np.vectorize(lambda t: LIST_OF.get(int(t), -1))(mtype), -1))
        info = dict(w_env=w_env, mis_env=mis_env, w_q=w_q, mis_q=mis_q, w_c=w_c, cons=cons, slot=slot, own=own, texel=texel, pickEnv=pickEnv,
                    pickQuad=pickQuad, lit=lit, r0=r0, r1=r1, r2=r2, roul=roul, stop=stop, contProb=contProb, turn=turn, back=back, miss=miss, quad=quad,
                    nee=nee, cosTh=cosTh, r_roul=r)
        return dict(out=out, changed=changed, exact=exact, info=info)
    return fn


class Verdict:
    """bsdf_cases.Verdict's method over the logic step's float outputs: nominal values, per-case decided flags, per-element tolerances."""

    def __init__(self, fn, n, seed=77):
        with np.errstate(all="ignore"):
            E0 = bc.Eval(n)
            self.nom = fn(E0)
            rng = np.random.RandomState(seed)
            runs = []
            for _ in range(bc.JITTER):
                E = bc.Eval(n, rng)
                runs.append((fn(E), E))
            flip = E0.bad.copy()
            for o, E in runs:
                flip |= E.bad
                assert len(E.branches) == len(E0.branches)
                for (i0, b0), (_, b1) in zip(E0.branches, E.branches):
                    flip[i0] |= b0 != b1
                for k, x in self.nom["exact"].items():
                    flip |= np.asarray(o["exact"][k] != x)
            self.flip = flip
            self.out, self.changed, self.exact, self.info = self.nom["out"], self.nom["changed"], self.nom["exact"], self.nom["info"]
            self.tol, ok = {}, ~flip
            for k in self.out:
                nom = self.out[k]
                spr = np.max([np.abs(o["out"][k] - nom) for o, _ in runs], axis=0)
                scale = np.max(np.abs(nom), axis=1, keepdims=True)
                finite = np.isfinite(nom).all(1) & np.isfinite(spr).all(1)
                ok &= finite & (spr.max(1) <= bc.MAX_SPREAD * scale[:, 0])
                self.tol[k] = bc.TOL_SPREAD * spr + bc.TOL_FLOOR * 2.0 ** -24 * scale
            self.decided = ok

    def ratio(self, k, got):
        """|got - out| / tol per case (the largest component)"""
        with np.errstate(all="ignore"):
            err = np.abs(np.asarray(got, np.float64) - self.out[k])
            return np.where(err == 0.0, 0.0, err / self.tol[k]).max(1)


@functools.lru_cache(None)
def verdict(cfg, mode):
    c = cases(cfg)
    return Verdict(restatement(scene(), c, mode), c.n)


def undecided_share(v, group):
    return {g: float((~v.decided[group == g]).mean()) for g in np.unique(group)}


# ---------------------------------------------------------------------------------------------------------------------------------
# the assertions on one run of the logic step
def check(v, c, st_in, st_out, px, counters, queues, what, chained=False, index=None):
    """st_in / st_out: reference-layout states (64, N) before and after; px: the framebuffer (N, 4) after, zero before; counters and
    queues after the step.  chained: genRays and the material kernels ran behind the logic step (terminating paths are regenerated, so
    only their pixel speaks for them; T, seed and the extension ray belong to the material step).  index: where case k sits in the
    state (default k).  Returns (largest error / tolerance, its label)."""
    n = c.n
    at = np.arange(n) if index is None else np.asarray(index)
    ui, uo = st_in.view(np.uint32), st_out.view(np.uint32)
    ex = v.exact
    term, cont, dec = ex["terminate"], ex["cont"], v.decided
    worst, worst_label = 0.0, ""
    for k, (col, w) in {**FLOAT_OUT, **RAW_OUT}.items():
        if (chained and k == "T") or k not in v.out:
            continue
        sel = dec & (cont if chained else np.ones(n, bool))
        got = st_out[col:col + w][:, at].T.astype(np.float64)
        r = np.where(sel, v.ratio(k, got), 0.0)
        i = int(np.argmax(r))
        if r[i] > worst:
            worst, worst_label = float(r[i]), f"{k} of case {i} ({c.group[i]}: {c.label[i]})"
        assert (r <= 1.0).all(), f"{what}: {k}: {int((r > 1.0).sum())} decided cases off float64, worst {r[i]:.3g} at {i} ({c.group[i]}: {c.label[i]}): " \
                                 f"{got[i].tolist()} vs {v.out[k][i].tolist()} (tol {v.tol[k][i].tolist()})"
        same = sel & ~v.changed[k]
        bad = same & (uo[col:col + w][:, at] != ui[col:col + w][:, at]).any(0)
        assert not bad.any(), f"{what}: {k} changed on {int(bad.sum())} paths the restatement leaves alone, first {int(np.argmax(bad))} ({c.label[int(np.argmax(bad))]})"
    # the pixel: Ei and one sample where a path ends with pathLen > 0, nothing elsewhere
    splat = ex["splat"]
    pix = np.asarray(px, np.float64)[at]
    r = np.where(dec & splat, v.ratio("Ei", pix[:, :3]), 0.0)
    i = int(np.argmax(r))
    if r[i] > worst:
        worst, worst_label = float(r[i]), f"pixel of case {i} ({c.group[i]}: {c.label[i]})"
    assert (r <= 1.0).all(), f"{what}: pixel: {int((r > 1.0).sum())} decided cases off float64, worst {r[i]:.3g} at {i} ({c.label[i]})"
    assert np.array_equal(pix[dec, 3], splat[dec].astype(np.float64)), f"{what}: sample counts"
    assert not np.asarray(px)[at][dec & ~splat].any(), f"{what}: a path that does not end (or ends with pathLen 0) wrote its pixel"
    if not chained:
        m = dec & splat
        assert np.array_equal(np.asarray(px, F)[at][m, :3].view(np.uint32), uo[COL.EI:COL.EI + 3][:, at].T[m]), f"{what}: the pixel of a lone path is its Ei"
    # exact outputs
    sel = dec & (cont if chained else np.ones(n, bool))
    if not chained:
        assert np.array_equal(uo[COL.SEED, at][sel], ex["seed"][sel]), f"{what}: seed"
    assert np.array_equal(uo[COL.SHADOW_BLOCKED, at][sel], ex["blocked"][sel].astype(np.uint32)), f"{what}: shadowRayBlocked"
    m = dec & cont
    assert np.array_equal(uo[COL.BACKFACE, at][m], ex["backface"][m].astype(np.uint32)), f"{what}: backfaceHit"
    if "P" in v.out:
        io = st_out.view(np.int32)
        for k, col in (("hitI", COL.HIT_I), ("mat", COL.MAT_ID), ("alh", COL.AREA_LIGHT_HIT), ("pathLen", COL.PATH_LEN)):
            assert np.array_equal(io[col, at][m], ex[k][m]), f"{what}: the committed {k}"
    # queue membership
    cnt = np.asarray(counters)
    member = lambda qi: np.isin(at, np.asarray(queues[qi][:int(cnt[qi])], np.int64))
    assert np.array_equal(member(Q.RAYGEN)[dec], term[dec]), f"{what}: raygen queue"
    assert np.array_equal(member(Q.SHADOW)[dec], ex["shadow"][dec]), f"{what}: shadow queue"
    for qi in (Q.DIFFUSE, Q.GLOSSY, Q.GGX_REFL, Q.GGX_REFR, Q.DELTA):
        assert np.array_equal(member(qi)[dec], (ex["list"] == qi)[dec]), f"{what}: material queue {qi}"
    return worst, worst_label


def snapshot(ctx):
    """(state, framebuffer, counters, queues) of a context once its stream has drained"""
    cnt = ctx.get_counters()
    ctx.finish()                                     # (the device's counters arrive with the stream)
    cnt = np.array(cnt, copy=True)
    return ctx.state_export().copy(), np.array(ctx.read_pixels(0), copy=True), cnt, {qi: ctx.queue_read(qi).copy() for qi in range(Q.NUM)}


def check_regenerated(v, c, st_out, counters, queues, n_tasks, npix, what):
    """genRays ran behind the logic step: the paths that ended -- the decided cases the restatement ends, and every inert path -- are
    regenerated, in path-id order, each on pixel cursor + rank (the cursor is 0 after a reset) with pathLen 0.  Their rays are out of scope."""
    cnt = int(np.asarray(counters)[Q.RAYGEN])
    rq = np.asarray(queues[Q.RAYGEN][:cnt], np.int64)
    assert (np.diff(rq) > 0).all(), f"{what}: the raygen queue is not in path-id order"
    inert = np.setdiff1d(np.arange(n_tasks), c.index if hasattr(c, "index") else np.arange(c.n))
    assert np.isin(inert, rq).all(), f"{what}: an inert path was not regenerated"
    undecided = int((~v.decided).sum())
    want = inert.size + int(v.exact["terminate"][v.decided].sum())
    assert want <= cnt <= want + undecided, f"{what}: {cnt} paths regenerated, the restatement ends {want} (+ at most {undecided} undecided)"
    u = st_out.view(np.uint32)
    assert np.array_equal(u[COL.PIXEL_INDEX, rq], np.arange(cnt) % npix), f"{what}: pixel words of the regenerated paths (cursor + rank)"
    assert (u[COL.PATH_LEN, rq] == 0).all(), f"{what}: pathLen of the regenerated paths"
    return cnt
