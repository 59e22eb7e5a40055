"""Cases of tests/test_gpu_wf_mesh_lights.py: the MESH instance of the plain logic pass (csrc/logic.hip).

  emissive_mixed_scene   common.mixed_material_scene() with Ke set on three materials (or none): the lockstep scene of "off is off".
  WfImplicit             mesh_light_step_cases.ImplicitCases as wavefront paths: loaded as logic_step_cases.load_rays loads its rays, traced by
                         wf_extend, then one wf_logic.  The parametric quad of the sub-cases is StepScene.quad_light(), 0.2 below the lamp
                         'quad_lamp': no other lamp's rays are aimed through it (ImplicitCases.quad_clear says which rays stay clear of its edge).
  implicit_restatement   float64, written from 4.2.3: relative to mesh_light_step_cases.implicit_restatement the kind probability 1 / den enters
                         the MIS weight, den = useEnvMap + useAreaLight + 1.
  WfSampled              mesh_light_step_cases.SampledCases as wavefront paths with committed hit records, every seed re-made so that its FIRST
                         draw (the kind draw) selects the lamps and draws 2 to 4 are the case's own (pick, r1, r2); kind_edges() are the seeds
                         at both thresholds of the kind draw and the draws on either side of them.
  sample_restatement     float64 of what the mesh sample stores (SAMPLE_OUT of logic_step_cases), per 4.2.3.
The mesh shadow rays of WfSampled are traced with useAreaLight = 0 wherever their verdict is compared with the brute force: the shadow kernels
test the parametric quad first (src/wf_shadowrays.cl:32-33), and the brute force knows only triangles -- mesh shadow rays are kept clear of the quad."""
import functools
import numpy as np
import bsdf_cases as bc
import common
import mesh_light_step_cases as SC
from common import COL

F = np.float32
EXTRA = SC.EXTRA
LIGHTS = {"none": dict(useEnvMap=0, useAreaLight=0), "env": dict(useEnvMap=1, useAreaLight=0, envMapStrength=1.5),
          "quad": dict(useEnvMap=0, useAreaLight=1), "both": dict(useEnvMap=1, useAreaLight=1, envMapStrength=1.5)}


def den_of(cfg):
    return LIGHTS[cfg]["useEnvMap"] + LIGHTS[cfg]["useAreaLight"] + 1


def emissive_mixed_scene(emissive=True):
    d = common.mixed_material_scene()
    if emissive:
        for m in (1, 3, 4):
            d.materials[m]["Ke"]["x"], d.materials[m]["Ke"]["y"], d.materials[m]["Ke"]["z"] = 3.0, 2.0, 1.0
    return d


# ---------------------------------------------------------------------------------------------------------------------------------
# implicit hits
class WfImplicit:
    def __init__(self, c):
        self.c, self.n = c, c.n
        self.n_tasks = c.n + EXTRA
        self.index = np.arange(c.n)

    def state(self, st):
        """the paths before the extension kernel traces them; every other path inert (T = 0, pathLen 0, no hit)"""
        c, u = self.c, st.view(np.uint32)
        n = c.n
        assert st.shape[1] == self.n_tasks
        st[COL.T:COL.T + 3, :] = 0.0
        st[COL.EI:COL.EI + 3, :] = 0.0
        u[COL.PATH_LEN, :] = 0
        u[COL.SHADOW_BLOCKED, :] = 1                                       # no light sample of an earlier vertex to consume
        u[COL.FIRST_DIFFUSE, :] = 0
        u[COL.BACKFACE, :] = 0
        st.view(np.int32)[COL.HIT_I, :] = -1
        st[COL.ORIG:COL.ORIG + 3, :n] = c.orig.T
        st[COL.DIR:COL.DIR + 3, :n] = c.dir.T
        st[COL.T:COL.T + 3, :n] = c.T.T
        st[COL.EI:COL.EI + 3, :n] = c.Ei.T
        st[COL.LAST_PDF_W, :n] = c.lastPdfW
        st[COL.LAST_PICK_PROB, :n] = 0.123                                 # never read by the mesh branch: the kind probability comes from the parameters
        u[COL.LAST_SPECULAR, :n] = c.lastSpecular
        u[COL.PATH_LEN, :n] = c.len_before
        u[COL.SEED, :n] = np.arange(n) * 2654435761 % 2 ** 32
        u[COL.PIXEL_INDEX, :] = np.arange(st.shape[1])
        return st


def implicit_restatement(S, c, tab, mode, den, quad=False):
    """fn(E) of SC.Verdict: Ei after the logic pass.  w = lastPdfW / (lastPdfW + pdf_a_to_w(pdfA, |hitP - rayOrig|, cos) (1 / den))"""
    expl, impl = mode
    pick = np.asarray(tab[2], np.float64)
    pickable = bool((pick > 0).any())
    n = c.n
    hit = c.hit >= 0
    tri = np.where(hit, c.hit, 0)
    k = S.listed(tri, tab)
    ke = S.ke[tri]
    emissive = hit & (ke > 0).any(1)
    len_after = c.len_before + 1
    counted = (len_after == 1) | bool(impl)
    alive = (c.T != 0).any(1)                                              # a path without throughput ends before anything is collected
    P3 = S.P[tri]
    kind = bc.F32(1.0) / bc.F32(den)

    def fn(E):
        E.idx = np.arange(n)
        dirj = E.j(c.dir)
        cr = E.j(np.cross(E.j(P3[:, 1] - P3[:, 0]), E.j(P3[:, 2] - P3[:, 0])))
        ng = E.normalize(cr)
        side = E.br((SC._dot(ng, dirj) < 0.0) & emissive)
        contrib = emissive & side & counted & alive
        if quad:
            contrib = contrib & ~c.quad_wins
        mis = contrib & bool(expl) & (len_after > 1) & (c.lastSpecular == 0) & pickable & (k >= 0)
        area = E.j(0.5 * np.sqrt(SC._dot(cr, cr)))
        pdfA = E.j(pick[np.maximum(k, 0)] / area)
        t = E.j(SC._dot(E.j(P3[:, 0] - c.orig), cr) / SC._dot(dirj, cr))
        X = E.j(c.orig + E.j(t[:, None] * dirj))
        d = E.j(np.sqrt(SC._dot(X - c.orig, X - c.orig)))
        cos = SC._dot(E.normalize(-dirj), ng)
        pdfW = E.j(E.j(pdfA * E.j(d * d) / np.abs(cos)) * float(kind))
        w = np.where(mis, E.j(c.lastPdfW / E.j(c.lastPdfW + pdfW)), 1.0)
        E.chk(np.where(mis, pdfW, 1.0))
        delta = np.where(contrib[:, None], E.j(E.j(c.T * w[:, None]) * ke), 0.0)
        return dict(out=c.Ei + delta, delta=delta, contrib=contrib, mis=mis, w=w)
    return fn


def implicit_verdict(S, c, tab, mode, cfg):
    quad = bool(LIGHTS[cfg]["useAreaLight"]) and bool(mode[1])             # the extension kernel meets the quad only under sampleImpl
    robust = c.robust & (c.hit >= 0) & ((c.quad_clear & ~c.quad_wins) if quad else True)
    return SC.Verdict(implicit_restatement(S, c, tab, mode, den_of(cfg), quad), c.n, robust), robust


@functools.lru_cache(None)
def implicit_cases():
    S = SC.step_scene()
    return S, SC.ImplicitCases(S)


# ---------------------------------------------------------------------------------------------------------------------------------
# sampled lights
def kind_thresholds(cfg):
    """the fp32 thresholds of the one kind draw: r < t_env selects the environment map, otherwise r < t_quad the quad, otherwise the lamps"""
    L, den = LIGHTS[cfg], den_of(cfg)
    return F(F(L["useEnvMap"]) / F(den)), F(F(L["useEnvMap"] + L["useAreaLight"]) / F(den))


def kind_of(cfg, r):
    te, tq = kind_thresholds(cfg)
    r = np.asarray(r, F)
    return np.where(r < te, 0, np.where(r < tq, 1, 2))                      # 0 environment, 1 quad, 2 lamps


def seed_before(seed, draws=1):
    """the seed whose stream, `draws` draws on, is the stream of `seed`"""
    s = np.asarray(seed, np.uint64)
    for _ in range(draws):
        s = bc.unhash_u32(s)
    return s


class WfSampled:
    """SampledCases with one more draw in front: the kind draw.  seed[i] is chosen so that draw 1 is `kind_draw[i]` and draws 2.. are the
    case's own stream -- possible exactly because a draw is the hash chain's next state: the case's seed is the state after the kind draw."""

    def __init__(self, c, cfg):
        self.c, self.n, self.cfg = c, c.n, cfg
        self.n_tasks = c.n + EXTRA
        self.seed = seed_before(c.seed).astype(np.uint64)
        self.kind_draw, after = bc.rand01(self.seed.copy())
        assert np.array_equal(after.astype(np.uint64), c.seed.astype(np.uint64))
        self.kind = kind_of(cfg, self.kind_draw)

    def state(self, st):
        c, u = self.c, st.view(np.uint32)
        n = c.n
        assert st.shape[1] == self.n_tasks
        st[COL.T:COL.T + 3, :] = 0.0
        st[COL.EI:COL.EI + 3, :] = 0.0
        u[COL.PATH_LEN, :] = 0
        u[COL.SHADOW_BLOCKED, :] = 1
        u[COL.FIRST_DIFFUSE, :] = 0
        u[COL.BACKFACE, :] = 0
        st.view(np.int32)[COL.HIT_I, :] = -1
        st[COL.P:COL.P + 3, :n] = c.P.T
        st[COL.N:COL.N + 3, :n] = c.N.T
        st[COL.UV:COL.UV + 2, :n] = c.uv.T
        st[COL.DIR:COL.DIR + 3, :n] = c.dir.T
        st[COL.ORIG:COL.ORIG + 3, :n] = (c.P - c.dir).T.astype(F)
        st[COL.T:COL.T + 3, :n] = c.T.T
        st[COL.EI:COL.EI + 3, :n] = c.Ei.T
        st[COL.HIT_T, :n] = 1.0
        st[COL.LAST_PDF_W, :n] = 1.0
        u[COL.SEED, :n] = self.seed.astype(np.uint32)
        u[COL.MAT_ID, :n] = c.mat
        u[COL.HIT_I, :n] = c.hitI
        u[COL.AREA_LIGHT_HIT, :n] = 0
        u[COL.PATH_LEN, :n] = 1
        u[COL.LAST_SPECULAR, :n] = 0
        u[COL.PIXEL_INDEX, :] = np.arange(st.shape[1])
        return st


def kind_edges(cfg):
    """fp32 kind draws at both thresholds and the reachable draws on either side of them, with the kind each must select"""
    out = []
    for t in sorted(set(float(x) for x in kind_thresholds(cfg))):
        if 0.0 < t < 1.0:
            for v in (SC.reachable(F(t)), SC.reachable(F(t), below=True), SC.reachable(np.nextafter(F(t), F(1.0)))):
                out.append(F(v))
    out += [F(0.0), F(1.0), SC.BELOW1]
    return np.array(out, F)


def sample_restatement(S, c, g, tab, den):
    """float64 of the stored light sample of a mesh pick, from 4.2.3: dict of (n, k) arrays + `lit` (cosLight > 0: the path joins the shadow queue)"""
    pick = np.asarray(tab[2], np.float64)
    P3 = S.P[g.tri]
    cr = np.cross(P3[:, 1] - P3[:, 0], P3[:, 2] - P3[:, 0])
    ng = cr / np.linalg.norm(cr, axis=1, keepdims=True)
    area = 0.5 * np.linalg.norm(cr, axis=1)
    Nn = np.where(c.back[:, None], -c.N, c.N)
    cosLight = np.maximum(SC._dot(ng, -g.L), 0.0)
    with np.errstate(all="ignore"):
        pdfW = pick[g.k] / area * g.lenL ** 2 / np.where(cosLight > 0, cosLight, 1.0)
    return dict(shadowOrig=g.orig, shadowDir=g.L, shadowRayLen=0.995 * g.lenL, lastPdfDirect=pdfW, lastEmission=S.ke[g.tri],
                lastCosTh=np.maximum(SC._dot(g.L, Nn), 0.0), lastLightPickProb=np.full(c.n, float(F(1.0) / F(den))), cosLight=cosLight)


SAMPLE_COLS = {"shadowOrig": (COL.SHADOW_ORIG, 3), "shadowDir": (COL.SHADOW_DIR, 3), "shadowRayLen": (COL.SHADOW_LEN, 1), "lastPdfDirect": (COL.LAST_PDF_DIRECT, 1),
               "lastEmission": (COL.LAST_EMISSION, 3), "lastCosTh": (COL.LAST_COS_TH, 1), "lastLightPickProb": (COL.LAST_PICK_PROB, 1)}
# Relative bounds of the fp32 evaluation against float64, in units of 2^-24, counted along the kernel's own operations (each rounds once):
#   shadowOrig    P - 1e-3 dir: 2 operations on values of the scene's size                                      -> 2 ulp of |P| + 1e-3
#   shadowDir     point (3 products, 2 sums, the coefficients 2 more) - orig, then normalize (3 + 2 + sqrt + div): the subtraction
#                 cancels -- its absolute error is 8 ulp of the scene's size, relative to |L|                    -> (8 size / |L| + 8) ulp
#   shadowRayLen  the same L, its length, one product                                                            -> (8 size / |L| + 6) ulp
#   lastPdfDirect pick / area (area: two edge differences, a cross product, a length: ~8) * |L|^2 / cosLight; cosLight = dot(n_g, -L)
#                 carries n_g's and L's errors in absolute terms, relative to cosLight                           -> (2 * 8 size / |L| + 24 + (16 + 8 size / |L|) / cosLight) ulp
#   lastCosTh     dot(L, N): absolute (8 size / |L| + 8) ulp
#   lastEmission, lastLightPickProb: exact (a copy; one division of small integers)
SIZE = 8.0                                                                  # the step scene fits in [-8, 8]^3


def sample_bounds(r):
    """absolute bounds, one (n, 1) array per column group"""
    u = 2.0 ** -24
    lenL = r["shadowRayLen"] / 0.995
    n = lenL.size
    canc = 8.0 * SIZE / lenL
    cl = np.where(r["cosLight"] > 0, r["cosLight"], 1.0)
    b = dict(shadowOrig=np.full(n, 2.0 * u * (SIZE + 1e-3)), shadowDir=(canc + 8.0) * u, shadowRayLen=(canc + 6.0) * u * r["shadowRayLen"],
             lastPdfDirect=(2.0 * canc + 24.0 + (16.0 + canc) / cl) * u * np.abs(r["lastPdfDirect"]), lastEmission=np.zeros(n),
             lastCosTh=(canc + 8.0) * u, lastLightPickProb=np.zeros(n))
    return {k: np.asarray(v, np.float64).reshape(n, 1) for k, v in b.items()}
