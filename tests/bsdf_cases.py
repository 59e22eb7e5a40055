"""Adversarial inputs for the material step (csrc/flx_bsdf.h material_step, oracle/wf_oracle.cpp k_material_queue), a float64 restatement of
the reference's BSDF formulas, and a classifier that says where fp32 can still be held to float64.

Device vs oracle is bit-exact, but both are hand restatements over the same include/flx_math.h, so a mistake made the same way in both passes
that comparison.  Here the question is "is this what the reference's formulas give?", asked in float64 on inputs chosen for the edges of the
BSDFs rather than for realism.

  Cases         64-column reference-layout states (wire.COL) + one queue entry per path, for every BSDF type: Ns / Ni / Ks / texture sweeps,
                cos(theta_i) down to +-0 and slightly negative, front and back faces, non-unit dir, NEE directions L above / below the horizon,
                +-N, the mirror direction, -dir, zero and grazing, seeds whose draws are exactly 0, exactly 1.0 or one ulp either side of the
                Fresnel threshold (hash_u32 inverted), and uv at 0, 1, -0, 1 - ulp, negative, 1e6, 3e9 / w, +-inf and NaN.
  Restatement   numpy float64, formula by formula from the reference (src/diffuse.cl, glossy.cl, ggx.cl, fresnel.cl, ideal_reflection.cl,
                ideal_dielectric.cl, bxdf_partial.cl, wf_mat_*.cl; utils.cl for the texel fetch): the RNG stream exactly in uint32, every output
                the material step writes.  The formulas are the target, not physical correctness (the GGX dielectric refracts about N).
  Classifier    a case is DECIDED when no branch the kernel takes flips across JITTER evaluations in which every computed fp32 value that enters
                the formulas (inputs, normalised vectors, transcendental arguments and results) moves by a few ulp, no value leaves the fp32
                range, and the outputs spread by at most MAX_SPREAD.  The tolerance of a decided case is derived from that spread, with a floor.
"""
import contextlib
import numpy as np
from fluctus_amd import wire
from common import COL, Q

BXDF = wire.BXDF
TYPES = (BXDF.DIFFUSE, BXDF.GLOSSY, BXDF.GGX_ROUGH_REFLECTION, BXDF.GGX_ROUGH_DIELECTRIC, BXDF.IDEAL_REFLECTION, BXDF.IDEAL_DIELECTRIC)
TYPE_NAMES = {BXDF.DIFFUSE: "diffuse", BXDF.GLOSSY: "glossy", BXDF.GGX_ROUGH_REFLECTION: "ggx_refl", BXDF.GGX_ROUGH_DIELECTRIC: "ggx_refr",
              BXDF.IDEAL_REFLECTION: "mirror", BXDF.IDEAL_DIELECTRIC: "dielectric"}
QUEUE_OF = {BXDF.DIFFUSE: Q.DIFFUSE, BXDF.GLOSSY: Q.GLOSSY, BXDF.GGX_ROUGH_REFLECTION: Q.GGX_REFL, BXDF.GGX_ROUGH_DIELECTRIC: Q.GGX_REFR,
            BXDF.IDEAL_REFLECTION: Q.DELTA, BXDF.IDEAL_DIELECTRIC: Q.DELTA}
DRAWS = {BXDF.DIFFUSE: 2, BXDF.GLOSSY: 3, BXDF.GGX_ROUGH_REFLECTION: 2, BXDF.GGX_ROUGH_DIELECTRIC: 3, BXDF.IDEAL_REFLECTION: 0,
         BXDF.IDEAL_DIELECTRIC: 1}
FRESNEL_DRAW = {BXDF.GLOSSY: 1, BXDF.GGX_ROUGH_DIELECTRIC: 3, BXDF.IDEAL_DIELECTRIC: 1}     # which draw the `rand < Fr` choice consumes

# ---- the classifier's constants, in one place ------------------------------------------------------------------------------------
JITTER = 16                   # jittered evaluations per case
ULPS = 4.0                    # relative jitter of every computed fp32 value, in units of 2^-24
MAX_SPREAD = 1e-3             # largest spread of an output (relative to the scale of its vector) a decided case may have
TOL_SPREAD = 4.0              # tolerance = TOL_SPREAD * spread + TOL_FLOOR * 2^-24 * scale
TOL_FLOOR = 16.0
FR_ABS = 4 * ULPS * 2.0 ** -24   # absolute fp32 error of a Fresnel reflectance (a ratio of O(1) terms, squared)
FP32_BIG, FP32_TINY = 1e37, 1e-36     # a value past these (in any evaluation) leaves fp32's normal range: undecided

F32 = lambda x: float(np.float32(x))
PI, INV_PI, TWO_PI = F32(3.14159265358979323846), F32(0.3183098861837907), F32(6.2831853071795864)
EPS_ORIG = F32(1e-4)
HORIZON = F32(1e-5)
OUTPUTS = {"lastBsdf": (COL.LAST_BSDF, 3), "lastPdfImplicit": (COL.LAST_PDF_IMPLICIT, 1), "T": (COL.T, 3), "orig": (COL.ORIG, 3),
           "lastPdfW": (COL.LAST_PDF_W, 1), "dir": (COL.DIR, 3)}


# ---------------------------------------------------------------------------------------------------------------------------------
# RNG (include/flx_math.h hash_u32 / rand01, src/random.cl), exactly in uint32
M32 = np.uint64(0xFFFFFFFF)


def hash_u32(s):
    s = np.asarray(s, np.uint64) & M32
    s = (s ^ np.uint64(61)) ^ (s >> np.uint64(16))
    s = (s * np.uint64(9)) & M32
    s = s ^ (s >> np.uint64(4))
    s = (s * np.uint64(0x27d4eb2d)) & M32
    s = s ^ (s >> np.uint64(15))
    return s


def _unxorshift(y, k):
    x = y.copy()
    for _ in range(32 // k + 1):
        x = y ^ (x >> np.uint64(k))
    return x & M32


def unhash_u32(h):
    """The inverse of hash_u32 (every step is a bijection of uint32)."""
    h = np.asarray(h, np.uint64) & M32
    s = _unxorshift(h, 15)
    s = (s * np.uint64(pow(0x27d4eb2d, -1, 1 << 32))) & M32
    s = _unxorshift(s, 4)
    s = (s * np.uint64(pow(9, -1, 1 << 32))) & M32
    hi = s >> np.uint64(16)
    return ((hi << np.uint64(16)) | ((s & np.uint64(0xFFFF)) ^ np.uint64(61) ^ hi)) & M32


def rand01(s):
    """(the draw as the kernels see it, the next seed): (float)(uint) * 2^-32, the conversion rounding to nearest fp32."""
    s = hash_u32(s)
    return s.astype(np.float32).astype(np.float64) * 2.0 ** -32, s


def seed_for_draw(k, value):
    """A seed whose k-th draw (1-based) is exactly `value` (an fp32 in [0, 1]; values below 2^-9 round to the nearest multiple of 2^-32)."""
    h = np.uint64(min(int(round(float(np.float32(value)) * 2.0 ** 32)), 0xFFFFFFFF))
    s = np.array([h], np.uint64)
    for _ in range(k):
        s = unhash_u32(s)
    return int(s[0])


# ---------------------------------------------------------------------------------------------------------------------------------
# textures: the nearest-texel fetch (src/utils.cl:114-133).  The texel index is integer logic on the reference's fp32 arithmetic, so it is
# restated in fp32 (np.float32), with the project's choice where the reference's int conversion is undefined (texel wrap).
def texel_coord(x, n):
    """x = uv * size as the kernels compute it (fp32), n the texture size: the texel coordinate, or an exception if it left [0, n)."""
    x = np.atleast_1d(np.asarray(x, np.float32))
    out = np.zeros(x.shape, np.int64)
    fin = np.isfinite(x)
    with np.errstate(all="ignore"):
        f = np.floor(x)
        fi = np.where(fin, f, 0).astype(np.float64)
        u = np.where(np.abs(fi) < 2.0 ** 63, np.mod(fi, 2.0 ** 32), 0.0)          # floor(x) modulo 2^32 (exact: fi is an integer)
        t = (u.astype(np.uint64) % np.uint64(n)).astype(np.int64)
        c = (t.astype(np.float32) + x) - f                                        # the reference's (tx + uv - floor(uv)), in fp32
        c = np.where(fin, c, 0).astype(np.float64)
    assert (np.abs(c) < 2.0 ** 31).all(), "the texel coordinate's int conversion would be undefined"
    out[:] = np.clip(np.trunc(c), 0, n - 1)
    return out


class Textures:
    """A texture set (wire TEXDESC + RGBA8 bytes) and its fetch."""

    def __init__(self, sizes, seed=11):
        rng = np.random.RandomState(seed)
        self.desc = np.zeros(len(sizes), wire.TEXDESC)
        data, off = [], 0
        for i, (w, h) in enumerate(sizes):
            t = rng.randint(0, 256, size=(h, w, 4)).astype(np.uint8)
            t[..., 3] = 255
            t[0, 0, :3] = (0, 1, 255)                                     # texel 0: a black-ish channel (pow(0, 2.2) = 0) and a full one
            self.desc[i] = (off, w, h)
            data.append(t.reshape(-1))
            off += t.size
        self.data = np.concatenate(data).astype(np.uint8)

    def fetch(self, idx, uv):
        """(n, 3) float64 texel / 255 of texture idx[i] at uv[i] (idx -1: NaN, the caller uses its fallback)."""
        out = np.full((uv.shape[0], 3), np.nan)
        for k in range(self.desc.size):
            m = idx == k
            if not m.any():
                continue
            off, w, h = (int(v) for v in self.desc[k])
            cx = texel_coord(uv[m, 0].astype(np.float32) * np.float32(w), w)
            cy = texel_coord(uv[m, 1].astype(np.float32) * np.float32(h), h)
            p = off + (cx + cy * w) * 4
            out[m] = np.stack([self.data[p], self.data[p + 1], self.data[p + 2]], 1) / 255.0
        return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the float64 restatement
def _dot(a, b):
    return (a * b).sum(-1)


def _cross(a, b):
    return np.cross(a, b)


class Eval:
    """One evaluation of the restatement: nominal (rng None) or jittered.  Records every branch outcome and every case whose values leave
    the fp32 range."""

    def __init__(self, n, rng=None):
        self.rng = rng
        self.branches = []
        self.bad = np.zeros(n, bool)
        self.idx = None
        self.mask = None

    @contextlib.contextmanager
    def only(self, m):
        """Branches and ranges inside count only where m holds (the side of a choice the case takes; both sides are computed)."""
        old = self.mask
        self.mask = np.asarray(m, bool) if old is None else old & m
        yield
        self.mask = old

    def j(self, x, k=1.0):
        """A computed fp32 value: moved by up to k * ULPS ulp in a jittered evaluation."""
        x = np.asarray(x, np.float64)
        if self.rng is None:
            return x
        return x * (1.0 + k * ULPS * 2.0 ** -24 * self.rng.uniform(-1.0, 1.0, x.shape))

    def br(self, cond, near=None):
        """A branch; `near`: where its outcome is within fp32 error of the other anyway (a comparison whose sides are that close)."""
        cond = np.asarray(cond, bool)
        c = cond.reshape(cond.shape[0], -1).any(1) if cond.ndim > 1 else cond
        self.branches.append((self.idx, c if self.mask is None else c & self.mask))
        if near is not None:
            self.bad[self.idx] |= near if self.mask is None else near & self.mask
        return cond

    def fresnel_choice(self, u, fr):
        """`rand < Fr`.  Fr is a sum of squares: it cannot change sign under jitter, but fp32 can round it to exactly 0 (Ni = 1) or move it
        by a few ulp of 1 -- a draw that close to it is undecided."""
        return self.br(u < fr, near=~(np.abs(u - fr) > FR_ABS))

    def chk(self, x):
        a = np.abs(np.asarray(x, np.float64))
        a = a.reshape(a.shape[0], -1) if a.ndim > 1 else a[:, None]
        big = ~(a <= FP32_BIG) & ~np.isnan(a)
        tiny = (a > 0) & (a < FP32_TINY)
        bad = (big | tiny).any(1)
        self.bad[self.idx] |= bad if self.mask is None else bad & self.mask
        return x

    # ---- vector helpers with the flx_math.h contract (normalize: zero stays zero)
    def normalize(self, a):
        l2 = _dot(a, a)
        self.chk(l2)
        with np.errstate(all="ignore"):
            r = np.where((l2 == 0)[:, None], a, a / np.sqrt(l2)[:, None])
        return self.j(r)

    def sincos(self, x):
        x = self.j(x)
        return self.j(np.sin(x)), self.j(np.cos(x))

    def sqrt(self, x):
        return self.j(np.sqrt(x))


class Case:
    """The inputs of the material step for n paths (float64 holding fp32 values)."""
    FIELDS = ("P", "N", "uv", "dir", "L", "T", "seed", "backface", "mat")

    def __init__(self, **kw):
        for k in self.FIELDS:
            setattr(self, k, kw[k])


def _fresnel(E, cosI, etaI, etaT):
    """src/fresnel.cl:5-20."""
    sinI = E.sqrt(np.fmax(0.0, 1.0 - cosI * cosI))
    sinT = E.j(etaI / etaT) * sinI
    cosT = E.sqrt(np.fmax(0.0, 1.0 - sinT * sinT))
    tir = E.br(sinT >= 1.0)
    parl = E.j((etaT * cosI - etaI * cosT) / (etaT * cosI + etaI * cosT))
    perp = E.j((etaI * cosI - etaT * cosT) / (etaI * cosI + etaT * cosT))
    return np.where(tir, 1.0, 0.5 * (parl * parl + perp * perp))


def _reflect(d, n):
    return d - 2.0 * _dot(d, n)[:, None] * n


def _refract(wi, n, eta):
    """src/utils.cl:36-43."""
    iDotN = _dot(-wi, n)
    sin2I = np.fmax(0.0, 1.0 - iDotN * iDotN)
    sin2T = eta * eta * sin2I
    cosT = np.sqrt(np.fmax(0.0, 1.0 - sin2T))
    return wi * eta[:, None] + n * (eta * iDotN - cosT)[:, None]


def _alpha(E, Ns):
    """src/ggx.cl toRoughness."""
    with np.errstate(all="ignore"):
        return E.sqrt(E.j(2.0 / (2.0 + Ns)))


def _lobe(E, alpha, N, seed):
    """src/ggx.cl:sampleGGX with utils.cl makeOrthoBasis: the microfacet normal H, two draws."""
    neq = (N[:, 0] != N[:, 1]) | (N[:, 0] != N[:, 2])
    X = np.where(neq[:, None], np.stack([N[:, 2] - N[:, 1], N[:, 0] - N[:, 2], N[:, 1] - N[:, 0]], 1),
                 np.stack([N[:, 2] - N[:, 1], N[:, 0] + N[:, 2], -N[:, 1] - N[:, 0]], 1))
    X = E.normalize(X)
    Y = E.j(_cross(N, X))
    rx, seed = rand01(seed)
    ry, seed = rand01(seed)
    theta = E.j(np.arctan2(E.j(alpha * E.sqrt(rx)), E.sqrt(1.0 - rx)))
    phi = E.j(TWO_PI * ry)
    sT, cT = E.sincos(theta)
    sP, cP = E.sincos(phi)
    return E.normalize(X * (sT * cP)[:, None] + Y * (sT * sP)[:, None] + N * cT[:, None]), seed


def _g1(E, alpha, v, n, m):
    mDotV, nDotV = _dot(m, v), _dot(n, v)
    zero = E.br(nDotV * mDotV <= 0.0)
    c2 = nDotV * nDotV
    with np.errstate(all="ignore"):
        tan2 = np.where(c2 > 0.0, (1.0 - c2) / c2, 0.0)
        r = 2.0 / (1.0 + E.sqrt(1.0 + alpha * alpha * tan2))
    E.chk(np.where(zero, 1.0, tan2))
    return np.where(zero, 0.0, r)


def _d(E, alpha, n, m):
    nDotM = _dot(n, m)
    neg = E.br(nDotM <= 0.0)
    c2 = nDotM * nDotM
    a2 = alpha * alpha
    with np.errstate(all="ignore"):
        tan2 = np.where(nDotM != 0.0, (1.0 - c2) / c2, 0.0)
        den = PI * c2 * c2 * (a2 + tan2) * (a2 + tan2)
        r = np.where(den > 0.0, a2 / den, 0.0)
    E.chk(np.where(neg, 1.0, den))
    E.br(~neg & (den > 0.0))
    return np.where(neg, 0.0, r)


def _pdf_reflect(E, alpha, dirOut, N, H):
    nDotH, oDotH = np.abs(_dot(N, H)), np.abs(_dot(dirOut, H))
    jInv = 4.0 * oDotH
    z = E.br(jInv == 0.0)
    with np.errstate(all="ignore"):
        return np.where(z, 0.0, _d(E, alpha, N, H) * nDotH / jInv)


def _pdf_refract(E, alpha, etaI, etaO, dirIn, dirOut, N, H):
    nDotH, iDotH, oDotH = np.abs(_dot(N, H)), np.abs(_dot(dirIn, H)), np.abs(_dot(dirOut, H))
    s = etaI * iDotH + etaO * oDotH
    z = E.br(s == 0.0)
    with np.errstate(all="ignore"):
        return np.where(z, 0.0, _d(E, alpha, N, H) * nDotH * oDotH * etaO * etaO / (s * s))


class Restatement:
    """The material step of every case, in float64.  `m` is the material table (wire MATERIAL), `tex` the Textures."""

    def __init__(self, mats, tex):
        self.mats, self.tex = mats, tex

    # ---- material parameters
    def _ks(self, E, c, Ks, mapKs):
        t = self.tex.fetch(mapKs, c.uv) if mapKs is not None else None
        return Ks if t is None else np.where((mapKs != -1)[:, None], t, Ks)

    def _albedo(self, E, c, Kd, mapKd):
        """src/utils.cl:136-141 matGetAlbedo: pow(., 2.2); powf_ of x <= FLT_MIN is 0 (include/flx_math.h)."""
        v = np.where((mapKd != -1)[:, None], self.tex.fetch(mapKd, c.uv), Kd)
        with np.errstate(all="ignore"):
            lg = np.log(np.where(v > 1.17549435e-38, v, 1.0))
            r = E.j(np.exp(2.2 * lg), 1.0 + np.abs(2.2 * lg))           # exp's error grows with its argument
        return np.where(v > 1.17549435e-38, r, 0.0)

    # ---- the six BSDFs: (f, pdf) toward L and the sample
    def diffuse(self, E, c, m, dirIn, L, seed):
        alb = self._albedo(E, c, m["Kd"], m["mapKd"]) * INV_PI
        f, pdfL = alb, _dot(c.N, L) * INV_PI
        # src/utils.cl:83-112 cosSampleHemisphere
        r1, seed = rand01(seed)
        r2, seed = rand01(seed)
        r1 = E.j(2.0 * PI * r1)
        r2s = E.sqrt(r2)
        w = c.N
        big = np.abs(w[:, 0]) > 0.1
        u = np.where(big[:, None], _cross(np.array([0.0, 1.0, 0.0]), w), _cross(np.array([1.0, 0.0, 0.0]), w))
        u = E.normalize(u)
        v = E.j(_cross(w, u))
        s, co = E.sincos(r1)
        d = u * (co * r2s)[:, None] + v * (s * r2s)[:, None] + w * E.sqrt(1.0 - r2)[:, None]
        pdf = E.j(_dot(c.N, d) / PI)
        return f, pdfL, alb, d, pdf, seed

    def _ggx_reflect_eval(self, E, c, Ks, mapKs, alpha, Ni, dirIn, dirOut, H=None):
        """src/ggx.cl:115-136 (H given: the sampler's microfacet normal, :89-113)."""
        wi = -dirIn
        if H is None:
            H = E.normalize(wi + dirOut)
        iDotN, oDotN = _dot(wi, c.N), _dot(dirOut, c.N)
        gt = E.br(Ni > 1.0)
        with E.only(gt):
            fr = np.where(gt, _fresnel(E, iDotN, np.ones_like(Ni), Ni), 1.0)
        ks = self._ks(E, c, Ks, mapKs)
        D = _d(E, alpha, c.N, H)
        G = _g1(E, alpha, wi, c.N, H) * _g1(E, alpha, dirOut, c.N, H)
        den = 4.0 * iDotN * oDotN
        z = E.br(den == 0.0)
        with np.errstate(all="ignore"):
            r = ks * (fr * G * D / den)[:, None]
        E.chk(np.where(z, 1.0, den))
        return np.where(z[:, None], 0.0, r)

    def _ggx_reflect_pdf(self, E, c, alpha, dirIn, dirOut):
        H = E.normalize(-dirIn + dirOut)
        return _pdf_reflect(E, alpha, dirOut, c.N, H)

    def _ggx_reflect_sample(self, E, c, Ks, mapKs, alpha, Ni, dirIn, seed):
        H, seed = _lobe(E, alpha, c.N, seed)
        d = E.j(_reflect(dirIn, H))                  # reflect(-(-dirIn), H)
        pdf = _pdf_reflect(E, alpha, d, c.N, H)
        return self._ggx_reflect_eval(E, c, Ks, mapKs, alpha, Ni, dirIn, d, H), d, pdf, seed

    def ggx_refl(self, E, c, m, dirIn, L, seed):
        alpha = _alpha(E, m["Ns"])
        f = self._ggx_reflect_eval(E, c, m["Ks"], m["mapKs"], alpha, m["Ni"], dirIn, L)
        pdfL = self._ggx_reflect_pdf(E, c, alpha, dirIn, L)
        b, d, pdf, seed = self._ggx_reflect_sample(E, c, m["Ks"], m["mapKs"], alpha, m["Ni"], dirIn, seed)
        return f, pdfL, b, d, pdf, seed

    def glossy(self, E, c, m, dirIn, L, seed):
        """src/glossy.cl: a Fresnel-blended diffuse base under a GGX coat."""
        Ks = self._ks(E, c, m["Ks"], m["mapKs"])
        k = np.clip(Ks.sum(1) / 3.0, 0.0, F32(0.99))
        Ni = np.where(m["Ni"] > 0.0, m["Ni"], E.j((E.sqrt(k) + 1.0) / (1.0 - E.sqrt(k))))
        alpha = _alpha(E, m["Ns"])
        cosTh = _dot(E.normalize(-dirIn), c.N)
        fr = _fresnel(E, cosTh, np.ones_like(Ni), Ni)
        # eval / pdf toward L (:66-101): Ks of a zero length from eta (eval only; the sampler tests isZero -- the same for Ks >= 0)
        with np.errstate(all="ignore"):
            r = np.where(Ni > 0.0, (Ni - 1.0) / (Ni + 1.0), 0.0)
        KsE = np.where((Ks == 0).all(1)[:, None], np.repeat((r * r)[:, None], 3, 1), Ks)
        alb = self._albedo(E, c, m["Kd"], m["mapKd"]) * INV_PI
        coatL = self._ggx_reflect_eval(E, c, KsE, m["mapKs"], alpha, Ni, dirIn, L)
        f = alb * (1.0 - fr)[:, None] + coatL
        pdfL = (1.0 - fr) * (_dot(c.N, L) * INV_PI) + fr * self._ggx_reflect_pdf(E, c, alpha, dirIn, L)
        # the sample (:24-64)
        u, seed = rand01(seed)
        spec = E.fresnel_choice(u, fr)
        with E.only(spec):
            bS, dS, pS, seedS = self._ggx_reflect_sample(E, c, KsE, m["mapKs"], alpha, Ni, dirIn, seed)
        with E.only(~spec):
            _, _, albD, dD, pD, seedD = self.diffuse(E, c, m, dirIn, L, seed)
            coatD = self._ggx_reflect_eval(E, c, KsE, m["mapKs"], alpha, Ni, dirIn, dD)
            coatPdfD = self._ggx_reflect_pdf(E, c, alpha, dirIn, dD)
        d = np.where(spec[:, None], dS, dD)
        base = np.where(spec[:, None], alb, albD)
        basePdf = np.where(spec, _dot(c.N, dS) * INV_PI, pD)
        coat = np.where(spec[:, None], bS, coatD)
        coatPdf = np.where(spec, pS, coatPdfD)
        seed = np.where(spec, seedS, seedD)
        below = E.br(_dot(c.N, d) < HORIZON)
        pdf = np.where(below, 0.0, (1.0 - fr) * basePdf + fr * coatPdf)
        b = np.where(below[:, None], 0.0, base * (1.0 - fr)[:, None] + coat)
        return f, pdfL, b, d, pdf, seed

    def ggx_refr(self, E, c, m, dirIn, L, seed):
        """src/ggx.cl:156-292."""
        alpha = _alpha(E, m["Ns"])
        bf = c.backface
        etaI = np.where(bf, m["Ni"], 1.0)
        etaO = np.where(bf, 1.0, m["Ni"])
        wi = -dirIn
        wiN = E.normalize(wi)
        iDotN = _dot(wiN, c.N)
        fr = _fresnel(E, iDotN, etaI, etaO)
        Nn = np.where(bf[:, None], -c.N, c.N)
        ks = self._ks(E, c, m["Ks"], m["mapKs"])
        eta = E.j(etaI / etaO)

        def refr_f(dOut, dRaw, H, oDotN, Nn):
            iDotH, oDotH = np.abs(_dot(wiN, H)), np.abs(_dot(dOut, H))
            s = etaI * iDotH + etaO * oDotH
            den = iDotN * oDotN * s * s
            z = E.br(den == 0.0)
            E.chk(np.where(z, 1.0, den))
            with np.errstate(all="ignore"):
                focus = etaO * etaO * iDotH * oDotH / den
                D, G = _d(E, alpha, Nn, H), _g1(E, alpha, wi, Nn, H) * _g1(E, alpha, dRaw, Nn, H)
                r = (eta * eta)[:, None] * ks * ((1.0 - fr) * D * G * focus)[:, None]
            return np.where(z[:, None], 0.0, r)

        def refl_f(dOut, H, oDotN):
            D, G = _d(E, alpha, c.N, H), _g1(E, alpha, wi, c.N, H) * _g1(E, alpha, dOut, c.N, H)
            den = 4.0 * iDotN * oDotN
            z = E.br(den == 0.0)
            E.chk(np.where(z, 1.0, den))
            with np.errstate(all="ignore"):
                return np.where(z, 0.0, fr * G * D / den)

        # eval / pdf toward L: reflection on the front, transmission on the back (:223-292)
        LN = E.normalize(L)
        oDotNL = _dot(LN, c.N)
        Hf = E.normalize(wi + L)
        Hb = E.normalize(-(wi * etaI[:, None] + L * etaO[:, None]))
        with E.only(~bf):
            front = np.repeat(refl_f(L, Hf, oDotNL)[:, None], 3, 1)
            pdfF = _pdf_reflect(E, alpha, L, c.N, Hf)
        with E.only(bf):
            back = refr_f(LN, L, Hb, oDotNL, -c.N)
            pdfB = _pdf_refract(E, alpha, etaI, etaO, wi, L, -c.N, Hb)
        f = np.where(bf[:, None], back, front)
        pdfL = np.where(bf, pdfB, pdfF)
        # the sample (:156-221)
        raylen = E.j(np.sqrt(_dot(wi, wi)))
        H, seed = _lobe(E, alpha, c.N, seed)
        u, seed = rand01(seed)
        refl = E.fresnel_choice(u, fr)
        with E.only(refl):
            dR = E.j(raylen[:, None] * _reflect(-wiN, H))
            pR = _pdf_reflect(E, alpha, dR, c.N, H)
            bR = np.repeat(refl_f(dR, H, _dot(dR, c.N))[:, None], 3, 1)
        with E.only(~refl):
            dT = E.j(raylen[:, None] * _refract(-wiN, c.N, eta))
            HT = E.normalize(-(wi * etaI[:, None] + dT * etaO[:, None]))
            pT = _pdf_refract(E, alpha, etaI, etaO, wi, dT, Nn, HT)
            bT = refr_f(dT, dT, HT, _dot(dT, c.N), Nn)
        return (f, pdfL, np.where(refl[:, None], bR, bT), np.where(refl[:, None], dR, dT), np.where(refl, pR, pT), seed)

    def mirror(self, E, c, m, dirIn, L, seed):
        """src/ideal_reflection.cl:9-22."""
        ln = E.j(np.sqrt(_dot(dirIn, dirIn)))
        d = E.j(ln[:, None] * _reflect(E.normalize(dirIn), c.N))
        ks = self._ks(E, c, m["Ks"], m["mapKs"])
        cosO = _dot(E.normalize(d), c.N)
        z = E.br(cosO == 0.0)
        with np.errstate(all="ignore"):
            b = np.where(z[:, None], 0.0, ks / cosO[:, None])
        E.chk(np.where(z, 1.0, cosO))
        zero = np.zeros_like(ln)
        return np.zeros_like(d), zero, b, d, np.ones_like(ln), seed

    def dielectric(self, E, c, m, dirIn, L, seed):
        """src/ideal_dielectric.cl:10-45."""
        raylen = E.j(np.sqrt(_dot(dirIn, dirIn)))
        cosI = _dot(E.normalize(-dirIn), c.N)
        n1 = np.where(c.backface, m["Ni"], 1.0)
        n2 = np.where(c.backface, 1.0, m["Ni"])
        eta = E.j(n1 / n2)
        fr = _fresnel(E, cosI, n1, n2)
        u, seed = rand01(seed)
        refl = E.fresnel_choice(u, fr)
        dn = E.normalize(dirIn)
        d = E.j(raylen[:, None] * np.where(refl[:, None], _reflect(dn, c.N), _refract(dn, c.N, eta)))
        ks = self._ks(E, c, m["Ks"], m["mapKs"])
        b = np.where(refl[:, None], 1.0, (eta * eta)[:, None] * ks)
        cosO = _dot(E.normalize(d), c.N)
        E.chk(cosO)
        with np.errstate(all="ignore"):
            b = b / cosO[:, None]
        zero = np.zeros_like(raylen)
        return np.zeros_like(d), zero, b, d, np.ones_like(raylen), seed

    FN = {BXDF.DIFFUSE: "diffuse", BXDF.GLOSSY: "glossy", BXDF.GGX_ROUGH_REFLECTION: "ggx_refl", BXDF.GGX_ROUGH_DIELECTRIC: "ggx_refr",
          BXDF.IDEAL_REFLECTION: "mirror", BXDF.IDEAL_DIELECTRIC: "dielectric"}

    def _mat_arrays(self, E, mid):
        mt = self.mats[mid]
        v3 = lambda f: np.stack([mt[f][k] for k in "xyz"], 1).astype(np.float64)
        return {"Kd": E.j(v3("Kd")), "Ks": E.j(v3("Ks")), "Ns": mt["Ns"].astype(np.float64), "Ni": mt["Ni"].astype(np.float64),
                "mapKd": mt["map_Kd"].astype(np.int64), "mapKs": mt["map_Ks"].astype(np.int64), "type": mt["type"].astype(np.int64)}

    def run(self, c, E):
        """{output: (n, k) float64} + seed (uint32) + lastSpecular for every case (wf_mat_*.cl:30-62)."""
        n = c.N.shape[0]
        out = {k: np.zeros((n, w)) for k, (_, w) in OUTPUTS.items()}
        seed_out = np.zeros(n, np.uint64)
        mt = self.mats["type"][c.mat]
        for t in TYPES:
            idx = np.nonzero(mt == t)[0]
            if not idx.size:
                continue
            E.idx = idx
            s = Case(**{k: getattr(c, k)[idx] for k in Case.FIELDS})
            s.N, s.P, s.T = E.j(s.N), E.j(s.P), E.j(s.T)
            dirIn, L = E.j(s.dir), E.j(s.L)
            m = self._mat_arrays(E, s.mat)
            f, pdfL, b, d, pdf, seed = getattr(self, self.FN[t])(E, s, m, dirIn, L, s.seed.astype(np.uint64))
            with np.errstate(all="ignore"):
                f = f * np.ones((1, 3))
                costh = _dot(s.N, E.normalize(d))
                zero = E.br((pdf == 0.0) | (b == 0.0).all(1))
                newT = np.where(zero[:, None], 0.0, s.T * b * (costh / pdf)[:, None])
            E.chk(np.where(zero[:, None], 0.0, newT))
            E.chk(np.where(zero, 1.0, pdf))
            out["lastBsdf"][idx] = f
            out["lastPdfImplicit"][idx, 0] = np.fmax(0.0, pdfL)
            out["T"][idx] = newT
            out["orig"][idx] = s.P + EPS_ORIG * d
            out["lastPdfW"][idx, 0] = pdf
            out["dir"][idx] = d
            seed_out[idx] = seed
        return out, seed_out.astype(np.uint32), ((mt & (BXDF.IDEAL_REFLECTION | BXDF.IDEAL_DIELECTRIC)) != 0).astype(np.uint32)


class Verdict:
    """Nominal float64 outputs, per-case decided flags and per-element tolerances."""

    def __init__(self, rs, c, seed=1234):
        n = c.N.shape[0]
        with np.errstate(all="ignore"):
            E0 = Eval(n)
            self.out, self.seed, self.singular = rs.run(c, E0)
            runs = []
            rng = np.random.RandomState(seed)
            for _ in range(JITTER):
                E = Eval(n, rng)
                o, s, _ = rs.run(c, E)
                assert np.array_equal(s, self.seed)            # the seed stream does not depend on the jitter
                runs.append((o, E))
        flip = E0.bad.copy()
        for o, E in runs:
            flip |= E.bad
            assert len(E.branches) == len(E0.branches)
            for (i0, b0), (i1, b1) in zip(E0.branches, E.branches):
                flip[i0] |= b0 != b1
        self.flip = flip
        self.tol, spread_ok = {}, ~flip
        for k in OUTPUTS:
            nom = self.out[k]
            with np.errstate(all="ignore"):
                spr = np.max([np.abs(o[k] - nom) for o, _ in runs], axis=0)
                scale = np.max(np.abs(nom), axis=1, keepdims=True)
                finite = np.isfinite(nom).all(1) & np.isfinite(spr).all(1)
                spread_ok &= finite & (spr.max(1) <= MAX_SPREAD * scale[:, 0])
                self.tol[k] = TOL_SPREAD * spr + TOL_FLOOR * 2.0 ** -24 * scale
        self.decided = spread_ok

    def check(self, st, mask=None):
        """Failures of a reference-layout state (64, >= n) against the float64 outputs on the decided cases (and `mask`)."""
        n = self.seed.size
        fails = []
        m = self.decided if mask is None else self.decided & mask
        for k, (col, w) in OUTPUTS.items():
            got = st[col:col + w, :n].T.astype(np.float64)
            with np.errstate(all="ignore"):
                bad = ~(np.abs(got - self.out[k]) <= self.tol[k]).all(1) & m
            if bad.any():
                i = int(np.argmax(bad))
                fails.append(f"{k}: {int(bad.sum())} decided cases off float64, first {i}: {got[i].tolist()} vs {self.out[k][i].tolist()} "
                             f"(tol {self.tol[k][i].tolist()})")
        return fails


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
NS_SWEEP = [0.0, 1e-3, 1.0, 60.0, 5000.0, 1e4, 1e5, 1e7, 1e30, F32(np.nextafter(np.float32(-2), np.float32(0))), -1.99, -1.5]
NI_SWEEP = [0.0, 0.67, F32(np.nextafter(np.float32(1), np.float32(0))), 1.0, F32(np.nextafter(np.float32(1), np.float32(2))), 1.5, 2.4, 1e3]
KS_SWEEP = [(0.0, 0.0, 0.0), (0.9, 0.5, 0.1), (0.04, 0.04, 0.04)]
TEX_SIZES = [(16, 16), (3, 5), (8, 8)]          # 0: a power of two wide, 1: not, 2: the normal map
COS_SWEEP = [1.0, 0.5, 1e-2, 1e-4, 1e-7, 0.0, -0.0, -1e-3]
UV_SWEEP = [0.0, 1.0, -0.0, F32(np.nextafter(np.float32(1), np.float32(0))), -0.3, -2.7, 1e6, np.inf, -np.inf, np.nan]
L_KINDS = ("above", "below", "+N", "-N", "mirror", "-dir", "zero", "grazing")


def materials():
    """(material table, [(type, label, material index)]): per type a base, and the sweeps of the parameters it reads."""
    from common import make_material
    out, tags = [], []

    def add(t, label, **kw):
        out.append(make_material(t, **kw))
        tags.append((t, label, len(out) - 1))

    base = {BXDF.DIFFUSE: dict(kd=(0.6, 0.5, 0.4)), BXDF.GLOSSY: dict(kd=(0.2, 0.5, 0.7), ks=(0.3, 0.3, 0.3), ns=300.0, ni=1.5),
            BXDF.GGX_ROUGH_REFLECTION: dict(ks=(0.9, 0.8, 0.5), ns=60.0, ni=1.5), BXDF.GGX_ROUGH_DIELECTRIC: dict(ks=(0.95, 0.9, 0.85), ns=400.0, ni=1.5),
            BXDF.IDEAL_REFLECTION: dict(ks=(0.9, 0.9, 0.9)), BXDF.IDEAL_DIELECTRIC: dict(ks=(0.9, 0.95, 1.0), ni=1.5)}
    for t in TYPES:
        add(t, "base", **base[t])
        if t in (BXDF.GLOSSY, BXDF.GGX_ROUGH_REFLECTION, BXDF.GGX_ROUGH_DIELECTRIC):
            for ns in NS_SWEEP:
                add(t, f"Ns={ns:g}", **{**base[t], "ns": ns})
        if t in (BXDF.GLOSSY, BXDF.GGX_ROUGH_REFLECTION, BXDF.GGX_ROUGH_DIELECTRIC, BXDF.IDEAL_DIELECTRIC):
            for ni in NI_SWEEP:
                add(t, f"Ni={ni:.9g}", **{**base[t], "ni": ni})
        if t != BXDF.DIFFUSE:
            for ks in KS_SWEEP:
                add(t, f"Ks={ks}", **{**base[t], "ks": ks})
        for k in (0, 1):                                                   # Kd / Ks from a texture (power of two wide, and not)
            if t in (BXDF.DIFFUSE, BXDF.GLOSSY):
                add(t, f"mapKd{k}", **{**base[t], "map_kd": k})
            if t != BXDF.DIFFUSE:
                add(t, f"mapKs{k}", **{**base[t], "map_ks": k})
        if t == BXDF.GLOSSY:
            add(t, "Ni=0 mapKs0", **{**base[t], "ni": 0.0, "map_ks": 0})
            add(t, "Ni=0 Ks=0", **{**base[t], "ni": 0.0, "ks": (0.0, 0.0, 0.0)})
        add(t, "mapN", **{**base[t], "map_n": 2})
    return np.array(out, wire.MATERIAL), tags


def _frame(kind, rng):
    """An orthonormal (N, tangent) pair: axis-aligned (exact fp32 zeros in the dot products) or tilted."""
    if kind == 0:
        return np.array([0.0, 1.0, 0.0]), np.array([1.0, 0.0, 0.0])
    n = rng.normal(size=3)
    n /= np.linalg.norm(n)
    t = np.cross(n, rng.normal(size=3))
    return n, t / np.linalg.norm(t)


def _dir_for(cos, n, t, length):
    """An incoming direction d with dot(-d, n) = cos (d points at the surface)."""
    if cos == 0.0:                                         # axis-aligned frame: exactly +-0 along n
        d = -t * length
        d[np.argmax(np.abs(n))] = -cos * length
        return d
    s = np.sqrt(max(0.0, 1.0 - cos * cos))
    return -(cos * n + s * t) * length


def _L_for(kind, n, t, d, rng):
    b = np.cross(n, t)
    wi = -d / np.linalg.norm(d)
    if kind == "above":
        v = rng.normal(size=3); v /= np.linalg.norm(v); return v if v @ n > 0 else -v
    if kind == "below":
        v = rng.normal(size=3); v /= np.linalg.norm(v); return v if v @ n < 0 else -v
    if kind == "+N":
        return n
    if kind == "-N":
        return -n
    if kind == "mirror":
        r = 2 * (wi @ n) * n - wi
        return r / max(np.linalg.norm(r), 1e-300)
    if kind == "-dir":
        return wi
    if kind == "zero":
        return np.zeros(3)
    return 1e-6 * n + b                                            # grazing


class CaseSet:
    """All cases: arrays of fp32 inputs (as float64), the group / type / label of each, and the material table and textures they use."""

    def __init__(self, seed=3):
        rng = np.random.RandomState(seed)
        self.mats, self.tags = materials()
        self.tex = Textures(TEX_SIZES)
        rows, self.group, self.label = [], [], []
        by_type = {t: [i for tt, _, i in self.tags if tt == t] for t in TYPES}
        base_of = {t: [i for tt, lb, i in self.tags if tt == t and lb == "base"][0] for t in TYPES}

        def add(group, label, mid, cos=0.5, face=0, frame=1, length=1.0, L="above", seed=None, uv=(0.25, 0.75)):
            n, t = _frame(frame, rng)                                   # (on a back face the logic step has turned N toward the ray)
            d = _dir_for(cos, n, t, length)
            rows.append(dict(P=rng.uniform(-2, 2, 3), N=n, uv=np.array(uv, np.float64), dir=d, L=_L_for(L, n, t, d, rng),
                             T=rng.uniform(0.2, 1.0, 3), seed=int(rng.randint(0, 2 ** 32, dtype=np.uint64)) if seed is None else seed,
                             backface=face, mat=mid))
            self.group.append(group)
            self.label.append(label)

        for t in TYPES:
            # every material of the type, a few geometries
            for mid in by_type[t]:
                lb = self.tags[mid][1]
                for cos, face, L in ((1.0, 0, "above"), (0.5, 0, "mirror"), (1e-2, 0, "above"), (0.5, 1, "+N"), (0.7, 1, "below")):
                    add("material", lb, mid, cos=cos, face=face, L=L)
            # the geometry axes on the base material and a rough / sharp lobe
            mids = [base_of[t]] + [i for tt, lb, i in self.tags if tt == t and lb in ("Ns=1", "Ns=100000")]
            for mid in mids:
                for cos in COS_SWEEP:
                    for face in (0, 1):
                        for length in (1.0, 3.7, 1e-3):
                            for L in L_KINDS:
                                add("geometry", f"cos={cos:g}", mid, cos=cos, face=face, frame=(0 if cos == 0.0 else 1), length=length, L=L)
            # draws: exactly 0, exactly 1.0, and one ulp either side of the Fresnel threshold
            for mid in mids:
                for k in range(1, DRAWS[t] + 1):
                    for v in (0.0, 1.0):
                        for cos, face in ((0.5, 0), (0.9, 1), (1e-2, 0)):
                            add("draws", f"draw{k}={v:g}", mid, cos=cos, face=face, seed=seed_for_draw(k, v))
            # uv: every texture-mapped material, both coordinates
            for mid in [i for tt, lb, i in self.tags if tt == t and lb.startswith("map")]:
                for u in UV_SWEEP:
                    for uv in ((u, 0.5), (0.5, u), (u, u)):
                        add("uv", f"u={u:g}", mid, uv=uv)
                for k in (0, 1):
                    w, h = TEX_SIZES[k]
                    for uv in ((3e9 / w, 0.5), (0.5, 3e9 / h), (-3e9 / w, -3e9 / h), (1e30, 0.5), (2.0 ** 31 / w + 0.5, 0.25)):
                        add("uv", "huge", mid, uv=uv)
            # plain random control
            for _ in range(160):
                mid = by_type[t][rng.randint(len(by_type[t]))]
                add("random", "random", mid, cos=float(rng.uniform(0.05, 1.0)), face=int(rng.randint(2)), L=L_KINDS[rng.randint(2)],
                    length=float(rng.choice([1.0, 2.5])))
        self.n = len(rows)
        f32 = lambda k: np.array([r[k] for r in rows], np.float64).astype(np.float32).astype(np.float64)
        self.case = Case(P=f32("P"), N=f32("N"), uv=f32("uv"), dir=f32("dir"), L=f32("L"), T=f32("T"),
                         seed=np.array([r["seed"] for r in rows], np.uint64), backface=np.array([r["backface"] for r in rows], bool),
                         mat=np.array([r["mat"] for r in rows], np.int64))
        self.group, self.label = np.array(self.group), np.array(self.label)
        self.type = self.mats["type"][self.case.mat].astype(np.int64)
        self._fresnel_seeds()

    def _fresnel_seeds(self):
        """Seeds whose Fresnel draw lands on fp32(Fr) and one ulp either side of it (Fr from the nominal restatement), appended as group
        'fresnel' for every case of the 'material' group of a type with a Fresnel choice."""
        rs = Restatement(self.mats, self.tex)
        sel = np.nonzero((self.group == "material") & np.isin(self.type, list(FRESNEL_DRAW)))[0]
        c = Case(**{k: getattr(self.case, k)[sel] for k in Case.FIELDS})
        E = Eval(sel.size)
        fr = np.zeros(sel.size)
        with np.errstate(all="ignore"):
            for t in FRESNEL_DRAW:
                idx = np.nonzero(self.type[sel] == t)[0]
                if not idx.size:
                    continue
                E.idx = idx
                s = Case(**{k: getattr(c, k)[idx] for k in Case.FIELDS})
                m = rs._mat_arrays(E, s.mat)
                if t == BXDF.GLOSSY:
                    Ks = rs._ks(E, s, m["Ks"], m["mapKs"])
                    k = np.clip(Ks.sum(1) / 3.0, 0.0, F32(0.99))
                    Ni = np.where(m["Ni"] > 0.0, m["Ni"], (np.sqrt(k) + 1.0) / (1.0 - np.sqrt(k)))
                    fr[idx] = _fresnel(E, _dot(E.normalize(-s.dir), s.N), np.ones_like(Ni), Ni)
                else:
                    etaI, etaO = np.where(s.backface, m["Ni"], 1.0), np.where(s.backface, 1.0, m["Ni"])
                    fr[idx] = _fresnel(E, _dot(E.normalize(-s.dir), s.N), etaI, etaO)
        new = []
        for i, f in zip(sel, fr):
            if not (0.0 < f < 1.0) or not np.isfinite(f):
                continue
            f32 = np.float32(f)
            for v, lb in ((np.nextafter(f32, np.float32(0)), "Fr-ulp"), (f32, "Fr"), (np.nextafter(f32, np.float32(1)), "Fr+ulp")):
                new.append((i, seed_for_draw(FRESNEL_DRAW[int(self.type[i])], float(v)), lb))
        if not new:
            return
        src = np.array([i for i, _, _ in new])
        for k in Case.FIELDS:
            a = getattr(self.case, k)
            extra = a[src].copy()
            if k == "seed":
                extra = np.array([s for _, s, _ in new], np.uint64)
            setattr(self.case, k, np.concatenate([a, extra]))
        self.group = np.concatenate([self.group, np.full(src.size, "fresnel")])
        self.label = np.concatenate([self.label, np.array([lb for _, _, lb in new])])
        self.type = np.concatenate([self.type, self.type[src]])
        self.n = self.case.N.shape[0]

    def subset(self, idx):
        """A CaseSet view holding only the cases idx (same materials and textures)."""
        s = object.__new__(CaseSet)
        s.mats, s.tags, s.tex = self.mats, self.tags, self.tex
        s.case = Case(**{k: getattr(self.case, k)[idx] for k in Case.FIELDS})
        s.group, s.label, s.type, s.n = self.group[idx], self.label[idx], self.type[idx], len(idx)
        return s

    def scene(self):
        """A SceneData with the cases' materials and textures (and a few triangles: the material step reads no geometry)."""
        import common
        from fluctus_amd import host
        d = common.small_mesh_scene(n=2)
        d.tris["matId"] = 0
        d.materials = self.mats
        d.texdesc, d.texdata = self.tex.desc, self.tex.data
        host.build_bvh(d, "sbvh")
        return d

    def restatement(self):
        return Restatement(self.mats, self.tex)


# ---------------------------------------------------------------------------------------------------------------------------------
# contexts
def state_of(cs, st):
    """Write the cases' inputs into a reference-layout state (64, >= n) in place."""
    n, c = cs.n, cs.case
    assert st.shape[1] >= n
    assert (c.mat >= 0).all() and (c.mat < cs.mats.size).all()
    u = st.view(np.uint32)
    st[COL.P:COL.P + 3, :n] = c.P.T
    st[COL.N:COL.N + 3, :n] = c.N.T
    st[COL.UV:COL.UV + 2, :n] = c.uv.T
    st[COL.DIR:COL.DIR + 3, :n] = c.dir.T
    st[COL.SHADOW_DIR:COL.SHADOW_DIR + 3, :n] = c.L.T
    st[COL.T:COL.T + 3, :n] = c.T.T
    u[COL.SEED, :n] = c.seed.astype(np.uint32)
    u[COL.BACKFACE, :n] = c.backface.astype(np.uint32)
    u[COL.MAT_ID, :n] = c.mat.astype(np.uint32)
    u[COL.HIT_I, :n] = 0
    u[COL.PATH_LEN, :n] = 1
    return st


def queues_of(cs, order=None, separate=True):
    """{queue: path ids}: every case in its material queue (separate) or all in the diffuse queue (single queue), in `order` (default: id)."""
    ids = np.arange(cs.n, dtype=np.uint32) if order is None else np.asarray(order, np.uint32)
    if not separate:
        return {Q.DIFFUSE: ids}
    return {q: ids[np.isin(cs.type[ids], [t for t, qq in QUEUE_OF.items() if qq == q])] for q in sorted(set(QUEUE_OF.values()))}


def load(ctx, cs, queues):
    """Import the cases into a context (whose other paths keep their state) with the given material queues and empty others."""
    st = state_of(cs, ctx.state_export())
    ctx.state_import(st)
    cnt = np.array(ctx.get_counters(), copy=True)
    if hasattr(ctx, "finish"):
        ctx.finish()
    cnt = np.array(cnt, copy=True)
    cnt[:] = 0
    for q, ids in queues.items():
        assert (np.asarray(ids) < st.shape[1]).all()
        ctx.queue_write(q, np.asarray(ids, np.uint32))
        cnt[q] = len(ids)
    ctx.set_counters(cnt)


def params(d, separate=True):
    p = wire.default_params(8, 8, d.world_radius, d.tris.size)
    p["wfSeparateQueues"] = int(separate)
    return p
