/*
 * flx_denoise.h -- the guided a-trous denoiser (flx_denoise), defined once, per pixel.
 *
 * Edge-avoiding a-trous wavelet filter (Dammertz, Sewtz, Hanika, Lensch: "Edge-Avoiding A-Trous Wavelet Transform for fast Global
 * Illumination Filtering", HPG 2010) on linear radiance, guided by the first-hit albedo and normal feature buffers and demodulated by
 * the albedo.  The kernels (csrc/denoise.hip) and the CPU counterpart (tests/denoise_cpu.cpp) both include this header; with
 * -ffp-contract=off, flx::expf_ and the fixed summation order below their results are BIT-IDENTICAL.  tests/denoise_reference.py
 * restates every formula in float64.
 *
 * Per local pixel i (flat index, W x H image, context unpartitioned):
 *   c_i  = sum.rgb / count                          raw accumulation (flx_read_pixels which = 0)
 *   n_i, a_i                                         the guides resolved from their accumulators (which = 5 / 4) by k_postprocess' rule
 *   a'_i = max(a_i, FLX_DN_EPS_ALBEDO) per channel
 *   e_i  = c_i / a'_i                                demodulated radiance
 *   valid iff count > 0 and e_i, a'_i, n_i are finite; an invalid pixel is never a neighbour and is passed through unchanged
 *   pass k = 0..K-1, step s = 2^k:   e_i <- sum_j w_ij e_j / sum_j w_ij over the 5 x 5 taps j = i + s * (dx, dy), inside the image, valid,
 *                                     w_ij = h[dx] h[dy] exp(-(|e_i-e_j|^2 ic_k + |n_i-n_j|^2 i_n + |a'_i-a'_j|^2 i_a)),
 *                                     h = {1, 4, 6, 4, 1} / 16, ic_k = 1 / (sigma_c 2^-k)^2, i_n = 1 / sigma_n^2, i_a = 1 / sigma_a^2
 *   d_i  = e_i a'_i;   out_i = blend c_i + (1 - blend) d_i   (OptiX' blendFactor: 0 = fully denoised)
 */
#ifndef FLX_DENOISE_H
#define FLX_DENOISE_H

#include "../../include/flx_math.h"

namespace flx {

#define FLX_DN_EPS_ALBEDO 1e-3f
#define FLX_DN_MAX_ITERATIONS 8
/* defaults (chosen with the quality test of tests/test_denoise.py) */
#define FLX_DN_DEFAULT_ITERATIONS 5
#define FLX_DN_DEFAULT_SIGMA_COLOR 2.0f
#define FLX_DN_DEFAULT_SIGMA_NORMAL 0.3f
#define FLX_DN_DEFAULT_SIGMA_ALBEDO 0.1f
/* an exponent argument below -FLX_DN_EXP_CUT contributes weight 0 (expf_ is defined for |x| < 87) */
#define FLX_DN_EXP_CUT 87.0f

/* one pixel of the filter's working set: demodulated radiance, normal guide, floored albedo guide */
struct dn_pix { f3 e; f3 n; f3 a; bool valid; };

FLX_HD bool dn_finite(float v) { return absf(v) <= FLX_FLT_MAX; }
FLX_HD bool dn_finite3(f3 v) { return dn_finite(v.x) && dn_finite(v.y) && dn_finite(v.z); }

/* the guided filter's part of a pixel, for code shared by both filters (flx_denoise_vg.h: dn_part of a vg_pix) */
FLX_HD const dn_pix &dn_part(const dn_pix &p) { return p; }
FLX_HD dn_pix &dn_part(dn_pix &p) { return p; }

/* B3-spline tap of offset t in -2..2 */
FLX_HD float dn_h(int t) { return t == 0 ? 0.375f : (t == 1 || t == -1) ? 0.25f : 0.0625f; }

/* the blend as DenoiserOptix::setBlend takes it: clamped to [0, 1] */
FLX_HD float dn_blend(float b) { return clampf(b, 0.0f, 1.0f); }
/* blend == 1 or no pass: the output is the input colour, exactly */
FLX_HD bool dn_identity(float blend, int iterations) { return blend == 1.0f || iterations == 0; }

/* 1 / sigma^2, saturated at FLT_MAX so that a zero difference always weighs exp(0) = 1 (0 * inf would be NaN) */
FLX_HD float dn_inv_sq(float sigma) { return fminf_(1.0f / (sigma * sigma), FLX_FLT_MAX); }
/* ic_k: the colour sigma halves every pass (Dammertz) -- an exact power-of-two scale */
FLX_HD float dn_inv_sq_color(float sigma_c, int k) { return dn_inv_sq(sigma_c * u2f((uint32_t)(127 - k) << 23)); }

/* a guide accumulator resolved as k_postprocess resolves it (src/mk_postprocess.cl:49-54): w > 1 ? sum / w : as is */
FLX_HD f3 dn_resolve(const float g[4]) { return g[3] > 1.0f ? mk3(g[0] / g[3], g[1] / g[3], g[2] / g[3]) : mk3(g[0], g[1], g[2]); }

/* the prepare step: raw accumulation px, albedo and normal accumulators -> colour c (valid pixels only) and the working set */
FLX_HD dn_pix dn_prepare(const float px[4], const float alb[4], const float nrm[4], f3 *c)
{
    dn_pix o;
    o.n = dn_resolve(nrm);
    o.a = max3(dn_resolve(alb), mk3(FLX_DN_EPS_ALBEDO));
    const float count = px[3];
    *c = count > 0.0f ? mk3(px[0], px[1], px[2]) / count : mk3(0.0f);
    o.e = *c / o.a;
    o.valid = count > 0.0f && dn_finite3(o.e) && dn_finite3(o.a) && dn_finite3(o.n);
    return o;
}

/* one a-trous tap weight: h[dx] h[dy] exp(-q), ONE expf_ */
FLX_HD float dn_weight(const dn_pix &pi, const dn_pix &pj, int dx, int dy, float ic, float in_, float ia)
{
    const f3 de = pi.e - pj.e, dn = pi.n - pj.n, da = pi.a - pj.a;
    const float q = dot(de, de) * ic + dot(dn, dn) * in_ + dot(da, da) * ia;
    const float hw = dn_h(dx) * dn_h(dy);
    return q < FLX_DN_EXP_CUT ? hw * expf_(-q) : 0.0f;
}

/* the taps of the (2R+1) x (2R+1) stencil at step s around (x, y) that lie inside the W x H image, row-major (dy outer, dx inner), the centre
 * included: tap(xj, yj, dx, dy) for each.  Every filter loop of this header and of flx_denoise_vg.h is this walk; its order is the summation order. */
template <int R, class Tap>
FLX_HD void dn_taps(int x, int y, int W, int H, int s, Tap tap)
{
    for (int dy = -R; dy <= R; dy++) {
        const int yj = y + dy * s;
        if (yj < 0 || yj >= H) continue;
        for (int dx = -R; dx <= R; dx++) {
            const int xj = x + dx * s;
            if (xj < 0 || xj >= W) continue;
            tap(xj, yj, dx, dy);
        }
    }
}

/* one pass at pixel (x, y) of a valid centre pi, step s: the 5 x 5 taps of dn_taps; taps on an invalid pixel are skipped and the weights
 * renormalise.  fetch(xj, yj) -> dn_pix of pixel (xj, yj) in this pass' input.  The centre tap weighs h[0]^2 > 0, so the sum of weights is
 * never zero. */
template <class Fetch>
FLX_HD f3 dn_atrous(int x, int y, int W, int H, int s, const dn_pix &pi, float ic, float in_, float ia, Fetch fetch)
{
    f3 acc = mk3(0.0f);
    float ws = 0.0f;
    dn_taps<2>(x, y, W, H, s, [&](int xj, int yj, int dx, int dy) {
        const dn_pix pj = fetch(xj, yj);
        if (!pj.valid) return;
        const float w = dn_weight(pi, pj, dx, dy, ic, in_, ia);
        acc = acc + pj.e * w;
        ws = ws + w;
    });
    return acc / ws;
}

/* dn_atrous as both filters call it (flx_denoise_vg.h: the overloads for a vg_pix): a prefiltered variance gv and an out-argument for what
 * the pass propagates, neither of which the guided filter has */
template <class Fetch>
FLX_HD float dn_prefilter(int, int, int, int, const dn_pix &, Fetch) { return 0.0f; }
template <class Fetch>
FLX_HD f3 dn_atrous(int x, int y, int W, int H, int s, const dn_pix &pi, float, float ic, float in_, float ia, Fetch fetch, float *)
{
    return dn_atrous(x, y, W, H, s, pi, ic, in_, ia, fetch);
}

/* the finish step: which = 6 of pixel i.  Invalid: the raw accumulation unchanged.  Valid: (out_i, 1) with out_i the blend of c_i and
 * the remodulated filter output ef; identity (blend == 1 or K == 0) returns c_i itself, not a round trip through the demodulation. */
FLX_HD void dn_finish(const float px[4], const dn_pix &pi, f3 c, f3 ef, float blend, bool identity, float out[4])
{
    if (!pi.valid) { out[0] = px[0]; out[1] = px[1]; out[2] = px[2]; out[3] = px[3]; return; }
    f3 o = c;
    if (!identity) {
        const f3 d = ef * pi.a;
        o = c * blend + d * (1.0f - blend);
    }
    out[0] = o.x; out[1] = o.y; out[2] = o.z; out[3] = 1.0f;
}

/* ---- luminance of a sample (option "moments": the integrators' splats accumulate (sum l, sum l^2, 0, n) per pixel, flx_read_pixels which = 7;
 * the variance-guided filter of flx_denoise_vg.h).  Rec. 709 weights in this fixed order; every file that includes this header is built with
 * -ffp-contract=off, so no product is fused into an FMA and the host, the device and numpy float32 give the same bits. */
FLX_HD float flx_lum(f3 v) { return (0.2126f * v.x + 0.7152f * v.y) + 0.0722f * v.z; }

/* ---- the post-process (reference: src/mk_postprocess.cl:7-55, src/tonemap.cl:3-26): k_postprocess and the denoiser's preview */
FLX_HD f3 uc2_tonemap(f3 x)
{
    const float A = 0.22f, B = 0.30f, C = 0.10f, D = 0.20f, E = 0.01f, Fq = 0.30f;
    return ((x * (A * x + mk3(C * B)) + mk3(D * E)) / (x * (A * x + mk3(B)) + mk3(D * Fq))) - mk3(E / Fq);
}
FLX_HD void postprocess_px(const float in[4], float exposure, uint32_t tmOperator, float out[4])
{
    f3 col = mk3(in[0], in[1], in[2]); float w = in[3];
    if (w > 0.0f) { col = col / w; w = w / w; }
    col = col * exposure;
    if (tmOperator == 1u) col = col / (mk3(1.0f) + col);
    if (tmOperator == 2u) col = uc2_tonemap(2.0f * col) / uc2_tonemap(mk3(11.2f));
    col = pow3(col, 1.0f / 2.2f);
    out[0] = col.x; out[1] = col.y; out[2] = col.z; out[3] = w;
}

} /* namespace flx */

#endif /* FLX_DENOISE_H */
