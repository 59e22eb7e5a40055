/*
 * flx_denoise_vg.h -- the variance-guided a-trous denoiser (flx_denoise_variance_guided), defined once, per pixel.
 *
 * The spatial filter of SVGF (Schied et al.: "Spatiotemporal Variance-Guided Filtering", HPG 2017) on top of the guided filter of
 * flx_denoise.h: the fixed colour stop is replaced by a luminance stop scaled by a per-pixel estimate of the standard deviation of the
 * pixel mean, which the integrators supply as luminance moments (option "moments", flx_read_pixels which = 7), and the variance is
 * carried through the passes.  The kernels (csrc/denoise.hip) and the CPU counterpart (tests/denoise_cpu.cpp) include this header;
 * their results are BIT-IDENTICAL.  tests/denoise_vg_reference.py restates every formula in float64.
 *
 * Per local pixel i (flat index, W x H image, context unpartitioned), with l(v) = flx_lum(v) (Rec. 709, flx_denoise.h):
 *   c_i, e_i, n_i, a'_i, valid_i      as dn_prepare (flx_denoise.h); invalid pixels pass through and are never a neighbour
 *   guided_i                          valid_i and the albedo accumulator's count (which = 4, w) > 0: some sample of the pixel hit a surface.
 *                                     A valid pixel that is not guided (every sample saw the area light or the environment directly: its
 *                                     guides are the resets' placeholders) is returned as c_i, exactly, and is never a neighbour -- there is
 *                                     nothing to stop an edge with, and its error is coverage noise that averaging only spreads (DESIGN.md
 *                                     4.3.2).  Below, "valid" means guided.
 *   (S1, S2, _, m)_i                  the moments (which = 7): sums of l and l^2 over the m samples the integrator splatted.  m is the
 *                                     moments' own count; it may differ from the colour's (flx_write_pixels), only m enters the variance
 *   initial variance, valid i:
 *     per pixel, when m >= 2 and m, S1/m, S2/m and (S1/m)^2 are finite:
 *       var_i = max(0, S2/m - (S1/m)^2) / m / l(a'_i)^2          the variance of the pixel MEAN of l, demodulated to the units of l(e)
 *     otherwise (m < 2, a non-finite or overflowing sum): the spatial fallback -- the spread of l(e_j) over the valid 3 x 3 neighbours j
 *     (the centre included) weighted by the guides alone:
 *       u_j = exp(-(|n_i-n_j|^2 i_n + |a'_i-a'_j|^2 i_a)),  var_i = max(0, sum u l(e)^2 / sum u - (sum u l(e) / sum u)^2)
 *     (a spread of pixel means is already a variance of the mean: no / m).  Invalid i: var_i = 0.
 *     Every variance is capped: NaN -> FLX_VG_VAR_MAX, otherwise clamped to [0, FLX_VG_VAR_MAX].
 *   pass k = 0..K-1, step s = 2^k, valid i:
 *     g_i  = min(var_i, sum_j g(dx) g(dy) var_j / sum_j g(dx) g(dy)) over the valid 3 x 3 taps at distance 1, g = {1, 2, 1} / 4
 *            (the prefilter, clamped by the centre's own variance: a low-variance pixel next to an outlier does not take the outlier in)
 *     w_ij = h[dx] h[dy] exp(-(|l(e_i) - l(e_j)| / (sigma_l sqrt(g_i) + FLX_VG_EPS) + |n_i-n_j|^2 i_n + |a'_i-a'_j|^2 i_a))
 *            over the 5 x 5 taps j = i + s (dx, dy) inside the image and valid, h = {1, 4, 6, 4, 1} / 16, as dn_atrous
 *     e_i <- sum_j w_ij e_j / sum_j w_ij,     var_i <- cap(sum_j w_ij^2 var_j / (sum_j w_ij)^2)
 *   finish: dn_finish (remodulate by a'_i, blend as OptiX' blendFactor); K = 0 or blend = 1 returns c_i exactly, as does a valid pixel that
 *   is not guided.
 */
#ifndef FLX_DENOISE_VG_H
#define FLX_DENOISE_VG_H

#include "flx_denoise.h"

namespace flx {

/* defaults (sigma_l from the sweep of tests/test_denoise_variance.py; sigma_n, sigma_a as flx_denoise) */
#define FLX_VG_DEFAULT_ITERATIONS 5
#define FLX_VG_DEFAULT_SIGMA_LUMINANCE 4.0f
#define FLX_VG_DEFAULT_SIGMA_NORMAL FLX_DN_DEFAULT_SIGMA_NORMAL
#define FLX_VG_DEFAULT_SIGMA_ALBEDO FLX_DN_DEFAULT_SIGMA_ALBEDO
/* the luminance stop's epsilon (a pixel with zero variance keeps only neighbours of its own luminance) and the variance cap (keeps every
 * sum of the propagation finite: 25 taps x w^2 <= 1 x cap / (sum w)^2 >= h[0]^4) */
#define FLX_VG_EPS 1e-10f
#define FLX_VG_VAR_MAX 1e30f

/* the prepare step: dn_prepare, then valid only where guided (the albedo accumulator counted a surface hit) */
FLX_HD dn_pix vg_prepare(const float px[4], const float alb[4], const float nrm[4], f3 *c)
{
    dn_pix o = dn_prepare(px, alb, nrm, c);
    o.valid = o.valid && alb[3] > 0.0f;
    return o;
}

/* one pixel of the working set: the guided filter's pixel and its variance */
struct vg_pix { dn_pix d; float v; };

/* the guided filter's part of a pixel, for code shared by both filters (flx_denoise.h: dn_part of a dn_pix) */
FLX_HD const dn_pix &dn_part(const vg_pix &p) { return p.d; }
FLX_HD dn_pix &dn_part(vg_pix &p) { return p.d; }

FLX_HD float vg_cap(float v) { return v == v ? clampf(v, 0.0f, FLX_VG_VAR_MAX) : FLX_VG_VAR_MAX; }

/* the per-pixel estimate from the moments; false when it does not exist (m < 2, or a non-finite term) */
FLX_HD bool vg_pixel_variance(const float mom[4], f3 a, float *var)
{
    const float m = mom[3];
    if (!(m >= 2.0f) || !dn_finite(m)) return false;
    const float m1 = mom[0] / m, m2 = mom[1] / m, sq = m1 * m1;
    if (!dn_finite(m1) || !dn_finite(m2) || !dn_finite(sq)) return false;
    const float la = flx_lum(a);
    *var = vg_cap(fmaxf_(m2 - sq, 0.0f) / m / (la * la));
    return true;
}

/* the guides-only weight of the spatial fallback: exp(-(|dn|^2 i_n + |da|^2 i_a)), ONE expf_ */
FLX_HD float vg_guide_weight(const dn_pix &pi, const dn_pix &pj, float in_, float ia)
{
    const f3 dn = pi.n - pj.n, da = pi.a - pj.a;
    const float q = dot(dn, dn) * in_ + dot(da, da) * ia;
    return q < FLX_DN_EXP_CUT ? expf_(-q) : 0.0f;
}

/* the initial variance of a valid centre pi at (x, y): the per-pixel estimate, else the spatial fallback over the valid 3 x 3 neighbours
 * (the 3 x 3 taps of dn_taps, the centre included: its weight is 1, so the sum never vanishes).  fetch(xj, yj) -> dn_pix as prepared. */
template <class Fetch>
FLX_HD float vg_initial_variance(int x, int y, int W, int H, const dn_pix &pi, const float mom[4], float in_, float ia, Fetch fetch)
{
    float v;
    if (vg_pixel_variance(mom, pi.a, &v)) return v;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    dn_taps<1>(x, y, W, H, 1, [&](int xj, int yj, int, int) {
        const dn_pix pj = fetch(xj, yj);
        if (!pj.valid) return;
        const float u = vg_guide_weight(pi, pj, in_, ia), l = flx_lum(pj.e);
        s0 = s0 + u;
        s1 = s1 + u * l;
        s2 = s2 + u * (l * l);
    });
    const float mean = s1 / s0;
    return vg_cap(fmaxf_(s2 / s0 - mean * mean, 0.0f));
}

/* 3 x 3 tap of offset t in -1..1 */
FLX_HD float vg_g(int t) { return t == 0 ? 0.5f : 0.25f; }

/* the 3 x 3 prefilter of the variance at a valid centre (x, y), distance 1, valid taps only, renormalised.  fetch(xj, yj) -> vg_pix. */
template <class Fetch>
FLX_HD float vg_prefilter(int x, int y, int W, int H, Fetch fetch)
{
    float acc = 0.0f, ws = 0.0f;
    dn_taps<1>(x, y, W, H, 1, [&](int xj, int yj, int dx, int dy) {
        const vg_pix pj = fetch(xj, yj);
        if (!pj.d.valid) return;
        const float g = vg_g(dx) * vg_g(dy);
        acc = acc + g * pj.v;
        ws = ws + g;
    });
    return acc / ws;
}

/* one a-trous tap weight: h[dx] h[dy] exp(-(|l_i - l_j| / den + |dn|^2 i_n + |da|^2 i_a)), ONE expf_ */
FLX_HD float vg_weight(const dn_pix &pi, float li, const dn_pix &pj, int dx, int dy, float den, float in_, float ia)
{
    const f3 dn = pi.n - pj.n, da = pi.a - pj.a;
    const float q = absf(li - flx_lum(pj.e)) / den + dot(dn, dn) * in_ + dot(da, da) * ia;
    const float hw = dn_h(dx) * dn_h(dy);
    return q < FLX_DN_EXP_CUT ? hw * expf_(-q) : 0.0f;
}

/* one pass at a valid centre pi at (x, y), step s, prefiltered variance gv (clamped here by the centre's): the 5 x 5 taps, skipping and
 * renormalisation of the guided dn_atrous, whose overload for a vg_pix this is.  fetch(xj, yj) -> vg_pix.
 * -> the filtered e; *vout the propagated variance.  The centre weighs h[0]^2 > 0, so the sums never vanish. */
template <class Fetch>
FLX_HD f3 dn_atrous(int x, int y, int W, int H, int s, const vg_pix &pi, float gv, float sigma_l, float in_, float ia, Fetch fetch, float *vout)
{
    const float li = flx_lum(pi.d.e), den = sigma_l * sqrtf(fminf_(gv, pi.v)) + FLX_VG_EPS;
    f3 acc = mk3(0.0f);
    float ws = 0.0f, vs = 0.0f;
    dn_taps<2>(x, y, W, H, s, [&](int xj, int yj, int dx, int dy) {
        const vg_pix pj = fetch(xj, yj);
        if (!pj.d.valid) return;
        const float w = vg_weight(pi.d, li, pj.d, dx, dy, den, in_, ia);
        acc = acc + pj.d.e * w;
        ws = ws + w;
        vs = vs + (w * w) * pj.v;
    });
    *vout = vg_cap(vs / (ws * ws));
    return acc / ws;
}

/* the variance-guided pass under its own name */
template <class Fetch>
FLX_HD f3 vg_atrous(int x, int y, int W, int H, int s, const vg_pix &pi, float gv, float sigma_l, float in_, float ia, Fetch fetch, float *vout)
{
    return dn_atrous(x, y, W, H, s, pi, gv, sigma_l, in_, ia, fetch, vout);
}

/* the prefilter as the overload of dn_prefilter (flx_denoise.h) for a vg_pix centre */
template <class Fetch>
FLX_HD float dn_prefilter(int x, int y, int W, int H, const vg_pix &, Fetch fetch) { return vg_prefilter(x, y, W, H, fetch); }

} /* namespace flx */

#endif /* FLX_DENOISE_VG_H */
