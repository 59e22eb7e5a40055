/*
 * flx_rectify.h -- history rectification (flx_history_mark / flx_history_rectify), defined once, per pixel.
 *
 * Temporal reprojection (flx_reproject.h) knows where a surface point WAS; it cannot notice that its radiance CHANGED: a moved object's shadow on a
 * surface that did not move, a dimmed lamp.  This is the missing half, a temporal-gradient test in the spirit of A-SVGF's adaptive history
 * (Schied, Peters, Dachsbacher, HPG 2018) without re-tracing old seeds: remember the accumulation at a MARK, let the integrators add samples on
 * top, compare the two over an edge-stopped window, and take out, per pixel, the share of the marked history that the new samples contradict.
 * The kernels (csrc/rectify.hip) and the CPU counterpart (tests/rectify_cpu.cpp) both include this header; with -ffp-contract=off, the contract
 * functions of flx_math.h and the fixed tap order below their results are BIT-IDENTICAL.  tests/rectify_reference.py restates every formula in
 * float64.
 *
 * Per pixel q, from A (the accumulation now, which = 0: rgb sum, count), S (the marked copy of it) and the current G-buffer record G0
 * (the prepare step, rc_prepare -> the record (n, a, h, ok)):
 *   n_q = A.w - S.w          a_q = lum(A.rgb - S.rgb) / n_q   (the new samples' mean luminance)       h_q = lum(S.rgb) / S.w  (the history's)
 *   ok_q  iff  G0 is a hit, S.w > 0, n_q >= 0.5 and S.w, n_q, a_q, h_q and a_q - h_q are all finite        (lum = flx_lum, flx_denoise.h)
 *
 * Per centre pixel p (rc_lambda).  p must hold a surface, S_p.w > 0, and A_p and S_p finite; otherwise lambda = 0.  Taps q over the
 * (2 r + 1)^2 window in row-major order (dy outer, dx inner); a tap counts iff it lies inside the image, ok_q holds,
 *       |dot(P_q - P_p, N_p)| <= plane_tolerance_px * t_p * footprint,   footprint = 2 tan(fov / 2) / H of the current slot's camera,
 *       dot(N_q, N_p) >= normal_cos            (rp_same_plane / rp_same_facing: the two tests of rp_pixel, flx_reproject.h)
 * With x_q = a_q - h_q, sums in fp32 in that order:  N = number of counted taps,  K = sum n_q,  sum n x,  sum (n x) x,  sum n a,  sum n h.  Then
 *       d = (sum n x) / K      v = max(0, (sum n x^2) / K - d d)      se = sqrt(v / N)      e = max(0, |d| - gamma se)
 *       lambda = min(1, sensitivity e / (max(sum n a / K, sum n h / K) + lum_floor))
 * N < min_pixels: lambda = 0.  Every comparison is written so that a NaN gives lambda = 0: doubt keeps the history.
 * The difference is taken PER PIXEL (x_q) before it is pooled, so static texture inside the window cancels and se measures noise, not albedo.
 *
 * Output (rc_apply).  lambda = 0: the pixel is not written.  Otherwise A' = A - lambda S on all four components and S' = S (1 - lambda)
 * replaces the mark; M' = M - lambda SM and SM' = SM (1 - lambda) for the moments when they are on now and were on at the mark.  A' - S' stays
 * the new samples, so the call may be repeated as evidence grows; lambda = 1 leaves exactly the new samples.
 *
 * The defaults are choices, not measurements.  Luminance only: a pure change of hue is not seen.  Pixels that miss the scene
 * keep their history.  Curved surfaces count fewer taps and so keep more history.
 */
#ifndef FLX_RECTIFY_H
#define FLX_RECTIFY_H

#include "flx_reproject.h"
#include "flx_denoise.h"

namespace flx {

#define FLX_RC_DEFAULT_RADIUS 3
#define FLX_RC_DEFAULT_GAMMA 3.0f
#define FLX_RC_DEFAULT_SENSITIVITY 2.0f
#define FLX_RC_DEFAULT_LUM_FLOOR 0.01f
#define FLX_RC_DEFAULT_MIN_PIXELS 8
#define FLX_RC_MAX_RADIUS 4

struct rc_params { int radius; float gamma, sensitivity, lum_floor; int min_pixels; float plane_tolerance_px, normal_cos; };

FLX_HD rc_params rc_defaults()
{
    rc_params p;
    p.radius = FLX_RC_DEFAULT_RADIUS; p.gamma = FLX_RC_DEFAULT_GAMMA; p.sensitivity = FLX_RC_DEFAULT_SENSITIVITY; p.lum_floor = FLX_RC_DEFAULT_LUM_FLOOR;
    p.min_pixels = FLX_RC_DEFAULT_MIN_PIXELS; p.plane_tolerance_px = FLX_RP_DEFAULT_PLANE_TOLERANCE_PX; p.normal_cos = FLX_RP_DEFAULT_NORMAL_COS;
    return p;
}
FLX_HD bool rc_params_ok(const rc_params &p)
{
    if (p.radius < 1 || p.radius > FLX_RC_MAX_RADIUS) return false;
    const int side = 2 * p.radius + 1;
    return rp_finite(p.gamma) && p.gamma >= 0.0f && rp_finite(p.sensitivity) && p.sensitivity > 0.0f && rp_finite(p.lum_floor) && p.lum_floor >= 0.0f &&
           p.min_pixels >= 1 && p.min_pixels <= side * side && rp_finite(p.plane_tolerance_px) && p.plane_tolerance_px > 0.0f &&
           p.normal_cos >= -1.0f && p.normal_cos <= 1.0f;
}
FLX_HD float rc_footprint(float fovDegrees, int H) { return 2.0f * rp_tan_half_fov(fovDegrees) / (float)H; }
FLX_HD bool rc_finite4(rp4 v) { return rp_finite(v.x) && rp_finite(v.y) && rp_finite(v.z) && rp_finite(v.w); }

/* the prepare step: the record (n, a, h, ok) of one pixel; ok is 1 or 0, and a record that is not ok is all zeros */
FLX_HD rp4 rc_prepare(rp4 A, rp4 S, rp4 g0)
{
    const rp4 none = mk_rp4(0.0f, 0.0f, 0.0f, 0.0f);
    if (!rp_is_hit(g0) || !(S.w > 0.0f) || !rp_finite(S.w)) return none;
    const float n = A.w - S.w;
    if (!(n >= 0.5f) || !rp_finite(n)) return none;
    const float a = flx_lum(mk3(A.x - S.x, A.y - S.y, A.z - S.z)) / n;
    const float h = flx_lum(mk3(S.x, S.y, S.z)) / S.w;
    if (!rp_finite(a) || !rp_finite(h) || !rp_finite(a - h)) return none;
    return mk_rp4(n, a, h, 1.0f);
}

/* lambda of the centre pixel (x, y).  g0 / g1: its record of the current G-buffer; A / S: its accumulation and mark.  rec(xq, yq) -> the
 * prepare record, gp(xq, yq) -> (P.xyz, anything), gn(xq, yq) -> (N.xyz, anything) of a tap INSIDE the image.  *counted: N (0 where the
 * centre itself is refused). */
template <class Rec, class GP, class GN>
FLX_HD float rc_lambda(const rc_params &rc, float footprint, int W, int H, int x, int y, rp4 g0, rp4 g1, rp4 A, rp4 S, Rec rec, GP gp, GN gn,
                       uint32_t *counted)
{
    *counted = 0u;
    if (!rp_is_hit(g0) || !(S.w > 0.0f) || !rc_finite4(S) || !rc_finite4(A)) return 0.0f;
    const f3 P = mk3(g0.x, g0.y, g0.z), N = mk3(g1.x, g1.y, g1.z);
    const float tol = rc.plane_tolerance_px * g1.w * footprint;
    uint32_t cnt = 0u;
    float K = 0.0f, snx = 0.0f, snx2 = 0.0f, sna = 0.0f, snh = 0.0f;
    for (int dy = -rc.radius; dy <= rc.radius; dy++) {
        const int yq = y + dy;
        if (yq < 0 || yq >= H) continue;
        for (int dx = -rc.radius; dx <= rc.radius; dx++) {
            const int xq = x + dx;
            if (xq < 0 || xq >= W) continue;
            const rp4 r = rec(xq, yq);
            if (!(r.w > 0.0f)) continue;
            const rp4 pq = gp(xq, yq);
            if (!rp_same_plane(mk3(pq.x, pq.y, pq.z), P, N, tol)) continue;
            const rp4 nq = gn(xq, yq);
            if (!rp_same_facing(mk3(nq.x, nq.y, nq.z), N, rc.normal_cos)) continue;
            const float xd = r.y - r.z, nx = r.x * xd;
            cnt++;
            K = K + r.x;
            snx = snx + nx;
            snx2 = snx2 + nx * xd;
            sna = sna + r.x * r.y;
            snh = snh + r.x * r.z;
        }
    }
    *counted = cnt;
    if ((int)cnt < rc.min_pixels || !(K > 0.0f) || !rp_finite(K)) return 0.0f;
    const float d = snx / K;
    const float v = fmaxf_(0.0f, snx2 / K - d * d);
    if (!rp_finite(d) || !rp_finite(v)) return 0.0f;
    const float se = sqrtf(v / (float)cnt);
    const float e = fmaxf_(0.0f, absf(d) - rc.gamma * se);
    const float den = fmaxf_(sna / K, snh / K) + rc.lum_floor;
    if (!(e > 0.0f) || !(den > 0.0f) || !rp_finite(den)) return 0.0f;
    const float lam = rc.sensitivity * e / den;
    if (!(lam > 0.0f)) return 0.0f;
    return fminf_(1.0f, lam);
}

/* false (lambda = 0, or a NaN): the pixel is NOT written -- it stays bit for bit, an inf or NaN in it included.  true: what is written,
 * now' = now - lambda mark on all four components, mark' = mark (1 - lambda): for (A, S) and for (M, SM) */
FLX_HD bool rc_apply(float lam, rp4 now, rp4 mark, rp4 *outNow, rp4 *outMark)
{
    if (!(lam > 0.0f)) return false;
    const float k = 1.0f - lam;
    *outNow = mk_rp4(now.x - lam * mark.x, now.y - lam * mark.y, now.z - lam * mark.z, now.w - lam * mark.w);
    *outMark = mk_rp4(mark.x * k, mark.y * k, mark.z * k, mark.w * k);
    return true;
}

} /* namespace flx */

#endif /* FLX_RECTIFY_H */
