/*
 * flx_reproject.h -- temporal reprojection of the accumulated image (flx_reproject), defined once, per pixel.
 *
 * The temporal half of SVGF (Schied et al., HPG 2017) for a static scene under a moving camera: the accumulation (which = 0) and the luminance
 * moments (which = 7) captured under the previous camera are resampled into the new view through the primary-visibility G-buffers of both
 * views (flx_gbuffer).  The kernel (csrc/reproject.hip) and the CPU counterpart (tests/reproject_cpu.cpp) both include this header; with
 * -ffp-contract=off, the contract functions of flx_math.h and the fixed tap order below their results are BIT-IDENTICAL.
 * tests/reproject_reference.py restates every formula in float64.
 *
 * G-buffer, two float4 per pixel:  G0 = (P.xyz, bits(hit index)), index < 0: no surface;  G1 = (Ng.xyz, t), Ng the unit geometric normal facing
 * the camera, t the distance along the (unit) centre ray.
 *
 * ASSUMED OF THE CAMERA FRAME: right, up and dir are unit vectors and mutually orthogonal (Tracer builds them so), and the primary ray of
 * pixel (x, y) leaves pos towards  dir + right * sx + up * sy  with  sx = (2 (x + 0.5) / W - 1) * (W / H) * tan(fov / 2),
 * sy = (2 (y + 0.5) / H - 1) * tan(fov / 2)  (flx_shading.h: camera_direction with the jitter 0.5, 0.5 and the lens at pos).  Then a point P
 * with v = P - pos, z = dot(v, dir) > 0 projects to sx = dot(v, right) / z, sy = dot(v, up) / z, and the continuous pixel coordinates whose
 * integer values are pixel centres are
 *     xf = ((sx / tan(fov / 2) / (W / H)) + 1) / 2 * W - 0.5,      yf = ((sy / tan(fov / 2)) + 1) / 2 * H - 0.5.
 * With a frame that is not orthonormal the projection is only approximate; the plane and normal tests below still reject wrong surfaces.
 *
 * Per new pixel (x, y), current G-buffer (P, i, N, t), previous camera, previous G-buffer, history (rgb sum, n), history moments:
 *   i < 0                                        -> pixel (0, 0, 0, 0), moments 0
 *   z <= 0, z or (xf, yf) not finite, or no tap inside the image -> no history: zeros
 *   taps j = (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1), x0 = floor(xf), y0 = floor(yf), bilinear weights b_j, in this order;
 *   tap j counts iff it lies inside the image, its previous hit index is >= 0, its history count n_j > 0 with rgb_j and n_j finite,
 *       |dot(P_j - P, N)| <= plane_tolerance_px * t * footprint,  footprint = 2 tan(fov_cur / 2) / H  (a PLANE test: grazing surfaces pass),
 *       dot(Ng_j, N) >= normal_cos          (every comparison written so that a NaN rejects the tap)
 *   S = sum b_j over the counted taps;  S < min_weight -> no history: zeros
 *   c = sum (b_j / S) (rgb_j / n_j),   nbar = sum (b_j / S) n_j,   n' = min(nbar, max_history),   pixel = (c n', n')
 *   moments (sum l, sum l^2, 0, n_m): over the counted taps whose n_m_j > 0 and whose sums are finite, weights b_j renormalised by THEIR sum
 *       S_m:  m1 = sum (b_j / S_m) (suml_j / n_m_j), m2 likewise,  output (m1 n', m2 n', 0, n').
 *       RULE for a counted tap with n_m_j <= 0 (or non-finite sums): it is left out of the moments' mix; when no tap remains (S_m == 0) the
 *       moments are (0, 0, 0, 0) -- count 0 sends the pixel to the variance-guided filter's spatial estimate.  A convex mix of points with
 *       m2 >= m1^2 keeps that property, so the variance stays >= 0.
 */
#ifndef FLX_REPROJECT_H
#define FLX_REPROJECT_H

#include "../../include/flx_math.h"

namespace flx {

#define FLX_RP_DEFAULT_MAX_HISTORY 32.0f
#define FLX_RP_DEFAULT_PLANE_TOLERANCE_PX 2.0f
#define FLX_RP_DEFAULT_NORMAL_COS 0.9f
#define FLX_RP_DEFAULT_MIN_WEIGHT 0.01f

struct rp4 { float x, y, z, w; };
FLX_HD rp4 mk_rp4(float x, float y, float z, float w) { rp4 r; r.x = x; r.y = y; r.z = z; r.w = w; return r; }

struct rp_params { float max_history, plane_tolerance_px, normal_cos, min_weight; };

/* what a call needs of the two cameras: the previous frame and its scale, the current view's pixel footprint at distance 1 */
struct rp_view {
    f3 pos, dir, up, right;     /* previous camera */
    float scale, aspect;        /* tan(fov_prev / 2), W / H */
    float footprint;            /* 2 tan(fov_cur / 2) / H */
    int W, H;
};

FLX_HD bool rp_finite(float v) { return absf(v) <= FLX_FLT_MAX; }
FLX_HD float rp_tan_half_fov(float fovDegrees) { return tanf_(0.5f * fovDegrees * FLX_PI / 180.0f); }     /* camera_direction's `scale` */
FLX_HD bool rp_params_ok(const rp_params &p)
{
    return rp_finite(p.max_history) && p.max_history >= 1.0f && rp_finite(p.plane_tolerance_px) && p.plane_tolerance_px > 0.0f &&
           p.normal_cos >= -1.0f && p.normal_cos <= 1.0f && p.min_weight > 0.0f && p.min_weight <= 1.0f;
}

/* pos / dir / up / right / fov of the PREVIOUS camera, fov of the current one */
FLX_HD rp_view rp_make_view(f3 pos, f3 dir, f3 up, f3 right, float fovPrev, float fovCur, int W, int H)
{
    rp_view v;
    v.pos = pos; v.dir = dir; v.up = up; v.right = right;
    v.scale = rp_tan_half_fov(fovPrev);
    v.aspect = (float)W / (float)H;
    v.footprint = 2.0f * rp_tan_half_fov(fovCur) / (float)H;
    v.W = W; v.H = H;
    return v;
}

/* P in the previous view: continuous pixel coordinates (integers = pixel centres).  false: behind the camera or not finite */
FLX_HD bool rp_project(const rp_view &vw, f3 P, float *xf, float *yf)
{
    const f3 v = P - vw.pos;
    const float z = dot(v, vw.dir);
    if (!(z > 0.0f) || !rp_finite(z)) return false;
    const float sx = dot(v, vw.right) / z, sy = dot(v, vw.up) / z;
    const float scrx = sx / vw.scale / vw.aspect, scry = sy / vw.scale;
    *xf = (scrx + 1.0f) * 0.5f * (float)vw.W - 0.5f;
    *yf = (scry + 1.0f) * 0.5f * (float)vw.H - 0.5f;
    return rp_finite(*xf) && rp_finite(*yf);
}

FLX_HD bool rp_is_hit(rp4 g0) { return (int32_t)f2u(g0.w) >= 0; }
/* the two tests that tie a tap (Pq, Nq) to the surface of the pixel (P, N); tol = plane_tolerance_px * t * footprint.  A NaN rejects. */
FLX_HD bool rp_same_plane(f3 Pq, f3 P, f3 N, float tol) { const float d = dot(Pq - P, N); return absf(d) <= tol; }
FLX_HD bool rp_same_facing(f3 Nq, f3 N, float normal_cos) { return dot(Nq, N) >= normal_cos; }

/* The new pixel from the current G-buffer record (g0, g1).  prevG0(j) / prevG1(j) / hist(j) / mom(j) -> rp4 of previous-view pixel j (flat index);
 * mom is only called when `moments`.  Returns the bit mask of the counted taps (tap order above; 0: zeros were written). */
template <class G0, class G1, class Hist, class Mom>
FLX_HD uint32_t rp_pixel(const rp_view &vw, const rp_params &rp, rp4 g0, rp4 g1, bool moments, G0 prevG0, G1 prevG1, Hist hist, Mom mom,
                         rp4 *outPx, rp4 *outMom)
{
    *outPx = mk_rp4(0.0f, 0.0f, 0.0f, 0.0f);
    *outMom = mk_rp4(0.0f, 0.0f, 0.0f, 0.0f);
    if (!rp_is_hit(g0)) return 0u;
    const f3 P = mk3(g0.x, g0.y, g0.z), N = mk3(g1.x, g1.y, g1.z);
    float xf, yf;
    if (!rp_project(vw, P, &xf, &yf)) return 0u;
    /* all four taps outside the image (also keeps the conversions to int in range) */
    if (!(xf > -1.0f && xf < (float)vw.W && yf > -1.0f && yf < (float)vw.H)) return 0u;
    const float fx0 = floorf(xf), fy0 = floorf(yf);
    const int x0 = (int)fx0, y0 = (int)fy0;
    const float fx = xf - fx0, fy = yf - fy0;
    const float tol = rp.plane_tolerance_px * g1.w * vw.footprint;

    float b[4]; rp4 h[4]; uint32_t idx[4];
    uint32_t mask = 0u;
    float S = 0.0f;
    for (int k = 0; k < 4; k++) {
        const int xj = x0 + (k & 1), yj = y0 + (k >> 1);
        if (xj < 0 || xj >= vw.W || yj < 0 || yj >= vw.H) continue;
        const uint32_t j = (uint32_t)yj * (uint32_t)vw.W + (uint32_t)xj;
        const rp4 q0 = prevG0(j);
        if (!rp_is_hit(q0)) continue;
        const rp4 hj = hist(j);
        if (!(hj.w > 0.0f) || !rp_finite(hj.w) || !rp_finite(hj.x) || !rp_finite(hj.y) || !rp_finite(hj.z)) continue;
        if (!rp_same_plane(mk3(q0.x, q0.y, q0.z), P, N, tol)) continue;
        const rp4 q1 = prevG1(j);
        if (!rp_same_facing(mk3(q1.x, q1.y, q1.z), N, rp.normal_cos)) continue;
        b[k] = ((k & 1) ? fx : 1.0f - fx) * ((k >> 1) ? fy : 1.0f - fy);
        h[k] = hj; idx[k] = j;
        S = S + b[k];
        mask |= 1u << k;
    }
    if (!mask || !(S >= rp.min_weight)) return 0u;

    f3 c = mk3(0.0f);
    float nbar = 0.0f;
    for (int k = 0; k < 4; k++) {
        if (!(mask & (1u << k))) continue;
        const float w = b[k] / S;
        c = c + (mk3(h[k].x, h[k].y, h[k].z) / h[k].w) * w;
        nbar = nbar + w * h[k].w;
    }
    const float n = fminf_(nbar, rp.max_history);
    *outPx = mk_rp4(c.x * n, c.y * n, c.z * n, n);

    if (moments) {
        rp4 m[4]; uint32_t mm = 0u;
        float Sm = 0.0f;
        for (int k = 0; k < 4; k++) {
            if (!(mask & (1u << k))) continue;
            m[k] = mom(idx[k]);
            if (!(m[k].w > 0.0f) || !rp_finite(m[k].w) || !rp_finite(m[k].x) || !rp_finite(m[k].y)) continue;
            Sm = Sm + b[k];
            mm |= 1u << k;
        }
        if (mm && Sm > 0.0f) {
            float m1 = 0.0f, m2 = 0.0f;
            for (int k = 0; k < 4; k++) {
                if (!(mm & (1u << k))) continue;
                const float w = b[k] / Sm;
                m1 = m1 + w * (m[k].x / m[k].w);
                m2 = m2 + w * (m[k].y / m[k].w);
            }
            *outMom = mk_rp4(m1 * n, m2 * n, 0.0f, n);
        }
    }
    return mask;
}

} /* namespace flx */

#endif /* FLX_REPROJECT_H */
