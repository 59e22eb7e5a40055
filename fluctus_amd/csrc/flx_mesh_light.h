// flx_mesh_light.h -- emissive triangles as lights (option "mesh_lights"): which triangles are lights, what they weigh, the
// table they are picked from, and the three functions the integrator calls.  Plain C++ that compiles for the host and the device, in the
// manner of flx_refit.h and flx_tree_cost.h: the kernels (mesh_light.hip, microkernel.hip) and the CPU side (host_capi.cpp: fh_mesh_light_*)
// run the very same functions, under the arithmetic contract of flx_math.h (fp32, no contraction, fixed order), so that a table built on the
// device and one built on the host are the SAME BYTES.
//
// LIGHT.  Triangle i is a light when its material has any Ke component > 0 (ml_is_emissive).  The list holds the indices of the lights in
// ascending order; it depends on the materials alone and is made once per flx_upload_scene.
// WEIGHT.  w = 0.5 |(p1 - p0) x (p2 - p0)| * luminance(Ke) in fp32 (ml_area, ml_luminance, ml_weight); anything that is not a positive finite
// number -- a zero-area triangle, a Ke whose luminance is not positive -- weighs 0.
// SIDE.  A light emits Ke on the side its geometric normal n_g = normalize((p1 - p0) x (p2 - p0)) faces, and nothing on the other: the rule of
// the parametric quad (light_quad culls dot(dir, N) > 0) and pbrt's default.
// TABLE, for light k of n, in THIS ORDER (ML_SCAN_BLOCK = 256 lights form a run; the runs are independent until step 2):
//   1. local64[k] = w[b 256] + ... + w[k], summed LEFT TO RIGHT in fp64 from the first light of k's run b; runSum[b] = local64 of the run's last light
//   2. off64[0] = 0, off64[b + 1] = off64[b] + runSum[b], left to right;  total64 = off64[runs]
//   3. prefix64[k] = off64[b] + local64[k];  cdf[k] = (float)(prefix64[k] / total64), and 1.0f exactly at the LAST light with w > 0
//   4. pick[k] = cdf[k] - cdf[k - 1] in fp32 (cdf[-1] = 0): the probability that enters every pdf, on both sides of the MIS weight
// Every sum adds a non-negative term to a non-negative sum, so prefix64 never decreases (round-to-nearest is monotone; across a seam
// off64[b + 1] IS the expression prefix64 of the run's last light), and neither does cdf.  A light too small for its difference to survive the
// rounding has pick = 0: it is never returned by ml_pick, and an implicit hit on it gets the MIS weight 1 (pdfA = 0), so the estimator stays
// unbiased.  total64 = 0 means NO LIGHTS: cdf and pick are all 0 and lastPick is ML_NONE.  lastPick is the last light with pick > 0.
// (Why not a tree-shaped scan: its partial sums are not monotone in k, and a cdf that steps back by an ulp is a negative probability.)
#pragma once
#include <stdint.h>
#include "../../include/flx_math.h"

#define ML_SCAN_BLOCK 256u
#define ML_NONE 0xFFFFFFFFu

namespace flxml {
using flx::f3;

FLX_HD bool ml_is_emissive(float kex, float key, float kez) { return kex > 0.0f || key > 0.0f || kez > 0.0f; }
FLX_HD float ml_luminance(f3 v) { return 0.212671f * v.x + 0.715160f * v.y + 0.072169f * v.z; }      // flx_shading.h: luminance
FLX_HD f3 ml_cross(f3 p0, f3 p1, f3 p2) { return flx::cross(p1 - p0, p2 - p0); }
FLX_HD float ml_area(f3 p0, f3 p1, f3 p2) { return 0.5f * flx::length(ml_cross(p0, p1, p2)); }
FLX_HD f3 ml_normal(f3 p0, f3 p1, f3 p2) { return flx::normalize(ml_cross(p0, p1, p2)); }
FLX_HD float ml_weight(f3 p0, f3 p1, f3 p2, f3 ke)
{
    const float w = ml_area(p0, p1, p2) * ml_luminance(ke);
    return (w > 0.0f && w <= FLX_FLT_MAX) ? w : 0.0f;
}

// steps 3 and 4 for one light: prefix64 of the light and of the one before it (0 for k = 0)
FLX_HD float ml_cdf(double prefix, double total, bool lastLive) { return total > 0.0 ? (lastLive ? 1.0f : (float)(prefix / total)) : 0.0f; }

// the first k with cdf[k] > r; none (r >= every entry: rand01 returns exactly 1.0f when (float)seed * 2^-32 rounds up) -> lastPick.
// cdf[k - 1] <= r < cdf[k] makes pick[k] > 0, so a light with pick = 0 is never returned.  Needs n > 0 and lastPick != ML_NONE.
FLX_HD uint32_t ml_pick(const float *cdf, uint32_t n, uint32_t lastPick, float r)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2u; if (cdf[mid] > r) hi = mid; else lo = mid + 1u; }
    return lo < n ? lo : lastPick;
}

// the light record of triangle `tri`: a binary search of the ascending list; ML_NONE when the triangle is no light
FLX_HD uint32_t ml_find(const uint32_t *list, uint32_t n, uint32_t tri)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2u; if (list[mid] < tri) lo = mid + 1u; else hi = mid; }
    return (lo < n && list[lo] == tri) ? lo : ML_NONE;
}

// uniform by area: s = sqrt(r1), P = (1 - s) p0 + s (1 - r2) p1 + s r2 p2, coefficients first, terms added left to right
FLX_HD f3 ml_bary(float r1, float r2) { const float s = sqrtf(r1); return flx::mk3(1.0f - s, s * (1.0f - r2), s * r2); }
FLX_HD f3 ml_sample_triangle(f3 p0, f3 p1, f3 p2, float r1, float r2)
{
    const f3 b = ml_bary(r1, r2);
    return b.x * p0 + b.y * p1 + b.z * p2;
}
// the area pdf of a point on light k, for the sample and for an implicit hit alike
FLX_HD float ml_pdf_area(float pick, float area) { return pick / area; }

#if !defined(__HIP_DEVICE_COMPILE__)
// The whole table on the host, steps 1-4 in the order above.  pos(i, v) -> f3 is vertex v of triangle i, ke(i) -> f3 the Ke of its material;
// list[0..n) the ascending lights.  cdf / pick: n floats each.  Returns total64; *lastPick as described.
template <class Pos, class Ke>
inline double ml_build_table(const uint32_t *list, uint32_t n, Pos pos, Ke ke, float *cdf, float *pick, uint32_t *lastPick)
{
    const uint32_t runs = (n + ML_SCAN_BLOCK - 1u) / ML_SCAN_BLOCK;
    double *local = n ? new double[n] : nullptr, *off = new double[runs + 1u];
    uint32_t lastLive = ML_NONE;
    off[0] = 0.0;
    for (uint32_t b = 0; b < runs; b++) {
        double s = 0.0;
        for (uint32_t k = b * ML_SCAN_BLOCK; k < n && k < (b + 1u) * ML_SCAN_BLOCK; k++) {
            const float w = ml_weight(pos(list[k], 0), pos(list[k], 1), pos(list[k], 2), ke(list[k]));
            if (w > 0.0f) lastLive = k;
            s = s + (double)w; local[k] = s;
        }
        off[b + 1u] = off[b] + s;
    }
    const double total = off[runs];
    *lastPick = ML_NONE;
    float prev = 0.0f;
    for (uint32_t k = 0; k < n; k++) {
        cdf[k] = ml_cdf(off[k / ML_SCAN_BLOCK] + local[k], total, k == lastLive);
        pick[k] = cdf[k] - prev; prev = cdf[k];
        if (pick[k] > 0.0f) *lastPick = k;
    }
    delete[] local; delete[] off;
    return total;
}
#endif

} // namespace flxml
