/*
 * flx_adaptive.h -- the stopping rule of the adaptive microkernel render (flx_mk_adaptive_update), defined once, per pixel.
 *
 * The second consumer of the luminance moments (option "moments", which = 7): a pixel stops taking samples when the standard error of
 * its mean luminance is small against the mean.  The kernels (csrc/adaptive.hip) and the CPU counterpart (tests/adaptive_cpu.cpp) both
 * include this header; with -ffp-contract=off and the contract functions of flx_math.h their flags and lists are BIT-IDENTICAL.
 * tests/adaptive_reference.py restates every formula in float64.
 *
 * Per pixel, from the moments record (S1, S2, _, n) -- sums of l and l^2 over the n samples splatted; only the moments' own n enters:
 *   mu = S1 / n,   v = max(0, S2 / n - mu^2) / n   (the variance of the MEAN, the expression of flx_denoise_vg.h),
 *   r  = sqrt(v) / (mu + lum_floor)                (the relative standard error; lum_floor keeps a black pixel from never converging)
 *   done       n >= max_samples
 *   converged  n >= min_samples and n >= 2 and r <= threshold, with S1, S2, n, mu, S2 / n and mu^2 finite and mu + lum_floor > 0;
 *              every comparison is written so that a NaN or a non-finite sum gives "not converged" -- such a pixel runs to max_samples.
 *              (fmaxf_ is minNum/maxNum: max(0, NaN) = 0, so the finiteness tests are what keeps a NaN pixel from converging with r = 0.)
 *   own        !done && !converged
 *   active     !done && (own || (dilate && one of the 3 x 3 neighbours inside the image has own))
 * The dilation guards a pixel whose first samples all missed a caustic or a light edge that its neighbour has seen: a converged pixel
 * next to an unconverged one keeps sampling, so it may RESUME -- harmless, the integrator's state is per pixel.
 *
 * The list of active pixels is ascending in the pixel index (a stable compaction), so it is reproducible and equals the counterpart's.
 */
#ifndef FLX_ADAPTIVE_H
#define FLX_ADAPTIVE_H

#include "../../include/flx_math.h"

namespace flx {

/* defaults (threshold from the sweep of tests/test_adaptive.py over the oracle's per-sample renders) */
#define FLX_AD_DEFAULT_THRESHOLD 0.05f
#define FLX_AD_DEFAULT_MIN_SAMPLES 4u
#define FLX_AD_DEFAULT_MAX_SAMPLES 32u
#define FLX_AD_DEFAULT_LUM_FLOOR 0.01f
#define FLX_AD_DEFAULT_DILATE 1u

/* flag bits of one pixel */
enum { FLX_AD_OWN = 1u, FLX_AD_ACTIVE = 2u, FLX_AD_DONE = 4u, FLX_AD_CONVERGED = 8u };

struct ad4 { float x, y, z, w; };
struct ad_params { float threshold; uint32_t min_samples, max_samples; float lum_floor; uint32_t dilate; };

FLX_HD bool ad_finite(float v) { return absf(v) <= FLX_FLT_MAX; }
/* min_samples and max_samples are compared with the float count: both must be exactly representable */
FLX_HD bool ad_params_ok(const ad_params &p)
{
    return p.threshold >= 0.0f && ad_finite(p.threshold) && p.lum_floor >= 0.0f && ad_finite(p.lum_floor) &&
           p.max_samples >= 1u && p.min_samples <= p.max_samples && p.max_samples <= (1u << 24) && p.dilate <= 1u;
}

/* the relative standard error of the pixel mean; false (and *r = FLX_FLT_MAX) where it does not exist */
FLX_HD bool ad_rel_error(ad4 m, float lum_floor, float *r)
{
    *r = FLX_FLT_MAX;
    const float n = m.w;
    if (!(n > 0.0f) || !ad_finite(n) || !ad_finite(m.x) || !ad_finite(m.y)) return false;
    const float mu = m.x / n, m2 = m.y / n, sq = mu * mu;
    if (!ad_finite(mu) || !ad_finite(m2) || !ad_finite(sq)) return false;
    const float den = mu + lum_floor;
    if (!(den > 0.0f)) return false;
    const float v = fmaxf_(m2 - sq, 0.0f) / n;
    *r = sqrtf(v) / den;
    return *r == *r;
}

FLX_HD bool ad_done(ad4 m, const ad_params &p) { return m.w >= (float)p.max_samples; }
FLX_HD bool ad_converged(ad4 m, const ad_params &p)
{
    float r;
    if (!ad_rel_error(m, p.lum_floor, &r)) return false;
    return m.w >= (float)p.min_samples && m.w >= 2.0f && r <= p.threshold;
}
/* FLX_AD_DONE | FLX_AD_CONVERGED | FLX_AD_OWN of one record */
FLX_HD uint32_t ad_own_flags(ad4 m, const ad_params &p)
{
    const bool d = ad_done(m, p), c = ad_converged(m, p);
    return (d ? FLX_AD_DONE : 0u) | (c ? FLX_AD_CONVERGED : 0u) | (!d && !c ? FLX_AD_OWN : 0u);
}

/* all four flags of pixel (x, y).  mom(j) -> ad4 of pixel j (flat index); neighbours in row-major order, left out beyond the border */
template <class Mom>
FLX_HD uint32_t ad_pixel(int x, int y, int W, int H, const ad_params &p, Mom mom)
{
    uint32_t f = ad_own_flags(mom((uint32_t)y * (uint32_t)W + (uint32_t)x), p);
    bool act = (f & FLX_AD_OWN) != 0u;
    if (!act && !(f & FLX_AD_DONE) && p.dilate) {
        for (int dy = -1; dy <= 1 && !act; dy++)
            for (int dx = -1; dx <= 1 && !act; dx++) {
                const int xj = x + dx, yj = y + dy;
                if ((dx == 0 && dy == 0) || xj < 0 || xj >= W || yj < 0 || yj >= H) continue;
                act = (ad_own_flags(mom((uint32_t)yj * (uint32_t)W + (uint32_t)xj), p) & FLX_AD_OWN) != 0u;
            }
    }
    return f | (act ? FLX_AD_ACTIVE : 0u);
}

} /* namespace flx */

#endif /* FLX_ADAPTIVE_H */
