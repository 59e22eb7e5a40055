// flx_refit.h -- the arithmetic of the refit (refit.hip): new boxes for BOTH traversal trees from moved triangles, topology untouched.
// Plain C++ that compiles for the host and the device, so the CPU tests run the very functions the kernels run (host_capi.cpp: fh_refit_quantise).
//
// WHAT IS REFITTED.  Leaves first: a leaf box is the exact fp32 union of the FULL bounds of the leaf's triangles.  An SBVH leaf that a spatial
// split had clipped to its side of the plane (src/sbvh.cpp:410-449) therefore becomes UNCLIPPED: it still contains every point of its triangles
// that the clipped box contained, so every hit the builder's tree finds is found -- the box is only looser.  Inner boxes are the union of their
// children.  min / max do not depend on the order of their operands (up to the sign of a zero, which no comparison sees; the kernels and
// BVH::refit still fold in ONE order -- index-list order, v0 v1 v2, left before right -- so that their results agree bit for bit).
//
// WHY THE TRAVERSAL KERNELS NEED NO CHANGE.  flx_wide.h's exactness argument asks for (1) nested boxes: true by construction, a parent is the union
// of its children; (2) quantised planes that contain the child's exact box in REAL arithmetic: rf_quantise_axis below; (3) an exact fp32 leaf box
// tested with the reference's slab arithmetic: the leaf header is rewritten with the same union the binary tree's parent record gets.
//
// A SUBSET (flx_update_triangles_subset) rewrites only the leaves holding a listed triangle and the records above them, with the
// same folds and the same quantiser; a leaf none of whose triangles is listed keeps its box, clipped or not -- its triangles have not moved -- and
// the three conditions hold as above, since every rewritten box is a union of what lies below it.
//
// THE QUANTISER IN FP64. The host (flx_wide.h: quantise_children) works in long double; the device has fp64.  For fp32 operands c >= lo the
// difference d = c - lo is NOT always an fp64 number (2^61 - 2^-100 needs 161 bits), but TwoSum (Knuth; Moller 1965) gives it as an unevaluated
// sum d = dh + dl EXACTLY, dh = fl(c - lo), |dl| <= ulp(dh) / 2: no operand overflows (|c|, |lo| <= 2^62) and every quantity is a multiple of
// 2^-149, far above fp64's subnormals, so the six operations are error free.  With s = 2^e:
//   lower plane  q = floor(dh / s)  (the division by a power of two is exact), r = dh - q s in [0, s) is exact (q = 0: r = dh; q >= 1:
//                dh / 2 <= q s <= dh, Sterbenz).  q s <= d  <=>  r + dl >= 0  <=>  r >= -dl (both fp64 numbers: an exact comparison).  Otherwise q - 1:
//                (q - 1) s = dh - r - s <= dh - s <= d, because |dl| <= dh 2^-53 <= 255 s 2^-53 < s.
//   upper plane  q = ceil(dh / s), r = q s - dh in [0, s).  q >= 2: q s < 2 dh, Sterbenz, r exact.  q = 1: dh <= s; for dh >= s / 2 Sterbenz again, for
//                dh < s / 2 the rounded r is >= s / 2 > |dl|.  q = 0: dh = 0, hence c == lo and dl = 0.  q s >= d  <=>  r >= dl; otherwise q + 1 (as above).
//                q > 255: this scale does not fit, take the next.
// The first exponent tried is floor(log2(ext / 255)) clamped to -108 -- at or below every exponent that can fit, since a fitting s has
// 255 s >= ext -- and `fits` is monotone in e, so the loop ends on the SMALLEST power of two that fits.  The host's first guess is the rounded
// ceil(log2()) of the same number: at a power-of-two boundary it may start one higher, where its grid is valid too (tests: scale <= 2 x host).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FLX_RF_HD __host__ __device__ inline
#else
#define FLX_RF_HD inline
#endif

namespace flxrf {

#define FLX_RF_MIN_EXP (-108)          // flx_wide.h: the smallest scale exponent a WNode carries

FLX_RF_HD double rf_pow2d(int e) { const uint64_t b = (uint64_t)(e + 1023) << 52; double d; __builtin_memcpy(&d, &b, 8); return d; }
FLX_RF_HD float rf_pow2f(int e) { const uint32_t b = (uint32_t)(e + 127) << 23; float f; __builtin_memcpy(&f, &b, 4); return f; }
FLX_RF_HD int rf_exponent(double x) { uint64_t b; __builtin_memcpy(&b, &x, 8); return (int)((b >> 52) & 0x7FFu) - 1023; }   // floor(log2 x), x normal and > 0

// first-of-equals folds, as Box::expand (host/bvh.hpp) folds
FLX_RF_HD float rf_min(float acc, float v) { return v < acc ? v : acc; }
FLX_RF_HD float rf_max(float acc, float v) { return v > acc ? v : acc; }

// The shading record of one wire triangle -- ten 4-float vectors: v0 {p, n, t} v1 {p, n, t} v2 {p, n, t} {matId, pad} -- as the traversal and
// material kernels read it (ShadeRec, flx_device.h): the three normals, the uvs packed into the spare words, the matId's bits last.  V4 is
// float4 on both sides (a template only so that this header needs no vector type); flx_upload_scene and the refit's shade pass both call it.
template <class V4> FLX_RF_HD void rf_shade_rec(const V4 t[10], V4 &a, V4 &b, V4 &c, V4 &d)
{
    a.x = t[1].x; a.y = t[1].y; a.z = t[1].z; a.w = t[2].x;
    b.x = t[4].x; b.y = t[4].y; b.z = t[4].z; b.w = t[2].y;
    c.x = t[7].x; c.y = t[7].y; c.z = t[7].z; c.w = t[5].x;
    d.x = t[5].y; d.y = t[8].x; d.z = t[8].y; d.w = t[9].x;
}

struct Split { double h, l; };         // h + l, exactly
FLX_RF_HD Split rf_diff(float c, float lo)
{
    const double a = (double)c, b = -(double)lo;
    const double s = a + b, bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}

// One axis of one wide node: the children's [cmin, cmax] (ns of them, 2..4) -> origin, scale, the packed planes (byte k = child k; unused
// slots inverted: lo 255, hi 0).  Returns the exponent chosen.
FLX_RF_HD int rf_quantise_axis(const float cmin[4], const float cmax[4], int ns, float *o, float *s, uint32_t *qlo, uint32_t *qhi)
{
    float lo = cmin[0], hi = cmax[0];
    for (int k = 1; k < ns; k++) { lo = rf_min(lo, cmin[k]); hi = rf_max(hi, cmax[k]); }
    const double ext = (double)hi - (double)lo;
    int e = ext > 0.0 ? rf_exponent(ext * (1.0 / 255.0)) - 1 : FLX_RF_MIN_EXP;       // (-1: the product by 1 / 255 is rounded)
    if (e < FLX_RF_MIN_EXP) e = FLX_RF_MIN_EXP;
    for (;; e++) {
        const double sc = rf_pow2d(e), inv = rf_pow2d(-e);
        uint32_t pl = 0, ph = 0; bool ok = true;
        for (int k = 0; k < 4; k++) {
            if (k >= ns) { pl |= 255u << (8 * k); continue; }
            const Split dlo = rf_diff(cmin[k], lo), dhi = rf_diff(cmax[k], lo);
            double ql = __builtin_floor(dlo.h * inv);
            if (ql > 255.0) { ok = false; break; }
            if (ql > 0.0 && dlo.h - ql * sc < -dlo.l) ql -= 1.0;
            double qh = __builtin_ceil(dhi.h * inv);
            if (qh > 255.0) { ok = false; break; }
            if (qh * sc - dhi.h < dhi.l) qh += 1.0;
            if (qh > 255.0) { ok = false; break; }
            pl |= (uint32_t)ql << (8 * k); ph |= (uint32_t)qh << (8 * k);
        }
        if (ok || e >= 127) { *o = lo; *s = rf_pow2f(e); *qlo = pl; *qhi = ph; return e; }     // (e = 127 is out of reach: |coordinate| <= 2^62)
    }
}

} // namespace flxrf
