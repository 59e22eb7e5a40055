/*
 * flx_reproject_deform.h -- temporal reprojection across a per-triangle move (flx_reproject with option "deform_history"),
 * defined once: the moved test per triangle and the per-pixel function.
 *
 * flx_reproject_motion.h follows an object through one matrix.  A skinned character, a cloth or a morph target has no matrix: every vertex goes
 * its own way.  What is known instead is WHERE ON ITS TRIANGLE a pixel's surface point lies -- the barycentrics (u, v) the traversal returned,
 * kept by flx_gbuffer in a plane beside the slot -- and where the triangle's three vertices were at the capture (a snapshot of the positions,
 * taken lazily by the first move after a capture).  The point's place at the capture is the same barycentric mix of the old vertices.
 * The kernels (csrc/reproject.hip: k_moved_flags, k_reproject_deform) and the CPU counterpart (tests/reproject_deform_cpu.cpp) both include this
 * header; with -ffp-contract=off and the contract functions of flx_math.h their results are BIT-IDENTICAL.
 * tests/reproject_deform_reference.py restates every formula in float64.  Plain C++: nothing here needs a HIP compiler.
 *
 * PER TRIANGLE (rd_moved): moved(i) holds when any of the nine position words now differs BITWISE from the snapshot's (-0 against +0 is a move,
 * a NaN against the same NaN is none).  One byte per triangle.
 *
 * PER NEW PIXEL: the current G-buffer record (P, i, N, t), its barycentric record (u, v), the triangle's positions now p0..p2 and at the
 * capture q0..q2:
 *   a miss (i < 0)                                   -> pixel (0, 0, 0, 0), moments 0, as rp_pixel
 *   (u, v) is the sentinel (-1, -1) -- a pixel of the implicit area-light quad, whose hit index 0 names no triangle -- or i is not below the
 *   triangle count                                   -> static: P' = P, N' = N
 *   moved(i) does not hold                           -> P' = P, N' = N: the very bits
 *   otherwise   P' = bary(u, v, q0, q1, q2) = (1 - u - v) q0 + u q1 + v q2 in flx_math.h's order (u weighs vertex 1, v vertex 2: the convention
 *               of hit_values, flx_trace.h);
 *               N' = s normalize(cross(q1 - q0, q2 - q0)), s = -1 when dot(normalize(cross(p1 - p0, p2 - p0)), N) < 0 and +1 otherwise -- N faces the
 *               camera, which the winding need not -- the normalisation of N' with sqrtf and three divisions as rm_source does it.  A triangle that
 *               was degenerate at the capture has a cross product of length 0: N' is not finite, every comparison of rp_pixel rejects on a NaN,
 *               the pixel gets no history.
 *   the rest is rp_pixel (flx_reproject.h) on (P', i, N', t), with ONE more tap test, handed over as rm_pixel hands its own over (the tap is
 *   marked "holds no surface"): a tap that holds a surface is rejected when moved(i_tap) != moved(i), i_tap the tap's hit index in the previous
 *   slot; a tap with the sentinel (or an index beyond the triangle count) counts as unmoved.
 *     - a moved thing sliding over a coplanar static one shares no tap with it, either way;
 *     - a static pixel that a moved triangle has just revealed takes nothing from the moved triangle that covered it;
 *     - neighbouring triangles of one deforming mesh have both moved and keep sharing taps.
 *   KNOWN PROPERTY: two DIFFERENT moved surfaces that slide coplanar over each other both have moved(.) set and still share taps; the plane and
 *   normal tests are all that separates them (an object-aware test on top of this one is out of scope).
 * t and footprint are the CURRENT view's, as in rp_pixel.
 *
 * THE PROPERTY THAT PINS THIS: when no triangle has moved since the capture every pixel equals rp_pixel's output bit for bit (the records reach
 * rp_pixel unchanged and the extra tap test never rejects: unmoved against unmoved).
 */
#ifndef FLX_REPROJECT_DEFORM_H
#define FLX_REPROJECT_DEFORM_H

#include "flx_reproject.h"

namespace flx {

#define FLX_RD_SNAP_V4 3            /* float4 per triangle in the snapshot: (q0, 0), (q1, 0), (q2, 0) -- 48 B, one 16-byte access per vertex */
#define FLX_RD_NO_BARY (-1.0f)      /* both words of a barycentric record that names no triangle */

struct rd_tri { f3 a, b, c; };
struct rd_uv { float u, v; };

FLX_HD bool rd_no_triangle(rd_uv b) { return b.u == FLX_RD_NO_BARY && b.v == FLX_RD_NO_BARY; }

/* any of the nine position words differs bitwise */
FLX_HD bool rd_moved(const rd_tri &p, const rd_tri &q)
{
    return ((f2u(p.a.x) ^ f2u(q.a.x)) | (f2u(p.a.y) ^ f2u(q.a.y)) | (f2u(p.a.z) ^ f2u(q.a.z)) | (f2u(p.b.x) ^ f2u(q.b.x)) | (f2u(p.b.y) ^ f2u(q.b.y)) |
            (f2u(p.b.z) ^ f2u(q.b.z)) | (f2u(p.c.x) ^ f2u(q.c.x)) | (f2u(p.c.y) ^ f2u(q.c.y)) | (f2u(p.c.z) ^ f2u(q.c.z))) != 0u;
}

/* has the triangle behind this record moved?  moved(i) -> the byte of triangle i; only called with i < ntris */
template <class Moved> FLX_HD bool rd_record_moved(rp4 g0, rd_uv b, uint32_t ntris, Moved moved)
{
    const uint32_t i = f2u(g0.w);
    return !rd_no_triangle(b) && i < ntris && moved(i) != 0;
}

/* The record rp_pixel is given in place of (g0, g1) for a pixel whose triangle moved: p its positions now, q at the capture */
FLX_HD void rd_source(rd_uv b, const rd_tri &p, const rd_tri &q, rp4 *g0, rp4 *g1)
{
    const f3 N = mk3(g1->x, g1->y, g1->z);
    const f3 P = bary(b.u, b.v, q.a, q.b, q.c);
    const float s = dot(normalize(cross(p.b - p.a, p.c - p.a)), N) < 0.0f ? -1.0f : 1.0f;
    const f3 c = cross(q.b - q.a, q.c - q.a);
    const float ux = s * c.x, uy = s * c.y, uz = s * c.z;
    const float len = sqrtf((ux * ux + uy * uy) + uz * uz);
    g0->x = P.x; g0->y = P.y; g0->z = P.z;
    g1->x = ux / len; g1->y = uy / len; g1->z = uz / len;
}

/* The new pixel.  (g0, g1), b: the current record and its barycentrics; now(i) / cap(i) -> rd_tri of triangle i now / at the capture (only
 * called for a moved i < ntris); moved(i) -> its byte; prevBary(j) -> the barycentric record of previous-view pixel j (only called for a tap that
 * holds a surface); the other accessors, the outputs and the returned tap mask are rp_pixel's. */
template <class G0, class G1, class Hist, class Mom, class Bary, class Now, class Cap, class Moved>
FLX_HD uint32_t rd_pixel(const rp_view &vw, const rp_params &rp, rp4 g0, rp4 g1, rd_uv b, uint32_t ntris, bool moments, G0 prevG0, G1 prevG1,
                         Hist hist, Mom mom, Bary prevBary, Now now, Cap cap, Moved moved, rp4 *outPx, rp4 *outMom)
{
    *outPx = mk_rp4(0.0f, 0.0f, 0.0f, 0.0f);
    *outMom = mk_rp4(0.0f, 0.0f, 0.0f, 0.0f);
    if (!rp_is_hit(g0)) return 0u;
    const bool movedI = rd_record_moved(g0, b, ntris, moved);
    if (movedI) { const uint32_t i = f2u(g0.w); rd_source(b, now(i), cap(i), &g0, &g1); }
    /* the moved test, as a tap that holds no surface: rp_pixel looks at nothing else of such a tap */
    auto tapG0 = [&](uint32_t j) {
        rp4 q = prevG0(j);
        if (rp_is_hit(q) && rd_record_moved(q, prevBary(j), ntris, moved) != movedI) q.w = u2f(0xFFFFFFFFu);
        return q;
    };
    return rp_pixel(vw, rp, g0, g1, moments, tapG0, prevG1, hist, mom, outPx, outMom);
}

} /* namespace flx */

#endif /* FLX_REPROJECT_DEFORM_H */
