/*
 * flx_reproject_motion.h -- temporal reprojection across a pose of objects (flx_reproject with option "motion_history"),
 * defined once: the per-object table and the per-pixel function.
 *
 * flx_reproject.h carries the accumulated image across a camera move of a static scene.  flx_objects_pose moves an object by one ABSOLUTE
 * 3 x 4 matrix (flx_pose.h), so where a surface point of a posed object was at the capture is one matrix product away and no per-vertex
 * history is involved.  The kernel (csrc/reproject.hip: k_reproject_motion) and the CPU counterpart (tests/reproject_motion_cpu.cpp) both
 * include this header; with -ffp-contract=off and the contract functions of flx_math.h their results are BIT-IDENTICAL.
 * tests/reproject_motion_reference.py restates every formula in float64.  Plain C++: nothing here needs a HIP compiler.
 *
 * PER OBJECT (rm_make_table, host only; the library and the tests call this one function).  X_cap: the object's pose at the capture, X_now: its
 * pose now, each with a `known` flag -- a pose is unknown until the object has been posed since its definition, because the uploaded triangles
 * need not be the rest pose.  Four 4-float rows per object (64 B):
 *     rows 0..2   D = X_cap . X_now^-1 as a 3 x 4 affine matrix: current world -> world at the capture.  The inverse and the product are
 *                 computed in float64 and every entry is rounded ONCE to fp32.
 *     row 3       (moved, no_history, 0, 0) as 0.0f / 1.0f
 *   never posed (X_now unknown)                 -> static: D = identity, moved = 0
 *   posed since, pose at the capture unknown    -> no_history = 1 (and moved = 1: where it was is not known, so it shares no tap), D = identity
 *   the 48 bytes of X_cap and X_now are equal   -> D is EXACTLY the identity, moved = 0
 *   otherwise                                   -> moved = 1
 *
 * PER NEW PIXEL: the current G-buffer record (P, i, N, t), its object id o (the object plane of flx_gbuffer: FLX_NO_OBJECT for a miss, the
 * implicit area-light quad and a triangle of no object; an id >= nobjects is read as FLX_NO_OBJECT), then
 *   o == FLX_NO_OBJECT or moved[o] == 0   -> P' = P, N' = N: the very bits, not a product by the identity
 *   no_history[o]                         -> pixel (0, 0, 0, 0), moments 0
 *   otherwise   P'.x = ((d00 P.x + d01 P.y) + d02 P.z) + d03, likewise y and z;  N' = s C(D) N renormalised with sqrtf and three divisions
 *               -- flx_pose.h's operations in flx_pose.h's order (ps_row, ps_cofactors): C the cofactor matrix of D's linear part, s = -1 when
 *               its determinant is not > 0.  A non-finite N' rejects every tap (every comparison of rp_pixel is written so that a NaN rejects).
 *   the rest is rp_pixel (flx_reproject.h) on (P', i, N', t): projection into the previous view, four bilinear taps in its order, plane test
 *   |(P_j - P') . N'| <= plane_tolerance_px t footprint, normal test, renormalisation, max_history, the moments' rule -- with ONE more tap test:
 *   a tap whose object id o_j differs from o is rejected when moved[o] or moved[o_j].  (A decal sliding on a wall, a box standing on the
 *   floor: coplanar and parallel, so the plane and normal tests pass.)  When neither moved the tap is judged as rp_pixel judges it: two unmoved
 *   objects that tile one floor keep sharing history.
 * t and footprint are the CURRENT view's, as in rp_pixel.  Under a D that scales, lengths at the capture differ from lengths now by that scale,
 * so the plane tolerance is only approximately plane_tolerance_px pixels of the previous view.
 *
 * THE PROPERTY THAT PINS THIS: when no object has moved every pixel equals rp_pixel's output bit for bit (the records reach rp_pixel unchanged
 * and the extra tap test never rejects).
 */
#ifndef FLX_REPROJECT_MOTION_H
#define FLX_REPROJECT_MOTION_H

#include "flx_reproject.h"
#include "flx_pose.h"

namespace flx {

#define FLX_RM_ROWS 4               /* 4-float rows per object in the motion table (64 B) */

/* the object id as the per-pixel function uses it */
FLX_HD uint32_t rm_object_id(uint32_t o, uint32_t nobjects) { return o < nobjects ? o : FLX_PS_NO_OBJECT; }

/* The record rp_pixel is given in place of (g0, g1).  tab(o, r) -> row r of object o.  Returns 0: unchanged (no object, or one that did not
 * move), 1: moved -- *g0 / *g1 now hold (P', i) and (N', t), 2: the object has no history */
template <class Tab> FLX_HD int rm_source(uint32_t o, Tab tab, rp4 *g0, rp4 *g1)
{
    if (o == FLX_PS_NO_OBJECT) return 0;
    const rp4 fl = tab(o, 3);
    if (fl.y != 0.0f) return 2;
    if (fl.x == 0.0f) return 0;
    const rp4 r0 = tab(o, 0), r1 = tab(o, 1), r2 = tab(o, 2);
    const float D[12] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w};
    const ps_normal_xf nx = ps_cofactors(D);
    const float px = g0->x, py = g0->y, pz = g0->z, nxx = g1->x, nyy = g1->y, nzz = g1->z;
    g0->x = ps_row(D[0], D[1], D[2], px, py, pz) + D[3];
    g0->y = ps_row(D[4], D[5], D[6], px, py, pz) + D[7];
    g0->z = ps_row(D[8], D[9], D[10], px, py, pz) + D[11];
    const float ux = nx.s * ps_row(nx.c[0], nx.c[1], nx.c[2], nxx, nyy, nzz);
    const float uy = nx.s * ps_row(nx.c[3], nx.c[4], nx.c[5], nxx, nyy, nzz);
    const float uz = nx.s * ps_row(nx.c[6], nx.c[7], nx.c[8], nxx, nyy, nzz);
    const float len = sqrtf((ux * ux + uy * uy) + uz * uz);
    g1->x = ux / len; g1->y = uy / len; g1->z = uz / len;
    return 1;
}

/* The new pixel.  (g0, g1), o: the current record and its object id; prevObj(j) -> the object id of previous-view pixel j; the other
 * accessors, the outputs and the returned tap mask are rp_pixel's.  prevObj and tab are only called for a tap that holds a surface. */
template <class G0, class G1, class Hist, class Mom, class Obj, class Tab>
FLX_HD uint32_t rm_pixel(const rp_view &vw, const rp_params &rp, rp4 g0, rp4 g1, uint32_t o, uint32_t nobjects, bool moments, G0 prevG0, G1 prevG1,
                         Hist hist, Mom mom, Obj prevObj, Tab tab, rp4 *outPx, rp4 *outMom)
{
    *outPx = mk_rp4(0.0f, 0.0f, 0.0f, 0.0f);
    *outMom = mk_rp4(0.0f, 0.0f, 0.0f, 0.0f);
    if (!rp_is_hit(g0)) return 0u;
    o = rm_object_id(o, nobjects);
    const int src = rm_source(o, tab, &g0, &g1);
    if (src == 2) return 0u;
    const bool movedO = src == 1;
    /* the object test, as a tap that holds no surface: rp_pixel looks at nothing else of such a tap */
    auto tapG0 = [&](uint32_t j) {
        rp4 q = prevG0(j);
        if (rp_is_hit(q)) {
            const uint32_t oj = rm_object_id(prevObj(j), nobjects);
            if (oj != o && (movedO || (oj != FLX_PS_NO_OBJECT && tab(oj, 3).x != 0.0f))) q.w = u2f(0xFFFFFFFFu);
        }
        return q;
    };
    return rp_pixel(vw, rp, g0, g1, moments, tapG0, prevG1, hist, mom, outPx, outMom);
}

/* ---- the per-object table (host) ---- */

struct rm_row { float x, y, z, w; };

/* Xcap / Xnow: nobjects x 12 floats (row-major [M | t]), knownCap / knownNow: one byte per object; out: nobjects x FLX_RM_ROWS rows.
 * Returns true when any object has moved or no_history set (then the motion-aware kernel is needed). */
inline bool rm_make_table(uint32_t nobjects, const float *Xcap, const uint8_t *knownCap, const float *Xnow, const uint8_t *knownNow, rm_row *out)
{
    bool any = false;
    for (uint32_t o = 0; o < nobjects; o++) {
        rm_row *r = out + (size_t)o * FLX_RM_ROWS;
        r[0] = rm_row{1.0f, 0.0f, 0.0f, 0.0f}; r[1] = rm_row{0.0f, 1.0f, 0.0f, 0.0f}; r[2] = rm_row{0.0f, 0.0f, 1.0f, 0.0f};
        r[3] = rm_row{0.0f, 0.0f, 0.0f, 0.0f};
        if (!knownNow[o]) continue;                                     /* never posed: static */
        const float *A = Xcap + 12 * (size_t)o, *B = Xnow + 12 * (size_t)o;
        if (!knownCap[o]) { r[3].x = 1.0f; r[3].y = 1.0f; any = true; continue; }
        if (memcmp(A, B, 48) == 0) continue;                            /* the same bytes: D is exactly the identity */
        /* B^-1 = [Mi | -Mi t] with Mi the adjugate over the determinant, in float64 */
        const double m00 = B[0], m01 = B[1], m02 = B[2], m10 = B[4], m11 = B[5], m12 = B[6], m20 = B[8], m21 = B[9], m22 = B[10];
        const double c00 = m11 * m22 - m12 * m21, c01 = m12 * m20 - m10 * m22, c02 = m10 * m21 - m11 * m20;
        const double c10 = m21 * m02 - m22 * m01, c11 = m22 * m00 - m20 * m02, c12 = m20 * m01 - m21 * m00;
        const double c20 = m01 * m12 - m02 * m11, c21 = m02 * m10 - m00 * m12, c22 = m00 * m11 - m01 * m10;
        const double det = m00 * c00 + m01 * c01 + m02 * c02;
        const double Mi[9] = {c00 / det, c10 / det, c20 / det, c01 / det, c11 / det, c21 / det, c02 / det, c12 / det, c22 / det};
        double Bi[12];
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) Bi[4 * i + j] = Mi[3 * i + j];
            Bi[4 * i + 3] = -(Mi[3 * i] * (double)B[3] + Mi[3 * i + 1] * (double)B[7] + Mi[3 * i + 2] * (double)B[11]);
        }
        float D[12];
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 4; j++) {
                double v = (double)A[4 * i] * Bi[j] + (double)A[4 * i + 1] * Bi[4 + j] + (double)A[4 * i + 2] * Bi[8 + j];
                if (j == 3) v += (double)A[4 * i + 3];
                D[4 * i + j] = (float)v;
            }
        }
        r[0] = rm_row{D[0], D[1], D[2], D[3]}; r[1] = rm_row{D[4], D[5], D[6], D[7]}; r[2] = rm_row{D[8], D[9], D[10], D[11]};
        r[3].x = 1.0f; any = true;
    }
    return any;
}

} /* namespace flx */

#endif /* FLX_REPROJECT_MOTION_H */
