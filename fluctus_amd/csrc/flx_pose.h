/*
 * flx_pose.h -- posing an object by its transform (flx_objects_pose), defined once, per triangle.
 *
 * The kernel (csrc/pose.hip), the host library (host/tracer.cpp, host_capi.cpp: fh_pose_triangles) and the CPU test program
 * (tests/pose_cpu.cpp) all include this header; with -ffp-contract=off their results are BIT-IDENTICAL.  tests/pose_cases.py restates every
 * formula in float32 numpy operations and in float64.  Plain C++: nothing here needs a HIP compiler.
 *
 * X = [M | t] is a 3 x 4 row-major affine transform, X[4 r + c]: the ABSOLUTE rest -> world transform of an object.  A wire triangle is ten
 * 4-float vectors: v0 {p, n, t} v1 {p, n, t} v2 {p, n, t} {matId, pad} (flx_refit.h: rf_shade_rec).  All arithmetic is fp32, in this order:
 *   position  p'.x = ((m00 p.x + m01 p.y) + m02 p.z) + t.x,  likewise y and z
 *   normal    u = s (C n), each row r as (c_r0 n.x + c_r1 n.y) + c_r2 n.z, then times s.  C is the cofactor matrix of M (= det M x the inverse
 *             transpose, so no division and no failure for a near-singular M), c_00 = m11 m22 - m12 m21 and so on cyclically; det M =
 *             (m00 c_00 + m01 c_01) + m02 c_02; s = +1 when det M > 0, else -1: a mirroring transform keeps a normal on the side of the
 *             surface it was on.  Then n' = u / sqrt(u.u) with u.u = (u.x u.x + u.y u.y) + u.z u.z, the correctly rounded sqrt and three
 *             divisions.  A u of length 0 or of non-finite length gives what these operations give (NaN); it is stored as computed.
 *   copied    every .w word of the nine vectors, the three texcoords, matId and the pad words: bytes of the rest triangle, unchanged.
 *
 * IDENTITY.  With X = identity C is the identity, s = +1, every product by 1 is exact and every sum adds a zero: the posed positions,
 * texcoords, matId and pad words ARE the rest triangle's bytes (but for the sign of a zero: -0 + 0 = +0, which no comparison sees).  A rest
 * normal whose fp32 length is 1 to the last bit -- sqrt(fl(n.n)) == 1 -- stays too; any other is RENORMALISED, so its bytes may change.
 *
 * POSES DO NOT COMPOSE: a pose is computed from the rest triangle every time, so posing by Y after X gives what posing by Y alone gives and
 * nothing drifts however many poses follow one another.
 */
#ifndef FLX_POSE_H
#define FLX_POSE_H

#include "../../include/flx_math.h"
#include <stddef.h>

namespace flx {

#define FLX_PS_TRI_V4 10            /* 4-float vectors per wire triangle (160 B) */

/* cofactors of M (row-major, c[3 r + c]), det M and the normals' sign */
struct ps_normal_xf { float c[9]; float det, s; };

FLX_HD float ps_row(float a, float b, float c, float x, float y, float z) { return (a * x + b * y) + c * z; }

FLX_HD ps_normal_xf ps_cofactors(const float X[12])
{
    const float m00 = X[0], m01 = X[1], m02 = X[2], m10 = X[4], m11 = X[5], m12 = X[6], m20 = X[8], m21 = X[9], m22 = X[10];
    ps_normal_xf n;
    n.c[0] = m11 * m22 - m12 * m21; n.c[1] = m12 * m20 - m10 * m22; n.c[2] = m10 * m21 - m11 * m20;
    n.c[3] = m21 * m02 - m22 * m01; n.c[4] = m22 * m00 - m20 * m02; n.c[5] = m20 * m01 - m21 * m00;
    n.c[6] = m01 * m12 - m02 * m11; n.c[7] = m02 * m10 - m00 * m12; n.c[8] = m00 * m11 - m01 * m10;
    n.det = ps_row(m00, m01, m02, n.c[0], n.c[1], n.c[2]);
    n.s = n.det > 0.0f ? 1.0f : -1.0f;
    return n;
}

/* what flx_objects_pose asks of a transform: twelve finite entries and a finite, non-zero determinant (as computed above) */
FLX_HD bool ps_finite(float v) { return absf(v) <= FLX_FLT_MAX; }
FLX_HD bool ps_xform_finite(const float X[12])
{
    bool ok = true;
    for (int i = 0; i < 12; i++) ok = ok && ps_finite(X[i]);
    return ok;
}
FLX_HD bool ps_xform_invertible(const float X[12]) { const float d = ps_cofactors(X).det; return ps_finite(d) && d != 0.0f; }

/* one wire triangle: V4 is any struct of four floats x, y, z, w (float4 on the device; a template only so that this header needs no vector
 * type, as rf_shade_rec).  in and out may be the same array. */
template <class V4> FLX_HD void ps_pose_triangle(const float X[12], const ps_normal_xf &nx, const V4 in[FLX_PS_TRI_V4], V4 out[FLX_PS_TRI_V4])
{
    for (int v = 0; v < 3; v++) {
        const V4 p = in[3 * v], n = in[3 * v + 1];
        V4 q = p, u = n;
        q.x = ps_row(X[0], X[1], X[2], p.x, p.y, p.z) + X[3];
        q.y = ps_row(X[4], X[5], X[6], p.x, p.y, p.z) + X[7];
        q.z = ps_row(X[8], X[9], X[10], p.x, p.y, p.z) + X[11];
        u.x = nx.s * ps_row(nx.c[0], nx.c[1], nx.c[2], n.x, n.y, n.z);
        u.y = nx.s * ps_row(nx.c[3], nx.c[4], nx.c[5], n.x, n.y, n.z);
        u.z = nx.s * ps_row(nx.c[6], nx.c[7], nx.c[8], n.x, n.y, n.z);
        const float len = sqrtf((u.x * u.x + u.y * u.y) + u.z * u.z);
        u.x = u.x / len; u.y = u.y / len; u.z = u.z / len;
        out[3 * v] = q; out[3 * v + 1] = u; out[3 * v + 2] = in[3 * v + 2];
    }
    out[9] = in[9];
}

/* ---- the host side of flx_objects_define (and of Tracer::defineObjects): which triangles belong to an object, in triangle order ---- */

#define FLX_PS_NO_OBJECT 0xFFFFFFFFu        /* include/fluctus_hip.h: FLX_NO_OBJECT */

/* counts[o] (nobjects words, zeroed here) = members of object o; returns the number of members of all objects, or (size_t)-1 with *bad = the
 * first triangle whose id is neither < nobjects nor FLX_PS_NO_OBJECT */
inline size_t ps_count_members(const uint32_t *objectOf, size_t ntris, uint32_t nobjects, uint32_t *counts, size_t *bad)
{
    for (uint32_t o = 0; o < nobjects; o++) counts[o] = 0;
    size_t members = 0;
    for (size_t i = 0; i < ntris; i++) {
        const uint32_t o = objectOf[i];
        if (o == FLX_PS_NO_OBJECT) continue;
        if (o >= nobjects) { *bad = i; return (size_t)-1; }
        counts[o]++; members++;
    }
    return members;
}

/* member k (ascending triangle order): its triangle index, its object and its 160-byte rest triangle; every output holds `members` entries */
inline void ps_compact_members(const void *rest160, const uint32_t *objectOf, size_t ntris, uint32_t *memberTri, uint32_t *memberObj, void *memberRest160)
{
    size_t k = 0;
    for (size_t i = 0; i < ntris; i++) {
        if (objectOf[i] == FLX_PS_NO_OBJECT) continue;
        memberTri[k] = (uint32_t)i; memberObj[k] = objectOf[i];
        memcpy((char *)memberRest160 + k * 160, (const char *)rest160 + i * 160, 160);
        k++;
    }
}

/* host helper: pose `count` 160-byte wire triangles (in and out may be the same buffer, any alignment) */
struct ps_v4 { float x, y, z, w; };
inline void ps_pose_triangles(const float X[12], const void *in160, void *out160, size_t count)
{
    const ps_normal_xf nx = ps_cofactors(X);
    for (size_t i = 0; i < count; i++) {
        ps_v4 t[FLX_PS_TRI_V4];
        memcpy(t, (const char *)in160 + i * 160, 160);
        ps_pose_triangle(X, nx, t, t);
        memcpy((char *)out160 + i * 160, t, 160);
    }
}

} /* namespace flx */

#endif /* FLX_POSE_H */
