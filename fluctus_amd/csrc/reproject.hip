// reproject.hip -- flx_gbuffer and flx_reproject: the primary-visibility G-buffer of the current camera and the temporal
// reprojection of csrc/flx_reproject.h on the device.
//
// k_gbuffer<TREE>: one un-jittered pinhole ray through every pixel centre -- camera_direction (flx_shading.h) with the jitter (0.5, 0.5) and the
// lens at camera.pos, no lens draws -- traced with the closest-hit traversal of the extension kernels (TREE 2: flx_trace.h traverse, the
// reference's visit order; TREE 4: flx_trace4.h traverse4) and committed with hit_values (flx_trace.h), the function the logic pass commits a
// raw hit with: the implicit area-light quad included.  One lane per pixel: primary rays of neighbouring pixels are coherent, and the call runs
// once per camera change.  The grid is the extension kernels' (one lane per PATH, whatever the image size) and strides over the pixels, so the
// traversal stacks' spill columns are the ones those kernels use and stay inside their allocation.  Writes two float4 per pixel and nothing else.
// k_gbuffer<TREE, true> (option "motion_history" with objects defined) also writes the pixel's object id into the slot's object
// plane: the object of the hit triangle, FLX_NO_OBJECT for a miss, for the implicit area-light quad (whose hit index is 0) and for a triangle of
// no object.  The G-buffer records are the same bytes either way.
//
// k_reproject: one thread per pixel in 16 x 16 groups like denoise.hip; a pure gather with 16-byte accesses.  Every value comes from rp_pixel
// in its order, so the result equals tests/reproject_cpu.cpp bit for bit.
//
// k_reproject_motion: the same shape for rm_pixel (csrc/flx_reproject_motion.h) -- plus one 4-byte object id per pixel and per tap that holds a
// surface, and the motion table read through the pixel's object id (four float4 per object).  No atomics, no LDS.  Equals
// tests/reproject_motion_cpu.cpp bit for bit.
//
// Option "deform_history" (csrc/flx_reproject_deform.h).  k_gbuffer<TREE, false, true> also writes the traversal's (u, v) into the
// slot's barycentric plane, (-1, -1) on a miss and on the implicit area-light quad.  k_snapshot_positions: one thread per triangle copies its nine
// position floats out of the 160-byte records into three float4 (48 B).  k_moved_flags: one thread per triangle, one byte: the positions now
// against the snapshot, bitwise.  k_reproject_deform: k_reproject_motion's shape for rd_pixel -- plus 8 bytes of barycentrics and one flag byte per
// pixel and per tap that holds a surface, and six float4 of positions for a pixel whose triangle moved.  No atomics, no LDS.  Equals
// tests/reproject_deform_cpu.cpp bit for bit.
#include "flx_trace4.h"
#include "flx_shading.h"
#include "flx_reproject_motion.h"
#include "flx_reproject_deform.h"
#include "flx_launch.h"

namespace flxd {

// how the barycentric plane reaches k_gbuffer: an EMPTY struct in the instances without it (as MeshArg, flx_launch.h)
template <bool BARY> struct BaryArg { };
template <> struct BaryArg<true> { float2 *plane; };
__device__ __forceinline__ void bary_store(const BaryArg<false> &, uint32_t, float, float) { }
__device__ __forceinline__ void bary_store(const BaryArg<true> &b, uint32_t idx, float u, float v) { b.plane[idx] = make_float2(u, v); }

template <int TREE, bool OBJ, bool BARY>
__global__ __launch_bounds__(TRACE_BLOCK) void k_gbuffer(Scene sc, Frame fr, flx_render_params p, TraceAux aux, float4 *gb, uint32_t npix, uint32_t *objPlane,
                                                         const uint32_t *objectOfTri, BaryArg<BARY> baryArg)
{
    static_assert(TRACE_BLOCK == WIDE_BLOCK && LDS_LEVELS == WIDE_LDS_LEVELS, "one LDS stack for both trees");
    __shared__ uint32_t s_stack[LDS_LEVELS * TRACE_BLOCK];
    const uint32_t tid = blockIdx.x * TRACE_BLOCK + threadIdx.x;      // < aux.totalThreads: the spill column of this lane
    const f3 orig = V(p.camera.pos);
    for (uint32_t idx = tid; idx < npix; idx += aux.totalThreads) {
        const f3 dir = camera_direction(fr, p, idx, 0.5f, 0.5f, orig);
        float t = FLX_FLT_MAX, u = 0.0f, v = 0.0f;
        int tri = -1;
        uint32_t nInner = 0, nTri = 0, nLeaf = 0;
        if (TREE == 4) {
            WStack stk;
            stk.lds = s_stack + threadIdx.x; stk.stride = aux.totalThreads; stk.spill = aux.spill + tid; stk.base = 0;
            traverse4<false, false>(sc, stk, orig, dir, t, u, v, tri, nInner, nTri, nLeaf);
        } else {
            Stack stk;
            stk.lds = s_stack + threadIdx.x; stk.stride = aux.totalThreads; stk.spill = aux.spill + tid;
            traverse<false, false>(sc, stk, orig, dir, t, u, v, tri, nInner, nTri);
        }
        const HitVals h = hit_values<true>(sc, p, orig, dir, t, u, v, tri);
        float4 g0 = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1)), g1 = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
        if (h.tri >= 0) {
            f3 ng;
            if (h.flags & 1u) ng = V(p.areaLight.N);                    // the implicit area-light quad (it faces the ray: light_quad)
            else {
                const flx_triangle *tp = sc.tris + h.tri;
                const f3 p0 = V(tp->v0.p), p1 = V(tp->v1.p), p2 = V(tp->v2.p);
                ng = normalize(cross(p1 - p0, p2 - p0));
                if (dot(ng, dir) > 0.0f) ng = -ng;
            }
            g0 = mk4u(h.P, (uint32_t)h.tri);
            g1 = mk4(ng, h.t);
        }
        gb[2 * (size_t)idx] = g0;
        gb[2 * (size_t)idx + 1] = g1;
        if (OBJ) objPlane[idx] = (h.tri >= 0 && !(h.flags & 1u)) ? objectOfTri[h.tri] : FLX_PS_NO_OBJECT;     // (h.tri < the scene's triangle count, the table's length)
        if (BARY) {                                                     // a triangle hit: where on the triangle; anything else names no triangle
            const bool onTri = h.tri >= 0 && !(h.flags & 1u);
            bary_store(baryArg, idx, onTri ? u : FLX_RD_NO_BARY, onTri ? v : FLX_RD_NO_BARY);
        }
    }
}

// the whole call: npix = width * height of an unpartitioned context; tree 2 | 4 as flx_wf_extend picks it; spill / numTasks: the extension
// kernels' spill area and the path count it was sized for
void launch_gbuffer(hipStream_t s, const Scene &sc, const flx_render_params &p, uint32_t *spill, uint32_t numTasks, int tree, float4 *gb, uint32_t npix,
                    uint32_t *objPlane, const uint32_t *objectOfTri, float2 *baryPlane)
{
    const uint32_t maxBlocks = (numTasks + TRACE_BLOCK - 1) / TRACE_BLOCK;
    uint32_t blocks = (npix + TRACE_BLOCK - 1) / TRACE_BLOCK;
    if (blocks > maxBlocks) blocks = maxBlocks;
    TraceAux aux{spill, blocks * TRACE_BLOCK, nullptr};
    Frame fr {};
    fr.rank = 0; fr.nranks = 1; fr.localPixels = npix;
    const bool obj = objPlane && objectOfTri;                           // ("motion_history" and "deform_history" refuse each other: never both planes)
    const BaryArg<false> none; const BaryArg<true> bary{baryPlane};
    if (baryPlane && tree == 4) hipLaunchKernelGGL((k_gbuffer<4, false, true>), dim3(blocks), dim3(TRACE_BLOCK), 0, s, sc, fr, p, aux, gb, npix, nullptr, nullptr, bary);
    else if (baryPlane) hipLaunchKernelGGL((k_gbuffer<2, false, true>), dim3(blocks), dim3(TRACE_BLOCK), 0, s, sc, fr, p, aux, gb, npix, nullptr, nullptr, bary);
    else if (tree == 4 && obj) hipLaunchKernelGGL((k_gbuffer<4, true, false>), dim3(blocks), dim3(TRACE_BLOCK), 0, s, sc, fr, p, aux, gb, npix, objPlane, objectOfTri, none);
    else if (tree == 4) hipLaunchKernelGGL((k_gbuffer<4, false, false>), dim3(blocks), dim3(TRACE_BLOCK), 0, s, sc, fr, p, aux, gb, npix, nullptr, nullptr, none);
    else if (obj) hipLaunchKernelGGL((k_gbuffer<2, true, false>), dim3(blocks), dim3(TRACE_BLOCK), 0, s, sc, fr, p, aux, gb, npix, objPlane, objectOfTri, none);
    else hipLaunchKernelGGL((k_gbuffer<2, false, false>), dim3(blocks), dim3(TRACE_BLOCK), 0, s, sc, fr, p, aux, gb, npix, nullptr, nullptr, none);
}

#define RP_BX 16
#define RP_BY 16

__device__ __forceinline__ rp4 to_rp4(float4 v) { return mk_rp4(v.x, v.y, v.z, v.w); }

// cur / prev: the G-buffer slots (2 float4 per pixel); hist / histMom: the captured accumulation and moments; px / mom: the framebuffers
// (mom == nullptr: the moments are not written)
__global__ __launch_bounds__(RP_BX * RP_BY) void k_reproject(rp_view vw, rp_params rp, const float4 *cur, const float4 *prev, const float4 *hist,
                                                             const float4 *histMom, float4 *px, float4 *mom)
{
    const int x = blockIdx.x * RP_BX + threadIdx.x, y = blockIdx.y * RP_BY + threadIdx.y;
    if (x >= vw.W || y >= vw.H) return;
    const uint32_t i = (uint32_t)y * (uint32_t)vw.W + (uint32_t)x;
    rp4 o, om;
    rp_pixel(vw, rp, to_rp4(cur[2 * (size_t)i]), to_rp4(cur[2 * (size_t)i + 1]), mom != nullptr,
             [&](uint32_t j) { return to_rp4(prev[2 * (size_t)j]); }, [&](uint32_t j) { return to_rp4(prev[2 * (size_t)j + 1]); },
             [&](uint32_t j) { return to_rp4(hist[j]); }, [&](uint32_t j) { return to_rp4(histMom[j]); }, &o, &om);
    px[i] = make_float4(o.x, o.y, o.z, o.w);
    if (mom) mom[i] = make_float4(om.x, om.y, om.z, om.w);
}

void launch_reproject(hipStream_t s, const rp_view &vw, const rp_params &rp, const float4 *cur, const float4 *prev, const float4 *hist,
                      const float4 *histMom, float4 *px, float4 *mom)
{
    const dim3 blk(RP_BX, RP_BY), grid((vw.W + RP_BX - 1) / RP_BX, (vw.H + RP_BY - 1) / RP_BY);
    hipLaunchKernelGGL(k_reproject, grid, blk, 0, s, vw, rp, cur, prev, hist, histMom, px, mom);
}

// curObj / prevObj: the slots' object planes; tab: the motion table, FLX_RM_ROWS float4 per object (an id >= nobjects never reaches it: rm_object_id)
__global__ __launch_bounds__(RP_BX * RP_BY) void k_reproject_motion(rp_view vw, rp_params rp, const float4 *cur, const float4 *prev, const float4 *hist,
                                                                    const float4 *histMom, float4 *px, float4 *mom, const uint32_t *curObj,
                                                                    const uint32_t *prevObj, const float4 *tab, uint32_t nobjects)
{
    const int x = blockIdx.x * RP_BX + threadIdx.x, y = blockIdx.y * RP_BY + threadIdx.y;
    if (x >= vw.W || y >= vw.H) return;
    const uint32_t i = (uint32_t)y * (uint32_t)vw.W + (uint32_t)x;
    rp4 o, om;
    rm_pixel(vw, rp, to_rp4(cur[2 * (size_t)i]), to_rp4(cur[2 * (size_t)i + 1]), curObj[i], nobjects, mom != nullptr,
             [&](uint32_t j) { return to_rp4(prev[2 * (size_t)j]); }, [&](uint32_t j) { return to_rp4(prev[2 * (size_t)j + 1]); },
             [&](uint32_t j) { return to_rp4(hist[j]); }, [&](uint32_t j) { return to_rp4(histMom[j]); },
             [&](uint32_t j) { return prevObj[j]; }, [&](uint32_t ob, int r) { return to_rp4(tab[(size_t)ob * FLX_RM_ROWS + r]); }, &o, &om);
    px[i] = make_float4(o.x, o.y, o.z, o.w);
    if (mom) mom[i] = make_float4(om.x, om.y, om.z, om.w);
}

void launch_reproject_motion(hipStream_t s, const rp_view &vw, const rp_params &rp, const float4 *cur, const float4 *prev, const float4 *hist,
                             const float4 *histMom, float4 *px, float4 *mom, const uint32_t *curObj, const uint32_t *prevObj, const float4 *tab,
                             uint32_t nobjects)
{
    const dim3 blk(RP_BX, RP_BY), grid((vw.W + RP_BX - 1) / RP_BX, (vw.H + RP_BY - 1) / RP_BY);
    hipLaunchKernelGGL(k_reproject_motion, grid, blk, 0, s, vw, rp, cur, prev, hist, histMom, px, mom, curObj, prevObj, tab, nobjects);
}

// ---- option "deform_history": the positions at the capture, the moved flags, the per-vertex reprojection
#define RD_BLOCK 256

__device__ __forceinline__ rd_tri rd_load(const float4 *a) { rd_tri t; t.a = ld3(a[0]); t.b = ld3(a[1]); t.c = ld3(a[2]); return t; }
__device__ __forceinline__ rd_tri rd_load_now(const Scene &sc, uint32_t tri)
{
    rd_tri t; ml_vertices(sc, tri, &t.a, &t.b, &t.c); return t;
}

// snap: FLX_RD_SNAP_V4 float4 per triangle
__global__ __launch_bounds__(RD_BLOCK) void k_snapshot_positions(Scene sc, uint32_t ntris, float4 *snap)
{
    const uint32_t i = blockIdx.x * RD_BLOCK + threadIdx.x;
    if (i >= ntris) return;
    const rd_tri t = rd_load_now(sc, i);
    float4 *o = snap + (size_t)i * FLX_RD_SNAP_V4;
    o[0] = mk4(t.a, 0.0f); o[1] = mk4(t.b, 0.0f); o[2] = mk4(t.c, 0.0f);
}
void launch_snapshot_positions(hipStream_t s, const Scene &sc, uint32_t ntris, float4 *snap)
{
    if (!ntris) return;
    hipLaunchKernelGGL(k_snapshot_positions, dim3((ntris + RD_BLOCK - 1) / RD_BLOCK), dim3(RD_BLOCK), 0, s, sc, ntris, snap);
}

__global__ __launch_bounds__(RD_BLOCK) void k_moved_flags(Scene sc, uint32_t ntris, const float4 *snap, uint8_t *moved)
{
    const uint32_t i = blockIdx.x * RD_BLOCK + threadIdx.x;
    if (i >= ntris) return;
    moved[i] = rd_moved(rd_load_now(sc, i), rd_load(snap + (size_t)i * FLX_RD_SNAP_V4)) ? 1 : 0;
}
void launch_moved_flags(hipStream_t s, const Scene &sc, uint32_t ntris, const float4 *snap, uint8_t *moved)
{
    if (!ntris) return;
    hipLaunchKernelGGL(k_moved_flags, dim3((ntris + RD_BLOCK - 1) / RD_BLOCK), dim3(RD_BLOCK), 0, s, sc, ntris, snap, moved);
}

// curBary / prevBary: the slots' barycentric planes; snap / moved: the positions at the capture and the flags of k_moved_flags (a hit index
// >= ntris never reaches either: rd_record_moved)
__global__ __launch_bounds__(RP_BX * RP_BY) void k_reproject_deform(rp_view vw, rp_params rp, const float4 *cur, const float4 *prev, const float4 *hist,
                                                                    const float4 *histMom, float4 *px, float4 *mom, const float2 *curBary,
                                                                    const float2 *prevBary, Scene sc, uint32_t ntris, const float4 *snap, const uint8_t *moved)
{
    const int x = blockIdx.x * RP_BX + threadIdx.x, y = blockIdx.y * RP_BY + threadIdx.y;
    if (x >= vw.W || y >= vw.H) return;
    const uint32_t i = (uint32_t)y * (uint32_t)vw.W + (uint32_t)x;
    const float2 b = curBary[i];
    rp4 o, om;
    rd_pixel(vw, rp, to_rp4(cur[2 * (size_t)i]), to_rp4(cur[2 * (size_t)i + 1]), rd_uv{b.x, b.y}, ntris, mom != nullptr,
             [&](uint32_t j) { return to_rp4(prev[2 * (size_t)j]); }, [&](uint32_t j) { return to_rp4(prev[2 * (size_t)j + 1]); },
             [&](uint32_t j) { return to_rp4(hist[j]); }, [&](uint32_t j) { return to_rp4(histMom[j]); },
             [&](uint32_t j) { const float2 q = prevBary[j]; return rd_uv{q.x, q.y}; },
             [&](uint32_t t) { return rd_load_now(sc, t); }, [&](uint32_t t) { return rd_load(snap + (size_t)t * FLX_RD_SNAP_V4); },
             [&](uint32_t t) { return moved[t]; }, &o, &om);
    px[i] = make_float4(o.x, o.y, o.z, o.w);
    if (mom) mom[i] = make_float4(om.x, om.y, om.z, om.w);
}

void launch_reproject_deform(hipStream_t s, const rp_view &vw, const rp_params &rp, const float4 *cur, const float4 *prev, const float4 *hist,
                             const float4 *histMom, float4 *px, float4 *mom, const float2 *curBary, const float2 *prevBary, const Scene &sc,
                             uint32_t ntris, const float4 *snap, const uint8_t *moved)
{
    const dim3 blk(RP_BX, RP_BY), grid((vw.W + RP_BX - 1) / RP_BX, (vw.H + RP_BY - 1) / RP_BY);
    hipLaunchKernelGGL(k_reproject_deform, grid, blk, 0, s, vw, rp, cur, prev, hist, histMom, px, mom, curBary, prevBary, sc, ntris, snap, moved);
}

} // namespace flxd
