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
#include "flx_trace4.h"
#include "flx_shading.h"
#include "flx_reproject_motion.h"
#include "flx_launch.h"

namespace flxd {

template <int TREE, bool OBJ>
__global__ __launch_bounds__(TRACE_BLOCK) void k_gbuffer(Scene sc, Frame fr, flx_render_params p, TraceAux aux, float4 *gb, uint32_t npix, uint32_t *objPlane,
                                                         const uint32_t *objectOfTri)
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
    }
}

// the whole call: npix = width * height of an unpartitioned context; tree 2 | 4 as flx_wf_extend picks it; spill / numTasks: the extension
// kernels' spill area and the path count it was sized for
void launch_gbuffer(hipStream_t s, const Scene &sc, const flx_render_params &p, uint32_t *spill, uint32_t numTasks, int tree, float4 *gb, uint32_t npix,
                    uint32_t *objPlane, const uint32_t *objectOfTri)
{
    const uint32_t maxBlocks = (numTasks + TRACE_BLOCK - 1) / TRACE_BLOCK;
    uint32_t blocks = (npix + TRACE_BLOCK - 1) / TRACE_BLOCK;
    if (blocks > maxBlocks) blocks = maxBlocks;
    TraceAux aux{spill, blocks * TRACE_BLOCK, nullptr};
    Frame fr {};
    fr.rank = 0; fr.nranks = 1; fr.localPixels = npix;
    const bool obj = objPlane && objectOfTri;
    if (tree == 4 && obj) hipLaunchKernelGGL((k_gbuffer<4, true>), dim3(blocks), dim3(TRACE_BLOCK), 0, s, sc, fr, p, aux, gb, npix, objPlane, objectOfTri);
    else if (tree == 4) hipLaunchKernelGGL((k_gbuffer<4, false>), dim3(blocks), dim3(TRACE_BLOCK), 0, s, sc, fr, p, aux, gb, npix, nullptr, nullptr);
    else if (obj) hipLaunchKernelGGL((k_gbuffer<2, true>), dim3(blocks), dim3(TRACE_BLOCK), 0, s, sc, fr, p, aux, gb, npix, objPlane, objectOfTri);
    else hipLaunchKernelGGL((k_gbuffer<2, false>), dim3(blocks), dim3(TRACE_BLOCK), 0, s, sc, fr, p, aux, gb, npix, nullptr, nullptr);
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

} // namespace flxd
