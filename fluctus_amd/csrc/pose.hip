// pose.hip -- flx_objects_pose: the wire triangles of the listed objects, posed on the device from the rest triangles kept
// there (arithmetic: flx_pose.h) and compacted into an ASCENDING (triangle, index) list, the device source of the subset refit (refit.hip).
//
// The members -- every triangle that belongs to an object -- are kept in triangle order.  A call stamps the listed objects with its epoch and
// records their position k in the list (k_pose_mark), then runs adaptive.hip's scheme over the members, no atomics at all:
//   k_pose_count   one thread per member in 1-D blocks of 256 CONSECUTIVE members: does the member's object carry this call's stamp; the block's
//                  count from four 64-bit ballots.
//   the scan       adaptive.hip's one-block exclusive scan of the block counts (launch_block_scan).
//   k_pose_write   stamp -> ballot -> rank by mbcnt: out[block offset + waves before + rank] = the posed triangle, ten whole 16-byte stores, and
//                  idx[...] = its triangle index.  Blocks and lanes are in member order and the members in triangle order, so idx is strictly
//                  ascending, as the subset refit requires.
#include "flx_device.h"
#include "flx_pose.h"
#include "flx_launch.h"

namespace flxd {

#define PS_BLOCK 256

__global__ __launch_bounds__(PS_BLOCK) void k_pose_mark(const uint32_t *__restrict__ ids, uint32_t count, uint32_t epoch, uint32_t *__restrict__ stamp, uint32_t *__restrict__ slot)
{
    const uint32_t k = blockIdx.x * PS_BLOCK + threadIdx.x;
    if (k >= count) return;
    const uint32_t o = ids[k];                      // (< nobjects and distinct: the host has checked the list)
    stamp[o] = epoch; slot[o] = k;
}

__device__ __forceinline__ bool ps_listed(const ObjectTables &ob, uint32_t gid) { return gid < ob.members && ob.stamp[ob.memberObj[gid]] == ob.epoch; }

__global__ __launch_bounds__(PS_BLOCK) void k_pose_count(ObjectTables ob)
{
    __shared__ uint32_t s_cnt[PS_BLOCK / 64];
    const uint64_t b = __ballot(ps_listed(ob, blockIdx.x * PS_BLOCK + threadIdx.x));
    if ((threadIdx.x & 63u) == 0u) s_cnt[threadIdx.x >> 6] = (uint32_t)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0u) ob.blockCounts[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

__global__ __launch_bounds__(PS_BLOCK) void k_pose_write(ObjectTables ob)
{
    __shared__ uint32_t s_cnt[PS_BLOCK / 64];
    const uint32_t gid = blockIdx.x * PS_BLOCK + threadIdx.x;
    const bool on = ps_listed(ob, gid);
    const uint64_t b = __ballot(on);
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) s_cnt[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    if (!on) return;
    uint32_t r = ob.blockCounts[blockIdx.x];        // (the scan has left the exclusive offsets there)
    for (uint32_t w = 0; w < wave; w++) r += s_cnt[w];
    r += mbcnt(b);                                  // r < the listed objects' members <= ob.members: both outputs hold ob.members entries
    const float4 *xf = ob.xforms + (size_t)ob.slot[ob.memberObj[gid]] * 3;
    float X[12];
    for (int j = 0; j < 3; j++) { const float4 v = xf[j]; X[4 * j] = v.x; X[4 * j + 1] = v.y; X[4 * j + 2] = v.z; X[4 * j + 3] = v.w; }
    float4 t[FLX_PS_TRI_V4];
    for (int j = 0; j < FLX_PS_TRI_V4; j++) t[j] = ob.rest[(size_t)gid * FLX_PS_TRI_V4 + j];
    flx::ps_pose_triangle(X, flx::ps_cofactors(X), t, t);
    for (int j = 0; j < FLX_PS_TRI_V4; j++) ob.out[(size_t)r * FLX_PS_TRI_V4 + j] = t[j];
    ob.outIdx[r] = ob.memberTri[gid];
}

// option "motion_history": objectOfTri[memberTri[k]] = memberObj[k] (the members are distinct triangles < the table's length: flx_objects_define)
__global__ __launch_bounds__(PS_BLOCK) void k_object_of_triangle(const uint32_t *__restrict__ memberTri, const uint32_t *__restrict__ memberObj, uint32_t members,
                                                                 uint32_t *__restrict__ objectOfTri)
{
    const uint32_t k = blockIdx.x * PS_BLOCK + threadIdx.x;
    if (k < members) objectOfTri[memberTri[k]] = memberObj[k];
}
void launch_object_of_triangle(hipStream_t s, const ObjectTables &ob, uint32_t *objectOfTri)
{
    if (!ob.members) return;
    hipLaunchKernelGGL(k_object_of_triangle, dim3((ob.members + PS_BLOCK - 1) / PS_BLOCK), dim3(PS_BLOCK), 0, s, ob.memberTri, ob.memberObj, ob.members, objectOfTri);
}

uint32_t pose_blocks(uint32_t members) { return (members + PS_BLOCK - 1) / PS_BLOCK; }

// ob.ids / ob.xforms hold the call's list (count entries); ob.epoch is the call's.  Afterwards ob.out / ob.outIdx hold the posed triangles of
// the listed objects and their triangle indices, ascending.
void launch_pose(hipStream_t s, const ObjectTables &ob, uint32_t count)
{
    if (!count || !ob.members) return;
    const uint32_t nb = pose_blocks(ob.members);
    hipLaunchKernelGGL(k_pose_mark, dim3((count + PS_BLOCK - 1) / PS_BLOCK), dim3(PS_BLOCK), 0, s, ob.ids, count, ob.epoch, ob.stamp, ob.slot);
    hipLaunchKernelGGL(k_pose_count, dim3(nb), dim3(PS_BLOCK), 0, s, ob);
    launch_block_scan(s, ob.blockCounts, nb, ob.total);
    hipLaunchKernelGGL(k_pose_write, dim3(nb), dim3(PS_BLOCK), 0, s, ob);
}

} // namespace flxd
