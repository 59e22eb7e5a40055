// tree_cost.hip -- flx_tree_cost's kernels: the surface-area cost sums of the binary and of the 4-wide tree as they stand in device memory
// (flx_tree_cost.h: what is summed).
//
// SCHEDULE.  One thread per record of the refit's level lists (RefitTables: blevel / wlevel -- every reachable record once; level 0 is the root
// alone, so the FIRST listed record is the root), 16-byte loads, four fp64 partial sums per thread.  A wave folds them with shuffles, the block's
// four waves through LDS, and every block stores its four sums to its row of a slab.  A second, single-block launch adds the rows: thread t takes
// rows t, t + 256, ... in order, then the same wave / LDS fold.  No floating-point atomics and no dependence on which block runs when: the
// eight numbers are a function of the arrays and of TC_BLOCK alone, bit for bit from call to call and from context to context.
#include "flx_launch.h"
#include "flx_wide.h"
#include "flx_tree_cost.h"

namespace flxd {
using namespace flxtc;

static constexpr int TC_BLOCK = 256;
static inline uint32_t tc_grid(uint32_t n) { return (n + TC_BLOCK - 1) / TC_BLOCK; }

// Every thread of the block calls it (no early returns before it).  Thread 0 stores the block's sums, waves added in wave order.
__device__ __forceinline__ void tc_block_fold(double v[TC_SUMS], double *dst)
{
    __shared__ double sm[TC_BLOCK / 64][TC_SUMS];
    for (int k = 0; k < TC_SUMS; k++)
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off, 64);
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) for (int k = 0; k < TC_SUMS; k++) sm[wave][k] = v[k];
    __syncthreads();
    if (threadIdx.x == 0) {
        double r[TC_SUMS];
        for (int k = 0; k < TC_SUMS; k++) { r[k] = sm[0][k]; for (int w = 1; w < TC_BLOCK / 64; w++) r[k] += sm[w][k]; }
        double2 *d = reinterpret_cast<double2 *>(dst);
        d[0] = make_double2(r[0], r[1]); d[1] = make_double2(r[2], r[3]);
    }
    __syncthreads();                                             // (sm is reused by the second fold of k_tree_cost_final)
}

__global__ __launch_bounds__(TC_BLOCK) void k_tree_cost_binary(const BNode *__restrict__ bnodes, const TriRec *__restrict__ trirecs, const uint32_t *__restrict__ list,
                                                                uint32_t n, double *__restrict__ slab)
{
    const uint32_t i = blockIdx.x * TC_BLOCK + threadIdx.x;
    double s[TC_SUMS] = {0.0, 0.0, 0.0, 0.0};
    if (i < n) {
        const float4 *rec = reinterpret_cast<const float4 *>(bnodes + list[i]);
        const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
        const float w[12] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w};
        const uint32_t left = __float_as_uint(r3.x), right = __float_as_uint(r3.y);
        uint32_t counts[2] = {0u, 0u};
        if (left & FLX_LEAF_BIT) counts[0] = __float_as_uint(trirecs[left & ~FLX_LEAF_BIT].b.w);
        if (right & FLX_LEAF_BIT) counts[1] = left == right ? counts[0] : __float_as_uint(trirecs[right & ~FLX_LEAF_BIT].b.w);
        tc_binary_record(w, left, right, counts, i == 0, s);
    }
    tc_block_fold(s, slab + (size_t)blockIdx.x * TC_SUMS);
}

__device__ __forceinline__ double tc_header(const float4 *h)
{
    const float4 h0 = h[0], h1 = h[1];
    const float mn[3] = {h0.x, h0.y, h0.z}, mx[3] = {h1.x, h1.y, h1.z};
    return tc_leaf_header(mn, mx, __float_as_uint(h0.w));
}

__global__ __launch_bounds__(TC_BLOCK) void k_tree_cost_wide(const float4 *__restrict__ wnodes, const float4 *__restrict__ wleaf, const uint32_t *__restrict__ list,
                                                              uint32_t n, double *__restrict__ slab)
{
    const uint32_t i = blockIdx.x * TC_BLOCK + threadIdx.x;
    double s[TC_SUMS] = {0.0, 0.0, 0.0, 0.0};
    if (i < n) {
        const float4 *rec = wnodes + (size_t)list[i] * 4;
        const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];       // flx_wide.h: WNode
        const float sc[3] = {r0.w, r1.x, r1.y};
        const uint32_t refs[4] = {__float_as_uint(r1.z), __float_as_uint(r1.w), __float_as_uint(r2.x), __float_as_uint(r2.y)};
        const uint32_t qlo[3] = {__float_as_uint(r2.z), __float_as_uint(r2.w), __float_as_uint(r3.x)};
        const uint32_t qhi[3] = {__float_as_uint(r3.y), __float_as_uint(r3.z), __float_as_uint(r3.w)};
        double leafTri[4] = {0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < 4; k++)
            if (refs[k] != FLX_WIDE_EMPTY && (refs[k] & FLX_WIDE_LEAF_BIT)) leafTri[k] = tc_header(wleaf + (refs[k] & FLX_WIDE_OFF_MASK));
        tc_wide_node(sc, refs, qlo, qhi, leafTri, i == 0, s);
    }
    tc_block_fold(s, slab + (size_t)blockIdx.x * TC_SUMS);
}

// the rows of both slabs -> out8; a tree without rows (the wide root is a leaf block) takes the sums of that block's header
__global__ __launch_bounds__(TC_BLOCK) void k_tree_cost_final(const double *__restrict__ slabB, uint32_t rowsB, const double *__restrict__ slabW, uint32_t rowsW,
                                                               const float4 *__restrict__ wleaf, uint32_t wrootRef, double *__restrict__ out8)
{
    for (int tree = 0; tree < 2; tree++) {
        const double2 *slab = reinterpret_cast<const double2 *>(tree ? slabW : slabB);
        const uint32_t rows = tree ? rowsW : rowsB;
        double s[TC_SUMS] = {0.0, 0.0, 0.0, 0.0};
        for (uint32_t r = threadIdx.x; r < rows; r += TC_BLOCK) {
            const double2 a = slab[2 * (size_t)r], b = slab[2 * (size_t)r + 1];
            s[0] += a.x; s[1] += a.y; s[2] += b.x; s[3] += b.y;
        }
        if (tree && rows == 0 && (wrootRef & FLX_WIDE_LEAF_BIT) && threadIdx.x == 0) {
            const float4 *h = wleaf + (wrootRef & FLX_WIDE_OFF_MASK);
            const float4 h0 = h[0], h1 = h[1];
            const float mn[3] = {h0.x, h0.y, h0.z}, mx[3] = {h1.x, h1.y, h1.z};
            s[TC_A_ROOT] = s[TC_S_LEAF] = tc_area(mn, mx);
            s[TC_S_TRI] = tc_leaf_header(mn, mx, __float_as_uint(h0.w));
        }
        tc_block_fold(s, out8 + tree * TC_SUMS);
    }
}

// ---- launcher (flx_launch.h).  slab: tree_cost_slab_doubles(rt) doubles -- the binary rows, the wide rows, then the eight results
static inline uint32_t tc_rows(const std::vector<uint32_t> &levelStart) { return levelStart.empty() ? 0u : tc_grid(levelStart.back()); }
size_t tree_cost_slab_doubles(const RefitTables &rt) { return ((size_t)tc_rows(rt.blevelStart) + tc_rows(rt.wlevelStart)) * TC_SUMS + 2 * TC_SUMS; }
double *launch_tree_cost(hipStream_t s, const Scene &sc, const RefitTables &rt, double *slab)
{
    const uint32_t nb = rt.blevelStart.empty() ? 0u : rt.blevelStart.back(), nw = rt.wlevelStart.empty() ? 0u : rt.wlevelStart.back();
    const uint32_t rowsB = tc_grid(nb), rowsW = tc_grid(nw);
    double *slabB = slab, *slabW = slabB + (size_t)rowsB * TC_SUMS, *out8 = slabW + (size_t)rowsW * TC_SUMS;
    const float4 *wleaf = sc.wleaf;
    if (nb) k_tree_cost_binary<<<rowsB, TC_BLOCK, 0, s>>>(sc.bnodes, sc.trirecs, rt.blevel, nb, slabB);
    if (nw) k_tree_cost_wide<<<rowsW, TC_BLOCK, 0, s>>>(reinterpret_cast<const float4 *>(sc.wnodes), wleaf, rt.wlevel, nw, slabW);
    k_tree_cost_final<<<1, TC_BLOCK, 0, s>>>(slabB, rowsB, slabW, rowsW, wleaf, sc.wrootRef, out8);
    return out8;
}

} // namespace flxd
