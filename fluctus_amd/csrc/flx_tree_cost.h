// flx_tree_cost.h -- the surface-area cost sums of both traversal trees (tree_cost.hip, flx_tree_cost): what is summed, once.
// Plain C++ that compiles for the host and the device, like flx_refit.h: the kernels include it, and so does the host library, whose CPU tests
// run these very functions (host_capi.cpp: fh_tree_cost_*).
//
// FOUR SUMS PER TREE, over the records the traversal kernels walk, as they stand in device memory (fresh upload or any number of refits):
//   A_root   the area of the root box
//   S_node   the areas of the boxes a ray tests to ENTER AN INNER NODE (A_root included: the root is entered by every ray that is counted)
//   S_leaf   the areas of the boxes a ray tests to enter a leaf
//   S_tri    per leaf, the area of the last box tested before its triangles x the number of triangles
// A(box) = 2 (dx dy + dy dz + dz dx) in fp64.  The two-constant SAH with both constants 1 is (S_node + S_tri) / A_root (include/fluctus_hip.h:
// flxTreeCostValue); the sums are reported apart so that other constants need no new kernel.
//
// BINARY TREE (BNode, flx_device.h).  Each half of a listed record is a child box: an inner child's goes to S_node, a leaf run's to S_leaf and,
// times the count in the run's first TriRec, to S_tri.  A_root is the union of the root record's halves.  The synthetic root of a one-leaf scene
// follows the same rule: both halves lead to the same leaf and both count (the kernels test both).
//
// 4-WIDE TREE (WNode, flx_wide.h).  A used slot's box is the one the node test sees, decoded from the grid: [o + qlo s, o + qhi s] per axis.  Its
// extent (qhi - qlo) s is exact in fp64 (an 8-bit integer times a power of two), so the area carries the roundings of the products and sums only;
// the union of a node's slots has the extent (max qhi - min qlo) s, exact likewise (one origin per node).  An inner slot's area goes to S_node,
// a leaf slot's to S_leaf; S_tri takes the leaf header's EXACT fp32 box -- the box the kernels test before the triangles -- times the
// header's count.  A root that is a leaf block: A_root = S_leaf = header area, S_node = 0, S_tri = header area x count.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FLX_TC_HD __host__ __device__ inline
#else
#define FLX_TC_HD inline
#endif

namespace flxtc {

enum { TC_A_ROOT = 0, TC_S_NODE = 1, TC_S_LEAF = 2, TC_S_TRI = 3, TC_SUMS = 4 };
#define FLX_TC_LEAF_BIT 0x80000000u        // FLX_LEAF_BIT and FLX_WIDE_LEAF_BIT
#define FLX_TC_WIDE_EMPTY 0x80000000u      // FLX_WIDE_EMPTY

FLX_TC_HD double tc_area_ext(double dx, double dy, double dz) { return 2.0 * ((dx * dy + dy * dz) + dz * dx); }
// the area of an fp32 box {mn, mx}; the differences are taken in fp64
FLX_TC_HD double tc_area(const float mn[3], const float mx[3])
{
    return tc_area_ext((double)mx[0] - (double)mn[0], (double)mx[1] - (double)mn[1], (double)mx[2] - (double)mn[2]);
}
FLX_TC_HD float tc_min(float a, float b) { return b < a ? b : a; }
FLX_TC_HD float tc_max(float a, float b) { return b > a ? b : a; }

// One BNode record as its sixteen words: lmin lmax rmin rmax left right pad pad.  counts[h]: the leaf count of half h when it is a leaf run (the
// caller reads it from the run's first TriRec), unused otherwise.  Adds to s[TC_S_NODE .. TC_S_TRI]; with `root`, sets s[TC_A_ROOT] too.
FLX_TC_HD void tc_binary_record(const float w[12], uint32_t left, uint32_t right, const uint32_t counts[2], bool root, double s[TC_SUMS])
{
    const uint32_t refs[2] = {left, right};
    for (int h = 0; h < 2; h++) {
        const double a = tc_area(w + 6 * h, w + 6 * h + 3);
        if (refs[h] & FLX_TC_LEAF_BIT) { s[TC_S_LEAF] += a; s[TC_S_TRI] += a * (double)counts[h]; }
        else s[TC_S_NODE] += a;
    }
    if (root) {
        float mn[3], mx[3];
        for (int k = 0; k < 3; k++) { mn[k] = tc_min(w[k], w[6 + k]); mx[k] = tc_max(w[3 + k], w[9 + k]); }
        const double a = tc_area(mn, mx);
        s[TC_A_ROOT] = a; s[TC_S_NODE] += a;
    }
}

// One WNode as its words: scale s[3], refs[4], planes qlo[3] / qhi[3] (byte k = slot k).  leafTri[k]: header area x count of slot k's leaf block when
// the slot is a leaf (the caller reads the header), unused otherwise.
FLX_TC_HD void tc_wide_node(const float sc[3], const uint32_t refs[4], const uint32_t qlo[3], const uint32_t qhi[3], const double leafTri[4], bool root,
                            double s[TC_SUMS])
{
    uint32_t lo[3] = {255u, 255u, 255u}, hi[3] = {0u, 0u, 0u};
    bool any = false;
    for (int k = 0; k < 4; k++) {
        if (refs[k] == FLX_TC_WIDE_EMPTY) continue;
        double d[3];
        for (int a = 0; a < 3; a++) {
            const uint32_t ql = (qlo[a] >> (8 * k)) & 255u, qh = (qhi[a] >> (8 * k)) & 255u;
            d[a] = (double)((int)qh - (int)ql) * (double)sc[a];
            lo[a] = ql < lo[a] ? ql : lo[a]; hi[a] = qh > hi[a] ? qh : hi[a];
        }
        const double a = tc_area_ext(d[0], d[1], d[2]);
        if (refs[k] & FLX_TC_LEAF_BIT) { s[TC_S_LEAF] += a; s[TC_S_TRI] += leafTri[k]; }
        else s[TC_S_NODE] += a;
        any = true;
    }
    if (root && any) {
        const double a = tc_area_ext((double)((int)hi[0] - (int)lo[0]) * (double)sc[0], (double)((int)hi[1] - (int)lo[1]) * (double)sc[1],
                                     (double)((int)hi[2] - (int)lo[2]) * (double)sc[2]);
        s[TC_A_ROOT] = a; s[TC_S_NODE] += a;
    }
}

// the leaf header {bmin.xyz, count} {bmax.xyz, 0} -> its exact box area x count
FLX_TC_HD double tc_leaf_header(const float h0[3], const float h1[3], uint32_t count) { return tc_area(h0, h1) * (double)count; }

} // namespace flxtc
