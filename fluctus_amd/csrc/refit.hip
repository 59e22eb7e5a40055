// refit.hip -- flx_update_triangles' kernels (and, below them, flx_update_triangles_subset's: the same passes, rewriting only what is dirty): validate the new triangles, rewrite the shading and the leaf triangle records, then refit the boxes
// of the binary and of the 4-wide tree bottom-up (flx_refit.h: what is computed and why the traversal kernels walk the result unchanged).
//
// SCHEDULE: level-synchronous.  flx_upload_scene lists the records of each depth (RefitTables: blevel / wlevel); the deepest level is launched
// first, one launch per level, so a record's children are complete when its thread runs (stream order): no atomics, no fences.  A pass is
// bandwidth-bound and the result is a pure function of the children, so a single kernel with arrival counters would compute the same bytes;
// only this schedule was built.
// Every record is written whole with 16-byte stores; the words a pass does not own (triangle index, leaf count, end-of-run flag, child refs) are
// carried over from the record it has just read.
#include "flx_launch.h"
#include "flx_wide.h"
#include "flx_refit.h"

namespace flxd {
using namespace flxrf;

static constexpr int RF_BLOCK = 256;
static inline uint32_t rf_grid(uint32_t n) { return (n + RF_BLOCK - 1) / RF_BLOCK; }

// a wire triangle is ten float4: v0 {p, n, t} v1 {p, n, t} v2 {p, n, t} {matId, pad}
enum { TRI_F4 = 10, TRI_P0 = 0, TRI_P1 = 3, TRI_P2 = 6, TRI_MAT = 9 };

// ---- validation: out[0] != 0 a non-finite position, out[1] bits of the largest |coordinate| (non-negative floats order as their bits),
// out[2] != 0 a matId outside [0, nmat)
__global__ __launch_bounds__(RF_BLOCK) void k_refit_validate(const float4 *__restrict__ src, uint32_t ntris, uint32_t nmat, uint32_t *__restrict__ out)
{
    __shared__ uint32_t sBad, sMax, sMat;
    if (threadIdx.x == 0) { sBad = 0; sMax = 0; sMat = 0; }
    __syncthreads();
    const uint32_t i = blockIdx.x * RF_BLOCK + threadIdx.x;
    if (i < ntris) {
        const float4 *t = src + (size_t)i * TRI_F4;
        const float4 a = t[TRI_P0], b = t[TRI_P1], c = t[TRI_P2];
        const float v[9] = {a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z};
        uint32_t bad = 0, mx = 0;
        for (int k = 0; k < 9; k++) {
            const uint32_t bits = __float_as_uint(v[k]) & 0x7FFFFFFFu;
            if (bits >= 0x7F800000u) bad = 1; else mx = bits > mx ? bits : mx;
        }
        const int m = __float_as_int(t[TRI_MAT].x);
        if (bad) atomicOr(&sBad, 1u);
        atomicMax(&sMax, mx);
        if (m < 0 || (uint32_t)m >= nmat) atomicOr(&sMat, 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (sBad) atomicOr(&out[0], 1u);
        atomicMax(&out[1], sMax);
        if (sMat) atomicOr(&out[2], 1u);
    }
}

// ---- shade pass: ShadeRec exactly as step 3 of flx_upload_scene lays it out, and the device copy of the wire triangles
__global__ __launch_bounds__(RF_BLOCK) void k_refit_shade(const float4 *__restrict__ src, uint32_t ntris, ShadeRec *__restrict__ shade, float4 *__restrict__ tris)
{
    const uint32_t i = blockIdx.x * RF_BLOCK + threadIdx.x;
    if (i >= ntris) return;
    float4 r[TRI_F4];
    for (int k = 0; k < TRI_F4; k++) r[k] = src[(size_t)i * TRI_F4 + k];
    ShadeRec s;
    s.a = make_float4(r[1].x, r[1].y, r[1].z, r[2].x);
    s.b = make_float4(r[4].x, r[4].y, r[4].z, r[2].y);
    s.c = make_float4(r[7].x, r[7].y, r[7].z, r[5].x);
    s.d = make_float4(r[5].y, r[8].x, r[8].y, r[TRI_MAT].x);
    shade[i] = s;
    for (int k = 0; k < TRI_F4; k++) tris[(size_t)i * TRI_F4 + k] = r[k];
}

// ---- gather pass: thread t < nidx rewrites index-list slot t of the binary tree's leaf runs, thread nidx + j the j-th triangle of the wide
// leaf blocks (wtriOff[j]: its first float4).  The triangle index is the record's own first .w word.
__global__ __launch_bounds__(RF_BLOCK) void k_refit_gather(const float4 *__restrict__ src, uint32_t ntris, TriRec *__restrict__ trirecs, uint32_t nidx,
                                                            float4 *__restrict__ wleaf, const uint32_t *__restrict__ wtriOff, uint32_t nwtri)
{
    const uint32_t t = blockIdx.x * RF_BLOCK + threadIdx.x;
    if (t >= nidx + nwtri) return;
    float4 *rec = t < nidx ? &trirecs[t].a : wleaf + wtriOff[t - nidx];
    const float4 a = rec[0], b = rec[1], c = rec[2];
    const uint32_t ti = __float_as_uint(a.w);
    if (ti >= ntris) return;                                   // (the upload checked every index; a record never written keeps its bytes)
    const float4 *p = src + (size_t)ti * TRI_F4;
    const float4 p0 = p[TRI_P0], p1 = p[TRI_P1], p2 = p[TRI_P2];
    rec[0] = make_float4(p0.x, p0.y, p0.z, a.w);
    rec[1] = make_float4(p1.x, p1.y, p1.z, b.w);
    rec[2] = make_float4(p2.x, p2.y, p2.z, c.w);
}

struct RfBox { float mn[3], mx[3]; };
__device__ __forceinline__ void rf_first(RfBox &b, const float4 &p) { b.mn[0] = b.mx[0] = p.x; b.mn[1] = b.mx[1] = p.y; b.mn[2] = b.mx[2] = p.z; }
__device__ __forceinline__ void rf_expand(RfBox &b, const float4 &p)
{
    b.mn[0] = rf_min(b.mn[0], p.x); b.mn[1] = rf_min(b.mn[1], p.y); b.mn[2] = rf_min(b.mn[2], p.z);
    b.mx[0] = rf_max(b.mx[0], p.x); b.mx[1] = rf_max(b.mx[1], p.y); b.mx[2] = rf_max(b.mx[2], p.z);
}
// exact fp32 union of the full bounds of `count` consecutive triangle records (three float4 each), in record order
__device__ __forceinline__ RfBox rf_leaf_box(const float4 *rec, uint32_t count)
{
    RfBox b; rf_first(b, rec[0]);
    for (uint32_t k = 0; k < count; k++) { if (k) rf_expand(b, rec[3 * k]); rf_expand(b, rec[3 * k + 1]); rf_expand(b, rec[3 * k + 2]); }
    return b;
}

// ---- wide leaf headers: one thread per leaf block
__global__ __launch_bounds__(RF_BLOCK) void k_refit_wide_leaves(float4 *__restrict__ wleaf, const uint32_t *__restrict__ wleafOff, uint32_t nleaves)
{
    const uint32_t i = blockIdx.x * RF_BLOCK + threadIdx.x;
    if (i >= nleaves) return;
    float4 *h = wleaf + wleafOff[i];
    const float4 h0 = h[0], h1 = h[1];
    const RfBox b = rf_leaf_box(h + 2, __float_as_uint(h0.w));
    h[0] = make_float4(b.mn[0], b.mn[1], b.mn[2], h0.w);
    h[1] = make_float4(b.mx[0], b.mx[1], b.mx[2], h1.w);
}

// ---- one level of the binary tree: both halves of each listed record from what hangs below them
__device__ __forceinline__ RfBox rf_binary_child(const BNode *bnodes, const TriRec *trirecs, uint32_t ref)
{
    if (ref & FLX_LEAF_BIT) {
        const float4 *rec = &trirecs[ref & ~FLX_LEAF_BIT].a;
        return rf_leaf_box(rec, __float_as_uint(rec[1].w));
    }
    const float4 *c = reinterpret_cast<const float4 *>(bnodes + ref);
    const float4 c0 = c[0], c1 = c[1], c2 = c[2];                           // lmin.xyz lmax.x | lmax.yz rmin.xy | rmin.z rmax.xyz
    RfBox b;
    b.mn[0] = rf_min(c0.x, c1.z); b.mn[1] = rf_min(c0.y, c1.w); b.mn[2] = rf_min(c0.z, c2.x);
    b.mx[0] = rf_max(c0.w, c2.y); b.mx[1] = rf_max(c1.x, c2.z); b.mx[2] = rf_max(c1.y, c2.w);
    return b;
}
__global__ __launch_bounds__(RF_BLOCK) void k_refit_binary_level(BNode *__restrict__ bnodes, const TriRec *__restrict__ trirecs, const uint32_t *__restrict__ list, uint32_t n)
{
    const uint32_t i = blockIdx.x * RF_BLOCK + threadIdx.x;
    if (i >= n) return;
    float4 *rec = reinterpret_cast<float4 *>(bnodes + list[i]);
    const float4 refs = rec[3];
    const uint32_t left = __float_as_uint(refs.x), right = __float_as_uint(refs.y);
    const RfBox L = rf_binary_child(bnodes, trirecs, left);
    const RfBox R = left == right ? L : rf_binary_child(bnodes, trirecs, right);     // (the synthetic root of a one-leaf scene)
    rec[0] = make_float4(L.mn[0], L.mn[1], L.mn[2], L.mx[0]);
    rec[1] = make_float4(L.mx[1], L.mx[2], R.mn[0], R.mn[1]);
    rec[2] = make_float4(R.mn[2], R.mx[0], R.mx[1], R.mx[2]);
    rec[3] = refs;
}

// ---- one level of the wide tree: the node's exact box (wexact: {min, max} per WNode) and its grid from the children's exact boxes
// (one WNode: r1, r2 are the words of the record that hold its child refs)
__device__ __forceinline__ void rf_wide_node(float4 *__restrict__ rec, const float4 &r1, const float4 &r2, const float4 *__restrict__ wleaf, float4 *__restrict__ wexact, uint32_t wi)
{
    const uint32_t refs[4] = {__float_as_uint(r1.z), __float_as_uint(r1.w), __float_as_uint(r2.x), __float_as_uint(r2.y)};
    float cmin[3][4], cmax[3][4];
    int ns = 0;                                                 // build_wide fills the slots from 0: the used ones come first
    for (int k = 0; k < 4; k++) {
        if (refs[k] == FLX_WIDE_EMPTY) continue;
        const float4 *b = (refs[k] & FLX_WIDE_LEAF_BIT) ? wleaf + (refs[k] & FLX_WIDE_OFF_MASK) : wexact + (size_t)refs[k] * 2;
        const float4 lo = b[0], hi = b[1];
        cmin[0][ns] = lo.x; cmin[1][ns] = lo.y; cmin[2][ns] = lo.z; cmax[0][ns] = hi.x; cmax[1][ns] = hi.y; cmax[2][ns] = hi.z;
        ns++;
    }
    if (ns == 0) return;
    float o[3], s[3], emn[3], emx[3]; uint32_t qlo[3], qhi[3];
    for (int a = 0; a < 3; a++) {
        rf_quantise_axis(cmin[a], cmax[a], ns, &o[a], &s[a], &qlo[a], &qhi[a]);
        emn[a] = o[a]; emx[a] = cmax[a][0];
        for (int k = 1; k < ns; k++) emx[a] = rf_max(emx[a], cmax[a][k]);
    }
    wexact[(size_t)wi * 2] = make_float4(emn[0], emn[1], emn[2], 0.0f);
    wexact[(size_t)wi * 2 + 1] = make_float4(emx[0], emx[1], emx[2], 0.0f);
    rec[0] = make_float4(o[0], o[1], o[2], s[0]);
    rec[1] = make_float4(s[1], s[2], r1.z, r1.w);
    rec[2] = make_float4(r2.x, r2.y, __uint_as_float(qlo[0]), __uint_as_float(qlo[1]));
    rec[3] = make_float4(__uint_as_float(qlo[2]), __uint_as_float(qhi[0]), __uint_as_float(qhi[1]), __uint_as_float(qhi[2]));
}
__global__ __launch_bounds__(RF_BLOCK) void k_refit_wide_level(float4 *__restrict__ wnodes, const float4 *__restrict__ wleaf, float4 *__restrict__ wexact,
                                                                const uint32_t *__restrict__ list, uint32_t n)
{
    const uint32_t i = blockIdx.x * RF_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t wi = list[i];
    float4 *rec = wnodes + (size_t)wi * 4;
    const float4 r1 = rec[1], r2 = rec[2];
    rf_wide_node(rec, r1, r2, wleaf, wexact, wi);
}

// =================================================================================================================================
// flx_update_triangles_subset: the same passes over the same level lists, but a record is rewritten only when something below
// it moved.  DIRTINESS travels upward through plain stores of the call's epoch into stamp arrays (RefitTables): the validation stamps the listed
// triangles, the leaf-header pass the wide leaf blocks holding one, each level pass the records it rewrites; a reader compares a stamp with the
// epoch.  The level-synchronous schedule orders every such store before its reader (stream order), so the passes need no atomics and no fences,
// and the result is a pure function of the previous arrays and the listed set.  Every record NOT rewritten keeps its bytes: no thread stores
// to it.  What a dirty record gets is computed by the very functions the full refit uses (rf_leaf_box, rf_binary_child, rf_wide_node).

// ---- validation, before anything a render or flx_tree_read can see is overwritten.  out[0] != 0 a non-finite position, out[1] bits of the largest
// |coordinate| of the listed triangles, out[2] != 0 a matId outside [0, nmat), out[3] bit 0 the list is not strictly ascending, bit 1 an index
// >= ntris.  Stamps the listed triangles: k_subset_rest_max then folds the STORED positions of all others into out[1], which makes it the
// maximum over the whole resulting set.  (The reductions use integer max / or on LDS and global words, as k_refit_validate does: their result does
// not depend on the order of arrival.  A refused call has spent its epoch; its stamps match no later call.)
__global__ __launch_bounds__(RF_BLOCK) void k_subset_validate(const float4 *__restrict__ src, const uint32_t *__restrict__ indices, uint32_t count, uint32_t ntris,
                                                               uint32_t nmat, uint32_t epoch, uint32_t *__restrict__ triStamp, uint32_t *__restrict__ out)
{
    __shared__ uint32_t sBad, sMax, sMat, sIdx;
    if (threadIdx.x == 0) { sBad = 0; sMax = 0; sMat = 0; sIdx = 0; }
    __syncthreads();
    const uint32_t k = blockIdx.x * RF_BLOCK + threadIdx.x;
    if (k < count) {
        const uint32_t ti = indices[k];
        uint32_t idxBad = (k && indices[k - 1] >= ti) ? 1u : 0u;
        if (ti >= ntris) idxBad |= 2u; else triStamp[ti] = epoch;
        const float4 *t = src + (size_t)k * TRI_F4;
        const float4 a = t[TRI_P0], b = t[TRI_P1], c = t[TRI_P2];
        const float v[9] = {a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z};
        uint32_t bad = 0, mx = 0;
        for (int j = 0; j < 9; j++) {
            const uint32_t bits = __float_as_uint(v[j]) & 0x7FFFFFFFu;
            if (bits >= 0x7F800000u) bad = 1; else mx = bits > mx ? bits : mx;
        }
        const int m = __float_as_int(t[TRI_MAT].x);
        if (bad) atomicOr(&sBad, 1u);
        atomicMax(&sMax, mx);
        if (m < 0 || (uint32_t)m >= nmat) atomicOr(&sMat, 1u);
        if (idxBad) atomicOr(&sIdx, idxBad);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (sBad) atomicOr(&out[0], 1u);
        atomicMax(&out[1], sMax);
        if (sMat) atomicOr(&out[2], 1u);
        if (sIdx) atomicOr(&out[3], sIdx);
    }
}
__global__ __launch_bounds__(RF_BLOCK) void k_subset_rest_max(const float4 *__restrict__ tris, uint32_t ntris, const uint32_t *__restrict__ triStamp, uint32_t epoch,
                                                               uint32_t *__restrict__ out)
{
    __shared__ uint32_t sMax;
    if (threadIdx.x == 0) sMax = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * RF_BLOCK + threadIdx.x;
    if (i < ntris && triStamp[i] != epoch) {
        const float4 *t = tris + (size_t)i * TRI_F4;
        const float4 a = t[TRI_P0], b = t[TRI_P1], c = t[TRI_P2];
        const float v[9] = {a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z};
        uint32_t mx = 0;
        for (int j = 0; j < 9; j++) { const uint32_t bits = __float_as_uint(v[j]) & 0x7FFFFFFFu; mx = bits > mx ? bits : mx; }     // (stored positions are finite)
        atomicMax(&sMax, mx);
    }
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(&out[1], sMax);
}

// ---- shade pass: one thread per listed triangle; ShadeRec and the device copy of the wire triangle exactly as k_refit_shade lays them out
__global__ __launch_bounds__(RF_BLOCK) void k_subset_shade(const float4 *__restrict__ src, const uint32_t *__restrict__ indices, uint32_t count, uint32_t ntris,
                                                            ShadeRec *__restrict__ shade, float4 *__restrict__ tris)
{
    const uint32_t k = blockIdx.x * RF_BLOCK + threadIdx.x;
    if (k >= count) return;
    const uint32_t i = indices[k];
    if (i >= ntris) return;                                    // (the validation has refused such a list)
    float4 r[TRI_F4];
    for (int j = 0; j < TRI_F4; j++) r[j] = src[(size_t)k * TRI_F4 + j];
    ShadeRec s;
    s.a = make_float4(r[1].x, r[1].y, r[1].z, r[2].x);
    s.b = make_float4(r[4].x, r[4].y, r[4].z, r[2].y);
    s.c = make_float4(r[7].x, r[7].y, r[7].z, r[5].x);
    s.d = make_float4(r[5].y, r[8].x, r[8].y, r[TRI_MAT].x);
    shade[i] = s;
    for (int j = 0; j < TRI_F4; j++) tris[(size_t)i * TRI_F4 + j] = r[j];
}

__device__ __forceinline__ bool rf_stamped(const uint32_t *__restrict__ triStamp, uint32_t ntris, uint32_t ti, uint32_t epoch) { return ti < ntris && triStamp[ti] == epoch; }
// does a run of `count` triangle records (three float4 each; the triangle index is the first .w word) hold a stamped triangle
__device__ __forceinline__ bool rf_run_stamped(const float4 *rec, uint32_t count, const uint32_t *__restrict__ triStamp, uint32_t ntris, uint32_t epoch)
{
    bool d = false;
    for (uint32_t k = 0; k < count; k++) d |= rf_stamped(triStamp, ntris, __float_as_uint(rec[3 * k].w), epoch);
    return d;
}

// ---- gather pass, threads as in k_refit_gather; a slot is rewritten -- from the device copy of the wire triangles, which the shade pass has
// brought up to date -- only when its triangle carries this call's stamp (the dependent read: record .w -> stamp -> triangle)
__global__ __launch_bounds__(RF_BLOCK) void k_subset_gather(const float4 *__restrict__ tris, uint32_t ntris, const uint32_t *__restrict__ triStamp, uint32_t epoch,
                                                             TriRec *__restrict__ trirecs, uint32_t nidx, float4 *__restrict__ wleaf, const uint32_t *__restrict__ wtriOff, uint32_t nwtri)
{
    const uint32_t t = blockIdx.x * RF_BLOCK + threadIdx.x;
    if (t >= nidx + nwtri) return;
    float4 *rec = t < nidx ? &trirecs[t].a : wleaf + wtriOff[t - nidx];
    const float4 a = rec[0];
    const uint32_t ti = __float_as_uint(a.w);
    if (!rf_stamped(triStamp, ntris, ti, epoch)) return;
    const float4 b = rec[1], c = rec[2];
    const float4 *p = tris + (size_t)ti * TRI_F4;
    const float4 p0 = p[TRI_P0], p1 = p[TRI_P1], p2 = p[TRI_P2];
    rec[0] = make_float4(p0.x, p0.y, p0.z, a.w);
    rec[1] = make_float4(p1.x, p1.y, p1.z, b.w);
    rec[2] = make_float4(p2.x, p2.y, p2.z, c.w);
}

// ---- wide leaf headers: one thread per leaf block; a block holding a stamped triangle gets the exact union of its triangles and its stamp
__global__ __launch_bounds__(RF_BLOCK) void k_subset_wide_leaves(float4 *__restrict__ wleaf, const uint32_t *__restrict__ wleafOff, uint32_t nleaves,
                                                                  const uint32_t *__restrict__ triStamp, uint32_t ntris, uint32_t epoch, uint32_t *__restrict__ lStamp)
{
    const uint32_t i = blockIdx.x * RF_BLOCK + threadIdx.x;
    if (i >= nleaves) return;
    const uint32_t off = wleafOff[i];
    float4 *h = wleaf + off;
    const float4 h0 = h[0];
    const uint32_t cnt = __float_as_uint(h0.w);
    if (!rf_run_stamped(h + 2, cnt, triStamp, ntris, epoch)) return;
    const float4 h1 = h[1];
    const RfBox b = rf_leaf_box(h + 2, cnt);
    h[0] = make_float4(b.mn[0], b.mn[1], b.mn[2], h0.w);
    h[1] = make_float4(b.mx[0], b.mx[1], b.mx[2], h1.w);
    lStamp[off] = epoch;
}

// ---- one level of the binary tree: a half is dirty when its leaf run holds a stamped triangle, or its inner child's record carries this call's
// stamp; a dirty half is recomputed as rf_binary_child does, a clean half keeps the bits it has, a record with a dirty half is written whole
__device__ __forceinline__ bool rf_binary_dirty(const TriRec *trirecs, uint32_t ref, const uint32_t *__restrict__ triStamp, uint32_t ntris, const uint32_t *__restrict__ bStamp, uint32_t epoch)
{
    if (!(ref & FLX_LEAF_BIT)) return bStamp[ref] == epoch;
    const float4 *rec = &trirecs[ref & ~FLX_LEAF_BIT].a;
    return rf_run_stamped(rec, __float_as_uint(rec[1].w), triStamp, ntris, epoch);
}
__global__ __launch_bounds__(RF_BLOCK) void k_subset_binary_level(BNode *__restrict__ bnodes, const TriRec *__restrict__ trirecs, const uint32_t *__restrict__ list, uint32_t n,
                                                                   const uint32_t *__restrict__ triStamp, uint32_t ntris, uint32_t *__restrict__ bStamp, uint32_t epoch)
{
    const uint32_t i = blockIdx.x * RF_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t ri = list[i];
    float4 *rec = reinterpret_cast<float4 *>(bnodes + ri);
    const float4 refs = rec[3];
    const uint32_t left = __float_as_uint(refs.x), right = __float_as_uint(refs.y);
    const bool dl = rf_binary_dirty(trirecs, left, triStamp, ntris, bStamp, epoch);
    const bool dr = left == right ? dl : rf_binary_dirty(trirecs, right, triStamp, ntris, bStamp, epoch);
    if (!dl && !dr) return;
    const float4 c0 = rec[0], c1 = rec[1], c2 = rec[2];                    // lmin.xyz lmax.x | lmax.yz rmin.xy | rmin.z rmax.xyz
    RfBox L, R;
    if (dl) L = rf_binary_child(bnodes, trirecs, left);
    else { L.mn[0] = c0.x; L.mn[1] = c0.y; L.mn[2] = c0.z; L.mx[0] = c0.w; L.mx[1] = c1.x; L.mx[2] = c1.y; }
    if (left == right) R = L;                                              // (the synthetic root of a one-leaf scene)
    else if (dr) R = rf_binary_child(bnodes, trirecs, right);
    else { R.mn[0] = c1.z; R.mn[1] = c1.w; R.mn[2] = c2.x; R.mx[0] = c2.y; R.mx[1] = c2.z; R.mx[2] = c2.w; }
    rec[0] = make_float4(L.mn[0], L.mn[1], L.mn[2], L.mx[0]);
    rec[1] = make_float4(L.mx[1], L.mx[2], R.mn[0], R.mn[1]);
    rec[2] = make_float4(R.mn[2], R.mx[0], R.mx[1], R.mx[2]);
    rec[3] = refs;
    bStamp[ri] = epoch;
}

// ---- one level of the wide tree: a WNode with a dirty child -- a stamped leaf block or a stamped WNode -- recomputes its exact box and its grid
// from ALL its children's exact boxes (clean children: the stored wexact / leaf header); every other WNode and its wexact entry is not written
__global__ __launch_bounds__(RF_BLOCK) void k_subset_wide_level(float4 *__restrict__ wnodes, const float4 *__restrict__ wleaf, float4 *__restrict__ wexact,
                                                                 const uint32_t *__restrict__ list, uint32_t n, const uint32_t *__restrict__ lStamp, uint32_t *__restrict__ wStamp, uint32_t epoch)
{
    const uint32_t i = blockIdx.x * RF_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t wi = list[i];
    float4 *rec = wnodes + (size_t)wi * 4;
    const float4 r1 = rec[1], r2 = rec[2];
    const uint32_t refs[4] = {__float_as_uint(r1.z), __float_as_uint(r1.w), __float_as_uint(r2.x), __float_as_uint(r2.y)};
    bool dirty = false;
    for (int k = 0; k < 4; k++) {
        if (refs[k] == FLX_WIDE_EMPTY) continue;
        dirty |= ((refs[k] & FLX_WIDE_LEAF_BIT) ? lStamp[refs[k] & FLX_WIDE_OFF_MASK] : wStamp[refs[k]]) == epoch;
    }
    if (!dirty) return;
    rf_wide_node(rec, r1, r2, wleaf, wexact, wi);
    wStamp[wi] = epoch;
}

// ---- launchers (flx_launch.h)
void launch_refit_validate(hipStream_t s, const void *src, uint32_t ntris, uint32_t nmat, uint32_t *out3)
{
    k_refit_validate<<<rf_grid(ntris), RF_BLOCK, 0, s>>>((const float4 *)src, ntris, nmat, out3);
}
void launch_refit(hipStream_t s, const void *src, const Scene &sc, const RefitTables &rt)
{
    const float4 *p = (const float4 *)src;
    k_refit_shade<<<rf_grid(rt.ntris), RF_BLOCK, 0, s>>>(p, rt.ntris, const_cast<ShadeRec *>(sc.shade), reinterpret_cast<float4 *>(const_cast<flx_triangle *>(sc.tris)));
    TriRec *trirecs = const_cast<TriRec *>(sc.trirecs);
    float4 *wleaf = const_cast<float4 *>(sc.wleaf);
    k_refit_gather<<<rf_grid(rt.nidx + rt.nwtri), RF_BLOCK, 0, s>>>(p, rt.ntris, trirecs, rt.nidx, wleaf, rt.wtriOff, rt.nwtri);
    if (rt.nwleaf) k_refit_wide_leaves<<<rf_grid(rt.nwleaf), RF_BLOCK, 0, s>>>(wleaf, rt.wleafOff, rt.nwleaf);
    BNode *bnodes = const_cast<BNode *>(sc.bnodes);
    for (size_t l = rt.blevelStart.empty() ? 0 : rt.blevelStart.size() - 1; l-- > 0;) {
        const uint32_t a = rt.blevelStart[l], n = rt.blevelStart[l + 1] - a;
        if (n) k_refit_binary_level<<<rf_grid(n), RF_BLOCK, 0, s>>>(bnodes, trirecs, rt.blevel + a, n);
    }
    float4 *wnodes = reinterpret_cast<float4 *>(const_cast<void *>(sc.wnodes));
    for (size_t l = rt.wlevelStart.empty() ? 0 : rt.wlevelStart.size() - 1; l-- > 0;) {
        const uint32_t a = rt.wlevelStart[l], n = rt.wlevelStart[l + 1] - a;
        if (n) k_refit_wide_level<<<rf_grid(n), RF_BLOCK, 0, s>>>(wnodes, wleaf, rt.wexact, rt.wlevel + a, n);
    }
}

void launch_refit_subset_validate(hipStream_t s, const void *src, const uint32_t *indices, uint32_t count, const Scene &sc, const RefitTables &rt, uint32_t *out4)
{
    if (count) k_subset_validate<<<rf_grid(count), RF_BLOCK, 0, s>>>((const float4 *)src, indices, count, rt.ntris, rt.nmat, rt.epoch, rt.triStamp, out4);
    k_subset_rest_max<<<rf_grid(rt.ntris), RF_BLOCK, 0, s>>>(reinterpret_cast<const float4 *>(sc.tris), rt.ntris, rt.triStamp, rt.epoch, out4);
}
void launch_refit_subset(hipStream_t s, const void *src, const uint32_t *indices, uint32_t count, const Scene &sc, const RefitTables &rt)
{
    if (!count) return;
    const uint32_t e = rt.epoch;
    float4 *tris = reinterpret_cast<float4 *>(const_cast<flx_triangle *>(sc.tris));
    k_subset_shade<<<rf_grid(count), RF_BLOCK, 0, s>>>((const float4 *)src, indices, count, rt.ntris, const_cast<ShadeRec *>(sc.shade), tris);
    TriRec *trirecs = const_cast<TriRec *>(sc.trirecs);
    float4 *wleaf = const_cast<float4 *>(sc.wleaf);
    k_subset_gather<<<rf_grid(rt.nidx + rt.nwtri), RF_BLOCK, 0, s>>>(tris, rt.ntris, rt.triStamp, e, trirecs, rt.nidx, wleaf, rt.wtriOff, rt.nwtri);
    if (rt.nwleaf) k_subset_wide_leaves<<<rf_grid(rt.nwleaf), RF_BLOCK, 0, s>>>(wleaf, rt.wleafOff, rt.nwleaf, rt.triStamp, rt.ntris, e, rt.lStamp);
    BNode *bnodes = const_cast<BNode *>(sc.bnodes);
    for (size_t l = rt.blevelStart.empty() ? 0 : rt.blevelStart.size() - 1; l-- > 0;) {
        const uint32_t a = rt.blevelStart[l], n = rt.blevelStart[l + 1] - a;
        if (n) k_subset_binary_level<<<rf_grid(n), RF_BLOCK, 0, s>>>(bnodes, trirecs, rt.blevel + a, n, rt.triStamp, rt.ntris, rt.bStamp, e);
    }
    float4 *wnodes = reinterpret_cast<float4 *>(const_cast<void *>(sc.wnodes));
    for (size_t l = rt.wlevelStart.empty() ? 0 : rt.wlevelStart.size() - 1; l-- > 0;) {
        const uint32_t a = rt.wlevelStart[l], n = rt.wlevelStart[l + 1] - a;
        if (n) k_subset_wide_level<<<rf_grid(n), RF_BLOCK, 0, s>>>(wnodes, wleaf, rt.wexact, rt.wlevel + a, n, rt.lStamp, rt.wStamp, e);
    }
}

} // namespace flxd
