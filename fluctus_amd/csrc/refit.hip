// refit.hip -- the kernels of flx_update_triangles and flx_update_triangles_subset: validate the new triangles, rewrite the shading and the leaf
// triangle records, then refit the boxes of the binary and of the 4-wide tree bottom-up (flx_refit.h: what is computed and why the traversal
// kernels walk the result unchanged).  ONE set of passes in two modes, a compile-time switch: SUBSET == false rewrites every record (a full refit
// is a subset refit in which everything is dirty: no stamp is read or written), SUBSET == true only the records with something moved below them.
//
// SCHEDULE: level-synchronous.  flx_upload_scene lists the records of each depth (RefitTables: blevel / wlevel); the deepest level is launched
// first, one launch per level, so a record's children are complete when its thread runs (stream order): no atomics, no fences.  A pass is
// bandwidth-bound and the result is a pure function of the children, so a single kernel with arrival counters would compute the same bytes;
// only this schedule was built.
// Every record is written whole with 16-byte stores; the words a pass does not own (triangle index, leaf count, end-of-run flag, child refs) are
// carried over from the record it has just read.
//
// SUBSET: DIRTINESS travels upward through plain stores of the call's epoch into stamp arrays (RefitTables): the validation
// stamps the listed triangles, the leaf-header pass the wide leaf blocks holding one, each level pass the records it rewrites; a reader compares a
// stamp with the epoch.  The schedule orders every such store before its reader (stream order), so the passes need no atomics and no fences, and
// the result is a pure function of the previous arrays and the listed set.  Every record NOT rewritten keeps its bytes: no thread stores to it.
#include "flx_launch.h"
#include "flx_wide.h"
#include "flx_refit.h"

namespace flxd {
using namespace flxrf;

static constexpr int RF_BLOCK = 256;
static inline uint32_t rf_grid(uint32_t n) { return (n + RF_BLOCK - 1) / RF_BLOCK; }

// a wire triangle is ten float4: v0 {p, n, t} v1 {p, n, t} v2 {p, n, t} {matId, pad}
enum { TRI_F4 = 10, TRI_P0 = 0, TRI_P1 = 3, TRI_P2 = 6, TRI_MAT = 9 };

// what the SUBSET passes know of a call (RefitTables); the other mode's kernels take one too and never look at it
struct Stamps { uint32_t *__restrict__ tri, *__restrict__ b, *__restrict__ w, *__restrict__ l; uint32_t epoch; };

// ---- validation, before anything a render or flx_tree_read can see is overwritten.  out[0] != 0 a non-finite position, out[1] bits of the largest
// |coordinate| (non-negative floats order as their bits), out[2] != 0 a matId outside [0, nmat), out[3] (SUBSET) bit 0 the list is not strictly
// ascending, bit 1 an index >= ntris.
// one triangle's share of out[0..2]; `stored`: a triangle an earlier call has accepted -- finite, matId in range -- so only v[1] is computed
__device__ __forceinline__ void rf_scan(const float4 *__restrict__ t, uint32_t nmat, uint32_t v[4], bool stored = false)
{
    const float4 a = t[TRI_P0], b = t[TRI_P1], c = t[TRI_P2];
    const float p[9] = {a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z};
    v[0] = v[1] = 0;
    for (int k = 0; k < 9; k++) {
        const uint32_t bits = __float_as_uint(p[k]) & 0x7FFFFFFFu;
        if (!stored && bits >= 0x7F800000u) v[0] = 1; else v[1] = bits > v[1] ? bits : v[1];
    }
    if (stored) return;
    const int m = __float_as_int(t[TRI_MAT].x);
    v[2] = (m < 0 || (uint32_t)m >= nmat) ? 1u : 0u;
}
// The block's reduction into out[]: between the two barriers every thread lets `scan` fill its v (false: it has none), and the words WORDS names
// are folded, word 1 by max, the others by or.  Integer max / or on LDS and global words: the result does not depend on the order of arrival.
template <uint32_t WORDS, class F> __device__ __forceinline__ void rf_reduce(uint32_t *__restrict__ out, F scan)
{
    __shared__ uint32_t s[4];
    if (threadIdx.x == 0)
        for (int w = 0; w < 4; w++) if (WORDS >> w & 1u) s[w] = 0;
    __syncthreads();
    uint32_t v[4] = {0, 0, 0, 0};
    if (scan(v))
        for (int w = 0; w < 4; w++) {
            if (!(WORDS >> w & 1u)) continue;
            if (w == 1) atomicMax(&s[1], v[1]); else if (v[w]) atomicOr(&s[w], v[w]);
        }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 0; w < 4; w++) {
            if (!(WORDS >> w & 1u)) continue;
            if (w == 1) atomicMax(&out[1], s[1]); else if (s[w]) atomicOr(&out[w], s[w]);
        }
}
// Thread k scans source triangle k.  SUBSET: it is triangle indices[k]; the list is checked and the listed triangles are stamped, and
// k_subset_rest_max then folds the STORED positions of all others into out[1], which makes it the maximum over the whole resulting set.  (A refused
// call has spent its epoch; its stamps match no later call.)
template <bool SUBSET> __global__ __launch_bounds__(RF_BLOCK) void k_refit_validate(const float4 *__restrict__ src, const uint32_t *__restrict__ indices, uint32_t count, uint32_t ntris,
                                                                                     uint32_t nmat, Stamps st, uint32_t *__restrict__ out)
{
    rf_reduce<SUBSET ? 15u : 7u>(out, [&](uint32_t v[4]) {
        const uint32_t k = blockIdx.x * RF_BLOCK + threadIdx.x;
        if (k >= count) return false;
        if constexpr (SUBSET) {
            const uint32_t ti = indices[k];
            v[3] = (k && indices[k - 1] >= ti) ? 1u : 0u;
            if (ti >= ntris) v[3] |= 2u; else st.tri[ti] = st.epoch;
        }
        rf_scan(src + (size_t)k * TRI_F4, nmat, v);
        return true;
    });
}
__global__ __launch_bounds__(RF_BLOCK) void k_subset_rest_max(const float4 *__restrict__ tris, uint32_t ntris, const uint32_t *__restrict__ triStamp, uint32_t epoch,
                                                               uint32_t *__restrict__ out)
{
    rf_reduce<2u>(out, [&](uint32_t v[4]) {
        const uint32_t i = blockIdx.x * RF_BLOCK + threadIdx.x;
        if (i >= ntris || triStamp[i] == epoch) return false;
        rf_scan(tris + (size_t)i * TRI_F4, 0, v, true);
        return true;
    });
}

// ---- shade pass: thread k writes source triangle k's ShadeRec, exactly as step 3 of flx_upload_scene lays it out (rf_shade_rec), and its slot of
// the device copy of the wire triangles.  SUBSET: it is triangle indices[k].
template <bool SUBSET> __global__ __launch_bounds__(RF_BLOCK) void k_refit_shade(const float4 *__restrict__ src, const uint32_t *__restrict__ indices, uint32_t count, uint32_t ntris,
                                                                                  ShadeRec *__restrict__ shade, float4 *__restrict__ tris)
{
    const uint32_t k = blockIdx.x * RF_BLOCK + threadIdx.x;
    if (k >= count) return;
    uint32_t i = k;
    if constexpr (SUBSET) {
        i = indices[k];
        if (i >= ntris) return;                                // (the validation has refused such a list)
    }
    float4 r[TRI_F4];
    for (int j = 0; j < TRI_F4; j++) r[j] = src[(size_t)k * TRI_F4 + j];
    ShadeRec s;
    rf_shade_rec(r, s.a, s.b, s.c, s.d);
    shade[i] = s;
    for (int j = 0; j < TRI_F4; j++) tris[(size_t)i * TRI_F4 + j] = r[j];
}

// is triangle ti one this call moves: every triangle of the scene, SUBSET: those carrying the call's stamp
template <bool SUBSET> __device__ __forceinline__ bool rf_moved(const Stamps &st, uint32_t ntris, uint32_t ti)
{
    if constexpr (SUBSET) return ti < ntris && st.tri[ti] == st.epoch;
    return ti < ntris;
}
// does a run of `count` triangle records (three float4 each; the triangle index is the first .w word) hold a stamped triangle
__device__ __forceinline__ bool rf_run_stamped(const float4 *rec, uint32_t count, const Stamps &st, uint32_t ntris)
{
    bool d = false;
    for (uint32_t k = 0; k < count; k++) d |= rf_moved<true>(st, ntris, __float_as_uint(rec[3 * k].w));
    return d;
}

// ---- gather pass: thread t < nidx rewrites index-list slot t of the binary tree's leaf runs, thread nidx + j the j-th triangle of the wide
// leaf blocks (wtriOff[j]: its first float4), from the wire triangles at pos.  The triangle index is the record's own first .w word; the three .w
// words are carried over.  SUBSET: pos is the device copy, which the shade pass has brought up to date, and a slot is rewritten only when its
// triangle carries this call's stamp (the dependent read: record .w -> stamp -> triangle).
template <bool SUBSET> __global__ __launch_bounds__(RF_BLOCK) void k_refit_gather(const float4 *__restrict__ pos, uint32_t ntris, Stamps st, TriRec *__restrict__ trirecs, uint32_t nidx,
                                                                                   float4 *__restrict__ wleaf, const uint32_t *__restrict__ wtriOff, uint32_t nwtri)
{
    const uint32_t t = blockIdx.x * RF_BLOCK + threadIdx.x;
    if (t >= nidx + nwtri) return;
    float4 *rec = t < nidx ? &trirecs[t].a : wleaf + wtriOff[t - nidx];
    const float4 a = rec[0];
    const uint32_t ti = __float_as_uint(a.w);
    if (!rf_moved<SUBSET>(st, ntris, ti)) return;              // (the upload checked every index; a record never written keeps its bytes)
    const float4 b = rec[1], c = rec[2];
    const float4 *p = pos + (size_t)ti * TRI_F4;
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

// ---- wide leaf headers: one thread per leaf block writes the exact union of its triangles.  SUBSET: only into a block holding a stamped
// triangle, which gets its stamp.
template <bool SUBSET> __global__ __launch_bounds__(RF_BLOCK) void k_refit_wide_leaves(float4 *__restrict__ wleaf, const uint32_t *__restrict__ wleafOff, uint32_t nleaves, Stamps st, uint32_t ntris)
{
    const uint32_t i = blockIdx.x * RF_BLOCK + threadIdx.x;
    if (i >= nleaves) return;
    const uint32_t off = wleafOff[i];
    float4 *h = wleaf + off;
    const float4 h0 = h[0];
    const uint32_t cnt = __float_as_uint(h0.w);
    if constexpr (SUBSET) if (!rf_run_stamped(h + 2, cnt, st, ntris)) return;
    const float4 h1 = h[1];
    const RfBox b = rf_leaf_box(h + 2, cnt);
    h[0] = make_float4(b.mn[0], b.mn[1], b.mn[2], h0.w);
    h[1] = make_float4(b.mx[0], b.mx[1], b.mx[2], h1.w);
    if constexpr (SUBSET) st.l[off] = st.epoch;
}

// ---- one level of the binary tree: both halves of each listed record from what hangs below them.  SUBSET: a half is dirty when its leaf run holds
// a stamped triangle, or its inner child's record carries this call's stamp; a dirty half is recomputed, a clean half keeps the bits it has, a
// record with a dirty half is written whole and stamped.
// (a BNode record's first three float4 <-> its two halves: lmin.xyz lmax.x | lmax.yz rmin.xy | rmin.z rmax.xyz)
__device__ __forceinline__ void rf_halves(const float4 *rec, RfBox &L, RfBox &R)
{
    const float4 c0 = rec[0], c1 = rec[1], c2 = rec[2];
    L.mn[0] = c0.x; L.mn[1] = c0.y; L.mn[2] = c0.z; L.mx[0] = c0.w; L.mx[1] = c1.x; L.mx[2] = c1.y;
    R.mn[0] = c1.z; R.mn[1] = c1.w; R.mn[2] = c2.x; R.mx[0] = c2.y; R.mx[1] = c2.z; R.mx[2] = c2.w;
}
__device__ __forceinline__ void rf_put_halves(float4 *rec, const RfBox &L, const RfBox &R)
{
    rec[0] = make_float4(L.mn[0], L.mn[1], L.mn[2], L.mx[0]);
    rec[1] = make_float4(L.mx[1], L.mx[2], R.mn[0], R.mn[1]);
    rec[2] = make_float4(R.mn[2], R.mx[0], R.mx[1], R.mx[2]);
}
__device__ __forceinline__ RfBox rf_binary_child(const BNode *bnodes, const TriRec *trirecs, uint32_t ref)
{
    if (ref & FLX_LEAF_BIT) {
        const float4 *rec = &trirecs[ref & ~FLX_LEAF_BIT].a;
        return rf_leaf_box(rec, __float_as_uint(rec[1].w));
    }
    RfBox L, R, b;
    rf_halves(reinterpret_cast<const float4 *>(bnodes + ref), L, R);
    for (int k = 0; k < 3; k++) { b.mn[k] = rf_min(L.mn[k], R.mn[k]); b.mx[k] = rf_max(L.mx[k], R.mx[k]); }     // left first
    return b;
}
__device__ __forceinline__ bool rf_binary_dirty(const TriRec *trirecs, uint32_t ref, const Stamps &st, uint32_t ntris)
{
    if (!(ref & FLX_LEAF_BIT)) return st.b[ref] == st.epoch;
    const float4 *rec = &trirecs[ref & ~FLX_LEAF_BIT].a;
    return rf_run_stamped(rec, __float_as_uint(rec[1].w), st, ntris);
}
template <bool SUBSET> __global__ __launch_bounds__(RF_BLOCK) void k_refit_binary_level(BNode *__restrict__ bnodes, const TriRec *__restrict__ trirecs, const uint32_t *__restrict__ list, uint32_t n,
                                                                                         Stamps st, uint32_t ntris)
{
    const uint32_t i = blockIdx.x * RF_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t ri = list[i];
    float4 *rec = reinterpret_cast<float4 *>(bnodes + ri);
    const float4 refs = rec[3];
    const uint32_t left = __float_as_uint(refs.x), right = __float_as_uint(refs.y);
    bool dl = true, dr = true;
    RfBox L, R;
    if constexpr (SUBSET) {
        dl = rf_binary_dirty(trirecs, left, st, ntris);
        dr = left == right ? dl : rf_binary_dirty(trirecs, right, st, ntris);
        if (!dl && !dr) return;
        rf_halves(rec, L, R);
    }
    if (dl) L = rf_binary_child(bnodes, trirecs, left);
    if (left == right) R = L;                                              // (the synthetic root of a one-leaf scene)
    else if (dr) R = rf_binary_child(bnodes, trirecs, right);
    rf_put_halves(rec, L, R);
    rec[3] = refs;
    if constexpr (SUBSET) st.b[ri] = st.epoch;
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
// SUBSET: only a WNode with a dirty child -- a stamped leaf block or a stamped WNode -- recomputes its exact box and its grid, from ALL its
// children's exact boxes (clean children: the stored wexact / leaf header), and gets its stamp; every other WNode and its wexact entry is not written
template <bool SUBSET> __global__ __launch_bounds__(RF_BLOCK) void k_refit_wide_level(float4 *__restrict__ wnodes, const float4 *__restrict__ wleaf, float4 *__restrict__ wexact,
                                                                                       const uint32_t *__restrict__ list, uint32_t n, Stamps st)
{
    const uint32_t i = blockIdx.x * RF_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t wi = list[i];
    float4 *rec = wnodes + (size_t)wi * 4;
    const float4 r1 = rec[1], r2 = rec[2];
    if constexpr (SUBSET) {
        const uint32_t refs[4] = {__float_as_uint(r1.z), __float_as_uint(r1.w), __float_as_uint(r2.x), __float_as_uint(r2.y)};
        bool dirty = false;
        for (int k = 0; k < 4; k++) {
            if (refs[k] == FLX_WIDE_EMPTY) continue;
            dirty |= ((refs[k] & FLX_WIDE_LEAF_BIT) ? st.l[refs[k] & FLX_WIDE_OFF_MASK] : st.w[refs[k]]) == st.epoch;
        }
        if (!dirty) return;
    }
    rf_wide_node(rec, r1, r2, wleaf, wexact, wi);
    if constexpr (SUBSET) st.w[wi] = st.epoch;
}

// ---- launchers (flx_launch.h): a null index list means every triangle, and src then holds all rt.ntris of them
static Stamps rf_stamps(const RefitTables &rt) { return Stamps{rt.triStamp, rt.bStamp, rt.wStamp, rt.lStamp, rt.epoch}; }
void launch_refit_validate(hipStream_t s, const void *src, const uint32_t *indices, uint32_t count, const Scene &sc, const RefitTables &rt, uint32_t *out4)
{
    const float4 *p = (const float4 *)src;
    if (!indices) { k_refit_validate<false><<<rf_grid(rt.ntris), RF_BLOCK, 0, s>>>(p, nullptr, rt.ntris, rt.ntris, rt.nmat, Stamps{}, out4); return; }
    if (count) k_refit_validate<true><<<rf_grid(count), RF_BLOCK, 0, s>>>(p, indices, count, rt.ntris, rt.nmat, rf_stamps(rt), out4);
    k_subset_rest_max<<<rf_grid(rt.ntris), RF_BLOCK, 0, s>>>(reinterpret_cast<const float4 *>(sc.tris), rt.ntris, rt.triStamp, rt.epoch, out4);
}
// the lists of one tree, deepest level first: f(first entry, entries)
template <class F> static void rf_levels(const std::vector<uint32_t> &start, F f)
{
    for (size_t l = start.empty() ? 0 : start.size() - 1; l-- > 0;)
        if (start[l + 1] > start[l]) f(start[l], start[l + 1] - start[l]);
}
template <bool SUBSET> static void rf_passes(hipStream_t s, const float4 *src, const uint32_t *indices, uint32_t count, const Scene &sc, const RefitTables &rt)
{
    const Stamps st = SUBSET ? rf_stamps(rt) : Stamps{};
    float4 *tris = reinterpret_cast<float4 *>(const_cast<flx_triangle *>(sc.tris));
    k_refit_shade<SUBSET><<<rf_grid(count), RF_BLOCK, 0, s>>>(src, indices, count, rt.ntris, const_cast<ShadeRec *>(sc.shade), tris);
    TriRec *trirecs = const_cast<TriRec *>(sc.trirecs);
    float4 *wleaf = const_cast<float4 *>(sc.wleaf);
    k_refit_gather<SUBSET><<<rf_grid(rt.nidx + rt.nwtri), RF_BLOCK, 0, s>>>(SUBSET ? tris : src, rt.ntris, st, trirecs, rt.nidx, wleaf, rt.wtriOff, rt.nwtri);
    if (rt.nwleaf) k_refit_wide_leaves<SUBSET><<<rf_grid(rt.nwleaf), RF_BLOCK, 0, s>>>(wleaf, rt.wleafOff, rt.nwleaf, st, rt.ntris);
    BNode *bnodes = const_cast<BNode *>(sc.bnodes);
    rf_levels(rt.blevelStart, [&](uint32_t a, uint32_t n) { k_refit_binary_level<SUBSET><<<rf_grid(n), RF_BLOCK, 0, s>>>(bnodes, trirecs, rt.blevel + a, n, st, rt.ntris); });
    float4 *wnodes = reinterpret_cast<float4 *>(const_cast<void *>(sc.wnodes));
    rf_levels(rt.wlevelStart, [&](uint32_t a, uint32_t n) { k_refit_wide_level<SUBSET><<<rf_grid(n), RF_BLOCK, 0, s>>>(wnodes, wleaf, rt.wexact, rt.wlevel + a, n, st); });
}
void launch_refit(hipStream_t s, const void *src, const uint32_t *indices, uint32_t count, const Scene &sc, const RefitTables &rt)
{
    if (!indices) rf_passes<false>(s, (const float4 *)src, nullptr, rt.ntris, sc, rt);
    else if (count) rf_passes<true>(s, (const float4 *)src, indices, count, sc, rt);
}

} // namespace flxd
