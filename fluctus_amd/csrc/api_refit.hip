// api_refit.hip -- flx_update_triangles and flx_update_triangles_subset: the uploaded scene's triangles (or a listed subset of them) move, both traversal trees are refitted on the device over the topology
// flx_upload_scene built (kernels: refit.hip; arithmetic and the exactness argument: flx_refit.h), and its test hook
// flx_tree_read, and flx_tree_cost (kernels: tree_cost.hip; what is summed: flx_tree_cost.h): how far the refits have degraded
// the trees.  Validation runs on the device BEFORE anything is overwritten, so a refused call leaves the old scene as it was.
#include "flx_ctx.h"
#include "flx_wide.h"
#include "flx_trace4.h"
#include <cstring>

namespace flxd {
float wideClampFor(float maxAbsCoord) { return maxAbsCoord < 67108864.0f ? FLX_WIDE_DINV_MAX : FLX_WIDE_DINV_FAR; }
int wideFar(const flx_ctx *c) { return c->sc.wideClamp == FLX_WIDE_DINV_FAR ? 1 : 0; }
}

// The boundary of both calls, written once.  flx_update_triangles: every triangle, count must be the scene's.  flx_update_triangles_subset
// (`subset`): the source is a list, validation also checks the list and reduces the maximum |coordinate| over the unmoved triangles' stored
// positions (the clamp is that of the WHOLE resulting set, never a running maximum), and the passes rewrite only what is dirty (refit.hip: one
// set of passes, two modes).  Every message carries the name of the call it refuses.
static int updateTriangles(flx_ctx *c, bool subset, const void *tris160, const uint32_t *indices, size_t count, int src_on_device)
{
    const std::string fn = subset ? "flx_update_triangles_subset: " : "flx_update_triangles: ";
    ENTER(c, CALL_OBSERVE);                               // deferred and fused launches run against the OLD scene
    NEED(c, c->sc.bnodes, fn + "upload a scene first (flx_upload_scene)");
    RefitTables &rf = c->rf;
    if (subset) {
        NEED(c, count <= rf.ntris, fn + "more triangles listed than the uploaded scene has (" + std::to_string(count) + " vs " + std::to_string(rf.ntris) + ")");
        NEED(c, count == 0 || (tris160 && indices), fn + "null triangles or indices");
    } else {
        NEED(c, tris160, fn + "null triangles");
        NEED(c, count == rf.ntris, fn + "the triangle count differs from the uploaded scene's (" + std::to_string(count) + " vs " + std::to_string(rf.ntris) + ")");
    }
    HIPCHK(c, hipSetDevice(c->device));
    const void *src = tris160; const uint32_t *idx = subset ? indices : nullptr;
    if (!subset || count) {                               // (nothing listed: no byte of any tree changes)
        if (src_on_device) {
            if (subset) NEED(c, ((uintptr_t)tris160 & 15u) == 0 && ((uintptr_t)indices & 3u) == 0, fn + "a device source must be 16-byte (triangles) and 4-byte (indices) aligned");
            else NEED(c, ((uintptr_t)tris160 & 15u) == 0, fn + "a device source must be 16-byte aligned");
        } else {                                          // first host source: the staging buffers (ntris wire triangles, ntris indices) stay with the scene allocations
            if (!rf.stage) {
                flx_triangle *st = nullptr;
                if (dalloc(c, c->sceneAllocs, &st, rf.ntris)) return 1;
                rf.stage = st;
            }
            HIPCHK(c, hipMemcpyAsync(rf.stage, tris160, count * sizeof(flx_triangle), hipMemcpyHostToDevice, c->stream));
            src = rf.stage;
            if (subset) {
                if (!rf.stageIdx && dalloc(c, c->sceneAllocs, &rf.stageIdx, rf.ntris)) return 1;
                HIPCHK(c, hipMemcpyAsync(rf.stageIdx, indices, count * 4, hipMemcpyHostToDevice, c->stream));
                idx = rf.stageIdx;
            }
        }
        if (subset) {
            if (!rf.triStamp) {                           // first subset call on this scene: the stamps stay with the scene allocations, zeroed ONCE
                const size_t nb = c->wideInfo[6], nw = c->wideInfo[0], nl = c->wideInfo[1];
                uint32_t *st = nullptr;
                if (dalloc(c, c->sceneAllocs, &st, (size_t)rf.ntris + nb + nw + nl)) return 1;
                rf.stampWords = (size_t)rf.ntris + nb + nw + nl;
                HIPCHK(c, hipMemsetAsync(st, 0, rf.stampWords * 4, c->stream));
                rf.triStamp = st; rf.bStamp = st + rf.ntris; rf.wStamp = rf.bStamp + nb; rf.lStamp = rf.wStamp + nw;
                rf.epoch = 0;
            }
            if (++rf.epoch == 0) {                        // the counter wrapped: stamps of 2^32 calls ago would read as this call's
                HIPCHK(c, hipMemsetAsync(rf.triStamp, 0, rf.stampWords * 4, c->stream));
                rf.epoch = 1;
            }
        }
        // one reduction over the source, one small blocking read (as flx_mk_adaptive_update reads its count)
        uint32_t v[4] = {0, 0, 0, 0};
        HIPCHK(c, hipMemsetAsync(rf.valid, 0, 16, c->stream));
        launch_refit_validate(c->stream, src, idx, (uint32_t)count, c->sc, rf, rf.valid);
        LAUNCHED(c);
        HIPCHK(c, hipMemcpyAsync(v, rf.valid, 16, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        float maxAbs; memcpy(&maxAbs, &v[1], 4);
        NEED(c, !(v[3] & 2u), fn + "triangle index out of range");              // (v[3]: the list's word, zero without one)
        NEED(c, !(v[3] & 1u), fn + "the indices are not strictly ascending");
        NEED(c, !v[0], fn + "triangle with a NaN or infinite vertex");
        NEED(c, maxAbs <= FLX_WIDE_COORD_MAX, fn + "vertex beyond +-2^62");
        NEED(c, !v[2], fn + "triangle material id out of range");
        // the root box is the union of the vertices: the same maximum -- over the moved triangles' new and the unmoved triangles' stored
        // positions -- re-derives the node test's clamp
        c->sc.wideClamp = wideClampFor(maxAbs);
    }
    // what flx_upload_scene clears: a list of active pixels and a G-buffer belong to the render of one geometry
    c->ad.have = false;
    c->temporal.gbTraced[0] = c->temporal.gbTraced[1] = false; c->temporal.histHave = false;
    if (subset && !count) return 0;
    {
        ScopedTimer t(c, FLX_K_REFIT);
        launch_refit(c->stream, src, idx, (uint32_t)count, c->sc, rf);
    }
    LAUNCHED(c);
    return 0;
}

extern "C" {

int flx_update_triangles(flx_ctx *c, const void *tris160, size_t ntris, int src_on_device)
{
    return updateTriangles(c, false, tris160, nullptr, ntris, src_on_device);
}

int flx_update_triangles_subset(flx_ctx *c, const void *tris160, const uint32_t *indices, size_t count, int src_on_device)
{
    return updateTriangles(c, true, tris160, indices, count, src_on_device);
}

int flx_tree_read(flx_ctx *c, int which, void *out, size_t bytes, size_t *needed)
{
    ENTER(c, CALL_QUIET);                                 // a read-back of arrays no deferred launch writes
    NEED(c, c->sc.bnodes, "flx_tree_read: upload a scene first (flx_upload_scene)");
    NEED(c, which >= 0 && which <= 4 && needed, "flx_tree_read: which must be 0..4 and needed not null");
    const void *p[5] = {c->sc.bnodes, c->sc.trirecs, c->sc.shade, c->sc.wnodes, c->sc.wleaf};
    const size_t n[5] = {(size_t)c->wideInfo[6] * sizeof(BNode), (size_t)c->rf.nidx * sizeof(TriRec), (size_t)c->rf.ntris * sizeof(ShadeRec),
                         (size_t)c->wideInfo[0] * sizeof(flxw::WNode), (size_t)c->wideInfo[1] * sizeof(float4)};
    *needed = n[which];
    if (!out) return 0;
    NEED(c, bytes >= n[which], "flx_tree_read: buffer too small");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(out, p[which], n[which], hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int flx_tree_cost(flx_ctx *c, double *out8)
{
    ENTER(c, CALL_QUIET);                                 // reads arrays no deferred launch writes; stream-ordered behind a refit
    NEED(c, c->sc.bnodes, "flx_tree_cost: upload a scene first (flx_upload_scene)");
    NEED(c, out8, "flx_tree_cost: null out8");
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->rf.costSlab && dalloc(c, c->sceneAllocs, &c->rf.costSlab, tree_cost_slab_doubles(c->rf))) return 1;   // stays with the scene allocations
    const double *res;
    {
        ScopedTimer t(c, FLX_K_TREE_COST);
        res = launch_tree_cost(c->stream, c->sc, c->rf, c->rf.costSlab);
    }
    LAUNCHED(c);
    HIPCHK(c, hipMemcpyAsync(out8, res, 8 * sizeof(double), hipMemcpyDeviceToHost, c->stream));   // one small blocking read, as flx_update_triangles' validation
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

} // extern "C"
