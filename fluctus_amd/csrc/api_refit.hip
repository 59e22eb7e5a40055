// api_refit.hip -- flx_update_triangles and flx_update_triangles_subset: the uploaded scene's triangles (or a listed subset of them) move, both traversal trees are refitted on the device over the topology
// flx_upload_scene built (kernels: refit.hip; arithmetic and the exactness argument: flx_refit.h), and its test hook
// flx_tree_read, and flx_tree_cost (kernels: tree_cost.hip; what is summed: flx_tree_cost.h): how far the refits have degraded
// the trees.  Validation runs on the device BEFORE anything is overwritten, so a refused call leaves the old scene as it was.
// flx_objects_define / flx_objects_pose (kernels: pose.hip; arithmetic: flx_pose.h): objects over the uploaded triangles, moved by
// a matrix each -- their triangles are produced on the device and handed to the subset refit as a device source -- and the test hook flx_objects_read.
#include "flx_ctx.h"
#include "flx_pose.h"
#include "flx_wide.h"
#include "flx_trace4.h"
#include <cstring>

namespace flxd {
float wideClampFor(float maxAbsCoord) { return maxAbsCoord < 67108864.0f ? FLX_WIDE_DINV_MAX : FLX_WIDE_DINV_FAR; }
int wideFar(const flx_ctx *c) { return c->sc.wideClamp == FLX_WIDE_DINV_FAR ? 1 : 0; }
// option "motion_history" (DESIGN.md 4.3.4): the object of every triangle and the per-object motion table, made by the first flx_gbuffer or
// flx_objects_pose that finds the option on and objects defined; they live and die with the definition (flx_ctx::Objects)
int motionTables(flx_ctx *c)
{
    flx_ctx::Objects &ob = c->ob;
    if (!c->motionHistory || !ob.have || ob.objectOfTri) return 0;
    uint32_t *oot = nullptr; float4 *tab = nullptr; void *pin = nullptr;
    const size_t rows = (size_t)ob.t.nobjects * 4;
    if (dalloc(c, ob.allocs, &oot, c->rf.ntris) || dalloc(c, ob.allocs, &tab, rows)) return 1;       // (a failed call leaves what it allocated to the definition's release)
    HIPCHK(c, hipHostMalloc(&pin, rows * sizeof(float4)));
    ob.motion = tab; ob.motionPinned = (float4 *)pin;
    HIPCHK(c, hipMemsetAsync(oot, 0xFF, (size_t)c->rf.ntris * 4, c->stream));                         // FLX_NO_OBJECT
    launch_object_of_triangle(c->stream, ob.t, oot);
    LAUNCHED(c);
    ob.objectOfTri = oot;
    return 0;
}
}

// The boundary of both calls, written once.  flx_update_triangles: every triangle, count must be the scene's.  flx_update_triangles_subset
// (`subset`): the source is a list, validation also checks the list and reduces the maximum |coordinate| over the unmoved triangles' stored
// positions (the clamp is that of the WHOLE resulting set, never a running maximum), and the passes rewrite only what is dirty (refit.hip: one
// set of passes, two modes).  Every message carries the name of the call it refuses (`as`: flx_objects_pose, which ends in the subset call and says
// so with `byPose`: what a pose keeps of a captured history, TemporalState::trianglesMoved).
static int updateTriangles(flx_ctx *c, bool subset, const void *tris160, const uint32_t *indices, size_t count, int src_on_device, const char *as = nullptr,
                           bool byPose = false)
{
    const std::string fn = as ? as : subset ? "flx_update_triangles_subset: " : "flx_update_triangles: ";
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
    c->ad.state.dropped();
    // option "deform_history" (DESIGN.md 4.3.6): the first accepted move after a capture copies every triangle's positions aside, on the stream,
    // before launch_refit overwrites any; later moves before the next capture keep that snapshot
    if (c->temporal.state.needsSnapshot(c->deformHistory != 0)) {
        if (!rf.snapPos && (dalloc(c, c->sceneAllocs, &rf.snapPos, (size_t)rf.ntris * 3) || dalloc(c, c->sceneAllocs, &rf.movedFlags, rf.ntris))) { rf.snapPos = nullptr; return 1; }
        { ScopedTimer t(c, FLX_K_SNAPSHOT); launch_snapshot_positions(c->stream, c->sc, rf.ntris, rf.snapPos); }
        LAUNCHED(c);
    }
    c->temporal.state.trianglesMoved(byPose, c->motionHistory != 0, c->deformHistory != 0);
    if (!byPose) c->ob.pose.trianglesSetDirectly();
    if (subset && !count) return 0;
    {
        ScopedTimer t(c, FLX_K_REFIT);
        launch_refit(c->stream, src, idx, (uint32_t)count, c->sc, rf);
    }
    LAUNCHED(c);
    c->ml.state.trianglesMoved();                         // option "mesh_lights": a moved lamp has another area; rebuilt on the stream behind the refit
    return meshLightsSync(c);
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

int flx_objects_define(flx_ctx *c, const void *tris160_rest, size_t ntris, const uint32_t *object_of_triangle, uint32_t nobjects)
{
    const std::string fn = "flx_objects_define: ";
    ENTER(c, CALL_OBSERVE);
    NEED(c, c->sc.bnodes, fn + "upload a scene first (flx_upload_scene)");
    HIPCHK(c, hipSetDevice(c->device));
    if (!nobjects) { c->ob.release(); c->temporal.state.definitionChanged(c->motionHistory); return 0; }
    NEED(c, tris160_rest && object_of_triangle, fn + "null triangles or object ids");
    NEED(c, ntris == c->rf.ntris, fn + "the triangle count differs from the uploaded scene's (" + std::to_string(ntris) + " vs " + std::to_string(c->rf.ntris) + ")");
    flx_ctx::Objects ob;                                  // built aside: a refused or failed call leaves the earlier definition in place
    ob.counts.resize(nobjects);
    size_t bad = 0;
    const size_t members = flx::ps_count_members(object_of_triangle, ntris, nobjects, ob.counts.data(), &bad);
    NEED(c, members != (size_t)-1, fn + "triangle " + std::to_string(bad) + " has an object id that is neither below the object count nor FLX_NO_OBJECT");
    std::vector<uint32_t> tri(members), obj(members);
    std::vector<flx_triangle> rest(members);
    flx::ps_compact_members(tris160_rest, object_of_triangle, ntris, tri.data(), obj.data(), rest.data());
    ObjectTables &t = ob.t;
    t.nobjects = nobjects; t.members = (uint32_t)members;
    const uint32_t nb = pose_blocks(t.members);
    struct Guard { flx_ctx::Objects &o; bool keep = false; ~Guard() { if (!keep) freeAll(o.allocs); } } guard{ob};
    if (dalloc(c, ob.allocs, &t.memberTri, members) || dalloc(c, ob.allocs, &t.memberObj, members) || dalloc(c, ob.allocs, &t.rest, members * FLX_PS_TRI_V4) ||
        dalloc(c, ob.allocs, &t.stamp, (size_t)nobjects * 2) || dalloc(c, ob.allocs, &t.ids, nobjects) || dalloc(c, ob.allocs, &t.xforms, (size_t)nobjects * 3) ||
        dalloc(c, ob.allocs, &t.out, members * FLX_PS_TRI_V4) || dalloc(c, ob.allocs, &t.outIdx, members) || dalloc(c, ob.allocs, &t.blockCounts, (size_t)nb + 1)) return 1;
    t.slot = t.stamp + nobjects; t.total = t.blockCounts + nb;
    if (members) {
        HIPCHK(c, hipMemcpy(t.memberTri, tri.data(), members * 4, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(t.memberObj, obj.data(), members * 4, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(t.rest, rest.data(), members * sizeof(flx_triangle), hipMemcpyHostToDevice));
    }
    HIPCHK(c, hipMemset(t.stamp, 0, (size_t)nobjects * 8));  // epoch 0 is never a call's
    ob.have = true;
    ob.pose.defined(nobjects);                            // every pose unknown
    guard.keep = true;
    c->ob.release();
    c->ob = std::move(ob);
    c->temporal.state.definitionChanged(c->motionHistory);
    return 0;
}

int flx_objects_pose(flx_ctx *c, const uint32_t *object_ids, const float *xforms12, uint32_t count)
{
    const char *name = "flx_objects_pose: ";
    const std::string fn = name;
    ENTER(c, CALL_OBSERVE);                               // deferred and fused launches run against the OLD scene
    NEED(c, c->sc.bnodes, fn + "upload a scene first (flx_upload_scene)");
    NEED(c, c->ob.have, fn + "no objects are defined (flx_objects_define)");
    ObjectTables &t = c->ob.t;
    NEED(c, count <= t.nobjects, fn + "more objects listed than are defined (" + std::to_string(count) + " vs " + std::to_string(t.nobjects) + ")");
    NEED(c, count == 0 || (object_ids && xforms12), fn + "null object ids or transforms");
    size_t n = 0;
    for (uint32_t k = 0; k < count; k++) {
        const uint32_t o = object_ids[k];
        NEED(c, o < t.nobjects, fn + "object id out of range (" + std::to_string(o) + " of " + std::to_string(t.nobjects) + ")");
        NEED(c, k == 0 || o > object_ids[k - 1], fn + "the object ids are not strictly ascending");
        NEED(c, flx::ps_xform_finite(xforms12 + 12 * (size_t)k), fn + "the transform of object " + std::to_string(o) + " has a NaN or infinite entry");
        NEED(c, flx::ps_xform_invertible(xforms12 + 12 * (size_t)k), fn + "the transform of object " + std::to_string(o) + " has a zero or non-finite determinant");
        n += c->ob.counts[o];
    }
    HIPCHK(c, hipSetDevice(c->device));
    if (motionTables(c)) return 1;
    if (n) {
        // the list goes up as flx_update_triangles_subset's host source does: read by the time the validation's blocking read returns
        HIPCHK(c, hipMemcpyAsync(t.ids, object_ids, (size_t)count * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(t.xforms, xforms12, (size_t)count * 48, hipMemcpyHostToDevice, c->stream));
        if (++t.epoch == 0) {                             // the counter wrapped: stamps of 2^32 calls ago would read as this call's
            HIPCHK(c, hipMemsetAsync(t.stamp, 0, (size_t)t.nobjects * 4, c->stream));
            t.epoch = 1;
        }
        {
            ScopedTimer tm(c, FLX_K_REFIT);               // (the refit's own pair follows the validation: one pose is two timed spans of this id)
            launch_pose(c->stream, t, count);
        }
        LAUNCHED(c);
    }
    if (updateTriangles(c, true, t.out, t.outIdx, n, 1, name, true)) return 1;
    c->ob.pose.posed(object_ids, xforms12, count);        // accepted: these are the listed objects' poses now
    return 0;
}

int flx_objects_read(flx_ctx *c, uint32_t *out_counts, uint32_t *out_nobjects, uint32_t *out_members)
{
    ENTER(c, CALL_QUIET);                                 // a read-back of arrays no deferred launch writes
    NEED(c, c->ob.have, "flx_objects_read: no objects are defined (flx_objects_define)");
    NEED(c, out_nobjects, "flx_objects_read: null out_nobjects");
    const ObjectTables &t = c->ob.t;
    *out_nobjects = t.nobjects;
    if (out_counts) memcpy(out_counts, c->ob.counts.data(), (size_t)t.nobjects * 4);
    if (out_members && t.members) {
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipMemcpyAsync(out_members, t.memberTri, (size_t)t.members * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return 0;
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
