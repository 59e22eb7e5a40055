// flx_feature_state.h -- what the context knows about the data derived from the framebuffers and the scene, and WHICH CALL INVALIDATES WHAT
// (DESIGN.md 4.3.5): the logical state of the G-buffer slots and the captured history, of the objects' poses, of the list of active pixels and of
// the table of emissive triangles,
// each with its transitions named after what happened.  The entry points (csrc/api*.hip) call a transition and ask a predicate; none writes a
// flag.  Plain C++17, no HIP, nothing that owns device memory: the buffers stay in flx_ctx (flx_ctx.h), whose Temporal, Objects, Adaptive and MeshLight embed
// these types and release them to their defaults with the buffers.  tests/feature_state_cpu.cpp runs the table of tests/feature_state_cases.py
// through this header without a GPU, tests/test_gpu_feature_state.py the same table through the C ABI.
#pragma once
#include "../../include/fluctus_hip.h"
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace flxd {
// temporal reprojection (reproject.hip).  Two G-buffer slots, [0] current, [1] previous, each with the camera and the size it
// was traced with.  traced: the slot holds a G-buffer.  objects (option "motion_history"): the object plane beside the slot
// belongs to the slot's G-buffer and to the current definition -- never set without `traced`.  bary (option "deform_history"):
// the barycentric plane beside the slot belongs to the slot's G-buffer and to the uploaded triangle set -- never set without `traced`.
// hist: flx_history_capture has copied the accumulation; histMom: and the moments with it ("moments" was on then).  histMom is rewritten by the
// next capture and by nothing else.  snap ("deform_history"): triangles moved since the capture and their positions at the capture were
// snapshotted first -- flx_reproject follows them (flx_reproject_deform.h); never set without a history.
// mark (history rectification): flx_history_mark has copied the accumulation of a markW x markH image; markMom: and the moments
// with it.  The mark belongs to the accumulation it was copied from and to the current slot's G-buffer: whatever restarts the accumulation,
// re-partitions or re-shapes the image, hands the current slot over, un-traces it or uploads a scene drops it.
struct TemporalState {
    struct Slot { flx_camera cam = {}; uint32_t W = 0, H = 0; bool traced = false, objects = false, bary = false; };
    Slot slot[2];
    bool hist = false, histMom = false, snap = false;
    bool mark = false, markMom = false; uint32_t markW = 0, markH = 0;

    // flx_gbuffer traced slot 0 (withObjects: the option is on and objects are defined) | flx_gbuffer_write wrote a slot (its plane, kept only
    // while the option is on, shows no object) | flx_gbuffer_objects_write wrote the plane behind it
    void traced(const flx_camera &cam, uint32_t W, uint32_t H, bool withObjects) { slot[0] = Slot{cam, W, H, true, withObjects}; }
    void written(int s, const flx_camera &cam, uint32_t W, uint32_t H, bool motionHistory) { slot[s] = Slot{cam, W, H, true, motionHistory}; }
    void objectsWritten(int s) { slot[s].objects = true; }
    // ... and, right behind traced() / written(): the slot's barycentric plane was written with it (deformHistory: the option's value; a written
    // G-buffer's plane holds the sentinel) | flx_gbuffer_bary_write wrote the plane
    void baryWith(int s, bool deformHistory) { slot[s].bary = deformHistory; }
    void baryWritten(int s) { slot[s].bary = true; }
    // flx_history_capture: the current slot becomes the previous one (the caller swaps the buffers) and no longer is the current one; nothing
    // has moved since THIS capture
    void captured(bool withMoments) { slot[1] = slot[0]; slot[1].traced = true; slot[0].traced = slot[0].objects = slot[0].bary = false; hist = true; histMom = withMoments; snap = false; markDropped(); }
    // a G-buffer and a history belong to the render of one geometry
    void dropHistory() { slot[0].traced = slot[1].traced = false; slot[0].objects = slot[1].objects = false; slot[0].bary = slot[1].bary = false; hist = false; snap = false; markDropped(); }
    // triangles moved.  By flx_objects_pose with a history it can follow (flx_reproject_motion.h): the previous slot and the history stay, only
    // the current slot is gone.  Otherwise, and always for triangles set one by one -- nobody knows where those were -- everything goes.
    bool poseKeepsHistory(bool motionHistory) const { return motionHistory && hasHistory() && slot[1].objects; }
    void trianglesMoved(bool byPose, bool motionHistory) { snap = false; markDropped(); if (byPose && poseKeepsHistory(motionHistory)) slot[0].traced = slot[0].objects = slot[0].bary = false; else dropHistory(); }
    // ... unless option "deform_history" knows where they were: with a history whose G-buffer has a barycentric plane, ANY move (one by one, a
    // subset, a pose) keeps the previous slot and the history -- the caller has snapshotted the positions before it overwrites them when
    // needsSnapshot() said so -- and only the current slot is gone.  Any other move does what it does without the option.
    bool moveKeepsHistory(bool deformHistory) const { return deformHistory && hasHistory() && slot[1].bary; }
    bool needsSnapshot(bool deformHistory) const { return moveKeepsHistory(deformHistory) && !snap; }
    void trianglesMoved(bool byPose, bool motionHistory, bool deformHistory)
    {
        if (!moveKeepsHistory(deformHistory)) { trianglesMoved(byPose, motionHistory); return; }
        snap = true; slot[0].traced = slot[0].objects = slot[0].bary = false; markDropped();
    }
    // flx_upload_scene, flx_objects_define: the planes name the objects of the earlier definition; with the option on the history goes with it
    void definitionChanged(bool motionHistory) { motionHistoryOff(); if (motionHistory) dropHistory(); }
    void motionHistoryOff() { slot[0].objects = slot[1].objects = false; }     // planes not kept up while the option is off are nobody's
    // flx_upload_scene (behind definitionChanged): the hit indices no longer name the same triangles and the snapshot went with the scene
    void sceneUploaded(bool deformHistory) { if (deformHistory) dropHistory(); snap = false; markDropped(); }
    // "deform_history" switched off: the planes are nobody's; a move the history has not been told of otherwise takes the history with it --
    // never a reprojection that ignores a move
    void deformHistoryOff() { slot[0].bary = slot[1].bary = false; if (snap) dropHistory(); }

    // flx_history_mark copied the accumulation (and the moments) under the current slot | flx_wf_reset, flx_mk_reset: the accumulation restarted |
    // flx_set_params with another width or height | flx_set_partition -- and every transition above that takes the current slot away
    void marked(bool withMoments) { mark = true; markMom = withMoments; markW = slot[0].W; markH = slot[0].H; }
    void accumulationReset() { markDropped(); }
    void imageResized() { markDropped(); }
    void partitionSet() { markDropped(); }
    void markDropped() { mark = false; markMom = false; }

    bool holds(int s) const { return slot[s].traced; }
    bool holdsSized(int s, uint32_t W, uint32_t H) const { return slot[s].traced && slot[s].W == W && slot[s].H == H; }
    bool holdsObjects(int s) const { return slot[s].traced && slot[s].objects; }
    bool holdsBary(int s) const { return slot[s].traced && slot[s].bary; }
    bool hasHistory() const { return hist && slot[1].traced; }
    bool historyFits(uint32_t W, uint32_t H) const { return slot[0].W == W && slot[0].H == H && slot[1].W == W && slot[1].H == H; }
    bool followsMoves() const { return snap && hasHistory(); }                  // flx_reproject runs the per-vertex kernels
    bool followsMovesReady() const { return holdsBary(0) && holdsBary(1); }     // ... and has both planes for them
    bool hasMark() const { return mark; }
    bool markLive() const { return mark && holdsSized(0, markW, markH); }       // flx_history_rectify: the mark and the G-buffer it is compared under
    bool markHasMoments() const { return mark && markMom; }
};

// every object's pose now and at the last flx_history_capture (12 floats each, flx_objects_pose's matrices) with a `known` byte: unknown until
// the object has been posed since the definition -- the uploaded triangles need not be the rest pose.  Kept whatever the options say.
struct PoseState {
    std::vector<float> xNow, xCap; std::vector<uint8_t> known, knownCap;

    void defined(uint32_t nobjects) { xNow.assign((size_t)nobjects * 12, 0.0f); xCap = xNow; known.assign(nobjects, 0); knownCap = known; }
    void posed(const uint32_t *ids, const float *x12, uint32_t count) { for (uint32_t k = 0; k < count; k++) { memcpy(&xNow[12 * (size_t)ids[k]], x12 + 12 * (size_t)k, 48); known[ids[k]] = 1; } }
    void trianglesSetDirectly() { std::fill(known.begin(), known.end(), (uint8_t)0); }      // no object is where its last pose put it
    void captured() { xCap = xNow; knownCap = known; }                                       // every object's pose under this history
    // rm_make_table's arguments (flx_reproject_motion.h: X_cap, X_now)
    struct Poses { const float *atCapture; const uint8_t *atCaptureKnown; const float *now; const uint8_t *nowKnown; };
    Poses sinceCapture() const { return {xCap.data(), knownCap.data(), xNow.data(), known.data()}; }
    size_t count() const { return known.size(); }
};

// the adaptive microkernel render (adaptive.hip): while `have`, the sample pass's four kernels run over a list of `count`
// active pixels (ascending; 0 = the calls are no-ops) out of `pix`; have false = every pixel.  The list belongs to one scene, one geometry,
// one image size and partition, and to the moments it was derived from: each of those drops it.
struct ActiveListState {
    uint32_t pix = 0, count = 0; bool have = false;
    void installed(uint32_t n) { count = n; have = true; }
    void dropped() { have = false; }
};

// the table of emissive triangles (option "mesh_lights"; mesh_light.hip).  `listed`: the uploaded scene's `lights` emissive
// triangles are known (the list depends on the materials, which only flx_upload_scene brings).  `built`: the device table was built from the
// triangles as they stand.  Every call that moves triangles makes it stale; while the option is on the same call rebuilds it before it returns
// (api_mesh_light.hip: meshLightsSync), so between two calls the table is never stale with the option on.
// `wavefront` (option "mesh_lights_wavefront"): the wavefront integrator's logic pass sees the lamps too.  A wish of its own: set
// and cleared by its option alone, in either order with "mesh_lights", kept across uploads; it takes effect only while lit() holds.
struct MeshLightState {
    bool on = false, listed = false, built = false, wavefront = false; uint32_t lights = 0;
    void optionSet(bool v) { on = v; if (!v) built = false; }           // kept up only while the option is on: switching it on builds
    void wavefrontSet(bool v) { wavefront = v; }
    void sceneUploaded(uint32_t n) { listed = true; built = false; lights = n; }
    void trianglesMoved() { built = false; }
    void rebuilt() { built = true; }
    bool needsBuild() const { return on && listed && !built; }
    bool usable() const { return on && listed && built; }
    bool lit() const { return usable() && lights > 0; }             // the MESH instances of the microkernels run; otherwise the plain ones do
    bool litWavefront() const { return lit() && wavefront; }        // the MESH instance of the plain logic pass runs, and no pass is fused (api_wavefront.hip)
};
}
