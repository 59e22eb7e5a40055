// history_state.hpp -- what the Tracer knows about whether the device holds a HISTORY WORTH KEEPING, and what each public Tracer call does to that
// knowledge: the switches of temporal, motion-aware and per-vertex reprojection and of history rectification, the G-buffer
// the accumulation is being rendered under, the two frame counts and the pending mark, each transition named after what happened.  The state
// DECIDES AND KEEPS THE BOOKS; THE TRACER CALLS THE DEVICE: where update() or a move has to act on the outcome, the transition returns a small plan
// and the Tracer executes it in the order update() and moveTriangles() spell out.  tracer.cpp writes no member of this struct and reads them only
// through the predicates.  Plain C++17, no HIP, no HipContext, no Tracer; tests/tracer_history_cpu.cpp runs the table of
// tests/tracer_history_cases.py through this header without a GPU.  (The device's half of the same knowledge: csrc/flx_feature_state.h.)
//
// Invariants, which the order of the Tracer's statements used to imply:
//   - haveGbuffer: the context's current slot holds the G-buffer of the camera the accumulation is being rendered under, traced under gbParams at
//     gbWidth x gbHeight.  gbParams, gbWidth, gbHeight, framesSinceGbuffer and capturedThisFrame are NEVER READ WITHOUT haveGbuffer (historyExists
//     asks it first), so whatever clears haveGbuffer may leave them stale.  markPending is read without it (rectifyDue), so dropped() clears it --
//     runBenchmark leaves iteration != 0 and no frame start would -- and capturedThisFrame with it: one call says "no history" in every state.
//     (Tracer::init, which also sets iteration = 0 and arms the parameters, needs no more than haveGbuffer = false; it calls dropped() like the rest.)
//   - capturedThisFrame: flx_history_capture has already run since the last parameters reached the device -- a move of triangles under its switch
//     made it (or shared it) -- so the current slot is handed over and untraced.  The next paramsReachDevice() must not capture again (the device
//     refuses an untraced slot) and reprojects that capture; a second move, or a camera change pending in the same frame, shares it.  AT MOST ONE
//     CAPTURE PER FRAME.  Cleared when parameters reach the device and by dropped().
//   - markPending: a frame has run flx_history_mark and its rectify has not run yet.  The device drops its mark with every reset of the
//     accumulation, so every frame that starts at iteration 0 clears it (frameStarts), a frame that reprojects sets it again at its end.
//   - framesSinceGbuffer: frames rendered since the G-buffer was traced; > 0 (or capturedThisFrame): there is an accumulation worth capturing.
//   - temporalFrames: frames since the last DISCARDED history -- the denoiser's schedule while temporalOn (denoiserSchedule).  Only a frame that
//     starts at iteration 0 without reprojecting, and temporalSet(), restart it.
//
// What each public Tracer call does to the history ("drops": dropped(); P: the Tracer also sets paramsUpdatePending; I: and iteration = 0):
//   init                                   drops; P, I
//   updateGeometry (both), poseObjects     beforeMove -> [flx_history_capture] -> the move -> drops (P, I) -> afterMove: under the call's switch
//                                          (deformOn; poseObjects: motionOn or deformOn) and with a history the capture is kept and the next frame
//                                          reprojects it, unless a rebuild inside the call re-uploaded the topology.  A move the device refuses changes
//                                          nothing but P after a capture (the next frame traces the handed-over slot again and reprojects)
//   a rebuild the policy adopts            drops; P, I
//   defineObjects                          drops while motionOn (the object plane names the earlier definition's objects), else nothing
//   setEnvMap                              drops; P
//   setTemporalReprojection                temporalSet: drops, restarts the denoiser's schedule; off also switches the other three off
//   setMotionReprojection, setDeform...    motionSet / deformSet: drops (the G-buffer was traced without the plane the other setting needs)
//   setHistoryRectification                rectifySet: clears the pending mark
//   setRectifyDelay                        rectifyDelaySet
//   toggleRenderer, setMeshLights, setMeshLightsWavefront (when it changes something)      drops; I
//   renderSingle, renderAdaptive, runBenchmark       drops (parameters reach the device without a G-buffer)
//   update                                 paramsReachDevice (only while P) -> frameStarts -> the frame -> marked | rectifyDue, rectified ->
//                                          frameRendered; the microkernel branch returns before the last three and drops in the first
//   setDenoiser, setDenoiserMode, paramsChanged, loadState, setMaxHistory                   nothing here (P or I: the next frame decides)
#pragma once
#include "../../include/fluctus_hip.h"
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace fluctus {

struct HistoryState {
    bool temporalOn = false, motionOn = false, deformOn = false, rectifyOn = false;
    bool haveGbuffer = false;
    flx_render_params gbParams {};
    uint32_t gbWidth = 0, gbHeight = 0;
    uint32_t framesSinceGbuffer = 0, temporalFrames = 0;
    bool capturedThisFrame = false, markPending = false;
    uint32_t rectifyDelay = 0;                               // 0: the default, 2 maxBounces + 2

    // ---- what happened
    // the G-buffer and the accumulation no longer belong to what the next frame renders
    void dropped() { haveGbuffer = false; capturedThisFrame = false; markPending = false; }
    // the switches; the Tracer's setters refuse first and set the device's options
    void temporalSet(bool on) { temporalOn = on; dropped(); temporalFrames = 0; }
    void motionSet(bool on) { motionOn = on; dropped(); }    // a G-buffer traced under the other setting has no object plane (or one nobody keeps up)
    void deformSet(bool on) { deformOn = on; dropped(); }    // ... no barycentric plane (or one nobody keeps up)
    void rectifySet(bool on) { rectifyOn = on; markPending = false; }
    void rectifyDelaySet(uint32_t frames) { rectifyDelay = frames; }
    // defineObjects: the G-buffer's object plane names the earlier definition's objects (the device has dropped its history too)
    void objectsDefined() { if (motionOn) dropped(); }

    // Triangles are about to move.  switchOn: the switch under which this kind of move keeps the history.  keep: there is
    // a history by update()'s own conditions, and the move keeps it; captureNow: the Tracer runs flx_history_capture before the ranks move -- at
    // most once per frame -- so that the device keeps it (a refused move must then re-arm update()).
    struct MovePlan { bool keep, captureNow; };
    MovePlan beforeMove(bool switchOn, const flx_render_params &params, bool useWavefront)
    {
        MovePlan p;
        p.keep = switchOn && historyExists(params, useWavefront, true);
        p.captureNow = p.keep && !capturedThisFrame;
        if (p.captureNow) capturedThisFrame = true;
        return p;
    }
    // ... they have moved, and dropped() has been called for the new geometry: the device still has the history, unless a rebuild inside the move
    // re-uploaded the topology (the device dropped its history with the upload)
    void afterMove(bool keep, bool topologyReuploaded) { if (keep && !topologyReuploaded) { haveGbuffer = true; capturedThisFrame = true; } }

    // update() with parameters pending.  The Tracer runs, in this order: flx_history_capture if captureNow (under the old camera's slot, BEFORE the
    // parameters reach the device), updateParams on every rank, flx_gbuffer if traceGbuffer; reprojectNow: the frame reprojects behind its reset.
    // Without a G-buffer (temporal reprojection off, the other integrator) the update is consumed and the slot is another camera's: dropped.
    struct ParamsPlan { bool captureNow, traceGbuffer, reprojectNow; };
    ParamsPlan paramsReachDevice(const flx_render_params &params, bool useWavefront)
    {
        ParamsPlan p;
        const bool temporal = temporalOn && useWavefront;
        // (a move has captured it already: a camera change pending in the same frame shares that capture)
        const bool history = historyExists(params, useWavefront, capturedThisFrame);
        p.captureNow = history && !capturedThisFrame;
        capturedThisFrame = false;
        p.traceGbuffer = temporal;
        p.reprojectNow = temporal && history;
        if (temporal) { haveGbuffer = true; gbParams = params; gbWidth = params.width; gbHeight = params.height; framesSinceGbuffer = 0; }
        else dropped();
        return p;
    }
    // a frame starts (behind paramsReachDevice).  Returns markNow: the frame ends on flx_history_mark
    bool frameStarts(uint32_t iteration, bool reprojectNow, bool useWavefront)
    {
        if (iteration == 0 && !reprojectNow) temporalFrames = 0;        // the accumulation restarts from nothing
        if (iteration == 0) markPending = false;                         // the frame's reset drops the device's mark
        return rectifyOn && reprojectNow && iteration == 0 && useWavefront;
    }
    // history rectification: the frame that reprojected marks what it has (history + preview); the frame at whose end
    // rectifyDelayFrames() frames have been rendered since that G-buffer compares, once, unless a newer reprojection has replaced the mark
    void marked() { markPending = true; }
    bool rectifyDue(uint32_t maxBounces) const { return rectifyOn && markPending && framesSinceGbuffer + 1 >= rectifyDelayFrames(maxBounces); }
    void rectified() { markPending = false; }
    // a wavefront frame has been rendered (the microkernel branch counts only its iteration)
    void frameRendered() { framesSinceGbuffer++; temporalFrames++; }

    // ---- predicates
    // a history exists: at least one frame rendered since the last G-buffer (or a move has captured it already), at the same size (a resize frees
    // the device's slots) and with nothing but the camera changed since (lights, bounces, sampling switches: the kept radiance would be stale)
    bool historyExists(const flx_render_params &params, bool useWavefront, bool posed) const
    {
        return temporalOn && useWavefront && haveGbuffer && (capturedThisFrame || framesSinceGbuffer > 0) && gbWidth == params.width && gbHeight == params.height &&
               onlyCameraChanged(params, posed);
    }
    // everything of the parameters that shapes the radiance of a point, i.e. all but the camera (bytes 96..175) and the post-process (exposure,
    // tmOperator: 176..183), equals what the G-buffer's frames were rendered with (posed: worldRadius aside, which a move re-derives)
    bool onlyCameraChanged(const flx_render_params &params, bool posed) const
    {
        flx_render_params now = params;
        if (posed) now.worldRadius = gbParams.worldRadius;
        if (rectifyOn) now.areaLight = gbParams.areaLight;   // history rectification sheds what a changed area light contradicts
        const char *a = (const char *)&now, *b = (const char *)&gbParams;
        return std::memcmp(a, b, offsetof(flx_render_params, camera)) == 0 &&
               std::memcmp(a + offsetof(flx_render_params, width), b + offsetof(flx_render_params, width), sizeof(flx_render_params) - offsetof(flx_render_params, width)) == 0;
    }
    // which frame the denoiser's "every 10th frame from frame 10 on" counts: frames since the last discarded history, or since the last restart
    uint32_t denoiserSchedule(uint32_t iteration) const { return temporalOn ? temporalFrames : iteration; }
    uint32_t rectifyDelayFrames(uint32_t maxBounces) const { return rectifyDelay ? rectifyDelay : 2 * maxBounces + 2; }
    bool temporal() const { return temporalOn; }
    bool motion() const { return motionOn; }
    bool deform() const { return deformOn; }
    bool rectify() const { return rectifyOn; }
};

} // namespace fluctus
