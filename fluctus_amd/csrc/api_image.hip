// api_image.hip -- what works on the image rather than on the wavefront queues: flx_postprocess, the two a-trous denoisers, temporal
// reprojection (G-buffer slots, history capture), and the microkernel integrator with its adaptive render and statistics.
#include "flx_ctx.h"
#include "flx_denoise.h"
#include "flx_denoise_vg.h"
#include "flx_reproject_motion.h"
#include "flx_reproject_deform.h"
#include "flx_rectify.h"
#include "flx_adaptive.h"
#include <cstring>

extern "C" {

int flx_postprocess(flx_ctx *c) { READY(c, CALL_OBSERVE); { ScopedTimer t(c, FLX_K_POSTPROCESS); launch_postprocess(c->stream, c->fr, c->params); } LAUNCHED(c); return 0; }

// flx_denoise and flx_denoise_variance_guided: the checks, the working set (allocated by the first call), the timer and dnHave.  fn names the
// entry point in the messages, sigma0 its first sigma; the variance-guided filter needs the luminance moments.
typedef void (*DenoiseLaunch)(hipStream_t, const Frame &, float4 *, float4 *, float4 *, float2 *, float *, int, int, int, float, float, float, float,
                              const flx_render_params &);
static int denoiseCall(flx_ctx *c, const char *fn, DenoiseLaunch launch, bool moments, const char *sigma0, int iterations, float s0, float sigma_n,
                       float sigma_a, float blend)
{
    READY(c, CALL_OBSERVE);
    NEED(c, c->denoiser && c->fr.aovAlbedo && c->fr.aovNormal, std::string(fn) + ": needs the feature buffers: flx_set_option(ctx, \"denoiser\", 1)");
    if (moments)
        NEED(c, c->moments && c->fr.moments, std::string(fn) + ": needs the luminance moments: flx_set_option(ctx, \"moments\", 1)");
    NEED(c, c->fr.nranks == 1, std::string(fn) + ": the context is partitioned (nranks > 1): a pixel's neighbours are on other ranks -- single-GPU only");
    NEED(c, iterations >= 0 && iterations <= FLX_DN_MAX_ITERATIONS, std::string(fn) + ": iterations must be 0..8");
    NEED(c, dn_finite(s0) && s0 > 0.0f && dn_finite(sigma_n) && sigma_n > 0.0f && dn_finite(sigma_a) && sigma_a > 0.0f,
         std::string(fn) + ": " + sigma0 + ", sigma_normal and sigma_albedo must be finite and > 0");
    NEED(c, blend == blend, std::string(fn) + ": blend is NaN");
    const int W = (int)c->params.width, H = (int)c->params.height;
    NEED(c, (uint64_t)W * H == c->fr.localPixels, std::string(fn) + ": framebuffer does not match width x height");
    if (!c->dn.out) {
        const size_t n = c->fr.localPixels;
        if (dalloc(c, c->dn.allocs, &c->dn.e[0], n) || dalloc(c, c->dn.allocs, &c->dn.e[1], n) || dalloc(c, c->dn.allocs, &c->dn.g, n) ||
            dalloc(c, c->dn.allocs, &c->dn.g2, n) || dalloc(c, c->dn.allocs, &c->dn.out, n * 4)) { c->dn.release(); return 1; }
    }
    { ScopedTimer t(c, FLX_K_DENOISE);
      launch(c->stream, c->fr, c->dn.e[0], c->dn.e[1], c->dn.g, c->dn.g2, c->dn.out, W, H, iterations, s0, sigma_n, sigma_a, dn_blend(blend), c->params); }
    LAUNCHED(c);
    c->dn.have = true;
    return 0;
}

// DenoiserOptix::denoise (reference: src/denoiser/OptixDenoiser.cpp) as the guided a-trous filter of csrc/flx_denoise.h: reads which = 0 / 4 / 5,
// writes which = 6 and the preview (which = 1).  Asynchronous; deferred and fused launches are flushed first (CALL_OBSERVE).
int flx_denoise(flx_ctx *c, const flx_denoise_params *pp)
{
    flx_denoise_params p = {FLX_DN_DEFAULT_ITERATIONS, FLX_DN_DEFAULT_SIGMA_COLOR, FLX_DN_DEFAULT_SIGMA_NORMAL, FLX_DN_DEFAULT_SIGMA_ALBEDO, 0.0f};
    if (pp) p = *pp;
    return denoiseCall(c, "flx_denoise", launch_denoise<DnGuided>, false, "sigma_color", p.iterations, p.sigma_color, p.sigma_normal, p.sigma_albedo,
                       p.blend);
}

// the variance-guided filter of csrc/flx_denoise_vg.h: flx_denoise's inputs plus the luminance moments (which = 7); the same
// outputs, working set (the variance rides in e.w), timer and flushing.
int flx_denoise_variance_guided(flx_ctx *c, const flx_denoise_vg_params *pp)
{
    flx_denoise_vg_params p = {FLX_VG_DEFAULT_ITERATIONS, FLX_VG_DEFAULT_SIGMA_LUMINANCE, FLX_VG_DEFAULT_SIGMA_NORMAL, FLX_VG_DEFAULT_SIGMA_ALBEDO, 0.0f};
    if (pp) p = *pp;
    return denoiseCall(c, "flx_denoise_variance_guided", launch_denoise<DnVg>, true, "sigma_luminance", p.iterations, p.sigma_luminance,
                       p.sigma_normal, p.sigma_albedo, p.blend);
}

// ---- temporal reprojection (csrc/flx_reproject.h, reproject.hip).  All of it needs an unpartitioned context: a pixel's
// neighbours must be local.  Every entry point flushes deferred and fused launches first (CALL_OBSERVE) and touches no path state, queue or counter.
static int temporalReady(flx_ctx *c, const char *fn)
{
    NEED(c, c->haveParams && c->fr.pixels, std::string(fn) + ": set params first (flx_set_params)");
    NEED(c, c->fr.nranks == 1, std::string(fn) + ": the context is partitioned (nranks > 1): a pixel's neighbours are on other ranks -- single-GPU only");
    NEED(c, (uint64_t)c->params.width * c->params.height == c->fr.localPixels, std::string(fn) + ": framebuffer does not match width x height");
    return 0;
}
static int gbufferSlots(flx_ctx *c)
{
    const size_t n = (size_t)c->fr.localPixels * 2;
    if (!c->temporal.gb[0] && (dalloc(c, c->temporal.allocs, &c->temporal.gb[0], n) || dalloc(c, c->temporal.allocs, &c->temporal.gb[1], n))) { c->temporal.release(); return 1; }
    // option "motion_history": one object id per pixel beside each slot; off: nothing is allocated
    if (c->motionHistory && !c->temporal.objPlane[0] &&
        (dalloc(c, c->temporal.allocs, &c->temporal.objPlane[0], n / 2) || dalloc(c, c->temporal.allocs, &c->temporal.objPlane[1], n / 2))) { c->temporal.release(); return 1; }
    // option "deform_history": one float2 of barycentrics per pixel beside each slot; off: nothing is allocated
    if (c->deformHistory && !c->temporal.baryPlane[0] &&
        (dalloc(c, c->temporal.allocs, &c->temporal.baryPlane[0], n / 2) || dalloc(c, c->temporal.allocs, &c->temporal.baryPlane[1], n / 2))) { c->temporal.release(); return 1; }
    return 0;
}
int flx_gbuffer(flx_ctx *c)
{
    READY(c, CALL_OBSERVE);
    if (temporalReady(c, "flx_gbuffer") || gbufferSlots(c) || motionTables(c)) return 1;
    const bool obj = c->motionHistory && c->ob.have;      // the object plane is written only while the option is on and objects are defined
    { ScopedTimer t(c, FLX_K_GBUFFER);
      launch_gbuffer(c->stream, c->sc, c->params, c->spill, c->numTasks, (c->extendTree == 4 && c->wideOK) ? 4 : 2, c->temporal.gb[0], c->fr.localPixels,
                     obj ? c->temporal.objPlane[0] : nullptr, obj ? c->ob.objectOfTri : nullptr, c->deformHistory ? c->temporal.baryPlane[0] : nullptr); }
    LAUNCHED(c);
    c->temporal.state.traced(c->params.camera, c->params.width, c->params.height, obj);
    c->temporal.state.baryWith(0, c->deformHistory != 0);
    return 0;
}
int flx_history_capture(flx_ctx *c)
{
    ENTER(c, CALL_OBSERVE);
    HIPCHK(c, hipSetDevice(c->device));
    if (temporalReady(c, "flx_history_capture")) return 1;
    NEED(c, c->temporal.gb[0] && c->temporal.state.holds(0), "flx_history_capture: no G-buffer has been traced for the current slot (flx_gbuffer first)");
    NEED(c, c->temporal.state.holdsSized(0, c->params.width, c->params.height), "flx_history_capture: the image size differs from the G-buffer's");
    const size_t n = c->fr.localPixels;
    const bool withMom = c->moments && c->fr.moments;
    // (the moments' copy is allocated when first needed; a failed allocation releases slots and history together, so a retry starts clean)
    if ((!c->temporal.hist && dalloc(c, c->temporal.allocs, &c->temporal.hist, n)) || (withMom && !c->temporal.histMomBuf && dalloc(c, c->temporal.allocs, &c->temporal.histMomBuf, n))) {
        const std::string why = c->err; c->temporal.release(); c->err = "flx_history_capture: " + why; return 1;
    }
    HIPCHK(c, hipMemcpyAsync(c->temporal.hist, c->fr.pixels, n * 16, hipMemcpyDeviceToDevice, c->stream));
    if (withMom) HIPCHK(c, hipMemcpyAsync(c->temporal.histMomBuf, c->fr.moments, n * 16, hipMemcpyDeviceToDevice, c->stream));
    std::swap(c->temporal.gb[0], c->temporal.gb[1]);
    std::swap(c->temporal.objPlane[0], c->temporal.objPlane[1]);
    std::swap(c->temporal.baryPlane[0], c->temporal.baryPlane[1]);
    c->temporal.state.captured(withMom);
    c->ob.pose.captured();
    return 0;
}
int flx_reproject(flx_ctx *c, const flx_reproject_params *pp)
{
    ENTER(c, CALL_OBSERVE);
    HIPCHK(c, hipSetDevice(c->device));
    if (temporalReady(c, "flx_reproject")) return 1;
    rp_params rp = {FLX_RP_DEFAULT_MAX_HISTORY, FLX_RP_DEFAULT_PLANE_TOLERANCE_PX, FLX_RP_DEFAULT_NORMAL_COS, FLX_RP_DEFAULT_MIN_WEIGHT};
    if (pp) { rp.max_history = pp->max_history; rp.plane_tolerance_px = pp->plane_tolerance_px; rp.normal_cos = pp->normal_cos; rp.min_weight = pp->min_weight; }
    NEED(c, rp_params_ok(rp), "flx_reproject: parameters must be finite with max_history >= 1, plane_tolerance_px > 0, normal_cos in [-1, 1], min_weight in (0, 1]");
    const TemporalState &ts = c->temporal.state;
    NEED(c, ts.hasHistory(), "flx_reproject: no captured history (flx_history_capture first)");
    NEED(c, ts.holds(0), "flx_reproject: no G-buffer has been traced for the current camera (flx_gbuffer first)");
    NEED(c, ts.historyFits(c->params.width, c->params.height), "flx_reproject: the image size changed between the capture and the reprojection");
    const flx_camera &pc = ts.slot[1].cam;
    const rp_view vw = rp_make_view(mk3(pc.pos.x, pc.pos.y, pc.pos.z), mk3(pc.dir.x, pc.dir.y, pc.dir.z), mk3(pc.up.x, pc.up.y, pc.up.z), mk3(pc.right.x, pc.right.y, pc.right.z), pc.fov, ts.slot[0].cam.fov, (int)c->params.width, (int)c->params.height);
    const bool mom = c->moments && c->fr.moments && ts.histMom;
    // objects posed since the capture (only flx_objects_pose under "motion_history" keeps a history across a move of triangles): the motion-aware
    // kernel with the table of flx_reproject_motion.h, nobjects x 64 bytes uploaded on the stream; no object moved: k_reproject as ever
    // triangles moved since the capture under "deform_history" (api_refit.hip took the snapshot first): the flags, then the per-vertex kernel of
    // flx_reproject_deform.h.  No read decides between kernels: with nothing moved its result is k_reproject's bit for bit.
    const bool deform = ts.followsMoves();
    if (deform)
        NEED(c, c->deformHistory && c->rf.snapPos && c->rf.movedFlags && c->temporal.baryPlane[0] && ts.followsMovesReady(),
             "flx_reproject: triangles moved since the capture: needs option \"deform_history\" on and both G-buffers traced with it (flx_gbuffer)");
    flx_ctx::Objects &ob = c->ob;
    bool moved = false;
    std::vector<rm_row> table;
    if (!deform && ob.have && ob.t.nobjects) {        // (under "deform_history" a pose is a move of triangles like any other: the snapshot follows it)
        table.resize((size_t)ob.t.nobjects * FLX_RM_ROWS);
        const PoseState::Poses p = ob.pose.sinceCapture();
        moved = rm_make_table(ob.t.nobjects, p.atCapture, p.atCaptureKnown, p.now, p.nowKnown, table.data());
    }
    if (moved) {
        NEED(c, c->motionHistory && ob.motion && ts.holdsObjects(0) && ts.holdsObjects(1),
             "flx_reproject: objects were posed since the capture: needs option \"motion_history\" on and both G-buffers traced with it (flx_gbuffer)");
        memcpy(ob.motionPinned, table.data(), table.size() * sizeof(rm_row));
        HIPCHK(c, hipMemcpyAsync(ob.motion, ob.motionPinned, table.size() * sizeof(rm_row), hipMemcpyHostToDevice, c->stream));
    }
    { ScopedTimer t(c, FLX_K_REPROJECT);
      float4 *px = reinterpret_cast<float4 *>(c->fr.pixels), *pm = mom ? reinterpret_cast<float4 *>(c->fr.moments) : nullptr;
      if (deform) {
          launch_moved_flags(c->stream, c->sc, c->rf.ntris, c->rf.snapPos, c->rf.movedFlags);
          launch_reproject_deform(c->stream, vw, rp, c->temporal.gb[0], c->temporal.gb[1], c->temporal.hist, c->temporal.histMomBuf, px, pm,
                                  c->temporal.baryPlane[0], c->temporal.baryPlane[1], c->sc, c->rf.ntris, c->rf.snapPos, c->rf.movedFlags);
      } else if (moved) launch_reproject_motion(c->stream, vw, rp, c->temporal.gb[0], c->temporal.gb[1], c->temporal.hist, c->temporal.histMomBuf, px, pm,
                                         c->temporal.objPlane[0], c->temporal.objPlane[1], ob.motion, ob.t.nobjects);
      else launch_reproject(c->stream, vw, rp, c->temporal.gb[0], c->temporal.gb[1], c->temporal.hist, c->temporal.histMomBuf, px, pm); }
    LAUNCHED(c);
    return 0;
}
// ---- history rectification (csrc/flx_rectify.h, rectify.hip): the mark and the test of the new samples against it.  Like the
// calls above: an unpartitioned context, CALL_OBSERVE, no path state, queue or counter.
int flx_history_mark(flx_ctx *c)
{
    ENTER(c, CALL_OBSERVE);
    HIPCHK(c, hipSetDevice(c->device));
    if (temporalReady(c, "flx_history_mark")) return 1;
    NEED(c, c->temporal.gb[0] && c->temporal.state.holdsSized(0, c->params.width, c->params.height),
         "flx_history_mark: no G-buffer of the current size has been traced for the current slot (flx_gbuffer first)");
    flx_ctx::Temporal &t = c->temporal;
    const size_t n = c->fr.localPixels;
    const bool withMom = c->moments && c->fr.moments;
    // (a failed allocation releases slots, history and mark together, so a retry starts clean: as flx_history_capture)
    if ((!t.mark && (dalloc(c, t.allocs, &t.mark, n) || dalloc(c, t.allocs, &t.rcRec, n) || dalloc(c, t.allocs, &t.lambda, n))) ||
        (withMom && !t.markMomBuf && dalloc(c, t.allocs, &t.markMomBuf, n))) {
        const std::string why = c->err; t.release(); c->err = "flx_history_mark: " + why; return 1;
    }
    HIPCHK(c, hipMemcpyAsync(t.mark, c->fr.pixels, n * 16, hipMemcpyDeviceToDevice, c->stream));
    if (withMom) HIPCHK(c, hipMemcpyAsync(t.markMomBuf, c->fr.moments, n * 16, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(t.lambda, 0, n * 4, c->stream));      // no flx_history_rectify has looked at this mark
    t.state.marked(withMom);
    return 0;
}
int flx_history_rectify(flx_ctx *c, const flx_rectify_params *pp)
{
    ENTER(c, CALL_OBSERVE);
    HIPCHK(c, hipSetDevice(c->device));
    if (temporalReady(c, "flx_history_rectify")) return 1;
    rc_params rc = rc_defaults();
    if (pp) { rc.radius = pp->radius; rc.gamma = pp->gamma; rc.sensitivity = pp->sensitivity; rc.lum_floor = pp->lum_floor; rc.min_pixels = pp->min_pixels;
              rc.plane_tolerance_px = pp->plane_tolerance_px; rc.normal_cos = pp->normal_cos; }
    NEED(c, rc_params_ok(rc), "flx_history_rectify: parameters must be finite with radius in 1..4, gamma >= 0, sensitivity > 0, lum_floor >= 0, "
                              "min_pixels in 1..(2 radius + 1)^2, plane_tolerance_px > 0, normal_cos in [-1, 1]");
    flx_ctx::Temporal &t = c->temporal;
    const TemporalState &ts = t.state;
    NEED(c, ts.hasMark() && t.mark && t.rcRec && t.lambda, "flx_history_rectify: no mark (flx_history_mark first)");
    NEED(c, ts.markLive() && t.gb[0] && ts.holdsSized(0, c->params.width, c->params.height),
         "flx_history_rectify: the current slot holds no G-buffer of the mark's size (flx_gbuffer)");
    const bool mom = c->moments && c->fr.moments && ts.markHasMoments() && t.markMomBuf;
    const int W = (int)c->params.width, H = (int)c->params.height;
    { ScopedTimer tm(c, FLX_K_RECTIFY);
      launch_rectify(c->stream, rc, rc_footprint(ts.slot[0].cam.fov, H), W, H, t.gb[0], t.rcRec, reinterpret_cast<float4 *>(c->fr.pixels), t.mark,
                     mom ? reinterpret_cast<float4 *>(c->fr.moments) : nullptr, mom ? t.markMomBuf : nullptr, t.lambda); }
    LAUNCHED(c);
    return 0;
}
// test hook: the mark (4 floats per pixel), its moments (refused when the mark has none) and lambda as the last flx_history_rectify since the
// mark left it (1 float per pixel; zeros before one).  Any output may be null.  Blocking.
int flx_history_mark_read(flx_ctx *c, float *out_mark4, float *out_mark_mom4, float *out_lambda)
{
    ENTER(c, CALL_OBSERVE);
    HIPCHK(c, hipSetDevice(c->device));
    if (temporalReady(c, "flx_history_mark_read")) return 1;
    flx_ctx::Temporal &t = c->temporal;
    NEED(c, t.state.hasMark() && t.mark && t.lambda, "flx_history_mark_read: no mark (flx_history_mark first)");
    NEED(c, !out_mark_mom4 || (t.state.markHasMoments() && t.markMomBuf), "flx_history_mark_read: the mark holds no moments (option \"moments\" was off at flx_history_mark)");
    const size_t n = (size_t)t.state.markW * t.state.markH;
    if (out_mark4) HIPCHK(c, hipMemcpyAsync(out_mark4, t.mark, n * 16, hipMemcpyDeviceToHost, c->stream));
    if (out_mark_mom4) HIPCHK(c, hipMemcpyAsync(out_mark_mom4, t.markMomBuf, n * 16, hipMemcpyDeviceToHost, c->stream));
    if (out_lambda) HIPCHK(c, hipMemcpyAsync(out_lambda, t.lambda, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
// test hooks in the spirit of flx_state_import: slot 0 = current, 1 = previous; 8 floats per pixel (G0, G1) and the slot's 80-byte camera.  Blocking.
int flx_gbuffer_read(flx_ctx *c, int slot, float *out8, void *camera80)
{
    ENTER(c, CALL_OBSERVE);
    HIPCHK(c, hipSetDevice(c->device));
    NEED(c, slot == 0 || slot == 1, "flx_gbuffer_read: slot must be 0 (current) or 1 (previous)");
    NEED(c, out8, "flx_gbuffer_read: null output");
    NEED(c, c->temporal.gb[slot] && c->temporal.state.holds(slot), "flx_gbuffer_read: the slot holds no G-buffer");
    const TemporalState::Slot &s = c->temporal.state.slot[slot];
    HIPCHK(c, hipMemcpyAsync(out8, c->temporal.gb[slot], (size_t)s.W * s.H * 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (camera80) memcpy(camera80, &s.cam, sizeof(flx_camera));
    return 0;
}
int flx_gbuffer_write(flx_ctx *c, int slot, const float *in8, const void *camera80)
{
    ENTER(c, CALL_OBSERVE);
    HIPCHK(c, hipSetDevice(c->device));
    NEED(c, slot == 0 || slot == 1, "flx_gbuffer_write: slot must be 0 (current) or 1 (previous)");
    NEED(c, in8 && camera80, "flx_gbuffer_write: null G-buffer or camera");
    if (temporalReady(c, "flx_gbuffer_write") || gbufferSlots(c)) return 1;
    HIPCHK(c, hipMemcpyAsync(c->temporal.gb[slot], in8, (size_t)c->fr.localPixels * 32, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->motionHistory) {                               // a written G-buffer shows no object until flx_gbuffer_objects_write says otherwise
        HIPCHK(c, hipMemsetAsync(c->temporal.objPlane[slot], 0xFF, (size_t)c->fr.localPixels * 4, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    if (c->deformHistory) {                               // ... and names no triangle until flx_gbuffer_bary_write says otherwise
        const std::vector<float> none((size_t)c->fr.localPixels * 2, FLX_RD_NO_BARY);
        HIPCHK(c, hipMemcpyAsync(c->temporal.baryPlane[slot], none.data(), none.size() * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    flx_camera cam; memcpy(&cam, camera80, sizeof(flx_camera));
    c->temporal.state.written(slot, cam, c->params.width, c->params.height, c->motionHistory);
    c->temporal.state.baryWith(slot, c->deformHistory != 0);
    return 0;
}
// ... and of the slots' object planes (option "motion_history"): one uint32 per pixel, FLX_NO_OBJECT or an object id (an id that is not below
// the object count is read as FLX_NO_OBJECT, csrc/flx_reproject_motion.h).  Blocking.
int flx_gbuffer_objects_read(flx_ctx *c, int slot, uint32_t *out)
{
    ENTER(c, CALL_OBSERVE);
    HIPCHK(c, hipSetDevice(c->device));
    NEED(c, slot == 0 || slot == 1, "flx_gbuffer_objects_read: slot must be 0 (current) or 1 (previous)");
    NEED(c, out, "flx_gbuffer_objects_read: null output");
    NEED(c, c->temporal.objPlane[slot] && c->temporal.state.holdsObjects(slot),
         "flx_gbuffer_objects_read: the slot holds no object plane (option \"motion_history\" on, objects defined, flx_gbuffer)");
    const TemporalState::Slot &s = c->temporal.state.slot[slot];
    HIPCHK(c, hipMemcpyAsync(out, c->temporal.objPlane[slot], (size_t)s.W * s.H * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
int flx_gbuffer_objects_write(flx_ctx *c, int slot, const uint32_t *in)
{
    ENTER(c, CALL_OBSERVE);
    HIPCHK(c, hipSetDevice(c->device));
    NEED(c, slot == 0 || slot == 1, "flx_gbuffer_objects_write: slot must be 0 (current) or 1 (previous)");
    NEED(c, in, "flx_gbuffer_objects_write: null object ids");
    NEED(c, c->motionHistory, "flx_gbuffer_objects_write: needs flx_set_option(ctx, \"motion_history\", 1)");
    if (temporalReady(c, "flx_gbuffer_objects_write")) return 1;
    NEED(c, c->temporal.gb[slot] && c->temporal.state.holdsSized(slot, c->params.width, c->params.height),
         "flx_gbuffer_objects_write: the slot holds no G-buffer of the current size (flx_gbuffer or flx_gbuffer_write first)");
    if (gbufferSlots(c)) return 1;
    HIPCHK(c, hipMemcpyAsync(c->temporal.objPlane[slot], in, (size_t)c->fr.localPixels * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->temporal.state.objectsWritten(slot);
    return 0;
}

// ... and of the slots' barycentric planes (option "deform_history"): two floats per pixel, (u, v) of the hit or (-1, -1) where the pixel names
// no triangle (csrc/flx_reproject_deform.h).  Blocking.
int flx_gbuffer_bary_read(flx_ctx *c, int slot, float *out2)
{
    ENTER(c, CALL_OBSERVE);
    HIPCHK(c, hipSetDevice(c->device));
    NEED(c, slot == 0 || slot == 1, "flx_gbuffer_bary_read: slot must be 0 (current) or 1 (previous)");
    NEED(c, out2, "flx_gbuffer_bary_read: null output");
    NEED(c, c->temporal.baryPlane[slot] && c->temporal.state.holdsBary(slot),
         "flx_gbuffer_bary_read: the slot holds no barycentric plane (option \"deform_history\" on, flx_gbuffer)");
    const TemporalState::Slot &s = c->temporal.state.slot[slot];
    HIPCHK(c, hipMemcpyAsync(out2, c->temporal.baryPlane[slot], (size_t)s.W * s.H * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
int flx_gbuffer_bary_write(flx_ctx *c, int slot, const float *in2)
{
    ENTER(c, CALL_OBSERVE);
    HIPCHK(c, hipSetDevice(c->device));
    NEED(c, slot == 0 || slot == 1, "flx_gbuffer_bary_write: slot must be 0 (current) or 1 (previous)");
    NEED(c, in2, "flx_gbuffer_bary_write: null barycentrics");
    NEED(c, c->deformHistory, "flx_gbuffer_bary_write: needs flx_set_option(ctx, \"deform_history\", 1)");
    if (temporalReady(c, "flx_gbuffer_bary_write")) return 1;
    NEED(c, c->temporal.gb[slot] && c->temporal.state.holdsSized(slot, c->params.width, c->params.height),
         "flx_gbuffer_bary_write: the slot holds no G-buffer of the current size (flx_gbuffer or flx_gbuffer_write first)");
    if (gbufferSlots(c)) return 1;
    HIPCHK(c, hipMemcpyAsync(c->temporal.baryPlane[slot], in2, (size_t)c->fr.localPixels * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->temporal.state.baryWritten(slot);
    return 0;
}
// ... and of the snapshot: the nine position floats of every triangle at the capture and -- computed now, as flx_reproject would -- one moved byte
// per triangle.  Either output may be null.  Blocking; fails when no move has snapshotted since the last capture.
int flx_deform_read(flx_ctx *c, float *out9, uint8_t *out_moved)
{
    ENTER(c, CALL_OBSERVE);
    HIPCHK(c, hipSetDevice(c->device));
    NEED(c, c->sc.bnodes, "flx_deform_read: upload a scene first (flx_upload_scene)");
    NEED(c, c->temporal.state.followsMoves() && c->rf.snapPos && c->rf.movedFlags,
         "flx_deform_read: no snapshot (option \"deform_history\" on, flx_gbuffer, flx_history_capture, then a move of triangles)");
    const size_t n = c->rf.ntris;
    if (out9) {
        std::vector<float> v4(n * FLX_RD_SNAP_V4 * 4);
        HIPCHK(c, hipMemcpyAsync(v4.data(), c->rf.snapPos, v4.size() * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (size_t i = 0; i < n * 3; i++) memcpy(out9 + 3 * i, &v4[4 * i], 12);
    }
    if (out_moved) {
        { ScopedTimer t(c, FLX_K_MOVED_FLAGS); launch_moved_flags(c->stream, c->sc, c->rf.ntris, c->rf.snapPos, c->rf.movedFlags); }
        LAUNCHED(c);
        HIPCHK(c, hipMemcpyAsync(out_moved, c->rf.movedFlags, n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return 0;
}

// ---- microkernel integrator.  One path per pixel, framebuffers indexed by the path id: single-GPU only, the pixel
// partition belongs to the wavefront path (allocFrame sizes the buffers for the rank's LOCAL pixels).
#define MK_READY(c) do { READY(c, CALL_OBSERVE); NEED(c, (c)->fr.nranks == 1, "the microkernel integrator is single-GPU: flx_set_partition(ctx, 0, 1) first"); } while (0)
int flx_mk_reset(flx_ctx *c) { MK_READY(c); c->ad.state.dropped(); c->temporal.state.accumulationReset(); launch_mk_reset(c->stream, c->st, c->fr, c->params); LAUNCHED(c); return 0; }
// with a list of active pixels installed (flx_mk_adaptive_update / flx_mk_active_write) the four kernels of a sample pass run their list-driven
// instances over it; an empty list makes them no-ops (microkernel.hip: mk_dispatch).  With option "mesh_lights" and emissive triangles the two
// kernels that see lights run their MESH instances.
static const uint32_t *mkList(const flx_ctx *c) { return c->ad.state.have ? c->ad.list : nullptr; }
static const MeshLights *mkLamps(const flx_ctx *c) { return c->ml.state.lit() ? &c->ml.t : nullptr; }
int flx_mk_raygen(flx_ctx *c) { MK_READY(c); launch_mk_raygen(c->stream, c->st, c->params, mkList(c), c->ad.state.count); LAUNCHED(c); return 0; }
int flx_mk_next_vertex(flx_ctx *c)
{
    MK_READY(c);
    launch_mk_next_vertex(c->stream, c->st, c->sc, c->fr, c->params, c->spill, c->mkStats, mkList(c), c->ad.state.count, mkLamps(c));
    LAUNCHED(c); return 0;
}
int flx_mk_sample_bsdf(flx_ctx *c)
{
    MK_READY(c);
    launch_mk_sample_bsdf(c->stream, c->st, c->sc, c->fr, c->params, c->spill, c->mkStats, mkList(c), c->ad.state.count, mkLamps(c));
    LAUNCHED(c); return 0;
}
int flx_mk_splat(flx_ctx *c) { MK_READY(c); launch_mk_splat(c->stream, c->st, c->fr, c->params, c->mkStats, 0, mkList(c), c->ad.state.count); LAUNCHED(c); return 0; }
int flx_mk_splat_preview(flx_ctx *c) { MK_READY(c); launch_mk_splat(c->stream, c->st, c->fr, c->params, c->mkStats, 1, nullptr, 0u); LAUNCHED(c); return 0; }

// ---- adaptive sampling (adaptive.hip, csrc/flx_adaptive.h)
static int adaptiveReady(flx_ctx *c, const char *fn)
{
    NEED(c, c->fr.nranks == 1, std::string(fn) + ": the microkernel integrator is single-GPU: flx_set_partition(ctx, 0, 1) first");
    const uint64_t npix = (uint64_t)c->params.width * c->params.height;
    NEED(c, npix <= c->numTasks, std::string(fn) + ": needs one path per pixel: width * height <= num_tasks");
    if (c->ad.state.pix != (uint32_t)npix || !c->ad.list) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->ad.release();
        if (dalloc(c, c->ad.allocs, &c->ad.flags, (size_t)npix) || dalloc(c, c->ad.allocs, &c->ad.scratch, (size_t)adaptive_blocks((uint32_t)npix)) ||
            dalloc(c, c->ad.allocs, &c->ad.list, (size_t)npix) || dalloc(c, c->ad.allocs, &c->ad.countDev, 1)) { c->ad.release(); return 1; }
        c->ad.state.pix = (uint32_t)npix;
    }
    return 0;
}
int flx_mk_adaptive_update(flx_ctx *c, const flx_adaptive_params *pp, uint32_t *out_active)
{
    READY(c, CALL_OBSERVE);
    NEED(c, c->moments && c->fr.moments, "flx_mk_adaptive_update: needs the luminance moments: flx_set_option(ctx, \"moments\", 1)");
    NEED(c, out_active, "flx_mk_adaptive_update: null output");
    ad_params ap = {FLX_AD_DEFAULT_THRESHOLD, FLX_AD_DEFAULT_MIN_SAMPLES, FLX_AD_DEFAULT_MAX_SAMPLES, FLX_AD_DEFAULT_LUM_FLOOR, FLX_AD_DEFAULT_DILATE};
    if (pp) { ap.threshold = pp->threshold; ap.min_samples = pp->min_samples; ap.max_samples = pp->max_samples; ap.lum_floor = pp->lum_floor; ap.dilate = pp->dilate; }
    NEED(c, ad_params_ok(ap), "flx_mk_adaptive_update: threshold and lum_floor must be finite and >= 0, 1 <= max_samples <= 2^24, min_samples <= max_samples, dilate 0 or 1");
    if (adaptiveReady(c, "flx_mk_adaptive_update")) return 1;
    launch_adaptive_update(c->stream, reinterpret_cast<const float4 *>(c->fr.moments), (int)c->params.width, (int)c->params.height, ap, c->ad.flags, c->ad.scratch,
                           c->ad.list, c->ad.countDev);
    LAUNCHED(c);
    uint32_t n = 0;
    HIPCHK(c, hipMemcpyAsync(&n, c->ad.countDev, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    NEED(c, n <= c->ad.state.pix, "flx_mk_adaptive_update: the device returned an impossible count");
    c->ad.state.installed(n);
    *out_active = n;
    return 0;
}
int flx_mk_adaptive_clear(flx_ctx *c) { ENTER(c, CALL_OBSERVE); c->ad.state.dropped(); return 0; }
// test hooks in the spirit of flx_gbuffer_read / flx_gbuffer_write.  Blocking.
int flx_mk_active_read(flx_ctx *c, uint32_t *out_list, uint32_t *out_count, uint8_t *out_flags)
{
    ENTER(c, CALL_OBSERVE);
    HIPCHK(c, hipSetDevice(c->device));
    NEED(c, out_count, "flx_mk_active_read: null count");
    NEED(c, c->ad.state.have, "flx_mk_active_read: no list of active pixels is installed");
    *out_count = c->ad.state.count;
    if (out_list && c->ad.state.count) HIPCHK(c, hipMemcpyAsync(out_list, c->ad.list, (size_t)c->ad.state.count * 4, hipMemcpyDeviceToHost, c->stream));
    if (out_flags) HIPCHK(c, hipMemcpyAsync(out_flags, c->ad.flags, (size_t)c->ad.state.pix, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
int flx_mk_active_write(flx_ctx *c, const uint32_t *in_list, uint32_t n)
{
    READY(c, CALL_OBSERVE);
    NEED(c, in_list || !n, "flx_mk_active_write: null list");
    const uint64_t npix = (uint64_t)c->params.width * c->params.height;
    NEED(c, n <= npix, "flx_mk_active_write: more entries than pixels");
    for (uint32_t i = 0; i < n; i++) {
        NEED(c, in_list[i] < npix, "flx_mk_active_write: pixel index out of range");
        NEED(c, i == 0 || in_list[i] > in_list[i - 1], "flx_mk_active_write: the list must be strictly ascending");
    }
    if (adaptiveReady(c, "flx_mk_active_write")) return 1;
    HIPCHK(c, hipMemsetAsync(c->ad.flags, 0, c->ad.state.pix, c->stream));       // (the flags describe a classification; a written list has none)
    if (n) HIPCHK(c, hipMemcpyAsync(c->ad.list, in_list, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->ad.state.installed(n);
    return 0;
}

int flx_mk_stats_async(flx_ctx *c, void *out16)
{
    ENTER(c, CALL_OBSERVE);
    NEED(c, out16, "flx_mk_stats_async: null");
    HIPCHK(c, hipSetDevice(c->device));
    if ((int)c->pendingMk.size() >= c->pinnedSlots) { c->err = "too many outstanding stats reads; call flx_finish"; return 1; }
    int slot = c->nextMkSlot; c->nextMkSlot = (c->nextMkSlot + 1) % c->pinnedSlots;
    HIPCHK(c, hipMemcpyAsync(c->pinnedMk + 4 * slot, c->mkStats, 16, hipMemcpyDeviceToHost, c->stream));
    c->pendingMk.push_back({out16, slot});
    return 0;
}
int flx_mk_stats_reset(flx_ctx *c) { ENTER(c, CALL_OBSERVE); HIPCHK(c, hipSetDevice(c->device)); HIPCHK(c, hipMemsetAsync(c->mkStats, 0, 16, c->stream)); return 0; }

} // extern "C"
