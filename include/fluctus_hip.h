/*
 * fluctus_hip.h -- C ABI of libfluctus_hip.so, the MI355X (gfx950) implementation of the
 * wavefront path-tracing hot path.
 *
 * This is the drop-in boundary: every entry point replaces one method of the reference's device
 * context `class CLContext` (reference: src/clcontext.hpp:26-211, src/clcontext.cpp), the only
 * object `Tracer` talks to for device work.  Plain pointers and sizes; no C++ or torch types.
 * All functions return 0 on success and non-zero on failure (message: flx_last_error()); nothing
 * throws or exits across the boundary (reference behaviour: clt::check() aborts,
 * src/clcontext.cpp:931-936).
 *
 * Threading/ordering (same contract as the reference's single in-order cl::CommandQueue,
 * src/clcontext.cpp:25-29): one host thread per context; every flx_wf_*, flx_clear_queues,
 * flx_get_counters_async, flx_set_params, flx_pixel_index_* call is ASYNCHRONOUS and executes in
 * issue order on the context's HIP stream; flx_finish() is the only synchronisation point
 * (uploads and the read-back helpers are blocking).  Inputs are copied; the caller keeps ownership.
 *
 * Wire formats: include/fluctus_wire.h.
 */
#ifndef FLUCTUS_HIP_H
#define FLUCTUS_HIP_H

#include <stdint.h>
#include <stddef.h>
#include "fluctus_wire.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct flx_ctx flx_ctx;

/* CLContext::CLContext + setup (src/clcontext.cpp:18-69): pick HIP device `device`, create the
 * stream, allocate path state for `num_tasks` paths (Settings wfBufferSize, src/settings.cpp:20)
 * and the 8 index queues + counters (src/clcontext.cpp:116-141). */
int flx_create(int device, uint32_t num_tasks, flx_ctx **out);
int flx_destroy(flx_ctx *ctx);
/* last error text of this context (or of flx_create when ctx == NULL) */
const char *flx_last_error(flx_ctx *ctx);

/* CLContext::uploadSceneData + packTextures (src/clcontext.cpp:522-611).  Takes the reference's
 * wire arrays (160-B triangles, u32 index list, 48-B nodes, 80-B materials, 12-B texture
 * descriptors + RGBA8 blob) and re-lays them out for CDNA4 on the device. */
int flx_upload_scene(flx_ctx *ctx, const void *tris, size_t ntris, const uint32_t *indices, size_t nidx,
                     const void *nodes, size_t nnodes, const void *materials, size_t nmat,
                     const void *texdesc, size_t ntex, const uint8_t *texdata, size_t texbytes);

/* Moving the triangles of the uploaded scene (no counterpart in the reference, which rebuilds and re-uploads, src/tracer.cpp:574-590;
 * csrc/flx_refit.h, csrc/refit.hip -- its passes with every record dirty --): replaces every triangle by the `ntris` 160-byte wire triangles given -- positions, normals,
 * uvs, matId -- and REFITS both traversal trees on the device: new leaf triangle records, shading records and boxes; the index list, the
 * topology of both trees, materials, textures and the environment map stay as uploaded.  A leaf box becomes the union of the full bounds of its
 * triangles (a leaf an SBVH spatial split had clipped becomes unclipped: correct, only looser) and traversal quality decays as the geometry
 * leaves the shape the tree was built for: rebuild (flx_upload_scene) when that matters.  tris160: host memory, or device memory (16-byte
 * aligned) when src_on_device != 0.  Flushes deferred and fused launches against the OLD scene first; clears the adaptive list and marks the
 * G-buffer slots and the captured history of the temporal reprojection not traced; touches no path state, queue or counter; allocates nothing
 * after the first call with a host source.  One small blocking read (the validation), then asynchronous on the context stream, timed under
 * FLX_K_REFIT.  Fails -- and leaves the old scene in place, untouched -- when no scene is uploaded, ntris differs from the uploaded count, a
 * position is not finite or beyond +-2^62 (FLX_WIDE_COORD_MAX), or a matId is outside the uploaded materials. */
int flx_update_triangles(flx_ctx *ctx, const void *tris160, size_t ntris, int src_on_device);
/* Moving a SUBSET of the triangles (a dragged object; csrc/refit.hip -- the same passes in their SUBSET mode --): tris160[k] is the new 160-byte wire triangle for
 * triangle indices[k] of the uploaded scene -- positions, normals, uvs and matId may all change.  Only what hangs above the listed triangles is
 * rewritten: their shading records and leaf triangle records, the headers of the wide leaf blocks holding one (the union of the full bounds of the
 * block's triangles), the halves of the binary records and the 4-wide nodes with such a leaf below them.  EVERY OTHER BYTE of the five
 * flx_tree_read arrays stays as it was, so an SBVH leaf a spatial split had clipped stays clipped unless one of its own triangles is listed (moving
 * a triangle back does not re-clip its leaves).  Both pointers are host memory, or device memory when src_on_device != 0 (tris160 16-byte,
 * indices 4-byte aligned).  The boundary is flx_update_triangles' (one function, csrc/api_refit.hip): flushes deferred and fused launches against the OLD scene first, clears the
 * adaptive list, marks the G-buffer slots and the captured history not traced, touches no path state, queue or counter, keeps what the upload
 * chose; allocates only at its first call (stamps; the staging buffers at the first call with a host source), one small blocking read (the
 * validation), timed under FLX_K_REFIT.  The wide node test's clamp is re-derived from the whole resulting triangle set (read-only option
 * "wide_far").  Fails -- before anything is overwritten -- when no scene is uploaded, count exceeds the uploaded triangle count, a pointer is
 * null while count > 0, indices is not strictly ascending (duplicates included) or holds an index outside the uploaded triangles, a position
 * is not finite or beyond +-2^62, or a matId is outside the uploaded materials.  count == 0 is accepted and changes no byte of any tree. */
int flx_update_triangles_subset(flx_ctx *ctx, const void *tris160, const uint32_t *indices, size_t count, int src_on_device);
/* Moving OBJECTS by their transforms (csrc/pose.hip, csrc/flx_pose.h).  flx_objects_define, once per upload: host pointers;
 * tris160_rest are the ntris wire triangles of the REST pose (ntris must be the uploaded count), object_of_triangle[i] < nobjects is the object
 * triangle i belongs to, FLX_NO_OBJECT a triangle that never moves; an object without a triangle is legal.  The members and their rest triangles
 * are kept on the device.  Blocking; changes no byte of any tree; replaces an earlier definition; nobjects == 0 drops it, and so does
 * flx_upload_scene.  Fails -- and keeps the earlier definition -- when no scene is uploaded, ntris differs from the uploaded count, a pointer is
 * null or an id is neither < nobjects nor FLX_NO_OBJECT.
 * flx_objects_pose: xforms12 + 12 k is the 3 x 4 row-major affine transform [M | t] of object object_ids[k] (host pointers, ids strictly
 * ascending and < nobjects) -- the ABSOLUTE rest -> world transform, not an increment: a pose is computed from the rest triangles every time, so
 * nothing drifts and posing by Y after X gives what Y alone gives.  Objects not listed keep the pose they have.  Positions go through [M | t],
 * normals through the cofactor matrix of M (turned round when det M < 0) and are renormalised; texcoords, matId and every spare word are the rest
 * triangle's (the arithmetic, operation by operation: csrc/flx_pose.h).  The triangles are produced on the device -- 48 bytes per object cross
 * the bus, not 160 per triangle -- and handed to flx_update_triangles_subset as a device source, whose boundary this call has word for word:
 * deferred and fused launches run against the OLD scene first, the one small blocking read of the validation refuses a posed vertex that is not
 * finite or beyond +-2^62 before anything is overwritten, the adaptive list and the reprojection history are dropped (the history is kept under
 * option "motion_history", see flx_reproject), "wide_far" is re-derived;
 * timed under FLX_K_REFIT (two spans: the pose kernels, the refit).  The identity transform gives back the rest triangles (csrc/flx_pose.h says
 * exactly when bit for bit) but does not re-clip a leaf an earlier pose has unclipped.  count == 0, or a list of objects without triangles,
 * changes no byte.  Fails -- leaving trees and every object's pose as they were -- when no objects are defined, an id is out of range or the ids
 * are not strictly ascending, a matrix entry is not finite, or the fp32 determinant of M (csrc/flx_pose.h) is zero or not finite.
 * flx_objects_read: test hook, blocking.  *out_nobjects, and where not NULL out_counts[nobjects] = the triangles of each object and out_members =
 * the device's list of all objects' triangles, ascending (room for the uploaded triangle count); fails when no objects are defined. */
#define FLX_NO_OBJECT 0xFFFFFFFFu
int flx_objects_define(flx_ctx *ctx, const void *tris160_rest, size_t ntris, const uint32_t *object_of_triangle, uint32_t nobjects);
int flx_objects_pose(flx_ctx *ctx, const uint32_t *object_ids, const float *xforms12, uint32_t count);
int flx_objects_read(flx_ctx *ctx, uint32_t *out_counts, uint32_t *out_nobjects, uint32_t *out_members);
/* Emissive triangles as lights (csrc/flx_mesh_light.h, csrc/mesh_light.hip): flx_set_option(ctx, "mesh_lights", 1), default 0,
 * readable through flx_get_option.  While it is on, every triangle whose material has a Ke component > 0 is a one-sided light (it emits Ke on the
 * side its geometric normal (p1 - p0) x (p2 - p0) faces) for the MICROKERNEL integrator: flx_mk_next_vertex collects the emission of a hit,
 * flx_mk_sample_bsdf samples one light per vertex from a table by power (area x luminance(Ke)), both MIS-weighted as the parametric quad is; the
 * list-driven (adaptive) instances do the same.  The table is built on the stream when the option is switched on and rebuilt at the end of every
 * call that moves triangles -- flx_upload_scene, flx_update_triangles, flx_update_triangles_subset, flx_objects_pose -- so the next sample sees the
 * lamps where and as large as they are.  The option survives flx_upload_scene.  With the option off, or on with no emissive triangle, every entry
 * point launches the kernels it launches without it and returns the same bits.  THE flx_wf_* CALLS IGNORE THIS OPTION ALONE: the wavefront integrator
 * sees emissive triangles only with the second option below.
 * flx_set_option(ctx, "mesh_lights_wavefront", 1), default 0, readable through flx_get_option: the wavefront integrator sees the
 * lamps too.  Inert unless "mesh_lights" is on and the scene has an emissive triangle; the two options may be set in either order, and both survive
 * flx_upload_scene.  While it takes effect, flx_wf_logic runs the MESH instance of the plain logic pass: the lamps are a third kind of light in the
 * one-draw light choice (probability 1 / (useEnvMap + useAreaLight + 1) each kind), sampled into the usual light-sample columns, and an implicit hit
 * on a lamp adds its Ke with the MIS weight of that pdf and does not end the path; an implicit hit on the environment map is weighed the same way,
 * lastPdfW / (lastPdfW + pdf * kind probability), not with the reference's weight, which loses environment light once a second kind exists.
 * COST: the chain is the unfused one whatever "fuse" says ("fuse" still reads back what was set) -- flx_wf_logic does not defer, RAW hit records are committed first, flx_wf_materials launches the separate
 * material kernels.  Off, or on without lamps, every flx_wf_* call launches what it launches without it and returns the same bits.
 * flx_mesh_lights_read, blocking: *out_count = the lights listed (0 when their total weight is 0: no lights), and where not NULL (room for the
 * count a first call reported) out_tris = their ascending triangle indices, out_cdf / out_pick = the table, *out_total = the fp64 total weight.
 * flx_mesh_lights_sample: test hook beside flx_math_probe, blocking.  r3 = n triples (pick, r1, r2) of host floats; out_light[i] = the light picked,
 * out8 + 8 i = {P.xyz, pdfA, n_g.xyz, area} of the point sampled on it.  Fails when the table holds no light.
 * Both fail, with a message, while the option is off or no scene is uploaded. */
int flx_mesh_lights_read(flx_ctx *ctx, uint32_t *out_count, uint32_t *out_tris, float *out_cdf, float *out_pick, double *out_total);
int flx_mesh_lights_sample(flx_ctx *ctx, const float *r3, uint32_t n, uint32_t *out_light, float *out8);
/* test hook, blocking: one device array of the uploaded scene as it is now.  which = 0 the binary tree's 64-byte inner-node records, 1 the
 * 48-byte leaf triangle records (index-list order), 2 the 64-byte shading records, 3 the 64-byte nodes of the 4-wide tree, 4 its leaf data
 * (16-byte units).  *needed = the array's size in bytes; out NULL only reports it, otherwise bytes must be at least that. */
int flx_tree_read(flx_ctx *ctx, int which, void *out, size_t bytes, size_t *needed);
/* How far refits have degraded the trees (csrc/flx_tree_cost.h, csrc/tree_cost.hip): the surface-area cost sums of both
 * device trees as they stand now -- after a fresh upload or after any number of flx_update_triangles -- over the records the traversal kernels
 * walk.  out8[0..3] the binary tree, out8[4..7] the 4-wide tree, each {A_root, S_node, S_leaf, S_tri}: the area of the root box; the areas of the
 * boxes tested to enter an inner node (A_root included); the areas of the boxes tested to enter a leaf; per leaf, the area of the last box
 * tested before its triangles (binary: the parent's half; 4-wide: the leaf header's exact box) x its triangle count.  A(box) = 2 (dx dy + dy dz +
 * dz dx) in fp64; a 4-wide slot's box is the quantised one the node test sees.  flxTreeCostValue below turns four sums into one figure; the ratio
 * of that figure to its value right after the upload is what a caller compares with a threshold to decide on a rebuild (Tracer::setRebuildPolicy).
 * Reduced without floating-point atomics: the eight numbers are bit-identical from call to call and from context to context.  Changes no state
 * a render can observe; allocates its partial-sum slab with the scene at the first call; one small blocking read, timed under FLX_K_TREE_COST.
 * Fails when no scene is uploaded or out8 is NULL. */
int flx_tree_cost(flx_ctx *ctx, double out8[8]);

/* CLContext::createEnvMap (src/clcontext.cpp:467-511): RGB float image + alias/prob/pdf tables. */
int flx_upload_envmap(flx_ctx *ctx, const float *rgb, int w, int h, const float *prob, const int *alias, const float *pdf);

/* CLContext::updateParams (src/clcontext.cpp:703-707), 240-byte RenderParams.  A change of
 * width*height re-allocates the framebuffers (CLContext::setupPixelStorage/resizeBuffers). */
int flx_set_params(flx_ctx *ctx, const void *render_params_240);

/* enqueueWfResetKernel / RaygenKernel / ExtRayKernel / ShadowRayKernel / LogicKernel /
 * MaterialKernels (src/clcontext.cpp:765-848).  Kernels: src/wf_reset.cl, wf_raygen.cl,
 * wf_extrays.cl, wf_shadowrays.cl, wf_logic.cl, wf_mat_*.cl.
 * All of them enqueue and return, as the reference's do.  With option "fuse" (default on, see flx_set_option) flx_wf_logic and a
 * flx_wf_raygen directly behind it are enqueued by the NEXT call on the context instead -- together with the material kernels as one
 * pass when that call is flx_wf_materials -- which no other call can tell from immediate launches except by timing. */
int flx_wf_reset(flx_ctx *ctx);
int flx_wf_raygen(flx_ctx *ctx);
int flx_wf_extend(flx_ctx *ctx);
int flx_wf_shadow(flx_ctx *ctx);
int flx_wf_logic(flx_ctx *ctx, int first_iteration);
int flx_wf_materials(flx_ctx *ctx);           /* dispatches on params.wfSeparateQueues */

/* enqueueClearWfQueues (src/clcontext.cpp:877-883) */
int flx_clear_queues(flx_ctx *ctx);
/* enqueueGetCounters (src/clcontext.cpp:668-671): asynchronous 32-byte read; *out32 (a
 * flx_queue_counters) is valid only after the next flx_finish(). */
int flx_get_counters_async(flx_ctx *ctx, void *out32);
/* finishQueue (src/clcontext.cpp:885-889) */
int flx_finish(flx_ctx *ctx);
/* updatePixelIndex / resetPixelIndex (src/clcontext.cpp:891-901) */
int flx_pixel_index_update(flx_ctx *ctx, uint32_t num_pixels, uint32_t num_new_paths);
int flx_pixel_index_reset(flx_ctx *ctx);
/* Device-side end of a benchmark-style iteration (no counterpart in the reference, which needs a
 * host round trip per iteration to move the cursor, src/tracer.cpp:456-462): in stream order,
 * (1) add the 8 queue counters to 64-bit running totals, (2) cursor = (cursor + raygenQueue) %
 * local pixels -- the value updatePixelIndex would write -- and (3) zero the counters
 * (enqueueClearWfQueues).  Lets a caller run K iterations with a single flx_finish(). */
int flx_end_iteration_async(flx_ctx *ctx);
/* running totals accumulated by flx_end_iteration_async (8 x u64, flx_queue_counters order); blocking */
int flx_counter_totals(flx_ctx *ctx, uint64_t *out8, int reset);
/* getNumTasks (src/clcontext.cpp:903-906) */
uint32_t flx_num_tasks(flx_ctx *ctx);

/* enqueuePostprocessKernel (src/clcontext.cpp:750-763; kernel src/mk_postprocess.cl) -- headless:
 * the preview buffer is a plain device buffer, no GL interop. */
int flx_postprocess(flx_ctx *ctx);
/* saveImage's read-back half (src/clcontext.cpp:386-465): which = 0 raw accumulation (rgb sum,
 * sample count), 1 = post-processed preview.  Blocking; out = float4 per (local) pixel.
 * With flx_set_option(ctx, "denoiser", 1) -- the reference's USE_OPTIX_DENOISER kernel build (recompileKernels,
 * src/clcontext.cpp:852-874; buffers :337-338) -- `logic` / the microkernels also accumulate the denoiser feature
 * buffers and flx_postprocess resolves them: which = 2 albedo of the first non-singular hit, 3 first-hit normal in
 * camera space (both as written to denoiserAlbedoGL / denoiserNormalGL, src/mk_postprocess.cl:49-54), 4 / 5 the raw
 * accumulators (sum, count); 6 the output of the last flx_denoise or flx_denoise_variance_guided.
 * which = 7, with flx_set_option(ctx, "moments", 1): the luminance moments (sum l, sum l^2, 0, n) of the samples splatted into each pixel,
 * l = the Rec. 709 luminance of the sample (csrc/flx_denoise.h: flx_lum).  The moments are LOCAL to a rank: flx_gather does not carry them. */
int flx_read_pixels(flx_ctx *ctx, int which, float *out_rgba);
/* the blocking counterpart of flx_read_pixels for which = 0 (raw accumulation), 4 / 5 (the albedo / normal accumulators; option "denoiser"),
 * 7 (the luminance moments; option "moments"): lets a caller hand the denoisers an accumulation of its own */
int flx_write_pixels(flx_ctx *ctx, int which, const float *in_rgba);

/* DenoiserOptix::denoise / setBlend / bindBuffers (src/denoiser/OptixDenoiser.cpp, src/tracer.cpp:310-328) as a guided a-trous wavelet
 * filter for gfx950 (Dammertz et al., HPG 2010; csrc/flx_denoise.h): linear radiance (which = 0) demodulated by the floored
 * first-hit albedo, edge-stopped by albedo and normal (which = 4 / 5, resolved as flx_postprocess resolves them -- it need not have run),
 * `iterations` passes of step 1, 2, 4, ...  Writes the denoised linear image, readable as flx_read_pixels(ctx, 6, ...) (rgb, w = 1; a pixel
 * with no samples or a non-finite value is passed through as it is), and the preview (which = 1) post-processed from it.  blend is OptiX'
 * blendFactor (0 = fully denoised, 1 = the input), clamped to [0, 1]; blend 1 or 0 iterations return the input colour exactly.
 * Asynchronous on the context stream like flx_postprocess.  Fails when the option "denoiser" is off, when the context is partitioned,
 * when iterations is outside 0..8, when a sigma is not finite or <= 0, or when blend is NaN.  params NULL = the defaults. */
typedef struct { int iterations; float sigma_color, sigma_normal, sigma_albedo, blend; } flx_denoise_params;
int flx_denoise(flx_ctx *ctx, const flx_denoise_params *params);

/* The variance-guided a-trous filter (the spatial filter of SVGF, Schied et al., HPG 2017; csrc/flx_denoise_vg.h): flx_denoise
 * with the fixed colour stop replaced by a luminance stop scaled by sigma_luminance times the prefiltered standard deviation of each pixel's
 * mean, estimated from the luminance moments (which = 7; a spatial estimate where a pixel has fewer than 2 samples) and carried through the
 * passes (the prefilter clamped by the pixel's own variance).  A pixel none of whose samples hit a surface (albedo accumulator count 0: it saw
 * the area light or the environment directly) is returned as its colour and is never a neighbour.
 * Needs the options "denoiser" and "moments" on and an unpartitioned context; writes which = 6 and the preview exactly as flx_denoise
 * does, timed under FLX_K_DENOISE.  Fails as flx_denoise does (iterations outside 0..8, a sigma not finite or <= 0, a NaN blend) and when
 * the option "moments" is off.  params NULL = the defaults. */
typedef struct { int iterations; float sigma_luminance, sigma_normal, sigma_albedo, blend; } flx_denoise_vg_params;
int flx_denoise_variance_guided(flx_ctx *ctx, const flx_denoise_vg_params *params);

/* ---- temporal reprojection (no counterpart in the reference, which restarts the accumulation at every camera change, src/tracer.cpp:189-207;
 * csrc/flx_reproject.h): keep the accumulated image across a camera move of a static scene.  Opt-in; the sequence is
 *     ... render under camera A ...   flx_gbuffer            (any time after flx_set_params(A))
 *     flx_history_capture                                    (copies which = 0 / 7; the current G-buffer slot becomes the previous one)
 *     flx_set_params(B); flx_gbuffer; flx_wf_reset or flx_mk_reset (unchanged: they zero the accumulation); flx_reproject; ... render on ...
 * All five calls need an unpartitioned context and fail with a message otherwise; all flush deferred and fused launches first and touch no
 * path state, queue or counter.  The slots and the history exist from the first call on and are freed with the framebuffers (a
 * flx_set_params that changes width * height, flx_set_partition).
 *
 * flx_gbuffer: one un-jittered pinhole ray through the centre of every pixel of the current camera (no lens draws), closest hit with the
 * traversal flx_wf_extend uses (honours "extend_tree"; with 2 the hit index and t equal flx_wf_extend's bit for bit for the same ray).  Per
 * pixel G0 = (P.xyz, bits(hit index)), P as the logic pass computes it from a raw hit (the implicit area-light quad included), index -1 on a
 * miss; G1 = (Ng.xyz, t), Ng the triangle's unit geometric normal facing the ray origin (the light's N on the quad); a miss is (0, 0, 0, -1).
 * Asynchronous.
 * flx_history_capture: on the stream, copies of the accumulation (which = 0) and, with option "moments" on, of the moments (which = 7); the
 * current G-buffer slot with its camera becomes the previous slot (pointer swap) and the current slot is marked not traced.  Fails when the
 * current slot was not traced or the image size differs from the slot's.
 * flx_reproject: overwrites which = 0 for EVERY pixel -- and which = 7 when "moments" is on now and was on at the capture -- with the history
 * resampled into the new view (four bilinear taps, each accepted by a plane-distance and a normal test against the current G-buffer; the
 * weights renormalise; the count is capped at max_history, so a new sample weighs at least 1 / (max_history + 1) and view-dependent radiance
 * recovers); a pixel without history is (0, 0, 0, 0).  Writes nothing else.  Needs a captured history and a traced current slot of the same
 * size.  params NULL = the defaults {32, 2, 0.9, 0.01}; fails unless they are finite with max_history >= 1, plane_tolerance_px > 0,
 * normal_cos in [-1, 1], min_weight in (0, 1].  Asynchronous.
 * The sample count it leaves is FRACTIONAL, which is legal for every consumer of which = 0 / 7: flx_postprocess divides by it, flx_mk_splat and
 * the wavefront splat add 1 to it, the denoisers only compare it with 0 and 2.
 * flx_gbuffer_read / flx_gbuffer_write: test hooks in the spirit of flx_state_import -- slot 0 = current, 1 = previous; 8 floats per pixel
 * (G0, G1) and the 80-byte camera of the slot; the write marks the slot traced at the current image size.  Blocking. */
typedef struct { float max_history, plane_tolerance_px, normal_cos, min_weight; } flx_reproject_params;
int flx_gbuffer(flx_ctx *ctx);
int flx_history_capture(flx_ctx *ctx);
int flx_reproject(flx_ctx *ctx, const flx_reproject_params *params);
int flx_gbuffer_read(flx_ctx *ctx, int slot, float *out_8_floats_per_pixel, void *camera80);
int flx_gbuffer_write(flx_ctx *ctx, int slot, const float *in_8_floats_per_pixel, const void *camera80);
/* ---- ... across a pose of objects: flx_set_option(ctx, "motion_history", 1)  (csrc/flx_reproject_motion.h).  Off (the
 * default) every call does what it does without the option.  On, with objects defined (flx_objects_define), the sequence is
 *     ... render under pose A, camera A ...
 *     flx_gbuffer; flx_history_capture         (the capture also notes every object's current pose)
 *     flx_objects_pose(B)                      (keeps the PREVIOUS slot and the captured history; only the current slot becomes "not traced")
 *     [flx_set_params(camera B)]               (camera and objects may move in the same frame)
 *     flx_gbuffer; flx_wf_reset or flx_mk_reset (unchanged); flx_reproject; ... render on ...
 * What the option changes:
 * flx_gbuffer also writes one object id per pixel beside the slot (the object of the hit triangle; FLX_NO_OBJECT on a miss, on the implicit
 * area-light quad and on a triangle of no object); G0 / G1 are the same bytes.  flx_history_capture swaps these planes with the slots.
 * flx_objects_pose keeps a captured history whose G-buffer has such a plane; without one, and in flx_update_triangles /
 * flx_update_triangles_subset always, the history is dropped as without the option.  flx_upload_scene and flx_objects_define drop it.
 * flx_reproject (same signature, same parameters): where no object's pose differs from its pose at the capture it is the call above, bit for
 * bit.  Otherwise a pixel of a posed object looks its history up where that surface point WAS: P' = D P, N' = the normal through D's
 * cofactors, D = X_capture X_now^-1 (one 3 x 4 matrix per object, inverse and product in float64, rounded once), and a tap showing another
 * object is refused when either of the two moved.  An object posed for the first time since its definition has no known pose at the capture
 * (the uploaded triangles need not be the rest pose): its pixels get no history.  Per-triangle motion is not followed.  A moved object changes
 * shadows and reflections on surfaces that did not move: their history is stale and decays only through max_history -- unless
 * flx_history_mark / flx_history_rectify (below) take it out.
 * The object of every triangle, the two planes and the per-object table are allocated by the first flx_gbuffer or flx_objects_pose that finds
 * the option on and objects defined; turning the option off invalidates the planes.
 * flx_gbuffer_objects_read / flx_gbuffer_objects_write: test hooks beside flx_gbuffer_read / _write, one uint32 per pixel, blocking.  The write
 * needs the option on and the slot traced at the current size; while the option is on flx_gbuffer_write fills the slot's plane with
 * FLX_NO_OBJECT, so a test writes G first and objects second.  An id that is not below the object count reads as FLX_NO_OBJECT. */
int flx_gbuffer_objects_read(flx_ctx *ctx, int slot, uint32_t *out_1_uint32_per_pixel);
int flx_gbuffer_objects_write(flx_ctx *ctx, int slot, const uint32_t *in_1_uint32_per_pixel);
/* ---- ... across a per-triangle move (an animated mesh: skinning, cloth, morph targets): flx_set_option(ctx, "deform_history", 1)
 * (csrc/flx_reproject_deform.h).  Off (the default) every call does what it does without the option.  On, the sequence is
 *     ... render under shape A, camera A ...
 *     flx_gbuffer; flx_history_capture
 *     flx_update_triangles(B) | flx_update_triangles_subset(B) | flx_objects_pose(B), any number of them
 *                                              (the FIRST one after a capture copies every triangle's positions aside before it overwrites any;
 *                                               all keep the PREVIOUS slot and the captured history; only the current slot becomes "not traced")
 *     [flx_set_params(camera B)]               (camera and triangles may move in the same frame)
 *     flx_gbuffer; flx_wf_reset or flx_mk_reset (unchanged); flx_reproject; ... render on ...
 * What the option changes:
 * flx_gbuffer also writes one float2 per pixel beside the slot: the barycentrics (u, v) the traversal returned for a triangle hit (u weighs vertex
 * 1, v vertex 2), (-1, -1) on a miss and on the implicit area-light quad; G0 / G1 are the same bytes.  flx_history_capture swaps these planes
 * with the slots.
 * A move of triangles -- by any of the three calls, from a host or a device source -- keeps a captured history whose G-buffer has such a plane;
 * without one the history is dropped as without the option.  A refused call snapshots nothing and changes no state.  flx_upload_scene drops the
 * history while the option is on (the hit indices no longer name the same triangles).  Switching the option off after a move drops it too.
 * flx_reproject (same signature, same parameters): without a move since the capture it is the call above; after one, a pixel whose triangle's
 * nine position words differ bitwise from the snapshot looks its history up where that surface point WAS: P' = (1 - u - v) q0 + u q1 + v q2 over
 * the positions at the capture, N' = the old triangle's unit normal on the side N is on, and a tap is refused when exactly one of the tap's and
 * the pixel's triangles moved.  With nothing moved every pixel equals the plain call bit for bit.  A triangle that was degenerate at the capture
 * gets no history.  Two different moved surfaces sliding coplanar over each other still share taps.  Stale shadows and reflections on surfaces that
 * did not move decay only through max_history, as under "motion_history" (or are taken out by flx_history_rectify, below).  After a move, a slot
 * without its plane is refused with a message.
 * "deform_history" and "motion_history" refuse each other: this option follows flx_objects_pose as well.
 * The planes are allocated by the first flx_gbuffer / flx_gbuffer_write that finds the option on, the snapshot (48 B per triangle) and the flags
 * (1 B per triangle) by the first move that needs them; they stay with the scene.
 * flx_gbuffer_bary_read / flx_gbuffer_bary_write: test hooks beside flx_gbuffer_objects_read / _write, two floats per pixel, blocking.  The write
 * needs the option on and the slot traced at the current size; while the option is on flx_gbuffer_write fills the slot's plane with (-1, -1), so
 * a test writes G first and barycentrics second.
 * flx_deform_read: test hook, blocking: the nine position floats of every triangle as snapshotted and one byte per triangle, 1 where the
 * positions now differ from them (either may be NULL).  Fails when no move has snapshotted since the last capture. */
int flx_gbuffer_bary_read(flx_ctx *ctx, int slot, float *out_2_floats_per_pixel);
int flx_gbuffer_bary_write(flx_ctx *ctx, int slot, const float *in_2_floats_per_pixel);
int flx_deform_read(flx_ctx *ctx, float *out_9_floats_per_triangle, uint8_t *out_1_byte_per_triangle);
/* ---- history rectification (csrc/flx_rectify.h): shed stale history where new samples disagree.  Reprojection knows where a
 * surface point WAS, not that its radiance CHANGED (a moved object's shadow on a floor that did not move, a dimmed lamp).  Opt-in; the sequence is
 *     ... flx_gbuffer; flx_history_capture; [move / flx_set_params]; flx_gbuffer; flx_wf_reset or flx_mk_reset; flx_reproject;
 *     flx_history_mark; ... sample passes ...; flx_history_rectify [; ... more passes ...; flx_history_rectify ...]
 * A mark works without any reprojection as well: flx_gbuffer; flx_history_mark; change a light WITHOUT resetting; render; flx_history_rectify.
 * All three calls need an unpartitioned context, flush deferred and fused launches first, touch no path state, queue or counter, and a refused
 * call changes nothing.
 * flx_history_mark: on the stream, copies of the accumulation (which = 0) and, with option "moments" on, of the moments (which = 7) into the
 * mark.  Needs a traced current G-buffer slot of the current size.  The buffers (48 B per pixel, 64 B with moments) are allocated by the first
 * call and freed with the framebuffers.  Asynchronous.  The mark is dropped by flx_wf_reset, flx_mk_reset, a change of the image size,
 * flx_set_partition, flx_history_capture, flx_upload_scene and every call that un-traces the current slot (any move of triangles);
 * flx_write_pixels keeps it.
 * flx_history_rectify: per pixel with a surface, compares the mean luminance of the samples added since the mark with the marked history's over
 * the (2 radius + 1)^2 window of pixels on the same surface (flx_reproject's plane and normal tests under the current slot's camera), pooling
 * the PER-PIXEL differences so that static texture cancels, and takes the share lambda = min(1, sensitivity max(0, |d| - gamma se) / (max of
 * the two means + lum_floor)) of the marked history out of which = 0 (and of which = 7 when "moments" is on now and was on at the mark):
 * A' = A - lambda S, and the mark becomes S (1 - lambda), so A' - S' stays the new samples and the call may be repeated as evidence grows.  Fewer
 * than min_pixels usable pixels in the window, a pixel that misses the scene, a non-finite value anywhere: lambda = 0, and a pixel whose lambda
 * is 0 is not written.  Luminance only: a pure change of hue is not seen; curved surfaces count fewer pixels and keep more history.  Needs a
 * live mark and the current slot traced at the mark's size.  params NULL = the defaults {3, 3, 2, 0.01, 8, 2, 0.9}; fails unless radius is in
 * 1..4, gamma finite and >= 0, sensitivity finite and > 0, lum_floor finite and >= 0, min_pixels in 1..(2 radius + 1)^2, plane_tolerance_px > 0
 * and normal_cos in [-1, 1].  Asynchronous, timed under FLX_K_RECTIFY.
 * flx_history_mark_read: test hook, blocking: the mark (4 floats per pixel), its moments (refused when the mark has none) and lambda (1 float
 * per pixel) as the last flx_history_rectify since the mark left it, zeros before one.  Any output may be NULL. */
typedef struct { int radius; float gamma, sensitivity, lum_floor; int min_pixels; float plane_tolerance_px, normal_cos; } flx_rectify_params;
int flx_history_mark(flx_ctx *ctx);
int flx_history_rectify(flx_ctx *ctx, const flx_rectify_params *params);
int flx_history_mark_read(flx_ctx *ctx, float *out_mark_4_floats_per_pixel, float *out_mark_moments_4_floats_per_pixel, float *out_lambda_1_float_per_pixel);

/* ---- microkernel integrator (the reference's second integrator).  One path per pixel (needs
 * num_tasks >= width*height to cover the image), `phase` state machine, exactly one sample per pixel per pass.
 * enqueueResetKernel / RayGenKernel / NextVertexKernel / BsdfSampleKernel / SplatKernel / SplatPreviewKernel
 * (src/clcontext.cpp:709-750; kernels src/mk_reset.cl, mk_raygen.cl, mk_next_vertex.cl, mk_sample_bsdf.cl, mk_splat.cl,
 * mk_splat_preview.cl).  Single-GPU (the pixel partition applies to the wavefront path only). */
int flx_mk_reset(flx_ctx *ctx);
int flx_mk_raygen(flx_ctx *ctx);
int flx_mk_next_vertex(flx_ctx *ctx);
int flx_mk_sample_bsdf(flx_ctx *ctx);
int flx_mk_splat(flx_ctx *ctx);
int flx_mk_splat_preview(flx_ctx *ctx);
/* ---- adaptive sampling for the microkernel integrator (no counterpart in the reference, which gives every pixel the same sample count,
 * src/tracer.cpp:95-169; csrc/flx_adaptive.h, csrc/adaptive.hip): stop sampling a pixel when it is converged.
 * Per pixel, from the luminance moments (which = 7; only their own n enters): mu = S1 / n, v = max(0, S2 / n - mu^2) / n (the variance of the
 * MEAN), r = sqrt(v) / (mu + lum_floor);  done: n >= max_samples;  converged: n >= min_samples, n >= 2 and r <= threshold (a NaN or a non-finite
 * sum never converges: such a pixel runs to max_samples);  own = !done && !converged;  active = !done && (own || (dilate && a 3 x 3
 * neighbour inside the image has own)).
 * flx_mk_adaptive_update classifies every pixel, compacts the active ones into an ASCENDING list (reproducible: no atomics) and INSTALLS it:
 * the following flx_mk_raygen / flx_mk_next_vertex / flx_mk_sample_bsdf / flx_mk_splat run over the listed pixels only -- a listed pixel advances
 * exactly as in an unlisted pass, bit for bit (the integrator's state, seed chain included, is per pixel), an unlisted pixel is not touched, and
 * flx_mk_stats counts the listed samples only.  *out_active = the length of the list (one blocking 4-byte read); 0 installs an empty list: the
 * four calls are no-ops.  flx_mk_splat_preview ignores the list.  Needs option "moments", an unpartitioned context and
 * width * height <= num_tasks; params NULL = the defaults {0.05, 4, 32, 0.01, 1}.  Fails when threshold or lum_floor is not
 * finite or < 0, max_samples is 0 or > 2^24, min_samples > max_samples, or dilate is not 0 / 1.
 * flx_mk_adaptive_clear: back to "every pixel".  flx_mk_reset, a flx_set_params that changes the image size, flx_set_partition,
 * flx_upload_scene and flx_set_option(ctx, "moments", 0) clear it too, so no call sequence written before these entry points meets a list.
 * flx_mk_active_read / flx_mk_active_write: test hooks like flx_gbuffer_read / _write.  read: *out_count and, where not NULL, the installed list
 * (out_list: room for width * height entries) and the flag byte of every pixel as the last update left it (bit 0 own, 1 active, 2 done,
 * 3 converged; zeros after a write); fails when no list is installed.  write: installs an arbitrary list; fails unless every entry is
 * < width * height and the list is strictly ascending.  Blocking. */
typedef struct { float threshold; uint32_t min_samples, max_samples; float lum_floor; uint32_t dilate; } flx_adaptive_params;
int flx_mk_adaptive_update(flx_ctx *ctx, const flx_adaptive_params *params, uint32_t *out_active);
int flx_mk_adaptive_clear(flx_ctx *ctx);
int flx_mk_active_read(flx_ctx *ctx, uint32_t *out_list, uint32_t *out_count, uint8_t *out_flags);
int flx_mk_active_write(flx_ctx *ctx, const uint32_t *in_list, uint32_t n);
/* fetchStatsAsync / resetStats (src/clcontext.cpp:634-646): RenderStats {primaryRays, extensionRays, shadowRays, samples}
 * (4 x u32, src/geom.h:254-260) accumulated on the device by the microkernels; *out16 valid after flx_finish() */
int flx_mk_stats_async(flx_ctx *ctx, void *out16);
int flx_mk_stats_reset(flx_ctx *ctx);

/* ---- multi-GPU (no counterpart in the reference: one cl::CommandQueue, one device).
 * Rank r of R owns global pixels p*R + r; its framebuffer holds ceil((w*h - r)/R) local pixels. */
int flx_set_partition(flx_ctx *ctx, uint32_t rank, uint32_t nranks);
uint32_t flx_local_pixels(flx_ctx *ctx);
/* device-to-device copy of the raw accumulation buffer (local pixels, float4) into a caller-owned
 * device buffer (e.g. a torch tensor handed to an RCCL gather); asynchronous on the context stream */
int flx_copy_pixels_to_device(flx_ctx *ctx, void *dst_device_ptr);
/* the context's hipStream_t, for callers that order their own work after ours */
void *flx_stream(flx_ctx *ctx);

/* ---- multi-GPU group and gather over RCCL / xGMI (SURVEY 8(b) flx_create_group / flx_gather, 8(e)).  librccl.so.1 is bound with
 * dlopen at the first call, so single-GPU users never load it.  Two ways to form the group:
 *   one process per GPU (torchrun / MPI style): rank 0 calls flx_group_unique_id and ships the 128 bytes to the other ranks by
 *     whatever channel the launcher has; every rank then calls flx_group_init(ctx, rank, nranks, id) (= ncclCommInitRank +
 *     flx_set_partition), renders, and all ranks call flx_gather(ctx, root, out) -- a collective; `out` (width*height float4,
 *     host) is written on the root only.
 *   one process, N contexts on N devices (the reference's single-process Tracer driving a node): flx_group_init_local(ctxs, n)
 *     (= ncclCommInitAll + partitions 0..n-1) and flx_gather_local(ctxs, n, root, out).  If several of the contexts sit on the SAME
 *     device (a 1-GPU box standing in for N ranks) the tiles travel by device-to-device copies instead of RCCL, everything else
 *     (partition, staging, de-interleave) is the same code.
 * Each rank sends its compact float4[local pixels] accumulation tile (rgb sum, sample count) point-to-point to the root
 * (grouped ncclSend / ncclRecv); the root de-interleaves global pixel p*R + r <- tile r, pixel p.  Blocking. */
#define FLX_GROUP_ID_BYTES 128
int flx_group_unique_id(void *out128);
int flx_group_init(flx_ctx *ctx, uint32_t rank, uint32_t nranks, const void *id128);
int flx_group_init_local(flx_ctx **ctxs, uint32_t n);
int flx_gather(flx_ctx *ctx, uint32_t root, float *out_rgba_host);
int flx_gather_local(flx_ctx **ctxs, uint32_t n, uint32_t root, float *out_rgba_host);
int flx_group_destroy(flx_ctx *ctx);
/* what the communicator itself reports: out2 = {ncclCommCount, ncclCommUserRank} (a same-device local group reports its partition) */
int flx_group_info(flx_ctx *ctx, uint32_t *out2);

/* ---- measurement.  Per-kernel HIP-event timing on the context's stream (the reference attaches
 * cl::Events to the two trace kernels, src/clcontext.cpp:673-701,780,786).  kernel ids: */
enum { FLX_K_RESET = 0, FLX_K_RAYGEN = 1, FLX_K_EXTEND = 2, FLX_K_SHADOW = 3, FLX_K_LOGIC = 4, FLX_K_MATERIALS = 5,
       FLX_K_POSTPROCESS = 6,
       FLX_K_TRACE_SPAN = 7,   /* start of the extension kernel .. end of the (concurrent) shadow kernel */
       FLX_K_LOGIC_FUSED = 8,  /* logic + the inlined material step as one pass (option "fuse"); FLX_K_MATERIALS then covers the rest */
       FLX_K_DENOISE = 9,      /* the whole of one flx_denoise or flx_denoise_variance_guided */
       FLX_K_GBUFFER = 10,     /* flx_gbuffer */
       FLX_K_REPROJECT = 11,   /* flx_reproject */
       FLX_K_REFIT = 12,       /* the kernels of one flx_update_triangles / _subset; flx_objects_pose adds its pose kernels as a span of their own */
       FLX_K_TREE_COST = 13,   /* the kernels of one flx_tree_cost */
       FLX_K_SNAPSHOT = 14,    /* option "deform_history": the copy of the positions a move of triangles makes after a capture */
       FLX_K_MOVED_FLAGS = 15, /* ... and the moved-flag pass as flx_deform_read launches it (inside flx_reproject it is part of FLX_K_REPROJECT) */
       FLX_K_RECTIFY = 16,     /* the two kernels of one flx_history_rectify */
       FLX_K_COUNT = 17 };
/* on: 0 off | 1 time every kernel | 2 time only the two trace kernels (+ their span), as the reference does | 3 only the
 * extension kernel | 4 the three kernels bench.py prices against a roof: extension, logic (the fused pass incl. its queue scan + scatter), shadow.
 * Each event pair costs a few microseconds of stream time, which shows at ~11 launches per 0.7 ms
 * iteration: level 1 costs 7 % of the throughput, level 3 about 1.5 % (at 1 M paths; at the bench's 8 M a quarter of that). */
int flx_profile_enable(flx_ctx *ctx, int on);
/* after flx_finish(): accumulated milliseconds and launch count since the last reset */
int flx_profile_get(flx_ctx *ctx, int kernel, double *total_ms, uint64_t *launches);
int flx_profile_reset(flx_ctx *ctx);
/* traversal work counters (algorithmic-bytes model): when enabled the trace kernels
 * accumulate {ext rays, ext inner-node visits, ext triangle tests, ext hits, shadow inner,
 * shadow triangle tests, shadow rays}.  Counting launches are not used inside timed regions. */
int flx_trace_stats_enable(flx_ctx *ctx, int on);
int flx_trace_stats_get(flx_ctx *ctx, uint64_t *out7);
/* the same 7 counters + out16[8..11] / [12..15]: wave-level trip counts of the extension / shadow traversal
 * {outer iterations, inner-node branch executions, leaf branch executions, triangle-loop trips}; SIMD efficiency of
 * the traversal = lane-level visits / (64 x wave-level trips) */
int flx_trace_stats_get_ex(flx_ctx *ctx, uint64_t *out16);
/* the 16 above + out24[16] / [17]: leaf visits of the extension / shadow traversal ([18..23] reserved) */
#define FLX_NUM_TRACE_STATS 24
int flx_trace_stats_get_all(flx_ctx *ctx, uint64_t *out24);
int flx_trace_stats_reset(flx_ctx *ctx);
/* what flx_upload_scene built: out8 = {wide nodes, wide leaf data (16-byte units), wide traversal-stack bound, boxes nested (1/0),
 * binary tree depth, spill levels per lane, binary inner-node records, largest leaf} */
int flx_scene_info(flx_ctx *ctx, uint32_t *out8);

/* ---- test hooks: path state in the reference's GPUTaskState SoA layout (64 columns x num_tasks
 * words, src/geom.h:199-236), queues and counters.  Blocking. */
int flx_state_export(flx_ctx *ctx, float *out_64xN);
/* the arithmetic contract (include/flx_math.h) evaluated on the device over n operand pairs, results as bit patterns.  fn: 0 sin, 1 cos,
 * 2 tan, 3 atan2(a, b), 4 acos, 5 pow(a, b), 6 log, 7 exp, 8 asin, 9 atan, 10 fmin, 11 fmax, 12 a / b, 13 sqrt, 14 a * b, 15 a + b.
 * The oracle's orc_math_array is the CPU half: both sides must agree bit for bit, signed zeros included. */
int flx_math_probe(flx_ctx *ctx, int fn, const float *a, const float *b, uint32_t n, uint32_t *out_bits);
/* test hook: the per-texel light-sample table the library builds at flx_upload_envmap (8 floats per texel: {L.xyz, pdfW, Li.xyz, 0}).
 * The oracle's orc_env_sample_table computes the same values inline, as the reference's logic kernel does per path (src/wf_logic.cl:236-249). */
int flx_env_sample_table(flx_ctx *ctx, float *out_8_per_texel);
int flx_state_import(flx_ctx *ctx, const float *in_64xN);
int flx_queue_read(flx_ctx *ctx, int queue, uint32_t *out_N);
int flx_queue_write(flx_ctx *ctx, int queue, const uint32_t *in, uint32_t n);
int flx_set_counters(flx_ctx *ctx, const void *in32);
/* options.  Unknown names fail.
 *   shadow_tree       4 (default): flx_wf_shadow walks the 4-wide quantised tree built at upload over the reference tree's leaves
 *                     (csrc/flx_wide.h) -- bit-identical results to the binary tree (order-free query, conservative boxes, exact
 *                     leaf test) | 2: the reference's binary tree
 *   extend_tree       4 (default): flx_wf_extend on the 4-wide tree -- same closest hit except where the visit ORDER decides
 *                     (exact ties in t, box-vs-triangle rounding near-ties; SURVEY 8(c) budgets <= 1e-5 of rays, measured in
 *                     DESIGN.md 4.1) | 2: the reference's binary tree in the reference's visit order (bit-exact)
 *   overlap           0 serial | 1 flx_wf_shadow directly after flx_wf_extend runs concurrently with it on a second stream |
 *                     2 as 1, and it starts as soon as `logic` is done when only raygen / materials / extend
 *                     were enqueued since flx_wf_logic (see flx_wf_shadow in api_wavefront.hip) | -1 (default) = 2; flx_get_option returns the
 *                     effective value
 *   refill_extend     the closest-hit query on the 4-wide tree as a PERSISTENT kernel (csrc/trace4r.hip): value = refillMin | waitMax << 8
 *                     -- lanes that finished take new rays when refillMin lanes are idle; a descent round ends when waitMax lanes
 *                     stand on a leaf.  Default 16 | 32 << 8; 0 = the thread-per-ray kernel.  Bit-identical results.  The kernel leaves
 *                     RAW hit records; they are committed by the next fused logic pass, or by a separate pass as soon as any call that
 *                     could observe a hit record is made -- no call sees a raw one
 *   refill_shadow     the same for the any-hit query; -1 (default) = 0: two persistent kernels cannot share the machine, so the any-hit
 *                     kernel stays thread-per-ray and fills the slots the persistent closest-hit kernel's waves leave (api.hip: pickSchedule)
 *   shadow_split      the thread-per-ray any-hit query as a SPLIT launch (csrc/trace4.hip: k_shadow4s): value = K | K2 << 8.  A pass over
 *                     the shadow queue gives every ray K node visits; a ray that is not done by then parks {queue position, stack} in a 64-byte
 *                     continuation record and frees its lane.  K2 == 0: the suspended rays are then finished by persistent waves that refill
 *                     their lanes from the records (csrc/trace4r.hip: k_trace4r_resume; see shadow_resume).  K2 > 0: a second thread-per-record
 *                     pass with budget K2 and a third without.  0 = off (k_shadow4) | -1 (default) = the library's choice, made at every launch
 *                     from the render parameters: K = 8 when every shadow ray runs toward the environment light (useEnvMap && !useAreaLight), else
 *                     0.  An explicit value holds, 0 included; flx_get_option returns what flx_wf_shadow will really launch: 0 also under
 *                     refill_shadow, shadow_tree 2, a scene without a usable wide tree and the trace statistics.  Bit-identical results.  The
 *                     records are allocated when the choice first becomes non-zero -- in flx_set_params, flx_upload_scene or this option, not in a
 *                     launch call -- and kept: 32 B per path (numTasks / 2 records; ~540 MB at 16 M paths), plus 8 B per path for the second set
 *                     once a K2 > 0 is used.  When the library's own choice does not fit it becomes 0 for the context (shadow_split_fallback); an
 *                     explicit value that does not fit fails the call
 *   shadow_split_fallback   read-only: 1 when the records of the library's own choice did not fit into device memory and the choice is 0 for this context
 *   shadow_resume     1 (default) | 0: with 0 the suspended rays of a split launch without K2 are finished one lane per record slot (the round-5
 *                     pass 2); for A/B and tests
 *   shadow_split_limit      test hook: use only this many record slots per sub-list (0 = all); rays that find their list full finish in the first pass
 *   shadow_split_suspended  read-only: the number of rays the last split launch suspended in its first pass (0 before the first one); waits for the stream
 *   fuse              1 (default): flx_wf_logic is DEFERRED -- launched by the next call on this context; when that call is
 *                     flx_wf_materials (a flx_wf_raygen between the two is deferred along and launched right after), logic and the
 *                     material step of the most common BSDF types run as ONE pass over the path state (logic.hip: k_logic<FUSED>),
 *                     the other types through their queues as usual; when it is anything else, the plain kernel runs first.  No call
 *                     can observe a state, queue or counter the separate kernels would not have produced (but see ext_order for
 *                     the ORDER of the extension queue); an error raised by a deferred launch is reported by the call that launched it.  Needs the
 *                     material queues empty (flx_clear_queues / flx_end_iteration_async since the last logic) and wfSeparateQueues
 *                     (or a build that inlines every type) -- otherwise, and with 0, every call launches its own kernels at once
 *   fuse_set          BSDF types the fused pass inlines: 1 diffuse only | 31 all six.  flx_upload_scene picks it from the scene
 *                     (diffuse surfaces >= 3/4 of the triangle area: 1, else 31); set it after the upload to override.  OVERRIDDEN while
 *                     params.wfSeparateQueues == 0: with a single material queue every BSDF type sits in the diffuse list and only the pass
 *                     that inlines all types can serve it, so that pass runs whatever fuse_set says -- flx_get_option("fuse_set") still returns
 *                     the stored value, the read-only "fuse_set_now" the set the next fused pass will really inline (an A/B of fuse_set under a
 *                     single material queue compares the all-types pass with itself)
 *   regen_prep        1 (default) | 0: inside the fused chain logic -> genRays -> materials the RAW logic pass computes, for the paths it terminates, the half
 *                     of genRays that is a function of the path's seed alone (jitter, thin-lens origin, throughput + the seed genRays leaves,
 *                     shadowRayBlocked, lastLightPickProb) and stores it with its full-line stores; the genRays launch of the same chain then stores
 *                     only the direction and the pixel (logic.hip / misc.hip: PREPARED REGENERATION).  Bit-identical results; no call can run
 *                     between the two launches
 *   regroup           the all-types fused pass hands its material step through LDS sorted by BSDF type, so that a wave runs one type
 *                     (logic.hip: LOGIC_REGROUP; 96 VGPRs + 20 KB of LDS per block): 0 | 1 | -1 (default) = on; flx_get_option returns the
 *                     effective value.
 *                     Bit-identical results.  Takes effect when the path count is a multiple of 256 (whole blocks)
 *   ext_order         how the fused pass lists the traced paths in the extension queue: 0 one segment per material queue, in the
 *                     separate kernels' order | 1 all continuing paths by path id | 2 continuing AND regenerated paths merged into one
 *                     list by path id (genRays then does not append; needs genRays between logic and the material kernels, else as 1).
 *                     The same SET of paths either way; the reference's order is whatever its atomic_inc produces.  flx_upload_scene picks
 *                     it with fuse_set (1 with 31, 2 with 1); set it afterwards to override
 *   node_layout       1 (default) sibling-pair record numbering of the binary tree | 0 DFS numbering; takes effect at the next flx_upload_scene
 *   denoiser          1: accumulate the denoiser feature buffers (see flx_read_pixels); default 0
 *   moments           1: the splats (flx_wf_logic, flx_mk_splat) also accumulate the luminance moments of their samples (flx_read_pixels
 *                     which = 7), three more scattered float atomics per terminating path in the wavefront integrator; the resets zero
 *                     them.  Default 0.  Local to each rank (flx_gather does not carry them)
 *   xcd_remap, eager_bump: A/B knobs of the binary kernels */
int flx_set_option(flx_ctx *ctx, const char *name, int value);
/* current value of an option above, or of the read-only "fused_queue_mask" (bit q set = the fused pass inlines the material step of
 * queue q's paths, flx_queue_counters order), or of the read-only "phase": the state of the call-sequence state machine behind the
 * deferred / fused / early-started kernels (flx_ctx.h: enum Phase) -- bits 0-2: 0 idle, 1 flx_wf_logic deferred, 2 flx_wf_logic +
 * flx_wf_raygen deferred, 3 only genRays / material kernels enqueued since logic, 4 ... and the extension kernel last, 5 the extension
 * kernel last with the chain since logic broken; bit 3: the hit records of the last extension launch are still RAW; bit 4: the material
 * queues are known to be empty; or of the read-only "wide_far": 1 when the 4-wide node test clamps 1 / dir for a scene reaching beyond +-2^26
 * (FLX_WIDE_DINV_FAR), else 0 -- re-derived by every upload, flx_update_triangles and flx_update_triangles_subset from the triangles the
 * scene then holds.  Never changes any state (tests/test_gpu_fuzz.py reports its coverage with it). */
int flx_get_option(flx_ctx *ctx, const char *name, int *value);

#ifdef __cplusplus
}
#endif

/* The two-constant surface-area heuristic with both constants 1 over four sums of flx_tree_cost: (S_node + S_tri) / A_root -- the expected
 * number of node entries plus triangle tests of a random ray that hits the root box.  The constants are a choice, not a measurement (DESIGN.md
 * 4.10.1).  NaN when A_root is not a positive finite number: a caller treats NaN as "no decision". */
static inline double flxTreeCostValue(const double sums4[4])
{
    const double a = sums4[0];
    if (!(a > 0.0) || a > 1.7976931348623157e308) return __builtin_nan("");
    return (sums4[1] + sums4[3]) / a;
}
#endif /* FLUCTUS_HIP_H */
