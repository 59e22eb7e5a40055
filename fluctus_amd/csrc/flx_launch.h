// flx_launch.h -- the host-side launchers and helpers of the kernel files, declared ONCE: every .hip file that defines one of them includes
// this header and so does every file that calls one, so a definition that drifts from its declaration is an error of the build (an overload the
// caller cannot reach is left undefined, and the library is linked with -Wl,--no-undefined: fluctus_amd/build.py).
#pragma once
#include "flx_device.h"
#include <vector>

namespace flx { struct ad_params; struct rp_view; struct rp_params; struct rc_params; }     // flx_adaptive.h, flx_reproject.h, flx_rectify.h: passed by reference only

namespace flxd {
// What flx_upload_scene keeps for flx_update_triangles (refit.hip): the records of each depth of both trees (deepest level launched first), where
// the wide leaf blocks and their triangles start, the exact fp32 box of every wide node.  Device arrays live with the scene allocations.
struct RefitTables {
    uint32_t ntris = 0, nidx = 0, nmat = 0, nwtri = 0, nwleaf = 0;
    uint32_t *blevel = nullptr, *wlevel = nullptr;      // BNode record / WNode numbers sorted by depth; level l = [levelStart[l], levelStart[l + 1])
    std::vector<uint32_t> blevelStart, wlevelStart;
    uint32_t *wtriOff = nullptr, *wleafOff = nullptr;   // per wide leaf triangle / per wide leaf block: its offset in the leaf data (16-byte units)
    float4 *wexact = nullptr;                           // {min, max} per WNode: the box of its binary node as uploaded, rewritten by every refit
    uint32_t *valid = nullptr;                          // 4 words: the validation pass's result
    void *stage = nullptr;                              // ntris wire triangles for a host source; allocated by the first such call
    double *costSlab = nullptr;                         // flx_tree_cost's per-block partial sums and results (tree_cost.hip); allocated by the first call
    // flx_update_triangles_subset.  A record is dirty in a call when its stamp equals that call's epoch: one stamp per triangle,
    // per BNode record, per WNode and per wide leaf block (lStamp is indexed by the block's OFFSET in the leaf data, the very number a wide leaf
    // reference carries: no table from reference to block number, and no dependent read of one).  ONE allocation, made and zeroed by the first
    // call; epoch 0 is never a call's, and a wrap of the counter re-zeroes the stamps.
    uint32_t *triStamp = nullptr, *bStamp = nullptr, *wStamp = nullptr, *lStamp = nullptr;
    size_t stampWords = 0;
    uint32_t epoch = 0;
    uint32_t *stageIdx = nullptr;                       // ntris indices for a host source (the triangles go to `stage`); allocated by the first such call
    // option "deform_history" (DESIGN.md 4.3.6): the positions at the last capture, three float4 per triangle, and one moved byte per triangle;
    // allocated by the first move that snapshots.  Whether the snapshot is of THIS capture is TemporalState::snap's to say.
    float4 *snapPos = nullptr; uint8_t *movedFlags = nullptr;
};
// (source triangles, index list, listed count: a null list means every triangle of the scene, the full refit)
void launch_refit_validate(hipStream_t, const void *, const uint32_t *, uint32_t, const Scene &, const RefitTables &, uint32_t *);
void launch_refit(hipStream_t, const void *, const uint32_t *, uint32_t, const Scene &, const RefitTables &);
// What flx_objects_define keeps for flx_objects_pose (pose.hip); passed to the kernels by value.  Device arrays live with the
// scene allocations.  A member is a triangle that belongs to an object; members are kept in ascending triangle order.
struct ObjectTables {
    uint32_t nobjects = 0, members = 0;
    uint32_t *memberTri = nullptr, *memberObj = nullptr;        // per member: its triangle index, its object
    float4 *rest = nullptr;                                     // per member: its rest triangle, ten float4
    uint32_t *stamp = nullptr, *slot = nullptr;                 // per object: the epoch of the last call that listed it, its position in that call's list
    uint32_t *ids = nullptr; float4 *xforms = nullptr;          // a call's list: up to nobjects ids, three float4 (a 3 x 4 matrix) each
    float4 *out = nullptr; uint32_t *outIdx = nullptr;          // `members` posed wire triangles and their triangle indices: the subset refit's device source
    uint32_t *blockCounts = nullptr, *total = nullptr;          // pose_blocks(members) words, one word
    uint32_t epoch = 0;                                         // epoch 0 is never a call's; a wrap of the counter re-zeroes the stamps (as RefitTables::epoch)
};
// The table of emissive triangles (option "mesh_lights"; what each array holds and in which order it is summed: flx_mesh_light.h; kernels:
// mesh_light.hip); passed to the kernels by value.  Device arrays live with the scene allocations (flx_ctx::MeshLight).
struct MeshLights {
    uint32_t n = 0;                                             // lights listed (ascending triangle indices in `tri`)
    uint32_t *tri = nullptr;
    float *w = nullptr, *cdf = nullptr, *pick = nullptr;        // per light
    double *local = nullptr;                                    // per light: the prefix sum inside its run
    double *runSum = nullptr, *off = nullptr; uint32_t *runLast = nullptr;      // per run (off: runs + 1)
    double *total = nullptr;                                    // total64; 0 = no lights
    uint32_t *hdr = nullptr;                                    // [0] the last light with w > 0, [1] the last light with pick > 0 (ML_NONE: none)
};
__device__ __forceinline__ void ml_vertices(const Scene &sc, uint32_t tri, f3 *p0, f3 *p1, f3 *p2)
{
    const float4 *t = reinterpret_cast<const float4 *>(sc.tris + tri);
    *p0 = ld3(t[0]); *p1 = ld3(t[3]); *p2 = ld3(t[6]);
}
__device__ __forceinline__ int ml_material(const Scene &sc, uint32_t tri) { return sc.tris[tri].matId; }
// how the table reaches a kernel that exists with and without the lamps (template <bool MESH>): by value, and as an EMPTY struct in the instance without
template <bool MESH> struct MeshArg { static constexpr bool on = false; __device__ MeshLights get() const { return MeshLights(); } };
template <> struct MeshArg<true> { static constexpr bool on = true; MeshLights t; __device__ MeshLights get() const { return t; } };
uint32_t mesh_light_runs(uint32_t n);
void launch_mesh_light_build(hipStream_t, const Scene &, const MeshLights &);
void launch_mesh_light_probe(hipStream_t, const Scene &, const MeshLights &, const float *, uint32_t, uint32_t *, float *);
uint32_t pose_blocks(uint32_t members);
void launch_pose(hipStream_t, const ObjectTables &, uint32_t count);
void launch_object_of_triangle(hipStream_t, const ObjectTables &, uint32_t *objectOfTri);     // the members' objects scattered into a table the caller has filled with FLX_NO_OBJECT
void launch_block_scan(hipStream_t, uint32_t *blockCounts, uint32_t nb, uint32_t *total);      // adaptive.hip: in place, counts -> exclusive offsets
size_t tree_cost_slab_doubles(const RefitTables &);
double *launch_tree_cost(hipStream_t, const Scene &, const RefitTables &, double *);      // -> where the eight results land in the slab
void launch_extend(hipStream_t, const State &, const Queues &, const Scene &, const flx_render_params &, uint32_t *, unsigned long long *, int);
void launch_shadow(hipStream_t, const State &, const Queues &, const Scene &, const flx_render_params &, uint32_t *, unsigned long long *, int);
void launch_extend4(hipStream_t, const State &, const Queues &, const Scene &, const flx_render_params &, uint32_t *, unsigned long long *);
void launch_shadow4(hipStream_t, const State &, const Queues &, const Scene &, const flx_render_params &, uint32_t *, unsigned long long *);
void launch_shadow4_split(hipStream_t, const State &, const Queues &, const Scene &, const flx_render_params &, uint32_t *, uint32_t *, uint32_t, uint4 *, uint32_t, uint4 *, uint32_t, int, int, uint32_t,
                          int resume, uint32_t numCUs);
void launch_shadow4_resume(hipStream_t, const State &, const Queues &, const Scene &, const flx_render_params &, uint32_t *, uint32_t numCUs, const uint32_t *count, const uint4 *rec, uint32_t subCap, uint32_t limit);
uint32_t shadow_split_lists(); uint32_t shadow_split_count_words();
uint32_t shadow_split_suspended(const uint32_t *hostCounts, uint32_t parity, uint32_t subCapA, uint32_t limit);
void launch_extend4r(hipStream_t, const State &, const Queues &, const Scene &, const flx_render_params &, uint32_t *, uint32_t, int, uint32_t *);
void launch_shadow4r(hipStream_t, const State &, const Queues &, const Scene &, const flx_render_params &, uint32_t *, uint32_t, int, uint32_t *);
void launch_logic(hipStream_t, const State &, const Queues &, const Scene &, const Frame &, const flx_render_params &, uint8_t *, uint32_t *, uint32_t *, int, int, int, int, int, int,
                  unsigned long long *, uint32_t, int, int, uint32_t *, int, uint32_t, uint32_t, const MeshLights *);     // (the last: non-null = the MESH instance of the plain pass)
void launch_env_nee_table(hipStream_t, const Scene &, float4 *, uint32_t);
int logic_can_regenerate();
int logic_can_lazy_commit(int fuse);     // does the RAW pass of this BSDF set have an instance that leaves the hit point / uv records out (logic.hip: LAZY)?
uint32_t logic_lookback_words(uint32_t numTasks);
void launch_materialise(hipStream_t, const State &, const Scene &, const flx_render_params &, uint32_t);
void launch_settle_hits(hipStream_t, const State &, const Scene &, const flx_render_params &, uint32_t);
void launch_materials(hipStream_t, const State &, const Queues &, const Scene &, uint32_t);
void launch_materials_after_fused(hipStream_t, const State &, const Queues &, const Scene &, uint32_t, int);
uint32_t fused_queue_mask(int);
uint32_t logic_aux_stride(uint32_t);
uint32_t logic_queue_aux_words(uint32_t);
void launch_reset(hipStream_t, const State &, const Queues &, const Frame &, const flx_render_params &);
void launch_raygen(hipStream_t, const State &, const Queues &, const Frame &, const flx_render_params &, int, int);
void launch_postprocess(hipStream_t, const Frame &, const flx_render_params &);
void launch_state_export(hipStream_t, const State &, float *, float);
void launch_state_import(hipStream_t, const State &, const float *);
void launch_math_probe(hipStream_t, int, const float *, const float *, uint32_t, uint32_t *);
void launch_mk_reset(hipStream_t, const State &, const Frame &, const flx_render_params &);
// the four steps of a sample pass: (list of active pixels or null = every pixel, its count; an installed list that is EMPTY launches nothing), and for
// the two that see lights the table of the lamps or null (option "mesh_lights")
void launch_mk_raygen(hipStream_t, const State &, const flx_render_params &, const uint32_t *, uint32_t);
void launch_mk_next_vertex(hipStream_t, const State &, const Scene &, const Frame &, const flx_render_params &, uint32_t *, uint32_t *, const uint32_t *, uint32_t, const MeshLights *);
void launch_mk_sample_bsdf(hipStream_t, const State &, const Scene &, const Frame &, const flx_render_params &, uint32_t *, uint32_t *, const uint32_t *, uint32_t, const MeshLights *);
void launch_mk_splat(hipStream_t, const State &, const Frame &, const flx_render_params &, uint32_t *, int, const uint32_t *, uint32_t);
uint32_t adaptive_blocks(uint32_t);
void launch_adaptive_update(hipStream_t, const float4 *, int, int, const ad_params &, uint8_t *, uint32_t *, uint32_t *, uint32_t *);
void launch_end_iteration(hipStream_t, uint32_t *, unsigned long long *, uint32_t *, uint32_t, uint32_t, uint32_t *);
void launch_bump_extension(hipStream_t, uint32_t *, uint32_t);
void launch_deinterleave(hipStream_t, const float *, float *, uint32_t, uint32_t, uint32_t);
struct DnGuided; struct DnVg;     // the two filters of denoise.hip
template <class F> void launch_denoise(hipStream_t, const Frame &, float4 *, float4 *, float4 *, float2 *, float *, int, int, int, float, float, float,
                                       float, const flx_render_params &);
// (the last three: the slot's object plane and the object of every triangle -- both null: no plane is written; the slot's barycentric plane or null)
void launch_gbuffer(hipStream_t, const Scene &, const flx_render_params &, uint32_t *, uint32_t, int, float4 *, uint32_t, uint32_t *, const uint32_t *, float2 *);
void launch_reproject(hipStream_t, const rp_view &, const rp_params &, const float4 *, const float4 *, const float4 *, const float4 *, float4 *, float4 *);
// (... then the current and the previous object plane, the motion table and the object count)
void launch_reproject_motion(hipStream_t, const rp_view &, const rp_params &, const float4 *, const float4 *, const float4 *, const float4 *, float4 *, float4 *,
                             const uint32_t *, const uint32_t *, const float4 *, uint32_t);
// option "deform_history" (flx_reproject_deform.h): (triangle count, the snapshot: three float4 per triangle) | (..., one moved byte per triangle) |
// launch_reproject's arguments, then the current and the previous barycentric plane, the scene, the triangle count, the snapshot and the flags
void launch_snapshot_positions(hipStream_t, const Scene &, uint32_t, float4 *);
void launch_moved_flags(hipStream_t, const Scene &, uint32_t, const float4 *, uint8_t *);
void launch_reproject_deform(hipStream_t, const rp_view &, const rp_params &, const float4 *, const float4 *, const float4 *, const float4 *, float4 *, float4 *,
                             const float2 *, const float2 *, const Scene &, uint32_t, const float4 *, const uint8_t *);
// flx_history_rectify (flx_rectify.h, rectify.hip): parameters, the current camera's footprint, W, H, the current G-buffer slot, the prepare records
// (scratch, one float4 per pixel), which = 0 and its mark, which = 7 and its mark (both null: the moments are left alone), the lambda plane
void launch_rectify(hipStream_t, const rc_params &, float, int, int, const float4 *, float4 *, float4 *, float4 *, float4 *, float4 *, float *);
#ifdef FLX_LAB_RSTATS
extern unsigned long long *g_lab_rstats;
#endif
}
