// flx_ctx.h -- PRIVATE to the api*.hip units that implement include/fluctus_hip.h: the context, the error / sequencing macros, the allocation
// and timing helpers, and the few functions one unit defines for the others.  One concern per unit:
//   api.hip            context lifetime, parameters, partition, framebuffers, flx_finish, counters, pixel read-back, options
//   api_upload.hip     flx_upload_scene (the CDNA4 re-layout of the BVH, the wide tree), flx_upload_envmap
//   api_wavefront.hip  the call-sequence state machine and the flx_wf_* entry points it serves
//   api_image.hip      post-process, the two denoisers, temporal reprojection, the microkernel integrator and its adaptive render
//   api_group.hip      the multi-GPU group: RCCL binding, flx_group_*, flx_gather*
//   api_hooks.hip      measurement and test hooks
//   api_refit.hip      flx_update_triangles / flx_update_triangles_subset (moved triangles -> refitted trees, refit.hip), their test hook flx_tree_read, flx_tree_cost (tree_cost.hip),
//                      flx_objects_define / flx_objects_pose (objects posed on the device, pose.hip, handed to the subset refit) and their test hook flx_objects_read
//   api_mesh_light.hip flx_mesh_lights_read / flx_mesh_lights_sample and the rebuild of the table of emissive triangles (option "mesh_lights", mesh_light.hip)
// The state of the image features -- G-buffer slots and history, poses, the list of active pixels -- and which call invalidates what: flx_feature_state.h;
// the units above call its transitions and ask its predicates, none of them writes one of its flags.
// Everything here that is not `struct flx_ctx` (the C header's opaque type) lives in namespace flxd, like the launchers (flx_launch.h), so the
// library's extern "C" surface is include/fluctus_hip.h and nothing else.
#pragma once
#include "flx_launch.h"
#include "flx_feature_state.h"
#include "../../include/fluctus_hip.h"
#include <string>
#include <vector>
#include <utility>
#include <rccl/rccl.h>      // types and prototypes only: librccl.so.1 is bound with dlopen at the first group call (api_group.hip)

using namespace flxd;

namespace flxd {
struct PendingCounters { void *user; int slot; };
struct PendingEvent { int kernel; hipEvent_t a, b; };
inline void freeAll(std::vector<void *> &v) { for (void *p : v) (void)hipFree(p); v.clear(); }

// ---- The call-sequence state machine.  The library defers and fuses behind the reference's entry points; what may be deferred, fused,
// left raw or started early depends on WHAT WAS CALLED SINCE -- one explicit phase, one transition function, every entry point declares
// its class of call.  (Rounds 2-3 kept this in ten booleans and five macros; tests/test_gpu_fuzz.py covers the (phase, call) pairs.)
//   PH_IDLE                nothing deferred, nothing known about the calls since the last `logic`
//   PH_DEFER_LOGIC         flx_wf_logic was called and is DEFERRED: the next call decides whether it runs fused with the material kernels
//   PH_DEFER_LOGIC_RAYGEN  ... and flx_wf_raygen behind it, deferred along (its queue does not exist yet)
//   PH_CHAIN               `logic` has been launched and only genRays / material kernels were enqueued since: the shadow kernel's inputs are
//                          complete and nothing enqueued since touches them (flx_wf_shadow)
//   PH_CHAIN_EXT           ... and the extension kernel is the last thing enqueued: flx_wf_shadow may start right behind `logic` (overlap 2)
//   PH_EXT                 the extension kernel is the last thing enqueued, the chain since `logic` is broken: flx_wf_shadow runs beside it (overlap 1, 2)
// Orthogonal DATA flags stay what they are: rawHits (hit records of the last extension launch are RAW, flx_trace.h), matQueuesEmpty,
// qs.extPend (lazy extension counter), cursorDirty.  The transition function, enter() and the entry points it serves: api_wavefront.hip.
enum Phase { PH_IDLE = 0, PH_DEFER_LOGIC = 1, PH_DEFER_LOGIC_RAYGEN = 2, PH_CHAIN = 3, PH_CHAIN_EXT = 4, PH_EXT = 5 };
enum Call {
    CALL_LOGIC, CALL_RAYGEN, CALL_MATERIALS, CALL_EXTEND, CALL_SHADOW,
    CALL_QUIET,        // enqueues at most a read-back of counters / nothing: flx_get_counters_async, flx_finish, flx_counter_totals, flx_profile_enable
    CALL_NEUTRAL,      // touches counters, cursor or framebuffer, never a hit record: flx_clear_queues, flx_pixel_index_*, flx_end_iteration_async, flx_read_pixels
    CALL_PEEK,         // may observe hit records or queues, or changes how later kernels run, without enqueueing work of its own: flx_stream, flx_queue_read, trace-stat getters, plain options
    CALL_OBSERVE       // everything else: exports, imports, uploads, parameters, resets, options that re-plan the schedule, the microkernels, the gather
};
}

// An optional feature keeps its device buffers and what it knows about them in ONE nested struct of the context: `allocs` owns the buffers,
// release() frees them and returns the struct to its default-constructed state.  flx_ctx::releaseFrameFeatures() lists the ones whose buffers are
// sized by the framebuffers (allocFrame and flx_destroy call it); a new feature adds its struct and one line there.
struct flx_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;              // the shadow kernel runs here, concurrently with the extension kernel
    hipEvent_t evPreExt = nullptr, evShadow = nullptr, evPostLogic = nullptr;
#ifdef FLX_LAB_NOJOIN
    // lab build only (-DFLX_LAB_NOJOIN; RESULTS INVALID, timing only): the ceiling of taking the any-hit kernel's tail off the step's critical
    // path -- the main stream does not join the shadow stream after flx_wf_shadow; the next-but-one `logic` waits for it instead (the throttle a
    // deferred NEE-consume kernel would impose).  The kernel reads a snapshot of the queue counters (the live ones are cleared under it).
    hipEvent_t evLab[2] = {nullptr, nullptr}; uint32_t labIter = 0; uint32_t *labCounters = nullptr;
#endif
    int phase = 0;                              // the call-sequence state machine (enum Phase): ONE explicit state instead of deferral / chain booleans
    int overlap = 2;                            // 0 serial | 1 shadow || extension | 2 shadow starts right after logic (the EFFECTIVE schedule)
    int overlapOpt = -1;                        // option "overlap": -1 = the default (pickSchedule), else as set
    uint32_t *spill2 = nullptr;
    // logic + material kernels as one pass (logic.hip: k_logic<FUSED>).  flx_wf_logic is DEFERRED while `fuse` is on: it is
    // launched by the next call -- fused with the material kernels when that call is flx_wf_materials (a flx_wf_raygen between
    // the two is deferred along and launched right after), as the plain kernel when it is anything else.  Every entry point
    // takes one step of the state machine first (enter()), so no call ever observes a state the separate kernels would not have produced.
    int fuse = 1;
    int extOrder = 0;                           // fused pass: extension queue lists the continuing paths 1 by path id | 2 merged with the regenerated ones by path id | 0 one segment per material queue; chosen at flx_upload_scene
    int fuseSet = 1;                            // BSDF types the fused pass inlines (logic.hip): 1 diffuse | 31 all six; chosen at flx_upload_scene
    int regroup = 0, regroupAuto = 0, regroupOpt = -1;           // all-types fused pass with its material step sorted by BSDF type inside each block (logic.hip: LOGIC_REGROUP): the EFFECTIVE choice (flx_upload_scene) | option "regroup": -1 = that choice, 0 / 1 as set
    int pendFirst = 0;                          // the deferred flx_wf_logic's `first` (phases PH_DEFER_*)
    bool matQueuesEmpty = false;                // the five material counters are known to be zero (cleared, nothing appended since)
    bool raygenQueueEmpty = false;              // ... and the raygen counter (ext_order 2 ranks the regenerated paths from zero: extOrderFor)
    uint32_t numTasks = 0;
    std::string err;
    State st {};
    Queues qs {};
    Scene sc {};
    Frame fr {};
    flx_render_params params {};
    bool haveParams = false;
    uint32_t hostPixelIdx = 0;
    // logic aux
    uint8_t *member = nullptr; uint32_t *blockCounts = nullptr;
    // the queue build's segment totals (two buffers: every logic pass flips queueParity, its build kernel zeroes the other one) and counter snapshot (logic.hip)
    uint32_t *queueAux = nullptr; uint32_t queueParity = 0;
    // in-kernel regeneration of the fused RAW pass (logic.hip: REGEN): look-back status words (one per wave, epoch-stamped: never reset), launch counter,
    // device error flag (a look-back that gave up), option "regen" (1: on where the pass allows it), and whether the LAST fused pass regenerated its
    // terminating paths itself -- then the genRays of the chain is not launched (flx_wf_materials)
    unsigned long long *lookback = nullptr; uint32_t logicEpoch = 0; uint32_t *logicError = nullptr; int regenOpt = 0; bool regenDone = false; bool regenUsed = false; int prepOpt = 1; bool prepDone = false;      // (off by default: profiles/r05_regen_ab.txt -- the look-back costs more than genRays)
    // trace aux
    uint32_t *spill = nullptr;
    unsigned long long *stats = nullptr;   // device, 16 counters
    unsigned long long *totals = nullptr;  // device, 8 running queue-length totals
    uint32_t *mkStats = nullptr;           // device RenderStats of the microkernel integrator (4 x u32)
    uint32_t *pinnedMk = nullptr; std::vector<std::pair<void *, int>> pendingMk; int nextMkSlot = 0;
    bool statsOn = false;
    int xcdRemap = 0;           // 1: each XCD gets a contiguous eighth of the queue (measured slower: round-robin keeps all XCDs on the same part of the tree)
    // which tree each traversal kernel walks: 2 = the reference's binary tree in the reference's visit order (bit-exact closest hit),
    // 4 = the 4-wide quantised tree over the same leaves (flx_wide.h): any-hit bit-exact by construction, closest hit exact up to
    // visit-order ties
    int shadowTree = 4, extendTree = 4;
    // persistent waves with lane refill for the 4-wide kernels (trace4r.hip): 0 = thread-per-ray kernels, n > 0 = refill when n lanes are idle
    // (closest hit: on by default -- refillMin 16, waitMax 32: kitchen 0.82 -> 0.61 ms per 4 M rays; any hit: off by default, pickSchedule)
    int refillExt = 16 | (32 << 8), refillShadow = 0;
    int refillShadowOpt = -1;                   // option "refill_shadow": -1 = the default (off), else as set
    // tail splitting of the thread-per-ray any-hit kernel (trace4.hip: k_shadow4s): budget of the pass over the queue | budget of a second pass << 8
    // (0 = the second pass finishes every ray); 0 = off (k_shadow4).  Continuation records: 64 B each, in sub-lists of splitCapA / splitCapB slots (numTasks / 2 and / 8 in all).
    // Option "shadow_split": -1 = the library's choice (the initial value), made at the launch from the render parameters -- FLX_SPLIT_DEFAULT where the
    // far -> near order runs (shadow rays toward an environment light: the long-tailed population), 0 elsewhere: effectiveSplit().  An explicit value holds.
    int shadowSplitOpt = -1;
    int shadowResume = 1;                       // option "shadow_resume": the suspended rays of a split launch WITHOUT second budget are finished 1 by persistent waves that refill from the records (trace4r.hip: k_trace4r_resume) | 0 one lane per record slot
    bool splitAllocFailed = false;              // the records of the library's own choice did not fit: the choice is 0 for this context
    uint32_t splitLastLimit = 0; bool splitLaunched = false;      // read-only option "shadow_split_suspended": the slot limit of the last split launch, and that there was one
    uint32_t splitParity = 0;                   // counter set of the next split launch (trace4.hip: launch_shadow4_split)
    uint32_t splitLimit = 0;                    // test hook (option shadow_split_limit): use only this many slots per sub-list (0 = all), to reach the full-list path
    uint32_t *splitCounts = nullptr; uint4 *splitRecA = nullptr, *splitRecB = nullptr; uint32_t splitCapA = 0, splitCapB = 0;
    // The persistent-wave extension kernel leaves RAW hit records (flx_trace.h): true from flx_wf_extend until they are committed -- by the
    // fused logic pass of the next iteration (the steady state: nothing else touches hit records between the extension kernel and logic),
    // or by k_materialise as soon as an entry point that could observe a hit record runs (transition(): commitRaw).
    bool rawHits = false;
    // PREVIOUS HITS PENDING.  The fused RAW pass with option "lazy_hit_commit" does the commit in registers and stores neither the hit point
    // nor the uv record (logic.hip: LAZY): the paths it served keep their RAW {u, v, triangle, t}, and the ray those were traced with survives in
    // st.other[] (flx_device.h).  True from that pass until the extension launch of an INTACT chain -- only genRays / the fused pass's material kernel /
    // quiet calls since the pass: its queue holds every one of those paths and the kernel overwrites every such record -- or until k_settle_hits has
    // written the two records the pass left out, which transition() asks for before any other call that could see them or break that chain.
    // Never true together with rawHits: the pass that sets it consumes rawHits, and an extension launch clears or settles it before it sets rawHits.
    bool prevHitsPending = false;
    int lazyCommitOpt = 1;                      // option "lazy_hit_commit"
    bool cursorDirty[2] = {false, false};       // block cursors of the persistent kernels (closest hit, any hit) used since they were last zeroed

    uint32_t wideInfo[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // flx_scene_info
    RefitTables rf;             // flx_upload_scene -> flx_update_triangles (flx_launch.h)
    bool wideOK = false;        // the uploaded scene has a wide tree whose exactness conditions hold (nested boxes)
    uint32_t spillLevels = 0;   // levels per lane in each spill buffer (sized at upload from the tree's depth)
    int eagerBump = 0;          // A/B: bump the extension counter right after raygen / materials (option eager_bump)
    int denoiser = 0;           // USE_OPTIX_DENOISER of the reference: accumulate the denoiser feature buffers
    std::vector<void *> aovAllocs;
    // flx_denoise (denoise.hip): working set (ping-pong radiance, packed guides) and which = 6; allocated by the first call, freed with the
    // framebuffers or the feature buffers.  have: which = 6 holds the output of a flx_denoise on the current buffers
    struct Denoise {
        std::vector<void *> allocs;
        float4 *e[2] = {nullptr, nullptr}, *g = nullptr; float2 *g2 = nullptr; float *out = nullptr;
        bool have = false;
        void release() { freeAll(allocs); *this = Denoise(); }
    } dn;
    int moments = 0;            // option "moments": the splats accumulate the luminance moments (Frame::moments, which = 7)
    std::vector<void *> momAllocs;
    // temporal reprojection (TemporalState): the two G-buffer slots of 2 float4 per pixel, allocated by the first flx_gbuffer / flx_gbuffer_write; the
    // accumulation and the moments as flx_history_capture copied them (histMomBuf null: "moments" was never on at a capture); one object id per
    // pixel beside each slot, swapped with the slots, allocated by the first of those calls that finds "motion_history" on; likewise one float2 of
    // barycentrics per pixel beside each slot under "deform_history".  Freed with the framebuffers.
    struct Temporal {
        std::vector<void *> allocs;
        float4 *gb[2] = {nullptr, nullptr}, *hist = nullptr, *histMomBuf = nullptr; uint32_t *objPlane[2] = {nullptr, nullptr};
        float2 *baryPlane[2] = {nullptr, nullptr};
        // history rectification: the accumulation and the moments as flx_history_mark copied them (markMomBuf null: "moments" was
        // never on at a mark), the prepare records and the lambda plane of flx_history_rectify; allocated by the first flx_history_mark
        float4 *mark = nullptr, *markMomBuf = nullptr, *rcRec = nullptr; float *lambda = nullptr;
        TemporalState state;
        void release() { freeAll(allocs); *this = Temporal(); }
    } temporal;
    int motionHistory = 0;      // option "motion_history": flx_objects_pose keeps a captured history, flx_reproject follows the posed objects
    int deformHistory = 0;      // option "deform_history": every move of triangles keeps a captured history, flx_reproject follows the vertices
    // the adaptive microkernel render (ActiveListState): flag bytes, block counts and the list of active pixels, allocated by the first
    // flx_mk_adaptive_update / flx_mk_active_write for state.pix pixels and freed with the framebuffers
    struct Adaptive {
        std::vector<void *> allocs;
        uint8_t *flags = nullptr; uint32_t *scratch = nullptr, *list = nullptr, *countDev = nullptr;
        ActiveListState state;
        void release() { freeAll(allocs); *this = Adaptive(); }
    } ad;
    void releaseFrameFeatures() { dn.release(); temporal.release(); ad.release(); }
    // objects over the uploaded triangles (flx_objects_define / flx_objects_pose; pose.hip): the device tables and, per object,
    // its member count.  The buffers are sized by the scene: a successful flx_upload_scene, a new definition and flx_destroy release them.
    // have false = no objects are defined.
    struct Objects {
        std::vector<void *> allocs;
        ObjectTables t;
        std::vector<uint32_t> counts;
        bool have = false;
        PoseState pose;
        // option "motion_history": the object of every triangle (FLX_NO_OBJECT: none) and the per-object motion table of flx_reproject_motion.h
        // (four float4 per object) with its pinned staging copy; made by the first flx_gbuffer or flx_objects_pose that finds the option on
        uint32_t *objectOfTri = nullptr; float4 *motion = nullptr, *motionPinned = nullptr;
        void release() { freeAll(allocs); if (motionPinned) (void)hipHostFree(motionPinned); *this = Objects(); }
    } ob;
    // the emissive triangles as lights (MeshLightState; flx_mesh_light.h, mesh_light.hip): the host's ascending list (made by every
    // flx_upload_scene, whatever the option says) and the device table, allocated by the first build for this scene.  The buffers are sized by the
    // scene: a successful flx_upload_scene and flx_destroy release them; the option and the state survive an upload.
    struct MeshLight {
        std::vector<void *> allocs;
        std::vector<uint32_t> list;
        MeshLights t;
        MeshLightState state;
        void releaseBuffers() { freeAll(allocs); t = MeshLights(); }
    } ml;
    int nodeLayout = 1;         // 1 = sibling-pair record numbering (see flx_upload_scene), 0 = DFS
    int numCUs = 256;
    // multi-GPU group (flx_group_*): RCCL communicator of this rank, root-side staging
    ncclComm_t comm = nullptr;
    bool commShared = false;                    // same-device local group: no communicator, device copies instead
    struct Gather {
        std::vector<void *> allocs;
        float *stage = nullptr, *full = nullptr; size_t stageFloats = 0, fullFloats = 0;
        void release() { freeAll(allocs); *this = Gather(); }
    } gather;
    // owned device allocations
    std::vector<void *> sceneAllocs, envAllocs, frameAllocs, fixedAllocs, spillAllocs;
    // async counter read-back
    flx_queue_counters *pinned = nullptr; int pinnedSlots = 64, nextSlot = 0;
    uint32_t *pinnedIdx = nullptr; int nextIdxSlot = 0;
    std::vector<PendingCounters> pending;
    // profiling
    int profile = 0;              // 0 off | 1 time every kernel | 2 the traversal kernels + span | 3 the extension kernel only | 4 extension + logic + shadow
    hipEvent_t spanStart = nullptr;             // pending FLX_K_TRACE_SPAN start (recorded in flx_wf_extend)
    std::vector<PendingEvent> events;
    std::vector<hipEvent_t> eventPool;
    double kMs[FLX_K_COUNT] = {0}; uint64_t kLaunches[FLX_K_COUNT] = {0};
};

#define HIPCHK(c, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { (c)->err = std::string(#expr) + ": " + hipGetErrorString(e_); return 1; } } while (0)
#define NEED(c, cond, msg) do { if (!(cond)) { (c)->err = msg; return 1; } } while (0)
#define ENTER(c, call) do { if (enter(c, call)) return 1; } while (0)
#define READY(c, call) do { ENTER(c, call); NEED(c, (c)->haveParams, "set params first (flx_set_params)"); NEED(c, (c)->sc.bnodes, "upload a scene first (flx_upload_scene)"); HIPCHK(c, hipSetDevice((c)->device)); } while (0)
#define LAUNCHED(c) HIPCHK(c, hipGetLastError())

namespace flxd {
template <class T> int dalloc(flx_ctx *c, std::vector<void *> &own, T **p, size_t count)
{
    void *d = nullptr;
    HIPCHK(c, hipMalloc(&d, (count ? count : 1) * sizeof(T)));
    own.push_back(d);
    *p = (T *)d;
    return 0;
}

inline hipEvent_t getEvent(flx_ctx *c)
{
    if (!c->eventPool.empty()) { hipEvent_t e = c->eventPool.back(); c->eventPool.pop_back(); return e; }
    hipEvent_t e; (void)hipEventCreate(&e); return e;
}
struct ScopedTimer {
    flx_ctx *c; int k; hipStream_t s; hipEvent_t a = nullptr, b = nullptr;
    bool on;
    // profile level 1 = every kernel, 2 = the two traversal kernels + their span, 3 = the extension kernel only, 4 = the three kernels the bench line
    // prices against a roof: extension, (fused) logic, shadow  (each event pair costs a few us of stream time)
    ScopedTimer(flx_ctx *c_, int k_, hipStream_t s_ = nullptr) : c(c_), k(k_), s(s_ ? s_ : c_->stream)
    {
        on = c->profile == 1 || (c->profile == 2 && (k == FLX_K_EXTEND || k == FLX_K_SHADOW)) || (c->profile == 3 && k == FLX_K_EXTEND) ||
             (c->profile == 4 && (k == FLX_K_EXTEND || k == FLX_K_SHADOW || k == FLX_K_LOGIC || k == FLX_K_LOGIC_FUSED));
        if (on) { a = getEvent(c); b = getEvent(c); (void)hipEventRecord(a, s); }
    }
    ~ScopedTimer() { if (on) { (void)hipEventRecord(b, s); c->events.push_back({k, a, b}); } }
};

// what one unit defines for the others
extern thread_local std::string g_create_error;     // api.hip: the error of a call that has no context to carry it (flx_last_error(nullptr))
int enter(flx_ctx *c, Call call);                   // api_wavefront.hip: one step of the state machine; every entry point takes it first (ENTER)
void flushExt(flx_ctx *c);                          // api_wavefront.hip: the lazy extension counter
int fuseSetNow(const flx_ctx *c);                   // api_wavefront.hip: the BSDF set the fused pass inlines now (read-only options)
float wideClampFor(float maxAbsCoord);              // api_refit.hip: the bound of |1 / dir| in the wide node test for a scene reaching this far (flx_trace4.h: WRay::setup)
int motionTables(flx_ctx *c);                       // api_refit.hip: objectOfTri and the motion table, made once per definition while "motion_history" is on
int meshLightsSync(flx_ctx *c);                     // api_mesh_light.hip: (re)build the table of emissive triangles on the stream when the option is on and it is stale
int wideFar(const flx_ctx *c);                      // api_refit.hip: 1 when sc.wideClamp is the far clamp (read-only option "wide_far")
void pickSchedule(flx_ctx *c);                      // api.hip: the effective overlap / refill_shadow (options, flx_upload_scene)
int effectiveSplit(const flx_ctx *c);               // api.hip: "shadow_split" under the current render parameters (option or the library's choice)
int splitNow(const flx_ctx *c);                     // api.hip: ... and what the next flx_wf_shadow really launches with it (0 where another any-hit kernel runs)
int splitPrepare(flx_ctx *c);                       // api.hip: allocate the records of that launch, or fall back to 0 when the library's own choice does not fit
int splitBuffers(flx_ctx *c, bool second);          // api.hip: the continuation records, allocated on first use (the second set only for a second budget)
}
