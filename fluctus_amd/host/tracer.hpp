// tracer.hpp -- headless render driver: the host loop that sequences the wavefront kernels.
//
// Restates the wavefront branch of the reference's Tracer (reference: src/tracer.hpp:31-43,
// src/tracer.cpp): resetParams (:38-52), init (:55-80), initHierarchy (:574-590, BVH cache keyed by a hash of
// the mesh), update() WF branch (:222-266, :302-340) and runBenchmark() WF body (:362-528, CSV schema
// `scene;time;primary;extension;shadow;total;samples` :393), plus the microkernel integrator's branches of the same
// functions and renderSingle (:95-187), and the denoiser step of update() / renderSingle (:160-165, :310-328)
// with flx_denoise in place of OptiX.  No window, no GL.
#pragma once
#include <memory>
#include <string>
#include <vector>
#include "hipcontext.hpp"
#include "history_state.hpp"
#include "rebuild_job.hpp"

namespace fluctus {

class Tracer {
public:
    Tracer(int width, int height, int device = 0, uint32_t numTasks = 1u << 20);
    // one process driving several GPUs of a node: devices[0] is the root; every device runs the complete wavefront loop
    // on its own interleaved pixel subset with its own numTasks paths, scene replicated; tiles are gathered over RCCL for read-back.
    // The same device may be listed more than once (1-GPU stand-in for N ranks).
    Tracer(int width, int height, const std::vector<int> &devices, uint32_t numTasks);
    uint32_t numRanks() const { return 1u + (uint32_t)peers.size(); }
    // full-resolution accumulation image (rgb sum, sample count) assembled from all ranks
    void readAccumulation(std::vector<float> &rgba);
    ~Tracer();

    void init(int width, int height, const std::string &sceneFile);             // file path or "proc:<kind>:<tris>:<seed>"
    void setEnvMap(const std::string &hdrFile);                                   // Tracer::initEnvMap
    // move the scene's triangles (same count and materials): refits the host tree and every rank's device trees (flx_update_triangles), re-derives
    // worldRadius, drops the reprojection history and restarts the accumulation.  Topology is kept: init() rebuilds when quality matters.
    void updateGeometry(const std::vector<flx_triangle> &tris);
    // move a SUBSET of them (a dragged object): tris[k] replaces triangle indices[k], indices strictly ascending.  Every rank's
    // flx_update_triangles_subset and the host tree's BVH::refitSubset recompute only the boxes above the listed triangles; every other box --
    // a clipped SBVH leaf among them -- keeps its bytes.  Everything else, the rebuild policy included, as the full overload;
    // a background tree that finishes later is refitted to the full current triangle set.  A refused call (bad list or triangle) throws and
    // leaves the old geometry in place.
    void updateGeometry(const std::vector<uint32_t> &indices, const std::vector<flx_triangle> &tris);
    // Move OBJECTS by their transforms.  defineObjects: objectOfTriangle[i] < nobjects is the object of triangle i,
    // FLX_NO_OBJECT a triangle that never moves; the REST pose is the scene's triangles at this moment (the Tracer keeps the members' rest
    // triangles; every rank gets the definition, flx_objects_define).  nobjects == 0 drops the definition, and so does init().  Without
    // arguments: the objects the OBJ loader found (Scene::objectOfTriangle / objectNames).
    // poseObjects: xforms12[12 k ..] is the 3 x 4 row-major ABSOLUTE rest -> world transform of object ids[k] (strictly ascending); objects not
    // listed keep their pose.  Every rank poses the triangles on the device (flx_objects_pose: 48 bytes per object cross the bus); the host's
    // triangle copy is posed with the same function (csrc/flx_pose.h) and the host tree refitted (BVH::refitSubset) -- worldRadius, the rebuild
    // policy's snapshots and refits need it.  Otherwise updateGeometry(indices, tris): the rebuild policy takes part unchanged, and the rest pose
    // survives a rebuild (the ranks are given the definition again behind every topology upload).  A refused call throws and leaves everything as it was.
    void defineObjects(const std::vector<uint32_t> &objectOfTriangle, uint32_t nobjects);
    void defineObjects();
    void poseObjects(const std::vector<uint32_t> &ids, const std::vector<float> &xforms12);
    uint32_t numObjects() const { return nObjects; }
    // Rebuild policy, default Off: updateGeometry only refits, exactly as described above.  Otherwise every updateGeometry
    // reads the root rank's flx_tree_cost after its refit and forms  ratio = cost of the 4-wide tree now / the same right after the last topology
    // upload  (flxTreeCostValue: (S_node + S_tri) / A_root).  When ratio > threshold and no rebuild is in flight:
    //   Blocking    builds the SBVH for the new triangles inside the call and uploads it (no refit behind it: the pose is the tree's);
    //   Background  starts a worker thread (RebuildJob) on a snapshot of the new triangles and returns; frames go on with refits.  A finished
    //               build is picked up at the start of the next updateGeometry or update(): the new topology is uploaded to every rank with its
    //               snapshot, the cost baseline is re-read, then one refit brings it to the current triangles (skipped when none moved since
    //               the snapshot) -- so the ratio never hides the drift since the snapshot.  worldRadius, the dropped reprojection history and the
    //               restarted accumulation as in updateGeometry.  The upload still runs on the calling thread (build_wide and the copies).
    // At most one job is in flight; init() discards one.  The environment map, the parameters and what the first upload chose for the options
    // "fuse_set" / "ext_order" survive a swap.  threshold: required for Blocking / Background, > 1 and finite, else the call throws; DESIGN.md
    // 4.10.1 tabulates what a value means.  A NaN ratio (degenerate root box) is "no decision".  Switching the policy on after geometry updates
    // takes the trees as they stand then as the baseline: set the policy before the first updateGeometry.  Switching to Off keeps a job in
    // flight; it is adopted, and refitted to the triangles of that moment, once a policy is on again.
    enum RebuildMode { RebuildOff = 0, RebuildBlocking = 1, RebuildBackground = 2 };
    void setRebuildPolicy(RebuildMode mode, double threshold);
    RebuildMode getRebuildMode() const { return rebuildMode; }
    uint32_t rebuildCount() const { return rebuilds; }                            // topologies uploaded by the policy since construction
    bool rebuildPending() const { return job.active(); }                          // a job was started and its tree is not uploaded yet
    void waitForRebuild() { job.wait(); }                                         // joins the worker; swaps nothing (the next updateGeometry / update does)
    double lastCostRatio() const { return lastRatio; }                            // of the last updateGeometry under a policy (1 after a Blocking rebuild); NaN: none yet
    std::array<double, 8> treeCost() { return clctx->treeCost(); }                // the root rank's flx_tree_cost
    // ---- TEST HOOKS ONLY (tests/test_gpu_rebuild.py); a host has no use for them
    // holdRebuild (RebuildJob::hold): while held, a finished build stays unpublished, so a test decides between which two calls a job completes;
    // waitForRebuild and the destructor release it.  getOption / treeRead: a rank's HipContext::getOption / flx_tree_read.
    void holdRebuild(bool on) { job.hold(on); }
    int getOption(uint32_t rank, const std::string &name);
    void treeRead(uint32_t rank, int which, std::vector<uint8_t> &out);
    // ----
    void update();                                                                // one frame (iteration 0 = 2-bounce preview x3)
    // benchmark-style iterations for `seconds` (reference: 30 s per scene) or exactly `iterations` if > 0;
    // returns the CSV text (header + one row per 0.5 s of wall time)
    std::string runBenchmark(double seconds, int iterations = 0);
    // final-frame render: exactly `spp` samples in every pixel (reference: src/tracer.cpp:95-187).  Switches to the
    // microkernel integrator and turns Russian roulette off, as the reference does; needs numTasks >= width*height.
    void renderSingle(int spp, bool denoise = false);                             // denoise: also fill the denoiser feature buffers (and denoise, strength > 0)
    // renderSingle to a noise threshold: every pixel takes minSpp samples, then only the pixels whose relative standard error of the
    // mean luminance is still above `threshold` (and their 3 x 3 neighbours) go on, to at most maxSpp.  Same set-up as renderSingle (roulette off,
    // single GPU, throws like it); turns the option "moments" on for the render when it is off and restores it.  Returns the samples taken;
    // the per-pixel count is the accumulation's w.
    uint64_t renderAdaptive(int minSpp, int maxSpp, float threshold, bool denoise = false);
    // the reference's denoiser strength slider (src/tracer_ui.cpp:359): blend = 1 - strength.  0 (this library's default; the reference's is 1,
    // INTEGRATION.md) only fills the feature buffers; > 0 denoises the preview every 10th frame from frame 10 on, and renderSingle's final frame.
    // Single-GPU: throws on a multi-rank Tracer.
    void setDenoiserStrength(float s);
    float getDenoiserStrength() const { return denoiserStrength; }
    void setDenoiser(bool on) { useDenoiser = on; for (auto *c : ranks()) c->recompileKernels(on); applyMoments(); iteration = 0; }
    // which filter the denoiser step runs: Guided (default, flx_denoise) or VarianceGuided (flx_denoise_variance_guided, which also needs
    // the luminance moments: while the denoiser is on in this mode, every rank accumulates them).  Same schedule either way.
    enum DenoiserMode { Guided = 0, VarianceGuided = 1 };
    void setDenoiserMode(DenoiserMode m);
    DenoiserMode getDenoiserMode() const { return denoiserMode; }
    // Temporal reprojection, default off.  On: a parameter update (camera move) on the WAVEFRONT integrator no longer throws the
    // accumulation away -- update() captures it with the old camera's G-buffer, traces the new camera's, runs today's reset sequence unchanged and
    // reprojects the capture into the new view before the first logic pass.  Without a history (first frame, new scene, resize) only the
    // G-buffer is traced.  The denoiser schedule then counts frames since the last DISCARDED history instead of since the last move, so the filter
    // also runs on frames after a move.  The history is kept only when NOTHING BUT THE CAMERA changed since the G-buffer it belongs to was traced:
    // an update that changes the lights, the environment map, the bounce count or the sampling switches, a frame on the other integrator,
    // renderSingle and runBenchmark all discard it, and the next frame restarts as on the default path.  The frame after a move is still the
    // 2-bounce preview (three passes), now added onto the kept image: under continuous motion the image drifts towards the 2-bounce estimate
    // until the camera rests.  The interactive microkernel branch overwrites the pixel with its preview splat and keeps today's reset;
    // renderSingle is unaffected.  Single-GPU: throws on a multi-rank Tracer.
    void setTemporalReprojection(bool on);
    bool getTemporalReprojection() const { return history.temporal(); }
    void setMaxHistory(float n);                                                  // flx_reproject's max_history (>= 1; default 32)
    // Motion-aware reprojection, default off; needs setTemporalReprojection(true) and throws without it or on a multi-rank
    // Tracer.  On: poseObjects on the WAVEFRONT integrator no longer throws the accumulation away -- it captures the history (at most once per
    // frame, shared with a camera change pending in the same frame), poses, and arms the next update() to trace the G-buffer, run the reset
    // sequence unchanged and reproject, each posed object's pixels looking their history up where the object was.  Everything else that changes
    // the geometry restarts as ever: updateGeometry in either form, a rebuild the policy runs or adopts, the microkernel branch, renderSingle.
    void setMotionReprojection(bool on);
    bool getMotionReprojection() const { return history.motion(); }
    // Per-vertex reprojection, default off; needs setTemporalReprojection(true) and throws without it, on a multi-rank Tracer
    // and while motion-aware reprojection is on (the two options refuse each other on the device; this one follows poseObjects as well).  On:
    // updateGeometry in both forms and poseObjects on the WAVEFRONT integrator keep the accumulation as poseObjects does under
    // setMotionReprojection -- capture (at most once per frame), move, and the next update() traces the G-buffer, resets and reprojects, each
    // moved triangle's pixels looking their history up where that point of the triangle was.  A rebuild the policy runs or adopts, the
    // microkernel branch and renderSingle restart as ever.
    void setDeformReprojection(bool on);
    bool getDeformReprojection() const { return history.deform(); }
    float getMaxHistory() const { return maxHistory; }
    // History rectification, default off; needs setTemporalReprojection(true) and throws without it or on a multi-rank Tracer.
    // On: a frame that reprojects runs exactly as without the switch, preview passes included, and ends on flx_history_mark (the preview's
    // samples count as history, as they effectively do anyway); the frame at whose end `delay` frames have been rendered since that G-buffer
    // runs flx_history_rectify once, unless a newer reprojection has replaced the mark by then -- under continuous motion it never fires, it
    // fires once the view rests.  The delay defaults to 2 maxBounces + 2 frames: the wavefront integrator splats a path when it ENDS, so for the
    // first ~maxBounces frames after a reset the samples over-represent short paths, which would read as a change everywhere.
    // And a moved, resized or re-coloured AREA LIGHT no longer discards the accumulation: it takes the reprojection route like a camera move
    // (capture, G-buffer, reset, reprojection, mark) and the rectification sheds what the new light contradicts.  Every other parameter change,
    // setEnvMap included, discards the history as ever.  lastRetainedShare: the mark's sample count after the last rectify over the one before
    // it (NaN before one; two blocking reads per rectify while measureRetained is set).
    void setHistoryRectification(bool on);
    bool getHistoryRectification() const { return history.rectify(); }
    void setRectifyDelay(int frames);                                             // >= 1; 0 = the default, 2 maxBounces + 2
    uint32_t getRectifyDelay() const { return history.rectifyDelayFrames(params.maxBounces); }
    bool measureRetained = false;
    double lastRetainedShare() const { return retainedShare; }
    uint32_t rectifyCount() const { return rectifies; }                           // how many times update() has run flx_history_rectify
    // Emissive triangles as lights, default off: only the microkernel integrator sees them, so while this is on update() takes
    // its microkernel branch (as renderSingle forces it) and toggleRenderer() to the wavefront loop THROWS -- lamps never go silently dark.
    // Single-GPU like that integrator: throws on a multi-rank Tracer.  meshLightCount: the lights listed on the device (throws while off).
    void setMeshLights(bool on);
    bool getMeshLights() const { return meshLightsOn; }
    uint32_t meshLightCount() { return clctx->meshLightCount(); }
    // ... and the wavefront integrator too, default off: throws unless setMeshLights(true) came first and on a multi-rank Tracer.
    // While on, toggleRenderer() reaches the wavefront loop and update() renders the lamps there (the unfused chain: INTEGRATION.md).  Switching it
    // off on the wavefront loop returns to the microkernel branch; setMeshLights(false) clears it.
    void setMeshLightsWavefront(bool on);
    bool getMeshLightsWavefront() const { return meshLightsWavefrontOn; }
    void toggleRenderer();                                                        // src/tracer.cpp:881-886 (no history across integrators)
    void setOption(const std::string &name, int value) { for (auto *c : ranks()) c->setOption(name, value); }   // every rank (HipContext::setOption)
    bool usesWavefront() const { return useWavefront; }
    void saveImage(const std::string &filename) { clctx->saveImage(filename, params); }

    RenderParams &getParams() { return params; }
    void paramsChanged() { paramsUpdatePending = true; }
    HipContext *getContext() { return clctx.get(); }
    Scene *getScene() { return scene.get(); }
    uint32_t getIteration() const { return iteration; }
    const QueueCounters &lastCounters() const { return lastCnt; }
    // on-disk caches in the reference's formats and names (src/tracer.cpp:573-590, 625-684): <dir>/hierarchy_<hash>.bin and
    // <dir>/state_<hash>.dat, hash = XXH64 of the scene file in decimal (of the triangle array for procedural scenes)
    std::string hierarchyCacheDir = "";                                           // empty = no on-disk BVH cache ("data/hierarchies" in the reference)
    std::string stateDir = "";                                                    // "data/states" in the reference
    bool saveState() const;                                                       // Tracer::saveState: camera, lights, sampling and post-processing parameters
    bool loadState();                                                             // false when there is no (complete) state file for this scene
    const std::string &getSceneHash() const { return sceneHash; }
    float cameraRotation[2] = {0.0f, 0.0f};                                       // UI state the file carries (src/tracer.hpp: cameraRotation, cameraSpeed)
    float cameraSpeed = 1.0f;

private:
    void resetParams(int width, int height);
    void initCamera();
    void initPostProcessing();
    void initAreaLight();
    void initHierarchy();
    void updateMicrokernel();

    RenderParams params;
    std::unique_ptr<Scene> scene;
    std::unique_ptr<EnvironmentMap> envMap;
    std::unique_ptr<HipContext> clctx;                                            // rank 0
    std::vector<std::unique_ptr<HipContext>> peers;                               // ranks 1..R-1 (multi-GPU wavefront path)
    std::vector<HipContext *> ranks() { std::vector<HipContext *> r{clctx.get()}; for (auto &p : peers) r.push_back(p.get()); return r; }
    BVH *bvh = nullptr;
    // the rebuild policy
    RebuildMode rebuildMode = RebuildOff;
    double rebuildThreshold = 0.0;
    double baselineCost = 0.0;                                                    // flxTreeCostValue of the 4-wide tree right after the last topology upload; valid while haveBaseline
    bool haveBaseline = false;
    double lastRatio = 0.0;                                                       // (set to NaN by the constructor)
    uint32_t rebuilds = 0;
    bool movedSinceSnapshot = false;                                              // an updateGeometry happened since the job in flight took its snapshot
    RebuildJob job;
    // objects (defineObjects): per member -- a triangle that belongs to an object, ascending -- its triangle, its object and its rest triangle
    uint32_t nObjects = 0;
    std::vector<uint32_t> objMemberTri, objMemberObj;
    std::vector<flx_triangle> objRest;
    void defineObjectsOnRanks(const std::vector<flx_triangle> &tris);             // flx_objects_define on every rank: `tris` with the members' rest triangles put in
    double wideCost();                                                            // flxTreeCostValue of the root rank's 4-wide tree now
    void uploadTopology(BVH *tree, const std::vector<flx_triangle> &tris);        // every rank; keeps the first upload's option choices; re-reads the baseline
    void refitAll(const std::vector<flx_triangle> &tris);                         // every rank + the host tree + the scene's triangles
    bool adoptFinishedRebuild();                                                  // a finished job -> uploaded and refitted to the current triangles
    void afterMove();                                                             // geometryChanged + the rebuild policy: what every move ends on
    void geometryChanged();                                                       // worldRadius, history, accumulation: what a change of the trees resets
    uint32_t iteration = 0;
    bool paramsUpdatePending = true;
    bool useDenoiser = false;                                                     // the feature buffers (+ flx_denoise while denoiserStrength > 0)
    float denoiserStrength = 0.0f;
    DenoiserMode denoiserMode = Guided;
    bool momentsOn = false;                                                       // the ranks' option "moments" as applyMoments left it
    void applyMoments();                                                          // "moments" on iff the denoiser is on in VarianceGuided mode
    void denoiseStep();                                                           // the mode's filter with blend = 1 - strength (rank 0; single-GPU)
    // whether the device holds a history worth keeping: history_state.hpp decides and keeps the books, this class calls the device
    HistoryState history;
    float maxHistory = 32.0f;
    uint32_t rectifies = 0;
    double retainedShare = 0.0;                                                   // (set to NaN by the constructor)
    void refuseSwitch(const char *setter, bool on, bool needsTemporal = true) const;   // what the reprojection switches refuse alike: several ranks; on without temporal reprojection
    // the body of both updateGeometry overloads and poseObjects; keepSwitch: the switch under which this kind of move keeps the history
    template <class MoveRanks, class MoveHost> void moveTriangles(bool keepSwitch, MoveRanks moveRanks, MoveHost moveHost);
    bool meshLightsOn = false, meshLightsWavefrontOn = false;
    bool useWavefront = true;                                                     // this library's default; the reference starts on MK (src/tracer.cpp:11)
    QueueCounters lastCnt {};
    std::string sceneName;
    std::string sceneHash;
};

} // namespace fluctus
