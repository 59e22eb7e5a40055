// hipcontext.hpp -- C++ device context over the C ABI of libfluctus_hip.so.
//
// Same method surface as the reference's `class CLContext` (reference: src/clcontext.hpp:31-79) for the
// wavefront path and the microkernel integrator, so the Tracer loop reads like the reference's; every method forwards to one flx_* entry
// point (include/fluctus_hip.h).  The HIP library is bound with dlopen at construction: libfluctus_host.so
// itself has no GPU dependency and there is NO CPU fallback -- a missing library or device throws.
#pragma once
#include <string>
#include <vector>
#include <array>
#include <cstdint>
#include "../../include/fluctus_hip.h"
#include "../csrc/flx_adaptive.h"       // FLX_AD_DEFAULT_*
#include "scene.hpp"
#include "bvh.hpp"
#include "envmap.hpp"

namespace fluctus {

typedef flx_render_params RenderParams;
typedef flx_queue_counters QueueCounters;
struct PerfNumbers { double primary = 0, extension = 0, shadow = 0, samples = 0, total = 0; };   // src/clcontext.hpp:19-24
struct RenderStats { uint64_t primaryRays = 0, extensionRays = 0, shadowRays = 0, samples = 0; }; // src/geom.h:254-260 (64-bit here)

class HipContext {
public:
    HipContext(int device, uint32_t numTasks, const std::string &libPath = "");
    ~HipContext();
    HipContext(const HipContext &) = delete;

    void uploadSceneData(BVH *bvh, Scene *scene);                 // src/clcontext.cpp:522-566
    // ... with the triangles the tree was built for given apart from the scene's (a rebuilt tree and its snapshot: Tracer's rebuild policy)
    void uploadSceneData(BVH *bvh, Scene *scene, const std::vector<flx_triangle> &tris);
    void updateTriangles(const std::vector<flx_triangle> &tris);  // flx_update_triangles: the uploaded triangles move, both trees are refitted on the device
    // flx_update_triangles_subset: tris[k] replaces triangle indices[k] (strictly ascending); only the boxes above them are refitted
    void updateTriangles(const std::vector<uint32_t> &indices, const std::vector<flx_triangle> &tris);
    // flx_objects_define / flx_objects_pose: objects over the uploaded triangles (objectOfTriangle[i] < nobjects, or
    // FLX_NO_OBJECT), then moved by a 3 x 4 row-major matrix each -- the absolute rest -> world transform of object ids[k] (strictly ascending) at
    // xforms12[12 k]; the triangles are posed on the device and go through the subset refit
    void defineObjects(const std::vector<flx_triangle> &rest, const std::vector<uint32_t> &objectOfTriangle, uint32_t nobjects);
    void poseObjects(const std::vector<uint32_t> &ids, const std::vector<float> &xforms12);
    // flx_tree_cost: {A_root, S_node, S_leaf, S_tri} of the binary tree [0..3] and of the 4-wide tree [4..7] as they stand on the device (blocking);
    // flxTreeCostValue (include/fluctus_hip.h) turns four of them into one figure
    std::array<double, 8> treeCost();
    uint32_t meshLightCount();                                 // flx_mesh_lights_read: the emissive triangles listed as lights (option "mesh_lights" on)
    void treeRead(int which, std::vector<uint8_t> &out);          // flx_tree_read (test hook): device array `which` of the uploaded scene
    void createEnvMap(EnvironmentMap *map);                       // src/clcontext.cpp:467-511
    void updateParams(const RenderParams &params);                // src/clcontext.cpp:703-707
    void enqueueWfResetKernel(const RenderParams &params);        // src/clcontext.cpp:765-770
    void enqueueWfRaygenKernel(const RenderParams &params);
    void enqueueWfExtRayKernel(const RenderParams &params);
    void enqueueWfShadowRayKernel(const RenderParams &params);
    void enqueueWfLogicKernel(const RenderParams &params, bool firstIteration);
    void enqueueWfMaterialKernels(const RenderParams &params);
    // microkernel integrator (src/clcontext.hpp:45-51)
    void enqueueResetKernel(const RenderParams &params);
    void enqueueRayGenKernel(const RenderParams &params);
    void enqueueNextVertexKernel(const RenderParams &params);
    void enqueueBsdfSampleKernel(const RenderParams &params);
    void enqueueSplatKernel(const RenderParams &params);
    void enqueueSplatPreviewKernel(const RenderParams &params);
    void fetchStatsAsync();                                       // src/clcontext.cpp:642-646; folded into statsAsync by finishQueue()
    void recompileKernels(bool useDenoiser);                      // src/clcontext.cpp:852-874: here only the denoiser-feature switch
    // kernel selection the reference makes through Settings + recompile (src/settings.cpp): "extend_tree" / "shadow_tree" 2 | 4, ...
    // (include/fluctus_hip.h, flx_set_option)
    void setOption(const std::string &name, int value);
    int getOption(const std::string &name);                    // flx_get_option: current value, e.g. what the upload picked for "fuse_set"
    void enqueueClearWfQueues();                                  // src/clcontext.cpp:877-883
    void enqueueGetCounters(QueueCounters *cnt);                  // async; valid after finishQueue()
    void enqueuePostprocessKernel(const RenderParams &params);
    // DenoiserOptix::denoise (reference: src/denoiser/OptixDenoiser.cpp) as the guided a-trous filter of flx_denoise: the feature buffers in,
    // the preview out; blend = DenoiserOptix' blendFactor (0 = fully denoised).  Asynchronous, like enqueuePostprocessKernel.
    struct DenoiseParams { int iterations = 5; float sigmaColor = 2.0f, sigmaNormal = 0.3f, sigmaAlbedo = 0.1f, blend = 0.0f; };
    void denoise(const DenoiseParams &params);
    // the variance-guided filter (flx_denoise_variance_guided): needs the options "denoiser" and "moments"; otherwise as denoise()
    struct DenoiseVgParams { int iterations = 5; float sigmaLuminance = 4.0f, sigmaNormal = 0.3f, sigmaAlbedo = 0.1f, blend = 0.0f; };
    void denoiseVarianceGuided(const DenoiseVgParams &params);
    // adaptive sampling on the microkernel integrator (flx_mk_adaptive_update / _clear): classify the pixels by the luminance
    // moments, install the list of active ones for the following enqueueRayGenKernel ... enqueueSplatKernel, return its length (blocking)
    // (defaults: the library's own, csrc/flx_adaptive.h)
    struct AdaptiveParams {
        float threshold = FLX_AD_DEFAULT_THRESHOLD; uint32_t minSamples = FLX_AD_DEFAULT_MIN_SAMPLES, maxSamples = FLX_AD_DEFAULT_MAX_SAMPLES;
        float lumFloor = FLX_AD_DEFAULT_LUM_FLOOR; bool dilate = FLX_AD_DEFAULT_DILATE != 0u;
    };
    uint32_t adaptiveUpdate(const AdaptiveParams &params);
    void adaptiveClear();
    // temporal reprojection (flx_gbuffer / flx_history_capture / flx_reproject): the primary-visibility G-buffer of the current
    // camera; the snapshot of the accumulation (and moments) with that G-buffer as the previous one; the snapshot resampled into the current
    // view over the freshly reset accumulation.  Single-GPU, asynchronous.
    struct ReprojectParams { float maxHistory = 32.0f, planeTolerancePx = 2.0f, normalCos = 0.9f, minWeight = 0.01f; };
    void gbuffer();
    void historyCapture();
    void reproject(const ReprojectParams &params);
    // history rectification (flx_history_mark / flx_history_rectify): the copy of the accumulation the next rectify compares the
    // new samples with; the share of it that they contradict taken out (no argument: the library's defaults).  Single-GPU, asynchronous.
    // markedSamples: the sum of the mark's sample counts (blocking; throws without a mark) -- what share of a history a rectify kept.
    struct RectifyParams { int radius = 3; float gamma = 3.0f, sensitivity = 2.0f, lumFloor = 0.01f; int minPixels = 8; float planeTolerancePx = 2.0f, normalCos = 0.9f; };
    void historyMark();
    void historyRectify();
    void historyRectify(const RectifyParams &params);
    double markedSamples();
    void finishQueue();
    void updatePixelIndex(uint32_t numPixels, uint32_t numNewPaths);
    void resetPixelIndex();
    uint32_t getNumTasks() const;
    void setPartition(uint32_t rank, uint32_t nranks);
    // multi-GPU from ONE process (no counterpart in the reference, one cl::CommandQueue): the contexts become ranks 0..n-1 of an RCCL
    // group with the pixel-interleaved partition; gatherLocal collects the accumulation tiles on `root` (flx_group_init_local / flx_gather_local)
    static void groupInitLocal(const std::vector<HipContext *> &ranks);
    static void gatherLocal(const std::vector<HipContext *> &ranks, uint32_t root, std::vector<float> &rgba);
    uint32_t localPixels() const;

    // image export: raw accumulation (.pfm, float RGB = sum/count) or tonemapped preview (.ppm)
    // (reference: CLContext::saveImage via DevIL, src/clcontext.cpp:386-465)
    void saveImage(const std::string &filename, const RenderParams &params);
    void readPixels(int which, std::vector<float> &rgba);

    void updateRenderPerf(float deltaT);                          // src/clcontext.cpp:648-656
    const PerfNumbers getRenderPerf() const { return renderPerf; }
    const RenderStats getStats() const { return statsAsync; }
    void resetStats() { statsAsync = RenderStats(); }
    RenderStats statsAsync;                                       // Tracer adds queue lengths here (src/tracer.cpp:336-339)

    flx_ctx *raw() { return ctx; }

private:
    void check(int rc, const char *what);
    void foldMkStats();
    RenderParams lastParams {};
    uint32_t mkStats[4] = {0, 0, 0, 0};
    bool mkPending = false;
    void *dl = nullptr;
    flx_ctx *ctx = nullptr;
    PerfNumbers renderPerf;
    struct Api;
    Api *api = nullptr;
};

} // namespace fluctus
