// tracer.cpp -- see tracer.hpp.
#include "tracer.hpp"
#include "../csrc/flx_pose.h"     // the pose arithmetic and the member compaction: what the kernels and flx_objects_define run
#include <chrono>
#include <sstream>
#include <fstream>
#include <cstring>
#include <cstddef>
#include <cmath>
#include <algorithm>
#include <stdexcept>

namespace fluctus {

static flx_vec3 v3(float x, float y, float z, float w = 0.0f) { return flx_vec3{x, y, z, w}; }

Tracer::Tracer(int width, int height, int device, uint32_t numTasks)
{
    std::memset(&params, 0, sizeof(params));
    resetParams(width, height);
    initCamera();
    initPostProcessing();
    initAreaLight();
    scene.reset(new Scene());
    clctx.reset(new HipContext(device, numTasks));
    lastRatio = std::nan(""); retainedShare = std::nan("");
}

Tracer::Tracer(int width, int height, const std::vector<int> &devices, uint32_t numTasks) : Tracer(width, height, devices.empty() ? 0 : devices[0], numTasks)
{
    for (size_t i = 1; i < devices.size(); i++) peers.emplace_back(new HipContext(devices[i], numTasks));
    if (!peers.empty()) HipContext::groupInitLocal(ranks());
}

Tracer::~Tracer() { delete bvh; }

void Tracer::readAccumulation(std::vector<float> &rgba)
{
    if (peers.empty()) { clctx->readPixels(0, rgba); return; }
    HipContext::gatherLocal(ranks(), 0, rgba);
}

// reference: src/tracer.cpp:38-52
void Tracer::resetParams(int width, int height)
{
    params.width = (uint32_t)width; params.height = (uint32_t)height;
    params.useEnvMap = 0; params.useAreaLight = 1; params.envMapStrength = 1.0f; params.maxBounces = 10;
    params.sampleImpl = 1; params.sampleExpl = 1; params.useRoulette = 0; params.wfSeparateQueues = 0;
}
// reference: src/tracer.cpp:760-776
void Tracer::initCamera()
{
    flx_camera &c = params.camera;
    c.pos = v3(0.0f, 1.0f, 3.5f); c.right = v3(1.0f, 0.0f, 0.0f); c.up = v3(0.0f, 1.0f, 0.0f); c.dir = v3(0.0f, 0.0f, -1.0f);
    c.fov = 60.0f; c.apertureSize = 0.0f; c.focalDist = 0.5f;
    paramsUpdatePending = true;
}
// reference: src/tracer.cpp:778-786
void Tracer::initPostProcessing() { params.exposure = 1.0f; params.tmOperator = 2; paramsUpdatePending = true; }
// reference: src/tracer.cpp:788-797
void Tracer::initAreaLight()
{
    flx_arealight &l = params.areaLight;
    l.E = v3(200.0f, 200.0f, 200.0f); l.right = v3(0.0f, 0.0f, -1.0f); l.up = v3(0.0f, 1.0f, 0.0f);
    l.N = v3(-1.0f, 0.0f, 0.0f, 0.0f); l.pos = v3(1.0f, 1.0f, 0.0f, 1.0f); l.size.x = 0.5f; l.size.y = 0.5f;
    paramsUpdatePending = true;
}

// reference: src/tracer.cpp:573-590 -- cached hierarchy if present, else SBVH (always SplitMode::SAH -> SBVH) + export
void Tracer::initHierarchy()
{
    delete bvh; bvh = new BVH();
    auto &tris = scene->getTriangles();
    params.n_tris = (uint32_t)tris.size();
    std::string cache;
    if (!hierarchyCacheDir.empty()) {
        cache = hierarchyCacheDir + "/hierarchy_" + sceneHash + ".bin";
        if (bvh->importFrom(cache)) return;
    }
    bvh->build(&tris, BVH::Mode::SBVH);
    if (!cache.empty()) bvh->exportTo(cache);
}

// reference: src/tracer.cpp:55-80
void Tracer::init(int width, int height, const std::string &sceneFile)
{
    job.discard();                                           // a rebuild in flight belongs to the scene that goes away (joins the worker)
    movedSinceSnapshot = false; haveBaseline = false; lastRatio = std::nan("");
    nObjects = 0; objMemberTri.clear(); objMemberObj.clear(); objRest.clear();     // (the ranks drop theirs with the upload below)
    resetParams(width, height);
    scene.reset(new Scene());
    sceneName = sceneFile;
    if (sceneFile.compare(0, 5, "proc:") == 0) {
        std::string kind; uint32_t tris = 100000, seed = 42;
        std::istringstream ss(sceneFile.substr(5)); std::string tok;
        if (std::getline(ss, tok, ':')) kind = tok;
        if (std::getline(ss, tok, ':')) tris = (uint32_t)std::stoul(tok);
        if (std::getline(ss, tok, ':')) seed = (uint32_t)std::stoul(tok);
        scene->generate(kind, tris, seed);
        sceneHash = std::to_string(xxh64(scene->getTriangles().data(), scene->getTriangles().size() * sizeof(flx_triangle)));   // no file to hash
    } else {
        scene->loadModel(sceneFile);
        sceneHash = std::to_string(fileHash(sceneFile));                 // Scene::hashString (src/scene.cpp:46-51, 95)
    }
    initHierarchy();
    params.worldRadius = bvh->worldRadius();                 // :66-67
    for (auto *c : ranks()) c->uploadSceneData(bvh, scene.get());    // replicated: read-only, 288 GB per GPU
    if (rebuildMode != RebuildOff) { baselineCost = wideCost(); haveBaseline = true; }
    // (the reference deletes the hierarchy here, :72-73; it stays for updateGeometry's refit: 48 bytes per node and the index list)
    paramsUpdatePending = true;
    iteration = 0;
    history.dropped();                                       // a new scene: no history
}

// The scene's triangles move (an animated mesh, a dragged object): same count, same materials.  The host tree and both device trees are refitted
// over their topology instead of rebuilt; quality decays under strong deformation -- init() again rebuilds, or a rebuild policy
// does when the trees' cost says so.
void Tracer::refitAll(const std::vector<flx_triangle> &tris)
{
    for (auto *c : ranks()) c->updateTriangles(tris);         // refused (non-finite / out-of-range input): throws, and everything is still the old geometry's
    bvh->refit(tris);
    scene->getTriangles() = tris;
}
void Tracer::geometryChanged()
{
    params.worldRadius = bvh->worldRadius();
    paramsUpdatePending = true;
    history.dropped();                                       // the G-buffer and the accumulation belong to the old geometry
    iteration = 0;
}
// What every move of triangles runs, in this order (reprojection across it: DESIGN.md 4.3.4, 4.3.6; history_state.hpp).  keepSwitch: the switch
// under which this kind of move keeps the history.  moveRanks: the device call on every rank; refused (bad input), it throws and everything is
// still the old geometry's.  moveHost: the host tree and the scene's copy follow.
template <class MoveRanks, class MoveHost> void Tracer::moveTriangles(bool keepSwitch, MoveRanks moveRanks, MoveHost moveHost)
{
    if (rebuildMode != RebuildOff) adoptFinishedRebuild();
    const HistoryState::MovePlan plan = history.beforeMove(keepSwitch, params, useWavefront);
    if (plan.captureNow) clctx->historyCapture();            // before the ranks move, so that the device keeps the history
    try {
        moveRanks();
    } catch (...) {
        if (plan.captureNow) paramsUpdatePending = true;     // the capture has handed the current slot over: the next update() traces it again and reprojects (nothing moved)
        throw;
    }
    moveHost();
    const uint32_t topologies = rebuilds;
    afterMove();                                             // (its geometryChanged drops the host's view of the history ...)
    history.afterMove(plan.keep, rebuilds != topologies);    // (... which the device still has, unless a rebuild in there uploaded a topology)
}
void Tracer::updateGeometry(const std::vector<flx_triangle> &tris)
{
    if (!scene || !bvh) throw std::runtime_error("Tracer::updateGeometry: no scene (init first)");
    if (tris.size() != scene->getTriangles().size()) throw std::runtime_error("Tracer::updateGeometry: the triangle count differs from the scene's");
    moveTriangles(history.deform(), [&] { refitAll(tris); }, [] {});          // (refitAll moves the host copy behind the ranks)
}
// ... a subset of them (flx_update_triangles_subset, BVH::refitSubset): only the boxes above the listed triangles are refitted.
// Takes part in the rebuild policy exactly as the full overload does.
void Tracer::updateGeometry(const std::vector<uint32_t> &indices, const std::vector<flx_triangle> &tris)
{
    if (!scene || !bvh) throw std::runtime_error("Tracer::updateGeometry: no scene (init first)");
    if (indices.size() != tris.size()) throw std::runtime_error("Tracer::updateGeometry: as many triangles as indices");
    moveTriangles(history.deform(),
                  [&] { for (auto *c : ranks()) c->updateTriangles(indices, tris); },
                  [&] {
                      std::vector<flx_triangle> all = scene->getTriangles();
                      for (size_t k = 0; k < indices.size(); k++) all[indices[k]] = tris[k];      // (the device has checked the list: ascending, in range)
                      bvh->refitSubset(all, indices);
                      scene->getTriangles().swap(all);
                  });
}
// Objects moved by their transforms: updateGeometry(indices, tris) with the triangles made where they are needed -- on every rank
// by flx_objects_pose, here by the same csrc/flx_pose.h function for the host tree and the scene's copy.
void Tracer::defineObjects(const std::vector<uint32_t> &objectOfTriangle, uint32_t nobjects)
{
    if (!scene || !bvh) throw std::runtime_error("Tracer::defineObjects: no scene (init first)");
    const std::vector<flx_triangle> &tris = scene->getTriangles();
    std::vector<uint32_t> counts(nobjects), tri, obj;
    std::vector<flx_triangle> rest;
    if (nobjects) {
        if (objectOfTriangle.size() != tris.size()) throw std::runtime_error("Tracer::defineObjects: one object id per triangle of the scene");
        size_t bad = 0;
        const size_t members = flx::ps_count_members(objectOfTriangle.data(), tris.size(), nobjects, counts.data(), &bad);
        if (members == (size_t)-1) throw std::runtime_error("Tracer::defineObjects: triangle " + std::to_string(bad) + " has an object id that is neither below the object count nor FLX_NO_OBJECT");
        tri.resize(members); obj.resize(members); rest.resize(members);
        flx::ps_compact_members(tris.data(), objectOfTriangle.data(), tris.size(), tri.data(), obj.data(), rest.data());
    }
    for (auto *c : ranks()) c->defineObjects(nobjects ? tris : std::vector<flx_triangle>(), nobjects ? objectOfTriangle : std::vector<uint32_t>(), nobjects);
    nObjects = nobjects; objMemberTri.swap(tri); objMemberObj.swap(obj); objRest.swap(rest);
    history.objectsDefined();
}
void Tracer::defineObjects()
{
    if (!scene) throw std::runtime_error("Tracer::defineObjects: no scene (init first)");
    defineObjects(scene->objectOfTriangle(), (uint32_t)scene->objectNames().size());
}
void Tracer::defineObjectsOnRanks(const std::vector<flx_triangle> &tris)
{
    if (!nObjects) return;
    std::vector<flx_triangle> rest = tris;
    std::vector<uint32_t> objectOf(tris.size(), FLX_NO_OBJECT);
    for (size_t k = 0; k < objMemberTri.size(); k++) { rest[objMemberTri[k]] = objRest[k]; objectOf[objMemberTri[k]] = objMemberObj[k]; }
    for (auto *c : ranks()) c->defineObjects(rest, objectOf, nObjects);
}
void Tracer::poseObjects(const std::vector<uint32_t> &ids, const std::vector<float> &xforms12)
{
    if (!scene || !bvh) throw std::runtime_error("Tracer::poseObjects: no scene (init first)");
    if (!nObjects) throw std::runtime_error("Tracer::poseObjects: no objects are defined (defineObjects)");
    moveTriangles(history.motion() || history.deform(),      // (under per-vertex reprojection a pose is a move of triangles like any other)
                  [&] { for (auto *c : ranks()) c->poseObjects(ids, xforms12); },       // refused: a bad list or matrix, a vertex out of range
                  [&] {
                      std::vector<uint32_t> slot(nObjects, FLX_NO_OBJECT);               // (the device has checked the list: ascending, in range)
                      for (size_t k = 0; k < ids.size(); k++) slot[ids[k]] = (uint32_t)k;
                      std::vector<flx_triangle> all = scene->getTriangles();
                      std::vector<uint32_t> indices;
                      for (size_t k = 0; k < objMemberTri.size(); k++) {
                          const uint32_t s = slot[objMemberObj[k]];
                          if (s == FLX_NO_OBJECT) continue;
                          flx::ps_pose_triangles(xforms12.data() + 12 * (size_t)s, &objRest[k], &all[objMemberTri[k]], 1);
                          indices.push_back(objMemberTri[k]);
                      }
                      bvh->refitSubset(all, indices);
                      scene->getTriangles().swap(all);
                  });
}
// what follows every move of the triangles: the resets of geometryChanged, then the rebuild policy on the trees as they stand now
void Tracer::afterMove()
{
    geometryChanged();
    if (job.active()) movedSinceSnapshot = true;             // (under Off too: a job started before the policy was switched off -- whoever adopts it later must refit)
    if (rebuildMode == RebuildOff) return;
    if (!haveBaseline) { lastRatio = std::nan(""); return; }
    lastRatio = wideCost() / baselineCost;
    if (!(lastRatio > rebuildThreshold) || job.active()) return;     // (a NaN ratio: no decision)
    const std::vector<flx_triangle> tris = scene->getTriangles();
    if (rebuildMode == RebuildBackground) { job.start(tris, BVH::Mode::SBVH); movedSinceSnapshot = false; return; }
    std::unique_ptr<BVH> fresh(new BVH());
    fresh->build(&tris, BVH::Mode::SBVH);
    uploadTopology(fresh.get(), tris);                       // the pose is the tree's: no refit behind it
    delete bvh; bvh = fresh.release();
    geometryChanged();
    lastRatio = 1.0;
}

void Tracer::setRebuildPolicy(RebuildMode mode, double threshold)
{
    if (mode != RebuildOff && mode != RebuildBlocking && mode != RebuildBackground) throw std::runtime_error("setRebuildPolicy: unknown mode");
    if (mode != RebuildOff && (!(threshold > 1.0) || !std::isfinite(threshold))) throw std::runtime_error("setRebuildPolicy: the threshold must be finite and > 1");
    rebuildMode = mode; rebuildThreshold = threshold;
    if (mode != RebuildOff && !haveBaseline && bvh) { baselineCost = wideCost(); haveBaseline = true; }
}
double Tracer::wideCost()
{
    const std::array<double, 8> s = clctx->treeCost();
    return flxTreeCostValue(s.data() + 4);
}
void Tracer::treeRead(uint32_t rank, int which, std::vector<uint8_t> &out)
{
    auto R = ranks();
    if (rank >= R.size()) throw std::runtime_error("treeRead: no such rank");
    R[rank]->treeRead(which, out);
}
int Tracer::getOption(uint32_t rank, const std::string &name)
{
    auto R = ranks();
    if (rank >= R.size()) throw std::runtime_error("getOption: no such rank");
    return R[rank]->getOption(name);
}
void Tracer::uploadTopology(BVH *tree, const std::vector<flx_triangle> &tris)
{
    for (auto *c : ranks()) {
        // flx_upload_scene re-derives "fuse_set" / "ext_order" from the triangles it is given; the first upload's choice (or the caller's override) stays
        const int fuseSet = c->getOption("fuse_set"), extOrder = c->getOption("ext_order");
        c->uploadSceneData(tree, scene.get(), tris);
        c->setOption("fuse_set", fuseSet); c->setOption("ext_order", extOrder);
    }
    defineObjectsOnRanks(tris);                              // the upload has dropped the ranks' objects; the rest pose survives a rebuild
    baselineCost = wideCost(); haveBaseline = true;          // before any refit: the ratio never hides the drift since the snapshot
    rebuilds++;
}
bool Tracer::adoptFinishedRebuild()
{
    if (!job.ready()) return false;
    std::unique_ptr<BVH> fresh; std::vector<flx_triangle> snapshot;
    const bool moved = movedSinceSnapshot;
    movedSinceSnapshot = false;
    job.take(fresh, snapshot);                               // (rethrows a failed build; the old trees stay)
    uploadTopology(fresh.get(), snapshot);
    delete bvh; bvh = fresh.release();
    if (moved) {
        const std::vector<flx_triangle> current = scene->getTriangles();
        refitAll(current);
    }
    geometryChanged();
    return true;
}

void Tracer::setEnvMap(const std::string &hdrFile)
{
    envMap.reset(new EnvironmentMap(hdrFile));
    for (auto *c : ranks()) c->createEnvMap(envMap.get());
    params.useEnvMap = 1;
    paramsUpdatePending = true;
    history.dropped();                                       // another light: the accumulated radiance is stale
}

// reference: src/tracer.cpp:625-684 (iterateStateItems): one item after the other in native byte order
namespace {
struct StateIO {
    std::fstream f; bool write;
    template <class T> void rw(T &v) { if (write) f.write((const char *)&v, sizeof(T)); else f.read((char *)&v, sizeof(T)); }
    void vec(flx_vec3 &v) { rw(v.x); rw(v.y); rw(v.z); }
};
}
static bool stateItems(const std::string &path, bool write, RenderParams &p, float *cameraRotation, float &cameraSpeed)
{
    StateIO io; io.write = write;
    io.f.open(path, std::ios::binary | (write ? std::ios::out : std::ios::in));
    if (!io.f.good()) return false;
    io.rw(cameraRotation[0]); io.rw(cameraRotation[1]); io.rw(cameraSpeed);
    io.rw(p.camera.fov); io.rw(p.camera.focalDist); io.rw(p.camera.apertureSize);
    io.vec(p.camera.dir); io.vec(p.camera.pos); io.vec(p.camera.right); io.vec(p.camera.up);
    io.vec(p.areaLight.N); io.vec(p.areaLight.pos); io.vec(p.areaLight.right); io.vec(p.areaLight.up); io.vec(p.areaLight.E);
    io.rw(p.areaLight.size.x); io.rw(p.areaLight.size.y); io.rw(p.envMapStrength);
    io.rw(p.maxBounces); io.rw(p.useAreaLight); io.rw(p.useEnvMap); io.rw(p.sampleExpl); io.rw(p.sampleImpl); io.rw(p.useRoulette);
    io.rw(p.exposure); io.rw(p.tmOperator);
    return io.f.good();
}
bool Tracer::saveState() const
{
    if (stateDir.empty()) return false;
    RenderParams p = params; float rot[2] = {cameraRotation[0], cameraRotation[1]}; float speed = cameraSpeed;
    return stateItems(stateDir + "/state_" + sceneHash + ".dat", true, p, rot, speed);
}
bool Tracer::loadState()
{
    if (stateDir.empty()) return false;
    RenderParams p = params; float rot[2] = {0.0f, 0.0f}; float speed = 1.0f;
    if (!stateItems(stateDir + "/state_" + sceneHash + ".dat", false, p, rot, speed)) return false;
    params = p; cameraRotation[0] = rot[0]; cameraRotation[1] = rot[1]; cameraSpeed = speed;
    paramsUpdatePending = true;
    return true;
}

void Tracer::setDenoiserStrength(float s)
{
    if (s > 0.0f && !peers.empty()) throw std::runtime_error("setDenoiserStrength: the denoiser is single-GPU (a pixel's neighbours are on other ranks)");
    denoiserStrength = s;
}
// what the four reprojection switches refuse alike, under the setter's own name
void Tracer::refuseSwitch(const char *setter, bool on, bool needsTemporal) const
{
    const std::string name(setter);
    if (on && !peers.empty()) throw std::runtime_error(name + ": temporal reprojection is single-GPU (a pixel's neighbours are on other ranks)");
    if (on && needsTemporal && !history.temporal()) throw std::runtime_error(name + ": needs setTemporalReprojection(true)");
}
void Tracer::setTemporalReprojection(bool on)
{
    refuseSwitch("setTemporalReprojection", on, false);
    history.temporalSet(on);
    if (!on && history.motion()) setMotionReprojection(false);
    if (!on && history.deform()) setDeformReprojection(false);
    if (!on && history.rectify()) setHistoryRectification(false);
}
void Tracer::setHistoryRectification(bool on)
{
    refuseSwitch("setHistoryRectification", on);
    history.rectifySet(on);
}
void Tracer::setRectifyDelay(int frames)
{
    if (frames < 0) throw std::runtime_error("setRectifyDelay: the delay is a number of frames >= 1 (0: the default, 2 maxBounces + 2)");
    history.rectifyDelaySet((uint32_t)frames);
}
void Tracer::setMotionReprojection(bool on)
{
    refuseSwitch("setMotionReprojection", on);
    if (on && history.deform()) throw std::runtime_error("setMotionReprojection: per-vertex reprojection is on, which follows poseObjects too; setDeformReprojection(false) first");
    for (auto *c : ranks()) c->setOption("motion_history", on ? 1 : 0);
    history.motionSet(on);
}
void Tracer::setDeformReprojection(bool on)
{
    refuseSwitch("setDeformReprojection", on);
    if (on && history.motion()) throw std::runtime_error("setDeformReprojection: motion-aware reprojection is on; setMotionReprojection(false) first (this switch follows poseObjects too)");
    for (auto *c : ranks()) c->setOption("deform_history", on ? 1 : 0);
    history.deformSet(on);
}
void Tracer::toggleRenderer()
{
    if (!useWavefront && meshLightsOn && !meshLightsWavefrontOn)
        throw std::runtime_error("toggleRenderer: mesh lights are on and the wavefront integrator does not see emissive triangles -- the scene's lamps would go dark; setMeshLights(false) first");
    useWavefront = !useWavefront; iteration = 0; history.dropped();
}
void Tracer::setMeshLights(bool on)
{
    if (on && !peers.empty()) throw std::runtime_error("setMeshLights: emissive triangles light the microkernel integrator, which is single-GPU");
    if (on && useWavefront) toggleRenderer();                            // as renderSingle does
    clctx->setOption("mesh_lights", on ? 1 : 0);
    meshLightsOn = on;
    if (!on && meshLightsWavefrontOn) { clctx->setOption("mesh_lights_wavefront", 0); meshLightsWavefrontOn = false; }
    iteration = 0; history.dropped();                                    // the accumulation was lit differently
}
// ... and the wavefront integrator: the logic pass's MESH instance samples and collects the lamps, so the wavefront loop is
// allowed again.  The integrator in use stays the one it is: toggleRenderer() switches.
void Tracer::setMeshLightsWavefront(bool on)
{
    if (on && !peers.empty()) throw std::runtime_error("setMeshLightsWavefront: emissive triangles as lights are single-GPU");
    if (on && !meshLightsOn) throw std::runtime_error("setMeshLightsWavefront: needs setMeshLights(true) first");
    if (on == meshLightsWavefrontOn) return;                             // nothing changes: the accumulation stays
    if (!on && meshLightsOn && useWavefront) toggleRenderer();           // back to the integrator that sees the lamps, as setMeshLights(true) does
    clctx->setOption("mesh_lights_wavefront", on ? 1 : 0);
    meshLightsWavefrontOn = on;
    iteration = 0; history.dropped();
}
void Tracer::setMaxHistory(float n)
{
    if (!(n >= 1.0f) || !std::isfinite(n)) throw std::runtime_error("setMaxHistory: must be finite and >= 1");
    maxHistory = n;
}
// DenoiserOptix::setBlend(1 - strength) + denoise (src/tracer.cpp:310-328): behind the post-process, on the stream
void Tracer::denoiseStep()
{
    if (denoiserMode == VarianceGuided) {
        HipContext::DenoiseVgParams dp;
        dp.blend = 1.0f - denoiserStrength;
        clctx->denoiseVarianceGuided(dp);
        return;
    }
    HipContext::DenoiseParams dp;
    dp.blend = 1.0f - denoiserStrength;
    clctx->denoise(dp);
}
void Tracer::applyMoments()
{
    const bool on = useDenoiser && denoiserMode == VarianceGuided;
    if (on == momentsOn) return;
    for (auto *c : ranks()) c->setOption("moments", on ? 1 : 0);
    momentsOn = on;
}
void Tracer::setDenoiserMode(DenoiserMode m)
{
    if (m != Guided && m != VarianceGuided) throw std::runtime_error("setDenoiserMode: unknown mode");
    if (m == denoiserMode) return;
    denoiserMode = m;
    const bool was = momentsOn;
    applyMoments();
    if (momentsOn != was) iteration = 0;                                 // restart the accumulation with its moments
}

// reference: src/tracer.cpp:95-187
void Tracer::renderSingle(int spp, bool denoise)
{
    if (!peers.empty()) throw std::runtime_error("renderSingle: the microkernel integrator is single-GPU");
    if (useWavefront) toggleRenderer();                                  // only MK guarantees the spp of every pixel (:99-101)
    if ((uint64_t)params.width * params.height > clctx->getNumTasks())
        throw std::runtime_error("renderSingle: width*height exceeds the context's numTasks (one path per pixel)");
    params.useRoulette = 0;                                              // :104-108
    if (denoise) setDenoiser(true);                                      // :110-114
    clctx->updateParams(params); paramsUpdatePending = false;
    history.dropped();                                                   // parameters reach the device without a G-buffer
    clctx->enqueueResetKernel(params);
    for (int sample = 0; sample < spp; sample++) {
        clctx->enqueueRayGenKernel(params);
        for (uint32_t bounce = 0; bounce < params.maxBounces + 1; bounce++) {
            clctx->enqueueNextVertexKernel(params);
            clctx->enqueueBsdfSampleKernel(params);
        }
        clctx->enqueueSplatKernel(params);
        clctx->enqueuePostprocessKernel(params);
        clctx->fetchStatsAsync();
        clctx->finishQueue();
        iteration++;
    }
    if (denoise && denoiserStrength > 0.0f) { denoiseStep(); clctx->finishQueue(); }   // :160-165 (output_<spp>_denoised)
}

// renderSingle to a noise threshold (no counterpart in the reference): minSpp uniform passes, then every pass runs over the
// pixels flx_mk_adaptive_update still lists, until none is left or maxSpp passes ran.  Returns the samples taken.
uint64_t Tracer::renderAdaptive(int minSpp, int maxSpp, float threshold, bool denoise)
{
    if (!peers.empty()) throw std::runtime_error("renderAdaptive: the microkernel integrator is single-GPU");
    if (minSpp < 1 || maxSpp < minSpp || maxSpp > (1 << 24)) throw std::runtime_error("renderAdaptive: needs 1 <= minSpp <= maxSpp <= 2^24");
    if (!(threshold >= 0.0f) || std::isinf(threshold)) throw std::runtime_error("renderAdaptive: the threshold must be finite and >= 0");
    if (useWavefront) toggleRenderer();
    if ((uint64_t)params.width * params.height > clctx->getNumTasks())
        throw std::runtime_error("renderAdaptive: width*height exceeds the context's numTasks (one path per pixel)");
    params.useRoulette = 0;
    if (denoise) setDenoiser(true);
    const bool hadMoments = momentsOn;
    // whatever happens below, the context is left without a list of active pixels and with "moments" as it was
    auto restore = [&] { clctx->adaptiveClear(); if (!hadMoments) clctx->setOption("moments", 0); };
    uint64_t total = 0;
    try {
    if (!hadMoments) clctx->setOption("moments", 1);                     // for this render only
    clctx->updateParams(params); paramsUpdatePending = false;
    history.dropped();
    clctx->enqueueResetKernel(params);                                   // (also clears a list of active pixels)
    HipContext::AdaptiveParams ap;
    ap.threshold = threshold; ap.minSamples = (uint32_t)minSpp; ap.maxSamples = (uint32_t)maxSpp;
    uint64_t active = (uint64_t)params.width * params.height;
    for (int sample = 0; sample < maxSpp && active > 0; sample++) {
        if (sample >= minSpp && (active = clctx->adaptiveUpdate(ap)) == 0) break;
        clctx->enqueueRayGenKernel(params);
        for (uint32_t bounce = 0; bounce < params.maxBounces + 1; bounce++) {
            clctx->enqueueNextVertexKernel(params);
            clctx->enqueueBsdfSampleKernel(params);
        }
        clctx->enqueueSplatKernel(params);
        clctx->enqueuePostprocessKernel(params);
        clctx->fetchStatsAsync();
        clctx->finishQueue();
        total += active;
        iteration++;
    }
    clctx->adaptiveClear();
    if (denoise && denoiserStrength > 0.0f) { denoiseStep(); clctx->finishQueue(); }
    } catch (...) {
        try { restore(); } catch (...) {}                                // (the first error is the one to report)
        throw;
    }
    restore();
    return total;
}

// reference: src/tracer.cpp:268-299, microkernel branch of update()
void Tracer::updateMicrokernel()
{
    if (iteration == 0) {                                                // interactive preview: two segments, splat incomplete paths
        clctx->enqueueResetKernel(params);
        clctx->enqueueRayGenKernel(params);
        clctx->enqueueNextVertexKernel(params);
        clctx->enqueueBsdfSampleKernel(params);
        clctx->enqueueNextVertexKernel(params);
        clctx->enqueueBsdfSampleKernel(params);
        clctx->enqueueSplatPreviewKernel(params);
    } else {                                                             // one state-machine step of every path per frame
        clctx->enqueueRayGenKernel(params);
        clctx->enqueueNextVertexKernel(params);
        clctx->enqueueBsdfSampleKernel(params);
        clctx->enqueueSplatKernel(params);
    }
    clctx->enqueuePostprocessKernel(params);
    if (useDenoiser && denoiserStrength > 0.0f && iteration >= 10 && iteration % 10 == 0) denoiseStep();   // :310-328
    clctx->fetchStatsAsync();                                            // :343-344
    clctx->finishQueue();
    iteration++;
}

// reference: src/tracer.cpp:189-358.  With several ranks every enqueue* call fans out over the devices (all asynchronous: one host
// thread keeps them busy); each rank has its own counters and pixel cursor.
void Tracer::update()
{
    if (rebuildMode != RebuildOff) adoptFinishedRebuild();
    auto R = ranks();
    bool reprojectNow = false;
    if (paramsUpdatePending) {
        const HistoryState::ParamsPlan plan = history.paramsReachDevice(params, useWavefront);
        if (plan.captureNow) clctx->historyCapture();                    // under the old camera's slot: before the parameters reach the device
        for (auto *c : R) c->updateParams(params);
        paramsUpdatePending = false; iteration = 0;
        if (plan.traceGbuffer) clctx->gbuffer();
        reprojectNow = plan.reprojectNow;
    }
    const bool markNow = history.frameStarts(iteration, reprojectNow, useWavefront);
    if (!useWavefront) {
        if (!peers.empty()) throw std::runtime_error("update: the microkernel integrator is single-GPU");
        updateMicrokernel(); return;
    }
    std::vector<QueueCounters> cnt(R.size());
    std::memset(cnt.data(), 0, cnt.size() * sizeof(QueueCounters));
    uint32_t maxBounces = params.maxBounces;
    int N = 1;
    if (iteration == 0) {
        params.maxBounces = std::min((uint32_t)2, maxBounces);           // 2-bounce preview
        N = 3;
        for (auto *c : R) {
            c->updateParams(params);
            c->resetPixelIndex();
            c->enqueueWfResetKernel(params);
            if (reprojectNow) { HipContext::ReprojectParams rp; rp.maxHistory = maxHistory; c->reproject(rp); }      // (single rank: setTemporalReprojection)
            c->enqueueWfRaygenKernel(params);
            c->enqueueWfExtRayKernel(params);
            c->enqueueClearWfQueues();
        }
    }
    for (int i = 0; i < N; i++) {
        for (size_t r = 0; r < R.size(); r++) {
            HipContext *c = R[r];
            c->enqueueWfLogicKernel(params, iteration == 0);
            c->enqueueWfRaygenKernel(params);
            c->enqueueWfMaterialKernels(params);
            c->enqueueGetCounters(&cnt[r]);
            c->enqueueWfExtRayKernel(params);
            c->enqueueWfShadowRayKernel(params);
            c->enqueueClearWfQueues();
        }
    }
    if (iteration == 0) { params.maxBounces = maxBounces; for (auto *c : R) c->updateParams(params); }
    // history rectification: the frame that reprojected marks what it has (history + preview); the frame that completes the delay compares
    if (markNow) { clctx->historyMark(); history.marked(); }
    else if (history.rectifyDue(params.maxBounces)) {
        const double before = measureRetained ? clctx->markedSamples() : 0.0;
        clctx->historyRectify();
        if (measureRetained) retainedShare = before > 0.0 ? clctx->markedSamples() / before : std::nan("");
        history.rectified(); rectifies++;
    }
    for (auto *c : R) c->enqueuePostprocessKernel(params);
    const uint32_t sched = history.denoiserSchedule(iteration);          // temporal reprojection: frames since the last discarded history
    if (useDenoiser && denoiserStrength > 0.0f && sched >= 10 && sched % 10 == 0) denoiseStep();   // :310-328 (single-GPU: setDenoiserStrength)
    for (auto *c : R) c->finishQueue();
    QueueCounters sum; std::memset(&sum, 0, sizeof(sum));
    for (size_t r = 0; r < R.size(); r++) {
        R[r]->updatePixelIndex(R[r]->localPixels(), cnt[r].raygenQueue);
        sum.raygenQueue += cnt[r].raygenQueue; sum.extensionQueue += cnt[r].extensionQueue; sum.shadowQueue += cnt[r].shadowQueue;
        sum.diffuseQueue += cnt[r].diffuseQueue; sum.glossyQueue += cnt[r].glossyQueue; sum.ggxReflQueue += cnt[r].ggxReflQueue;
        sum.ggxRefrQueue += cnt[r].ggxRefrQueue; sum.deltaQueue += cnt[r].deltaQueue;
    }
    clctx->statsAsync.extensionRays += sum.extensionQueue;               // :336-339
    clctx->statsAsync.shadowRays += sum.shadowQueue;
    clctx->statsAsync.primaryRays += sum.raygenQueue;
    clctx->statsAsync.samples += (iteration > 0) ? sum.raygenQueue : 0;
    lastCnt = sum;
    iteration++; history.frameRendered();
}

// reference: src/tracer.cpp:362-528, wavefront body
std::string Tracer::runBenchmark(double seconds, int iterations)
{
    using clk = std::chrono::steady_clock;
    auto now = [] { return std::chrono::duration<double>(clk::now().time_since_epoch()).count(); };
    std::ostringstream csv;
    csv << "scene;time;primary;extension;shadow;total;samples\n";
    auto R = ranks();
    if (!useWavefront && !peers.empty()) throw std::runtime_error("runBenchmark: the microkernel integrator is single-GPU");
    // resetRenderer (:372-382)
    iteration = 0;
    paramsUpdatePending = false;
    history.dropped();
    for (auto *c : R) {
        c->updateParams(params);
        c->resetPixelIndex();
        c->enqueueWfResetKernel(params);
        c->enqueueClearWfQueues();
        if (peers.empty()) { c->enqueueResetKernel(params); c->fetchStatsAsync(); }   // :377; drains + zeroes the device-side MK counters
        c->finishQueue();
        c->resetStats();
    }
    double startT = now(), lastLog = startT, currT = startT;
    int it = 0;
    auto log = [&](double t) {
        RenderStats s = clctx->getStats(); clctx->resetStats();
        double dt = t - lastLog, sc = 1e6 * dt; lastLog = t;
        csv << sceneName << ";" << (t - startT) << ";" << s.primaryRays / sc << ";" << s.extensionRays / sc << ";" << s.shadowRays / sc << ";"
            << (s.primaryRays + s.extensionRays + s.shadowRays) / sc << ";" << s.samples / sc << "\n";
    };
    std::vector<QueueCounters> cnt(R.size());
    while (iterations > 0 ? it < iterations : currT - startT < seconds) {
        std::memset(cnt.data(), 0, cnt.size() * sizeof(QueueCounters));
        for (size_t r = 0; r < R.size(); r++) {
            HipContext *c = R[r];
            if (useWavefront) {
                c->enqueueWfLogicKernel(params, false);
                c->enqueueWfRaygenKernel(params);
                c->enqueueWfMaterialKernels(params);
                c->enqueueGetCounters(&cnt[r]);
                c->enqueueWfExtRayKernel(params);
                c->enqueueWfShadowRayKernel(params);
                c->enqueueClearWfQueues();
            } else {                                                     // :441-447
                c->enqueueRayGenKernel(params);
                c->enqueueNextVertexKernel(params);
                c->enqueueBsdfSampleKernel(params);
                c->enqueueSplatKernel(params);
                c->fetchStatsAsync();
            }
            c->enqueuePostprocessKernel(params);
        }
        for (auto *c : R) c->finishQueue();
        QueueCounters sum; std::memset(&sum, 0, sizeof(sum));
        for (size_t r = 0; r < R.size(); r++) {
            if (useWavefront) {
                clctx->statsAsync.extensionRays += cnt[r].extensionQueue;
                clctx->statsAsync.shadowRays += cnt[r].shadowQueue;
                clctx->statsAsync.primaryRays += cnt[r].raygenQueue;
                clctx->statsAsync.samples += (iteration > 0) ? cnt[r].raygenQueue : 0;
            }
            R[r]->updatePixelIndex(R[r]->localPixels(), cnt[r].raygenQueue);
            sum.raygenQueue += cnt[r].raygenQueue; sum.extensionQueue += cnt[r].extensionQueue; sum.shadowQueue += cnt[r].shadowQueue;
            sum.diffuseQueue += cnt[r].diffuseQueue; sum.glossyQueue += cnt[r].glossyQueue; sum.ggxReflQueue += cnt[r].ggxReflQueue;
            sum.ggxRefrQueue += cnt[r].ggxRefrQueue; sum.deltaQueue += cnt[r].deltaQueue;
        }
        lastCnt = sum;
        iteration++; it++;
        currT = now();
        if (currT - lastLog > 0.5) log(currT);
    }
    log(now());
    return csv.str();
}

} // namespace fluctus
