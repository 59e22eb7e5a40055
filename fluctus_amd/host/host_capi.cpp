// host_capi.cpp -- C entry points of libfluctus_host.so (scene / BVH / env-map preparation).
// Pure CPU, no device code.  Consumed by the Python harness (tests, bench.py) through ctypes and
// by the C++ Tracer.  Every function returns 0 on success, non-zero on error (message via
// fh_last_error()), never throws across the boundary.
#include "scene.hpp"
#include "bvh.hpp"
#include "envmap.hpp"
#include "texture.hpp"
#include "rebuild_job.hpp"
#include "../../include/fluctus_hip.h"   // flxTreeCostValue
#include <memory>
#include <array>
#include "../csrc/flx_refit.h"     // the refit's fp64 quantiser compiles for the host too: the CPU tests run what the kernels run
#include "../csrc/flx_tree_cost.h" // the cost sums of flx_tree_cost, likewise
#include "../csrc/flx_pose.h"      // the pose arithmetic of flx_objects_pose, likewise
#include "../csrc/flx_mesh_light.h" // the table of emissive triangles (option "mesh_lights"), likewise
#include "../csrc/flx_wide.h"      // the 4-wide tree builder is plain host C++ (flx_upload_scene runs it); exposed here for CPU-side tests
#include <cstring>
#include <string>
#include <exception>
#include <stdexcept>

using namespace fluctus;

static thread_local std::string g_err;
#define FH_TRY try {
#define FH_CATCH } catch (const std::exception &e) { g_err = e.what(); return 1; } catch (...) { g_err = "unknown error"; return 1; } return 0;

extern "C" {

const char *fh_last_error() { return g_err.c_str(); }

// ---- Scene
int fh_scene_create(void **out) { FH_TRY *out = new Scene(); FH_CATCH }
int fh_scene_destroy(void *s) { delete (Scene *)s; return 0; }
int fh_scene_load(void *s, const char *path) { FH_TRY ((Scene *)s)->loadModel(path); FH_CATCH }
int fh_scene_world_up(void *s, float *out3) { flx_vec3 u = ((Scene *)s)->getWorldUp(); out3[0] = u.x; out3[1] = u.y; out3[2] = u.z; return 0; }
int fh_scene_generate(void *s, const char *kind, uint32_t targetTris, uint32_t seed) { FH_TRY ((Scene *)s)->generate(kind, targetTris, seed); FH_CATCH }
int fh_scene_counts(void *s, uint64_t *ntris, uint64_t *nmats, uint64_t *ntex, uint64_t *texbytes, uint32_t *typeBits)
{
    FH_TRY
    Scene *sc = (Scene *)s;
    *ntris = sc->getTriangles().size(); *nmats = sc->getMaterials().size(); *ntex = sc->getTextures().size();
    uint64_t b = 0; for (auto &t : sc->getTextures()) b += (uint64_t)t.width * t.height * 4;
    *texbytes = b; *typeBits = sc->getMaterialTypes();
    FH_CATCH
}
int fh_scene_get(void *s, void *tris, void *mats, void *texdesc, uint8_t *texdata)
{
    FH_TRY
    Scene *sc = (Scene *)s;
    if (tris) memcpy(tris, sc->getTriangles().data(), sc->getTriangles().size() * sizeof(flx_triangle));
    if (mats) memcpy(mats, sc->getMaterials().data(), sc->getMaterials().size() * sizeof(flx_material));
    std::vector<flx_texdesc> d; std::vector<uint8_t> blob;
    sc->packTextures(d, blob);
    if (texdesc && !d.empty()) memcpy(texdesc, d.data(), d.size() * sizeof(flx_texdesc));
    if (texdata && !blob.empty()) memcpy(texdata, blob.data(), blob.size());
    FH_CATCH
}
int fh_scene_add_material(void *s, const void *mat80, int *idx) { FH_TRY *idx = ((Scene *)s)->addMaterial(*(const flx_material *)mat80); FH_CATCH }
int fh_scene_set_tri_material(void *s, uint64_t first, uint64_t count, int matId)
{
    FH_TRY
    auto &t = ((Scene *)s)->getTriangles();
    for (uint64_t i = first; i < first + count && i < t.size(); i++) t[i].matId = matId;
    FH_CATCH
}

// PNG or JPEG by file signature (the name is historical); RGBA8, lower-left origin
int fh_png_load(const char *path, uint32_t *w, uint32_t *h, uint8_t *rgba /* null: query size */)
{
    FH_TRY
    Texture t = loadTexture(path);
    *w = t.width; *h = t.height;
    if (rgba) memcpy(rgba, t.rgba.data(), t.rgba.size());
    FH_CATCH
}

// JPEG from memory: RGB8, top-left origin (libjpeg scanline order); rgb == null queries the size
int fh_jpeg_decode(const uint8_t *data, uint64_t size, uint32_t *w, uint32_t *h, uint8_t *rgb, uint64_t cap)
{
    FH_TRY
    std::vector<uint8_t> out;
    decodeJPEG(data, (size_t)size, w, h, out);
    if (rgb) { if (out.size() > cap) throw std::runtime_error("fh_jpeg_decode: buffer too small"); memcpy(rgb, out.data(), out.size()); }
    FH_CATCH
}

// ---- BVH   mode: 0 = SBVH, 1 = SAH sweep, 2 = binned
int fh_bvh_build(const void *tris, uint64_t ntris, int mode, void **out)
{
    FH_TRY
    std::vector<flx_triangle> *copy = new std::vector<flx_triangle>((const flx_triangle *)tris, (const flx_triangle *)tris + ntris);
    BVH *b = new BVH();
    try { b->build(copy, mode == 0 ? BVH::Mode::SBVH : mode == 1 ? BVH::Mode::SAH : BVH::Mode::Binned); }
    catch (...) { delete copy; delete b; throw; }
    delete copy;
    *out = b;
    FH_CATCH
}
// threads: 0 = every core this process may use (affinity capped by the cgroup CPU quota), 1 = the serial recursion; jobSize 0 = default
int fh_bvh_build_ex(const void *tris, uint64_t ntris, int mode, int threads, uint64_t jobSize, void **out)
{
    FH_TRY
    std::vector<flx_triangle> *copy = new std::vector<flx_triangle>((const flx_triangle *)tris, (const flx_triangle *)tris + ntris);
    BVH *b = new BVH();
    b->sbvhThreads = threads; b->sbvhJobSize = (size_t)jobSize;
    try { b->build(copy, mode == 0 ? BVH::Mode::SBVH : mode == 1 ? BVH::Mode::SAH : BVH::Mode::Binned); }
    catch (...) { delete copy; delete b; throw; }
    delete copy;
    *out = b;
    FH_CATCH
}
// Build the 4-wide quantised tree of a scene on the CPU exactly as flx_upload_scene does and CHECK its invariants (tests/test_host.py):
//  every quantised child box contains the child's exact box (real arithmetic), every binary leaf is referenced exactly once and its
//  block carries the leaf's box, count and triangles, every inner record is referenced exactly once, unused slots point at the dummy
//  leaf.  out8 = {wide nodes, leaf data float4s, stack bound, nested, leaves, max children per node histogram packed: [5]=2-slot nodes,
//  [6]=3-slot, [7]=4-slot}.
static int wide_tree_check(const void *nodesv, uint64_t nnodes, const void *trisv, uint64_t ntris, const uint32_t *indices, uint64_t nidx, uint64_t *out8, double *areas2);
int fh_wide_tree_check(const void *nodesv, uint64_t nnodes, const void *trisv, uint64_t ntris, const uint32_t *indices, uint64_t nidx, uint64_t *out8)
{
    return wide_tree_check(nodesv, nnodes, trisv, ntris, indices, nidx, out8, nullptr);
}
// + areas2 = {sum of the EXACT surface areas of everything a wide-node slot refers to, sum of the slots' QUANTISED box areas}: their ratio
// is what the 8-bit boxes cost in expected visits (surface-area heuristic)
int fh_wide_tree_areas(const void *nodesv, uint64_t nnodes, const void *trisv, uint64_t ntris, const uint32_t *indices, uint64_t nidx, uint64_t *out8, double *areas2)
{
    return wide_tree_check(nodesv, nnodes, trisv, ntris, indices, nidx, out8, areas2);
}
static int wide_tree_check(const void *nodesv, uint64_t nnodes, const void *trisv, uint64_t ntris, const uint32_t *indices, uint64_t nidx, uint64_t *out8, double *areas2)
{
    FH_TRY
    double areaExact = 0.0, areaQuant = 0.0;
    const flx_node *nodes = (const flx_node *)nodesv;
    const flx_triangle *tris = (const flx_triangle *)trisv;
    flxw::WideTree w; const char *err = nullptr;
    if (!flxw::build_wide(nodes, nnodes, tris, ntris, indices, nidx, w, &err)) throw std::runtime_error(err ? err : "build_wide failed");
    // leaf blocks by offset
    std::vector<uint32_t> leafOfOffset(w.leafdata.size(), 0xFFFFFFFFu);
    uint64_t nleaves = 0;
    {
        size_t off = 5;                                                   // after the dummy leaf
        for (size_t i = 0; i < nnodes; i++) {
            if (!nodes[i].nPrims) continue;
            nleaves++;
            if (off + 2 + 3 * (size_t)nodes[i].nPrims > w.leafdata.size()) throw std::runtime_error("leaf data too short");
            const flxw::F4 &h0 = w.leafdata[off], &h1 = w.leafdata[off + 1];
            int cnt; memcpy(&cnt, &h0.w, 4);
            if (cnt != nodes[i].nPrims || h0.x != nodes[i].bmin.x || h0.y != nodes[i].bmin.y || h0.z != nodes[i].bmin.z ||
                h1.x != nodes[i].bmax.x || h1.y != nodes[i].bmax.y || h1.z != nodes[i].bmax.z) throw std::runtime_error("leaf header differs from the binary leaf");
            for (uint32_t k = 0; k < nodes[i].nPrims; k++) {
                const flxw::F4 &a = w.leafdata[off + 2 + 3 * k];
                int ti; memcpy(&ti, &a.w, 4);
                if ((uint32_t)ti != indices[nodes[i].iStartOrRight + k] || a.x != tris[ti].v0.p.x) throw std::runtime_error("leaf triangle order differs from the index list");
            }
            leafOfOffset[off] = (uint32_t)i;
            off += 2 + 3 * (size_t)nodes[i].nPrims;
        }
        if (off != w.leafdata.size()) throw std::runtime_error("leaf data size");
    }
    uint64_t hist[5] = {0, 0, 0, 0, 0};
    if (w.rootRef & FLX_WIDE_LEAF_BIT) { out8[0] = w.nodes.size(); out8[1] = w.leafdata.size(); out8[2] = w.maxStack; out8[3] = w.nested; out8[4] = nleaves; out8[5] = out8[6] = out8[7] = 0; return 0; }
    // children are numbered after their parent, so one backwards sweep sees every child before its parent: exact[i] = union of the
    // exact leaf boxes below wide node i, and every slot's REAL-arithmetic planes must enclose the exact box of what hangs there
    std::vector<uint8_t> leafSeen(nnodes, 0), nodeSeen(w.nodes.size(), 0);
    std::vector<Box> exact(w.nodes.size());
    nodeSeen[0] = 1;
    for (size_t wi = w.nodes.size(); wi-- > 0;) {
        const flxw::WNode &n = w.nodes[wi];
        const uint32_t refs[4] = {n.c0, n.c1, n.c2, n.c3};
        const uint32_t ql[3] = {n.qlox, n.qloy, n.qloz}, qh[3] = {n.qhix, n.qhiy, n.qhiz};
        const long double o[3] = {n.ox, n.oy, n.oz}, sc[3] = {n.sx, n.sy, n.sz};
        int used = 0;
        for (int c = 0; c < 4; c++) {
            if (refs[c] == FLX_WIDE_EMPTY) {
                for (int a = 0; a < 3; a++) if (((ql[a] >> (8 * c)) & 255u) != 255u || ((qh[a] >> (8 * c)) & 255u) != 0u) throw std::runtime_error("unused slot without an inverted box");
                continue;
            }
            used++;
            Box sub;
            if (refs[c] & FLX_WIDE_LEAF_BIT) {
                const uint32_t off = refs[c] & FLX_WIDE_OFF_MASK;
                if (off >= leafOfOffset.size() || leafOfOffset[off] == 0xFFFFFFFFu) throw std::runtime_error("leaf ref does not point at a leaf block");
                const uint32_t li = leafOfOffset[off];
                if (leafSeen[li]++) throw std::runtime_error("leaf referenced twice");
                sub.expand(&nodes[li].bmin.x); sub.expand(&nodes[li].bmax.x);
            } else {
                if (refs[c] >= w.nodes.size() || refs[c] <= wi) throw std::runtime_error("inner ref out of range or not after its parent");
                if (nodeSeen[refs[c]]++) throw std::runtime_error("wide node referenced twice");
                sub = exact[refs[c]];
            }
            for (int a = 0; a < 3; a++) {
                const long double lo = o[a] + (long double)((ql[a] >> (8 * c)) & 255u) * sc[a], hi = o[a] + (long double)((qh[a] >> (8 * c)) & 255u) * sc[a];
                if (lo > (long double)sub.mn[a] || hi < (long double)sub.mx[a]) throw std::runtime_error("quantised box does not contain the exact box of its subtree");
            }
            {
                double q[3];
                for (int a = 0; a < 3; a++) q[a] = (double)(((qh[a] >> (8 * c)) & 255u) - (long double)((ql[a] >> (8 * c)) & 255u)) * (double)sc[a];
                areaQuant += q[0] * q[1] + q[1] * q[2] + q[2] * q[0];
                const double e0 = (double)sub.mx[0] - sub.mn[0], e1 = (double)sub.mx[1] - sub.mn[1], e2 = (double)sub.mx[2] - sub.mn[2];
                areaExact += e0 * e1 + e1 * e2 + e2 * e0;
            }
            exact[wi].expand(sub);
        }
        if (used < 2) throw std::runtime_error("wide node with fewer than two children");
        hist[used]++;
        for (int a = 0; a < 3; a++) if ((long double)exact[wi].mn[a] < o[a]) throw std::runtime_error("grid origin above the subtree's min corner");
    }
    {   // the root's exact box is the binary root's
        const flx_node &r = nodes[0];
        if (exact[0].mn[0] != r.bmin.x || exact[0].mn[1] != r.bmin.y || exact[0].mn[2] != r.bmin.z || exact[0].mx[0] != r.bmax.x || exact[0].mx[1] != r.bmax.y || exact[0].mx[2] != r.bmax.z)
            throw std::runtime_error("union of the leaf boxes differs from the binary root's box");
    }
    for (size_t i = 0; i < nnodes; i++) if (nodes[i].nPrims && leafSeen[i] != 1) throw std::runtime_error("binary leaf not referenced exactly once");
    for (size_t i = 0; i < w.nodes.size(); i++) if (!nodeSeen[i]) throw std::runtime_error("wide node unreachable");
    out8[0] = w.nodes.size(); out8[1] = w.leafdata.size(); out8[2] = w.maxStack; out8[3] = w.nested; out8[4] = nleaves;
    out8[5] = hist[2]; out8[6] = hist[3]; out8[7] = hist[4];
    if (areas2) { areas2[0] = areaExact; areas2[1] = areaQuant; }
    FH_CATCH
}

// BVH::refit over caller-owned arrays: the nodes are rewritten in place, *worldRadius follows the new root box
int fh_bvh_refit(void *nodes, uint64_t nnodes, const uint32_t *indices, uint64_t nidx, const void *tris, uint64_t ntris, float *worldRadius)
{
    FH_TRY
    BVH b;
    b.m_nodes.assign((const flx_node *)nodes, (const flx_node *)nodes + nnodes);
    b.m_indices.assign(indices, indices + nidx);
    b.refit(std::vector<flx_triangle>((const flx_triangle *)tris, (const flx_triangle *)tris + ntris));
    memcpy(nodes, b.m_nodes.data(), nnodes * sizeof(flx_node));
    if (worldRadius) *worldRadius = b.worldRadius();
    FH_CATCH
}
// BVH::refitSubset likewise: tris is the full array with the moved triangles in place, moved lists them (strictly ascending)
int fh_bvh_refit_subset(void *nodes, uint64_t nnodes, const uint32_t *indices, uint64_t nidx, const void *tris, uint64_t ntris, const uint32_t *moved, uint64_t nmoved,
                        float *worldRadius)
{
    FH_TRY
    BVH b;
    b.m_nodes.assign((const flx_node *)nodes, (const flx_node *)nodes + nnodes);
    b.m_indices.assign(indices, indices + nidx);
    b.refitSubset(std::vector<flx_triangle>((const flx_triangle *)tris, (const flx_triangle *)tris + ntris), std::vector<uint32_t>(moved, moved + nmoved));
    memcpy(nodes, b.m_nodes.data(), nnodes * sizeof(flx_node));
    if (worldRadius) *worldRadius = b.worldRadius();
    FH_CATCH
}
// flx_pose.h on the CPU: out160[k] = in160[k] posed by the 3 x 4 row-major transform xform12 (in and out may be the same buffer)
int fh_pose_triangles(const void *in160, void *out160, uint64_t count, const float *xform12)
{
    FH_TRY
    if (!xform12 || (count && (!in160 || !out160))) throw std::runtime_error("fh_pose_triangles: null argument");
    flx::ps_pose_triangles(xform12, in160, out160, (size_t)count);
    FH_CATCH
}
// ---- emissive triangles as lights on the CPU (csrc/flx_mesh_light.h: the functions the kernels run, in the order the kernels sum)
// the ascending list of the triangles whose material emits
static std::vector<uint32_t> meshLightList(const flx_triangle *t, uint64_t ntris, const flx_material *m, uint64_t nmat)
{
    std::vector<uint32_t> list;
    for (uint64_t i = 0; i < ntris; i++) {
        if (t[i].matId < 0 || (uint64_t)t[i].matId >= nmat) throw std::runtime_error("fh_mesh_light: triangle material id out of range");
        const flx_vec3 &ke = m[t[i].matId].Ke;
        if (flxml::ml_is_emissive(ke.x, ke.y, ke.z)) list.push_back((uint32_t)i);
    }
    return list;
}
static flx::f3 meshLightVertex(const flx_triangle &t, int v) { const flx_vertex &x = v == 0 ? t.v0 : v == 1 ? t.v1 : t.v2; return flx::mk3(x.p.x, x.p.y, x.p.z); }
struct MeshLightTable { std::vector<uint32_t> list; std::vector<float> cdf, pick; double total = 0.0; uint32_t lastPick = ML_NONE; };
static MeshLightTable meshLightTable(const flx_triangle *t, uint64_t ntris, const flx_material *m, uint64_t nmat)
{
    MeshLightTable T;
    T.list = meshLightList(t, ntris, m, nmat);
    const uint32_t n = (uint32_t)T.list.size();
    T.cdf.assign(n, 0.0f); T.pick.assign(n, 0.0f);
    T.total = flxml::ml_build_table(T.list.data(), n, [&](uint32_t i, int v) { return meshLightVertex(t[i], v); },
                                    [&](uint32_t i) { const flx_vec3 &ke = m[t[i].matId].Ke; return flx::mk3(ke.x, ke.y, ke.z); }, T.cdf.data(), T.pick.data(), &T.lastPick);
    return T;
}
// what flx_mesh_lights_read returns for the same triangles and materials, byte for byte; null arrays = the count only
int fh_mesh_light_table(const void *tris160, uint64_t ntris, const void *mats80, uint64_t nmat, uint32_t *outCount, uint32_t *outTris, float *outCdf, float *outPick,
                        double *outTotal)
{
    FH_TRY
    const MeshLightTable T = meshLightTable((const flx_triangle *)tris160, ntris, (const flx_material *)mats80, nmat);
    const size_t n = T.total > 0.0 ? T.list.size() : 0;
    if (outCount) *outCount = (uint32_t)n;
    if (outTotal) *outTotal = T.total;
    if (n && outTris) memcpy(outTris, T.list.data(), n * 4);
    if (n && outCdf) memcpy(outCdf, T.cdf.data(), n * 4);
    if (n && outPick) memcpy(outPick, T.pick.data(), n * 4);
    FH_CATCH
}
// ml_pick over a given table for m values of r (lastPick: the last entry of pick that is > 0); ml_find over a given list for m triangles
int fh_mesh_light_pick(const float *cdf, const float *pick, uint32_t n, const float *r, uint64_t m, uint32_t *out)
{
    FH_TRY
    uint32_t lastPick = ML_NONE;
    for (uint32_t k = 0; k < n; k++) if (pick[k] > 0.0f) lastPick = k;
    if (lastPick == ML_NONE) throw std::runtime_error("fh_mesh_light_pick: the table has no light with pick > 0");
    for (uint64_t i = 0; i < m; i++) out[i] = flxml::ml_pick(cdf, n, lastPick, r[i]);
    FH_CATCH
}
int fh_mesh_light_find(const uint32_t *list, uint32_t n, const uint32_t *tri, uint64_t m, uint32_t *out)
{
    FH_TRY
    for (uint64_t i = 0; i < m; i++) out[i] = flxml::ml_find(list, n, tri[i]);
    FH_CATCH
}
// what flx_mesh_lights_sample returns: m triples (pick, r1, r2) -> the light, out8 = {P.xyz, pdfA, n_g.xyz, area}, and (where not null) the
// three barycentric coefficients of P
int fh_mesh_light_sample(const void *tris160, uint64_t ntris, const void *mats80, uint64_t nmat, const float *r3, uint64_t m, uint32_t *outLight, float *out8, float *outBary3)
{
    FH_TRY
    const flx_triangle *t = (const flx_triangle *)tris160;
    const MeshLightTable T = meshLightTable(t, ntris, (const flx_material *)mats80, nmat);
    if (T.lastPick == ML_NONE) throw std::runtime_error("fh_mesh_light_sample: the scene has no light (no emissive triangle with a positive weight)");
    for (uint64_t i = 0; i < m; i++) {
        const uint32_t k = flxml::ml_pick(T.cdf.data(), (uint32_t)T.list.size(), T.lastPick, r3[3 * i]);
        const flx_triangle &tr = t[T.list[k]];
        const flx::f3 p0 = meshLightVertex(tr, 0), p1 = meshLightVertex(tr, 1), p2 = meshLightVertex(tr, 2);
        const flx::f3 P = flxml::ml_sample_triangle(p0, p1, p2, r3[3 * i + 1], r3[3 * i + 2]), ng = flxml::ml_normal(p0, p1, p2);
        const float area = flxml::ml_area(p0, p1, p2);
        outLight[i] = k;
        float *o = out8 + 8 * i;
        o[0] = P.x; o[1] = P.y; o[2] = P.z; o[3] = flxml::ml_pdf_area(T.pick[k], area); o[4] = ng.x; o[5] = ng.y; o[6] = ng.z; o[7] = area;
        if (outBary3) { const flx::f3 b = flxml::ml_bary(r3[3 * i + 1], r3[3 * i + 2]); outBary3[3 * i] = b.x; outBary3[3 * i + 1] = b.y; outBary3[3 * i + 2] = b.z; }
    }
    FH_CATCH
}
// Scene::objectOfTriangle / objectNames: ids (room for the scene's triangles) and the names joined by '\n' (*needed: bytes incl. the final 0)
int fh_scene_objects(void *s, uint32_t *objectOf, uint32_t *nobjects, char *names, uint64_t cap, uint64_t *needed)
{
    FH_TRY
    Scene *sc = (Scene *)s;
    std::string joined;
    for (const std::string &n : sc->objectNames()) { joined += n; joined += '\n'; }
    if (nobjects) *nobjects = (uint32_t)sc->objectNames().size();
    if (needed) *needed = joined.size() + 1;
    if (objectOf) { const std::vector<uint32_t> v = sc->objectOfTriangle(); if (!v.empty()) memcpy(objectOf, v.data(), v.size() * 4); }
    if (names) { if (cap < joined.size() + 1) throw std::runtime_error("fh_scene_objects: buffer too small"); memcpy(names, joined.c_str(), joined.size() + 1); }
    FH_CATCH
}
// the grid of one wide node from its ns child boxes (cmin / cmax: ns x 3 floats): which = 0 build_wide's quantiser (long double), 1 the refit's
// (fp64 with error-free differences, csrc/flx_refit.h).  out12 = {o.xyz, s.xyz (float bits), qlo.xyz, qhi.xyz}
int fh_wide_quantise(int which, const float *cmin, const float *cmax, int ns, uint32_t *out12)
{
    FH_TRY
    if (ns < 1 || ns > 4) throw std::runtime_error("fh_wide_quantise: 1..4 children");
    float o[3], s[3]; uint32_t qlo[3], qhi[3];
    if (which == 0) {
        float mn[4][3], mx[4][3];
        for (int k = 0; k < ns; k++) for (int a = 0; a < 3; a++) { mn[k][a] = cmin[3 * k + a]; mx[k][a] = cmax[3 * k + a]; }
        if (!flxw::quantise_children(mn, mx, ns, o, s, qlo, qhi)) throw std::runtime_error("wide tree: box extent out of range");
    } else {
        for (int a = 0; a < 3; a++) {
            float mn[4], mx[4];
            for (int k = 0; k < ns; k++) { mn[k] = cmin[3 * k + a]; mx[k] = cmax[3 * k + a]; }
            flxrf::rf_quantise_axis(mn, mx, ns, &o[a], &s[a], &qlo[a], &qhi[a]);
        }
    }
    memcpy(out12, o, 12); memcpy(out12 + 3, s, 12); memcpy(out12 + 6, qlo, 12); memcpy(out12 + 9, qhi, 12);
    FH_CATCH
}
// build_wide's extra outputs (parent, depth and leaf tables) checked against the child refs they restate
int fh_wide_tables_check(const void *nodesv, uint64_t nnodes, const void *trisv, uint64_t ntris, const uint32_t *indices, uint64_t nidx, uint64_t *out2)
{
    FH_TRY
    flxw::WideTree w; const char *err = nullptr;
    if (!flxw::build_wide((const flx_node *)nodesv, nnodes, (const flx_triangle *)trisv, ntris, indices, nidx, w, &err)) throw std::runtime_error(err ? err : "build_wide failed");
    if (w.nodeParent.size() != w.nodes.size() || w.nodeDepth.size() != w.nodes.size() || w.leafParent.size() != w.leafOffset.size()) throw std::runtime_error("table sizes");
    auto ref = [&](uint32_t up) { const flxw::WNode &p = w.nodes[up & 0x3FFFFFFFu]; const uint32_t r[4] = {p.c0, p.c1, p.c2, p.c3}; return r[up >> 30]; };
    const bool oneLeaf = (w.rootRef & FLX_WIDE_LEAF_BIT) != 0;
    for (size_t i = 0; i < w.nodes.size(); i++) {
        if (i == 0) { if (w.nodeParent[0] != FLX_WIDE_NO_PARENT || w.nodeDepth[0] != 0) throw std::runtime_error("root has a parent"); continue; }
        const uint32_t up = w.nodeParent[i];
        if ((up & 0x3FFFFFFFu) >= i || ref(up) != i) throw std::runtime_error("node parent does not refer back");
        if (w.nodeDepth[i] != w.nodeDepth[up & 0x3FFFFFFFu] + 1) throw std::runtime_error("node depth");
    }
    size_t off = 5;
    for (size_t l = 0; l < w.leafOffset.size(); l++) {
        if (w.leafOffset[l] != off) throw std::runtime_error("leaf offset");
        int cnt; memcpy(&cnt, &w.leafdata[off].w, 4); off += 2 + 3 * (size_t)cnt;
        if (oneLeaf) { if (w.leafParent[l] != FLX_WIDE_NO_PARENT) throw std::runtime_error("the only leaf has a parent"); continue; }
        if (ref(w.leafParent[l]) != (FLX_WIDE_LEAF_BIT | w.leafOffset[l])) throw std::runtime_error("leaf parent does not refer back");
    }
    if (off != w.leafdata.size()) throw std::runtime_error("leaf offsets do not cover the leaf data");
    out2[0] = w.nodes.size(); out2[1] = w.leafOffset.size();
    FH_CATCH
}

// ---- the cost sums of flx_tree_cost on the CPU (csrc/flx_tree_cost.h: the functions the kernels run) and the header's helper
// the binary tree's four sums from a BNode array as flx_tree_read returns it, the listed records (the first is the root) and the TriRec array
int fh_tree_cost_binary(const void *bnodes64, const uint32_t *list, uint64_t n, const void *trirecs48, uint64_t nrec, double *out4)
{
    FH_TRY
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (uint64_t i = 0; i < n; i++) {
        const float *w = (const float *)bnodes64 + 16 * (size_t)list[i];
        uint32_t refs[2], counts[2] = {0, 0};
        memcpy(refs, w + 12, 8);
        for (int h = 0; h < 2; h++) if (refs[h] & FLX_TC_LEAF_BIT) {
            const uint64_t slot = refs[h] & ~FLX_TC_LEAF_BIT;
            if (slot >= nrec) throw std::runtime_error("fh_tree_cost_binary: leaf slot outside the triangle records");
            memcpy(&counts[h], (const float *)trirecs48 + 12 * slot + 7, 4);
        }
        flxtc::tc_binary_record(w, refs[0], refs[1], counts, i == 0, s);
    }
    memcpy(out4, s, sizeof(s));
    FH_CATCH
}
double fh_tree_cost_value(const double *sums4) { return flxTreeCostValue(sums4); }

// ---- RebuildJob (rebuild_job.hpp): one BVH build on a worker thread
int fh_rebuild_job_create(void **out) { FH_TRY *out = new RebuildJob(); FH_CATCH }
int fh_rebuild_job_destroy(void *j) { delete (RebuildJob *)j; return 0; }
int fh_rebuild_job_start(void *j, const void *tris, uint64_t ntris, int mode, int threads)
{
    FH_TRY
    ((RebuildJob *)j)->start(std::vector<flx_triangle>((const flx_triangle *)tris, (const flx_triangle *)tris + ntris),
                             mode == 0 ? BVH::Mode::SBVH : mode == 1 ? BVH::Mode::SAH : BVH::Mode::Binned, threads);
    FH_CATCH
}
int fh_rebuild_job_ready(void *j) { return ((RebuildJob *)j)->ready() ? 1 : 0; }
int fh_rebuild_job_wait(void *j) { FH_TRY ((RebuildJob *)j)->wait(); FH_CATCH }
int fh_rebuild_job_hold(void *j, int on) { FH_TRY ((RebuildJob *)j)->hold(on != 0); FH_CATCH }
// hands the tree over as a BVH handle (fh_bvh_counts / fh_bvh_get / fh_bvh_destroy) and, where snapshot is not null, the snapshot's triangles
int fh_rebuild_job_take(void *j, void **bvh, void *snapshot, uint64_t capTris, uint64_t *ntris)
{
    FH_TRY
    std::unique_ptr<BVH> b; std::vector<flx_triangle> snap;
    ((RebuildJob *)j)->take(b, snap);
    if (ntris) *ntris = snap.size();
    if (snapshot) { if (snap.size() > capTris) throw std::runtime_error("fh_rebuild_job_take: buffer too small"); memcpy(snapshot, snap.data(), snap.size() * sizeof(flx_triangle)); }
    *bvh = b.release();
    FH_CATCH
}

int fh_usable_threads() { return BVH::usableThreads(); }
int fh_bvh_destroy(void *b) { delete (BVH *)b; return 0; }
int fh_bvh_counts(void *b, uint64_t *nnodes, uint64_t *nidx, uint32_t *metrics4)
{
    FH_TRY
    BVH *v = (BVH *)b; *nnodes = v->m_nodes.size(); *nidx = v->m_indices.size();
    if (metrics4) { metrics4[0] = v->metrics.depth; metrics4[1] = v->metrics.splits; metrics4[2] = v->metrics.duplicates; metrics4[3] = v->metrics.spatialSplits; }
    FH_CATCH
}
int fh_bvh_get(void *b, void *nodes, uint32_t *indices, float *worldRadius)
{
    FH_TRY
    BVH *v = (BVH *)b;
    if (nodes) memcpy(nodes, v->m_nodes.data(), v->m_nodes.size() * sizeof(flx_node));
    if (indices) memcpy(indices, v->m_indices.data(), v->m_indices.size() * 4);
    if (worldRadius) *worldRadius = v->worldRadius();
    FH_CATCH
}
int fh_bvh_export(void *b, const char *path) { FH_TRY ((BVH *)b)->exportTo(path); FH_CATCH }
int fh_bvh_import(const char *path, void **out)
{
    FH_TRY
    BVH *b = new BVH();
    if (!b->importFrom(path)) { delete b; throw std::runtime_error(std::string("cannot import BVH from ") + path); }
    *out = b;
    FH_CATCH
}

// ---- Environment map
int fh_envmap_load(const char *path, void **out) { FH_TRY *out = new EnvironmentMap(path); FH_CATCH }
int fh_envmap_from_memory(int w, int h, const float *rgb, void **out) { FH_TRY *out = new EnvironmentMap(w, h, rgb); FH_CATCH }
int fh_envmap_destroy(void *e) { delete (EnvironmentMap *)e; return 0; }
int fh_envmap_dims(void *e, int *w, int *h) { *w = ((EnvironmentMap *)e)->getWidth(); *h = ((EnvironmentMap *)e)->getHeight(); return 0; }
int fh_envmap_get(void *e, float *rgb, float *prob, int *alias, float *pdf)
{
    FH_TRY
    EnvironmentMap *m = (EnvironmentMap *)e; size_t n = (size_t)m->getWidth() * m->getHeight();
    if (rgb) memcpy(rgb, m->getData(), n * 3 * 4);
    if (prob) memcpy(prob, m->getProbTable(), n * 4);
    if (alias) memcpy(alias, m->getAliasTable(), n * 4);
    if (pdf) memcpy(pdf, m->getPdfTable(), n * 4);
    FH_CATCH
}

} // extern "C"

// ---- headless Tracer (C++ render driver over HipContext / libfluctus_hip.so)
#include "tracer.hpp"
extern "C" {
int fh_tracer_create(int width, int height, int device, uint32_t numTasks, void **out) { FH_TRY *out = new Tracer(width, height, device, numTasks); FH_CATCH }
int fh_tracer_create_multi(int width, int height, const int *devices, int ndev, uint32_t numTasks, void **out)
{
    FH_TRY *out = new Tracer(width, height, std::vector<int>(devices, devices + ndev), numTasks); FH_CATCH
}
int fh_tracer_num_ranks(void *t) { return (int)((Tracer *)t)->numRanks(); }
int fh_tracer_read_accumulation(void *t, float *out, uint64_t capFloats)
{
    FH_TRY
    std::vector<float> px; ((Tracer *)t)->readAccumulation(px);
    if (px.size() > capFloats) throw std::runtime_error("fh_tracer_read_accumulation: buffer too small");
    memcpy(out, px.data(), px.size() * sizeof(float));
    FH_CATCH
}
int fh_tracer_destroy(void *t) { delete (Tracer *)t; return 0; }
int fh_tracer_init(void *t, int width, int height, const char *scene) { FH_TRY ((Tracer *)t)->init(width, height, scene); FH_CATCH }
int fh_tracer_update_geometry(void *t, const void *tris, uint64_t ntris)
{
    FH_TRY ((Tracer *)t)->updateGeometry(std::vector<flx_triangle>((const flx_triangle *)tris, (const flx_triangle *)tris + ntris)); FH_CATCH
}
int fh_tracer_update_geometry_subset(void *t, const void *tris, const uint32_t *indices, uint64_t count)
{
    FH_TRY
    ((Tracer *)t)->updateGeometry(std::vector<uint32_t>(indices, indices + count), std::vector<flx_triangle>((const flx_triangle *)tris, (const flx_triangle *)tris + count));
    FH_CATCH
}
int fh_tracer_define_objects(void *t, const uint32_t *objectOf, uint64_t ntris, uint32_t nobjects)
{
    FH_TRY ((Tracer *)t)->defineObjects(std::vector<uint32_t>(objectOf, objectOf + (objectOf ? ntris : 0)), nobjects); FH_CATCH
}
int fh_tracer_define_scene_objects(void *t, uint32_t *nobjects) { FH_TRY ((Tracer *)t)->defineObjects(); if (nobjects) *nobjects = ((Tracer *)t)->numObjects(); FH_CATCH }
int fh_tracer_pose_objects(void *t, const uint32_t *ids, const float *xforms12, uint32_t count)
{
    FH_TRY ((Tracer *)t)->poseObjects(std::vector<uint32_t>(ids, ids + (ids ? count : 0)), std::vector<float>(xforms12, xforms12 + (xforms12 ? 12 * (size_t)count : 0))); FH_CATCH
}
int fh_tracer_get_triangles(void *t, void *out, uint64_t capTris, uint64_t *ntris)
{
    FH_TRY
    auto &tr = ((Tracer *)t)->getScene()->getTriangles();
    *ntris = tr.size();
    if (out) { if (tr.size() > capTris) throw std::runtime_error("fh_tracer_get_triangles: buffer too small"); memcpy(out, tr.data(), tr.size() * sizeof(flx_triangle)); }
    FH_CATCH
}
// the rebuild policy (Tracer::setRebuildPolicy).  mode: 0 off, 1 blocking, 2 background
int fh_tracer_set_rebuild_policy(void *t, int mode, double threshold) { FH_TRY ((Tracer *)t)->setRebuildPolicy((Tracer::RebuildMode)mode, threshold); FH_CATCH }
int fh_tracer_rebuild_state(void *t, uint32_t *count, int *pending, double *lastRatio)
{
    FH_TRY
    Tracer *tr = (Tracer *)t;
    if (count) *count = tr->rebuildCount();
    if (pending) *pending = tr->rebuildPending() ? 1 : 0;
    if (lastRatio) *lastRatio = tr->lastCostRatio();
    FH_CATCH
}
int fh_tracer_wait_for_rebuild(void *t) { FH_TRY ((Tracer *)t)->waitForRebuild(); FH_CATCH }
int fh_tracer_get_option(void *t, uint32_t rank, const char *name, int *value) { FH_TRY *value = ((Tracer *)t)->getOption(rank, name ? name : ""); FH_CATCH }
int fh_tracer_hold_rebuild(void *t, int on) { FH_TRY ((Tracer *)t)->holdRebuild(on != 0); FH_CATCH }
int fh_tracer_tree_cost(void *t, double *out8) { FH_TRY const std::array<double, 8> s = ((Tracer *)t)->treeCost(); memcpy(out8, s.data(), sizeof(s)); FH_CATCH }
int fh_tracer_tree_read(void *t, uint32_t rank, int which, void *out, uint64_t cap, uint64_t *needed)
{
    FH_TRY
    std::vector<uint8_t> a; ((Tracer *)t)->treeRead(rank, which, a);
    *needed = a.size();
    if (out) { if (a.size() > cap) throw std::runtime_error("fh_tracer_tree_read: buffer too small"); memcpy(out, a.data(), a.size()); }
    FH_CATCH
}
int fh_tracer_set_envmap(void *t, const char *hdr) { FH_TRY ((Tracer *)t)->setEnvMap(hdr); FH_CATCH }
int fh_tracer_params(void *t, void *out240, const void *in240)
{
    FH_TRY
    Tracer *tr = (Tracer *)t;
    if (in240) { memcpy(&tr->getParams(), in240, 240); tr->paramsChanged(); }
    if (out240) memcpy(out240, &tr->getParams(), 240);
    FH_CATCH
}
int fh_tracer_update(void *t, void *counters32) { FH_TRY ((Tracer *)t)->update(); if (counters32) memcpy(counters32, &((Tracer *)t)->lastCounters(), 32); FH_CATCH }
int fh_tracer_set_cache_dirs(void *t, const char *hierarchies, const char *states) { ((Tracer *)t)->hierarchyCacheDir = hierarchies ? hierarchies : ""; ((Tracer *)t)->stateDir = states ? states : ""; return 0; }
int fh_tracer_save_state(void *t) { return ((Tracer *)t)->saveState() ? 0 : 1; }
int fh_tracer_load_state(void *t) { return ((Tracer *)t)->loadState() ? 0 : 1; }
int fh_tracer_scene_hash(void *t, char *out, uint64_t cap) { const std::string &h = ((Tracer *)t)->getSceneHash(); if (h.size() + 1 > cap) return 1; memcpy(out, h.c_str(), h.size() + 1); return 0; }
uint64_t fh_xxh64(const void *data, uint64_t len, uint64_t seed) { return xxh64(data, (size_t)len, seed); }
int fh_tracer_render_single(void *t, int spp, int denoise) { FH_TRY ((Tracer *)t)->renderSingle(spp, denoise != 0); FH_CATCH }
int fh_tracer_render_adaptive(void *t, int minSpp, int maxSpp, float threshold, int denoise, uint64_t *outSamples)
{ FH_TRY const uint64_t n = ((Tracer *)t)->renderAdaptive(minSpp, maxSpp, threshold, denoise != 0); if (outSamples) *outSamples = n; FH_CATCH }
int fh_tracer_set_option(void *t, const char *name, int value) { FH_TRY ((Tracer *)t)->setOption(name ? name : "", value); FH_CATCH }
int fh_tracer_set_denoiser(void *t, int on) { FH_TRY ((Tracer *)t)->setDenoiser(on != 0); FH_CATCH }
int fh_tracer_set_denoiser_strength(void *t, float s) { FH_TRY ((Tracer *)t)->setDenoiserStrength(s); FH_CATCH }
int fh_tracer_set_denoiser_mode(void *t, int mode) { FH_TRY ((Tracer *)t)->setDenoiserMode((Tracer::DenoiserMode)mode); FH_CATCH }
int fh_tracer_set_temporal_reprojection(void *t, int on) { FH_TRY ((Tracer *)t)->setTemporalReprojection(on != 0); FH_CATCH }
int fh_tracer_get_temporal_reprojection(void *t) { return ((Tracer *)t)->getTemporalReprojection() ? 1 : 0; }
int fh_tracer_set_motion_reprojection(void *t, int on) { FH_TRY ((Tracer *)t)->setMotionReprojection(on != 0); FH_CATCH }
int fh_tracer_get_motion_reprojection(void *t) { return ((Tracer *)t)->getMotionReprojection() ? 1 : 0; }
int fh_tracer_set_deform_reprojection(void *t, int on) { FH_TRY ((Tracer *)t)->setDeformReprojection(on != 0); FH_CATCH }
int fh_tracer_get_deform_reprojection(void *t) { return ((Tracer *)t)->getDeformReprojection() ? 1 : 0; }
int fh_tracer_set_max_history(void *t, float n) { FH_TRY ((Tracer *)t)->setMaxHistory(n); FH_CATCH }
int fh_tracer_set_history_rectification(void *t, int on) { FH_TRY ((Tracer *)t)->setHistoryRectification(on != 0); FH_CATCH }
int fh_tracer_get_history_rectification(void *t) { return ((Tracer *)t)->getHistoryRectification() ? 1 : 0; }
int fh_tracer_set_rectify_delay(void *t, int frames) { FH_TRY ((Tracer *)t)->setRectifyDelay(frames); FH_CATCH }
int fh_tracer_get_rectify_delay(void *t) { return (int)((Tracer *)t)->getRectifyDelay(); }
// measure != 0: every rectify of update() also reads the mark before and after (blocking).  out_share: the last such share (NaN before one)
int fh_tracer_rectify_info(void *t, int measure, double *out_share, uint32_t *out_count)
{
    FH_TRY Tracer *tr = (Tracer *)t; tr->measureRetained = measure != 0; if (out_share) *out_share = tr->lastRetainedShare(); if (out_count) *out_count = tr->rectifyCount(); FH_CATCH
}
int fh_tracer_set_mesh_lights(void *t, int on) { FH_TRY ((Tracer *)t)->setMeshLights(on != 0); FH_CATCH }
int fh_tracer_set_mesh_lights_wavefront(void *t, int on) { FH_TRY ((Tracer *)t)->setMeshLightsWavefront(on != 0); FH_CATCH }
int fh_tracer_get_mesh_lights_wavefront(void *t) { return ((Tracer *)t)->getMeshLightsWavefront() ? 1 : 0; }
int fh_tracer_mesh_light_count(void *t, uint32_t *out) { FH_TRY *out = ((Tracer *)t)->meshLightCount(); FH_CATCH }
int fh_tracer_toggle_renderer(void *t) { FH_TRY ((Tracer *)t)->toggleRenderer(); FH_CATCH }
int fh_tracer_uses_wavefront(void *t) { return ((Tracer *)t)->usesWavefront() ? 1 : 0; }
int fh_tracer_stats(void *t, uint64_t *out4)
{
    FH_TRY RenderStats s = ((Tracer *)t)->getContext()->getStats(); out4[0] = s.primaryRays; out4[1] = s.extensionRays; out4[2] = s.shadowRays; out4[3] = s.samples; FH_CATCH
}
int fh_tracer_run_benchmark(void *t, double seconds, int iterations, char *csv, uint64_t cap)
{
    FH_TRY
    std::string s = ((Tracer *)t)->runBenchmark(seconds, iterations);
    if (csv && cap) { size_t n = s.size() < cap - 1 ? s.size() : cap - 1; memcpy(csv, s.data(), n); csv[n] = 0; }
    FH_CATCH
}
int fh_tracer_read_pixels(void *t, int which, float *out, uint64_t capFloats)
{
    FH_TRY
    std::vector<float> px; ((Tracer *)t)->getContext()->readPixels(which, px);
    if (px.size() > capFloats) throw std::runtime_error("fh_tracer_read_pixels: buffer too small");
    memcpy(out, px.data(), px.size() * 4);
    FH_CATCH
}
int fh_tracer_save_image(void *t, const char *path) { FH_TRY ((Tracer *)t)->saveImage(path); FH_CATCH }
}
