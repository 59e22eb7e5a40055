// api_mesh_light.hip -- emissive triangles as lights (option "mesh_lights"): the rebuild of their table on the stream
// (kernels: mesh_light.hip; what is summed in which order: flx_mesh_light.h), which flx_upload_scene, flx_update_triangles(_subset),
// flx_objects_pose and the option itself end in, and the two calls that look at it: flx_mesh_lights_read, flx_mesh_lights_sample.
// Whether the table is current is MeshLightState's business (flx_feature_state.h); nothing here writes a flag.
#include "flx_ctx.h"
#include "flx_mesh_light.h"

namespace flxd {
int meshLightsSync(flx_ctx *c)
{
    flx_ctx::MeshLight &m = c->ml;
    if (!m.state.needsBuild()) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    if (!m.t.hdr) {                                       // first build for this scene: the buffers stay until the next upload
        const size_t n = m.list.size(), runs = mesh_light_runs((uint32_t)n);
        MeshLights t;
        if (dalloc(c, m.allocs, &t.tri, n) || dalloc(c, m.allocs, &t.w, n) || dalloc(c, m.allocs, &t.cdf, n) || dalloc(c, m.allocs, &t.pick, n) ||
            dalloc(c, m.allocs, &t.local, n) || dalloc(c, m.allocs, &t.runSum, runs) || dalloc(c, m.allocs, &t.off, runs + 1) ||
            dalloc(c, m.allocs, &t.runLast, runs) || dalloc(c, m.allocs, &t.total, 1) || dalloc(c, m.allocs, &t.hdr, 2)) { m.releaseBuffers(); return 1; }
        if (n) HIPCHK(c, hipMemcpyAsync(t.tri, m.list.data(), n * 4, hipMemcpyHostToDevice, c->stream));
        t.n = (uint32_t)n;
        m.t = t;
    }
    launch_mesh_light_build(c->stream, c->sc, m.t);
    LAUNCHED(c);
    m.state.rebuilt();
    return 0;
}
}

static int meshLightsReady(flx_ctx *c, const char *fn)
{
    NEED(c, c->ml.state.on, std::string(fn) + ": needs flx_set_option(ctx, \"mesh_lights\", 1)");
    NEED(c, c->sc.bnodes, std::string(fn) + ": upload a scene first (flx_upload_scene)");
    NEED(c, c->ml.state.usable(), std::string(fn) + ": the table of emissive triangles was not built (an earlier call failed)");
    HIPCHK(c, hipSetDevice(c->device));
    return 0;
}

extern "C" {

int flx_mesh_lights_read(flx_ctx *c, uint32_t *out_count, uint32_t *out_tris, float *out_cdf, float *out_pick, double *out_total)
{
    ENTER(c, CALL_QUIET);                                 // a read-back of arrays no deferred launch writes
    if (meshLightsReady(c, "flx_mesh_lights_read")) return 1;
    NEED(c, out_count, "flx_mesh_lights_read: null out_count");
    const MeshLights &t = c->ml.t;
    double total = 0.0;
    HIPCHK(c, hipMemcpyAsync(&total, t.total, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint32_t n = total > 0.0 ? t.n : 0u;
    *out_count = n;
    if (out_total) *out_total = total;
    if (n && out_tris) HIPCHK(c, hipMemcpyAsync(out_tris, t.tri, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    if (n && out_cdf) HIPCHK(c, hipMemcpyAsync(out_cdf, t.cdf, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    if (n && out_pick) HIPCHK(c, hipMemcpyAsync(out_pick, t.pick, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int flx_mesh_lights_sample(flx_ctx *c, const float *r3, uint32_t n, uint32_t *out_light, float *out8)
{
    ENTER(c, CALL_QUIET);
    if (meshLightsReady(c, "flx_mesh_lights_sample")) return 1;
    if (!n) return 0;
    NEED(c, r3 && out_light && out8, "flx_mesh_lights_sample: null argument");
    uint32_t hdr[2] = {ML_NONE, ML_NONE};
    HIPCHK(c, hipMemcpyAsync(hdr, c->ml.t.hdr, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    NEED(c, c->ml.t.n && hdr[1] != ML_NONE, "flx_mesh_lights_sample: the scene has no light (no emissive triangle with a positive weight)");
    std::vector<void *> tmp;
    struct Guard { std::vector<void *> &v; ~Guard() { freeAll(v); } } guard{tmp};
    float *dR = nullptr, *dO = nullptr; uint32_t *dL = nullptr;
    if (dalloc(c, tmp, &dR, (size_t)n * 3) || dalloc(c, tmp, &dO, (size_t)n * 8) || dalloc(c, tmp, &dL, n)) return 1;
    HIPCHK(c, hipMemcpyAsync(dR, r3, (size_t)n * 12, hipMemcpyHostToDevice, c->stream));
    launch_mesh_light_probe(c->stream, c->sc, c->ml.t, dR, n, dL, dO);
    LAUNCHED(c);
    HIPCHK(c, hipMemcpyAsync(out_light, dL, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(out8, dO, (size_t)n * 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

} // extern "C"
