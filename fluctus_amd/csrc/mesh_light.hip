// mesh_light.hip -- the table of emissive triangles (option "mesh_lights") built on the stream from the triangles as they stand
// (Scene::tris, which every refit keeps current): weights, prefix sums and normalisation in the order flx_mesh_light.h fixes, no atomics, so two
// builds of the same inputs are the same bytes and host_capi.cpp's fh_mesh_light_table gives them too.  And the test hook behind
// flx_mesh_lights_sample.  The integrator that samples the table: microkernel.hip.
#include "flx_launch.h"
#include "flx_mesh_light.h"

namespace flxd {
using namespace flxml;

#define ML_BLOCK 256            // threads per block of the per-light kernels (== ML_SCAN_BLOCK: one block's lights are one run)
static_assert(ML_BLOCK == ML_SCAN_BLOCK, "k_ml_finish reduces lastPick per run");

__global__ __launch_bounds__(ML_BLOCK) void k_ml_weights(Scene sc, MeshLights ml)
{
    const uint32_t k = blockIdx.x * ML_BLOCK + threadIdx.x;
    if (k >= ml.n) return;
    f3 p0, p1, p2;
    ml_vertices(sc, ml.tri[k], &p0, &p1, &p2);
    ml.w[k] = ml_weight(p0, p1, p2, V(sc.materials[ml_material(sc, ml.tri[k])].Ke));
}

// step 1: one thread per run of ML_SCAN_BLOCK lights, left to right
__global__ __launch_bounds__(64) void k_ml_scan(MeshLights ml, uint32_t runs)
{
    const uint32_t b = blockIdx.x * 64 + threadIdx.x;
    if (b >= runs) return;
    const uint32_t first = b * ML_SCAN_BLOCK, end = first + ML_SCAN_BLOCK < ml.n ? first + ML_SCAN_BLOCK : ml.n;
    double s = 0.0; uint32_t last = ML_NONE;
    for (uint32_t k = first; k < end; k++) {
        const float w = ml.w[k];
        if (w > 0.0f) last = k;
        s = s + (double)w; ml.local[k] = s;
    }
    ml.runSum[b] = s; ml.runLast[b] = last;
}

// step 2, and the last light with a weight: one thread, left to right over the runs
__global__ void k_ml_offsets(MeshLights ml, uint32_t runs)
{
    if (blockIdx.x | threadIdx.x) return;
    double o = 0.0; uint32_t last = ML_NONE;
    ml.off[0] = 0.0;
    for (uint32_t b = 0; b < runs; b++) {
        o = o + ml.runSum[b]; ml.off[b + 1] = o;
        if (ml.runLast[b] != ML_NONE) last = ml.runLast[b];
    }
    *ml.total = o; ml.hdr[0] = last;
}

// steps 3 and 4: one thread per light; the run's last light with pick > 0 by a tree of maxima in LDS (order cannot matter: integers)
__global__ __launch_bounds__(ML_BLOCK) void k_ml_finish(MeshLights ml)
{
    __shared__ uint32_t s_last[ML_BLOCK];
    const uint32_t k = blockIdx.x * ML_BLOCK + threadIdx.x;
    uint32_t mine = 0u;                                         // k + 1 of a light with pick > 0
    if (k < ml.n) {
        const double total = *ml.total; const uint32_t lastLive = ml.hdr[0];
        const float c = ml_cdf(ml.off[k / ML_SCAN_BLOCK] + ml.local[k], total, k == lastLive);
        const float prev = k ? ml_cdf(ml.off[(k - 1u) / ML_SCAN_BLOCK] + ml.local[k - 1u], total, k - 1u == lastLive) : 0.0f;
        const float pk = c - prev;
        ml.cdf[k] = c; ml.pick[k] = pk;
        if (pk > 0.0f) mine = k + 1u;
    }
    s_last[threadIdx.x] = mine;
    __syncthreads();
    for (uint32_t o = ML_BLOCK / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) { const uint32_t a = s_last[threadIdx.x], b = s_last[threadIdx.x + o]; s_last[threadIdx.x] = a > b ? a : b; }
        __syncthreads();
    }
    if (threadIdx.x == 0) ml.runLast[blockIdx.x] = s_last[0];
}

__global__ void k_ml_header(MeshLights ml, uint32_t runs)
{
    if (blockIdx.x | threadIdx.x) return;
    uint32_t last = 0u;
    for (uint32_t b = 0; b < runs; b++) if (ml.runLast[b] > last) last = ml.runLast[b];
    ml.hdr[1] = last ? last - 1u : ML_NONE;
}

// flx_mesh_lights_sample: ml_pick + ml_sample_triangle for given triples; a table without a pickable light returns ML_NONE and zeros
__global__ __launch_bounds__(ML_BLOCK) void k_ml_probe(Scene sc, MeshLights ml, const float *r3, uint32_t count, uint32_t *outLight, float *out8)
{
    const uint32_t i = blockIdx.x * ML_BLOCK + threadIdx.x;
    if (i >= count) return;
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a;
    uint32_t k = ML_NONE;
    const uint32_t lastPick = ml.hdr[1];
    if (ml.n && lastPick != ML_NONE) {
        k = ml_pick(ml.cdf, ml.n, lastPick, r3[3 * (size_t)i]);
        f3 p0, p1, p2;
        ml_vertices(sc, ml.tri[k], &p0, &p1, &p2);
        const f3 P = ml_sample_triangle(p0, p1, p2, r3[3 * (size_t)i + 1], r3[3 * (size_t)i + 2]), n = ml_normal(p0, p1, p2);
        const float area = ml_area(p0, p1, p2);
        a = mk4(P, ml_pdf_area(ml.pick[k], area)); b = mk4(n, area);
    }
    outLight[i] = k;
    reinterpret_cast<float4 *>(out8)[2 * (size_t)i] = a; reinterpret_cast<float4 *>(out8)[2 * (size_t)i + 1] = b;
}

uint32_t mesh_light_runs(uint32_t n) { return (n + ML_SCAN_BLOCK - 1u) / ML_SCAN_BLOCK; }

void launch_mesh_light_build(hipStream_t s, const Scene &sc, const MeshLights &ml)
{
    const uint32_t runs = mesh_light_runs(ml.n);
    if (ml.n) {
        k_ml_weights<<<runs, ML_BLOCK, 0, s>>>(sc, ml);
        k_ml_scan<<<(runs + 63u) / 64u, 64, 0, s>>>(ml, runs);
    }
    k_ml_offsets<<<1, 64, 0, s>>>(ml, runs);
    if (ml.n) k_ml_finish<<<runs, ML_BLOCK, 0, s>>>(ml);
    k_ml_header<<<1, 64, 0, s>>>(ml, runs);
}

void launch_mesh_light_probe(hipStream_t s, const Scene &sc, const MeshLights &ml, const float *r3, uint32_t count, uint32_t *outLight, float *out8)
{
    if (count) k_ml_probe<<<(count + ML_BLOCK - 1) / ML_BLOCK, ML_BLOCK, 0, s>>>(sc, ml, r3, count, outLight, out8);
}

} // namespace flxd
