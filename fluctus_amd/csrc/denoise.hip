// denoise.hip -- flx_denoise: the guided a-trous denoiser of csrc/flx_denoise.h on the device.
//
// Pipeline per call: k_dn_prepare (resolve the guides, demodulate, pack the working set once), K a-trous passes over two ping-pong
// buffers, the last one fused with the finish step (remodulate, blend, which = 6, the post-processed preview).  blend == 1 or K == 0
// runs k_dn_identity alone.  Every pixel value comes from the header's functions in the header's order, so the results equal
// tests/denoise_cpu.cpp bit for bit.
//
// Layout: 16 x 16 workgroups over the image.  The passes of step 1 and 2 stage their tile plus a halo of 2 s pixels in LDS
// (20^2 / 24^2 records of 40 B: 16 / 23 KB); the wider steps, whose halo would outweigh the tile, gather from L2.  The working set is
// SoA: e = float4 (demodulated radiance, w = valid), g = float4 (normal, a'.x), g2 = float2 (a'.y, a'.z) -- the guides are packed once
// and read by every pass.
#include "flx_device.h"
#include "flx_denoise.h"
#include "flx_denoise_vg.h"

namespace flxd {

#define DN_BX 16
#define DN_BY 16

struct DnWork {
    float4 *e[2];       // ping-pong demodulated radiance (w: 1 valid / 0 invalid)
    float4 *g;          // normal.xyz, a'.x
    float2 *g2;         // a'.y, a'.z
};

__device__ __forceinline__ dn_pix dn_unpack(float4 e, float4 g, float2 g2)
{
    dn_pix p;
    p.e = mk3(e.x, e.y, e.z); p.valid = e.w != 0.0f;
    p.n = mk3(g.x, g.y, g.z); p.a = mk3(g.w, g2.x, g2.y);
    return p;
}

__device__ __forceinline__ dn_pix dn_prepare_at(const Frame &fr, uint32_t i, f3 *c, float4 *px)
{
    *px = reinterpret_cast<const float4 *>(fr.pixels)[i];
    const float4 a = reinterpret_cast<const float4 *>(fr.aovAlbedo)[i], n = reinterpret_cast<const float4 *>(fr.aovNormal)[i];
    return dn_prepare(&px->x, &a.x, &n.x, c);
}

// which = 6 and the preview of pixel i
__device__ __forceinline__ void dn_store(const Frame &fr, float *out6, uint32_t i, const float4 &px, const dn_pix &pi, f3 c, f3 ef,
                                         float blend, bool identity, const flx_render_params &p)
{
    float4 o, pv;
    dn_finish(&px.x, pi, c, ef, blend, identity, &o.x);
    postprocess_px(&o.x, p.exposure, p.tmOperator, &pv.x);
    reinterpret_cast<float4 *>(out6)[i] = o;
    reinterpret_cast<float4 *>(fr.preview)[i] = pv;
}

__global__ __launch_bounds__(DN_BX * DN_BY) void k_dn_prepare(Frame fr, DnWork wk, int W, int H)
{
    const int x = blockIdx.x * DN_BX + threadIdx.x, y = blockIdx.y * DN_BY + threadIdx.y;
    if (x >= W || y >= H) return;
    const uint32_t i = (uint32_t)y * W + x;
    f3 c; float4 px;
    const dn_pix p = dn_prepare_at(fr, i, &c, &px);
    wk.e[0][i] = make_float4(p.e.x, p.e.y, p.e.z, p.valid ? 1.0f : 0.0f);
    wk.g[i] = make_float4(p.n.x, p.n.y, p.n.z, p.a.x);
    wk.g2[i] = make_float2(p.a.y, p.a.z);
}

__global__ __launch_bounds__(DN_BX * DN_BY) void k_dn_identity(Frame fr, float *out6, int W, int H, flx_render_params p)
{
    const int x = blockIdx.x * DN_BX + threadIdx.x, y = blockIdx.y * DN_BY + threadIdx.y;
    if (x >= W || y >= H) return;
    const uint32_t i = (uint32_t)y * W + x;
    f3 c; float4 px;
    const dn_pix pi = dn_prepare_at(fr, i, &c, &px);
    dn_store(fr, out6, i, px, pi, c, mk3(0.0f), 1.0f, true, p);
}

// one a-trous pass.  S = 1 or 2: the step, tile + halo in LDS; S = 0: step `s`, taps gathered from global memory (L2).
// FINISH: the last pass -- writes which = 6 and the preview instead of the next working set.
template <int S, bool FINISH>
__global__ __launch_bounds__(DN_BX * DN_BY) void k_dn_pass(Frame fr, DnWork wk, int src, int W, int H, int s, float ic, float in_, float ia,
                                                           float *out6, float blend, flx_render_params p)
{
    constexpr int TW = DN_BX + 4 * (S > 0 ? S : 0), TH = DN_BY + 4 * (S > 0 ? S : 0), TN = S > 0 ? TW * TH : 1;
    __shared__ float4 le[TN], lg[TN];
    __shared__ float2 lg2[TN];
    const float4 *E = wk.e[src];
    const int x = blockIdx.x * DN_BX + threadIdx.x, y = blockIdx.y * DN_BY + threadIdx.y;
    const int ox = (int)blockIdx.x * DN_BX - 2 * S, oy = (int)blockIdx.y * DN_BY - 2 * S;     // tile origin (S > 0)
    if (S > 0) {
        for (int t = threadIdx.y * DN_BX + threadIdx.x; t < TN; t += DN_BX * DN_BY) {
            const int gx = ox + t % TW, gy = oy + t / TW;
            if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
                const uint32_t j = (uint32_t)gy * W + gx;
                le[t] = E[j]; lg[t] = wk.g[j]; lg2[t] = wk.g2[j];
            } else {
                le[t] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);     // never read: dn_atrous skips taps outside the image
            }
        }
        __syncthreads();
    }
    if (x >= W || y >= H) return;
    const uint32_t i = (uint32_t)y * W + x;
    dn_pix pi;
    if (S > 0) { const int t = (y - oy) * TW + (x - ox); pi = dn_unpack(le[t], lg[t], lg2[t]); }
    else pi = dn_unpack(E[i], wk.g[i], wk.g2[i]);
    f3 ef = pi.e;
    if (pi.valid) {
        if (S > 0)
            ef = dn_atrous(x, y, W, H, S, pi, ic, in_, ia, [&](int xj, int yj) { const int t = (yj - oy) * TW + (xj - ox); return dn_unpack(le[t], lg[t], lg2[t]); });
        else
            ef = dn_atrous(x, y, W, H, s, pi, ic, in_, ia, [&](int xj, int yj) { const uint32_t j = (uint32_t)yj * W + xj; return dn_unpack(E[j], wk.g[j], wk.g2[j]); });
    }
    if (FINISH) {
        f3 c; float4 px;
        const dn_pix p0 = dn_prepare_at(fr, i, &c, &px);          // the centre as prepared: colour, floored albedo, validity
        dn_store(fr, out6, i, px, p0, c, ef, blend, false, p);
    } else {
        wk.e[src ^ 1][i] = make_float4(ef.x, ef.y, ef.z, pi.valid ? 1.0f : 0.0f);
    }
}

template <bool FINISH>
static void launch_pass(hipStream_t st, dim3 grid, dim3 blk, const Frame &fr, const DnWork &wk, int src, int W, int H, int s, float ic, float in_, float ia,
                        float *out6, float blend, const flx_render_params &p)
{
    if (s == 1) hipLaunchKernelGGL((k_dn_pass<1, FINISH>), grid, blk, 0, st, fr, wk, src, W, H, s, ic, in_, ia, out6, blend, p);
    else if (s == 2) hipLaunchKernelGGL((k_dn_pass<2, FINISH>), grid, blk, 0, st, fr, wk, src, W, H, s, ic, in_, ia, out6, blend, p);
    else hipLaunchKernelGGL((k_dn_pass<0, FINISH>), grid, blk, 0, st, fr, wk, src, W, H, s, ic, in_, ia, out6, blend, p);
}

// the whole call: W * H == fr.localPixels (unpartitioned context), blend already clamped
void launch_denoise(hipStream_t st, const Frame &fr, float4 *e0, float4 *e1, float4 *g, float2 *g2, float *out6, int W, int H, int iterations,
                    float sigma_c, float sigma_n, float sigma_a, float blend, const flx_render_params &p)
{
    const dim3 blk(DN_BX, DN_BY), grid((W + DN_BX - 1) / DN_BX, (H + DN_BY - 1) / DN_BY);
    if (dn_identity(blend, iterations)) {
        hipLaunchKernelGGL(k_dn_identity, grid, blk, 0, st, fr, out6, W, H, p);
        return;
    }
    DnWork wk; wk.e[0] = e0; wk.e[1] = e1; wk.g = g; wk.g2 = g2;
    hipLaunchKernelGGL(k_dn_prepare, grid, blk, 0, st, fr, wk, W, H);
    const float in_ = dn_inv_sq(sigma_n), ia = dn_inv_sq(sigma_a);
    for (int k = 0; k < iterations; k++) {
        const float ic = dn_inv_sq_color(sigma_c, k);
        if (k + 1 == iterations) launch_pass<true>(st, grid, blk, fr, wk, k & 1, W, H, 1 << k, ic, in_, ia, out6, blend, p);
        else launch_pass<false>(st, grid, blk, fr, wk, k & 1, W, H, 1 << k, ic, in_, ia, out6, blend, p);
    }
}

// ---- flx_denoise_variance_guided: the variance-guided filter of csrc/flx_denoise_vg.h.  The same pipeline and layout; the
// variance rides in e.w of the ping-pong radiance (>= 0: valid, the pixel's variance; -1: invalid), so the LDS records stay 40 B and step 2
// keeps its 23 KB tile.  Every pass also needs the 3 x 3 prefilter of the variance at distance 1, which the halo of steps 1 / 2 covers.
__device__ __forceinline__ vg_pix vg_unpack(float4 e, float4 g, float2 g2)
{
    vg_pix p;
    p.d.e = mk3(e.x, e.y, e.z); p.d.valid = e.w >= 0.0f; p.v = e.w;
    p.d.n = mk3(g.x, g.y, g.z); p.d.a = mk3(g.w, g2.x, g2.y);
    return p;
}

// dn_prepare_at with vg_prepare's validity (guided pixels only)
__device__ __forceinline__ dn_pix vg_prepare_at(const Frame &fr, uint32_t i, f3 *c)
{
    const float4 px = reinterpret_cast<const float4 *>(fr.pixels)[i];
    const float4 a = reinterpret_cast<const float4 *>(fr.aovAlbedo)[i], n = reinterpret_cast<const float4 *>(fr.aovNormal)[i];
    return vg_prepare(&px.x, &a.x, &n.x, c);
}

__global__ __launch_bounds__(DN_BX * DN_BY) void k_vg_prepare(Frame fr, DnWork wk, int W, int H, float in_, float ia)
{
    const int x = blockIdx.x * DN_BX + threadIdx.x, y = blockIdx.y * DN_BY + threadIdx.y;
    if (x >= W || y >= H) return;
    const uint32_t i = (uint32_t)y * W + x;
    f3 c;
    const dn_pix p = vg_prepare_at(fr, i, &c);
    float v = -1.0f;
    if (p.valid) {
        const float4 m = reinterpret_cast<const float4 *>(fr.moments)[i];
        v = vg_initial_variance(x, y, W, H, p, &m.x, in_, ia, [&](int xj, int yj) { f3 cj; return vg_prepare_at(fr, (uint32_t)yj * W + xj, &cj); });
    }
    wk.e[0][i] = make_float4(p.e.x, p.e.y, p.e.z, v);
    wk.g[i] = make_float4(p.n.x, p.n.y, p.n.z, p.a.x);
    wk.g2[i] = make_float2(p.a.y, p.a.z);
}

// one variance-guided pass; S and FINISH as k_dn_pass
template <int S, bool FINISH>
__global__ __launch_bounds__(DN_BX * DN_BY) void k_vg_pass(Frame fr, DnWork wk, int src, int W, int H, int s, float sl, float in_, float ia,
                                                           float *out6, float blend, flx_render_params p)
{
    constexpr int TW = DN_BX + 4 * (S > 0 ? S : 0), TH = DN_BY + 4 * (S > 0 ? S : 0), TN = S > 0 ? TW * TH : 1;
    __shared__ float4 le[TN], lg[TN];
    __shared__ float2 lg2[TN];
    const float4 *E = wk.e[src];
    const int x = blockIdx.x * DN_BX + threadIdx.x, y = blockIdx.y * DN_BY + threadIdx.y;
    const int ox = (int)blockIdx.x * DN_BX - 2 * S, oy = (int)blockIdx.y * DN_BY - 2 * S;     // tile origin (S > 0)
    if (S > 0) {
        for (int t = threadIdx.y * DN_BX + threadIdx.x; t < TN; t += DN_BX * DN_BY) {
            const int gx = ox + t % TW, gy = oy + t / TW;
            if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
                const uint32_t j = (uint32_t)gy * W + gx;
                le[t] = E[j]; lg[t] = wk.g[j]; lg2[t] = wk.g2[j];
            } else {
                le[t] = make_float4(0.0f, 0.0f, 0.0f, -1.0f);    // never read: the filter skips taps outside the image
            }
        }
        __syncthreads();
    }
    if (x >= W || y >= H) return;
    const uint32_t i = (uint32_t)y * W + x;
    auto lds = [&](int xj, int yj) { const int t = (yj - oy) * TW + (xj - ox); return vg_unpack(le[t], lg[t], lg2[t]); };
    auto l2 = [&](int xj, int yj) { const uint32_t j = (uint32_t)yj * W + xj; return vg_unpack(E[j], wk.g[j], wk.g2[j]); };
    const vg_pix pi = S > 0 ? lds(x, y) : l2(x, y);
    f3 ef = pi.d.e;
    float v = pi.v;
    if (pi.d.valid) {
        if (S > 0) ef = vg_atrous(x, y, W, H, S, pi, vg_prefilter(x, y, W, H, lds), sl, in_, ia, lds, &v);
        else ef = vg_atrous(x, y, W, H, s, pi, vg_prefilter(x, y, W, H, l2), sl, in_, ia, l2, &v);
    }
    if (FINISH) {
        f3 c; float4 px;
        const dn_pix p0 = dn_prepare_at(fr, i, &c, &px);
        dn_store(fr, out6, i, px, p0, c, ef, blend, !pi.d.valid, p);    // valid but not guided: c itself
    } else {
        wk.e[src ^ 1][i] = make_float4(ef.x, ef.y, ef.z, v);
    }
}

template <bool FINISH>
static void launch_vg_pass(hipStream_t st, dim3 grid, dim3 blk, const Frame &fr, const DnWork &wk, int src, int W, int H, int s, float sl, float in_,
                           float ia, float *out6, float blend, const flx_render_params &p)
{
    if (s == 1) hipLaunchKernelGGL((k_vg_pass<1, FINISH>), grid, blk, 0, st, fr, wk, src, W, H, s, sl, in_, ia, out6, blend, p);
    else if (s == 2) hipLaunchKernelGGL((k_vg_pass<2, FINISH>), grid, blk, 0, st, fr, wk, src, W, H, s, sl, in_, ia, out6, blend, p);
    else hipLaunchKernelGGL((k_vg_pass<0, FINISH>), grid, blk, 0, st, fr, wk, src, W, H, s, sl, in_, ia, out6, blend, p);
}

// the whole call: W * H == fr.localPixels (unpartitioned context), fr.moments set, blend already clamped
void launch_denoise_vg(hipStream_t st, const Frame &fr, float4 *e0, float4 *e1, float4 *g, float2 *g2, float *out6, int W, int H, int iterations,
                       float sigma_l, float sigma_n, float sigma_a, float blend, const flx_render_params &p)
{
    const dim3 blk(DN_BX, DN_BY), grid((W + DN_BX - 1) / DN_BX, (H + DN_BY - 1) / DN_BY);
    if (dn_identity(blend, iterations)) {
        hipLaunchKernelGGL(k_dn_identity, grid, blk, 0, st, fr, out6, W, H, p);
        return;
    }
    DnWork wk; wk.e[0] = e0; wk.e[1] = e1; wk.g = g; wk.g2 = g2;
    const float in_ = dn_inv_sq(sigma_n), ia = dn_inv_sq(sigma_a);
    hipLaunchKernelGGL(k_vg_prepare, grid, blk, 0, st, fr, wk, W, H, in_, ia);
    for (int k = 0; k < iterations; k++) {
        if (k + 1 == iterations) launch_vg_pass<true>(st, grid, blk, fr, wk, k & 1, W, H, 1 << k, sigma_l, in_, ia, out6, blend, p);
        else launch_vg_pass<false>(st, grid, blk, fr, wk, k & 1, W, H, 1 << k, sigma_l, in_, ia, out6, blend, p);
    }
}

} // namespace flxd
