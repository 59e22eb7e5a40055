// denoise.hip -- flx_denoise and flx_denoise_variance_guided: the a-trous denoisers of csrc/flx_denoise.h (guided) and
// csrc/flx_denoise_vg.h (variance-guided) on the device.  One pipeline; a filter is a policy type (DnGuided, DnVg) that
// supplies its pixel, its prepare step, its per-pass parameter and what the pixel carries in e.w.  The pass is the headers' dn_prefilter and
// dn_atrous, overloaded on the pixel; the kernel calls them directly (a member that forwards to them costs VGPRs: DESIGN.md 4.3.2).
//
// Pipeline per call: k_dn_prepare<F> (resolve the guides, demodulate, pack the working set once), K a-trous passes k_dn_pass<F, S, FINISH>
// over two ping-pong buffers, the last one fused with the finish step (remodulate, blend, which = 6, the post-processed preview).  blend == 1
// or K == 0 runs k_dn_identity alone.  Every pixel value comes from the headers' functions in the headers' order, so the results equal
// tests/denoise_cpu.cpp bit for bit.
//
// Layout: 16 x 16 workgroups over the image.  The passes of step 1 and 2 stage their tile plus a halo of 2 s pixels in LDS
// (20^2 / 24^2 records of 40 B: 16 / 23 KB); the wider steps, whose halo would outweigh the tile, gather from L2.  The working set is
// SoA: e = float4 (demodulated radiance, w), g = float4 (normal, a'.x), g2 = float2 (a'.y, a'.z) -- the guides are packed once and read by
// every pass.  e.w >= 0: a valid pixel (the variance-guided filter keeps the pixel's variance there, the guided filter 0); -1: invalid.
// So the variance costs no extra record, and the variance-guided prefilter's distance-1 taps lie inside the halo of steps 1 / 2.
#include "flx_device.h"
#include "flx_denoise.h"
#include "flx_denoise_vg.h"
#include "flx_launch.h"

namespace flxd {

#define DN_BX 16
#define DN_BY 16

struct DnWork {
    float4 *e[2];       // ping-pong demodulated radiance (w: >= 0 valid / -1 invalid)
    float4 *g;          // normal.xyz, a'.x
    float2 *g2;         // a'.y, a'.z
};

// a working-set record as a dn_pix (the variance-guided filter adds e.w as the variance)
__device__ __forceinline__ dn_pix dn_unpack(float4 e, float4 g, float2 g2)
{
    dn_pix p;
    p.e = mk3(e.x, e.y, e.z); p.valid = e.w >= 0.0f;
    p.n = mk3(g.x, g.y, g.z); p.a = mk3(g.w, g2.x, g2.y);
    return p;
}

// pixel i of the raw buffers through the prepare step of filter F: colour c, raw accumulation px
template <class F>
__device__ __forceinline__ dn_pix prepare_at(const Frame &fr, uint32_t i, f3 *c, float4 *px)
{
    *px = reinterpret_cast<const float4 *>(fr.pixels)[i];
    const float4 a = reinterpret_cast<const float4 *>(fr.aovAlbedo)[i], n = reinterpret_cast<const float4 *>(fr.aovNormal)[i];
    return F::prep(&px->x, &a.x, &n.x, c);
}

// The guided filter (flx_denoise.h).  Per-pass parameter: ic_k.
struct DnGuided {
    using Pix = dn_pix;
    __device__ __forceinline__ static dn_pix prep(const float px[4], const float a[4], const float n[4], f3 *c) { return dn_prepare(px, a, n, c); }
    __device__ __forceinline__ static dn_pix unpack(float4 e, float4 g, float2 g2) { return dn_unpack(e, g, g2); }
    static float param(float sigma_c, int k) { return dn_inv_sq_color(sigma_c, k); }
    __device__ __forceinline__ static float w(const dn_pix &p) { return p.valid ? 0.0f : -1.0f; }
    // the working-set pixel (x, y); *w its e.w
    __device__ __forceinline__ static dn_pix prepare(const Frame &fr, int x, int y, int W, int, float, float, float *w)
    {
        f3 c; float4 px;
        const dn_pix p = prepare_at<DnGuided>(fr, (uint32_t)y * W + x, &c, &px);
        *w = p.valid ? 0.0f : -1.0f;
        return p;
    }
};

// The variance-guided filter (flx_denoise_vg.h).  Per-pass parameter: sigma_l.  Valid means guided.
struct DnVg {
    using Pix = vg_pix;
    __device__ __forceinline__ static dn_pix prep(const float px[4], const float a[4], const float n[4], f3 *c) { return vg_prepare(px, a, n, c); }
    __device__ __forceinline__ static vg_pix unpack(float4 e, float4 g, float2 g2)
    {
        vg_pix p;
        p.d = dn_unpack(e, g, g2); p.v = e.w;
        return p;
    }
    static float param(float sigma_l, int) { return sigma_l; }
    __device__ __forceinline__ static float w(const vg_pix &p) { return p.v; }
    // the working-set pixel (x, y); *w its initial variance, or -1.  The fallback re-prepares the 3 x 3 neighbours from the raw buffers.
    __device__ __forceinline__ static dn_pix prepare(const Frame &fr, int x, int y, int W, int H, float in_, float ia, float *w)
    {
        const uint32_t i = (uint32_t)y * W + x;
        f3 c; float4 px;
        const dn_pix p = prepare_at<DnVg>(fr, i, &c, &px);
        *w = -1.0f;
        if (p.valid) {
            const float4 m = reinterpret_cast<const float4 *>(fr.moments)[i];
            *w = vg_initial_variance(x, y, W, H, p, &m.x, in_, ia,
                                     [&](int xj, int yj) { f3 cj; float4 pxj; return prepare_at<DnVg>(fr, (uint32_t)yj * W + xj, &cj, &pxj); });
        }
        return p;
    }
};

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

template <class F>
__global__ __launch_bounds__(DN_BX * DN_BY) void k_dn_prepare(Frame fr, DnWork wk, int W, int H, float in_, float ia)
{
    const int x = blockIdx.x * DN_BX + threadIdx.x, y = blockIdx.y * DN_BY + threadIdx.y;
    if (x >= W || y >= H) return;
    const uint32_t i = (uint32_t)y * W + x;
    float w;
    const dn_pix p = F::prepare(fr, x, y, W, H, in_, ia, &w);
    wk.e[0][i] = make_float4(p.e.x, p.e.y, p.e.z, w);
    wk.g[i] = make_float4(p.n.x, p.n.y, p.n.z, p.a.x);
    wk.g2[i] = make_float2(p.a.y, p.a.z);
}

__global__ __launch_bounds__(DN_BX * DN_BY) void k_dn_identity(Frame fr, float *out6, int W, int H, flx_render_params p)
{
    const int x = blockIdx.x * DN_BX + threadIdx.x, y = blockIdx.y * DN_BY + threadIdx.y;
    if (x >= W || y >= H) return;
    const uint32_t i = (uint32_t)y * W + x;
    f3 c; float4 px;
    const dn_pix pi = prepare_at<DnGuided>(fr, i, &c, &px);
    dn_store(fr, out6, i, px, pi, c, mk3(0.0f), 1.0f, true, p);
}

// one a-trous pass of filter F with per-pass parameter fp.  S = 1 or 2: the step, tile + halo in LDS; S = 0: step `s`, taps gathered from
// global memory (L2).  FINISH: the last pass -- writes which = 6 and the preview instead of the next working set.
template <class F, int S, bool FINISH>
__global__ __launch_bounds__(DN_BX * DN_BY) void k_dn_pass(Frame fr, DnWork wk, int src, int W, int H, int s, float fp, float in_, float ia,
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
                le[t] = make_float4(0.0f, 0.0f, 0.0f, -1.0f);    // never read: the filters skip taps outside the image
            }
        }
        __syncthreads();
    }
    if (x >= W || y >= H) return;
    const uint32_t i = (uint32_t)y * W + x;
    auto lds = [&](int xj, int yj) { const int t = (yj - oy) * TW + (xj - ox); return F::unpack(le[t], lg[t], lg2[t]); };
    auto l2 = [&](int xj, int yj) { const uint32_t j = (uint32_t)yj * W + xj; return F::unpack(E[j], wk.g[j], wk.g2[j]); };
    const typename F::Pix pi = S > 0 ? lds(x, y) : l2(x, y);
    const bool valid = dn_part(pi).valid;
    f3 ef = dn_part(pi).e;
    float w = F::w(pi);
    if (valid) {
        if (S > 0) ef = dn_atrous(x, y, W, H, S, pi, dn_prefilter(x, y, W, H, pi, lds), fp, in_, ia, lds, &w);
        else ef = dn_atrous(x, y, W, H, s, pi, dn_prefilter(x, y, W, H, pi, l2), fp, in_, ia, l2, &w);
    }
    if (FINISH) {
        f3 c; float4 px;
        const dn_pix p0 = prepare_at<DnGuided>(fr, i, &c, &px);     // the centre as dn_prepare sees it: colour, floored albedo, validity
        dn_store(fr, out6, i, px, p0, c, ef, blend, !valid, p);     // a valid pixel the filter does not take (not guided): c itself
    } else {
        wk.e[src ^ 1][i] = make_float4(ef.x, ef.y, ef.z, w);
    }
}

template <class F, bool FINISH>
static void launch_pass(hipStream_t st, dim3 grid, dim3 blk, const Frame &fr, const DnWork &wk, int src, int W, int H, int s, float fp, float in_,
                        float ia, float *out6, float blend, const flx_render_params &p)
{
    if (s == 1) hipLaunchKernelGGL((k_dn_pass<F, 1, FINISH>), grid, blk, 0, st, fr, wk, src, W, H, s, fp, in_, ia, out6, blend, p);
    else if (s == 2) hipLaunchKernelGGL((k_dn_pass<F, 2, FINISH>), grid, blk, 0, st, fr, wk, src, W, H, s, fp, in_, ia, out6, blend, p);
    else hipLaunchKernelGGL((k_dn_pass<F, 0, FINISH>), grid, blk, 0, st, fr, wk, src, W, H, s, fp, in_, ia, out6, blend, p);
}

// the whole call: W * H == fr.localPixels (unpartitioned context), blend already clamped, fr.moments set for DnVg.  sigma: sigma_c (DnGuided)
// or sigma_l (DnVg)
template <class F>
void launch_denoise(hipStream_t st, const Frame &fr, float4 *e0, float4 *e1, float4 *g, float2 *g2, float *out6, int W, int H, int iterations,
                    float sigma, float sigma_n, float sigma_a, float blend, const flx_render_params &p)
{
    const dim3 blk(DN_BX, DN_BY), grid((W + DN_BX - 1) / DN_BX, (H + DN_BY - 1) / DN_BY);
    if (dn_identity(blend, iterations)) {
        hipLaunchKernelGGL(k_dn_identity, grid, blk, 0, st, fr, out6, W, H, p);
        return;
    }
    DnWork wk; wk.e[0] = e0; wk.e[1] = e1; wk.g = g; wk.g2 = g2;
    const float in_ = dn_inv_sq(sigma_n), ia = dn_inv_sq(sigma_a);
    hipLaunchKernelGGL(k_dn_prepare<F>, grid, blk, 0, st, fr, wk, W, H, in_, ia);
    for (int k = 0; k < iterations; k++) {
        const float fp = F::param(sigma, k);
        if (k + 1 == iterations) launch_pass<F, true>(st, grid, blk, fr, wk, k & 1, W, H, 1 << k, fp, in_, ia, out6, blend, p);
        else launch_pass<F, false>(st, grid, blk, fr, wk, k & 1, W, H, 1 << k, fp, in_, ia, out6, blend, p);
    }
}

template void launch_denoise<DnGuided>(hipStream_t, const Frame &, float4 *, float4 *, float4 *, float2 *, float *, int, int, int, float, float,
                                       float, float, const flx_render_params &);
template void launch_denoise<DnVg>(hipStream_t, const Frame &, float4 *, float4 *, float4 *, float2 *, float *, int, int, int, float, float, float,
                                   float, const flx_render_params &);

} // namespace flxd
