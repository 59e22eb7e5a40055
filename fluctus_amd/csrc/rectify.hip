// rectify.hip -- flx_history_rectify on the device (csrc/flx_rectify.h): two passes over the image, one thread per pixel, no atomics.
//
// k_rectify_prepare: the record (n, a, h, ok) of every pixel from the accumulation, the mark and the current G-buffer's G0; 16 bytes out.
//
// k_rectify_window<MOM>: the hot path.  One 16 x 16 block stages its tile plus an r-pixel halo in LDS as three float4 planes -- the prepare
// record, (P, t) and (N, hit word) of the current G-buffer -- and walks the (2 r + 1)^2 taps of rc_lambda out of them in the header's order.  A halo
// cell outside the image is staged as a record that is not ok, so image edges and tile edges cost no per-tap global read.  The planes' row
// stride is RC_STRIDE = 32 float4 whatever r is (the tile is 18 .. 24 wide): a wave covers four rows of 16 lanes, a ds_read_b128 is served in
// groups of 16 lanes that take lanes from two neighbouring rows of the block (lanes 0-3, 12-15 of one, 4-11 of the next), and with a stride that is
// a multiple of 16 slots of 16 bytes those two part rows land on complementary banks for every tap offset -- a stride of 24 would put them on the
// same ones.  LDS: 3 x 32 x (16 + 2 r) x 16 B = 27 / 33 / 36 KiB at r = 1 / 3 / 4.  Every value comes from rc_lambda / rc_apply in their order, so the
// result equals tests/rectify_cpu.cpp bit for bit.  The pass updates the accumulation and the mark in place: a thread reads A and S of its OWN
// pixel only, its neighbours through the records of the prepare pass.  lambda goes to its plane for every pixel; A, S (and M, SM) are written
// only where lambda > 0, with 16-byte stores.
#include "flx_launch.h"
#include "flx_rectify.h"

namespace flxd {

#define RC_BX 16
#define RC_BY 16
#define RC_STRIDE 32

__device__ __forceinline__ rp4 rc_ld(const float4 *p) { const float4 v = *p; return mk_rp4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ float4 rc_f4(rp4 v) { return make_float4(v.x, v.y, v.z, v.w); }

// px: which = 0 now; mark: the marked copy; cur: the current G-buffer slot (2 float4 per pixel); rec: npix records out
__global__ __launch_bounds__(256) void k_rectify_prepare(const float4 *px, const float4 *mark, const float4 *cur, float4 *rec, uint32_t npix)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= npix) return;
    rec[i] = rc_f4(rc_prepare(rc_ld(px + i), rc_ld(mark + i), rc_ld(cur + 2 * (size_t)i)));
}

template <bool MOM>
__global__ __launch_bounds__(RC_BX * RC_BY) void k_rectify_window(rc_params rc, float footprint, int W, int H, const float4 *cur, const float4 *rec,
                                                                   float4 *px, float4 *mark, float4 *mom, float4 *markMom, float *lambda)
{
    extern __shared__ float4 s_rc[];
    const int r = rc.radius, tw = RC_BX + 2 * r, th = RC_BY + 2 * r;
    float4 *sRec = s_rc, *sP = s_rc + RC_STRIDE * th, *sN = s_rc + 2 * RC_STRIDE * th;
    const int x0 = (int)blockIdx.x * RC_BX - r, y0 = (int)blockIdx.y * RC_BY - r;     // the image pixel of tile cell (0, 0)
    for (int c = (int)(threadIdx.y * RC_BX + threadIdx.x); c < tw * th; c += RC_BX * RC_BY) {
        const int lx = c % tw, ly = c / tw, gx = x0 + lx, gy = y0 + ly;
        float4 q = make_float4(0.0f, 0.0f, 0.0f, 0.0f), p = q, n = q;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const size_t g = (size_t)gy * (size_t)W + (size_t)gx;
            const float4 g0 = cur[2 * g], g1 = cur[2 * g + 1];
            q = rec[g];
            p = make_float4(g0.x, g0.y, g0.z, g1.w);
            n = make_float4(g1.x, g1.y, g1.z, g0.w);
        }
        const int s = ly * RC_STRIDE + lx;
        sRec[s] = q; sP[s] = p; sN[s] = n;
    }
    __syncthreads();
    const int x = (int)blockIdx.x * RC_BX + (int)threadIdx.x, y = (int)blockIdx.y * RC_BY + (int)threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t i = (size_t)y * (size_t)W + (size_t)x;
    const int sc = ((int)threadIdx.y + r) * RC_STRIDE + (int)threadIdx.x + r;
    const float4 cp = sP[sc], cn = sN[sc];
    const rp4 A = rc_ld(px + i), S = rc_ld(mark + i);
    auto at = [&](const float4 *plane, int xq, int yq) { const float4 v = plane[(yq - y0) * RC_STRIDE + (xq - x0)]; return mk_rp4(v.x, v.y, v.z, v.w); };
    uint32_t counted;
    const float lam = rc_lambda(rc, footprint, W, H, x, y, mk_rp4(cp.x, cp.y, cp.z, cn.w), mk_rp4(cn.x, cn.y, cn.z, cp.w), A, S,
                                [&](int xq, int yq) { return at(sRec, xq, yq); }, [&](int xq, int yq) { return at(sP, xq, yq); },
                                [&](int xq, int yq) { return at(sN, xq, yq); }, &counted);
    lambda[i] = lam;
    rp4 a, s;
    if (!rc_apply(lam, A, S, &a, &s)) return;
    px[i] = rc_f4(a); mark[i] = rc_f4(s);
    if (MOM) {
        rc_apply(lam, rc_ld(mom + i), rc_ld(markMom + i), &a, &s);
        mom[i] = rc_f4(a); markMom[i] = rc_f4(s);
    }
}

// the whole call: W x H of an unpartitioned context, rc checked (rc_params_ok: radius <= FLX_RC_MAX_RADIUS bounds the LDS tile); mom and markMom
// both null: the moments are left alone
void launch_rectify(hipStream_t s, const rc_params &rc, float footprint, int W, int H, const float4 *cur, float4 *rec, float4 *px, float4 *mark,
                    float4 *mom, float4 *markMom, float *lambda)
{
    const uint32_t npix = (uint32_t)W * (uint32_t)H;
    hipLaunchKernelGGL(k_rectify_prepare, dim3((npix + 255u) / 256u), dim3(256), 0, s, px, mark, cur, rec, npix);
    const dim3 blk(RC_BX, RC_BY), grid((W + RC_BX - 1) / RC_BX, (H + RC_BY - 1) / RC_BY);
    const size_t lds = (size_t)3 * RC_STRIDE * (RC_BY + 2 * rc.radius) * sizeof(float4);
    if (mom && markMom) hipLaunchKernelGGL(k_rectify_window<true>, grid, blk, lds, s, rc, footprint, W, H, cur, rec, px, mark, mom, markMom, lambda);
    else hipLaunchKernelGGL(k_rectify_window<false>, grid, blk, lds, s, rc, footprint, W, H, cur, rec, px, mark, nullptr, nullptr, lambda);
}

} // namespace flxd
