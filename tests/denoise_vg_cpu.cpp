// denoise_vg_cpu.cpp -- the CPU counterpart of flx_denoise_variance_guided (fluctus_amd/csrc/denoise.hip): the same per-pixel functions of
// fluctus_amd/csrc/flx_denoise_vg.h, run pass by pass over the whole image.  Built by the tests with g++ -O2 -ffp-contract=off; its output
// must equal the device's bit for bit.
//
//   denoise_vg_cpu <in> <out>
//   in:  int32 W, H, iterations; float32 sigma_luminance, sigma_normal, sigma_albedo, blend, exposure; uint32 tmOperator;
//        float32 pixels[W*H*4] (which = 0), albedo[W*H*4] (which = 4), normal[W*H*4] (which = 5), moments[W*H*4] (which = 7)
//   out: float32 denoised[W*H*4] (which = 6), preview[W*H*4] (which = 1), initial variance[W*H] (-1 = invalid pixel)
#include "../fluctus_amd/csrc/flx_denoise_vg.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace flx;

static bool readAll(FILE *f, void *p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: denoise_vg_cpu <in> <out>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t hdr[3]; float sig[5]; uint32_t tm;
    if (!readAll(f, hdr, 12) || !readAll(f, sig, 20) || !readAll(f, &tm, 4)) { fprintf(stderr, "short header\n"); return 2; }
    const int W = hdr[0], H = hdr[1], K = hdr[2];
    if (W <= 0 || H <= 0 || K < 0 || K > FLX_DN_MAX_ITERATIONS) { fprintf(stderr, "bad header\n"); return 2; }
    const size_t N = (size_t)W * H;
    std::vector<float> px(N * 4), alb(N * 4), nrm(N * 4), mom(N * 4);
    if (!readAll(f, px.data(), N * 16) || !readAll(f, alb.data(), N * 16) || !readAll(f, nrm.data(), N * 16) || !readAll(f, mom.data(), N * 16)) {
        fprintf(stderr, "short input\n"); return 2;
    }
    fclose(f);

    const float blend = dn_blend(sig[3]);
    const bool identity = dn_identity(blend, K);
    const float in_ = dn_inv_sq(sig[1]), ia = dn_inv_sq(sig[2]);
    std::vector<dn_pix> prep(N);
    std::vector<f3> col(N);
    std::vector<dn_pix> prep0(N);                                    // dn_prepare: the finish step's view (valid, colour, a')
    for (size_t i = 0; i < N; i++) {
        prep0[i] = dn_prepare(&px[i * 4], &alb[i * 4], &nrm[i * 4], &col[i]);
        prep[i] = vg_prepare(&px[i * 4], &alb[i * 4], &nrm[i * 4], &col[i]);
    }
    std::vector<vg_pix> cur(N), nxt(N);
    std::vector<float> var0(N);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t i = (size_t)y * W + x;
            cur[i].d = prep[i];
            cur[i].v = prep[i].valid ? vg_initial_variance(x, y, W, H, prep[i], &mom[i * 4], in_, ia, [&](int xj, int yj) { return prep[(size_t)yj * W + xj]; })
                                     : -1.0f;
            var0[i] = cur[i].v;
        }
    if (!identity) {
        for (int k = 0; k < K; k++) {
            auto fetch = [&](int xj, int yj) { return cur[(size_t)yj * W + xj]; };
            for (int y = 0; y < H; y++)
                for (int x = 0; x < W; x++) {
                    const size_t i = (size_t)y * W + x;
                    nxt[i] = cur[i];
                    if (!cur[i].d.valid) continue;
                    const float gv = vg_prefilter(x, y, W, H, fetch);
                    nxt[i].d.e = vg_atrous(x, y, W, H, 1 << k, cur[i], gv, sig[0], in_, ia, fetch, &nxt[i].v);
                }
            cur.swap(nxt);
        }
    }
    std::vector<float> out(N * 4), prev(N * 4);
    for (size_t i = 0; i < N; i++) {
        dn_finish(&px[i * 4], prep0[i], col[i], cur[i].d.e, blend, identity || !prep[i].valid, &out[i * 4]);
        postprocess_px(&out[i * 4], sig[4], tm, &prev[i * 4]);
    }
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    if (fwrite(out.data(), 1, N * 16, f) != N * 16 || fwrite(prev.data(), 1, N * 16, f) != N * 16 || fwrite(var0.data(), 1, N * 4, f) != N * 4) {
        fprintf(stderr, "short write\n"); return 2;
    }
    fclose(f);
    return 0;
}
