// denoise_cpu.cpp -- the CPU counterpart of flx_denoise and flx_denoise_variance_guided (fluctus_amd/csrc/denoise.hip): the same per-pixel
// functions of fluctus_amd/csrc/flx_denoise.h and flx_denoise_vg.h, run pass by pass over the whole image.  Built by the tests with
// g++ -O2 -ffp-contract=off; its output must equal the device's bit for bit.
//
//   denoise_cpu <in> <out>
//   in:  int32 W, H, iterations, filter (0: guided, 1: variance-guided); float32 sigma (sigma_color / sigma_luminance), sigma_normal,
//        sigma_albedo, blend, exposure; uint32 tmOperator;
//        float32 pixels[W*H*4] (which = 0), albedo[W*H*4] (which = 4), normal[W*H*4] (which = 5)[, moments[W*H*4] (which = 7): filter 1]
//   out: float32 denoised[W*H*4] (which = 6), preview[W*H*4] (which = 1)[, initial variance[W*H] (-1 = invalid pixel): filter 1]
#include "../fluctus_amd/csrc/flx_denoise_vg.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace flx;

static bool readAll(FILE *f, void *p, size_t n) { return fread(p, 1, n, f) == n; }

// where a pass leaves what the pixel carries beside e: the variance of a vg_pix, nothing for a dn_pix
static float *carried(dn_pix &) { return nullptr; }
static float *carried(vg_pix &p) { return &p.v; }

// K passes over the image from the working set cur; param(k) the per-pass parameter of pass k.  Invalid pixels stay as they are.
template <class Pix, class Param>
static std::vector<Pix> passes(int W, int H, int K, std::vector<Pix> cur, Param param, float in_, float ia)
{
    std::vector<Pix> nxt(cur.size());
    for (int k = 0; k < K; k++) {
        const float p = param(k);
        auto fetch = [&](int xj, int yj) { return cur[(size_t)yj * W + xj]; };
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                const size_t i = (size_t)y * W + x;
                nxt[i] = cur[i];
                if (dn_part(cur[i]).valid)
                    dn_part(nxt[i]).e = dn_atrous(x, y, W, H, 1 << k, cur[i], dn_prefilter(x, y, W, H, cur[i], fetch), p, in_, ia, fetch, carried(nxt[i]));
            }
        cur.swap(nxt);
    }
    return cur;
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: denoise_cpu <in> <out>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t hdr[4]; float sig[5]; uint32_t tm;
    if (!readAll(f, hdr, 16) || !readAll(f, sig, 20) || !readAll(f, &tm, 4)) { fprintf(stderr, "short header\n"); return 2; }
    const int W = hdr[0], H = hdr[1], K = hdr[2];
    const bool vg = hdr[3] == 1;
    if (W <= 0 || H <= 0 || K < 0 || K > FLX_DN_MAX_ITERATIONS || (hdr[3] != 0 && hdr[3] != 1)) { fprintf(stderr, "bad header\n"); return 2; }
    const size_t N = (size_t)W * H;
    std::vector<float> px(N * 4), alb(N * 4), nrm(N * 4), mom(vg ? N * 4 : 0);
    if (!readAll(f, px.data(), N * 16) || !readAll(f, alb.data(), N * 16) || !readAll(f, nrm.data(), N * 16) || !readAll(f, mom.data(), mom.size() * 4)) {
        fprintf(stderr, "short input\n"); return 2;
    }
    fclose(f);

    const float blend = dn_blend(sig[3]);
    const bool identity = dn_identity(blend, K);
    const float in_ = dn_inv_sq(sig[1]), ia = dn_inv_sq(sig[2]);
    const int passK = identity ? 0 : K;
    std::vector<dn_pix> prep(N);                                     // dn_prepare: the finish step's view (valid, colour, a')
    std::vector<f3> col(N), ef(N);
    std::vector<bool> filtered(N);                                   // valid for the filter (variance-guided: guided)
    std::vector<float> var0;
    for (size_t i = 0; i < N; i++) prep[i] = dn_prepare(&px[i * 4], &alb[i * 4], &nrm[i * 4], &col[i]);
    if (vg) {
        std::vector<vg_pix> cur(N);
        for (size_t i = 0; i < N; i++) cur[i].d = vg_prepare(&px[i * 4], &alb[i * 4], &nrm[i * 4], &col[i]);
        var0.resize(N);
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                const size_t i = (size_t)y * W + x;
                cur[i].v = cur[i].d.valid ? vg_initial_variance(x, y, W, H, cur[i].d, &mom[i * 4], in_, ia, [&](int xj, int yj) { return cur[(size_t)yj * W + xj].d; })
                                          : -1.0f;
                var0[i] = cur[i].v;
            }
        cur = passes(W, H, passK, cur, [&](int) { return sig[0]; }, in_, ia);
        for (size_t i = 0; i < N; i++) { ef[i] = cur[i].d.e; filtered[i] = cur[i].d.valid; }
    } else {
        const std::vector<dn_pix> cur = passes(W, H, passK, prep, [&](int k) { return dn_inv_sq_color(sig[0], k); }, in_, ia);
        for (size_t i = 0; i < N; i++) { ef[i] = cur[i].e; filtered[i] = cur[i].valid; }
    }
    std::vector<float> out(N * 4), prev(N * 4);
    for (size_t i = 0; i < N; i++) {
        dn_finish(&px[i * 4], prep[i], col[i], ef[i], blend, identity || !filtered[i], &out[i * 4]);
        postprocess_px(&out[i * 4], sig[4], tm, &prev[i * 4]);
    }
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    if (fwrite(out.data(), 1, N * 16, f) != N * 16 || fwrite(prev.data(), 1, N * 16, f) != N * 16 || fwrite(var0.data(), 1, var0.size() * 4, f) != var0.size() * 4) {
        fprintf(stderr, "short write\n"); return 2;
    }
    fclose(f);
    return 0;
}
