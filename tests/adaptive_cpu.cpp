// adaptive_cpu.cpp -- the CPU counterpart of flx_mk_adaptive_update (fluctus_amd/csrc/adaptive.hip): the same per-pixel function of
// fluctus_amd/csrc/flx_adaptive.h over the whole image and the ascending list of the active pixels.  Built by the tests with
// g++ -O2 -ffp-contract=off; its flags, list and count must equal the device's bit for bit.
//
//   adaptive_cpu <in> <out>
//     in:  int32 W, H; float32 threshold; uint32 min_samples, max_samples; float32 lum_floor; uint32 dilate; float32 moments[W*H*4]
//     out: uint8 flags[W*H] (bit 0 own, 1 active, 2 done, 3 converged); float32 r[W*H] (the relative standard error, FLT_MAX where it does
//          not exist); uint32 count; uint32 list[count]
#include "../fluctus_amd/csrc/flx_adaptive.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace flx;

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: adaptive_cpu <in> <out>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t wh[2]; ad_params ap;
    if (fread(wh, 4, 2, f) != 2 || fread(&ap.threshold, 4, 1, f) != 1 || fread(&ap.min_samples, 4, 1, f) != 1 || fread(&ap.max_samples, 4, 1, f) != 1 ||
        fread(&ap.lum_floor, 4, 1, f) != 1 || fread(&ap.dilate, 4, 1, f) != 1 || wh[0] <= 0 || wh[1] <= 0) { fprintf(stderr, "bad header\n"); return 2; }
    if (!ad_params_ok(ap)) { fprintf(stderr, "bad parameters\n"); return 2; }
    const int W = wh[0], H = wh[1];
    const size_t N = (size_t)W * H;
    std::vector<float> mom(N * 4);
    if (fread(mom.data(), 4, N * 4, f) != N * 4) { fprintf(stderr, "short input\n"); return 2; }
    fclose(f);
    auto at = [&](uint32_t j) { ad4 m; m.x = mom[4 * (size_t)j]; m.y = mom[4 * (size_t)j + 1]; m.z = mom[4 * (size_t)j + 2]; m.w = mom[4 * (size_t)j + 3]; return m; };
    std::vector<uint8_t> flags(N);
    std::vector<float> r(N);
    std::vector<uint32_t> list;
    for (size_t i = 0; i < N; i++) {
        const uint32_t fl = ad_pixel((int)(i % (size_t)W), (int)(i / (size_t)W), W, H, ap, at);
        flags[i] = (uint8_t)fl;
        ad_rel_error(at((uint32_t)i), ap.lum_floor, &r[i]);
        if (fl & FLX_AD_ACTIVE) list.push_back((uint32_t)i);
    }
    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    const uint32_t count = (uint32_t)list.size();
    fwrite(flags.data(), 1, N, o); fwrite(r.data(), 4, N, o); fwrite(&count, 4, 1, o); fwrite(list.data(), 4, list.size(), o);
    fclose(o);
    return 0;
}
