// reproject_motion_cpu.cpp -- the CPU counterpart of flx_reproject with option "motion_history" (fluctus_amd/csrc/reproject.hip:
// k_reproject_motion): the per-pixel function of fluctus_amd/csrc/flx_reproject_motion.h over the whole image, and the header's per-object
// table function.  Built by the tests with g++ -O2 -ffp-contract=off; its output must equal the device's bit for bit.
//
//   reproject_motion_cpu reproject <in> <out>
//     in:  int32 W, H, moments, nobjects; float32 max_history, plane_tolerance_px, normal_cos, min_weight; float32 prevCamera[20] (the 80-byte
//          flx_camera); float32 fovCur; float32 curG[W*H*8], prevG[W*H*8], hist[W*H*4][, histMom[W*H*4]: moments]; uint32 curObj[W*H],
//          prevObj[W*H]; float32 table[nobjects*16] (rm_make_table's rows)
//     out: float32 pixels[W*H*4], moments[W*H*4] (zeros without moments); int32 tap[W*H*4] (previous-view pixel of each counted tap, -1: not
//          counted); float32 weight[W*H*4] (the taps' bilinear weights before renormalisation)
//   reproject_motion_cpu table <in> <out>
//     in:  int32 nobjects; float32 Xcap[nobjects*12]; int32 knownCap[nobjects]; float32 Xnow[nobjects*12]; int32 knownNow[nobjects]
//     out: float32 table[nobjects*16]; int32 any
#include "../fluctus_amd/csrc/flx_reproject_motion.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <string>

using namespace flx;

static bool readAll(FILE *f, void *p, size_t n) { return fread(p, 1, n, f) == n; }
struct Cam { f3 pos, dir, up, right; float fov; };
static Cam cam20(const float *c) { return Cam{mk3(c[0], c[1], c[2]), mk3(c[4], c[5], c[6]), mk3(c[8], c[9], c[10]), mk3(c[12], c[13], c[14]), c[16]}; }

static int table(FILE *f, const char *outPath)
{
    int32_t n;
    if (!readAll(f, &n, 4) || n < 0) { fprintf(stderr, "bad header\n"); return 2; }
    std::vector<float> xc((size_t)n * 12), xn((size_t)n * 12);
    std::vector<int32_t> kc(n), kn(n);
    if (!readAll(f, xc.data(), xc.size() * 4) || !readAll(f, kc.data(), kc.size() * 4) || !readAll(f, xn.data(), xn.size() * 4) || !readAll(f, kn.data(), kn.size() * 4)) {
        fprintf(stderr, "short input\n"); return 2;
    }
    std::vector<uint8_t> bc(n), bn(n);
    for (int32_t i = 0; i < n; i++) { bc[i] = kc[i] != 0; bn[i] = kn[i] != 0; }
    std::vector<rm_row> rows((size_t)n * FLX_RM_ROWS);
    const int32_t any = rm_make_table((uint32_t)n, xc.data(), bc.data(), xn.data(), bn.data(), rows.data()) ? 1 : 0;
    FILE *o = fopen(outPath, "wb");
    if (!o) { perror(outPath); return 2; }
    fwrite(rows.data(), sizeof(rm_row), rows.size(), o); fwrite(&any, 4, 1, o);
    fclose(o);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: reproject_motion_cpu reproject|table <in> <out>\n"); return 2; }
    const std::string mode = argv[1];
    FILE *f = fopen(argv[2], "rb");
    if (!f) { perror(argv[2]); return 2; }
    if (mode == "table") { const int r = table(f, argv[3]); fclose(f); return r; }
    if (mode != "reproject") { fprintf(stderr, "unknown mode\n"); return 2; }
    int32_t hdr[4];
    float par[4], cam[20], fovCur;
    if (!readAll(f, hdr, 16) || !readAll(f, par, 16) || !readAll(f, cam, 80) || !readAll(f, &fovCur, 4) || hdr[0] <= 0 || hdr[1] <= 0 || hdr[3] < 0) { fprintf(stderr, "bad header\n"); return 2; }
    const int W = hdr[0], H = hdr[1];
    const bool moments = hdr[2] != 0;
    const uint32_t nobjects = (uint32_t)hdr[3];
    const size_t N = (size_t)W * H;
    std::vector<float> cur(N * 8), prev(N * 8), hist(N * 4), hmom(moments ? N * 4 : 0), tab((size_t)nobjects * 16);
    std::vector<uint32_t> curObj(N), prevObj(N);
    if (!readAll(f, cur.data(), N * 32) || !readAll(f, prev.data(), N * 32) || !readAll(f, hist.data(), N * 16) || !readAll(f, hmom.data(), hmom.size() * 4) ||
        !readAll(f, curObj.data(), N * 4) || !readAll(f, prevObj.data(), N * 4) || !readAll(f, tab.data(), tab.size() * 4)) {
        fprintf(stderr, "short input\n"); return 2;
    }
    fclose(f);
    const rp_params rp = {par[0], par[1], par[2], par[3]};
    if (!rp_params_ok(rp)) { fprintf(stderr, "bad parameters\n"); return 2; }
    const Cam pc = cam20(cam);
    const rp_view vw = rp_make_view(pc.pos, pc.dir, pc.up, pc.right, pc.fov, fovCur, W, H);
    auto at4 = [](const std::vector<float> &v, size_t i) { return mk_rp4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]); };
    auto row = [&](uint32_t o, int r) { return at4(tab, (size_t)o * FLX_RM_ROWS + r); };
    std::vector<float> px(N * 4), mom(N * 4, 0.0f), wt(N * 4, 0.0f);
    std::vector<int32_t> tap(N * 4, -1);
    for (size_t i = 0; i < N; i++) {
        rp4 o, om;
        const uint32_t mask = rm_pixel(vw, rp, at4(cur, 2 * i), at4(cur, 2 * i + 1), curObj[i], nobjects, moments,
                                       [&](uint32_t j) { return at4(prev, 2 * (size_t)j); }, [&](uint32_t j) { return at4(prev, 2 * (size_t)j + 1); },
                                       [&](uint32_t j) { return at4(hist, j); }, [&](uint32_t j) { return at4(hmom, j); },
                                       [&](uint32_t j) { return prevObj[j]; }, row, &o, &om);
        px[4 * i] = o.x; px[4 * i + 1] = o.y; px[4 * i + 2] = o.z; px[4 * i + 3] = o.w;
        mom[4 * i] = om.x; mom[4 * i + 1] = om.y; mom[4 * i + 2] = om.z; mom[4 * i + 3] = om.w;
        if (mask) {     // the taps again, for the tests' agreement check: rm_pixel's own source record and rp_pixel's projection of it
            rp4 g0 = at4(cur, 2 * i), g1 = at4(cur, 2 * i + 1);
            rm_source(rm_object_id(curObj[i], nobjects), row, &g0, &g1);
            float xf, yf;
            rp_project(vw, mk3(g0.x, g0.y, g0.z), &xf, &yf);
            const float fx0 = floorf(xf), fy0 = floorf(yf), fx = xf - fx0, fy = yf - fy0;
            for (int k = 0; k < 4; k++)
                if (mask & (1u << k)) {
                    tap[4 * i + k] = ((int)fy0 + (k >> 1)) * W + (int)fx0 + (k & 1);
                    wt[4 * i + k] = ((k & 1) ? fx : 1.0f - fx) * ((k >> 1) ? fy : 1.0f - fy);
                }
        }
    }
    FILE *o = fopen(argv[3], "wb");
    if (!o) { perror(argv[3]); return 2; }
    fwrite(px.data(), 4, px.size(), o); fwrite(mom.data(), 4, mom.size(), o); fwrite(tap.data(), 4, tap.size(), o); fwrite(wt.data(), 4, wt.size(), o);
    fclose(o);
    return 0;
}
