// reproject_deform_cpu.cpp -- the CPU counterpart of flx_reproject with option "deform_history" (fluctus_amd/csrc/reproject.hip: k_moved_flags,
// k_reproject_deform): the moved test of fluctus_amd/csrc/flx_reproject_deform.h over every triangle, then the header's per-pixel function over
// the whole image.  Built by the tests with g++ -O2 -ffp-contract=off; its output must equal the device's bit for bit.
//
//   reproject_deform_cpu <in> <out>
//     in:  int32 W, H, moments, ntris; float32 max_history, plane_tolerance_px, normal_cos, min_weight; float32 prevCamera[20] (the 80-byte
//          flx_camera); float32 fovCur; float32 curG[W*H*8], prevG[W*H*8], hist[W*H*4][, histMom[W*H*4]: moments]; float32 curBary[W*H*2],
//          prevBary[W*H*2]; float32 now[ntris*9], cap[ntris*9] (three positions per triangle: now, at the capture)
//     out: float32 pixels[W*H*4], moments[W*H*4] (zeros without moments); int32 tap[W*H*4] (previous-view pixel of each counted tap, -1: not
//          counted); float32 weight[W*H*4] (the taps' bilinear weights before renormalisation); int32 moved[ntris]
#include "../fluctus_amd/csrc/flx_reproject_deform.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace flx;

static bool readAll(FILE *f, void *p, size_t n) { return fread(p, 1, n, f) == n; }
struct Cam { f3 pos, dir, up, right; float fov; };
static Cam cam20(const float *c) { return Cam{mk3(c[0], c[1], c[2]), mk3(c[4], c[5], c[6]), mk3(c[8], c[9], c[10]), mk3(c[12], c[13], c[14]), c[16]}; }

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: reproject_deform_cpu <in> <out>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t hdr[4];
    float par[4], cam[20], fovCur;
    if (!readAll(f, hdr, 16) || !readAll(f, par, 16) || !readAll(f, cam, 80) || !readAll(f, &fovCur, 4) || hdr[0] <= 0 || hdr[1] <= 0 || hdr[3] < 0) { fprintf(stderr, "bad header\n"); return 2; }
    const int W = hdr[0], H = hdr[1];
    const bool moments = hdr[2] != 0;
    const uint32_t ntris = (uint32_t)hdr[3];
    const size_t N = (size_t)W * H;
    std::vector<float> cur(N * 8), prev(N * 8), hist(N * 4), hmom(moments ? N * 4 : 0), curB(N * 2), prevB(N * 2), now((size_t)ntris * 9), cap((size_t)ntris * 9);
    if (!readAll(f, cur.data(), N * 32) || !readAll(f, prev.data(), N * 32) || !readAll(f, hist.data(), N * 16) || !readAll(f, hmom.data(), hmom.size() * 4) ||
        !readAll(f, curB.data(), N * 8) || !readAll(f, prevB.data(), N * 8) || !readAll(f, now.data(), now.size() * 4) || !readAll(f, cap.data(), cap.size() * 4)) {
        fprintf(stderr, "short input\n"); return 2;
    }
    fclose(f);
    const rp_params rp = {par[0], par[1], par[2], par[3]};
    if (!rp_params_ok(rp)) { fprintf(stderr, "bad parameters\n"); return 2; }
    const Cam pc = cam20(cam);
    const rp_view vw = rp_make_view(pc.pos, pc.dir, pc.up, pc.right, pc.fov, fovCur, W, H);
    auto at4 = [](const std::vector<float> &v, size_t i) { return mk_rp4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]); };
    auto tri = [](const std::vector<float> &v, uint32_t i) {
        const float *p = &v[9 * (size_t)i];
        rd_tri t; t.a = mk3(p[0], p[1], p[2]); t.b = mk3(p[3], p[4], p[5]); t.c = mk3(p[6], p[7], p[8]); return t;
    };
    auto uv = [](const std::vector<float> &v, size_t i) { return rd_uv{v[2 * i], v[2 * i + 1]}; };
    std::vector<int32_t> moved(ntris);
    for (uint32_t i = 0; i < ntris; i++) moved[i] = rd_moved(tri(now, i), tri(cap, i)) ? 1 : 0;            // k_moved_flags
    auto movedOf = [&](uint32_t i) { return moved[i]; };
    std::vector<float> px(N * 4), mom(N * 4, 0.0f), wt(N * 4, 0.0f);
    std::vector<int32_t> tap(N * 4, -1);
    for (size_t i = 0; i < N; i++) {
        rp4 o, om;
        const uint32_t mask = rd_pixel(vw, rp, at4(cur, 2 * i), at4(cur, 2 * i + 1), uv(curB, i), ntris, moments,
                                       [&](uint32_t j) { return at4(prev, 2 * (size_t)j); }, [&](uint32_t j) { return at4(prev, 2 * (size_t)j + 1); },
                                       [&](uint32_t j) { return at4(hist, j); }, [&](uint32_t j) { return at4(hmom, j); },
                                       [&](uint32_t j) { return uv(prevB, j); }, [&](uint32_t t) { return tri(now, t); }, [&](uint32_t t) { return tri(cap, t); },
                                       movedOf, &o, &om);
        px[4 * i] = o.x; px[4 * i + 1] = o.y; px[4 * i + 2] = o.z; px[4 * i + 3] = o.w;
        mom[4 * i] = om.x; mom[4 * i + 1] = om.y; mom[4 * i + 2] = om.z; mom[4 * i + 3] = om.w;
        if (mask) {     // the taps again, for the tests' agreement check: rd_pixel's own source record and rp_pixel's projection of it
            rp4 g0 = at4(cur, 2 * i), g1 = at4(cur, 2 * i + 1);
            if (rd_record_moved(g0, uv(curB, i), ntris, movedOf)) rd_source(uv(curB, i), tri(now, f2u(g0.w)), tri(cap, f2u(g0.w)), &g0, &g1);
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
    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    fwrite(px.data(), 4, px.size(), o); fwrite(mom.data(), 4, mom.size(), o); fwrite(tap.data(), 4, tap.size(), o); fwrite(wt.data(), 4, wt.size(), o);
    fwrite(moved.data(), 4, moved.size(), o);
    fclose(o);
    return 0;
}
