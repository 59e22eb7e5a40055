// reproject_cpu.cpp -- the CPU counterpart of flx_reproject (fluctus_amd/csrc/reproject.hip): the same per-pixel function of
// fluctus_amd/csrc/flx_reproject.h over the whole image, and the centre rays flx_gbuffer traces.  Built by the tests with
// g++ -O2 -ffp-contract=off; its output must equal the device's bit for bit.
//
//   reproject_cpu reproject <in> <out>
//     in:  int32 W, H, moments; float32 max_history, plane_tolerance_px, normal_cos, min_weight; float32 prevCamera[20] (the 80-byte flx_camera);
//          float32 fovCur; float32 curG[W*H*8], prevG[W*H*8], hist[W*H*4][, histMom[W*H*4]: moments]
//     out: float32 pixels[W*H*4], moments[W*H*4] (zeros without moments); int32 tap[W*H*4] (previous-view pixel of each counted tap, -1: not
//          counted); float32 weight[W*H*4] (the taps' bilinear weights before renormalisation)
//   reproject_cpu rays <in> <out>
//     in:  int32 W, H; float32 camera[20]        out: float32 dir[W*H*3] -- camera_direction (csrc/flx_shading.h) of every pixel with the jitter
//          (0.5, 0.5) and the lens at camera.pos, restated for the host (the device function is __device__ only); the origin is camera.pos
#include "../fluctus_amd/csrc/flx_reproject.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <string>

using namespace flx;

static bool readAll(FILE *f, void *p, size_t n) { return fread(p, 1, n, f) == n; }
struct Cam { f3 pos, dir, up, right; float fov, focalDist; };
static Cam cam20(const float *c) { return Cam{mk3(c[0], c[1], c[2]), mk3(c[4], c[5], c[6]), mk3(c[8], c[9], c[10]), mk3(c[12], c[13], c[14]), c[16], c[18]}; }

static f3 centre_ray(const Cam &c, int W, int H, uint32_t pixelIdx)
{
    float x = (float)(pixelIdx % (uint32_t)W), y = (float)(pixelIdx / (uint32_t)W);
    x += 0.5f; y += 0.5f;
    float SCRx = 2.0f * (x / (float)W) - 1.0f, SCRy = 2.0f * (y / (float)H) - 1.0f;
    SCRx *= (float)W / (float)H;
    const float scale = tanf_(0.5f * c.fov * FLX_PI / 180.0f);
    SCRx *= scale; SCRy *= scale;
    const f3 target = c.pos + c.right * SCRx + c.up * SCRy + c.dir;
    const f3 d = normalize(target - c.pos);
    const f3 fp = c.pos + d * c.focalDist;
    return normalize(fp - c.pos);
}

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: reproject_cpu reproject|rays <in> <out>\n"); return 2; }
    const std::string mode = argv[1];
    FILE *f = fopen(argv[2], "rb");
    if (!f) { perror(argv[2]); return 2; }
    int32_t hdr[3];
    if (mode == "rays") {
        float cam[20];
        if (!readAll(f, hdr, 8) || !readAll(f, cam, 80) || hdr[0] <= 0 || hdr[1] <= 0) { fprintf(stderr, "bad input\n"); return 2; }
        fclose(f);
        const int W = hdr[0], H = hdr[1];
        const Cam c = cam20(cam);
        std::vector<float> out((size_t)W * H * 3);
        for (uint32_t i = 0; i < (uint32_t)(W * H); i++) { const f3 d = centre_ray(c, W, H, i); out[3 * (size_t)i] = d.x; out[3 * (size_t)i + 1] = d.y; out[3 * (size_t)i + 2] = d.z; }
        FILE *o = fopen(argv[3], "wb");
        if (!o || fwrite(out.data(), 4, out.size(), o) != out.size()) { perror(argv[3]); return 2; }
        fclose(o);
        return 0;
    }
    if (mode != "reproject") { fprintf(stderr, "unknown mode\n"); return 2; }
    float par[4], cam[20], fovCur;
    if (!readAll(f, hdr, 12) || !readAll(f, par, 16) || !readAll(f, cam, 80) || !readAll(f, &fovCur, 4) || hdr[0] <= 0 || hdr[1] <= 0) { fprintf(stderr, "bad header\n"); return 2; }
    const int W = hdr[0], H = hdr[1];
    const bool moments = hdr[2] != 0;
    const size_t N = (size_t)W * H;
    std::vector<float> cur(N * 8), prev(N * 8), hist(N * 4), hmom(moments ? N * 4 : 0);
    if (!readAll(f, cur.data(), N * 32) || !readAll(f, prev.data(), N * 32) || !readAll(f, hist.data(), N * 16) || !readAll(f, hmom.data(), hmom.size() * 4)) {
        fprintf(stderr, "short input\n"); return 2;
    }
    fclose(f);
    const rp_params rp = {par[0], par[1], par[2], par[3]};
    if (!rp_params_ok(rp)) { fprintf(stderr, "bad parameters\n"); return 2; }
    const Cam pc = cam20(cam);
    const rp_view vw = rp_make_view(pc.pos, pc.dir, pc.up, pc.right, pc.fov, fovCur, W, H);
    auto at4 = [](const std::vector<float> &v, size_t i) { return mk_rp4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]); };
    std::vector<float> px(N * 4), mom(N * 4, 0.0f), wt(N * 4, 0.0f);
    std::vector<int32_t> tap(N * 4, -1);
    for (size_t i = 0; i < N; i++) {
        rp4 o, om;
        const uint32_t mask = rp_pixel(vw, rp, at4(cur, 2 * i), at4(cur, 2 * i + 1), moments,
                                       [&](uint32_t j) { return at4(prev, 2 * (size_t)j); }, [&](uint32_t j) { return at4(prev, 2 * (size_t)j + 1); },
                                       [&](uint32_t j) { return at4(hist, j); }, [&](uint32_t j) { return at4(hmom, j); }, &o, &om);
        px[4 * i] = o.x; px[4 * i + 1] = o.y; px[4 * i + 2] = o.z; px[4 * i + 3] = o.w;
        mom[4 * i] = om.x; mom[4 * i + 1] = om.y; mom[4 * i + 2] = om.z; mom[4 * i + 3] = om.w;
        if (mask) {     // the taps again, for the tests' agreement check: rp_pixel's own projection
            float xf, yf;
            rp_project(vw, mk3(cur[8 * i], cur[8 * i + 1], cur[8 * i + 2]), &xf, &yf);
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
