// rectify_cpu.cpp -- the CPU counterpart of flx_history_rectify (fluctus_amd/csrc/rectify.hip): the same per-pixel functions of
// fluctus_amd/csrc/flx_rectify.h over the whole image -- the prepare pass first, then the window pass on its records.  Built by the tests with
// g++ -O2 -ffp-contract=off; its output must equal the device's bit for bit.
//
//   rectify_cpu <in> <out>
//     in:  int32 W, H, moments (bit 0: which = 7 is on now, bit 1: the mark has moments; both: the moments are rectified), radius, min_pixels;
//          float32 gamma, sensitivity, lum_floor, plane_tolerance_px, normal_cos, fov (the current slot's camera);
//          float32 curG[W*H*8], A[W*H*4], S[W*H*4][, M[W*H*4]: bit 0][, SM[W*H*4]: bit 1]
//     out: float32 A'[W*H*4], S'[W*H*4], M'[W*H*4], SM'[W*H*4] (the inputs where not rectified, zeros where absent), lambda[W*H];
//          int32 counted[W*H] (N of the window), uint32 taps[W*H] (sum of (k + 1)^2 over the counted taps, k the tap's row-major number in the
//          window: the tests' agreement check)
#include "../fluctus_amd/csrc/flx_rectify.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace flx;

static bool readAll(FILE *f, void *p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: rectify_cpu <in> <out>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t hdr[5]; float par[6];
    if (!readAll(f, hdr, 20) || !readAll(f, par, 24) || hdr[0] <= 0 || hdr[1] <= 0) { fprintf(stderr, "bad header\n"); return 2; }
    const int W = hdr[0], H = hdr[1];
    const bool haveM = hdr[2] & 1, haveSM = (hdr[2] & 2) != 0, moments = haveM && haveSM;
    rc_params rc; rc.radius = hdr[3]; rc.min_pixels = hdr[4]; rc.gamma = par[0]; rc.sensitivity = par[1]; rc.lum_floor = par[2];
    rc.plane_tolerance_px = par[3]; rc.normal_cos = par[4];
    if (!rc_params_ok(rc)) { fprintf(stderr, "bad parameters\n"); return 3; }
    const float footprint = rc_footprint(par[5], H);
    const size_t N = (size_t)W * H;
    std::vector<float> cur(N * 8), A(N * 4), S(N * 4), M(N * 4, 0.0f), SM(N * 4, 0.0f);
    if (!readAll(f, cur.data(), N * 32) || !readAll(f, A.data(), N * 16) || !readAll(f, S.data(), N * 16) || (haveM && !readAll(f, M.data(), N * 16)) ||
        (haveSM && !readAll(f, SM.data(), N * 16))) { fprintf(stderr, "short input\n"); return 2; }
    fclose(f);
    auto at4 = [](const std::vector<float> &v, size_t i) { return mk_rp4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]); };
    auto put4 = [](std::vector<float> &v, size_t i, rp4 q) { v[4 * i] = q.x; v[4 * i + 1] = q.y; v[4 * i + 2] = q.z; v[4 * i + 3] = q.w; };
    std::vector<float> rec(N * 4);
    for (size_t i = 0; i < N; i++) put4(rec, i, rc_prepare(at4(A, i), at4(S, i), at4(cur, 2 * i)));
    std::vector<float> oA = A, oS = S, oM = M, oSM = SM, lam(N, 0.0f);
    std::vector<int32_t> counted(N, 0);
    std::vector<uint32_t> taps(N, 0u);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t i = (size_t)y * W + x;
            const rp4 g0 = at4(cur, 2 * i), g1 = at4(cur, 2 * i + 1);
            auto pix = [&](int xq, int yq) { return (size_t)yq * W + xq; };
            uint32_t cnt;
            const float l = rc_lambda(rc, footprint, W, H, x, y, g0, g1, at4(A, i), at4(S, i),
                                      [&](int xq, int yq) { return at4(rec, pix(xq, yq)); }, [&](int xq, int yq) { return at4(cur, 2 * pix(xq, yq)); },
                                      [&](int xq, int yq) { return at4(cur, 2 * pix(xq, yq) + 1); }, &cnt);
            lam[i] = l; counted[i] = (int32_t)cnt;
            if (cnt) {      // the taps again, for the tests' agreement check: rc_lambda's own tests
                const f3 P = mk3(g0.x, g0.y, g0.z), Nn = mk3(g1.x, g1.y, g1.z);
                const float tol = rc.plane_tolerance_px * g1.w * footprint;
                uint32_t k = 0, sum = 0;
                for (int dy = -rc.radius; dy <= rc.radius; dy++)
                    for (int dx = -rc.radius; dx <= rc.radius; dx++, k++) {
                        const int xq = x + dx, yq = y + dy;
                        if (xq < 0 || xq >= W || yq < 0 || yq >= H || !(rec[4 * pix(xq, yq) + 3] > 0.0f)) continue;
                        const rp4 q0 = at4(cur, 2 * pix(xq, yq)), q1 = at4(cur, 2 * pix(xq, yq) + 1);
                        if (rp_same_plane(mk3(q0.x, q0.y, q0.z), P, Nn, tol) && rp_same_facing(mk3(q1.x, q1.y, q1.z), Nn, rc.normal_cos)) sum += (k + 1) * (k + 1);
                    }
                taps[i] = sum;
            }
            rp4 a, s;
            if (!rc_apply(l, at4(A, i), at4(S, i), &a, &s)) continue;
            put4(oA, i, a); put4(oS, i, s);
            if (moments) { rc_apply(l, at4(M, i), at4(SM, i), &a, &s); put4(oM, i, a); put4(oSM, i, s); }
        }
    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    fwrite(oA.data(), 4, oA.size(), o); fwrite(oS.data(), 4, oS.size(), o); fwrite(oM.data(), 4, oM.size(), o); fwrite(oSM.data(), 4, oSM.size(), o);
    fwrite(lam.data(), 4, N, o); fwrite(counted.data(), 4, N, o); fwrite(taps.data(), 4, N, o);
    fclose(o);
    return 0;
}
