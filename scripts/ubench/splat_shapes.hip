// Microbenchmark: the SHAPE of the fused logic pass's splat on gfx950 -- four float atomics into one aligned 16-byte pixel {r, g, b, n} per terminating path.
// Modelled on logic_stream.hip MODE 6: 8 M threads (thread = path, 256-thread blocks), 21 % of them terminating by a hash of the id, a 1920x1080 float4
// framebuffer (33 MB), pixels by a hash that also puts several terminators of one wave on ONE pixel (a quarter of the lanes take the pixel of their group of 16).
// Shapes:
//   0 (a)  as shipped: the terminating lane issues four atomic instructions, one dword each -- a wave-instruction touches ~13 pixels with 4 bytes each
//   1 (b)  wave-transposed by cross-lane moves: the terminators are compacted to the low lanes (ds_permute), then lane 4k+c adds component c of the k-th one
//          (ds_bpermute + select), in rounds of 16 pixels -- a pixel is one contiguous 16-byte piece of one instruction
//   2 (b') the same transposition through a wave-private LDS stage (one 16-byte + one 4-byte LDS write per terminator, two 4-byte reads per adding lane; no barrier)
//   3 (c)  the terminators of the whole BLOCK compacted through LDS (two barriers), so that the atomic instructions are full: 64 lanes = 16 pixels
//   4 (-)  no splat at all: the floor (what the lab build -DFLX_LAB_LOGIC_NOSPLAT is to the product)
// Each shape ALONE (nothing but the splat), behind the MODE-5 streaming pattern of logic_stream.hip (terminating lanes store 3 of 12 records) and behind the MODE-2
// pattern (every lane stores every record: what the shipped pass does, LOGIC_FULL_STORES).  Five repetitions of 20 launches each, the configurations interleaved,
// behind one repetition that is not counted (clocks, first touches); min / median / max per configuration.  The added values are small integers, so the framebuffer must equal launches x the host's sums EXACTLY, counts included.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <vector>
#include <algorithm>
#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)
typedef float v4f __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 rd4(const float4 *p) { v4f v = __builtin_nontemporal_load((const v4f *)p); return make_float4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ void wr4(float4 *p, float4 v) { v4f t; t.x = v.x; t.y = v.y; t.z = v.z; t.w = v.w; __builtin_nontemporal_store(t, (v4f *)p); }
struct St { float4 *rec[12]; uint32_t *blocked; float *pick; uint8_t *member; const float4 *shade; uint32_t nshade; uint32_t n; };
#define NPIX 2073600u

__host__ __device__ inline uint32_t mix(uint32_t x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x; }
__host__ __device__ inline bool is_term(uint32_t gid) { return ((gid * 2654435761u) >> 8) % 100u < 21u; }
__host__ __device__ inline uint32_t pixel_of(uint32_t gid) { const uint32_t key = ((mix(gid ^ 0x5bd1e995u) >> 5) & 3u) == 0u ? (gid | 15u) + 1u : gid; return mix(key) % NPIX; }
__host__ __device__ inline void value_of(uint32_t gid, float *v) { v[0] = (float)((gid & 7u) + 1u); v[1] = (float)((gid >> 3) & 7u); v[2] = (float)((gid >> 7) & 7u); v[3] = 1.0f; }
__device__ __forceinline__ uint32_t mbcnt64(uint64_t m) { return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)); }

template <int SHAPE, int STREAM>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5, 5))) void k(St st, float *fb)
{
    const uint32_t gid = blockIdx.x * 256 + threadIdx.x;          // (n is a multiple of 256: every thread of a block is here, shape 3 has barriers)
    const bool term = is_term(gid);
    if (STREAM != 0) {                                            // logic_stream.hip, MODE 2 (full stores) or MODE 5 (holes)
        const uint32_t b = st.blocked[gid]; const float pk = st.pick[gid];
        float4 r0 = rd4(st.rec[0] + gid), r1 = rd4(st.rec[1] + gid), r2 = rd4(st.rec[2] + gid), r3 = rd4(st.rec[3] + gid), r4 = rd4(st.rec[4] + gid), r5 = rd4(st.rec[5] + gid);
        float4 acc = make_float4(r0.x + r1.x + pk, r2.y + r3.y, r4.z + r5.z, r0.w);
        if (b == 0u) {
            float4 a = rd4(st.rec[8] + gid), c = rd4(st.rec[9] + gid), d = rd4(st.rec[10] + gid), e = rd4(st.rec[11] + gid);
            acc.x += a.x * c.y; acc.y += d.z * e.w;
        }
        {
            const float4 *sp = st.shade + (size_t)(__float_as_uint(r4.z) % st.nshade) * 4;
            float4 a = sp[0], c = sp[1], d = sp[2], e = sp[3];
            acc.z += a.x + c.y + d.z + e.w;
        }
        const bool holes = STREAM == 5 && term;
        #pragma unroll
        for (int r = 0; r < 12; r++) if (!holes || r == 4 || r == 5 || r == 6) wr4(st.rec[r] + gid, make_float4(acc.x + r, acc.y, acc.z, r == 4 ? r4.z : acc.w));
        st.member[gid] = (uint8_t)(b + 1u);
    }
    const uint32_t pix = pixel_of(gid);
    float v[4]; value_of(gid, v);
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    if (SHAPE == 0) {
        if (term) {
            float *px = fb + (size_t)pix * 4;
            unsafeAtomicAdd(px + 0, v[0]); unsafeAtomicAdd(px + 1, v[1]); unsafeAtomicAdd(px + 2, v[2]); unsafeAtomicAdd(px + 3, v[3]);
        }
    } else if (SHAPE == 1) {
        const uint64_t tb = __ballot(term), ab = __ballot(true);
        const uint32_t n = (uint32_t)__popcll(tb), rank = mbcnt64(tb);
        const int dest = (int)((term ? rank : n + mbcnt64(ab) - rank) << 2);          // a permutation of the active lanes: terminators first, in lane order
        const int ci = __builtin_amdgcn_ds_permute(dest, (int)pix);
        const int c0 = __builtin_amdgcn_ds_permute(dest, __float_as_int(v[0])), c1 = __builtin_amdgcn_ds_permute(dest, __float_as_int(v[1]));
        const int c2 = __builtin_amdgcn_ds_permute(dest, __float_as_int(v[2])), c3 = __builtin_amdgcn_ds_permute(dest, __float_as_int(v[3]));
        const uint32_t c = lane & 3u;
        for (uint32_t base = 0; base < n; base += 16u) {
            const uint32_t s = base + (lane >> 2);
            const int src = (int)((s & 63u) << 2);
            const int pi = __builtin_amdgcn_ds_bpermute(src, ci);
            const int w0 = __builtin_amdgcn_ds_bpermute(src, c0), w1 = __builtin_amdgcn_ds_bpermute(src, c1);
            const int w2 = __builtin_amdgcn_ds_bpermute(src, c2), w3 = __builtin_amdgcn_ds_bpermute(src, c3);
            const int w = c == 0u ? w0 : c == 1u ? w1 : c == 2u ? w2 : w3;
            if (s < n) unsafeAtomicAdd(fb + (size_t)(uint32_t)pi * 4 + c, __int_as_float(w));
        }
    } else if (SHAPE == 2) {
        __shared__ float4 s_v[4][64];
        __shared__ uint32_t s_i[4][64];
        const uint64_t tb = __ballot(term);
        const uint32_t n = (uint32_t)__popcll(tb), rank = mbcnt64(tb);
        if (term) { s_v[wv][rank] = make_float4(v[0], v[1], v[2], v[3]); s_i[wv][rank] = pix; }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const uint32_t c = lane & 3u;
        for (uint32_t base = 0; base < n; base += 16u) {
            const uint32_t s = base + (lane >> 2);
            if (s < n) unsafeAtomicAdd(fb + (size_t)s_i[wv][s] * 4 + c, ((const float *)s_v[wv])[s * 4u + c]);
        }
    } else if (SHAPE == 3) {
        __shared__ float4 s_v[256];
        __shared__ uint32_t s_i[256];
        __shared__ uint32_t s_n[4];
        const uint64_t tb = __ballot(term);
        const uint32_t rank = mbcnt64(tb);
        if (lane == 0u) s_n[wv] = (uint32_t)__popcll(tb);
        __syncthreads();
        uint32_t before = 0u, total = 0u;
        for (uint32_t w = 0; w < 4u; w++) { const uint32_t m = s_n[w]; total += m; if (w < wv) before += m; }
        if (term) { s_v[before + rank] = make_float4(v[0], v[1], v[2], v[3]); s_i[before + rank] = pix; }
        __syncthreads();
        for (uint32_t t = threadIdx.x; t < 4u * total; t += 256u) unsafeAtomicAdd(fb + (size_t)s_i[t >> 2] * 4 + (t & 3u), ((const float *)s_v)[t]);
    }
}

template <int SHAPE, int STREAM>
static float run(St st, float *fb, int reps)
{
    hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    const dim3 g(st.n / 256), b(256);
    for (int i = 0; i < 3; i++) hipLaunchKernelGGL((k<SHAPE, STREAM>), g, b, 0, 0, st, fb);
    (void)hipEventRecord(e0, 0);
    for (int i = 0; i < reps; i++) hipLaunchKernelGGL((k<SHAPE, STREAM>), g, b, 0, 0, st, fb);
    (void)hipEventRecord(e1, 0); (void)hipEventSynchronize(e1);
    float ms; (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return ms / reps;
}

int main()
{
    St st; st.n = 1u << 23; st.nshade = 30u * 1024 * 1024 / 64;
    for (int r = 0; r < 12; r++) { CHECK(hipMalloc(&st.rec[r], (size_t)st.n * 16)); CHECK(hipMemset(st.rec[r], 0, (size_t)st.n * 16)); }
    CHECK(hipMalloc(&st.blocked, st.n * 4)); CHECK(hipMalloc(&st.pick, st.n * 4)); CHECK(hipMalloc(&st.member, st.n));
    float4 *sh; CHECK(hipMalloc(&sh, (size_t)st.nshade * 64)); CHECK(hipMemset(sh, 0, (size_t)st.nshade * 64)); st.shade = sh;
    std::vector<uint32_t> hb(st.n); std::vector<float4> h4(st.n);
    uint32_t s = 12345u;
    for (uint32_t i = 0; i < st.n; i++) { s = s * 1664525u + 1013904223u; hb[i] = ((s >> 8) % 100u) < 26u ? 0u : 1u; h4[i] = make_float4(0.f, 0.f, 0.f, 0.f); uint32_t t = s ^ (s >> 13); h4[i].z = *(float *)&t; }
    CHECK(hipMemcpy(st.blocked, hb.data(), st.n * 4, hipMemcpyHostToDevice));
    CHECK(hipMemset(st.pick, 0, st.n * 4));

    // the host's sums of ONE launch, and how the terminators fall on the waves
    std::vector<uint32_t> want((size_t)NPIX * 4, 0u);
    uint64_t nterm = 0, dupLanes = 0; uint32_t maxPerWave = 0;
    for (uint32_t w = 0; w < st.n / 64; w++) {
        uint32_t inWave = 0, seen[64];
        for (uint32_t l = 0; l < 64; l++) {
            const uint32_t gid = w * 64 + l;
            if (!is_term(gid)) continue;
            const uint32_t pix = pixel_of(gid); float v[4]; value_of(gid, v);
            for (int c = 0; c < 4; c++) want[(size_t)pix * 4 + c] += (uint32_t)v[c];
            for (uint32_t j = 0; j < inWave; j++) if (seen[j] == pix) { dupLanes++; break; }
            seen[inWave++] = pix;
        }
        nterm += inWave; maxPerWave = std::max(maxPerWave, inWave);
    }
    printf("%u threads, %llu terminate (%.1f %%), at most %u per wave, %llu lanes share a pixel with an earlier lane of their wave\n",
           st.n, (unsigned long long)nterm, 100.0 * nterm / st.n, maxPerWave, (unsigned long long)dupLanes);

    float *fb[5]; uint32_t launches[5] = {0, 0, 0, 0, 0};
    for (int i = 0; i < 5; i++) { CHECK(hipMalloc(&fb[i], (size_t)NPIX * 16)); CHECK(hipMemset(fb[i], 0, (size_t)NPIX * 16)); }
    const int reps = 20, REPEAT = 5;
    static float ms[3][5][REPEAT + 1];
    for (int r = 0; r <= REPEAT; r++) {                     // (the first one is dropped below)
#define RUN(SH, STR, row) do { CHECK(hipMemcpy(st.rec[4], h4.data(), (size_t)st.n * 16, hipMemcpyHostToDevice)); ms[row][SH][r] = run<SH, STR>(st, fb[SH], reps); launches[SH] += reps + 3; } while (0)
        RUN(0, 0, 0); RUN(1, 0, 0); RUN(2, 0, 0); RUN(3, 0, 0); RUN(4, 0, 0);
        RUN(0, 5, 1); RUN(1, 5, 1); RUN(2, 5, 1); RUN(3, 5, 1); RUN(4, 5, 1);
        RUN(0, 2, 2); RUN(1, 2, 2); RUN(2, 2, 2); RUN(3, 2, 2); RUN(4, 2, 2);
    }
    CHECK(hipDeviceSynchronize());
    const char *rows[3] = {"alone", "behind the MODE-5 stream (holes)", "behind the MODE-2 stream (full stores)"};
    const char *shapes[5] = {"(a)  shipped, 4 instructions x 1 dword", "(b)  wave-transposed, cross-lane moves", "(b') wave-transposed, wave-private LDS", "(c)  block-compacted through LDS",
                             "(-)  no splat"};
    for (int row = 0; row < 3; row++) {
        printf("%s\n", rows[row]);
        for (int sh = 0; sh < 5; sh++) {
            float *m = ms[row][sh] + 1; std::sort(m, m + REPEAT);
            printf("  %-42s min %.4f  median %.4f  max %.4f ms   (", shapes[sh], m[0], m[REPEAT / 2], m[REPEAT - 1]);
            for (int r = 0; r < REPEAT; r++) printf("%s%.4f", r ? " " : "", m[r]);
            printf(")\n");
        }
    }
    int bad = 0;
    std::vector<float> got((size_t)NPIX * 4);
    for (int sh = 0; sh < 5; sh++) {
        CHECK(hipMemcpy(got.data(), fb[sh], (size_t)NPIX * 16, hipMemcpyDeviceToHost));
        uint64_t wrong = 0;
        for (size_t i = 0; i < got.size(); i++) if (got[i] != (sh == 4 ? 0.0f : (float)((uint64_t)want[i] * launches[sh]))) wrong++;
        printf("check %-42s %u launches: %llu of %zu sums differ from the host's (exact compare, counts included)\n", shapes[sh], launches[sh], (unsigned long long)wrong, got.size());
        if (wrong) bad = 1;
    }
    printf(bad ? "FAILED\n" : "OK\n");
    return bad;
}
