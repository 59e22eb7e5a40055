// pose_cpu.cpp -- a stand-alone run of the host side of flx_objects_define (the member compaction) and of csrc/flx_pose.h, built by
// tests/test_pose.py with g++ -fsanitize=address,undefined and never loaded into Python.  Heap buffers of exactly the sizes the callers
// allocate, so that a read or write past a member list, a rest array or a triangle is a sanitizer report.  Prints "ok" and a checksum.
#include "../fluctus_amd/csrc/flx_pose.h"
#include "../include/fluctus_wire.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

static uint32_t rnd(uint32_t &s) { return s = flx::hash_u32(s + 0x9E3779B9u); }

int main()
{
    uint32_t seed = 1;
    uint64_t sum = 0;
    // ntris 0 and 1, sizes around the kernels' block of 256, every triangle a member, none, runs and interleaved ids, an empty object
    const size_t sizes[] = {0, 1, 2, 255, 256, 257, 1568};
    for (size_t ntris : sizes) {
        for (int map = 0; map < 4; map++) {
            const uint32_t nobjects = map == 3 ? 1u : 4u;
            std::vector<flx_triangle> rest(ntris);
            std::vector<uint32_t> objectOf(ntris);
            for (size_t i = 0; i < ntris; i++) {
                float *f = (float *)&rest[i];
                for (int k = 0; k < 40; k++) f[k] = (float)(rnd(seed) & 0xFFFF) / 4096.0f - 8.0f;
                rest[i].matId = (int32_t)(rnd(seed) & 7);
                objectOf[i] = map == 0 ? (uint32_t)(i % 3 == 2 ? FLX_PS_NO_OBJECT : i % 3)      // interleaved; object 2 and 3 stay empty
                            : map == 1 ? FLX_PS_NO_OBJECT                                       // no member at all
                            : map == 2 ? (uint32_t)(i < ntris / 3 ? 3 : i < ntris / 2 ? FLX_PS_NO_OBJECT : 1)
                            : 0u;                                                                // one object holds everything
            }
            std::vector<uint32_t> counts(nobjects);
            size_t bad = 0;
            const size_t members = flx::ps_count_members(objectOf.data(), ntris, nobjects, counts.data(), &bad);
            if (members == (size_t)-1) { printf("refused a valid map\n"); return 1; }
            std::vector<uint32_t> tri(members), obj(members);
            std::vector<flx_triangle> mrest(members);
            flx::ps_compact_members(rest.data(), objectOf.data(), ntris, tri.data(), obj.data(), mrest.data());
            size_t total = 0;
            for (uint32_t o = 0; o < nobjects; o++) total += counts[o];
            if (total != members) { printf("counts do not add up\n"); return 1; }
            for (size_t k = 0; k < members; k++) {
                if ((k && tri[k] <= tri[k - 1]) || objectOf[tri[k]] != obj[k] || memcmp(&mrest[k], &rest[tri[k]], 160)) { printf("bad member %zu\n", k); return 1; }
            }
            // pose the members: into a second buffer and in place
            const float X[12] = {0.5f, -1.25f, 0.0f, 3.0f, 2.0f, 0.75f, 0.5f, -1.0f, 0.0f, 0.25f, -1.5f, 0.125f};
            if (!flx::ps_xform_finite(X) || !flx::ps_xform_invertible(X)) { printf("refused a valid transform\n"); return 1; }
            std::vector<flx_triangle> out(members);
            flx::ps_pose_triangles(X, mrest.data(), out.data(), members);
            flx::ps_pose_triangles(X, mrest.data(), mrest.data(), members);
            if (members && memcmp(out.data(), mrest.data(), members * 160)) { printf("in place differs\n"); return 1; }
            for (size_t k = 0; k < members; k++) sum += flx::f2u(out[k].v1.p.y) + (uint64_t)out[k].matId;
            // an id out of range is refused with its triangle
            if (ntris) {
                objectOf[ntris - 1] = nobjects;
                if (flx::ps_count_members(objectOf.data(), ntris, nobjects, counts.data(), &bad) != (size_t)-1 || bad != ntris - 1) { printf("accepted a bad id\n"); return 1; }
            }
        }
    }
    const float singular[12] = {1, 2, 3, 0, 2, 4, 6, 0, 0, 1, 0, 0};
    float nan12[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    nan12[7] = __builtin_nanf("");
    if (flx::ps_xform_invertible(singular) || flx::ps_xform_finite(nan12)) { printf("accepted a bad transform\n"); return 1; }
    printf("ok %llu\n", (unsigned long long)sum);
    return 0;
}
