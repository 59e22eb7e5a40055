// rebuild_job_main.cpp -- the hand-over of RebuildJob (fluctus_amd/host/rebuild_job.hpp) under ThreadSanitizer: a stand-alone program, compiled
// with g++ -fsanitize=thread together with rebuild_job.cpp and bvh.cpp and run by tests/test_tree_cost.py.
//
//   1. one thread runs a job while the main thread refits ANOTHER tree over triangles that keep changing, and polls ready();
//   2. the result is taken and compared, node for node and index for index, with a serial build of the snapshot;
//   3. a second job is destroyed while parked at the hold gate, a third right after start(), in the middle of its build: the destructor joins.
//
// The worker's builder is forced serial (threads = 1 -> BVH::sbvhThreads = 1), and so is the main thread's: ThreadSanitizer does not see
// libgomp's barriers and would report the OpenMP team's own synchronisation, not ours.  What is checked is the job's hand-over -- the snapshot,
// the release / acquire pair on `done`, the join -- which does not depend on how many threads the builder uses.
#include "../fluctus_amd/host/rebuild_job.hpp"
#include <cstdio>
#include <cstring>

using namespace fluctus;

static uint32_t g_seed = 12345u;
static float rnd() { g_seed = g_seed * 1664525u + 1013904223u; return (float)(g_seed >> 8) * (1.0f / 16777216.0f); }

static std::vector<flx_triangle> scene(size_t n)
{
    std::vector<flx_triangle> t(n);
    std::memset(t.data(), 0, n * sizeof(flx_triangle));
    for (auto &tri : t) {
        const float c[3] = {rnd() * 10.0f, rnd() * 10.0f, rnd() * 10.0f};
        flx_vertex *v[3] = {&tri.v0, &tri.v1, &tri.v2};
        for (int k = 0; k < 3; k++) { v[k]->p.x = c[0] + rnd(); v[k]->p.y = c[1] + rnd(); v[k]->p.z = c[2] + rnd(); }
    }
    return t;
}

static int fail(const char *what) { std::printf("FAILED: %s\n", what); return 1; }

int main()
{
    const std::vector<flx_triangle> base = scene(3000);
    std::vector<flx_triangle> moving = base;
    BVH other; other.sbvhThreads = 1;
    other.build(&base, BVH::Mode::SBVH);

    std::unique_ptr<BVH> built; std::vector<flx_triangle> snapshot;
    {
        RebuildJob job;
        job.start(moving, BVH::Mode::SBVH, 1);
        unsigned polls = 0;
        do {                                                  // the frames: the caller's triangles move on, another tree is refitted, the job is polled
            const float step = (polls & 1u) ? -0.25f : 0.25f;              // back and forth: the moving scene stays a scene a builder handles
            for (auto &t : moving) { t.v0.p.x += step; t.v1.p.y -= step; }
            other.refit(moving);
            polls++;
        } while (!job.ready());
        job.take(built, snapshot);
        if (job.active() || job.ready()) return fail("the job is not idle after take()");
        std::printf("polled %u times while the worker built\n", polls);
    }
    if (snapshot.size() != base.size() || std::memcmp(snapshot.data(), base.data(), base.size() * sizeof(flx_triangle)) != 0)
        return fail("the snapshot is not the triangles start() was given");
    BVH serial; serial.sbvhThreads = 1;
    serial.build(&base, BVH::Mode::SBVH);
    if (built->m_nodes.size() != serial.m_nodes.size() || std::memcmp(built->m_nodes.data(), serial.m_nodes.data(), serial.m_nodes.size() * sizeof(flx_node)) != 0)
        return fail("the job's nodes differ from a serial build of the snapshot");
    if (built->m_indices != serial.m_indices) return fail("the job's index list differs from a serial build of the snapshot");

    {
        RebuildJob second;
        second.hold(true);
        second.start(moving, BVH::Mode::SBVH, 1);
        if (second.ready()) return fail("a held job reports ready");
        bool threw = false;
        try { second.take(built, snapshot); } catch (const std::exception &) { threw = true; }
        if (!threw) return fail("take() before ready() did not throw");
    }                                                         // destroyed mid-flight: joins
    {
        RebuildJob third;                                     // ... and one that is really building when it goes (nothing holds it)
        third.start(base, BVH::Mode::SBVH, 1);
    }
    std::printf("ok\n");
    return 0;
}
