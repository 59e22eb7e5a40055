// rebuild_job.cpp -- see rebuild_job.hpp.
#include "rebuild_job.hpp"
#include <stdexcept>

namespace fluctus {

RebuildJob::~RebuildJob() { wait(); }

void RebuildJob::hold(bool on)
{
    { std::lock_guard<std::mutex> lk(gate); held = on; }
    gateCv.notify_all();
}

void RebuildJob::start(const std::vector<flx_triangle> &tris, BVH::Mode mode, int threads, size_t jobSize)
{
    if (running) throw std::runtime_error("RebuildJob::start: a job is in flight (take or discard it first)");
    snap = tris;                                            // the snapshot: the build never sees the caller's array
    tree.reset(new BVH());
    tree->sbvhThreads = threads; tree->sbvhJobSize = jobSize;
    error.clear();
    done.store(false, std::memory_order_relaxed);
    running = true;
    worker = std::thread([this, mode] {
        try { tree->build(&snap, mode); }
        catch (const std::exception &e) { error = e.what(); if (error.empty()) error = "BVH build failed"; }
        catch (...) { error = "BVH build failed"; }
        { std::unique_lock<std::mutex> lk(gate); gateCv.wait(lk, [this] { return !held; }); }
        done.store(true, std::memory_order_release);
    });
}

void RebuildJob::wait() { hold(false); if (worker.joinable()) worker.join(); }

void RebuildJob::take(std::unique_ptr<BVH> &bvh, std::vector<flx_triangle> &snapshot)
{
    if (!ready()) throw std::runtime_error(running ? "RebuildJob::take: the build has not finished (poll ready() or wait())" : "RebuildJob::take: no job was started");
    wait();
    running = false;
    if (!error.empty()) { tree.reset(); snap.clear(); throw std::runtime_error("RebuildJob: " + error); }
    bvh = std::move(tree);
    snapshot = std::move(snap);
    snap.clear();
}

void RebuildJob::discard()
{
    wait();
    running = false;
    tree.reset(); snap.clear(); error.clear();
}

} // namespace fluctus
