// rebuild_job.hpp -- one BVH build on a worker thread, off the frame's critical path (asynchronous construction: Ize, Wald, Parker 2007;
// DESIGN.md 4.10.1).  GPU-free: the worker copies nothing but triangles, calls BVH::build and touches no Tracer or device state, so the
// frames go on with refits while it runs and the owner decides when to look at the result.
//
//   start(tris, mode)   copies the triangles (the SNAPSHOT: later changes to the caller's array do not reach the build) and starts the worker
//   ready()             polls: the worker has finished (with a tree or with an error)
//   wait()              blocks until it has
//   take(bvh, snapshot) hands over the tree and the snapshot it was built for; rethrows the builder's error; the job is idle again
//   ~RebuildJob()       joins: a job destroyed mid-build finishes its build first (the builder has no cancellation point)
//   hold(on)            test hook: while held, a worker that has finished its build does not publish it -- ready() stays false -- so a test decides
//                       between which two calls of the owner a job completes, without sleeping.  wait(), discard() and the destructor release it.
// One owner thread calls all of these.  The hand-over is one release store / acquire load of `done` plus the join; what the worker wrote is
// read only behind it.  The builder sizes its OpenMP team by BVH::usableThreads() exactly as an inline BVH::build does (threads = 0).
#pragma once
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <memory>
#include <string>
#include <thread>
#include <vector>
#include "bvh.hpp"

namespace fluctus {

class RebuildJob {
public:
    RebuildJob() {}
    ~RebuildJob();
    RebuildJob(const RebuildJob &) = delete;
    RebuildJob &operator=(const RebuildJob &) = delete;

    // threads / jobSize: BVH::sbvhThreads / sbvhJobSize of the worker's builder (0 = the defaults)
    void start(const std::vector<flx_triangle> &tris, BVH::Mode mode, int threads = 0, size_t jobSize = 0);
    bool active() const { return running; }               // started and not yet taken
    bool ready() const { return running && done.load(std::memory_order_acquire); }
    void wait();                                           // no-op when idle
    void take(std::unique_ptr<BVH> &bvh, std::vector<flx_triangle> &snapshot);
    void discard();                                        // joins and drops the result (a job made obsolete)
    void hold(bool on);

private:
    std::thread worker;
    std::atomic<bool> done {false};
    bool running = false;
    std::unique_ptr<BVH> tree;
    std::vector<flx_triangle> snap;
    std::string error;
    std::mutex gate;
    std::condition_variable gateCv;
    bool held = false;
};

} // namespace fluctus
