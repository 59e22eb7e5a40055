// api.hip -- the C ABI of libfluctus_hip.so (include/fluctus_hip.h), first of six units (flx_ctx.h lists them): the context's lifetime, parameters,
// partition and framebuffers, flx_finish, the asynchronous counter and pixel-index calls, pixel read-back, options.
#include "flx_ctx.h"
#include <cstring>
#include <cstdlib>

thread_local std::string flxd::g_create_error;

static uint32_t localPixels(const flx_ctx *c)
{
    uint32_t npix = c->params.width * c->params.height;
    if (npix <= c->fr.rank) return 1;
    return (npix - c->fr.rank + c->fr.nranks - 1) / c->fr.nranks;
}

// the luminance moments (float4 per local pixel) exist only while the option "moments" is on; zeroed when made
static int allocMoments(flx_ctx *c)
{
    freeAll(c->momAllocs);
    c->fr.moments = nullptr;
    if (!c->moments || !c->fr.localPixels) return 0;
    const size_t n = (size_t)c->fr.localPixels * 4;
    HIPCHK(c, dalloc(c, c->momAllocs, &c->fr.moments, n) ? hipErrorOutOfMemory : hipSuccess);
    HIPCHK(c, hipMemsetAsync(c->fr.moments, 0, n * 4, c->stream));
    return 0;
}
// denoiser feature buffers (4 x float4 per local pixel) exist only while the option is on
static int allocAov(flx_ctx *c)
{
    c->dn.release();
    freeAll(c->aovAllocs);
    c->fr.aovAlbedo = c->fr.aovNormal = c->fr.aovAlbedoOut = c->fr.aovNormalOut = nullptr;
    if (!c->denoiser || !c->fr.localPixels) return 0;
    const size_t n = (size_t)c->fr.localPixels * 4;
    float *buf[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int i = 0; i < 4; i++) {
        HIPCHK(c, dalloc(c, c->aovAllocs, &buf[i], n) ? hipErrorOutOfMemory : hipSuccess);
        HIPCHK(c, hipMemsetAsync(buf[i], 0, n * 4, c->stream));
    }
    c->fr.aovAlbedo = buf[0]; c->fr.aovNormal = buf[1]; c->fr.aovAlbedoOut = buf[2]; c->fr.aovNormalOut = buf[3];
    return 0;
}

static int allocFrame(flx_ctx *c)
{
    uint32_t lp = localPixels(c);
    if (lp == c->fr.localPixels && c->fr.pixels) return 0;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->releaseFrameFeatures();
    freeAll(c->frameAllocs);
    HIPCHK(c, dalloc(c, c->frameAllocs, &c->fr.pixels, (size_t)lp * 4) ? hipErrorOutOfMemory : hipSuccess);
    HIPCHK(c, dalloc(c, c->frameAllocs, &c->fr.preview, (size_t)lp * 4) ? hipErrorOutOfMemory : hipSuccess);
    HIPCHK(c, hipMemsetAsync(c->fr.pixels, 0, (size_t)lp * 16, c->stream));
    HIPCHK(c, hipMemsetAsync(c->fr.preview, 0, (size_t)lp * 16, c->stream));
    c->fr.localPixels = lp;
    if (allocMoments(c)) return 1;
    return allocAov(c);
}

// refill = refillMin | waitMax << 8 (trace4r.hip).  refillMin 0 with a waitMax of 1..63 would end every descent round before a node is
// visited (0 finished lanes >= refillMin) while no lane is idle for the refill to serve: the kernel would spin forever.  0 = the
// thread-per-ray kernel; otherwise refillMin 1..64 and waitMax 0 (= 64) .. 64.
static bool refill_value_ok(int v) { return v == 0 || (v > 0 && (v & 0xFF) >= 1 && (v & 0xFF) <= 64 && (v >> 8) <= 64); }

// How the two traversals share the machine.  Two persistent kernels cannot run side by side (each fills every wave slot), so the second stream
// serves the THREAD-PER-RAY any-hit kernel: started right after `logic` (schedule 2) it runs beside genRays / the material kernels and then
// fills the slots the persistent closest-hit kernel's waves leave as they retire.  Measured with the final round-3 kernels (blocks handed out
// on demand; profiles/r03_wave_slots_sweep.txt, one box, Mrays/s, schedule 1 / schedule 2 / serial with a persistent any-hit kernel):
//   kitchen 4951-5249 / 5208-5489 / 4800-4840     conference 4931-4996 / 5017-5019 / 4590-4720     courtyard 2165 / 2181 / 1998-2076
// (an earlier build with a static share of blocks per wave preferred the serial schedule for the courtyard, whose tree comes from HBM; with
// balanced waves it does not).  Options "overlap" and "refill_shadow" override; -1 = these defaults.
// The thread-per-ray any-hit kernel of the second stream is itself a split launch where the light makes its rays long-tailed -- a budgeted pass, then ONE
// persistent kernel over the suspended rays only, which retires progressively beside the closest-hit kernel like the thread-per-ray waves do: that
// choice depends on the render parameters, not on the scene, and is made at the launch (effectiveSplit, below).
void flxd::pickSchedule(flx_ctx *c)
{
    c->overlap = c->overlapOpt >= 0 ? c->overlapOpt : 2;
    c->refillShadow = c->refillShadowOpt >= 0 ? c->refillShadowOpt : 0;
}

// The thread-per-ray any-hit kernel itself is one launch or a SPLIT one (trace4.hip: launch_shadow4_split): a pass over the queue under a
// budget of node visits, then the suspended rays in persistent waves that refill from the continuation records.  Which, is not the scene's business but the
// light's, and the render parameters can change from launch to launch, so the choice is made from them: where every shadow ray runs toward an environment
// light -- the condition under which launch_shadow4 takes the far -> near visit order -- the rays are unbounded and their lengths long-tailed, and the split
// pays; toward an area light they are short and it does not.  Option "shadow_split" overrides, 0 included; -1 = this choice.  How K was chosen and what
// it is worth: DESIGN.md 4.8.1, profiles/shadow_resume_ab.txt.
#define FLX_SPLIT_DEFAULT 8
int flxd::effectiveSplit(const flx_ctx *c)
{
    if (c->shadowSplitOpt >= 0) return c->shadowSplitOpt;
    return (c->haveParams && c->params.useEnvMap && !c->params.useAreaLight && !c->splitAllocFailed) ? FLX_SPLIT_DEFAULT : 0;
}
// ... and what the next flx_wf_shadow launches: the split exists for the thread-per-ray kernel on the 4-wide tree only -- not under "refill_shadow", the
// binary tree, a scene without a usable wide tree, or the counting kernels.  This is what flx_get_option("shadow_split") reports.
int flxd::splitNow(const flx_ctx *c)
{
    const bool wideKnown = c->sc.bnodes != nullptr;      // (before the first upload nothing says the wide tree is unusable)
    return (c->shadowTree == 4 && (c->wideOK || !wideKnown) && c->refillShadow == 0 && !c->statsOn) ? effectiveSplit(c) : 0;
}
// The records of the split the next launch will make, allocated where the choice can change -- flx_set_params, flx_upload_scene, the option -- so that no
// launch call allocates or waits (flx_wf_shadow calls it again for the paths that change the choice elsewhere: it then finds them).  When the library's OWN
// choice does not fit into device memory the choice becomes 0 for this context and the read-only option "shadow_split_fallback" says so; an explicit value fails.
int flxd::splitPrepare(flx_ctx *c)
{
    const int split = splitNow(c);
    if (split <= 0 || (c->splitRecA && ((split >> 8) == 0 || c->splitRecB))) return 0;
    if (splitBuffers(c, (split >> 8) > 0)) {
        if (c->shadowSplitOpt >= 0) return 1;
        c->splitAllocFailed = true; c->err.clear();
    }
    return 0;
}

// The continuation records of the split any-hit launch, allocated on first use and kept until the context goes away: the counters and the first set (64 B
// for numTasks / 2 records: ~540 MB at 16 M paths), and the second set (numTasks / 8 records) only when a launch has a second budget.
int flxd::splitBuffers(flx_ctx *c, bool second)
{
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->splitRecA) {
        uint32_t *cnt = nullptr; uint4 *a = nullptr;
        if (dalloc(c, c->fixedAllocs, &cnt, shadow_split_count_words()) || dalloc(c, c->fixedAllocs, &a, (size_t)c->splitCapA * shadow_split_lists() * 4)) {
            (void)hipGetLastError(); c->err = "shadow_split: out of device memory for the continuation records"; return 1;
        }
        HIPCHK(c, hipMemsetAsync(cnt, 0, (size_t)shadow_split_count_words() * 4, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));      // (once per context; the launch that follows may be on the second stream)
        c->splitCounts = cnt; c->splitRecA = a;
    }
    if (second && !c->splitRecB) {
        uint4 *b = nullptr;
        if (dalloc(c, c->fixedAllocs, &b, (size_t)c->splitCapB * shadow_split_lists() * 4)) { (void)hipGetLastError(); c->err = "shadow_split: out of device memory for the continuation records"; return 1; }
        c->splitRecB = b;
    }
    return 0;
}

// Device buffers of a feature that is off by default, allocated when the option is first switched on and kept until the context goes away.
static int optionBuffers(flx_ctx *c, bool regen)
{
    HIPCHK(c, hipSetDevice(c->device));
    if (regen && !c->lookback) {
        unsigned long long *lb = nullptr;
        if (dalloc(c, c->fixedAllocs, &lb, (size_t)logic_lookback_words(c->numTasks))) { c->err = "flx_set_option(regen): out of device memory for the look-back words"; return 1; }
        HIPCHK(c, hipMemsetAsync(lb, 0, (size_t)logic_lookback_words(c->numTasks) * 8, c->stream));
        c->lookback = lb;
    }
    return 0;
}

extern "C" {

const char *flx_last_error(flx_ctx *c) { return c ? c->err.c_str() : g_create_error.c_str(); }

int flx_create(int device, uint32_t num_tasks, flx_ctx **out)
{
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) { g_create_error = "flx_create: no HIP device available (libfluctus_hip.so has no CPU fallback)"; return 1; }
    if (device < 0 || device >= ndev) { g_create_error = "flx_create: bad device index"; return 1; }
    if (num_tasks == 0) { g_create_error = "flx_create: num_tasks must be > 0"; return 1; }
    flx_ctx *c = new flx_ctx();
    c->device = device; c->numTasks = num_tasks;
#ifdef FLX_LAB
    // lab build only (scripts/build_variants.py, -DFLX_LAB): A/B hooks for whole test-suite runs -- the defaults of the refill_extend /
    // refill_shadow options.  The shipped library reads no environment variable here.
    if (const char *e = getenv("FLX_REFILL_EXTEND")) { const int v = atoi(e); if (refill_value_ok(v)) c->refillExt = v; }
    if (const char *e = getenv("FLX_REFILL_SHADOW")) { const int v = atoi(e); if (v < 0 || refill_value_ok(v)) { c->refillShadowOpt = v; c->refillShadow = v < 0 ? 0 : v; } }
#endif
    auto fail = [&](const char *what, hipError_t err) { g_create_error = std::string(what) + ": " + hipGetErrorString(err); flx_destroy(c); return 1; };
    if ((e = hipSetDevice(device)) != hipSuccess) return fail("hipSetDevice", e);
    // (stream priorities were tried: a high-priority shadow stream keeps the extension kernel at its undisturbed 0.86 ms and inflates
    //  the material kernel instead, a high-priority main stream changes nothing -- resident waves are not displaced; the step time
    //  stays within 0.7 % in every combination, so both streams have the default priority)
#ifndef FLX_STREAM_PRIO          // 0: both streams at the default priority | 1: the main stream (logic -> genRays -> materials -> closest hit) above the any-hit stream
#define FLX_STREAM_PRIO 0
#endif
    {
        int least = 0, greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
        const int pMain = FLX_STREAM_PRIO ? greatest : 0, pSecond = FLX_STREAM_PRIO ? least : 0;
        if ((e = hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, pMain)) != hipSuccess) return fail("hipStreamCreate", e);
        if ((e = hipStreamCreateWithPriority(&c->stream2, hipStreamNonBlocking, pSecond)) != hipSuccess) return fail("hipStreamCreate", e);
    }
    if ((e = hipEventCreateWithFlags(&c->evPreExt, hipEventDisableTiming)) != hipSuccess || (e = hipEventCreateWithFlags(&c->evShadow, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&c->evPostLogic, hipEventDisableTiming)) != hipSuccess) return fail("hipEventCreate", e);
    const size_t N = num_tasks;
    c->st.numTasks = num_tasks;
    // (staggering the twelve arrays inside their allocations -- 272 / 4112 / 65808 elements per array -- changes nothing: the fused pass lands on
    //  one of three levels, 0.457 / 0.479 / 0.507 ms, from one process to the next with or without it, and so does ONE allocation for all twelve; profiles/r03_state_stagger_ab.txt, r03_state_slab_ab.txt)
    for (int r = 0; r < S_NUM_REC; r++) {
        if (dalloc(c, c->fixedAllocs, &c->st.rec[r], N)) return fail("hipMalloc(state)", hipErrorOutOfMemory);
        (void)hipMemsetAsync(c->st.rec[r], 0, N * sizeof(float4), c->stream);
    }
    for (int r = 0; r < 2; r++) {                        // the second {ORIG, DIR} pair (flx_device.h: State::other); freed with fixedAllocs whichever pair is current
        if (dalloc(c, c->fixedAllocs, &c->st.other[r], N)) return fail("hipMalloc(state)", hipErrorOutOfMemory);
        (void)hipMemsetAsync(c->st.other[r], 0, N * sizeof(float4), c->stream);
    }
    if (dalloc(c, c->fixedAllocs, &c->st.phase, N) || dalloc(c, c->fixedAllocs, &c->mkStats, 4)) return fail("hipMalloc(state)", hipErrorOutOfMemory);
    (void)hipMemsetAsync(c->st.phase, 0, N * 4, c->stream); (void)hipMemsetAsync(c->mkStats, 0, 16, c->stream);
    if (dalloc(c, c->fixedAllocs, &c->st.blocked, N) || dalloc(c, c->fixedAllocs, &c->st.pickProb, N) || dalloc(c, c->fixedAllocs, &c->st.firstDiffuse, N))
        return fail("hipMalloc(state)", hipErrorOutOfMemory);
    (void)hipMemsetAsync(c->st.blocked, 0, N * 4, c->stream); (void)hipMemsetAsync(c->st.pickProb, 0, N * 4, c->stream); (void)hipMemsetAsync(c->st.firstDiffuse, 0, N * 4, c->stream);
    for (int q = 0; q < FLX_NUM_QUEUES; q++) {
        if (dalloc(c, c->fixedAllocs, &c->qs.q[q], N)) return fail("hipMalloc(queue)", hipErrorOutOfMemory);
        (void)hipMemsetAsync(c->qs.q[q], 0, N * 4, c->stream);
    }
    if (dalloc(c, c->fixedAllocs, &c->qs.counters, 8) || dalloc(c, c->fixedAllocs, &c->qs.cursors, FLX_NUM_BLOCK_CURSORS * FLX_CURSOR_STRIDE)) return fail("hipMalloc(counters)", hipErrorOutOfMemory);
    (void)hipMemsetAsync(c->qs.counters, 0, 32, c->stream);
    (void)hipMemsetAsync(c->qs.cursors, 0, 4 * FLX_NUM_BLOCK_CURSORS * FLX_CURSOR_STRIDE, c->stream);
    const size_t auxStride = logic_aux_stride(num_tasks);          // per list, padded to whole segments of the queue build
    const size_t queueAuxWords = logic_queue_aux_words(num_tasks); // its segment totals (two buffers) and counter snapshot
    if (dalloc(c, c->fixedAllocs, &c->member, N) || dalloc(c, c->fixedAllocs, &c->blockCounts, (size_t)7 * auxStride) || dalloc(c, c->fixedAllocs, &c->queueAux, queueAuxWords))
        return fail("hipMalloc(logic aux)", hipErrorOutOfMemory);
    // (the look-back words of option "regen" and the continuation records of option "shadow_split" -- both off by default, together ~45 B per path -- are
    //  allocated when the option is first switched on: optionBuffers)
    if (dalloc(c, c->fixedAllocs, &c->logicError, 1)) return fail("hipMalloc(logic error flag)", hipErrorOutOfMemory);
    (void)hipMemsetAsync(c->logicError, 0, 4, c->stream);
    (void)hipMemsetAsync(c->blockCounts, 0, (size_t)7 * auxStride * 4, c->stream);      // the pad behind each list's counts stays zero
    (void)hipMemsetAsync(c->queueAux, 0, queueAuxWords * 4, c->stream);                // both totals buffers start at zero; from then on the build kernels keep them so
    { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) c->numCUs = prop.multiProcessorCount; }
    if (dalloc(c, c->fixedAllocs, &c->stats, FLX_NUM_TRACE_STATS)) return fail("hipMalloc(stats)", hipErrorOutOfMemory);
    (void)hipMemsetAsync(c->stats, 0, FLX_NUM_TRACE_STATS * 8, c->stream);
#ifdef FLX_LAB_RSTATS
    flxd::g_lab_rstats = c->stats;
#endif
    // per sub-list: numTasks / 2 (first pass) and / 8 (second pass) records over all lists, whole waves (allocated by optionBuffers)
    c->splitCapA = ((num_tasks / 2 / shadow_split_lists()) + 64u) & ~63u; c->splitCapB = ((num_tasks / 8 / shadow_split_lists()) + 64u) & ~63u;
    if (dalloc(c, c->fixedAllocs, &c->totals, 8)) return fail("hipMalloc(totals)", hipErrorOutOfMemory);
    (void)hipMemsetAsync(c->totals, 0, 64, c->stream);
    if (dalloc(c, c->fixedAllocs, &c->fr.currPixelIdx, 1)) return fail("hipMalloc(cursor)", hipErrorOutOfMemory);
    (void)hipMemsetAsync(c->fr.currPixelIdx, 0, 4, c->stream);
    c->fr.rank = 0; c->fr.nranks = 1; c->fr.localPixels = 0;
    if ((e = hipHostMalloc((void **)&c->pinned, sizeof(flx_queue_counters) * c->pinnedSlots)) != hipSuccess) return fail("hipHostMalloc", e);
    if ((e = hipHostMalloc((void **)&c->pinnedIdx, sizeof(uint32_t) * c->pinnedSlots)) != hipSuccess) return fail("hipHostMalloc", e);
    if ((e = hipHostMalloc((void **)&c->pinnedMk, 16 * c->pinnedSlots)) != hipSuccess) return fail("hipHostMalloc", e);
    // dummy 1x1 black environment map (reference: CLContext::setupScene, src/clcontext.cpp:513-518)
    {
        float4 *rgba; float2 *rec; float *pdf;
        if (dalloc(c, c->envAllocs, &rgba, 1) || dalloc(c, c->envAllocs, &rec, 1) || dalloc(c, c->envAllocs, &pdf, 1))
            return fail("hipMalloc(env)", hipErrorOutOfMemory);
        const float one = 1.0f; const float2 rec1 = make_float2(1.0f, 0.0f /* alias 0 */);
        (void)hipMemsetAsync(rgba, 0, 16, c->stream);
        (void)hipMemcpy(rec, &rec1, 8, hipMemcpyHostToDevice); (void)hipMemcpy(pdf, &one, 4, hipMemcpyHostToDevice);
        c->sc.envRGBA = rgba; c->sc.aliasRec = rec; c->sc.pdfTable = pdf; c->sc.envW = c->sc.envH = 1;
        float4 *nee; if (dalloc(c, c->envAllocs, &nee, 2)) return fail("hipMalloc(env)", hipErrorOutOfMemory);
        launch_env_nee_table(c->stream, c->sc, nee, 1u); c->sc.neeRec = nee;
    }
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return fail("hipStreamSynchronize", e);
    *out = c;
    return 0;
}

int flx_destroy(flx_ctx *c)
{
    if (!c) return 0;
    c->phase = PH_IDLE;                                 // deferred kernels of a context that is going away: dropped
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->comm) { flx_group_destroy(c); }
    c->releaseFrameFeatures(); c->gather.release(); c->ob.release(); c->ml.releaseBuffers();
    freeAll(c->sceneAllocs); freeAll(c->spillAllocs); freeAll(c->envAllocs); freeAll(c->frameAllocs); freeAll(c->aovAllocs); freeAll(c->momAllocs); freeAll(c->fixedAllocs);
    if (c->pinned) (void)hipHostFree(c->pinned);
    if (c->pinnedIdx) (void)hipHostFree(c->pinnedIdx);
    if (c->pinnedMk) (void)hipHostFree(c->pinnedMk);
    for (auto &ev : c->events) { (void)hipEventDestroy(ev.a); (void)hipEventDestroy(ev.b); }
    for (auto e : c->eventPool) (void)hipEventDestroy(e);
    if (c->stream2) { (void)hipStreamSynchronize(c->stream2); (void)hipStreamDestroy(c->stream2); }
    if (c->evPreExt) (void)hipEventDestroy(c->evPreExt);
    if (c->evShadow) (void)hipEventDestroy(c->evShadow);
    if (c->evPostLogic) (void)hipEventDestroy(c->evPostLogic);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return 0;
}

uint32_t flx_num_tasks(flx_ctx *c) { return c->numTasks; }
// (an interop caller enqueues its own work behind ours on this stream: a deferred flx_wf_logic / flx_wf_raygen must be in it by then)
void *flx_stream(flx_ctx *c) { (void)enter(c, CALL_PEEK); return (void *)c->stream; }

int flx_set_params(flx_ctx *c, const void *p240)
{
    ENTER(c, CALL_OBSERVE);
    NEED(c, p240, "flx_set_params: null");
    HIPCHK(c, hipSetDevice(c->device));
    const uint32_t oldW = c->params.width, oldH = c->params.height;
    memcpy(&c->params, p240, sizeof(flx_render_params));   // kernels receive the struct by value at launch = in-order semantics
    NEED(c, c->params.width > 0 && c->params.height > 0, "flx_set_params: zero-sized framebuffer");
    if (c->params.width != oldW || c->params.height != oldH) { c->ad.state.dropped(); c->temporal.state.imageResized(); }      // the list of active pixels and the mark index the old image
    c->haveParams = true;
    if (splitPrepare(c)) return 1;                       // the light decides whether the any-hit launch splits (effectiveSplit)
    return allocFrame(c);
}

int flx_set_partition(flx_ctx *c, uint32_t rank, uint32_t nranks)
{
    ENTER(c, CALL_OBSERVE);
    NEED(c, nranks >= 1 && rank < nranks, "flx_set_partition: bad rank");
    c->fr.rank = rank; c->fr.nranks = nranks;
    c->ad.state.dropped();                               // the list of active pixels indexes the pixels of the old partition
    c->temporal.state.partitionSet();                    // ... and so does the mark of flx_history_mark
    return c->haveParams ? allocFrame(c) : 0;
}
uint32_t flx_local_pixels(flx_ctx *c) { return c->fr.localPixels; }

int flx_get_counters_async(flx_ctx *c, void *out32)
{
    NEED(c, out32, "flx_get_counters_async: null");
    ENTER(c, CALL_QUIET);
    HIPCHK(c, hipSetDevice(c->device));
    flushExt(c);
    if ((int)c->pending.size() >= c->pinnedSlots) { c->err = "too many outstanding counter reads; call flx_finish"; return 1; }
    int slot = c->nextSlot; c->nextSlot = (c->nextSlot + 1) % c->pinnedSlots;
    HIPCHK(c, hipMemcpyAsync(&c->pinned[slot], c->qs.counters, 32, hipMemcpyDeviceToHost, c->stream));
    c->pending.push_back({out32, slot});
    return 0;
}

int flx_finish(flx_ctx *c)
{
    ENTER(c, CALL_QUIET);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->regenUsed) {                                  // a look-back of the fused pass that gave up (logic.hip): fail loudly, never silently wrong pixels
        // (only when a pass with in-kernel regeneration ran since the last check: the default configuration pays no read-back here)
        uint32_t e = 0; HIPCHK(c, hipMemcpy(&e, c->logicError, 4, hipMemcpyDeviceToHost));
        c->regenUsed = false;
        if (e) {                                         // reported ONCE: the flag is cleared, the regenerated paths of that pass are wrong -- the caller resets the renderer
            HIPCHK(c, hipMemset(c->logicError, 0, 4));
            c->err = "k_logic: the in-kernel regeneration's look-back timed out (paths regenerated by that pass are invalid: reset the renderer)"; return 1;
        }
    }
    for (auto &p : c->pending) memcpy(p.user, &c->pinned[p.slot], 32);
    c->pending.clear();
    for (auto &p : c->pendingMk) memcpy(p.first, c->pinnedMk + 4 * p.second, 16);
    c->pendingMk.clear();
    for (auto &ev : c->events) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, ev.a, ev.b) == hipSuccess) { c->kMs[ev.kernel] += ms; c->kLaunches[ev.kernel]++; }
        c->eventPool.push_back(ev.a); c->eventPool.push_back(ev.b);
    }
    c->events.clear();
    return 0;
}

int flx_pixel_index_update(flx_ctx *c, uint32_t npix, uint32_t nnew)
{
    ENTER(c, CALL_NEUTRAL);
    NEED(c, npix > 0, "flx_pixel_index_update: zero pixels");
    HIPCHK(c, hipSetDevice(c->device));
    c->hostPixelIdx = (uint32_t)(((uint64_t)c->hostPixelIdx + nnew) % npix);
    int slot = c->nextIdxSlot; c->nextIdxSlot = (c->nextIdxSlot + 1) % c->pinnedSlots;
    c->pinnedIdx[slot] = c->hostPixelIdx;
    HIPCHK(c, hipMemcpyAsync(c->fr.currPixelIdx, &c->pinnedIdx[slot], 4, hipMemcpyHostToDevice, c->stream));
    return 0;
}
int flx_pixel_index_reset(flx_ctx *c)
{
    ENTER(c, CALL_NEUTRAL);
    HIPCHK(c, hipSetDevice(c->device));
    c->hostPixelIdx = 0;
    HIPCHK(c, hipMemsetAsync(c->fr.currPixelIdx, 0, 4, c->stream));
    return 0;
}

int flx_counter_totals(flx_ctx *c, uint64_t *out8, int reset)
{
    ENTER(c, CALL_QUIET);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(out8, c->totals, 64, hipMemcpyDeviceToHost, c->stream));
    if (reset) HIPCHK(c, hipMemsetAsync(c->totals, 0, 64, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int flx_read_pixels(flx_ctx *c, int which, float *out)
{
    ENTER(c, CALL_NEUTRAL);                                       // framebuffers only
    NEED(c, c->fr.pixels && out, "flx_read_pixels: no framebuffer");
    HIPCHK(c, hipSetDevice(c->device));
    NEED(c, which >= 0 && which <= 7, "flx_read_pixels: which must be 0..7");
    NEED(c, which != 6 || c->dn.have, "flx_read_pixels: which = 6 is the output of flx_denoise (option \"denoiser\" on): none since the buffers were made");
    NEED(c, which != 7 || c->fr.moments, "flx_read_pixels: which = 7 (the luminance moments) needs flx_set_option(ctx, \"moments\", 1)");
    const float *src[8] = {c->fr.pixels, c->fr.preview, c->fr.aovAlbedoOut, c->fr.aovNormalOut, c->fr.aovAlbedo, c->fr.aovNormal, c->dn.out, c->fr.moments};
    NEED(c, src[which], "flx_read_pixels: the denoiser feature buffers need flx_set_option(ctx, \"denoiser\", 1)");
    HIPCHK(c, hipMemcpyAsync(out, src[which], (size_t)c->fr.localPixels * 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
int flx_write_pixels(flx_ctx *c, int which, const float *in)
{
    ENTER(c, CALL_NEUTRAL);                                       // framebuffers only
    NEED(c, c->fr.pixels && in, "flx_write_pixels: no framebuffer");
    HIPCHK(c, hipSetDevice(c->device));
    NEED(c, which == 0 || which == 4 || which == 5 || which == 7, "flx_write_pixels: which must be 0, 4 or 5, or 7 with option \"moments\"");
    NEED(c, which != 7 || c->fr.moments, "flx_write_pixels: which = 7 (the luminance moments) needs flx_set_option(ctx, \"moments\", 1)");
    float *dst = which == 0 ? c->fr.pixels : which == 4 ? c->fr.aovAlbedo : which == 5 ? c->fr.aovNormal : c->fr.moments;
    NEED(c, dst, "flx_write_pixels: the denoiser feature buffers need flx_set_option(ctx, \"denoiser\", 1)");
    HIPCHK(c, hipMemcpyAsync(dst, in, (size_t)c->fr.localPixels * 16, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
int flx_copy_pixels_to_device(flx_ctx *c, void *dst)
{
    ENTER(c, CALL_OBSERVE);
    NEED(c, c->fr.pixels && dst, "flx_copy_pixels_to_device: no framebuffer");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(dst, c->fr.pixels, (size_t)c->fr.localPixels * 16, hipMemcpyDeviceToDevice, c->stream));
    return 0;
}

int flx_set_option(flx_ctx *c, const char *name, int value)
{
    ENTER(c, CALL_PEEK);
    if (name && strcmp(name, "xcd_remap") == 0) { c->xcdRemap = value; return 0; }
    if (name && strcmp(name, "fuse") == 0 && (value == 0 || value == 1)) { c->fuse = value; return 0; }
    if (name && strcmp(name, "ext_order") == 0 && value >= 0 && value <= 2) { c->extOrder = value; return 0; }
    if (name && strcmp(name, "regen") == 0 && (value == 0 || value == 1)) { if (value && optionBuffers(c, true)) return 1; c->regenOpt = value; return 0; }
    if (name && strcmp(name, "regen_prep") == 0 && (value == 0 || value == 1)) { c->prepOpt = value; return 0; }
    // 1: the fused RAW pass leaves the committed hit point / uv record to k_settle_hits | 0: it stores them itself.  (CALL_PEEK above has settled what was pending.)
    if (name && strcmp(name, "lazy_hit_commit") == 0 && (value == 0 || value == 1)) { c->lazyCommitOpt = value; return 0; }
    if (name && strcmp(name, "regroup") == 0 && value >= -1 && value <= 1) { c->regroupOpt = value; c->regroup = value >= 0 ? value : c->regroupAuto; return 0; }
    if (name && strcmp(name, "fuse_set") == 0 && (value == 1 || value == 31)) { c->fuseSet = value; return 0; }
    if (name && strcmp(name, "overlap") == 0 && value >= -1 && value <= 2) { ENTER(c, CALL_OBSERVE); c->overlapOpt = value; pickSchedule(c); return 0; }
    if (name && strcmp(name, "shadow_tree") == 0 && (value == 2 || value == 4)) { ENTER(c, CALL_OBSERVE); c->shadowTree = value; return 0; }
    if (name && strcmp(name, "extend_tree") == 0 && (value == 2 || value == 4)) { ENTER(c, CALL_OBSERVE); c->extendTree = value; return 0; }
    if (name && strcmp(name, "denoiser") == 0 && (value == 0 || value == 1)) {
        ENTER(c, CALL_OBSERVE);
        if (c->denoiser != value) { c->denoiser = value; HIPCHK(c, hipSetDevice(c->device)); HIPCHK(c, hipStreamSynchronize(c->stream)); return allocAov(c); }
        return 0;
    }
    if (name && strcmp(name, "moments") == 0 && (value == 0 || value == 1)) {
        ENTER(c, CALL_OBSERVE);
        if (!value) c->ad.state.dropped();                   // the list of active pixels is derived from the moments
        if (c->moments != value) { c->moments = value; HIPCHK(c, hipSetDevice(c->device)); HIPCHK(c, hipStreamSynchronize(c->stream)); return allocMoments(c); }
        return 0;
    }
    if (name && strcmp(name, "motion_history") == 0 && (value == 0 || value == 1)) {
        ENTER(c, CALL_OBSERVE);
        NEED(c, !value || !c->deformHistory, "flx_set_option: \"motion_history\" cannot be switched on while \"deform_history\" is on (which keeps the history across flx_objects_pose too)");
        if (!value) c->temporal.state.motionHistoryOff();
        c->motionHistory = value;
        return 0;
    }
    if (name && strcmp(name, "deform_history") == 0 && (value == 0 || value == 1)) {     // per-vertex reprojection
        ENTER(c, CALL_OBSERVE);
        NEED(c, !value || !c->motionHistory, "flx_set_option: \"deform_history\" cannot be switched on while \"motion_history\" is on (switch that off: this option follows a pose too)");
        if (!value) c->temporal.state.deformHistoryOff();
        c->deformHistory = value;
        return 0;
    }
    if (name && strcmp(name, "mesh_lights") == 0 && (value == 0 || value == 1)) {        // emissive triangles light the microkernel integrator
        ENTER(c, CALL_OBSERVE);
        c->ml.state.optionSet(value != 0);
        return meshLightsSync(c);                            // switched on over an uploaded scene: the table is built now
    }
    if (name && strcmp(name, "mesh_lights_wavefront") == 0 && (value == 0 || value == 1)) {      // ... and the wavefront integrator; inert without lamps
        ENTER(c, CALL_OBSERVE);                              // a deferred logic pass was deferred under the old setting: it runs first
        c->ml.state.wavefrontSet(value != 0);
        return 0;
    }
    if (name && strcmp(name, "refill_extend") == 0 && refill_value_ok(value)) { ENTER(c, CALL_OBSERVE); c->refillExt = value; return 0; }
    if (name && strcmp(name, "refill_shadow") == 0 && (value == -1 || refill_value_ok(value))) { ENTER(c, CALL_OBSERVE); c->refillShadowOpt = value; pickSchedule(c); return 0; }
    if (name && (strcmp(name, "refill_extend") == 0 || strcmp(name, "refill_shadow") == 0)) { c->err = "flx_set_option: refill value must be 0 or refillMin (1..64) | waitMax (0..64) << 8"; return 1; }
    // (-1 = the library's choice: effectiveSplit.  An explicit value allocates its records now, so that the caller learns here when they do not fit)
    if (name && strcmp(name, "shadow_split") == 0 && (value == -1 || (value >= 0 && (value >> 8) <= 255 && ((value & 0xFF) > 0 || value == 0)))) {
        ENTER(c, CALL_OBSERVE);
        if (value > 0 && splitBuffers(c, (value >> 8) > 0)) return 1;
        c->shadowSplitOpt = value;
        return splitPrepare(c);
    }
    if (name && strcmp(name, "shadow_resume") == 0 && (value == 0 || value == 1)) { ENTER(c, CALL_OBSERVE); c->shadowResume = value; return 0; }
    if (name && strcmp(name, "shadow_split_limit") == 0 && value >= 0) { ENTER(c, CALL_OBSERVE); c->splitLimit = (uint32_t)value; return 0; }
    if (name && strcmp(name, "eager_bump") == 0 && (value == 0 || value == 1)) { c->eagerBump = value; return 0; }
    if (name && strcmp(name, "node_layout") == 0 && (value == 0 || value == 1)) { c->nodeLayout = value; return 0; }
    c->err = std::string("flx_set_option: unknown option ") + (name ? name : "(null)");
    return 1;
}
// the state machine's state as one number (read-only option "phase"; tests/test_gpu_fuzz.py reports which (phase, call) pairs it exercised):
// bits 0-2 enum Phase, bit 3 RAW hit records pending, bit 4 material queues known empty, bit 5 previous hits pending (flx_ctx::prevHitsPending)
static int phaseCode(const flx_ctx *c)
{
    return c->phase | (c->rawHits ? 8 : 0) | (c->matQueuesEmpty ? 16 : 0) | (c->prevHitsPending ? 32 : 0);
}
int flx_get_option(flx_ctx *c, const char *name, int *value)
{
    NEED(c, name && value, "flx_get_option: null");
    const struct { const char *n; int v; } tab[] = {
        {"xcd_remap", c->xcdRemap}, {"fuse", c->fuse}, {"overlap", c->overlap}, {"shadow_tree", c->shadowTree}, {"extend_tree", c->extendTree},
        {"denoiser", c->denoiser}, {"moments", c->moments}, {"motion_history", c->motionHistory}, {"deform_history", c->deformHistory},{"mesh_lights", c->ml.state.on ? 1 : 0}, {"mesh_lights_wavefront", c->ml.state.wavefront ? 1 : 0}, {"eager_bump", c->eagerBump}, {"node_layout", c->nodeLayout}, {"fuse_set", c->fuseSet}, {"ext_order", c->extOrder}, {"regen", c->regenOpt}, {"regroup", c->regroup}, {"regen_prep", c->prepOpt}, {"lazy_hit_commit", c->lazyCommitOpt}, {"refill_extend", c->refillExt}, {"refill_shadow", c->refillShadow}, {"shadow_split", splitNow(c)}, {"shadow_split_fallback", c->splitAllocFailed ? 1 : 0}, {"shadow_resume", c->shadowResume},{"fused_queue_mask", (int)fused_queue_mask(fuseSetNow(c))}, {"fuse_set_now", fuseSetNow(c)}};
    for (const auto &t : tab) if (strcmp(name, t.n) == 0) { *value = t.v; return 0; }
    if (strcmp(name, "phase") == 0) { *value = phaseCode(c); return 0; }
    if (strcmp(name, "wide_far") == 0) { *value = wideFar(c); return 0; }
    if (strcmp(name, "shadow_split_suspended") == 0) {       // rays the last split launch suspended: its counter set, read behind the stream (the main stream has joined the second one)
        ENTER(c, CALL_OBSERVE);
        *value = 0;
        if (!c->splitLaunched) return 0;
        std::vector<uint32_t> host(shadow_split_count_words());
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(host.data(), c->splitCounts, host.size() * 4, hipMemcpyDeviceToHost));
        *value = (int)shadow_split_suspended(host.data(), c->splitParity - 1u, c->splitCapA, c->splitLastLimit);
        return 0;
    }
    c->err = std::string("flx_get_option: unknown option ") + name;
    return 1;
}

} // extern "C"
