// api_hooks.hip -- measurement (per-kernel timings, traversal statistics, scene figures) and the test hooks that read or write device state
// behind the renderer's back (path state, queues, counters, the NEE table, the math probe).
#include "flx_ctx.h"
#include <cstring>

extern "C" {

// ---- measurement
int flx_profile_enable(flx_ctx *c, int on) { ENTER(c, CALL_QUIET); c->profile = on < 0 ? 0 : on > 4 ? 1 : on; return 0; }
int flx_profile_get(flx_ctx *c, int k, double *ms, uint64_t *n) { NEED(c, k >= 0 && k < FLX_K_COUNT, "bad kernel id"); *ms = c->kMs[k]; *n = c->kLaunches[k]; return 0; }
int flx_profile_reset(flx_ctx *c) { for (int k = 0; k < FLX_K_COUNT; k++) { c->kMs[k] = 0; c->kLaunches[k] = 0; } return 0; }
int flx_trace_stats_enable(flx_ctx *c, int on) { ENTER(c, CALL_PEEK); c->statsOn = on != 0; return 0; }
static int traceStatsRead(flx_ctx *c, uint64_t *out, size_t bytes)
{
    ENTER(c, CALL_PEEK);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(out, c->stats, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
int flx_trace_stats_get(flx_ctx *c, uint64_t *out7) { return traceStatsRead(c, out7, 56); }
int flx_trace_stats_get_ex(flx_ctx *c, uint64_t *out16) { return traceStatsRead(c, out16, 128); }
int flx_trace_stats_get_all(flx_ctx *c, uint64_t *out24) { return traceStatsRead(c, out24, FLX_NUM_TRACE_STATS * 8); }
int flx_trace_stats_reset(flx_ctx *c) { ENTER(c, CALL_OBSERVE); HIPCHK(c, hipSetDevice(c->device)); HIPCHK(c, hipMemsetAsync(c->stats, 0, FLX_NUM_TRACE_STATS * 8, c->stream)); return 0; }
int flx_scene_info(flx_ctx *c, uint32_t *out8) { NEED(c, out8, "flx_scene_info: null"); memcpy(out8, c->wideInfo, 32); return 0; }

// ---- test hooks
int flx_state_export(flx_ctx *c, float *out)
{
    ENTER(c, CALL_OBSERVE);
    HIPCHK(c, hipSetDevice(c->device));
    float *d = nullptr; size_t bytes = (size_t)FLX_NUM_COLS * c->numTasks * 4;
    HIPCHK(c, hipMalloc((void **)&d, bytes));
    launch_state_export(c->stream, c->st, d, c->haveParams ? 2.0f * c->params.worldRadius : 0.0f);
    hipError_t e = hipMemcpyAsync(out, d, bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d);
    HIPCHK(c, e);
    return 0;
}
int flx_state_import(flx_ctx *c, const float *in)
{
    ENTER(c, CALL_OBSERVE);
    HIPCHK(c, hipSetDevice(c->device));
    float *d = nullptr; size_t bytes = (size_t)FLX_NUM_COLS * c->numTasks * 4;
    HIPCHK(c, hipMalloc((void **)&d, bytes));
    hipError_t e = hipMemcpyAsync(d, in, bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) { launch_state_import(c->stream, c->st, d); e = hipStreamSynchronize(c->stream); }
    (void)hipFree(d);
    HIPCHK(c, e);
    return 0;
}
int flx_env_sample_table(flx_ctx *c, float *out)
{
    ENTER(c, CALL_QUIET);
    NEED(c, out, "flx_env_sample_table: null");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, c->sc.neeRec, (size_t)c->sc.envW * c->sc.envH * 32, hipMemcpyDeviceToHost));
    return 0;
}
int flx_math_probe(flx_ctx *c, int fn, const float *a, const float *b, uint32_t n, uint32_t *out_bits)
{
    ENTER(c, CALL_OBSERVE);
    NEED(c, a && b && out_bits && n && fn >= 0 && fn <= 15, "flx_math_probe: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    float *d = nullptr;
    HIPCHK(c, hipMalloc((void **)&d, (size_t)n * 12));
    hipError_t e = hipMemcpyAsync(d, a, (size_t)n * 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d + n, b, (size_t)n * 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) { launch_math_probe(c->stream, fn, d, d + n, n, reinterpret_cast<uint32_t *>(d + 2 * (size_t)n)); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipMemcpyAsync(out_bits, d + 2 * (size_t)n, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d);
    HIPCHK(c, e);
    return 0;
}
int flx_queue_read(flx_ctx *c, int q, uint32_t *out)
{
    NEED(c, q >= 0 && q < FLX_NUM_QUEUES, "bad queue id");
    ENTER(c, CALL_PEEK);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(out, c->qs.q[q], (size_t)c->numTasks * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
int flx_queue_write(flx_ctx *c, int q, const uint32_t *in, uint32_t n)
{
    ENTER(c, CALL_OBSERVE);
    NEED(c, q >= 0 && q < FLX_NUM_QUEUES && n <= c->numTasks, "bad queue id / length");
    HIPCHK(c, hipSetDevice(c->device));
    if (n) HIPCHK(c, hipMemcpyAsync(c->qs.q[q], in, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
int flx_set_counters(flx_ctx *c, const void *in32)
{
    ENTER(c, CALL_OBSERVE);
    c->qs.extPend = 0;                                  // the caller's counters are complete
    c->matQueuesEmpty = false; c->raygenQueueEmpty = false;   // ... and unknown here
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(c->qs.counters, in32, 32, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

} // extern "C"
