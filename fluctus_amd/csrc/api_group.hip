// api_group.hip -- the multi-GPU group: librccl bound with dlopen, flx_group_*, flx_gather and flx_gather_local.
#include "flx_ctx.h"
#include <cstring>
#include <cstdlib>
#include <dlfcn.h>

extern "C" {

// ---- multi-GPU group: RCCL gather of the per-rank radiance tiles (SURVEY 8(b) flx_create_group / flx_gather, 8(e)).
// The reference is single-device (one cl::CommandQueue, src/clcontext.cpp:25-29).  Rank r renders global pixels p * R + r
// (flx_set_partition); at read-back every rank sends its compact float4[localPixels] accumulation tile to the root over
// RCCL point-to-point (grouped ncclSend / ncclRecv = a gather; xGMI links into the root work in parallel), the root
// de-interleaves into the full image.  Nothing is exchanged per iteration.
namespace {
struct Rccl {
    void *dl = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    decltype(&ncclCommCount) CommCount = nullptr;
    decltype(&ncclCommUserRank) CommUserRank = nullptr;
    decltype(&ncclCommAbort) CommAbort = nullptr;
    std::string err;
};
Rccl g_rccl;
// TEST HOOK: FLX_RCCL_LIB is honoured only together with FLX_ALLOW_RCCL_OVERRIDE=1, so that a stray variable in a production
// environment cannot make the library dlopen an arbitrary path or change which gather path a local group takes.
const char *rccl_override()
{
    const char *over = getenv("FLX_RCCL_LIB"), *allow = getenv("FLX_ALLOW_RCCL_OVERRIDE");
    return (over && *over && allow && strcmp(allow, "1") == 0) ? over : nullptr;
}
bool rccl_load()
{
    if (g_rccl.dl) return true;
    // FLX_RCCL_LIB=<path> + FLX_ALLOW_RCCL_OVERRIDE=1: bind another library with the same entry points (tests/fake_rccl.cpp moves the tiles
    // between host threads on ONE device, so that the N > 1 send / receive code below runs on a 1-GPU box; never set in production)
    void *dl = nullptr;
    const char *over = rccl_override();
    if (over) {
        dl = dlopen(over, RTLD_NOW | RTLD_LOCAL);
        if (!dl) { g_rccl.err = std::string("FLX_RCCL_LIB=") + over + " not loadable: " + dlerror(); return false; }
    }
    if (!dl) dl = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!dl) dl = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!dl) dl = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!dl) { g_rccl.err = std::string("librccl.so.1 not loadable: ") + dlerror(); return false; }
#define RSYM(field, name) g_rccl.field = (decltype(g_rccl.field))dlsym(dl, #name); if (!g_rccl.field) { g_rccl.err = "librccl: missing symbol " #name; dlclose(dl); return false; }
    RSYM(GetUniqueId, ncclGetUniqueId) RSYM(CommInitRank, ncclCommInitRank) RSYM(CommInitAll, ncclCommInitAll) RSYM(CommDestroy, ncclCommDestroy)
    RSYM(Send, ncclSend) RSYM(Recv, ncclRecv) RSYM(GroupStart, ncclGroupStart) RSYM(GroupEnd, ncclGroupEnd) RSYM(GetErrorString, ncclGetErrorString)
    RSYM(CommCount, ncclCommCount) RSYM(CommUserRank, ncclCommUserRank) RSYM(CommAbort, ncclCommAbort)
#undef RSYM
    g_rccl.dl = dl;
    return true;
}
}
#define NCCLCHK(c, expr) do { ncclResult_t r_ = (expr); if (r_ != ncclSuccess) { (c)->err = std::string(#expr) + ": " + g_rccl.GetErrorString(r_); return 1; } } while (0)

static uint32_t tilePixels(uint32_t npix, uint32_t rank, uint32_t nranks) { return npix <= rank ? 0u : (npix - rank + nranks - 1) / nranks; }

int flx_group_unique_id(void *out128)
{
    if (!out128 || !rccl_load()) { g_create_error = out128 ? g_rccl.err : "flx_group_unique_id: null"; return 1; }
    ncclUniqueId id;
    ncclResult_t r = g_rccl.GetUniqueId(&id);
    if (r != ncclSuccess) { g_create_error = std::string("ncclGetUniqueId: ") + g_rccl.GetErrorString(r); return 1; }
    static_assert(sizeof(ncclUniqueId) == FLX_GROUP_ID_BYTES, "ncclUniqueId size");
    memcpy(out128, &id, sizeof(id));
    return 0;
}

int flx_group_destroy(flx_ctx *c)
{
    if (c->comm && g_rccl.dl) { (void)hipSetDevice(c->device); (void)g_rccl.CommDestroy(c->comm); }
    c->comm = nullptr; c->commShared = false;
    return 0;
}

static int gatherBuffers(flx_ctx *root, uint32_t nranks);

// Calls between ncclGroupStart and ncclGroupEnd: remember the first failure and keep going, so that the group is ALWAYS closed
// (returning with it open would leave every later collective of the process inside a dangling group).
struct NcclGroup {
    ncclResult_t first = ncclSuccess; const char *what = nullptr;
    void operator()(ncclResult_t r, const char *w) { if (r != ncclSuccess && first == ncclSuccess) { first = r; what = w; } }
    int fail(flx_ctx *c) const { if (first == ncclSuccess) return 0; c->err = std::string(what) + ": " + g_rccl.GetErrorString(first); return 1; }
};
#define NCCLTRY(g, expr) (g)((expr), #expr)

// a rank that cannot take part in a collective its peers have already entered tears the communicator down, so that they fail
// instead of waiting for it forever
static void abortGroup(flx_ctx *c) { if (c->comm && g_rccl.dl) { (void)hipSetDevice(c->device); (void)g_rccl.CommAbort(c->comm); } c->comm = nullptr; }

int flx_group_init(flx_ctx *c, uint32_t rank, uint32_t nranks, const void *id128)
{
    ENTER(c, CALL_OBSERVE);
    NEED(c, id128 && nranks >= 1 && rank < nranks, "flx_group_init: bad arguments");
    NEED(c, rccl_load(), g_rccl.err);
    HIPCHK(c, hipSetDevice(c->device));
    flx_group_destroy(c);
    ncclUniqueId id; memcpy(&id, id128, sizeof(id));
    NCCLCHK(c, g_rccl.CommInitRank(&c->comm, (int)nranks, id, (int)rank));
    if (flx_set_partition(c, rank, nranks)) return 1;
    // Any rank may be asked to be the root of flx_gather: its staging buffers are allocated HERE, where every rank allocates the same
    // amount and an out-of-memory condition is an error of this call on every rank alike -- not inside the collective, where a root
    // that fails before posting its receives would leave the peers blocked in ncclSend.  (A later flx_set_params with a larger frame
    // re-allocates in flx_gather; if THAT fails the root aborts the communicator.)
    if (c->haveParams && gatherBuffers(c, nranks)) return 1;
    return 0;
}

int flx_group_info(flx_ctx *c, uint32_t *out2)
{
    NEED(c, out2, "flx_group_info: null");
    out2[0] = out2[1] = 0;
    if (c->commShared) { out2[0] = c->fr.nranks; out2[1] = c->fr.rank; return 0; }
    NEED(c, c->comm, "flx_group_info: no group");
    int n = 0, r = 0;
    NCCLCHK(c, g_rccl.CommCount(c->comm, &n));
    NCCLCHK(c, g_rccl.CommUserRank(c->comm, &r));
    out2[0] = (uint32_t)n; out2[1] = (uint32_t)r;
    return 0;
}

int flx_group_init_local(flx_ctx **ctxs, uint32_t n)
{
    if (!ctxs || !n || !ctxs[0]) { g_create_error = "flx_group_init_local: bad arguments"; return 1; }
    flx_ctx *c0 = ctxs[0];
    bool distinct = true;
    for (uint32_t i = 0; i < n; i++) { NEED(c0, ctxs[i], "flx_group_init_local: null context"); for (uint32_t j = 0; j < i; j++) if (ctxs[i]->device == ctxs[j]->device) distinct = false; }
    for (uint32_t i = 0; i < n; i++) { ENTER(ctxs[i], CALL_OBSERVE); flx_group_destroy(ctxs[i]); }
    // (with a stand-in transport bound through FLX_RCCL_LIB the communicator path is taken whatever the devices are: tests)
    if (rccl_override()) distinct = true;
    if (distinct) {
        NEED(c0, rccl_load(), g_rccl.err);
        std::vector<ncclComm_t> comms(n); std::vector<int> devs(n);
        for (uint32_t i = 0; i < n; i++) devs[i] = ctxs[i]->device;
        NCCLCHK(c0, g_rccl.CommInitAll(comms.data(), (int)n, devs.data()));
        for (uint32_t i = 0; i < n; i++) ctxs[i]->comm = comms[i];
    } else {
        // several contexts on one device (a 1-GPU box standing in for N ranks: tests): RCCL refuses duplicate devices, the tiles
        // travel with device-to-device copies instead; partition, staging and de-interleave are the same code
        for (uint32_t i = 0; i < n; i++) ctxs[i]->commShared = true;
    }
    for (uint32_t i = 0; i < n; i++) if (flx_set_partition(ctxs[i], i, n)) { if (ctxs[i] != c0) c0->err = ctxs[i]->err; return 1; }
    return 0;
}

static int gatherBuffers(flx_ctx *root, uint32_t nranks)
{
    const uint32_t npix = root->params.width * root->params.height;
    const size_t maxlp = tilePixels(npix, 0, nranks);
    const size_t needStage = (size_t)nranks * maxlp * 4, needFull = (size_t)npix * 4;
    if (needStage > root->gather.stageFloats || needFull > root->gather.fullFloats) {
        HIPCHK(root, hipStreamSynchronize(root->stream));
        root->gather.release();
        if (dalloc(root, root->gather.allocs, &root->gather.stage, needStage) || dalloc(root, root->gather.allocs, &root->gather.full, needFull)) return 1;
        root->gather.stageFloats = needStage; root->gather.fullFloats = needFull;
    }
    return 0;
}

static int gatherFinish(flx_ctx *root, uint32_t nranks, float *out_host)
{
    const uint32_t npix = root->params.width * root->params.height;
    launch_deinterleave(root->stream, root->gather.stage, root->gather.full, npix, nranks, tilePixels(npix, 0, nranks));
    LAUNCHED(root);
    HIPCHK(root, hipMemcpyAsync(out_host, root->gather.full, (size_t)npix * 16, hipMemcpyDeviceToHost, root->stream));
    HIPCHK(root, hipStreamSynchronize(root->stream));
    return 0;
}

// multi-process: every rank of the communicator calls this; out_host (width*height float4) is written on `root` only.
// Error paths: argument errors that every rank sees alike (no group, no frame, root out of range) return before anything is posted.
// Past that point the peers are, or soon will be, blocked in their ncclSend, so the root either posts every matching receive
// (also when its own output pointer is null: the tiles are received and the error reported afterwards) or aborts the communicator.
int flx_gather(flx_ctx *c, uint32_t root, float *out_host)
{
    ENTER(c, CALL_OBSERVE);
    NEED(c, c->comm, "flx_gather: no group (flx_group_init first)");
    NEED(c, c->fr.pixels && c->haveParams, "flx_gather: no framebuffer");
    const uint32_t R = c->fr.nranks, me = c->fr.rank, npix = c->params.width * c->params.height;
    NEED(c, root < R, "flx_gather: bad root");
    HIPCHK(c, hipSetDevice(c->device));
    if (me != root) {
        NcclGroup g;
        NCCLTRY(g, g_rccl.GroupStart());
        NCCLTRY(g, g_rccl.Send(c->fr.pixels, (size_t)tilePixels(npix, me, R) * 4, ncclFloat32, (int)root, c->comm, c->stream));
        NCCLTRY(g, g_rccl.GroupEnd());
        if (g.fail(c)) return 1;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return 0;
    }
    if (gatherBuffers(c, R)) { const std::string why = c->err; abortGroup(c); c->err = "flx_gather: root cannot allocate its staging buffers (" + why + "); communicator aborted"; return 1; }
    const size_t maxlp = tilePixels(npix, 0, R);
    NcclGroup g;
    NCCLTRY(g, g_rccl.GroupStart());
    for (uint32_t r = 0; r < R; r++) {
        if (r == me) continue;
        NCCLTRY(g, g_rccl.Recv(c->gather.stage + (size_t)r * maxlp * 4, (size_t)tilePixels(npix, r, R) * 4, ncclFloat32, (int)r, c->comm, c->stream));
    }
    NCCLTRY(g, g_rccl.GroupEnd());
    if (g.fail(c)) return 1;
    HIPCHK(c, hipMemcpyAsync(c->gather.stage + (size_t)me * maxlp * 4, c->fr.pixels, (size_t)c->fr.localPixels * 16, hipMemcpyDeviceToDevice, c->stream));
    if (!out_host) { HIPCHK(c, hipStreamSynchronize(c->stream)); c->err = "flx_gather: null output on the root (the tiles were received and dropped)"; return 1; }
    return gatherFinish(c, R, out_host);
}

// single process: the n contexts of flx_group_init_local, driven by one host thread
int flx_gather_local(flx_ctx **ctxs, uint32_t n, uint32_t root, float *out_host)
{
    if (!ctxs || !n || root >= n || !ctxs[root]) { g_create_error = "flx_gather_local: bad arguments"; return 1; }
    flx_ctx *rc = ctxs[root];
    NEED(rc, out_host, "flx_gather_local: null output");
    for (uint32_t i = 0; i < n; i++) {
        ENTER(ctxs[i], CALL_OBSERVE);
        NEED(rc, ctxs[i]->fr.nranks == n && ctxs[i]->fr.rank == i && ctxs[i]->fr.pixels && ctxs[i]->haveParams, "flx_gather_local: contexts are not the group of flx_group_init_local");
        NEED(rc, (ctxs[i]->comm != nullptr) != ctxs[i]->commShared, "flx_gather_local: no group (flx_group_init_local first)");
    }
    HIPCHK(rc, hipSetDevice(rc->device));
    if (gatherBuffers(rc, n)) return 1;                                 // nothing posted yet: a plain error
    const uint32_t npix = rc->params.width * rc->params.height;
    const size_t maxlp = tilePixels(npix, 0, n);
    if (rc->comm) {
        NcclGroup g; hipError_t he = hipSuccess;
        NCCLTRY(g, g_rccl.GroupStart());
        for (uint32_t r = 0; r < n && he == hipSuccess; r++) {
            if (r == root) continue;
            if ((he = hipSetDevice(ctxs[r]->device)) != hipSuccess) break;
            NCCLTRY(g, g_rccl.Send(ctxs[r]->fr.pixels, (size_t)ctxs[r]->fr.localPixels * 4, ncclFloat32, (int)root, ctxs[r]->comm, ctxs[r]->stream));
            if ((he = hipSetDevice(rc->device)) != hipSuccess) break;
            NCCLTRY(g, g_rccl.Recv(rc->gather.stage + (size_t)r * maxlp * 4, (size_t)ctxs[r]->fr.localPixels * 4, ncclFloat32, (int)r, rc->comm, rc->stream));
        }
        NCCLTRY(g, g_rccl.GroupEnd());                                  // always closed, whatever happened above
        (void)hipSetDevice(rc->device);
        if (he != hipSuccess) { rc->err = std::string("flx_gather_local: hipSetDevice: ") + hipGetErrorString(he); return 1; }
        if (g.fail(rc)) return 1;
        for (uint32_t r = 0; r < n; r++) if (r != root) { HIPCHK(rc, hipSetDevice(ctxs[r]->device)); HIPCHK(rc, hipStreamSynchronize(ctxs[r]->stream)); }
        HIPCHK(rc, hipSetDevice(rc->device));
    } else {
        for (uint32_t r = 0; r < n; r++) {
            if (r == root) continue;
            HIPCHK(rc, hipStreamSynchronize(ctxs[r]->stream));           // the tile is complete
            HIPCHK(rc, hipMemcpyAsync(rc->gather.stage + (size_t)r * maxlp * 4, ctxs[r]->fr.pixels, (size_t)ctxs[r]->fr.localPixels * 16, hipMemcpyDeviceToDevice, rc->stream));
        }
    }
    HIPCHK(rc, hipMemcpyAsync(rc->gather.stage + (size_t)root * maxlp * 4, rc->fr.pixels, (size_t)rc->fr.localPixels * 16, hipMemcpyDeviceToDevice, rc->stream));
    return gatherFinish(rc, n, out_host);
}

} // extern "C"
