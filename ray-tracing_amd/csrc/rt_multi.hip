/*
 * rt_multi.hip — several GPUs: RtMulti (n contexts of one host process with cyclic 8-row strips), its gathers, and rt_gather_rccl
 * for one context per process, with the RCCL loader.  Everything here goes through the contexts' own entry points and the helpers
 * of rt_context.h; the one kernel a gather needs is rt_context.hip's (unpack_strips_enqueue).
 */
#include <hip/hip_runtime.h>

#include <dlfcn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <mutex>
#include <vector>

#include "rt_context.h"
#include "rt_scene_prep.h"

extern "C" {

/* ------------------------------------------------------------------------------------------
 * Several GPUs from one host process: n contexts with cyclic 8-row strips, gather at readback.
 * ---------------------------------------------------------------------------------------- */
struct RtMulti {
    std::vector<RtContext*> ctx;
    /* pinned staging of the gather: every context's packed rows, copied device -> host concurrently */
    void* pinned = nullptr;
    size_t pinnedBytes = 0;
    double lastGatherMs = 0;
    /* peer access between the distinct devices of this multi-context (hipDeviceCanAccessPeer / hipDeviceEnablePeerAccess at
     * creation): peerPairs = ordered pairs of distinct devices, peerEnabled = of those, the pairs with direct access (xGMI or
     * PCIe P2P).  Without it hipMemcpyPeerAsync still works — the runtime stages through host memory — only slower. */
    int peerPairs = 0, peerEnabled = 0;
};

/* launch what every context holds back BEFORE waiting for any of them: a per-context synchronise in a loop would start
 * device i+1's held frames only after device i has finished */
static int multi_flush_all(RtMulti* m)
{
    for (RtContext* c : m->ctx) {
        int rc = rt_flush(c);
        if (rc != RT_OK) return rc;
    }
    return RT_OK;
}

/* wait for whatever the contexts' streams hold (error paths of the gathers: nothing may still be writing into the caller's
 * buffer when an error is returned) */
static void multi_drain(RtMulti* m)
{
    for (RtContext* c : m->ctx) {
        if (hipSetDevice(c->device) != hipSuccess) { (void)hipGetLastError(); continue; }
        (void)hipStreamSynchronize(joined(c));
        (void)hipGetLastError();
    }
}

int rt_create_multi(const int* device_ids, int n_devices, RtMulti** out)
{
    if (!out) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_create_multi: out is null");
    *out = nullptr;
    if (!device_ids || n_devices <= 0) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_create_multi: no devices");
    RtMulti* m = new RtMulti();
    for (int i = 0; i < n_devices; i++) {
        RtContext* c = nullptr;
        int rc = rt_create(device_ids[i], &c);
        if (rc == RT_OK) rc = rt_set_partition(c, 8, i, n_devices);
        if (rc != RT_OK) {
            if (c) rt_destroy(c);
            rt_destroy_multi(m);
            return rc;
        }
        m->ctx.push_back(c);
    }
    /* direct device-to-device copies (scene replication at upload, rt_gather_*_to_device) need peer access enabled in both
     * directions; "already enabled" is fine, "cannot" leaves the pair on the runtime's host-staged path */
    for (int i = 0; i < n_devices; i++)
        for (int j = 0; j < n_devices; j++) {
            const int di = m->ctx[i]->device, dj = m->ctx[j]->device;
            if (di == dj) continue;
            bool seen = false; /* the same pair listed twice (virtual shards on one device list) counts once */
            for (int i2 = 0; i2 < n_devices && !seen; i2++)
                for (int j2 = 0; j2 < n_devices && !seen; j2++)
                    if ((i2 < i || (i2 == i && j2 < j)) && m->ctx[i2]->device == di && m->ctx[j2]->device == dj) seen = true;
            if (seen) continue;
            m->peerPairs++;
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, di, dj) != hipSuccess) { (void)hipGetLastError(); can = 0; }
            if (!can) continue;
            if (hipSetDevice(di) != hipSuccess) { (void)hipGetLastError(); continue; }
            const hipError_t e = hipDeviceEnablePeerAccess(dj, 0);
            if (e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled) m->peerEnabled++;
            (void)hipGetLastError();
        }
    *out = m;
    return RT_OK;
}

/* How device-to-device copies between this multi-context's GPUs travel: 2 = every pair of distinct devices has direct peer access
 * (xGMI / PCIe P2P), 1 = some pairs, 0 = none (the runtime stages through host memory), -1 = one device only (nothing to copy
 * between devices).  *pairs / *enabled (optional) receive the counts. */
int rt_multi_peer_access(const RtMulti* m, int* pairs, int* enabled)
{
    if (!m) return RT_ERR_INVALID_ARG;
    if (pairs) *pairs = m->peerPairs;
    if (enabled) *enabled = m->peerEnabled;
    if (m->peerPairs == 0) return -1;
    return m->peerEnabled == m->peerPairs ? 2 : (m->peerEnabled > 0 ? 1 : 0);
}

void rt_destroy_multi(RtMulti* m)
{
    if (!m) return;
    for (RtContext* c : m->ctx) rt_destroy(c);
    if (m->pinned) hipHostFree(m->pinned);
    delete m;
}

int rt_multi_count(const RtMulti* m) { return m ? (int)m->ctx.size() : 0; }
RtContext* rt_multi_context(RtMulti* m, int i) { return (m && i >= 0 && i < (int)m->ctx.size()) ? m->ctx[i] : nullptr; }

#define RT_MULTI_FORWARD(call)                                                 \
    do {                                                                       \
        if (!m) return fail(nullptr, RT_ERR_INVALID_ARG, "null multi context"); \
        for (RtContext* c : m->ctx) {                                          \
            int rc_ = (call);                                                  \
            if (rc_ != RT_OK) return rc_;                                      \
        }                                                                      \
        return RT_OK;                                                          \
    } while (0)

int rt_multi_resize(RtMulti* m, int width, int height) { RT_MULTI_FORWARD(rt_resize(c, width, height)); }
int rt_multi_upload_scene(RtMulti* m, const RtModel* models, int n_models, const RtTriangle* triangles, int n_triangles,
                          const RtBVHNode* nodes, int n_nodes, const RtSphere* spheres, int n_spheres)
{
    /* validated and re-laid out once; context 0 gets it from the host, the others copy context 0's device arrays
     * (hipMemcpyPeerAsync on their own streams: all destinations at once, over xGMI between different devices) */
    if (!m || m->ctx.empty()) return fail(nullptr, RT_ERR_INVALID_ARG, "null multi context");
    int rc = multi_flush_all(m);
    if (rc) return rc;
    PreparedScene ps;
    RtContext* c0 = m->ctx[0];
    if ((rc = prepare_scene(models, n_models, triangles, n_triangles, nodes, n_nodes, spheres, n_spheres, ps))) return fail(c0, rc, "%s", ps.error.c_str());
    if ((rc = commit_scene(c0, ps, nullptr))) return rc;
    const bool peerCopies = getenv("RT_MULTI_PEER_UPLOAD") == nullptr || atoi(getenv("RT_MULTI_PEER_UPLOAD")) != 0;
    for (size_t i = 1; i < m->ctx.size(); i++) {
        rc = commit_scene(m->ctx[i], ps, peerCopies ? c0 : nullptr);
        if (rc != RT_OK && peerCopies) rc = commit_scene(m->ctx[i], ps, nullptr); /* no peer path between the two: from the host */
        if (rc != RT_OK) return rc;
    }
    for (size_t i = 1; i < m->ctx.size(); i++) { /* the copies read context 0's arrays: done before anyone may replace them */
        RtContext* c = m->ctx[i];
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return RT_OK;
}
int rt_multi_update_models(RtMulti* m, const RtModel* models, int n_models) { RT_MULTI_FORWARD(rt_update_models(c, models, n_models)); }
int rt_multi_update_spheres(RtMulti* m, const RtSphere* spheres, int n_spheres) { RT_MULTI_FORWARD(rt_update_spheres(c, spheres, n_spheres)); }
int rt_multi_set_params(RtMulti* m, const RtParams* params) { RT_MULTI_FORWARD(rt_set_params(c, params)); }
int rt_multi_reset_accumulation(RtMulti* m) { RT_MULTI_FORWARD(rt_reset_accumulation(c)); }
int rt_multi_render_frame(RtMulti* m) { RT_MULTI_FORWARD(rt_render_frame(c)); }
int rt_multi_render_frames(RtMulti* m, int n) { RT_MULTI_FORWARD(rt_render_frames(c, n)); }
int rt_multi_synchronize(RtMulti* m)
{
    if (!m) return fail(nullptr, RT_ERR_INVALID_ARG, "null multi context");
    int rc = multi_flush_all(m);
    if (rc) return rc;
    RT_MULTI_FORWARD(rt_synchronize(c));
}
double rt_multi_last_gather_ms(const RtMulti* m) { return m ? m->lastGatherMs : 0.0; }

static int multi_gather(RtMulti* m, float* rgba, size_t bytes, bool accumulated)
{
    if (!m || m->ctx.empty()) return fail(nullptr, RT_ERR_INVALID_ARG, "null multi context");
    RtContext* c0 = m->ctx[0];
    const int W = c0->W, H = c0->H;
    if (!rgba || bytes != (size_t)W * H * 16) return fail(c0, RT_ERR_INVALID_ARG, "rt_gather: bytes %zu != H*W*16 = %zu", bytes, (size_t)W * H * 16);
    const size_t rowBytes = (size_t)W * 16;
    size_t total = 0;
    for (RtContext* c : m->ctx) {
        if (c->W != W || c->H != H) return fail(c0, RT_ERR_STATE, "rt_gather: contexts disagree on the resolution");
        total += (size_t)c->localRows * rowBytes;
    }
    if (m->pinnedBytes < total) {
        if (m->pinned) hipHostFree(m->pinned);
        m->pinned = nullptr;
        m->pinnedBytes = 0;
        HIP_TRY(c0, hipHostMalloc(&m->pinned, total ? total : 16, hipHostMallocDefault));
        m->pinnedBytes = total;
    }
    /* every device's held frames are launched, then every device's tile is on its way to pinned host memory (each on
     * its own stream and its own link), and only then does the host wait — device by device, scattering the tile that
     * has arrived while the others are still in flight */
    int rc = multi_flush_all(m);
    if (rc) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    size_t off = 0;
    for (RtContext* c : m->ctx) {
        const size_t n = (size_t)c->localRows * rowBytes;
        if (n) {
            const float* src = image_target(c, accumulated);
            hipError_t e = hipSetDevice(c->device);
            if (e == hipSuccess) e = hipMemcpyAsync((char*)m->pinned + off, src, n, hipMemcpyDeviceToHost, joined(c));
            if (e != hipSuccess) { /* copies already enqueued still write into m->pinned: wait for them before handing the error back */
                multi_drain(m);
                return fail(c, RT_ERR_HIP, "rt_gather: %s", hipGetErrorString(e));
            }
        }
        off += n;
    }
    off = 0;
    for (RtContext* c : m->ctx) {
        const int rows = c->localRows;
        const size_t n = (size_t)rows * rowBytes;
        if (!n) continue;
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        flush_timer(c);
        if ((rc = check_watchdog(c, c0, "rt_gather"))) { /* the later contexts' copies still write into m->pinned */
            multi_drain(m);
            return rc;
        }
        /* packed local rows -> their global rows; a strip's rows are contiguous in both */
        for (int l = 0; l < rows;) {
            const int g = rt_local_to_global_row(c, l);
            int run = c->stripRows - (g % c->stripRows);
            if (run > rows - l) run = rows - l;
            memcpy((char*)rgba + (size_t)g * rowBytes, (const char*)m->pinned + off + (size_t)l * rowBytes, (size_t)run * rowBytes);
            l += run;
        }
        off += n;
    }
    m->lastGatherMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return RT_OK;
}
/* The gather with a DEVICE destination: every context's strips go straight into their global rows of an image on the
 * device of context `root` — device-to-device copies on each source context's own stream (ordered after its frames; xGMI
 * between different GPUs, all sources concurrently), no host memory in between.  For hosts that display or post-process on
 * one of the GPUs. */
static int multi_gather_device(RtMulti* m, int root, void* d_rgba, size_t bytes, bool accumulated)
{
    if (!m || m->ctx.empty()) return fail(nullptr, RT_ERR_INVALID_ARG, "null multi context");
    RtContext* c0 = m->ctx[0];
    if (root < 0 || root >= (int)m->ctx.size()) return fail(c0, RT_ERR_INVALID_ARG, "rt_gather_*_to_device: root %d out of range", root);
    const int W = c0->W, H = c0->H;
    if (!d_rgba || bytes != (size_t)W * H * 16) return fail(c0, RT_ERR_INVALID_ARG, "rt_gather_*_to_device: bytes %zu != H*W*16 = %zu", bytes, (size_t)W * H * 16);
    const size_t rowBytes = (size_t)W * 16;
    const int rootDev = m->ctx[root]->device;
    for (RtContext* c : m->ctx) /* before anything is enqueued */
        if (c->W != W || c->H != H) return fail(c0, RT_ERR_STATE, "rt_gather: contexts disagree on the resolution");
    int rc = multi_flush_all(m);
    if (rc) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    for (RtContext* c : m->ctx) {
        const int rows = c->localRows;
        if (!rows) continue;
        const char* src = (const char*)image_target(c, accumulated);
        hipError_t e = hipSetDevice(c->device);
        hipStream_t st = joined(c);
        for (int l = 0; l < rows && e == hipSuccess;) { /* a strip's rows are contiguous in the packed tile and in the image */
            const int g = rt_local_to_global_row(c, l);
            int run = c->stripRows - (g % c->stripRows);
            if (run > rows - l) run = rows - l;
            e = hipMemcpyPeerAsync((char*)d_rgba + (size_t)g * rowBytes, rootDev, src + (size_t)l * rowBytes, c->device, (size_t)run * rowBytes, st);
            l += run;
        }
        if (e != hipSuccess) { /* earlier contexts' copies into the caller's buffer are still in flight: wait before returning */
            multi_drain(m);
            return fail(c, RT_ERR_HIP, "rt_gather_*_to_device: %s", hipGetErrorString(e));
        }
    }
    for (RtContext* c : m->ctx) {
        if (!c->localRows) continue;
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        flush_timer(c);
    }
    for (RtContext* c : m->ctx) /* after every copy into the caller's buffer has completed */
        if (c->localRows && (rc = check_watchdog(c, c0, "rt_gather_*_to_device"))) return rc;
    m->lastGatherMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return RT_OK;
}
int rt_gather_accumulated_to_device(RtMulti* m, int root, void* d_rgba, size_t bytes) { return multi_gather_device(m, root, d_rgba, bytes, true); }
int rt_gather_frame_to_device(RtMulti* m, int root, void* d_rgba, size_t bytes) { return multi_gather_device(m, root, d_rgba, bytes, false); }
int rt_gather_accumulated(RtMulti* m, float* rgba, size_t bytes) { return multi_gather(m, rgba, bytes, true); }
int rt_gather_frame(RtMulti* m, float* rgba, size_t bytes) { return multi_gather(m, rgba, bytes, false); }

/* ---- RCCL, loaded on first use (no link-time dependency): the handful of entry points rt_gather_rccl needs */
namespace {
struct Rccl {
    void* lib = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*Send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*Recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*CommCount)(void*, int*) = nullptr;
    int (*CommUserRank)(void*, int*) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    bool ok = false;
};
Rccl* rccl()
{
    static Rccl r;
    static std::once_flag once;
    std::call_once(once, [] {
        const char* names[] = {getenv("RT_RCCL_LIB"), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        for (const char* n : names) {
            if (!n) continue;
            r.lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
            if (r.lib) break;
        }
        if (!r.lib) return;
        r.GroupStart = (int (*)())dlsym(r.lib, "ncclGroupStart");
        r.GroupEnd = (int (*)())dlsym(r.lib, "ncclGroupEnd");
        r.Send = (int (*)(const void*, size_t, int, int, void*, hipStream_t))dlsym(r.lib, "ncclSend");
        r.Recv = (int (*)(void*, size_t, int, int, void*, hipStream_t))dlsym(r.lib, "ncclRecv");
        r.CommCount = (int (*)(void*, int*))dlsym(r.lib, "ncclCommCount");
        r.CommUserRank = (int (*)(void*, int*))dlsym(r.lib, "ncclCommUserRank");
        r.GetErrorString = (const char* (*)(int))dlsym(r.lib, "ncclGetErrorString");
        r.ok = r.GroupStart && r.GroupEnd && r.Send && r.Recv && r.CommCount && r.CommUserRank;
    });
    return &r;
}
} // namespace

int rt_gather_rccl(RtContext* ctx, void* nccl_comm, int root, int use_accumulated, void* d_rgba, size_t bytes)
{
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    RT_FLUSH(ctx);
    if (!nccl_comm) return fail(ctx, RT_ERR_INVALID_ARG, "rt_gather_rccl: null communicator");
    if (ctx->W == 0) return fail(ctx, RT_ERR_STATE, "rt_gather_rccl before rt_resize");
    Rccl* R = rccl();
    if (!R->ok) return fail(ctx, RT_ERR_STATE, "rt_gather_rccl: librccl.so could not be loaded (%s)", R->lib ? "missing symbols" : "dlopen failed; RT_RCCL_LIB names another path");
    int world = 0, rank = -1;
    if (R->CommCount(nccl_comm, &world) != 0 || R->CommUserRank(nccl_comm, &rank) != 0) return fail(ctx, RT_ERR_INVALID_ARG, "rt_gather_rccl: not a communicator");
    if (world != ctx->partCount || rank != ctx->partIndex)
        return fail(ctx, RT_ERR_STATE, "rt_gather_rccl: communicator rank %d of %d, context partition %d of %d", rank, world, ctx->partIndex, ctx->partCount);
    if (root < 0 || root >= world) return fail(ctx, RT_ERR_INVALID_ARG, "rt_gather_rccl: root %d out of range", root);
    const int W = ctx->W, H = ctx->H;
    const bool isRoot = rank == root;
    /* a collective: what only ONE rank can get wrong must not keep it out of the exchange (its peers would block in ncclSend for ever):
     * a root with a bad destination still receives every tile, and says so afterwards (include/rt_abi.h) */
    const bool badDst = isRoot && (!d_rgba || bytes != (size_t)W * H * 16);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = joined(ctx);
    const float* src = image_target(ctx, use_accumulated);
    /* root: one staging area for every rank's packed tile (H rows in all), then one watchdog word per rank, in the display scratch */
    std::vector<size_t> rowOff(world + 1, 0);
    for (int r = 0; r < world; r++) rowOff[r + 1] = rowOff[r] + (size_t)local_rows_for(H, ctx->stripRows, r, world);
    const size_t tileBytes = rowOff[world] * (size_t)W * 16;
    char* staging = nullptr;
    unsigned long long* flags = nullptr;
    if (isRoot) {
        const int rc = grow_scratch(ctx, &ctx->dDisplay, &ctx->displayBytes, tileBytes + (size_t)world * sizeof(unsigned long long));
        if (rc) return rc;
        staging = (char*)ctx->dDisplay;
        flags = (unsigned long long*)(staging + tileBytes);
    }
    auto check = [&](int e, const char* what) -> int {
        if (e == 0) return RT_OK;
        return fail(ctx, RT_ERR_HIP, "rt_gather_rccl: %s: %s", what, R->GetErrorString ? R->GetErrorString(e) : "RCCL error");
    };
    /* every rank sends its tile to root, root receives from every rank — its own included, so that a one-rank communicator runs the
     * same code; one group: the transfers progress together.  Behind its tile each rank sends its watchdog word (a tripped rank still
     * takes part in the exchange: the root learns of it and fails) */
    int rc = check(R->GroupStart(), "ncclGroupStart");
    if (rc) return rc;
    int e = 0;
    if (ctx->localRows) e = R->Send(src, (size_t)ctx->localRows * W * 4, /*ncclFloat32*/ 7, root, nccl_comm, st);
    if (e == 0) e = R->Send(ctx->dCounters + kWatchdogWord, 1, /*ncclUint64*/ 5, root, nccl_comm, st);
    if (isRoot)
        for (int r = 0; r < world && e == 0; r++) {
            const size_t rows = rowOff[r + 1] - rowOff[r];
            if (rows) e = R->Recv(staging + rowOff[r] * (size_t)W * 16, rows * W * 4, 7, r, nccl_comm, st);
            if (e == 0) e = R->Recv(flags + r, 1, 5, r, nccl_comm, st);
        }
    const int eEnd = R->GroupEnd();
    if ((rc = check(e, "ncclSend / ncclRecv"))) return rc;
    if ((rc = check(eEnd, "ncclGroupEnd"))) return rc;
    if (isRoot && !badDst)
        for (int r = 0; r < world; r++) {
            const int rows = (int)(rowOff[r + 1] - rowOff[r]);
            if (!rows) continue;
            HIP_TRY(ctx, unpack_strips_enqueue(ctx, st, staging + rowOff[r] * (size_t)W * 16, d_rgba, W, rows, ctx->stripRows, r, world));
        }
    HIP_TRY(ctx, hipStreamSynchronize(st));
    flush_timer(ctx);
    if ((rc = check_watchdog(ctx, ctx, "rt_gather_rccl"))) return rc;
    if (isRoot) {
        std::vector<unsigned long long> fired(world);
        HIP_TRY(ctx, hipMemcpy(fired.data(), flags, (size_t)world * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (int r = 0; r < world; r++)
            if (fired[r]) {
                char what[64];
                snprintf(what, sizeof(what), "rt_gather_rccl (rank %d of %d)", r, world);
                return watchdog_failure(ctx, what, fired[r]);
            }
    }
    if (badDst) return fail(ctx, RT_ERR_INVALID_ARG, "rt_gather_rccl: bytes %zu != H*W*16 = %zu (the tiles were received and dropped)", bytes, (size_t)W * H * 16);
    return RT_OK;
}

int rt_debug_multi_pending_frames(const RtMulti* m)
{
    if (!m) return RT_ERR_INVALID_ARG;
    int most = 0;
    for (const RtContext* c : m->ctx) most = c->pending > most ? c->pending : most;
    return most;
}

int rt_multi_get_counters(RtMulti* m, RtCounters* out)
{
    if (!m || !out) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_multi_get_counters: null argument");
    memset(out, 0, sizeof(*out));
    {
        int rc = multi_flush_all(m);
        if (rc) return rc;
    }
    for (size_t i = 0; i < m->ctx.size(); i++) {
        RtContext* c = m->ctx[i];
        RtCounters k;
        int rc = rt_get_counters(c, &k);
        if (rc != RT_OK) return i == 0 ? rc : fail(m->ctx[0], rc, "context %zu: %s", i, c->err); /* read through context 0 */
        out->segments += k.segments; out->innerSteps += k.innerSteps; out->leafSteps += k.leafSteps; out->triTests += k.triTests;
        out->sphereTests += k.sphereTests; out->modelVisits += k.modelVisits; out->pixelFrames += k.pixelFrames;
        if (k.gpuMs > out->gpuMs) out->gpuMs = k.gpuMs;
    }
    return RT_OK;
}

} /* extern "C" */
