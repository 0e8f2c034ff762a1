// C ABI of libpccm.so (include/pccm.h): context, ingest, nn dispatch, getters, reductions,
// profiling.  Host-side only; kernels live in pccm_brute.hip / pccm_grid.hip / pccm_point.hip.
#include <cxxabi.h>
#include <dlfcn.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <chrono>
#include <new>
#include <thread>
#include <type_traits>

#include "pccm_stale.h"

namespace pccm {

static thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int ensure(pccm_ctx *ctx, DevBuf &b, size_t bytes)
{
    if (bytes <= b.bytes && b.p) return PCCM_OK;
    if (ctx->capturing) {
        ctx->capture_failed = true;
        return fail(PCCM_E_STATE, "a buffer must grow during graph capture: run the same call sequence once before capturing");
    }
    ctx->epoch++;
    if (b.p) {
        PCCM_HIP(hipStreamSynchronize(ctx->stream));
        PCCM_HIP(hipFree(b.p));
        b.p = nullptr;
        b.bytes = 0;
    }
    size_t want = bytes < 256 ? 256 : bytes;
    PCCM_HIP(hipMalloc(&b.p, want));
    b.bytes = want;
    return PCCM_OK;
}

int grow(void **p, size_t &cap, size_t bytes)
{
    if (*p && cap >= bytes) return PCCM_OK;
    if (*p) {
        (void)hipFree(*p);
        *p = nullptr;
        cap = 0;
    }
    PCCM_HIP(hipMalloc(p, bytes ? bytes : 1));
    cap = bytes;
    return PCCM_OK;
}

// Called behind a wait for the GPU by everything that hands results out: a kernel that met a state it cannot be in has set a
// bit of the context's error word instead of answering wrongly.  The word is cleared when reported; the results are not usable.
int check_device_errors(pccm_ctx *ctx)
{
    if (!ctx->host_err) return PCCM_OK;
    const uint32_t e = __atomic_exchange_n(ctx->host_err, 0u, __ATOMIC_RELAXED);
    if (!e) return PCCM_OK;
    results_dropped(ctx);
    return fail(PCCM_E_STATE, "a search kernel reported an inconsistent state (device error word 0x%x: %s%s%s%s): the results of this search were "
                              "dropped, run it again", e, (e & 1u) ? "the tail launch's wait for its own workgroups ran out; " : "",
                (e & 2u) ? "a voxel brick contradicts its cell start; " : "", (e & kErrMergeTable) ? "the duplicate table overflowed; " : "",
                (e & 8u) ? "a filed tail list overflowed or a filed query was not settled within three rings" : "");
}

static hipEvent_t take_event(pccm_ctx *ctx)
{
    if (!ctx->event_pool.empty()) {
        hipEvent_t e = ctx->event_pool.back();
        ctx->event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

ProfScope::ProfScope(pccm_ctx *c, int k) : ctx(c), cls(k)
{
    // not while capturing: on ROCm 7.2 event-record nodes replayed by a hipGraph return meaningless
    // (negative) elapsed times, so kernels are timed in eager launches only
    if (!ctx->prof_on || ctx->capturing) return;
    a = take_event(ctx);
    b = take_event(ctx);
    if (a) (void)hipEventRecord(a, ctx->stream);
}

ProfScope::~ProfScope()
{
    if (!ctx->prof_on || ctx->capturing || !a || !b) return;
    (void)hipEventRecord(b, ctx->stream);
    ctx->spans.push_back({a, b, cls});
}

static int collect_spans(pccm_ctx *ctx)
{
    if (ctx->spans.empty()) return PCCM_OK;
    PCCM_HIP(hipStreamSynchronize(ctx->stream));
    for (auto &s : ctx->spans) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) {
            ctx->prof_ms[s.cls] += ms;
            ctx->prof_n[s.cls] += 1;
        }
        ctx->event_pool.push_back(s.a);
        ctx->event_pool.push_back(s.b);
    }
    ctx->spans.clear();
    return PCCM_OK;
}

static void free_buf(DevBuf &b)
{
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.bytes = 0;
}

static void free_cloud(Cloud &c)
{
    for (void **p : {(void **)&c.xyz32, (void **)&c.xyz64, (void **)&c.xyz32r, (void **)&c.nrm64, (void **)&c.nrm32, (void **)&c.rgb64,
                     (void **)&c.rgb8, (void **)&c.sp, (void **)&c.ssim64, (void **)&c.res64, (void **)&c.refl64}) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
    c.cap32 = c.cap64 = c.cap32r = c.cap_nrm = c.cap_nrm32 = c.cap_rgb = c.cap_rgb8 = c.cap_sp = c.cap_ssim = c.cap_res = c.cap_refl = 0;
    drop_cloud(c);
}

static void free_nn(NNResult &r)
{
    free_buf(r.flagged);
    free_buf(r.flag_thr);
    free_buf(r.tail);
    free_buf(r.rec);
    r.form = NNForm{};
    if (r.idx) (void)hipFree(r.idx);
    if (r.d2) (void)hipFree(r.d2);
    r.idx = nullptr;
    r.d2 = nullptr;
    r.cap = 0;
}

static int dir_clouds(pccm_ctx *ctx, int dir, const Cloud **it, const Cloud **se)
{
    if (dir == PCCM_DIR_LEFT) { *it = &ctx->cloud[0]; *se = &ctx->cloud[1]; }
    else if (dir == PCCM_DIR_RIGHT) { *it = &ctx->cloud[1]; *se = &ctx->cloud[0]; }
    else if (dir == PCCM_DIR_SELF) { *it = &ctx->cloud[0]; *se = &ctx->cloud[0]; }
    else return fail(PCCM_E_ARG, "bad direction %d", dir);
    if ((*it)->n <= 0 || (*se)->n <= 0) return fail(PCCM_E_STATE, "clouds are not set");
    return PCCM_OK;
}

// ---- transfers between caller memory and the device ---------------------------------------------------------------------------
// A copy on a few host threads (one thread moves ~10 GB/s, the link 50)
static void host_copy(void *dst, const void *src, size_t bytes)
{
    constexpr size_t kPiece = 1u << 20;
    const int nt = bytes >= 8 * kPiece ? 4 : bytes >= 2 * kPiece ? 2 : 1;
    if (nt == 1) {
        memcpy(dst, src, bytes);
        return;
    }
    std::thread th[3];
    const size_t part = (bytes / nt + 63) & ~(size_t)63;
    for (int k = 1; k < nt; ++k) {
        const size_t off = (size_t)k * part, len = k + 1 < nt ? part : bytes - off;
        th[k - 1] = std::thread([=] { memcpy((char *)dst + off, (const char *)src + off, len); });
    }
    memcpy(dst, src, part);
    for (int k = 1; k < nt; ++k) th[k - 1].join();
}

static int pin_ensure(pccm_ctx *ctx, int which, size_t bytes)
{
    if (ctx->pin_cap[which] >= bytes) return PCCM_OK;
    if (ctx->pin[which]) {
        PCCM_HIP(hipDeviceSynchronize());                       // (a copy out of the old buffer may be in flight)
        (void)hipHostFree(ctx->pin[which]);
        ctx->pin[which] = nullptr;
        ctx->pin_cap[which] = 0;
    }
    const size_t cap = (bytes + (bytes >> 2) + 4095) & ~(size_t)4095;
    if (hipHostMalloc(&ctx->pin[which], cap, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        ctx->pin[which] = nullptr;
        return fail(PCCM_E_OOM, "hipHostMalloc of %zu bytes (transfer staging) failed", cap);
    }
    ctx->pin_cap[which] = cap;
    return PCCM_OK;
}

constexpr size_t kStagedFrom = 32u << 10;        // (smaller transfers go through the runtime's own bounce buffers)
constexpr size_t kPinWindow = 64u << 20;         // most pinned memory one of the three buffers holds: larger transfers reuse it window by window

// host -> device on stream `st` (the context's main or copy stream)
static int h2d(pccm_ctx *ctx, void *dev, const void *host, size_t bytes, hipStream_t st)
{
    if (!ctx->io_staged || bytes < kStagedFrom) {
        PCCM_HIP(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, st));
        return PCCM_OK;
    }
    const int which = st == ctx->stream ? 0 : 1;
    if (!ctx->pin_ev[which]) PCCM_HIP(hipEventCreateWithFlags(&ctx->pin_ev[which], hipEventDisableTiming));
    if (ctx->pin_ev_set[which]) PCCM_HIP(hipEventSynchronize(ctx->pin_ev[which]));      // the previous upload has left the buffer
    int rc = pin_ensure(ctx, which, bytes < kPinWindow ? bytes : kPinWindow);
    if (rc) return rc;
    constexpr size_t kPiece = 4u << 20;                          // the copy of piece k + 1 runs beside the DMA of piece k
    static_assert(kPinWindow % kPiece == 0, "whole pieces per window");
    for (size_t off = 0; off < bytes; off += kPiece) {
        const size_t len = bytes - off < kPiece ? bytes - off : kPiece, at = off % kPinWindow;
        if (off && at == 0) {                                    // the window is full: its pieces must have left before it is refilled
            PCCM_HIP(hipEventRecord(ctx->pin_ev[which], st));
            PCCM_HIP(hipEventSynchronize(ctx->pin_ev[which]));
        }
        host_copy((char *)ctx->pin[which] + at, (const char *)host + off, len);
        PCCM_HIP(hipMemcpyAsync((char *)dev + off, (char *)ctx->pin[which] + at, len, hipMemcpyHostToDevice, st));
    }
    PCCM_HIP(hipEventRecord(ctx->pin_ev[which], st));
    ctx->pin_ev_set[which] = true;
    return PCCM_OK;
}

// device -> host on the main stream; the data are in `host` when the call returns only in staged mode -- callers synchronise the
// stream behind it either way
static int d2h(pccm_ctx *ctx, void *host, const void *dev, size_t bytes)
{
    if (!ctx->io_staged || bytes < kStagedFrom) {
        PCCM_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
        return PCCM_OK;
    }
    int rc = pin_ensure(ctx, 2, bytes < kPinWindow ? bytes : kPinWindow);
    if (rc) return rc;
    for (size_t off = 0; off < bytes; off += kPinWindow) {
        const size_t len = bytes - off < kPinWindow ? bytes - off : kPinWindow;
        PCCM_HIP(hipMemcpyAsync(ctx->pin[2], (const char *)dev + off, len, hipMemcpyDeviceToHost, ctx->stream));
        PCCM_HIP(hipStreamSynchronize(ctx->stream));
        host_copy((char *)host + off, ctx->pin[2], len);
    }
    return PCCM_OK;
}

static int upload(pccm_ctx *ctx, const void *src, size_t bytes, int on_device, const void **dev_src)
{
    if (on_device) {
        *dev_src = src;
        return PCCM_OK;
    }
    int rc = ensure(ctx, ctx->staging, bytes);
    if (rc) return rc;
    rc = h2d(ctx, ctx->staging.p, src, bytes, ctx->stream);
    if (rc) return rc;
    *dev_src = ctx->staging.p;
    return PCCM_OK;
}

// upload + widening copy + validation of one cloud's normals on stream `st` (staging buffer `stage` for host sources)
static int ingest_normals(pccm_ctx *ctx, Cloud &c, int which, const void *nrm, int64_t n, int dtype, int on_device, hipStream_t st, DevBuf &stage)
{
    const size_t esz = dtype == PCCM_F32 ? 4 : 8;
    const void *dsrc = nrm;
    if (!on_device) {
        int rc = ensure(ctx, stage, (size_t)n * 3 * esz);
        if (rc) return rc;
        rc = h2d(ctx, stage.p, nrm, (size_t)n * 3 * esz, st);
        if (rc) return rc;
        dsrc = stage.p;
    }
    unsigned long long *stats = (unsigned long long *)ctx->stats.p + (st == ctx->stream ? 0 : 12);
    PCCM_HIP(hipMemsetAsync(stats, 0, 3 * sizeof(unsigned long long), st));
    hipStream_t keep = ctx->stream;
    ctx->stream = st;                                  // (the launcher takes the context's stream)
    int rc = launch_ingest_normals(ctx, dsrc, dtype, n, c.nrm64, (float *)c.nrm32, stats);
    ctx->stream = keep;
    if (rc) return rc;
    unsigned long long h[3];
    PCCM_HIP(hipMemcpyAsync(h, stats, sizeof(h), hipMemcpyDeviceToHost, st));
    PCCM_HIP(hipStreamSynchronize(st));
    if (h[2] != 0) {
        c.n_nrm = 0;
        return fail(PCCM_E_ARG, "normals of cloud %d are not finite", which);      // n_nrm stays 0: no normals
    }
    c.n_nrm = n;
    c.nrm_exact32 = h[1] == 0;      // the search's fused projection then gathers 16 bytes per normal instead of 24 unaligned ones
    return PCCM_OK;
}

int normals_ready(pccm_ctx *ctx, Cloud &c)
{
    if (!c.nrm_deferred) return PCCM_OK;
    if (ctx->capturing) {
        ctx->capture_failed = true;
        return fail(PCCM_E_STATE, "deferred normals must be uploaded before graph capture: call pccm_flush_uploads first");
    }
    if (!ctx->copy_stream) PCCM_HIP(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    c.nrm_deferred = false;
    const void *src = c.nrm_host;
    c.nrm_host = nullptr;
    const int64_t n = c.n_nrm;
    c.n_nrm = 0;
    return ingest_normals(ctx, c, (int)(&c - ctx->cloud), src, n, c.nrm_host_dtype, 0, ctx->copy_stream, ctx->staging2);
}


}  // namespace pccm

using namespace pccm;

#define CHECK_CTX(ctx)                                                                            \
    if (!(ctx)) return fail(PCCM_E_ARG, "null context");                                          \
    std::lock_guard<std::recursive_mutex> ctx_guard_((ctx)->mu);                                  \
    do {                                                                                          \
        hipError_t _e = hipSetDevice((ctx)->device);                                              \
        if (_e != hipSuccess) return fail(PCCM_E_HIP, "hipSetDevice: %s", hipGetErrorString(_e)); \
    } while (0)

static void graph_free(GraphRec &g);
static int ensure_plain(pccm_ctx *ctx, NNResult &res, bool need_idx = true);
static int ensure_ties(pccm_ctx *ctx, int dir, bool want_nrm, bool want_rgb, bool want_ang = false);

#define NOT_CAPTURING(ctx)                                                                          \
    do {                                                                                           \
        if ((ctx)->capturing) {                                                                    \
            (ctx)->capture_failed = true;                                                          \
            return fail(PCCM_E_STATE, "%s is not allowed between pccm_graph_begin and pccm_graph_end", __func__); \
        }                                                                                          \
    } while (0)

extern "C" {

int pccm_version(void) { return PCCM_VERSION; }

const char *pccm_last_error(void) { return g_err; }

int pccm_device_count(int *n)
{
    if (!n) return fail(PCCM_E_ARG, "null pointer");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        c = 0;
    }
    *n = c;
    return PCCM_OK;
}

int pccm_ctx_create(int device, void *hip_stream, pccm_ctx **out)
{
    if (!out) return fail(PCCM_E_ARG, "null pointer");
    *out = nullptr;
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess || c <= 0) {
        (void)hipGetLastError();
        return fail(PCCM_E_NODEV, "no HIP device is visible: libpccm has no CPU path");
    }
    if (device < 0 || device >= c) return fail(PCCM_E_ARG, "device %d out of range (0..%d)", device, c - 1);
    PCCM_HIP(hipSetDevice(device));
    pccm_ctx *ctx = new (std::nothrow) pccm_ctx();
    if (!ctx) return fail(PCCM_E_OOM, "host allocation failed");
    ctx->device = device;
    if (hip_stream) {
        ctx->stream = (hipStream_t)hip_stream;
    } else {
        hipError_t e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
        if (e != hipSuccess) {
            delete ctx;
            return fail(PCCM_E_HIP, "hipStreamCreate: %s", hipGetErrorString(e));
        }
        ctx->own_stream = true;
    }
    int rc = ensure(ctx, ctx->counters, 16 * sizeof(uint32_t));      // [0..5] per-direction counters, [8..11] rescan tickets, [12..15] tail-launch counts
    // host-coherent: the host may read it on the completion counter's word alone (wait_batch), with no end-of-stream flush
    if (!rc && hipHostMalloc((void **)&ctx->host_err, 64, hipHostMallocCoherent) != hipSuccess) {
        ctx->host_err = nullptr;
        rc = fail(PCCM_E_OOM, "hipHostMalloc of the device error word failed");
    }
    if (!rc) *ctx->host_err = 0u;
    if (!rc && hipHostMalloc((void **)&ctx->done, 128, hipHostMallocCoherent) != hipSuccess) {     // a cache line of its own
        ctx->done = nullptr;
        rc = fail(PCCM_E_OOM, "hipHostMalloc of the completion counter failed");
    }
    if (!rc) *ctx->done = 0;
    if (!rc && hipHostMalloc((void **)&ctx->sel_host, pccm_ctx::kSelSlots * sizeof(double), hipHostMallocCoherent) != hipSuccess) {
        ctx->sel_host = nullptr;
        rc = fail(PCCM_E_OOM, "hipHostMalloc of the selection results failed");
    }
    if (!rc && hipEventCreateWithFlags(&ctx->batch_ev, hipEventDisableTiming) != hipSuccess) rc = fail(PCCM_E_HIP, "hipEventCreate failed");
    if (!rc) rc = ensure(ctx, ctx->stats, 32 * sizeof(unsigned long long));      // [0..9] the main stream's scratch, [12..14] the copy stream's, [16..22] colour reduction of the other direction
    if (!rc && hipMemsetAsync(ctx->counters.p, 0, 16 * sizeof(uint32_t), ctx->stream) != hipSuccess)
        rc = fail(PCCM_E_HIP, "hipMemsetAsync failed");
    if (rc) {
        pccm_ctx_destroy(ctx);
        return rc;
    }
    for (int d = 0; d < 3; ++d) ctx->nn[d].nflag_dev = (uint32_t *)ctx->counters.p + 2 * d;
    *out = ctx;
    return PCCM_OK;
}

int pccm_ctx_destroy(pccm_ctx *ctx)
{
    if (!ctx) return PCCM_OK;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (auto &s : ctx->spans) {
        (void)hipEventDestroy(s.a);
        (void)hipEventDestroy(s.b);
    }
    for (auto e : ctx->event_pool) (void)hipEventDestroy(e);
    if (ctx->batch_ev) (void)hipEventDestroy(ctx->batch_ev);
    ctx->batch_ev = nullptr;
    if (ctx->host_err) (void)hipHostFree(ctx->host_err);
    ctx->host_err = nullptr;
    if (ctx->done) (void)hipHostFree(ctx->done);
    ctx->done = nullptr;
    if (ctx->sel_host) (void)hipHostFree(ctx->sel_host);
    ctx->sel_host = nullptr;
    for (int k = 0; k < 2; ++k) free_cloud(ctx->cloud[k]);
    for (int d = 0; d < 2; ++d) {
        if (ctx->p2d64[d]) (void)hipFree(ctx->p2d64[d]);
        ctx->p2d64[d] = nullptr;
        ctx->cap_p2d[d] = 0;
        for (int c = 0; c < 2; ++c) {
            if (ctx->p2d_cj64[d][c]) (void)hipFree(ctx->p2d_cj64[d][c]);
            ctx->p2d_cj64[d][c] = nullptr;
            ctx->cap_p2d_cj[d][c] = 0;
        }
    }
    for (int d = 0; d < 3; ++d) free_nn(ctx->nn[d]);
    DevBuf *bufs[] = {&ctx->part_b1, &ctx->part_g, &ctx->part_b2, &ctx->val, &ctx->stats, &ctx->staging, &ctx->staging2,
                      &ctx->counters, &ctx->color_cols, &ctx->color_idx, &ctx->colsum_scratch, &ctx->rescan_part, &ctx->tail_sync,
                      &ctx->ssim_scratch, &ctx->carry_ws, &ctx->merge_ws, &ctx->occupancy_ws, &ctx->merge_refl, &ctx->merge_map[0], &ctx->merge_map[1], &ctx->tie_list, &ctx->sel_hist, &ctx->sel_state,
                      &ctx->match[0].buf, &ctx->match[1].buf};
    for (DevBuf *b : bufs) free_buf(*b);
    if (ctx->xf_scratch) (void)hipFree(ctx->xf_scratch);
    for (pccm_ctx::TieCols *t : {&ctx->tie[0], &ctx->tie[1], &ctx->tie_rows})
        for (DevBuf *b : {&t->pos, &t->nrm, &t->rgb, &t->k, &t->ang}) free_buf(*b);
    for (auto &g : ctx->graphs) graph_free(g);
    for (auto &s : ctx->slots) free_buf(s.val);
    for_each_slot(ctx, [](auto &s) {
        if constexpr (std::is_base_of_v<SlotHost, std::remove_reference_t<decltype(s)>>)
            if (s.host) (void)hipHostFree(s.host);
    });
    grid_release(ctx);
    if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
    for (auto &pbuf : ctx->pin)
        if (pbuf) (void)hipHostFree(pbuf);
    for (auto &pe : ctx->pin_ev)
        if (pe) (void)hipEventDestroy(pe);
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return PCCM_OK;
}

// behind launch_ingest_points: the ten statistics read back (one wait) and written into the cloud -- pccm_set_cloud and
// pccm_transform_cloud end alike
static int ingest_points_finish(pccm_ctx *ctx, Cloud &c, int which, int64_t n, int64_t n_pad, const unsigned long long *stats)
{
    unsigned long long h[10];
    PCCM_HIP(hipMemcpyAsync(h, stats, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    PCCM_HIP(hipStreamSynchronize(ctx->stream));
    double maxabs;
    memcpy(&maxabs, &h[0], sizeof(double));
    if (h[2] != 0 || !(maxabs <= kMaxAbsCoord)) {
        drop_cloud(c);
        return fail(PCCM_E_ARG, "cloud %d has non-finite coordinates or |x| > 1e15", which);
    }
    c.n = n;
    c.n_pad = n_pad;
    c.maxabs = maxabs;
    c.exact32 = (h[1] == 0);
    c.all_int = (h[1] == 0 && h[9] == 0);
    for (int k = 0; k < 3; ++k) {
        auto unkey = [](unsigned long long b) {
            b = (b >> 63) ? (b & 0x7fffffffffffffffull) : ~b;
            double v;
            memcpy(&v, &b, sizeof(v));
            return v;
        };
        c.bb_min[k] = unkey(h[3 + k]);
        c.bb_max[k] = unkey(h[6 + k]);
    }
    return PCCM_OK;
}

int pccm_set_cloud(pccm_ctx *ctx, int which, const void *xyz, int64_t n, int dtype, int on_device)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    if (which != 0 && which != 1) return fail(PCCM_E_ARG, "cloud index must be 0 or 1");
    if (!xyz || n <= 0) return fail(PCCM_E_ARG, "empty cloud (the reference cannot evaluate one either)");
    if (n > 0x7fffff00LL) return fail(PCCM_E_ARG, "more than 2^31 points per cloud are not supported");
    if (dtype != PCCM_F32 && dtype != PCCM_F64) return fail(PCCM_E_ARG, "dtype must be PCCM_F32 or PCCM_F64");
    Cloud &c = ctx->cloud[which];
    PCCM_HIP(hipStreamSynchronize(ctx->stream));
    points_changed(ctx, which);
    const int64_t n_pad = (n + kScanTile - 1) / kScanTile * kScanTile;
    int rc = grow((void **)&c.xyz32, c.cap32, (size_t)n_pad * 3 * sizeof(float));
    if (!rc) rc = grow((void **)&c.xyz64, c.cap64, (size_t)n * 3 * sizeof(double));
    if (!rc) rc = grow((void **)&c.xyz32r, c.cap32r, (size_t)n * sizeof(float4));
    if (rc) return rc;
    const size_t esz = dtype == PCCM_F32 ? 4 : 8;
    const void *dsrc = nullptr;
    rc = upload(ctx, xyz, (size_t)n * 3 * esz, on_device, &dsrc);
    if (rc) return rc;
    unsigned long long *stats = (unsigned long long *)ctx->stats.p;
    PCCM_HIP(hipMemsetAsync(stats, 0, 10 * sizeof(unsigned long long), ctx->stream));
    PCCM_HIP(hipMemsetAsync(stats + 3, 0xff, 3 * sizeof(unsigned long long), ctx->stream));
    rc = launch_ingest_points(ctx, dsrc, dtype, n, n_pad, c.xyz32, c.xyz64, c.xyz32r, stats);
    if (rc) return rc;
    return ingest_points_finish(ctx, c, which, n, n_pad, stats);
}

// the front of the two normals setters: arguments, the stream drained, everything made from the old normals forgotten
// (normals_changed), room for the new ones
static int normals_front(pccm_ctx *ctx, int which, const void *nrm, int64_t n, int dtype)
{
    if (which != 0 && which != 1) return fail(PCCM_E_ARG, "cloud index must be 0 or 1");
    if (!nrm || n <= 0) return fail(PCCM_E_ARG, "empty normals");
    if (dtype != PCCM_F32 && dtype != PCCM_F64) return fail(PCCM_E_ARG, "dtype must be PCCM_F32 or PCCM_F64");
    Cloud &c = ctx->cloud[which];
    PCCM_HIP(hipStreamSynchronize(ctx->stream));
    normals_changed(ctx, which);
    int rc = grow((void **)&c.nrm64, c.cap_nrm, (size_t)n * 3 * sizeof(double));
    if (rc) return rc;
    return grow((void **)&c.nrm32, c.cap_nrm32, (size_t)n * sizeof(float4));
}

int pccm_set_normals(pccm_ctx *ctx, int which, const void *nrm, int64_t n, int dtype, int on_device)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    int rc = normals_front(ctx, which, nrm, n, dtype);
    if (rc) return rc;
    return ingest_normals(ctx, ctx->cloud[which], which, nrm, n, dtype, on_device, ctx->stream, ctx->staging);
}

int pccm_set_normals_deferred(pccm_ctx *ctx, int which, const void *nrm, int64_t n, int dtype)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    int rc = normals_front(ctx, which, nrm, n, dtype);
    if (rc) return rc;
    Cloud &c = ctx->cloud[which];
    c.n_nrm = n;                                       // announced: the searches know that (and how many) normals exist
    c.nrm_host = nrm;
    c.nrm_host_dtype = dtype;
    c.nrm_deferred = true;
    return PCCM_OK;
}

// pccm_transform_cloud (include/pccm.h).  The two ingest kernels in their moving mode read the cloud's own fp64 rows and write the
// moved rows into a scratch buffer, which is then swapped with the cloud's: source and destination never alias (the kernels'
// pointers stay __restrict__, and a normal's three threads each read the whole row).  The buffer the points leave behind is the
// scratch the normals are moved into.
int pccm_transform_cloud(pccm_ctx *ctx, int which, const double *m)
{
    CHECK_CTX(ctx);
    if (which != 0 && which != 1) return fail(PCCM_E_ARG, "cloud index must be 0 or 1");
    if (!m) return fail(PCCM_E_ARG, "null pointer");
    for (int k = 0; k < 12; ++k)
        if (!std::isfinite(m[k])) return fail(PCCM_E_ARG, "the matrix has a non-finite entry");
    NOT_CAPTURING(ctx);
    Cloud &c = ctx->cloud[which];
    if (c.n <= 0) return fail(PCCM_E_STATE, "cloud %d is not set", which);
    if (ctx->sharded()) return fail(PCCM_E_STATE, "moving a cloud needs the whole cloud on this GPU (world = 1)");
    if (c.n_nrm != 0 && c.n_nrm != c.n)
        return fail(PCCM_E_STATE, "cloud %d has %lld points but %lld normals: they cannot be moved with it", which, (long long)c.n, (long long)c.n_nrm);
    bool identity = true;
    for (int k = 0; k < 12; ++k) identity = identity && m[k] == ((k % 4 == k / 4) ? 1.0 : 0.0);
    if (identity) return PCCM_OK;                          // nothing is rewritten, nothing goes stale
    // no coordinate can leave the range the ingest accepts: |x'| <= (|a0| + |a1| + |a2|) maxabs + |t| per row, with room for the
    // four roundings (refused before anything is written)
    for (int a = 0; a < 3; ++a) {
        const double bound = (fabs(m[4 * a]) + fabs(m[4 * a + 1]) + fabs(m[4 * a + 2])) * c.maxabs + fabs(m[4 * a + 3]);
        if (!(bound * (1.0 + 0x1p-48) <= kMaxAbsCoord))
            return fail(PCCM_E_ARG, "moving cloud %d could take a coordinate beyond |x| = 1e15", which);
    }
    int rc = normals_ready(ctx, c);
    if (rc) return rc;
    PCCM_HIP(hipStreamSynchronize(ctx->stream));
    points_moved(ctx, which);                              // (normals carried to this cloud are gone now: they are not moved)
    const int64_t n = c.n, n_pad = c.n_pad;
    if ((rc = grow((void **)&ctx->xf_scratch, ctx->cap_xf, (size_t)n * 3 * sizeof(double)))) return rc;
    IngestMove mv;
    mv.on = 1;
    memcpy(mv.m, m, sizeof mv.m);
    unsigned long long *stats = (unsigned long long *)ctx->stats.p;
    PCCM_HIP(hipMemsetAsync(stats, 0, 10 * sizeof(unsigned long long), ctx->stream));
    PCCM_HIP(hipMemsetAsync(stats + 3, 0xff, 3 * sizeof(unsigned long long), ctx->stream));
    if ((rc = launch_ingest_points(ctx, c.xyz64, PCCM_F64, n, n_pad, c.xyz32, ctx->xf_scratch, c.xyz32r, stats, &mv))) return rc;
    std::swap(c.xyz64, ctx->xf_scratch);
    std::swap(c.cap64, ctx->cap_xf);
    if ((rc = ingest_points_finish(ctx, c, which, n, n_pad, stats))) return rc;
    if (c.n_nrm == n) {
        if ((rc = grow((void **)&ctx->xf_scratch, ctx->cap_xf, (size_t)n * 3 * sizeof(double)))) return rc;
        // (estimated and carried normals come without the fp32 words: the ingest writes them, so they must be there)
        if ((rc = grow((void **)&c.nrm32, c.cap_nrm32, (size_t)n * sizeof(float4)))) return rc;
        PCCM_HIP(hipMemsetAsync(stats, 0, 3 * sizeof(unsigned long long), ctx->stream));
        if ((rc = launch_ingest_normals(ctx, c.nrm64, PCCM_F64, n, ctx->xf_scratch, (float *)c.nrm32, stats, &mv))) return rc;
        std::swap(c.nrm64, ctx->xf_scratch);
        std::swap(c.cap_nrm, ctx->cap_xf);
        unsigned long long h[3];
        PCCM_HIP(hipMemcpyAsync(h, stats, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
        PCCM_HIP(hipStreamSynchronize(ctx->stream));
        if (h[2] != 0) {
            drop_normals(c);
            return fail(PCCM_E_ARG, "the moved normals of cloud %d are not finite", which);
        }
        c.nrm_exact32 = h[1] == 0;
    }
    return PCCM_OK;
}

int pccm_get_bounds(pccm_ctx *ctx, int which, double *lo, double *hi)
{
    CHECK_CTX(ctx);
    if (which != 0 && which != 1) return fail(PCCM_E_ARG, "cloud index must be 0 or 1");
    if (!lo || !hi) return fail(PCCM_E_ARG, "null pointer");
    const Cloud &c = ctx->cloud[which];
    if (c.n <= 0) return fail(PCCM_E_STATE, "cloud %d is not set", which);
    for (int a = 0; a < 3; ++a) {
        lo[a] = c.bb_min[a];
        hi[a] = c.bb_max[a];
    }
    return PCCM_OK;
}

int pccm_set_io_staged(pccm_ctx *ctx, int on)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    PCCM_HIP(hipStreamSynchronize(ctx->stream));
    ctx->io_staged = on != 0;
    return PCCM_OK;
}

int pccm_set_wait(pccm_ctx *ctx, int mode)
{
    CHECK_CTX(ctx);
#ifdef PCCM_DIAG
    if (mode == 2) { ctx->wait_mode = mode; return PCCM_OK; }     // diagnostic build: a hipEventQuery spin, for A/B timing
#endif
    if (mode != PCCM_WAIT_SPIN && mode != PCCM_WAIT_EVENT) return fail(PCCM_E_ARG, "bad wait mode %d", mode);
    ctx->wait_mode = mode;
    return PCCM_OK;
}

int pccm_wait_counter(pccm_ctx *ctx, uint64_t *out)
{
    CHECK_CTX(ctx);
    if (!out) return fail(PCCM_E_ARG, "null pointer");
    *out = __atomic_load_n(ctx->done, __ATOMIC_ACQUIRE);
    return PCCM_OK;
}

int pccm_flush_uploads(pccm_ctx *ctx)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    for (int k = 0; k < 2; ++k) {
        int rc = normals_ready(ctx, ctx->cloud[k]);
        if (rc) return rc;
    }
    return PCCM_OK;
}

// the front of the two colour setters: arguments, the point count, the stream drained, everything made from the old colours
// forgotten (colors_changed), room for the new ones in both forms
static int colors_front(pccm_ctx *ctx, int which, const void *rgb, int64_t n, int dtype)
{
    if (which != 0 && which != 1) return fail(PCCM_E_ARG, "cloud index must be 0 or 1");
    if (!rgb || n <= 0) return fail(PCCM_E_ARG, "empty colours");
    if (dtype != PCCM_F32 && dtype != PCCM_F64) return fail(PCCM_E_ARG, "dtype must be PCCM_F32 or PCCM_F64");
    Cloud &c = ctx->cloud[which];
    if (c.n == 0) return fail(PCCM_E_STATE, "set cloud %d before its colours", which);
    if (n != c.n) return fail(PCCM_E_ARG, "cloud %d has %lld points but %lld colours", which, (long long)c.n, (long long)n);
    PCCM_HIP(hipStreamSynchronize(ctx->stream));
    colors_changed(ctx, which);
    int rc = grow((void **)&c.rgb64, c.cap_rgb, (size_t)n * 3 * sizeof(double));
    if (rc) return rc;
    return grow((void **)&c.rgb8, c.cap_rgb8, (size_t)n * sizeof(uint32_t));
}

int pccm_set_colors(pccm_ctx *ctx, int which, const void *rgb, int64_t n, int dtype, int on_device)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    int rc = colors_front(ctx, which, rgb, n, dtype);
    if (rc) return rc;
    Cloud &c = ctx->cloud[which];
    const void *dsrc = nullptr;
    rc = upload(ctx, rgb, (size_t)n * 3 * (dtype == PCCM_F32 ? 4 : 8), on_device, &dsrc);
    if (rc) return rc;
    unsigned long long *stats = (unsigned long long *)ctx->stats.p;
    PCCM_HIP(hipMemsetAsync(stats, 0, 3 * sizeof(unsigned long long), ctx->stream));
    rc = launch_ingest_normals(ctx, dsrc, dtype, n, c.rgb64, nullptr, stats);      // same widening copy; non-finite values are
    if (rc) return rc;                                                    // allowed here (NumPy propagates them)
    // colours that are bytes / 255 (nearly all are) also as packed words: Cloud::rgb8
    PCCM_HIP(hipMemsetAsync(stats + 4, 0, sizeof(unsigned long long), ctx->stream));
    if ((rc = launch_rgb8(ctx, c, nullptr, (unsigned int *)(stats + 4)))) return rc;
    unsigned long long not_bytes = 1;
    PCCM_HIP(hipMemcpyAsync(&not_bytes, stats + 4, sizeof(not_bytes), hipMemcpyDeviceToHost, ctx->stream));
    PCCM_HIP(hipStreamSynchronize(ctx->stream));
    c.rgb8_valid = not_bytes == 0;
    c.n_rgb = n;
    return PCCM_OK;
}

int pccm_set_colors_u8(pccm_ctx *ctx, int which, const unsigned char *rgb, int64_t n)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    int rc = colors_front(ctx, which, rgb, n, PCCM_F64);      // (bytes: no dtype to check, they widen to fp64)
    if (rc) return rc;
    Cloud &c = ctx->cloud[which];
    const void *dsrc = nullptr;
    rc = upload(ctx, rgb, (size_t)n * 3, 0, &dsrc);
    if (rc) return rc;
    rc = launch_colors_from_u8(ctx, (const unsigned char *)dsrc, n * 3, c.rgb64);
    if (rc) return rc;
    if ((rc = launch_rgb8(ctx, c, (const unsigned char *)dsrc, nullptr))) return rc;
    PCCM_HIP(hipStreamSynchronize(ctx->stream));
    c.rgb8_valid = true;
    c.n_rgb = n;
    return PCCM_OK;
}

// The two reflectance setters: arguments, the point count, the stream drained, what read the old column forgotten
// (reflectance_changed), the upload (bytes per value: esz), the widening ingest and its count of non-finite values.
static int set_reflectance(pccm_ctx *ctx, int which, const void *r, int64_t n, int dtype, size_t esz, int on_device)
{
    if (which != 0 && which != 1) return fail(PCCM_E_ARG, "cloud index must be 0 or 1");
    if (!r || n <= 0) return fail(PCCM_E_ARG, "empty reflectance");
    Cloud &c = ctx->cloud[which];
    if (c.n == 0) return fail(PCCM_E_STATE, "set cloud %d before its reflectance", which);
    if (n != c.n) return fail(PCCM_E_ARG, "cloud %d has %lld points but %lld reflectance values", which, (long long)c.n, (long long)n);
    PCCM_HIP(hipStreamSynchronize(ctx->stream));
    reflectance_changed(ctx, which);
    int rc = grow((void **)&c.refl64, c.cap_refl, (size_t)n * sizeof(double));
    if (rc) return rc;
    const void *dsrc = nullptr;
    if ((rc = upload(ctx, r, (size_t)n * esz, on_device, &dsrc))) return rc;
    unsigned long long *stats = (unsigned long long *)ctx->stats.p;
    PCCM_HIP(hipMemsetAsync(stats, 0, 3 * sizeof(unsigned long long), ctx->stream));
    if ((rc = launch_ingest_reflectance(ctx, dsrc, dtype, n, c.refl64, stats))) return rc;
    unsigned long long bad = 1;
    PCCM_HIP(hipMemcpyAsync(&bad, stats + 2, sizeof(bad), hipMemcpyDeviceToHost, ctx->stream));
    PCCM_HIP(hipStreamSynchronize(ctx->stream));
    if (bad != 0) return fail(PCCM_E_ARG, "reflectance of cloud %d is not finite", which);      // n_refl stays 0: no reflectance
    c.n_refl = n;
    return PCCM_OK;
}

int pccm_set_reflectance(pccm_ctx *ctx, int which, const void *r, int64_t n, int dtype, int on_device)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    if (dtype != PCCM_F32 && dtype != PCCM_F64) return fail(PCCM_E_ARG, "dtype must be PCCM_F32 or PCCM_F64");
    return set_reflectance(ctx, which, r, n, dtype, dtype == PCCM_F32 ? 4 : 8, on_device);
}

int pccm_set_reflectance_u16(pccm_ctx *ctx, int which, const uint16_t *r, int64_t n)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    if (which != 0 && which != 1) return fail(PCCM_E_ARG, "cloud index must be 0 or 1");
    if (!r || n <= 0) return fail(PCCM_E_ARG, "empty reflectance");
    if (ctx->cloud[which].n == 0) return fail(PCCM_E_STATE, "set cloud %d before its reflectance", which);
    if (n != ctx->cloud[which].n)
        return fail(PCCM_E_ARG, "cloud %d has %lld points but %lld reflectance values", which, (long long)ctx->cloud[which].n, (long long)n);
    // every 16-bit value is a float: widened exactly here, the float ingest takes it from there (four bytes per point up)
    std::vector<float> wide;
    try { wide.assign(r, r + n); } catch (const std::bad_alloc &) { return fail(PCCM_E_OOM, "no host memory for %lld reflectance values", (long long)n); }
    return set_reflectance(ctx, which, wide.data(), n, PCCM_F32, sizeof(float), 0);
}

// common front end of the two colour calls: operands of direction `dir` and the neighbour rows to use
// (*drecs: matched records that carry the rows -- the kernel reads the row out of the record, no unpacked copy is made for it)
// (*dmean: PCCM_TIES_MEAN -- the averaged neighbour colour of every row, read instead of the gather)
static int color_operands(pccm_ctx *ctx, int dir, int scheme, const int32_t *rows, int64_t nrows,
                          const Cloud **own, const Cloud **other, const int32_t **drows, const float4 **drecs, const double **dmean)
{
    *drecs = nullptr;
    *dmean = nullptr;
    if (dir != PCCM_DIR_LEFT && dir != PCCM_DIR_RIGHT) return fail(PCCM_E_ARG, "colour metrics exist for directions 0 and 1");
    if (scheme < 0 || scheme > 2) return fail(PCCM_E_ARG, "unknown colour scheme %d", scheme);
    const Cloud &it = ctx->cloud[dir == PCCM_DIR_LEFT ? 0 : 1], &se = ctx->cloud[dir == PCCM_DIR_LEFT ? 1 : 0];
    if (it.n_rgb <= 0 || se.n_rgb <= 0) return fail(PCCM_E_STATE, "both clouds need colours (pccm_set_colors)");
    if (rows) {
        if (nrows != it.n) return fail(PCCM_E_ARG, "%lld neighbour rows for %lld points", (long long)nrows, (long long)it.n);
        int rc = ensure(ctx, ctx->color_idx, (size_t)nrows * sizeof(int32_t));
        if (rc) return rc;
        { int rch = h2d(ctx, ctx->color_idx.p, rows, (size_t)nrows * sizeof(int32_t), ctx->stream); if (rch) return rch; }
        *drows = (const int32_t *)ctx->color_idx.p;
        const NNResult &res = ctx->nn[dir];
        if ((res.valid ? res.ties : ctx->ties) == PCCM_TIES_MEAN) {
            // the gathered rows of a sharded search: the tie sets of the whole iterating cloud, distances formed from the rows
            pccm_ctx::TieCols &t = ctx->tie_rows;
            const size_t n3 = (size_t)nrows * 3 * sizeof(double);
            if ((rc = ensure(ctx, t.pos, n3)) || (rc = ensure(ctx, t.rgb, n3)) || (rc = ensure(ctx, t.k, (size_t)nrows * sizeof(int32_t)))) return rc;
            if ((rc = tie_mean(ctx, dir, *drows, nullptr, 0, nrows, nullptr, se.rgb64, (double *)t.pos.p, (int32_t *)t.k.p, nullptr,
                               (double *)t.rgb.p)))
                return rc;
            *dmean = (const double *)t.rgb.p;
        }
    } else {
        NNResult &res = ctx->nn[dir];
        if (!res.valid) return fail(PCCM_E_STATE, "run pccm_nn for direction %d first", dir);
        if (res.begin != 0 || res.end != it.n)
            return fail(PCCM_E_STATE, "the search of direction %d was sharded: pass the gathered neighbour rows", dir);
        if (res.form.matched_in_place()) {
            *drows = nullptr;
            *drecs = (const float4 *)res.rec.p;
        } else {
            int rc = ensure_plain(ctx, res);
            if (rc) return rc;
            *drows = res.idx;
        }
        if (res.ties == PCCM_TIES_MEAN) {
            int rc = ensure_ties(ctx, dir, false, true);
            if (rc) return rc;
            *dmean = (const double *)ctx->tie[dir].rgb.p;
        }
    }
    *own = &it;
    *other = &se;
    return PCCM_OK;
}

int pccm_color_reduce(pccm_ctx *ctx, int dir, int scheme, double scale, const int32_t *rows, int64_t nrows,
                      double sum_out[3], double max_out[3])
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    if (!sum_out || !max_out) return fail(PCCM_E_ARG, "null output");
    const Cloud *own[2], *other[2];
    const int32_t *drows[2];
    const float4 *drecs[2];
    const double *dmean[2] = {nullptr, nullptr};
    int rc = color_operands(ctx, dir, scheme, rows, nrows, &own[0], &other[0], &drows[0], &drecs[0], &dmean[0]);
    if (rc) return rc;
    pccm_ctx::ColorMemo &memo = ctx->color_memo;
    if (!rows && memo.valid && memo.dir == dir && memo.scheme == scheme && memo.scale == scale && memo.gen == ctx->nn_gen[dir] &&
        memo.rgb_gen == ctx->rgb_gen) {
        memo.valid = false;                               // (answered once: the host side keeps what it was given)
        if (memo.range_bad) return fail(PCCM_E_RANGE, "a neighbour row is outside the other cloud");
        memcpy(max_out, memo.max, sizeof(memo.max));
        memcpy(sum_out, memo.sum, sizeof(memo.sum));
        return PCCM_OK;
    }
    memo.valid = false;
    // the other direction rides along when it could be asked for the same way: the pair's own rows, an unsharded result
    int njobs = 1;
    const int sib = dir == PCCM_DIR_LEFT ? PCCM_DIR_RIGHT : PCCM_DIR_LEFT;
    if (!rows && ctx->nn[sib].valid && ctx->nn[sib].begin == 0 && ctx->nn[sib].end == ctx->cloud[sib == PCCM_DIR_LEFT ? 0 : 1].n &&
        color_operands(ctx, sib, scheme, nullptr, 0, &own[1], &other[1], &drows[1], &drecs[1], &dmean[1]) == PCCM_OK)
        njobs = 2;
    const int64_t n[2] = {own[0]->n, njobs == 2 ? own[1]->n : 0};
    rc = ensure(ctx, ctx->color_cols, (size_t)(n[0] + n[1]) * 3 * sizeof(double));
    if (rc) return rc;
    // stats scratch per job: [0..2] column maxima as bit keys, [3..5] column sums, [6] range flag; the second job at word 16
    unsigned long long *small[2] = {(unsigned long long *)ctx->stats.p, (unsigned long long *)ctx->stats.p + 16};
    const double *cols[2] = {(const double *)ctx->color_cols.p, (const double *)ctx->color_cols.p + 3 * n[0]};
    double *sums[2] = {(double *)(small[0] + 3), (double *)(small[1] + 3)};
    PCCM_HIP(hipMemsetAsync(small[0], 0, (njobs == 2 ? 23 : 7) * sizeof(unsigned long long), ctx->stream));      // (one fill for both jobs' words)
    for (int k = 0; k < njobs; ++k) {
        const bool bytes = own[k]->rgb8_valid && other[k]->rgb8_valid;
        rc = launch_color_rows(ctx, own[k]->rgb64, other[k]->rgb64, drows[k], n[k], other[k]->n, scheme, scale, 4, (double *)cols[k], nullptr,
                               (unsigned int *)(small[k] + 6), bytes ? own[k]->rgb8 : nullptr, bytes ? other[k]->rgb8 : nullptr, drecs[k],
                               dmean[k]);
        if (rc) return rc;
    }
    rc = launch_color_colsums(ctx, njobs, cols, n, sums, small);      // (+ the columns' maxima as bit keys into small[k][0..2])
    if (rc) return rc;
    unsigned long long h[2][7];
    for (int k = 0; k < njobs; ++k) PCCM_HIP(hipMemcpyAsync(h[k], small[k], sizeof(h[k]), hipMemcpyDeviceToHost, ctx->stream));
    PCCM_HIP(hipStreamSynchronize(ctx->stream));
    if (njobs == 2) {
        memo.valid = true;
        memo.range_bad = h[1][6] != 0;
        memo.dir = sib;
        memo.scheme = scheme;
        memo.scale = scale;
        memo.gen = ctx->nn_gen[sib];
        memo.rgb_gen = ctx->rgb_gen;
        memcpy(memo.max, h[1], sizeof(memo.max));
        memcpy(memo.sum, h[1] + 3, sizeof(memo.sum));
    }
    if (h[0][6]) return fail(PCCM_E_RANGE, "a neighbour row is outside the other cloud");
    memcpy(max_out, h[0], 3 * sizeof(double));
    memcpy(sum_out, h[0] + 3, 3 * sizeof(double));
    return PCCM_OK;
}

int pccm_obb_frames(pccm_ctx *ctx, const double *verts, int64_t nv, const double *tri, int64_t nt, double ext_out[3], double *vol_out)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    if (!verts || !tri || !ext_out || nv <= 0 || nt <= 0) return fail(PCCM_E_ARG, "bad argument");
    // scratch: [nv][3] vertices | [nt][9] triangles | [nt][3] extents | [nt] volumes
    const size_t bytes = ((size_t)nv * 3 + (size_t)nt * 13) * sizeof(double);
    int rc = ensure(ctx, ctx->color_cols, bytes);
    if (rc) return rc;
    double *dv = (double *)ctx->color_cols.p, *dt = dv + 3 * nv, *de = dt + 9 * nt, *dvol = de + 3 * nt;
    // (two uploads through one pinned buffer: the second waits for the first's copy out of it)
    if ((rc = h2d(ctx, dv, verts, (size_t)nv * 3 * sizeof(double), ctx->stream))) return rc;
    if ((rc = h2d(ctx, dt, tri, (size_t)nt * 9 * sizeof(double), ctx->stream))) return rc;
    rc = launch_obb_frames(ctx, dv, nv, dt, nt, de, dvol);
    if (rc) return rc;
    std::vector<double> ext((size_t)nt * 3), vol((size_t)nt);
    PCCM_HIP(hipMemcpyAsync(ext.data(), de, ext.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    PCCM_HIP(hipMemcpyAsync(vol.data(), dvol, vol.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    PCCM_HIP(hipStreamSynchronize(ctx->stream));
    int64_t best = -1;
    for (int64_t t = 0; t < nt; ++t)                      // first smallest finite volume (np.argmin's choice)
        if (vol[t] < INFINITY && (best < 0 || vol[t] < vol[best])) best = t;
    if (best < 0) return fail(PCCM_E_ARG, "degenerate convex hull: no triangle spans a box of finite volume");
    for (int k = 0; k < 3; ++k) ext_out[k] = ext[3 * best + k];
    if (vol_out) *vol_out = vol[best];
    return PCCM_OK;
}

int pccm_extreme_rows(pccm_ctx *ctx, int which, const float *dirs, int ndirs, int32_t *rows_out)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    if ((which != 0 && which != 1) || !dirs || !rows_out || ndirs <= 0 || ndirs > 1024) return fail(PCCM_E_ARG, "bad argument (1..1024 directions)");
    const Cloud &c = ctx->cloud[which];
    if (c.n <= 0) return fail(PCCM_E_STATE, "cloud %d is not set", which);
    int rc = ensure(ctx, ctx->color_cols, (size_t)ndirs * (3 * sizeof(float) + sizeof(unsigned long long)));
    if (rc) return rc;
    unsigned long long *best = (unsigned long long *)ctx->color_cols.p;
    float *ddirs = (float *)(best + ndirs);
    PCCM_HIP(hipMemsetAsync(best, 0, (size_t)ndirs * sizeof(unsigned long long), ctx->stream));
    PCCM_HIP(hipMemcpyAsync(ddirs, dirs, (size_t)ndirs * 3 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    rc = launch_extreme_rows(ctx, c.xyz64, c.n, ddirs, ndirs, best);
    if (rc) return rc;
    std::vector<unsigned long long> h((size_t)ndirs);
    PCCM_HIP(hipMemcpyAsync(h.data(), best, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    PCCM_HIP(hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < ndirs; ++k) rows_out[k] = (int32_t)(h[k] & 0xffffffffull);
    return PCCM_OK;
}

int pccm_rows_outside(pccm_ctx *ctx, int which, const double *planes, int nplanes, double margin, int32_t *rows_out, int64_t *count)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    if ((which != 0 && which != 1) || !planes || !rows_out || !count || nplanes <= 0 || !(margin >= 0.0)) return fail(PCCM_E_ARG, "bad argument");
    const Cloud &c = ctx->cloud[which];
    if (c.n <= 0) return fail(PCCM_E_STATE, "cloud %d is not set", which);
    int rc = ensure(ctx, ctx->color_cols, (size_t)nplanes * 4 * sizeof(double) + (size_t)c.n * sizeof(int32_t) + 16);
    if (rc) return rc;
    double *dpl = (double *)ctx->color_cols.p;
    unsigned int *dcount = (unsigned int *)(dpl + 4 * (size_t)nplanes);
    int32_t *drows = (int32_t *)(dcount + 4);
    PCCM_HIP(hipMemcpyAsync(dpl, planes, (size_t)nplanes * 4 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    PCCM_HIP(hipMemsetAsync(dcount, 0, sizeof(unsigned int), ctx->stream));
    rc = launch_outside_planes(ctx, c.xyz64, c.n, dpl, nplanes, margin, drows, dcount);
    if (rc) return rc;
    unsigned int hc = 0;
    PCCM_HIP(hipMemcpyAsync(&hc, dcount, sizeof(hc), hipMemcpyDeviceToHost, ctx->stream));
    PCCM_HIP(hipStreamSynchronize(ctx->stream));
    if (hc) {
        if ((rc = d2h(ctx, rows_out, drows, (size_t)hc * sizeof(int32_t)))) return rc;
        PCCM_HIP(hipStreamSynchronize(ctx->stream));
    }
    *count = (int64_t)hc;
    return PCCM_OK;
}

int pccm_seq_colsum(pccm_ctx *ctx, const double *cols, int64_t n, double out[3])
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    if (!cols || !out || n <= 0) return fail(PCCM_E_ARG, "bad argument");
    int rc = ensure(ctx, ctx->color_cols, (size_t)n * 3 * sizeof(double));
    if (rc) return rc;
    if ((rc = h2d(ctx, ctx->color_cols.p, cols, (size_t)n * 3 * sizeof(double), ctx->stream))) return rc;
    double *dsum = (double *)ctx->stats.p + 3;
    rc = launch_color_colsum(ctx, (const double *)ctx->color_cols.p, n, dsum);
    if (rc) return rc;
    PCCM_HIP(hipMemcpyAsync(out, dsum, 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    PCCM_HIP(hipStreamSynchronize(ctx->stream));
    return PCCM_OK;
}

int pccm_color_rows(pccm_ctx *ctx, int dir, int scheme, double scale, int what, const int32_t *rows, int64_t nrows,
                    double *out)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    if (!out) return fail(PCCM_E_ARG, "null output");
    if (what < 0 || what > 3) return fail(PCCM_E_ARG, "what must be 0..3");
    const Cloud *own, *other;
    const int32_t *drows;
    const float4 *drecs;
    const double *dmean;
    int rc = color_operands(ctx, dir, scheme, rows, nrows, &own, &other, &drows, &drecs, &dmean);
    if (rc) return rc;
    const int64_t n = own->n;
    rc = ensure(ctx, ctx->color_cols, (size_t)n * 3 * sizeof(double));
    if (rc) return rc;
    unsigned long long *small = (unsigned long long *)ctx->stats.p;
    PCCM_HIP(hipMemsetAsync(small + 6, 0, sizeof(unsigned long long), ctx->stream));
    const bool bytes = own->rgb8_valid && other->rgb8_valid;
    rc = launch_color_rows(ctx, own->rgb64, other->rgb64, drows, n, other->n, scheme, scale, what, (double *)ctx->color_cols.p,
                           small, (unsigned int *)(small + 6), bytes ? own->rgb8 : nullptr, bytes ? other->rgb8 : nullptr, drecs, dmean);
    if (rc) return rc;
    unsigned long long flag = 0;
    if ((rc = d2h(ctx, out, ctx->color_cols.p, (size_t)n * 3 * sizeof(double)))) return rc;
    PCCM_HIP(hipMemcpyAsync(&flag, small + 6, sizeof(flag), hipMemcpyDeviceToHost, ctx->stream));
    PCCM_HIP(hipStreamSynchronize(ctx->stream));
    if (flag) return fail(PCCM_E_RANGE, "a neighbour row is outside the other cloud");
    return PCCM_OK;
}

int pccm_estimate_normals(pccm_ctx *ctx, int which, int knn)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    if (which != 0 && which != 1) return fail(PCCM_E_ARG, "cloud index must be 0 or 1");
    return estimate_normals(ctx, which, knn);
}

// the back of the getters (each has decided that what it hands out is there): the copy and the wait for it
static int fetch(pccm_ctx *ctx, void *out, const void *dev, size_t bytes)
{
    int rc = d2h(ctx, out, dev, bytes);
    if (rc) return rc;
    PCCM_HIP(hipStreamSynchronize(ctx->stream));
    return PCCM_OK;
}

int pccm_get_normals(pccm_ctx *ctx, int which, double *out)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    if (which != 0 && which != 1) return fail(PCCM_E_ARG, "cloud index must be 0 or 1");
    if (!out) return fail(PCCM_E_ARG, "null pointer");
    Cloud &c = ctx->cloud[which];
    { int rcn = normals_ready(ctx, c); if (rcn) return rcn; }
    if (c.n_nrm <= 0) return fail(PCCM_E_STATE, "cloud %d has no normals", which);
    return fetch(ctx, out, c.nrm64, (size_t)c.n_nrm * 3 * sizeof(double));
}

int pccm_carry_normals(pccm_ctx *ctx, int from, int *built)
{
    CHECK_CTX(ctx);
    if (built) *built = 0;
    if (from != 0 && from != 1) return fail(PCCM_E_ARG, "cloud index must be 0 or 1");
    const int to = 1 - from;
    Cloud &cf = ctx->cloud[from], &ct = ctx->cloud[to];
    if (cf.n <= 0 || ct.n <= 0) return fail(PCCM_E_STATE, "carrying normals needs both clouds");
    if (ctx->sharded()) return fail(PCCM_E_STATE, "carrying normals needs whole clouds on this GPU (world = 1)");
    if (ctx->ties != PCCM_TIES_PICK) return fail(PCCM_E_STATE, "carrying normals is not defined under PCCM_TIES_MEAN");
    if (!ctx->capturing) { int rcn = normals_ready(ctx, cf); if (rcn) return rcn; }
    if (cf.n_nrm != cf.n || cf.nrm_deferred) return fail(PCCM_E_STATE, "cloud %d has no normal for every point to carry over", from);
    const int dir_f = from == 0 ? PCCM_DIR_LEFT : PCCM_DIR_RIGHT, dir_g = from == 0 ? PCCM_DIR_RIGHT : PCCM_DIR_LEFT;
    NNResult &rf = ctx->nn[dir_f], &rg = ctx->nn[dir_g];
    if (!rf.valid || !rg.valid) return fail(PCCM_E_STATE, "carrying normals needs the results of both directional searches (pccm_nn_pair)");
    if (rf.ties != PCCM_TIES_PICK || rg.ties != PCCM_TIES_PICK)
        return fail(PCCM_E_STATE, "the searches ran under PCCM_TIES_MEAN: carrying normals is not defined there");
    if (ctx->carry.to == to && ct.n_nrm == ct.n && ctx->carry.run_f == ctx->nn_run[dir_f] && ctx->carry.run_g == ctx->nn_run[dir_g])
        return PCCM_OK;                                // (what is there already needs no work, and may be asked for while capturing)
    if (ctx->capturing) {
        ctx->capture_failed = true;
        return fail(PCCM_E_STATE, "normals are carried before graph capture");
    }
    int rc;
    if ((rc = ensure_plain(ctx, rf, true)) || (rc = ensure_plain(ctx, rg, true))) return rc;     // (repeats a search that left the rows out)
    PCCM_HIP(hipStreamSynchronize(ctx->stream));
    if ((rc = grow((void **)&ct.nrm64, ct.cap_nrm, (size_t)ct.n * 3 * sizeof(double)))) return rc;
    if ((rc = ensure(ctx, ctx->carry_ws, carry_ws_bytes(cf.n, ct.n)))) return rc;
    normals_changed(ctx, to);                          // (normals carried the other way were made from the ones being replaced)
    ct.n_nrm = ct.n;
    if ((rc = launch_carry(ctx, rf.idx, rg.idx, cf.nrm64, cf.n, ct.n, (uint32_t *)ctx->carry_ws.p, ct.nrm64, 3))) {
        ct.n_nrm = 0;
        return rc;
    }
    ctx->carry.to = to;
    ctx->carry.run_f = ctx->nn_run[dir_f];
    ctx->carry.run_g = ctx->nn_run[dir_g];
    if (built) *built = 1;
    return PCCM_OK;
}

int pccm_merge_duplicates(pccm_ctx *ctx, int which, int mode, int64_t *n_out)
{
    CHECK_CTX(ctx);
    if (which != 0 && which != 1) return fail(PCCM_E_ARG, "cloud index must be 0 or 1");
    if (mode != PCCM_DUP_DROP && mode != PCCM_DUP_AVERAGE) return fail(PCCM_E_ARG, "mode must be PCCM_DUP_DROP or PCCM_DUP_AVERAGE");
    NOT_CAPTURING(ctx);
    Cloud &c = ctx->cloud[which];
    if (c.n <= 0) return fail(PCCM_E_STATE, "cloud %d is not set", which);
    if (ctx->sharded()) return fail(PCCM_E_STATE, "merging duplicates needs the whole cloud on this GPU (world = 1)");
    { int rcn = normals_ready(ctx, c); if (rcn) return rcn; }
    if (c.n_nrm != 0 && c.n_nrm != c.n)
        return fail(PCCM_E_STATE, "cloud %d has %lld points but %lld normals: rows cannot be merged", which, (long long)c.n, (long long)c.n_nrm);
    if (c.n_rgb != 0 && c.n_rgb != c.n)
        return fail(PCCM_E_STATE, "cloud %d has %lld points but %lld colours: rows cannot be merged", which, (long long)c.n, (long long)c.n_rgb);
    if (c.n_refl != 0 && c.n_refl != c.n)
        return fail(PCCM_E_STATE, "cloud %d has %lld points but %lld reflectance values: rows cannot be merged", which, (long long)c.n, (long long)c.n_refl);
    const int64_t n = c.n;
    int rc;
    if ((rc = ensure(ctx, ctx->merge_ws, merge_ws_bytes(n)))) return rc;
    const MergeLayout L = merge_layout(n);
    double *wd = (double *)ctx->merge_ws.p;
    uint32_t *ww = (uint32_t *)(wd + L.doubles);
    if ((rc = launch_merge_find(ctx, c.xyz64, n, ww))) return rc;
    uint32_t n_new = 0;
    PCCM_HIP(hipMemcpyAsync(&n_new, ww, sizeof(n_new), hipMemcpyDeviceToHost, ctx->stream));
    PCCM_HIP(hipStreamSynchronize(ctx->stream));
    if ((rc = check_device_errors(ctx))) return rc;
    if (n_new == 0 || (int64_t)n_new > n) return fail(PCCM_E_HIP, "merging duplicates counted %u groups in %lld rows", n_new, (long long)n);
    if (n_out) *n_out = (int64_t)n_new;
    if ((int64_t)n_new == n) return PCCM_OK;               // no duplicate: nothing is rewritten, nothing goes stale
    // rows go: what was made from the old rows goes with them, exactly as for new points (pccm_set_cloud below) -- normals that
    // were carried to this cloud among it: they are not merged
    const bool has_nrm = c.n_nrm == n && ctx->carry.to != which, has_rgb = c.n_rgb == n;
    const double *rgb = has_rgb ? c.rgb64 : nullptr;
    if (has_rgb && mode == PCCM_DUP_AVERAGE) {
        // the carry's passes with nn_F := rep: per representative the colours of its group, summed in ascending row order
        if ((rc = ensure(ctx, ctx->carry_ws, carry_ws_bytes(n, n)))) return rc;
        const int32_t *rep = (const int32_t *)(ww + L.rep);
        if ((rc = launch_carry(ctx, rep, nullptr, c.rgb64, n, n, (uint32_t *)ctx->carry_ws.p, wd, 3))) return rc;
        rgb = wd;
    }
    // the reflectance likewise, by the same passes over rows of one double: merge_refl holds the merged column [n] and, behind it,
    // the averages by original row [n]
    const bool has_refl = c.n_refl == n, refl_avg = has_refl && mode == PCCM_DUP_AVERAGE;
    const double *refl = has_refl ? c.refl64 : nullptr;
    double *rd = nullptr;
    if (has_refl) {
        if ((rc = ensure(ctx, ctx->merge_refl, (size_t)(refl_avg ? 2 : 1) * n * sizeof(double)))) return rc;
        rd = (double *)ctx->merge_refl.p;
    }
    if (refl_avg) {
        if ((rc = ensure(ctx, ctx->carry_ws, carry_ws_bytes(n, n)))) return rc;
        if ((rc = launch_carry(ctx, (const int32_t *)(ww + L.rep), nullptr, c.refl64, n, n, (uint32_t *)ctx->carry_ws.p, rd + n, 1))) return rc;
        refl = rd + n;
    }
    if ((rc = ensure(ctx, ctx->merge_map[which], (size_t)n * sizeof(int32_t)))) return rc;
    if ((rc = launch_merge_gather(ctx, c.xyz64, has_nrm ? c.nrm64 : nullptr, rgb, refl, n, wd + 3 * n, rd, ww, (int32_t *)ctx->merge_map[which].p)))
        return rc;
    // the merged rows enter the way any resident fp64 rows do (one ingest path: statistics, fp32 copies, invalidation)
    if ((rc = pccm_set_cloud(ctx, which, wd + 3 * n, (int64_t)n_new, PCCM_F64, 1))) return rc;
    if (has_nrm && (rc = pccm_set_normals(ctx, which, wd + 6 * n, (int64_t)n_new, PCCM_F64, 1))) return rc;
    if (has_rgb && (rc = pccm_set_colors(ctx, which, wd + 9 * n, (int64_t)n_new, PCCM_F64, 1))) return rc;
    if (has_refl && (rc = pccm_set_reflectance(ctx, which, rd, (int64_t)n_new, PCCM_F64, 1))) return rc;
    ctx->merge_n[which] = n;
    return PCCM_OK;
}

int pccm_get_merge_map(pccm_ctx *ctx, int which, int32_t *out, int64_t *n_before)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    if (which != 0 && which != 1) return fail(PCCM_E_ARG, "cloud index must be 0 or 1");
    const Cloud &c = ctx->cloud[which];
    if (c.n <= 0) return fail(PCCM_E_STATE, "cloud %d is not set", which);
    const int64_t nb = ctx->merge_n[which] ? ctx->merge_n[which] : c.n;
    if (n_before) *n_before = nb;
    if (!out) return PCCM_OK;
    if (!ctx->merge_n[which]) {                            // never merged: the identity
        for (int64_t i = 0; i < nb; ++i) out[i] = (int32_t)i;
        return PCCM_OK;
    }
    return fetch(ctx, out, ctx->merge_map[which].p, (size_t)nb * sizeof(int32_t));
}

int pccm_voxel_occupancy(pccm_ctx *ctx, int n, const double *voxels, int64_t *out)
{
    CHECK_CTX(ctx);
    if (!voxels || !out) return fail(PCCM_E_ARG, "null pointer");
    if (n < 1 || n > kOccupancyMax) return fail(PCCM_E_ARG, "a call takes 1..%d voxel sizes, not %d", kOccupancyMax, n);
    for (int k = 0; k < n; ++k)
        if (!std::isfinite(voxels[k]) || !(voxels[k] > 0.0)) return fail(PCCM_E_ARG, "voxel size %d is not a finite number > 0", k);
    NOT_CAPTURING(ctx);
    const Cloud &c0 = ctx->cloud[0], &c1 = ctx->cloud[1];
    for (int k = 0; k < 2; ++k)
        if (ctx->cloud[k].n <= 0) return fail(PCCM_E_STATE, "cloud %d is not set", k);
    if (ctx->sharded()) return fail(PCCM_E_STATE, "voxel occupancy needs the whole clouds on this GPU (world = 1)");
    if ((uint64_t)c0.n + (uint64_t)c1.n >= 0xffffffffull)
        return fail(PCCM_E_ARG, "voxel occupancy stores rows in 32-bit words: %lld + %lld rows are too many", (long long)c0.n, (long long)c1.n);
    const OccupancyLayout L = occupancy_layout(c0.n, c1.n);
    int rc;
    // behind the layout (whose end is 8-byte aligned): the tallies of each size, gathered for one copy back
    if ((rc = ensure(ctx, ctx->occupancy_ws, L.bytes() + (size_t)kOccupancyMax * 3 * sizeof(unsigned long long)))) return rc;
    uint32_t *ww = (uint32_t *)ctx->occupancy_ws.p;
    unsigned long long *all = (unsigned long long *)(ww + L.words);
    for (int k = 0; k < n; ++k) {
        if ((rc = launch_occupancy(ctx, c0.xyz64, c0.n, c1.xyz64, c1.n, voxels[k], ww))) return rc;
        PCCM_HIP(hipMemcpyAsync(all + 3 * k, ww + L.tally, 3 * sizeof(unsigned long long), hipMemcpyDeviceToDevice, ctx->stream));
    }
    unsigned long long t[3 * kOccupancyMax] = {};
    PCCM_HIP(hipMemcpyAsync(t, all, (size_t)n * 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    PCCM_HIP(hipStreamSynchronize(ctx->stream));
    if ((rc = check_device_errors(ctx))) return rc;
    for (int k = 0; k < n; ++k) {
        const unsigned long long uni = t[3 * k], a = t[3 * k + 1], both = t[3 * k + 2];
        if (a == 0 || a > uni || both > a || uni > (unsigned long long)(c0.n + c1.n))
            return fail(PCCM_E_HIP, "voxel occupancy counted %llu voxels, %llu of cloud 0 and %llu shared", uni, a, both);
        out[3 * k] = (int64_t)a;
        out[3 * k + 1] = (int64_t)(uni - a + both);       // |B| = |A u B| - |A| + |A n B|
        out[3 * k + 2] = (int64_t)both;
    }
    return PCCM_OK;
}

int pccm_get_points(pccm_ctx *ctx, int which, double *out)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    if (which != 0 && which != 1) return fail(PCCM_E_ARG, "cloud index must be 0 or 1");
    if (!out) return fail(PCCM_E_ARG, "null pointer");
    const Cloud &c = ctx->cloud[which];
    if (c.n <= 0) return fail(PCCM_E_STATE, "cloud %d is not set", which);
    return fetch(ctx, out, c.xyz64, (size_t)c.n * 3 * sizeof(double));
}

int pccm_get_colors(pccm_ctx *ctx, int which, double *out)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    if (which != 0 && which != 1) return fail(PCCM_E_ARG, "cloud index must be 0 or 1");
    if (!out) return fail(PCCM_E_ARG, "null pointer");
    const Cloud &c = ctx->cloud[which];
    if (c.n_rgb <= 0) return fail(PCCM_E_STATE, "cloud %d has no colours", which);
    return fetch(ctx, out, c.rgb64, (size_t)c.n_rgb * 3 * sizeof(double));
}

int pccm_get_reflectance(pccm_ctx *ctx, int which, double *out)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    if (which != 0 && which != 1) return fail(PCCM_E_ARG, "cloud index must be 0 or 1");
    if (!out) return fail(PCCM_E_ARG, "null pointer");
    const Cloud &c = ctx->cloud[which];
    if (c.n_refl <= 0) return fail(PCCM_E_STATE, "cloud %d has no reflectance", which);
    return fetch(ctx, out, c.refl64, (size_t)c.n_refl * sizeof(double));
}

int pccm_ssim_features(pccm_ctx *ctx, int which, int k, int attrs, int *built)
{
    CHECK_CTX(ctx);
    if (built) *built = 0;
    if (which != 0 && which != 1) return fail(PCCM_E_ARG, "cloud index must be 0 or 1");
    if (k < 2 || k > 64) return fail(PCCM_E_ARG, "PointSSIM neighbourhoods have 2..64 points, not %d", k);
    if (attrs <= 0 || attrs > 15) return fail(PCCM_E_ARG, "bad PointSSIM attribute mask %d", attrs);
    Cloud &c = ctx->cloud[which];
    if (c.n <= 0) return fail(PCCM_E_STATE, "cloud %d is not set", which);
    if (attrs & PCCM_SSIM_NORMAL) {
        if (!ctx->capturing) { int rcn = normals_ready(ctx, c); if (rcn) return rcn; }
        if (c.n_nrm != c.n || c.nrm_deferred) return fail(PCCM_E_STATE, "PointSSIM normal features need the normals of cloud %d", which);
    }
    if ((attrs & PCCM_SSIM_COLOR) && c.n_rgb != c.n) return fail(PCCM_E_STATE, "PointSSIM colour features need the colours of cloud %d", which);
    return ssim_features(ctx, which, k, attrs, built);    // (what is there already needs no work, and may be asked for while capturing)
}

int pccm_get_ssim_features(pccm_ctx *ctx, int which, int attr, double *out)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    if (which != 0 && which != 1) return fail(PCCM_E_ARG, "cloud index must be 0 or 1");
    if (!out) return fail(PCCM_E_ARG, "null pointer");
    if (attr != PCCM_SSIM_GEOMETRY && attr != PCCM_SSIM_NORMAL && attr != PCCM_SSIM_CURVATURE && attr != PCCM_SSIM_COLOR)
        return fail(PCCM_E_ARG, "one PointSSIM attribute expected, not %d", attr);
    const Cloud &c = ctx->cloud[which];
    if (!(c.ssim_attrs & attr)) return fail(PCCM_E_STATE, "cloud %d has no PointSSIM features of attribute %d", which, attr);
    const int a = attr == PCCM_SSIM_GEOMETRY ? 0 : attr == PCCM_SSIM_NORMAL ? 1 : attr == PCCM_SSIM_CURVATURE ? 2 : 3;
    return fetch(ctx, out, c.ssim64 + (size_t)a * c.n, (size_t)c.n * sizeof(double));
}

int pccm_resolution_build(pccm_ctx *ctx, int which, int K, int *built)
{
    CHECK_CTX(ctx);
    if (built) *built = 0;
    if (which != 0 && which != 1) return fail(PCCM_E_ARG, "cloud index must be 0 or 1");
    if (K < 1 || K > 63) return fail(PCCM_E_ARG, "point spacings average 1..63 neighbours, not %d", K);
    if (ctx->cloud[which].n <= 0) return fail(PCCM_E_STATE, "cloud %d is not set", which);
    if (ctx->sharded()) return fail(PCCM_E_STATE, "point spacings need the whole cloud on this GPU (world = 1)");
    return resolution_build(ctx, which, K, built);     // (what is there already needs no work, and may be asked for while capturing)
}

int pccm_get_resolution(pccm_ctx *ctx, int which, double *out)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    if (which != 0 && which != 1) return fail(PCCM_E_ARG, "cloud index must be 0 or 1");
    if (!out) return fail(PCCM_E_ARG, "null pointer");
    const Cloud &c = ctx->cloud[which];
    if (c.n <= 0 || c.res_k <= 0) return fail(PCCM_E_STATE, "the point spacings of cloud %d are not built (pccm_resolution_build)", which);
    return fetch(ctx, out, c.res64, (size_t)c.n * sizeof(double));
}

int pccm_p2d_build_attrs(pccm_ctx *ctx, int k, int attrs, int *built)
{
    CHECK_CTX(ctx);
    if (built) *built = 0;
    if (k < 4 || k > 64) return fail(PCCM_E_ARG, "point-to-distribution neighbourhoods have 4..64 points, not %d", k);
    if (attrs & ~(PCCM_P2D_GEOMETRY | PCCM_P2D_COLOR)) return fail(PCCM_E_ARG, "unknown point-to-distribution attributes 0x%x", attrs);
    for (int which = 0; which < 2; ++which)
        if (ctx->cloud[which].n <= 0) return fail(PCCM_E_STATE, "cloud %d is not set", which);
    if (ctx->sharded()) return fail(PCCM_E_STATE, "point-to-distribution columns need whole clouds on this GPU (world = 1)");
    if (attrs & PCCM_P2D_COLOR)
        for (int which = 0; which < 2; ++which)
            if (ctx->cloud[which].n_rgb != ctx->cloud[which].n)
                return fail(PCCM_E_STATE, "cloud %d has no colours (PCCM_P2D_COLOR)", which);
    return p2d_build(ctx, k, attrs, built);            // (what is there already needs no work, and may be asked for while capturing)
}

int pccm_p2d_build(pccm_ctx *ctx, int k, int *built)
{
    return pccm_p2d_build_attrs(ctx, k, PCCM_P2D_GEOMETRY, built);
}

int pccm_get_p2d_neighbours(pccm_ctx *ctx, int dir, int32_t *out, int32_t *count)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    if (dir != PCCM_DIR_LEFT && dir != PCCM_DIR_RIGHT) return fail(PCCM_E_ARG, "point-to-distribution exists for directions 0 and 1");
    if (!out || !count) return fail(PCCM_E_ARG, "null pointer");
    if (ctx->p2d_k <= 0) return fail(PCCM_E_STATE, "no point-to-distribution columns (pccm_p2d_build)");
    const int64_t n = ctx->cloud[dir].n;
    const int32_t *nbr, *cnt;
    int rc = p2d_neighbours(ctx, dir, ctx->p2d_k, &nbr, &cnt);
    if (rc) return rc;
    if ((rc = d2h(ctx, out, nbr, (size_t)n * ctx->p2d_k * sizeof(int32_t)))) return rc;
    if ((rc = d2h(ctx, count, cnt, (size_t)n * sizeof(int32_t)))) return rc;
    PCCM_HIP(hipStreamSynchronize(ctx->stream));
    return PCCM_OK;
}

int pccm_set_shard(pccm_ctx *ctx, int rank, int world)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    if (world < 1 || rank < 0 || rank >= world) return fail(PCCM_E_ARG, "bad shard %d of %d", rank, world);
    for (int d = 0; d < 3; ++d) {
        ctx->shard_rank[d] = rank;
        ctx->shard_world[d] = world;
    }
    shard_changed(ctx, kDirsAll);
    return PCCM_OK;
}

int pccm_set_shard_dir(pccm_ctx *ctx, int dir, int rank, int world)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    if (dir < 0 || dir > 2) return fail(PCCM_E_ARG, "bad direction %d", dir);
    if (world < 0 || (world > 0 && (rank < 0 || rank >= world))) return fail(PCCM_E_ARG, "bad shard %d of %d", rank, world);
    ctx->shard_rank[dir] = world > 0 ? rank : 0;
    ctx->shard_world[dir] = world;
    shard_changed(ctx, 1 << dir);
    return PCCM_OK;
}

int pccm_shard_range(pccm_ctx *ctx, int dir, int64_t *begin, int64_t *end)
{
    CHECK_CTX(ctx);
    if (!begin || !end) return fail(PCCM_E_ARG, "null pointer");
    const Cloud *it, *se;
    int rc = dir_clouds(ctx, dir, &it, &se);
    if (rc) return rc;
    shard_of(it->n, ctx->shard_rank[dir], ctx->shard_world[dir], begin, end);
    return PCCM_OK;
}

// shard range, result buffers and bookkeeping of one direction; *trivial = 1 when nothing is left to compute
static int prepare_nn(pccm_ctx *ctx, int dir, int *trivial)
{
    const Cloud *it, *se;
    int rc = dir_clouds(ctx, dir, &it, &se);
    if (rc) return rc;
    NNResult &res = ctx->nn[dir];
    results_void(ctx, 1 << dir);
    ctx->nn_run[dir]++;
    shard_of(it->n, ctx->shard_rank[dir], ctx->shard_world[dir], &res.begin, &res.end);
    const int64_t ns = res.end - res.begin;
    if (ctx->capturing) {
        GraphOp op;
        op.kind = 1;
        op.dir = dir;
        ctx->cap_ops.push_back(op);
    }
    if (ns > res.cap) {
        if (ctx->capturing) {
            ctx->capture_failed = true;
            return fail(PCCM_E_STATE, "result buffers must grow during graph capture: run pccm_nn once before capturing");
        }
        ctx->epoch++;
        PCCM_HIP(hipStreamSynchronize(ctx->stream));
        if (res.idx) (void)hipFree(res.idx);
        if (res.d2) (void)hipFree(res.d2);
        res.idx = nullptr;
        res.d2 = nullptr;
        res.cap = 0;
        PCCM_HIP(hipMalloc((void **)&res.idx, (size_t)ns * sizeof(int32_t)));
        PCCM_HIP(hipMalloc((void **)&res.d2, (size_t)ns * sizeof(double)));
        res.cap = ns;
    }
    {
        int rc2 = ensure(ctx, res.rec, (size_t)(ns > 0 ? ns : 1) * sizeof(double4));   // 32-byte result records (grid engine)
        if (rc2) return rc2;
    }
    res.form = ns <= 0 ? NNForm::columns() : NNForm{};      // an empty shard has nothing to unpack
    res.ties = dir == PCCM_DIR_SELF ? PCCM_TIES_PICK : ctx->ties;
    res.stats[0] = res.stats[1] = res.stats[2] = 0;
    *trivial = 0;
    if (dir == PCCM_DIR_SELF && it->n < 2) {
        // Open3D's compute_nearest_neighbor_distance returns zeros for fewer than two points
        if (ns > 0) {
            PCCM_HIP(hipMemsetAsync(res.idx, 0xff, (size_t)ns * sizeof(int32_t), ctx->stream));
            PCCM_HIP(hipMemsetAsync(res.d2, 0, (size_t)ns * sizeof(double), ctx->stream));
        }
        PCCM_HIP(hipMemsetAsync(res.nflag_dev, 0, 2 * sizeof(uint32_t), ctx->stream));
        res.form = NNForm::columns();
        *trivial = 1;
    }
    return PCCM_OK;
}

static int pick_engine(int engine)
{
    if (engine != PCCM_ENGINE_AUTO) return engine;
    const char *e = getenv("PCCM_ENGINE");
    if (e && !strcmp(e, "brute")) return PCCM_ENGINE_BRUTE;
    return PCCM_ENGINE_GRID;
}

static int run_nn(pccm_ctx *ctx, int ndirs, const int *dirs, int engine)
{
    unsigned mask = 0;
    for (int k = 0; k < ndirs; ++k) mask |= 1u << dirs[k];
    PathScope path(ctx, mask);
    const bool automatic = engine == PCCM_ENGINE_AUTO && !getenv("PCCM_ENGINE");
    engine = pick_engine(engine);
    if (automatic && ctx->cloud[0].n > 0 && ctx->cloud[1].n > 0) {
        // distributions no uniform grid can separate (see decide_scale) go to the engine whose cost is flat
        bool hostile = false;
        int rc = grid_decide(ctx, &hostile);
        if (rc) return rc;
        if (!hostile && (rc = grid_prefers_brute(ctx, &hostile))) return rc;
        if (hostile) engine = PCCM_ENGINE_BRUTE;
    }
    if (engine != PCCM_ENGINE_BRUTE && engine != PCCM_ENGINE_GRID) return fail(PCCM_E_ARG, "unknown engine %d", engine);
    int todo[3], ntodo = 0, rc;
    for (int k = 0; k < ndirs; ++k) {
        int trivial = 0;
        if ((rc = prepare_nn(ctx, dirs[k], &trivial))) return rc;
        if (!trivial) todo[ntodo++] = dirs[k];
    }
    if (engine == PCCM_ENGINE_GRID) {
        if (ntodo > 0 && (rc = nn_grid(ctx, ntodo, todo))) return rc;
    } else {
        for (int k = 0; k < ntodo; ++k) {
            const Cloud *it, *se;
            if ((rc = dir_clouds(ctx, todo[k], &it, &se))) return rc;
            ctx->nn[todo[k]].form = NNForm::columns();            // the brute-force engine writes the plain columns
            if ((rc = nn_brute(ctx, *it, *se, todo[k] == PCCM_DIR_SELF, ctx->nn[todo[k]]))) return rc;
        }
    }
    for (int k = 0; k < ndirs; ++k) ctx->nn[dirs[k]].valid = true;
    return PCCM_OK;
}

int pccm_nn(pccm_ctx *ctx, int dir, int engine)
{
    CHECK_CTX(ctx);
    if (dir < 0 || dir > 2) return fail(PCCM_E_ARG, "bad direction %d", dir);
    return run_nn(ctx, 1, &dir, engine);
}

int pccm_nn_pair(pccm_ctx *ctx, int engine)
{
    CHECK_CTX(ctx);
    const int dirs[2] = {PCCM_DIR_LEFT, PCCM_DIR_RIGHT};
    return run_nn(ctx, 2, dirs, engine);
}

// The result of direction `dir`, for a reader.  A direction whose tails lie filed (NNForm::tails_filed: a capture left the tail
// launch out for the settling reduction) has the classic tail launch settle them first, for every reader but the reduction batch
// itself (binds: slot_prepare -- launch_unit_jobs decides there, job by job).
static int need_nn(pccm_ctx *ctx, int dir, const Cloud **it, const Cloud **se, NNResult **res, bool binds = false)
{
    int rc = dir_clouds(ctx, dir, it, se);
    if (rc) return rc;
    *res = &ctx->nn[dir];
    if (!(*res)->valid) return fail(PCCM_E_STATE, "pccm_nn(dir=%d) has not run for the current clouds/shard", dir);
    if ((*res)->form.tails_filed && !binds) return filed_tails_resolve(ctx);
    return PCCM_OK;
}

// the plain idx / d2 columns of a result: the grid engine leaves 32-byte records, unpacked here when somebody
// wants columns (getters, colour kernels, the separate point kernel)
static int ensure_plain(pccm_ctx *ctx, NNResult &res, bool need_idx)
{
    if (res.form.tails_filed) {                    // (the records are about to be read or rewritten: need_nn)
        const int rc = filed_tails_resolve(ctx);
        if (rc) return rc;
    }
    if (res.form.plain_ready(need_idx)) return PCCM_OK;
    if (!res.form.has_records()) return fail(PCCM_E_STATE, "no nearest-neighbour result to read");
    const int dir = (int)(&res - ctx->nn);
    if (need_idx && res.form.rows_need_repeat()) {
        // the search ran without the matched rows (pccm_nn_want_idx off) and now somebody asks for them: run it again
        // for this direction with the rows on -- same results, 32-byte records; the clouds and the grid are resident
        if (ctx->capturing) {
            ctx->capture_failed = true;
            return fail(PCCM_E_STATE, "matched rows are needed during graph capture: switch pccm_nn_want_idx on before the search");
        }
        PathScope path(ctx, 1u << dir);
        int rc = nn_grid(ctx, 1, &dir, /*force_idx=*/1);
        if (rc) return rc;
        records_rewritten(ctx, dir);           // (jobs bound to the old records must not be read again: pccm_stale.h)
    }
    const bool rows = res.form.has_rows();
    const Cloud &uit = ctx->cloud[dir == PCCM_DIR_RIGHT ? 1 : 0];
    int rc = launch_unpack(ctx, (const double *)res.rec.p, res.form.stride(), res.form.layout(), uit.xyz32r, res.begin, res.end - res.begin,
                           rows ? res.idx : nullptr, res.d2);
    if (rc) return rc;
    res.form.plain = rows ? NNForm::kPlainAll : NNForm::kPlainD2;
    return PCCM_OK;
}

// PCCM_TIES_MEAN: the virtual neighbours of the shard's rows of direction `dir` (0 or 1), made once per search and kept;
// want_nrm / want_rgb: the averaged normals (the caller has checked them: check_normals) / colours too; want_ang: the tie-set mean
// of PCCM_METRIC_ANGULAR (the caller has checked both clouds' normals: check_angular)
static int ensure_ties(pccm_ctx *ctx, int dir, bool want_nrm, bool want_rgb, bool want_ang)
{
    pccm_ctx::TieCols &t = ctx->tie[dir];
    NNResult &res = ctx->nn[dir];
    const Cloud &se = ctx->cloud[dir == PCCM_DIR_LEFT ? 1 : 0];
    const Cloud &it = ctx->cloud[dir == PCCM_DIR_LEFT ? 0 : 1];
    // the colours the searched cloud has on the device ride along (one walk per direction and search, not one per consumer);
    // what is wanted but missing is not averaged (the consumers report the missing normals / colours themselves)
    const bool nrm_on = se.n_nrm == se.n && !se.nrm_deferred, rgb_on = se.n_rgb == se.n;
    const bool ang_on = nrm_on && it.n_nrm == it.n && !it.nrm_deferred;
    want_nrm = want_nrm && nrm_on;
    want_rgb = want_rgb && rgb_on;
    want_ang = want_ang && ang_on;
    const bool fresh = t.gen == ctx->nn_gen[dir];
    const bool have_nrm = fresh && t.nrm_gen == ctx->nrm_gen, have_rgb = fresh && t.rgb_gen == ctx->rgb_gen;
    const bool have_ang = fresh && t.ang_gen == ctx->nrm_gen;
    if (fresh && (!want_nrm || have_nrm) && (!want_rgb || have_rgb) && (!want_ang || have_ang)) return PCCM_OK;
    if (ctx->capturing) {
        ctx->capture_failed = true;
        return fail(PCCM_E_STATE, "PCCM_TIES_MEAN cannot be captured in a graph");
    }
    want_nrm = (want_nrm || have_nrm) && nrm_on;            // (averaged normals only where a neighbour-indexed projection asks)
    want_ang = (want_ang || have_ang) && ang_on;            // (... and the angular column only where a report asks for it)
    want_rgb = rgb_on;
    int rc = ensure_plain(ctx, res, true);
    if (rc) return rc;
    const int64_t ns = res.end - res.begin;
    const size_t n3 = (size_t)(ns > 0 ? ns : 1) * 3 * sizeof(double);
    if ((rc = ensure(ctx, t.pos, n3)) || (rc = ensure(ctx, t.k, (size_t)(ns + 1) * sizeof(int32_t)))) return rc;   // (+ the scan count)
    if (want_nrm && (rc = ensure(ctx, t.nrm, n3))) return rc;
    if (want_rgb && (rc = ensure(ctx, t.rgb, n3))) return rc;
    if (want_ang && (rc = ensure(ctx, t.ang, (size_t)(ns > 0 ? ns : 1) * sizeof(double)))) return rc;
    t.gen = 0;
    PathScope path(ctx, 1u << dir, /*keep=*/true);
    rc = tie_mean(ctx, dir, res.idx, res.d2, res.begin, ns, want_nrm ? se.nrm64 : nullptr, want_rgb ? se.rgb64 : nullptr, (double *)t.pos.p,
                  (int32_t *)t.k.p, (double *)t.nrm.p, (double *)t.rgb.p, want_ang ? it.nrm64 : nullptr, want_ang ? se.nrm64 : nullptr,
                  want_ang ? (double *)t.ang.p : nullptr);
    if (rc) return rc;
    // behind the k column: how many of these queries the pass left to the exact scan (pccm_nn_stats, PCCM_STATS_TIES)
    if (ns > 0) PCCM_HIP(hipMemcpyAsync((int32_t *)t.k.p + ns, ctx->tie_list.p, sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
    else PCCM_HIP(hipMemsetAsync(t.k.p, 0, sizeof(int32_t), ctx->stream));
    t.gen = ctx->nn_gen[dir];
    t.nrm_gen = want_nrm ? ctx->nrm_gen : 0;
    t.rgb_gen = want_rgb ? ctx->rgb_gen : 0;
    t.ang_gen = want_ang ? ctx->nrm_gen : 0;
    return PCCM_OK;
}

int pccm_set_ties(pccm_ctx *ctx, int policy)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    if (policy != PCCM_TIES_PICK && policy != PCCM_TIES_MEAN) return fail(PCCM_E_ARG, "unknown tie policy %d", policy);
    if (ctx->ties != policy) {
        ctx->ties = policy;
        ctx->epoch++;                                        // captured searches carry the old policy
    }
    return PCCM_OK;
}

int pccm_tie_counts(pccm_ctx *ctx, int dir, int32_t *k)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    if (!k) return fail(PCCM_E_ARG, "null pointer");
    if (dir != PCCM_DIR_LEFT && dir != PCCM_DIR_RIGHT) return fail(PCCM_E_ARG, "ties are resolved for directions 0 and 1");
    const Cloud *it, *se;
    NNResult *res;
    int rc = need_nn(ctx, dir, &it, &se, &res);
    if (rc) return rc;
    if (res->ties != PCCM_TIES_MEAN) return fail(PCCM_E_STATE, "the search of direction %d did not run under PCCM_TIES_MEAN", dir);
    if ((rc = ensure_ties(ctx, dir, false, false))) return rc;
    const int64_t ns = res->end - res->begin;
    if (ns > 0 && (rc = d2h(ctx, k, ctx->tie[dir].k.p, (size_t)ns * sizeof(int32_t)))) return rc;
    PCCM_HIP(hipStreamSynchronize(ctx->stream));
    return check_device_errors(ctx);
}

int pccm_nn_want_idx(pccm_ctx *ctx, int on)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    if ((ctx->want_idx != 0) != (on != 0)) {
        ctx->want_idx = on ? 1 : 0;
        ctx->epoch++;                                        // captured searches carry the old record layout
    }
    return PCCM_OK;
}

int pccm_nn_fuse(pccm_ctx *ctx, int dir, int normal_mode)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    if (dir != PCCM_DIR_LEFT && dir != PCCM_DIR_RIGHT) return fail(PCCM_E_ARG, "the projection exists for directions 0 and 1");
    if (normal_mode != -1 && normal_mode != PCCM_NORMAL_ROW && normal_mode != PCCM_NORMAL_NEIGHBOUR)
        return fail(PCCM_E_ARG, "bad normal mode %d", normal_mode);
    if (ctx->fuse_mode[dir] != normal_mode) {
        ctx->fuse_mode[dir] = normal_mode;
        ctx->epoch++;                                        // captured searches carry the old choice
    }
    return PCCM_OK;
}

int pccm_nn_fetch(pccm_ctx *ctx, int dir, int32_t *idx, double *d2)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    const Cloud *it, *se;
    NNResult *res;
    int rc = need_nn(ctx, dir, &it, &se, &res);
    if (rc) return rc;
    if ((rc = ensure_plain(ctx, *res, idx != nullptr))) return rc;
    const int64_t ns = res->end - res->begin;
    if (ns > 0 && idx) { int rcd = d2h(ctx, idx, res->idx, (size_t)ns * sizeof(int32_t)); if (rcd) return rcd; }
    if (ns > 0 && d2) { int rcd = d2h(ctx, d2, res->d2, (size_t)ns * sizeof(double)); if (rcd) return rcd; }
    PCCM_HIP(hipStreamSynchronize(ctx->stream));
    return check_device_errors(ctx);
}

static int check_normals(pccm_ctx *ctx, const Cloud &it, const Cloud &se, const NNResult &res, int normal_mode)
{
    if (normal_mode != PCCM_NORMAL_ROW && normal_mode != PCCM_NORMAL_NEIGHBOUR)
        return fail(PCCM_E_ARG, "bad normal mode %d", normal_mode);
    {   // whoever checks the normals is about to read them: announced ones (pccm_set_normals_deferred) cross PCIe now
        int rcn = normals_ready(ctx, const_cast<Cloud &>(se));
        if (rcn) return rcn;
    }
    if (se.n_nrm <= 0) return fail(PCCM_E_STATE, "the searched cloud has no normals (pccm_set_normals)");
    // sharded: the test is on the whole iterating cloud, so that every rank raises (or none does) -- a per-shard test
    // would let the low ranks walk into the exchange while the last one raises
    if (normal_mode == PCCM_NORMAL_ROW && (ctx->sharded() ? it.n : res.end) > se.n_nrm)
        return fail(PCCM_E_RANGE, "index %lld is out of bounds for axis 0 with size %lld (row-indexed normals, reference quirk Q1)",
                    (long long)se.n_nrm, (long long)se.n_nrm);
    if (normal_mode == PCCM_NORMAL_NEIGHBOUR && se.n_nrm != se.n)
        return fail(PCCM_E_ARG, "neighbour-indexed normals need one normal per point");
    return PCCM_OK;
}

// PCCM_METRIC_ANGULAR reads the normals of BOTH clouds (the iterating row's and the matched row's; normal_mode does not apply)
static int check_angular(pccm_ctx *ctx, int dir, const Cloud &it, const Cloud &se)
{
    if (dir == PCCM_DIR_SELF) return fail(PCCM_E_ARG, "angular similarity is not defined for the self search");
    for (const Cloud *c : {&it, &se}) {      // announced normals (pccm_set_normals_deferred) cross PCIe now
        int rcn = normals_ready(ctx, const_cast<Cloud &>(*c));
        if (rcn) return rcn;
    }
    if (it.n_nrm <= 0 || se.n_nrm <= 0) return fail(PCCM_E_STATE, "angular similarity needs the normals of both clouds (pccm_set_normals)");
    if (it.n_nrm != it.n || se.n_nrm != se.n) return fail(PCCM_E_ARG, "angular similarity needs one normal per point");
    return PCCM_OK;
}

// PCCM_METRIC_SSIM_*: both clouds' feature columns of the attribute, made at the same k (pccm_ssim_features)
static int check_ssim(pccm_ctx *ctx, int dir, const Cloud &it, const Cloud &se, const NNResult &res, int metric)
{
    if (dir == PCCM_DIR_SELF) return fail(PCCM_E_ARG, "PointSSIM similarity is not defined for the self search");
    if (res.ties == PCCM_TIES_MEAN) return fail(PCCM_E_STATE, "PointSSIM similarity is not defined under PCCM_TIES_MEAN");
    const int bit = 1 << (metric - PCCM_METRIC_SSIM_GEOMETRY);
    if (!(it.ssim_attrs & bit) || !(se.ssim_attrs & bit) || it.ssim_k != se.ssim_k)
        return fail(PCCM_E_STATE, "PointSSIM similarity needs both clouds' features at the same k (pccm_ssim_features)");
    return PCCM_OK;
}

// PCCM_METRIC_REFLECTANCE: one reflectance per point on both clouds (pccm_set_reflectance*)
static int check_reflectance(int dir, const Cloud &it, const Cloud &se, const NNResult &res)
{
    if (dir == PCCM_DIR_SELF) return fail(PCCM_E_ARG, "the reflectance error is not defined for the self search");
    if (res.ties == PCCM_TIES_MEAN) return fail(PCCM_E_STATE, "the reflectance error is not defined under PCCM_TIES_MEAN");
    if (it.n_refl != it.n || se.n_refl != se.n)
        return fail(PCCM_E_STATE, "the reflectance error needs the reflectance of both clouds (pccm_set_reflectance)");
    return PCCM_OK;
}

// the feature column of a PCCM_METRIC_SSIM_* metric
static const double *ssim_column(const Cloud &c, int metric)
{
    return c.ssim64 + (size_t)(metric - PCCM_METRIC_SSIM_GEOMETRY) * c.n;
}

// columns that compare a row with its matched row (PCCM_METRIC_ANGULAR, PCCM_METRIC_SSIM_*, PCCM_METRIC_REFLECTANCE): normal_mode
// does not apply
static bool matched_column(int metric)
{
    return metric == PCCM_METRIC_ANGULAR || is_ssim_metric(metric) || metric == PCCM_METRIC_REFLECTANCE;
}

// PCCM_METRIC_P2D*: a stored column of the direction (pccm_p2d_build_attrs); neither the matched rows nor normal_mode enter it
static int check_p2d(pccm_ctx *ctx, int dir, int metric)
{
    if (dir == PCCM_DIR_SELF) return fail(PCCM_E_ARG, "point-to-distribution is not defined for the self search");
    if (ctx->p2d_k <= 0) return fail(PCCM_E_STATE, "point-to-distribution columns are not built (pccm_p2d_build)");
    if (metric != PCCM_METRIC_P2D && !ctx->p2d_color)
        return fail(PCCM_E_STATE, "point-to-distribution colour columns are not built (pccm_p2d_build_attrs, PCCM_P2D_COLOR)");
    return PCCM_OK;
}

// PCCM_METRIC_RESOLUTION: the stored spacing column of the cloud the direction iterates (pccm_resolution_build)
static int check_resolution(const pccm_ctx *ctx, int dir)
{
    if (dir == PCCM_DIR_SELF) return fail(PCCM_E_ARG, "the spacing column belongs to directions 0 and 1, not to the self search");
    if (ctx->cloud[dir].res_k <= 0) return fail(PCCM_E_STATE, "the point spacings of cloud %d are not built (pccm_resolution_build)", dir);
    return PCCM_OK;
}

// the column of a stored metric (is_stored_metric) that column_check has passed
static const double *stored_column(const pccm_ctx *ctx, int dir, int metric)
{
    if (metric == PCCM_METRIC_RESOLUTION) return ctx->cloud[dir].res64;
    return metric == PCCM_METRIC_P2D ? ctx->p2d64[dir] : ctx->p2d_cj64[dir][metric - PCCM_METRIC_P2D_COLOR];
}

// What a (dir, metric, normal_mode) request of the direction's search needs before any column is bound -- one answer for
// pccm_point_metric, the reductions and the selections: the metric exists, it is defined for this search, its operands are there.
static int column_check(pccm_ctx *ctx, int dir, int metric, int normal_mode, const Cloud &it, const Cloud &se, const NNResult &res)
{
    if (metric == PCCM_METRIC_D1) return PCCM_OK;
    if (metric == PCCM_METRIC_ANGULAR) return check_angular(ctx, dir, it, se);
    if (is_ssim_metric(metric)) return check_ssim(ctx, dir, it, se, res, metric);
    if (metric == PCCM_METRIC_REFLECTANCE) return check_reflectance(dir, it, se, res);
    if (is_p2d_metric(metric)) return check_p2d(ctx, dir, metric);
    if (metric == PCCM_METRIC_RESOLUTION) return check_resolution(ctx, dir);
    if (!normal_mode_enters(metric)) return fail(PCCM_E_ARG, "bad metric %d", metric);
    if (dir == PCCM_DIR_SELF) return fail(PCCM_E_ARG, "point-to-plane is not defined for the self search");
    return check_normals(ctx, it, se, res, normal_mode);
}

// The k_point_jobs job of a checked request (column_check): the D2 / PROJ / ANGULAR / SSIM_* / REFLECTANCE column of the shard's rows into out
// ([ns]), or -- PCCM_METRIC_D1 -- their error vectors ([ns][3]).  recs: the matched rows are read from the direction's matched
// records in place (ColumnSource::recs); otherwise from the plain idx column, which the caller has made ready.
static int point_job_fill(pccm_ctx *ctx, int dir, int metric, int normal_mode, double *out, bool recs, const Cloud &it, const Cloud &se,
                          const NNResult &res, PointJob &P)
{
    const bool matched = matched_column(metric), ssim = is_ssim_metric(metric);
    P.q64 = it.xyz64; P.r64 = se.xyz64;
    const bool refl = metric == PCCM_METRIC_REFLECTANCE;
    P.nrm = ssim ? ssim_column(se, metric) : refl ? se.refl64 : se.nrm64;
    P.inrm = !matched ? nullptr : ssim ? ssim_column(it, metric) : refl ? it.refl64 : it.nrm64;
    P.c64 = P.cn64 = nullptr;
    if (!matched && res.ties == PCCM_TIES_MEAN) {           // the virtual neighbours, and their averaged normals where they are indexed
        const bool nmean = normal_mode_enters(metric) && normal_mode == PCCM_NORMAL_NEIGHBOUR;
        int rc = ensure_ties(ctx, dir, nmean, false);
        if (rc) return rc;
        P.c64 = (const double *)ctx->tie[dir].pos.p;
        if (nmean) P.cn64 = (const double *)ctx->tie[dir].nrm.p;
    }
    P.idx = recs ? nullptr : res.idx;
    P.recs = recs ? (const float4 *)res.rec.p : nullptr;
    P.q_begin = res.begin; P.metric = metric; P.normal_mode = matched ? PCCM_NORMAL_NEIGHBOUR : normal_mode; P.val = out;
    return PCCM_OK;
}

// The getters' point pass: one job, always from the plain columns -- pccm_point_metric forms D2 / PROJ here even when the records
// hold a fused projection, and the matched columns from idx, not from matched records: an operand route apart from the reductions'
static int point_pass(pccm_ctx *ctx, int dir, int metric, int normal_mode, double *out, const Cloud &it, const Cloud &se, NNResult &res)
{
    int rc = ensure_plain(ctx, res, true);
    if (rc) return rc;
    PointJobs pj = {};
    pj.njobs = 1;
    pj.off[1] = res.end - res.begin;
    if ((rc = point_job_fill(ctx, dir, metric, normal_mode, out, false, it, se, res, pj.j[0]))) return rc;
    return launch_point_jobs(ctx, pj);
}

int pccm_error_vectors(pccm_ctx *ctx, int dir, double *out)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    if (!out) return fail(PCCM_E_ARG, "null pointer");
    const Cloud *it, *se;
    NNResult *res;
    int rc = need_nn(ctx, dir, &it, &se, &res);
    if (rc) return rc;
    const int64_t ns = res->end - res->begin;
    if (ns <= 0) return PCCM_OK;
    if ((rc = ensure(ctx, ctx->val, (size_t)ns * 3 * sizeof(double)))) return rc;
    if ((rc = point_pass(ctx, dir, PCCM_METRIC_D1, PCCM_NORMAL_ROW, (double *)ctx->val.p, *it, *se, *res))) return rc;
    { int rcd = d2h(ctx, out, ctx->val.p, (size_t)ns * 3 * sizeof(double)); if (rcd) return rcd; }
    PCCM_HIP(hipStreamSynchronize(ctx->stream));
    return PCCM_OK;
}

// device pointer to the shard's per-point metric (computing it into ctx->val when needed)
static int metric_on_device(pccm_ctx *ctx, int dir, int metric, int normal_mode, const double **dev, int64_t *ns_out)
{
    const Cloud *it, *se;
    NNResult *res;
    int rc = need_nn(ctx, dir, &it, &se, &res);
    if (rc) return rc;
    const int64_t ns = res->end - res->begin;
    *ns_out = ns;
    if ((rc = column_check(ctx, dir, metric, normal_mode, *it, *se, *res))) return rc;
    if (metric == PCCM_METRIC_D1) {
        if ((rc = ensure_plain(ctx, *res, false))) return rc;
        *dev = res->d2;
    } else if (is_stored_metric(metric)) {
        *dev = stored_column(ctx, dir, metric) + res->begin;
    } else if (metric == PCCM_METRIC_ANGULAR && res->ties == PCCM_TIES_MEAN) {     // the tie pass makes the column
        if ((rc = ensure_ties(ctx, dir, false, false, true))) return rc;
        *dev = (const double *)ctx->tie[dir].ang.p;
    } else {
        if ((rc = ensure(ctx, ctx->val, (size_t)(ns > 0 ? ns : 1) * sizeof(double)))) return rc;
        if ((rc = point_pass(ctx, dir, metric, normal_mode, (double *)ctx->val.p, *it, *se, *res))) return rc;
        *dev = (const double *)ctx->val.p;
    }
    return PCCM_OK;
}

int pccm_tie_exposure(pccm_ctx *ctx, int dir, int normal_mode, double out[8])
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    if (!out) return fail(PCCM_E_ARG, "null pointer");
    if (dir != PCCM_DIR_LEFT && dir != PCCM_DIR_RIGHT) return fail(PCCM_E_ARG, "tie exposure exists for directions 0 and 1");
    const Cloud *it, *se;
    NNResult *res;
    int rc = need_nn(ctx, dir, &it, &se, &res);
    if (rc) return rc;
    if (normal_mode >= 0 && (rc = check_normals(ctx, *it, *se, *res, normal_mode))) return rc;
    if ((rc = ensure_plain(ctx, *res, true))) return rc;
    PathScope path(ctx, 1u << dir, /*keep=*/true);
    return tie_exposure(ctx, dir, *it, *se, *res, normal_mode, out);
}

int pccm_point_metric(pccm_ctx *ctx, int dir, int metric, int normal_mode, double *out)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    if (!out) return fail(PCCM_E_ARG, "null pointer");
    const double *dev;
    int64_t ns;
    int rc = metric_on_device(ctx, dir, metric, normal_mode, &dev, &ns);
    if (rc) return rc;
    if (ns > 0) { int rcd = d2h(ctx, out, dev, (size_t)ns * sizeof(double)); if (rcd) return rcd; }
    PCCM_HIP(hipStreamSynchronize(ctx->stream));
    return PCCM_OK;
}

int64_t pccm_xvec_len(int64_t n_iter) { return slot_shape(n_iter, 0, n_iter).xvec_len(); }

// ---- reductions: enqueue (prefetch) and consume ---------------------------------------------------------
// A reduction is enqueued into a slot: point kernel (D2/PROJ) -> per-unit sums/min/max -> async copy of
// the unit arrays and of the shard's raw tail values into pinned host memory -> event.  pccm_reduce()
// consumes a slot (enqueuing it first when nobody prefetched it), so a caller that prefetches every
// column it will need waits for the GPU once per step instead of once per column.

// Until a slot's numbers are on the host.  PCCM_WAIT_SPIN: a wave behind the batch's last kernel bumps the context's completion
// counter once they are (k_publish, pccm_point.hip), and the host watches that word -- the runtime's event completion path
// wakes a waiting thread ~13 us after the kernel ends.  The spin is bounded: past kSpinBound, or for a
// slot the counter does not cover (wait_seq 0), the batch event says it, and reports a fault or a hang as a HIP error.
static int wait_batch(pccm_ctx *ctx, uint64_t want, hipEvent_t wait_ev)
{
    constexpr auto kSpinBound = std::chrono::milliseconds(2);
    if (ctx->wait_mode == PCCM_WAIT_SPIN && want) {
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned k = 0;; ++k) {
            if (__atomic_load_n(ctx->done, __ATOMIC_ACQUIRE) >= want) return PCCM_OK;
            __builtin_ia32_pause();
            if ((k & 255) == 255 && std::chrono::steady_clock::now() - t0 > kSpinBound) break;
        }
    }
#ifdef PCCM_DIAG
    if (ctx->wait_mode == 2 && wait_ev) {
        hipError_t e;
        while ((e = hipEventQuery(wait_ev)) == hipErrorNotReady) __builtin_ia32_pause();
        PCCM_HIP(e);
        return PCCM_OK;
    }
#endif
    if (wait_ev) PCCM_HIP(hipEventSynchronize(wait_ev));
    return PCCM_OK;
}

// ---- one life cycle for the slots of every table ("A reduction slot") --------------------------------------------
extern "C++" {       // (templates)
// The slots a call takes for its new requests.  It acquires a slot, describes the request in it and marks it pending before it
// acquires the next (pick_free and find_pending then see it while the batch is assembled); finish() follows the last launch.
template <class Slot, size_t N>
struct SlotBatch {
    pccm_ctx *ctx;
    Slot (&table)[N];
    Slot *fresh[8] = {};
    int nfresh = 0;
    SlotBatch(pccm_ctx *c, Slot (&t)[N]) : ctx(c), table(t) {}

    // a slot for a new request, idle; a pending one of another call is waited for first (its kernels may still write its host outputs)
    int acquire(const char *none_free, Slot **out)
    {
        Slot *s = pick_free(table, fresh, nfresh, ctx->nn_gen);
        if (!s) return fail(PCCM_E_STATE, "%s", none_free);
        int rc = s->pending && !ctx->capturing && s->wait_ev ? wait_batch(ctx, s->wait_seq, s->wait_ev) : PCCM_OK;
        if (rc) return rc;
        s->pending = false;
        fresh[nfresh++] = s;
        *out = s;
        return PCCM_OK;
    }

    // seq: the batch's count on the completion counter (while capturing: its ordinal in the captured sequence).  Eagerly one record
    // of the batch event serves every slot; a capture keeps the slots' snapshots, and whoever launches the graph arms them (rearm).
    int finish(uint64_t seq)
    {
        for (int k = 0; k < nfresh; ++k) {
            Slot &s = *fresh[k];
            s.wait_seq = seq;
            s.wait_ev = ctx->capturing ? nullptr : ctx->batch_ev;
            if (!ctx->capturing) continue;
            GraphOp op;
            op.slot = (int)(&s - table);
            op.snap = snapshot(s);
            op.kind = 2 + (int)op.snap.index();
            ctx->cap_ops.push_back(op);
        }
        if (!ctx->capturing) PCCM_HIP(hipEventRecord(ctx->batch_ev, ctx->stream));
        return PCCM_OK;
    }
};

// A captured batch runs again: its slot takes the snapshot's description back, for the generation its direction has by now.
template <class Slot>
static int slot_replay(pccm_ctx *ctx, Slot &s, const SlotSnap<typename Slot::What> &snap)
{
    const bool in_use = s.pending && s.gen == ctx->nn_gen[s.dir] && s.wait_ev;       // by someone else, still
    int rc = in_use ? wait_batch(ctx, s.wait_seq, s.wait_ev) : PCCM_OK;
    if (rc) return rc;
    restore(s, snap);
    s.gen = ctx->nn_gen[s.dir];
    s.pending = true;
    rearm(s, ctx, snap.key.wait_seq);
    return PCCM_OK;
}

// Consume n <= 8 requests: find(i) is request i's pending slot (null: `lost`), read(i, slot) takes its numbers once they are on
// the host.  The slots stay pending until every request is read.
template <class Find, class Read>
static int consume(pccm_ctx *ctx, int n, const char *lost, Find find, Read read)
{
    decltype(find(0)) got[8];
    for (int i = 0; i < n; ++i) {
        auto *s = find(i);
        if (!s) return fail(PCCM_E_STATE, "%s", lost);
        int rc = wait_batch(ctx, s->wait_seq, s->wait_ev);
        if (!rc) rc = check_device_errors(ctx);
        if (rc) return rc;
        read(i, *s);
        got[i] = s;
    }
    for (int i = 0; i < n; ++i) got[i]->pending = false;
    return PCCM_OK;
}

// What selections, counts and mapped reductions (`what`) ask of their requests alike: 1..8 of them with every array there
// (`arrays`), the whole columns on this GPU, directions 0 and 1, D1 / D2 columns, a search behind each.  Request i's own key is
// checked by key_first(i) before the search is asked for, and by key_last(i, iterating cloud) behind it.
template <class KeyFirst, class KeyLast>
static int request_check(pccm_ctx *ctx, const char *who, const char *what, int n, bool arrays, const int *dirs, const int *metrics,
                         KeyFirst key_first, KeyLast key_last)
{
    if (n < 0 || n > 8 || (n > 0 && !arrays)) return fail(PCCM_E_ARG, "1..8 requests expected");
    if (ctx->sharded()) return fail(PCCM_E_STATE, "%s needs the whole columns on this GPU (world = 1)", who);
    for (int i = 0; i < n; ++i) {
        if (dirs[i] != PCCM_DIR_LEFT && dirs[i] != PCCM_DIR_RIGHT) return fail(PCCM_E_ARG, "%s read directions 0 and 1, not %d", what, dirs[i]);
        if (metrics[i] != PCCM_METRIC_D1 && metrics[i] != PCCM_METRIC_D2)
            return fail(PCCM_E_ARG, "%s read PCCM_METRIC_D1 and PCCM_METRIC_D2 columns, not metric %d", what, metrics[i]);
        const Cloud *it, *se;
        NNResult *res;
        int rc = key_first(i);
        if (!rc) rc = need_nn(ctx, dirs[i], &it, &se, &res);
        if (!rc) rc = key_last(i, *it);
        if (rc) return rc;
    }
    return PCCM_OK;
}
}  // extern "C++"

// A slot's pinned host block holds `doubles` doubles at least.  Growing it moves what a captured graph writes to: captured graphs
// go stale, and a capture in progress fails with `while_capturing`.
static int host_reserve(pccm_ctx *ctx, SlotHost &h, int64_t doubles, const char *while_capturing)
{
    const size_t need = (size_t)doubles * sizeof(double);
    if (need <= h.host_cap) return PCCM_OK;
    if (ctx->capturing) {
        ctx->capture_failed = true;
        return fail(PCCM_E_STATE, "%s", while_capturing);
    }
    ctx->epoch++;
    if (h.host) (void)hipHostFree(h.host);
    h.host = nullptr; h.host_cap = 0;
    PCCM_HIP(hipHostMalloc((void **)&h.host, need, hipHostMallocCoherent));   // no XCD's L2 keeps any of it (wait_batch)
    h.host_cap = need;
    return PCCM_OK;
}

// Where a reduction column is read from (given the form and tie policy of the direction's search), and what has to happen before
// it can be bound.  slot_prepare binds from the first answer; prefetch_many acts on the second for every request before binding
// any: a repeated search rewrites the records, and a column bound to them earlier would read them through the wrong stride.
struct ColumnSource {
    enum From {
        kRecords,         // a field of the result records: off (0: squared distance, 1: projection), square, defer (UnitJob)
        kPlainD2,         // the plain d2 column (no records: the engine wrote the plain columns)
        kPointJob,        // a k_point_jobs job that reads the matched rows from the plain idx column, or from matched records (recs)
        kTieColumn,       // the tie pass's column (PCCM_TIES_MEAN)
        kStored,          // a stride-1 column kept with the context or a cloud (PCCM_METRIC_P2D*, PCCM_METRIC_RESOLUTION)
    } from = kPointJob;
    // the plain columns: none needed or they are there; the binder unpacks them; or they come before any column of the batch is
    // bound.  Which columns the binder unpacks (an unfused projection over stride-4 records) is today's split: it decides which
    // pccm_nn_path log lists the k_unpack -- the binder's joins the batch's log (PCCM_PATH_REDUCE), the first pass runs before it
    enum Prep { kReady, kBinderUnpacks, kPlainFirst } prep = kReady;
    int off = 0, square = 0, defer = 0;
    bool recs = false;
};

static ColumnSource column_source(const pccm_ctx *ctx, int dir, int metric, int normal_mode)
{
    const NNResult &res = ctx->nn[dir];
    const NNForm &f = res.form;
    const bool mean = res.ties == PCCM_TIES_MEAN;
    ColumnSource c;
    if (!res.valid) return c;                              // (slot_prepare reports what is missing)
    if (metric == PCCM_METRIC_D1) {
        c.from = f.has_records() ? ColumnSource::kRecords : ColumnSource::kPlainD2;
        if (f.layout() == 1) c.defer = 3;                  // matched records: the reduction forms the distance (NNOut::layout)
        return c;
    }
    if (dir == PCCM_DIR_SELF) return c;
    if (is_stored_metric(metric)) {
        c.from = ColumnSource::kStored;
        return c;
    }
    if (matched_column(metric)) {                          // the matched rows in place, or from the plain idx column
        if (mean) c.from = ColumnSource::kTieColumn;
        else if (f.matched_in_place()) c.recs = true;
        else if (!f.plain_ready(true)) c.prep = ColumnSource::kPlainFirst;
        return c;
    }
    if (!mean && f.holds_projection(normal_mode)) {       // (under PCCM_TIES_MEAN the records hold the pick's projection)
        c.from = ColumnSource::kRecords;
        c.off = 1;
        c.square = metric == PCCM_METRIC_D2 ? 1 : 0;       // metric.py:179: the square of the stored projection
        // ... which the reduction forms itself from a matched record (NNOut::layout): with the normal of the query's row
        // (streamed) or of the matched row the record carries (gathered: what a separate point pass would gather too)
        if (f.layout() == 1)
            c.defer = (ctx->cloud[dir == PCCM_DIR_LEFT ? 1 : 0].nrm_exact32 ? 1 : 2) + (normal_mode == PCCM_NORMAL_NEIGHBOUR ? 3 : 0);
        return c;
    }
    if (!f.plain_ready(true))                              // (the virtual neighbours of PCCM_TIES_MEAN need them too)
        c.prep = mean || f.rows_need_repeat() ? ColumnSource::kPlainFirst : ColumnSource::kBinderUnpacks;
    return c;
}

// bookkeeping + buffers of one slot; the kernels are launched for all new slots together (slots_launch)
static int slot_prepare(pccm_ctx *ctx, ReduceSlot &s, int dir, int metric, int normal_mode, bool want_units, PointJobs &pj,
                        UnitJobs &uj)
{
    const Cloud *it, *se;
    NNResult *res;
    int rc = need_nn(ctx, dir, &it, &se, &res, /*binds=*/true);
    if (rc) return rc;
    const int64_t ns = res->end - res->begin;
    if ((rc = column_check(ctx, dir, metric, normal_mode, *it, *se, *res))) return rc;
    const ColumnSource src = column_source(ctx, dir, metric, normal_mode);
    // (filed tails: a column that is not reduced straight from the records reads them in a kernel of its own first)
    if (res->form.tails_filed && src.from != ColumnSource::kRecords && (rc = filed_tails_resolve(ctx))) return rc;
    const double *dev = (const double *)res->rec.p;
    int stride = 1;
    switch (src.from) {
    case ColumnSource::kRecords: stride = res->form.stride(); break;
    case ColumnSource::kPlainD2: dev = res->d2; break;
    case ColumnSource::kTieColumn:
        if ((rc = ensure_ties(ctx, dir, false, false, true))) return rc;
        dev = (const double *)ctx->tie[dir].ang.p;
        break;
    case ColumnSource::kStored: dev = stored_column(ctx, dir, metric) + res->begin; break;
    case ColumnSource::kPointJob:
        // (PCCM_METRIC_SSIM_* / REFLECTANCE: the angular column's job on the two clouds' feature / reflectance columns instead of their normals)
        if (src.prep != ColumnSource::kReady && (rc = ensure_plain(ctx, *res, true))) return rc;
        if ((rc = ensure(ctx, s.val, (size_t)(ns > 0 ? ns : 1) * sizeof(double)))) return rc;
        dev = (const double *)s.val.p;
        if (ns > 0) {
            if (pj.njobs >= 4)
                return fail(PCCM_E_ARG, matched_column(metric) ? "at most four unfused point-to-plane, angular, PointSSIM or reflectance columns per call"
                                                               : "at most four unfused point-to-plane columns per call");
            if ((rc = point_job_fill(ctx, dir, metric, normal_mode, (double *)s.val.p, src.recs, *it, *se, *res, pj.j[pj.njobs]))) return rc;
            pj.off[pj.njobs + 1] = pj.off[pj.njobs] + ns;
            pj.njobs++;
        }
        break;
    }
    s.dir = dir; s.metric = metric; s.mode = normal_mode;
    s.gen = ctx->nn_gen[dir];
    static_cast<SlotShape &>(s) = slot_shape(it->n, res->begin, res->end);
    s.has_units = want_units;
    s.has_job = false;
    if ((rc = host_reserve(ctx, s, s.host_doubles(), "a reduction slot must be allocated during graph capture: run the sequence once first")))
        return rc;
    if (s.nunits > 0) {
        UnitCol col;
        col.off = src.off;
        col.square = src.square;
        bind_outputs(col, SlotView(s, s.host), want_units);
        // the column as a job of its own (what a selection of this column ranks: pccm_select_prefetch_many)
        UnitJob &U = s.job;
        U.val = dev; U.stride = stride; U.ncols = 1;
        U.defer = src.defer; U.nrm64 = se->nrm64; U.nrm32 = se->nrm32; U.nrm_rows = se->n_nrm; U.q32 = it->xyz32r; U.row0 = res->begin;
        U.c[0] = col; U.c[1] = col;
        bind_shape(U, s);
        s.has_job = true;
        // a second column over the same result records rides along with the job that already reads them
        UnitJob *host_job = nullptr;
        static const bool merge = [] {
            const char *e = PCCM_DIAG_ENV("PCCM_REDUCE_MERGE");
            return !(e && e[0] == '0');
        }();
        if (stride >= 2 && merge)
            for (int k = 0; k < uj.njobs; ++k)
                if (uj.j[k].stride >= 2 && uj.j[k].val == dev && uj.j[k].ncols == 1 &&
                    (uj.j[k].defer == src.defer || uj.j[k].defer == 3 || src.defer == 3))      // (one normal per job: row- and neighbour-indexed D2 do not share one)
                    host_job = &uj.j[k];
        if (host_job) {
            host_job->c[1] = col;
            host_job->ncols = 2;
            if (src.defer && src.defer != 3 && (host_job->defer == 0 || host_job->defer == 3)) host_job->defer = src.defer;   // (3: distances only so far)
        } else {
            if (uj.njobs >= 8) return fail(PCCM_E_ARG, "too many columns in one reduction batch");
            uj.j[uj.njobs] = s.job;
            const int64_t lanes = (s.nunits * 8 + 255) / 256 * 256;
            uj.uoff[uj.njobs + 1] = uj.uoff[uj.njobs] + lanes;
            uj.toff[uj.njobs + 1] = uj.toff[uj.njobs] + s.tail_n;
            uj.njobs++;
        }
    }
    return PCCM_OK;
}

static int prefetch_many(pccm_ctx *ctx, int n, const int *dirs, const int *metrics, const int *normal_modes, bool want_units);

int pccm_reduce_prefetch_many(pccm_ctx *ctx, int n, const int *dirs, const int *metrics, const int *normal_modes)
{
    CHECK_CTX(ctx);
    // per-leaf results cross PCIe only when a sharded exchange will need them: shards that start and end on whole chunks
    // exchange chunk sums (pccm_reduce_chunks_many), which the block results already hold
    bool units = false;
    if (ctx->sharded() && dirs)
        for (int k = 0; k < n && !units; ++k) {
            if (dirs[k] < 0 || dirs[k] > 2) continue;                 // reported by prefetch_many
            const NNResult &res = ctx->nn[dirs[k]];
            const Cloud &it = ctx->cloud[dirs[k] == PCCM_DIR_RIGHT ? 1 : 0];
            units = !slot_shape(it.n, res.begin, res.end).chunk_aligned();
        }
    return prefetch_many(ctx, n, dirs, metrics, normal_modes, units);
}

static int prefetch_many(pccm_ctx *ctx, int n, const int *dirs, const int *metrics, const int *normal_modes, bool want_units)
{
    if (n < 0 || n > 8 || (n > 0 && (!dirs || !metrics || !normal_modes))) return fail(PCCM_E_ARG, "1..8 requests expected");
    PointJobs pj;
    UnitJobs uj;
    pj.njobs = 0; pj.off[0] = 0;
    uj.njobs = 0; uj.uoff[0] = 0; uj.toff[0] = 0;
    for (int k = 0; k < n; ++k)
        if (dirs[k] < 0 || dirs[k] > 2) return fail(PCCM_E_ARG, "bad direction %d", dirs[k]);
    SlotBatch batch(ctx, ctx->slots);
    // first, whatever may change the layout of a direction's result records: a column that needs the plain columns before
    // the batch is bound (column_source) gets them now -- when the search left the matched rows out it is repeated
    // (ensure_plain), with the rows, and with the projection fused when the normals have arrived meanwhile.  Only then are the
    // columns of this batch bound to the records.  Under PCCM_TIES_MEAN the tie pass makes the angular column, together with
    // the averaged normals a neighbour-indexed projection of the same batch wants: one walk per direction.
    bool tie_ang[2] = {false, false}, tie_nrm[2] = {false, false};
    for (int k = 0; k < n; ++k) {
        if (dirs[k] == PCCM_DIR_SELF) continue;
        NNResult &res = ctx->nn[dirs[k]];
        if (!res.valid || res.ties != PCCM_TIES_MEAN) continue;
        if (metrics[k] == PCCM_METRIC_ANGULAR) tie_ang[dirs[k]] = true;
        else if (normal_mode_enters(metrics[k]) && normal_modes[k] == PCCM_NORMAL_NEIGHBOUR) tie_nrm[dirs[k]] = true;
    }
    for (int d = 0; d < 2; ++d) {
        if (!tie_ang[d] || find_pending(ctx->slots, ctx->nn_gen, d, PCCM_METRIC_ANGULAR, 0, want_units)) continue;
        const Cloud *it, *se;
        NNResult *res;
        int rc = need_nn(ctx, d, &it, &se, &res);
        if (!rc) rc = check_angular(ctx, d, *it, *se);
        if (rc) return rc;
        if (tie_nrm[d] && check_normals(ctx, *it, *se, *res, PCCM_NORMAL_NEIGHBOUR) != PCCM_OK) tie_nrm[d] = false;   // (reported below)
        if ((rc = ensure_ties(ctx, d, tie_nrm[d], false, true))) return rc;
    }
    for (int k = 0; k < n; ++k) {
        if (column_source(ctx, dirs[k], metrics[k], normal_modes[k]).prep != ColumnSource::kPlainFirst ||
            find_pending(ctx->slots, ctx->nn_gen, dirs[k], metrics[k], normal_modes[k], want_units))
            continue;
        int rc = ensure_plain(ctx, ctx->nn[dirs[k]], true);
        if (rc) return rc;
    }
    const int path_kept = ctx->path_n[3];
    PathScope path(ctx, 1u << 3);          // the batch's kernels: per-point columns (slot_prepare), point and unit jobs
    for (int k = 0; k < n; ++k) {
        if (find_pending(ctx->slots, ctx->nn_gen, dirs[k], metrics[k], normal_modes[k], want_units)) continue;
        ReduceSlot *s;
        int rc = batch.acquire("no free reduction slot: more than 24 live columns in one batch", &s);
        if (!rc) rc = slot_prepare(ctx, *s, dirs[k], metrics[k], normal_modes[k], want_units, pj, uj);
        if (rc) return rc;
        s->pending = true;
    }
    if (batch.nfresh == 0) {
        ctx->path_n[3] = path_kept;        // no batch: the log still describes the last one
        return PCCM_OK;
    }
    int rc;
    if (pj.njobs > 0 && (rc = filed_tails_resolve(ctx))) return rc;      // (point jobs read matched records in place)
    if ((rc = launch_point_jobs(ctx, pj))) return rc;
    uint64_t seq = 0;
    if ((rc = launch_unit_jobs(ctx, uj, &seq))) return rc;
    return batch.finish(seq);
}

int pccm_reduce_prefetch(pccm_ctx *ctx, int dir, int metric, int normal_mode)
{
    return pccm_reduce_prefetch_many(ctx, 1, &dir, &metric, &normal_mode);
}

// the slot of one column, enqueued when nobody has, once its numbers are on the host (units: with the per-leaf results)
static int take_slot(pccm_ctx *ctx, int dir, int metric, int normal_mode, bool units, ReduceSlot **out)
{
    if (dir < 0 || dir > 2) return fail(PCCM_E_ARG, "bad direction %d", dir);
    auto find = [&](int) { return find_pending(ctx->slots, ctx->nn_gen, dir, metric, normal_mode, units); };
    if (!find(0)) {
        int rc = prefetch_many(ctx, 1, &dir, &metric, &normal_mode, units);
        if (rc) return rc;
    }
    return consume(ctx, 1, "reduction slot lost", find, [&](int, ReduceSlot &s) { *out = &s; });
}

int pccm_reduce(pccm_ctx *ctx, int dir, int metric, int normal_mode, double *xvec, double *minmax)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    if (!xvec || !minmax) return fail(PCCM_E_ARG, "null pointer");
    ReduceSlot *s;
    { int rc = take_slot(ctx, dir, metric, normal_mode, true, &s); if (rc) return rc; }
    slot_fill_xvec(*s, SlotView(*s, s->host), xvec, minmax);
    return PCCM_OK;
}

int pccm_finish_sum(const double *xvec, int64_t n_iter, double *sum)
{
    if (!xvec || !sum || n_iter < 0) return fail(PCCM_E_ARG, "bad argument");
    const SlotShape w = slot_shape(n_iter, 0, n_iter);       // the whole column
    *sum = np_chunked_sum(w.nfull(), [=](int64_t c) { return leaf_tree(xvec + c * kLeavesPerChunk, kLeavesPerChunk); },
                          xvec + w.nfull() * kLeavesPerChunk, w.tail_n);
    return PCCM_OK;
}

// one column's total from its slot (unsharded, begin = 0)
static int total_from_slot(pccm_ctx *ctx, int dir, int metric, int normal_mode, double out[3])
{
    ReduceSlot *s;
    { int rc = take_slot(ctx, dir, metric, normal_mode, false, &s); if (rc) return rc; }
    slot_total(*s, SlotView(*s, s->host), out);
    return PCCM_OK;
}

int64_t pccm_cvec_len(int64_t n_iter) { return slot_shape(n_iter, 0, n_iter).cvec_len(); }

// one column's chunk vector from its slot
static int chunks_from_slot(pccm_ctx *ctx, int dir, int metric, int normal_mode, double *cvec, double minmax[2])
{
    ReduceSlot *s;
    { int rc = take_slot(ctx, dir, metric, normal_mode, false, &s); if (rc) return rc; }
    if (!s->chunk_aligned())
        return fail(PCCM_E_STATE, "rows [%lld, %lld) do not start and end on 8192-row chunks: use pccm_reduce", (long long)s->begin,
                    (long long)s->end);
    slot_fill_cvec(*s, SlotView(*s, s->host), cvec, minmax);
    return PCCM_OK;
}

int pccm_reduce_chunks_many(pccm_ctx *ctx, int n, const int *dirs, const int *metrics, const int *normal_modes, double *cvecs, double *minmax)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    if (n < 0 || n > 8 || (n > 0 && (!dirs || !metrics || !normal_modes || !cvecs || !minmax))) return fail(PCCM_E_ARG, "1..8 requests expected");
    int rc = prefetch_many(ctx, n, dirs, metrics, normal_modes, false);       // whatever is not enqueued yet, in one batch
    if (rc) return rc;
    for (int k = 0; k < n; ++k) {
        const Cloud *it, *se;
        if ((rc = dir_clouds(ctx, dirs[k], &it, &se))) return rc;
        if ((rc = chunks_from_slot(ctx, dirs[k], metrics[k], normal_modes[k], cvecs, minmax + 2 * k))) return rc;
        cvecs += pccm_cvec_len(it->n);
    }
    return PCCM_OK;
}

int pccm_finish_chunks(const double *cvec, int64_t n_iter, double *sum)
{
    if (!cvec || !sum || n_iter < 0) return fail(PCCM_E_ARG, "bad argument");
    const SlotShape w = slot_shape(n_iter, 0, n_iter);       // the whole column
    *sum = np_chunked_sum(w.nfull(), [=](int64_t c) { return cvec[c]; }, cvec + w.nfull(), w.tail_n);
    return PCCM_OK;
}

int pccm_reduce_total(pccm_ctx *ctx, int dir, int metric, int normal_mode, double out[3])
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    if (!out) return fail(PCCM_E_ARG, "null pointer");
    if (ctx->sharded()) return fail(PCCM_E_STATE, "pccm_reduce_total needs the whole column on this GPU (world = 1)");
    return total_from_slot(ctx, dir, metric, normal_mode, out);
}

int pccm_reduce_total_many(pccm_ctx *ctx, int n, const int *dirs, const int *metrics, const int *normal_modes, double *out)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    if (n < 0 || n > 8 || (n > 0 && (!dirs || !metrics || !normal_modes || !out))) return fail(PCCM_E_ARG, "1..8 requests expected");
    if (ctx->sharded()) return fail(PCCM_E_STATE, "pccm_reduce_total_many needs the whole columns on this GPU (world = 1)");
    int rc = prefetch_many(ctx, n, dirs, metrics, normal_modes, false);       // whatever is not enqueued yet, in one batch
    if (rc) return rc;
    for (int k = 0; k < n; ++k)
        if ((rc = total_from_slot(ctx, dirs[k], metrics[k], normal_modes[k], out + 3 * k))) return rc;
    return PCCM_OK;
}

// The plain reductions of the columns that a call's new selections, counts or mapped reductions read, enqueued in one batch where
// none is pending, and their slots: a column is read as its reduction's job describes it (need_job: a column without rows won't do).
static int column_slots(pccm_ctx *ctx, const RequestGroups &g, bool need_job, const ReduceSlot **cslot)
{
    int rc = prefetch_many(ctx, g.ncols, g.dir, g.metric, g.mode, false);
    if (rc) return rc;
    for (int c = 0; c < g.ncols; ++c) {
        cslot[c] = find_pending(ctx->slots, ctx->nn_gen, g.dir[c], g.metric[c], g.mode[c]);
        if (!cslot[c] || (need_job && !cslot[c]->has_job)) return fail(PCCM_E_STATE, "reduction slot lost");
    }
    return PCCM_OK;
}

// ---- selections and counts: the k-th smallest element of a column, the rows of a column <= x (include/pccm.h) ---------------
// One slot table, one enqueue path: a request is (kind, column, key) -- the key a selection's rank or the bit pattern of a count's
// threshold -- and the two differ in the check of the key, the launches and the type of the host word.
static int select_check(pccm_ctx *ctx, int kind, const char *who, int n, const int *dirs, const int *metrics, const int *normal_modes,
                        const int64_t *ks)
{
    static_assert(kSelMax == 8, "the slot batches hold eight requests");
    const char *what = kind == kSlotCount ? "counts" : "selections";
    return request_check(ctx, who, what, n, dirs && metrics && normal_modes && ks, dirs, metrics, [](int) { return PCCM_OK; },
                         [&](int i, const Cloud &it) {
        if (it.n >= ((int64_t)1 << 32)) return fail(PCCM_E_ARG, "%s count rows in 32 bits: columns of 2^32 rows or more are not supported", what);
        if (kind == kSlotCount) {
            double x;
            memcpy(&x, &ks[i], sizeof x);
            if (x != x) return fail(PCCM_E_ARG, "a count's threshold is a number or an infinity, not NaN");
        } else if (ks[i] < 1 || ks[i] > it.n) {
            return fail(PCCM_E_ARG, "rank %lld outside 1..%lld", (long long)ks[i], (long long)it.n);
        }
        return PCCM_OK;
    });
}

// check, then enqueue what is not enqueued yet, by column
static int select_prefetch(pccm_ctx *ctx, int kind, const char *who, int n, const int *dirs, const int *metrics, const int *normal_modes,
                           const int64_t *ks)
{
    int rc = select_check(ctx, kind, who, n, dirs, metrics, normal_modes, ks);
    if (rc) return rc;
    const RequestGroups g = group_requests(n, dirs, metrics, normal_modes, ks, nullptr, [&](int i) {
        return find_pending(ctx->sel_slots, ctx->nn_gen, dirs[i], metrics[i], normal_modes[i], ks[i], kind) != nullptr;
    });
    if (g.ntodo == 0) return PCCM_OK;
    const ReduceSlot *cslot[kSelMax];
    rc = ensure(ctx, ctx->sel_hist, (size_t)kSelPasses * kSelMax * kSelBins * sizeof(uint32_t));
    if (!rc) rc = ensure(ctx, ctx->sel_state, (size_t)kSelPasses * kSelMax * sizeof(SelState));
    if (!rc) rc = column_slots(ctx, g, true, cslot);
    if (rc) return rc;
    SlotBatch batch(ctx, ctx->sel_slots);
    bool placed[kSelMax] = {};
    PathScope path(ctx, 1u << 3, true);            // the selection's launches join the log of the column's reduction batch
    for (int left = g.ntodo; left > 0;) {          // rounds of at most kSelPerCol requests per column (two at the most)
        UnitJobs uj;
        uj.njobs = 0;
        for (int k = 0; k < 9; ++k) uj.uoff[k] = uj.toff[k] = 0;
        UnitSelect &S = uj.sel;
        S.hist = (uint32_t *)ctx->sel_hist.p;
        S.state = (SelState *)ctx->sel_state.p;
        for (int c = 0; c < g.ncols; ++c) {
            int taken = 0;
            for (int j = 0; j < g.ntodo && taken < kSelPerCol; ++j) {
                if (placed[j] || g.col_of[j] != c) continue;
                SelectSlot *q;
                if ((rc = batch.acquire("no free selection slot", &q))) return rc;
                const int i = g.todo[j];
                q->kind = kind;
                q->dir = dirs[i]; q->metric = metrics[i]; q->mode = normal_modes[i]; q->k = ks[i];
                q->gen = ctx->nn_gen[dirs[i]];
                q->pending = true;
                if (taken == 0) {
                    uj.j[uj.njobs] = cslot[c]->job;
                    S.sfirst[uj.njobs] = S.nsel;
                    uj.njobs++;
                }
                S.k[S.nsel] = (unsigned long long)ks[i];
                S.out[S.nsel] = ctx->sel_host + (q - ctx->sel_slots);
                S.nsel++;
                placed[j] = true;
                taken++;
                left--;
            }
        }
        for (int k = uj.njobs; k < 9; ++k) S.sfirst[k] = S.nsel;
        for (int k = uj.njobs; k < 8; ++k) uj.j[k] = uj.j[0];
        if ((rc = kind == kSlotCount ? launch_unit_count(ctx, uj) : launch_unit_select(ctx, uj))) return rc;
    }
    uint64_t seq = 0;
    if ((rc = launch_publish(ctx, &seq))) return rc;
    return batch.finish(seq);
}

// consume: enqueue first what nobody prefetched, in one batch; wait once; word[i]: the host word of request i
static int select_consume(pccm_ctx *ctx, int kind, const char *who, int n, const int *dirs, const int *metrics, const int *normal_modes,
                          const int64_t *ks, double *word)
{
    int rc = select_prefetch(ctx, kind, who, n, dirs, metrics, normal_modes, ks);
    if (rc) return rc;
    auto find = [&](int i) { return find_pending(ctx->sel_slots, ctx->nn_gen, dirs[i], metrics[i], normal_modes[i], ks[i], kind); };
    return consume(ctx, n, "selection slot lost", find, [&](int i, SelectSlot &q) { word[i] = ctx->sel_host[&q - ctx->sel_slots]; });
}

int pccm_select_prefetch_many(pccm_ctx *ctx, int n, const int *dirs, const int *metrics, const int *normal_modes, const int64_t *ks)
{
    CHECK_CTX(ctx);
    return select_prefetch(ctx, kSlotSelect, "pccm_select_prefetch_many", n, dirs, metrics, normal_modes, ks);
}

int pccm_select_many(pccm_ctx *ctx, int n, const int *dirs, const int *metrics, const int *normal_modes, const int64_t *ks, double *out)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    if (n > 0 && !out) return fail(PCCM_E_ARG, "null pointer");
    return select_consume(ctx, kSlotSelect, "pccm_select_many", n, dirs, metrics, normal_modes, ks, out);
}

// the thresholds as slot keys: their bit patterns (0.0 and -0.0 are two keys with one answer)
static int count_keys(int n, const double *xs, int64_t *keys)
{
    if (n < 0 || n > kSelMax || (n > 0 && !xs)) return fail(PCCM_E_ARG, "1..8 requests expected");
    memcpy(keys, xs, (size_t)n * sizeof(double));
    return PCCM_OK;
}

int pccm_count_prefetch_many(pccm_ctx *ctx, int n, const int *dirs, const int *metrics, const int *normal_modes, const double *xs)
{
    CHECK_CTX(ctx);
    int64_t keys[kSelMax];
    int rc = count_keys(n, xs, keys);
    if (rc) return rc;
    return select_prefetch(ctx, kSlotCount, "pccm_count_prefetch_many", n, dirs, metrics, normal_modes, keys);
}

int pccm_count_many(pccm_ctx *ctx, int n, const int *dirs, const int *metrics, const int *normal_modes, const double *xs, int64_t *out)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    if (n > 0 && !out) return fail(PCCM_E_ARG, "null pointer");
    int64_t keys[kSelMax];
    double words[kSelMax];
    int rc = count_keys(n, xs, keys);
    if (!rc) rc = select_consume(ctx, kSlotCount, "pccm_count_many", n, dirs, metrics, normal_modes, keys, words);
    if (rc) return rc;
    memcpy(out, words, (size_t)n * sizeof(double));       // (the store launch wrote 64-bit counts into the slots' words)
    return PCCM_OK;
}

// ---- mapped reductions: np.sum / min / max of f(column) without the column (include/pccm.h) ---------------------------------
// A request is (column, map, cap).  Like a selection it reads the column as the column's plain reduction describes it
// (ReduceWhat::job), enqueued first where nobody has; unlike one it is a reduction launch: the job's column carries the map,
// reduce_shape() gives such a job no lean kernel, and k_unit_jobs writes block results and the raw tail into the slot's own host
// region.  Two requests on one column share a job -- its two columns, one read of the records.
static int map_check(pccm_ctx *ctx, const char *who, int n, const int *dirs, const int *metrics, const int *normal_modes, const int *maps,
                     const double *xs)
{
    return request_check(ctx, who, "mapped reductions", n, dirs && metrics && normal_modes && maps && xs, dirs, metrics, [&](int i) {
        if (maps[i] < 1 || maps[i] > (PCCM_MAP_CLAMP | PCCM_MAP_ROOT))
            return fail(PCCM_E_ARG, "map %d is no combination of PCCM_MAP_CLAMP and PCCM_MAP_ROOT (0: pccm_reduce_total_many)", maps[i]);
        if ((maps[i] & PCCM_MAP_CLAMP) && xs[i] != xs[i]) return fail(PCCM_E_ARG, "a clamp's cap is a number or an infinity, not NaN");
        return PCCM_OK;
    }, [](int, const Cloud &) { return PCCM_OK; });
}

// Where the matched rows of a direction's result are read (matched_row, pccm_internal.h): in place from records that carry them
// (idx null), else from the plain idx column.  A search that left the rows out -- NNForm::kPair, pccm_nn_want_idx off;
// kMatchedNoRows, the voxel-brick search -- is repeated with the rows on (ensure_plain, records_rewritten included; PCCM_E_STATE
// during graph capture), as for the colour calls and pccm_carry_normals; records that have the rows are never unpacked for this.
struct RowSource {
    const int32_t *idx = nullptr;
    const double *rec = nullptr;
    int stride = 0;
};
static int row_source(pccm_ctx *ctx, NNResult &res, RowSource *out)
{
    int rc = res.form.rows_need_repeat() ? ensure_plain(ctx, res, true) : PCCM_OK;
    if (rc) return rc;
    if (res.form.has_rows()) *out = {nullptr, (const double *)res.rec.p, res.form.stride()};
    else if (res.form.plain_ready(true)) *out = {res.idx, nullptr, 0};
    else return fail(PCCM_E_STATE, "no matched rows to read");
    return PCCM_OK;
}

// The match counts of direction dir (pccm_ctx::match): made once per search -- valid while their generation is the direction's --
// by a memset and a launch of the carry's count pass on the stream.  A capture records both, and an op that gives the counts the
// generation the replayed search leaves (graph_replay), once per captured search.
static int match_counts_ensure(pccm_ctx *ctx, int dir, const Cloud &se, const NNResult &res, const RowSource &src)
{
    pccm_ctx::MatchCounts &mc = ctx->match[dir];
    bool there = mc.gen == ctx->nn_gen[dir];
    if (there && ctx->capturing) {                     // ... by this capture, behind its last search of the direction?
        there = false;
        for (size_t k = ctx->cap_ops.size(); k-- > 0 && !there;) {
            const GraphOp &op = ctx->cap_ops[k];
            if (op.dir != dir) continue;
            if (op.kind == 1) break;
            there = op.kind == 5;
        }
    }
    if (there) return PCCM_OK;
    const void *was = mc.buf.p;
    int rc = ensure(ctx, mc.buf, (size_t)(se.n > 0 ? se.n : 1) * sizeof(uint32_t));
    if (rc) return rc;
    if (was && was != mc.buf.p) column_moved(ctx);
    mc.gen = 0;
    if ((rc = launch_match_counts(ctx, src.idx, src.rec, src.stride, res.end - res.begin, se.n, (uint32_t *)mc.buf.p))) return rc;
    mc.gen = ctx->nn_gen[dir];
    if (ctx->capturing) {
        GraphOp op;
        op.kind = 5;
        op.dir = dir;
        ctx->cap_ops.push_back(op);
    }
    return PCCM_OK;
}

static int map_enqueue(pccm_ctx *ctx, int n, const int *dirs, const int *metrics, const int *normal_modes, const int *maps, const double *xs,
                       const RowSource *rows);

static int map_prefetch(pccm_ctx *ctx, const char *who, int n, const int *dirs, const int *metrics, const int *normal_modes, const int *maps,
                        const double *xs)
{
    int rc = map_check(ctx, who, n, dirs, metrics, normal_modes, maps, xs);
    if (rc) return rc;
    return map_enqueue(ctx, n, dirs, metrics, normal_modes, maps, xs, nullptr);
}

// enqueue what is not enqueued yet of n checked requests; rows[d]: where a density or moment map of direction d reads the matched rows
static int map_enqueue(pccm_ctx *ctx, int n, const int *dirs, const int *metrics, const int *normal_modes, const int *maps, const double *xs,
                       const RowSource *rows)
{
    int rc;
    int64_t which[8];
    uint64_t bits[8];
    for (int i = 0; i < n; ++i) {
        which[i] = maps[i];
        bits[i] = map_cap_bits(maps[i], xs[i]);
    }
    const RequestGroups g = group_requests(n, dirs, metrics, normal_modes, which, bits, [&](int i) {
        return find_pending(ctx->map_slots, ctx->nn_gen, dirs[i], metrics[i], normal_modes[i], maps[i], bits[i]) != nullptr;
    });
    if (g.ntodo == 0) return PCCM_OK;
    const ReduceSlot *cslot[8];
    if ((rc = column_slots(ctx, g, false, cslot))) return rc;
    SlotBatch batch(ctx, ctx->map_slots);
    int open_job[8];                               // open_job[c]: the job of column c that still has one column free, or -1
    for (int c = 0; c < 8; ++c) open_job[c] = -1;
    UnitJobs uj;
    uj.njobs = 0; uj.uoff[0] = 0; uj.toff[0] = 0;
    PathScope path(ctx, 1u << 3, true);            // the launch joins the log of the columns' reduction batch
    for (int j = 0; j < g.ntodo; ++j) {
        const int i = g.todo[j], c = g.col_of[j];
        MapSlot *m;
        if ((rc = batch.acquire("no free mapped-reduction slot", &m))) return rc;
        SlotShape hs = *cslot[c];                  // the column's shape; no per-leaf results cross to the host
        hs.nunits = 0;
        if ((rc = host_reserve(ctx, *m, hs.host_doubles(), "a mapped-reduction slot must be allocated during graph capture: run the sequence once first")))
            return rc;
        m->dir = dirs[i]; m->metric = metrics[i]; m->mode = normal_modes[i];
        m->gen = ctx->nn_gen[dirs[i]];
        m->shape = hs;
        m->map = maps[i];
        m->cap_bits = bits[i];
        m->pending = true;
        if (!cslot[c]->has_job) continue;          // a column without rows: nothing to launch, the total of nothing
        UnitCol col = cslot[c]->job.c[0];
        col.map = maps[i];
        col.cap = (maps[i] & (PCCM_MAP_CLAMP | PCCM_MAP_MOMENT)) ? xs[i] : 0.0;
        col.alpha = (maps[i] & PCCM_MAP_DENSITY) ? xs[i] : 0.0;
        bind_outputs(col, SlotView(hs, m->host), false);
        if (open_job[c] >= 0) {                    // the second map over the fields the job already reads
            uj.j[open_job[c]].c[1] = col;
            uj.j[open_job[c]].ncols = 2;
            open_job[c] = -1;
        } else {
            UnitJob &U = uj.j[uj.njobs];
            U = cslot[c]->job;
            U.ncols = 1;
            U.c[0] = col; U.c[1] = col;
            if (maps[i] & PCCM_MAP_DENSITY) {      // (a call's maps are all density maps or none is: a job's two columns agree)
                const int d = dirs[i];
                U.rows = rows[d].idx;
                U.cnt = (const uint32_t *)ctx->match[d].buf.p;
                U.cnt_rows = ctx->cloud[d == PCCM_DIR_LEFT ? 1 : 0].n;
            }
            if (maps[i] & PCCM_MAP_MOMENT) {       // (likewise: a call's maps are all moment maps or none is)
                const int d = dirs[i];
                const Cloud &it = ctx->cloud[d == PCCM_DIR_LEFT ? 0 : 1], &se = ctx->cloud[d == PCCM_DIR_LEFT ? 1 : 0];
                U.rows = rows[d].idx;
                U.cnt_rows = se.n;
                U.mom_it = it.xyz64;
                U.mom_se = se.xyz64;
                for (int a = 0; a < 3; ++a) memcpy(&U.pivot[a], &ctx->moment_pivot[a], sizeof(double));
            }
            const int64_t lanes = (U.nunits * 8 + 255) / 256 * 256;
            uj.uoff[uj.njobs + 1] = uj.uoff[uj.njobs] + lanes;
            uj.toff[uj.njobs + 1] = uj.toff[uj.njobs] + U.tail_n;
            open_job[c] = uj.njobs++;
        }
    }
    uint64_t seq = 0;
    if ((rc = launch_unit_jobs(ctx, uj, &seq))) return rc;
    if (!seq && (rc = launch_publish(ctx, &seq))) return rc;      // (columns without rows: the batch still publishes)
    return batch.finish(seq);
}

int pccm_reduce_map_prefetch_many(pccm_ctx *ctx, int n, const int *dirs, const int *metrics, const int *normal_modes, const int *maps,
                                  const double *xs)
{
    CHECK_CTX(ctx);
    return map_prefetch(ctx, "pccm_reduce_map_prefetch_many", n, dirs, metrics, normal_modes, maps, xs);
}

int pccm_reduce_map_total_many(pccm_ctx *ctx, int n, const int *dirs, const int *metrics, const int *normal_modes, const int *maps,
                               const double *xs, double *out)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    if (n > 0 && !out) return fail(PCCM_E_ARG, "null pointer");
    int rc = map_prefetch(ctx, "pccm_reduce_map_total_many", n, dirs, metrics, normal_modes, maps, xs);
    if (rc) return rc;
    auto find = [&](int i) {
        return find_pending(ctx->map_slots, ctx->nn_gen, dirs[i], metrics[i], normal_modes[i], maps[i], map_cap_bits(maps[i], xs[i]));
    };
    return consume(ctx, n, "mapped-reduction slot lost", find, [&](int i, MapSlot &m) { slot_total(m.shape, SlotView(m.shape, m.host), out + 3 * i); });
}

// ---- match counts and the density-aware Chamfer terms (include/pccm.h) -------------------------------------------------------
// A density request is a mapped reduction of the direction's D1 column whose map is PCCM_MAP_DENSITY, with PCCM_MAP_ROOT in front
// of it unless `squared`, and whose key is alpha: it lives in the mapped-reduction slots and shares their life cycle.  In front of
// the mapped launch go, per direction and where the search's are not there yet, the match counts.
static int density_maps(int n, const int *dirs, const int *squared, const double *alphas, int *metrics, int *modes, int *maps)
{
    if (n < 0 || n > 8 || (n > 0 && (!dirs || !squared || !alphas))) return fail(PCCM_E_ARG, "0..8 requests expected");
    for (int i = 0; i < n; ++i) {
        metrics[i] = PCCM_METRIC_D1;
        modes[i] = PCCM_NORMAL_ROW;
        maps[i] = PCCM_MAP_DENSITY | (squared[i] ? 0 : PCCM_MAP_ROOT);
    }
    return PCCM_OK;
}

static int density_ties_check(const pccm_ctx *ctx, int dir)
{
    if (ctx->nn[dir].ties == PCCM_TIES_MEAN)
        return fail(PCCM_E_STATE, "the search of direction %d ran under PCCM_TIES_MEAN: a virtual neighbour has no row to count", dir);
    return PCCM_OK;
}

static int density_prefetch(pccm_ctx *ctx, const char *who, int n, const int *dirs, const int *squared, const double *alphas, int *metrics,
                            int *modes, int *maps)
{
    int rc = density_maps(n, dirs, squared, alphas, metrics, modes, maps);
    if (!rc)
        rc = request_check(ctx, who, "density reductions", n, true, dirs, metrics, [&](int i) {
            if (squared[i] != 0 && squared[i] != 1) return fail(PCCM_E_ARG, "squared is 0 or 1, not %d", squared[i]);
            if (!(alphas[i] >= 0.0) || alphas[i] == INFINITY) return fail(PCCM_E_ARG, "alpha is a finite number >= 0");
            return PCCM_OK;
        }, [&](int i, const Cloud &) { return density_ties_check(ctx, dirs[i]); });
    if (rc || n == 0) return rc;
    // the rows first (a repeated search rewrites the records the columns are bound to), then the counts, then the columns
    RowSource rows[2];
    bool seen[2] = {false, false};
    for (int i = 0; i < n; ++i) {
        const int d = dirs[i];
        if (seen[d]) continue;
        seen[d] = true;
        const Cloud *it, *se;
        NNResult *res;
        if ((rc = need_nn(ctx, d, &it, &se, &res)) || (rc = row_source(ctx, *res, &rows[d]))) return rc;
    }
    for (int d = 0; d < 2; ++d) {
        if (!seen[d]) continue;
        const Cloud *it, *se;
        NNResult *res;
        if ((rc = need_nn(ctx, d, &it, &se, &res)) || (rc = match_counts_ensure(ctx, d, *se, *res, rows[d]))) return rc;
    }
    return map_enqueue(ctx, n, dirs, metrics, modes, maps, alphas, rows);
}

int pccm_reduce_density_prefetch_many(pccm_ctx *ctx, int n, const int *dirs, const int *squared, const double *alphas)
{
    CHECK_CTX(ctx);
    int metrics[8], modes[8], maps[8];
    return density_prefetch(ctx, "pccm_reduce_density_prefetch_many", n, dirs, squared, alphas, metrics, modes, maps);
}

int pccm_reduce_density_total_many(pccm_ctx *ctx, int n, const int *dirs, const int *squared, const double *alphas, double *out)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    if (!out) return fail(PCCM_E_ARG, "null pointer");
    int metrics[8], modes[8], maps[8];
    int rc = density_prefetch(ctx, "pccm_reduce_density_total_many", n, dirs, squared, alphas, metrics, modes, maps);
    if (rc || n == 0) return rc;
    auto find = [&](int i) {
        return find_pending(ctx->map_slots, ctx->nn_gen, dirs[i], metrics[i], modes[i], maps[i], map_cap_bits(maps[i], alphas[i]));
    };
    return consume(ctx, n, "mapped-reduction slot lost", find, [&](int i, MapSlot &m) { slot_total(m.shape, SlotView(m.shape, m.host), out + 3 * i); });
}

int pccm_match_counts(pccm_ctx *ctx, int dir, uint32_t *out)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    if (dir != PCCM_DIR_LEFT && dir != PCCM_DIR_RIGHT) return fail(PCCM_E_ARG, "match counts exist for directions 0 and 1, not %d", dir);
    if (!out) return fail(PCCM_E_ARG, "null pointer");
    if (ctx->sharded()) return fail(PCCM_E_STATE, "pccm_match_counts needs the whole column on this GPU (world = 1)");
    const Cloud *it, *se;
    NNResult *res;
    RowSource rows;
    int rc = need_nn(ctx, dir, &it, &se, &res);
    if (!rc) rc = density_ties_check(ctx, dir);
    if (!rc) rc = row_source(ctx, *res, &rows);
    if (!rc) rc = match_counts_ensure(ctx, dir, *se, *res, rows);
    if (rc) return rc;
    if (se->n > 0 && (rc = d2h(ctx, out, ctx->match[dir].buf.p, (size_t)se->n * sizeof(uint32_t)))) return rc;
    PCCM_HIP(hipStreamSynchronize(ctx->stream));
    return check_device_errors(ctx);
}

// ---- alignment moments (include/pccm.h) ---------------------------------------------------------------------------------------
// A moment request is a mapped reduction of the direction's D1 column whose map is PCCM_MAP_MOMENT | kind << 8 and whose key is the
// inlier bound: it lives in the mapped-reduction slots and shares their life cycle.  The pivot is the call's, not the request's:
// pending moments made with another pivot are given up before the call looks for its own.
static int moment_prefetch(pccm_ctx *ctx, const char *who, int n, const int *dirs, const int *kinds, const double *caps, const double *pivot,
                           int *metrics, int *modes, int *maps)
{
    if (n < 0 || n > 8 || (n > 0 && (!dirs || !kinds || !caps))) return fail(PCCM_E_ARG, "0..8 requests expected");
    if (!pivot || !std::isfinite(pivot[0]) || !std::isfinite(pivot[1]) || !std::isfinite(pivot[2]))
        return fail(PCCM_E_ARG, "the pivot is three finite numbers");
    for (int i = 0; i < n; ++i) {
        metrics[i] = PCCM_METRIC_D1;
        modes[i] = PCCM_NORMAL_ROW;
        maps[i] = PCCM_MAP_MOMENT | ((kinds[i] & 0xff) << 8);
    }
    int rc = request_check(ctx, who, "alignment moments", n, true, dirs, metrics, [&](int i) {
        if (kinds[i] < 0 || kinds[i] > 15) return fail(PCCM_E_ARG, "a moment's kind is 0..15, not %d", kinds[i]);
        if (caps[i] != caps[i]) return fail(PCCM_E_ARG, "a moment's inlier bound is a number or an infinity, not NaN");
        return PCCM_OK;
    }, [&](int i, const Cloud &) {
        if (ctx->nn[dirs[i]].ties == PCCM_TIES_MEAN)
            return fail(PCCM_E_STATE, "the search of direction %d ran under PCCM_TIES_MEAN: a virtual neighbour is no row of the cloud", dirs[i]);
        return PCCM_OK;
    });
    if (rc || n == 0) return rc;
    uint64_t pv[3];
    memcpy(pv, pivot, sizeof pv);
    if (pv[0] != ctx->moment_pivot[0] || pv[1] != ctx->moment_pivot[1] || pv[2] != ctx->moment_pivot[2]) {
        for (MapSlot &m : ctx->map_slots)
            if (m.map & PCCM_MAP_MOMENT) m.pending = false;
        memcpy(ctx->moment_pivot, pv, sizeof pv);
    }
    // the rows first (a repeated search rewrites the records the columns are bound to), then the columns
    RowSource rows[2];
    bool seen[2] = {false, false};
    for (int i = 0; i < n; ++i) {
        const int d = dirs[i];
        if (seen[d]) continue;
        seen[d] = true;
        const Cloud *it, *se;
        NNResult *res;
        if ((rc = need_nn(ctx, d, &it, &se, &res)) || (rc = row_source(ctx, *res, &rows[d]))) return rc;
    }
    return map_enqueue(ctx, n, dirs, metrics, modes, maps, caps, rows);
}

int pccm_reduce_moment_prefetch_many(pccm_ctx *ctx, int n, const int *dirs, const int *kinds, const double *caps, const double *pivot)
{
    CHECK_CTX(ctx);
    int metrics[8], modes[8], maps[8];
    return moment_prefetch(ctx, "pccm_reduce_moment_prefetch_many", n, dirs, kinds, caps, pivot, metrics, modes, maps);
}

int pccm_reduce_moment_total_many(pccm_ctx *ctx, int n, const int *dirs, const int *kinds, const double *caps, const double *pivot, double *out)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    if (!out) return fail(PCCM_E_ARG, "null pointer");
    int metrics[8], modes[8], maps[8];
    int rc = moment_prefetch(ctx, "pccm_reduce_moment_total_many", n, dirs, kinds, caps, pivot, metrics, modes, maps);
    if (rc || n == 0) return rc;
    auto find = [&](int i) {
        return find_pending(ctx->map_slots, ctx->nn_gen, dirs[i], metrics[i], modes[i], maps[i], map_cap_bits(maps[i], caps[i]));
    };
    return consume(ctx, n, "mapped-reduction slot lost", find, [&](int i, MapSlot &m) { slot_total(m.shape, SlotView(m.shape, m.host), out + 3 * i); });
}

// Host helper for the colour metrics (metric.py:261-290): out[r] = M * rgb[r] for the BT.709 "ycc" (1) or
// the "yuv" (2) matrix.  The reference maps every row with np.matmul(M, c); on the authoring host
// (NumPy 2.2.6 / OpenBLAS dgemv) that evaluates each component as fma(m2*c2, fma(m0*c0, m1*c1)) -- pinned
// by tests/golden/*color* -- and that is the order used here.
int pccm_color_transform(const double *rgb, int64_t n, int scheme, double *out)
{
    static const double kYcc[9] = {0.2126, 0.7152, 0.0722, -0.1146, -0.3854, 0.5, 0.5, -0.4542, -0.0458};
    static const double kYuv[9] = {0.25, 0.5, 0.25, 1, 0, -1, -0.5, 1, -0.5};
    if (!rgb || !out || n < 0) return fail(PCCM_E_ARG, "bad argument");
    const double *m = scheme == 1 ? kYcc : (scheme == 2 ? kYuv : nullptr);
    if (!m) return fail(PCCM_E_ARG, "unknown colour scheme %d", scheme);
    for (int64_t r = 0; r < n; ++r) {
        const double c0 = rgb[3 * r], c1 = rgb[3 * r + 1], c2 = rgb[3 * r + 2];
        for (int i = 0; i < 3; ++i) out[3 * r + i] = fma(m[3 * i + 2], c2, fma(m[3 * i], c0, m[3 * i + 1] * c1));
    }
    return PCCM_OK;
}

// Host helper for the PCD reader (io.py): liblzf decompression (binary_compressed bodies).  Format: a control byte c;
// c < 32: c + 1 literal bytes follow; otherwise a back reference of length (c >> 5) + 2 (7 in the field: one more
// length byte is added) at distance (((c & 31) << 8) | next byte) + 1.
int pccm_lzf_decompress(const unsigned char *in, int64_t in_len, unsigned char *out, int64_t out_cap, int64_t *out_len)
{
    if (!in || !out || !out_len || in_len < 0 || out_cap < 0) return fail(PCCM_E_ARG, "bad argument");
    int64_t ip = 0, op = 0;
    while (ip < in_len) {
        const unsigned c = in[ip++];
        if (c < 32) {
            const int64_t run = (int64_t)c + 1;
            if (ip + run > in_len || op + run > out_cap) return fail(PCCM_E_ARG, "corrupt LZF stream (literal run)");
            memcpy(out + op, in + ip, (size_t)run);
            ip += run;
            op += run;
        } else {
            int64_t len = c >> 5;
            if (len == 7) {
                if (ip >= in_len) return fail(PCCM_E_ARG, "corrupt LZF stream (length)");
                len += in[ip++];
            }
            if (ip >= in_len) return fail(PCCM_E_ARG, "corrupt LZF stream (offset)");
            const int64_t ref = op - ((int64_t)(c & 31) << 8) - in[ip++] - 1;
            len += 2;
            if (ref < 0 || op + len > out_cap) return fail(PCCM_E_ARG, "corrupt LZF stream (back reference)");
            for (int64_t k = 0; k < len; ++k) out[op + k] = out[ref + k];      // may overlap: byte by byte
            op += len;
        }
    }
    *out_len = op;
    return PCCM_OK;
}

int pccm_drop_caches(pccm_ctx *ctx)
{
    CHECK_CTX(ctx);
    if (ctx->capturing) {
        GraphOp op;
        op.kind = 0;
        ctx->cap_ops.push_back(op);
    } else if (ctx->grid.key != 0) {
        // The caller drops a search structure it has used: it is going to search the same resident clouds AGAIN (a sequence
        // of reports, the bench's steps).  That is when the spatial order pays -- one more counting sort per cloud now, every
        // later rebuild reads coherent rows (Cloud::sp) -- and a pair that is searched once (the command line, `end_to_end`)
        // never pays for it.
        for (int k = 0; k < 2; ++k) {
            Cloud &c = ctx->cloud[k];
            if (c.n <= 0 || c.sp_valid || c.sp_tried) continue;
            c.sp_tried = true;
            int rc = spatial_order(ctx, c);
            if (rc) return rc;
            if (c.sp_valid) ctx->epoch++;                    // graphs captured before carry the row-order build
        }
    }
    grid_invalidate(ctx);
    return PCCM_OK;
}

// ---- hipGraph capture of a call sequence ------------------------------------------------------------------
// A report over resident clouds is ~45 small launches; issued eagerly the host cannot feed the GPU fast
// enough (MI355X_MICROARCH.md: ~3.5 us per launch).  pccm_graph_begin/end capture the sequence
// {pccm_drop_caches, pccm_nn, pccm_reduce_prefetch}* on the context's stream into a hipGraph;
// pccm_graph_launch replays it with one launch and re-applies the host-side bookkeeping of every call.
static void graph_free(GraphRec &g)
{
    if (g.exec) (void)hipGraphExecDestroy(g.exec);
    if (g.graph) (void)hipGraphDestroy(g.graph);
    g.exec = nullptr;
    g.graph = nullptr;
    g.valid = false;
    g.ops.clear();
}

static int graph_replay(pccm_ctx *ctx, GraphRec &g)
{
    for (auto &op : g.ops) {
        if (op.kind == 1) {
            ctx->nn_gen[op.dir]++;
            ctx->nn[op.dir].valid = true;
            ctx->nn[op.dir].form = op.form;
        } else if (op.kind == 5) {                                   // (the graph counts again, behind the search)
            ctx->match[op.dir].gen = ctx->nn_gen[op.dir];
        } else if (op.kind >= 2) {                                   // (in order: a slot takes the generation a kind 1 op before it left)
            int rc = std::visit([&](const auto &snap) { return slot_replay(ctx, table_of(ctx, snap)[op.slot], snap); }, op.snap);
            if (rc) return rc;
        }
    }
    ctx->batches_issued += g.batches;                            // before the launch: a failed one only delays a waiter
    PCCM_HIP(hipGraphLaunch(g.exec, ctx->stream));
    PCCM_HIP(hipEventRecord(ctx->batch_ev, ctx->stream));          // one record for every reduction of the graph
    return PCCM_OK;
}

int pccm_set_tail_filing(pccm_ctx *ctx, int on)
{
    CHECK_CTX(ctx);
    if (!ctx->capturing) return fail(PCCM_E_STATE, "pccm_set_tail_filing speaks of the capture in progress: call pccm_graph_begin first");
    ctx->tail_file.wish = on != 0;
    return PCCM_OK;
}

int pccm_graph_tail_filed(pccm_ctx *ctx, int graph_id, int *filed)
{
    CHECK_CTX(ctx);
    if (!filed) return fail(PCCM_E_ARG, "null pointer");
    if (graph_id < 0 || graph_id >= (int)ctx->graphs.size() || !ctx->graphs[graph_id].valid)
        return fail(PCCM_E_ARG, "unknown graph %d", graph_id);
    *filed = ctx->graphs[graph_id].tails_filed ? 1 : 0;
    return PCCM_OK;
}

int pccm_graph_begin(pccm_ctx *ctx)
{
    CHECK_CTX(ctx);
    if (ctx->capturing) return fail(PCCM_E_STATE, "already capturing");
    if (ctx->ties != PCCM_TIES_PICK) return fail(PCCM_E_STATE, "searches under PCCM_TIES_MEAN run eagerly: no graph capture");
    PCCM_HIP(hipStreamSynchronize(ctx->stream));
    // filed tails: what the eager step in front of this capture left decides whether the capture may file (pccm_tail_wave.h)
    ctx->tail_file.wish = true;
    ctx->tail_file.left_out = ctx->tail_file.resolved = false;
    int rcf = tail_facts(ctx, &ctx->tail_file.allowed, &ctx->tail_file.fact_dirs);
    if (rcf) return rcf;
    for_each_slot(ctx, [](SlotKey &k) { k.pending = false; });      // nothing outside the graph may be half-consumed
    ctx->cap_ops.clear();
    ctx->cap_batches = 0;
    ctx->capture_failed = false;
    PCCM_HIP(hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
    ctx->capturing = true;
    return PCCM_OK;
}

int pccm_graph_end(pccm_ctx *ctx, int *graph_id)
{
    CHECK_CTX(ctx);
    if (!graph_id) return fail(PCCM_E_ARG, "null pointer");
    if (!ctx->capturing) return fail(PCCM_E_STATE, "pccm_graph_begin was not called");
    // filed tails nobody has consumed (no reduction of that direction in the sequence): the classic tail launch ends the graph
    const int rct = ctx->capture_failed ? PCCM_OK : filed_tails_resolve(ctx);
    if (rct) ctx->capture_failed = true;
    ctx->nn[PCCM_DIR_LEFT].form.tails_filed = ctx->nn[PCCM_DIR_RIGHT].form.tails_filed = false;
    ctx->capturing = false;
    GraphRec g;
    g.tails_filed = ctx->tail_file.left_out && !ctx->tail_file.resolved;
    ctx->tail_file.wish = ctx->tail_file.left_out = ctx->tail_file.resolved = false;
    hipError_t e = hipStreamEndCapture(ctx->stream, &g.graph);
    if (e != hipSuccess || ctx->capture_failed || !g.graph) {
        (void)hipGetLastError();
        if (g.graph) (void)hipGraphDestroy(g.graph);
        // whatever the captured calls recorded on the host never ran on the GPU
        results_dropped(ctx);
        grid_invalidate(ctx);
        return fail(PCCM_E_STATE, "graph capture failed (%s); the context is usable, results were invalidated",
                    e != hipSuccess ? hipGetErrorString(e) : "a captured call reported an error");
    }
    e = hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0);
    if (e != hipSuccess) {
        (void)hipGraphDestroy(g.graph);
        results_dropped(ctx);
        grid_invalidate(ctx);
        return fail(PCCM_E_HIP, "hipGraphInstantiate: %s", hipGetErrorString(e));
    }
    g.ops = ctx->cap_ops;
    for (auto &op : g.ops)
        if (op.kind == 1) op.form = ctx->nn[op.dir].form;  // the state the captured sequence leaves behind
    g.epoch = ctx->epoch;
    g.batches = ctx->cap_batches;
    g.valid = true;
    // the captured calls changed the host bookkeeping but nothing ran yet: run the graph once now
    for (auto &op : g.ops)
        if (op.kind >= 2 && op.kind <= 4) std::visit([&](const auto &snap) { rearm(table_of(ctx, snap)[op.slot], ctx, snap.key.wait_seq); }, op.snap);
    ctx->batches_issued += g.batches;
    PCCM_HIP(hipGraphLaunch(g.exec, ctx->stream));
    PCCM_HIP(hipEventRecord(ctx->batch_ev, ctx->stream));
    int id = -1;
    for (size_t k = 0; k < ctx->graphs.size(); ++k)
        if (!ctx->graphs[k].valid && !ctx->graphs[k].exec) { id = (int)k; break; }
    if (id < 0) { ctx->graphs.emplace_back(); id = (int)ctx->graphs.size() - 1; }
    ctx->graphs[id] = g;
    *graph_id = id;
    return PCCM_OK;
}

int pccm_graph_launch(pccm_ctx *ctx, int graph_id)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    if (graph_id < 0 || graph_id >= (int)ctx->graphs.size() || !ctx->graphs[graph_id].valid)
        return fail(PCCM_E_ARG, "unknown graph %d", graph_id);
    GraphRec &g = ctx->graphs[graph_id];
    if (g.epoch != ctx->epoch) {
        graph_free(g);
        return fail(PCCM_E_STATE, "graph %d is stale: inputs, shard or buffers changed since it was captured", graph_id);
    }
    return graph_replay(ctx, g);
}

int pccm_graph_destroy(pccm_ctx *ctx, int graph_id)
{
    CHECK_CTX(ctx);
    if (graph_id < 0 || graph_id >= (int)ctx->graphs.size()) return fail(PCCM_E_ARG, "unknown graph %d", graph_id);
    PCCM_HIP(hipStreamSynchronize(ctx->stream));
    graph_free(ctx->graphs[graph_id]);
    return PCCM_OK;
}

int pccm_ctx_reset(pccm_ctx *ctx)
{
    CHECK_CTX(ctx);
    ctx->nn[PCCM_DIR_LEFT].form.tails_filed = ctx->nn[PCCM_DIR_RIGHT].form.tails_filed = false;
    ctx->tail_file.wish = ctx->tail_file.allowed = ctx->tail_file.left_out = ctx->tail_file.resolved = false;
    ctx->tail_file.fact_dirs = 0;
    ctx->tail_file.brick_key = 0;
    ctx->tail_file.eager_ok = ctx->tail_file.eager_bad = 0;
    if (ctx->capturing) {                              // an abandoned capture: end it, discard what it recorded
        hipGraph_t g = nullptr;
        (void)hipStreamEndCapture(ctx->stream, &g);
        if (g) (void)hipGraphDestroy(g);
        ctx->capturing = false;
        ctx->capture_failed = false;
        ctx->cap_ops.clear();
    }
    PCCM_HIP(hipStreamSynchronize(ctx->stream));
    ctx->io_staged = false;                            // (the next owner of the context says what it wants)
    ctx->ties = PCCM_TIES_PICK;
    context_cleared(ctx);
    for (auto &g : ctx->graphs) graph_free(g);
    ctx->graphs.clear();
    grid_invalidate(ctx);                              // the geometry decisions stay: the next pair may inherit them
    int rc = collect_spans(ctx);
    ctx->prof_on = false;
    for (int k = 0; k < PCCM_K_COUNT; ++k) { ctx->prof_ms[k] = 0.0; ctx->prof_n[k] = 0; }
    return rc;
}

int pccm_sync(pccm_ctx *ctx)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    PCCM_HIP(hipStreamSynchronize(ctx->stream));
    return check_device_errors(ctx);
}

int pccm_profile_enable(pccm_ctx *ctx, int on)
{
    CHECK_CTX(ctx);
    int rc = collect_spans(ctx);
    ctx->prof_on = on != 0;
    return rc;
}

int pccm_profile_reset(pccm_ctx *ctx)
{
    CHECK_CTX(ctx);
    int rc = collect_spans(ctx);
    for (int k = 0; k < PCCM_K_COUNT; ++k) {
        ctx->prof_ms[k] = 0.0;
        ctx->prof_n[k] = 0;
    }
    return rc;
}

int pccm_profile_get(pccm_ctx *ctx, int kernel_class, double *ms_total, int64_t *launches)
{
    CHECK_CTX(ctx);
    if (kernel_class < 0 || kernel_class >= PCCM_K_COUNT || !ms_total || !launches) return fail(PCCM_E_ARG, "bad argument");
    int rc = collect_spans(ctx);
    if (rc) return rc;
    *ms_total = ctx->prof_ms[kernel_class];
    *launches = ctx->prof_n[kernel_class];
    return PCCM_OK;
}

// "k_brick_query<false, 4, 2, 2176, false, 0, true>" for a kernel handle: its symbol demangled, without the return type, the
// namespace and the parameter list -- how `nm -C` names the kernel's host stub after "__device_stub__"
static std::string kernel_name(const void *k)
{
    Dl_info info;
    if (!dladdr(k, &info) || !info.dli_sname || info.dli_saddr != k) return "?";
    int st = 0;
    char *dm = abi::__cxa_demangle(info.dli_sname, nullptr, nullptr, &st);
    std::string s = st == 0 && dm ? dm : info.dli_sname;
    free(dm);
    if (s.compare(0, 5, "void ") == 0) s.erase(0, 5);
    if (s.compare(0, 6, "pccm::") == 0) s.erase(0, 6);
    int depth = 0;
    for (size_t i = 0; i < s.size(); ++i) {
        if (s[i] == '<') ++depth;
        else if (s[i] == '>') --depth;
        else if (s[i] == '(' && depth == 0) return s.substr(0, i);
    }
    return s;
}

int pccm_nn_path(pccm_ctx *ctx, int which, char *buf, int64_t cap, int64_t *len)
{
    CHECK_CTX(ctx);
    if (which < 0 || which > PCCM_PATH_REDUCE || (cap > 0 && !buf) || cap < 0) return fail(PCCM_E_ARG, "bad argument");
    std::string s;
    for (int i = 0; i < ctx->path_n[which]; ++i) {
        if (i) s += ';';
        s += kernel_name(ctx->path[which][i]);
    }
    if (ctx->path_over[which]) s += ";...";
    if (len) *len = (int64_t)s.size();
    if (cap > 0) {
        const size_t n = s.size() < (size_t)cap - 1 ? s.size() : (size_t)cap - 1;
        memcpy(buf, s.data(), n);
        buf[n] = 0;
    }
    return PCCM_OK;
}

int pccm_grid_geometry(pccm_ctx *ctx, double org[3], double h[3], int32_t dim[3])
{
    CHECK_CTX(ctx);
    if (!org || !h || !dim) return fail(PCCM_E_ARG, "null pointer");
    if (ctx->grid.ncells <= 0) return fail(PCCM_E_STATE, "no grid search has run");
    for (int a = 0; a < 3; ++a) {
        org[a] = ctx->grid.org[a];
        h[a] = ctx->grid.h[a];
        dim[a] = ctx->grid.dim[a];
    }
    return PCCM_OK;
}

int pccm_build_plan(pccm_ctx *ctx, int which, int64_t plan[PCCM_BP_COUNT], double geom[6])
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    if (!plan || !geom) return fail(PCCM_E_ARG, "null pointer");
    return build_plan(ctx, which, plan, geom);
}

int pccm_build_fetch(pccm_ctx *ctx, int which, uint32_t *cell_start, int32_t *rows, double *xyz, uint32_t *occ)
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    return build_fetch(ctx, which, cell_start, rows, xyz, occ);
}

int pccm_nn_stats(pccm_ctx *ctx, int dir, int64_t out[3])
{
    CHECK_CTX(ctx);
    NOT_CAPTURING(ctx);
    if (!out) return fail(PCCM_E_ARG, "null pointer");
    const Cloud *it, *se;
    NNResult *res;
    const bool tail = (dir & PCCM_STATS_TAIL) != 0, ties = (dir & PCCM_STATS_TIES) != 0;
    dir &= ~(PCCM_STATS_TAIL | PCCM_STATS_TIES);
    int rc = need_nn(ctx, dir, &it, &se, &res);
    if (rc) return rc;
    if (ties) {
        if (res->ties != PCCM_TIES_MEAN) return fail(PCCM_E_STATE, "the search of direction %d did not run under PCCM_TIES_MEAN", dir);
        if ((rc = ensure_ties(ctx, dir, false, false))) return rc;
        const int64_t ns = res->end - res->begin;
        int32_t nl = 0;
        PCCM_HIP(hipMemcpyAsync(&nl, (const int32_t *)ctx->tie[dir].k.p + (ns > 0 ? ns : 0), sizeof(nl), hipMemcpyDeviceToHost, ctx->stream));
        PCCM_HIP(hipStreamSynchronize(ctx->stream));
        out[0] = nl;
        out[1] = out[2] = 0;
        return PCCM_OK;
    }
    if (tail) {
        uint32_t nt = 0;
        PCCM_HIP(hipMemcpyAsync(&nt, res->nflag_dev + 1, sizeof(nt), hipMemcpyDeviceToHost, ctx->stream));
        PCCM_HIP(hipStreamSynchronize(ctx->stream));
        out[0] = nt;
        out[1] = out[2] = 0;
        return PCCM_OK;
    }
    uint32_t nf = 0;
    PCCM_HIP(hipMemcpyAsync(&nf, res->nflag_dev, sizeof(nf), hipMemcpyDeviceToHost, ctx->stream));
    PCCM_HIP(hipStreamSynchronize(ctx->stream));
    out[0] = nf;
    out[1] = res->stats[1];
    out[2] = res->stats[2];
    return PCCM_OK;
}

}  // extern "C"
