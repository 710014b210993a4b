// hsflow_api.cpp -- the C ABI declared in include/hsflow.h.
//
// Host side of the drop-in boundary for HornSchunckOF/hornSchunck.cpp:
//   getFlow      (hornSchunck.cpp:43-75) -> hsflow_flow / hsflow_flow_device
//   getGradients (hornSchunck.cpp:19-41) -> hsflow_gradients / *_device
// Context = device + stream + grow-only device buffers, so repeated getFlow
// calls on same-size frames (main.cpp:97-98 in a loop) never reallocate.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/hsflow.h"
#include "hsflow_internal.h"

using hsflow::JacobiArgs;

struct hsflow_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    // device buffers (grow-only)
    void *d_in = nullptr;
    size_t d_in_bytes = 0;  // holds I0 and I1
    void *d_out = nullptr;
    size_t d_out_bytes = 0;  // holds u, v (or gx, gy, gt)
    void *d_ws = nullptr;
    size_t d_ws_bytes = 0;
    // pinned host staging of f32 planes on their way to f64 rows
    char *h_stage = nullptr;
    size_t h_stage_bytes = 0;
    // one event per downloaded row chunk (created on first use)
    std::vector<hipEvent_t> dl_ev;
    // hsflow_ctx_set_prefilter: what the warped, bidirectional and interpolating
    // host-buffer calls run on the frames first (mode 0: nothing)
    hsflow_prefilter pf{0, 0.0f, 0.0f, 0.0f};
    // hsflow_ctx_set_smoothness: the smoothness term of the same calls' solves
    // (mode 0: the quadratic one)
    hsflow_smoothness sm{0, 0.0f};
};

namespace {

thread_local std::string g_err;  // errors from calls without a context
int g_kb_override = 0;
// Jacobi pass kernel (hsflow_set_jacobi_kernel): 0 = automatic (K4 strips
// where built, else K2), 2 = K2 tiles everywhere, 4 = K4 where built
int g_kernel_override = 0;
// K4 rows per segment (hsflow_set_strip_rows): 0 = automatic
int g_strip_rows = 0;


// Kernel and blocking depth of a launch's passes.  K4 (streaming strips)
// runs the full-depth passes when it is built for the window's default
// depth and -- automatic choice -- its waves fill the chip (launches too
// small for it keep K2's tiles, whose depth adapts to the fill);
// hsflow_set_jacobi_kernel(4) forces it wherever it is built.
struct PassPlan {
    int kb;
    bool strip;
};

// K4's depth: the caller's (hsflow_set_iters_per_launch) or the window's default
int strip_kb(int window) {
    return g_kb_override > 0 ? g_kb_override : hsflow::default_kb(window);
}

bool strip_use(int window, int rows, int cols, int batch) {
    const int kb = strip_kb(window);
    if (g_kernel_override == 2 || window > 9 || !hsflow::strip_supported(window, kb)) return false;
    if (g_kernel_override == 4) return true;
    return rows > 0 && cols > 0 && batch > 0 &&
           hsflow::strip_fills(window, kb, rows, cols, batch, 8 * hsflow::device_cus());
}

int fail(hsflow_ctx *ctx, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx)
        ctx->err = buf;
    else
        g_err = buf;
    return code;
}

int hip_fail(hsflow_ctx *ctx, hipError_t e, const char *what) {
    return fail(ctx, e == hipErrorOutOfMemory ? HSFLOW_ERR_OOM : HSFLOW_ERR_HIP,
                "%s: %s (%d)", what, hipGetErrorString(e), (int)e);
}

#define HIP_TRY(ctx, expr)                                    \
    do {                                                      \
        hipError_t e_ = (expr);                               \
        if (e_ != hipSuccess) return hip_fail(ctx, e_, #expr); \
    } while (0)

constexpr size_t kAlign = 256;
size_t align_up(size_t x) { return (x + kAlign - 1) / kAlign * kAlign; }

// Largest frame: plane bytes must fit the 31-bit buffer offsets of K2.
constexpr long long kMaxPlanePixels = (1ll << 29) - 1;

// Largest batch: pairs index gridDim.y / gridDim.z of the kernels (65535);
// tallest plane: the 64 x 4 per-pixel kernels put rows / 4 in gridDim.y.
constexpr int kMaxBatch = 65535;
constexpr int kMaxRows = 4 * 65535;

bool sizes_ok(int rows, int cols, int batch) {
    return rows >= 1 && rows <= kMaxRows && cols >= 1 && batch >= 1 &&
           batch <= kMaxBatch && (long long)rows * cols <= kMaxPlanePixels;
}

struct Workspace {
    uint32_t *gpack;
    float *gx, *gy, *gt, *u2, *v2;
    uint32_t *flags;
    size_t bytes;
};

Workspace carve(void *base, int rows, int cols, int batch) {
    const size_t n = (size_t)rows * cols * batch;
    Workspace w{};
    size_t off = 0;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off = align_up(off + bytes);
        return (char *)base + o;
    };
    w.gpack = (uint32_t *)take(n * 4);
    w.gx = (float *)take(n * 4);
    w.gy = (float *)take(n * 4);
    w.gt = (float *)take(n * 4);
    w.u2 = (float *)take(n * 4);
    w.v2 = (float *)take(n * 4);
    w.flags = (uint32_t *)take((size_t)batch * 4);
    w.bytes = off;
    return w;
}

int elem_size(int dtype) {
    switch (dtype) {
    case HSFLOW_U8: return 1;
    case HSFLOW_F32: return 4;
    case HSFLOW_F64: return 8;
    case HSFLOW_F16: return 2;
    default: return 0;
    }
}

// element size of the device copy of a host input (every input type is
// uploaded as it is: K1 reads u8, f16, f32 and f64 frames)
int dev_elem_size(int dtype) { return elem_size(dtype); }

bool device_dtype_ok(int dtype) {
    return dtype == HSFLOW_U8 || dtype == HSFLOW_F32 || dtype == HSFLOW_F16 ||
           dtype == HSFLOW_F64;
}

// `batch`: every pair in flight at once (the whole batch, also when it is
// split over side streams); 0 = shape unknown (no fill adjustment)
PassPlan plan_passes(int window, bool need_f32, int rows = 0, int cols = 0, int batch = 0) {
    if (window > 9) return {1, false};
    if (strip_use(window, rows, cols, batch)) return {strip_kb(window), true};
    if (g_kb_override > 0 && hsflow::kb_supported(window, g_kb_override, need_f32))
        return {g_kb_override, false};
    int kb = hsflow::fill_kb(window, hsflow::default_kb(window), rows, cols, batch);
    while (kb > 1 && !hsflow::kb_supported(window, kb, need_f32)) kb /= 2;
    return {kb, false};
}

int pick_kb(int window, bool need_f32, int rows = 0, int cols = 0, int batch = 0) {
    return plan_passes(window, need_f32, rows, cols, batch).kb;
}

// Per-thread, per-device side streams for splitting a batch: each sub-batch
// runs its Jacobi passes on its own stream, so the launches of the two halves
// overlap (one's tail and boundary with the other's work).  Default 2 halves:
// same-box bench, 1080p x 8 / 4K x 2 Mpix*iter/s: 1 stream 905k / 960k,
// 2 streams 967k / 1034k, 4 streams 901k / 1033k, 8 streams 865k / 1032k
// (scripts/streams_ab.sh).  Fork and join are event based (capturable into a
// hipGraph).  Never destroyed: they live until the process exits (no
// static-destruction-order hazards).
// The *_device entry points run on the device their stream belongs to
// (the current device for the null stream), whatever device the calling
// thread has current: side streams, the CU count and the launches all follow
// the caller's stream.
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(hipStream_t s) {
        int cur = 0;
        hipDevice_t d = 0;
        if (!s || hipGetDevice(&cur) != hipSuccess || hipStreamGetDevice(s, &d) != hipSuccess)
            return;
        if (d != cur && hipSetDevice(d) == hipSuccess) prev = cur;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

struct SidePool {
    int device = -1;
    std::vector<hipStream_t> streams;
    std::vector<hipEvent_t> events;  // [0] fork, [1..] joins
};

// hsflow_set_max_streams: 0 = automatic (split in 2 eagerly, not at all
// while the caller's stream is capturing), n >= 1 = up to n streams always
int g_split_override = 0;

// Streams a batch of `batch` pairs on `s` is split over.  Under stream
// capture the automatic choice does not split: a stream forked inside a
// capture from a capturing stream that is not the capture's origin crashes
// hipStreamEndCapture on ROCm 7.2 (profiles/r04_capture_crash.txt; legal in
// CUDA), and the library cannot tell an origin from a forked stream.  A
// caller that captures on the origin itself may ask for the split with
// hsflow_set_max_streams(n >= 2) (the bench's timed graphs do).
int split_for(int batch, hipStream_t s) {
    if (g_split_override > 0) return std::min(batch, g_split_override);
    if (batch < 2) return 1;
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) != hipSuccess || st != hipStreamCaptureStatusNone) return 1;
    return 2;
}

SidePool *side_pool(int need) {
    // one pool per device and thread: a thread that alternates devices keeps
    // each device's streams (re-creating them per switch would leak them)
    thread_local std::vector<SidePool> pools;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) return nullptr;
    if ((int)pools.size() <= dev) pools.resize(dev + 1);
    SidePool &pool = pools[dev];
    pool.device = dev;
    while ((int)pool.streams.size() < need) {
        hipStream_t st;
        if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return nullptr;
        pool.streams.push_back(st);
    }
    while ((int)pool.events.size() < need + 1) {
        hipEvent_t ev;
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return nullptr;
        pool.events.push_back(ev);
    }
    return &pool;
}

// hsflow_set_first_pass_fusion: a cold K4 solve computes K1's outputs in its
// first pass (1, default) or runs K1 in front of the passes (0)
int g_first_fusion = 1;
// hsflow_first_pass_launches: fused first passes launched so far
std::atomic<long long> g_first_launches{0};

// The frames of a cold solve whose first pass has K1 fused in (fuse_first);
// null for every other solve: the workspace then holds K1's outputs already.
struct Frames {
    const void *I0, *I1;
    int dtype;
};

int jacobi_one(hsflow_ctx *ctx, int rows, int cols, int batch, int window, int iters,
               float alpha, bool warm, bool maybe_f32, float *u, float *v,
               void *workspace, size_t ws_bytes, hipStream_t s, const Frames *fr = nullptr,
               const float *g = nullptr);
int check_jacobi_args(hsflow_ctx *ctx, int rows, int cols, int batch, int window,
                      int iters, const float *u, const float *v, void *workspace,
                      size_t ws_bytes);
int jacobi_sub(hsflow_ctx *ctx, int rows, int cols, int nb, int first, int batch,
               int window, int iters, float alpha, bool warm, bool maybe_f32, float *u,
               float *v, const Workspace &w, hipStream_t s, const Frames *fr = nullptr,
               const float *g = nullptr);

// `g`: the weights of the flow-driven smoothness term (batch planes, as u and
// v); then the passes are KJ's weighted ones (always warm, f32 planes), else
// the plain Jacobi passes.
int jacobi_impl(hsflow_ctx *ctx, int rows, int cols, int batch, int window, int iters,
                float alpha, bool warm, bool maybe_f32, float *u, float *v,
                void *workspace, size_t ws_bytes, hipStream_t s, const Frames *fr = nullptr,
                const float *g = nullptr) {
    int rc0 = check_jacobi_args(ctx, rows, cols, batch, window, iters, u, v, workspace,
                                ws_bytes);
    if (rc0) return rc0;
    const int split = split_for(batch, s);
    if (split <= 1 || iters == 0)
        return jacobi_one(ctx, rows, cols, batch, window, iters, alpha, warm, maybe_f32, u,
                          v, workspace, ws_bytes, s, fr, g);
    Workspace w = carve(workspace, rows, cols, batch);
    SidePool *pool = side_pool(split);
    if (!pool)
        return jacobi_one(ctx, rows, cols, batch, window, iters, alpha, warm, maybe_f32, u,
                          v, workspace, ws_bytes, s, fr, g);
    const size_t plane = (size_t)rows * cols;
    HIP_TRY(ctx, hipEventRecord(pool->events[0], s));
    int first = 0, forked = 0, rc = HSFLOW_OK;
    for (int k = 0; k < split && rc == HSFLOW_OK; ++k) {
        const int nb = batch / split + (k < batch % split ? 1 : 0);
        hipStream_t sk = pool->streams[k];
        hipError_t e = hipStreamWaitEvent(sk, pool->events[0], 0);
        if (e != hipSuccess) {
            rc = hip_fail(ctx, e, "hipStreamWaitEvent (fork)");
            break;
        }
        ++forked;
        // the sub-batch's slice of every workspace plane, as its own workspace
        rc = jacobi_sub(ctx, rows, cols, nb, first, batch, window, iters, alpha, warm,
                        maybe_f32, u + first * plane, v + first * plane, w, sk, fr,
                        g ? g + first * plane : nullptr);
        first += nb;
    }
    // join every forked stream back, the error path included (a capture
    // must not be left with streams that never rejoin its origin)
    for (int k = 0; k < forked; ++k) {
        hipError_t e = hipEventRecord(pool->events[1 + k], pool->streams[k]);
        if (e == hipSuccess) e = hipStreamWaitEvent(s, pool->events[1 + k], 0);
        if (e != hipSuccess && rc == HSFLOW_OK) rc = hip_fail(ctx, e, "stream join");
    }
    return rc;
}

// KJ's depth: the caller's (hsflow_set_iters_per_launch) where KJ is built for
// it, else the window's default
int weighted_kb(int window) {
    return hsflow::weighted_kb_supported(window, g_kb_override) ? g_kb_override
                                                                : hsflow::weighted_default_kb(window);
}

// `iters` weighted iterations (KJ) of `batch` pairs from (u, v), the f32
// gradient planes of `w` and the weights g; ping-pong with w.u2 / w.v2 as
// run_passes does, the last pass landing in (u, v).
int run_weighted_passes(hsflow_ctx *ctx, int rows, int cols, int batch, int window, int iters,
                        float alpha, const float *g, float *u, float *v, const Workspace &w,
                        hipStream_t s) {
    if (iters == 0) return HSFLOW_OK;
    const size_t n = (size_t)rows * cols * batch;
    const int kb = weighted_kb(window);
    const int passes = (iters + kb - 1) / kb;
    JacobiArgs a{};
    a.rows = rows;
    a.cols = cols;
    a.batch = batch;
    a.alpha2 = (float)((double)alpha * (double)alpha);
    a.gx = w.gx;
    a.gy = w.gy;
    a.gt = w.gt;
    auto dst_is_user = [&](int pass) { return ((passes - 1 - pass) & 1) == 0; };
    const float *src_u = u, *src_v = v;
    if (dst_is_user(0)) {  // would read and write (u, v) in one pass
        HIP_TRY(ctx, hipMemcpyAsync(w.u2, u, n * 4, hipMemcpyDeviceToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(w.v2, v, n * 4, hipMemcpyDeviceToDevice, s));
        src_u = w.u2;
        src_v = w.v2;
    }
    int done = 0;
    for (int pass = 0; pass < passes; ++pass) {
        a.iters = std::min(kb, iters - done);
        a.u_in = src_u;
        a.v_in = src_v;
        a.u_out = dst_is_user(pass) ? u : w.u2;
        a.v_out = dst_is_user(pass) ? v : w.v2;
        hipError_t e = hsflow::launch_jacobi_weighted(a, g, window, kb, s);
        if (e != hipSuccess) return hip_fail(ctx, e, "weighted jacobi launch");
        src_u = a.u_out;
        src_v = a.v_out;
        done += a.iters;
    }
    return HSFLOW_OK;
}

// The Jacobi passes of `batch` pairs whose workspace planes are `w` (a view
// that may start at any pair of a larger workspace).
int run_passes(hsflow_ctx *ctx, int rows, int cols, int batch, int window, int iters,
               float alpha, bool warm, bool maybe_f32, float *u, float *v,
               const Workspace &w, hipStream_t s, int fill_batch, const Frames *fr = nullptr,
               const float *g = nullptr) {
    if (g) return run_weighted_passes(ctx, rows, cols, batch, window, iters, alpha, g, u, v, w, s);
    const size_t n = (size_t)rows * cols * batch;
    if (iters == 0) {
        // hornSchunck.cpp:49-50: the loop does not run, u = v = 0
        if (!warm) {
            HIP_TRY(ctx, hipMemsetAsync(u, 0, n * 4, s));
            HIP_TRY(ctx, hipMemsetAsync(v, 0, n * 4, s));
        }
        if (fr) {  // the workspace still gets K1's outputs
            if (fr->dtype != HSFLOW_U8)
                HIP_TRY(ctx, hipMemsetAsync(w.flags, 0, (size_t)batch * 4, s));
            hipError_t e = hsflow::launch_gradients(fr->I0, fr->I1, fr->dtype, rows, cols, batch,
                                                    w.gpack, w.gx, w.gy, w.gt, w.flags, false, s);
            if (e != hipSuccess) return hip_fail(ctx, e, "gradients launch");
        }
        return HSFLOW_OK;
    }
    const PassPlan plan = plan_passes(window, maybe_f32, rows, cols, fill_batch);
    const int kb = plan.kb;
    const int passes = (iters + kb - 1) / kb;
    // K4 for the full-depth passes (two waves per SIMD: 8 per CU), K2 for a
    // shorter last pass -- identical bits either way
    const bool strip = plan.strip;
    // K4 segment height from every pair in flight (the halves of a split
    // batch run concurrently and share the chip's slots)
    int strip_rows = g_strip_rows;
    if (strip && strip_rows <= 0) {
        int nseg = 0, nstrips = 0;
        strip_rows = hsflow::strip_seg_rows(window, kb, rows, cols, fill_batch,
                                            8 * hsflow::device_cus(), &nseg, &nstrips, 0);
    }
    JacobiArgs a{};
    a.rows = rows;
    a.cols = cols;
    a.batch = batch;
    a.alpha2 = (float)((double)alpha * (double)alpha);  // pow(alpha, 2)
    a.inv_w2 = (float)(1.0 / ((double)window * (double)window));
    a.gpack = w.gpack;
    a.gx = w.gx;
    a.gy = w.gy;
    a.gt = w.gt;
    a.flags = w.flags;
    a.write_through =
        hsflow::fill_limited(window, kb, strip, rows, cols, fill_batch, strip_rows) ? 1 : 0;

    // pass p writes the caller's buffers iff (passes-1-p) is even, so the
    // last pass always lands in (u, v)
    auto dst_is_user = [&](int pass) { return ((passes - 1 - pass) & 1) == 0; };
    const float *src_u = nullptr, *src_v = nullptr;
    if (warm) {
        if (dst_is_user(0)) {  // would read and write (u, v) in one pass
            HIP_TRY(ctx, hipMemcpyAsync(w.u2, u, n * 4, hipMemcpyDeviceToDevice, s));
            HIP_TRY(ctx, hipMemcpyAsync(w.v2, v, n * 4, hipMemcpyDeviceToDevice, s));
            src_u = w.u2;
            src_v = w.v2;
        } else {
            src_u = u;
            src_v = v;
        }
    }
    // `fr`: K1 has not run for these pairs.  Where this plan has a full-depth
    // K4 pass it is fused into pass 0: this chain's flags zeroed, the fused
    // pass, then K1f for the chain's pairs, whose planes pass 1 may read (it
    // returns at once for the others).  Under any other plan (cold_solve
    // hands the frames down only when it expects this one) the chain runs K1
    // itself in front of its passes.
    const bool fuse = fr && strip && !warm && iters >= kb;
    if (fr && fr->dtype != HSFLOW_U8)
        HIP_TRY(ctx, hipMemsetAsync(w.flags, 0, (size_t)batch * 4, s));
    if (fr && !fuse) {
        hipError_t e = hsflow::launch_gradients(fr->I0, fr->I1, fr->dtype, rows, cols, batch,
                                                w.gpack, w.gx, w.gy, w.gt, w.flags, false, s);
        if (e != hipSuccess) return hip_fail(ctx, e, "gradients launch");
    }
    int done = 0;
    for (int pass = 0; pass < passes; ++pass) {
        a.iters = std::min(kb, iters - done);
        a.u_in = src_u;
        a.v_in = src_v;
        a.u_out = dst_is_user(pass) ? u : w.u2;
        a.v_out = dst_is_user(pass) ? v : w.v2;
        if (fuse && pass == 0) {
            const hsflow::FirstArgs f{fr->I0, fr->I1, w.gpack, w.flags, 0};
            hipError_t e =
                hsflow::launch_jacobi_strip_first(a, f, fr->dtype, window, kb, strip_rows, s);
            if (e == hipSuccess)
                e = hsflow::launch_gradients_f32(fr->I0, fr->I1, fr->dtype, rows, cols, batch,
                                                 w.gx, w.gy, w.gt, w.flags, s);
            if (e != hipSuccess) return hip_fail(ctx, e, "fused first pass launch");
            g_first_launches.fetch_add(1, std::memory_order_relaxed);
            src_u = a.u_out;
            src_v = a.v_out;
            done += a.iters;
            continue;
        }
        // a K2 pass (a shorter last pass of a K4 solve) takes a depth K2 is
        // built for: any depth >= its iterations gives the same bits
        int kb2 = kb;
        if (!hsflow::kb_supported(window, kb2, maybe_f32)) {
            kb2 = a.iters;
            while (kb2 < 8 && !hsflow::kb_supported(window, kb2, maybe_f32)) ++kb2;
            if (!hsflow::kb_supported(window, kb2, maybe_f32))
                return fail(ctx, HSFLOW_ERR_ARG, "no K2 depth >= %d for window %d", a.iters,
                            window);
        }
        hipError_t e = (strip && a.iters == kb)
                           ? hsflow::launch_jacobi_strip(a, window, kb, strip_rows, s)
                           : hsflow::launch_jacobi(a, window, kb2, s);
        if (e != hipSuccess) return hip_fail(ctx, e, "jacobi launch");
        src_u = a.u_out;
        src_v = a.v_out;
        done += a.iters;
    }
    return HSFLOW_OK;
}

int check_jacobi_args(hsflow_ctx *ctx, int rows, int cols, int batch, int window,
                      int iters, const float *u, const float *v, void *workspace,
                      size_t ws_bytes) {
    if (!sizes_ok(rows, cols, batch))
        return fail(ctx, HSFLOW_ERR_ARG, "bad size %dx%d batch %d", rows, cols, batch);
    if (window < 1 || window > HSFLOW_MAX_WINDOW)
        return fail(ctx, HSFLOW_ERR_ARG, "windowSize %d outside [1, %d]", window,
                    HSFLOW_MAX_WINDOW);
    if (iters < 0) return fail(ctx, HSFLOW_ERR_ARG, "maxIterations %d < 0", iters);
    if (!u || !v || !workspace) return fail(ctx, HSFLOW_ERR_ARG, "null device pointer");
    if (ws_bytes < carve(workspace, rows, cols, batch).bytes)
        return fail(ctx, HSFLOW_ERR_ARG, "workspace %zu < %zu bytes", ws_bytes,
                    carve(workspace, rows, cols, batch).bytes);
    return HSFLOW_OK;
}

int jacobi_one(hsflow_ctx *ctx, int rows, int cols, int batch, int window, int iters,
               float alpha, bool warm, bool maybe_f32, float *u, float *v,
               void *workspace, size_t ws_bytes, hipStream_t s, const Frames *fr,
               const float *g) {
    int rc = check_jacobi_args(ctx, rows, cols, batch, window, iters, u, v, workspace,
                               ws_bytes);
    if (rc) return rc;
    return run_passes(ctx, rows, cols, batch, window, iters, alpha, warm, maybe_f32, u, v,
                      carve(workspace, rows, cols, batch), s, batch, fr, g);
}

// pairs [first, first + nb) of a `batch`-pair workspace w
int jacobi_sub(hsflow_ctx *ctx, int rows, int cols, int nb, int first, int batch,
               int window, int iters, float alpha, bool warm, bool maybe_f32, float *u,
               float *v, const Workspace &w, hipStream_t s, const Frames *fr, const float *g) {
    const size_t off = (size_t)first * rows * cols;
    Workspace sub = w;
    sub.gpack = w.gpack + off;
    sub.gx = w.gx + off;
    sub.gy = w.gy + off;
    sub.gt = w.gt + off;
    sub.u2 = w.u2 + off;
    sub.v2 = w.v2 + off;
    sub.flags = w.flags + first;
    // the split's halves run concurrently: the depth is chosen for the batch
    // ... and the sub-batch's frames, for a fused first pass
    Frames sf{};
    if (fr) {
        const size_t fo = off * (size_t)elem_size(fr->dtype);
        sf = Frames{(const char *)fr->I0 + fo, (const char *)fr->I1 + fo, fr->dtype};
    }
    return run_passes(ctx, rows, cols, nb, window, iters, alpha, warm, maybe_f32, u, v, sub,
                      s, batch, fr ? &sf : nullptr, g);
}

int gradients_impl(hsflow_ctx *ctx, const void *I0, const void *I1, int dtype_in,
                   int rows, int cols, int batch, float *gx, float *gy, float *gt,
                   void *workspace, size_t ws_bytes, hipStream_t s) {
    if (!sizes_ok(rows, cols, batch))
        return fail(ctx, HSFLOW_ERR_ARG, "bad size %dx%d batch %d", rows, cols, batch);
    if (!device_dtype_ok(dtype_in))
        return fail(ctx, HSFLOW_ERR_ARG, "device input dtype must be U8, F16, F32 or F64");
    if (!I0 || !I1 || !workspace) return fail(ctx, HSFLOW_ERR_ARG, "null device pointer");
    Workspace w = carve(workspace, rows, cols, batch);
    if (ws_bytes < w.bytes)
        return fail(ctx, HSFLOW_ERR_ARG, "workspace %zu < %zu bytes", ws_bytes, w.bytes);
    // K1 stores 8-bit frames' flags itself (always 0); the others OR into zeros
    if (dtype_in != HSFLOW_U8) HIP_TRY(ctx, hipMemsetAsync(w.flags, 0, (size_t)batch * 4, s));
    // the f32 planes for every pair only when the caller takes them
    hipError_t e = hsflow::launch_gradients(I0, I1, dtype_in, rows, cols, batch, w.gpack,
                                            w.gx, w.gy, w.gt, w.flags, gx || gy || gt, s);
    if (e != hipSuccess) return hip_fail(ctx, e, "gradients launch");
    const size_t n = (size_t)rows * cols * batch;
    if (gx) HIP_TRY(ctx, hipMemcpyAsync(gx, w.gx, n * 4, hipMemcpyDeviceToDevice, s));
    if (gy) HIP_TRY(ctx, hipMemcpyAsync(gy, w.gy, n * 4, hipMemcpyDeviceToDevice, s));
    if (gt) HIP_TRY(ctx, hipMemcpyAsync(gt, w.gt, n * 4, hipMemcpyDeviceToDevice, s));
    return HSFLOW_OK;
}

// A cold solve whose caller takes no gradient planes: K1, then the passes.
// Where the plan is K4 with at least one full-depth pass and the frames are
// u8, f16 or f32, K1 is fused into pass 0 instead (hsflow_strips.hip): the
// fork moves in front of the prologue, and each chain zeroes its own flags,
// runs the fused pass and K1f for its pairs on its side stream, so no kernel
// of a split batch stays on the caller's stream between fork and join.
// Same bits either way ((u, v), the packed plane and the flags).
bool fuse_first(int dtype_in, bool maybe_f32, int rows, int cols, int batch, int window,
                int iters) {
    if (!g_first_fusion) return false;
    if (dtype_in != HSFLOW_U8 && dtype_in != HSFLOW_F16 && dtype_in != HSFLOW_F32) return false;
    if (window < 1 || window > HSFLOW_MAX_WINDOW || !sizes_ok(rows, cols, batch)) return false;
    const PassPlan plan = plan_passes(window, maybe_f32, rows, cols, batch);
    return plan.strip && iters >= plan.kb;
}

int cold_solve(hsflow_ctx *ctx, const void *I0, const void *I1, int dtype_in, int rows,
               int cols, int batch, int window, int iters, float alpha, bool maybe_f32,
               float *u, float *v, void *workspace, size_t ws_bytes, hipStream_t s) {
    if (I0 && I1 && fuse_first(dtype_in, maybe_f32, rows, cols, batch, window, iters)) {
        const Frames fr{I0, I1, dtype_in};
        return jacobi_impl(ctx, rows, cols, batch, window, iters, alpha, false, maybe_f32, u, v,
                           workspace, ws_bytes, s, &fr);
    }
    int rc = gradients_impl(ctx, I0, I1, dtype_in, rows, cols, batch, nullptr, nullptr, nullptr,
                            workspace, ws_bytes, s);
    if (rc) return rc;
    return jacobi_impl(ctx, rows, cols, batch, window, iters, alpha, false, maybe_f32, u, v,
                       workspace, ws_bytes, s);
}

int grow(hsflow_ctx *ctx, void **p, size_t *have, size_t need) {
    if (*have >= need) return HSFLOW_OK;
    if (*p) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx, hipFree(*p));
        *p = nullptr;
        *have = 0;
    }
    HIP_TRY(ctx, hipMalloc(p, need));
    *have = need;
    return HSFLOW_OK;
}

int grow_host(hsflow_ctx *ctx, size_t need) {
    if (ctx->h_stage_bytes >= need) return HSFLOW_OK;
    if (ctx->h_stage) {
        HIP_TRY(ctx, hipHostFree(ctx->h_stage));
        ctx->h_stage = nullptr;
        ctx->h_stage_bytes = 0;
    }
    HIP_TRY(ctx, hipHostMalloc((void **)&ctx->h_stage, need, hipHostMallocDefault));
    ctx->h_stage_bytes = need;
    return HSFLOW_OK;
}

// Two host frames (any supported dtype, any row steps) -> dense device rows
// of the same type (K1 takes the Sobel sums of CV_64FC1 frames in float64,
// as hornSchunck.cpp:23-28 do, and rounds each gradient to f32 once).  The
// runtime's own pageable upload is the fastest route measured
// (hsflow_hostio.cpp).
int upload_pair(hsflow_ctx *ctx, const void *I0, const void *I1, int elem, int rows, int cols,
                size_t step0, size_t step1, void *dst0, void *dst1) {
    const size_t rb = (size_t)cols * elem;
    HIP_TRY(ctx, hipMemcpy2DAsync(dst0, rb, I0, step0, rb, rows, hipMemcpyHostToDevice,
                                  ctx->stream));
    HIP_TRY(ctx, hipMemcpy2DAsync(dst1, rb, I1, step1, rb, rows, hipMemcpyHostToDevice,
                                  ctx->stream));
    return HSFLOW_OK;
}

// n dense device f32 planes -> host rows of dtype_out with step `step`
// (hsflow_hostio.cpp: f32 straight down, f64 through the pinned stage,
// widened by the host pool chunk by chunk as the copies land).
int download_planes(hsflow_ctx *ctx, const float *const *src, void *const *dst, int n,
                    int rows, int cols, int dtype_out, size_t step) {
    const bool f64 = dtype_out == HSFLOW_F64;
    if (f64) {
        int rc = grow_host(ctx, (size_t)n * rows * cols * 4);
        if (rc) return rc;
    }
    HIP_TRY(ctx, hsflow::download_planes_pipelined(src, dst, n, rows, cols, f64, step,
                                                   (float *)ctx->h_stage, ctx->dl_ev,
                                                   ctx->stream));
    return HSFLOW_OK;
}

int check_host_args(hsflow_ctx *ctx, const void *I0, const void *I1, int dtype_in,
                    int rows, int cols, size_t step0, size_t step1, int dtype_out,
                    size_t out_step) {
    if (!ctx) return HSFLOW_ERR_ARG;
    if (!I0 || !I1) return fail(ctx, HSFLOW_ERR_ARG, "null image");
    if (!sizes_ok(rows, cols, 1))
        return fail(ctx, HSFLOW_ERR_ARG, "bad size %dx%d", rows, cols);
    const int es = elem_size(dtype_in);
    if (!es) return fail(ctx, HSFLOW_ERR_ARG, "unsupported input dtype %d", dtype_in);
    if (step0 < (size_t)cols * es || step1 < (size_t)cols * es)
        return fail(ctx, HSFLOW_ERR_ARG, "input steps %zu, %zu < row bytes %zu", step0, step1,
                    (size_t)cols * es);
    if (dtype_out != HSFLOW_F32 && dtype_out != HSFLOW_F64)
        return fail(ctx, HSFLOW_ERR_ARG, "output dtype must be F32 or F64");
    if (out_step < (size_t)cols * elem_size(dtype_out))
        return fail(ctx, HSFLOW_ERR_ARG, "output step %zu < row bytes", out_step);
    return HSFLOW_OK;
}

// ---- config 5 pyramid ----------------------------------------------------
// Workspace: [Jacobi workspace of level 0][integrality flags][per level
// l >= 1: I0_l, I1_l, u_l, v_l (batch x level plane, f32)].  Coarser levels
// reuse the front of the level-0 Jacobi workspace.
struct PyrLayout {
    int levels;
    int R[HSFLOW_MAX_LEVELS], C[HSFLOW_MAX_LEVELS];
    size_t jac_bytes, flags_off;
    size_t off[HSFLOW_MAX_LEVELS][4];  // I0, I1, u, v of level l >= 1
    size_t bytes;
};

PyrLayout pyr_layout(int rows, int cols, int batch, int levels) {
    PyrLayout L{};
    L.levels = levels;
    L.R[0] = rows;
    L.C[0] = cols;
    for (int l = 1; l < levels; ++l) {
        L.R[l] = (L.R[l - 1] + 1) / 2;
        L.C[l] = (L.C[l - 1] + 1) / 2;
    }
    L.jac_bytes = carve(nullptr, rows, cols, batch).bytes;
    L.flags_off = L.jac_bytes;
    size_t off = align_up(L.flags_off + (size_t)batch * 4);
    for (int l = 1; l < levels; ++l) {
        const size_t plane = align_up((size_t)L.R[l] * L.C[l] * batch * 4);
        for (int k = 0; k < 4; ++k) {
            L.off[l][k] = off;
            off += plane;
        }
    }
    L.bytes = off;
    return L;
}

// Arguments of a pyramid solve (plain or warped), checked before any device work.
int check_pyramid_args(hsflow_ctx *ctx, const void *I0, const void *I1, int dtype_in, int rows,
                       int cols, int batch, int levels, const float *u, const float *v,
                       const void *ws, size_t ws_bytes) {
    if (levels < 1 || levels > HSFLOW_MAX_LEVELS)
        return fail(ctx, HSFLOW_ERR_ARG, "levels %d outside [1, %d]", levels,
                    HSFLOW_MAX_LEVELS);
    if (!sizes_ok(rows, cols, batch))
        return fail(ctx, HSFLOW_ERR_ARG, "bad size %dx%d batch %d", rows, cols, batch);
    if (!device_dtype_ok(dtype_in))
        return fail(ctx, HSFLOW_ERR_ARG, "device input dtype must be U8, F16, F32 or F64");
    if (!I0 || !I1 || !u || !v || !ws)
        return fail(ctx, HSFLOW_ERR_ARG, "null device pointer");
    const size_t need = pyr_layout(rows, cols, batch, levels).bytes;
    if (ws_bytes < need)
        return fail(ctx, HSFLOW_ERR_ARG, "workspace %zu < %zu bytes", ws_bytes, need);
    return HSFLOW_OK;
}

// Levels 1..levels-1 of both frames into the workspace (layout L).
int build_levels(hsflow_ctx *ctx, const void *I0, const void *I1, int dtype_in, int rows,
                 int cols, int batch, const PyrLayout &L, void *ws, hipStream_t s) {
    if (L.levels <= 1) return HSFLOW_OK;
    char *base = (char *)ws;
    // integrality of each pair (K1's flag at level 0) decides the rounding
    // of every level; saved because each level's K1 rewrites the flags
    int rc = gradients_impl(ctx, I0, I1, dtype_in, rows, cols, batch, nullptr, nullptr,
                            nullptr, ws, L.jac_bytes, s);
    if (rc) return rc;
    uint32_t *intf = (uint32_t *)(base + L.flags_off);
    HIP_TRY(ctx, hipMemcpyAsync(intf, carve(ws, rows, cols, batch).flags, (size_t)batch * 4,
                                hipMemcpyDeviceToDevice, s));
    for (int l = 1; l < L.levels; ++l)
        for (int k = 0; k < 2; ++k) {
            const void *src = l == 1 ? (k ? I1 : I0) : base + L.off[l - 1][k];
            hipError_t e = hsflow::launch_pyrdown(
                src, l == 1 ? dtype_in : HSFLOW_F32, L.R[l - 1], L.C[l - 1], batch,
                (float *)(base + L.off[l][k]), intf, s);
            if (e != hipSuccess) return hip_fail(ctx, e, "pyrdown launch");
        }
    return HSFLOW_OK;
}

int pyramid_impl(hsflow_ctx *ctx, const void *I0, const void *I1, int dtype_in, int rows,
                 int cols, int batch, int levels, int window, int iters, float alpha,
                 float *u, float *v, void *ws, size_t ws_bytes, hipStream_t s) {
    int rc = check_pyramid_args(ctx, I0, I1, dtype_in, rows, cols, batch, levels, u, v, ws,
                                ws_bytes);
    if (rc) return rc;
    const PyrLayout L = pyr_layout(rows, cols, batch, levels);
    const bool maybe_f32 = dtype_in != HSFLOW_U8;
    char *base = (char *)ws;
    if ((rc = build_levels(ctx, I0, I1, dtype_in, rows, cols, batch, L, ws, s))) return rc;
    for (int l = levels - 1; l >= 0; --l) {
        float *ul = l ? (float *)(base + L.off[l][2]) : u;
        float *vl = l ? (float *)(base + L.off[l][3]) : v;
        const bool warm = l < levels - 1;
        if (warm) {
            hipError_t e = hsflow::launch_upflow(
                (const float *)(base + L.off[l + 1][2]), (const float *)(base + L.off[l + 1][3]),
                L.R[l + 1], L.C[l + 1], ul, vl, L.R[l], L.C[l], batch, s);
            if (e != hipSuccess) return hip_fail(ctx, e, "upflow launch");
        }
        const void *f0 = l ? (const void *)(base + L.off[l][0]) : I0;
        const void *f1 = l ? (const void *)(base + L.off[l][1]) : I1;
        const int fdt = l ? HSFLOW_F32 : dtype_in;
        if (!warm) {  // the coarsest level: a cold solve (K1 may fuse into pass 0)
            rc = cold_solve(ctx, f0, f1, fdt, L.R[l], L.C[l], batch, window, iters, alpha,
                            maybe_f32, ul, vl, ws, L.jac_bytes, s);
            if (rc) return rc;
            continue;
        }
        rc = gradients_impl(ctx, f0, f1, fdt, L.R[l], L.C[l], batch, nullptr, nullptr, nullptr,
                            ws, L.jac_bytes, s);
        if (rc) return rc;
        rc = jacobi_impl(ctx, L.R[l], L.C[l], batch, window, iters, alpha, warm, maybe_f32,
                         ul, vl, ws, L.jac_bytes, s);
        if (rc) return rc;
    }
    return HSFLOW_OK;
}

// ---- warped coarse-to-fine solve -------------------------------------------
// KW: one level's gradients linearised around (u0, v0), into the Jacobi
// workspace's f32 planes (flags[pair] = 1: the passes read the planes).
int warp_gradients_impl(hsflow_ctx *ctx, const void *I0, const void *I1, int dtype_in,
                        int rows, int cols, int batch, const float *u0, const float *v0,
                        float *gx, float *gy, float *gt, void *workspace, size_t ws_bytes,
                        hipStream_t s) {
    if (!sizes_ok(rows, cols, batch))
        return fail(ctx, HSFLOW_ERR_ARG, "bad size %dx%d batch %d", rows, cols, batch);
    if (!device_dtype_ok(dtype_in))
        return fail(ctx, HSFLOW_ERR_ARG, "device input dtype must be U8, F16, F32 or F64");
    if (!I0 || !I1 || !u0 || !v0 || !workspace)
        return fail(ctx, HSFLOW_ERR_ARG, "null device pointer");
    Workspace w = carve(workspace, rows, cols, batch);
    if (ws_bytes < w.bytes)
        return fail(ctx, HSFLOW_ERR_ARG, "workspace %zu < %zu bytes", ws_bytes, w.bytes);
    hipError_t e = hsflow::launch_warp_gradients(I0, I1, dtype_in, rows, cols, batch, u0, v0,
                                                 w.gx, w.gy, w.gt, w.flags, s);
    if (e != hipSuccess) return hip_fail(ctx, e, "warp gradients launch");
    const size_t n = (size_t)rows * cols * batch;
    if (gx) HIP_TRY(ctx, hipMemcpyAsync(gx, w.gx, n * 4, hipMemcpyDeviceToDevice, s));
    if (gy) HIP_TRY(ctx, hipMemcpyAsync(gy, w.gy, n * 4, hipMemcpyDeviceToDevice, s));
    if (gt) HIP_TRY(ctx, hipMemcpyAsync(gt, w.gt, n * 4, hipMemcpyDeviceToDevice, s));
    return HSFLOW_OK;
}

constexpr int kMaxWarps = 16;

int check_warped_args(hsflow_ctx *ctx, int warps, int window, int iters) {
    if (warps < 1 || warps > kMaxWarps)
        return fail(ctx, HSFLOW_ERR_ARG, "warps %d outside [1, %d]", warps, kMaxWarps);
    if (window < 1 || window > HSFLOW_MAX_WINDOW)
        return fail(ctx, HSFLOW_ERR_ARG, "windowSize %d outside [1, %d]", window,
                    HSFLOW_MAX_WINDOW);
    if (iters < 0) return fail(ctx, HSFLOW_ERR_ARG, "maxIterations %d < 0", iters);
    return HSFLOW_OK;
}

// ---- median filtering of the flow between warps ----------------------------
// `median` of the *_median solves: 0 = none, else KM's size
int check_median_arg(hsflow_ctx *ctx, int median) {
    if (median != 0 && median != 3 && median != 5)
        return fail(ctx, HSFLOW_ERR_ARG, "median %d is not 0, 3 or 5", median);
    return HSFLOW_OK;
}

bool ranges_overlap(const float *a, const float *b, size_t n) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + n * 4 && pb < pa + n * 4;
}

int median_impl(hsflow_ctx *ctx, const float *u, const float *v, int rows, int cols, int batch,
                int ksize, float *u_out, float *v_out, hipStream_t s) {
    if (ksize != 3 && ksize != 5)
        return fail(ctx, HSFLOW_ERR_ARG, "median size %d is not 3 or 5", ksize);
    if (!sizes_ok(rows, cols, batch))
        return fail(ctx, HSFLOW_ERR_ARG, "bad size %dx%d batch %d", rows, cols, batch);
    if (!u || !v || !u_out || !v_out) return fail(ctx, HSFLOW_ERR_ARG, "null device pointer");
    const size_t n = (size_t)rows * cols * batch;
    if (ranges_overlap(u_out, u, n) || ranges_overlap(u_out, v, n) ||
        ranges_overlap(v_out, u, n) || ranges_overlap(v_out, v, n) ||
        ranges_overlap(u_out, v_out, n))
        return fail(ctx, HSFLOW_ERR_ARG, "median outputs overlap the inputs or each other");
    hipError_t e = hsflow::launch_median(u, v, rows, cols, batch, ksize, u_out, v_out, s);
    if (e != hipSuccess) return hip_fail(ctx, e, "median launch");
    return HSFLOW_OK;
}

// KM on a level's (u, v) in place: into the Jacobi workspace's second u/v
// planes -- scratch of the passes, idle between solves (run_passes rewrites
// them before it reads them) -- and back with two device copies.
int median_in_place(hsflow_ctx *ctx, float *u, float *v, int rows, int cols, int batch,
                    int ksize, void *ws, hipStream_t s) {
    const Workspace w = carve(ws, rows, cols, batch);
    const size_t n = (size_t)rows * cols * batch;
    hipError_t e = hsflow::launch_median(u, v, rows, cols, batch, ksize, w.u2, w.v2, s);
    if (e != hipSuccess) return hip_fail(ctx, e, "median launch");
    HIP_TRY(ctx, hipMemcpyAsync(u, w.u2, n * 4, hipMemcpyDeviceToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(v, w.v2, n * 4, hipMemcpyDeviceToDevice, s));
    return HSFLOW_OK;
}

// ---- flow-driven smoothness ---------------------------------------------------
bool sm_on(const hsflow_smoothness *sm) { return sm && sm->mode != HSFLOW_SMOOTH_QUADRATIC; }

// a setting that is on: the mode and lambda (negated comparisons: NaN fails)
int check_smoothness(hsflow_ctx *ctx, const hsflow_smoothness *sm) {
    if (sm->mode != HSFLOW_SMOOTH_FLOW_DRIVEN)
        return fail(ctx, HSFLOW_ERR_ARG, "smoothness mode %d is not 0 or 1", sm->mode);
    if (!(sm->lambda > 0.0f && sm->lambda <= 3.0e38f))
        return fail(ctx, HSFLOW_ERR_ARG, "smoothness lambda %g must be finite and > 0",
                    (double)sm->lambda);
    return HSFLOW_OK;
}

// ... and the window of a solve that runs with it: the sizes KJ is built for
int check_smoothness_for(hsflow_ctx *ctx, const hsflow_smoothness *sm, int window) {
    if (!sm_on(sm)) return HSFLOW_OK;
    int rc = check_smoothness(ctx, sm);
    if (rc) return rc;
    if (window != 3 && window != 5)
        return fail(ctx, HSFLOW_ERR_ARG,
                    "flow-driven smoothness needs windowSize 3 or 5, not %d", window);
    return HSFLOW_OK;
}

bool floats_overlap(const float *a, size_t na, const void *b, size_t nb_bytes) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb_bytes && pb < pa + na * 4;
}

// KG alone
int diffusivity_impl(hsflow_ctx *ctx, const float *u, const float *v, int rows, int cols,
                     int batch, float lambda, float *g, hipStream_t s) {
    const hsflow_smoothness sm{HSFLOW_SMOOTH_FLOW_DRIVEN, lambda};
    int rc = check_smoothness(ctx, &sm);
    if (rc) return rc;
    if (!sizes_ok(rows, cols, batch))
        return fail(ctx, HSFLOW_ERR_ARG, "bad size %dx%d batch %d", rows, cols, batch);
    if (!u || !v || !g) return fail(ctx, HSFLOW_ERR_ARG, "null device pointer");
    const size_t n = (size_t)rows * cols * batch;
    if (ranges_overlap(g, u, n) || ranges_overlap(g, v, n))
        return fail(ctx, HSFLOW_ERR_ARG, "the weights overlap the flow");
    hipError_t e = hsflow::launch_diffusivity(u, v, rows, cols, batch, lambda, g, s);
    if (e != hipSuccess) return hip_fail(ctx, e, "diffusivity launch");
    return HSFLOW_OK;
}

// KJ alone: `iters` weighted iterations from the workspace's f32 planes
int jacobi_weighted_impl(hsflow_ctx *ctx, int rows, int cols, int batch, int window, int iters,
                         float alpha, const float *g, float *u, float *v, void *workspace,
                         size_t ws_bytes, hipStream_t s) {
    if (window != 3 && window != 5)
        return fail(ctx, HSFLOW_ERR_ARG, "weighted iterations need windowSize 3 or 5, not %d",
                    window);
    int rc = check_jacobi_args(ctx, rows, cols, batch, window, iters, u, v, workspace, ws_bytes);
    if (rc) return rc;
    if (!g) return fail(ctx, HSFLOW_ERR_ARG, "null device pointer");
    const size_t n = (size_t)rows * cols * batch;
    const size_t wsb = carve(workspace, rows, cols, batch).bytes;
    if (ranges_overlap(g, u, n) || ranges_overlap(g, v, n) || ranges_overlap(u, v, n) ||
        floats_overlap(g, n, workspace, wsb) || floats_overlap(u, n, workspace, wsb) ||
        floats_overlap(v, n, workspace, wsb))
        return fail(ctx, HSFLOW_ERR_ARG,
                    "the weights, the flow and the workspace overlap each other");
    return jacobi_impl(ctx, rows, cols, batch, window, iters, alpha, true, true, u, v, workspace,
                       ws_bytes, s, nullptr, g);
}

// The pyramid of pyramid_impl; per level, coarsest first: (u, v) = 0 or the
// coarser result projected up, then `warps` times KW around the current
// (u, v), `iters` Jacobi iterations warm-started from it and, for median != 0,
// KM (median x median) on the level's (u, v).  median = 0 launches exactly
// what the solve without the filter always has.  With a smoothness mode on,
// KG turns each warp's (u, v) into weights -- in the Jacobi workspace's packed
// gradient plane, which a warped solve never reads (KW sets flags[pair] = 1) --
// and the iterations are KJ's weighted ones; off, the launches are unchanged.
int warped_impl(hsflow_ctx *ctx, const void *I0, const void *I1, int dtype_in, int rows,
                int cols, int batch, int levels, int warps, int median, int window, int iters,
                float alpha, float *u, float *v, void *ws, size_t ws_bytes, hipStream_t s,
                const hsflow_smoothness *sm = nullptr) {
    int rc = check_warped_args(ctx, warps, window, iters);
    if (rc) return rc;
    if ((rc = check_median_arg(ctx, median))) return rc;
    if ((rc = check_smoothness_for(ctx, sm, window))) return rc;
    rc = check_pyramid_args(ctx, I0, I1, dtype_in, rows, cols, batch, levels, u, v, ws,
                            ws_bytes);
    if (rc) return rc;
    const PyrLayout L = pyr_layout(rows, cols, batch, levels);
    char *base = (char *)ws;
    if ((rc = build_levels(ctx, I0, I1, dtype_in, rows, cols, batch, L, ws, s))) return rc;
    for (int l = levels - 1; l >= 0; --l) {
        float *ul = l ? (float *)(base + L.off[l][2]) : u;
        float *vl = l ? (float *)(base + L.off[l][3]) : v;
        const size_t n = (size_t)L.R[l] * L.C[l] * batch;
        if (l == levels - 1) {
            HIP_TRY(ctx, hipMemsetAsync(ul, 0, n * 4, s));
            HIP_TRY(ctx, hipMemsetAsync(vl, 0, n * 4, s));
        } else {
            hipError_t e = hsflow::launch_upflow(
                (const float *)(base + L.off[l + 1][2]), (const float *)(base + L.off[l + 1][3]),
                L.R[l + 1], L.C[l + 1], ul, vl, L.R[l], L.C[l], batch, s);
            if (e != hipSuccess) return hip_fail(ctx, e, "upflow launch");
        }
        for (int k = 0; k < warps; ++k) {
            rc = warp_gradients_impl(ctx, l ? (const void *)(base + L.off[l][0]) : I0,
                                     l ? (const void *)(base + L.off[l][1]) : I1,
                                     l ? HSFLOW_F32 : dtype_in, L.R[l], L.C[l], batch, ul, vl,
                                     nullptr, nullptr, nullptr, ws, L.jac_bytes, s);
            if (rc) return rc;
            float *g = nullptr;
            if (sm_on(sm)) {
                g = (float *)carve(ws, L.R[l], L.C[l], batch).gpack;
                hipError_t e = hsflow::launch_diffusivity(ul, vl, L.R[l], L.C[l], batch,
                                                          sm->lambda, g, s);
                if (e != hipSuccess) return hip_fail(ctx, e, "diffusivity launch");
            }
            // need_f32: the planes are f32 for every pair
            rc = jacobi_impl(ctx, L.R[l], L.C[l], batch, window, iters, alpha, true, true, ul,
                             vl, ws, L.jac_bytes, s, nullptr, g);
            if (rc) return rc;
            if (median) {
                rc = median_in_place(ctx, ul, vl, L.R[l], L.C[l], batch, median, ws, s);
                if (rc) return rc;
            }
        }
    }
    return HSFLOW_OK;
}

// ---- bidirectional warped solve + forward-backward check -------------------
// thresholds of the check: finite and >= 0 (negated, so NaN fails)
int check_thresholds(hsflow_ctx *ctx, float rel, float abs_thr) {
    if (!(rel >= 0.0f && rel <= 3.0e38f) || !(abs_thr >= 0.0f && abs_thr <= 3.0e38f))
        return fail(ctx, HSFLOW_ERR_ARG, "thresholds rel %g, abs %g must be finite and >= 0",
                    (double)rel, (double)abs_thr);
    return HSFLOW_OK;
}

int check_consistency_args(hsflow_ctx *ctx, const float *uf, const float *vf, const float *ub,
                           const float *vb, int rows, int cols, int batch, float rel,
                           float abs_thr) {
    if (!sizes_ok(rows, cols, batch))
        return fail(ctx, HSFLOW_ERR_ARG, "bad size %dx%d batch %d", rows, cols, batch);
    if (!uf || !vf || !ub || !vb) return fail(ctx, HSFLOW_ERR_ARG, "null device pointer");
    return check_thresholds(ctx, rel, abs_thr);
}

// KC on checked arguments: counts zeroed stream-ordered, then one launch
int consistency_run(hsflow_ctx *ctx, const float *uf, const float *vf, const float *ub,
                    const float *vb, int rows, int cols, int batch, float rel, float abs_thr,
                    float *err, uint8_t *mask, uint32_t *counts, hipStream_t s) {
    if (counts) HIP_TRY(ctx, hipMemsetAsync(counts, 0, (size_t)batch * 3 * 4, s));
    hipError_t e = hsflow::launch_consistency(uf, vf, ub, vb, rows, cols, batch, rel, abs_thr,
                                              err, mask, counts, s);
    if (e != hipSuccess) return hip_fail(ctx, e, "consistency launch");
    return HSFLOW_OK;
}

int consistency_impl(hsflow_ctx *ctx, const float *uf, const float *vf, const float *ub,
                     const float *vb, int rows, int cols, int batch, float rel, float abs_thr,
                     float *err, uint8_t *mask, uint32_t *counts, hipStream_t s) {
    int rc = check_consistency_args(ctx, uf, vf, ub, vb, rows, cols, batch, rel, abs_thr);
    if (rc) return rc;
    if (!err && !mask && !counts)
        return fail(ctx, HSFLOW_ERR_ARG, "no output: err, mask and counts are all null");
    return consistency_run(ctx, uf, vf, ub, vb, rows, cols, batch, rel, abs_thr, err, mask,
                           counts, s);
}

// Both directions one after the other on the caller's stream, each the
// warped solve itself (so the flows are hsflow_flow_warped_device's bits by
// construction) in the one pyramid workspace, then KC per direction asked for.
int bidir_impl(hsflow_ctx *ctx, const void *I0, const void *I1, int dtype_in, int rows,
               int cols, int batch, int levels, int warps, int median, int window, int iters,
               float alpha,
               float rel, float abs_thr, float *uf, float *vf, float *ub, float *vb,
               float *err_f, uint8_t *mask_f, uint32_t *counts_f, float *err_b,
               uint8_t *mask_b, uint32_t *counts_b, void *ws, size_t ws_bytes, hipStream_t s,
               const hsflow_smoothness *sm = nullptr) {
    int rc = check_warped_args(ctx, warps, window, iters);
    if (rc) return rc;
    if ((rc = check_median_arg(ctx, median))) return rc;
    if ((rc = check_smoothness_for(ctx, sm, window))) return rc;
    rc = check_pyramid_args(ctx, I0, I1, dtype_in, rows, cols, batch, levels, uf, vf, ws,
                            ws_bytes);
    if (rc) return rc;
    if (!ub || !vb) return fail(ctx, HSFLOW_ERR_ARG, "null device pointer");
    if ((rc = check_thresholds(ctx, rel, abs_thr))) return rc;
    rc = warped_impl(ctx, I0, I1, dtype_in, rows, cols, batch, levels, warps, median, window,
                     iters, alpha, uf, vf, ws, ws_bytes, s, sm);
    if (rc) return rc;
    rc = warped_impl(ctx, I1, I0, dtype_in, rows, cols, batch, levels, warps, median, window,
                     iters, alpha, ub, vb, ws, ws_bytes, s, sm);
    if (rc) return rc;
    if (err_f || mask_f || counts_f) {
        rc = consistency_run(ctx, uf, vf, ub, vb, rows, cols, batch, rel, abs_thr, err_f,
                             mask_f, counts_f, s);
        if (rc) return rc;
    }
    if (err_b || mask_b || counts_b)
        rc = consistency_run(ctx, ub, vb, uf, vf, rows, cols, batch, rel, abs_thr, err_b,
                             mask_b, counts_b, s);
    return rc;
}

// ---- brightness-robust prefilter --------------------------------------------
// A checked hsflow_prefilter: the radius and the Gaussian's weights w[0..radius],
// normalised to sum 1 (w[0] + 2 sum w[i]) in double and rounded to f32 once.
struct PfPlan {
    int mode, radius;
    float w[HSFLOW_PREFILTER_MAX_RADIUS + 1];
    float eps, scale;
};

bool pf_on(const hsflow_prefilter *pf) { return pf && pf->mode != 0; }

int plan_prefilter(hsflow_ctx *ctx, const hsflow_prefilter *pf, PfPlan *P) {
    if (!pf) return fail(ctx, HSFLOW_ERR_ARG, "null prefilter");
    if (pf->mode != HSFLOW_PREFILTER_HIGHPASS && pf->mode != HSFLOW_PREFILTER_NORMALIZE)
        return fail(ctx, HSFLOW_ERR_ARG, "prefilter mode %d is not 1 or 2", pf->mode);
    // negated comparisons: NaN fails
    if (!(pf->sigma >= 0.5f && pf->sigma <= 5.0f))
        return fail(ctx, HSFLOW_ERR_ARG, "prefilter sigma %g outside [0.5, 5]", (double)pf->sigma);
    if (!(pf->eps > 0.0f && pf->eps <= 3.0e38f))
        return fail(ctx, HSFLOW_ERR_ARG, "prefilter eps %g must be finite and > 0",
                    (double)pf->eps);
    if (!(pf->scale > 0.0f && pf->scale <= 3.0e38f))
        return fail(ctx, HSFLOW_ERR_ARG, "prefilter scale %g must be finite and > 0",
                    (double)pf->scale);
    const double sigma = (double)pf->sigma;
    P->mode = pf->mode;
    P->radius = std::min((int)std::ceil(3.0 * sigma), HSFLOW_PREFILTER_MAX_RADIUS);
    P->eps = pf->eps;
    P->scale = pf->scale;
    double w[HSFLOW_PREFILTER_MAX_RADIUS + 1], sum = 0.0;
    for (int i = 0; i <= P->radius; ++i) {
        w[i] = std::exp(-(double)(i * i) / (2.0 * sigma * sigma));
        sum += i ? 2.0 * w[i] : w[i];
    }
    for (int i = 0; i <= HSFLOW_PREFILTER_MAX_RADIUS; ++i)
        P->w[i] = i <= P->radius ? (float)(w[i] / sum) : 0.0f;
    return HSFLOW_OK;
}

// the two f32 planes the *_pf solves prefilter the frames into
size_t pf_planes_bytes(int rows, int cols, int batch) {
    return 2 * align_up((size_t)rows * cols * batch * 4);
}

int prefilter_run(hsflow_ctx *ctx, const void *I, int dtype_in, int rows, int cols, int batch,
                  const PfPlan &P, float *out, hipStream_t s) {
    hipError_t e = hsflow::launch_prefilter(I, dtype_in, rows, cols, batch, P.mode, P.radius, P.w,
                                            P.eps, P.scale, out, s);
    if (e != hipSuccess) return hip_fail(ctx, e, "prefilter launch");
    return HSFLOW_OK;
}

int prefilter_impl(hsflow_ctx *ctx, const void *I, int dtype_in, int rows, int cols, int batch,
                   const hsflow_prefilter *pf, float *out, hipStream_t s) {
    PfPlan P;
    int rc = plan_prefilter(ctx, pf, &P);
    if (rc) return rc;
    if (!sizes_ok(rows, cols, batch))
        return fail(ctx, HSFLOW_ERR_ARG, "bad size %dx%d batch %d", rows, cols, batch);
    if (!device_dtype_ok(dtype_in))
        return fail(ctx, HSFLOW_ERR_ARG, "device input dtype must be U8, F16, F32 or F64");
    if (!I || !out) return fail(ctx, HSFLOW_ERR_ARG, "null device pointer");
    const size_t n = (size_t)rows * cols * batch;
    const uintptr_t pi = (uintptr_t)I, po = (uintptr_t)out;
    if (pi < po + n * 4 && po < pi + n * elem_size(dtype_in))
        return fail(ctx, HSFLOW_ERR_ARG, "prefilter output overlaps the input");
    return prefilter_run(ctx, I, dtype_in, rows, cols, batch, P, out, s);
}

// What a *_pf solve does in front of the call it extends, whose own workspace
// is the first `solve_bytes` (256-aligned) of `ws`: the checks, then KN on both
// frames into the two planes behind it.  The caller has checked sizes, dtype
// and the pointers.
int prefilter_pair(hsflow_ctx *ctx, const void *I0, const void *I1, int dtype_in, int rows,
                   int cols, int batch, const PfPlan &P, void *ws, size_t solve_bytes,
                   float **p0, float **p1, hipStream_t s) {
    const size_t n = (size_t)rows * cols * batch;
    *p0 = (float *)((char *)ws + solve_bytes);
    *p1 = (float *)((char *)ws + solve_bytes + align_up(n * 4));
    int rc = prefilter_run(ctx, I0, dtype_in, rows, cols, batch, P, *p0, s);
    if (rc) return rc;
    return prefilter_run(ctx, I1, dtype_in, rows, cols, batch, P, *p1, s);
}

// the frames of a *_pf solve must not share a byte with its workspace: the
// planes are written while the frames are still to be read
int check_pf_workspace(hsflow_ctx *ctx, const void *I0, const void *I1, size_t frame_bytes,
                       const void *ws, size_t ws_bytes, size_t need) {
    if (ws_bytes < need)
        return fail(ctx, HSFLOW_ERR_ARG, "workspace %zu < %zu bytes", ws_bytes, need);
    const uintptr_t w = (uintptr_t)ws;
    for (const void *I : {I0, I1}) {
        const uintptr_t p = (uintptr_t)I;
        if (p < w + need && w < p + frame_bytes)
            return fail(ctx, HSFLOW_ERR_ARG, "the frames overlap the workspace");
    }
    return HSFLOW_OK;
}

// hsflow_flow_warped_pf_device: KN on both frames, then warped_impl on the planes
// as f32 frames (not integer-valued, so the pyramid does not round them) -- the
// public pieces one after the other, so the bits are theirs by construction.
// No prefilter: warped_impl itself.
int warped_pf_impl(hsflow_ctx *ctx, const void *I0, const void *I1, int dtype_in, int rows,
                   int cols, int batch, int levels, int warps, int median, int window, int iters,
                   float alpha, float *u, float *v, const hsflow_prefilter *pf, void *ws,
                   size_t ws_bytes, hipStream_t s, const hsflow_smoothness *sm = nullptr) {
    if (!pf_on(pf))
        return warped_impl(ctx, I0, I1, dtype_in, rows, cols, batch, levels, warps, median, window,
                           iters, alpha, u, v, ws, ws_bytes, s, sm);
    PfPlan P;
    int rc = plan_prefilter(ctx, pf, &P);
    if (rc) return rc;
    if ((rc = check_warped_args(ctx, warps, window, iters))) return rc;
    if ((rc = check_median_arg(ctx, median))) return rc;
    if ((rc = check_smoothness_for(ctx, sm, window))) return rc;
    rc = check_pyramid_args(ctx, I0, I1, dtype_in, rows, cols, batch, levels, u, v, ws, ws_bytes);
    if (rc) return rc;
    const size_t solve = align_up(pyr_layout(rows, cols, batch, levels).bytes);
    rc = check_pf_workspace(ctx, I0, I1, (size_t)rows * cols * batch * elem_size(dtype_in), ws,
                            ws_bytes, solve + pf_planes_bytes(rows, cols, batch));
    if (rc) return rc;
    float *p0, *p1;
    rc = prefilter_pair(ctx, I0, I1, dtype_in, rows, cols, batch, P, ws, solve, &p0, &p1, s);
    if (rc) return rc;
    return warped_impl(ctx, p0, p1, HSFLOW_F32, rows, cols, batch, levels, warps, median, window,
                       iters, alpha, u, v, ws, solve, s, sm);
}

// hsflow_flow_bidir_pf_device: likewise in front of bidir_impl
int bidir_pf_impl(hsflow_ctx *ctx, const void *I0, const void *I1, int dtype_in, int rows,
                  int cols, int batch, int levels, int warps, int median, int window, int iters,
                  float alpha, float rel, float abs_thr, float *uf, float *vf, float *ub,
                  float *vb, float *err_f, uint8_t *mask_f, uint32_t *counts_f, float *err_b,
                  uint8_t *mask_b, uint32_t *counts_b, const hsflow_prefilter *pf, void *ws,
                  size_t ws_bytes, hipStream_t s, const hsflow_smoothness *sm = nullptr) {
    if (!pf_on(pf))
        return bidir_impl(ctx, I0, I1, dtype_in, rows, cols, batch, levels, warps, median, window,
                          iters, alpha, rel, abs_thr, uf, vf, ub, vb, err_f, mask_f, counts_f,
                          err_b, mask_b, counts_b, ws, ws_bytes, s, sm);
    PfPlan P;
    int rc = plan_prefilter(ctx, pf, &P);
    if (rc) return rc;
    if ((rc = check_warped_args(ctx, warps, window, iters))) return rc;
    if ((rc = check_median_arg(ctx, median))) return rc;
    if ((rc = check_smoothness_for(ctx, sm, window))) return rc;
    rc = check_pyramid_args(ctx, I0, I1, dtype_in, rows, cols, batch, levels, uf, vf, ws,
                            ws_bytes);
    if (rc) return rc;
    if (!ub || !vb) return fail(ctx, HSFLOW_ERR_ARG, "null device pointer");
    if ((rc = check_thresholds(ctx, rel, abs_thr))) return rc;
    const size_t solve = align_up(pyr_layout(rows, cols, batch, levels).bytes);
    rc = check_pf_workspace(ctx, I0, I1, (size_t)rows * cols * batch * elem_size(dtype_in), ws,
                            ws_bytes, solve + pf_planes_bytes(rows, cols, batch));
    if (rc) return rc;
    float *p0, *p1;
    rc = prefilter_pair(ctx, I0, I1, dtype_in, rows, cols, batch, P, ws, solve, &p0, &p1, s);
    if (rc) return rc;
    return bidir_impl(ctx, p0, p1, HSFLOW_F32, rows, cols, batch, levels, warps, median, window,
                      iters, alpha, rel, abs_thr, uf, vf, ub, vb, err_f, mask_f, counts_f, err_b,
                      mask_b, counts_b, ws, solve, s, sm);
}

// The host-buffer form of both pyramid solves: warps = 0 is hsflow_flow_pyramid,
// warps >= 1 hsflow_flow_warped[_median] (same upload, download, f64 widening
// and huge-page advice).
int pyramid_host(hsflow_ctx *ctx, const void *I0, const void *I1, int dtype_in, int rows,
                 int cols, size_t in_step0, size_t in_step1, int levels, int warps, int median,
                 int window, int iters, double alpha, void *u, void *v, int dtype_out,
                 size_t out_step) {
    int rc = check_host_args(ctx, I0, I1, dtype_in, rows, cols, in_step0, in_step1,
                             dtype_out, out_step);
    if (rc) return rc;
    if (!u || !v) return fail(ctx, HSFLOW_ERR_ARG, "null output");
    if (levels < 1 || levels > HSFLOW_MAX_LEVELS)
        return fail(ctx, HSFLOW_ERR_ARG, "levels %d outside [1, %d]", levels,
                    HSFLOW_MAX_LEVELS);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)rows * cols;
    const size_t in_es = (size_t)dev_elem_size(dtype_in);
    if ((rc = grow(ctx, &ctx->d_in, &ctx->d_in_bytes, align_up(n * in_es) * 2))) return rc;
    if ((rc = grow(ctx, &ctx->d_out, &ctx->d_out_bytes, align_up(n * 4) * 3))) return rc;
    // the warped solves honour the context's prefilter (its planes lie behind
    // the solve's workspace); hsflow_flow_pyramid keeps the reference's semantics
    const bool pf = warps && pf_on(&ctx->pf);
    const size_t wsb = hsflow_pyramid_workspace_bytes(rows, cols, 1, levels) +
                       (pf ? pf_planes_bytes(rows, cols, 1) : 0);
    if ((rc = grow(ctx, &ctx->d_ws, &ctx->d_ws_bytes, wsb))) return rc;
    char *in0 = (char *)ctx->d_in, *in1 = in0 + align_up(n * in_es);
    float *du = (float *)ctx->d_out, *dv = (float *)((char *)du + align_up(n * 4));
    if ((rc = upload_pair(ctx, I0, I1, (int)in_es, rows, cols, in_step0, in_step1, in0, in1)))
        return rc;
    const int dt0 = dtype_in;
    rc = warps ? warped_pf_impl(ctx, in0, in1, dt0, rows, cols, 1, levels, warps, median, window,
                                iters, (float)alpha, du, dv, &ctx->pf, ctx->d_ws,
                                ctx->d_ws_bytes, ctx->stream, &ctx->sm)
               : pyramid_impl(ctx, in0, in1, dt0, rows, cols, 1, levels, window, iters,
                              (float)alpha, du, dv, ctx->d_ws, ctx->d_ws_bytes, ctx->stream);
    if (rc) return rc;
    {
        const float *srcs[2] = {du, dv};
        void *dsts[2] = {u, v};
        if ((rc = download_planes(ctx, srcs, dsts, 2, rows, cols, dtype_out, out_step)))
            return rc;
    }
    return HSFLOW_OK;
}

// The host-buffer form of the bidirectional solve: pyramid_host's upload and
// download around bidir_impl; the masks and counts come down on the same
// stream ahead of the flows, whose download drains it.
int bidir_host(hsflow_ctx *ctx, const void *I0, const void *I1, int dtype_in, int rows,
               int cols, size_t in_step0, size_t in_step1, int levels, int warps, int median,
               int window, int iters, double alpha, float rel, float abs_thr, void *u, void *v,
               void *ub, void *vb, int dtype_out, size_t out_step, uint8_t *mask_f,
               uint8_t *mask_b, size_t mask_step, uint32_t *counts) {
    int rc = check_host_args(ctx, I0, I1, dtype_in, rows, cols, in_step0, in_step1,
                             dtype_out, out_step);
    if (rc) return rc;
    if (!u || !v) return fail(ctx, HSFLOW_ERR_ARG, "null output");
    if (levels < 1 || levels > HSFLOW_MAX_LEVELS)
        return fail(ctx, HSFLOW_ERR_ARG, "levels %d outside [1, %d]", levels,
                    HSFLOW_MAX_LEVELS);
    if ((rc = check_warped_args(ctx, warps, window, iters))) return rc;
    if ((rc = check_median_arg(ctx, median))) return rc;
    if ((rc = check_thresholds(ctx, rel, abs_thr))) return rc;
    if ((mask_f || mask_b) && mask_step < (size_t)cols)
        return fail(ctx, HSFLOW_ERR_ARG, "mask step %zu < row bytes %d", mask_step, cols);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)rows * cols;
    const size_t in_es = (size_t)dev_elem_size(dtype_in);
    // d_out: uf, vf, ub, vb (f32), the two masks (u8), counts (2 x 3 words)
    const size_t fb = align_up(n * 4), mb = align_up(n);
    if ((rc = grow(ctx, &ctx->d_in, &ctx->d_in_bytes, align_up(n * in_es) * 2))) return rc;
    if ((rc = grow(ctx, &ctx->d_out, &ctx->d_out_bytes, fb * 4 + mb * 2 + kAlign))) return rc;
    const size_t wsb = hsflow_pyramid_workspace_bytes(rows, cols, 1, levels) +
                       (pf_on(&ctx->pf) ? pf_planes_bytes(rows, cols, 1) : 0);
    if ((rc = grow(ctx, &ctx->d_ws, &ctx->d_ws_bytes, wsb))) return rc;
    char *in0 = (char *)ctx->d_in, *in1 = in0 + align_up(n * in_es);
    char *out = (char *)ctx->d_out;
    float *d[4] = {(float *)out, (float *)(out + fb), (float *)(out + 2 * fb),
                   (float *)(out + 3 * fb)};
    uint8_t *dmf = (uint8_t *)(out + 4 * fb), *dmb = dmf + mb;
    uint32_t *dc = (uint32_t *)(dmb + mb);
    if ((rc = upload_pair(ctx, I0, I1, (int)in_es, rows, cols, in_step0, in_step1, in0, in1)))
        return rc;
    rc = bidir_pf_impl(ctx, in0, in1, dtype_in, rows, cols, 1, levels, warps, median, window,
                       iters, (float)alpha, rel, abs_thr, d[0], d[1], d[2], d[3], nullptr,
                       mask_f ? dmf : nullptr, counts ? dc : nullptr, nullptr,
                       mask_b ? dmb : nullptr, counts ? dc + 3 : nullptr, &ctx->pf, ctx->d_ws,
                       ctx->d_ws_bytes, ctx->stream, &ctx->sm);
    if (rc) return rc;
    if (mask_f)
        HIP_TRY(ctx, hipMemcpy2DAsync(mask_f, mask_step, dmf, (size_t)cols, (size_t)cols, rows,
                                      hipMemcpyDeviceToHost, ctx->stream));
    if (mask_b)
        HIP_TRY(ctx, hipMemcpy2DAsync(mask_b, mask_step, dmb, (size_t)cols, (size_t)cols, rows,
                                      hipMemcpyDeviceToHost, ctx->stream));
    if (counts)
        HIP_TRY(ctx, hipMemcpyAsync(counts, dc, 6 * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                    ctx->stream));
    const float *srcs[4] = {d[0], d[1], nullptr, nullptr};
    void *dsts[4] = {u, v, nullptr, nullptr};
    int np = 2;
    if (ub) srcs[np] = d[2], dsts[np++] = ub;
    if (vb) srcs[np] = d[3], dsts[np++] = vb;
    return download_planes(ctx, srcs, dsts, np, rows, cols, dtype_out, out_step);
}

// ---- frame warp and frame interpolation ------------------------------------
// byte ranges [a, a + na) and [b, b + nb) share a byte (a null range: none)
bool bytes_overlap(const void *a, size_t na, const void *b, size_t nb) {
    if (!a || !b) return false;
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

struct ByteRange {
    const void *p;
    size_t n;
};

// no output shares a byte with an input or with another output
bool outputs_disjoint(const ByteRange *in, int n_in, const ByteRange *out, int n_out) {
    for (int o = 0; o < n_out; ++o) {
        for (int i = 0; i < n_in; ++i)
            if (bytes_overlap(out[o].p, out[o].n, in[i].p, in[i].n)) return false;
        for (int q = o + 1; q < n_out; ++q)
            if (bytes_overlap(out[o].p, out[o].n, out[q].p, out[q].n)) return false;
    }
    return true;
}

int warp_image_impl(hsflow_ctx *ctx, const void *I, int dtype_in, int rows, int cols, int batch,
                    const float *u, const float *v, float *out, uint8_t *oof, hipStream_t s) {
    if (!sizes_ok(rows, cols, batch))
        return fail(ctx, HSFLOW_ERR_ARG, "bad size %dx%d batch %d", rows, cols, batch);
    if (!device_dtype_ok(dtype_in))
        return fail(ctx, HSFLOW_ERR_ARG, "device input dtype must be U8, F16, F32 or F64");
    if (!I || !u || !v || !out) return fail(ctx, HSFLOW_ERR_ARG, "null device pointer");
    const size_t n = (size_t)rows * cols * batch;
    const ByteRange in[3] = {{I, n * elem_size(dtype_in)}, {u, n * 4}, {v, n * 4}};
    const ByteRange outs[2] = {{out, n * 4}, {oof, n}};
    if (!outputs_disjoint(in, 3, outs, 2))
        return fail(ctx, HSFLOW_ERR_ARG, "warp outputs overlap the inputs or each other");
    hipError_t e = hsflow::launch_warp_image(I, dtype_in, rows, cols, batch, u, v, out, oof, s);
    if (e != hipSuccess) return hip_fail(ctx, e, "warp image launch");
    return HSFLOW_OK;
}

// times (host), nt and the output type of an interpolation
int check_interp_args(hsflow_ctx *ctx, const float *times, int nt, int dtype_out, bool host) {
    if (nt < 1 || nt > HSFLOW_MAX_TIMES)
        return fail(ctx, HSFLOW_ERR_ARG, "nt %d outside [1, %d]", nt, HSFLOW_MAX_TIMES);
    if (!times) return fail(ctx, HSFLOW_ERR_ARG, "null times");
    for (int k = 0; k < nt; ++k)
        if (!(times[k] >= 0.0f && times[k] <= 1.0f))  // negated: NaN fails
            return fail(ctx, HSFLOW_ERR_ARG, "time %d (%g) outside [0, 1]", k, (double)times[k]);
    if (dtype_out != HSFLOW_F32 && dtype_out != HSFLOW_U8 && !(host && dtype_out == HSFLOW_F64))
        return fail(ctx, HSFLOW_ERR_ARG, host ? "output dtype must be U8, F32 or F64"
                                              : "device output dtype must be U8 or F32");
    return HSFLOW_OK;
}

// KI on checked arguments: trusted zeroed stream-ordered, then one launch
int frame_interp_run(hsflow_ctx *ctx, const void *I0, const void *I1, int dtype_in, int rows,
                     int cols, int batch, const float *uf, const float *vf, const float *ub,
                     const float *vb, const uint8_t *mask_f, const uint8_t *mask_b,
                     const float *times, int nt, void *out, int dtype_out, uint8_t *flags,
                     uint32_t *trusted, hipStream_t s) {
    if (trusted) HIP_TRY(ctx, hipMemsetAsync(trusted, 0, (size_t)batch * nt * 4, s));
    hipError_t e = hsflow::launch_frame_interp(I0, I1, dtype_in, rows, cols, batch, uf, vf, ub, vb,
                                               mask_f, mask_b, times, nt, out,
                                               dtype_out == HSFLOW_U8, flags, trusted, s);
    if (e != hipSuccess) return hip_fail(ctx, e, "frame interpolation launch");
    return HSFLOW_OK;
}

int frame_interp_impl(hsflow_ctx *ctx, const void *I0, const void *I1, int dtype_in, int rows,
                      int cols, int batch, const float *uf, const float *vf, const float *ub,
                      const float *vb, const uint8_t *mask_f, const uint8_t *mask_b,
                      const float *times, int nt, void *out, int dtype_out, uint8_t *flags,
                      uint32_t *trusted, hipStream_t s) {
    if (!sizes_ok(rows, cols, batch))
        return fail(ctx, HSFLOW_ERR_ARG, "bad size %dx%d batch %d", rows, cols, batch);
    if (!device_dtype_ok(dtype_in))
        return fail(ctx, HSFLOW_ERR_ARG, "device input dtype must be U8, F16, F32 or F64");
    if (!I0 || !I1 || !uf || !vf || !ub || !vb || !out)
        return fail(ctx, HSFLOW_ERR_ARG, "null device pointer");
    int rc = check_interp_args(ctx, times, nt, dtype_out, false);
    if (rc) return rc;
    const size_t n = (size_t)rows * cols * batch, fb = n * elem_size(dtype_in);
    const ByteRange in[8] = {{I0, fb},    {I1, fb},    {uf, n * 4},  {vf, n * 4},
                             {ub, n * 4}, {vb, n * 4}, {mask_f, n}, {mask_b, n}};
    const ByteRange outs[3] = {{out, n * nt * elem_size(dtype_out)},
                               {flags, n * nt},
                               {trusted, (size_t)batch * nt * 4}};
    if (!outputs_disjoint(in, 8, outs, 3))
        return fail(ctx, HSFLOW_ERR_ARG,
                    "interpolation outputs overlap the inputs or each other");
    return frame_interp_run(ctx, I0, I1, dtype_in, rows, cols, batch, uf, vf, ub, vb, mask_f,
                            mask_b, times, nt, out, dtype_out, flags, trusted, s);
}

// Workspace of the fused call: [the bidirectional solve's][uf][vf][ub][vb]
// (f32 batch planes)[mask_f][mask_b] (u8 batch planes), each 256-byte aligned.
struct InterpLayout {
    size_t solve_bytes, flow[4], mask[2], bytes;
};

InterpLayout interp_layout(int rows, int cols, int batch, int levels) {
    InterpLayout L{};
    const size_t n = (size_t)rows * cols * batch;
    L.solve_bytes = align_up(pyr_layout(rows, cols, batch, levels).bytes);
    size_t off = L.solve_bytes;
    for (int k = 0; k < 4; ++k) L.flow[k] = off, off += align_up(n * 4);
    for (int k = 0; k < 2; ++k) L.mask[k] = off, off += align_up(n);
    L.bytes = off;
    return L;
}

// hsflow_flow_bidir_median_device into the workspace's planes (the masks only
// when flags or trusted needs them), then KI: the two public calls one after
// the other, so the bits are theirs by construction.  With a prefilter (the
// _pf entry point, or the context's setting) the solve runs on the two
// prefiltered f32 planes behind that layout; KI samples the frames themselves.
int flow_interp_impl(hsflow_ctx *ctx, const void *I0, const void *I1, int dtype_in, int rows,
                     int cols, int batch, int levels, int warps, int median, int window,
                     int iters, float alpha, float rel, float abs_thr, const float *times, int nt,
                     void *out, int dtype_out, uint8_t *flags, uint32_t *trusted,
                     const hsflow_prefilter *pf, void *ws, size_t ws_bytes, hipStream_t s,
                     const hsflow_smoothness *sm = nullptr) {
    PfPlan P;
    int rc = pf_on(pf) ? plan_prefilter(ctx, pf, &P) : HSFLOW_OK;
    if (rc) return rc;
    if ((rc = check_warped_args(ctx, warps, window, iters))) return rc;
    if ((rc = check_median_arg(ctx, median))) return rc;
    if ((rc = check_smoothness_for(ctx, sm, window))) return rc;
    if (levels < 1 || levels > HSFLOW_MAX_LEVELS)
        return fail(ctx, HSFLOW_ERR_ARG, "levels %d outside [1, %d]", levels,
                    HSFLOW_MAX_LEVELS);
    if (!sizes_ok(rows, cols, batch))
        return fail(ctx, HSFLOW_ERR_ARG, "bad size %dx%d batch %d", rows, cols, batch);
    if (!device_dtype_ok(dtype_in))
        return fail(ctx, HSFLOW_ERR_ARG, "device input dtype must be U8, F16, F32 or F64");
    if (!I0 || !I1 || !out || !ws) return fail(ctx, HSFLOW_ERR_ARG, "null device pointer");
    if ((rc = check_thresholds(ctx, rel, abs_thr))) return rc;
    if ((rc = check_interp_args(ctx, times, nt, dtype_out, false))) return rc;
    const InterpLayout L = interp_layout(rows, cols, batch, levels);
    const size_t need = L.bytes + (pf_on(pf) ? pf_planes_bytes(rows, cols, batch) : 0);
    if (ws_bytes < need)
        return fail(ctx, HSFLOW_ERR_ARG, "workspace %zu < %zu bytes", ws_bytes, need);
    const size_t n = (size_t)rows * cols * batch, fb = n * elem_size(dtype_in);
    const ByteRange in[3] = {{I0, fb}, {I1, fb}, {ws, need}};
    const ByteRange outs[3] = {{out, n * nt * elem_size(dtype_out)},
                               {flags, n * nt},
                               {trusted, (size_t)batch * nt * 4}};
    if (!outputs_disjoint(in, 3, outs, 3))
        return fail(ctx, HSFLOW_ERR_ARG,
                    "interpolation outputs overlap the frames, the workspace or each other");
    if (pf_on(pf) && (rc = check_pf_workspace(ctx, I0, I1, fb, ws, ws_bytes, need))) return rc;
    char *base = (char *)ws;
    float *f[4];
    for (int k = 0; k < 4; ++k) f[k] = (float *)(base + L.flow[k]);
    const bool masks = flags || trusted;
    uint8_t *mf = masks ? (uint8_t *)(base + L.mask[0]) : nullptr;
    uint8_t *mb = masks ? (uint8_t *)(base + L.mask[1]) : nullptr;
    // the frames the solve sees: the prefiltered planes, or the frames themselves
    const void *S0 = I0, *S1 = I1;
    int dtype_solve = dtype_in;
    if (pf_on(pf)) {
        float *p0, *p1;
        rc = prefilter_pair(ctx, I0, I1, dtype_in, rows, cols, batch, P, ws, L.bytes, &p0, &p1, s);
        if (rc) return rc;
        S0 = p0, S1 = p1, dtype_solve = HSFLOW_F32;
    }
    rc = bidir_impl(ctx, S0, S1, dtype_solve, rows, cols, batch, levels, warps, median, window,
                    iters, alpha, rel, abs_thr, f[0], f[1], f[2], f[3], nullptr, mf, nullptr,
                    nullptr, mb, nullptr, ws, L.solve_bytes, s, sm);
    if (rc) return rc;
    return frame_interp_run(ctx, I0, I1, dtype_in, rows, cols, batch, f[0], f[1], f[2], f[3], mf,
                            mb, times, nt, out, dtype_out, flags, trusted, s);
}

// The host-buffer form: bidir_host's upload, flow_interp_impl on the context's
// buffers, then flags and trusted down on the same stream ahead of the frames,
// whose download drains it.
int flow_interp_host(hsflow_ctx *ctx, const void *I0, const void *I1, int dtype_in, int rows,
                     int cols, size_t in_step0, size_t in_step1, int levels, int warps,
                     int median, int window, int iters, double alpha, float rel, float abs_thr,
                     const float *times, int nt, void *const *out, int dtype_out,
                     size_t out_step, uint8_t *const *flags, size_t flags_step,
                     uint32_t *trusted) {
    if (!ctx) return HSFLOW_ERR_ARG;
    int rc = check_interp_args(ctx, times, nt, dtype_out, true);
    if (rc) return rc;
    // the frames, sizes and input steps (the output type is checked above)
    rc = check_host_args(ctx, I0, I1, dtype_in, rows, cols, in_step0, in_step1, HSFLOW_F32,
                         (size_t)cols * 4);
    if (rc) return rc;
    if (out_step < (size_t)cols * elem_size(dtype_out))
        return fail(ctx, HSFLOW_ERR_ARG, "output step %zu < row bytes", out_step);
    if (!out) return fail(ctx, HSFLOW_ERR_ARG, "null output");
    for (int k = 0; k < nt; ++k)
        if (!out[k] || (flags && !flags[k]))
            return fail(ctx, HSFLOW_ERR_ARG, "null output plane %d", k);
    if (flags && flags_step < (size_t)cols)
        return fail(ctx, HSFLOW_ERR_ARG, "flags step %zu < row bytes %d", flags_step, cols);
    if (levels < 1 || levels > HSFLOW_MAX_LEVELS)
        return fail(ctx, HSFLOW_ERR_ARG, "levels %d outside [1, %d]", levels,
                    HSFLOW_MAX_LEVELS);
    if ((rc = check_warped_args(ctx, warps, window, iters))) return rc;
    if ((rc = check_median_arg(ctx, median))) return rc;
    if ((rc = check_thresholds(ctx, rel, abs_thr))) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)rows * cols;
    const size_t in_es = (size_t)dev_elem_size(dtype_in);
    const int dev_out = dtype_out == HSFLOW_U8 ? HSFLOW_U8 : HSFLOW_F32;
    // d_out: the nt frames (f32 or u8), the nt flag planes, trusted
    const size_t ob = align_up(n * nt * elem_size(dev_out)), flb = align_up(n * nt);
    if ((rc = grow(ctx, &ctx->d_in, &ctx->d_in_bytes, align_up(n * in_es) * 2))) return rc;
    if ((rc = grow(ctx, &ctx->d_out, &ctx->d_out_bytes, ob + flb + kAlign))) return rc;
    const size_t wsb = hsflow_flow_interp_workspace_bytes(rows, cols, 1, levels) +
                       (pf_on(&ctx->pf) ? pf_planes_bytes(rows, cols, 1) : 0);
    if ((rc = grow(ctx, &ctx->d_ws, &ctx->d_ws_bytes, wsb))) return rc;
    char *in0 = (char *)ctx->d_in, *in1 = in0 + align_up(n * in_es);
    char *dout = (char *)ctx->d_out;
    uint8_t *dfl = (uint8_t *)(dout + ob);
    uint32_t *dtr = (uint32_t *)(dout + ob + flb);
    if ((rc = upload_pair(ctx, I0, I1, (int)in_es, rows, cols, in_step0, in_step1, in0, in1)))
        return rc;
    rc = flow_interp_impl(ctx, in0, in1, dtype_in, rows, cols, 1, levels, warps, median, window,
                          iters, (float)alpha, rel, abs_thr, times, nt, dout, dev_out,
                          flags ? dfl : nullptr, trusted ? dtr : nullptr, &ctx->pf, ctx->d_ws,
                          ctx->d_ws_bytes, ctx->stream, &ctx->sm);
    if (rc) return rc;
    if (flags)
        for (int k = 0; k < nt; ++k)
            HIP_TRY(ctx, hipMemcpy2DAsync(flags[k], flags_step, dfl + k * n, (size_t)cols,
                                          (size_t)cols, rows, hipMemcpyDeviceToHost,
                                          ctx->stream));
    if (trusted)
        HIP_TRY(ctx, hipMemcpyAsync(trusted, dtr, (size_t)nt * sizeof(uint32_t),
                                    hipMemcpyDeviceToHost, ctx->stream));
    if (dev_out == HSFLOW_U8) {
        for (int k = 0; k < nt; ++k)
            HIP_TRY(ctx, hipMemcpy2DAsync(out[k], out_step, dout + k * n, (size_t)cols,
                                          (size_t)cols, rows, hipMemcpyDeviceToHost,
                                          ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return HSFLOW_OK;
    }
    const float *srcs[HSFLOW_MAX_TIMES];
    for (int k = 0; k < nt; ++k) srcs[k] = (const float *)dout + k * n;
    return download_planes(ctx, srcs, out, nt, rows, cols, dtype_out, out_step);
}

// ---- colour (BGR) frame warp and frame interpolation ------------------------
int check_bgr_out_dtype(hsflow_ctx *ctx, int dtype_out) {
    if (dtype_out != HSFLOW_F32 && dtype_out != HSFLOW_U8)
        return fail(ctx, HSFLOW_ERR_ARG, "BGR output dtype must be U8 or F32");
    return HSFLOW_OK;
}

int warp_image_bgr_impl(hsflow_ctx *ctx, const uint8_t *bgr, int rows, int cols, int batch,
                        const float *u, const float *v, void *out, int dtype_out, uint8_t *oof,
                        hipStream_t s) {
    if (!sizes_ok(rows, cols, batch))
        return fail(ctx, HSFLOW_ERR_ARG, "bad size %dx%d batch %d", rows, cols, batch);
    if (!bgr || !u || !v || !out) return fail(ctx, HSFLOW_ERR_ARG, "null device pointer");
    int rc = check_bgr_out_dtype(ctx, dtype_out);
    if (rc) return rc;
    const size_t n = (size_t)rows * cols * batch;
    const ByteRange in[3] = {{bgr, n * 3}, {u, n * 4}, {v, n * 4}};
    const ByteRange outs[2] = {{out, n * 3 * elem_size(dtype_out)}, {oof, n}};
    if (!outputs_disjoint(in, 3, outs, 2))
        return fail(ctx, HSFLOW_ERR_ARG, "warp outputs overlap the inputs or each other");
    hipError_t e = hsflow::launch_warp_image_bgr(bgr, rows, cols, batch, u, v, out,
                                                 dtype_out == HSFLOW_U8, oof, s);
    if (e != hipSuccess) return hip_fail(ctx, e, "BGR warp image launch");
    return HSFLOW_OK;
}

// KIC on checked arguments: trusted zeroed stream-ordered, then one launch
int frame_interp_bgr_run(hsflow_ctx *ctx, const uint8_t *bgr0, const uint8_t *bgr1, int rows,
                         int cols, int batch, const float *uf, const float *vf, const float *ub,
                         const float *vb, const uint8_t *mask_f, const uint8_t *mask_b,
                         const float *times, int nt, void *out, int dtype_out, uint8_t *flags,
                         uint32_t *trusted, hipStream_t s) {
    if (trusted) HIP_TRY(ctx, hipMemsetAsync(trusted, 0, (size_t)batch * nt * 4, s));
    hipError_t e = hsflow::launch_frame_interp_bgr(bgr0, bgr1, rows, cols, batch, uf, vf, ub, vb,
                                                   mask_f, mask_b, times, nt, out,
                                                   dtype_out == HSFLOW_U8, flags, trusted, s);
    if (e != hipSuccess) return hip_fail(ctx, e, "BGR frame interpolation launch");
    return HSFLOW_OK;
}

int frame_interp_bgr_impl(hsflow_ctx *ctx, const uint8_t *bgr0, const uint8_t *bgr1, int rows,
                          int cols, int batch, const float *uf, const float *vf, const float *ub,
                          const float *vb, const uint8_t *mask_f, const uint8_t *mask_b,
                          const float *times, int nt, void *out, int dtype_out, uint8_t *flags,
                          uint32_t *trusted, hipStream_t s) {
    if (!sizes_ok(rows, cols, batch))
        return fail(ctx, HSFLOW_ERR_ARG, "bad size %dx%d batch %d", rows, cols, batch);
    if (!bgr0 || !bgr1 || !uf || !vf || !ub || !vb || !out)
        return fail(ctx, HSFLOW_ERR_ARG, "null device pointer");
    int rc = check_interp_args(ctx, times, nt, dtype_out, false);
    if (rc) return rc;
    const size_t n = (size_t)rows * cols * batch;
    const ByteRange in[8] = {{bgr0, n * 3}, {bgr1, n * 3}, {uf, n * 4},  {vf, n * 4},
                             {ub, n * 4},   {vb, n * 4},   {mask_f, n}, {mask_b, n}};
    const ByteRange outs[3] = {{out, n * nt * 3 * elem_size(dtype_out)},
                               {flags, n * nt},
                               {trusted, (size_t)batch * nt * 4}};
    if (!outputs_disjoint(in, 8, outs, 3))
        return fail(ctx, HSFLOW_ERR_ARG,
                    "interpolation outputs overlap the inputs or each other");
    return frame_interp_bgr_run(ctx, bgr0, bgr1, rows, cols, batch, uf, vf, ub, vb, mask_f, mask_b,
                                times, nt, out, dtype_out, flags, trusted, s);
}

// Workspace of the fused BGR call: [the grey interpolation's (InterpLayout)]
// [grey I0][grey I1] (u8 batch planes), each 256-byte aligned.
struct InterpBgrLayout {
    InterpLayout grey;
    size_t gray[2], bytes;
};

InterpBgrLayout interp_bgr_layout(int rows, int cols, int batch, int levels) {
    InterpBgrLayout L{};
    const size_t n = (size_t)rows * cols * batch;
    L.grey = interp_layout(rows, cols, batch, levels);
    size_t off = L.grey.bytes;
    for (int k = 0; k < 2; ++k) L.gray[k] = off, off += align_up(n);
    L.bytes = off;
    return L;
}

// hsflow_bgr_to_gray_device of both frames into the workspace,
// hsflow_flow_bidir_median_device on the grey planes (the masks only when
// flags or trusted needs them), then KIC on the BGR frames: three public
// calls one after the other, so the bits are theirs by construction.  With a
// prefilter the grey planes are prefiltered into two f32 planes behind that
// layout and the solve runs on those.
int flow_interp_bgr_impl(hsflow_ctx *ctx, const uint8_t *bgr0, const uint8_t *bgr1, int rows,
                         int cols, int batch, int levels, int warps, int median, int window,
                         int iters, float alpha, float rel, float abs_thr, const float *times,
                         int nt, void *out, int dtype_out, uint8_t *flags, uint32_t *trusted,
                         const hsflow_prefilter *pf, void *ws, size_t ws_bytes, hipStream_t s,
                         const hsflow_smoothness *sm = nullptr) {
    PfPlan P;
    int rc = pf_on(pf) ? plan_prefilter(ctx, pf, &P) : HSFLOW_OK;
    if (rc) return rc;
    if ((rc = check_warped_args(ctx, warps, window, iters))) return rc;
    if ((rc = check_median_arg(ctx, median))) return rc;
    if ((rc = check_smoothness_for(ctx, sm, window))) return rc;
    if (levels < 1 || levels > HSFLOW_MAX_LEVELS)
        return fail(ctx, HSFLOW_ERR_ARG, "levels %d outside [1, %d]", levels,
                    HSFLOW_MAX_LEVELS);
    if (!sizes_ok(rows, cols, batch))
        return fail(ctx, HSFLOW_ERR_ARG, "bad size %dx%d batch %d", rows, cols, batch);
    if (!bgr0 || !bgr1 || !out || !ws) return fail(ctx, HSFLOW_ERR_ARG, "null device pointer");
    if ((rc = check_thresholds(ctx, rel, abs_thr))) return rc;
    if ((rc = check_interp_args(ctx, times, nt, dtype_out, false))) return rc;
    const InterpBgrLayout L = interp_bgr_layout(rows, cols, batch, levels);
    const size_t need = L.bytes + (pf_on(pf) ? pf_planes_bytes(rows, cols, batch) : 0);
    if (ws_bytes < need)
        return fail(ctx, HSFLOW_ERR_ARG, "workspace %zu < %zu bytes", ws_bytes, need);
    const size_t n = (size_t)rows * cols * batch;
    const ByteRange in[3] = {{bgr0, n * 3}, {bgr1, n * 3}, {ws, need}};
    const ByteRange outs[3] = {{out, n * nt * 3 * elem_size(dtype_out)},
                               {flags, n * nt},
                               {trusted, (size_t)batch * nt * 4}};
    if (!outputs_disjoint(in, 3, outs, 3))
        return fail(ctx, HSFLOW_ERR_ARG,
                    "interpolation outputs overlap the frames, the workspace or each other");
    // the frames must not overlap the workspace either: the grey planes are
    // written while the BGR frames are still to be read
    if (bytes_overlap(bgr0, n * 3, ws, need) || bytes_overlap(bgr1, n * 3, ws, need))
        return fail(ctx, HSFLOW_ERR_ARG, "the frames overlap the workspace");
    char *base = (char *)ws;
    uint8_t *g0 = (uint8_t *)(base + L.gray[0]), *g1 = (uint8_t *)(base + L.gray[1]);
    float *f[4];
    for (int k = 0; k < 4; ++k) f[k] = (float *)(base + L.grey.flow[k]);
    const bool masks = flags || trusted;
    uint8_t *mf = masks ? (uint8_t *)(base + L.grey.mask[0]) : nullptr;
    uint8_t *mb = masks ? (uint8_t *)(base + L.grey.mask[1]) : nullptr;
    hipError_t e = hsflow::launch_bgr2gray(bgr0, rows, cols, batch, g0, s);
    if (e == hipSuccess) e = hsflow::launch_bgr2gray(bgr1, rows, cols, batch, g1, s);
    if (e != hipSuccess) return hip_fail(ctx, e, "bgr2gray launch");
    const void *S0 = g0, *S1 = g1;
    int dtype_solve = HSFLOW_U8;
    if (pf_on(pf)) {
        float *p0, *p1;
        rc = prefilter_pair(ctx, g0, g1, HSFLOW_U8, rows, cols, batch, P, ws, L.bytes, &p0, &p1,
                            s);
        if (rc) return rc;
        S0 = p0, S1 = p1, dtype_solve = HSFLOW_F32;
    }
    rc = bidir_impl(ctx, S0, S1, dtype_solve, rows, cols, batch, levels, warps, median, window,
                    iters, alpha, rel, abs_thr, f[0], f[1], f[2], f[3], nullptr, mf, nullptr,
                    nullptr, mb, nullptr, ws, L.grey.solve_bytes, s, sm);
    if (rc) return rc;
    return frame_interp_bgr_run(ctx, bgr0, bgr1, rows, cols, batch, f[0], f[1], f[2], f[3], mf, mb,
                                times, nt, out, dtype_out, flags, trusted, s);
}

// The host-buffer form: the frames go up as 3 B/px (hsflow_flow_bgr's upload),
// flow_interp_bgr_impl on the context's buffers, then flags and trusted down on
// the same stream ahead of the frames, whose download drains it.
int flow_interp_bgr_host(hsflow_ctx *ctx, const uint8_t *bgr0, const uint8_t *bgr1, int rows,
                         int cols, size_t bgr_step0, size_t bgr_step1, int levels, int warps,
                         int median, int window, int iters, double alpha, float rel,
                         float abs_thr, const float *times, int nt, void *const *out,
                         int dtype_out, size_t out_step, uint8_t *const *flags,
                         size_t flags_step, uint32_t *trusted) {
    // the arguments first (a null context fails after them, so that they can
    // be checked where there is no device)
    int rc = check_interp_args(ctx, times, nt, dtype_out, false);
    if (rc) return rc;
    if (!bgr0 || !bgr1) return fail(ctx, HSFLOW_ERR_ARG, "null image");
    if (!sizes_ok(rows, cols, 1)) return fail(ctx, HSFLOW_ERR_ARG, "bad size %dx%d", rows, cols);
    if (bgr_step0 < (size_t)cols * 3 || bgr_step1 < (size_t)cols * 3)
        return fail(ctx, HSFLOW_ERR_ARG, "BGR steps %zu, %zu < row bytes", bgr_step0,
                    bgr_step1);
    const size_t es = (size_t)elem_size(dtype_out);
    if (out_step < (size_t)cols * 3 * es)
        return fail(ctx, HSFLOW_ERR_ARG, "output step %zu < row bytes", out_step);
    if (!out) return fail(ctx, HSFLOW_ERR_ARG, "null output");
    for (int k = 0; k < nt; ++k)
        if (!out[k] || (flags && !flags[k]))
            return fail(ctx, HSFLOW_ERR_ARG, "null output plane %d", k);
    if (flags && flags_step < (size_t)cols)
        return fail(ctx, HSFLOW_ERR_ARG, "flags step %zu < row bytes %d", flags_step, cols);
    if (levels < 1 || levels > HSFLOW_MAX_LEVELS)
        return fail(ctx, HSFLOW_ERR_ARG, "levels %d outside [1, %d]", levels,
                    HSFLOW_MAX_LEVELS);
    if ((rc = check_warped_args(ctx, warps, window, iters))) return rc;
    if ((rc = check_median_arg(ctx, median))) return rc;
    if ((rc = check_thresholds(ctx, rel, abs_thr))) return rc;
    if (!ctx) return fail(nullptr, HSFLOW_ERR_ARG, "null context");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)rows * cols;
    // d_out: the nt frames (f32 or u8 BGR), the nt flag planes, trusted
    const size_t ob = align_up(n * nt * 3 * es), flb = align_up(n * nt);
    if ((rc = grow(ctx, &ctx->d_in, &ctx->d_in_bytes, align_up(n * 3) * 2))) return rc;
    if ((rc = grow(ctx, &ctx->d_out, &ctx->d_out_bytes, ob + flb + kAlign))) return rc;
    const size_t wsb = interp_bgr_layout(rows, cols, 1, levels).bytes +
                       (pf_on(&ctx->pf) ? pf_planes_bytes(rows, cols, 1) : 0);
    if ((rc = grow(ctx, &ctx->d_ws, &ctx->d_ws_bytes, wsb))) return rc;
    uint8_t *in0 = (uint8_t *)ctx->d_in, *in1 = in0 + align_up(n * 3);
    char *dout = (char *)ctx->d_out;
    uint8_t *dfl = (uint8_t *)(dout + ob);
    uint32_t *dtr = (uint32_t *)(dout + ob + flb);
    if ((rc = upload_pair(ctx, bgr0, bgr1, 3, rows, cols, bgr_step0, bgr_step1, in0, in1)))
        return rc;
    rc = flow_interp_bgr_impl(ctx, in0, in1, rows, cols, 1, levels, warps, median, window, iters,
                              (float)alpha, rel, abs_thr, times, nt, dout, dtype_out,
                              flags ? dfl : nullptr, trusted ? dtr : nullptr, &ctx->pf, ctx->d_ws,
                              ctx->d_ws_bytes, ctx->stream, &ctx->sm);
    if (rc) return rc;
    if (flags)
        for (int k = 0; k < nt; ++k)
            HIP_TRY(ctx, hipMemcpy2DAsync(flags[k], flags_step, dfl + k * n, (size_t)cols,
                                          (size_t)cols, rows, hipMemcpyDeviceToHost,
                                          ctx->stream));
    if (trusted)
        HIP_TRY(ctx, hipMemcpyAsync(trusted, dtr, (size_t)nt * sizeof(uint32_t),
                                    hipMemcpyDeviceToHost, ctx->stream));
    if (dtype_out == HSFLOW_U8) {
        for (int k = 0; k < nt; ++k)
            HIP_TRY(ctx, hipMemcpy2DAsync(out[k], out_step, dout + k * n * 3, (size_t)cols * 3,
                                          (size_t)cols * 3, rows, hipMemcpyDeviceToHost,
                                          ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return HSFLOW_OK;
    }
    // f32: a BGR plane is rows x 3 cols floats
    const float *srcs[HSFLOW_MAX_TIMES];
    for (int k = 0; k < nt; ++k) srcs[k] = (const float *)dout + k * n * 3;
    return download_planes(ctx, srcs, out, nt, rows, cols * 3, HSFLOW_F32, out_step);
}

// hsflow_flow_multi's kept contexts: one per (device, slot), each behind its
// own lock (calls that list disjoint devices run concurrently); the registry
// lock only guards the table's shape.  Slots are never freed (stable
// pointers); hsflow_flow_multi_release destroys their contexts.
struct MultiSlot {
    std::mutex mu;
    hsflow_ctx *ctx = nullptr;
};
std::mutex g_multi_mu;
std::vector<std::vector<std::unique_ptr<MultiSlot>>> g_multi;  // [device][slot]

std::vector<MultiSlot *> multi_slots(const int *devices, int nw) {
    std::lock_guard<std::mutex> reg(g_multi_mu);
    std::vector<MultiSlot *> out(nw);
    for (int k = 0; k < nw; ++k) {
        int dup = 0;  // earlier workers on the same device
        for (int i = 0; i < k; ++i) dup += devices[i] == devices[k];
        if ((int)g_multi.size() <= devices[k]) g_multi.resize(devices[k] + 1);
        auto &dv = g_multi[devices[k]];
        while ((int)dv.size() <= dup) dv.push_back(std::make_unique<MultiSlot>());
        out[k] = dv[dup].get();
    }
    return out;
}

}  // namespace

extern "C" {

int hsflow_version(void) { return HSFLOW_VERSION; }

// No diagnostic build exists any more (the environment-honouring probe build
// of round 2 was retired with its switches); kept for ABI stability.
int hsflow_build_flags(void) { return 0; }

const char *hsflow_status_string(int status) {
    switch (status) {
    case HSFLOW_OK: return "ok";
    case HSFLOW_ERR_ARG: return "invalid argument";
    case HSFLOW_ERR_HIP: return "HIP runtime error";
    case HSFLOW_ERR_OOM: return "device out of memory";
    case HSFLOW_ERR_NODEV: return "no usable HIP device";
    case HSFLOW_ERR_SIZE: return "image sizes differ";
    default: return "unknown status";
    }
}

int hsflow_create(hsflow_ctx **out, int device) {
    if (!out) return fail(nullptr, HSFLOW_ERR_ARG, "null ctx pointer");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(nullptr, HSFLOW_ERR_NODEV, "no HIP device");
    if (device < 0 || device >= n)
        return fail(nullptr, HSFLOW_ERR_NODEV, "device %d of %d", device, n);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess)
        return fail(nullptr, HSFLOW_ERR_NODEV, "hipGetDeviceProperties failed");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, HSFLOW_ERR_NODEV, "device %d is %s, libhsflow is built for gfx950",
                    device, prop.gcnArchName);
    hsflow_ctx *ctx = new hsflow_ctx();
    ctx->device = device;
    if (hipSetDevice(device) != hipSuccess ||
        hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return fail(nullptr, HSFLOW_ERR_HIP, "stream creation failed");
    }
    *out = ctx;
    return HSFLOW_OK;
}

void hsflow_destroy(hsflow_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->d_in) (void)hipFree(ctx->d_in);
    if (ctx->d_out) (void)hipFree(ctx->d_out);
    if (ctx->d_ws) (void)hipFree(ctx->d_ws);
    if (ctx->h_stage) (void)hipHostFree(ctx->h_stage);
    for (hipEvent_t e : ctx->dl_ev) (void)hipEventDestroy(e);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char *hsflow_last_error(const hsflow_ctx *ctx) {
    return ctx ? ctx->err.c_str() : g_err.c_str();
}

void *hsflow_stream(hsflow_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

size_t hsflow_workspace_bytes(int rows, int cols, int batch) {
    if (!sizes_ok(rows, cols, batch)) return 0;
    return carve(nullptr, rows, cols, batch).bytes;
}

int hsflow_set_iters_per_launch(int k) {
    if (k < 0) return HSFLOW_ERR_ARG;
    g_kb_override = k;
    return HSFLOW_OK;
}

int hsflow_set_jacobi_kernel(int k) {
    if (k != 0 && k != 2 && k != 4) return HSFLOW_ERR_ARG;
    g_kernel_override = k;
    return HSFLOW_OK;
}

int hsflow_set_strip_rows(int seg_rows) {
    if (seg_rows < 0 || seg_rows > kMaxRows) return HSFLOW_ERR_ARG;
    g_strip_rows = seg_rows;
    return HSFLOW_OK;
}

const char *hsflow_jacobi_kernel_name(int rows, int cols, int batch, int window) {
    if (window < 1 || window > HSFLOW_MAX_WINDOW || !sizes_ok(rows, cols, batch)) return "";
    if (window > 9) return "hs_jacobi_generic_kernel";
    if (plan_passes(window, true, rows, cols, batch).strip) return "hs_jacobi_strip_kernel";
    return window >= 3 ? "hs_jacobi_wg_kernel" : "hs_jacobi_kernel";
}

int hsflow_strip_seg_rows(int rows, int cols, int batch, int window) {
    if (window < 1 || window > HSFLOW_MAX_WINDOW || !sizes_ok(rows, cols, batch)) return 0;
    if (!plan_passes(window, true, rows, cols, batch).strip) return 0;
    if (g_strip_rows > 0) {
        int nseg = 0, nstrips = 0;
        return hsflow::strip_seg_rows(window, strip_kb(window), rows, cols, batch, 1, &nseg,
                                      &nstrips, g_strip_rows);
    }
    int nseg = 0, nstrips = 0;
    return hsflow::strip_seg_rows(window, strip_kb(window), rows, cols, batch,
                                  8 * hsflow::device_cus(), &nseg, &nstrips, 0);
}

int hsflow_set_max_streams(int n) {
    if (n < 0 || n > 16) return HSFLOW_ERR_ARG;
    g_split_override = n;
    return HSFLOW_OK;
}

int hsflow_max_streams(void) { return g_split_override; }

int hsflow_set_first_pass_fusion(int on) {
    g_first_fusion = on ? 1 : 0;
    return HSFLOW_OK;
}

int hsflow_first_pass_fusion(void) { return g_first_fusion; }

long long hsflow_first_pass_launches(void) {
    return g_first_launches.load(std::memory_order_relaxed);
}

int hsflow_set_output_hugepages(int on) {
    return hsflow::g_output_hugepages.exchange(on ? 1 : 0);
}

int hsflow_iters_per_launch(int rows, int cols, int batch, int window) {
    if (window < 1 || window > HSFLOW_MAX_WINDOW) return HSFLOW_ERR_ARG;
    if (!sizes_ok(rows, cols, batch)) return HSFLOW_ERR_ARG;
    return pick_kb(window, true, rows, cols, batch);
}

int hsflow_gradients_device(const void *I0, const void *I1, int dtype_in, int rows,
                            int cols, int batch, float *gx, float *gy, float *gt,
                            void *workspace, size_t workspace_bytes, void *stream) {
    DeviceGuard g((hipStream_t)stream);
    return gradients_impl(nullptr, I0, I1, dtype_in, rows, cols, batch, gx, gy, gt,
                          workspace, workspace_bytes, (hipStream_t)stream);
}

int hsflow_jacobi_device(int rows, int cols, int batch, int window, int iters,
                         float alpha, int warm_start, float *u, float *v, void *workspace,
                         size_t workspace_bytes, void *stream) {
    DeviceGuard g((hipStream_t)stream);
    // the workspace flags say per pair which gradient format is valid; the
    // f32 variant is launched too unless we know every pair is packed
    return jacobi_impl(nullptr, rows, cols, batch, window, iters, alpha, warm_start != 0,
                       true, u, v, workspace, workspace_bytes, (hipStream_t)stream);
}

int hsflow_flow_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                       int batch, int window, int iters, float alpha, float *u, float *v,
                       void *workspace, size_t workspace_bytes, void *stream) {
    DeviceGuard g((hipStream_t)stream);
    // K1 fused into the first pass where the plan allows (cold_solve); else
    // K1 for the whole batch, then the passes (split over the side streams).
    // Running each half's stand-alone K1 on its side stream instead measured
    // 0.6 % slower (the halves' first passes start out of step;
    // profiles/r05_k1_ab.txt).
    // 8-bit inputs always give exact packed gradients: skip the f32 variant
    return cold_solve(nullptr, I0, I1, dtype_in, rows, cols, batch, window, iters, alpha,
                      dtype_in != HSFLOW_U8, u, v, workspace, workspace_bytes,
                      (hipStream_t)stream);
}

int hsflow_flow(hsflow_ctx *ctx, const void *I0, const void *I1, int dtype_in, int rows,
                int cols, size_t in_step0, size_t in_step1, int window, int iters,
                double alpha, void *u, void *v, int dtype_out, size_t out_step) {
    int rc = check_host_args(ctx, I0, I1, dtype_in, rows, cols, in_step0, in_step1,
                             dtype_out, out_step);
    if (rc) return rc;
    if (!u || !v) return fail(ctx, HSFLOW_ERR_ARG, "null output");
    if (window < 1 || window > HSFLOW_MAX_WINDOW)
        return fail(ctx, HSFLOW_ERR_ARG, "windowSize %d outside [1, %d]", window,
                    HSFLOW_MAX_WINDOW);
    if (iters < 0) return fail(ctx, HSFLOW_ERR_ARG, "maxIterations %d < 0", iters);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)rows * cols;
    const size_t in_es = (size_t)dev_elem_size(dtype_in);
    if ((rc = grow(ctx, &ctx->d_in, &ctx->d_in_bytes, align_up(n * in_es) * 2))) return rc;
    if ((rc = grow(ctx, &ctx->d_out, &ctx->d_out_bytes, align_up(n * 4) * 3))) return rc;
    const size_t wsb = hsflow_workspace_bytes(rows, cols, 1);
    if ((rc = grow(ctx, &ctx->d_ws, &ctx->d_ws_bytes, wsb))) return rc;
    char *in0 = (char *)ctx->d_in, *in1 = in0 + align_up(n * in_es);
    float *du = (float *)ctx->d_out, *dv = (float *)((char *)du + align_up(n * 4));
    if ((rc = upload_pair(ctx, I0, I1, (int)in_es, rows, cols, in_step0, in_step1, in0, in1)))
        return rc;
    const int dt0 = dtype_in;
    rc = cold_solve(ctx, in0, in1, dt0, rows, cols, 1, window, iters, (float)alpha,
                    dt0 != HSFLOW_U8, du, dv, ctx->d_ws, ctx->d_ws_bytes, ctx->stream);
    if (rc) return rc;
    {
        const float *srcs[2] = {du, dv};
        void *dsts[2] = {u, v};
        if ((rc = download_planes(ctx, srcs, dsts, 2, rows, cols, dtype_out, out_step)))
            return rc;
    }
    return HSFLOW_OK;
}

// Frame-parallel host API over several GPUs of the node from ONE process
// (include/hsflow.h): one host thread, context and stream per listed device,
// pair j on devices[j % n].  The per-pair work is exactly hsflow_flow.
int hsflow_flow_multi(const int *devices, int n_devices, int batch,
                      const void *const *I0, const void *const *I1, int dtype_in, int rows,
                      int cols, size_t in_step0, size_t in_step1, int window, int iters,
                      double alpha, void *const *u, void *const *v, int dtype_out,
                      size_t out_step) {
    if (!devices || n_devices < 1 || n_devices > 64)
        return fail(nullptr, HSFLOW_ERR_ARG, "need 1..64 devices, got %d", n_devices);
    if (batch < 0) return fail(nullptr, HSFLOW_ERR_ARG, "batch %d < 0", batch);
    if (batch == 0) return HSFLOW_OK;
    if (!I0 || !I1 || !u || !v) return fail(nullptr, HSFLOW_ERR_ARG, "null pair array");
    for (int j = 0; j < batch; ++j)
        if (!I0[j] || !I1[j] || !u[j] || !v[j])
            return fail(nullptr, HSFLOW_ERR_ARG, "null buffer in pair %d", j);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, HSFLOW_ERR_NODEV, "no HIP device");
    for (int k = 0; k < n_devices; ++k)
        if (devices[k] < 0 || devices[k] >= ndev)
            return fail(nullptr, HSFLOW_ERR_NODEV, "device %d of %d", devices[k], ndev);
    const int nw = std::min(n_devices, batch);
    std::vector<MultiSlot *> slot = multi_slots(devices, nw);
    std::vector<int> rc(nw, HSFLOW_OK);
    std::vector<std::string> msg(nw);
    std::vector<std::thread> pool;
    pool.reserve(nw);
    for (int k = 0; k < nw; ++k) {
        pool.emplace_back([&, k] {
            std::lock_guard<std::mutex> hold(slot[k]->mu);
            int r = HSFLOW_OK;
            if (!slot[k]->ctx) {
                r = hsflow_create(&slot[k]->ctx, devices[k]);
                if (r) {
                    rc[k] = r;
                    msg[k] = hsflow_last_error(nullptr);  // this worker's message
                    return;
                }
            }
            hsflow_ctx *ctx = slot[k]->ctx;
            for (int j = k; j < batch && r == HSFLOW_OK; j += nw)
                r = hsflow_flow(ctx, I0[j], I1[j], dtype_in, rows, cols, in_step0, in_step1,
                                window, iters, alpha, u[j], v[j], dtype_out, out_step);
            if (r) {
                msg[k] = hsflow_last_error(ctx);
                // a context that hit a runtime error is not trusted with the
                // next call; argument and size errors leave it as it was
                if (r != HSFLOW_ERR_ARG && r != HSFLOW_ERR_SIZE) {
                    hsflow_destroy(ctx);
                    slot[k]->ctx = nullptr;
                }
            }
            rc[k] = r;
        });
    }
    for (auto &t : pool) t.join();
    for (int k = 0; k < nw; ++k)
        if (rc[k]) return fail(nullptr, rc[k], "device %d: %s", devices[k], msg[k].c_str());
    return HSFLOW_OK;
}

void hsflow_flow_multi_release(void) {
    std::lock_guard<std::mutex> reg(g_multi_mu);
    for (auto &dv : g_multi)
        for (auto &sl : dv) {
            std::lock_guard<std::mutex> hold(sl->mu);
            if (sl->ctx) hsflow_destroy(sl->ctx);
            sl->ctx = nullptr;
        }
}

int hsflow_pyramid_level_size(int rows, int cols, int level, int *level_rows,
                              int *level_cols) {
    if (rows < 1 || cols < 1 || level < 0 || level >= HSFLOW_MAX_LEVELS) return HSFLOW_ERR_ARG;
    for (int l = 0; l < level; ++l) {
        rows = (rows + 1) / 2;
        cols = (cols + 1) / 2;
    }
    if (level_rows) *level_rows = rows;
    if (level_cols) *level_cols = cols;
    return HSFLOW_OK;
}

size_t hsflow_pyramid_workspace_bytes(int rows, int cols, int batch, int levels) {
    if (!sizes_ok(rows, cols, batch) || levels < 1 || levels > HSFLOW_MAX_LEVELS) return 0;
    return pyr_layout(rows, cols, batch, levels).bytes;
}

int hsflow_pyramid_build_device(const void *I0, const void *I1, int dtype_in, int rows,
                                int cols, int batch, int levels, float *const *I0_levels,
                                float *const *I1_levels, void *workspace,
                                size_t workspace_bytes, void *stream) {
    if (levels < 1 || levels > HSFLOW_MAX_LEVELS)
        return fail(nullptr, HSFLOW_ERR_ARG, "levels %d outside [1, %d]", levels,
                    HSFLOW_MAX_LEVELS);
    if (levels > 1 && (!I0_levels || !I1_levels))
        return fail(nullptr, HSFLOW_ERR_ARG, "null level array");
    for (int l = 1; l < levels; ++l)
        if (!I0_levels[l - 1] || !I1_levels[l - 1])
            return fail(nullptr, HSFLOW_ERR_ARG, "null level plane %d", l);
    hipStream_t s = (hipStream_t)stream;
    DeviceGuard g(s);
    // K1 at level 0 decides each pair's rounding (flags in the workspace)
    int rc = gradients_impl(nullptr, I0, I1, dtype_in, rows, cols, batch, nullptr, nullptr,
                            nullptr, workspace, workspace_bytes, s);
    if (rc || levels == 1) return rc;
    const uint32_t *flags = carve(workspace, rows, cols, batch).flags;
    int r = rows, c = cols;
    for (int l = 1; l < levels; ++l) {
        for (int k = 0; k < 2; ++k) {
            const void *src = l == 1 ? (k ? I1 : I0)
                                     : (const void *)(k ? I1_levels[l - 2] : I0_levels[l - 2]);
            hipError_t e = hsflow::launch_pyrdown(src, l == 1 ? dtype_in : HSFLOW_F32, r, c,
                                                  batch, k ? I1_levels[l - 1] : I0_levels[l - 1],
                                                  flags, s);
            if (e != hipSuccess) return hip_fail(nullptr, e, "pyrdown launch");
        }
        r = (r + 1) / 2;
        c = (c + 1) / 2;
    }
    return HSFLOW_OK;
}

int hsflow_upflow_device(const float *uc, const float *vc, int rc, int cc, float *u,
                         float *v, int rows, int cols, int batch, void *stream) {
    DeviceGuard g((hipStream_t)stream);
    if (!uc || !vc || !u || !v) return fail(nullptr, HSFLOW_ERR_ARG, "null device pointer");
    if (!sizes_ok(rows, cols, batch) || rc < (rows + 1) / 2 || cc < (cols + 1) / 2)
        return fail(nullptr, HSFLOW_ERR_ARG, "bad sizes %dx%d from %dx%d", rows, cols, rc, cc);
    hipError_t e = hsflow::launch_upflow(uc, vc, rc, cc, u, v, rows, cols, batch,
                                         (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(nullptr, e, "upflow launch");
    return HSFLOW_OK;
}

int hsflow_flow_pyramid_device(const void *I0, const void *I1, int dtype_in, int rows,
                               int cols, int batch, int levels, int window, int iters,
                               float alpha, float *u, float *v, void *workspace,
                               size_t workspace_bytes, void *stream) {
    DeviceGuard g((hipStream_t)stream);
    return pyramid_impl(nullptr, I0, I1, dtype_in, rows, cols, batch, levels, window, iters,
                        alpha, u, v, workspace, workspace_bytes, (hipStream_t)stream);
}

int hsflow_flow_pyramid(hsflow_ctx *ctx, const void *I0, const void *I1, int dtype_in,
                        int rows, int cols, size_t in_step0, size_t in_step1, int levels,
                        int window, int iters, double alpha, void *u, void *v,
                        int dtype_out, size_t out_step) {
    return pyramid_host(ctx, I0, I1, dtype_in, rows, cols, in_step0, in_step1, levels, 0, 0,
                        window, iters, alpha, u, v, dtype_out, out_step);
}

int hsflow_warp_gradients_device(const void *I0, const void *I1, int dtype_in, int rows,
                                 int cols, int batch, const float *u0, const float *v0,
                                 float *gx, float *gy, float *gt, void *workspace,
                                 size_t workspace_bytes, void *stream) {
    DeviceGuard g((hipStream_t)stream);
    return warp_gradients_impl(nullptr, I0, I1, dtype_in, rows, cols, batch, u0, v0, gx, gy,
                               gt, workspace, workspace_bytes, (hipStream_t)stream);
}

int hsflow_flow_warped_median_device(const void *I0, const void *I1, int dtype_in, int rows,
                                     int cols, int batch, int levels, int warps, int median,
                                     int window, int iters, float alpha, float *u, float *v,
                                     void *workspace, size_t workspace_bytes, void *stream) {
    DeviceGuard g((hipStream_t)stream);
    return warped_impl(nullptr, I0, I1, dtype_in, rows, cols, batch, levels, warps, median,
                       window, iters, alpha, u, v, workspace, workspace_bytes,
                       (hipStream_t)stream);
}

int hsflow_flow_warped_pf_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                                 int batch, int levels, int warps, int median, int window,
                                 int iters, float alpha, float *u, float *v,
                                 const hsflow_prefilter *pf, void *workspace,
                                 size_t workspace_bytes, void *stream) {
    DeviceGuard g((hipStream_t)stream);
    return warped_pf_impl(nullptr, I0, I1, dtype_in, rows, cols, batch, levels, warps, median,
                          window, iters, alpha, u, v, pf, workspace, workspace_bytes,
                          (hipStream_t)stream);
}

int hsflow_flow_warped_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                              int batch, int levels, int warps, int window, int iters,
                              float alpha, float *u, float *v, void *workspace,
                              size_t workspace_bytes, void *stream) {
    return hsflow_flow_warped_median_device(I0, I1, dtype_in, rows, cols, batch, levels, warps,
                                            0, window, iters, alpha, u, v, workspace,
                                            workspace_bytes, stream);
}

int hsflow_flow_warped_median(hsflow_ctx *ctx, const void *I0, const void *I1, int dtype_in,
                              int rows, int cols, size_t in_step0, size_t in_step1, int levels,
                              int warps, int median, int window, int iters, double alpha,
                              void *u, void *v, int dtype_out, size_t out_step) {
    if (!ctx) return HSFLOW_ERR_ARG;
    int rc = check_warped_args(ctx, warps, window, iters);
    if (rc) return rc;
    if ((rc = check_median_arg(ctx, median))) return rc;
    return pyramid_host(ctx, I0, I1, dtype_in, rows, cols, in_step0, in_step1, levels, warps,
                        median, window, iters, alpha, u, v, dtype_out, out_step);
}

int hsflow_flow_warped(hsflow_ctx *ctx, const void *I0, const void *I1, int dtype_in, int rows,
                       int cols, size_t in_step0, size_t in_step1, int levels, int warps,
                       int window, int iters, double alpha, void *u, void *v, int dtype_out,
                       size_t out_step) {
    return hsflow_flow_warped_median(ctx, I0, I1, dtype_in, rows, cols, in_step0, in_step1,
                                     levels, warps, 0, window, iters, alpha, u, v, dtype_out,
                                     out_step);
}

int hsflow_flow_median_device(const float *u, const float *v, int rows, int cols, int batch,
                              int ksize, float *u_out, float *v_out, void *stream) {
    DeviceGuard g((hipStream_t)stream);
    return median_impl(nullptr, u, v, rows, cols, batch, ksize, u_out, v_out,
                       (hipStream_t)stream);
}

size_t hsflow_flow_bidir_workspace_bytes(int rows, int cols, int batch, int levels) {
    // both directions run in the one pyramid workspace, one after the other
    return hsflow_pyramid_workspace_bytes(rows, cols, batch, levels);
}

int hsflow_flow_consistency_device(const float *uf, const float *vf, const float *ub,
                                   const float *vb, int rows, int cols, int batch, float rel,
                                   float abs_thr, float *err, uint8_t *mask, uint32_t *counts,
                                   void *stream) {
    DeviceGuard g((hipStream_t)stream);
    return consistency_impl(nullptr, uf, vf, ub, vb, rows, cols, batch, rel, abs_thr, err, mask,
                            counts, (hipStream_t)stream);
}

int hsflow_flow_bidir_median_device(const void *I0, const void *I1, int dtype_in, int rows,
                                    int cols, int batch, int levels, int warps, int median,
                                    int window, int iters, float alpha, float rel, float abs_thr,
                                    float *uf, float *vf, float *ub, float *vb, float *err_f,
                                    uint8_t *mask_f, uint32_t *counts_f, float *err_b,
                                    uint8_t *mask_b, uint32_t *counts_b, void *workspace,
                                    size_t workspace_bytes, void *stream) {
    DeviceGuard g((hipStream_t)stream);
    return bidir_impl(nullptr, I0, I1, dtype_in, rows, cols, batch, levels, warps, median, window,
                      iters, alpha, rel, abs_thr, uf, vf, ub, vb, err_f, mask_f, counts_f, err_b,
                      mask_b, counts_b, workspace, workspace_bytes, (hipStream_t)stream);
}

int hsflow_flow_bidir_pf_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                                int batch, int levels, int warps, int median, int window,
                                int iters, float alpha, float rel, float abs_thr, float *uf,
                                float *vf, float *ub, float *vb, float *err_f, uint8_t *mask_f,
                                uint32_t *counts_f, float *err_b, uint8_t *mask_b,
                                uint32_t *counts_b, const hsflow_prefilter *pf, void *workspace,
                                size_t workspace_bytes, void *stream) {
    DeviceGuard g((hipStream_t)stream);
    return bidir_pf_impl(nullptr, I0, I1, dtype_in, rows, cols, batch, levels, warps, median,
                         window, iters, alpha, rel, abs_thr, uf, vf, ub, vb, err_f, mask_f,
                         counts_f, err_b, mask_b, counts_b, pf, workspace, workspace_bytes,
                         (hipStream_t)stream);
}

int hsflow_flow_bidir_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                             int batch, int levels, int warps, int window, int iters,
                             float alpha, float rel, float abs_thr, float *uf, float *vf, float *ub,
                             float *vb, float *err_f, uint8_t *mask_f, uint32_t *counts_f,
                             float *err_b, uint8_t *mask_b, uint32_t *counts_b, void *workspace,
                             size_t workspace_bytes, void *stream) {
    return hsflow_flow_bidir_median_device(I0, I1, dtype_in, rows, cols, batch, levels, warps, 0,
                                           window, iters, alpha, rel, abs_thr, uf, vf, ub, vb,
                                           err_f, mask_f, counts_f, err_b, mask_b, counts_b,
                                           workspace, workspace_bytes, stream);
}

int hsflow_flow_bidir_median(hsflow_ctx *ctx, const void *I0, const void *I1, int dtype_in,
                             int rows, int cols, size_t in_step0, size_t in_step1, int levels,
                             int warps, int median, int window, int iters, double alpha,
                             float rel, float abs_thr, void *u, void *v, void *ub, void *vb,
                             int dtype_out, size_t out_step, uint8_t *mask_f, uint8_t *mask_b,
                             size_t mask_step, uint32_t *counts) {
    if (!ctx) return HSFLOW_ERR_ARG;
    return bidir_host(ctx, I0, I1, dtype_in, rows, cols, in_step0, in_step1, levels, warps,
                      median, window, iters, alpha, rel, abs_thr, u, v, ub, vb, dtype_out,
                      out_step, mask_f, mask_b, mask_step, counts);
}

int hsflow_flow_bidir(hsflow_ctx *ctx, const void *I0, const void *I1, int dtype_in, int rows,
                      int cols, size_t in_step0, size_t in_step1, int levels, int warps,
                      int window, int iters, double alpha, float rel, float abs_thr, void *u,
                      void *v, void *ub, void *vb, int dtype_out, size_t out_step,
                      uint8_t *mask_f, uint8_t *mask_b, size_t mask_step, uint32_t *counts) {
    return hsflow_flow_bidir_median(ctx, I0, I1, dtype_in, rows, cols, in_step0, in_step1, levels,
                                    warps, 0, window, iters, alpha, rel, abs_thr, u, v, ub, vb,
                                    dtype_out, out_step, mask_f, mask_b, mask_step, counts);
}

int hsflow_warp_image_device(const void *I, int dtype_in, int rows, int cols, int batch,
                             const float *u, const float *v, float *out, uint8_t *oof,
                             void *stream) {
    DeviceGuard g((hipStream_t)stream);
    return warp_image_impl(nullptr, I, dtype_in, rows, cols, batch, u, v, out, oof,
                           (hipStream_t)stream);
}

int hsflow_frame_interp_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                               int batch, const float *uf, const float *vf, const float *ub,
                               const float *vb, const uint8_t *mask_f, const uint8_t *mask_b,
                               const float *times, int nt, void *out, int dtype_out,
                               uint8_t *flags, uint32_t *trusted, void *stream) {
    DeviceGuard g((hipStream_t)stream);
    return frame_interp_impl(nullptr, I0, I1, dtype_in, rows, cols, batch, uf, vf, ub, vb, mask_f,
                             mask_b, times, nt, out, dtype_out, flags, trusted,
                             (hipStream_t)stream);
}

size_t hsflow_flow_interp_workspace_bytes(int rows, int cols, int batch, int levels) {
    if (!sizes_ok(rows, cols, batch) || levels < 1 || levels > HSFLOW_MAX_LEVELS) return 0;
    return interp_layout(rows, cols, batch, levels).bytes;
}

int hsflow_flow_interp_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                              int batch, int levels, int warps, int median, int window,
                              int iters, float alpha, float rel, float abs_thr,
                              const float *times, int nt, void *out, int dtype_out,
                              uint8_t *flags, uint32_t *trusted, void *workspace,
                              size_t workspace_bytes, void *stream) {
    return hsflow_flow_interp_pf_device(I0, I1, dtype_in, rows, cols, batch, levels, warps, median,
                                        window, iters, alpha, rel, abs_thr, times, nt, out,
                                        dtype_out, flags, trusted, nullptr, workspace,
                                        workspace_bytes, stream);
}

int hsflow_flow_interp_pf_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                                 int batch, int levels, int warps, int median, int window,
                                 int iters, float alpha, float rel, float abs_thr,
                                 const float *times, int nt, void *out, int dtype_out,
                                 uint8_t *flags, uint32_t *trusted, const hsflow_prefilter *pf,
                                 void *workspace, size_t workspace_bytes, void *stream) {
    DeviceGuard g((hipStream_t)stream);
    return flow_interp_impl(nullptr, I0, I1, dtype_in, rows, cols, batch, levels, warps, median,
                            window, iters, alpha, rel, abs_thr, times, nt, out, dtype_out, flags,
                            trusted, pf, workspace, workspace_bytes, (hipStream_t)stream);
}

int hsflow_flow_interp(hsflow_ctx *ctx, const void *I0, const void *I1, int dtype_in, int rows,
                       int cols, size_t in_step0, size_t in_step1, int levels, int warps,
                       int median, int window, int iters, double alpha, float rel, float abs_thr,
                       const float *times, int nt, void *const *out, int dtype_out,
                       size_t out_step, uint8_t *const *flags, size_t flags_step,
                       uint32_t *trusted) {
    return flow_interp_host(ctx, I0, I1, dtype_in, rows, cols, in_step0, in_step1, levels, warps,
                            median, window, iters, alpha, rel, abs_thr, times, nt, out, dtype_out,
                            out_step, flags, flags_step, trusted);
}

int hsflow_warp_image_bgr_device(const uint8_t *bgr, int rows, int cols, int batch, const float *u,
                                 const float *v, void *out, int dtype_out, uint8_t *oof,
                                 void *stream) {
    DeviceGuard g((hipStream_t)stream);
    return warp_image_bgr_impl(nullptr, bgr, rows, cols, batch, u, v, out, dtype_out, oof,
                               (hipStream_t)stream);
}

int hsflow_frame_interp_bgr_device(const uint8_t *bgr0, const uint8_t *bgr1, int rows, int cols,
                                   int batch, const float *uf, const float *vf, const float *ub,
                                   const float *vb, const uint8_t *mask_f, const uint8_t *mask_b,
                                   const float *times, int nt, void *out, int dtype_out,
                                   uint8_t *flags, uint32_t *trusted, void *stream) {
    DeviceGuard g((hipStream_t)stream);
    return frame_interp_bgr_impl(nullptr, bgr0, bgr1, rows, cols, batch, uf, vf, ub, vb, mask_f,
                                 mask_b, times, nt, out, dtype_out, flags, trusted,
                                 (hipStream_t)stream);
}

size_t hsflow_flow_interp_bgr_workspace_bytes(int rows, int cols, int batch, int levels) {
    if (!sizes_ok(rows, cols, batch) || levels < 1 || levels > HSFLOW_MAX_LEVELS) return 0;
    return interp_bgr_layout(rows, cols, batch, levels).bytes;
}

int hsflow_flow_interp_bgr_device(const uint8_t *bgr0, const uint8_t *bgr1, int rows, int cols,
                                  int batch, int levels, int warps, int median, int window,
                                  int iters, float alpha, float rel, float abs_thr,
                                  const float *times, int nt, void *out, int dtype_out,
                                  uint8_t *flags, uint32_t *trusted, void *workspace,
                                  size_t workspace_bytes, void *stream) {
    return hsflow_flow_interp_bgr_pf_device(bgr0, bgr1, rows, cols, batch, levels, warps, median,
                                            window, iters, alpha, rel, abs_thr, times, nt, out,
                                            dtype_out, flags, trusted, nullptr, workspace,
                                            workspace_bytes, stream);
}

int hsflow_flow_interp_bgr_pf_device(const uint8_t *bgr0, const uint8_t *bgr1, int rows, int cols,
                                     int batch, int levels, int warps, int median, int window,
                                     int iters, float alpha, float rel, float abs_thr,
                                     const float *times, int nt, void *out, int dtype_out,
                                     uint8_t *flags, uint32_t *trusted, const hsflow_prefilter *pf,
                                     void *workspace, size_t workspace_bytes, void *stream) {
    DeviceGuard g((hipStream_t)stream);
    return flow_interp_bgr_impl(nullptr, bgr0, bgr1, rows, cols, batch, levels, warps, median,
                                window, iters, alpha, rel, abs_thr, times, nt, out, dtype_out,
                                flags, trusted, pf, workspace, workspace_bytes,
                                (hipStream_t)stream);
}

int hsflow_flow_interp_bgr(hsflow_ctx *ctx, const uint8_t *bgr0, const uint8_t *bgr1, int rows,
                           int cols, size_t bgr_step0, size_t bgr_step1, int levels, int warps,
                           int median, int window, int iters, double alpha, float rel,
                           float abs_thr, const float *times, int nt, void *const *out,
                           int dtype_out, size_t out_step, uint8_t *const *flags,
                           size_t flags_step, uint32_t *trusted) {
    return flow_interp_bgr_host(ctx, bgr0, bgr1, rows, cols, bgr_step0, bgr_step1, levels, warps,
                                median, window, iters, alpha, rel, abs_thr, times, nt, out,
                                dtype_out, out_step, flags, flags_step, trusted);
}

int hsflow_set_interp_bgr_loads(int wide) { return hsflow::set_interp_bgr_wide_loads(wide); }

int hsflow_prefilter_device(const void *I, int dtype_in, int rows, int cols, int batch,
                            const hsflow_prefilter *pf, float *out, void *stream) {
    DeviceGuard g((hipStream_t)stream);
    return prefilter_impl(nullptr, I, dtype_in, rows, cols, batch, pf, out, (hipStream_t)stream);
}

size_t hsflow_prefilter_planes_bytes(int rows, int cols, int batch) {
    if (!sizes_ok(rows, cols, batch)) return 0;
    return pf_planes_bytes(rows, cols, batch);
}

int hsflow_ctx_set_prefilter(hsflow_ctx *ctx, const hsflow_prefilter *pf) {
    if (!ctx) return fail(nullptr, HSFLOW_ERR_ARG, "null context");
    if (pf_on(pf)) {
        PfPlan P;
        int rc = plan_prefilter(ctx, pf, &P);
        if (rc) return rc;
        ctx->pf = *pf;
    } else {
        ctx->pf = hsflow_prefilter{0, 0.0f, 0.0f, 0.0f};
    }
    return HSFLOW_OK;
}

int hsflow_ctx_prefilter(const hsflow_ctx *ctx, hsflow_prefilter *pf) {
    if (!ctx || !pf) return fail(nullptr, HSFLOW_ERR_ARG, "null %s", ctx ? "prefilter" : "context");
    *pf = ctx->pf;
    return HSFLOW_OK;
}

int hsflow_flow_diffusivity_device(const float *u, const float *v, int rows, int cols, int batch,
                                   float lambda, float *g, void *stream) {
    DeviceGuard guard((hipStream_t)stream);
    return diffusivity_impl(nullptr, u, v, rows, cols, batch, lambda, g, (hipStream_t)stream);
}

int hsflow_jacobi_weighted_device(int rows, int cols, int batch, int window, int iters,
                                  float alpha, const float *g, float *u, float *v,
                                  void *workspace, size_t workspace_bytes, void *stream) {
    DeviceGuard guard((hipStream_t)stream);
    return jacobi_weighted_impl(nullptr, rows, cols, batch, window, iters, alpha, g, u, v,
                                workspace, workspace_bytes, (hipStream_t)stream);
}

int hsflow_flow_warped_sm_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                                 int batch, int levels, int warps, int median, int window,
                                 int iters, float alpha, float *u, float *v,
                                 const hsflow_prefilter *pf, const hsflow_smoothness *sm,
                                 void *workspace, size_t workspace_bytes, void *stream) {
    DeviceGuard g((hipStream_t)stream);
    return warped_pf_impl(nullptr, I0, I1, dtype_in, rows, cols, batch, levels, warps, median,
                          window, iters, alpha, u, v, pf, workspace, workspace_bytes,
                          (hipStream_t)stream, sm);
}

int hsflow_flow_bidir_sm_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                                int batch, int levels, int warps, int median, int window,
                                int iters, float alpha, float rel, float abs_thr, float *uf,
                                float *vf, float *ub, float *vb, float *err_f, uint8_t *mask_f,
                                uint32_t *counts_f, float *err_b, uint8_t *mask_b,
                                uint32_t *counts_b, const hsflow_prefilter *pf,
                                const hsflow_smoothness *sm, void *workspace,
                                size_t workspace_bytes, void *stream) {
    DeviceGuard g((hipStream_t)stream);
    return bidir_pf_impl(nullptr, I0, I1, dtype_in, rows, cols, batch, levels, warps, median,
                         window, iters, alpha, rel, abs_thr, uf, vf, ub, vb, err_f, mask_f,
                         counts_f, err_b, mask_b, counts_b, pf, workspace, workspace_bytes,
                         (hipStream_t)stream, sm);
}

int hsflow_flow_interp_sm_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                                 int batch, int levels, int warps, int median, int window,
                                 int iters, float alpha, float rel, float abs_thr,
                                 const float *times, int nt, void *out, int dtype_out,
                                 uint8_t *flags, uint32_t *trusted, const hsflow_prefilter *pf,
                                 const hsflow_smoothness *sm, void *workspace,
                                 size_t workspace_bytes, void *stream) {
    DeviceGuard g((hipStream_t)stream);
    return flow_interp_impl(nullptr, I0, I1, dtype_in, rows, cols, batch, levels, warps, median,
                            window, iters, alpha, rel, abs_thr, times, nt, out, dtype_out, flags,
                            trusted, pf, workspace, workspace_bytes, (hipStream_t)stream, sm);
}

int hsflow_flow_interp_bgr_sm_device(const uint8_t *bgr0, const uint8_t *bgr1, int rows, int cols,
                                     int batch, int levels, int warps, int median, int window,
                                     int iters, float alpha, float rel, float abs_thr,
                                     const float *times, int nt, void *out, int dtype_out,
                                     uint8_t *flags, uint32_t *trusted, const hsflow_prefilter *pf,
                                     const hsflow_smoothness *sm, void *workspace,
                                     size_t workspace_bytes, void *stream) {
    DeviceGuard g((hipStream_t)stream);
    return flow_interp_bgr_impl(nullptr, bgr0, bgr1, rows, cols, batch, levels, warps, median,
                                window, iters, alpha, rel, abs_thr, times, nt, out, dtype_out,
                                flags, trusted, pf, workspace, workspace_bytes,
                                (hipStream_t)stream, sm);
}

int hsflow_ctx_set_smoothness(hsflow_ctx *ctx, const hsflow_smoothness *sm) {
    if (!ctx) return fail(nullptr, HSFLOW_ERR_ARG, "null context");
    if (sm_on(sm)) {
        int rc = check_smoothness(ctx, sm);
        if (rc) return rc;
        ctx->sm = *sm;
    } else {
        ctx->sm = hsflow_smoothness{HSFLOW_SMOOTH_QUADRATIC, 0.0f};
    }
    return HSFLOW_OK;
}

int hsflow_ctx_smoothness(const hsflow_ctx *ctx, hsflow_smoothness *sm) {
    if (!ctx || !sm) return fail(nullptr, HSFLOW_ERR_ARG, "null %s", ctx ? "smoothness" : "context");
    *sm = ctx->sm;
    return HSFLOW_OK;
}

int hsflow_bgr_to_gray_device(const uint8_t *bgr, int rows, int cols, int batch,
                              uint8_t *gray, void *stream) {
    DeviceGuard g((hipStream_t)stream);
    if (!bgr || !gray) return fail(nullptr, HSFLOW_ERR_ARG, "null device pointer");
    if (!sizes_ok(rows, cols, batch))
        return fail(nullptr, HSFLOW_ERR_ARG, "bad size %dx%d batch %d", rows, cols, batch);
    hipError_t e = hsflow::launch_bgr2gray(bgr, rows, cols, batch, gray, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(nullptr, e, "bgr2gray launch");
    return HSFLOW_OK;
}

int hsflow_download_device(void *dst, const void *src, size_t bytes, void *stream) {
    if (bytes == 0) return HSFLOW_OK;
    if (!dst || !src) return fail(nullptr, HSFLOW_ERR_ARG, "null pointer");
    DeviceGuard g((hipStream_t)stream);
    // As a pitched copy the runtime moves a device -> pinned host download
    // with its DMA engines at ~46 GB/s (a flat hipMemcpyAsync: ~29 GB/s;
    // torch's copy_ of pinned memory: a blit kernel that takes the Jacobi
    // passes' workgroup slots; scripts/pcie/d2h_engine_probe.hip).
    constexpr size_t kRow = 7680;  // bytes per pitched row
    const size_t rows = bytes / kRow, tail = bytes - rows * kRow;
    hipStream_t s = (hipStream_t)stream;
    if (rows > 0)
        HIP_TRY(nullptr, hipMemcpy2DAsync(dst, kRow, src, kRow, kRow, rows,
                                          hipMemcpyDeviceToHost, s));
    if (tail > 0)
        HIP_TRY(nullptr, hipMemcpyAsync((char *)dst + rows * kRow,
                                        (const char *)src + rows * kRow, tail,
                                        hipMemcpyDeviceToHost, s));
    return HSFLOW_OK;
}

int hsflow_flow_bgr(hsflow_ctx *ctx, const uint8_t *bgr0, const uint8_t *bgr1, int rows,
                    int cols, size_t bgr_step0, size_t bgr_step1, int window, int iters,
                    double alpha, void *u, void *v, int dtype_out, size_t out_step) {
    if (!ctx) return HSFLOW_ERR_ARG;
    if (!bgr0 || !bgr1 || !u || !v) return fail(ctx, HSFLOW_ERR_ARG, "null pointer");
    if (!sizes_ok(rows, cols, 1)) return fail(ctx, HSFLOW_ERR_ARG, "bad size %dx%d", rows, cols);
    if (bgr_step0 < (size_t)cols * 3 || bgr_step1 < (size_t)cols * 3)
        return fail(ctx, HSFLOW_ERR_ARG, "BGR steps %zu, %zu < row bytes", bgr_step0,
                    bgr_step1);
    if (dtype_out != HSFLOW_F32 && dtype_out != HSFLOW_F64)
        return fail(ctx, HSFLOW_ERR_ARG, "output dtype must be F32 or F64");
    if (out_step < (size_t)cols * elem_size(dtype_out))
        return fail(ctx, HSFLOW_ERR_ARG, "output step %zu < row bytes", out_step);
    if (window < 1 || window > HSFLOW_MAX_WINDOW)
        return fail(ctx, HSFLOW_ERR_ARG, "windowSize %d outside [1, %d]", window,
                    HSFLOW_MAX_WINDOW);
    if (iters < 0) return fail(ctx, HSFLOW_ERR_ARG, "maxIterations %d < 0", iters);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)rows * cols;
    // [bgr0 bgr1] back to back (one batch-2 launch), then [gray0 gray1]
    const size_t gray_off = align_up(6 * n);
    int rc;
    if ((rc = grow(ctx, &ctx->d_in, &ctx->d_in_bytes, gray_off + align_up(2 * n)))) return rc;
    if ((rc = grow(ctx, &ctx->d_out, &ctx->d_out_bytes, align_up(n * 4) * 3))) return rc;
    if ((rc = grow(ctx, &ctx->d_ws, &ctx->d_ws_bytes, hsflow_workspace_bytes(rows, cols, 1))))
        return rc;
    uint8_t *db = (uint8_t *)ctx->d_in, *dg = db + gray_off;
    if ((rc = upload_pair(ctx, bgr0, bgr1, 3, rows, cols, bgr_step0, bgr_step1, db, db + 3 * n)))
        return rc;
    hipError_t e = hsflow::launch_bgr2gray(db, rows, cols, 2, dg, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "bgr2gray launch");
    float *du = (float *)ctx->d_out, *dv = (float *)((char *)du + align_up(n * 4));
    rc = cold_solve(ctx, dg, dg + n, HSFLOW_U8, rows, cols, 1, window, iters, (float)alpha,
                    false, du, dv, ctx->d_ws, ctx->d_ws_bytes, ctx->stream);
    if (rc) return rc;
    {
        const float *srcs[2] = {du, dv};
        void *dsts[2] = {u, v};
        if ((rc = download_planes(ctx, srcs, dsts, 2, rows, cols, dtype_out, out_step)))
            return rc;
    }
    return HSFLOW_OK;
}

int hsflow_gradients(hsflow_ctx *ctx, const void *I0, const void *I1, int dtype_in,
                     int rows, int cols, size_t in_step0, size_t in_step1, void *gx,
                     void *gy, void *gt, int dtype_out, size_t out_step) {
    int rc = check_host_args(ctx, I0, I1, dtype_in, rows, cols, in_step0, in_step1,
                             dtype_out, out_step);
    if (rc) return rc;
    if (!gx || !gy || !gt) return fail(ctx, HSFLOW_ERR_ARG, "null output");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)rows * cols;
    const size_t in_es = (size_t)dev_elem_size(dtype_in);
    if ((rc = grow(ctx, &ctx->d_in, &ctx->d_in_bytes, align_up(n * in_es) * 2))) return rc;
    if ((rc = grow(ctx, &ctx->d_out, &ctx->d_out_bytes, align_up(n * 4) * 3))) return rc;
    const size_t wsb = hsflow_workspace_bytes(rows, cols, 1);
    if ((rc = grow(ctx, &ctx->d_ws, &ctx->d_ws_bytes, wsb))) return rc;
    char *in0 = (char *)ctx->d_in, *in1 = in0 + align_up(n * in_es);
    float *dx = (float *)ctx->d_out;
    float *dy = (float *)((char *)dx + align_up(n * 4));
    float *dt = (float *)((char *)dy + align_up(n * 4));
    if ((rc = upload_pair(ctx, I0, I1, (int)in_es, rows, cols, in_step0, in_step1, in0, in1)))
        return rc;
    const int dt0 = dtype_in;
    rc = gradients_impl(ctx, in0, in1, dt0, rows, cols, 1, dx, dy, dt, ctx->d_ws,
                        ctx->d_ws_bytes, ctx->stream);
    if (rc) return rc;
    {
        const float *srcs[3] = {dx, dy, dt};
        void *dsts[3] = {gx, gy, gt};
        if ((rc = download_planes(ctx, srcs, dsts, 3, rows, cols, dtype_out, out_step)))
            return rc;
    }
    return HSFLOW_OK;
}

}  // extern "C"
