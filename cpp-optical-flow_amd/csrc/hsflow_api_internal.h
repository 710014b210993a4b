// hsflow_api_internal.h -- what the two host C-ABI sources share
// (hsflow_api.cpp: contexts, the Jacobi and pyramid solves, host I/O;
// hsflow_api_warped.cpp: the warped family).  No .hip file includes it.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/hsflow.h"
#include "hsflow_internal.h"

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
    // hsflow_ctx_set_finest_level: the last pyramid level the same calls solve
    // (0: the full frame, the default)
    int finest = 0;
    // hsflow_ctx_set_projection: 1: the interpolating host calls carry the
    // flows to each time first (KS, KIP); 0, the default: KI as it is
    int projection = 0;
    // hsflow_ctx_set_fallback: what the interpolating host calls do with a pair
    // whose flows fail the check (mode 0, the default: nothing).  last_cut: the
    // verdict of the last such call, -1 where there is none; cut_byte: where
    // that call's verdict lands ahead of the drain
    hsflow_fallback fb{HSFLOW_FALLBACK_OFF, 0.0f};
    int last_cut = -1;
    uint8_t cut_byte = 0;
    // hsflow_ctx_set_temporal: sequence mode of the bidirectional host-buffer
    // calls.  d_pred (grow-only) holds KP's four planes uf, vf, ub, vb of the
    // last such call, each align_up(pred_rows * pred_cols * 4) bytes;
    // pred_valid: they are the start of the next call of that size
    int temporal = 0;
    void *d_pred = nullptr;
    size_t d_pred_bytes = 0;
    int pred_rows = 0, pred_cols = 0;
    bool pred_valid = false;
};

namespace hsflow::host {

// sets the context's error text (the calling thread's for a null context)
int fail(hsflow_ctx *ctx, int code, const char *fmt, ...);
int hip_fail(hsflow_ctx *ctx, hipError_t e, const char *what);

#define HIP_TRY(ctx, expr)                                    \
    do {                                                      \
        hipError_t e_ = (expr);                               \
        if (e_ != hipSuccess) return hip_fail(ctx, e_, #expr); \
    } while (0)

constexpr size_t kAlign = 256;
inline size_t align_up(size_t x) { return (x + kAlign - 1) / kAlign * kAlign; }

// Largest frame: 2^29 - 4 pixels.  The Jacobi kernels (K2, K2w, K4, KJ) give a
// lane outside the image the byte offset kOOB = 0x7FFFFFF0 into raw buffers of
// rows * cols * 4 bytes and rely on the range check there to read 0 and drop
// the store (the zero border).  A plane of more bytes than kOOB holds that
// offset: every such load would return its element 2^29 - 4 and every such
// store overwrite it.  So the cap is the sentinel over the element size; the
// two change together (tests/test_plane_cap.py).
constexpr long long kJacobiOobOffset = 0x7FFFFFF0;
constexpr long long kMaxPlanePixels = kJacobiOobOffset / 4;

// Largest batch: pairs index gridDim.y / gridDim.z of the kernels (65535);
// tallest plane: the 64 x 4 per-pixel kernels put rows / 4 in gridDim.y.
constexpr int kMaxBatch = 65535;
constexpr int kMaxRows = 4 * 65535;

inline bool sizes_ok(int rows, int cols, int batch) {
    return rows >= 1 && rows <= kMaxRows && cols >= 1 && batch >= 1 &&
           batch <= kMaxBatch && (long long)rows * cols <= kMaxPlanePixels;
}

// "bad size", "levels outside", "device input dtype": the checks of a device
// call's shape, each with its one text
int check_sizes(hsflow_ctx *ctx, int rows, int cols, int batch);
int check_levels(hsflow_ctx *ctx, int levels);
int check_device_dtype(hsflow_ctx *ctx, int dtype_in);
int check_workspace(hsflow_ctx *ctx, size_t ws_bytes, size_t need);

// byte ranges [a, a + na) and [b, b + nb) share a byte (a null range: none)
inline bool bytes_overlap(const void *a, size_t na, const void *b, size_t nb) {
    if (!a || !b) return false;
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

// The Jacobi workspace of `batch` pairs, carved from `base`.
struct Workspace {
    uint32_t *gpack;
    float *gx, *gy, *gt, *u2, *v2;
    uint32_t *flags;
    size_t bytes;
};
Workspace carve(void *base, int rows, int cols, int batch);

int elem_size(int dtype);

// Two dense batch frames of one type: a solve's input.  As jacobi_impl's
// `fr`: the frames of a cold solve whose first pass has K1 fused in; null for
// every other solve: the workspace then holds K1's outputs already.
struct Frames {
    const void *I0, *I1;
    int dtype;
};

// One level's Jacobi iterations.  warm: from the (u, v) given, else from zero;
// maybe_f32: some pair's gradients may be in the f32 planes (the workspace's
// flags say which), so the f32 variant of the pass is launched too.
struct JacobiSpec {
    int rows, cols, batch, window, iters;
    float alpha;
    bool warm, maybe_f32;
};

// `g`: the weights of the flow-driven smoothness term (batch planes, as u and
// v); then the passes are KJ's weighted ones (always warm, f32 planes), else
// the plain Jacobi passes.
int jacobi_impl(hsflow_ctx *ctx, const JacobiSpec &J, float *u, float *v, void *workspace,
                size_t ws_bytes, hipStream_t s, const Frames *fr, const float *g);
int check_window_iters(hsflow_ctx *ctx, int window, int iters);
int check_jacobi_args(hsflow_ctx *ctx, const JacobiSpec &J, const float *u, const float *v,
                      void *workspace, size_t ws_bytes);
// K1 into the workspace; the f32 planes also to gx, gy, gt where given
int gradients_impl(hsflow_ctx *ctx, const Frames &fr, int rows, int cols, int batch, float *gx,
                   float *gy, float *gt, void *workspace, size_t ws_bytes, hipStream_t s);

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
PyrLayout pyr_layout(int rows, int cols, int batch, int levels);
// Levels 1..levels-1 of both frames into the workspace (layout L).
int build_levels(hsflow_ctx *ctx, const Frames &fr, int rows, int cols, int batch,
                 const PyrLayout &L, void *ws, hipStream_t s);

// ---- the host-buffer forms ----------------------------------------------------
int grow(hsflow_ctx *ctx, void **p, size_t *have, size_t need);
int upload_pair(hsflow_ctx *ctx, const void *I0, const void *I1, int elem, int rows, int cols,
                size_t step0, size_t step1, void *dst0, void *dst1);
// What every host form does once its arguments are checked: the context's
// device current, its buffers grown (d_in to two frames of `elem` bytes per
// pixel, each 256-byte aligned; d_out and d_ws to the given sizes) and both
// frames uploaded to *in0 and *in1.
int stage_pair(hsflow_ctx *ctx, const void *I0, const void *I1, int elem, int rows, int cols,
               size_t step0, size_t step1, size_t out_bytes, size_t ws_bytes, char **in0,
               char **in1);
int download_planes(hsflow_ctx *ctx, const float *const *src, void *const *dst, int n, int rows,
                    int cols, int dtype_out, size_t step);
int check_host_args(hsflow_ctx *ctx, const void *I0, const void *I1, int dtype_in, int rows,
                    int cols, size_t step0, size_t step1, int dtype_out, size_t out_step);

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

}  // namespace hsflow::host
