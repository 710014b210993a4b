// hsflow_api_warped.cpp -- the warped family of the C ABI in include/hsflow.h:
// the warped coarse-to-fine solve, the median and the smoothness weights
// between its warps, the bidirectional solve with its consistency check, the
// prefilter in front of them, and the frame warp and frame interpolation
// (grey and BGR) behind them, with the fallback for a pair whose flows fail,
// and the same interpolation for YUV 4:2:0 frames (the grey call on the luma,
// KIY on the chroma).
//
// Every solve of the family is described by one SolveSpec, filled once in the
// extern "C" entry point and passed down by reference; check_solve checks it,
// solve_frames produces the frames the solve runs on, warped_run is the solve.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "hsflow_api_internal.h"

using namespace hsflow::host;

namespace {

// ---- what a call of the family is asked for ----------------------------------
struct SolveSpec {
    int rows, cols, batch, levels;
    int finest;  // the last level solved; its flow goes up to level 0 bilinearly
    int warps, median, window, iters;
    float alpha;
    const hsflow_prefilter *pf;   // null or mode 0: the frames as they are
    const hsflow_smoothness *sm;  // null or mode 0: the quadratic term
    const hsflow_flow_init *init;  // null or no plane: every solve starts cold
    // the interpolating calls: 0, KI on the flows at the output pixel; 1, KS
    // carries the flows to each time first and KIP reads them there
    int projection;
    // the interpolating calls: null or mode 0, nothing; else KF replaces the
    // frames of every pair whose flows fail the check
    const hsflow_fallback *fb;
};

// the outputs of one direction's consistency check (KC); each may be null
struct CheckOut {
    float *err;
    uint8_t *mask;
    uint32_t *counts;
};

// the bidirectional solve's outputs and the thresholds of its checks
struct BidirOut {
    float *uf, *vf, *ub, *vb;
    CheckOut f, b;
    float rel, abs_thr;
};

// the flows and masks an interpolation (KI, KIC) reads; the masks may be null.
// cells: KS's plane, for the projected interpolation (KIP); null: KI, KIC
struct FlowsIn {
    const float *uf, *vf, *ub, *vb;
    const uint8_t *mask_f, *mask_b;
    const uint64_t *cells;
};

// ... and what it writes: nt frames at `times` (host), flags and trusted; the
// calls with a fallback also the verdict per pair
struct InterpOut {
    const float *times;
    int nt;
    void *out;
    int dtype_out;
    uint8_t *flags;
    uint32_t *trusted;
    uint8_t *cut;
};

// the host form's: one host plane per time
struct HostInterpOut {
    const float *times;
    int nt;
    void *const *out;
    int dtype_out;
    size_t out_step;
    uint8_t *const *flags;
    size_t flags_step;
    uint32_t *trusted;
};

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

// the two f32 planes a prefiltered solve keeps behind its own workspace
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

// KN alone
int prefilter_impl(hsflow_ctx *ctx, const void *I, int dtype_in, int rows, int cols, int batch,
                   const hsflow_prefilter *pf, float *out, hipStream_t s) {
    PfPlan P;
    int rc = plan_prefilter(ctx, pf, &P);
    if (rc || (rc = check_sizes(ctx, rows, cols, batch)) ||
        (rc = check_device_dtype(ctx, dtype_in)))
        return rc;
    if (!I || !out) return fail(ctx, HSFLOW_ERR_ARG, "null device pointer");
    const size_t n = (size_t)rows * cols * batch;
    if (bytes_overlap(I, n * elem_size(dtype_in), out, n * 4))
        return fail(ctx, HSFLOW_ERR_ARG, "prefilter output overlaps the input");
    return prefilter_run(ctx, I, dtype_in, rows, cols, batch, P, out, s);
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

// KG alone
int diffusivity_impl(hsflow_ctx *ctx, const float *u, const float *v, int rows, int cols,
                     int batch, float lambda, float *g, hipStream_t s) {
    const hsflow_smoothness sm{HSFLOW_SMOOTH_FLOW_DRIVEN, lambda};
    int rc = check_smoothness(ctx, &sm);
    if (rc || (rc = check_sizes(ctx, rows, cols, batch))) return rc;
    if (!u || !v || !g) return fail(ctx, HSFLOW_ERR_ARG, "null device pointer");
    const size_t pb = (size_t)rows * cols * batch * 4;
    const ByteRange in[2] = {{u, pb}, {v, pb}}, out{g, pb};
    if (!outputs_disjoint(in, 2, &out, 1))
        return fail(ctx, HSFLOW_ERR_ARG, "the weights overlap the flow");
    hipError_t e = hsflow::launch_diffusivity(u, v, rows, cols, batch, lambda, g, s);
    if (e != hipSuccess) return hip_fail(ctx, e, "diffusivity launch");
    return HSFLOW_OK;
}

// KJ alone: J.iters weighted iterations from the workspace's f32 planes
int jacobi_weighted_impl(hsflow_ctx *ctx, const JacobiSpec &J, const float *g, float *u, float *v,
                         void *workspace, size_t ws_bytes, hipStream_t s) {
    if (J.window != 3 && J.window != 5)
        return fail(ctx, HSFLOW_ERR_ARG, "weighted iterations need windowSize 3 or 5, not %d",
                    J.window);
    int rc = check_jacobi_args(ctx, J, u, v, workspace, ws_bytes);
    if (rc) return rc;
    if (!g) return fail(ctx, HSFLOW_ERR_ARG, "null device pointer");
    const size_t pb = (size_t)J.rows * J.cols * J.batch * 4;
    const ByteRange w{workspace, carve(workspace, J.rows, J.cols, J.batch).bytes};
    const ByteRange planes[3] = {{g, pb}, {u, pb}, {v, pb}};
    if (!outputs_disjoint(&w, 1, planes, 3))
        return fail(ctx, HSFLOW_ERR_ARG,
                    "the weights, the flow and the workspace overlap each other");
    return jacobi_impl(ctx, J, u, v, workspace, ws_bytes, s, nullptr, g);
}

// ---- median filtering of the flow between warps ----------------------------
int median_impl(hsflow_ctx *ctx, const float *u, const float *v, int rows, int cols, int batch,
                int ksize, float *u_out, float *v_out, hipStream_t s) {
    if (ksize != 3 && ksize != 5)
        return fail(ctx, HSFLOW_ERR_ARG, "median size %d is not 3 or 5", ksize);
    int rc = check_sizes(ctx, rows, cols, batch);
    if (rc) return rc;
    if (!u || !v || !u_out || !v_out) return fail(ctx, HSFLOW_ERR_ARG, "null device pointer");
    const size_t pb = (size_t)rows * cols * batch * 4;
    const ByteRange in[2] = {{u, pb}, {v, pb}}, outs[2] = {{u_out, pb}, {v_out, pb}};
    if (!outputs_disjoint(in, 2, outs, 2))
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

// ---- the checks of a solve ----------------------------------------------------
constexpr int kMaxWarps = 16;

// warps, window, iterations and the median: what the host forms check before
// they upload (the rest of check_solve follows on the device copies)
int check_iteration_args(hsflow_ctx *ctx, const SolveSpec &S) {
    if (S.warps < 1 || S.warps > kMaxWarps)
        return fail(ctx, HSFLOW_ERR_ARG, "warps %d outside [1, %d]", S.warps, kMaxWarps);
    int rc = check_window_iters(ctx, S.window, S.iters);
    if (rc) return rc;
    if (S.median != 0 && S.median != 3 && S.median != 5)  // 0 = none, else KM's size
        return fail(ctx, HSFLOW_ERR_ARG, "median %d is not 0, 3 or 5", S.median);
    return HSFLOW_OK;
}

// the finest level solved, against levels (checked before it)
int check_finest(hsflow_ctx *ctx, const SolveSpec &S) {
    if (S.finest < 0 || S.finest >= S.levels)
        return fail(ctx, HSFLOW_ERR_ARG, "finest level %d outside [0, levels - 1 = %d]", S.finest,
                    S.levels - 1);
    return HSFLOW_OK;
}

// Everything a spec says, in the one order every call of the family reports
// it: the prefilter (planned into *P when on), warps / window / iterations,
// the median, the smoothness and the window it needs, levels, the finest
// level, sizes, and the frames' type.  Null pointers, thresholds and the workspace's size follow in
// the caller, each through its one routine.
// u16: a call that takes 16-bit frames (the YUV 4:2:0 ones), which every other
// call refuses with the text it always had.
int check_solve(hsflow_ctx *ctx, const SolveSpec &S, int dtype_in, PfPlan *P, bool u16 = false) {
    int rc = pf_on(S.pf) ? plan_prefilter(ctx, S.pf, P) : HSFLOW_OK;
    if (rc || (rc = check_iteration_args(ctx, S))) return rc;
    if (sm_on(S.sm)) {
        if ((rc = check_smoothness(ctx, S.sm))) return rc;
        if (S.window != 3 && S.window != 5)  // the sizes KJ is built for
            return fail(ctx, HSFLOW_ERR_ARG,
                        "flow-driven smoothness needs windowSize 3 or 5, not %d", S.window);
    }
    if ((rc = check_levels(ctx, S.levels)) || (rc = check_finest(ctx, S)) ||
        (rc = check_sizes(ctx, S.rows, S.cols, S.batch)))
        return rc;
    if (u16 && dtype_in == HSFLOW_U16) return HSFLOW_OK;
    return check_device_dtype(ctx, dtype_in);
}

int null_pointer(hsflow_ctx *ctx) { return fail(ctx, HSFLOW_ERR_ARG, "null device pointer"); }

// thresholds of the consistency check: finite and >= 0 (negated, so NaN fails)
int check_thresholds(hsflow_ctx *ctx, float rel, float abs_thr) {
    if (!(rel >= 0.0f && rel <= 3.0e38f) || !(abs_thr >= 0.0f && abs_thr <= 3.0e38f))
        return fail(ctx, HSFLOW_ERR_ARG, "thresholds rel %g, abs %g must be finite and >= 0",
                    (double)rel, (double)abs_thr);
    return HSFLOW_OK;
}

// ---- temporal warm start: the start of a solve --------------------------------
// the workspace a call whose own layout takes `own` bytes needs
size_t ws_need(const SolveSpec &S, size_t own) {
    return pf_on(S.pf) ? align_up(own) + pf_planes_bytes(S.rows, S.cols, S.batch) : own;
}

// some solve of the call starts from a given flow: the forward one, or for a
// bidirectional call (`bidir`) the backward one
bool init_on(const SolveSpec &S, bool bidir) {
    return S.init && (S.init->uf || (bidir && S.init->ub));
}

// The init's checks, the last of a call's: whole pairs, and where one is
// given the workspace's size first, then the planes against the outputs and
// the `need` bytes of the workspace.  The warped call reads only (uf, vf).
int check_init(hsflow_ctx *ctx, const SolveSpec &S, bool bidir, const ByteRange *outs, int n_outs,
               const void *ws, size_t ws_bytes, size_t need) {
    const hsflow_flow_init *in = S.init;
    if (!in) return HSFLOW_OK;
    if (!in->uf != !in->vf || (bidir && !in->ub != !in->vb))
        return fail(ctx, HSFLOW_ERR_ARG, "init flow: one plane of a pair without the other");
    if (!init_on(S, bidir)) return HSFLOW_OK;
    int rc = check_workspace(ctx, ws_bytes, need);
    if (rc) return rc;
    const size_t pb = (size_t)S.rows * S.cols * S.batch * 4;
    const ByteRange planes[4] = {{in->uf, pb}, {in->vf, pb}, {bidir ? in->ub : nullptr, pb},
                                 {bidir ? in->vb : nullptr, pb}};
    for (const ByteRange &p : planes) {
        if (bytes_overlap(p.p, p.n, ws, need))
            return fail(ctx, HSFLOW_ERR_ARG, "init flow overlaps the workspace");
        for (int o = 0; o < n_outs; ++o)
            if (bytes_overlap(p.p, p.n, outs[o].p, outs[o].n))
                return fail(ctx, HSFLOW_ERR_ARG, "init flow overlaps an output");
    }
    return HSFLOW_OK;
}

// KD alone
int downflow_impl(hsflow_ctx *ctx, const float *u, const float *v, int rows, int cols, float *uc,
                  float *vc, int rc, int cc, int batch, hipStream_t s) {
    int bad = check_sizes(ctx, rows, cols, batch);
    if (bad) return bad;
    if (!u || !v || !uc || !vc) return null_pointer(ctx);
    if (rc != (rows + 1) / 2 || cc != (cols + 1) / 2)
        return fail(ctx, HSFLOW_ERR_ARG, "level size %dx%d is not %dx%d, the next level of %dx%d",
                    rc, cc, (rows + 1) / 2, (cols + 1) / 2, rows, cols);
    const size_t pb = (size_t)rows * cols * batch * 4, cb = (size_t)rc * cc * batch * 4;
    const ByteRange in[2] = {{u, pb}, {v, pb}}, outs[2] = {{uc, cb}, {vc, cb}};
    if (!outputs_disjoint(in, 2, outs, 2))
        return fail(ctx, HSFLOW_ERR_ARG, "downflow outputs overlap the inputs or each other");
    hipError_t e = hsflow::launch_downflow(u, v, rows, cols, uc, vc, rc, cc, batch, s);
    if (e != hipSuccess) return hip_fail(ctx, e, "downflow launch");
    return HSFLOW_OK;
}

// KB alone
int upflow_bilinear_impl(hsflow_ctx *ctx, const float *uc, const float *vc, int rc, int cc,
                         float *u, float *v, int rows, int cols, int batch, hipStream_t s) {
    int bad = check_sizes(ctx, rows, cols, batch);
    if (bad) return bad;
    if (!uc || !vc || !u || !v) return null_pointer(ctx);
    if (rc != (rows + 1) / 2 || cc != (cols + 1) / 2)
        return fail(ctx, HSFLOW_ERR_ARG, "level size %dx%d is not %dx%d, the next level of %dx%d",
                    rc, cc, (rows + 1) / 2, (cols + 1) / 2, rows, cols);
    const size_t pb = (size_t)rows * cols * batch * 4, cb = (size_t)rc * cc * batch * 4;
    const ByteRange in[2] = {{uc, cb}, {vc, cb}}, outs[2] = {{u, pb}, {v, pb}};
    if (!outputs_disjoint(in, 2, outs, 2))
        return fail(ctx, HSFLOW_ERR_ARG,
                    "bilinear upflow outputs overlap the inputs or each other");
    hipError_t e = hsflow::launch_upflow_bilinear(uc, vc, rc, cc, u, v, rows, cols, batch, s);
    if (e != hipSuccess) return hip_fail(ctx, e, "bilinear upflow launch");
    return HSFLOW_OK;
}

// KP alone
int predict_impl(hsflow_ctx *ctx, const float *ub, const float *vb, int rows, int cols, int batch,
                 float *uf_next, float *vf_next, float *ub_next, float *vb_next, hipStream_t s) {
    int rc = check_sizes(ctx, rows, cols, batch);
    if (rc) return rc;
    if (!ub || !vb) return null_pointer(ctx);
    if (!uf_next != !vf_next || !ub_next != !vb_next)
        return fail(ctx, HSFLOW_ERR_ARG, "predict: one plane of an output pair without the other");
    if (!uf_next && !ub_next)
        return fail(ctx, HSFLOW_ERR_ARG, "no output: both predicted pairs are null");
    const size_t pb = (size_t)rows * cols * batch * 4;
    const ByteRange in[2] = {{ub, pb}, {vb, pb}};
    const ByteRange outs[4] = {{uf_next, pb}, {vf_next, pb}, {ub_next, pb}, {vb_next, pb}};
    if (!outputs_disjoint(in, 2, outs, 4))
        return fail(ctx, HSFLOW_ERR_ARG, "predicted flows overlap the inputs or each other");
    hipError_t e = hsflow::launch_flow_predict(ub, vb, rows, cols, batch, uf_next, vf_next,
                                               ub_next, vb_next, s);
    if (e != hipSuccess) return hip_fail(ctx, e, "flow predict launch");
    return HSFLOW_OK;
}

// ---- sequence mode of the bidirectional host-buffer calls ----------------------
size_t pred_plane_bytes(int rows, int cols) { return align_up((size_t)rows * cols * 4); }

void pred_planes(const hsflow_ctx *ctx, int rows, int cols, float **p) {
    for (int k = 0; k < 4; ++k)
        p[k] = (float *)((char *)ctx->d_pred + k * pred_plane_bytes(rows, cols));
}

// The stored prediction leaves the context, whatever the call does next (a
// failed call drops it); where the mode is on and it has the call's size, it
// is the call's start.
bool take_prediction(hsflow_ctx *ctx, int rows, int cols, hsflow_flow_init *init) {
    const bool fits = ctx->temporal && ctx->pred_valid && ctx->pred_rows == rows &&
                      ctx->pred_cols == cols;
    ctx->pred_valid = false;
    if (!fits) return false;
    float *p[4];
    pred_planes(ctx, rows, cols, p);
    *init = hsflow_flow_init{p[0], p[1], p[2], p[3]};
    return true;
}

// the context's four planes, large enough for this size (the device is current)
int grow_prediction(hsflow_ctx *ctx, int rows, int cols) {
    if (!ctx->temporal) return HSFLOW_OK;
    return grow(ctx, &ctx->d_pred, &ctx->d_pred_bytes, 4 * pred_plane_bytes(rows, cols));
}

// KP of the solve's (ub, vb) into them, on the context's stream: the solve
// that started from them has read them by then
int predict_run(hsflow_ctx *ctx, const float *ub, const float *vb, int rows, int cols) {
    if (!ctx->temporal) return HSFLOW_OK;
    float *p[4];
    pred_planes(ctx, rows, cols, p);
    hipError_t e =
        hsflow::launch_flow_predict(ub, vb, rows, cols, 1, p[0], p[1], p[2], p[3], ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "flow predict launch");
    ctx->pred_rows = rows, ctx->pred_cols = cols;
    return HSFLOW_OK;
}

// the call has succeeded: its prediction is the next call's start
int keep_prediction(hsflow_ctx *ctx, int rc) {
    if (!rc && ctx->temporal) ctx->pred_valid = true;
    return rc;
}

// The frames the solve sees, for a call whose own workspace layout is the
// first `own` bytes of ws: the workspace's size with the prefilter's planes
// behind that layout, the frames against the workspace (they must not share a
// byte with planes that are written while they are still to be read), then
// for BGR frames (`grey`: where their two grey planes go; null for grey
// frames) bgr2gray, and with the prefilter on KN of both into the two planes.
// *F: those planes as f32, non-integral frames, else the grey planes, else
// the frames themselves.  The caller has checked the spec and the pointers.
int solve_frames(hsflow_ctx *ctx, const SolveSpec &S, const PfPlan &P, const Frames &in,
                 uint8_t *const *grey, void *ws, size_t ws_bytes, size_t own, Frames *F,
                 hipStream_t s) {
    const bool pf = pf_on(S.pf);
    const size_t n = (size_t)S.rows * S.cols * S.batch;
    const size_t need = ws_need(S, own);
    int rc = check_workspace(ctx, ws_bytes, need);
    if (rc) return rc;
    const size_t fb = n * (grey ? 3 : elem_size(in.dtype));
    if ((pf || grey) && (bytes_overlap(in.I0, fb, ws, need) || bytes_overlap(in.I1, fb, ws, need)))
        return fail(ctx, HSFLOW_ERR_ARG, "the frames overlap the workspace");
    *F = in;
    if (grey) {
        hipError_t e = hsflow::launch_bgr2gray((const uint8_t *)in.I0, S.rows, S.cols, S.batch,
                                               grey[0], s);
        if (e == hipSuccess)
            e = hsflow::launch_bgr2gray((const uint8_t *)in.I1, S.rows, S.cols, S.batch, grey[1], s);
        if (e != hipSuccess) return hip_fail(ctx, e, "bgr2gray launch");
        *F = Frames{grey[0], grey[1], HSFLOW_U8};
    }
    if (!pf) return HSFLOW_OK;
    float *p0 = (float *)((char *)ws + align_up(own));
    float *p1 = (float *)((char *)p0 + align_up(n * 4));
    if ((rc = prefilter_run(ctx, F->I0, F->dtype, S.rows, S.cols, S.batch, P, p0, s))) return rc;
    if ((rc = prefilter_run(ctx, F->I1, F->dtype, S.rows, S.cols, S.batch, P, p1, s))) return rc;
    *F = Frames{p0, p1, HSFLOW_F32};
    return HSFLOW_OK;
}

// ---- warped coarse-to-fine solve -------------------------------------------
// KW: one level's gradients linearised around (u0, v0), into the Jacobi
// workspace's f32 planes (flags[pair] = 1: the passes read the planes).
int warp_gradients_run(hsflow_ctx *ctx, const Frames &fr, int rows, int cols, int batch,
                       const float *u0, const float *v0, void *workspace, hipStream_t s) {
    const Workspace w = carve(workspace, rows, cols, batch);
    hipError_t e = hsflow::launch_warp_gradients(fr.I0, fr.I1, fr.dtype, rows, cols, batch, u0, v0,
                                                 w.gx, w.gy, w.gt, w.flags, s);
    if (e != hipSuccess) return hip_fail(ctx, e, "warp gradients launch");
    return HSFLOW_OK;
}

// ... and copies of the planes to out[0..2] (gx, gy, gt) where given
int warp_gradients_impl(hsflow_ctx *ctx, const Frames &fr, int rows, int cols, int batch,
                        const float *u0, const float *v0, float *const *out, void *workspace,
                        size_t ws_bytes, hipStream_t s) {
    int rc = check_sizes(ctx, rows, cols, batch);
    if (rc || (rc = check_device_dtype(ctx, fr.dtype))) return rc;
    if (!fr.I0 || !fr.I1 || !u0 || !v0 || !workspace) return null_pointer(ctx);
    const Workspace w = carve(workspace, rows, cols, batch);
    if ((rc = check_workspace(ctx, ws_bytes, w.bytes))) return rc;
    if ((rc = warp_gradients_run(ctx, fr, rows, cols, batch, u0, v0, workspace, s))) return rc;
    const size_t n = (size_t)rows * cols * batch;
    const float *planes[3] = {w.gx, w.gy, w.gt};
    for (int k = 0; k < 3; ++k)
        if (out[k])
            HIP_TRY(ctx, hipMemcpyAsync(out[k], planes[k], n * 4, hipMemcpyDeviceToDevice, s));
    return HSFLOW_OK;
}

// The solve itself, on checked arguments.  The pyramid of the plain pyramid
// solve; per level, coarsest first: (u, v) = 0 or the coarser result projected
// up, then S.warps times KW around the current (u, v), S.iters Jacobi
// iterations warm-started from it and, for S.median != 0, KM (median x median)
// on the level's (u, v).  median = 0 launches exactly what the solve without
// the filter always has.  With a smoothness mode on, KG turns each warp's
// (u, v) into weights -- in the Jacobi workspace's packed gradient plane, which
// a warped solve never reads (KW sets flags[pair] = 1) -- and the iterations
// are KJ's weighted ones; off, the launches are unchanged.  (iu, iv): the
// start at full resolution, both or neither: KD takes it level by level into
// the workspace's per-level (u, v) planes -- upflow overwrites all but the
// coarsest later -- and the coarsest level starts from the last of them
// instead of zero (levels = 1: from a copy); null launches what it always has.
// S.finest > 0: the levels below it are not solved; KB takes the flow of level
// S.finest up through their sizes, one launch per level, into their per-level
// planes -- which nothing else uses once the init is reduced -- and at last
// into (u, v), which that launch alone writes.  S.finest = 0 launches what the
// solve always has.
int warped_run(hsflow_ctx *ctx, const SolveSpec &S, const Frames &F, float *u, float *v,
               const float *iu, const float *iv, void *ws, hipStream_t s) {
    const int batch = S.batch, levels = S.levels;
    const PyrLayout L = pyr_layout(S.rows, S.cols, batch, levels);
    char *base = (char *)ws;
    int rc = build_levels(ctx, F, S.rows, S.cols, batch, L, ws, s);
    if (rc) return rc;
    if (iu && levels == 1) {
        const size_t n = (size_t)S.rows * S.cols * batch;
        HIP_TRY(ctx, hipMemcpyAsync(u, iu, n * 4, hipMemcpyDeviceToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(v, iv, n * 4, hipMemcpyDeviceToDevice, s));
    }
    for (int l = 1; iu && l < levels; ++l) {
        float *ul = (float *)(base + L.off[l][2]), *vl = (float *)(base + L.off[l][3]);
        hipError_t e = hsflow::launch_downflow(iu, iv, L.R[l - 1], L.C[l - 1], ul, vl, L.R[l],
                                               L.C[l], batch, s);
        if (e != hipSuccess) return hip_fail(ctx, e, "downflow launch");
        iu = ul, iv = vl;
    }
    for (int l = levels - 1; l >= S.finest; --l) {
        float *ul = l ? (float *)(base + L.off[l][2]) : u;
        float *vl = l ? (float *)(base + L.off[l][3]) : v;
        const size_t n = (size_t)L.R[l] * L.C[l] * batch;
        if (l == levels - 1) {
            if (!iu) {
                HIP_TRY(ctx, hipMemsetAsync(ul, 0, n * 4, s));
                HIP_TRY(ctx, hipMemsetAsync(vl, 0, n * 4, s));
            }
        } else {
            hipError_t e = hsflow::launch_upflow(
                (const float *)(base + L.off[l + 1][2]), (const float *)(base + L.off[l + 1][3]),
                L.R[l + 1], L.C[l + 1], ul, vl, L.R[l], L.C[l], batch, s);
            if (e != hipSuccess) return hip_fail(ctx, e, "upflow launch");
        }
        const Frames fl = l ? Frames{base + L.off[l][0], base + L.off[l][1], HSFLOW_F32} : F;
        // warm; maybe_f32: the planes are f32 for every pair
        const JacobiSpec J{L.R[l], L.C[l], batch, S.window, S.iters, S.alpha, true, true};
        for (int k = 0; k < S.warps; ++k) {
            if ((rc = warp_gradients_run(ctx, fl, L.R[l], L.C[l], batch, ul, vl, ws, s))) return rc;
            float *g = nullptr;
            if (sm_on(S.sm)) {
                g = (float *)carve(ws, L.R[l], L.C[l], batch).gpack;
                hipError_t e = hsflow::launch_diffusivity(ul, vl, L.R[l], L.C[l], batch,
                                                          S.sm->lambda, g, s);
                if (e != hipSuccess) return hip_fail(ctx, e, "diffusivity launch");
            }
            if ((rc = jacobi_impl(ctx, J, ul, vl, ws, L.jac_bytes, s, nullptr, g))) return rc;
            if (S.median) {
                rc = median_in_place(ctx, ul, vl, L.R[l], L.C[l], batch, S.median, ws, s);
                if (rc) return rc;
            }
        }
    }
    for (int l = S.finest - 1; l >= 0; --l) {
        hipError_t e = hsflow::launch_upflow_bilinear(
            (const float *)(base + L.off[l + 1][2]), (const float *)(base + L.off[l + 1][3]),
            L.R[l + 1], L.C[l + 1], l ? (float *)(base + L.off[l][2]) : u,
            l ? (float *)(base + L.off[l][3]) : v, L.R[l], L.C[l], batch, s);
        if (e != hipSuccess) return hip_fail(ctx, e, "bilinear upflow launch");
    }
    return HSFLOW_OK;
}

// hsflow_flow_warped*_device: with a prefilter, KN on both frames and the solve
// on the planes -- the public pieces one after the other, so the bits are
// theirs by construction.
int warped_impl(hsflow_ctx *ctx, const SolveSpec &S, const Frames &in, float *u, float *v,
                void *ws, size_t ws_bytes, hipStream_t s) {
    PfPlan P;
    int rc = check_solve(ctx, S, in.dtype, &P);
    if (rc) return rc;
    if (!in.I0 || !in.I1 || !u || !v || !ws) return null_pointer(ctx);
    const size_t own = pyr_layout(S.rows, S.cols, S.batch, S.levels).bytes;
    const size_t pb = (size_t)S.rows * S.cols * S.batch * 4;
    const ByteRange outs[2] = {{u, pb}, {v, pb}};
    if ((rc = check_init(ctx, S, false, outs, 2, ws, ws_bytes, ws_need(S, own)))) return rc;
    Frames F;
    rc = solve_frames(ctx, S, P, in, nullptr, ws, ws_bytes, own, &F, s);
    if (rc) return rc;
    const bool warm = init_on(S, false);
    return warped_run(ctx, S, F, u, v, warm ? S.init->uf : nullptr, warm ? S.init->vf : nullptr,
                      ws, s);
}

// ---- bidirectional warped solve + forward-backward check -------------------
// KC on checked arguments: counts zeroed stream-ordered, then one launch
int consistency_run(hsflow_ctx *ctx, const float *uf, const float *vf, const float *ub,
                    const float *vb, int rows, int cols, int batch, float rel, float abs_thr,
                    const CheckOut &o, hipStream_t s) {
    if (o.counts) HIP_TRY(ctx, hipMemsetAsync(o.counts, 0, (size_t)batch * 3 * 4, s));
    hipError_t e = hsflow::launch_consistency(uf, vf, ub, vb, rows, cols, batch, rel, abs_thr,
                                              o.err, o.mask, o.counts, s);
    if (e != hipSuccess) return hip_fail(ctx, e, "consistency launch");
    return HSFLOW_OK;
}

int consistency_impl(hsflow_ctx *ctx, const float *uf, const float *vf, const float *ub,
                     const float *vb, int rows, int cols, int batch, float rel, float abs_thr,
                     const CheckOut &o, hipStream_t s) {
    int rc = check_sizes(ctx, rows, cols, batch);
    if (rc) return rc;
    if (!uf || !vf || !ub || !vb) return null_pointer(ctx);
    if ((rc = check_thresholds(ctx, rel, abs_thr))) return rc;
    if (!o.err && !o.mask && !o.counts)
        return fail(ctx, HSFLOW_ERR_ARG, "no output: err, mask and counts are all null");
    return consistency_run(ctx, uf, vf, ub, vb, rows, cols, batch, rel, abs_thr, o, s);
}

// Both directions one after the other on the caller's stream, each the
// warped solve itself (so the flows are hsflow_flow_warped_device's bits by
// construction) in the one pyramid workspace, then KC per direction asked for.
int bidir_run(hsflow_ctx *ctx, const SolveSpec &S, const Frames &F, const BidirOut &B, void *ws,
              hipStream_t s) {
    const hsflow_flow_init none{nullptr, nullptr, nullptr, nullptr};
    const hsflow_flow_init &I = S.init ? *S.init : none;  // a null pair: that direction cold
    int rc = warped_run(ctx, S, F, B.uf, B.vf, I.uf, I.vf, ws, s);
    if (rc) return rc;
    rc = warped_run(ctx, S, Frames{F.I1, F.I0, F.dtype}, B.ub, B.vb, I.ub, I.vb, ws, s);
    if (rc) return rc;
    if (B.f.err || B.f.mask || B.f.counts) {
        rc = consistency_run(ctx, B.uf, B.vf, B.ub, B.vb, S.rows, S.cols, S.batch, B.rel,
                             B.abs_thr, B.f, s);
        if (rc) return rc;
    }
    if (B.b.err || B.b.mask || B.b.counts)
        rc = consistency_run(ctx, B.ub, B.vb, B.uf, B.vf, S.rows, S.cols, S.batch, B.rel,
                             B.abs_thr, B.b, s);
    return rc;
}

// hsflow_flow_bidir*_device; a prefilter runs once, in front of both directions
int bidir_impl(hsflow_ctx *ctx, const SolveSpec &S, const Frames &in, const BidirOut &B, void *ws,
               size_t ws_bytes, hipStream_t s) {
    PfPlan P;
    int rc = check_solve(ctx, S, in.dtype, &P);
    if (rc) return rc;
    if (!in.I0 || !in.I1 || !B.uf || !B.vf || !B.ub || !B.vb || !ws) return null_pointer(ctx);
    if ((rc = check_thresholds(ctx, B.rel, B.abs_thr))) return rc;
    const size_t own = pyr_layout(S.rows, S.cols, S.batch, S.levels).bytes;
    const size_t n = (size_t)S.rows * S.cols * S.batch, cb = (size_t)S.batch * 3 * 4;
    const ByteRange outs[10] = {{B.uf, n * 4},    {B.vf, n * 4},   {B.ub, n * 4},    {B.vb, n * 4},
                                {B.f.err, n * 4}, {B.f.mask, n},   {B.f.counts, cb},
                                {B.b.err, n * 4}, {B.b.mask, n},   {B.b.counts, cb}};
    if ((rc = check_init(ctx, S, true, outs, 10, ws, ws_bytes, ws_need(S, own)))) return rc;
    Frames F;
    rc = solve_frames(ctx, S, P, in, nullptr, ws, ws_bytes, own, &F, s);
    if (rc) return rc;
    return bidir_run(ctx, S, F, B, ws, s);
}

// ---- frame warp and frame interpolation, grey and BGR ------------------------
// KR
int warp_image_impl(hsflow_ctx *ctx, const void *I, int dtype_in, int rows, int cols, int batch,
                    const float *u, const float *v, float *out, uint8_t *oof, hipStream_t s) {
    int rc = check_sizes(ctx, rows, cols, batch);
    if (rc || (rc = check_device_dtype(ctx, dtype_in))) return rc;
    if (!I || !u || !v || !out) return null_pointer(ctx);
    const size_t n = (size_t)rows * cols * batch;
    const ByteRange in[3] = {{I, n * elem_size(dtype_in)}, {u, n * 4}, {v, n * 4}};
    const ByteRange outs[2] = {{out, n * 4}, {oof, n}};
    if (!outputs_disjoint(in, 3, outs, 2))
        return fail(ctx, HSFLOW_ERR_ARG, "warp outputs overlap the inputs or each other");
    hipError_t e = hsflow::launch_warp_image(I, dtype_in, rows, cols, batch, u, v, out, oof, s);
    if (e != hipSuccess) return hip_fail(ctx, e, "warp image launch");
    return HSFLOW_OK;
}

// KRC
int warp_image_bgr_impl(hsflow_ctx *ctx, const uint8_t *bgr, int rows, int cols, int batch,
                        const float *u, const float *v, void *out, int dtype_out, uint8_t *oof,
                        hipStream_t s) {
    int rc = check_sizes(ctx, rows, cols, batch);
    if (rc) return rc;
    if (!bgr || !u || !v || !out) return null_pointer(ctx);
    if (dtype_out != HSFLOW_F32 && dtype_out != HSFLOW_U8)
        return fail(ctx, HSFLOW_ERR_ARG, "BGR output dtype must be U8 or F32");
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

// times (host), nt and the output type of an interpolation; f64: the grey host
// form, which widens on the way down
int check_times(hsflow_ctx *ctx, const float *times, int nt) {
    if (nt < 1 || nt > HSFLOW_MAX_TIMES)
        return fail(ctx, HSFLOW_ERR_ARG, "nt %d outside [1, %d]", nt, HSFLOW_MAX_TIMES);
    if (!times) return fail(ctx, HSFLOW_ERR_ARG, "null times");
    for (int k = 0; k < nt; ++k)
        if (!(times[k] >= 0.0f && times[k] <= 1.0f))  // negated: NaN fails
            return fail(ctx, HSFLOW_ERR_ARG, "time %d (%g) outside [0, 1]", k, (double)times[k]);
    return HSFLOW_OK;
}

// u16: the output of a call on 16-bit frames, U16 or F32
int check_interp_args(hsflow_ctx *ctx, const float *times, int nt, int dtype_out, bool f64,
                      bool u16 = false) {
    const int rc = check_times(ctx, times, nt);
    if (rc) return rc;
    if (u16) {
        if (dtype_out != HSFLOW_F32 && dtype_out != HSFLOW_U16)
            return fail(ctx, HSFLOW_ERR_ARG, "16-bit output dtype must be U16 or F32");
        return HSFLOW_OK;
    }
    if (dtype_out != HSFLOW_F32 && dtype_out != HSFLOW_U8 && !(f64 && dtype_out == HSFLOW_F64))
        return fail(ctx, HSFLOW_ERR_ARG, f64 ? "output dtype must be U8, F32 or F64"
                                             : "device output dtype must be U8 or F32");
    return HSFLOW_OK;
}

// what a launch writes for a checked dtype_out
int out_kind(int dtype_out) {
    return dtype_out == HSFLOW_U8    ? hsflow::kOutU8
           : dtype_out == HSFLOW_U16 ? hsflow::kOutU16
                                     : hsflow::kOutF32;
}

// the byte ranges an interpolation of `channels`-channel frames writes
void interp_out_ranges(const InterpOut &O, size_t n, int batch, int channels, ByteRange *r) {
    r[0] = {O.out, n * O.nt * channels * elem_size(O.dtype_out)};
    r[1] = {O.flags, n * O.nt};
    r[2] = {O.trusted, (size_t)batch * O.nt * 4};
    r[3] = {O.cut, (size_t)batch};
}

// KI (channels 1: frames of fr.dtype) or KIC (channels 3: 8-bit interleaved
// BGR), or with W.cells KIP on either, on checked arguments: trusted zeroed
// stream-ordered, then one launch
int frame_interp_run(hsflow_ctx *ctx, int channels, const Frames &fr, int rows, int cols, int batch,
                     const FlowsIn &W, const InterpOut &O, hipStream_t s) {
    if (O.trusted) HIP_TRY(ctx, hipMemsetAsync(O.trusted, 0, (size_t)batch * O.nt * 4, s));
    const int kind = out_kind(O.dtype_out);
    hipError_t e;
    if (channels == 3) {
        const bool u8 = kind == hsflow::kOutU8;  // the BGR calls have no u16 output
        const uint8_t *b0 = (const uint8_t *)fr.I0, *b1 = (const uint8_t *)fr.I1;
        e = W.cells ? hsflow::launch_frame_interp_bgr_proj(b0, b1, rows, cols, batch, W.uf, W.vf,
                                                           W.ub, W.vb, W.mask_f, W.mask_b, W.cells,
                                                           O.times, O.nt, O.out, u8, O.flags,
                                                           O.trusted, s)
                    : hsflow::launch_frame_interp_bgr(b0, b1, rows, cols, batch, W.uf, W.vf, W.ub,
                                                      W.vb, W.mask_f, W.mask_b, O.times, O.nt,
                                                      O.out, u8, O.flags, O.trusted, s);
        if (e != hipSuccess) return hip_fail(ctx, e, "BGR frame interpolation launch");
        return HSFLOW_OK;
    }
    e = W.cells ? hsflow::launch_frame_interp_proj(fr.I0, fr.I1, fr.dtype, rows, cols, batch, W.uf,
                                                   W.vf, W.ub, W.vb, W.mask_f, W.mask_b, W.cells,
                                                   O.times, O.nt, O.out, kind, O.flags, O.trusted,
                                                   s)
                : hsflow::launch_frame_interp(fr.I0, fr.I1, fr.dtype, rows, cols, batch, W.uf, W.vf,
                                              W.ub, W.vb, W.mask_f, W.mask_b, O.times, O.nt, O.out,
                                              kind, O.flags, O.trusted, s);
    if (e != hipSuccess) return hip_fail(ctx, e, "frame interpolation launch");
    return HSFLOW_OK;
}

// ---- flow projection (KS) -----------------------------------------------------
int check_cells(hsflow_ctx *ctx, const void *cells) {
    if (!cells) return null_pointer(ctx);
    if ((uintptr_t)cells & 7) return fail(ctx, HSFLOW_ERR_ARG, "cells must be 8-byte aligned");
    return HSFLOW_OK;
}

int check_projection(hsflow_ctx *ctx, int projection) {
    if (projection != 0 && projection != 1)
        return fail(ctx, HSFLOW_ERR_ARG, "projection %d is not 0 or 1", projection);
    return HSFLOW_OK;
}

// KS on checked arguments: the cells set to all ones stream-ordered, then one
// launch
int project_run(hsflow_ctx *ctx, const Frames &G, int rows, int cols, int batch, const FlowsIn &W,
                const float *times, int nt, uint64_t *cells, hipStream_t s) {
    HIP_TRY(ctx, hipMemsetAsync(cells, 0xFF, (size_t)rows * cols * batch * nt * 8, s));
    hipError_t e = hsflow::launch_flow_project(G.I0, G.I1, G.dtype, rows, cols, batch, W.uf, W.vf,
                                               W.ub, W.vb, times, nt, cells, s);
    if (e != hipSuccess) return hip_fail(ctx, e, "flow projection launch");
    return HSFLOW_OK;
}

// hsflow_flow_project_device
int project_impl(hsflow_ctx *ctx, const Frames &G, int rows, int cols, int batch, const FlowsIn &W,
                 const float *times, int nt, uint64_t *cells, hipStream_t s) {
    int rc = check_sizes(ctx, rows, cols, batch);
    if (rc || (rc = check_device_dtype(ctx, G.dtype))) return rc;
    if (!G.I0 || !G.I1 || !W.uf || !W.vf || !W.ub || !W.vb) return null_pointer(ctx);
    if ((rc = check_times(ctx, times, nt)) || (rc = check_cells(ctx, cells))) return rc;
    const size_t n = (size_t)rows * cols * batch, fb = n * elem_size(G.dtype);
    const ByteRange in[6] = {{G.I0, fb},    {G.I1, fb},    {W.uf, n * 4},
                             {W.vf, n * 4}, {W.ub, n * 4}, {W.vb, n * 4}};
    const ByteRange out{cells, n * nt * 8};
    if (!outputs_disjoint(in, 6, &out, 1))
        return fail(ctx, HSFLOW_ERR_ARG, "cells overlap the frames or the flows");
    return project_run(ctx, G, rows, cols, batch, W, times, nt, cells, s);
}

// hsflow_frame_interp_device, hsflow_frame_interp_bgr_device (fr.dtype: U8) and,
// `proj`, their *_proj_device forms, which read W.cells
int frame_interp_impl(hsflow_ctx *ctx, int channels, const Frames &fr, int rows, int cols,
                      int batch, const FlowsIn &W, const InterpOut &O, bool proj, hipStream_t s) {
    int rc = check_sizes(ctx, rows, cols, batch);
    if (rc || (rc = check_device_dtype(ctx, fr.dtype))) return rc;
    if (!fr.I0 || !fr.I1 || !W.uf || !W.vf || !W.ub || !W.vb || !O.out) return null_pointer(ctx);
    if ((rc = check_interp_args(ctx, O.times, O.nt, O.dtype_out, false))) return rc;
    if (proj && (rc = check_cells(ctx, W.cells))) return rc;
    const size_t n = (size_t)rows * cols * batch;
    const size_t fb = n * (channels == 3 ? 3 : elem_size(fr.dtype));
    const ByteRange in[9] = {{fr.I0, fb},   {fr.I1, fb},   {W.uf, n * 4},
                             {W.vf, n * 4}, {W.ub, n * 4}, {W.vb, n * 4},
                             {W.mask_f, n}, {W.mask_b, n},
                             {proj ? W.cells : nullptr, n * O.nt * 8}};
    ByteRange outs[4];
    interp_out_ranges(O, n, batch, channels, outs);
    if (!outputs_disjoint(in, 9, outs, 4))
        return fail(ctx, HSFLOW_ERR_ARG,
                    "interpolation outputs overlap the inputs or each other");
    return frame_interp_run(ctx, channels, fr, rows, cols, batch, W, O, s);
}

// ---- fallback for a failed pair (KF) --------------------------------------------
bool fb_on(const hsflow_fallback *fb) { return fb && fb->mode != HSFLOW_FALLBACK_OFF; }

// a setting that is on: the mode and the share (negated comparison: NaN fails)
int check_fallback(hsflow_ctx *ctx, const hsflow_fallback *fb) {
    if (fb->mode != HSFLOW_FALLBACK_NEAREST && fb->mode != HSFLOW_FALLBACK_BLEND)
        return fail(ctx, HSFLOW_ERR_ARG, "fallback mode %d is not 0, 1 or 2", fb->mode);
    if (!(fb->min_share >= 0.0f && fb->min_share <= 1.0f))
        return fail(ctx, HSFLOW_ERR_ARG, "fallback min_share %g outside [0, 1]",
                    (double)fb->min_share);
    return HSFLOW_OK;
}

// the smallest integer >= min_share * 2 * rows * cols: exact in double (24 bits
// of the share, at most 30 of the pixels of both directions)
uint64_t min_consistent(int rows, int cols, float min_share) {
    return (uint64_t)std::ceil((double)min_share * 2.0 * (double)rows * (double)cols);
}

size_t fb_counts_bytes(int batch) { return 2 * align_up((size_t)batch * 3 * 4); }

// KF on checked arguments: one launch
int fallback_run(hsflow_ctx *ctx, int channels, const Frames &fr, int rows, int cols, int batch,
                 const uint32_t *counts_f, const uint32_t *counts_b, const hsflow_fallback &fb,
                 const InterpOut &O, hipStream_t s) {
    const uint64_t m = min_consistent(rows, cols, fb.min_share);
    const int kind = out_kind(O.dtype_out);
    hipError_t e =
        channels == 3
            ? hsflow::launch_frame_fallback_bgr((const uint8_t *)fr.I0, (const uint8_t *)fr.I1,
                                                rows, cols, batch, counts_f, counts_b, m, fb.mode,
                                                O.times, O.nt, O.out, kind == hsflow::kOutU8,
                                                O.flags, O.trusted, O.cut, s)
            : hsflow::launch_frame_fallback(fr.I0, fr.I1, fr.dtype, rows, cols, batch, counts_f,
                                            counts_b, m, fb.mode, O.times, O.nt, O.out, kind,
                                            O.flags, O.trusted, O.cut, s);
    if (e != hipSuccess) return hip_fail(ctx, e, "frame fallback launch");
    return HSFLOW_OK;
}

// hsflow_frame_fallback_device, hsflow_frame_fallback_bgr_device (fr.dtype: U8)
int fallback_impl(hsflow_ctx *ctx, int channels, const Frames &fr, int rows, int cols, int batch,
                  const uint32_t *counts_f, const uint32_t *counts_b, const hsflow_fallback *fb,
                  const InterpOut &O, hipStream_t s) {
    int rc = check_sizes(ctx, rows, cols, batch);
    if (rc || (rc = check_device_dtype(ctx, fr.dtype))) return rc;
    if (!fr.I0 || !fr.I1 || !counts_f || !counts_b || !O.out) return null_pointer(ctx);
    if (!fb_on(fb))
        return fail(ctx, HSFLOW_ERR_ARG, "no fallback: a null setting or mode 0");
    if ((rc = check_fallback(ctx, fb))) return rc;
    if ((rc = check_interp_args(ctx, O.times, O.nt, O.dtype_out, false))) return rc;
    const size_t n = (size_t)rows * cols * batch, cb = (size_t)batch * 3 * 4;
    const size_t fbytes = n * (channels == 3 ? 3 : elem_size(fr.dtype));
    const ByteRange in[4] = {{fr.I0, fbytes}, {fr.I1, fbytes}, {counts_f, cb}, {counts_b, cb}};
    ByteRange outs[4];
    interp_out_ranges(O, n, batch, channels, outs);
    if (!outputs_disjoint(in, 4, outs, 4))
        return fail(ctx, HSFLOW_ERR_ARG, "fallback outputs overlap the inputs or each other");
    return fallback_run(ctx, channels, fr, rows, cols, batch, counts_f, counts_b, *fb, O, s);
}

// Workspace of the fused call: [the bidirectional solve's][uf][vf][ub][vb]
// (f32 batch planes)[mask_f][mask_b] (u8 batch planes), for BGR frames
// [grey I0][grey I1] (u8 batch planes), for a projected call of cell_nt
// times KS's [cells] (u64, batch x cell_nt planes) and, for a call with a
// fallback, KC's [counts_f][counts_b] (u32, batch x 3), each 256-byte aligned.
struct InterpLayout {
    size_t solve_bytes, flow[4], mask[2], gray[2], cells, counts[2], bytes;
};

InterpLayout interp_layout(int rows, int cols, int batch, int levels, int channels,
                           int cell_nt = 0, bool fb_counts = false) {
    InterpLayout L{};
    const size_t n = (size_t)rows * cols * batch;
    L.solve_bytes = align_up(pyr_layout(rows, cols, batch, levels).bytes);
    size_t off = L.solve_bytes;
    for (int k = 0; k < 4; ++k) L.flow[k] = off, off += align_up(n * 4);
    for (int k = 0; k < 2; ++k) L.mask[k] = off, off += align_up(n);
    if (channels == 3)
        for (int k = 0; k < 2; ++k) L.gray[k] = off, off += align_up(n);
    if (cell_nt > 0) L.cells = off, off += align_up(n * cell_nt * 8);
    if (fb_counts)
        for (int k = 0; k < 2; ++k) L.counts[k] = off, off += fb_counts_bytes(batch) / 2;
    L.bytes = off;
    return L;
}

// hsflow_flow_interp*_device (channels 1) and hsflow_flow_interp_bgr*_device
// (channels 3, in.dtype U8): for BGR frames hsflow_bgr_to_gray_device of both
// into the workspace, then hsflow_flow_bidir_median_device into the
// workspace's planes (the masks only when flags or trusted needs them), then
// KI or KIC on the frames themselves: public calls one after the other, so the
// bits are theirs by construction.  With a prefilter the solve runs on the two
// prefiltered f32 planes behind that layout.  S.projection = 1: KS
// (hsflow_flow_project_device) on the frames the solve ran on, into the
// workspace's cells, stands between the solve and the interpolation, which is
// then KIP (hsflow_frame_interp*_proj_device).  With a fallback on (S.fb) both
// checks run whatever is asked for, their counts go into the workspace, and KF
// (hsflow_frame_fallback*_device) follows the interpolation; off, the launches
// are unchanged and a given O.cut is zeroed.
int flow_interp_impl(hsflow_ctx *ctx, const SolveSpec &S, int channels, const Frames &in,
                     float rel, float abs_thr, const InterpOut &O, void *ws, size_t ws_bytes,
                     hipStream_t s, bool u16 = false) {
    PfPlan P;
    int rc = check_solve(ctx, S, in.dtype, &P, u16);
    if (rc) return rc;
    if (!in.I0 || !in.I1 || !O.out || !ws) return null_pointer(ctx);
    if ((rc = check_thresholds(ctx, rel, abs_thr))) return rc;
    if ((rc = check_interp_args(ctx, O.times, O.nt, O.dtype_out, false, u16))) return rc;
    if ((rc = check_projection(ctx, S.projection))) return rc;
    const bool fallback = fb_on(S.fb);
    if (fallback && (rc = check_fallback(ctx, S.fb))) return rc;
    const InterpLayout L = interp_layout(S.rows, S.cols, S.batch, S.levels, channels,
                                         S.projection ? O.nt : 0, fallback);
    const size_t need = L.bytes + (pf_on(S.pf) ? pf_planes_bytes(S.rows, S.cols, S.batch) : 0);
    const size_t n = (size_t)S.rows * S.cols * S.batch;
    const size_t fb = n * (channels == 3 ? 3 : elem_size(in.dtype));
    const ByteRange ins[3] = {{in.I0, fb}, {in.I1, fb}, {ws, need}};
    ByteRange outs[4];
    interp_out_ranges(O, n, S.batch, channels, outs);
    if (!outputs_disjoint(ins, 3, outs, 4))
        return fail(ctx, HSFLOW_ERR_ARG,
                    "interpolation outputs overlap the frames, the workspace or each other");
    if ((rc = check_init(ctx, S, true, outs, 4, ws, ws_bytes, need))) return rc;
    char *base = (char *)ws;
    uint8_t *const grey[2] = {(uint8_t *)(base + L.gray[0]), (uint8_t *)(base + L.gray[1])};
    Frames F;
    rc = solve_frames(ctx, S, P, in, channels == 3 ? grey : nullptr, ws, ws_bytes, L.bytes, &F, s);
    if (rc) return rc;
    const bool masks = O.flags || O.trusted;
    uint8_t *mf = masks ? (uint8_t *)(base + L.mask[0]) : nullptr;
    uint8_t *mb = masks ? (uint8_t *)(base + L.mask[1]) : nullptr;
    float *f[4];
    for (int k = 0; k < 4; ++k) f[k] = (float *)(base + L.flow[k]);
    uint32_t *cf = fallback ? (uint32_t *)(base + L.counts[0]) : nullptr;
    uint32_t *cb = fallback ? (uint32_t *)(base + L.counts[1]) : nullptr;
    const BidirOut B{f[0], f[1], f[2], f[3], {nullptr, mf, cf}, {nullptr, mb, cb}, rel, abs_thr};
    if ((rc = bidir_run(ctx, S, F, B, ws, s))) return rc;
    uint64_t *cells = S.projection ? (uint64_t *)(base + L.cells) : nullptr;
    const FlowsIn W{f[0], f[1], f[2], f[3], mf, mb, cells};
    if (cells && (rc = project_run(ctx, F, S.rows, S.cols, S.batch, W, O.times, O.nt, cells, s)))
        return rc;
    if ((rc = frame_interp_run(ctx, channels, in, S.rows, S.cols, S.batch, W, O, s))) return rc;
    if (fallback) return fallback_run(ctx, channels, in, S.rows, S.cols, S.batch, cf, cb, *S.fb, O, s);
    if (O.cut) HIP_TRY(ctx, hipMemsetAsync(O.cut, 0, (size_t)S.batch, s));
    return HSFLOW_OK;
}

// The host-buffer form of both: the frames go up as they are (BGR: 3 B/px),
// flow_interp_impl on the context's buffers, then flags and trusted down on
// the same stream ahead of the frames, whose download drains it.  Two
// differences between the two calls are their contract: the grey call takes
// HSFLOW_F64 output and fails at once on a null context; the BGR call takes
// U8 and F32 only and checks its arguments before the context, so that they
// can be checked where there is no device.
// In sequence mode (hsflow_ctx_set_temporal) the solve starts from the
// context's stored prediction and KP of its (ub, vb), which lie in the
// workspace, follows it on the stream ahead of the downloads.
// With the context's fallback on, the verdict comes down behind trusted; a cut
// leaves no prediction behind, so the next call starts cold.
int flow_interp_host(hsflow_ctx *ctx, const SolveSpec &spec, int channels, const void *I0,
                     const void *I1, int dtype_in, size_t step0, size_t step1, float rel,
                     float abs_thr, const HostInterpOut &O) {
    const bool bgr = channels == 3;
    SolveSpec S = spec;
    const int rows = S.rows, cols = S.cols, nt = O.nt;
    if (!bgr && !ctx) return HSFLOW_ERR_ARG;
    if (ctx) ctx->last_cut = -1;
    hsflow_flow_init init;
    if (ctx && take_prediction(ctx, rows, cols, &init)) S.init = &init;
    int rc = check_interp_args(ctx, O.times, nt, O.dtype_out, !bgr);
    if (rc) return rc;
    if (bgr) {
        if (!I0 || !I1) return fail(ctx, HSFLOW_ERR_ARG, "null image");
        if (!sizes_ok(rows, cols, 1))
            return fail(ctx, HSFLOW_ERR_ARG, "bad size %dx%d", rows, cols);
        if (step0 < (size_t)cols * 3 || step1 < (size_t)cols * 3)
            return fail(ctx, HSFLOW_ERR_ARG, "BGR steps %zu, %zu < row bytes", step0, step1);
    } else {
        // the frames, sizes and input steps (the output type is checked above)
        rc = check_host_args(ctx, I0, I1, dtype_in, rows, cols, step0, step1, HSFLOW_F32,
                             (size_t)cols * 4);
        if (rc) return rc;
    }
    if (O.out_step < (size_t)cols * channels * elem_size(O.dtype_out))
        return fail(ctx, HSFLOW_ERR_ARG, "output step %zu < row bytes", O.out_step);
    if (!O.out) return fail(ctx, HSFLOW_ERR_ARG, "null output");
    for (int k = 0; k < nt; ++k)
        if (!O.out[k] || (O.flags && !O.flags[k]))
            return fail(ctx, HSFLOW_ERR_ARG, "null output plane %d", k);
    if (O.flags && O.flags_step < (size_t)cols)
        return fail(ctx, HSFLOW_ERR_ARG, "flags step %zu < row bytes %d", O.flags_step, cols);
    if ((rc = check_levels(ctx, S.levels)) || (rc = check_finest(ctx, S)) ||
        (rc = check_iteration_args(ctx, S)) || (rc = check_thresholds(ctx, rel, abs_thr)))
        return rc;
    if (!ctx) return fail(nullptr, HSFLOW_ERR_ARG, "null context");
    const size_t n = (size_t)rows * cols, row = (size_t)cols * channels;
    const int dev_out = O.dtype_out == HSFLOW_U8 ? HSFLOW_U8 : HSFLOW_F32;
    // d_out: the nt frames (f32 or u8), the nt flag planes, trusted
    const size_t ob = align_up(n * nt * channels * elem_size(dev_out)), flb = align_up(n * nt);
    if ((rc = check_projection(ctx, S.projection))) return rc;
    const int cell_nt = S.projection ? nt : 0;
    const bool fb = fb_on(S.fb);
    const size_t wsb = interp_layout(rows, cols, 1, S.levels, channels, cell_nt, fb).bytes +
                       (pf_on(S.pf) ? pf_planes_bytes(rows, cols, 1) : 0);
    char *in0, *in1;
    rc = stage_pair(ctx, I0, I1, bgr ? 3 : elem_size(dtype_in), rows, cols, step0, step1,
                    ob + flb + kAlign, wsb, &in0, &in1);
    if (rc || (rc = grow_prediction(ctx, rows, cols))) return rc;
    char *dout = (char *)ctx->d_out;
    uint8_t *dfl = (uint8_t *)(dout + ob);
    uint32_t *dtr = (uint32_t *)(dout + ob + flb);
    uint8_t *dcut = (uint8_t *)(dtr + HSFLOW_MAX_TIMES);  // within the kAlign bytes
    const InterpOut D{O.times, nt, dout, dev_out, O.flags ? dfl : nullptr,
                      O.trusted ? dtr : nullptr, fb ? dcut : nullptr};
    rc = flow_interp_impl(ctx, S, channels, Frames{in0, in1, dtype_in}, rel, abs_thr, D, ctx->d_ws,
                          ctx->d_ws_bytes, ctx->stream);
    if (rc) return rc;
    const InterpLayout L = interp_layout(rows, cols, 1, S.levels, channels, cell_nt, fb);
    rc = predict_run(ctx, (const float *)((char *)ctx->d_ws + L.flow[2]),
                     (const float *)((char *)ctx->d_ws + L.flow[3]), rows, cols);
    if (rc) return rc;
    if (O.flags)
        for (int k = 0; k < nt; ++k)
            HIP_TRY(ctx, hipMemcpy2DAsync(O.flags[k], O.flags_step, dfl + k * n, (size_t)cols,
                                          (size_t)cols, rows, hipMemcpyDeviceToHost,
                                          ctx->stream));
    if (O.trusted)
        HIP_TRY(ctx, hipMemcpyAsync(O.trusted, dtr, (size_t)nt * sizeof(uint32_t),
                                    hipMemcpyDeviceToHost, ctx->stream));
    if (fb)
        HIP_TRY(ctx, hipMemcpyAsync(&ctx->cut_byte, dcut, 1, hipMemcpyDeviceToHost, ctx->stream));
    // the stream has drained: the verdict is here, and a cut keeps no prediction
    const auto finish = [&](int status) {
        if (status || !fb) return keep_prediction(ctx, status);
        ctx->last_cut = ctx->cut_byte ? 1 : 0;
        return ctx->last_cut ? HSFLOW_OK : keep_prediction(ctx, HSFLOW_OK);
    };
    if (dev_out == HSFLOW_U8) {
        for (int k = 0; k < nt; ++k)
            HIP_TRY(ctx, hipMemcpy2DAsync(O.out[k], O.out_step, dout + k * n * channels, row, row,
                                          rows, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return finish(HSFLOW_OK);
    }
    // f32 (widened to f64 on the way for the grey call): a plane is rows x
    // channels * cols floats
    const float *srcs[HSFLOW_MAX_TIMES];
    for (int k = 0; k < nt; ++k) srcs[k] = (const float *)dout + k * n * channels;
    return finish(download_planes(ctx, srcs, O.out, nt, rows, cols * channels, O.dtype_out,
                                  O.out_step));
}

// a host form's spec: one pair, the context's finest level, prefilter,
// smoothness, projection and fallback
SolveSpec host_spec(const hsflow_ctx *ctx, int rows, int cols, int levels, int warps, int median,
                    int window, int iters, double alpha) {
    return SolveSpec{rows,   cols,   1,     levels,       ctx ? ctx->finest : 0,
                     warps,  median, window, iters,       (float)alpha,
                     ctx ? &ctx->pf : nullptr,            ctx ? &ctx->sm : nullptr,
                     nullptr,                             ctx ? ctx->projection : 0,
                     ctx ? &ctx->fb : nullptr};
}

// ---- YUV 4:2:0 (KIY) -------------------------------------------------------------
// the luma's size, even each way, and the chroma's layout
int check_yuv_shape(hsflow_ctx *ctx, int layout, int rows, int cols, int batch) {
    const int rc = check_sizes(ctx, rows, cols, batch);
    if (rc) return rc;
    if ((rows | cols) & 1)
        return fail(ctx, HSFLOW_ERR_ARG, "YUV 4:2:0 needs even rows and cols, not %dx%d", rows,
                    cols);
    if (layout != HSFLOW_YUV_I420 && layout != HSFLOW_YUV_NV12)
        return fail(ctx, HSFLOW_ERR_ARG, "YUV layout %d is not 1 (I420) or 2 (NV12)", layout);
    return HSFLOW_OK;
}

// the chroma of a call: both frames', and the nt frames (times: host) it writes
// dtype: the samples', HSFLOW_U8 or HSFLOW_U16 (the *16 calls)
struct ChromaIO {
    const void *c0, *c1;
    int dtype;
    int layout;
    const float *times;
    int nt;
    void *out;
    int dtype_out;
};

// samples of the chroma of `batch` frames; the bytes of a call's, and of its output's
size_t chroma_samples(int rows, int cols, int batch) { return (size_t)rows * cols * batch / 2; }
size_t chroma_bytes(const ChromaIO &C, int rows, int cols, int batch) {
    return chroma_samples(rows, cols, batch) * elem_size(C.dtype);
}
size_t chroma_out_bytes(const ChromaIO &C, int rows, int cols, int batch) {
    return chroma_samples(rows, cols, batch) * C.nt * elem_size(C.dtype_out);
}

// KIY, or with W.cells KIYP, on checked arguments: one launch.  fb: null for no
// fallback
int chroma_interp_run(hsflow_ctx *ctx, const ChromaIO &C, int rows, int cols, int batch,
                      const FlowsIn &W, const uint32_t *counts_f, const uint32_t *counts_b,
                      const hsflow_fallback *fb, hipStream_t s) {
    const bool on = fb_on(fb);
    hipError_t e = hsflow::launch_chroma_interp(
        C.c0, C.c1, C.dtype, C.layout, rows, cols, batch, W.uf, W.vf, W.ub, W.vb,
        on ? counts_f : nullptr, on ? counts_b : nullptr,
        on ? min_consistent(rows, cols, fb->min_share) : 0, on ? fb->mode : 0, C.times, C.nt,
        C.out, out_kind(C.dtype_out), s, W.cells);
    if (e != hipSuccess) return hip_fail(ctx, e, "chroma interpolation launch");
    return HSFLOW_OK;
}

// hsflow_chroma_interp_device and, `proj`, hsflow_chroma_interp_proj_device, which
// reads W.cells (KS's, of the luma)
int chroma_interp_impl(hsflow_ctx *ctx, const ChromaIO &C, int rows, int cols, int batch,
                       const FlowsIn &W, const uint32_t *counts_f, const uint32_t *counts_b,
                       const hsflow_fallback *fb, bool proj, hipStream_t s) {
    int rc = check_yuv_shape(ctx, C.layout, rows, cols, batch);
    if (rc) return rc;
    if (!C.c0 || !C.c1 || !W.uf || !W.vf || !W.ub || !W.vb || !C.out) return null_pointer(ctx);
    const bool u16 = C.dtype == HSFLOW_U16;
    if ((rc = check_interp_args(ctx, C.times, C.nt, C.dtype_out, false, u16))) return rc;
    if (proj && (rc = check_cells(ctx, W.cells))) return rc;
    const bool on = fb_on(fb);
    if (on) {
        if ((rc = check_fallback(ctx, fb))) return rc;
        if (!counts_f || !counts_b) return null_pointer(ctx);
    }
    const size_t n = (size_t)rows * cols * batch, cb = chroma_bytes(C, rows, cols, batch);
    const size_t kb = (size_t)batch * 3 * 4;
    const ByteRange in[9] = {{C.c0, cb},    {C.c1, cb},    {W.uf, n * 4},
                             {W.vf, n * 4}, {W.ub, n * 4}, {W.vb, n * 4},
                             {on ? counts_f : nullptr, kb}, {on ? counts_b : nullptr, kb},
                             {proj ? W.cells : nullptr, n * C.nt * 8}};
    const ByteRange out{C.out, chroma_out_bytes(C, rows, cols, batch)};
    if (!outputs_disjoint(in, 9, &out, 1))
        return fail(ctx, HSFLOW_ERR_ARG, "chroma output overlaps the inputs");
    return chroma_interp_run(ctx, C, rows, cols, batch, W, counts_f, counts_b, fb, s);
}

// hsflow_cells_down_device (KSD)
int cells_down_impl(hsflow_ctx *ctx, const uint64_t *cells, int rows, int cols, int batch, int nt,
                    uint64_t *cells_c, hipStream_t s) {
    int rc = check_sizes(ctx, rows, cols, batch);
    if (rc) return rc;
    if ((rows | cols) & 1)
        return fail(ctx, HSFLOW_ERR_ARG, "YUV 4:2:0 needs even rows and cols, not %dx%d", rows,
                    cols);
    if (nt < 1 || nt > HSFLOW_MAX_TIMES)
        return fail(ctx, HSFLOW_ERR_ARG, "nt %d outside [1, %d]", nt, HSFLOW_MAX_TIMES);
    if ((rc = check_cells(ctx, cells)) || (rc = check_cells(ctx, cells_c))) return rc;
    const size_t n = (size_t)rows * cols * batch * nt;
    const ByteRange in{cells, n * 8}, out{cells_c, n * 2};
    if (!outputs_disjoint(&in, 1, &out, 1))
        return fail(ctx, HSFLOW_ERR_ARG, "the chroma cells overlap the luma cells");
    hipError_t e = hsflow::launch_cells_down(cells, rows, cols, batch * nt, cells_c, s);
    if (e != hipSuccess) return hip_fail(ctx, e, "cells reduction launch");
    return HSFLOW_OK;
}

// hsflow_flow_interp_yuv_device, hsflow_flow_interp_yuv_pj_device: what the chroma
// adds to the grey call's checks (first, so that nothing has run when one
// fails), flow_interp_impl on the luma planes, then KIY on the flows and counts
// that call left in the workspace; S.projection = 1: KIYP on those and on the
// cells KS left there
int flow_interp_yuv_impl(hsflow_ctx *ctx, const SolveSpec &S, const Frames &luma, const ChromaIO &C,
                         float rel, float abs_thr, const InterpOut &Y, void *ws, size_t ws_bytes,
                         hipStream_t s) {
    int rc = check_yuv_shape(ctx, C.layout, S.rows, S.cols, S.batch);
    if (rc || (rc = check_levels(ctx, S.levels))) return rc;
    if (!luma.I0 || !luma.I1 || !C.c0 || !C.c1 || !Y.out || !C.out || !ws)
        return null_pointer(ctx);
    const bool u16 = luma.dtype == HSFLOW_U16;
    if ((rc = check_interp_args(ctx, Y.times, Y.nt, Y.dtype_out, false, u16))) return rc;
    if ((rc = check_projection(ctx, S.projection))) return rc;
    const bool fallback = fb_on(S.fb);
    if (fallback && (rc = check_fallback(ctx, S.fb))) return rc;
    const InterpLayout L = interp_layout(S.rows, S.cols, S.batch, S.levels, 1,
                                         S.projection ? Y.nt : 0, fallback);
    const size_t need = L.bytes + (pf_on(S.pf) ? pf_planes_bytes(S.rows, S.cols, S.batch) : 0);
    const size_t n = (size_t)S.rows * S.cols * S.batch;
    const size_t yb = n * elem_size(luma.dtype), cb = chroma_bytes(C, S.rows, S.cols, S.batch);
    const ByteRange ins[5] = {{luma.I0, yb}, {luma.I1, yb}, {C.c0, cb}, {C.c1, cb}, {ws, need}};
    ByteRange outs[5];
    interp_out_ranges(Y, n, S.batch, 1, outs);
    outs[4] = {C.out, chroma_out_bytes(C, S.rows, S.cols, S.batch)};
    if (!outputs_disjoint(ins, 5, outs, 5))
        return fail(ctx, HSFLOW_ERR_ARG,
                    "interpolation outputs overlap the frames, the workspace or each other");
    if (S.init) {  // the planes a solve starts from, against the chroma output
        const float *planes[4] = {S.init->uf, S.init->vf, S.init->ub, S.init->vb};
        for (const float *p : planes)
            if (bytes_overlap(p, n * 4, outs[4].p, outs[4].n))
                return fail(ctx, HSFLOW_ERR_ARG, "init flow overlaps an output");
    }
    if ((rc = flow_interp_impl(ctx, S, 1, luma, rel, abs_thr, Y, ws, ws_bytes, s, u16))) return rc;
    char *base = (char *)ws;
    const FlowsIn W{(const float *)(base + L.flow[0]), (const float *)(base + L.flow[1]),
                    (const float *)(base + L.flow[2]), (const float *)(base + L.flow[3]),
                    nullptr, nullptr,
                    S.projection ? (const uint64_t *)(base + L.cells) : nullptr};
    return chroma_interp_run(ctx, C, S.rows, S.cols, S.batch, W,
                             fallback ? (const uint32_t *)(base + L.counts[0]) : nullptr,
                             fallback ? (const uint32_t *)(base + L.counts[1]) : nullptr, S.fb, s);
}

// hsflow_flow_interp_yuv: flow_interp_host for packed 4:2:0 frames.  Each frame
// goes up as it is, rows * 3 / 2 rows of cols bytes; the luma and the chroma of
// a time come down into its packed host frame.  projection < 0
// (hsflow_flow_interp_yuv): none, and a context that has it on is refused; 0 or
// 1 (hsflow_flow_interp_yuv_pj): that, whatever the context's setting.
// dtype_in: HSFLOW_U8, or HSFLOW_U16 (hsflow_flow_interp_yuv16): frames of
// 2-byte samples, out U16 or F32.
int flow_interp_yuv_host(hsflow_ctx *ctx, const SolveSpec &spec, const void *f0, const void *f1,
                         int dtype_in, int layout, float rel, float abs_thr, const float *times,
                         int nt, int projection, void *const *out, int dtype_out,
                         uint8_t *const *flags, uint32_t *trusted) {
    SolveSpec S = spec;
    const int rows = S.rows, cols = S.cols;
    if (ctx) ctx->last_cut = -1;
    hsflow_flow_init init;
    if (ctx && take_prediction(ctx, rows, cols, &init)) S.init = &init;
    const size_t is = elem_size(dtype_in);
    int rc = check_interp_args(ctx, times, nt, dtype_out, false, dtype_in == HSFLOW_U16);
    if (rc) return rc;
    if (!f0 || !f1) return fail(ctx, HSFLOW_ERR_ARG, "null image");
    if ((rc = check_yuv_shape(ctx, layout, rows, cols, 1))) return rc;
    if (projection >= 0 && (rc = check_projection(ctx, projection))) return rc;
    if (!out) return fail(ctx, HSFLOW_ERR_ARG, "null output");
    for (int k = 0; k < nt; ++k)
        if (!out[k] || (flags && !flags[k]))
            return fail(ctx, HSFLOW_ERR_ARG, "null output plane %d", k);
    if ((rc = check_levels(ctx, S.levels)) || (rc = check_finest(ctx, S)) ||
        (rc = check_iteration_args(ctx, S)) || (rc = check_thresholds(ctx, rel, abs_thr)))
        return rc;
    if (!ctx) return fail(nullptr, HSFLOW_ERR_ARG, "null context");
    if (projection >= 0)
        S.projection = projection;
    else if (S.projection)
        return fail(ctx, HSFLOW_ERR_ARG,
                    "the flow projection is not supported on YUV chroma: set the context's "
                    "projection to 0");
    const int cell_nt = S.projection ? nt : 0;
    const size_t n = (size_t)rows * cols, es = elem_size(dtype_out);
    // d_out: the nt luma planes, the nt chroma frames, the nt flag planes, trusted
    const size_t yb = align_up(n * nt * es), cb = align_up(n / 2 * nt * es), flb = align_up(n * nt);
    const bool fb = fb_on(S.fb);
    const size_t wsb = interp_layout(rows, cols, 1, S.levels, 1, cell_nt, fb).bytes +
                       (pf_on(S.pf) ? pf_planes_bytes(rows, cols, 1) : 0);
    char *in0, *in1;
    rc = stage_pair(ctx, f0, f1, is, rows / 2 * 3, cols, (size_t)cols * is, (size_t)cols * is,
                    yb + cb + flb + kAlign, wsb, &in0, &in1);
    if (rc || (rc = grow_prediction(ctx, rows, cols))) return rc;
    char *dy = (char *)ctx->d_out, *dc = dy + yb;
    uint8_t *dfl = (uint8_t *)(dc + cb);
    uint32_t *dtr = (uint32_t *)(dc + cb + flb);
    uint8_t *dcut = (uint8_t *)(dtr + HSFLOW_MAX_TIMES);  // within the kAlign bytes
    const InterpOut Y{times, nt, dy, dtype_out, flags ? dfl : nullptr, trusted ? dtr : nullptr,
                      fb ? dcut : nullptr};
    const ChromaIO C{in0 + n * is, in1 + n * is, dtype_in, layout, times, nt, dc, dtype_out};
    rc = flow_interp_yuv_impl(ctx, S, Frames{in0, in1, dtype_in}, C, rel, abs_thr, Y, ctx->d_ws,
                              ctx->d_ws_bytes, ctx->stream);
    if (rc) return rc;
    const InterpLayout L = interp_layout(rows, cols, 1, S.levels, 1, cell_nt, fb);
    rc = predict_run(ctx, (const float *)((char *)ctx->d_ws + L.flow[2]),
                     (const float *)((char *)ctx->d_ws + L.flow[3]), rows, cols);
    if (rc) return rc;
    if (flags)
        for (int k = 0; k < nt; ++k)
            HIP_TRY(ctx, hipMemcpyAsync(flags[k], dfl + k * n, n, hipMemcpyDeviceToHost,
                                        ctx->stream));
    if (trusted)
        HIP_TRY(ctx, hipMemcpyAsync(trusted, dtr, (size_t)nt * sizeof(uint32_t),
                                    hipMemcpyDeviceToHost, ctx->stream));
    if (fb)
        HIP_TRY(ctx, hipMemcpyAsync(&ctx->cut_byte, dcut, 1, hipMemcpyDeviceToHost, ctx->stream));
    for (int k = 0; k < nt; ++k) {
        char *dst = (char *)out[k];
        HIP_TRY(ctx, hipMemcpyAsync(dst, dy + k * n * es, n * es, hipMemcpyDeviceToHost,
                                    ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(dst + n * es, dc + k * (n / 2) * es, n / 2 * es,
                                    hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    // the stream has drained: the verdict is here, and a cut keeps no prediction
    if (!fb) return keep_prediction(ctx, HSFLOW_OK);
    ctx->last_cut = ctx->cut_byte ? 1 : 0;
    return ctx->last_cut ? HSFLOW_OK : keep_prediction(ctx, HSFLOW_OK);
}

}  // namespace

extern "C" {

int hsflow_warp_gradients_device(const void *I0, const void *I1, int dtype_in, int rows,
                                 int cols, int batch, const float *u0, const float *v0,
                                 float *gx, float *gy, float *gt, void *workspace,
                                 size_t workspace_bytes, void *stream) {
    DeviceGuard g((hipStream_t)stream);
    float *const out[3] = {gx, gy, gt};
    return warp_gradients_impl(nullptr, Frames{I0, I1, dtype_in}, rows, cols, batch, u0, v0, out,
                               workspace, workspace_bytes, (hipStream_t)stream);
}

int hsflow_flow_warped_lv_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                                 int batch, int levels, int finest, int warps, int median,
                                 int window, int iters, float alpha, float *u, float *v,
                                 const hsflow_prefilter *pf, const hsflow_smoothness *sm,
                                 const hsflow_flow_init *init, void *workspace,
                                 size_t workspace_bytes, void *stream) {
    DeviceGuard g((hipStream_t)stream);
    const SolveSpec S{rows,   cols,  batch, levels, finest, warps, median,
                      window, iters, alpha, pf,     sm,     init,  0};
    return warped_impl(nullptr, S, Frames{I0, I1, dtype_in}, u, v, workspace, workspace_bytes,
                       (hipStream_t)stream);
}

// the earlier entry points: the same solve with the later options off
int hsflow_flow_warped_init_device(const void *I0, const void *I1, int dtype_in, int rows,
                                   int cols, int batch, int levels, int warps, int median,
                                   int window, int iters, float alpha, float *u, float *v,
                                   const hsflow_prefilter *pf, const hsflow_smoothness *sm,
                                   const hsflow_flow_init *init, void *workspace,
                                   size_t workspace_bytes, void *stream) {
    return hsflow_flow_warped_lv_device(I0, I1, dtype_in, rows, cols, batch, levels, 0, warps,
                                        median, window, iters, alpha, u, v, pf, sm, init,
                                        workspace, workspace_bytes, stream);
}

int hsflow_flow_warped_sm_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                                 int batch, int levels, int warps, int median, int window,
                                 int iters, float alpha, float *u, float *v,
                                 const hsflow_prefilter *pf, const hsflow_smoothness *sm,
                                 void *workspace, size_t workspace_bytes, void *stream) {
    return hsflow_flow_warped_init_device(I0, I1, dtype_in, rows, cols, batch, levels, warps,
                                          median, window, iters, alpha, u, v, pf, sm, nullptr,
                                          workspace, workspace_bytes, stream);
}

int hsflow_flow_warped_pf_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                                 int batch, int levels, int warps, int median, int window,
                                 int iters, float alpha, float *u, float *v,
                                 const hsflow_prefilter *pf, void *workspace,
                                 size_t workspace_bytes, void *stream) {
    return hsflow_flow_warped_sm_device(I0, I1, dtype_in, rows, cols, batch, levels, warps, median,
                                        window, iters, alpha, u, v, pf, nullptr, workspace,
                                        workspace_bytes, stream);
}

int hsflow_flow_warped_median_device(const void *I0, const void *I1, int dtype_in, int rows,
                                     int cols, int batch, int levels, int warps, int median,
                                     int window, int iters, float alpha, float *u, float *v,
                                     void *workspace, size_t workspace_bytes, void *stream) {
    return hsflow_flow_warped_sm_device(I0, I1, dtype_in, rows, cols, batch, levels, warps, median,
                                        window, iters, alpha, u, v, nullptr, nullptr, workspace,
                                        workspace_bytes, stream);
}

int hsflow_flow_warped_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                              int batch, int levels, int warps, int window, int iters,
                              float alpha, float *u, float *v, void *workspace,
                              size_t workspace_bytes, void *stream) {
    return hsflow_flow_warped_sm_device(I0, I1, dtype_in, rows, cols, batch, levels, warps, 0,
                                        window, iters, alpha, u, v, nullptr, nullptr, workspace,
                                        workspace_bytes, stream);
}

// The host-buffer form: hsflow_flow_pyramid's upload, download, f64 widening
// and huge-page advice around the warped solve, which honours the context's
// prefilter (its planes lie behind the solve's workspace) and smoothness.
int hsflow_flow_warped_median(hsflow_ctx *ctx, const void *I0, const void *I1, int dtype_in,
                              int rows, int cols, size_t in_step0, size_t in_step1, int levels,
                              int warps, int median, int window, int iters, double alpha,
                              void *u, void *v, int dtype_out, size_t out_step) {
    if (!ctx) return HSFLOW_ERR_ARG;
    const SolveSpec S = host_spec(ctx, rows, cols, levels, warps, median, window, iters, alpha);
    int rc = check_iteration_args(ctx, S);
    if (rc) return rc;
    rc = check_host_args(ctx, I0, I1, dtype_in, rows, cols, in_step0, in_step1, dtype_out,
                         out_step);
    if (rc) return rc;
    if (!u || !v) return fail(ctx, HSFLOW_ERR_ARG, "null output");
    if ((rc = check_levels(ctx, levels)) || (rc = check_finest(ctx, S))) return rc;
    const size_t pb = align_up((size_t)rows * cols * 4);
    const size_t wsb = hsflow_pyramid_workspace_bytes(rows, cols, 1, levels) +
                       (pf_on(S.pf) ? pf_planes_bytes(rows, cols, 1) : 0);
    char *in0, *in1;
    rc = stage_pair(ctx, I0, I1, elem_size(dtype_in), rows, cols, in_step0, in_step1, pb * 3, wsb,
                    &in0, &in1);
    if (rc) return rc;
    float *du = (float *)ctx->d_out, *dv = (float *)((char *)du + pb);
    rc = warped_impl(ctx, S, Frames{in0, in1, dtype_in}, du, dv, ctx->d_ws, ctx->d_ws_bytes,
                     ctx->stream);
    if (rc) return rc;
    const float *srcs[2] = {du, dv};
    void *dsts[2] = {u, v};
    return download_planes(ctx, srcs, dsts, 2, rows, cols, dtype_out, out_step);
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
    return consistency_impl(nullptr, uf, vf, ub, vb, rows, cols, batch, rel, abs_thr,
                            CheckOut{err, mask, counts}, (hipStream_t)stream);
}

int hsflow_flow_bidir_lv_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                                int batch, int levels, int finest, int warps, int median,
                                int window, int iters, float alpha, float rel, float abs_thr,
                                float *uf, float *vf, float *ub, float *vb, float *err_f,
                                uint8_t *mask_f, uint32_t *counts_f, float *err_b, uint8_t *mask_b,
                                uint32_t *counts_b, const hsflow_prefilter *pf,
                                const hsflow_smoothness *sm, const hsflow_flow_init *init,
                                void *workspace, size_t workspace_bytes, void *stream) {
    DeviceGuard g((hipStream_t)stream);
    const SolveSpec S{rows,   cols,  batch, levels, finest, warps, median,
                      window, iters, alpha, pf,     sm,     init,  0};
    const BidirOut B{uf,  vf, ub, vb, {err_f, mask_f, counts_f}, {err_b, mask_b, counts_b},
                     rel, abs_thr};
    return bidir_impl(nullptr, S, Frames{I0, I1, dtype_in}, B, workspace, workspace_bytes,
                      (hipStream_t)stream);
}

int hsflow_flow_bidir_init_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                                  int batch, int levels, int warps, int median, int window,
                                  int iters, float alpha, float rel, float abs_thr, float *uf,
                                  float *vf, float *ub, float *vb, float *err_f, uint8_t *mask_f,
                                  uint32_t *counts_f, float *err_b, uint8_t *mask_b,
                                  uint32_t *counts_b, const hsflow_prefilter *pf,
                                  const hsflow_smoothness *sm, const hsflow_flow_init *init,
                                  void *workspace, size_t workspace_bytes, void *stream) {
    return hsflow_flow_bidir_lv_device(I0, I1, dtype_in, rows, cols, batch, levels, 0, warps,
                                       median, window, iters, alpha, rel, abs_thr, uf, vf, ub, vb,
                                       err_f, mask_f, counts_f, err_b, mask_b, counts_b, pf, sm,
                                       init, workspace, workspace_bytes, stream);
}

int hsflow_flow_bidir_sm_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                                int batch, int levels, int warps, int median, int window,
                                int iters, float alpha, float rel, float abs_thr, float *uf,
                                float *vf, float *ub, float *vb, float *err_f, uint8_t *mask_f,
                                uint32_t *counts_f, float *err_b, uint8_t *mask_b,
                                uint32_t *counts_b, const hsflow_prefilter *pf,
                                const hsflow_smoothness *sm, void *workspace,
                                size_t workspace_bytes, void *stream) {
    return hsflow_flow_bidir_init_device(I0, I1, dtype_in, rows, cols, batch, levels, warps,
                                         median, window, iters, alpha, rel, abs_thr, uf, vf, ub,
                                         vb, err_f, mask_f, counts_f, err_b, mask_b, counts_b, pf,
                                         sm, nullptr, workspace, workspace_bytes, stream);
}

int hsflow_flow_bidir_pf_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                                int batch, int levels, int warps, int median, int window,
                                int iters, float alpha, float rel, float abs_thr, float *uf,
                                float *vf, float *ub, float *vb, float *err_f, uint8_t *mask_f,
                                uint32_t *counts_f, float *err_b, uint8_t *mask_b,
                                uint32_t *counts_b, const hsflow_prefilter *pf, void *workspace,
                                size_t workspace_bytes, void *stream) {
    return hsflow_flow_bidir_sm_device(I0, I1, dtype_in, rows, cols, batch, levels, warps, median,
                                       window, iters, alpha, rel, abs_thr, uf, vf, ub, vb, err_f,
                                       mask_f, counts_f, err_b, mask_b, counts_b, pf, nullptr,
                                       workspace, workspace_bytes, stream);
}

int hsflow_flow_bidir_median_device(const void *I0, const void *I1, int dtype_in, int rows,
                                    int cols, int batch, int levels, int warps, int median,
                                    int window, int iters, float alpha, float rel, float abs_thr,
                                    float *uf, float *vf, float *ub, float *vb, float *err_f,
                                    uint8_t *mask_f, uint32_t *counts_f, float *err_b,
                                    uint8_t *mask_b, uint32_t *counts_b, void *workspace,
                                    size_t workspace_bytes, void *stream) {
    return hsflow_flow_bidir_sm_device(I0, I1, dtype_in, rows, cols, batch, levels, warps, median,
                                       window, iters, alpha, rel, abs_thr, uf, vf, ub, vb, err_f,
                                       mask_f, counts_f, err_b, mask_b, counts_b, nullptr, nullptr,
                                       workspace, workspace_bytes, stream);
}

int hsflow_flow_bidir_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                             int batch, int levels, int warps, int window, int iters,
                             float alpha, float rel, float abs_thr, float *uf, float *vf, float *ub,
                             float *vb, float *err_f, uint8_t *mask_f, uint32_t *counts_f,
                             float *err_b, uint8_t *mask_b, uint32_t *counts_b, void *workspace,
                             size_t workspace_bytes, void *stream) {
    return hsflow_flow_bidir_sm_device(I0, I1, dtype_in, rows, cols, batch, levels, warps, 0,
                                       window, iters, alpha, rel, abs_thr, uf, vf, ub, vb, err_f,
                                       mask_f, counts_f, err_b, mask_b, counts_b, nullptr, nullptr,
                                       workspace, workspace_bytes, stream);
}

// The host-buffer form of the bidirectional solve: hsflow_flow_warped_median's
// upload and download around bidir_impl; the masks and counts come down on
// the same stream ahead of the flows, whose download drains it.  In sequence
// mode the solve starts from the stored prediction and KP of (ub, vb) follows it.
int hsflow_flow_bidir_median(hsflow_ctx *ctx, const void *I0, const void *I1, int dtype_in,
                             int rows, int cols, size_t in_step0, size_t in_step1, int levels,
                             int warps, int median, int window, int iters, double alpha,
                             float rel, float abs_thr, void *u, void *v, void *ub, void *vb,
                             int dtype_out, size_t out_step, uint8_t *mask_f, uint8_t *mask_b,
                             size_t mask_step, uint32_t *counts) {
    if (!ctx) return HSFLOW_ERR_ARG;
    SolveSpec S = host_spec(ctx, rows, cols, levels, warps, median, window, iters, alpha);
    hsflow_flow_init init;
    if (take_prediction(ctx, rows, cols, &init)) S.init = &init;
    int rc = check_host_args(ctx, I0, I1, dtype_in, rows, cols, in_step0, in_step1,
                             dtype_out, out_step);
    if (rc) return rc;
    if (!u || !v) return fail(ctx, HSFLOW_ERR_ARG, "null output");
    if ((rc = check_levels(ctx, levels)) || (rc = check_finest(ctx, S)) ||
        (rc = check_iteration_args(ctx, S)) || (rc = check_thresholds(ctx, rel, abs_thr)))
        return rc;
    if ((mask_f || mask_b) && mask_step < (size_t)cols)
        return fail(ctx, HSFLOW_ERR_ARG, "mask step %zu < row bytes %d", mask_step, cols);
    const size_t n = (size_t)rows * cols;
    // d_out: uf, vf, ub, vb (f32), the two masks (u8), counts (2 x 3 words)
    const size_t fb = align_up(n * 4), mb = align_up(n);
    const size_t wsb = hsflow_pyramid_workspace_bytes(rows, cols, 1, levels) +
                       (pf_on(S.pf) ? pf_planes_bytes(rows, cols, 1) : 0);
    char *in0, *in1;
    rc = stage_pair(ctx, I0, I1, elem_size(dtype_in), rows, cols, in_step0, in_step1,
                    fb * 4 + mb * 2 + kAlign, wsb, &in0, &in1);
    if (rc || (rc = grow_prediction(ctx, rows, cols))) return rc;
    char *out = (char *)ctx->d_out;
    float *d[4] = {(float *)out, (float *)(out + fb), (float *)(out + 2 * fb),
                   (float *)(out + 3 * fb)};
    uint8_t *dmf = (uint8_t *)(out + 4 * fb), *dmb = dmf + mb;
    uint32_t *dc = (uint32_t *)(dmb + mb);
    const CheckOut cf{nullptr, mask_f ? dmf : nullptr, counts ? dc : nullptr};
    const CheckOut cb{nullptr, mask_b ? dmb : nullptr, counts ? dc + 3 : nullptr};
    const BidirOut B{d[0], d[1], d[2], d[3], cf, cb, rel, abs_thr};
    rc = bidir_impl(ctx, S, Frames{in0, in1, dtype_in}, B, ctx->d_ws, ctx->d_ws_bytes,
                    ctx->stream);
    if (rc || (rc = predict_run(ctx, d[2], d[3], rows, cols))) return rc;
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
    return keep_prediction(ctx, download_planes(ctx, srcs, dsts, np, rows, cols, dtype_out,
                                                out_step));
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
    return frame_interp_impl(nullptr, 1, Frames{I0, I1, dtype_in}, rows, cols, batch,
                             FlowsIn{uf, vf, ub, vb, mask_f, mask_b, nullptr},
                             InterpOut{times, nt, out, dtype_out, flags, trusted}, false,
                             (hipStream_t)stream);
}

int hsflow_flow_project_device(const void *G0, const void *G1, int dtype_in, int rows, int cols,
                               int batch, const float *uf, const float *vf, const float *ub,
                               const float *vb, const float *times, int nt, uint64_t *cells,
                               void *stream) {
    DeviceGuard g((hipStream_t)stream);
    return project_impl(nullptr, Frames{G0, G1, dtype_in}, rows, cols, batch,
                        FlowsIn{uf, vf, ub, vb, nullptr, nullptr, nullptr}, times, nt, cells,
                        (hipStream_t)stream);
}

int hsflow_frame_interp_proj_device(const void *I0, const void *I1, int dtype_in, int rows,
                                    int cols, int batch, const float *uf, const float *vf,
                                    const float *ub, const float *vb, const uint8_t *mask_f,
                                    const uint8_t *mask_b, const uint64_t *cells,
                                    const float *times, int nt, void *out, int dtype_out,
                                    uint8_t *flags, uint32_t *trusted, void *stream) {
    DeviceGuard g((hipStream_t)stream);
    return frame_interp_impl(nullptr, 1, Frames{I0, I1, dtype_in}, rows, cols, batch,
                             FlowsIn{uf, vf, ub, vb, mask_f, mask_b, cells},
                             InterpOut{times, nt, out, dtype_out, flags, trusted}, true,
                             (hipStream_t)stream);
}

size_t hsflow_flow_interp_pj_workspace_bytes(int rows, int cols, int batch, int levels, int nt) {
    if (!sizes_ok(rows, cols, batch) || levels < 1 || levels > HSFLOW_MAX_LEVELS || nt < 1 ||
        nt > HSFLOW_MAX_TIMES)
        return 0;
    return interp_layout(rows, cols, batch, levels, 1, nt).bytes;
}

int hsflow_flow_interp_pj_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                                 int batch, int levels, int finest, int warps, int median,
                                 int window, int iters, float alpha, float rel, float abs_thr,
                                 const float *times, int nt, int projection, void *out,
                                 int dtype_out, uint8_t *flags, uint32_t *trusted,
                                 const hsflow_prefilter *pf, const hsflow_smoothness *sm,
                                 const hsflow_flow_init *init, void *workspace,
                                 size_t workspace_bytes, void *stream) {
    return hsflow_flow_interp_fb_device(I0, I1, dtype_in, rows, cols, batch, levels, finest, warps,
                                        median, window, iters, alpha, rel, abs_thr, times, nt,
                                        projection, out, dtype_out, flags, trusted, nullptr, pf,
                                        sm, init, nullptr, workspace, workspace_bytes, stream);
}

int hsflow_flow_interp_fb_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                                 int batch, int levels, int finest, int warps, int median,
                                 int window, int iters, float alpha, float rel, float abs_thr,
                                 const float *times, int nt, int projection, void *out,
                                 int dtype_out, uint8_t *flags, uint32_t *trusted, uint8_t *cut,
                                 const hsflow_prefilter *pf, const hsflow_smoothness *sm,
                                 const hsflow_flow_init *init, const hsflow_fallback *fb,
                                 void *workspace, size_t workspace_bytes, void *stream) {
    DeviceGuard g((hipStream_t)stream);
    const SolveSpec S{rows,  cols,  batch, levels, finest, warps,      median, window,
                      iters, alpha, pf,    sm,     init,   projection, fb};
    return flow_interp_impl(nullptr, S, 1, Frames{I0, I1, dtype_in}, rel, abs_thr,
                            InterpOut{times, nt, out, dtype_out, flags, trusted, cut}, workspace,
                            workspace_bytes, (hipStream_t)stream);
}

size_t hsflow_fallback_min_consistent(int rows, int cols, float min_share) {
    if (!sizes_ok(rows, cols, 1) || !(min_share >= 0.0f && min_share <= 1.0f)) return 0;
    return (size_t)min_consistent(rows, cols, min_share);
}

size_t hsflow_fallback_counts_bytes(int batch) {
    if (batch < 1 || batch > kMaxBatch) return 0;
    return fb_counts_bytes(batch);
}

int hsflow_frame_fallback_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                                 int batch, const uint32_t *counts_f, const uint32_t *counts_b,
                                 const hsflow_fallback *fb, const float *times, int nt, void *out,
                                 int dtype_out, uint8_t *flags, uint32_t *trusted, uint8_t *cut,
                                 void *stream) {
    DeviceGuard g((hipStream_t)stream);
    return fallback_impl(nullptr, 1, Frames{I0, I1, dtype_in}, rows, cols, batch, counts_f,
                         counts_b, fb, InterpOut{times, nt, out, dtype_out, flags, trusted, cut},
                         (hipStream_t)stream);
}

int hsflow_frame_fallback_bgr_device(const uint8_t *bgr0, const uint8_t *bgr1, int rows, int cols,
                                     int batch, const uint32_t *counts_f,
                                     const uint32_t *counts_b, const hsflow_fallback *fb,
                                     const float *times, int nt, void *out, int dtype_out,
                                     uint8_t *flags, uint32_t *trusted, uint8_t *cut,
                                     void *stream) {
    DeviceGuard g((hipStream_t)stream);
    return fallback_impl(nullptr, 3, Frames{bgr0, bgr1, HSFLOW_U8}, rows, cols, batch, counts_f,
                         counts_b, fb, InterpOut{times, nt, out, dtype_out, flags, trusted, cut},
                         (hipStream_t)stream);
}

size_t hsflow_flow_interp_workspace_bytes(int rows, int cols, int batch, int levels) {
    if (!sizes_ok(rows, cols, batch) || levels < 1 || levels > HSFLOW_MAX_LEVELS) return 0;
    return interp_layout(rows, cols, batch, levels, 1).bytes;
}

int hsflow_flow_interp_lv_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                                 int batch, int levels, int finest, int warps, int median,
                                 int window, int iters, float alpha, float rel, float abs_thr,
                                 const float *times, int nt, void *out, int dtype_out,
                                 uint8_t *flags, uint32_t *trusted, const hsflow_prefilter *pf,
                                 const hsflow_smoothness *sm, const hsflow_flow_init *init,
                                 void *workspace, size_t workspace_bytes, void *stream) {
    DeviceGuard g((hipStream_t)stream);
    const SolveSpec S{rows,   cols,  batch, levels, finest, warps, median,
                      window, iters, alpha, pf,     sm,     init,  0};
    return flow_interp_impl(nullptr, S, 1, Frames{I0, I1, dtype_in}, rel, abs_thr,
                            InterpOut{times, nt, out, dtype_out, flags, trusted}, workspace,
                            workspace_bytes, (hipStream_t)stream);
}

int hsflow_flow_interp_init_device(const void *I0, const void *I1, int dtype_in, int rows,
                                   int cols, int batch, int levels, int warps, int median,
                                   int window, int iters, float alpha, float rel, float abs_thr,
                                   const float *times, int nt, void *out, int dtype_out,
                                   uint8_t *flags, uint32_t *trusted, const hsflow_prefilter *pf,
                                   const hsflow_smoothness *sm, const hsflow_flow_init *init,
                                   void *workspace, size_t workspace_bytes, void *stream) {
    return hsflow_flow_interp_lv_device(I0, I1, dtype_in, rows, cols, batch, levels, 0, warps,
                                        median, window, iters, alpha, rel, abs_thr, times, nt, out,
                                        dtype_out, flags, trusted, pf, sm, init, workspace,
                                        workspace_bytes, stream);
}

int hsflow_flow_interp_sm_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                                 int batch, int levels, int warps, int median, int window,
                                 int iters, float alpha, float rel, float abs_thr,
                                 const float *times, int nt, void *out, int dtype_out,
                                 uint8_t *flags, uint32_t *trusted, const hsflow_prefilter *pf,
                                 const hsflow_smoothness *sm, void *workspace,
                                 size_t workspace_bytes, void *stream) {
    return hsflow_flow_interp_init_device(I0, I1, dtype_in, rows, cols, batch, levels, warps,
                                          median, window, iters, alpha, rel, abs_thr, times, nt,
                                          out, dtype_out, flags, trusted, pf, sm, nullptr,
                                          workspace, workspace_bytes, stream);
}

int hsflow_flow_interp_pf_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                                 int batch, int levels, int warps, int median, int window,
                                 int iters, float alpha, float rel, float abs_thr,
                                 const float *times, int nt, void *out, int dtype_out,
                                 uint8_t *flags, uint32_t *trusted, const hsflow_prefilter *pf,
                                 void *workspace, size_t workspace_bytes, void *stream) {
    return hsflow_flow_interp_sm_device(I0, I1, dtype_in, rows, cols, batch, levels, warps, median,
                                        window, iters, alpha, rel, abs_thr, times, nt, out,
                                        dtype_out, flags, trusted, pf, nullptr, workspace,
                                        workspace_bytes, stream);
}

int hsflow_flow_interp_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                              int batch, int levels, int warps, int median, int window,
                              int iters, float alpha, float rel, float abs_thr,
                              const float *times, int nt, void *out, int dtype_out,
                              uint8_t *flags, uint32_t *trusted, void *workspace,
                              size_t workspace_bytes, void *stream) {
    return hsflow_flow_interp_sm_device(I0, I1, dtype_in, rows, cols, batch, levels, warps, median,
                                        window, iters, alpha, rel, abs_thr, times, nt, out,
                                        dtype_out, flags, trusted, nullptr, nullptr, workspace,
                                        workspace_bytes, stream);
}

int hsflow_flow_interp(hsflow_ctx *ctx, const void *I0, const void *I1, int dtype_in, int rows,
                       int cols, size_t in_step0, size_t in_step1, int levels, int warps,
                       int median, int window, int iters, double alpha, float rel, float abs_thr,
                       const float *times, int nt, void *const *out, int dtype_out,
                       size_t out_step, uint8_t *const *flags, size_t flags_step,
                       uint32_t *trusted) {
    const SolveSpec S = host_spec(ctx, rows, cols, levels, warps, median, window, iters, alpha);
    return flow_interp_host(ctx, S, 1, I0, I1, dtype_in, in_step0, in_step1, rel, abs_thr,
                            HostInterpOut{times, nt, out, dtype_out, out_step, flags, flags_step,
                                          trusted});
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
    return frame_interp_impl(nullptr, 3, Frames{bgr0, bgr1, HSFLOW_U8}, rows, cols, batch,
                             FlowsIn{uf, vf, ub, vb, mask_f, mask_b, nullptr},
                             InterpOut{times, nt, out, dtype_out, flags, trusted}, false,
                             (hipStream_t)stream);
}

int hsflow_frame_interp_bgr_proj_device(const uint8_t *bgr0, const uint8_t *bgr1, int rows,
                                        int cols, int batch, const float *uf, const float *vf,
                                        const float *ub, const float *vb, const uint8_t *mask_f,
                                        const uint8_t *mask_b, const uint64_t *cells,
                                        const float *times, int nt, void *out, int dtype_out,
                                        uint8_t *flags, uint32_t *trusted, void *stream) {
    DeviceGuard g((hipStream_t)stream);
    return frame_interp_impl(nullptr, 3, Frames{bgr0, bgr1, HSFLOW_U8}, rows, cols, batch,
                             FlowsIn{uf, vf, ub, vb, mask_f, mask_b, cells},
                             InterpOut{times, nt, out, dtype_out, flags, trusted}, true,
                             (hipStream_t)stream);
}

size_t hsflow_flow_interp_bgr_pj_workspace_bytes(int rows, int cols, int batch, int levels,
                                                 int nt) {
    if (!sizes_ok(rows, cols, batch) || levels < 1 || levels > HSFLOW_MAX_LEVELS || nt < 1 ||
        nt > HSFLOW_MAX_TIMES)
        return 0;
    return interp_layout(rows, cols, batch, levels, 3, nt).bytes;
}

int hsflow_flow_interp_bgr_pj_device(const uint8_t *bgr0, const uint8_t *bgr1, int rows, int cols,
                                     int batch, int levels, int finest, int warps, int median,
                                     int window, int iters, float alpha, float rel,
                                     float abs_thr, const float *times, int nt, int projection,
                                     void *out, int dtype_out, uint8_t *flags, uint32_t *trusted,
                                     const hsflow_prefilter *pf, const hsflow_smoothness *sm,
                                     const hsflow_flow_init *init, void *workspace,
                                     size_t workspace_bytes, void *stream) {
    return hsflow_flow_interp_bgr_fb_device(bgr0, bgr1, rows, cols, batch, levels, finest, warps,
                                            median, window, iters, alpha, rel, abs_thr, times, nt,
                                            projection, out, dtype_out, flags, trusted, nullptr,
                                            pf, sm, init, nullptr, workspace, workspace_bytes,
                                            stream);
}

int hsflow_flow_interp_bgr_fb_device(const uint8_t *bgr0, const uint8_t *bgr1, int rows, int cols,
                                     int batch, int levels, int finest, int warps, int median,
                                     int window, int iters, float alpha, float rel,
                                     float abs_thr, const float *times, int nt, int projection,
                                     void *out, int dtype_out, uint8_t *flags, uint32_t *trusted,
                                     uint8_t *cut, const hsflow_prefilter *pf,
                                     const hsflow_smoothness *sm, const hsflow_flow_init *init,
                                     const hsflow_fallback *fb, void *workspace,
                                     size_t workspace_bytes, void *stream) {
    DeviceGuard g((hipStream_t)stream);
    const SolveSpec S{rows,  cols,  batch, levels, finest, warps,      median, window,
                      iters, alpha, pf,    sm,     init,   projection, fb};
    return flow_interp_impl(nullptr, S, 3, Frames{bgr0, bgr1, HSFLOW_U8}, rel, abs_thr,
                            InterpOut{times, nt, out, dtype_out, flags, trusted, cut}, workspace,
                            workspace_bytes, (hipStream_t)stream);
}

size_t hsflow_flow_interp_bgr_workspace_bytes(int rows, int cols, int batch, int levels) {
    if (!sizes_ok(rows, cols, batch) || levels < 1 || levels > HSFLOW_MAX_LEVELS) return 0;
    return interp_layout(rows, cols, batch, levels, 3).bytes;
}

int hsflow_flow_interp_bgr_lv_device(const uint8_t *bgr0, const uint8_t *bgr1, int rows, int cols,
                                     int batch, int levels, int finest, int warps, int median,
                                     int window, int iters, float alpha, float rel,
                                     float abs_thr, const float *times, int nt, void *out,
                                     int dtype_out, uint8_t *flags, uint32_t *trusted,
                                     const hsflow_prefilter *pf, const hsflow_smoothness *sm,
                                     const hsflow_flow_init *init, void *workspace,
                                     size_t workspace_bytes, void *stream) {
    DeviceGuard g((hipStream_t)stream);
    const SolveSpec S{rows,   cols,  batch, levels, finest, warps, median,
                      window, iters, alpha, pf,     sm,     init,  0};
    return flow_interp_impl(nullptr, S, 3, Frames{bgr0, bgr1, HSFLOW_U8}, rel, abs_thr,
                            InterpOut{times, nt, out, dtype_out, flags, trusted}, workspace,
                            workspace_bytes, (hipStream_t)stream);
}

int hsflow_flow_interp_bgr_init_device(const uint8_t *bgr0, const uint8_t *bgr1, int rows,
                                       int cols, int batch, int levels, int warps, int median,
                                       int window, int iters, float alpha, float rel,
                                       float abs_thr, const float *times, int nt, void *out,
                                       int dtype_out, uint8_t *flags, uint32_t *trusted,
                                       const hsflow_prefilter *pf, const hsflow_smoothness *sm,
                                       const hsflow_flow_init *init, void *workspace,
                                       size_t workspace_bytes, void *stream) {
    return hsflow_flow_interp_bgr_lv_device(bgr0, bgr1, rows, cols, batch, levels, 0, warps,
                                            median, window, iters, alpha, rel, abs_thr, times, nt,
                                            out, dtype_out, flags, trusted, pf, sm, init,
                                            workspace, workspace_bytes, stream);
}

int hsflow_flow_interp_bgr_sm_device(const uint8_t *bgr0, const uint8_t *bgr1, int rows, int cols,
                                     int batch, int levels, int warps, int median, int window,
                                     int iters, float alpha, float rel, float abs_thr,
                                     const float *times, int nt, void *out, int dtype_out,
                                     uint8_t *flags, uint32_t *trusted, const hsflow_prefilter *pf,
                                     const hsflow_smoothness *sm, void *workspace,
                                     size_t workspace_bytes, void *stream) {
    return hsflow_flow_interp_bgr_init_device(bgr0, bgr1, rows, cols, batch, levels, warps, median,
                                              window, iters, alpha, rel, abs_thr, times, nt, out,
                                              dtype_out, flags, trusted, pf, sm, nullptr,
                                              workspace, workspace_bytes, stream);
}

int hsflow_flow_interp_bgr_pf_device(const uint8_t *bgr0, const uint8_t *bgr1, int rows, int cols,
                                     int batch, int levels, int warps, int median, int window,
                                     int iters, float alpha, float rel, float abs_thr,
                                     const float *times, int nt, void *out, int dtype_out,
                                     uint8_t *flags, uint32_t *trusted, const hsflow_prefilter *pf,
                                     void *workspace, size_t workspace_bytes, void *stream) {
    return hsflow_flow_interp_bgr_sm_device(bgr0, bgr1, rows, cols, batch, levels, warps, median,
                                            window, iters, alpha, rel, abs_thr, times, nt, out,
                                            dtype_out, flags, trusted, pf, nullptr, workspace,
                                            workspace_bytes, stream);
}

int hsflow_flow_interp_bgr_device(const uint8_t *bgr0, const uint8_t *bgr1, int rows, int cols,
                                  int batch, int levels, int warps, int median, int window,
                                  int iters, float alpha, float rel, float abs_thr,
                                  const float *times, int nt, void *out, int dtype_out,
                                  uint8_t *flags, uint32_t *trusted, void *workspace,
                                  size_t workspace_bytes, void *stream) {
    return hsflow_flow_interp_bgr_sm_device(bgr0, bgr1, rows, cols, batch, levels, warps, median,
                                            window, iters, alpha, rel, abs_thr, times, nt, out,
                                            dtype_out, flags, trusted, nullptr, nullptr, workspace,
                                            workspace_bytes, stream);
}

int hsflow_flow_interp_bgr(hsflow_ctx *ctx, const uint8_t *bgr0, const uint8_t *bgr1, int rows,
                           int cols, size_t bgr_step0, size_t bgr_step1, int levels, int warps,
                           int median, int window, int iters, double alpha, float rel,
                           float abs_thr, const float *times, int nt, void *const *out,
                           int dtype_out, size_t out_step, uint8_t *const *flags,
                           size_t flags_step, uint32_t *trusted) {
    const SolveSpec S = host_spec(ctx, rows, cols, levels, warps, median, window, iters, alpha);
    return flow_interp_host(ctx, S, 3, bgr0, bgr1, HSFLOW_U8, bgr_step0, bgr_step1, rel, abs_thr,
                            HostInterpOut{times, nt, out, dtype_out, out_step, flags, flags_step,
                                          trusted});
}

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
    const JacobiSpec J{rows, cols, batch, window, iters, alpha, true, true};
    return jacobi_weighted_impl(nullptr, J, g, u, v, workspace, workspace_bytes,
                                (hipStream_t)stream);
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

int hsflow_downflow_device(const float *u, const float *v, int rows, int cols, float *uc,
                           float *vc, int rc, int cc, int batch, void *stream) {
    DeviceGuard g((hipStream_t)stream);
    return downflow_impl(nullptr, u, v, rows, cols, uc, vc, rc, cc, batch, (hipStream_t)stream);
}

int hsflow_upflow_bilinear_device(const float *uc, const float *vc, int rc, int cc, float *u,
                                  float *v, int rows, int cols, int batch, void *stream) {
    DeviceGuard g((hipStream_t)stream);
    return upflow_bilinear_impl(nullptr, uc, vc, rc, cc, u, v, rows, cols, batch,
                                (hipStream_t)stream);
}

int hsflow_ctx_set_finest_level(hsflow_ctx *ctx, int finest) {
    if (!ctx) return fail(nullptr, HSFLOW_ERR_ARG, "null context");
    if (finest < 0 || finest >= HSFLOW_MAX_LEVELS)
        return fail(ctx, HSFLOW_ERR_ARG, "finest level %d outside [0, %d]", finest,
                    HSFLOW_MAX_LEVELS - 1);
    ctx->finest = finest;
    return HSFLOW_OK;
}

int hsflow_ctx_set_projection(hsflow_ctx *ctx, int projection) {
    if (!ctx) return fail(nullptr, HSFLOW_ERR_ARG, "null context");
    const int rc = check_projection(ctx, projection);
    if (rc) return rc;
    ctx->projection = projection;
    return HSFLOW_OK;
}

int hsflow_ctx_projection(const hsflow_ctx *ctx) {
    if (!ctx) return fail(nullptr, HSFLOW_ERR_ARG, "null context");
    return ctx->projection;
}

int hsflow_ctx_set_fallback(hsflow_ctx *ctx, const hsflow_fallback *fb) {
    if (!ctx) return fail(nullptr, HSFLOW_ERR_ARG, "null context");
    if (fb_on(fb)) {
        int rc = check_fallback(ctx, fb);
        if (rc) return rc;
        ctx->fb = *fb;
    } else {
        ctx->fb = hsflow_fallback{HSFLOW_FALLBACK_OFF, 0.0f};
    }
    return HSFLOW_OK;
}

int hsflow_ctx_fallback(const hsflow_ctx *ctx, hsflow_fallback *fb) {
    if (!ctx || !fb) return fail(nullptr, HSFLOW_ERR_ARG, "null %s", ctx ? "fallback" : "context");
    *fb = ctx->fb;
    return HSFLOW_OK;
}

int hsflow_ctx_last_cut(const hsflow_ctx *ctx) { return ctx ? ctx->last_cut : -1; }

int hsflow_ctx_finest_level(const hsflow_ctx *ctx) {
    if (!ctx) return fail(nullptr, HSFLOW_ERR_ARG, "null context");
    return ctx->finest;
}

int hsflow_flow_predict_device(const float *ub, const float *vb, int rows, int cols, int batch,
                               float *uf_next, float *vf_next, float *ub_next, float *vb_next,
                               void *stream) {
    DeviceGuard g((hipStream_t)stream);
    return predict_impl(nullptr, ub, vb, rows, cols, batch, uf_next, vf_next, ub_next, vb_next,
                        (hipStream_t)stream);
}

int hsflow_ctx_set_temporal(hsflow_ctx *ctx, int on) {
    if (!ctx) return fail(nullptr, HSFLOW_ERR_ARG, "null context");
    ctx->temporal = on ? 1 : 0;
    ctx->pred_valid = false;
    return HSFLOW_OK;
}

int hsflow_ctx_temporal(const hsflow_ctx *ctx) {
    if (!ctx) return fail(nullptr, HSFLOW_ERR_ARG, "null context");
    return ctx->temporal;
}

int hsflow_ctx_temporal_reset(hsflow_ctx *ctx) {
    if (!ctx) return fail(nullptr, HSFLOW_ERR_ARG, "null context");
    ctx->pred_valid = false;
    return HSFLOW_OK;
}

int hsflow_chroma_interp_device(const uint8_t *c0, const uint8_t *c1, int layout, int rows,
                                int cols, int batch, const float *uf, const float *vf,
                                const float *ub, const float *vb, const uint32_t *counts_f,
                                const uint32_t *counts_b, const hsflow_fallback *fb,
                                const float *times, int nt, void *out_c, int dtype_out,
                                void *stream) {
    DeviceGuard g((hipStream_t)stream);
    const ChromaIO C{c0, c1, HSFLOW_U8, layout, times, nt, out_c, dtype_out};
    return chroma_interp_impl(nullptr, C, rows, cols, batch,
                              FlowsIn{uf, vf, ub, vb, nullptr, nullptr, nullptr}, counts_f,
                              counts_b, fb, false, (hipStream_t)stream);
}

size_t hsflow_flow_interp_yuv_workspace_bytes(int rows, int cols, int batch, int levels,
                                              int fallback) {
    if (!sizes_ok(rows, cols, batch) || (rows | cols) & 1 || levels < 1 ||
        levels > HSFLOW_MAX_LEVELS)
        return 0;
    return interp_layout(rows, cols, batch, levels, 1, 0, fallback != 0).bytes;
}

int hsflow_flow_interp_yuv_device(const uint8_t *y0, const uint8_t *c0, const uint8_t *y1,
                                  const uint8_t *c1, int layout, int rows, int cols, int batch,
                                  int levels, int finest, int warps, int median, int window,
                                  int iters, float alpha, float rel, float abs_thr,
                                  const float *times, int nt, void *out_y, void *out_c,
                                  int dtype_out, uint8_t *flags, uint32_t *trusted, uint8_t *cut,
                                  const hsflow_prefilter *pf, const hsflow_smoothness *sm,
                                  const hsflow_flow_init *init, const hsflow_fallback *fb,
                                  void *workspace, size_t workspace_bytes, void *stream) {
    DeviceGuard g((hipStream_t)stream);
    const SolveSpec S{rows,  cols,  batch, levels, finest, warps, median, window,
                      iters, alpha, pf,    sm,     init,   0,     fb};
    return flow_interp_yuv_impl(nullptr, S, Frames{y0, y1, HSFLOW_U8},
                                ChromaIO{c0, c1, HSFLOW_U8, layout, times, nt, out_c, dtype_out},
                                rel, abs_thr,
                                InterpOut{times, nt, out_y, dtype_out, flags, trusted, cut},
                                workspace, workspace_bytes, (hipStream_t)stream);
}

int hsflow_flow_interp_yuv(hsflow_ctx *ctx, const uint8_t *f0, const uint8_t *f1, int layout,
                           int rows, int cols, int levels, int warps, int median, int window,
                           int iters, double alpha, float rel, float abs_thr, const float *times,
                           int nt, void *const *out, int dtype_out, uint8_t *const *flags,
                           uint32_t *trusted) {
    const SolveSpec S = host_spec(ctx, rows, cols, levels, warps, median, window, iters, alpha);
    return flow_interp_yuv_host(ctx, S, f0, f1, HSFLOW_U8, layout, rel, abs_thr, times, nt, -1,
                                out, dtype_out, flags, trusted);
}

int hsflow_cells_down_device(const uint64_t *cells, int rows, int cols, int batch, int nt,
                             uint64_t *cells_c, void *stream) {
    DeviceGuard g((hipStream_t)stream);
    return cells_down_impl(nullptr, cells, rows, cols, batch, nt, cells_c, (hipStream_t)stream);
}

int hsflow_chroma_interp_proj_device(const uint8_t *c0, const uint8_t *c1, int layout, int rows,
                                     int cols, int batch, const float *uf, const float *vf,
                                     const float *ub, const float *vb, const uint64_t *cells,
                                     const uint32_t *counts_f, const uint32_t *counts_b,
                                     const hsflow_fallback *fb, const float *times, int nt,
                                     void *out_c, int dtype_out, void *stream) {
    DeviceGuard g((hipStream_t)stream);
    const ChromaIO C{c0, c1, HSFLOW_U8, layout, times, nt, out_c, dtype_out};
    return chroma_interp_impl(nullptr, C, rows, cols, batch,
                              FlowsIn{uf, vf, ub, vb, nullptr, nullptr, cells}, counts_f, counts_b,
                              fb, true, (hipStream_t)stream);
}

size_t hsflow_flow_interp_yuv_pj_workspace_bytes(int rows, int cols, int batch, int levels,
                                                 int nt, int projection, int fallback) {
    if (!sizes_ok(rows, cols, batch) || (rows | cols) & 1 || levels < 1 ||
        levels > HSFLOW_MAX_LEVELS || nt < 1 || nt > HSFLOW_MAX_TIMES ||
        (projection != 0 && projection != 1))
        return 0;
    return interp_layout(rows, cols, batch, levels, 1, projection ? nt : 0, fallback != 0).bytes;
}

int hsflow_flow_interp_yuv_pj_device(const uint8_t *y0, const uint8_t *c0, const uint8_t *y1,
                                     const uint8_t *c1, int layout, int rows, int cols, int batch,
                                     int levels, int finest, int warps, int median, int window,
                                     int iters, float alpha, float rel, float abs_thr,
                                     const float *times, int nt, int projection, void *out_y,
                                     void *out_c, int dtype_out, uint8_t *flags,
                                     uint32_t *trusted, uint8_t *cut, const hsflow_prefilter *pf,
                                     const hsflow_smoothness *sm, const hsflow_flow_init *init,
                                     const hsflow_fallback *fb, void *workspace,
                                     size_t workspace_bytes, void *stream) {
    DeviceGuard g((hipStream_t)stream);
    const SolveSpec S{rows,  cols,  batch, levels, finest, warps,      median, window,
                      iters, alpha, pf,    sm,     init,   projection, fb};
    return flow_interp_yuv_impl(nullptr, S, Frames{y0, y1, HSFLOW_U8},
                                ChromaIO{c0, c1, HSFLOW_U8, layout, times, nt, out_c, dtype_out},
                                rel, abs_thr,
                                InterpOut{times, nt, out_y, dtype_out, flags, trusted, cut},
                                workspace, workspace_bytes, (hipStream_t)stream);
}

int hsflow_flow_interp_yuv_pj(hsflow_ctx *ctx, const uint8_t *f0, const uint8_t *f1, int layout,
                              int rows, int cols, int levels, int warps, int median, int window,
                              int iters, double alpha, float rel, float abs_thr,
                              const float *times, int nt, int projection, void *const *out,
                              int dtype_out, uint8_t *const *flags, uint32_t *trusted) {
    const SolveSpec S = host_spec(ctx, rows, cols, levels, warps, median, window, iters, alpha);
    return flow_interp_yuv_host(ctx, S, f0, f1, HSFLOW_U8, layout, rel, abs_thr, times, nt,
                                projection < 0 ? 2 : projection, out, dtype_out, flags, trusted);
}

int hsflow_chroma_interp16_device(const uint16_t *c0, const uint16_t *c1, int layout, int rows,
                                  int cols, int batch, const float *uf, const float *vf,
                                  const float *ub, const float *vb, const uint64_t *cells,
                                  const uint32_t *counts_f, const uint32_t *counts_b,
                                  const hsflow_fallback *fb, const float *times, int nt,
                                  void *out_c, int dtype_out, void *stream) {
    DeviceGuard g((hipStream_t)stream);
    return chroma_interp_impl(nullptr,
                              ChromaIO{c0, c1, HSFLOW_U16, layout, times, nt, out_c, dtype_out},
                              rows, cols, batch, FlowsIn{uf, vf, ub, vb, nullptr, nullptr, cells},
                              counts_f, counts_b, fb, cells != nullptr, (hipStream_t)stream);
}

int hsflow_flow_interp_yuv16_device(const uint16_t *y0, const uint16_t *c0, const uint16_t *y1,
                                    const uint16_t *c1, int layout, int rows, int cols, int batch,
                                    int levels, int finest, int warps, int median, int window,
                                    int iters, float alpha, float rel, float abs_thr,
                                    const float *times, int nt, int projection, void *out_y,
                                    void *out_c, int dtype_out, uint8_t *flags,
                                    uint32_t *trusted, uint8_t *cut, const hsflow_prefilter *pf,
                                    const hsflow_smoothness *sm, const hsflow_flow_init *init,
                                    const hsflow_fallback *fb, void *workspace,
                                    size_t workspace_bytes, void *stream) {
    DeviceGuard g((hipStream_t)stream);
    const SolveSpec S{rows,  cols,  batch, levels, finest, warps,      median, window,
                      iters, alpha, pf,    sm,     init,   projection, fb};
    return flow_interp_yuv_impl(nullptr, S, Frames{y0, y1, HSFLOW_U16},
                                ChromaIO{c0, c1, HSFLOW_U16, layout, times, nt, out_c, dtype_out},
                                rel, abs_thr,
                                InterpOut{times, nt, out_y, dtype_out, flags, trusted, cut},
                                workspace, workspace_bytes, (hipStream_t)stream);
}

int hsflow_flow_interp_yuv16(hsflow_ctx *ctx, const uint16_t *f0, const uint16_t *f1, int layout,
                             int rows, int cols, int levels, int warps, int median, int window,
                             int iters, double alpha, float rel, float abs_thr,
                             const float *times, int nt, int projection, void *const *out,
                             int dtype_out, uint8_t *const *flags, uint32_t *trusted) {
    const SolveSpec S = host_spec(ctx, rows, cols, levels, warps, median, window, iters, alpha);
    return flow_interp_yuv_host(ctx, S, f0, f1, HSFLOW_U16, layout, rel, abs_thr, times, nt,
                                projection < 0 ? 2 : projection, out, dtype_out, flags, trusted);
}

int hsflow_chroma_interp_proj_blocks_per_cu(void) { return hsflow::chroma_proj_blocks_per_cu(); }

int hsflow_chroma_interp_blocks_per_cu(void) { return hsflow::chroma_blocks_per_cu(); }

int hsflow_set_chroma_nv12_loads(int wide) { return hsflow::set_chroma_nv12_wide_loads(wide); }

}  // extern "C"
