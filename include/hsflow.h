/*
 * hsflow.h -- C ABI of libhsflow.so, the MI355X-native Horn-Schunck solver.
 *
 * Drop-in boundary.  The reference (liuyang9609/Cpp-Optical-Flow) exposes
 * its hot path as a header-style C++ class compiled into the caller
 * (HornSchunckOF/hornSchunck.cpp:8-76, pulled in by main.cpp:8):
 *
 *   hornSchunck(int windowSize, int maxIterations, double alpha)   :13-17
 *   void getGradients(cv::Mat prev, cv::Mat next,
 *                     cv::Mat& gx, cv::Mat& gy, cv::Mat& gt)       :19-41
 *   void getFlow(cv::Mat prev, cv::Mat next, cv::Mat& u, cv::Mat& v) :43-75
 *
 * Its FFI surface is therefore C++/cv::Mat; the functions below are the
 * plain-pointer entry points that surface lowers onto (include/hornSchunck.hpp
 * is the cv::Mat adapter with the reference's exact signatures; INTEGRATION.md
 * shows the binding).  No torch or OpenCV types cross this boundary.
 *
 * Semantics (identical to the reference, computed in fp32 on the GPU):
 *   Ix, Iy = 3x3 Sobel of I0 (reflect-101 border), It = I1 - I0;
 *   u = v = 0; repeat `iters` times:
 *     ubar, vbar = windowSize x windowSize box mean (zero border, anchor
 *                  windowSize - windowSize/2 - 1)
 *     c = (Ix ubar + Iy vbar + It) / (alpha^2 + Ix^2 + Iy^2)
 *     u = ubar - Ix c;  v = vbar - Iy c
 * Parity: max|u - u_ref| / max|u_ref| <= 1e-4 against the float64 reference.
 *
 * Threading: a context is used by one host thread at a time.  Host-buffer
 * calls are blocking (as the reference is).  *_device calls are
 * stream-ordered, never synchronise the host and never allocate, so they may
 * be captured into a hipGraph.
 */
#ifndef HSFLOW_H
#define HSFLOW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HSFLOW_VERSION 20000 /* 2.0.0: separate row steps for I0 and I1 */

/* Status codes (0 ok, <0 error).  The reference has no codes: OpenCV throws
 * cv::Exception (e.g. size mismatch in multiply, hornSchunck.cpp:63-70);
 * the cv::Mat adapter maps every non-zero status to an exception. */
enum {
    HSFLOW_OK = 0,
    HSFLOW_ERR_ARG = -1,   /* null pointer, bad size/window/dtype/stride     */
    HSFLOW_ERR_HIP = -2,   /* HIP runtime error; see hsflow_last_error()      */
    HSFLOW_ERR_OOM = -3,   /* device allocation failed                        */
    HSFLOW_ERR_NODEV = -4, /* no HIP device / device index out of range       */
    HSFLOW_ERR_SIZE = -5   /* prev/next sizes differ (main.cpp:71-73)         */
};

/* Element types.  U8 = CV_8UC1, F32 = CV_32FC1, F64 = CV_64FC1,
 * F16 = CV_16FC1 (config 5 inputs; input only), U16 = CV_16UC1 (the 16-bit
 * YUV 4:2:0 calls only, "16-bit YUV 4:2:0" below; every other call refuses it
 * as it refuses an unknown code). */
enum { HSFLOW_U8 = 0, HSFLOW_F32 = 1, HSFLOW_F64 = 2, HSFLOW_F16 = 3, HSFLOW_U16 = 4 };

/* Largest windowSize accepted (hornSchunck.cpp:53 allows any; OpenCV would
 * take a few seconds per iteration at this size already). */
#define HSFLOW_MAX_WINDOW 63

typedef struct hsflow_ctx hsflow_ctx;

int hsflow_version(void);
const char *hsflow_status_string(int status);

/* Build flags of the loaded library: 0 for every build (the diagnostic
 * build of v2.0 is retired; the library reads no environment variable). */
int hsflow_build_flags(void);

/* Context = device + stream + cached device buffers (grow-only). */
int hsflow_create(hsflow_ctx **ctx, int device);
void hsflow_destroy(hsflow_ctx *ctx);
const char *hsflow_last_error(const hsflow_ctx *ctx);
/* The HIP stream the host-buffer calls run on (hipStream_t as void*). */
void *hsflow_stream(hsflow_ctx *ctx);

/* ---- host-buffer, blocking: the reference's two methods ---------------- */

/* hornSchunck::getFlow (hornSchunck.cpp:43-75).  I0/I1: rows x cols, element
 * type dtype_in, row steps in BYTES, one per frame (cv::Mat::step of
 * imagePrev and imageNext; non-continuous ROIs ok, the two may differ).
 * u/v: rows x cols of dtype_out (HSFLOW_F64 = what the reference returns,
 * CV_64FC1, or HSFLOW_F32), row step out_step bytes.  Frames are uploaded as
 * they are; CV_64FC1 frames get their Sobel sums in float64 on the device
 * (hornSchunck.cpp:23-28), each gradient rounded to f32 once. */
int hsflow_flow(hsflow_ctx *ctx, const void *I0, const void *I1, int dtype_in,
                int rows, int cols, size_t in_step0, size_t in_step1, int window,
                int iters, double alpha, void *u, void *v, int dtype_out,
                size_t out_step);

/* Frame-parallel getFlow over several GPUs of this node from ONE process,
 * for C/C++ callers that do not run one process per GPU (the multi-rank
 * form is cpp-optical-flow_amd/frame_parallel.py over torch.distributed).
 * Pair j -- host frames I0[j], I1[j] (rows x cols, dtype_in, row steps
 * in_step0 / in_step1), host outputs u[j], v[j] (dtype_out, out_step) -- is
 * solved on devices[j % n_devices], each listed device by its own host
 * thread, context and stream, exactly as hsflow_flow (same bits).  A device
 * may be listed twice (two streams on one GPU).  Blocking; returns the
 * first error, its message in hsflow_last_error(NULL).  The per-device
 * contexts are kept by the library across calls (no allocation or device
 * synchronisation per call once warm); a context whose call failed is
 * destroyed, not reused.  Concurrent calls that list the same device slot
 * are serialised on that slot only. */
int hsflow_flow_multi(const int *devices, int n_devices, int batch,
                      const void *const *I0, const void *const *I1, int dtype_in, int rows,
                      int cols, size_t in_step0, size_t in_step1, int window, int iters,
                      double alpha, void *const *u, void *const *v, int dtype_out,
                      size_t out_step);

/* Destroys every context hsflow_flow_multi keeps (device buffers, pinned
 * stages, streams); the next multi call creates them again.  Waits for
 * multi calls in progress. */
void hsflow_flow_multi_release(void);

/* hornSchunck::getGradients (hornSchunck.cpp:19-41): gx, gy, gt. */
int hsflow_gradients(hsflow_ctx *ctx, const void *I0, const void *I1, int dtype_in,
                     int rows, int cols, size_t in_step0, size_t in_step1, void *gx,
                     void *gy, void *gt, int dtype_out, size_t out_step);

/* ---- device pointers, stream-ordered ------------------------------------
 * A batch is `batch` (1..65535) independent frame pairs stored back to back:
 * I0[b][rows][cols], dense (pitch = cols elements), likewise u, v.
 * Inputs are U8, F16, F32 or F64.  Outputs are f32.  `stream` is a hipStream_t
 * (NULL = the default stream of the CURRENT device: then the caller must
 * make the buffers' device current); a non-null stream's own device runs the
 * call, whatever device is current.  `workspace` is device memory of at least
 * hsflow_workspace_bytes(rows, cols, batch) bytes, 256-byte aligned.
 *
 * Sizes.  rows in 1..262140, cols >= 1 and rows * cols <= 2^29 - 4 pixels
 * (536870908: the byte offset 0x7FFFFFF0 that the Jacobi kernels give a lane
 * outside the image must lie past the end of a plane).  Anything else is
 * HSFLOW_ERR_ARG, "bad size", before any device work, and
 * hsflow_workspace_bytes returns 0 for it.
 *
 * Memory contract of the device calls (tests/test_footprint.py holds every
 * entry point below to it):
 * - Alignment.  A plane needs the alignment of its element and no more: 4
 *   bytes for every f32 plane (u, v, flows, init planes, err, gx / gy / gt, F32
 *   frames) and for counts / trusted, 2 for F16 frames, 8 for F64 frames, none
 *   for U8 and BGR frames, masks, flags and 8-bit outputs.  Only a workspace
 *   must be 256-byte aligned.  The kernels that move 8 or 16 bytes per lane --
 *   K2's and K4's column pairs, K4's interleaved state, which lives in the
 *   caller's u and v between two passes -- issue dword-aligned buffer accesses,
 *   which gfx950 takes at any 4-byte address: the same bits at every alignment.
 *   hsflow_upflow_bilinear_device uses its 8-byte loads and 16-byte stores only
 *   where the planes it is given are aligned for them, 4-byte accesses
 *   elsewhere: the same bits again.
 * - Footprint.  A call writes its outputs and the first <its size function>
 *   bytes of its workspace (hsflow_prefilter_planes_bytes more where a
 *   prefilter is on) and nothing else; it never writes an input.
 * - Prior contents.  What a workspace holds before a call never matters: any
 *   bytes, another call's leftovers included, give the same outputs.  The one
 *   hand-over is the documented one: the gradients hsflow_gradients_device /
 *   hsflow_warp_gradients_device leave for the hsflow_jacobi_device /
 *   hsflow_jacobi_weighted_device that follows in the same workspace.
 * - u, v of a cold solve (hsflow_flow_device, hsflow_jacobi_device without
 *   warm_start, hsflow_flow_pyramid_device, a warped solve without an init, a
 *   warped solve with finest > 0 with or without one) are write-only: never
 *   read, every element written. */
size_t hsflow_workspace_bytes(int rows, int cols, int batch);

/* Full solve: gradients + `iters` Jacobi iterations from u = v = 0.
 * u, v and the workspace must not overlap the frames or each other: the
 * first Jacobi pass may read the frames while it writes u and v
 * (hsflow_set_first_pass_fusion). */
int hsflow_flow_device(const void *I0, const void *I1, int dtype_in, int rows,
                       int cols, int batch, int window, int iters, float alpha,
                       float *u, float *v, void *workspace, size_t workspace_bytes,
                       void *stream);

/* The two phases separately (bench / profiling / warm starts):
 * gradients into the workspace (optionally also to gx/gy/gt, may be NULL)... */
int hsflow_gradients_device(const void *I0, const void *I1, int dtype_in, int rows,
                            int cols, int batch, float *gx, float *gy, float *gt,
                            void *workspace, size_t workspace_bytes, void *stream);
/* ...then `iters` Jacobi iterations from the gradients in the workspace,
 * starting from (u, v) when warm_start != 0, else from zero. */
int hsflow_jacobi_device(int rows, int cols, int batch, int window, int iters,
                         float alpha, int warm_start, float *u, float *v,
                         void *workspace, size_t workspace_bytes, void *stream);

/* Iterations fused per Jacobi launch (temporal blocking depth) the library
 * picks for this shape; 0 = automatic (default).  Results are bit-identical
 * for every depth.  Process-wide; not thread-safe against running solves.
 * The weighted passes of the flow-driven smoothness term (below) take k
 * where they are built for it (window 5: 2..4, window 3: 3, 4, 6), else their
 * own default (3 and 6). */
int hsflow_set_iters_per_launch(int k);
int hsflow_iters_per_launch(int rows, int cols, int batch, int window);

/* Kernel of the Jacobi passes (one launch per pass of iters_per_launch
 * iterations): 0 = automatic (default: K4 streaming strips where built --
 * windowSize 3 and 5 at their default depth -- K2 register tiles
 * elsewhere), 2 = K2 everywhere, 4 = K4 where built.  Every choice gives
 * identical bits.  Process-wide; not thread-safe against running solves. */
int hsflow_set_jacobi_kernel(int k);

/* Rows per segment of the K4 streaming passes (each wave streams one
 * segment of one 128-column strip); 0 = automatic (default, a cost model of
 * waves per SIMD and row loads).  Results are bit-identical for every
 * choice.  Process-wide; not thread-safe against running solves. */
int hsflow_set_strip_rows(int seg_rows);

/* Name of the kernel that runs the full-depth Jacobi passes of a solve of
 * this shape under the current settings ("hs_jacobi_strip_kernel",
 * "hs_jacobi_wg_kernel", "hs_jacobi_kernel" or "hs_jacobi_generic_kernel");
 * a static string.  For profiles and the bench's roofline record. */
const char *hsflow_jacobi_kernel_name(int rows, int cols, int batch, int window);

/* Rows per K4 segment that a solve of this shape uses under the current
 * settings (hsflow_set_strip_rows, else the automatic choice); 0 when its
 * full-depth passes do not run K4.  For profiles and tests. */
int hsflow_strip_seg_rows(int rows, int cols, int batch, int window);

/* Batches of >= 2 pairs are split over side streams (forked from and joined
 * back to the caller's stream with events) so that concurrent Jacobi
 * launches overlap.  0 = automatic (default): 2 streams for eager calls, no
 * split while the caller's stream is being captured (on ROCm 7.2 a stream
 * forked inside a capture from a capturing stream other than the capture's
 * origin crashes hipStreamEndCapture, and the library cannot tell the
 * origin apart); n >= 1 = up to n streams always (n >= 2 under capture only
 * when the caller captures on the origin stream itself).  Process-wide.
 * hsflow_max_streams returns the current setting. */
int hsflow_set_max_streams(int n);
int hsflow_max_streams(void);

/* A cold solve that takes no gradient planes (hsflow_flow_device, the
 * host-buffer hsflow_flow / hsflow_flow_bgr, the pyramid's coarsest level)
 * whose passes run K4, with at least one full-depth pass, on u8, f16 or f32
 * frames computes the gradients inside its first pass instead of in a
 * kernel of their own in front of it (K1).  on = 1 (default) fuses, 0 runs
 * K1 first.  (u, v), the workspace's packed gradients and its flags have
 * identical bits either way.  Process-wide; not thread-safe against running
 * solves.  hsflow_first_pass_fusion returns the current setting. */
int hsflow_set_first_pass_fusion(int on);
int hsflow_first_pass_fusion(void);
/* Fused first passes this process has launched so far: one per stream-ordered
 * chain of a solve that took the fused path (a batch split over n side
 * streams counts n).  For tests and profiles: the difference across a call
 * tells whether it fused. */
long long hsflow_first_pass_launches(void);

/* Between two full-depth K4 passes a solve keeps (u, v) interleaved: each
 * column pair's {u0, u1, v0, v1} as one 16-byte group, the even rows in the
 * plane that otherwise holds u and the odd rows in the one that holds v, so a
 * pass moves the state with one 16-byte access per lane where it took two
 * 8-byte ones.  It needs an even height and width (the interleaved rows must
 * fit the two planes they replace; the workspace is what it was) and K4 at
 * its default depth; other shapes, K2 passes, the caller's (u, v) on the way
 * in and every result are planar.  on = 1 (default), 0 keeps every pass
 * planar.  Identical bits either way.  During a solve the caller's u and v
 * hold intermediate state in either form, as before.  Process-wide; not
 * thread-safe against running solves.  hsflow_uv_interleave returns the
 * current setting. */
int hsflow_set_uv_interleave(int on);
int hsflow_uv_interleave(void);
/* How many passes of a Jacobi solve of this shape write their state
 * interleaved under the current settings: every full-depth K4 pass but the
 * last one, 0 where the solve stays planar.  Host only: nothing is launched.
 * (A fused first pass on frames that are not aligned to two elements writes
 * planes: one less.)  HSFLOW_ERR_ARG (< 0) for a bad shape. */
int hsflow_uv_interleave_passes(int rows, int cols, int batch, int window, int iters);
/* Passes launched so far that wrote their state interleaved (per
 * stream-ordered chain, as hsflow_first_pass_launches).  For tests and
 * profiles. */
long long hsflow_uv_interleave_launches(void);

/* Huge-page advice on f64 outputs of the host-buffer calls (hsflow_flow,
 * hsflow_flow_bgr, hsflow_flow_pyramid, hsflow_flow_multi with
 * dtype_out = HSFLOW_F64): before widening the downloaded f32 rows into
 * the caller's CV_64FC1 planes, the library advises MADV_HUGEPAGE over the
 * whole 2 MB extents inside each plane's rows and faults their pages in
 * while the device solve runs (a fresh 4K output: 18.5 ms of 4 KB faults on
 * one thread, ~1.2 ms as 2 MB pages).  The advice STAYS on the caller's
 * allocation after the call (khugepaged may later collapse other parts of
 * it into huge pages); it changes no byte, and memory already resident
 * keeps its pages.  on = 1 (default) advises, 0 does not (the pages are
 * still faulted in ahead, at 4 KB).  Process-wide; returns the previous
 * setting. */
int hsflow_set_output_hugepages(int on);

/* Stream-ordered download of `bytes` from device memory to pinned host
 * memory (hipHostMalloc / torch pin_memory), issued so the runtime moves it
 * with its DMA engines (~46 GB/s over PCIe Gen5) instead of a blit kernel:
 * a download of batch k then overlaps the Jacobi passes of batch k+1 on
 * other streams without taking their workgroup slots (main.cpp:99-104
 * consumes u, v on the host). */
int hsflow_download_device(void *dst, const void *src, size_t bytes, void *stream);

/* ---- coarse-to-fine warm start (north_star config 5) ---------------------
 * The reference's HS has no pyramid; the repository's own multi-resolution
 * code is the precedent (BMOpticalFlow/.../OpticalFlow/MultiResolution.cpp:
 * 9-97 Pyramider, OpticalFlow.cpp:197-210 Add_VectorOffset).  Level l is
 * ceil(rows / 2^l) x ceil(cols / 2^l), made from level l-1 by the 5-tap
 * kernel (2,5,4,5,2)/18 per axis (a = 0.4), stride 2, reflect-101; levels of
 * integer-valued pairs are rounded half-up to integers.  The coarsest level
 * starts from u = v = 0, every finer one from u = 2 u_coarse(y/2, x/2)
 * (likewise v); each level runs `iters` Jacobi iterations of the getFlow
 * loop (hornSchunck.cpp:56-74) on its own gradients.  levels = 1 is
 * hsflow_flow_device exactly. */
#define HSFLOW_MAX_LEVELS 8

/* Size of pyramid level `level` (0 = full size). */
int hsflow_pyramid_level_size(int rows, int cols, int level, int *level_rows,
                              int *level_cols);
size_t hsflow_pyramid_workspace_bytes(int rows, int cols, int batch, int levels);
int hsflow_flow_pyramid_device(const void *I0, const void *I1, int dtype_in, int rows,
                               int cols, int batch, int levels, int window, int iters,
                               float alpha, float *u, float *v, void *workspace,
                               size_t workspace_bytes, void *stream);
/* Host-buffer, blocking form (same conventions as hsflow_flow). */
int hsflow_flow_pyramid(hsflow_ctx *ctx, const void *I0, const void *I1, int dtype_in,
                        int rows, int cols, size_t in_step0, size_t in_step1, int levels,
                        int window, int iters, double alpha, void *u, void *v,
                        int dtype_out, size_t out_step);

/* The pyramid's pieces, for callers that schedule the levels themselves
 * (e.g. cpp-optical-flow_amd/row_bands.py, one 8K pair split over GPUs):
 * levels 1..levels-1 of both frames into caller planes I0_levels[l-1],
 * I1_levels[l-1] (dense f32, batch x level size), rounding decided per pair
 * exactly as hsflow_flow_pyramid_device does; `workspace` as for
 * hsflow_workspace_bytes(rows, cols, batch)... */
int hsflow_pyramid_build_device(const void *I0, const void *I1, int dtype_in, int rows,
                                int cols, int batch, int levels, float *const *I0_levels,
                                float *const *I1_levels, void *workspace,
                                size_t workspace_bytes, void *stream);
/* ...and the warm start of a finer level: u = 2 uc(y/2, x/2), v likewise
 * (rows x cols from rc x cc, dense, batch planes). */
int hsflow_upflow_device(const float *uc, const float *vc, int rc, int cc, float *u,
                         float *v, int rows, int cols, int batch, void *stream);

/* ---- warped coarse-to-fine solve (large displacements) -------------------
 * Every solve above linearises brightness constancy once, around zero flow
 * (the pyramid's coarser result only moves the Jacobi iteration's starting
 * point, not its fixed point), so a motion of more than about a pixel is not
 * recovered.  The warped solve re-linearises around the current flow
 * (u0, v0) at every level:
 *   I1w(y, x) = I1 sampled bilinearly at (y + 8 v0, x + 8 u0)
 *   It'       = (I1w - I0) - Ix u0 - Iy v0
 *   the getFlow loop (hornSchunck.cpp:56-74) from (u0, v0) with It' for It.
 * Units: Ix, Iy are the reference's unnormalised 3x3 Sobel sums (gain 8,
 * hornSchunck.cpp:27-28), so one unit of (u, v) is 8 px: multiply (u, v) by
 * 8 for displacements in pixels.  Each displacement is clamped to [-cols,
 * cols] / [-rows, rows] before it is split into integer and fraction (NaN
 * counts as the lower bound), and the four taps are clamped to the plane
 * (border replicated); zero flow gives It' = I1 - I0 bit for bit.  Ix, Iy
 * equal hsflow_gradients_device's planes bit for bit.
 * The pyramid (levels, rounding) is hsflow_flow_pyramid_device's.  Per level,
 * coarsest first: (u, v) = 0 or 2 (u, v)_coarse(y/2, x/2), then `warps`
 * (1..16) times { gradients around (u, v); `iters` Jacobi iterations
 * warm-started from (u, v) }.  levels = 1, warps = 1 computes what
 * hsflow_flow_device computes (from f32 gradient planes: same values within
 * rounding, not the same bits).  `workspace`: at least
 * hsflow_pyramid_workspace_bytes(rows, cols, batch, levels) bytes -- the warped
 * solve needs nothing beyond the pyramid's, so there is no size function of
 * its own.  All arguments are checked before any device work. */
#define HSFLOW_HAS_WARPED 1

/* Gradients of one level linearised around (u0, v0) (dense f32, batch planes)
 * into the workspace's f32 planes (hsflow_workspace_bytes(rows, cols, batch))
 * and optionally to gx/gy/gt (may be NULL); then
 * hsflow_jacobi_device(warm_start = 1) on (u, v) = (u0, v0) is one warp's
 * solve.  u0/v0 may be the solve's own u/v; they must not overlap the
 * workspace or gx/gy/gt. */
int hsflow_warp_gradients_device(const void *I0, const void *I1, int dtype_in, int rows,
                                 int cols, int batch, const float *u0, const float *v0,
                                 float *gx, float *gy, float *gt, void *workspace,
                                 size_t workspace_bytes, void *stream);
int hsflow_flow_warped_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                              int batch, int levels, int warps, int window, int iters,
                              float alpha, float *u, float *v, void *workspace,
                              size_t workspace_bytes, void *stream);
/* Host-buffer, blocking form (same conventions as hsflow_flow_pyramid). */
int hsflow_flow_warped(hsflow_ctx *ctx, const void *I0, const void *I1, int dtype_in, int rows,
                       int cols, size_t in_step0, size_t in_step1, int levels, int warps,
                       int window, int iters, double alpha, void *u, void *v, int dtype_out,
                       size_t out_step);

/* ---- bidirectional warped solve + forward-backward consistency -----------
 * Horn-Schunck returns a smooth flow at every pixel, also where none exists
 * (ground the next frame covers, the strip that leaves the frame, motion
 * beyond the pyramid's reach, a scene cut).  The forward-backward check
 * marks where a flow can be trusted: solve I0 -> I1 (uf, vf) and I1 -> I0
 * (ub, vb); following uf then ub must lead back to the start.  Per pixel
 * (y, x) of a pair, flows in solver units (8 px per unit, as above):
 *   dx = clamp(8 uf, -cols, cols), dy = clamp(8 vf, -rows, rows)   (NaN -> lower
 *        bound, as hsflow_warp_gradients_device splits its displacements)
 *   ubw, vbw = ub, vb sampled bilinearly at (y + dy, x + dx), taps clamped
 *        to the pair's plane (exact where dx, dy are whole)
 *   d2  = 64 ((uf + ubw)^2 + (vf + vbw)^2)                    px^2
 *   mag = 64 ((uf^2 + vf^2) + (ubw^2 + vbw^2))
 *   err = sqrt(d2)                                             px
 *   out = !(x + dx >= -0.5 && x + dx <= cols - 0.5 &&
 *           y + dy >= -0.5 && y + dy <= rows - 0.5)
 *   mask = out ? HSFLOW_OUT_OF_FRAME
 *              : !(d2 <= rel mag + abs) ? HSFLOW_INCONSISTENT : HSFLOW_CONSISTENT
 * The comparisons are negated: a NaN anywhere gives a non-zero mask, and a NaN
 * or infinite uf/vf is out of frame by the clamp; a d2 beyond f32's range is
 * inconsistent, as it is in exact arithmetic.  The half-pixel rim keeps a
 * zero flow at a border pixel in the frame whatever its last bit says.
 * rel, abs: finite, >= 0; 0.01 and 0.5 are Sundaram, Brox and Keutzer's (ECCV
 * 2010).  No index leaves a pair's plane, whatever the flows hold. */
#define HSFLOW_HAS_CONSISTENCY 1
#define HSFLOW_CONSISTENT 0
#define HSFLOW_INCONSISTENT 1
#define HSFLOW_OUT_OF_FRAME 2
#define HSFLOW_CONSISTENCY_REL 0.01f
#define HSFLOW_CONSISTENCY_ABS 0.5f

/* The check alone: (uf, vf) against (ub, vb), dense f32 [batch][rows][cols].
 * Outputs, each may be NULL but not all three: err (f32 plane, px), mask (u8
 * plane, values above), counts (uint32[batch][3], pixels per class; zeroed
 * stream-ordered by the call, integer sums: the same bytes every run).  The
 * outputs must not overlap the inputs.  Stream-ordered, no workspace. */
int hsflow_flow_consistency_device(const float *uf, const float *vf, const float *ub,
                                   const float *vb, int rows, int cols, int batch, float rel,
                                   float abs_thr, float *err, uint8_t *mask, uint32_t *counts,
                                   void *stream);

/* Both directions and both checks in one call.  (uf, vf) is
 * hsflow_flow_warped_device(I0, I1, ...) and (ub, vb) is
 * hsflow_flow_warped_device(I1, I0, ...), bit for bit; all four are required.
 * Then the check runs forward (uf, vf against ub, vb -> err_f, mask_f,
 * counts_f) and backward (roles swapped -> err_b, mask_b, counts_b); the six
 * are optional, and a direction with none given launches no check.
 * `workspace`: at least hsflow_flow_bidir_workspace_bytes(rows, cols, batch,
 * levels) bytes, 256-byte aligned.  Stream-ordered, never allocates or
 * synchronises, capturable; all arguments are checked before any device work. */
size_t hsflow_flow_bidir_workspace_bytes(int rows, int cols, int batch, int levels);
int hsflow_flow_bidir_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                             int batch, int levels, int warps, int window, int iters,
                             float alpha, float rel, float abs_thr, float *uf, float *vf,
                             float *ub, float *vb, float *err_f, uint8_t *mask_f,
                             uint32_t *counts_f, float *err_b, uint8_t *mask_b,
                             uint32_t *counts_b, void *workspace, size_t workspace_bytes,
                             void *stream);
/* Host-buffer, blocking form (same conventions as hsflow_flow_warped).  u, v:
 * the forward flow; ub, vb: the backward flow (same dtype_out and out_step);
 * mask_f, mask_b: rows x cols u8 with row step mask_step bytes; counts: host
 * uint32[6], forward classes then backward.  ub, vb, the masks and counts may
 * each be NULL. */
int hsflow_flow_bidir(hsflow_ctx *ctx, const void *I0, const void *I1, int dtype_in, int rows,
                      int cols, size_t in_step0, size_t in_step1, int levels, int warps,
                      int window, int iters, double alpha, float rel, float abs_thr, void *u,
                      void *v, void *ub, void *vb, int dtype_out, size_t out_step,
                      uint8_t *mask_f, uint8_t *mask_b, size_t mask_step, uint32_t *counts);

/* ---- median filtering of the flow between warps --------------------------
 * The quadratic smoothness term has to run at alpha ~ 400 to keep the warped
 * solve stable, and at that alpha a moving object's flow is smeared across
 * its boundary; at a lower alpha the solve develops isolated spikes.  A median
 * filter of u and of v after every warp's iterations removes the spikes
 * without moving edges (Wedel et al. 2008; Sun, Roth and Black, CVPR 2010) and
 * makes alpha ~ 100 usable.  ksize = 3 or 5, each component on its own:
 *   out(y, x) = the element of rank (ksize^2 - 1) / 2 of the ksize^2 taps
 *               in[clamp(y + j, 0, rows - 1)][clamp(x + i, 0, cols - 1)],
 *               |i|, |j| <= ksize / 2
 * (border replicated, as the warp's and the check's taps; no tap leaves the
 * pair's plane).  The order is the IEEE-754 total order of the f32 bit
 * patterns:
 *   key = bits ^ 0xFFFFFFFF if the sign bit is set, else bits | 0x80000000,
 * compared as unsigned: -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN.  The
 * result is one of the taps bit for bit and the choice is fixed whatever the
 * planes hold (a NaN is an extreme value, not a poison: a lone one vanishes).
 * The *_median solves are the warped and bidirectional solves above with `int
 * median` after `warps`: 0, 3 or 5.  For median != 0 the schedule per level
 * becomes `warps` times { gradients around (u, v); `iters` Jacobi iterations;
 * median x median filter of the level's (u, v) } -- every level and every
 * warp, the last warp of level 0 included, so the returned flow is filtered.
 * median = 0 runs the launches of the solves above and returns their bits
 * (those entry points are the median = 0 case of these).  hsflow_flow_bidir_median
 * filters both directions, then runs the check unchanged.
 * Workspace: the filter writes the Jacobi workspace's second (u, v) planes,
 * idle between solves, and copies them back, so the *_median solves need
 * nothing beyond hsflow_pyramid_workspace_bytes /
 * hsflow_flow_bidir_workspace_bytes and there is no size function of their
 * own. */
#define HSFLOW_HAS_MEDIAN 1

/* The filter alone: dense f32 [batch][rows][cols] planes u, v -> u_out, v_out.
 * No output plane range may overlap an input plane range or the other output
 * (HSFLOW_ERR_ARG).  Stream-ordered, no workspace, never allocates or
 * synchronises, capturable; all arguments are checked before any device work. */
int hsflow_flow_median_device(const float *u, const float *v, int rows, int cols, int batch,
                              int ksize, float *u_out, float *v_out, void *stream);
int hsflow_flow_warped_median_device(const void *I0, const void *I1, int dtype_in, int rows,
                                     int cols, int batch, int levels, int warps, int median,
                                     int window, int iters, float alpha, float *u, float *v,
                                     void *workspace, size_t workspace_bytes, void *stream);
int hsflow_flow_warped_median(hsflow_ctx *ctx, const void *I0, const void *I1, int dtype_in,
                              int rows, int cols, size_t in_step0, size_t in_step1, int levels,
                              int warps, int median, int window, int iters, double alpha,
                              void *u, void *v, int dtype_out, size_t out_step);
int hsflow_flow_bidir_median_device(const void *I0, const void *I1, int dtype_in, int rows,
                                    int cols, int batch, int levels, int warps, int median,
                                    int window, int iters, float alpha, float rel, float abs_thr,
                                    float *uf, float *vf, float *ub, float *vb, float *err_f,
                                    uint8_t *mask_f, uint32_t *counts_f, float *err_b,
                                    uint8_t *mask_b, uint32_t *counts_b, void *workspace,
                                    size_t workspace_bytes, void *stream);
int hsflow_flow_bidir_median(hsflow_ctx *ctx, const void *I0, const void *I1, int dtype_in,
                             int rows, int cols, size_t in_step0, size_t in_step1, int levels,
                             int warps, int median, int window, int iters, double alpha,
                             float rel, float abs_thr, void *u, void *v, void *ub, void *vb,
                             int dtype_out, size_t out_step, uint8_t *mask_f, uint8_t *mask_b,
                             size_t mask_step, uint32_t *counts);

/* ---- frame warp and motion-compensated frame interpolation --------------
 * What the bidirectional solve is for: the frame at a time t between I0
 * (t = 0) and I1 (t = 1).  Flows are f32 planes in solver units (8 px per
 * unit); (uf, vf) is the flow I0 -> I1, (ub, vb) the flow I1 -> I0, all four
 * read at the output pixel (y, x) (Jiang et al., CVPR 2018, eq. 4):
 *   s = 1 - t;  a = s t;  b = t t;  c = s s                        (f32)
 *   u0 = b ub - a uf;  v0 = b vb - a vf     flow from time t back to frame 0
 *   u1 = c uf - a ub;  v1 = c vf - a vb     flow from time t on to frame 1
 *   s0 = I0 at (y + 8 v0, x + 8 u0);  s1 = I1 at (y + 8 v1, x + 8 u1)
 *   in0, in1 = the targets lie within half a pixel of the frame (the check's
 *        rim test, negated comparisons: NaN -> out)
 *   wt  = t where in0 == in1;  0 where only in0;  1 where only in1
 *   out = (1 - wt) s0 + wt s1     (the bits of s0 where wt = 0, of s1 where 1)
 *   flags = !in0 * HSFLOW_INTERP_I0_OUT | !in1 * HSFLOW_INTERP_I1_OUT |
 *           (mask_f[n0] != 0) * HSFLOW_INTERP_FWD_FAILED |
 *           (mask_b[n1] != 0) * HSFLOW_INTERP_BWD_FAILED
 * The sampler is hsflow_warp_gradients_device's: each displacement clamped as
 * a float to [-cols, cols] / [-rows, rows] (NaN -> lower bound), floor split,
 * the four taps clamped to the pair's plane, top and bottom rows first, then
 * vertical; f64 frames are sampled in f64 and rounded once.  n0, n1 are the
 * source pixels nearest to the two targets (integer part, plus one where the
 * fraction >= 0.5, clamped to the plane); mask_f, mask_b are the u8 planes of
 * hsflow_flow_consistency_device (forward: uf, vf against ub, vb).  A pure
 * translation uf = d, ub = -d gives u0 = -t d and u1 = (1 - t) d; t = 0
 * returns I0 and t = 1 returns I1 bit for bit (f32 frames, finite flows).  The
 * masks are not blending weights -- that made the border strip and the
 * occlusion ring worse -- but flags == 0 marks the pixels whose
 * two sources both pass the check, which carry a far lower error than the
 * rest.  No index leaves a pair's plane, whatever the flows hold. */
#define HSFLOW_HAS_INTERP 1
#define HSFLOW_MAX_TIMES 16
#define HSFLOW_INTERP_I0_OUT 1     /* the target in I0 leaves the frame         */
#define HSFLOW_INTERP_I1_OUT 2     /* the target in I1 leaves the frame         */
#define HSFLOW_INTERP_FWD_FAILED 4 /* the I0 source fails the forward check     */
#define HSFLOW_INTERP_BWD_FAILED 8 /* the I1 source fails the backward check    */

/* Backward warp of a frame by a flow: out(y, x) = I at (y + 8 v, x + 8 u), the
 * I1w of hsflow_warp_gradients_device bit for bit.  I: dense [batch][rows][cols]
 * of dtype_in (U8, F16, F32, F64); u, v, out: f32; oof (u8, may be NULL): 1
 * where the target leaves the frame by more than half a pixel, else 0.  The
 * outputs must not overlap the inputs or each other.  Stream-ordered, no
 * workspace, never allocates or synchronises, capturable. */
int hsflow_warp_image_device(const void *I, int dtype_in, int rows, int cols, int batch,
                             const float *u, const float *v, float *out, uint8_t *oof,
                             void *stream);

/* The frames at `nt` (1..HSFLOW_MAX_TIMES) times, each in [0, 1], in one
 * launch.  `times` is a host array read at call time (the values travel in the
 * kernel arguments).  mask_f, mask_b may each be NULL: its flag bit is then
 * never set.  out: [batch][nt][rows][cols] of dtype_out, HSFLOW_F32 or
 * HSFLOW_U8 (floorf(out + 0.5f) clamped to 0..255, NaN -> 0); flags (may be
 * NULL): u8 [batch][nt][rows][cols]; trusted (may be NULL): uint32[batch][nt],
 * the number of pixels with flags == 0 (zeroed stream-ordered by the call,
 * integer sums).  The outputs must not overlap the inputs or each other.
 * Stream-ordered, no workspace, never allocates or synchronises, capturable;
 * all arguments are checked before any device work. */
int hsflow_frame_interp_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                               int batch, const float *uf, const float *vf, const float *ub,
                               const float *vb, const uint8_t *mask_f, const uint8_t *mask_b,
                               const float *times, int nt, void *out, int dtype_out,
                               uint8_t *flags, uint32_t *trusted, void *stream);

/* Solve and interpolate in one call: hsflow_flow_bidir_median_device into
 * planes of the workspace (both masks only when flags or trusted is asked
 * for), then hsflow_frame_interp_device -- bit for bit what the two calls give
 * one after the other.  `workspace`: at least
 * hsflow_flow_interp_workspace_bytes(rows, cols, batch, levels) bytes (the
 * bidirectional solve's, four f32 flow planes and two u8 mask planes),
 * 256-byte aligned. */
size_t hsflow_flow_interp_workspace_bytes(int rows, int cols, int batch, int levels);
int hsflow_flow_interp_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                              int batch, int levels, int warps, int median, int window,
                              int iters, float alpha, float rel, float abs_thr,
                              const float *times, int nt, void *out, int dtype_out,
                              uint8_t *flags, uint32_t *trusted, void *workspace,
                              size_t workspace_bytes, void *stream);
/* Host-buffer, blocking form (same conventions as hsflow_flow_bidir_median).
 * out: `nt` host planes rows x cols of dtype_out (HSFLOW_U8, HSFLOW_F32, or
 * HSFLOW_F64: the f32 result widened), row step out_step bytes; flags (may be
 * NULL): `nt` u8 planes, row step flags_step; trusted (may be NULL): host
 * uint32[nt]. */
int hsflow_flow_interp(hsflow_ctx *ctx, const void *I0, const void *I1, int dtype_in, int rows,
                       int cols, size_t in_step0, size_t in_step1, int levels, int warps,
                       int median, int window, int iters, double alpha, float rel, float abs_thr,
                       const float *times, int nt, void *const *out, int dtype_out,
                       size_t out_step, uint8_t *const *flags, size_t flags_step,
                       uint32_t *trusted);

/* ---- frame warp and frame interpolation of colour frames -----------------
 * The pipeline's input is colour (main.cpp decodes 8-bit BGR), the flow a
 * grey-level quantity: only the sampling has to know about channels.  Frames
 * are dense 8-bit interleaved BGR, [batch][rows][cols][3], what
 * hsflow_bgr_to_gray_device reads.  Per output pixel the flows, the two
 * targets, their taps and fractions, in0, in1, n0, n1, wt and flags are those
 * of hsflow_frame_interp_device, computed once; its three lerps and its blend
 * then run on each channel, so channel c of the result equals, bit for bit,
 * hsflow_frame_interp_device on the u8 plane bgr[..][c] with the same flows,
 * masks and times.  flags and trusted are per pixel, not per channel.  No
 * index leaves a pair's plane, whatever the flows hold. */
#define HSFLOW_HAS_INTERP_BGR 1

/* hsflow_warp_image_device for BGR frames: out(y, x, c) = bgr(.., c) at
 * (y + 8 v, x + 8 u).  out: [batch][rows][cols][3] of dtype_out, HSFLOW_F32 or
 * HSFLOW_U8 (floorf(out + 0.5f) clamped to 0..255); oof (u8, may be NULL):
 * [batch][rows][cols].  The outputs must not overlap the inputs or each other.
 * Stream-ordered, no workspace, never allocates or synchronises, capturable. */
int hsflow_warp_image_bgr_device(const uint8_t *bgr, int rows, int cols, int batch, const float *u,
                                 const float *v, void *out, int dtype_out, uint8_t *oof,
                                 void *stream);

/* hsflow_frame_interp_device for BGR frames, same conventions (NULL masks,
 * flags and trusted allowed; trusted zeroed stream-ordered by the call; the
 * outputs disjoint from the inputs and from each other; all arguments checked
 * before any device work).  out: [batch][nt][rows][cols][3] of dtype_out,
 * HSFLOW_F32 or HSFLOW_U8; flags: u8 [batch][nt][rows][cols]; trusted:
 * uint32[batch][nt].  Stream-ordered, no workspace, never allocates or
 * synchronises, capturable. */
int hsflow_frame_interp_bgr_device(const uint8_t *bgr0, const uint8_t *bgr1, int rows, int cols,
                                   int batch, const float *uf, const float *vf, const float *ub,
                                   const float *vb, const uint8_t *mask_f, const uint8_t *mask_b,
                                   const float *times, int nt, void *out, int dtype_out,
                                   uint8_t *flags, uint32_t *trusted, void *stream);

/* Convert, solve and interpolate in one call: hsflow_bgr_to_gray_device of
 * both frames into the workspace, hsflow_flow_bidir_median_device on the grey
 * u8 planes (both masks only when flags or trusted is asked for), then
 * hsflow_frame_interp_bgr_device on the BGR frames -- bit for bit what the
 * three calls give one after the other.  `workspace`: at least
 * hsflow_flow_interp_bgr_workspace_bytes(rows, cols, batch, levels) bytes
 * (hsflow_flow_interp_workspace_bytes plus two grey u8 planes), 256-byte
 * aligned; it must not overlap the frames. */
size_t hsflow_flow_interp_bgr_workspace_bytes(int rows, int cols, int batch, int levels);
int hsflow_flow_interp_bgr_device(const uint8_t *bgr0, const uint8_t *bgr1, int rows, int cols,
                                  int batch, int levels, int warps, int median, int window,
                                  int iters, float alpha, float rel, float abs_thr,
                                  const float *times, int nt, void *out, int dtype_out,
                                  uint8_t *flags, uint32_t *trusted, void *workspace,
                                  size_t workspace_bytes, void *stream);
/* Host-buffer, blocking form: two decoded 8-bit BGR frames (row steps
 * bgr_step0, bgr_step1 bytes) go up as 3 B/px, as hsflow_flow_bgr sends them.
 * out: `nt` host planes of rows x cols BGR pixels of dtype_out (HSFLOW_U8 or
 * HSFLOW_F32), row step out_step >= 3 * cols * element size bytes; flags and
 * trusted as in hsflow_flow_interp. */
int hsflow_flow_interp_bgr(hsflow_ctx *ctx, const uint8_t *bgr0, const uint8_t *bgr1, int rows,
                           int cols, size_t bgr_step0, size_t bgr_step1, int levels, int warps,
                           int median, int window, int iters, double alpha, float rel,
                           float abs_thr, const float *times, int nt, void *const *out,
                           int dtype_out, size_t out_step, uint8_t *const *flags,
                           size_t flags_step, uint32_t *trusted);

/* How the BGR kernels fetch the two horizontally adjacent taps of a row (six
 * consecutive bytes unless the pair is clamped at a frame edge): wide = 0
 * (default, the faster one measured) as six single bytes, wide != 0 as one
 * unaligned dword and one halfword.  Both give identical bits (DESIGN.md has
 * the timings).  Process-wide; returns the previous setting. */
int hsflow_set_interp_bgr_loads(int wide);

/* ---- brightness-robust prefilter (local contrast normalisation) -----------
 * Every solve rests on brightness constancy, I1(x + d) = I0(x); an exposure or
 * gain step, a fade or flicker breaks it, and the solver turns the change
 * into motion (a ten-grey-level offset costs two orders of magnitude of
 * accuracy).  The remedy is to solve on the locally normalised
 * texture of the frames.  Per plane, in exact arithmetic:
 *   G   = separable Gaussian of radius r = ceil(3 sigma), weights
 *         w[i] = exp(-i^2 / (2 sigma^2)), |i| <= r, normalised to sum 1 in
 *         double on the host and rounded to f32 once; border reflect-101
 *         folded with period 2 (n - 1) (n = 1: index 0), so any r works on
 *         any size
 *   v   = I - G*I
 *   mode HSFLOW_PREFILTER_HIGHPASS:   out = v           (removes an offset)
 *   mode HSFLOW_PREFILTER_NORMALIZE:  out = scale v / (sqrt(G*(v v)) + eps)
 *                                     (removes an offset and, up to the eps
 *                                     term, a gain)
 * G*(v v), not G*(I I) - (G*I)^2: it has no cancellation in f32.  sigma lies in
 * [0.5, 5] (r <= HSFLOW_PREFILTER_MAX_RADIUS); eps and scale are finite and
 * > 0; anything else is HSFLOW_ERR_ARG before any device work.  U8, F16 and F32
 * frames are computed in f32, F64 frames accumulated in f64 and rounded once.
 * The filter lowers the contrast of what the solver sees, so alpha has to go
 * down with it: recommended is alpha ~ 100 with the 5x5 median, sigma 4,
 * eps 1..4, scale 32; at alpha 400 without the median it does not help, and
 * at sigma 2 it hurts.
 * hsflow_flow, hsflow_flow_bgr, hsflow_flow_pyramid, hsflow_flow_multi and
 * hsflow_gradients are the reference's semantics and never prefilter,
 * whatever the context's setting. */
#define HSFLOW_HAS_PREFILTER 1
#define HSFLOW_PREFILTER_NONE 0
#define HSFLOW_PREFILTER_HIGHPASS 1
#define HSFLOW_PREFILTER_NORMALIZE 2
#define HSFLOW_PREFILTER_MAX_RADIUS 15

typedef struct hsflow_prefilter {
    int mode; /* 0 = none */
    float sigma, eps, scale;
} hsflow_prefilter;

/* The filter alone: I dense [batch][rows][cols] of dtype_in (U8, F16, F32,
 * F64) -> out, f32 of the same shape; one launch, no workspace.  out must not
 * overlap I (HSFLOW_ERR_ARG); pf->mode == 0 is an error for this call.
 * Stream-ordered, never allocates or synchronises, capturable (the weights
 * travel in the kernel arguments); all arguments are checked before any
 * device work. */
int hsflow_prefilter_device(const void *I, int dtype_in, int rows, int cols, int batch,
                            const hsflow_prefilter *pf, float *out, void *stream);
/* Bytes of the two f32 planes per pair a *_pf solve prefilters the frames
 * into (each 256-byte aligned); 0 for a bad size. */
size_t hsflow_prefilter_planes_bytes(int rows, int cols, int batch);

/* The *_median device solves and the two fused interpolations with `const
 * hsflow_prefilter *pf` in front of `workspace`.  They prefilter I0 and I1 into
 * two f32 planes that lie behind the workspace of the call they extend, so
 * `workspace` must hold that call's own size function
 * (hsflow_pyramid_workspace_bytes, hsflow_flow_bidir_workspace_bytes,
 * hsflow_flow_interp_workspace_bytes, hsflow_flow_interp_bgr_workspace_bytes)
 * plus hsflow_prefilter_planes_bytes, and must not overlap the frames; then
 * they run that call on the planes as HSFLOW_F32 frames (not integer-valued,
 * so the pyramid does not round them).  The two interpolations solve on the
 * prefiltered planes and sample the original frames; the BGR one prefilters
 * the grey u8 planes it makes anyway.  The result is bit for bit what the
 * public pieces give one after the other.  pf == NULL or pf->mode == 0 runs
 * the launches of the call without it and returns its bits. */
int hsflow_flow_warped_pf_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                                 int batch, int levels, int warps, int median, int window,
                                 int iters, float alpha, float *u, float *v,
                                 const hsflow_prefilter *pf, void *workspace,
                                 size_t workspace_bytes, void *stream);
int hsflow_flow_bidir_pf_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                                int batch, int levels, int warps, int median, int window,
                                int iters, float alpha, float rel, float abs_thr, float *uf,
                                float *vf, float *ub, float *vb, float *err_f, uint8_t *mask_f,
                                uint32_t *counts_f, float *err_b, uint8_t *mask_b,
                                uint32_t *counts_b, const hsflow_prefilter *pf, void *workspace,
                                size_t workspace_bytes, void *stream);
int hsflow_flow_interp_pf_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                                 int batch, int levels, int warps, int median, int window,
                                 int iters, float alpha, float rel, float abs_thr,
                                 const float *times, int nt, void *out, int dtype_out,
                                 uint8_t *flags, uint32_t *trusted, const hsflow_prefilter *pf,
                                 void *workspace, size_t workspace_bytes, void *stream);
int hsflow_flow_interp_bgr_pf_device(const uint8_t *bgr0, const uint8_t *bgr1, int rows, int cols,
                                     int batch, int levels, int warps, int median, int window,
                                     int iters, float alpha, float rel, float abs_thr,
                                     const float *times, int nt, void *out, int dtype_out,
                                     uint8_t *flags, uint32_t *trusted, const hsflow_prefilter *pf,
                                     void *workspace, size_t workspace_bytes, void *stream);

/* The context's prefilter: the host-buffer, blocking calls hsflow_flow_warped*,
 * hsflow_flow_bidir*, hsflow_flow_interp and hsflow_flow_interp_bgr honour it
 * and then equal their *_pf_device form bit for bit (there are no host _pf
 * variants).  NULL or mode 0: off, the default, which leaves every call as it
 * was.  A bad setting is HSFLOW_ERR_ARG and leaves the old one in place.
 * hsflow_ctx_prefilter reads the setting back. */
int hsflow_ctx_set_prefilter(hsflow_ctx *ctx, const hsflow_prefilter *pf);
int hsflow_ctx_prefilter(const hsflow_ctx *ctx, hsflow_prefilter *pf);

/* ---- flow-driven (edge-preserving) smoothness of the warped solves ---------
 * The smoothness term of every solve above is quadratic: each iteration
 * replaces (u, v) by its plain window mean, which averages across a motion
 * boundary, so the flow crosses an object's edge as a ramp about ten pixels
 * wide -- at pixels that are visible in both frames and that neither the median
 * nor the forward-backward check repairs.  The flow-driven term
 * weights each tap by a diffusivity g that is small where the flow around which
 * the warp linearises already has a large gradient (lagged diffusivity).  Per
 * level and per warp, from that warp's (u0, v0), U = 8 u0, V = 8 v0 in px:
 *   Ux = 0.5 (U[y][min(x+1, cols-1)] - U[y][max(x-1, 0)]),  Uy, Vx, Vy likewise
 *        (border replicated)
 *   s  = Ux^2 + Uy^2 + Vx^2 + Vy^2
 *   g  = 1 / sqrt(1 + s / lambda^2)                              in (0, 1]
 * `lambda` is the flow gradient, px per px, at which the weight drops to
 * 1/sqrt(2): finite and > 0, recommended 0.1 .. 0.3.  The iteration is the
 * getFlow loop with the two means replaced.  S = the window sum over the taps
 * inside the plane, m = the number of the window's taps outside it; those
 * count as u = 0 with weight 1, the reference's zero border:
 *   ubar = S(g u) / (S(g) + m);  vbar = S(g v) / (S(g) + m)
 *   c = (Ix ubar + Iy vbar + It') / (alpha^2 + Ix^2 + Iy^2)
 *   u = ubar - Ix c;  v = vbar - Iy c
 * g = 1 everywhere gives the plain iteration's values (within rounding, not
 * the same bits).  With the mode on `window` must be 3 or 5 (odd windows,
 * centred anchor); any other is HSFLOW_ERR_ARG before any device work.
 * Schedule per level, `warps` times: gradients around (u, v); g from (u, v);
 * `iters` weighted iterations warm-started from (u, v), g fixed; the median
 * if asked for.  At the first warp of the coarsest level the flow is zero and
 * g = 1: with levels = 1, warps = 1 the mode changes nothing but rounding.
 * Recommended: lambda 0.3 with alpha ~ 100, the 5x5 median and 4 warps.  A
 * true occlusion (ground one frame does not show) is not repaired by it.
 * hsflow_flow, hsflow_flow_bgr, hsflow_flow_pyramid, hsflow_flow_multi keep
 * the reference's semantics whatever the context's setting. */
#define HSFLOW_HAS_SMOOTHNESS 1
#define HSFLOW_SMOOTH_QUADRATIC 0   /* default: the solves above              */
#define HSFLOW_SMOOTH_FLOW_DRIVEN 1

typedef struct hsflow_smoothness {
    int mode; /* 0 = quadratic */
    float lambda;
} hsflow_smoothness;

/* The weights alone: (u, v) dense f32 [batch][rows][cols] in solver units ->
 * g, f32 of the same shape; one launch, no workspace.  g must not overlap u
 * or v.  Stream-ordered, never allocates or synchronises, capturable; all
 * arguments are checked before any device work. */
int hsflow_flow_diffusivity_device(const float *u, const float *v, int rows, int cols, int batch,
                                   float lambda, float *g, void *stream);
/* `iters` weighted iterations warm-started from (u, v), window 3 or 5.  The
 * gradients are the f32 planes of `workspace` (hsflow_workspace_bytes), the
 * state hsflow_warp_gradients_device leaves.  g, u and v must not overlap the
 * workspace or each other.  The result has the same bits however `iters` is
 * split into calls and whatever hsflow_set_iters_per_launch says.  A batch is
 * split over side streams as hsflow_jacobi_device's is (same bits). */
int hsflow_jacobi_weighted_device(int rows, int cols, int batch, int window, int iters,
                                  float alpha, const float *g, float *u, float *v,
                                  void *workspace, size_t workspace_bytes, void *stream);

/* The four *_pf_device solves with `const hsflow_smoothness *sm` after `pf`.
 * sm == NULL or sm->mode == 0 launches exactly what the *_pf_device call
 * launches and returns its bits (those calls are the sm = NULL case of
 * these).  The weights live in a plane of the solve's workspace that a warped
 * solve does not otherwise use, so the workspace sizes are the *_pf_device
 * calls'.  The result is bit for bit what the public pieces give one after
 * the other (pyramid, upflow, warp gradients, diffusivity, weighted
 * iterations, median). */
int hsflow_flow_warped_sm_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                                 int batch, int levels, int warps, int median, int window,
                                 int iters, float alpha, float *u, float *v,
                                 const hsflow_prefilter *pf, const hsflow_smoothness *sm,
                                 void *workspace, size_t workspace_bytes, void *stream);
int hsflow_flow_bidir_sm_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                                int batch, int levels, int warps, int median, int window,
                                int iters, float alpha, float rel, float abs_thr, float *uf,
                                float *vf, float *ub, float *vb, float *err_f, uint8_t *mask_f,
                                uint32_t *counts_f, float *err_b, uint8_t *mask_b,
                                uint32_t *counts_b, const hsflow_prefilter *pf,
                                const hsflow_smoothness *sm, void *workspace,
                                size_t workspace_bytes, void *stream);
int hsflow_flow_interp_sm_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                                 int batch, int levels, int warps, int median, int window,
                                 int iters, float alpha, float rel, float abs_thr,
                                 const float *times, int nt, void *out, int dtype_out,
                                 uint8_t *flags, uint32_t *trusted, const hsflow_prefilter *pf,
                                 const hsflow_smoothness *sm, void *workspace,
                                 size_t workspace_bytes, void *stream);
int hsflow_flow_interp_bgr_sm_device(const uint8_t *bgr0, const uint8_t *bgr1, int rows, int cols,
                                     int batch, int levels, int warps, int median, int window,
                                     int iters, float alpha, float rel, float abs_thr,
                                     const float *times, int nt, void *out, int dtype_out,
                                     uint8_t *flags, uint32_t *trusted, const hsflow_prefilter *pf,
                                     const hsflow_smoothness *sm, void *workspace,
                                     size_t workspace_bytes, void *stream);

/* The context's smoothness term: the host-buffer, blocking calls
 * hsflow_flow_warped*, hsflow_flow_bidir*, hsflow_flow_interp and
 * hsflow_flow_interp_bgr honour it and then equal their *_sm_device form bit
 * for bit.  NULL or mode 0: quadratic, the default.  A bad setting is
 * HSFLOW_ERR_ARG and leaves the old one in place (the window is checked by the
 * call that solves).  hsflow_ctx_smoothness reads the setting back. */
int hsflow_ctx_set_smoothness(hsflow_ctx *ctx, const hsflow_smoothness *sm);
int hsflow_ctx_smoothness(const hsflow_ctx *ctx, hsflow_smoothness *sm);

/* ---- temporal warm start: an initial flow, and sequence mode ----------------
 * In video the motion of pair k+1 is almost the motion of pair k.  The backward
 * flow of pair k, (ub, vb) for I1 -> I0, lives on I1's grid, and I1 is the
 * first frame of pair k+1: under constant velocity the forward flow of pair
 * k+1 is -(ub, vb) with no splatting, and its backward flow is (ub, vb) read
 * where that motion lands.  The warped solves take such a flow as their start
 * instead of zero.
 *
 * What it buys ("Temporal warm start"): for steady motion one level
 * and one warp from the predicted flow match the cold 3-level, 4-warp solve;
 * with the pyramid kept, a warm solve beats the cold solve of the same
 * schedule.  A warm start WITHOUT the pyramid (levels = 1) cannot repair a
 * prediction that is off by more than about a pixel.  So: keep `levels` and
 * halve `warps` when motion may change; use levels = 1 only for steady motion.
 * A scene cut makes the prediction worthless: with the fallback on
 * (hsflow_ctx_set_fallback) the interpolating calls find the cut themselves
 * and drop the prediction; the other calls' caller resets it. */
#define HSFLOW_HAS_TEMPORAL 1

/* The start of a solve: dense f32 planes [batch][rows][cols], solver units,
 * full resolution.  (uf, vf) starts the forward solve, (ub, vb) the backward
 * solve of the bidirectional calls.  A pair that is NULL starts cold; one
 * plane of a pair without the other is HSFLOW_ERR_ARG. */
typedef struct hsflow_flow_init {
    const float *uf, *vf, *ub, *vb;
} hsflow_flow_init;

/* hsflow_upflow_device's counterpart: (u, v) of a level, dense f32
 * [batch][rows][cols], one level down into (uc, vc), [batch][rc][cc] with rc,
 * cc the next level's size (hsflow_pyramid_level_size: ceil(n / 2); anything
 * else is HSFLOW_ERR_ARG).  Per component, in f32, in this order:
 *   a = u[2y][2x];               b = u[2y][min(2x+1, cols-1)]
 *   c = u[min(2y+1, rows-1)][2x]; d = u[min(2y+1, rows-1)][min(2x+1, cols-1)]
 *   uc[y][x] = ((a + b) + (c + d)) * 0.125f
 * the mean of the four, halved (px of the coarser level).  NaN and inf pass
 * through arithmetically.  The outputs must not overlap the inputs or each
 * other.  One launch, no workspace, stream-ordered, capturable. */
int hsflow_downflow_device(const float *u, const float *v, int rows, int cols, float *uc,
                           float *vc, int rc, int cc, int batch, void *stream);

/* Pair k's backward flow (ub, vb) into the start of pair k+1:
 *   uf_next = -ub;  vf_next = -vb                        (the sign bit flipped)
 *   ub_next = ub sampled at (y + 8 vb, x + 8 ub);  vb_next = vb at that point
 * with hsflow_warp_image_device's sampler, so ub_next equals
 * hsflow_warp_image_device(ub as an F32 frame, u = ub, v = vb) bit for bit,
 * vb_next likewise.  Each output pair may be NULL (both planes), not both
 * pairs.  The outputs must not overlap the inputs or each other.  One launch,
 * no workspace, never allocates or synchronises, capturable. */
int hsflow_flow_predict_device(const float *ub, const float *vb, int rows, int cols, int batch,
                               float *uf_next, float *vf_next, float *ub_next, float *vb_next,
                               void *stream);

/* The four *_sm_device solves with `const hsflow_flow_init *init` after `sm`.
 * init == NULL, or all four planes NULL, launches exactly what the *_sm_device
 * call launches and returns its bits (those calls are the init = NULL case of
 * these).  The forward solve starts from (uf, vf), the backward solve from
 * (ub, vb); the warped call reads only uf and vf.  With levels = 1 the flow
 * starts as a copy of the init.  With levels > 1 the init is reduced level by
 * level (hsflow_downflow_device) into the workspace's per-level flow planes,
 * which the projection up overwrites later, and the coarsest level starts from
 * the last reduction: the workspace sizes are the *_sm_device calls'.
 * Everything after the start is the solve unchanged; with a smoothness mode on
 * the first warp's weights come from the init.  The init planes must not
 * overlap the outputs or the workspace.  All arguments are checked before any
 * device work.  The result is bit for bit what the public pieces give one
 * after the other (pyramid, downflow, upflow, warp gradients, diffusivity,
 * iterations, median). */
int hsflow_flow_warped_init_device(const void *I0, const void *I1, int dtype_in, int rows,
                                   int cols, int batch, int levels, int warps, int median,
                                   int window, int iters, float alpha, float *u, float *v,
                                   const hsflow_prefilter *pf, const hsflow_smoothness *sm,
                                   const hsflow_flow_init *init, void *workspace,
                                   size_t workspace_bytes, void *stream);
int hsflow_flow_bidir_init_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                                  int batch, int levels, int warps, int median, int window,
                                  int iters, float alpha, float rel, float abs_thr, float *uf,
                                  float *vf, float *ub, float *vb, float *err_f, uint8_t *mask_f,
                                  uint32_t *counts_f, float *err_b, uint8_t *mask_b,
                                  uint32_t *counts_b, const hsflow_prefilter *pf,
                                  const hsflow_smoothness *sm, const hsflow_flow_init *init,
                                  void *workspace, size_t workspace_bytes, void *stream);
int hsflow_flow_interp_init_device(const void *I0, const void *I1, int dtype_in, int rows,
                                   int cols, int batch, int levels, int warps, int median,
                                   int window, int iters, float alpha, float rel, float abs_thr,
                                   const float *times, int nt, void *out, int dtype_out,
                                   uint8_t *flags, uint32_t *trusted, const hsflow_prefilter *pf,
                                   const hsflow_smoothness *sm, const hsflow_flow_init *init,
                                   void *workspace, size_t workspace_bytes, void *stream);
int hsflow_flow_interp_bgr_init_device(const uint8_t *bgr0, const uint8_t *bgr1, int rows,
                                       int cols, int batch, int levels, int warps, int median,
                                       int window, int iters, float alpha, float rel,
                                       float abs_thr, const float *times, int nt, void *out,
                                       int dtype_out, uint8_t *flags, uint32_t *trusted,
                                       const hsflow_prefilter *pf, const hsflow_smoothness *sm,
                                       const hsflow_flow_init *init, void *workspace,
                                       size_t workspace_bytes, void *stream);

/* Sequence mode of a context: off by default, and off leaves every call
 * exactly as it is.  On, the bidirectional host-buffer calls (hsflow_flow_bidir,
 * hsflow_flow_bidir_median, hsflow_flow_interp, hsflow_flow_interp_bgr)
 *   1. start from the context's stored prediction, if there is one and its
 *      rows x cols are the call's, and
 *   2. after the solve run hsflow_flow_predict_device on their (ub, vb) into
 *      four planes the context owns (grow-only), on the context's stream ahead
 *      of the download, with no extra synchronisation.
 * The result then equals the *_init_device call started from
 * hsflow_flow_predict_device's output for the previous call, bit for bit; the
 * first call, and a call without a stored prediction, is the cold call.  The
 * stored prediction is dropped by a failed call, a call of another size,
 * hsflow_ctx_temporal_reset and hsflow_ctx_set_temporal.  Feed the calls the
 * consecutive pairs of one clip, in order.  Keep `levels` and halve `warps`
 * when motion may change; use levels = 1 only for steady motion.  At a scene
 * cut hsflow_flow_interp and hsflow_flow_interp_bgr drop the prediction
 * themselves where the context's fallback is on (hsflow_ctx_set_fallback;
 * hsflow_ctx_last_cut tells); otherwise call hsflow_ctx_temporal_reset
 * there.  hsflow_flow_warped* has no
 * backward flow and ignores the mode, as do hsflow_flow, hsflow_flow_bgr,
 * hsflow_flow_pyramid and hsflow_flow_multi.  hsflow_ctx_temporal returns the
 * mode (0 or 1; HSFLOW_ERR_ARG for a null context). */
int hsflow_ctx_set_temporal(hsflow_ctx *ctx, int on);
int hsflow_ctx_temporal(const hsflow_ctx *ctx);
int hsflow_ctx_temporal_reset(hsflow_ctx *ctx);

/* ---- coarse solve: the flow at a reduced resolution, the frames at full ------
 * Level 0 holds 1 / (1 + 1/4 + 1/16) = 76 % of a 3-level solve's pixel x
 * iterations, and interpolation needs a flow good enough to fetch the right
 * source pixel, not a level-0 solve.  `finest` in 0 .. levels - 1 is the last
 * pyramid level the warped family solves:
 *   - `levels` still counts from the full frame: the pyramid, its rounding and
 *     the per-level schedule (init or zero start, downflow of an init, `warps`
 *     x { warp gradients; diffusivity if asked; iterations; median }) are those
 *     of the call without `finest`; a prefilter runs on the full frames;
 *   - levels levels-1 .. finest are solved, levels finest-1 .. 0 are not;
 *   - the flow of level `finest` reaches the full frame by `finest`
 *     applications of hsflow_upflow_bilinear_device, one per level, through the
 *     pyramid's own level sizes;
 *   - the flows returned are full-resolution planes in solver units, as ever;
 *     the forward-backward check runs on them at full resolution
 *     (hsflow_flow_consistency_device), interpolation samples the
 *     full-resolution frames, sequence mode predicts from the upsampled
 *     (ub, vb), and an init is full resolution and is reduced level by level
 *     all the same;
 *   - finest = 0 launches exactly what the call without it launches and
 *     returns its bits; finest < 0 or finest >= levels is HSFLOW_ERR_ARG before
 *     any device work.
 * What it buys and costs ("Coarse solve"): finest = 1 solves a
 * quarter of the pixels; pure shifts lose nothing visible, a motion boundary
 * becomes one coarse pixel wide. */
#define HSFLOW_HAS_FINEST 1

/* hsflow_upflow_device's bilinear counterpart, for a final flow rather than a
 * warm start: (uc, vc), dense f32 [batch][rc][cc], one level up into (u, v),
 * [batch][rows][cols]; rc, cc must be ceil(rows / 2), ceil(cols / 2) (anything
 * else is HSFLOW_ERR_ARG).  Pixel centres aligned, border replicated; per
 * component, in f32, in this order:
 *   sy = min(max(0.5f*y - 0.25f, 0), rc-1);  y0 = floor(sy);  fy = sy - y0;
 *   y1 = min(y0+1, rc-1);   sx, x0, fx, x1 likewise with cc
 *   top = a[y0][x0] + fx*(a[y0][x1] - a[y0][x0])
 *   bot = a[y1][x0] + fx*(a[y1][x1] - a[y1][x0])
 *   out = 2 * (top + fy*(bot - top))
 * with no multiply fused into an add.  The weights are 0, 0.25 or 0.75, exact
 * in f32.  NaN and inf pass through arithmetically (a tap of weight 0 counts);
 * no index leaves a pair's plane.  Planes need element alignment only.  The
 * outputs must not overlap the inputs or each other.  u and v go in one
 * launch; no workspace, never allocates or synchronises, capturable. */
int hsflow_upflow_bilinear_device(const float *uc, const float *vc, int rc, int cc, float *u,
                                  float *v, int rows, int cols, int batch, void *stream);

/* The four *_init_device solves with `int finest` after `levels` (those calls
 * are the finest = 0 case of these).  The workspaces are the *_init_device
 * calls': the flow of level `finest` and the upsampling steps live in the
 * per-level flow planes the workspace already has, and the outputs are
 * written by the last step alone.  The result is bit for bit what the public
 * pieces give one after the other (pyramid, downflow, upflow, warp gradients,
 * diffusivity, iterations, median, bilinear upflow; then the check and the
 * interpolation at full resolution). */
int hsflow_flow_warped_lv_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                                 int batch, int levels, int finest, int warps, int median,
                                 int window, int iters, float alpha, float *u, float *v,
                                 const hsflow_prefilter *pf, const hsflow_smoothness *sm,
                                 const hsflow_flow_init *init, void *workspace,
                                 size_t workspace_bytes, void *stream);
int hsflow_flow_bidir_lv_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                                int batch, int levels, int finest, int warps, int median,
                                int window, int iters, float alpha, float rel, float abs_thr,
                                float *uf, float *vf, float *ub, float *vb, float *err_f,
                                uint8_t *mask_f, uint32_t *counts_f, float *err_b, uint8_t *mask_b,
                                uint32_t *counts_b, const hsflow_prefilter *pf,
                                const hsflow_smoothness *sm, const hsflow_flow_init *init,
                                void *workspace, size_t workspace_bytes, void *stream);
int hsflow_flow_interp_lv_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                                 int batch, int levels, int finest, int warps, int median,
                                 int window, int iters, float alpha, float rel, float abs_thr,
                                 const float *times, int nt, void *out, int dtype_out,
                                 uint8_t *flags, uint32_t *trusted, const hsflow_prefilter *pf,
                                 const hsflow_smoothness *sm, const hsflow_flow_init *init,
                                 void *workspace, size_t workspace_bytes, void *stream);
int hsflow_flow_interp_bgr_lv_device(const uint8_t *bgr0, const uint8_t *bgr1, int rows, int cols,
                                     int batch, int levels, int finest, int warps, int median,
                                     int window, int iters, float alpha, float rel,
                                     float abs_thr, const float *times, int nt, void *out,
                                     int dtype_out, uint8_t *flags, uint32_t *trusted,
                                     const hsflow_prefilter *pf, const hsflow_smoothness *sm,
                                     const hsflow_flow_init *init, void *workspace,
                                     size_t workspace_bytes, void *stream);

/* The context's finest level: the host-buffer, blocking calls
 * hsflow_flow_warped*, hsflow_flow_bidir*, hsflow_flow_interp and
 * hsflow_flow_interp_bgr honour it and then equal their *_lv_device form bit
 * for bit (sequence mode included).  0, the default: the full frame.  A value
 * outside [0, HSFLOW_MAX_LEVELS - 1] is HSFLOW_ERR_ARG and leaves the old one
 * in place; the call that solves rejects finest >= its levels.  hsflow_flow,
 * hsflow_flow_bgr, hsflow_flow_pyramid, hsflow_flow_multi and hsflow_gradients
 * ignore the setting.  hsflow_ctx_finest_level reads it back (HSFLOW_ERR_ARG
 * for a null context). */
int hsflow_ctx_set_finest_level(hsflow_ctx *ctx, int finest);
int hsflow_ctx_finest_level(const hsflow_ctx *ctx);

/* ---- flow projection: the flows carried to time t before a frame is made -----
 * hsflow_frame_interp_device forms the time-t flow of an output pixel from the
 * four flows at that pixel.  Near a motion boundary the output pixel belongs
 * to whichever surface lands on it at time t, not to the one that sits there
 * in frame 0 or frame 1.  Projection (Baker et al., IJCV 2011, section 3.3.2)
 * carries every source pixel's flow to where that pixel is at time t, keeps
 * per target the candidate whose brightness matches best, and samples both
 * frames with the winner's flow.  Per pair and per time t, f32, s = 1 - t:
 *   candidates   every pixel p = (y, x) of both frames:
 *                  direction 0: frame A = G0, other = G1, (u, v) = (uf, vf), tau = t
 *                  direction 1: frame A = G1, other = G0, (u, v) = (ub, vb), tau = s
 *   displacement dx = 8 u, dy = 8 v, clamped as floats to [-cols, cols] and
 *                [-rows, rows] (NaN -> lower bound), hsflow_warp_image_device's
 *   cost         |w - A(p)|, w = the other frame sampled at (y + dy, x + dx) as
 *                hsflow_warp_image_device samples (f64 frames: in double,
 *                rounded to f32 once);  code = cost * 8 as a float;
 *                !(code < 2^30) -> 2^30 (NaN lands there); truncated to uint32
 *   target       qx = x + (int)floorf(tau dx + 0.5f), qy likewise (no multiply
 *                fused into an add; the displacement is rounded on its own, so
 *                the target is exact at any x, y); a candidate whose qx is
 *                outside [0, cols) or qy outside [0, rows) has none
 *   key          code << 32 | dir << 31 | (y cols + x)
 *   cells[pair][time][qy][qx] = the minimum key over the candidates that land
 *                there: an integer minimum, so the plane is the same bytes
 *                whatever the order of arrival; ties go to direction 0, then
 *                to the lower source index.  A cell nothing lands on stays
 *                all ones: a hole.
 * Resolve and blend at output pixel q (hsflow_frame_interp_proj_device): a hole
 * is hsflow_frame_interp_device's pixel unchanged, with HSFLOW_INTERP_HOLE in
 * its flags; else with (dir, p) decoded from the cell's low word,
 *   (ut, vt) = (uf, vf)[p] for direction 0, (-ub, -vb)[p] for direction 1
 *   u0 = -t ut;  v0 = -t vt;  u1 = s ut;  v1 = s vt
 * and from there hsflow_frame_interp_device's text: the two samples, in0, in1,
 * wt, the blend, the u8 rounding, n0, n1, the four flag bits from mask_f and
 * mask_b, trusted as the count of flags == 0.  t = 0 and t = 1 return I0 and
 * I1 exactly (finite flows).  The masks stay a confidence output.
 * What it buys ("Flow projection"): about a third of the error in
 * the band around a moving object and of the whole frame's; pure shifts are
 * unchanged; the narrow ring of real occlusion stays. */
#define HSFLOW_HAS_PROJECTION 1
#define HSFLOW_INTERP_HOLE 16 /* no candidate landed on the pixel at this time */

/* KS: the cells of `nt` times (host array, read at call time, each in [0, 1],
 * nt in 1 .. HSFLOW_MAX_TIMES) from the grey frames G0, G1 the flows were
 * solved on (dense [batch][rows][cols] of dtype_in: U8, F16, F32 or F64) and
 * the four flows (dense f32).  cells: [batch][nt][rows][cols] of uint64_t,
 * 8-byte aligned (else HSFLOW_ERR_ARG), disjoint from the inputs; the call
 * sets it to all ones stream-ordered, then one launch takes the minima.  NaN,
 * inf and huge flows are safe: no index leaves a pair's plane, and every
 * non-empty cell's low 31 bits are below rows * cols.  rows * cols beyond the
 * library's plane limit of 2^29 - 4 pixels (any product above 2^31 included)
 * is HSFLOW_ERR_ARG.
 * No workspace, never allocates or synchronises, capturable. */
int hsflow_flow_project_device(const void *G0, const void *G1, int dtype_in, int rows, int cols,
                               int batch, const float *uf, const float *vf, const float *ub,
                               const float *vb, const float *times, int nt, uint64_t *cells,
                               void *stream);

/* hsflow_frame_interp_device and hsflow_frame_interp_bgr_device reading the
 * time-t flow through `cells` (of the same times, 8-byte aligned, not
 * overlapping an output).  For colour frames the cells come from the grey
 * conversions (hsflow_bgr_to_gray_device) of both frames; each channel of the
 * result has the bits the grey call gives that channel's plane. */
int hsflow_frame_interp_proj_device(const void *I0, const void *I1, int dtype_in, int rows,
                                    int cols, int batch, const float *uf, const float *vf,
                                    const float *ub, const float *vb, const uint8_t *mask_f,
                                    const uint8_t *mask_b, const uint64_t *cells,
                                    const float *times, int nt, void *out, int dtype_out,
                                    uint8_t *flags, uint32_t *trusted, void *stream);
int hsflow_frame_interp_bgr_proj_device(const uint8_t *bgr0, const uint8_t *bgr1, int rows,
                                        int cols, int batch, const float *uf, const float *vf,
                                        const float *ub, const float *vb, const uint8_t *mask_f,
                                        const uint8_t *mask_b, const uint64_t *cells,
                                        const float *times, int nt, void *out, int dtype_out,
                                        uint8_t *flags, uint32_t *trusted, void *stream);

/* The fused calls: the *_lv_device forms with `int projection` after `nt`.
 * 0 makes exactly the launches of the *_lv_device call (and needs its
 * workspace only); 1 is the public pieces one after the other -- the
 * bidirectional solve, hsflow_flow_project_device on the grey frames the solve
 * ran on (after the conversion and the prefilter, where there is one), the
 * projected interpolation of the frames themselves -- and bit for bit what
 * they give; anything else is HSFLOW_ERR_ARG.  The workspace of projection = 1
 * is the *_lv_device call's plus the 256-byte-aligned cell plane of nt times
 * (and a prefilter's planes behind it, as ever).  All arguments are checked
 * before any device work. */
size_t hsflow_flow_interp_pj_workspace_bytes(int rows, int cols, int batch, int levels, int nt);
size_t hsflow_flow_interp_bgr_pj_workspace_bytes(int rows, int cols, int batch, int levels,
                                                 int nt);
int hsflow_flow_interp_pj_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                                 int batch, int levels, int finest, int warps, int median,
                                 int window, int iters, float alpha, float rel, float abs_thr,
                                 const float *times, int nt, int projection, void *out,
                                 int dtype_out, uint8_t *flags, uint32_t *trusted,
                                 const hsflow_prefilter *pf, const hsflow_smoothness *sm,
                                 const hsflow_flow_init *init, void *workspace,
                                 size_t workspace_bytes, void *stream);
int hsflow_flow_interp_bgr_pj_device(const uint8_t *bgr0, const uint8_t *bgr1, int rows, int cols,
                                     int batch, int levels, int finest, int warps, int median,
                                     int window, int iters, float alpha, float rel,
                                     float abs_thr, const float *times, int nt, int projection,
                                     void *out, int dtype_out, uint8_t *flags, uint32_t *trusted,
                                     const hsflow_prefilter *pf, const hsflow_smoothness *sm,
                                     const hsflow_flow_init *init, void *workspace,
                                     size_t workspace_bytes, void *stream);

/* The context's projection: hsflow_flow_interp and hsflow_flow_interp_bgr
 * honour it and then equal their *_pj_device form bit for bit.  0, the
 * default: as before.  A value other than 0 or 1 is HSFLOW_ERR_ARG and leaves
 * the old one in place.  hsflow_ctx_projection reads it back (HSFLOW_ERR_ARG
 * for a null context). */
int hsflow_ctx_set_projection(hsflow_ctx *ctx, int projection);
int hsflow_ctx_projection(const hsflow_ctx *ctx);

/* ---- fallback for a failed pair: a source frame where the flows are worthless --
 * A scene cut, a fade the prefilter is not set up for, a motion beyond the
 * pyramid's reach: the flows of such a pair mean nothing, and the frames
 * hsflow_frame_interp_device makes from them are morphs of two unrelated
 * pictures.  The forward-backward check tells such a pair from a good one: the
 * share of HSFLOW_CONSISTENT pixels, both directions together, is at least 0.55
 * for related pairs within reach and at most 0.32 for unrelated ones (DESIGN.md,
 * "Fallback for a failed pair").  The fallback takes that verdict per pair on
 * the device, with no host synchronisation, and replaces a failed pair's frames
 * by a source frame or a cross-fade.  A pair that is a cut in half the picture
 * lands at 0.43 - 0.54: no threshold decides that case.
 *
 * Threshold: min_share, finite and in [0, 1] (else HSFLOW_ERR_ARG).
 *   m = hsflow_fallback_min_consistent(rows, cols, min_share): the smallest
 *       integer >= (double)min_share * 2.0 * rows * cols, computed in double; 0
 *       for a bad size.  min_share = 0 gives 0: no pair ever fails.
 * Verdict of pair b, from the uint32[batch][3] counts of
 * hsflow_flow_consistency_device in both directions:
 *   cut[b] = (uint64)counts_f[b][HSFLOW_CONSISTENT]
 *            + counts_b[b][HSFLOW_CONSISTENT] < m
 * an integer comparison, the same at every time.
 * A pair with cut[b] == 1, at every time t of the call, with a, c the pixel of
 * I0 and of I1 as hsflow_frame_interp_device reads them at zero flow (the
 * element converted to f32; an f64 element rounded once):
 *   HSFLOW_FALLBACK_NEAREST  out = t < 0.5f ? a : c
 *   HSFLOW_FALLBACK_BLEND    out = t == 0 ? a : t == 1 ? c : fma(1 - t, a, t c)
 *                            (a select; 1 - t and t c are rounded to f32, the
 *                            multiply-add is fused: the interpolation's own
 *                            blend with wt = t as the library computes it)
 *   u8 output: floorf(x + 0.5f) clamped to 0..255, NaN -> 0, as the interpolation
 *   BGR: the same per channel
 *   flags = HSFLOW_INTERP_FALLBACK at every pixel, replacing what was there (the
 *           flags of a meaningless flow say nothing; flags == 0 stays the mark
 *           of a trusted pixel)
 *   trusted[b][t] = 0
 * A pair with cut[b] == 0: nothing of its out, flags or trusted is written.
 * So for finite frames the BLEND result equals hsflow_frame_interp_device on
 * four all-zero flow planes with NULL masks bit for bit, and the NEAREST result
 * equals that call at t = 0 or t = 1. */
#define HSFLOW_HAS_FALLBACK 1
#define HSFLOW_FALLBACK_OFF 0
#define HSFLOW_FALLBACK_NEAREST 1   /* t < 0.5 -> I0, else I1 */
#define HSFLOW_FALLBACK_BLEND 2     /* (1 - t) I0 + t I1 */
#define HSFLOW_FALLBACK_MIN_SHARE 0.4f
#define HSFLOW_INTERP_FALLBACK 32   /* flags: the pixel is the fallback's */
typedef struct hsflow_fallback { int mode; float min_share; } hsflow_fallback;

/* size_t: 64 bits on every platform the library builds for, so the comparison
 * above is made in 64 bits whatever the counts hold */
size_t hsflow_fallback_min_consistent(int rows, int cols, float min_share);

/* KF: the verdict of every pair and the replacement of the failed ones, over
 * the outputs of hsflow_frame_interp_device (or its _bgr_, _proj_ forms) for the
 * same frames, times and dtype_out: out [batch][nt] planes (U8 or F32;
 * required), flags [batch][nt] planes of u8, trusted uint32[batch][nt], cut
 * uint8[batch]; flags, trusted and cut may each be NULL, and every element of
 * a given cut is written.  counts_f, counts_b: device arrays, required.  fb:
 * required, mode NEAREST or BLEND (NULL or mode 0 is HSFLOW_ERR_ARG here).
 * `times`: host array, read at call time, each in [0, 1], nt in
 * 1 .. HSFLOW_MAX_TIMES.  Planes need element alignment only.  The outputs
 * must be disjoint from the inputs and from each other.  All arguments are
 * checked before any device work.  One launch for all times and pairs; the
 * blocks of a pair that passes read its two counts and leave.  Stream-ordered,
 * no workspace, never allocates or synchronises, capturable. */
int hsflow_frame_fallback_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                                 int batch, const uint32_t *counts_f, const uint32_t *counts_b,
                                 const hsflow_fallback *fb, const float *times, int nt, void *out,
                                 int dtype_out, uint8_t *flags, uint32_t *trusted, uint8_t *cut,
                                 void *stream);
int hsflow_frame_fallback_bgr_device(const uint8_t *bgr0, const uint8_t *bgr1, int rows, int cols,
                                     int batch, const uint32_t *counts_f,
                                     const uint32_t *counts_b, const hsflow_fallback *fb,
                                     const float *times, int nt, void *out, int dtype_out,
                                     uint8_t *flags, uint32_t *trusted, uint8_t *cut,
                                     void *stream);

/* The fused calls: the *_pj_device forms with `const hsflow_fallback *fb` after
 * `init` and `uint8_t *cut` (uint8[batch], may be NULL) after `trusted`; the
 * *_pj_device calls are the fb = NULL case of these.  fb == NULL or mode 0
 * makes exactly the *_pj_device launches and needs that call's workspace only;
 * a given cut is then zeroed stream-ordered.  With the fallback on both
 * consistency checks always launch, their counts go into the workspace (the
 * masks are still written only when flags or trusted is asked for), and
 * hsflow_frame_fallback*_device follows the interpolation on the stream: the
 * result is bit for bit the public pieces one after the other.  The workspace
 * is then the *_pj_device call's for the same projection plus
 * hsflow_fallback_counts_bytes(batch) -- two 256-byte-aligned uint32[batch][3]
 * arrays; 0 for a bad batch -- with a prefilter's planes behind it, as ever.
 * A bad mode or min_share is HSFLOW_ERR_ARG before any device work. */
size_t hsflow_fallback_counts_bytes(int batch);
int hsflow_flow_interp_fb_device(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                                 int batch, int levels, int finest, int warps, int median,
                                 int window, int iters, float alpha, float rel, float abs_thr,
                                 const float *times, int nt, int projection, void *out,
                                 int dtype_out, uint8_t *flags, uint32_t *trusted, uint8_t *cut,
                                 const hsflow_prefilter *pf, const hsflow_smoothness *sm,
                                 const hsflow_flow_init *init, const hsflow_fallback *fb,
                                 void *workspace, size_t workspace_bytes, void *stream);
int hsflow_flow_interp_bgr_fb_device(const uint8_t *bgr0, const uint8_t *bgr1, int rows, int cols,
                                     int batch, int levels, int finest, int warps, int median,
                                     int window, int iters, float alpha, float rel,
                                     float abs_thr, const float *times, int nt, int projection,
                                     void *out, int dtype_out, uint8_t *flags, uint32_t *trusted,
                                     uint8_t *cut, const hsflow_prefilter *pf,
                                     const hsflow_smoothness *sm, const hsflow_flow_init *init,
                                     const hsflow_fallback *fb, void *workspace,
                                     size_t workspace_bytes, void *stream);

/* The context's fallback: hsflow_flow_interp and hsflow_flow_interp_bgr honour
 * it and then equal their *_fb_device form bit for bit; the verdict comes down
 * with `trusted` on the stream the call drains anyway.  NULL or mode 0: off, the
 * default.  A bad mode or min_share is HSFLOW_ERR_ARG and leaves the old setting
 * in place.  hsflow_ctx_fallback reads it back.  hsflow_ctx_last_cut: the
 * verdict of the last such call on this context, 0 or 1; -1 where there was
 * none, it failed, or the fallback was off (and for a null context).  In
 * sequence mode a call whose verdict is a cut drops the stored prediction, so
 * the next call is the cold call, bit for bit; with the fallback off sequence
 * mode is what it was. */
int hsflow_ctx_set_fallback(hsflow_ctx *ctx, const hsflow_fallback *fb);
int hsflow_ctx_fallback(const hsflow_ctx *ctx, hsflow_fallback *fb);
int hsflow_ctx_last_cut(const hsflow_ctx *ctx);

/* ---- YUV 4:2:0 frame interpolation: I420 and NV12 in, the same layout out --
 * Video arrives as 4:2:0, not as BGR: a full-resolution luma plane and the two
 * chroma planes at half the size each way.  The luma plane is the grey frame
 * the solver wants, so it goes through the grey calls as it is -- no colour
 * conversion either way and half the bytes of BGR -- and the chroma follows
 * the same flows on its own grid.
 *
 * rows and cols are the luma's and both even (else HSFLOW_ERR_ARG);
 * rc = rows / 2, cc = cols / 2.  8-bit samples, dense planes (16-bit samples:
 * "16-bit YUV 4:2:0" further down).
 *   HSFLOW_YUV_I420  chroma [batch][2][rc][cc], the U plane then the V plane
 *   HSFLOW_YUV_NV12  chroma [batch][rc][cc][2], U and V interleaved
 * A packed frame p of rows * cols * 3 / 2 samples is y = p, c = p + rows * cols
 * in either layout.  Luma and chroma of a batch are separate dense arrays.
 *
 * The chroma of the frame at time t is, by definition and bit for bit,
 *   hsflow_downflow_device on (uf, vf) and on (ub, vb): per plane
 *     ((a + b) + (c + d)) * 0.125f over the 2 x 2 luma block, the block's mean
 *     flow in chroma pixels, and then
 *   hsflow_frame_interp_device (U8 frames, NULL masks) with those flows on the
 *     U planes of the two frames, rc x cc, and the same on the V planes.
 * So the sampler, the displacement clamp, the rim test (on the chroma grid),
 * the blend, the rounding of a U8 output and the handling of NaN and inf are
 * that call's.  A displacement is applied within the chroma grid, input and
 * output share their siting, so chroma siting does not enter.  Chroma has no
 * flags and no trusted count: the luma's are the frame's.
 * With a fallback a pair's verdict is the luma's: its counts against
 * hsflow_fallback_min_consistent(rows, cols, min_share), the luma's size.  A
 * pair that fails gets, per chroma byte, what hsflow_frame_fallback_device
 * writes for a grey U8 plane; a pair that passes keeps the interpolated chroma.
 * Luma projected and chroma not would fringe at motion boundaries, so the calls
 * below take no projection and the host call refuses a context that has it on;
 * the projected forms are further down ("YUV 4:2:0 with the flow projection":
 * hsflow_flow_interp_yuv_pj_device, hsflow_flow_interp_yuv_pj). */
#define HSFLOW_HAS_YUV 1
#define HSFLOW_YUV_I420 1
#define HSFLOW_YUV_NV12 2

/* KIY: the chroma of `nt` frames (times: host array, read at call time, each in
 * [0, 1], nt in 1 .. HSFLOW_MAX_TIMES) between the chroma c0 and c1 of `layout`,
 * from the four full-resolution flows (dense f32 [batch][rows][cols]).  out_c:
 * [batch][nt] chroma frames of the same layout, dtype_out U8 or F32.
 * counts_f, counts_b (device, uint32[batch][3], the luma's from
 * hsflow_flow_consistency_device) and fb: all given and fb's mode NEAREST or
 * BLEND for the fallback; fb NULL or mode 0 for none, the counts are then not
 * read.  Planes need element alignment only: flow planes on 8-byte boundaries
 * are read in 8-byte loads, a U8 output on a 4-byte boundary is written in
 * whole words, the bits are the same wherever they lie.  out_c must be disjoint
 * from every input.  All arguments are checked before any device work.  One
 * launch for both channels, all times and the whole batch.  Stream-ordered, no
 * workspace, never allocates or synchronises, capturable. */
int hsflow_chroma_interp_device(const uint8_t *c0, const uint8_t *c1, int layout, int rows,
                                int cols, int batch, const float *uf, const float *vf,
                                const float *ub, const float *vb, const uint32_t *counts_f,
                                const uint32_t *counts_b, const hsflow_fallback *fb,
                                const float *times, int nt, void *out_c, int dtype_out,
                                void *stream);

/* The fused call: hsflow_flow_interp_fb_device with projection 0 on the luma
 * planes y0, y1 (U8, dense [batch][rows][cols]) -- out_y, flags, trusted and cut
 * are that call's, bit for bit -- and then hsflow_chroma_interp_device on the
 * flows and counts that call leaves in the workspace.  out_y: [batch][nt] luma
 * planes, out_c: [batch][nt] chroma frames, both of dtype_out (U8 or F32).  The
 * form with a `projection` argument is hsflow_flow_interp_yuv_pj_device.  The
 * workspace is the grey call's: hsflow_flow_interp_yuv_workspace_bytes (fallback
 * != 0: with the counts of a fallback; 0 for a bad shape), a prefilter's planes
 * behind it, as ever.  No output may overlap an input, the workspace or another
 * output.  All arguments are checked before any device work. */
size_t hsflow_flow_interp_yuv_workspace_bytes(int rows, int cols, int batch, int levels,
                                              int fallback);
int hsflow_flow_interp_yuv_device(const uint8_t *y0, const uint8_t *c0, const uint8_t *y1,
                                  const uint8_t *c1, int layout, int rows, int cols, int batch,
                                  int levels, int finest, int warps, int median, int window,
                                  int iters, float alpha, float rel, float abs_thr,
                                  const float *times, int nt, void *out_y, void *out_c,
                                  int dtype_out, uint8_t *flags, uint32_t *trusted, uint8_t *cut,
                                  const hsflow_prefilter *pf, const hsflow_smoothness *sm,
                                  const hsflow_flow_init *init, const hsflow_fallback *fb,
                                  void *workspace, size_t workspace_bytes, void *stream);

/* Host, blocking: two packed frames f0, f1 of rows * cols * 3 / 2 bytes each in,
 * out[k] the packed frame at times[k] in the same layout, rows * cols * 3 / 2
 * elements of dtype_out (U8 or F32).  flags (NULL, or one dense rows x cols u8
 * plane per time) and trusted (NULL or uint32[nt]) are the luma's.  The context's
 * prefilter, smoothness, finest level, sequence mode and fallback are honoured
 * as by hsflow_flow_interp_bgr, and hsflow_ctx_last_cut is set; the result
 * equals the device call's bit for bit.  A context with the projection on is
 * HSFLOW_ERR_ARG: this call projects nothing; hsflow_flow_interp_yuv_pj takes the
 * projection as an argument. */
int hsflow_flow_interp_yuv(hsflow_ctx *ctx, const uint8_t *f0, const uint8_t *f1, int layout,
                           int rows, int cols, int levels, int warps, int median, int window,
                           int iters, double alpha, float rel, float abs_thr, const float *times,
                           int nt, void *const *out, int dtype_out, uint8_t *const *flags,
                           uint32_t *trusted);

/* The cap of KIY's grid in blocks per compute unit (each block takes tiles of
 * 512 chroma samples of one pair and strides), and how it fetches the two
 * adjacent taps of an NV12 row: as four bytes (0, the default) or as one
 * unaligned 32-bit load (1); same bits.  Returns the previous setting. */
/* The figure is the 8-bit policies' (5).  The 16-bit policies run under caps of
 * their own, never larger: I420-16 four blocks per CU, NV12-16 five
 * (hsflow_chroma_interp16_device). */
int hsflow_chroma_interp_blocks_per_cu(void);
int hsflow_set_chroma_nv12_loads(int wide);

/* ---- YUV 4:2:0 with the flow projection ---------------------------------------
 * The chroma reads its time-t flow through the luma's own winners, so that both
 * follow the same surface at a motion boundary.  `cells` is KS's plane
 * [batch][nt][rows][cols] from hsflow_flow_project_device on the luma frames
 * the solve ran on; rc = rows / 2, cc = cols / 2.
 *
 * KSD, the reduction: chroma cell (yc, xc) of a pair and time is the unsigned
 * 64-bit minimum of the luma cells (2 yc + {0, 1}, 2 xc + {0, 1}).  All ones is
 * the largest word: a hole loses to every candidate, and a chroma cell is a hole
 * only where all four are.  The winner keeps its upper word and its direction
 * bit; its source index p is clamped to rows * cols - 1, as KIP clamps a foreign
 * cell, and re-coded to the chroma grid, (p / cols >> 1) * cc + (p % cols >> 1).
 * The minimum comes first and the re-coding after it, so ties are the luma's:
 * the lower cost, then direction 0, then the lower luma index.
 *
 * The chroma of the frame at time t is, by definition and bit for bit,
 *   hsflow_downflow_device on (uf, vf) and on (ub, vb),
 *   hsflow_cells_down_device, and
 *   hsflow_frame_interp_proj_device (U8 frames, NULL masks, flags and trusted)
 *     with those flows and cells on the U planes, rc x cc, and on the V planes.
 * So a sample's time-t flow is the mean flow of the 2 x 2 luma block that holds
 * the winner, negated behind the mean for direction 1; a hole gets
 * hsflow_chroma_interp_device's value exactly.  No flags and no trusted count;
 * with a fallback a failed pair gets KF's value, as in
 * hsflow_chroma_interp_device. */
#define HSFLOW_HAS_YUV_PROJECTION 1

/* KSD: cells [batch][nt][rows][cols] -> cells_c [batch][nt][rc][cc], both
 * 8-byte aligned (a cell plane on a 16-byte boundary is read in 16-byte loads;
 * same words) and disjoint; rows and cols even, nt in 1 .. HSFLOW_MAX_TIMES.
 * All arguments are checked before any device work.  One launch.
 * Stream-ordered, no workspace, never allocates or synchronises, capturable. */
int hsflow_cells_down_device(const uint64_t *cells, int rows, int cols, int batch, int nt,
                             uint64_t *cells_c, void *stream);

/* KIYP: hsflow_chroma_interp_device with `cells` (KS's, of the luma, 8-byte
 * aligned) behind the flows: one launch for the three steps above on both
 * channels, all times and the whole batch; the chroma cells never reach memory.
 * Every other argument, the checks and the contract are that call's; out_c must
 * be disjoint from the cells too. */
int hsflow_chroma_interp_proj_device(const uint8_t *c0, const uint8_t *c1, int layout, int rows,
                                     int cols, int batch, const float *uf, const float *vf,
                                     const float *ub, const float *vb, const uint64_t *cells,
                                     const uint32_t *counts_f, const uint32_t *counts_b,
                                     const hsflow_fallback *fb, const float *times, int nt,
                                     void *out_c, int dtype_out, void *stream);

/* hsflow_flow_interp_yuv_device with `projection` after nt.  0: exactly that
 * call's launches and bits.  1: hsflow_flow_interp_fb_device with projection 1
 * on the luma -- out_y, flags (bit 16 for a hole), trusted and cut are that
 * call's -- and then hsflow_chroma_interp_proj_device on the flows, cells and
 * counts it leaves in the workspace.  Any other value is HSFLOW_ERR_ARG.  The
 * workspace: hsflow_flow_interp_yuv_pj_workspace_bytes (0 for a bad shape, nt or
 * projection), a prefilter's planes behind it. */
size_t hsflow_flow_interp_yuv_pj_workspace_bytes(int rows, int cols, int batch, int levels,
                                                 int nt, int projection, int fallback);
int hsflow_flow_interp_yuv_pj_device(const uint8_t *y0, const uint8_t *c0, const uint8_t *y1,
                                     const uint8_t *c1, int layout, int rows, int cols, int batch,
                                     int levels, int finest, int warps, int median, int window,
                                     int iters, float alpha, float rel, float abs_thr,
                                     const float *times, int nt, int projection, void *out_y,
                                     void *out_c, int dtype_out, uint8_t *flags,
                                     uint32_t *trusted, uint8_t *cut, const hsflow_prefilter *pf,
                                     const hsflow_smoothness *sm, const hsflow_flow_init *init,
                                     const hsflow_fallback *fb, void *workspace,
                                     size_t workspace_bytes, void *stream);

/* hsflow_flow_interp_yuv with an explicit `projection` (0 or 1, else
 * HSFLOW_ERR_ARG) after nt; the context's projection setting is not consulted.
 * Prefilter, smoothness, finest level, sequence mode and fallback are
 * honoured and hsflow_ctx_last_cut is set, as by that call; the result equals
 * hsflow_flow_interp_yuv_pj_device's bit for bit. */
int hsflow_flow_interp_yuv_pj(hsflow_ctx *ctx, const uint8_t *f0, const uint8_t *f1, int layout,
                              int rows, int cols, int levels, int warps, int median, int window,
                              int iters, double alpha, float rel, float abs_thr,
                              const float *times, int nt, int projection, void *const *out,
                              int dtype_out, uint8_t *const *flags, uint32_t *trusted);

/* The cap of KIYP's grid in blocks per compute unit (tiles of 512 chroma
 * samples of one pair, striding, as KIY). */
/* The figure is the 8-bit policies' (4); with cells the 16-bit policies run
 * under I420-16 three blocks per CU, NV12-16 four. */
int hsflow_chroma_interp_proj_blocks_per_cu(void);

/* ---- 16-bit YUV 4:2:0: yuv420p10le .. p16le (I420), P010 .. P016 (NV12) ------
 * The calls above take 8-bit samples, dense planes.  These take the frames a
 * 10-, 12- or 16-bit decoder hands out: the same two layouts with 2-byte
 * little-endian samples, in and out.
 *
 * A 16-bit sample is its value as a number, 0 .. 65535, whatever the bit depth:
 * yuv420p10le holds 0 .. 1023, P010 the value shifted left by 6.  Every kernel
 * converts a frame element to float on load and computes in f32, so a U16 plane
 * gives, bit for bit, what the same values give as an HSFLOW_F32 plane in the
 * 8-bit section's definitions -- with one stated exception, the pyramid: a U16
 * pair is never treated as 8-bit.  K1's integrality test (integers in [0, 255]
 * make the pyramid round every level to integers) is not run on U16 frames; the
 * levels are always the unrounded S / 324.  That is what F32 frames get
 * whenever either frame of the pair holds a sample above 255, so for such a
 * pair the equality with the F32 call is exact on every level.
 *
 * A U16 output element is floorf(x + 0.5f) clamped to 0 .. 65535, NaN -> 0, of
 * the f32 value x that the F32 output holds.  Sampling and blending are
 * convex, so a 10-bit input never leaves 0 .. 1023 and the calls take no depth
 * argument.  For P010 the low six bits of an output sample are in general not
 * zero: the result is a valid P016 frame, and nothing is masked.
 *
 * Alpha: a frame scaled by k behaves like alpha divided by k.  Relative to the
 * 8-bit recommendation of about 100, use alpha x 4 for 10-bit LSB-aligned
 * content (yuv420p10le) and alpha x 256 for P010. */
#define HSFLOW_HAS_YUV16 1

/* KIY (cells NULL) or KIYP (cells: KS's, of the luma, 8-byte aligned) on
 * 16-bit chroma: hsflow_chroma_interp_device's, or with cells
 * hsflow_chroma_interp_proj_device's, definition on the sample values, layouts
 * HSFLOW_YUV_I420 and HSFLOW_YUV_NV12 with 2-byte samples; out_c: [batch][nt]
 * chroma frames of the same layout, dtype_out HSFLOW_U16 or HSFLOW_F32.  The
 * contract is hsflow_chroma_interp_device's: the planes need element (2-byte;
 * an F32 output 4-byte) alignment only, out_c is disjoint from every input,
 * all arguments are checked before any device work, one launch,
 * stream-ordered, capturable, no allocation. */
int hsflow_chroma_interp16_device(const uint16_t *c0, const uint16_t *c1, int layout, int rows,
                                  int cols, int batch, const float *uf, const float *vf,
                                  const float *ub, const float *vb, const uint64_t *cells,
                                  const uint32_t *counts_f, const uint32_t *counts_b,
                                  const hsflow_fallback *fb, const float *times, int nt,
                                  void *out_c, int dtype_out, void *stream);

/* hsflow_flow_interp_yuv_pj_device on 16-bit frames: the luma through
 * hsflow_flow_interp_fb_device's path as HSFLOW_U16 frames (prefilter,
 * smoothness, finest level, init, projection 0 or 1 and fallback included; the
 * pyramid as stated above), then hsflow_chroma_interp16_device on the flows,
 * cells and counts left in the workspace.  out_y and out_c: dtype_out
 * HSFLOW_U16 or HSFLOW_F32.  The workspace is
 * hsflow_flow_interp_yuv_pj_workspace_bytes: the flows are f32 either way.
 * Stream-ordered; never allocates or synchronises.  Limitation: do not replay a
 * captured graph of this call more than once.  A first replay equals the eager
 * call; later replays of a graph of the fused YUV calls (this one and
 * hsflow_flow_interp_yuv_device / _pj_device alike) have been observed to differ
 * from it -- a pair that passes the check judged a cut -- while eager calls on
 * the same workspace stay right.  hsflow_chroma_interp16_device, one launch, is
 * not affected. */
int hsflow_flow_interp_yuv16_device(const uint16_t *y0, const uint16_t *c0, const uint16_t *y1,
                                    const uint16_t *c1, int layout, int rows, int cols, int batch,
                                    int levels, int finest, int warps, int median, int window,
                                    int iters, float alpha, float rel, float abs_thr,
                                    const float *times, int nt, int projection, void *out_y,
                                    void *out_c, int dtype_out, uint8_t *flags,
                                    uint32_t *trusted, uint8_t *cut, const hsflow_prefilter *pf,
                                    const hsflow_smoothness *sm, const hsflow_flow_init *init,
                                    const hsflow_fallback *fb, void *workspace,
                                    size_t workspace_bytes, void *stream);

/* The host form, hsflow_flow_interp_yuv_pj's on packed frames of rows * cols *
 * 3 / 2 16-bit samples (f0, f1 and each out[k]; out of dtype_out HSFLOW_U16 or
 * HSFLOW_F32).  Prefilter, smoothness, finest level, sequence mode and fallback
 * of the context are honoured and hsflow_ctx_last_cut is set; the result equals
 * hsflow_flow_interp_yuv16_device's bit for bit. */
int hsflow_flow_interp_yuv16(hsflow_ctx *ctx, const uint16_t *f0, const uint16_t *f1, int layout,
                             int rows, int cols, int levels, int warps, int median, int window,
                             int iters, double alpha, float rel, float abs_thr,
                             const float *times, int nt, int projection, void *const *out,
                             int dtype_out, uint8_t *const *flags, uint32_t *trusted);

/* ---- host utilities on the path to the hot loop ------------------------ */

/* main.cpp:13-14 cv::cvtColor(BGR2GRAY) for 8-bit BGR, OpenCV 4.x 15-bit
 * fixed point: Y = (9798 R + 19235 G + 3735 B + 16384) >> 15. */
int hsflow_bgr_to_gray(const uint8_t *bgr, int rows, int cols, size_t bgr_step,
                       uint8_t *gray, size_t gray_step);

/* The same conversion on the device (stream-ordered): `batch` dense BGR
 * planes [batch][rows][cols][3] -> dense gray [batch][rows][cols]. */
int hsflow_bgr_to_gray_device(const uint8_t *bgr, int rows, int cols, int batch,
                              uint8_t *gray, void *stream);

/* main.cpp:50-51 + :13-14 + :97-98 in one call: two decoded 8-bit BGR frames
 * (row steps bgr_step0, bgr_step1 bytes) are uploaded as BGR, converted on
 * the GPU and solved (hornSchunck::getFlow); u/v as in hsflow_flow. */
int hsflow_flow_bgr(hsflow_ctx *ctx, const uint8_t *bgr0, const uint8_t *bgr1, int rows,
                    int cols, size_t bgr_step0, size_t bgr_step1, int window, int iters,
                    double alpha, void *u, void *v, int dtype_out, size_t out_step);

/* Deterministic synthetic frame pair: I0 = smoothed hash noise
 * around 128 (integer-valued 0..255), I1 = I0's texture shifted by
 * (dy, dx) = (qdy/4, qdx/4) px with integer bilinear weights.  Outputs are
 * rows x cols f32 (dense) and/or u8 (either pointer may be NULL). */
int hsflow_synth_pair(uint64_t seed, int rows, int cols, int qdy, int qdx,
                      float *I0, float *I1, uint8_t *I0_u8, uint8_t *I1_u8);

#ifdef __cplusplus
}
#endif
#endif /* HSFLOW_H */
