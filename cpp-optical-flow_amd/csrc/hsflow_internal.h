// hsflow_internal.h -- shared between the kernels and the C-ABI layer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <atomic>
#include <vector>

namespace hsflow {

// Arguments of one Jacobi launch (hornSchunck.cpp:56-74 x `iters`).
struct JacobiArgs {
    int rows, cols, batch;
    int iters;             // iterations fused in this launch (<= KB)
    int tiles_x, tiles_y;  // filled by the launcher
    float alpha2;          // pow(alpha, 2)            (hornSchunck.cpp:68)
    float inv_w2;          // 1 / pow(windowSize, 2)   (hornSchunck.cpp:53)
    const float *u_in, *v_in;  // nullptr -> initial state u = v = 0 (:49-50)
    float *u_out, *v_out;
    const uint32_t *gpack;     // packed exact integer gradients
    const float *gx, *gy, *gt; // f32 gradients (non-integral inputs)
    const uint32_t *flags;     // per pair: 0 -> gpack valid, else f32 planes
    int seg_rows;              // K4 strip kernel: output rows per segment
    int write_through;         // store u', v' write-through (sc1) instead of nt: launches
                               // that do not fill the chip (fill_limited)
    int il_in, il_out;         // K4: the input / output state is interleaved: row r as
                               // {u0, u1, v0, v1} groups in the u plane (r even) or the v
                               // plane (r odd) at the offset of row r & ~1 (hsflow_strips.hip)
};

// What the fused first pass of a cold K4 solve takes besides JacobiArgs: the
// frames it computes K1's gradients from, and K1's outputs, which it writes
// (hsflow_strips.hip hs_jacobi_strip_first_kernel)
struct FirstArgs {
    const void *I0, *I1;  // the batch's frames (u8, f16 or f32), dense
    uint32_t *gpack;      // packed gradients of every pixel
    uint32_t *flags;      // per pair; zero before the launch unless the frames are u8
    int wide;             // the frames' base addresses allow one load per column pair
};

// K1 (+ K1f): packed gradients and flags; the f32 planes for every pair
// when `planes` (the gradients API), else only for the flagged pairs
hipError_t launch_gradients(const void *I0, const void *I1, int dtype_in, int rows,
                            int cols, int batch, uint32_t *gpack, float *gx, float *gy,
                            float *gt, uint32_t *flags, bool planes, hipStream_t s);
// K1f alone: the f32 planes of the pairs `flags` marks (after a fused first
// pass, which writes the packed plane and the flags itself); nothing to do
// for u8 frames
hipError_t launch_gradients_f32(const void *I0, const void *I1, int dtype_in, int rows,
                                int cols, int batch, float *gx, float *gy, float *gt,
                                const uint32_t *flags, hipStream_t s);
hipError_t launch_jacobi(JacobiArgs a, int W, int KB, hipStream_t s);
// config 5 pyramid (hsflow_pyramid.hip); dtype as HSFLOW_U8/F32/F16/U16
hipError_t launch_pyrdown(const void *src, int dtype, int rows, int cols, int batch,
                          float *dst, const uint32_t *flags, hipStream_t s);
// GPU input path (hsflow_input.hip): dense BGR u8 planes -> gray u8
hipError_t launch_bgr2gray(const uint8_t *bgr, int rows, int cols, int batch,
                           uint8_t *gray, hipStream_t s);
hipError_t launch_upflow(const float *uc, const float *vc, int rc, int cc, float *u,
                         float *v, int rows, int cols, int batch, hipStream_t s);
// KW (hsflow_warp.hip): one level's gradients linearised around (u0, v0) into
// the f32 planes -- gx, gy as K1's, gt' = (I1 warped by 8 (u0, v0)) - I0 -
// gx u0 - gy v0 -- and flags[pair] = 1 (the Jacobi passes read the planes)
hipError_t launch_warp_gradients(const void *I0, const void *I1, int dtype_in, int rows,
                                 int cols, int batch, const float *u0, const float *v0,
                                 float *gx, float *gy, float *gt, uint32_t *flags,
                                 hipStream_t s);
// KC (hsflow_consistency.hip): forward-backward check of (uf, vf) against
// (ub, vb), dense f32 batch planes -> err (f32, px), mask (u8: 0 consistent,
// 1 inconsistent, 2 out of frame) and counts[batch][3]; each output may be
// null.  counts must be zero before the launch (the kernel adds).
hipError_t launch_consistency(const float *uf, const float *vf, const float *ub,
                              const float *vb, int rows, int cols, int batch, float rel,
                              float abs_thr, float *err, uint8_t *mask, uint32_t *counts,
                              hipStream_t s);
// KM (hsflow_median.hip): ksize x ksize (3 or 5) median of u and of v, each
// on its own, dense f32 batch planes, out of place; border replicated, IEEE
// total order of the bit patterns (the result is one of the taps)
hipError_t launch_median(const float *u, const float *v, int rows, int cols, int batch, int ksize,
                         float *u_out, float *v_out, hipStream_t s);
// KR (hsflow_interp.hip): out (f32) = I sampled bilinearly at (y + 8 v, x + 8 u),
// KW's arithmetic; oof (u8, may be null): 1 where the target leaves the frame
// by more than half a pixel
hipError_t launch_warp_image(const void *I, int dtype_in, int rows, int cols, int batch,
                             const float *u, const float *v, float *out, uint8_t *oof,
                             hipStream_t s);
// KI (hsflow_interp.hip): the frames at `nt` (1..kInterpMaxTimes) times between
// I0 and I1 from the flows both ways -> out [batch][nt] planes (out_kind: f32,
// u8 or, for 16-bit frames only, u16), flags (u8, may be null) and
// trusted[batch][nt] (may be null; must be zero before the launch: the kernel
// adds).  mask_f / mask_b: KC's masks, each may be null.  `times` is read on the
// host at launch.
constexpr int kInterpMaxTimes = 16;
constexpr int kOutF32 = 0, kOutU8 = 1, kOutU16 = 2;  // what an interpolation writes
hipError_t launch_frame_interp(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                               int batch, const float *uf, const float *vf, const float *ub,
                               const float *vb, const uint8_t *mask_f, const uint8_t *mask_b,
                               const float *times, int nt, void *out, int out_kind,
                               uint8_t *flags, uint32_t *trusted, hipStream_t s);
// KRC, KIC (hsflow_interp_bgr.hip): KR and KI on dense 8-bit interleaved BGR
// frames [batch][rows][cols][3] -> out [..][rows][cols][3] (f32, or u8 when
// out_u8); oof, flags, trusted as KR's and KI's, one value per pixel
hipError_t launch_warp_image_bgr(const uint8_t *I, int rows, int cols, int batch, const float *u,
                                 const float *v, void *out, bool out_u8, uint8_t *oof,
                                 hipStream_t s);
hipError_t launch_frame_interp_bgr(const uint8_t *I0, const uint8_t *I1, int rows, int cols,
                                   int batch, const float *uf, const float *vf, const float *ub,
                                   const float *vb, const uint8_t *mask_f, const uint8_t *mask_b,
                                   const float *times, int nt, void *out, bool out_u8,
                                   uint8_t *flags, uint32_t *trusted, hipStream_t s);
// KS (hsflow_project.hip): both flows carried to each of `nt` times: every pixel
// of G0 (by uf, vf over t) and of G1 (by ub, vb over 1 - t) bids for the cell
// it lands on with cost << 32 | dir << 31 | its index; cells [batch][nt] planes
// of u64, all ones before the launch (the kernel takes minima).  `times` is
// read on the host at launch.
hipError_t launch_flow_project(const void *G0, const void *G1, int dtype_in, int rows, int cols,
                               int batch, const float *uf, const float *vf, const float *ub,
                               const float *vb, const float *times, int nt, uint64_t *cells,
                               hipStream_t s);
// KIP (hsflow_interp.hip, hsflow_interp_bgr.hip): KI and KIC with each output
// pixel's time-t flow read at the source pixel its cell names; an empty cell
// falls back to KI's formula and sets flag bit 16
hipError_t launch_frame_interp_proj(const void *I0, const void *I1, int dtype_in, int rows,
                                    int cols, int batch, const float *uf, const float *vf,
                                    const float *ub, const float *vb, const uint8_t *mask_f,
                                    const uint8_t *mask_b, const uint64_t *cells,
                                    const float *times, int nt, void *out, int out_kind,
                                    uint8_t *flags, uint32_t *trusted, hipStream_t s);
hipError_t launch_frame_interp_bgr_proj(const uint8_t *I0, const uint8_t *I1, int rows, int cols,
                                        int batch, const float *uf, const float *vf,
                                        const float *ub, const float *vb, const uint8_t *mask_f,
                                        const uint8_t *mask_b, const uint64_t *cells,
                                        const float *times, int nt, void *out, bool out_u8,
                                        uint8_t *flags, uint32_t *trusted, hipStream_t s);
// KF (hsflow_fallback.hip): for every pair whose consistent pixels, counts_f[b][0]
// + counts_b[b][0] of KC's counts as a 64-bit sum, number fewer than
// min_consistent: out of all nt times = I0 / I1 by `mode` (1: the nearer frame,
// 2: KI's blend at wt = t), flags = 32, trusted[b][t] = 0; cut[b] = the verdict
// of every pair.  A pair that passes keeps its out, flags and trusted.  flags,
// trusted and cut may be null.  `times` is read on the host at launch.
hipError_t launch_frame_fallback(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                                 int batch, const uint32_t *counts_f, const uint32_t *counts_b,
                                 uint64_t min_consistent, int mode, const float *times, int nt,
                                 void *out, int out_kind, uint8_t *flags, uint32_t *trusted,
                                 uint8_t *cut, hipStream_t s);
hipError_t launch_frame_fallback_bgr(const uint8_t *I0, const uint8_t *I1, int rows, int cols,
                                     int batch, const uint32_t *counts_f,
                                     const uint32_t *counts_b, uint64_t min_consistent, int mode,
                                     const float *times, int nt, void *out, bool out_u8,
                                     uint8_t *flags, uint32_t *trusted, uint8_t *cut,
                                     hipStream_t s);
// KIY (hsflow_yuv.hip): the chroma of the frames between two 4:2:0 frames, from
// the full-resolution flows of the luma solve (rows, cols: the luma's, even):
// KD's 2 x 2 reduction and KI on the rc x cc chroma grid for U and V in one
// launch, for all times and pairs.  layout 1: I420 [batch][2][rc][cc], 2: NV12
// [batch][rc][cc][2], of 8-bit (dtype_in 0) or 16-bit (dtype_in 4) samples; out
// [batch][nt] of that layout: f32 or the frames' own integer type (out_kind).
// With counts (both or neither; null: no fallback) a pair that fails
// min_consistent gets KF's value by `mode`.  `times` is read on the host at
// launch.
hipError_t launch_chroma_interp(const void *c0, const void *c1, int dtype_in, int layout,
                                int rows, int cols, int batch, const float *uf, const float *vf,
                                const float *ub, const float *vb, const uint32_t *counts_f,
                                const uint32_t *counts_b, uint64_t min_consistent, int mode,
                                const float *times, int nt, void *out, int out_kind,
                                hipStream_t s, const uint64_t *cells = nullptr);
// the cap of KIY's grid, in blocks per CU
int chroma_blocks_per_cu();
// KSD (hsflow_yuv.hip): KS's cells [planes][rows][cols] (planes = batch * nt)
// reduced to the chroma grid, cells_c [planes][rows / 2][cols / 2]: the 64-bit
// minimum of each 2 x 2 block, the winner's index re-coded to the chroma grid.
// KIYP: launch_chroma_interp with `cells` (KS's, [batch][nt][rows][cols]) reads
// each sample's time-t flow through that minimum, taken in registers.
hipError_t launch_cells_down(const uint64_t *cells, int rows, int cols, int planes,
                             uint64_t *cells_c, hipStream_t s);
// the cap of KIYP's grid, in blocks per CU
int chroma_proj_blocks_per_cu();
// how KIY fetches the two adjacent taps of an NV12 row: as four bytes (on == 0,
// default) or as one unaligned dword; same bits.  Returns the previous setting.
int set_chroma_nv12_wide_loads(int on);
// how KRC and KIC fetch the two adjacent taps of a row: as six bytes (on == 0,
// default) or as one unaligned dword and halfword; same bits.  Returns the
// previous setting.
int set_interp_bgr_wide_loads(int on);
// KN (hsflow_prefilter.hip): v = I - G*I (mode 1) or scale v / (sqrt(G*(v v)) +
// eps) (mode 2), G the separable Gaussian of `radius` (1..kPrefilterMaxRadius)
// with weights[0..radius] (read on the host at launch), reflect-101 folded;
// dense batch planes of dtype_in -> f32
constexpr int kPrefilterMaxRadius = 15;
hipError_t launch_prefilter(const void *I, int dtype_in, int rows, int cols, int batch, int mode,
                            int radius, const float *weights, float eps, float scale, float *out,
                            hipStream_t s);
// KG (hsflow_smooth.hip): the flow-driven smoothness weights of (u, v), dense
// f32 batch planes -> g = 1 / sqrt(1 + |grad (8u, 8v)|^2 / lambda^2), central
// differences with the border replicated
hipError_t launch_diffusivity(const float *u, const float *v, int rows, int cols, int batch,
                              float lambda, float *g, hipStream_t s);
// KJ (hsflow_smooth.hip): one pass of a.iters (<= KB) g-weighted Jacobi
// iterations from the f32 gradient planes (a.gx, a.gy, a.gt) and the weights
// g; a.u_in / a.v_in are required (always a warm start), a.gpack and a.flags
// are not read.  W = 3 or 5; same bits for every supported KB.
bool weighted_kb_supported(int W, int KB);
int weighted_default_kb(int W);
hipError_t launch_jacobi_weighted(JacobiArgs a, const float *g, int W, int KB, hipStream_t s);
// KD (hsflow_temporal.hip): a flow plane pair one level down, KU's
// counterpart: uc = the mean of the 2 x 2 block (border replicated) halved;
// rc, cc must be ceil(rows / 2), ceil(cols / 2)
hipError_t launch_downflow(const float *u, const float *v, int rows, int cols, float *uc,
                           float *vc, int rc, int cc, int batch, hipStream_t s);
// KP (hsflow_temporal.hip): pair k's backward flow (ub, vb) -> the start of
// pair k+1: (uf_next, vf_next) = -(ub, vb), (ub_next, vb_next) = (ub, vb)
// sampled at (y + 8 vb, x + 8 ub), KR's bits; either output pair may be null
hipError_t launch_flow_predict(const float *ub, const float *vb, int rows, int cols, int batch,
                               float *uf_next, float *vf_next, float *ub_next, float *vb_next,
                               hipStream_t s);
// KB (hsflow_upsample.hip): a flow plane pair one level up, bilinearly (pixel
// centres aligned, border replicated, values doubled): the way a coarse
// solve's flow reaches the full frame; rc, cc must be ceil(rows / 2),
// ceil(cols / 2)
hipError_t launch_upflow_bilinear(const float *uc, const float *vc, int rc, int cc, float *u,
                                  float *v, int rows, int cols, int batch, hipStream_t s);
// K4 (hsflow_strips.hip): the streaming pass for the (window, KB) pairs it
// is built for; `slots` = waves the chip holds at its occupancy
bool strip_supported(int W, int KB);
// the state between two K4 passes of this shape may be interleaved
// (JacobiArgs::il_in / il_out); a fused first pass writes it only from frames
// that are strip_first_wide
bool strip_interleave_ok(int W, int KB, int rows, int cols);
bool strip_first_wide(const void *I0, const void *I1, int dtype_in);
hipError_t launch_jacobi_strip(JacobiArgs a, int W, int KB, int seg_rows, hipStream_t s);
// pass 0 of a cold solve with K1 fused in (a.u_in / a.v_in ignored: u = v = 0);
// dtype_in HSFLOW_U8, F16 or F32
hipError_t launch_jacobi_strip_first(JacobiArgs a, FirstArgs f, int dtype_in, int W, int KB,
                                     int seg_rows, hipStream_t s);
int strip_seg_rows(int W, int KB, int rows, int cols, int batch, int slots, int *nseg,
                   int *nstrips, int override_rows);
bool strip_fills(int W, int KB, int rows, int cols, int batch, int slots);
// compute units of the current device (cached per device)
int device_cus();
int default_kb(int W);
// default_kb adjusted for launches that do not fill one round of slots
int fill_kb(int W, int kb, int rows, int cols, int batch);
bool kb_supported(int W, int KB, bool need_f32);
// the solve's launches leave most of the chip idle (all pairs in flight):
// their outputs are stored write-through (JacobiArgs::write_through);
// strip_rows = the K4 segment height the launches use (0: 84)
bool fill_limited(int W, int KB, bool strip, int rows, int cols, int batch, int strip_rows);

// ---- host I/O of the host-buffer entry points (hsflow_hostio.cpp) ----
// threads of the host copy pool (the caller included)
int host_pool_width();
// hsflow_set_output_hugepages: advise MADV_HUGEPAGE on f64 outputs (1, default)
extern std::atomic<int> g_output_hugepages;
// n dense device f32 planes -> host rows (f64 when `f64`, else f32; row step
// `step`).  f32: DMA copies straight into the rows.  f64: through `stage`
// (n * rows * cols floats, pinned) in row chunks, each widened by the pool
// as soon as it has arrived.  Returns when every row is in place (the
// stream has drained).
hipError_t download_planes_pipelined(const float *const *src, void *const *dst, int n, int rows,
                                     int cols, bool f64, size_t step, float *stage,
                                     std::vector<hipEvent_t> &events, hipStream_t s);

}  // namespace hsflow
