// hsflow_interp.hip -- what the bidirectional solve is for: warping a frame by
// a flow and synthesising the frame between two ("Frame
// interpolation").
//
//  KR hs_warp_image_kernel    out(y, x) = I sampled bilinearly at
//     (y + 8 v, x + 8 u) by the sampler KW uses (hsflow_sampler.h:
//     displacement clamped as a float to [-cols, cols] / [-rows, rows], NaN ->
//     lower bound; floorf split; taps clamped to the plane; top, bottom, then
//     vertical; f64 frames sampled in f64, rounded once), so the plane equals
//     the I1w inside KW's gt' bit for bit.  oof (optional, u8): 1 where the
//     target leaves the frame by more than half a pixel (KC's rim test).
//
//  KI hs_frame_interp_kernel  the frame at time t in [0, 1] between I0 and
//     I1 from the flows I0 -> I1 (uf, vf) and I1 -> I0 (ub, vb), solver units,
//     all four read at the output pixel (Jiang et al., CVPR 2018, eq. 4):
//       s = 1 - t;  a = s t;  b = t t;  c = s s
//       u0 = b ub - a uf;  v0 = b vb - a vf       time t back to frame 0
//       u1 = c uf - a ub;  v1 = c vf - a vb       time t on to frame 1
//       s0 = I0 at (y + 8 v0, x + 8 u0);  s1 = I1 at (y + 8 v1, x + 8 u1)   (KR)
//       in0, in1 = KC's rim test of the two targets (negated: NaN -> out)
//       wt  = t where in0 == in1, 0 where only in0, 1 where only in1
//       out = wt == 0 ? s0 : wt == 1 ? s1 : (1 - wt) s0 + wt s1
//       flags = !in0 | !in1 << 1 | (mask_f[n0] != 0) << 2 | (mask_b[n1] != 0) << 3
//     n0, n1: the source pixels nearest to the targets (integer part, plus one
//     where the fraction >= 0.5, clamped to the plane).  One launch serves nt
//     <= 16 times, which travel by value in the kernel arguments: a thread
//     loads the four flow values of each of its two pixels once and loops over
//     the times.  trusted[pair][time] counts the pixels with flags == 0.
//     The kernel is the sampler's, written once over a frame policy
//     (hsflow_frame_policy.h): GreyFrame here, BgrFrame in hsflow_interp_bgr.hip
//     (KIC).
//
// HBM-bound: 16 B/px of flows once and, per time, 8 B/px of f32 frames (the
// taps of neighbouring pixels overlap) read, 4 + 1 B/px written.  KI's map is
// KC's without the shifted tile start: a block of 256 threads takes tiles of
// 512 consecutive pixels of a pair's plane, thread t the pixels t and t + 256,
// so the flow loads, the taps of a smooth flow and the f32 stores coalesce and
// the two pixels' 16 tap loads are in flight at once (four pixels per thread
// cost 99 VGPRs and half the waves per SIMD).
// Quads of lanes hold the pixels 4q .. 4q + 3 of the plane; where those four
// bytes of a u8 plane (flags, u8 out) form an aligned dword -- every quad of
// every plane when rows * cols is a multiple of four and the base is aligned
// -- lane 0 of the quad collects them over DPP and stores them at once, else
// each lane stores its byte.  The grid is capped at six blocks per CU and
// strides over the tiles, so a (pair, time) count takes one atomic per block.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hsflow_frame_policy.h"
#include "hsflow_internal.h"
#include "hsflow_sampler.h"

namespace hsflow {
namespace {

using namespace sampler;

// ---- KR: block 64 x 4, one pixel per thread (KW's map);
// grid (ceil(cols/64), ceil(rows/4), batch)
template <typename T>
__global__ __launch_bounds__(256) void hs_warp_image_kernel(
    const T *__restrict__ I, const float *__restrict__ u, const float *__restrict__ v, int rows,
    int cols, float *__restrict__ out, uint8_t *__restrict__ oof) {
    const int x = blockIdx.x * 64 + threadIdx.x;
    const int y = blockIdx.y * 4 + threadIdx.y;
    if (x >= cols || y >= rows) return;
    const size_t plane = (size_t)rows * cols;
    const size_t o = blockIdx.z * plane + (size_t)y * cols + x;
    bool in;
    int nearest;
    const Taps t = sample_taps(rows, cols, x, y, u[o], v[o], in, nearest);
    out[o] = (float)sample_plane(I + blockIdx.z * plane, cols, t);
    if (oof) oof[o] = in ? 0 : 1;
}

}  // namespace

hipError_t launch_warp_image(const void *I, int dtype_in, int rows, int cols, int batch,
                             const float *u, const float *v, float *out, uint8_t *oof,
                             hipStream_t s) {
    const bool known = dispatch_frame_type(dtype_in, [&](auto t) {
        using T = decltype(t);
        dim3 blk(64, 4, 1), grd((cols + 63) / 64, (rows + 3) / 4, batch);
        hipLaunchKernelGGL(hs_warp_image_kernel<T>, grd, blk, 0, s, (const T *)I, u, v, rows, cols,
                           out, oof);
    });
    if (!known) return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_frame_interp(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                               int batch, const float *uf, const float *vf, const float *ub,
                               const float *vb, const uint8_t *mask_f, const uint8_t *mask_b,
                               const float *times, int nt, void *out, int out_kind,
                               uint8_t *flags, uint32_t *trusted, hipStream_t s) {
    hipError_t e = hipErrorInvalidValue;  // stays for an unknown dtype
    dispatch_frame_type(dtype_in, [&](auto t) {
        e = launch_frame_interp_as<GreyFrame<decltype(t)>>(I0, I1, rows, cols, batch, uf, vf, ub,
                                                           vb, mask_f, mask_b, times, nt, out,
                                                           out_kind, flags, trusted, s);
    });
    return e;
}

// KIP: KI with each output pixel's time-t flow taken from the source pixel its
// cell names (hsflow_project.hip)
hipError_t launch_frame_interp_proj(const void *I0, const void *I1, int dtype_in, int rows,
                                    int cols, int batch, const float *uf, const float *vf,
                                    const float *ub, const float *vb, const uint8_t *mask_f,
                                    const uint8_t *mask_b, const uint64_t *cells,
                                    const float *times, int nt, void *out, int out_kind,
                                    uint8_t *flags, uint32_t *trusted, hipStream_t s) {
    hipError_t e = hipErrorInvalidValue;  // stays for an unknown dtype or null cells
    if (!cells) return e;
    dispatch_frame_type(dtype_in, [&](auto t) {
        e = launch_frame_interp_as<GreyFrame<decltype(t)>>(I0, I1, rows, cols, batch, uf, vf, ub,
                                                           vb, mask_f, mask_b, times, nt, out,
                                                           out_kind, flags, trusted, s, cells);
    });
    return e;
}

}  // namespace hsflow
