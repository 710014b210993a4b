// hsflow_interp.hip -- what the bidirectional solve is for: warping a frame by
// a flow and synthesising the frame between two ("Frame
// interpolation").
//
//  KR hs_warp_image_kernel    out(y, x) = I sampled bilinearly at
//     (y + 8 v, x + 8 u), KW's arithmetic term for term (hsflow_warp.hip:
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
// each lane stores its byte.  The grid is capped at six blocks per CU (what
// every instantiation's registers let a CU hold) and strides over the tiles,
// so a (pair, time) count takes one atomic per block.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "hsflow_internal.h"
#include "hsflow_sampler.h"

namespace hsflow {
namespace {

using namespace sampler;

// double for CV_64FC1 frames (sampled in float64, one rounding), else float
template <typename T> struct SampleMath { using type = float; };
template <> struct SampleMath<double> { using type = double; };

// img (one pair's plane) at (y + 8 v, x + 8 u): KW's sample, the positions,
// weights and lerps of hsflow_sampler.h (shared with the colour kernels of
// hsflow_interp_bgr.hip).  in: the target is within half a pixel of the frame
// (KC's test); nearest: index in the plane of the source pixel nearest to the
// target.
template <typename T>
__device__ __forceinline__ float sample(const T *__restrict__ img, int rows, int cols, int x,
                                        int y, float u, float v, bool &in, int &nearest) {
    using F = typename SampleMath<T>::type;
    const Taps t = sample_taps(rows, cols, x, y, u, v, in, nearest);
    const T *top = img + (size_t)t.ya * cols;
    const T *bot = img + (size_t)t.yb * cols;
    const F ta = (F)top[t.xa], tb = (F)top[t.xb], ba = (F)bot[t.xa], bb = (F)bot[t.xb];
    return (float)lerp_taps<F>(ta, tb, ba, bb, t.fx, t.fy);
}

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
    out[o] = sample(I + blockIdx.z * plane, rows, cols, x, y, u[o], v[o], in, nearest);
    if (oof) oof[o] = in ? 0 : 1;
}

template <typename T>
void launch_warp_t(const void *I, const float *u, const float *v, int rows, int cols, int batch,
                   float *out, uint8_t *oof, hipStream_t s) {
    dim3 blk(64, 4, 1), grd((cols + 63) / 64, (rows + 3) / 4, batch);
    hipLaunchKernelGGL(hs_warp_image_kernel<T>, grd, blk, 0, s, (const T *)I, u, v, rows, cols,
                       out, oof);
}

// ---- KI
constexpr int kThreads = 256, kPix = 2, kTile = kThreads * kPix;

// grid (blocks per pair, batch)
template <typename T>
__global__ __launch_bounds__(kThreads) void hs_frame_interp_kernel(
    const T *__restrict__ I0, const T *__restrict__ I1, const float *__restrict__ uf,
    const float *__restrict__ vf, const float *__restrict__ ub, const float *__restrict__ vb,
    const uint8_t *__restrict__ mask_f, const uint8_t *__restrict__ mask_b, int rows, int cols,
    InterpTimes times, int nt, void *__restrict__ out, int out_u8, uint8_t *__restrict__ flags,
    uint32_t *__restrict__ trusted) {
    __shared__ uint32_t block_trusted[kInterpMaxTimes];
    const int plane = rows * cols;  // <= 2^29 - 1
    const size_t base = (size_t)blockIdx.y * plane;
    const int ntiles = (plane + kTile - 1) / kTile;
    const float inv_cols = 1.0f / (float)cols;
    const T *p0 = I0 + base, *p1 = I1 + base;
    const uint8_t *mf = mask_f ? mask_f + base : nullptr;
    const uint8_t *mb = mask_b ? mask_b + base : nullptr;
    const int t = threadIdx.x;
    if (t < kInterpMaxTimes) block_trusted[t] = 0;
    __syncthreads();

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int pk[kPix], x[kPix], y[kPix];
        float fu[kPix], fv[kPix], bu[kPix], bv[kPix];
#pragma unroll
        for (int k = 0; k < kPix; ++k) {
            pk[k] = tile * kTile + k * kThreads + t;
            // every lane computes (a pixel past the plane on its last one):
            // the quad exchange needs all lanes active
            const int p = min(pk[k], plane - 1);
            // y = p / cols from the f32 quotient, off by at most one: its
            // relative error is 3 ulp and y < 2^18 rows (kMaxRows)
            int yy = (int)((float)p * inv_cols);
            int xx = p - yy * cols;
            if (xx < 0) xx += cols, --yy;
            else if (xx >= cols) xx -= cols, ++yy;
            x[k] = xx, y[k] = yy;
            fu[k] = uf[base + p], fv[k] = vf[base + p];
            bu[k] = ub[base + p], bv[k] = vb[base + p];
        }
        for (int ti = 0; ti < nt; ++ti) {
            const float tt = times.t[ti];
            const float s = 1.0f - tt, a = s * tt, b = tt * tt, c = s * s;
            const size_t obase = ((size_t)blockIdx.y * nt + ti) * plane;
            uint32_t good = 0;
#pragma unroll
            for (int k = 0; k < kPix; ++k) {
                const bool valid = pk[k] < plane;
                const float u0 = b * bu[k] - a * fu[k], v0 = b * bv[k] - a * fv[k];
                const float u1 = c * fu[k] - a * bu[k], v1 = c * fv[k] - a * bv[k];
                bool in0, in1;
                int n0, n1;
                const float s0 = sample(p0, rows, cols, x[k], y[k], u0, v0, in0, n0);
                const float s1 = sample(p1, rows, cols, x[k], y[k], u1, v1, in1, n1);
                const float wt = blend_weight(in0, in1, tt);
                const float o = blend(wt, s0, s1);
                uint32_t fl = (in0 ? 0u : 1u) | (in1 ? 0u : 2u);
                if (mf) fl |= mf[n0] != 0 ? 4u : 0u;  // uniform
                if (mb) fl |= mb[n1] != 0 ? 8u : 0u;  // uniform
                good += valid && fl == 0u;
                const int q0 = pk[k] - (t & 3);  // the quad's first pixel
                if (out_u8) {                    // uniform
                    store_quad_u8((uint8_t *)out + obase, pk[k], q0, plane, valid, round_u8(o), t);
                } else if (valid) {
                    ((float *)out)[obase + pk[k]] = o;
                }
                if (flags)  // uniform
                    store_quad_u8(flags + obase, pk[k], q0, plane, valid, fl, t);
            }
            if (trusted) {  // uniform: butterfly sum, one LDS atomic per wave
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) good += __shfl_xor(good, off, 64);
                if ((t & 63) == 0 && good) atomicAdd(&block_trusted[ti], good);
            }
        }
    }
    if (!trusted) return;  // uniform over the grid
    __syncthreads();
    // per block: one ordinary global atomic per time with trusted pixels
    if (t < nt && block_trusted[t])
        atomicAdd(trusted + (size_t)blockIdx.y * nt + t, block_trusted[t]);
}

template <typename T>
void launch_interp_t(const void *I0, const void *I1, const float *uf, const float *vf,
                     const float *ub, const float *vb, const uint8_t *mask_f,
                     const uint8_t *mask_b, int rows, int cols, int batch, const InterpTimes &times,
                     int nt, void *out, int out_u8, uint8_t *flags, uint32_t *trusted,
                     hipStream_t s) {
    const size_t plane = (size_t)rows * cols;
    const int ntiles = (int)((plane + kTile - 1) / kTile);
    // six blocks of four waves are resident per CU (64 to 68 VGPRs: 7 waves
    // per SIMD; the cap predates that count); more blocks would wait for a slot and
    // only add atomics on the counts, which share a cache line
    const int cap = std::max(1, (6 * device_cus() + batch - 1) / batch);
    dim3 blk(kThreads, 1, 1), grd(std::min(ntiles, cap), batch, 1);
    hipLaunchKernelGGL(hs_frame_interp_kernel<T>, grd, blk, 0, s, (const T *)I0, (const T *)I1,
                       uf, vf, ub, vb, mask_f, mask_b, rows, cols, times, nt, out, out_u8, flags,
                       trusted);
}

}  // namespace

hipError_t launch_warp_image(const void *I, int dtype_in, int rows, int cols, int batch,
                             const float *u, const float *v, float *out, uint8_t *oof,
                             hipStream_t s) {
    switch (dtype_in) {
    case 0: launch_warp_t<uint8_t>(I, u, v, rows, cols, batch, out, oof, s); break;
    case 1: launch_warp_t<float>(I, u, v, rows, cols, batch, out, oof, s); break;
    case 2: launch_warp_t<double>(I, u, v, rows, cols, batch, out, oof, s); break;
    case 3: launch_warp_t<_Float16>(I, u, v, rows, cols, batch, out, oof, s); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_frame_interp(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                               int batch, const float *uf, const float *vf, const float *ub,
                               const float *vb, const uint8_t *mask_f, const uint8_t *mask_b,
                               const float *times, int nt, void *out, bool out_u8,
                               uint8_t *flags, uint32_t *trusted, hipStream_t s) {
    if (nt < 1 || nt > kInterpMaxTimes) return hipErrorInvalidValue;
    InterpTimes tm{};
    for (int k = 0; k < nt; ++k) tm.t[k] = times[k];
    const int u8 = out_u8 ? 1 : 0;
    switch (dtype_in) {
    case 0:
        launch_interp_t<uint8_t>(I0, I1, uf, vf, ub, vb, mask_f, mask_b, rows, cols, batch, tm, nt,
                                 out, u8, flags, trusted, s);
        break;
    case 1:
        launch_interp_t<float>(I0, I1, uf, vf, ub, vb, mask_f, mask_b, rows, cols, batch, tm, nt,
                               out, u8, flags, trusted, s);
        break;
    case 2:
        launch_interp_t<double>(I0, I1, uf, vf, ub, vb, mask_f, mask_b, rows, cols, batch, tm, nt,
                                out, u8, flags, trusted, s);
        break;
    case 3:
        launch_interp_t<_Float16>(I0, I1, uf, vf, ub, vb, mask_f, mask_b, rows, cols, batch, tm,
                                  nt, out, u8, flags, trusted, s);
        break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace hsflow
