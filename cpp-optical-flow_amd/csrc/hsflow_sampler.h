// hsflow_sampler.h -- the one text of sampling a plane at (y + 8 v, x + 8 u),
// for the seven kernels that do it: KW (hsflow_warp.hip), KC
// (hsflow_consistency.hip), KR / KI (hsflow_interp.hip), their colour forms
// KRC / KIC (hsflow_interp_bgr.hip) and KP (hsflow_temporal.hip), which samples
// a flow by itself.  The displacement split, the tap
// positions, the three lerps and the frame test; a tile's pixel -> (x, y); the
// quad store of a u8 plane; and the frame interpolation itself, KI's blend,
// rounding, times and kernel over a frame policy.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "hsflow_frame_types.h"
#include "hsflow_internal.h"

namespace hsflow {
namespace sampler {

// d (pixels) along an axis of length n is clamped to [-n, n] while still a
// float, so NaN (-> -n), +-inf and huge flows never reach the float -> int
// conversion and every tap index stays in the plane.  Returns floor(d); frac =
// d - floor(d), exact in f32; the clamped d comes back for the frame test.
__device__ __forceinline__ int split_disp(float &d, int n, float &frac) {
    d = fminf(fmaxf(d, -(float)n), (float)n);
    const float fl = floorf(d);
    frac = d - fl;
    return (int)fl;
}

// Where a sample at (y + 8 v, x + 8 u) of a rows x cols plane reads: the four
// taps (xa, xb) x (ya, yb), clamped to the plane (xb is xa or xa + 1, yb is ya
// or ya + 1), and the two fractions.  8 is the gain of the reference's
// unnormalised Sobel: one unit of (u, v) is 8 px.
struct Taps {
    int xa, xb, ya, yb;
    float fx, fy;
};

// in: the target is within half a pixel of the frame; nearest: index in the
// plane of the source pixel nearest to the target.
__device__ __forceinline__ Taps sample_taps(int rows, int cols, int x, int y, float u, float v,
                                            bool &in, int &nearest) {
    Taps t;
    float dx = 8.0f * u, dy = 8.0f * v;
    const int ix = split_disp(dx, cols, t.fx);
    const int iy = split_disp(dy, rows, t.fy);
    // |ix| <= cols, |iy| <= rows: the sums cannot overflow
    t.xa = clampi(x + ix, cols), t.xb = clampi(x + ix + 1, cols);
    t.ya = clampi(y + iy, rows), t.yb = clampi(y + iy + 1, rows);
    const float tx = (float)x + dx, ty = (float)y + dy;
    in = tx >= -0.5f && tx <= (float)cols - 0.5f && ty >= -0.5f && ty <= (float)rows - 0.5f;
    nearest = (t.fy >= 0.5f ? t.yb : t.ya) * cols + (t.fx >= 0.5f ? t.xb : t.xa);  // < 2^29
    return t;
}

// top row, bottom row, then vertical; exact at fx = fy = 0: zero flow returns
// the pixel itself
template <typename F>
__device__ __forceinline__ F lerp_taps(F ta, F tb, F ba, F bb, float fx, float fy) {
    const F t = ta + (F)fx * (tb - ta);
    const F w = ba + (F)fx * (bb - ba);
    return t + (F)fy * (w - t);
}

// img (one pair's plane of T) at the taps `t`, in T's math type
template <typename T>
__device__ __forceinline__ typename FrameMath<T>::type sample_plane(const T *__restrict__ img,
                                                                    int cols, const Taps &t) {
    using F = typename FrameMath<T>::type;
    const T *top = img + (size_t)t.ya * cols;
    const T *bot = img + (size_t)t.yb * cols;
    return lerp_taps<F>((F)top[t.xa], (F)top[t.xb], (F)bot[t.xa], (F)bot[t.xb], t.fx, t.fy);
}

// pixel p of a plane -> (x, y): y = p / cols from the f32 quotient, off by at
// most one (its relative error is 3 ulp and y < 2^18 rows, kMaxRows).  By
// value: through reference parameters KI compiled to 40 more instructions.
struct XY {
    int x, y;
};
__device__ __forceinline__ XY pixel_xy(int p, int cols, float inv_cols) {
    int y = (int)((float)p * inv_cols);
    int x = p - y * cols;
    if (x < 0) x += cols, --y;
    else if (x >= cols) x -= cols, ++y;
    return {x, y};
}

// value of lane `Q` of the caller's quad (DPP quad_perm broadcast)
template <int Q>
__device__ __forceinline__ uint32_t quad_lane(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, Q * 0x55, 0xf, 0xf, true);
}

// One byte per lane into a u8 plane at dst + pk (pk: the lane's pixel, q0 its
// quad's first, whole: the quad's four pixels lie in the plane): an aligned
// dword per quad where the quad is whole and its address allows, else a byte
// per valid lane.  Every lane of the wave calls (the exchange needs them all).
__device__ __forceinline__ void store_quad_u8(uint8_t *dst, int pk, int q0, bool whole,
                                              bool valid, uint32_t byte, int lane) {
    const uint32_t quad = byte | quad_lane<1>(byte) << 8 | quad_lane<2>(byte) << 16 |
                          quad_lane<3>(byte) << 24;
    if (whole && (((uintptr_t)dst + (size_t)q0) & 3) == 0) {
        if ((lane & 3) == 0) *reinterpret_cast<uint32_t *>(dst + q0) = quad;
    } else if (valid) {
        dst[pk] = (uint8_t)byte;
    }
}

// value of the other lane of the caller's pair (2j, 2j + 1): quad_perm 1 0 3 2
__device__ __forceinline__ uint32_t pair_lane(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xf, 0xf, true);
}

// One 16-bit sample per lane into a u16 plane at dst + pk (pk: the lane's
// pixel; its parity is the lane's, so the pair holds pk & ~1 and the next): an
// aligned dword per pair where both lie in the plane and the address allows,
// else two bytes per valid lane.  Every lane of the wave calls.
__device__ __forceinline__ void store_pair_u16(uint16_t *dst, int pk, int plane, uint32_t half,
                                               int lane) {
    const uint32_t other = pair_lane(half);
    const int p0 = pk - (lane & 1);  // the pair's first pixel, >= 0
    if (p0 + 1 < plane && ((uintptr_t)(dst + p0) & 3) == 0) {
        if ((lane & 1) == 0) *reinterpret_cast<uint32_t *>(dst + p0) = half | other << 16;
    } else if (pk < plane) {
        dst[pk] = (uint16_t)half;
    }
}

// ---- frame interpolation (KI, KIC)

// the weight of s1: t where both targets are in the frame or neither is
__device__ __forceinline__ float blend_weight(bool in0, bool in1, float tt) {
    return in0 == in1 ? tt : (in0 ? 0.0f : 1.0f);
}

// selects, never multiplies by zero: the bits of s0 at wt = 0, of s1 at wt = 1
__device__ __forceinline__ float blend(float wt, float s0, float s1) {
    return wt == 0.0f ? s0 : (wt == 1.0f ? s1 : (1.0f - wt) * s0 + wt * s1);
}

// floorf(o + 0.5f) clamped to 0..255; NaN -> 0 (fmaxf drops it)
__device__ __forceinline__ uint32_t round_u8(float o) {
    return (uint32_t)fminf(fmaxf(floorf(o + 0.5f), 0.0f), 255.0f);
}

// the same rule with the bound of a 16-bit sample
__device__ __forceinline__ uint32_t round_u16(float o) {
    return (uint32_t)fminf(fmaxf(floorf(o + 0.5f), 0.0f), 65535.0f);
}

// a sampled colour pixel: C channels in f32 (a grey one is a float)
template <int C>
struct Pixel {
    float c[C];
};

// the times of one launch, by value in the kernel arguments
struct InterpTimes {
    float t[kInterpMaxTimes];
};

constexpr int kInterpThreads = 256, kInterpPix = 2, kInterpTile = kInterpThreads * kInterpPix;

// The frame at each of nt times between I0 and I1 (hsflow_interp.hip has the
// arithmetic and the thread map).  Frame says what a pixel is:
//   Elem, kChannels     a frame is [rows][cols][kChannels] of Elem
//   Px                  a sampled pixel: float, or Pixel<kChannels>
//   sample(img, cols, taps) -> Px
//   store_f32(out, px, o)   pixel px of the whole f32 output
//   store_u8(out, obase, pk, q0, whole, valid, o, lane)   into the u8 plane
//       that starts at pixel obase of the whole output; a quad store as
//       store_quad_u8, every lane calls
//   kU16Out, store_u16(out, obase, pk, plane, o, lane)   whether the frame has
//       a u16 output (16-bit grey frames), and the pair store into it as
//       store_pair_u16, every lane calls
//   kBlocksPerCu        the grid's cap
// Proj says where the time-t flow of an output pixel comes from: false (KI,
// KIC) from the four flows at the pixel itself; true (KIP, DESIGN.md "Flow
// projection") from the source pixel that KS's cell [pair][time][pixel] names
// (hsflow_project.hip: dir << 31 | source index in its low 32 bits), the
// flows at the pixel itself only where the cell is empty (all ones), with flag
// bit 16.  Everything behind (u0, v0), (u1, v1) is one text.  The body of both
// kernels below; grid (blocks per pair, batch).
constexpr uint32_t kInterpHole = 16;  // HSFLOW_INTERP_HOLE

template <typename Frame, bool Proj>
__device__ __forceinline__ void frame_interp_body(
    const typename Frame::Elem *__restrict__ I0, const typename Frame::Elem *__restrict__ I1,
    const float *__restrict__ uf, const float *__restrict__ vf, const float *__restrict__ ub,
    const float *__restrict__ vb, const uint8_t *__restrict__ mask_f,
    const uint8_t *__restrict__ mask_b, const uint64_t *__restrict__ cells, int rows, int cols,
    const InterpTimes &times, int nt, void *__restrict__ out, int out_kind,
    uint8_t *__restrict__ flags, uint32_t *__restrict__ trusted) {
    constexpr int kThreads = kInterpThreads, kPix = kInterpPix, kTile = kInterpTile;
    constexpr int kCh = Frame::kChannels;
    __shared__ uint32_t block_trusted[kInterpMaxTimes];
    const int plane = rows * cols;  // <= 2^29 - 4
    const size_t base = (size_t)blockIdx.y * plane;
    const int ntiles = (plane + kTile - 1) / kTile;
    const float inv_cols = 1.0f / (float)cols;
    const typename Frame::Elem *p0 = I0 + base * kCh, *p1 = I1 + base * kCh;
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
            const XY q = pixel_xy(p, cols, inv_cols);
            x[k] = q.x, y[k] = q.y;
            if constexpr (!Proj) {
                fu[k] = uf[base + p], fv[k] = vf[base + p];
                bu[k] = ub[base + p], bv[k] = vb[base + p];
            }
        }
        for (int ti = 0; ti < nt; ++ti) {
            const float tt = times.t[ti];
            const float s = 1.0f - tt, a = s * tt, b = tt * tt, c = s * s;
            const size_t obase = ((size_t)blockIdx.y * nt + ti) * plane;
            uint32_t good = 0;
#pragma unroll
            for (int k = 0; k < kPix; ++k) {
                const bool valid = pk[k] < plane;
                float u0, v0, u1, v1;
                uint32_t fl = 0;
                if constexpr (Proj) {
                    const int p = min(pk[k], plane - 1);
                    const uint64_t cell = cells[obase + p];
                    if (cell == ~0ull) {  // nothing landed here: KI's flow
                        const float hfu = uf[base + p], hfv = vf[base + p];
                        const float hbu = ub[base + p], hbv = vb[base + p];
                        u0 = b * hbu - a * hfu, v0 = b * hbv - a * hfv;
                        u1 = c * hfu - a * hbu, v1 = c * hfv - a * hbv;
                        fl = kInterpHole;
                    } else {
                        // KS wrote an index below `plane`; a foreign cell
                        // plane cannot lead out of the pair's either
                        const size_t src = base + min((uint32_t)cell & 0x7fffffffu,
                                                      (uint32_t)(plane - 1));
                        const bool back = ((uint32_t)cell >> 31) != 0;
                        const float ut = back ? -ub[src] : uf[src];
                        const float vt = back ? -vb[src] : vf[src];
                        u0 = -tt * ut, v0 = -tt * vt;
                        u1 = s * ut, v1 = s * vt;
                    }
                } else {
                    u0 = b * bu[k] - a * fu[k], v0 = b * bv[k] - a * fv[k];
                    u1 = c * fu[k] - a * bu[k], v1 = c * fv[k] - a * bv[k];
                }
                bool in0, in1;
                int n0, n1;
                const Taps t0 = sample_taps(rows, cols, x[k], y[k], u0, v0, in0, n0);
                const typename Frame::Px s0 = Frame::sample(p0, cols, t0);
                const Taps t1 = sample_taps(rows, cols, x[k], y[k], u1, v1, in1, n1);
                const typename Frame::Px s1 = Frame::sample(p1, cols, t1);
                const float wt = blend_weight(in0, in1, tt);
                // Written out for either pixel: with the channel loop in a
                // function of its own KIC compiled to 30 more instructions, and
                // with a grey pixel as a Pixel<1> in this loop KI took 6 to 11
                // more VGPRs (f64 frames lost a wave per SIMD).
                typename Frame::Px o;
                if constexpr (kCh == 1) {
                    o = blend(wt, s0, s1);
                } else {
#pragma unroll
                    for (int ch = 0; ch < kCh; ++ch) o.c[ch] = blend(wt, s0.c[ch], s1.c[ch]);
                }
                fl |= (in0 ? 0u : 1u) | (in1 ? 0u : 2u);
                if (mf) fl |= mf[n0] != 0 ? 4u : 0u;  // uniform
                if (mb) fl |= mb[n1] != 0 ? 8u : 0u;  // uniform
                good += valid && fl == 0u;
                const int q0 = pk[k] - (t & 3);  // the quad's first pixel, >= 0
                const bool whole = q0 + 3 < plane;
                if (out_kind == kOutU8) {  // uniform
                    Frame::store_u8(out, obase, pk[k], q0, whole, valid, o, t);
                } else if (Frame::kU16Out && out_kind == kOutU16) {  // uniform
                    if constexpr (Frame::kU16Out) Frame::store_u16(out, obase, pk[k], plane, o, t);
                } else if (valid) {
                    Frame::store_f32(out, obase + pk[k], o);
                }
                if (flags)  // uniform
                    store_quad_u8(flags + obase, pk[k], q0, whole, valid, fl, t);
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

// KI / KIC
template <typename Frame>
__global__ __launch_bounds__(kInterpThreads) void hs_frame_interp_kernel(
    const typename Frame::Elem *__restrict__ I0, const typename Frame::Elem *__restrict__ I1,
    const float *__restrict__ uf, const float *__restrict__ vf, const float *__restrict__ ub,
    const float *__restrict__ vb, const uint8_t *__restrict__ mask_f,
    const uint8_t *__restrict__ mask_b, int rows, int cols, InterpTimes times, int nt,
    void *__restrict__ out, int out_kind, uint8_t *__restrict__ flags,
    uint32_t *__restrict__ trusted) {
    frame_interp_body<Frame, false>(I0, I1, uf, vf, ub, vb, mask_f, mask_b, nullptr, rows, cols,
                                    times, nt, out, out_kind, flags, trusted);
}

// KIP: the same over KS's cells [batch][nt][rows][cols]
template <typename Frame>
__global__ __launch_bounds__(kInterpThreads) void hs_frame_interp_proj_kernel(
    const typename Frame::Elem *__restrict__ I0, const typename Frame::Elem *__restrict__ I1,
    const float *__restrict__ uf, const float *__restrict__ vf, const float *__restrict__ ub,
    const float *__restrict__ vb, const uint8_t *__restrict__ mask_f,
    const uint8_t *__restrict__ mask_b, const uint64_t *__restrict__ cells, int rows, int cols,
    InterpTimes times, int nt, void *__restrict__ out, int out_kind,
    uint8_t *__restrict__ flags, uint32_t *__restrict__ trusted) {
    frame_interp_body<Frame, true>(I0, I1, uf, vf, ub, vb, mask_f, mask_b, cells, rows, cols,
                                   times, nt, out, out_kind, flags, trusted);
}

// `times` is read here, on the host.  The grid is capped at what a CU holds
// (Frame::kBlocksPerCu blocks of four waves): more blocks would wait for a
// slot and only add atomics on the counts, which share a cache line.  With
// `cells` the launch is KIP's.  out_kind: kOutF32, kOutU8 or, for a frame that
// has it, kOutU16.
template <typename Frame>
hipError_t launch_frame_interp_as(const void *I0, const void *I1, int rows, int cols, int batch,
                                  const float *uf, const float *vf, const float *ub,
                                  const float *vb, const uint8_t *mask_f, const uint8_t *mask_b,
                                  const float *times, int nt, void *out, int out_kind,
                                  uint8_t *flags, uint32_t *trusted, hipStream_t s,
                                  const uint64_t *cells = nullptr) {
    using Elem = typename Frame::Elem;
    if (nt < 1 || nt > kInterpMaxTimes) return hipErrorInvalidValue;
    if (out_kind != kOutF32 && out_kind != kOutU8 && !(Frame::kU16Out && out_kind == kOutU16))
        return hipErrorInvalidValue;
    InterpTimes tm{};
    for (int k = 0; k < nt; ++k) tm.t[k] = times[k];
    const size_t plane = (size_t)rows * cols;
    const int ntiles = (int)((plane + kInterpTile - 1) / kInterpTile);
    const int cap = std::max(1, (Frame::kBlocksPerCu * device_cus() + batch - 1) / batch);
    dim3 blk(kInterpThreads, 1, 1), grd(std::min(ntiles, cap), batch, 1);
    if (cells)
        hipLaunchKernelGGL(hs_frame_interp_proj_kernel<Frame>, grd, blk, 0, s, (const Elem *)I0,
                           (const Elem *)I1, uf, vf, ub, vb, mask_f, mask_b, cells, rows, cols, tm,
                           nt, out, out_kind, flags, trusted);
    else
        hipLaunchKernelGGL(hs_frame_interp_kernel<Frame>, grd, blk, 0, s, (const Elem *)I0,
                           (const Elem *)I1, uf, vf, ub, vb, mask_f, mask_b, rows, cols, tm, nt,
                           out, out_kind, flags, trusted);
    return hipGetLastError();
}

}  // namespace sampler
}  // namespace hsflow
