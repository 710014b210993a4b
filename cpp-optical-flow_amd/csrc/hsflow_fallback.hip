// hsflow_fallback.hip -- what becomes of a pair whose flows fail the
// forward-backward check ("Fallback for a failed pair"): a scene
// cut, a motion beyond the pyramid's reach.
//
//  KF hs_frame_fallback_kernel   per pair b, from KC's counts both ways:
//       cut = (u64)counts_f[b][CONSISTENT] + counts_b[b][CONSISTENT] < m
//     m = hsflow_fallback_min_consistent(rows, cols, min_share), an integer made
//     on the host.  A pair that passes is left alone: its blocks read the two
//     counts (block-uniform), block 0 writes cut[b] = 0, and all return.  For a
//     pair that fails, at every time t of the launch and every pixel, with a, c
//     the pixel of I0 and of I1 as KI reads it at zero flow (the element as f32;
//     an f64 element rounded once):
//       NEAREST  out = t < 0.5f ? a : c
//       BLEND    out = a at t = 0, c at t = 1, else fma(1 - t, a, t c) with t c
//                rounded on its own: KI's blend at wt = t as it is compiled (the
//                compiler contracts its (1 - wt) s0 + wt s1 to that
//                multiply-add).  Here it is spelled out, with contraction
//                off, so that KF's bits do not hang on a compiler's choice.
//     a u8 output through KI's round_u8 (u16: round_u16), flags = 32 (HSFLOW_INTERP_FALLBACK)
//     replacing what was there, trusted[b][t] = 0, cut[b] = 1.
//
// One launch serves all times and the whole batch.  The map is KI's (256
// threads, tiles of 512 consecutive pixels of a pair's plane, thread t the
// pixels t and t + 256, the grid capped per CU and striding over the tiles), and
// so are the stores, through the frame policies KI is written over: an aligned
// quad of u8 pixels leaves as whole dwords from the lanes that collected them
// over DPP, every other pixel as single bytes -- the same bits at any
// alignment.  HBM-bound where it works at all: per pixel two elements read once
// and, per time, one pixel and one flag byte written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "hsflow_frame_policy.h"
#include "hsflow_internal.h"

namespace hsflow {
namespace {

constexpr uint32_t kInterpFallback = 32;  // HSFLOW_INTERP_FALLBACK
constexpr int kNearest = 1;               // HSFLOW_FALLBACK_NEAREST

// pixel p of a pair's frame as KI's sampler returns it at zero flow
template <typename Frame>
__device__ __forceinline__ typename Frame::Px pixel_at(
    const typename Frame::Elem *__restrict__ img, size_t p) {
    if constexpr (Frame::kChannels == 1) {
        return (float)img[p];
    } else {
        typename Frame::Px r;
#pragma unroll
        for (int ch = 0; ch < Frame::kChannels; ++ch)
            r.c[ch] = (float)img[p * Frame::kChannels + ch];
        return r;
    }
}

#pragma clang fp contract(off)
__device__ __forceinline__ float fallback_value(int mode, float tt, float a, float c) {
    if (mode == kNearest) return tt < 0.5f ? a : c;
    // selects, never multiplies by zero, as KI's blend
    return tt == 0.0f ? a : (tt == 1.0f ? c : __builtin_fmaf(1.0f - tt, a, tt * c));
}

// grid (blocks per pair, batch)
template <typename Frame>
__global__ __launch_bounds__(kInterpThreads) void hs_frame_fallback_kernel(
    const typename Frame::Elem *__restrict__ I0, const typename Frame::Elem *__restrict__ I1,
    const uint32_t *__restrict__ counts_f, const uint32_t *__restrict__ counts_b,
    uint64_t min_consistent, int mode, int plane, InterpTimes times, int nt,
    void *__restrict__ out, int out_kind, uint8_t *__restrict__ flags,
    uint32_t *__restrict__ trusted, uint8_t *__restrict__ cut) {
    constexpr int kThreads = kInterpThreads, kPix = kInterpPix, kTile = kInterpTile;
    constexpr int kCh = Frame::kChannels;
    const int pair = blockIdx.y, t = threadIdx.x;
    // block-uniform: element 0 of a pair's three counts is HSFLOW_CONSISTENT
    const uint64_t good = (uint64_t)counts_f[(size_t)pair * 3] + counts_b[(size_t)pair * 3];
    const bool failed = good < min_consistent;
    if (blockIdx.x == 0 && t == 0 && cut) cut[pair] = failed ? 1 : 0;
    if (!failed) return;
    if (blockIdx.x == 0 && t < nt && trusted) trusted[(size_t)pair * nt + t] = 0;

    const size_t base = (size_t)pair * plane;  // plane <= 2^29 - 4
    const int ntiles = (plane + kTile - 1) / kTile;
    const typename Frame::Elem *p0 = I0 + base * kCh, *p1 = I1 + base * kCh;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int pk[kPix];
        typename Frame::Px a[kPix], c[kPix];
#pragma unroll
        for (int k = 0; k < kPix; ++k) {
            pk[k] = tile * kTile + k * kThreads + t;
            // every lane computes (a pixel past the plane on its last one):
            // the quad exchange needs all lanes active
            const size_t p = (size_t)min(pk[k], plane - 1);
            a[k] = pixel_at<Frame>(p0, p), c[k] = pixel_at<Frame>(p1, p);
        }
        for (int ti = 0; ti < nt; ++ti) {
            const float tt = times.t[ti];
            const size_t obase = ((size_t)pair * nt + ti) * plane;
#pragma unroll
            for (int k = 0; k < kPix; ++k) {
                const bool valid = pk[k] < plane;
                typename Frame::Px o;
                if constexpr (kCh == 1) {
                    o = fallback_value(mode, tt, a[k], c[k]);
                } else {
#pragma unroll
                    for (int ch = 0; ch < kCh; ++ch)
                        o.c[ch] = fallback_value(mode, tt, a[k].c[ch], c[k].c[ch]);
                }
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
                    store_quad_u8(flags + obase, pk[k], q0, whole, valid, kInterpFallback, t);
            }
        }
    }
}

// `times` is read here, on the host; the grid is KI's
template <typename Frame>
hipError_t launch_frame_fallback_as(const void *I0, const void *I1, int rows, int cols, int batch,
                                    const uint32_t *counts_f, const uint32_t *counts_b,
                                    uint64_t min_consistent, int mode, const float *times, int nt,
                                    void *out, int out_kind, uint8_t *flags, uint32_t *trusted,
                                    uint8_t *cut, hipStream_t s) {
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
    hipLaunchKernelGGL(hs_frame_fallback_kernel<Frame>, grd, blk, 0, s, (const Elem *)I0,
                       (const Elem *)I1, counts_f, counts_b, min_consistent, mode, (int)plane, tm,
                       nt, out, out_kind, flags, trusted, cut);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_frame_fallback(const void *I0, const void *I1, int dtype_in, int rows, int cols,
                                 int batch, const uint32_t *counts_f, const uint32_t *counts_b,
                                 uint64_t min_consistent, int mode, const float *times, int nt,
                                 void *out, int out_kind, uint8_t *flags, uint32_t *trusted,
                                 uint8_t *cut, hipStream_t s) {
    hipError_t e = hipErrorInvalidValue;  // stays for an unknown dtype
    dispatch_frame_type(dtype_in, [&](auto t) {
        e = launch_frame_fallback_as<GreyFrame<decltype(t)>>(I0, I1, rows, cols, batch, counts_f,
                                                             counts_b, min_consistent, mode, times,
                                                             nt, out, out_kind, flags, trusted,
                                                             cut, s);
    });
    return e;
}

hipError_t launch_frame_fallback_bgr(const uint8_t *I0, const uint8_t *I1, int rows, int cols,
                                     int batch, const uint32_t *counts_f,
                                     const uint32_t *counts_b, uint64_t min_consistent, int mode,
                                     const float *times, int nt, void *out, bool out_u8,
                                     uint8_t *flags, uint32_t *trusted, uint8_t *cut,
                                     hipStream_t s) {
    // KF samples nothing: the tap loads' form does not reach it
    return launch_frame_fallback_as<BgrFrame<false>>(I0, I1, rows, cols, batch, counts_f, counts_b,
                                                     min_consistent, mode, times, nt, out, out_u8,
                                                     flags, trusted, cut, s);
}

}  // namespace hsflow
