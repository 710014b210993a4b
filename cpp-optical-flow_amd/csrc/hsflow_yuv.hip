// hsflow_yuv.hip -- the chroma of the frame between two YUV 4:2:0 frames
// ("YUV 4:2:0 frame interpolation").  The luma plane of such a frame
// is the grey frame the solver wants and goes through the grey calls as it is;
// this is what remains.
//
//  KIY hs_chroma_interp_kernel   per chroma sample (y, x) of the rc x cc grid
//     (rc = rows / 2, cc = cols / 2, rows and cols the luma's, both even), from
//     the four full-resolution flows of the bidirectional solve:
//       f' = ((f[2y][2x] + f[2y][2x+1]) + (f[2y+1][2x] + f[2y+1][2x+1])) * 0.125f
//     for f in uf, vf, ub, vb: KD's expression, the 2 x 2 block's mean flow in
//     chroma pixels; then KI's body (hsflow_sampler.h) on the chroma grid with
//     those flows, for the U and for the V sample: times, displacement clamp,
//     taps, rim test, wt, blend and round_u8 are KI's, computed once for both
//     channels.  So the result is, bit for bit, hsflow_downflow_device on
//     (uf, vf) and (ub, vb) followed by hsflow_frame_interp_device (u8 frames,
//     NULL masks) on the U planes and on the V planes -- six launches, and for
//     NV12 the de-interleaving and interleaving around them -- without the four
//     half-resolution flow planes ever reaching memory.  No flags and no
//     trusted count: the luma's are the frame's.
//     With counts (KC's, of the luma solve) a pair whose consistent pixels
//     number fewer than min_consistent gets KF's value instead, per chroma
//     byte: the verdict is formed per block from the two counts, as KF forms
//     it, so KIY depends neither on KF's cut nor on the order of the two.
//
// Traffic: 16 B per luma pixel of flows once (64 B per chroma sample) and, per
// time, 4 B of chroma read (the taps of neighbouring samples overlap) and 2 or
// 8 B written per sample; at one time the flows bound the kernel, every further
// time costs the sampler's arithmetic and its sixteen byte loads per sample
// (DESIGN.md has the figures).  KI's map on the chroma plane: a block of 256
// threads takes tiles of 512 consecutive samples, thread t the samples t and
// t + 256, the grid capped per CU and striding over the tiles.  A thread reads
// its 2 x 2 block of a flow plane as two 8-byte loads where the plane's base is
// 8-byte aligned (cols is even, so every row start then is), else as four
// 4-byte loads; the same arithmetic either way.  u8 stores go through quads of
// lanes as KI's do.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "hsflow_frame_policy.h"
#include "hsflow_internal.h"
#include "hsflow_sampler.h"

namespace hsflow {
namespace {

using namespace sampler;

constexpr int kNearest = 1;  // HSFLOW_FALLBACK_NEAREST

// KD's value of the 2 x 2 block whose rows start at top and bot (the block's
// first element in each).  No multiply is followed by an add; contraction is
// off all the same, so that the bits do not hang on what surrounds the call.
__device__ __forceinline__ float down_block(const float *__restrict__ top,
                                            const float *__restrict__ bot, bool wide) {
#pragma clang fp contract(off)
    float a, b, c, d;
    if (wide) {  // uniform
        const float2 t = *reinterpret_cast<const float2 *>(top);
        const float2 w = *reinterpret_cast<const float2 *>(bot);
        a = t.x, b = t.y, c = w.x, d = w.y;
    } else {
        a = top[0], b = top[1], c = bot[0], d = bot[1];
    }
    return ((a + b) + (c + d)) * 0.125f;
}

// KF's value (hsflow_fallback.hip): the multiply-add spelled out
__device__ __forceinline__ float fallback_value(int mode, float tt, float a, float c) {
#pragma clang fp contract(off)
    if (mode == kNearest) return tt < 0.5f ? a : c;
    return tt == 0.0f ? a : (tt == 1.0f ? c : __builtin_fmaf(1.0f - tt, a, tt * c));
}

template <typename Frame>
__device__ __forceinline__ void store_sample(void *__restrict__ out, int out_u8, size_t frame,
                                             int plane, int pk, int t, const Uv &o) {
    const bool valid = pk < plane;
    const int q0 = pk - (t & 3);  // the quad's first sample, >= 0
    const bool whole = q0 + 3 < plane;
    if (out_u8) {  // uniform
        Frame::store_u8(out, frame, plane, pk, q0, whole, valid, o, t);
    } else if (valid) {
        Frame::store_f32(out, frame, plane, pk, o);
    }
}

// grid (blocks per pair, batch); rows, cols: the luma's
template <typename Frame>
__global__ __launch_bounds__(kInterpThreads) void hs_chroma_interp_kernel(
    const uint8_t *__restrict__ C0, const uint8_t *__restrict__ C1, const float *__restrict__ uf,
    const float *__restrict__ vf, const float *__restrict__ ub, const float *__restrict__ vb,
    const uint32_t *__restrict__ counts_f, const uint32_t *__restrict__ counts_b,
    uint64_t min_consistent, int mode, int rows, int cols, InterpTimes times, int nt,
    void *__restrict__ out, int out_u8) {
    constexpr int kThreads = kInterpThreads, kPix = kInterpPix, kTile = kInterpTile;
    const int rc = rows >> 1, cc = cols >> 1;
    const int plane = rc * cc;  // <= 2^27
    const int pair = blockIdx.y, t = threadIdx.x;
    const int ntiles = (plane + kTile - 1) / kTile;
    const uint8_t *p0 = C0 + (size_t)pair * 2 * plane, *p1 = C1 + (size_t)pair * 2 * plane;

    // block-uniform, as KF: element 0 of a pair's three counts is HSFLOW_CONSISTENT
    if (counts_f &&
        (uint64_t)counts_f[(size_t)pair * 3] + counts_b[(size_t)pair * 3] < min_consistent) {
        for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
            int pk[kPix];
            Uv a[kPix], c[kPix];
#pragma unroll
            for (int k = 0; k < kPix; ++k) {
                pk[k] = tile * kTile + k * kThreads + t;
                // every lane computes: the quad exchange needs all lanes active
                const int p = min(pk[k], plane - 1);
                a[k] = Frame::at(p0, plane, p), c[k] = Frame::at(p1, plane, p);
            }
            for (int ti = 0; ti < nt; ++ti) {
                const float tt = times.t[ti];
#pragma unroll
                for (int k = 0; k < kPix; ++k) {
                    const Uv o{{fallback_value(mode, tt, a[k].c[0], c[k].c[0]),
                                fallback_value(mode, tt, a[k].c[1], c[k].c[1])}};
                    store_sample<Frame>(out, out_u8, (size_t)pair * nt + ti, plane, pk[k], t, o);
                }
            }
        }
        return;
    }

    const size_t lbase = (size_t)pair * rows * cols;  // rows * cols <= 2^29 - 4
    const float *flow[4] = {uf + lbase, vf + lbase, ub + lbase, vb + lbase};
    bool wide[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) wide[f] = ((uintptr_t)flow[f] & 7) == 0;
    const float inv_cc = 1.0f / (float)cc;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int pk[kPix], x[kPix], y[kPix];
        float fl[kPix][4];  // uf', vf', ub', vb' of the sample
#pragma unroll
        for (int k = 0; k < kPix; ++k) {
            pk[k] = tile * kTile + k * kThreads + t;
            const int p = min(pk[k], plane - 1);
            const XY q = pixel_xy(p, cc, inv_cc);
            x[k] = q.x, y[k] = q.y;
            const int top = 2 * q.y * cols + 2 * q.x;  // < rows * cols
#pragma unroll
            for (int f = 0; f < 4; ++f)
                fl[k][f] = down_block(flow[f] + top, flow[f] + top + cols, wide[f]);
        }
        for (int ti = 0; ti < nt; ++ti) {
            const float tt = times.t[ti];
            const float s = 1.0f - tt, a = s * tt, b = tt * tt, c = s * s;
#pragma unroll
            for (int k = 0; k < kPix; ++k) {
                const float fu = fl[k][0], fv = fl[k][1], bu = fl[k][2], bv = fl[k][3];
                // KI's text from here on
                const float u0 = b * bu - a * fu, v0 = b * bv - a * fv;
                const float u1 = c * fu - a * bu, v1 = c * fv - a * bv;
                bool in0, in1;
                int n0, n1;
                const Taps t0 = sample_taps(rc, cc, x[k], y[k], u0, v0, in0, n0);
                const Uv s0 = Frame::sample(p0, plane, cc, t0);
                const Taps t1 = sample_taps(rc, cc, x[k], y[k], u1, v1, in1, n1);
                const Uv s1 = Frame::sample(p1, plane, cc, t1);
                const float wt = blend_weight(in0, in1, tt);
                const Uv o{{blend(wt, s0.c[0], s1.c[0]), blend(wt, s0.c[1], s1.c[1])}};
                store_sample<Frame>(out, out_u8, (size_t)pair * nt + ti, plane, pk[k], t, o);
            }
        }
    }
}

int g_nv12_wide = 0;

// `times` is read here, on the host; KI's grid on the chroma plane
template <typename Frame>
hipError_t launch_as(const uint8_t *c0, const uint8_t *c1, int rows, int cols, int batch,
                     const float *uf, const float *vf, const float *ub, const float *vb,
                     const uint32_t *counts_f, const uint32_t *counts_b, uint64_t min_consistent,
                     int mode, const float *times, int nt, void *out, bool out_u8, hipStream_t s) {
    InterpTimes tm{};
    for (int k = 0; k < nt; ++k) tm.t[k] = times[k];
    const size_t plane = (size_t)(rows / 2) * (cols / 2);
    const int ntiles = (int)((plane + kInterpTile - 1) / kInterpTile);
    const int cap = std::max(1, (Frame::kBlocksPerCu * device_cus() + batch - 1) / batch);
    dim3 blk(kInterpThreads, 1, 1), grd(std::min(ntiles, cap), batch, 1);
    hipLaunchKernelGGL(hs_chroma_interp_kernel<Frame>, grd, blk, 0, s, c0, c1, uf, vf, ub, vb,
                       counts_f, counts_b, min_consistent, mode, rows, cols, tm, nt, out,
                       out_u8 ? 1 : 0);
    return hipGetLastError();
}

}  // namespace

int chroma_blocks_per_cu() { return ChromaFrame<kYuvI420, false>::kBlocksPerCu; }

int set_chroma_nv12_wide_loads(int on) {
    const int prev = g_nv12_wide;
    g_nv12_wide = on ? 1 : 0;
    return prev;
}

hipError_t launch_chroma_interp(const uint8_t *c0, const uint8_t *c1, int layout, int rows,
                                int cols, int batch, const float *uf, const float *vf,
                                const float *ub, const float *vb, const uint32_t *counts_f,
                                const uint32_t *counts_b, uint64_t min_consistent, int mode,
                                const float *times, int nt, void *out, bool out_u8,
                                hipStream_t s) {
    if (nt < 1 || nt > kInterpMaxTimes || rows < 2 || cols < 2 || (rows | cols) & 1)
        return hipErrorInvalidValue;
    const auto go = [&](auto frame) {
        return launch_as<decltype(frame)>(c0, c1, rows, cols, batch, uf, vf, ub, vb, counts_f,
                                          counts_b, min_consistent, mode, times, nt, out, out_u8,
                                          s);
    };
    if (layout == kYuvI420) return go(ChromaFrame<kYuvI420, false>{});
    if (layout != kYuvNv12) return hipErrorInvalidValue;
    return g_nv12_wide ? go(ChromaFrame<kYuvNv12, true>{}) : go(ChromaFrame<kYuvNv12, false>{});
}

}  // namespace hsflow
