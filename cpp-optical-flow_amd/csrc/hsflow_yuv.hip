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
//  KSD hs_cells_down_kernel   KS's cells (hsflow_project.hip) reduced to the
//     chroma grid: cell (yc, xc) of a pair and time is the unsigned 64-bit
//     minimum of the luma cells (2 yc + {0, 1}, 2 xc + {0, 1}).  All ones is the
//     largest word, so a hole loses to every candidate and a chroma cell is a
//     hole only where all four are.  The winner keeps its upper word and its
//     direction bit; its source index p, clamped to rows cols - 1 as KIP clamps
//     a foreign cell, is re-coded to (p / cols >> 1) cc + (p % cols >> 1): the
//     minimum first, the re-coding after it, so ties are the luma's.
//
//  KIYP hs_chroma_interp_proj_kernel   KIY with the time-t flow of a sample
//     read through the luma's winners ("YUV 4:2:0 with projection"):
//     bit for bit KD on both flow pairs, KSD, and hsflow_frame_interp_proj_device
//     (U8 frames, NULL masks, flags and trusted) on the U and on the V planes.
//     Per sample and time the four luma cells are read and reduced in
//     registers -- the chroma cells never reach memory -- and the winner's
//     2 x 2 block of the two flow planes of its direction is gathered with
//     KD's expression, negated behind the mean for direction 1.  Only a hole
//     loads the sample's own four blocks, for KIY's value.  Thread map, stores
//     and fallback verdict are KIY's.
//
//  16-bit samples (ChromaFrame16; yuv420p10le .. p16le, P010 .. P016): the same
//     kernels over a policy whose element is uint16_t.  I420-16 samples the two
//     planes as KI samples a 16-bit grey plane and stores through pairs of
//     lanes; NV12-16 holds a sample's U and V in one dword, so a tap is one
//     (unaligned) dword load and a lane's U16 output one dword store.  A U16
//     output is round_u16 of the f32 value.  8 B read and 4 or 8 B written per
//     sample and time.
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

// out_kind: kOutF32 or the frame's own integer type (the launch has checked)
template <typename Frame>
__device__ __forceinline__ void store_sample(void *__restrict__ out, int out_kind, size_t frame,
                                             int plane, int pk, int t, const Uv &o) {
    const bool valid = pk < plane;
    const int q0 = pk - (t & 3);  // the quad's first sample, >= 0
    const bool whole = q0 + 3 < plane;
    if (out_kind != kOutF32) {  // uniform
        Frame::store_int(out, frame, plane, pk, q0, whole, valid, o, t);
    } else if (valid) {
        Frame::store_f32(out, frame, plane, pk, o);
    }
}

// KF's value for every sample of a failed pair, over KIY's tiles
template <typename Frame>
__device__ __forceinline__ void fallback_tiles(const typename Frame::Elem *__restrict__ p0,
                                               const typename Frame::Elem *__restrict__ p1,
                                               int plane, int pair, int mode,
                                               const InterpTimes &times, int nt,
                                               void *__restrict__ out, int out_kind) {
    constexpr int kThreads = kInterpThreads, kPix = kInterpPix, kTile = kInterpTile;
    const int t = threadIdx.x;
    const int ntiles = (plane + kTile - 1) / kTile;
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
                store_sample<Frame>(out, out_kind, (size_t)pair * nt + ti, plane, pk[k], t, o);
            }
        }
    }
}

// grid (blocks per pair, batch); rows, cols: the luma's
template <typename Frame>
__global__ __launch_bounds__(kInterpThreads) void hs_chroma_interp_kernel(
    const typename Frame::Elem *__restrict__ C0, const typename Frame::Elem *__restrict__ C1,
    const float *__restrict__ uf, const float *__restrict__ vf, const float *__restrict__ ub,
    const float *__restrict__ vb, const uint32_t *__restrict__ counts_f,
    const uint32_t *__restrict__ counts_b, uint64_t min_consistent, int mode, int rows, int cols,
    InterpTimes times, int nt, void *__restrict__ out, int out_kind) {
    constexpr int kThreads = kInterpThreads, kPix = kInterpPix, kTile = kInterpTile;
    const int rc = rows >> 1, cc = cols >> 1;
    const int plane = rc * cc;  // <= 2^27
    const int pair = blockIdx.y, t = threadIdx.x;
    const int ntiles = (plane + kTile - 1) / kTile;
    const typename Frame::Elem *p0 = C0 + (size_t)pair * 2 * plane,
                               *p1 = C1 + (size_t)pair * 2 * plane;

    // block-uniform, as KF: element 0 of a pair's three counts is HSFLOW_CONSISTENT
    if (counts_f &&
        (uint64_t)counts_f[(size_t)pair * 3] + counts_b[(size_t)pair * 3] < min_consistent) {
        fallback_tiles<Frame>(p0, p1, plane, pair, mode, times, nt, out, out_kind);
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
                store_sample<Frame>(out, out_kind, (size_t)pair * nt + ti, plane, pk[k], t, o);
            }
        }
    }
}

// ---- the projected form (KSD, KIYP)
constexpr unsigned long long kHole = ~0ull;

// the 64-bit minimum of the 2 x 2 block of cells whose rows start at top and
// bot: two 16-byte loads where the cell plane's base is 16-byte aligned (cols is
// even, so every block's rows then are), else four 8-byte loads
__device__ __forceinline__ unsigned long long cells_min(
    const unsigned long long *__restrict__ top, const unsigned long long *__restrict__ bot,
    bool wide) {
    unsigned long long a, b, c, d;
    if (wide) {  // uniform
        const ulonglong2 t = *reinterpret_cast<const ulonglong2 *>(top);
        const ulonglong2 w = *reinterpret_cast<const ulonglong2 *>(bot);
        a = t.x, b = t.y, c = w.x, d = w.y;
    } else {
        a = top[0], b = top[1], c = bot[0], d = bot[1];
    }
    const unsigned long long ab = a < b ? a : b, cd = c < d ? c : d;
    return ab < cd ? ab : cd;
}

// the luma pixel a winning cell names: its index clamped to the plane, as KIP
// clamps a foreign cell; pixel_xy stays exact past 2^24
__device__ __forceinline__ XY winner_xy(unsigned long long cell, int lplane, int cols,
                                        float inv_cols) {
    const uint32_t p = min((uint32_t)cell & 0x7fffffffu, (uint32_t)(lplane - 1));
    return pixel_xy((int)p, cols, inv_cols);
}

// KSD; grid (blocks per plane, planes up to the grid's limit, striding);
// rows, cols: the luma's; planes = batch * nt
__global__ __launch_bounds__(256) void hs_cells_down_kernel(
    const unsigned long long *__restrict__ cells, int rows, int cols, int planes,
    unsigned long long *__restrict__ cells_c) {
    const int rc = rows >> 1, cc = cols >> 1;
    const int plane = rc * cc, lplane = rows * cols;
    const float inv_cc = 1.0f / (float)cc, inv_cols = 1.0f / (float)cols;
    for (int pl = blockIdx.y; pl < planes; pl += gridDim.y) {
        const unsigned long long *src = cells + (size_t)pl * lplane;
        unsigned long long *dst = cells_c + (size_t)pl * plane;
        const bool wide = ((uintptr_t)src & 15) == 0;
        for (int p = blockIdx.x * 256 + threadIdx.x; p < plane; p += gridDim.x * 256) {
            const XY q = pixel_xy(p, cc, inv_cc);
            const int top = 2 * q.y * cols + 2 * q.x;  // < rows * cols
            unsigned long long m = cells_min(src + top, src + top + cols, wide);
            if (m != kHole) {
                const XY w = winner_xy(m, lplane, cols, inv_cols);
                m = (m & 0xffffffff80000000ull) | (uint32_t)((w.y >> 1) * cc + (w.x >> 1));
            }
            dst[p] = m;
        }
    }
}

// KIYP; grid (blocks per pair, batch); rows, cols: the luma's; cells: KS's
// [batch][nt][rows][cols]
template <typename Frame>
__global__ __launch_bounds__(kInterpThreads) void hs_chroma_interp_proj_kernel(
    const typename Frame::Elem *__restrict__ C0, const typename Frame::Elem *__restrict__ C1,
    const float *__restrict__ uf, const float *__restrict__ vf, const float *__restrict__ ub,
    const float *__restrict__ vb, const unsigned long long *__restrict__ cells,
    const uint32_t *__restrict__ counts_f, const uint32_t *__restrict__ counts_b,
    uint64_t min_consistent, int mode, int rows, int cols, InterpTimes times, int nt,
    void *__restrict__ out, int out_kind) {
    constexpr int kThreads = kInterpThreads, kPix = kInterpPix, kTile = kInterpTile;
    const int rc = rows >> 1, cc = cols >> 1;
    const int plane = rc * cc;  // <= 2^27
    const int lplane = rows * cols;  // <= 2^29 - 4
    const int pair = blockIdx.y, t = threadIdx.x;
    const int ntiles = (plane + kTile - 1) / kTile;
    const typename Frame::Elem *p0 = C0 + (size_t)pair * 2 * plane,
                               *p1 = C1 + (size_t)pair * 2 * plane;

    // block-uniform, as KF: element 0 of a pair's three counts is HSFLOW_CONSISTENT
    if (counts_f &&
        (uint64_t)counts_f[(size_t)pair * 3] + counts_b[(size_t)pair * 3] < min_consistent) {
        fallback_tiles<Frame>(p0, p1, plane, pair, mode, times, nt, out, out_kind);
        return;
    }

    const size_t lbase = (size_t)pair * lplane;
    const float *flow[4] = {uf + lbase, vf + lbase, ub + lbase, vb + lbase};
    bool wide[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) wide[f] = ((uintptr_t)flow[f] & 7) == 0;
    const float inv_cc = 1.0f / (float)cc, inv_cols = 1.0f / (float)cols;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int pk[kPix], x[kPix], y[kPix];
#pragma unroll
        for (int k = 0; k < kPix; ++k) {
            pk[k] = tile * kTile + k * kThreads + t;
            const int p = min(pk[k], plane - 1);
            const XY q = pixel_xy(p, cc, inv_cc);
            x[k] = q.x, y[k] = q.y;
        }
        for (int ti = 0; ti < nt; ++ti) {
            const float tt = times.t[ti];
            const float s = 1.0f - tt, a = s * tt, b = tt * tt, c = s * s;
            const unsigned long long *pc = cells + ((size_t)pair * nt + ti) * lplane;
            const bool wide_c = ((uintptr_t)pc & 15) == 0;
#pragma unroll
            for (int k = 0; k < kPix; ++k) {
                const int top = 2 * y[k] * cols + 2 * x[k];  // < rows * cols
                const unsigned long long cell = cells_min(pc + top, pc + top + cols, wide_c);
                float u0, v0, u1, v1;
                if (cell == kHole) {  // all four empty: KIY's flows, KI's formula
                    float fl[4];
#pragma unroll
                    for (int f = 0; f < 4; ++f)
                        fl[f] = down_block(flow[f] + top, flow[f] + top + cols, wide[f]);
                    u0 = b * fl[2] - a * fl[0], v0 = b * fl[3] - a * fl[1];
                    u1 = c * fl[0] - a * fl[2], v1 = c * fl[1] - a * fl[3];
                } else {
                    // KD's mean of the block that holds the winner, in the
                    // winner's direction: KIP's text on the chroma grid
                    const XY w = winner_xy(cell, lplane, cols, inv_cols);
                    const int wtop = (w.y & ~1) * cols + (w.x & ~1);
                    const bool back = ((uint32_t)cell >> 31) != 0;
                    const float *pu = back ? flow[2] : flow[0], *pv = back ? flow[3] : flow[1];
                    const bool wu = back ? wide[2] : wide[0], wv = back ? wide[3] : wide[1];
                    const float mu = down_block(pu + wtop, pu + wtop + cols, wu);
                    const float mv = down_block(pv + wtop, pv + wtop + cols, wv);
                    const float ut = back ? -mu : mu, vt = back ? -mv : mv;
                    u0 = -tt * ut, v0 = -tt * vt;
                    u1 = s * ut, v1 = s * vt;
                }
                // KI's text from here on
                bool in0, in1;
                int n0, n1;
                const Taps t0 = sample_taps(rc, cc, x[k], y[k], u0, v0, in0, n0);
                const Uv s0 = Frame::sample(p0, plane, cc, t0);
                const Taps t1 = sample_taps(rc, cc, x[k], y[k], u1, v1, in1, n1);
                const Uv s1 = Frame::sample(p1, plane, cc, t1);
                const float wt = blend_weight(in0, in1, tt);
                const Uv o{{blend(wt, s0.c[0], s1.c[0]), blend(wt, s0.c[1], s1.c[1])}};
                store_sample<Frame>(out, out_kind, (size_t)pair * nt + ti, plane, pk[k], t, o);
            }
        }
    }
}

int g_nv12_wide = 0;

// `times` is read here, on the host; KI's grid on the chroma plane.  With
// `cells` the launch is KIYP's.
template <typename Frame>
hipError_t launch_as(const void *c0v, const void *c1v, int rows, int cols, int batch,
                     const float *uf, const float *vf, const float *ub, const float *vb,
                     const uint32_t *counts_f, const uint32_t *counts_b, uint64_t min_consistent,
                     int mode, const float *times, int nt, void *out, int out_kind, hipStream_t s,
                     const uint64_t *cells = nullptr) {
    using Elem = typename Frame::Elem;
    if (out_kind != kOutF32 && out_kind != Frame::kIntOut) return hipErrorInvalidValue;
    const Elem *c0 = (const Elem *)c0v, *c1 = (const Elem *)c1v;
    InterpTimes tm{};
    for (int k = 0; k < nt; ++k) tm.t[k] = times[k];
    const size_t plane = (size_t)(rows / 2) * (cols / 2);
    const int ntiles = (int)((plane + kInterpTile - 1) / kInterpTile);
    const int per_cu = cells ? Frame::kProjBlocksPerCu : Frame::kBlocksPerCu;
    const int cap = std::max(1, (per_cu * device_cus() + batch - 1) / batch);
    dim3 blk(kInterpThreads, 1, 1), grd(std::min(ntiles, cap), batch, 1);
    if (cells)
        hipLaunchKernelGGL(hs_chroma_interp_proj_kernel<Frame>, grd, blk, 0, s, c0, c1, uf, vf, ub,
                           vb, (const unsigned long long *)cells, counts_f, counts_b,
                           min_consistent, mode, rows, cols, tm, nt, out, out_kind);
    else
        hipLaunchKernelGGL(hs_chroma_interp_kernel<Frame>, grd, blk, 0, s, c0, c1, uf, vf, ub, vb,
                           counts_f, counts_b, min_consistent, mode, rows, cols, tm, nt, out,
                           out_kind);
    return hipGetLastError();
}

}  // namespace

int chroma_blocks_per_cu() { return ChromaFrame<kYuvI420, false>::kBlocksPerCu; }

int chroma_proj_blocks_per_cu() { return ChromaFrame<kYuvI420, false>::kProjBlocksPerCu; }

hipError_t launch_cells_down(const uint64_t *cells, int rows, int cols, int planes,
                             uint64_t *cells_c, hipStream_t s) {
    if (planes < 1 || rows < 2 || cols < 2 || (rows | cols) & 1) return hipErrorInvalidValue;
    const size_t plane = (size_t)(rows / 2) * (cols / 2);
    // eight blocks of four waves fill a CU; more only queue
    const int cap = std::max(1, (8 * device_cus() + planes - 1) / planes);
    const int nblk = (int)((plane + 255) / 256);
    dim3 blk(256, 1, 1), grd(std::min(nblk, cap), std::min(planes, 65535), 1);
    hipLaunchKernelGGL(hs_cells_down_kernel, grd, blk, 0, s, (const unsigned long long *)cells,
                       rows, cols, planes, (unsigned long long *)cells_c);
    return hipGetLastError();
}

int set_chroma_nv12_wide_loads(int on) {
    const int prev = g_nv12_wide;
    g_nv12_wide = on ? 1 : 0;
    return prev;
}

hipError_t launch_chroma_interp(const void *c0, const void *c1, int dtype_in, int layout,
                                int rows, int cols, int batch, const float *uf, const float *vf,
                                const float *ub, const float *vb, const uint32_t *counts_f,
                                const uint32_t *counts_b, uint64_t min_consistent, int mode,
                                const float *times, int nt, void *out, int out_kind,
                                hipStream_t s, const uint64_t *cells) {
    if (nt < 1 || nt > kInterpMaxTimes || rows < 2 || cols < 2 || (rows | cols) & 1)
        return hipErrorInvalidValue;
    if (dtype_in != 0 && dtype_in != 4) return hipErrorInvalidValue;  // HSFLOW_U8, HSFLOW_U16
    const auto go = [&](auto frame) {
        return launch_as<decltype(frame)>(c0, c1, rows, cols, batch, uf, vf, ub, vb, counts_f,
                                          counts_b, min_consistent, mode, times, nt, out,
                                          out_kind, s, cells);
    };
    if (layout != kYuvI420 && layout != kYuvNv12) return hipErrorInvalidValue;
    if (dtype_in == 4) {
        if (layout == kYuvI420) return go(ChromaFrame16<kYuvI420, false>{});
        return g_nv12_wide ? go(ChromaFrame16<kYuvNv12, true>{})
                           : go(ChromaFrame16<kYuvNv12, false>{});
    }
    if (layout == kYuvI420) return go(ChromaFrame<kYuvI420, false>{});
    return g_nv12_wide ? go(ChromaFrame<kYuvNv12, true>{}) : go(ChromaFrame<kYuvNv12, false>{});
}

}  // namespace hsflow
