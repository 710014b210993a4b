// hsflow_interp_bgr.hip -- KR and KI (hsflow_interp.hip) for colour frames
// ("Colour frame interpolation").  Frames are dense 8-bit
// interleaved BGR, [batch][rows][cols][3], what hsflow_bgr_to_gray_device
// reads; the flow stays a grey-level quantity, so only the sampling knows
// about channels.
//
//  KRC hs_warp_image_bgr_kernel   out(y, x, c) = I(.., c) sampled bilinearly at
//     (y + 8 v, x + 8 u): KR's positions and weights once per pixel, its three
//     lerps per channel.  oof as KR's, one byte per pixel.
//
//  KIC hs_frame_interp_kernel<BgrFrame>  KI's kernel (hsflow_sampler.h) with a
//     pixel of three channels: per output pixel what KI does, once -- (u0, v0),
//     (u1, v1) of each time, the clamped displacement split, the four tap
//     positions and two fractions per source, in0, in1, n0, n1, wt, flags and
//     the trusted count -- then KI's three lerps and KI's blend on each of the
//     three channels, so channel c of the result has the bits KI gives the
//     plane bgr[..., c].
//
// Thread map: KI's, the same text (256 threads, tiles of 512 consecutive pixels
// of a pair's plane, thread t the pixels t and t + 256, flows loaded once and
// reused over the times, the grid capped per CU and striding over the tiles,
// one global atomic per block and time).
// Loads: a tap is three bytes at a data-dependent address.  The two
// horizontally adjacent taps of a row are six consecutive bytes unless the
// pair is clamped at a frame edge (xb == xa); `Wide` reads them as one
// unaligned dword and one unaligned halfword -- two loads for six -- and
// leaves single bytes to the clamped pairs.  Both forms give the same bits.
// Measured (scripts/interp_bgr_timing.py), the single bytes are the
// faster form -- a dword at a byte address is not one access -- so they are
// the default; hsflow_set_interp_bgr_loads switches.
// Stores: a quad of lanes holds the pixels 4q .. 4q + 3, twelve consecutive
// bytes of a u8 frame; where they form three aligned dwords, lanes 0..2 of the
// quad collect one each over DPP and store it, else (ragged quads at a
// plane's ends, odd planes, unaligned bases) every valid lane stores its three
// bytes.  An f32 pixel is one 12-byte store.  Byte offsets are size_t.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "hsflow_internal.h"
#include "hsflow_sampler.h"

namespace hsflow {
namespace {

using namespace sampler;

std::atomic<int> g_wide_loads{0};

using Bgr = Pixel<3>;

__device__ __forceinline__ uint32_t load_u32_unaligned(const uint8_t *p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
__device__ __forceinline__ uint32_t load_u16_unaligned(const uint8_t *p) {
    uint16_t v;
    __builtin_memcpy(&v, p, 2);
    return v;
}

// the taps xa and xb of one row of a BGR plane (row: its first byte)
template <bool Wide>
__device__ __forceinline__ void row_taps(const uint8_t *__restrict__ row, int xa, int xb, Bgr &a,
                                         Bgr &b) {
    const uint8_t *pa = row + (size_t)xa * 3;
    if (Wide && xb != xa) {  // xb == xa + 1: six bytes of this row
        const uint32_t lo = load_u32_unaligned(pa), hi = load_u16_unaligned(pa + 4);
        a.c[0] = (float)(lo & 0xFF), a.c[1] = (float)((lo >> 8) & 0xFF);
        a.c[2] = (float)((lo >> 16) & 0xFF), b.c[0] = (float)(lo >> 24);
        b.c[1] = (float)(hi & 0xFF), b.c[2] = (float)(hi >> 8);
    } else {
        const uint8_t *pb = row + (size_t)xb * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) a.c[c] = (float)pa[c], b.c[c] = (float)pb[c];
    }
}

// img (one pair's BGR plane) at the taps `t`: KR's sample, per channel
template <bool Wide>
__device__ __forceinline__ Bgr sample_bgr(const uint8_t *__restrict__ img, int cols,
                                          const Taps &t) {
    Bgr ta, tb, ba, bb, r;
    row_taps<Wide>(img + (size_t)t.ya * cols * 3, t.xa, t.xb, ta, tb);
    row_taps<Wide>(img + (size_t)t.yb * cols * 3, t.xa, t.xb, ba, bb);
#pragma unroll
    for (int c = 0; c < 3; ++c) r.c[c] = lerp_taps(ta.c[c], tb.c[c], ba.c[c], bb.c[c], t.fx, t.fy);
    return r;
}

// Three bytes per lane (bgr: B | G << 8 | R << 16) into a u8 BGR plane: quad:
// the first byte of the lane's quad of pixels, whole: its four pixels lie in
// the plane.  Three aligned dwords per quad where the address allows, else
// three bytes per valid lane.  Every lane of the wave calls.
__device__ __forceinline__ void store_quad_bgr_u8(uint8_t *quad, bool whole, bool valid,
                                                  uint32_t bgr, int lane) {
    const uint32_t p0 = quad_lane<0>(bgr), p1 = quad_lane<1>(bgr), p2 = quad_lane<2>(bgr),
                   p3 = quad_lane<3>(bgr);
    const int j = lane & 3;
    if (whole && ((uintptr_t)quad & 3) == 0) {
        // bytes: B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3
        const uint32_t w = j == 0 ? (p0 | p1 << 24) : j == 1 ? (p1 >> 8 | p2 << 16)
                                                             : (p2 >> 16 | p3 << 8);
        if (j < 3) reinterpret_cast<uint32_t *>(quad)[j] = w;
    } else if (valid) {
        uint8_t *d = quad + j * 3;
        d[0] = (uint8_t)bgr, d[1] = (uint8_t)(bgr >> 8), d[2] = (uint8_t)(bgr >> 16);
    }
}

__device__ __forceinline__ uint32_t pack_u8(const Bgr &o) {
    return round_u8(o.c[0]) | round_u8(o.c[1]) << 8 | round_u8(o.c[2]) << 16;
}

// one f32 pixel: a 12-byte store (the plane is 4-byte aligned)
struct alignas(4) Float3 {
    float c[3];
};

// ---- KRC: block 64 x 4, one pixel per thread (KR's map);
// grid (ceil(cols/64), ceil(rows/4), batch).  Every lane computes (a lane past
// the frame on a clamped pixel): the quad exchange needs all lanes active.
template <bool Wide>
__global__ __launch_bounds__(256) void hs_warp_image_bgr_kernel(
    const uint8_t *__restrict__ I, const float *__restrict__ u, const float *__restrict__ v,
    int rows, int cols, void *__restrict__ out, int out_u8, uint8_t *__restrict__ oof) {
    const int xr = blockIdx.x * 64 + threadIdx.x, yr = blockIdx.y * 4 + threadIdx.y;
    const bool valid = xr < cols && yr < rows;
    const int x = min(xr, cols - 1), y = min(yr, rows - 1);
    const size_t plane = (size_t)rows * cols;
    const size_t o = blockIdx.z * plane + (size_t)y * cols + x;
    bool in;
    int nearest;
    const Taps t = sample_taps(rows, cols, x, y, u[o], v[o], in, nearest);
    const Bgr r = sample_bgr<Wide>(I + blockIdx.z * plane * 3, cols, t);
    if (out_u8) {  // uniform
        const int xq = xr - (threadIdx.x & 3);  // the quad's first column
        const size_t oq = blockIdx.z * plane + (size_t)y * cols + xq;
        store_quad_bgr_u8((uint8_t *)out + oq * 3, yr < rows && xq + 3 < cols, valid, pack_u8(r),
                          threadIdx.x);
    } else if (valid) {
        reinterpret_cast<Float3 *>(out)[o] = Float3{{r.c[0], r.c[1], r.c[2]}};
    }
    if (oof && valid) oof[o] = in ? 0 : 1;
}

// ---- KIC: hs_frame_interp_kernel on a BGR frame
template <bool Wide>
struct BgrFrame {
    using Elem = uint8_t;
    static constexpr int kChannels = 3;
    using Px = Bgr;
    // 84 VGPRs with wide loads: five waves per SIMD, five blocks per CU (80
    // with byte loads, which would let a sixth in; one cap for both forms)
    static constexpr int kBlocksPerCu = 5;
    static __device__ __forceinline__ Bgr sample(const uint8_t *__restrict__ img, int cols,
                                                 const Taps &t) {
        return sample_bgr<Wide>(img, cols, t);
    }
    static __device__ __forceinline__ void store_f32(void *out, size_t px, const Bgr &o) {
        reinterpret_cast<Float3 *>(out)[px] = Float3{{o.c[0], o.c[1], o.c[2]}};
    }
    static __device__ __forceinline__ void store_u8(void *out, size_t obase, int, int q0,
                                                    bool whole, bool valid, const Bgr &o, int lane) {
        store_quad_bgr_u8((uint8_t *)out + (obase + (size_t)q0) * 3, whole, valid, pack_u8(o),
                          lane);
    }
};

}  // namespace

int set_interp_bgr_wide_loads(int on) { return g_wide_loads.exchange(on ? 1 : 0); }

hipError_t launch_warp_image_bgr(const uint8_t *I, int rows, int cols, int batch, const float *u,
                                 const float *v, void *out, bool out_u8, uint8_t *oof,
                                 hipStream_t s) {
    dim3 blk(64, 4, 1), grd((cols + 63) / 64, (rows + 3) / 4, batch);
    const int u8 = out_u8 ? 1 : 0;
    if (g_wide_loads.load())
        hipLaunchKernelGGL(hs_warp_image_bgr_kernel<true>, grd, blk, 0, s, I, u, v, rows, cols,
                           out, u8, oof);
    else
        hipLaunchKernelGGL(hs_warp_image_bgr_kernel<false>, grd, blk, 0, s, I, u, v, rows, cols,
                           out, u8, oof);
    return hipGetLastError();
}

hipError_t launch_frame_interp_bgr(const uint8_t *I0, const uint8_t *I1, int rows, int cols,
                                   int batch, const float *uf, const float *vf, const float *ub,
                                   const float *vb, const uint8_t *mask_f, const uint8_t *mask_b,
                                   const float *times, int nt, void *out, bool out_u8,
                                   uint8_t *flags, uint32_t *trusted, hipStream_t s) {
    const auto launch = g_wide_loads.load() ? launch_frame_interp_as<BgrFrame<true>>
                                            : launch_frame_interp_as<BgrFrame<false>>;
    return launch(I0, I1, rows, cols, batch, uf, vf, ub, vb, mask_f, mask_b, times, nt, out,
                  out_u8, flags, trusted, s, nullptr);
}

// KIP on BGR frames: the cells come from the grey planes (hsflow_project.hip)
hipError_t launch_frame_interp_bgr_proj(const uint8_t *I0, const uint8_t *I1, int rows, int cols,
                                        int batch, const float *uf, const float *vf,
                                        const float *ub, const float *vb, const uint8_t *mask_f,
                                        const uint8_t *mask_b, const uint64_t *cells,
                                        const float *times, int nt, void *out, bool out_u8,
                                        uint8_t *flags, uint32_t *trusted, hipStream_t s) {
    if (!cells) return hipErrorInvalidValue;
    const auto launch = g_wide_loads.load() ? launch_frame_interp_as<BgrFrame<true>>
                                            : launch_frame_interp_as<BgrFrame<false>>;
    return launch(I0, I1, rows, cols, batch, uf, vf, ub, vb, mask_f, mask_b, times, nt, out,
                  out_u8, flags, trusted, s, cells);
}

}  // namespace hsflow
