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
// The loads, the stores and BgrFrame are in hsflow_frame_policy.h, which KF
// (hsflow_fallback.hip) shares.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "hsflow_frame_policy.h"
#include "hsflow_internal.h"
#include "hsflow_sampler.h"

namespace hsflow {
namespace {

using namespace sampler;

std::atomic<int> g_wide_loads{0};

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
