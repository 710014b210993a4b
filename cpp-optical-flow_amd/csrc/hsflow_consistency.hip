// hsflow_consistency.hip -- the forward-backward check of a bidirectional
// solve ("Forward-backward consistency").
//
//  KC hs_flow_consistency_kernel   once per direction.  Per pixel (y, x) of a
//     pair, with (uf, vf) the flow under test and (ub, vb) the opposite one
//     (solver units: 8 px per unit, as KW):
//       dx, dy   = 8 uf, 8 vf clamped to [-cols, cols] / [-rows, rows]
//                  (clamped as floats, NaN -> lower bound);
//       ubw, vbw = ub, vb sampled bilinearly at (y + dy, x + dx), taps
//                  clamped to the plane: the sampler KW uses (hsflow_sampler.h);
//       su, sv   = uf + ubw, vf + vbw
//       d2       = 64 (su^2 + sv^2)                        px^2
//       mag      = 64 ((uf^2 + vf^2) + (ubw^2 + vbw^2))
//       err      = sqrt(d2)                                px
//       mask     = 2 if the target leaves the frame by more than half a pixel,
//                  else 1 if !(d2 <= rel mag + abs), else 0.
//     Both comparisons are negated, so a NaN anywhere gives a non-zero mask;
//     a d2 that overflows f32 is inconsistent too, as in exact arithmetic.
//
// HBM-bound: 8 B (uf, vf) + 8 B (ub, vb; the four taps of neighbouring
// pixels overlap, so each element comes from HBM once) read and 4 B + 1 B
// written per pixel.  A block of 1024 threads takes tiles of 4096 consecutive
// pixels of a pair's plane (rows run on into one another), thread t the
// pixels t, t + 1024, t + 2048, t + 3072 of the tile: consecutive lanes hold
// consecutive pixels, so the flow loads, the taps of a smooth flow and the err
// stores coalesce, and the four iterations' 32 tap loads are in flight at
// once.  A tile starts where its first element's index in the whole batch is
// a multiple of four (up to three pixels before the plane), so every quad of
// lanes owns one aligned dword of the mask: lane 0 of the quad collects the
// four classes over DPP and stores them at once, whatever rows*cols is.  A
// mask base that is not 4-byte aligned and the ragged quads at a plane's ends
// store bytes.  The grid is capped at two blocks per CU and strides over the
// tiles, so a pair's counts take at most 3 atomics per block.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "hsflow_internal.h"
#include "hsflow_sampler.h"

namespace hsflow {
namespace {

using namespace sampler;

constexpr int kThreads = 1024, kPix = 4, kTile = kThreads * kPix;

// grid (blocks per pair, batch); pack_mask: the mask's base is 4-byte aligned
__global__ __launch_bounds__(kThreads) void hs_flow_consistency_kernel(
    const float *__restrict__ uf, const float *__restrict__ vf, const float *__restrict__ ub,
    const float *__restrict__ vb, int rows, int cols, float rel, float abs_thr,
    float *__restrict__ err, uint8_t *__restrict__ mask, uint32_t *__restrict__ counts,
    int pack_mask) {
    __shared__ uint32_t wave_counts[kThreads / 64][3];
    const int plane = rows * cols;  // <= 2^29 - 4
    const size_t base = (size_t)blockIdx.y * plane;
    const int shift = (int)(base & 3);  // base + tile start is a multiple of 4
    const int ntiles = (plane + shift + kTile - 1) / kTile;
    const float inv_cols = 1.0f / (float)cols;
    const float *puf = uf + base, *pvf = vf + base, *pub = ub + base, *pvb = vb + base;
    const int t = threadIdx.x;
    uint32_t c0 = 0, c1 = 0, c2 = 0;

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int p0 = tile * kTile - shift + t;
#pragma unroll
        for (int k = 0; k < kPix; ++k) {
            const int pk = p0 + k * kThreads;
            const bool valid = pk >= 0 && pk < plane;
            // every lane computes (a pixel outside the plane on its nearest
            // one): the quad exchange below needs all lanes active
            const int p = clampi(pk, plane);
            const XY q = pixel_xy(p, cols, inv_cols);
            const int x = q.x, y = q.y;
            const float u = puf[p], v = pvf[p];
            bool in;
            int nearest;  // unused
            const Taps tp = sample_taps(rows, cols, x, y, u, v, in, nearest);
            const float ubw = sample_plane(pub, cols, tp), vbw = sample_plane(pvb, cols, tp);
            const float su = u + ubw, sv = v + vbw;
            const float d2 = 64.0f * (su * su + sv * sv);
            const float mag = 64.0f * ((u * u + v * v) + (ubw * ubw + vbw * vbw));
            // d2 <= FLT_MAX: a sum that overflows f32 fails the test, as it
            // does in exact arithmetic (inf <= inf would pass it)
            const bool ok = d2 <= rel * mag + abs_thr && d2 <= 3.402823466e38f;
            const uint32_t cls = !in ? 2u : (!ok ? 1u : 0u);
            c0 += valid && cls == 0u;
            c1 += valid && cls == 1u;
            c2 += valid && cls == 2u;
            if (err && valid) err[base + p] = sqrtf(d2);
            if (mask) {  // uniform
                // store_quad_u8 with the alignment decided on the host: base +
                // q0 is a multiple of four here, so only the mask's base counts
                // (the sampler's per-quad test costs KC 11 VGPRs and 2 % at
                // batch 8)
                const uint32_t quad = cls | quad_lane<1>(cls) << 8 | quad_lane<2>(cls) << 16 |
                                      quad_lane<3>(cls) << 24;
                const int q0 = pk - (t & 3);  // the quad's first pixel
                if (pack_mask && q0 >= 0 && q0 + 3 < plane) {
                    if ((t & 3) == 0) *reinterpret_cast<uint32_t *>(mask + base + q0) = quad;
                } else if (valid) {
                    mask[base + p] = (uint8_t)cls;
                }
            }
        }
    }
    if (!counts) return;  // uniform over the grid
    // per wave: butterfly sums; per block: one ordinary global atomic per
    // class that occurs
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        c0 += __shfl_xor(c0, off, 64);
        c1 += __shfl_xor(c1, off, 64);
        c2 += __shfl_xor(c2, off, 64);
    }
    const int wave = t >> 6, lane = t & 63;
    if (lane == 0) wave_counts[wave][0] = c0, wave_counts[wave][1] = c1, wave_counts[wave][2] = c2;
    __syncthreads();
    if (t < 3) {
        uint32_t c = 0;
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) c += wave_counts[w][t];
        if (c) atomicAdd(counts + (size_t)blockIdx.y * 3 + t, c);
    }
}

}  // namespace

hipError_t launch_consistency(const float *uf, const float *vf, const float *ub,
                              const float *vb, int rows, int cols, int batch, float rel,
                              float abs_thr, float *err, uint8_t *mask, uint32_t *counts,
                              hipStream_t s) {
    const size_t plane = (size_t)rows * cols;
    // a plane's first tile may start up to 3 pixels before it
    const int ntiles = (int)((plane + 3 + kTile - 1) / kTile);
    // two blocks of 16 waves fill a CU's 8 waves per SIMD; more blocks only
    // add atomics on the counts, which share a cache line
    const int cap = std::max(1, (2 * device_cus() + batch - 1) / batch);
    dim3 blk(kThreads, 1, 1), grd(std::min(ntiles, cap), batch, 1);
    hipLaunchKernelGGL(hs_flow_consistency_kernel, grd, blk, 0, s, uf, vf, ub, vb, rows, cols,
                       rel, abs_thr, err, mask, counts, ((uintptr_t)mask & 3) == 0 ? 1 : 0);
    return hipGetLastError();
}

}  // namespace hsflow
