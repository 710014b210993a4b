// hsflow_upsample.hip -- the coarse solve's way back to the full frame
// ("Coarse solve"): a flow solved down to pyramid level `finest`
// only is brought up level by level by a bilinear x2 step.
//
//  KB hs_upflow_bilinear_kernel  one level up, KU's counterpart for a final
//     flow (KU is nearest-neighbour: right for a warm start, blocky as a
//     result).  Pixel centres aligned, border replicated; per component, in
//     f32, in this order:
//       sy = min(max(0.5f*y - 0.25f, 0), rc-1); y0 = floor(sy); fy = sy - y0;
//       y1 = min(y0+1, rc-1);  sx, x0, fx, x1 likewise with cc
//       top = a[y0][x0] + fx*(a[y0][x1] - a[y0][x0])
//       bot = a[y1][x0] + fx*(a[y1][x1] - a[y1][x0])
//       out = 2 * (top + fy*(bot - top))
//     The weights are 0, 0.25 or 0.75, exact in f32; contraction is off, so
//     numpy f32 gives the same bits.  No index depends on a value: NaN and inf
//     pass through arithmetically.
//
// Thread map.  HBM-bound: 8 B written and 2 B read per fine pixel.  A lane owns
// the fine columns 4g .. 4g+3 of the two fine rows 2p-1 and 2p, which share
// their coarse rows (p-1 and p; fine rows 2p and 2p+1 would need three).  Its
// columns' taps are the four coarse columns 2g-1 .. 2g+2, clamped: per
// component 2 rows x 4 taps for 8 outputs.  Block 64 x 4, a wave per row pair:
// a wave writes 1 KiB of a row, contiguous.  Grid (ceil(ceil(cols/4)/64),
// ceil((rows/2 + 1)/4), batch).  Two bodies, the same arithmetic and bits:
//   wide    cols % 4 == 0, (u, v) 16-byte and (uc, vc) 8-byte aligned, so every
//           group of every row of every pair is aligned: the two middle taps
//           as one 8-byte load (a wave reads 512 contiguous bytes of a coarse
//           row), the outer two from the neighbouring lanes by shuffle, one
//           16-byte store per row and component;
//   scalar  any other plane (the contract asks for element alignment only):
//           four clamped 4-byte loads per row, 4-byte stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hsflow_internal.h"

#pragma clang fp contract(off)

namespace hsflow {
namespace {

// one fine row's four pixels of one component: t0 / t1 the taps of its coarse
// rows y0 / y1.  Pixel i reads x0 = tap {0, 1, 1, 2}[i] and x1 = tap
// {1, 2, 2, 3}[i]; `first`: the plane's first column, whose sx is clamped to 0,
// so that x0 = 0 (tap 0, clamped) and x1 = min(1, cc-1) (tap 2)
__device__ __forceinline__ void up_row(const float (&t0)[4], const float (&t1)[4], bool first,
                                       const float (&fx)[4], float fy, float (&o)[4]) {
    constexpr int k0[4] = {0, 1, 1, 2}, k1[4] = {1, 2, 2, 3};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float a1 = i == 0 && first ? t0[2] : t0[k1[i]];
        const float b1 = i == 0 && first ? t1[2] : t1[k1[i]];
        const float top = t0[k0[i]] + fx[i] * (a1 - t0[k0[i]]);
        const float bot = t1[k0[i]] + fx[i] * (b1 - t1[k0[i]]);
        o[i] = 2.0f * (top + fy * (bot - top));
    }
}

__device__ __forceinline__ void store_row(float *__restrict__ dst, const float (&o)[4], int n,
                                          bool vec) {
    if (vec) {
        *reinterpret_cast<float4 *>(dst) = make_float4(o[0], o[1], o[2], o[3]);
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (i < n) dst[i] = o[i];
}

// the four taps of one coarse row for a lane of the wide path: columns 2g and
// 2g+1 as one 8-byte load (cc is even there, so both exist and the address is
// aligned), 2g-1 and 2g+2 from the neighbouring lanes' loads; a lane whose
// neighbour holds no such value (the wave's first and last lane, the row's last
// group) loads that tap itself, clamped to the plane.  Every lane of the wave
// calls it: the shuffles need them all.
__device__ __forceinline__ void wide_taps(const float *__restrict__ row, int g, int cc,
                                          bool own_left, bool own_right, float (&t)[4]) {
    const float2 m = *reinterpret_cast<const float2 *>(row + 2 * g);
    t[1] = m.x;
    t[2] = m.y;
    t[0] = __shfl_up(m.y, 1);
    t[3] = __shfl_down(m.x, 1);
    if (own_left) t[0] = row[max(2 * g - 1, 0)];
    if (own_right) t[3] = row[min(2 * g + 2, cc - 1)];
}

// WIDE: cols % 4 == 0 (so cc is even and a row has cols / 4 whole groups), u and
// v 16-byte and uc and vc 8-byte aligned: 8-byte loads, 16-byte stores.
template <bool WIDE>
__global__ __launch_bounds__(256) void hs_upflow_bilinear_kernel(
    const float *__restrict__ uc, const float *__restrict__ vc, int rc, int cc,
    float *__restrict__ u, float *__restrict__ v, int rows, int cols) {
    const int groups = (cols + 3) / 4;
    const int g_own = blockIdx.x * 64 + threadIdx.x;
    const int p = blockIdx.y * 4 + threadIdx.y;  // one per wave
    if (2 * p - 1 >= rows) return;
    const bool live = g_own < groups;
    if (!WIDE && !live) return;
    // a lane past the row's end (wide path) reads the last group's taps and
    // writes nothing
    const int g = min(g_own, groups - 1);
    const int x = 4 * g;
    // coarse rows: p-1 and p; for p = 0 (fine row 0 alone) y0 = 0 and
    // y1 = min(1, rc-1), as the definition has it
    const int r0 = max(p - 1, 0), r1 = min(r0 + 1, rc - 1);
    float fx[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float sx = fminf(fmaxf(0.5f * (float)(x + i) - 0.25f, 0.0f), (float)(cc - 1));
        fx[i] = sx - floorf(sx);
    }
    const size_t cb = (size_t)blockIdx.z * rc * cc;
    const size_t i0 = cb + (size_t)r0 * cc, i1 = cb + (size_t)r1 * cc;
    float ut0[4], ut1[4], vt0[4], vt1[4];
    if (WIDE) {
        const bool own_left = threadIdx.x == 0, own_right = threadIdx.x == 63 || g_own >= groups - 1;
        wide_taps(uc + i0, g, cc, own_left, own_right, ut0);
        wide_taps(uc + i1, g, cc, own_left, own_right, ut1);
        wide_taps(vc + i0, g, cc, own_left, own_right, vt0);
        wide_taps(vc + i1, g, cc, own_left, own_right, vt1);
        if (!live) return;
    } else {
        // coarse columns 2g-1 .. 2g+2, clamped to the plane
        int c[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) c[k] = min(max(2 * g - 1 + k, 0), cc - 1);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            ut0[k] = uc[i0 + c[k]];
            ut1[k] = uc[i1 + c[k]];
            vt0[k] = vc[i0 + c[k]];
            vt1[k] = vc[i1 + c[k]];
        }
    }
    const int n = min(4, cols - x);
    const size_t fb = (size_t)blockIdx.z * rows * cols;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int y = 2 * p - 1 + j;
        if (y < 0 || y >= rows) continue;
        const float sy = fminf(fmaxf(0.5f * (float)y - 0.25f, 0.0f), (float)(rc - 1));
        const float fy = sy - floorf(sy);
        const size_t o = fb + (size_t)y * cols + x;
        float ou[4], ov[4];
        up_row(ut0, ut1, g == 0, fx, fy, ou);
        up_row(vt0, vt1, g == 0, fx, fy, ov);
        store_row(u + o, ou, n, WIDE);
        store_row(v + o, ov, n, WIDE);
    }
}

}  // namespace

hipError_t launch_upflow_bilinear(const float *uc, const float *vc, int rc, int cc, float *u,
                                  float *v, int rows, int cols, int batch, hipStream_t s) {
    if (rc != (rows + 1) / 2 || cc != (cols + 1) / 2) return hipErrorInvalidValue;
    // the wide path: every group of every row of every pair is aligned
    const bool wide = cols % 4 == 0 && (((uintptr_t)u | (uintptr_t)v) & 15) == 0 &&
                      (((uintptr_t)uc | (uintptr_t)vc) & 7) == 0;
    const int groups = (cols + 3) / 4, pairs = rows / 2 + 1;
    dim3 blk(64, 4, 1), grd((groups + 63) / 64, (pairs + 3) / 4, batch);
    if (wide)
        hipLaunchKernelGGL(hs_upflow_bilinear_kernel<true>, grd, blk, 0, s, uc, vc, rc, cc, u, v,
                           rows, cols);
    else
        hipLaunchKernelGGL(hs_upflow_bilinear_kernel<false>, grd, blk, 0, s, uc, vc, rc, cc, u, v,
                           rows, cols);
    return hipGetLastError();
}

}  // namespace hsflow
