// hsflow_temporal.hip -- the temporal warm start of the warped solves
// ("Temporal warm start"): a flow handed to a solve as its start,
// and the start of pair k+1 predicted from the backward flow of pair k.
//
//  KD hs_downflow_kernel      one level down, KU's counterpart: a flow plane
//     pair of level l becomes level l+1, size ceil(n / 2).  Per component:
//       a = u[2y][2x];               b = u[2y][min(2x+1, C-1)]
//       c = u[min(2y+1, R-1)][2x];   d = u[min(2y+1, R-1)][min(2x+1, C-1)]
//       uc[y][x] = ((a + b) + (c + d)) * 0.125f
//     the mean of the four, halved: px of the coarser level.  No multiply is
//     followed by an add, so nothing can be contracted and numpy f32 gives the
//     same bits.  No index depends on a value: NaN and inf pass through.
//
//  KP hs_flow_predict_kernel  pair k's backward flow (ub, vb), I1 -> I0 on I1's
//     grid, into the start of pair k+1, whose first frame is that I1.  Under
//     constant velocity:
//       uf' = -ub;  vf' = -vb                      (the sign bit flipped)
//       ub' = ub at (y + 8 vb, x + 8 ub);  vb' = vb at the same point
//     sampled by the one sampler (hsflow_sampler.h), so ub' is KR's output for
//     the plane ub under the flow (ub, vb) bit for bit, vb' likewise.  One
//     launch; the taps are computed once for both components.  Either output
//     pair may be null.
//
// Both are HBM-bound and one-off per solve: KD reads 8 and writes 2 B per fine
// pixel, KP reads 8 (the taps of a smooth flow hit the lines the centre loads
// fetched) and writes 16 B/px.  KR's map: block 64 x 4, one pixel per thread,
// grid (ceil(cols/64), ceil(rows/4), batch); consecutive lanes take
// consecutive pixels of a row.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hsflow_internal.h"
#include "hsflow_sampler.h"

namespace hsflow {
namespace {

using namespace sampler;

// grid over the coarse plane; rc = ceil(rows / 2), cc = ceil(cols / 2), so
// 2y <= rows - 1 and 2x <= cols - 1 for every pixel written
__global__ __launch_bounds__(256) void hs_downflow_kernel(const float *__restrict__ u,
                                                          const float *__restrict__ v, int rows,
                                                          int cols, float *__restrict__ uc,
                                                          float *__restrict__ vc, int rc, int cc) {
    const int x = blockIdx.x * 64 + threadIdx.x;
    const int y = blockIdx.y * 4 + threadIdx.y;
    if (x >= cc || y >= rc) return;
    const int xa = 2 * x, xb = min(2 * x + 1, cols - 1);
    const size_t base = (size_t)blockIdx.z * rows * cols;
    const size_t top = base + (size_t)(2 * y) * cols;
    const size_t bot = base + (size_t)min(2 * y + 1, rows - 1) * cols;
    const size_t o = (size_t)blockIdx.z * rc * cc + (size_t)y * cc + x;
    uc[o] = ((u[top + xa] + u[top + xb]) + (u[bot + xa] + u[bot + xb])) * 0.125f;
    vc[o] = ((v[top + xa] + v[top + xb]) + (v[bot + xa] + v[bot + xb])) * 0.125f;
}

__device__ __forceinline__ float flip_sign(float f) {
    return __uint_as_float(__float_as_uint(f) ^ 0x80000000u);
}

__global__ __launch_bounds__(256) void hs_flow_predict_kernel(
    const float *__restrict__ ub, const float *__restrict__ vb, int rows, int cols,
    float *__restrict__ uf_next, float *__restrict__ vf_next, float *__restrict__ ub_next,
    float *__restrict__ vb_next) {
    const int x = blockIdx.x * 64 + threadIdx.x;
    const int y = blockIdx.y * 4 + threadIdx.y;
    if (x >= cols || y >= rows) return;
    const size_t plane = (size_t)rows * cols;
    const size_t o = blockIdx.z * plane + (size_t)y * cols + x;
    const float bu = ub[o], bv = vb[o];
    if (uf_next) {  // uniform
        uf_next[o] = flip_sign(bu);
        vf_next[o] = flip_sign(bv);
    }
    if (ub_next) {  // uniform
        bool in;
        int nearest;
        const Taps t = sample_taps(rows, cols, x, y, bu, bv, in, nearest);
        ub_next[o] = sample_plane(ub + blockIdx.z * plane, cols, t);
        vb_next[o] = sample_plane(vb + blockIdx.z * plane, cols, t);
    }
}

}  // namespace

hipError_t launch_downflow(const float *u, const float *v, int rows, int cols, float *uc,
                           float *vc, int rc, int cc, int batch, hipStream_t s) {
    if (rc != (rows + 1) / 2 || cc != (cols + 1) / 2) return hipErrorInvalidValue;
    dim3 blk(64, 4, 1), grd((cc + 63) / 64, (rc + 3) / 4, batch);
    hipLaunchKernelGGL(hs_downflow_kernel, grd, blk, 0, s, u, v, rows, cols, uc, vc, rc, cc);
    return hipGetLastError();
}

hipError_t launch_flow_predict(const float *ub, const float *vb, int rows, int cols, int batch,
                               float *uf_next, float *vf_next, float *ub_next, float *vb_next,
                               hipStream_t s) {
    dim3 blk(64, 4, 1), grd((cols + 63) / 64, (rows + 3) / 4, batch);
    hipLaunchKernelGGL(hs_flow_predict_kernel, grd, blk, 0, s, ub, vb, rows, cols, uf_next,
                       vf_next, ub_next, vb_next);
    return hipGetLastError();
}

}  // namespace hsflow
