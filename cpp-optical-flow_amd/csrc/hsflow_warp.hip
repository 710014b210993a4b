// hsflow_warp.hip -- the warped coarse-to-fine solve's gradients: one level's
// brightness constancy linearised around the current flow (u0, v0) instead of
// around zero ("Warped coarse-to-fine solve").
//
//  KW hs_warp_gradients_kernel   once per warp of a level, next to `iters`
//     Jacobi iterations.  Per pixel:
//       gx, gy = 3x3 Sobel of I0, reflect-101 -- K1's arithmetic (sobel_at),
//                so the planes equal K1's bit for bit;
//       I1w    = I1 sampled bilinearly at (y + 8 v0, x + 8 u0), border
//                replicated: the sampler (hsflow_sampler.h); 8 is the gain of
//                the reference's unnormalised Sobel (hornSchunck.cpp:27-28):
//                one unit of (u, v) is 8 px;
//       gt'    = ((I1w - I0) - gx u0) - gy v0.
//     The Jacobi kernels then run hornSchunck.cpp:56-74 unchanged from these
//     f32 planes (flags[pair] != 0), warm-started from (u0, v0): the update
//     with It replaced by It' is the reference's own update of the
//     increment around (u0, v0).
//
// HBM-bound like K0 and KU (about 4 + 4 + 8 B read and 12 B written per pixel
// of f32 frames); the 3x3 and 2x2 neighbourhoods come from L1/L2, so the
// plain one-pixel-per-thread 64 x 4 map of hs_pyrdown_kernel is kept.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hsflow_internal.h"
#include "hsflow_sampler.h"

namespace hsflow {
namespace {

// K1's per-pixel arithmetic (hsflow_kernels.hip: reflect101, sobel_at; its
// GradMath is FrameMath), restated here term for term: that file and its
// headers are the Jacobi kernels' sources, whose md5 the committed counter
// profiles are tied to (bench.py kernel_source_md5), so they stay untouched.
// The sums associate as K1's do; tests/test_warped.py holds the two bit for bit.
__device__ __forceinline__ int reflect101(int p, int len) {
    // OpenCV borderInterpolate(BORDER_REFLECT_101) for |overshoot| <= 1.
    if (len == 1) return 0;
    p = p < 0 ? -p : p;
    return p >= len ? 2 * (len - 1) - p : p;
}

// Sobel dx, dy (ksize 3, reflect-101) of frame a at (r, c) and its centre
// pixel z_0, hornSchunck.cpp:27-28
template <typename T, typename F>
__device__ __forceinline__ void sobel_at(const T *a, int rows, int cols, int r, int c, F &dx,
                                         F &dy, F &z_0) {
    const int rm = reflect101(r - 1, rows), rp = reflect101(r + 1, rows);
    const int cm = reflect101(c - 1, cols), cp = reflect101(c + 1, cols);
    const T *pm = a + (size_t)rm * cols, *p0 = a + (size_t)r * cols,
            *pp = a + (size_t)rp * cols;
    const F m_m = (F)pm[cm], m_0 = (F)pm[c], m_p = (F)pm[cp];
    const F z_m = (F)p0[cm], z_p = (F)p0[cp];
    const F p_m = (F)pp[cm], p_0 = (F)pp[c], p_p = (F)pp[cp];
    z_0 = (F)p0[c];
    dx = (m_p - m_m) + (F)2 * (z_p - z_m) + (p_p - p_m);
    dy = (p_m - m_m) + (F)2 * (p_0 - m_0) + (p_p - m_p);
}

// block 64 x 4, one pixel per thread; grid (ceil(cols/64), ceil(rows/4), batch)
template <typename T>
__global__ __launch_bounds__(256) void hs_warp_gradients_kernel(
    const T *__restrict__ I0, const T *__restrict__ I1, const float *__restrict__ u0,
    const float *__restrict__ v0, int rows, int cols, float *__restrict__ gx,
    float *__restrict__ gy, float *__restrict__ gt, uint32_t *__restrict__ flags) {
    using F = typename FrameMath<T>::type;
    // the pair's Jacobi passes read the f32 planes, never the packed word
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && threadIdx.y == 0)
        flags[blockIdx.z] = 1u;
    const int x = blockIdx.x * 64 + threadIdx.x;
    const int y = blockIdx.y * 4 + threadIdx.y;
    if (x >= cols || y >= rows) return;
    const size_t plane = (size_t)rows * cols;
    const T *a = I0 + blockIdx.z * plane, *b = I1 + blockIdx.z * plane;
    const size_t o = blockIdx.z * plane + (size_t)y * cols + x;

    F dx, dy, z_0;
    sobel_at(a, rows, cols, y, x, dx, dy, z_0);

    const float u = u0[o], v = v0[o];
    bool in;
    int nearest;  // neither is used: dead code
    const sampler::Taps t = sampler::sample_taps(rows, cols, x, y, u, v, in, nearest);
    // exact at zero flow: I1w = I1 and gt' = I1 - I0
    const F I1w = sampler::sample_plane(b, cols, t);
    const F gtw = ((I1w - z_0) - dx * (F)u) - dy * (F)v;

    gx[o] = (float)dx;
    gy[o] = (float)dy;
    gt[o] = (float)gtw;
}

template <typename T>
void launch_t(const void *I0, const void *I1, const float *u0, const float *v0, int rows,
              int cols, int batch, float *gx, float *gy, float *gt, uint32_t *flags,
              hipStream_t s) {
    dim3 blk(64, 4, 1), grd((cols + 63) / 64, (rows + 3) / 4, batch);
    hipLaunchKernelGGL(hs_warp_gradients_kernel<T>, grd, blk, 0, s, (const T *)I0,
                       (const T *)I1, u0, v0, rows, cols, gx, gy, gt, flags);
}

}  // namespace

hipError_t launch_warp_gradients(const void *I0, const void *I1, int dtype_in, int rows,
                                 int cols, int batch, const float *u0, const float *v0,
                                 float *gx, float *gy, float *gt, uint32_t *flags,
                                 hipStream_t s) {
    const bool known = dispatch_frame_type(dtype_in, [&](auto t) {
        launch_t<decltype(t)>(I0, I1, u0, v0, rows, cols, batch, gx, gy, gt, flags, s);
    });
    if (!known) return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace hsflow
