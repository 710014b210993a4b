// hsflow_project.hip -- the flows of a bidirectional solve carried to time t
// before a frame is interpolated there ("Flow projection"; Baker
// et al., IJCV 2011, section 3.3.2).
//
//  KS hs_flow_project_kernel   every pixel p = (y, x) of both frames is one
//     candidate per time t (s = 1 - t), all in f32:
//       direction 0: frame A = I0, other frame I1, flow (uf, vf), tau = t
//       direction 1: frame A = I1, other frame I0, flow (ub, vb), tau = s
//       dx, dy = 8 u, 8 v clamped to [-cols, cols] / [-rows, rows] as floats
//                (split_disp's clamp: NaN -> lower bound)
//       w      = the other frame at (y + dy, x + dx), the sampler's taps and
//                lerps (hsflow_sampler.h; f64 frames in f64)
//       cost   = |w - A(p)|, rounded to f32 once
//       code   = cost * 8 as a float; !(code < 2^30) -> 2^30 (NaN lands there);
//                truncated to uint32
//       qx     = x + (int)floorf(tau dx + 0.5f), qy likewise, with no multiply
//                fused into an add: the displacement is rounded on its own, so
//                the target is as exact in row 262139 as in row 0; both tested
//                against [0, cols) / [0, rows): a candidate outside has no
//                target
//       key    = code << 32 | dir << 31 | (y cols + x)
//       cells[pair][time][qy][qx] = min(cells[..], key)     one 64-bit atomic
//     The minimum is an integer one, so the plane holds the same bytes
//     whatever order the candidates arrive in: the lowest cost wins a target,
//     then direction 0, then the lower source index.  The caller sets the plane
//     to all ones first; a cell that stays so received nothing (a hole).
//     The cost does not depend on t: a thread loads its pixel's four flows and
//     two frame values once, samples twice and issues up to 2 nt atomics.
//
// Thread map: KC's tiles (hsflow_consistency.hip) without the shifted start,
// which only KC's packed mask stores need: a block of 1024 threads takes tiles
// of 4096 consecutive pixels of a pair's plane, thread t the pixels t, t + 1024,
// t + 2048, t + 3072, so the flow and frame loads and the taps of a smooth flow
// coalesce, and neighbouring lanes' targets are neighbouring cells.  The grid
// is capped at two blocks per CU and strides over the tiles.
// Traffic per pixel: 16 B of flows, 2 x sizeof(T) of frames (the taps overlap
// the neighbours'), and per time two 8-byte atomics on a plane of 8 B/px that
// the memset wrote before.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "hsflow_internal.h"
#include "hsflow_sampler.h"

// the target's sum must round as written (the sampler's own functions, defined
// above this line, keep the compiler's choice, as in every kernel that samples)
#pragma clang fp contract(off)

namespace hsflow {
namespace {

using namespace sampler;

constexpr int kThreads = 1024, kPix = 4, kTile = kThreads * kPix;

// cost * 8 of candidate (x, y) of frame `own` (value a) against frame `other`
// at the flow's target, as the key's upper word
template <typename T>
__device__ __forceinline__ uint32_t cost_code(const T *__restrict__ other, T a, int rows, int cols,
                                              int x, int y, float u, float v) {
    using F = typename FrameMath<T>::type;
    bool in;
    int nearest;  // both unused
    const Taps tp = sample_taps(rows, cols, x, y, u, v, in, nearest);
    const F w = sample_plane(other, cols, tp);
    const F d = w - (F)a;
    const float cost = (float)(d < (F)0 ? -d : d);  // NaN stays NaN
    float code = cost * 8.0f;
    if (!(code < 1073741824.0f)) code = 1073741824.0f;
    return (uint32_t)code;
}

// the clamp of split_disp, on the displacement alone
__device__ __forceinline__ float clamp_disp(float d, int n) {
    return fminf(fmaxf(d, -(float)n), (float)n);
}

// one candidate at one time: the atomic, where the target is in the frame
__device__ __forceinline__ void splat(unsigned long long *__restrict__ plane_cells, int rows,
                                      int cols, int x, int y, float dx, float dy, float tau,
                                      unsigned long long key) {
    // The displacement is rounded on its own and added to the pixel as an
    // integer: floorf((float)y + tau * dy + 0.5f) holds the sum to 1/64 px from
    // row 2^17 on and sent 0.4 % of a 262140-row plane's candidates a row off.
    // dx, dy are clamped (never NaN) and the API admits tau in [0, 1] only, so
    // |tau dx| <= cols, |tau dy| <= rows and neither conversion can overflow.
    const int qx = x + (int)floorf(tau * dx + 0.5f);
    const int qy = y + (int)floorf(tau * dy + 0.5f);
    if (qx < 0 || qx >= cols || qy < 0 || qy >= rows) return;
    atomicMin(plane_cells + (size_t)qy * cols + qx, key);
}

// grid (blocks per pair, batch)
template <typename T>
__global__ __launch_bounds__(kThreads) void hs_flow_project_kernel(
    const T *__restrict__ G0, const T *__restrict__ G1, const float *__restrict__ uf,
    const float *__restrict__ vf, const float *__restrict__ ub, const float *__restrict__ vb,
    int rows, int cols, InterpTimes times, int nt, unsigned long long *__restrict__ cells) {
    const int plane = rows * cols;  // <= 2^29 - 4
    const size_t base = (size_t)blockIdx.y * plane;
    const int ntiles = (plane + kTile - 1) / kTile;
    const float inv_cols = 1.0f / (float)cols;
    const T *p0 = G0 + base, *p1 = G1 + base;
    unsigned long long *pc = cells + (size_t)blockIdx.y * nt * plane;
    const int t = threadIdx.x;

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
#pragma unroll
        for (int k = 0; k < kPix; ++k) {
            const int p = tile * kTile + k * kThreads + t;
            if (p >= plane) continue;
            const XY q = pixel_xy(p, cols, inv_cols);
            const float fu = uf[base + p], fv = vf[base + p];
            const float bu = ub[base + p], bv = vb[base + p];
            const T a0 = p0[p], a1 = p1[p];
            const uint32_t c0 = cost_code<T>(p1, a0, rows, cols, q.x, q.y, fu, fv);
            const uint32_t c1 = cost_code<T>(p0, a1, rows, cols, q.x, q.y, bu, bv);
            const unsigned long long k0 = (unsigned long long)c0 << 32 | (uint32_t)p;
            const unsigned long long k1 = (unsigned long long)c1 << 32 | 0x80000000u | (uint32_t)p;
            const float fdx = clamp_disp(8.0f * fu, cols), fdy = clamp_disp(8.0f * fv, rows);
            const float bdx = clamp_disp(8.0f * bu, cols), bdy = clamp_disp(8.0f * bv, rows);
            for (int ti = 0; ti < nt; ++ti) {
                const float tt = times.t[ti], s = 1.0f - tt;
                unsigned long long *plane_cells = pc + (size_t)ti * plane;
                splat(plane_cells, rows, cols, q.x, q.y, fdx, fdy, tt, k0);
                splat(plane_cells, rows, cols, q.x, q.y, bdx, bdy, s, k1);
            }
        }
    }
}

}  // namespace

hipError_t launch_flow_project(const void *G0, const void *G1, int dtype_in, int rows, int cols,
                               int batch, const float *uf, const float *vf, const float *ub,
                               const float *vb, const float *times, int nt, uint64_t *cells,
                               hipStream_t s) {
    if (nt < 1 || nt > kInterpMaxTimes) return hipErrorInvalidValue;
    InterpTimes tm{};
    for (int k = 0; k < nt; ++k) tm.t[k] = times[k];
    const size_t plane = (size_t)rows * cols;
    const int ntiles = (int)((plane + kTile - 1) / kTile);
    // two blocks of 16 waves fill a CU, as KC's
    const int cap = std::max(1, (2 * device_cus() + batch - 1) / batch);
    dim3 blk(kThreads, 1, 1), grd(std::min(ntiles, cap), batch, 1);
    const bool known = dispatch_frame_type(dtype_in, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(hs_flow_project_kernel<T>, grd, blk, 0, s, (const T *)G0,
                           (const T *)G1, uf, vf, ub, vb, rows, cols, tm, nt,
                           (unsigned long long *)cells);
    });
    if (!known) return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace hsflow
