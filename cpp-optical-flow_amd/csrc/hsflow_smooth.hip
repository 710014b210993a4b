// hsflow_smooth.hip -- flow-driven (edge-preserving) smoothness of the warped
// solves ("Flow-driven smoothness").
//
//  KG hs_diffusivity_kernel   (u, v) -> g, one thread per pixel.  Solver units,
//     U = 8 u, V = 8 v in px; central differences, border replicated:
//       Ux = 0.5 (U[y][min(x+1, cols-1)] - U[y][max(x-1, 0)]) = 4 (u[..] - u[..])
//       s  = Ux^2 + Uy^2 + Vx^2 + Vy^2,  g = 1 / sqrt(1 + s / lambda^2)
//     A wave is 64 consecutive columns of one row: the centre loads are one
//     coalesced 256-byte row piece each, the neighbours hit the same lines.
//     HBM: 8 B read and 4 B written per pixel.
//
//  KJ hs_jacobi_weighted_kernel<W, KB>   W = 3 or 5.  The getFlow loop with the
//     two window means replaced by g-weighted ones.  Taps outside the plane
//     count as u = 0 with weight 1 (the reference's zero border), so with the
//     plane padded by g = 1, u = 0 and S the plain W x W window sum
//       ubar = S(g u) / S(g),  vbar = S(g v) / S(g)
//       k = X ubar + Y vbar + T,  u' = ubar - X k,  v' = vbar - Y k
//     (X, Y, T) = (Ix, Iy, It') / sqrt(alpha^2 + Ix^2 + Iy^2), the normalised
//     operator of hsflow_device.h.
//     One wave owns a 24-row x 64-column region held in registers (u, v, X, Y,
//     T, g and 1 / S(g) per row), runs up to KB iterations on it and stores
//     the inner (24 - KB (W-1)) x (64 - KB (W-1)) pixels: the temporal halo of
//     KB (W/2) on every side is recomputed, never exchanged.  Horizontal sums
//     are DPP lane shifts, vertical sums a register ring.  S(g) does not change
//     during a launch: it is summed once, in front of the iterations.
//     Every window sum is evaluated in one fixed order relative to its own
//     pixel, every multiply-add is an explicit fma and contraction is off, so
//     the result does not depend on KB, on the tile a pixel falls into or on
//     how the iterations are split into launches.
//     HBM per pass: 8 (u, v) + 12 (gx, gy, gt') + 4 (g) read, 8 written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "hsflow_device.h"
#include "hsflow_frame_types.h"
#include "hsflow_internal.h"

#pragma clang fp contract(off)

namespace hsflow {
namespace {

// grid (ceil(cols / 64), ceil(rows / 4), batch), block (64, 4)
__global__ __launch_bounds__(256) void hs_diffusivity_kernel(const float *__restrict__ u,
                                                             const float *__restrict__ v,
                                                             int rows, int cols, float inv_l2,
                                                             float *__restrict__ g) {
    const int x = blockIdx.x * 64 + threadIdx.x;
    const int y = blockIdx.y * 4 + threadIdx.y;
    if (x >= cols || y >= rows) return;
    const size_t base = (size_t)blockIdx.z * rows * cols;  // rows * cols <= 2^29 - 4
    const float *ur = u + base + (size_t)y * cols, *vr = v + base + (size_t)y * cols;
    const int xl = clampi(x - 1, cols), xr = clampi(x + 1, cols);
    const size_t up = base + (size_t)clampi(y - 1, rows) * cols + x;
    const size_t dn = base + (size_t)clampi(y + 1, rows) * cols + x;
    const float ux = 4.0f * (ur[xr] - ur[xl]), uy = 4.0f * (u[dn] - u[up]);
    const float vx = 4.0f * (vr[xr] - vr[xl]), vy = 4.0f * (v[dn] - v[up]);
    const float s = fmaf_x(vy, vy, fmaf_x(vx, vx, fmaf_x(uy, uy, ux * ux)));
    // capped below f32's range: g stays > 0, so no window's S(g) is ever 0
    g[base + (size_t)y * cols + x] =
        __builtin_amdgcn_rsqf(fminf(fmaf_x(s, inv_l2, 1.0f), 3.0e38f));
}

// Horizontal W-tap sums of two fields in lockstep (hsflow_kernels.hip hsum2's
// order: each DPP read of a just-written VGPR has the other field's
// instruction as its wait state).  W = 5: a(l) = x(l-1) + x(l);
// h = (a(l-1) + a(l+1)) + x(l+2).  W = 3: h = (x(l-1) + x(l)) + x(l+1).
template <int W>
__device__ __forceinline__ void hsum2(float x, float y, float &hx, float &hy) {
    static_assert(W == 3 || W == 5, "KJ is built for windows 3 and 5");
    const float ax = from_left(x) + x;
    const float ay = from_left(y) + y;
    if constexpr (W == 5) {
        const float bx = from_left(ax) + from_right(ax);
        const float by = from_left(ay) + from_right(ay);
        const float cx = from_right(x);
        const float cy = from_right(y);
        hx = bx + from_right(cx);
        hy = by + from_right(cy);
    } else {
        hx = ax + from_right(x);
        hy = ay + from_right(y);
    }
}

// Vertical sum of the ring's W row sums around row y, top to bottom:
// W = 5: ((h(y-2) + h(y-1)) + (h(y) + h(y+1))) + h(y+2); W = 3: (h(y-1) + h(y)) + h(y+1)
template <int W>
__device__ __forceinline__ float vsum(const float (&h)[W], int y) {
    constexpr int H = W / 2;
    if constexpr (W == 5)
        return ((h[(y - 2) % W] + h[(y - 1) % W]) + (h[y % W] + h[(y + 1) % W])) +
               h[(y + 2) % W];
    else
        return (h[(y - H) % W] + h[y % W]) + h[(y + H) % W];
}

constexpr int kRegionRows = 24;
// the depths KJ is built for: a halo of at most 8 on every side, and no
// register spill of any kind (shallower ones spill a few SGPRs)
constexpr bool kj_kb_ok(int W, int KB) {
    return W == 3 ? (KB == 3 || KB == 4 || KB == 6) : (W == 5 && KB >= 2 && KB <= 4);
}

// One wave's region: rows [r0, r0 + RH) x the 64 columns starting at gc - lane;
// p.iters (<= KB) iterations; stores region rows [HL, RH - HL) of lanes
// [HL, 64 - HL) where they lie inside the plane.
template <int W, int KB, int RH>
__device__ __forceinline__ void weighted_region(const JacobiArgs &p, const float *gw, size_t pbase,
                                                int plane_bytes, int lane, int gc, int r0) {
    constexpr int H = W / 2, HL = KB * H;
    static_assert(64 - 2 * HL > 0 && RH - 2 * HL > 0, "halo too deep for the region");
    const int cols = p.cols;
    static_assert(RH <= 32, "the row mask is 32 bits");
    const bool col_in = (unsigned)gc < (unsigned)cols;
    uint32_t rowmask = 0;  // bit r: region row r lies inside the plane (wave-uniform)
#pragma unroll
    for (int r = 0; r < RH; ++r) rowmask |= (uint32_t)((unsigned)(r0 + r) < (unsigned)p.rows) << r;

    // Buffer descriptors over this pair's planes: a byte offset >= the plane
    // size reads 0 / drops the store (hsflow_kernels.hip jacobi_region)
    constexpr int kOOB = 0x7FFFFFF0;
    auto rsrc = [&](const float *q) {
        return __builtin_amdgcn_make_buffer_rsrc((void *)(q + pbase), 0, plane_bytes, 0x00020000);
    };
    float u[RH], v[RH], X[RH], Y[RH], T[RH], g[RH], rden[RH];
    {
        const auto u_rs = rsrc(p.u_in), v_rs = rsrc(p.v_in), g_rs = rsrc(gw);
        const auto gx_rs = rsrc(p.gx), gy_rs = rsrc(p.gy), gt_rs = rsrc(p.gt);
        // a running vector offset: RH scalar row offsets would not fit the SGPRs
        int rowoff = (r0 * cols + gc) * 4;
#pragma unroll
        for (int r = 0; r < RH; ++r) {
            const bool in = col_in && ((rowmask >> r) & 1u);
            const int off = in ? rowoff : kOOB;
            rowoff = launder(rowoff + cols * 4);
            u[r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(u_rs, off, 0, 0));
            v[r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(v_rs, off, 0, 0));
            const float ix = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(gx_rs, off, 0, 0));
            const float iy = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(gy_rs, off, 0, 0));
            const float it = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(gt_rs, off, 0, 0));
            const float gl = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(g_rs, off, 0, 0));
            // outside the plane: weight 1, and alpha^2 = 1 so that the zero
            // gradients give X = Y = T = 0 at alpha = 0 too (alpha2_cols)
            g[r] = in ? gl : 1.0f;
            const float s = __builtin_amdgcn_rsqf(
                fmaf_x(iy, iy, fmaf_x(ix, ix, in ? p.alpha2 : 1.0f)));
            X[r] = ix * s;
            Y[r] = iy * s;
            T[r] = it * s;
        }
    }
    // 1 / S(g) of the pixels inside the plane that have a whole window in the region
    {
        float hg[W], unused[W];
#pragma unroll
        for (int r = 0; r < RH; ++r) {
            hsum2<W>(g[r], g[r], hg[r % W], unused[r % W]);
            rden[r] = 0.0f;
            const int y = r - H;
            // 0 outside the plane: there ubar = vbar = 0 and, with X = Y = T = 0,
            // u' = v' = 0 -- the zero border, kept without a select per iteration
            if (y >= H)
                rden[y] = (col_in && ((rowmask >> y) & 1u)) ? 1.0f / vsum<W>(hg, y) : 0.0f;
        }
    }

    for (int it = 0; it < p.iters; ++it) {
        float hu[W], hv[W];
#pragma unroll
        for (int r = 0; r < RH; ++r) {
            hsum2<W>(g[r] * u[r], g[r] * v[r], hu[r % W], hv[r % W]);
            const int y = r - H;  // the row whose window ends at row r
            if (y >= H) {
                const float ub = vsum<W>(hu, y) * rden[y], vb = vsum<W>(hv, y) * rden[y];
                const float k = fmaf_x(X[y], ub, fmaf_x(Y[y], vb, T[y]));
                u[y] = fmaf_x(-X[y], k, ub);
                v[y] = fmaf_x(-Y[y], k, vb);
            }
            // rows in program order: hoisting every row's horizontal sums
            // would hold them all live (jacobi_region)
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    {
        const auto uo_rs = rsrc(p.u_out), vo_rs = rsrc(p.v_out);
        const bool st_lane = lane >= HL && lane < 64 - HL && col_in;
        int rowoff = launder(((r0 + HL) * cols + gc) * 4);
#pragma unroll
        for (int r = HL; r < RH - HL; ++r) {
            const bool in = st_lane && ((rowmask >> r) & 1u);
            const int off = in ? rowoff : kOOB;
            rowoff = launder(rowoff + cols * 4);
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(u[r]), uo_rs, off, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[r]), vo_rs, off, 0, 0);
        }
    }
}

// grid (ceil(tiles / 4), batch), block 256: one tile per wave
template <int W, int KB>
__global__ __launch_bounds__(256) void hs_jacobi_weighted_kernel(const JacobiArgs p,
                                                                 const float *gw) {
    constexpr int HL = KB * (W / 2);
    constexpr int OX = 64 - 2 * HL, OY = kRegionRows - 2 * HL;
    // XCD-aware block order (hs_jacobi_kernel): each XCD walks a contiguous
    // run of tiles, so the halo its regions re-read hits its L2
    const int nblk = gridDim.x * gridDim.y;
    const int lin = blockIdx.y * gridDim.x + blockIdx.x;
    const int q = nblk >> 3, rem = nblk & 7, xcd = lin & 7;
    const int logical = xcd * q + min(xcd, rem) + (lin >> 3);
    const int pair = logical / gridDim.x;
    const int lane = threadIdx.x & 63;
    const int tile = (logical - pair * gridDim.x) * 4 +
                     __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (tile >= p.tiles_x * p.tiles_y) return;
    const int ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
    const size_t pbase = (size_t)pair * (size_t)p.rows * (size_t)p.cols;
    weighted_region<W, KB, kRegionRows>(p, gw, pbase, p.rows * p.cols * 4, lane,
                                        tx * OX - HL + lane, ty * OY - HL);
}

template <int W, int KB>
hipError_t launch_weighted_t(JacobiArgs a, const float *g, hipStream_t s) {
    if constexpr (!kj_kb_ok(W, KB)) {
        return hipErrorInvalidValue;
    } else {
        constexpr int OX = 64 - KB * (W - 1), OY = kRegionRows - KB * (W - 1);
        a.tiles_x = (a.cols + OX - 1) / OX;
        a.tiles_y = (a.rows + OY - 1) / OY;
        const long ntiles = (long)a.tiles_x * a.tiles_y;
        dim3 grd((unsigned)((ntiles + 3) / 4), (unsigned)a.batch, 1);
        hipLaunchKernelGGL((hs_jacobi_weighted_kernel<W, KB>), grd, dim3(256), 0, s, a, g);
        return hipGetLastError();
    }
}

template <int W>
hipError_t launch_weighted_w(JacobiArgs a, const float *g, int KB, hipStream_t s) {
    switch (KB) {
    case 2: return launch_weighted_t<W, 2>(a, g, s);
    case 3: return launch_weighted_t<W, 3>(a, g, s);
    case 4: return launch_weighted_t<W, 4>(a, g, s);
    case 6: return launch_weighted_t<W, 6>(a, g, s);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t launch_diffusivity(const float *u, const float *v, int rows, int cols, int batch,
                              float lambda, float *g, hipStream_t s) {
    const float inv_l2 = (float)std::min(1.0 / ((double)lambda * (double)lambda), 3.0e38);
    dim3 grd((cols + 63) / 64, (rows + 3) / 4, batch);
    hipLaunchKernelGGL(hs_diffusivity_kernel, grd, dim3(64, 4, 1), 0, s, u, v, rows, cols, inv_l2,
                       g);
    return hipGetLastError();
}

bool weighted_kb_supported(int W, int KB) { return kj_kb_ok(W, KB); }

// measured on the MI355X (scripts/smoothness_timing.py): deeper
// blocking saves passes over the planes, but the recomputed halo grows with it
int weighted_default_kb(int W) { return W == 3 ? 6 : 3; }

hipError_t launch_jacobi_weighted(JacobiArgs a, const float *g, int W, int KB, hipStream_t s) {
    if (W == 3) return launch_weighted_w<3>(a, g, KB, s);
    if (W == 5) return launch_weighted_w<5>(a, g, KB, s);
    return hipErrorInvalidValue;
}

}  // namespace hsflow
