// hsflow_prefilter.hip -- brightness-robust prefilter of the frames
// ("Brightness-robust prefilter").
//
//  KN hs_prefilter_kernel   one launch per call, no workspace.  Per plane,
//     with G the separable Gaussian of radius r (weights w[0..r] in the kernel
//     arguments, reflect-101 folded with period 2 (n - 1)):
//       v   = I - G*I
//       out = v                                        (mode 1, high-pass)
//       out = scale v / (sqrt(G*(v v)) + eps)          (mode 2, normalise)
//     u8, f16 and f32 frames in f32; f64 frames in f64, rounded once.
//
// Thread map: a block of TW + 64 threads owns a strip of TW output columns and a
// segment of seg_rows output rows of one plane and streams the rows downwards
// once.  Mode 2 is two dependent blurs, so the strip carries a halo of 2r
// columns of I (r of them for v) and the segment a lead-in of 2r rows.  The
// stages run as a software pipeline, each on what the steps before left in
// LDS, so a step needs one barrier, and the loads from memory are issued a
// step before their values are used.  Step s:
//   L  row s + 1 of I -> registers, into rowbuf[(s + 1) & 1] at the step's end
//      (TW + 4r columns)
//   H  ringA[s] = horizontal blur of rowbuf[s & 1]           (TW + 2r columns)
//   V  yv = s - 1 - r:  v = I - vertical blur of ringA around yv -> ringB[yv]
//      (mode 1: stored to out, nothing below runs)
//   C  yc = s - 2 - r:  ringC[yc] = horizontal blur of ringB[yc]^2  (TW columns)
//   O  yo = s - 3 - 2r: out = scale ringB[yo] / (sqrt(vertical blur of ringC
//      around yo) + eps)
// Row y lives in slot y mod the ring's height: 2r + 2 rows for ringA and ringC
// (the 2r + 1 a blur reads and the one being written), r + 3 for ringB (from
// the numerator's row yo to the row V writes).  A reflected index lies within r
// of the index it is reflected for and inside the plane, so every tap is a row
// the ring still holds and a column the strip computed; the row buffers and
// ringB hold the reflected columns themselves (loaded, or computed, at the
// folded column), so only the vertical blurs fold, near the top and bottom.
// The radius is a template argument (r = ceil(3 sigma) = 2..15 for sigma in
// [0.5, 5]): the tap loops are unrolled and the weights sit in scalar
// registers.  Every output pixel runs the same operations in the same order
// whatever strip and segment it falls in, so the bits do not depend on the
// grid.  HBM: the input's 1, 2, 4 or 8 B read (each row once per strip and
// segment that needs it, plus the centre pixel again from L2) and 4 B written
// per pixel.
// LDS at r = 15: 48.3 KB (f32 math, TW = 128), 54.7 KB (f64 math, TW = 64).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "hsflow_frame_types.h"
#include "hsflow_internal.h"

namespace hsflow {
namespace {

struct Weights {
    float w[kPrefilterMaxRadius + 1];
};

// reflect-101 of any index: period 2 (n - 1), n = 1 -> 0
__device__ __forceinline__ int fold101(int p, int n) {
    if (n == 1) return 0;
    const int period = 2 * (n - 1);
    p %= period;
    if (p < 0) p += period;
    return p < n ? p : period - p;
}

__device__ __forceinline__ float fma_t(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_t(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float sqrt_t(float a) { return __builtin_sqrtf(a); }
__device__ __forceinline__ double sqrt_t(double a) { return __builtin_sqrt(a); }

// LDS elements of one block: two row buffers, ringA and for mode 2 ringB, ringC
__host__ __device__ constexpr int lds_elems(int TW, int r, bool norm) {
    const int D = norm ? r : 0;
    const int WI = TW + 2 * (r + D), WH = TW + 2 * D;
    return 2 * WI + (2 * r + 2) * WH + (norm ? (r + 3) * WH + (2 * r + 2) * TW : 0);
}

// sum over |j| <= r of w[|j|] ring[row fold(y + j)][col], the rows of a ring of
// `height` slots of `stride` elements; y - r..y + r inside the plane walks the
// slots, else each row is folded
template <int R, typename A>
__device__ __forceinline__ A vblur(const A *ring, int height, int stride, int col, int y, int rows,
                                   const Weights &W) {
    constexpr int r = R;
    const int s0 = y % height;
    A acc = (A)W.w[0] * ring[s0 * stride + col];
    if (y - r >= 0 && y + r < rows) {
        int up = s0, dn = s0;
#pragma unroll
        for (int i = 1; i <= r; ++i) {
            up = up == 0 ? height - 1 : up - 1;
            dn = dn + 1 == height ? 0 : dn + 1;
            acc = fma_t((A)W.w[i], ring[up * stride + col] + ring[dn * stride + col], acc);
        }
    } else {
#pragma unroll 1
        for (int i = 1; i <= r; ++i) {
            const int up = fold101(y - i, rows) % height, dn = fold101(y + i, rows) % height;
            acc = fma_t((A)W.w[i], ring[up * stride + col] + ring[dn * stride + col], acc);
        }
    }
    return acc;
}

// grid (ceil(cols / TW), ceil(rows / seg_rows), batch), block TW + 64 (every
// stage is at most that wide: 4r <= 60); dynamic LDS: lds_elems(TW, r, MODE == 2)
// elements of the math type
template <typename T, int TW, int MODE, int R>
__global__ __launch_bounds__(TW + 64) void hs_prefilter_kernel(const T *__restrict__ I, int rows,
                                                               int cols, Weights W, float eps,
                                                               float scale, int seg_rows,
                                                               float *__restrict__ out) {
    using A = typename FrameMath<T>::type;
    extern __shared__ __align__(8) unsigned char lds_raw[];
    A *lds = (A *)lds_raw;
    constexpr bool kNorm = MODE == 2;
    constexpr int r = R;
    constexpr int D = kNorm ? r : 0;  // halo of v, columns and rows
    constexpr int WI = TW + 2 * (r + D), WH = TW + 2 * D;
    constexpr int MA = 2 * r + 2, MB = r + 3;
    static_assert(WI <= TW + 64, "a stage is wider than the block");
    A *rowbuf = lds, *ringA = rowbuf + 2 * WI;
    A *ringB = ringA + MA * WH, *ringC = ringB + MB * WH;  // mode 2 only

    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * TW;
    const int ys = blockIdx.y * seg_rows, ye = min(rows, ys + seg_rows);
    const size_t base = (size_t)blockIdx.z * rows * cols;  // rows * cols <= 2^29 - 4
    const T *in = I + base;
    float *o = out + base;
    // This thread's column of a row buffer (cI), of a ringA / ringB row (cH) and
    // of the strip (cO).  The row buffers and ringB hold the plane continued by
    // reflection r columns past either edge -- element cI is I at fold101(cI),
    // element cH of ringB is v at fold101(cH) -- so no horizontal tap folds.
    const int cI = x0 - r - D + tid, cH = x0 - D + tid, cO = x0 + tid;
    const int fI = fold101(cI, cols), fH = fold101(cH, cols);
    const bool okI = tid < WI && cI >= -r && cI < cols + r;
    const bool okH = tid < WH && cH >= 0 && cH < cols;
    // v is computed at the reflected columns too where C reads them (mode 2);
    // fH lies in the strip's ringA range then: within r of an edge column
    const bool okV = kNorm ? tid < WH && cH >= -r && cH < cols + r : okH;
    const bool okO = tid < TW && cO < cols;
    const int lI = tid + r;           // cH's element of a row buffer (tid < WH)
    const int hV = fH - (x0 - D);     // fH's element of a ringA row
    // rows of I (blurred horizontally) and of v this segment needs
    const int h_lo = max(0, ys - r - D), h_hi = min(rows, ye + r + D);
    const int v_lo = max(0, ys - D), v_hi = min(rows, ye + D);
    const int s_first = ys - r - D;

    // Loads run one step ahead of their use, so a step never waits for memory:
    // `pre` is row s + 1 of I, put into its row buffer at the end of step s;
    // `centre` is I at the pixel whose v the next step computes.
    A pre = (A)0, centre = (A)0, centre_next = (A)0;
    if (okI && s_first >= h_lo && s_first < h_hi)
        rowbuf[(s_first & 1) * WI + tid] = (A)in[(size_t)s_first * cols + fI];
    __syncthreads();

    for (int s = s_first; s < ye + r + D + (kNorm ? 3 : 1); ++s) {
        const bool load_row = okI && s + 1 >= h_lo && s + 1 < h_hi;
        if (load_row) pre = (A)in[(size_t)(s + 1) * cols + fI];
        const int yv_next = s - r;
        if (okV && yv_next >= v_lo && yv_next < v_hi)
            centre_next = (A)in[(size_t)yv_next * cols + fH];

        // H: row s blurred horizontally
        if (okH && s >= h_lo && s < h_hi) {
            const A *src = rowbuf + (s & 1) * WI;
            A acc = (A)W.w[0] * src[lI];
#pragma unroll
            for (int i = 1; i <= r; ++i)
                acc = fma_t((A)W.w[i], src[lI - i] + src[lI + i], acc);
            ringA[(s % MA) * WH + tid] = acc;
        }
        // V: v of row yv
        const int yv = s - 1 - r;
        if (okV && yv >= v_lo && yv < v_hi) {
            const A v = centre - vblur<R>(ringA, MA, WH, hV, yv, rows, W);
            if constexpr (kNorm)
                ringB[(yv % MB) * WH + tid] = v;
            else
                o[(size_t)yv * cols + cH] = (float)v;
        }
        if constexpr (kNorm) {
            // C: v^2 of row yc blurred horizontally
            const int yc = s - 2 - r;
            if (okO && yc >= v_lo && yc < v_hi) {
                const int lh = tid + D;
                const A *vb = ringB + (yc % MB) * WH;
                A acc = (A)W.w[0] * (vb[lh] * vb[lh]);
#pragma unroll
                for (int i = 1; i <= r; ++i) {
                    const A a = vb[lh - i], b = vb[lh + i];
                    acc = fma_t((A)W.w[i], fma_t(a, a, b * b), acc);
                }
                ringC[(yc % MA) * TW + tid] = acc;
            }
            // O: the output row yo
            const int yo = s - 3 - 2 * r;
            if (okO && yo >= ys && yo < ye) {
                const A sum = vblur<R>(ringC, MA, TW, tid, yo, rows, W);
                const A v = ringB[(yo % MB) * WH + tid + D];
                o[(size_t)yo * cols + cO] = (float)(((A)scale * v) / (sqrt_t(sum) + (A)eps));
            }
        }
        if (load_row) rowbuf[((s + 1) & 1) * WI + tid] = pre;
        centre = centre_next;
        __syncthreads();
    }
}

template <typename T, int TW, int R>
void launch_r(const void *I, int rows, int cols, int batch, int mode, int r, const Weights &W,
              float eps, float scale, float *out, hipStream_t s) {
    using A = typename FrameMath<T>::type;
    const int D = mode == 2 ? r : 0;
    const size_t lds = sizeof(A) * (size_t)lds_elems(TW, r, mode == 2);
    // segments: about four blocks per compute unit, none shorter than its own
    // lead-in of 2 (r + D) rows (or 32)
    const int strips = (cols + TW - 1) / TW;
    const int min_seg = std::max(32, 2 * (r + D));
    const long long want = 4ll * device_cus() / ((long long)strips * batch);
    int nseg = (int)std::max(1ll, std::min<long long>(want, (rows + min_seg - 1) / min_seg));
    const int seg_rows = (rows + nseg - 1) / nseg;
    nseg = (rows + seg_rows - 1) / seg_rows;
    dim3 blk(TW + 64, 1, 1), grd(strips, nseg, batch);
    if (mode == 2)
        hipLaunchKernelGGL((hs_prefilter_kernel<T, TW, 2, R>), grd, blk, lds, s, (const T *)I, rows,
                           cols, W, eps, scale, seg_rows, out);
    else
        hipLaunchKernelGGL((hs_prefilter_kernel<T, TW, 1, R>), grd, blk, lds, s, (const T *)I, rows,
                           cols, W, eps, scale, seg_rows, out);
}

// every radius of sigma in [0.5, 5] is compiled in: r = ceil(3 sigma) = 2..15
template <typename T, int TW>
void launch_t(const void *I, int rows, int cols, int batch, int mode, int r, const Weights &W,
              float eps, float scale, float *out, hipStream_t s) {
#define HSFLOW_KN_RADIUS(R_) \
    case R_: launch_r<T, TW, R_>(I, rows, cols, batch, mode, r, W, eps, scale, out, s); break
    switch (r) {
        HSFLOW_KN_RADIUS(2);
        HSFLOW_KN_RADIUS(3);
        HSFLOW_KN_RADIUS(4);
        HSFLOW_KN_RADIUS(5);
        HSFLOW_KN_RADIUS(6);
        HSFLOW_KN_RADIUS(7);
        HSFLOW_KN_RADIUS(8);
        HSFLOW_KN_RADIUS(9);
        HSFLOW_KN_RADIUS(10);
        HSFLOW_KN_RADIUS(11);
        HSFLOW_KN_RADIUS(12);
        HSFLOW_KN_RADIUS(13);
        HSFLOW_KN_RADIUS(14);
        HSFLOW_KN_RADIUS(15);
    default: break;  // launch_prefilter has checked the radius
    }
#undef HSFLOW_KN_RADIUS
}

}  // namespace

hipError_t launch_prefilter(const void *I, int dtype_in, int rows, int cols, int batch, int mode,
                            int radius, const float *weights, float eps, float scale, float *out,
                            hipStream_t s) {
    if ((mode != 1 && mode != 2) || radius < 2 || radius > kPrefilterMaxRadius)
        return hipErrorInvalidValue;
    Weights W{};
    for (int i = 0; i <= radius; ++i) W.w[i] = weights[i];
    const bool known = dispatch_frame_type(dtype_in, [&](auto t) {
        using T = decltype(t);
        // f64 math: half the strip's width in about the same LDS
        constexpr int TW = sizeof(typename FrameMath<T>::type) == 8 ? 64 : 128;
        launch_t<T, TW>(I, rows, cols, batch, mode, radius, W, eps, scale, out, s);
    });
    if (!known) return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace hsflow
