// hsflow_median.hip -- median filtering of the flow between warps
// ("Median filtering between warps").
//
//  KM hs_flow_median_kernel<K>   K = 3 or 5, out of place, u and v each on
//     its own.  Output (y, x) of a pair's plane is the element of rank
//     (K^2 - 1) / 2 of the K^2 taps in[clamp(y + j, 0, rows - 1)][clamp(x + i,
//     0, cols - 1)], |i|, |j| <= K / 2 (border replicated, no tap leaves the
//     pair's plane), in the IEEE-754 total order of the f32 bit patterns:
//       key = bits ^ 0xFFFFFFFF if the sign bit is set, else bits | 0x80000000
//     compared as unsigned (-NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN).
//     The keys go through a network of integer min/max only, which permutes
//     them whatever they are: the result is one of the taps bit for bit, NaN
//     payloads included.
//
// Thread map: a thread owns column x and kRun = 4 consecutive rows; a wave is
// 64 consecutive columns, so each of its loads is one coalesced 256-byte row
// piece (the K loads per line differ by one column and hit the same lines in
// cache).  A line is the K taps of one row, sorted once (hsflow_median_net.h)
// and shared by the K outputs of the thread whose windows hold it: kRun + K - 1
// line loads and sorts per kRun outputs, then the selection over K sorted
// lines per output.  158 min/max per output and plane at K = 5 (18 per line
// sort, 140 select), 18 at K = 3 -- what scripts/median_network_check.cpp
// counts after proving both networks on all 2^25 and 2^9 0/1 inputs.
// HBM: 8 B read and 8 B written per pixel (u and v).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hsflow_frame_types.h"
#include "hsflow_internal.h"

#define HSFLOW_NET_FN __device__ __forceinline__
#include "hsflow_median_net.h"

namespace hsflow {
namespace {

struct KeyOps {
    static __device__ __forceinline__ uint32_t mn(uint32_t a, uint32_t b) { return min(a, b); }
    static __device__ __forceinline__ uint32_t mx(uint32_t a, uint32_t b) { return max(a, b); }
};

// f32 bits -> key of the total order, and back
__device__ __forceinline__ uint32_t to_key(uint32_t bits) {
    return bits ^ ((uint32_t)((int32_t)bits >> 31) | 0x80000000u);
}
__device__ __forceinline__ uint32_t from_key(uint32_t key) {
    return key ^ (~(uint32_t)((int32_t)key >> 31) | 0x80000000u);
}

constexpr int kCols = 64, kWaves = 4, kRun = 4;

// grid (ceil(cols / 64), ceil(rows / 16), batch), block (64, 4)
template <int K>
__global__ __launch_bounds__(kCols *kWaves) void hs_flow_median_kernel(
    const uint32_t *__restrict__ u, const uint32_t *__restrict__ v, int rows, int cols,
    uint32_t *__restrict__ u_out, uint32_t *__restrict__ v_out) {
    constexpr int H = K / 2;
    const int x = blockIdx.x * kCols + threadIdx.x;
    const int y0 = (blockIdx.y * kWaves + threadIdx.y) * kRun;  // uniform per wave
    if (x >= cols || y0 >= rows) return;
    const size_t base = (size_t)blockIdx.z * rows * cols;  // rows * cols <= 2^29 - 4
    int xs[K];
#pragma unroll
    for (int i = 0; i < K; ++i) xs[i] = clampi(x + i - H, cols);

#pragma unroll 1
    for (int c = 0; c < 2; ++c) {
        const uint32_t *in = (c ? v : u) + base;
        uint32_t *out = (c ? v_out : u_out) + base;
        uint32_t win[K][K];  // the window's lines, each ascending
        auto load_line = [&](uint32_t(&line)[K], int y) {
            const uint32_t *row = in + (size_t)clampi(y, rows) * cols;
#pragma unroll
            for (int i = 0; i < K; ++i) line[i] = to_key(row[xs[i]]);
            hsflow_net::sort_line<KeyOps>(line);
        };
#pragma unroll
        for (int j = 0; j < K - 1; ++j) load_line(win[j], y0 - H + j);
#pragma unroll
        for (int p = 0; p < kRun; ++p) {
            // rows past the plane's last repeat it: loaded, never stored
            load_line(win[K - 1], y0 + p + H);
            const uint32_t med = hsflow_net::median_of_lines<KeyOps>(win);
            if (y0 + p < rows) out[(size_t)(y0 + p) * cols + x] = from_key(med);
#pragma unroll
            for (int j = 0; j < K - 1; ++j)
#pragma unroll
                for (int i = 0; i < K; ++i) win[j][i] = win[j + 1][i];
        }
    }
}

}  // namespace

hipError_t launch_median(const float *u, const float *v, int rows, int cols, int batch, int ksize,
                         float *u_out, float *v_out, hipStream_t s) {
    dim3 blk(kCols, kWaves, 1);
    dim3 grd((cols + kCols - 1) / kCols, (rows + kWaves * kRun - 1) / (kWaves * kRun), batch);
    const uint32_t *ui = (const uint32_t *)u, *vi = (const uint32_t *)v;
    uint32_t *uo = (uint32_t *)u_out, *vo = (uint32_t *)v_out;
    if (ksize == 3)
        hipLaunchKernelGGL(hs_flow_median_kernel<3>, grd, blk, 0, s, ui, vi, rows, cols, uo, vo);
    else if (ksize == 5)
        hipLaunchKernelGGL(hs_flow_median_kernel<5>, grd, blk, 0, s, ui, vi, rows, cols, uo, vo);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace hsflow
