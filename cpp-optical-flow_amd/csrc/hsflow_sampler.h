// hsflow_sampler.h -- the arithmetic KR / KI (hsflow_interp.hip) and their
// colour forms KRC / KIC (hsflow_interp_bgr.hip) share, so that a channel of a
// colour frame gets the bits the grey kernels give its plane: KW's displacement
// split and tap positions, the three lerps, KI's blend and rounding, the times
// of a launch and the quad store of a u8 plane.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hsflow_internal.h"

namespace hsflow {
namespace sampler {

// KW's displacement split as KC restates it (the clamped float comes back for
// the rim test): d (pixels) along an axis of length n is clamped to [-n, n]
// while still a float, so NaN (-> -n), +-inf and huge flows never reach the
// float -> int conversion and every tap index stays in the plane.
__device__ __forceinline__ int split_disp(float &d, int n, float &frac) {
    d = fminf(fmaxf(d, -(float)n), (float)n);
    const float fl = floorf(d);
    frac = d - fl;
    return (int)fl;
}

__device__ __forceinline__ int clampi(int p, int len) { return min(max(p, 0), len - 1); }

// Where a sample at (y + 8 v, x + 8 u) of a rows x cols plane reads: the four
// taps (xa, xb) x (ya, yb), clamped to the plane (xb is xa or xa + 1, yb is ya
// or ya + 1), and the two fractions.
struct Taps {
    int xa, xb, ya, yb;
    float fx, fy;
};

// in: the target is within half a pixel of the frame (KC's test); nearest:
// index in the plane of the source pixel nearest to the target.
__device__ __forceinline__ Taps sample_taps(int rows, int cols, int x, int y, float u, float v,
                                            bool &in, int &nearest) {
    Taps t;
    float dx = 8.0f * u, dy = 8.0f * v;
    const int ix = split_disp(dx, cols, t.fx);
    const int iy = split_disp(dy, rows, t.fy);
    // |ix| <= cols, |iy| <= rows: the sums cannot overflow
    t.xa = clampi(x + ix, cols), t.xb = clampi(x + ix + 1, cols);
    t.ya = clampi(y + iy, rows), t.yb = clampi(y + iy + 1, rows);
    const float tx = (float)x + dx, ty = (float)y + dy;
    in = tx >= -0.5f && tx <= (float)cols - 0.5f && ty >= -0.5f && ty <= (float)rows - 0.5f;
    nearest = (t.fy >= 0.5f ? t.yb : t.ya) * cols + (t.fx >= 0.5f ? t.xb : t.xa);  // < 2^29
    return t;
}

// top row, bottom row, then vertical; exact at fx = fy = 0: zero flow returns
// the pixel itself
template <typename F>
__device__ __forceinline__ F lerp_taps(F ta, F tb, F ba, F bb, float fx, float fy) {
    const F t = ta + (F)fx * (tb - ta);
    const F w = ba + (F)fx * (bb - ba);
    return t + (F)fy * (w - t);
}

// the weight of s1: t where both targets are in the frame or neither is
__device__ __forceinline__ float blend_weight(bool in0, bool in1, float tt) {
    return in0 == in1 ? tt : (in0 ? 0.0f : 1.0f);
}

// selects, never multiplies by zero: the bits of s0 at wt = 0, of s1 at wt = 1
__device__ __forceinline__ float blend(float wt, float s0, float s1) {
    return wt == 0.0f ? s0 : (wt == 1.0f ? s1 : (1.0f - wt) * s0 + wt * s1);
}

// floorf(o + 0.5f) clamped to 0..255; NaN -> 0 (fmaxf drops it)
__device__ __forceinline__ uint32_t round_u8(float o) {
    return (uint32_t)fminf(fmaxf(floorf(o + 0.5f), 0.0f), 255.0f);
}

// the times of one launch, by value in the kernel arguments
struct InterpTimes {
    float t[kInterpMaxTimes];
};

// value of lane `Q` of the caller's quad (DPP quad_perm broadcast)
template <int Q>
__device__ __forceinline__ uint32_t quad_lane(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, Q * 0x55, 0xf, 0xf, true);
}

// One byte per lane into a u8 plane at dst + pk (pk: the lane's pixel, q0 its
// quad's first): an aligned dword per quad where the quad lies in the plane
// and its address allows, else a byte per valid lane.  Every lane of the wave
// calls (the exchange needs them all).
__device__ __forceinline__ void store_quad_u8(uint8_t *dst, int pk, int q0, int plane,
                                              bool valid, uint32_t byte, int lane) {
    const uint32_t quad = byte | quad_lane<1>(byte) << 8 | quad_lane<2>(byte) << 16 |
                          quad_lane<3>(byte) << 24;
    if (q0 + 3 < plane && (((uintptr_t)dst + (size_t)q0) & 3) == 0) {  // q0 >= 0 always
        if ((lane & 3) == 0) *reinterpret_cast<uint32_t *>(dst + q0) = quad;
    } else if (valid) {
        dst[pk] = (uint8_t)byte;
    }
}

}  // namespace sampler
}  // namespace hsflow
