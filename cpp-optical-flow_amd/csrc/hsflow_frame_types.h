// hsflow_frame_types.h -- what the kernels outside the Jacobi files share about
// a frame's element type: the type its arithmetic runs in, the dispatch from a
// dtype code to the element type, and the index clamp of a replicated border.
// Private to the .hip files (KW, KC, KR/KI, KRC/KIC, KN, KM, KG/KJ); the
// Jacobi kernels' sources keep their own copies (their md5 is pinned).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hsflow {

__device__ __forceinline__ int clampi(int p, int len) { return min(max(p, 0), len - 1); }

// double for CV_64FC1 frames (sums and lerps in float64, one rounding), else
// float (as K1)
template <typename T> struct FrameMath { using type = float; };
template <> struct FrameMath<double> { using type = double; };

// f(T{}) for the element type T of dtype code HSFLOW_U8 / F32 / F64 / F16 /
// U16; false for any other code, f not called
template <typename Fn>
bool dispatch_frame_type(int dtype_in, Fn &&f) {
    switch (dtype_in) {
    case 0: f(uint8_t{}); return true;
    case 1: f(float{}); return true;
    case 2: f(double{}); return true;
    case 3: f(_Float16{}); return true;
    case 4: f(uint16_t{}); return true;
    default: return false;
    }
}

}  // namespace hsflow
