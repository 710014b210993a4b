// hsflow_frame_policy.h -- what a frame's pixel is, for the kernels that are
// written once over a frame policy: KI / KIP (hsflow_sampler.h, launched from
// hsflow_interp.hip and hsflow_interp_bgr.hip) and KF (hsflow_fallback.hip).
// GreyFrame<T>: one element of T per pixel; BgrFrame<Wide>: three interleaved
// bytes, with KRC's tap loads and the quad store of a u8 BGR plane;
// ChromaFrame<Layout, Wide>: the U and V samples of a 4:2:0 frame, for KIY
// (hsflow_yuv.hip), which has a kernel of its own over KI's pieces, and
// ChromaFrame16<Layout, Wide>, the same of 16-bit samples.  Device
// code only; every including file gets its own copy (anonymous namespace).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "hsflow_sampler.h"

namespace hsflow {
namespace {

using namespace sampler;

// ---- KI: hs_frame_interp_kernel on a grey frame of T
template <typename T>
struct GreyFrame {
    using Elem = T;
    static constexpr int kChannels = 1;
    // six blocks of four waves are resident per CU (64 to 68 VGPRs: 7 waves
    // per SIMD; the cap predates that count).  16-bit frames with their pair
    // stores: 77 (KI) and 91 (KIP) VGPRs, six and five waves per SIMD, so five
    static constexpr int kBlocksPerCu = std::is_same<T, uint16_t>::value ? 5 : 6;
    using Px = float;
    static __device__ __forceinline__ float sample(const T *__restrict__ img, int cols,
                                                   const Taps &t) {
        return (float)sample_plane(img, cols, t);
    }
    static __device__ __forceinline__ void store_f32(void *out, size_t px, float o) {
        ((float *)out)[px] = o;
    }
    static __device__ __forceinline__ void store_u8(void *out, size_t obase, int pk, int q0,
                                                    bool whole, bool valid, float o, int lane) {
        store_quad_u8((uint8_t *)out + obase, pk, q0, whole, valid, round_u8(o), lane);
    }
    // 16-bit frames come back as 16-bit frames: pairs of lanes, one dword each
    static constexpr bool kU16Out = std::is_same<T, uint16_t>::value;
    static __device__ __forceinline__ void store_u16(void *out, size_t obase, int pk, int plane,
                                                     float o, int lane) {
        store_pair_u16((uint16_t *)out + obase, pk, plane, round_u16(o), lane);
    }
};

using Bgr = Pixel<3>;

__device__ __forceinline__ uint32_t load_u32_unaligned(const uint8_t *p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
__device__ __forceinline__ uint32_t load_u16_unaligned(const uint8_t *p) {
    uint16_t v;
    __builtin_memcpy(&v, p, 2);
    return v;
}

// the taps xa and xb of one row of a BGR plane (row: its first byte)
template <bool Wide>
__device__ __forceinline__ void row_taps(const uint8_t *__restrict__ row, int xa, int xb, Bgr &a,
                                         Bgr &b) {
    const uint8_t *pa = row + (size_t)xa * 3;
    if (Wide && xb != xa) {  // xb == xa + 1: six bytes of this row
        const uint32_t lo = load_u32_unaligned(pa), hi = load_u16_unaligned(pa + 4);
        a.c[0] = (float)(lo & 0xFF), a.c[1] = (float)((lo >> 8) & 0xFF);
        a.c[2] = (float)((lo >> 16) & 0xFF), b.c[0] = (float)(lo >> 24);
        b.c[1] = (float)(hi & 0xFF), b.c[2] = (float)(hi >> 8);
    } else {
        const uint8_t *pb = row + (size_t)xb * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) a.c[c] = (float)pa[c], b.c[c] = (float)pb[c];
    }
}

// img (one pair's BGR plane) at the taps `t`: KR's sample, per channel
template <bool Wide>
__device__ __forceinline__ Bgr sample_bgr(const uint8_t *__restrict__ img, int cols,
                                          const Taps &t) {
    Bgr ta, tb, ba, bb, r;
    row_taps<Wide>(img + (size_t)t.ya * cols * 3, t.xa, t.xb, ta, tb);
    row_taps<Wide>(img + (size_t)t.yb * cols * 3, t.xa, t.xb, ba, bb);
#pragma unroll
    for (int c = 0; c < 3; ++c) r.c[c] = lerp_taps(ta.c[c], tb.c[c], ba.c[c], bb.c[c], t.fx, t.fy);
    return r;
}

// Three bytes per lane (bgr: B | G << 8 | R << 16) into a u8 BGR plane: quad:
// the first byte of the lane's quad of pixels, whole: its four pixels lie in
// the plane.  Three aligned dwords per quad where the address allows, else
// three bytes per valid lane.  Every lane of the wave calls.
__device__ __forceinline__ void store_quad_bgr_u8(uint8_t *quad, bool whole, bool valid,
                                                  uint32_t bgr, int lane) {
    const uint32_t p0 = quad_lane<0>(bgr), p1 = quad_lane<1>(bgr), p2 = quad_lane<2>(bgr),
                   p3 = quad_lane<3>(bgr);
    const int j = lane & 3;
    if (whole && ((uintptr_t)quad & 3) == 0) {
        // bytes: B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3
        const uint32_t w = j == 0 ? (p0 | p1 << 24) : j == 1 ? (p1 >> 8 | p2 << 16)
                                                             : (p2 >> 16 | p3 << 8);
        if (j < 3) reinterpret_cast<uint32_t *>(quad)[j] = w;
    } else if (valid) {
        uint8_t *d = quad + j * 3;
        d[0] = (uint8_t)bgr, d[1] = (uint8_t)(bgr >> 8), d[2] = (uint8_t)(bgr >> 16);
    }
}

__device__ __forceinline__ uint32_t pack_u8(const Bgr &o) {
    return round_u8(o.c[0]) | round_u8(o.c[1]) << 8 | round_u8(o.c[2]) << 16;
}

// one f32 pixel: a 12-byte store (the plane is 4-byte aligned)
struct alignas(4) Float3 {
    float c[3];
};

// ---- KIC: hs_frame_interp_kernel on a BGR frame
template <bool Wide>
struct BgrFrame {
    using Elem = uint8_t;
    static constexpr int kChannels = 3;
    static constexpr bool kU16Out = false;
    using Px = Bgr;
    // 84 VGPRs with wide loads: five waves per SIMD, five blocks per CU (80
    // with byte loads, which would let a sixth in; one cap for both forms)
    static constexpr int kBlocksPerCu = 5;
    static __device__ __forceinline__ Bgr sample(const uint8_t *__restrict__ img, int cols,
                                                 const Taps &t) {
        return sample_bgr<Wide>(img, cols, t);
    }
    static __device__ __forceinline__ void store_f32(void *out, size_t px, const Bgr &o) {
        reinterpret_cast<Float3 *>(out)[px] = Float3{{o.c[0], o.c[1], o.c[2]}};
    }
    static __device__ __forceinline__ void store_u8(void *out, size_t obase, int, int q0,
                                                    bool whole, bool valid, const Bgr &o, int lane) {
        store_quad_bgr_u8((uint8_t *)out + (obase + (size_t)q0) * 3, whole, valid, pack_u8(o),
                          lane);
    }
};

// ---- KIY: hs_chroma_interp_kernel on the chroma of a 4:2:0 frame
// (hsflow_yuv.hip).  A pair's chroma is 2 * plane bytes, plane = rc * cc
// samples of U and of V: I420 [2][rc][cc], U then V; NV12 [rc][cc][2].  An
// output frame has the same layout in u8 or f32.  One sample of both channels
// is a Pixel<2>, U in c[0]; the taps are those of one chroma plane.
constexpr int kYuvI420 = 1, kYuvNv12 = 2;  // HSFLOW_YUV_I420, HSFLOW_YUV_NV12
using Uv = Pixel<2>;

// one f32 sample of both channels: an 8-byte store (the plane is 4-byte aligned)
struct alignas(4) Float2 {
    float c[2];
};

// sample pk of output frame `frame` (pair * nt + time) of the whole f32 output
template <int Layout>
__device__ __forceinline__ void store_uv_f32(void *out, size_t frame, int plane, int pk,
                                             const Uv &o) {
    if constexpr (Layout == kYuvI420) {
        float *d = (float *)out + frame * 2 * plane;
        d[pk] = o.c[0], d[(size_t)plane + pk] = o.c[1];
    } else {
        reinterpret_cast<Float2 *>(out)[frame * plane + pk] = Float2{{o.c[0], o.c[1]}};
    }
}

// What KIY asks of a chroma policy:
//   Elem, kIntOut       the sample type; the output kind of that type
//   at(img, plane, p)   sample p of a pair's chroma as KI reads it at zero flow
//   sample(img, plane, cc, taps)   KR's sample of the U and of the V plane
//   store_f32(out, frame, plane, pk, o)
//   store_int(out, frame, plane, pk, q0, whole, valid, o, lane)   into an
//       output of Elem; every lane of the wave calls
//   kBlocksPerCu        the grid's cap

// Wide (NV12 only): a row's two taps as one unaligned dword where xb == xa + 1
template <int Layout, bool Wide>
struct ChromaFrame {
    using Elem = uint8_t;
    static constexpr int kIntOut = kOutU8;
    using Px = Uv;
    // 81 (NV12) to 90 (I420) VGPRs: five waves per SIMD, five blocks of four
    // waves per CU, as KIC; KIYP 111 (NV12) to 120 (I420): four
    static constexpr int kBlocksPerCu = 5, kProjBlocksPerCu = 4;
    // img: a pair's chroma; sample p of the plane as KI reads it at zero flow
    static __device__ __forceinline__ Uv at(const uint8_t *__restrict__ img, int plane, int p) {
        if constexpr (Layout == kYuvI420)
            return Uv{{(float)img[p], (float)img[(size_t)plane + p]}};
        else
            return Uv{{(float)img[2 * (size_t)p], (float)img[2 * (size_t)p + 1]}};
    }
    static __device__ __forceinline__ void row_taps(const uint8_t *__restrict__ row, int xa,
                                                    int xb, Uv &a, Uv &b) {
        const uint8_t *pa = row + 2 * (size_t)xa;
        if (Wide && xb != xa) {  // xb == xa + 1: four bytes of this row
            const uint32_t w = load_u32_unaligned(pa);
            a.c[0] = (float)(w & 0xFF), a.c[1] = (float)((w >> 8) & 0xFF);
            b.c[0] = (float)((w >> 16) & 0xFF), b.c[1] = (float)(w >> 24);
        } else {
            const uint8_t *pb = row + 2 * (size_t)xb;
            a.c[0] = (float)pa[0], a.c[1] = (float)pa[1];
            b.c[0] = (float)pb[0], b.c[1] = (float)pb[1];
        }
    }
    // KR's sample of the U and of the V plane (cc columns) at the taps `t`
    static __device__ __forceinline__ Uv sample(const uint8_t *__restrict__ img, int plane, int cc,
                                                const Taps &t) {
        if constexpr (Layout == kYuvI420) {
            return Uv{{(float)sample_plane(img, cc, t), (float)sample_plane(img + plane, cc, t)}};
        } else {
            Uv ta, tb, ba, bb, r;
            row_taps(img + 2 * (size_t)t.ya * cc, t.xa, t.xb, ta, tb);
            row_taps(img + 2 * (size_t)t.yb * cc, t.xa, t.xb, ba, bb);
#pragma unroll
            for (int c = 0; c < 2; ++c)
                r.c[c] = lerp_taps(ta.c[c], tb.c[c], ba.c[c], bb.c[c], t.fx, t.fy);
            return r;
        }
    }
    static __device__ __forceinline__ void store_f32(void *out, size_t frame, int plane, int pk,
                                                     const Uv &o) {
        store_uv_f32<Layout>(out, frame, plane, pk, o);
    }
    // the same into a u8 output, through quads of lanes (q0: the quad's first
    // sample, whole: its four lie in the plane): I420 as store_quad_u8 of each
    // plane; NV12 the quad's eight bytes as two dwords where their address
    // allows, else two bytes per valid lane.  Every lane of the wave calls.
    static __device__ __forceinline__ void store_int(void *out, size_t frame, int plane, int pk,
                                                     int q0, bool whole, bool valid, const Uv &o,
                                                     int lane) {
        uint8_t *d = (uint8_t *)out + frame * 2 * plane;
        if constexpr (Layout == kYuvI420) {
            store_quad_u8(d, pk, q0, whole, valid, round_u8(o.c[0]), lane);
            store_quad_u8(d + plane, pk, q0, whole, valid, round_u8(o.c[1]), lane);
        } else {
            const uint32_t uv = round_u8(o.c[0]) | round_u8(o.c[1]) << 8;
            const uint32_t lo = quad_lane<0>(uv) | quad_lane<1>(uv) << 16;
            const uint32_t hi = quad_lane<2>(uv) | quad_lane<3>(uv) << 16;
            uint8_t *quad = d + 2 * (size_t)q0;
            const int j = lane & 3;
            if (whole && ((uintptr_t)quad & 3) == 0) {
                if (j < 2) reinterpret_cast<uint32_t *>(quad)[j] = j == 0 ? lo : hi;
            } else if (valid) {
                quad[2 * j] = (uint8_t)uv, quad[2 * j + 1] = (uint8_t)(uv >> 8);
            }
        }
    }
};

// ---- KIY on 16-bit samples (yuv420p10le .. p16le: I420; P010 .. P016: NV12).
// A sample is its value, 0 .. 65535.  The planes are 2-byte aligned only in
// general, so the one dword that holds an NV12 sample's U and V is loaded and
// stored as an unaligned dword.
__device__ __forceinline__ uint64_t load_u64_unaligned(const uint16_t *p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

__device__ __forceinline__ Uv split_uv16(uint32_t w) {
    return Uv{{(float)(w & 0xFFFF), (float)(w >> 16)}};
}

// Wide (NV12 only): a row's two taps as one unaligned 8-byte load where
// xb == xa + 1
template <int Layout, bool Wide>
struct ChromaFrame16 {
    using Elem = uint16_t;
    static constexpr int kIntOut = kOutU16;
    using Px = Uv;
    // KIY: 66 VGPRs (NV12, seven waves per SIMD; the cap stays the 8-bit
    // form's five) and 100 (I420, four waves: four blocks); KIYP: 96 to 98
    // (NV12, four to five waves: four blocks) and 130 (I420, three)
    static constexpr int kBlocksPerCu = Layout == kYuvI420 ? 4 : 5;
    static constexpr int kProjBlocksPerCu = Layout == kYuvI420 ? 3 : 4;
    static __device__ __forceinline__ Uv at(const uint16_t *__restrict__ img, int plane, int p) {
        if constexpr (Layout == kYuvI420)
            return Uv{{(float)img[p], (float)img[(size_t)plane + p]}};
        else
            return split_uv16(load_u32_unaligned((const uint8_t *)(img + 2 * (size_t)p)));
    }
    static __device__ __forceinline__ void row_taps(const uint16_t *__restrict__ row, int xa,
                                                    int xb, Uv &a, Uv &b) {
        const uint16_t *pa = row + 2 * (size_t)xa;
        if (Wide && xb != xa) {  // xb == xa + 1: eight bytes of this row
            const uint64_t w = load_u64_unaligned(pa);
            a = split_uv16((uint32_t)w), b = split_uv16((uint32_t)(w >> 32));
        } else {
            a = split_uv16(load_u32_unaligned((const uint8_t *)pa));
            b = split_uv16(load_u32_unaligned((const uint8_t *)(row + 2 * (size_t)xb)));
        }
    }
    static __device__ __forceinline__ Uv sample(const uint16_t *__restrict__ img, int plane,
                                                int cc, const Taps &t) {
        if constexpr (Layout == kYuvI420) {
            return Uv{{(float)sample_plane(img, cc, t), (float)sample_plane(img + plane, cc, t)}};
        } else {
            Uv ta, tb, ba, bb, r;
            row_taps(img + 2 * (size_t)t.ya * cc, t.xa, t.xb, ta, tb);
            row_taps(img + 2 * (size_t)t.yb * cc, t.xa, t.xb, ba, bb);
#pragma unroll
            for (int c = 0; c < 2; ++c)
                r.c[c] = lerp_taps(ta.c[c], tb.c[c], ba.c[c], bb.c[c], t.fx, t.fy);
            return r;
        }
    }
    static __device__ __forceinline__ void store_f32(void *out, size_t frame, int plane, int pk,
                                                     const Uv &o) {
        store_uv_f32<Layout>(out, frame, plane, pk, o);
    }
    // into a u16 output: I420 as store_pair_u16 of each plane; NV12 the lane's
    // U and V as one dword, unaligned where the output is.  Every lane calls.
    static __device__ __forceinline__ void store_int(void *out, size_t frame, int plane, int pk,
                                                     int, bool, bool valid, const Uv &o,
                                                     int lane) {
        uint16_t *d = (uint16_t *)out + frame * 2 * plane;
        if constexpr (Layout == kYuvI420) {
            store_pair_u16(d, pk, plane, round_u16(o.c[0]), lane);
            store_pair_u16(d + plane, pk, plane, round_u16(o.c[1]), lane);
        } else if (valid) {
            const uint32_t uv = round_u16(o.c[0]) | round_u16(o.c[1]) << 16;
            __builtin_memcpy(d + 2 * (size_t)pk, &uv, 4);
        }
    }
};

}  // namespace
}  // namespace hsflow
