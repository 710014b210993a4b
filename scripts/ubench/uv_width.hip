// K4's memory traffic with K4's geometry and no arithmetic: what can the
// shape of the memory instructions buy?  (the pass is held
// by memory; this bounds a change of the (u, v) layout between passes.)
//
// The headline leg's pass, 1080p x 8 at w 5 / KB 6: 19 strips x 13 segments
// x 8 pairs = 1976 waves in 64-thread workgroups, held to two per SIMD (20 KB
// of LDS per workgroup: 8 fit a CU's 160 KB), XCD-remapped as in
// hs_jacobi_strip_kernel.  A wave streams the 84 + 24 rows of its segment
// (even segments downwards, odd ones upwards), 128 columns per row, loads
// three rows ahead and stores the 104 interior columns of the row that K4's
// last stage would finish at that step, 12 rows behind.  Rows and columns
// outside the image are out-of-range buffer accesses, as in K4.  Input and
// output planes swap from launch to launch; the working set is the real one
// (12 B/px in + 8 B/px out over 16.6 Mpx = 332 MB).
//
//   form (a)  five planes, 8 B per lane: loads u, v, g; stores u', v'
//   form (b)  (u, v) interleaved {u0, u1, v0, v1}, 16 B per lane: loads uv, g;
//             stores uv'  (element (r, c) of field f at float index
//             4 (r P + c / 2) + 2 f + (c & 1), P = cols / 2)
//   form (c)  the same 16-byte groups kept in the two planes they replace, as
//             K4 has them: even rows in the u plane, odd rows in the v plane,
//             row r at the planar byte offset of row r & ~1
//
// The forms run in alternating rounds; the time is per launch, by events
// over `reps` launches.  No kernel writes outside its planes: every offset is
// either inside [0, plane_bytes) of a pair's plane or dropped by the range
// check of the buffer resource, whose size is the plane's.
//
//   hipcc --offload-arch=gfx950 -O3 -o uv_width uv_width.hip && ./uv_width
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <vector>

typedef unsigned u2v __attribute__((ext_vector_type(2)));
typedef unsigned u4v __attribute__((ext_vector_type(4)));

constexpr int kRows = 1080, kCols = 1920, kBatch = 8;
constexpr int kSeg = 84, kHaloR = 12, kHaloC = 12, kOut = 128 - 2 * kHaloC;  // KB 6, w 5
constexpr int kStrips = (kCols + kOut - 1) / kOut, kSegs = (kRows + kSeg - 1) / kSeg;
constexpr int kWaves = kStrips * kSegs * kBatch;
constexpr int kD = 3;  // rows in flight
constexpr int kOOB = 0x7FFFFFF0;
constexpr size_t kPx = size_t(kRows) * kCols;

struct Args {
    const unsigned *u, *v, *uv, *g;
    unsigned *uo, *vo, *uvo, *sink;
};

// IL: 0 = (a), 1 = (b), 2 = (c)
template <int IL> struct Row { u4v uv; u2v g; };
template <> struct Row<0> { u2v u, v, g; };

template <int IL>
__global__ __launch_bounds__(64) void stream(const Args p) {
    extern __shared__ unsigned hold[];  // occupancy only
    const int nblk = gridDim.x, lin = blockIdx.x;
    const int qn = nblk >> 3, rem = nblk & 7, xcd = lin & 7;
    const int logical = xcd * qn + min(xcd, rem) + (lin >> 3);
    const int per_pair = kStrips * kSegs;
    const int pair = logical / per_pair;
    const int r = logical - pair * per_pair;
    const int seg = r / kStrips, sx = r - seg * kStrips;
    const int lane = threadIdx.x & 63;
    const int c0 = sx * kOut - kHaloC;
    const int a = seg * kSeg, b = min(kRows, a + kSeg);
    const int dir = (seg & 1) ? -1 : 1;
    const int gce = c0 + 2 * lane;
    const bool ce = (unsigned)gce < (unsigned)kCols;
    const bool st_lane = lane >= kHaloC / 2 && lane < (128 - kHaloC) / 2;
    const int plane = kRows * kCols * 4;
    const size_t pb = size_t(pair) * kPx;
    // planar: 4 B per column; interleaved: 8 B per column of the uv plane
    const int ld8 = ce ? gce * 4 : kOOB, st8 = (st_lane && ce) ? gce * 4 : kOOB;
    const int ld16 = ce ? gce * 8 : kOOB, st16 = (st_lane && ce) ? gce * 8 : kOOB;
    auto mk = [](const void *q, int n) {
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(q), 0, n, 0x00020000);
    };
    const auto ru = mk(p.u + pb, IL == 1 ? 0 : plane), rv = mk(p.v + pb, IL == 1 ? 0 : plane);
    const auto ruo = mk(p.uo + pb, IL == 1 ? 0 : plane), rvo = mk(p.vo + pb, IL == 1 ? 0 : plane);
    const auto ruv = mk(p.uv + 2 * pb, IL == 1 ? 2 * plane : 0);
    const auto ruvo = mk(p.uvo + 2 * pb, IL == 1 ? 2 * plane : 0);
    const auto rg = mk(p.g + pb, plane);
    const int rb = kCols * 4;
    auto off = [&](int row) { return (unsigned)row < (unsigned)kRows ? row * rb : (int)0x80000000; };
    auto load = [&](Row<IL> &d, int row) {
        const int so = off(row);
        if constexpr (IL == 1) {
            // the uv plane's own row pitch; rows outside the image stay at 2^31
            const int so2 = so < 0 ? so : 2 * so;
            d.uv = __builtin_amdgcn_raw_buffer_load_b128(ruv, ld16, so2, 0);
        } else if constexpr (IL == 2) {
            const int so2 = so < 0 ? so : so - (row & 1) * rb;
            d.uv = __builtin_amdgcn_raw_buffer_load_b128((row & 1) ? rv : ru, ld16, so2, 0);
        } else {
            d.u = __builtin_amdgcn_raw_buffer_load_b64(ru, ld8, so, 0);
            d.v = __builtin_amdgcn_raw_buffer_load_b64(rv, ld8, so, 0);
        }
        d.g = __builtin_amdgcn_raw_buffer_load_b64(rg, ld8, so, 0);
    };
    const int t_first = dir > 0 ? a - kHaloR : ((b - 1 + kHaloR) | 1);
    const int nsteps = dir > 0 ? b - a + 2 * kHaloR : t_first - (a - kHaloR) + 1;
    Row<IL> buf[kD];
#pragma unroll
    for (int k = 0; k < kD; ++k) {
        load(buf[k], t_first + dir * k);
        __builtin_amdgcn_sched_barrier(0);  // in the loop's order: its waits count on it
    }
    unsigned acc = 0;
    for (int s = 0; s < nsteps; s += kD) {
#pragma unroll
        for (int k = 0; k < kD; ++k) {
            const int t = t_first + dir * (s + k);
            // the slot's row is stored, then reloaded in place (no register
            // copies at the loop's end, which would drain the loads)
            const Row<IL> cur = buf[k];
            const int y = t - dir * kHaloR;
            const int so = (y >= a && y < b) ? y * rb : (int)0x80000000;
            acc ^= cur.g.x ^ cur.g.y;
            if constexpr (IL == 1) {
                __builtin_amdgcn_raw_buffer_store_b128(cur.uv, ruvo, st16, so < 0 ? so : 2 * so, 2);
            } else if constexpr (IL == 2) {
                __builtin_amdgcn_raw_buffer_store_b128(cur.uv, (y & 1) ? rvo : ruo, st16,
                                                       so < 0 ? so : so - (y & 1) * rb, 2);
            } else {
                __builtin_amdgcn_raw_buffer_store_b64(cur.u, ruo, st8, so, 2);
                __builtin_amdgcn_raw_buffer_store_b64(cur.v, rvo, st8, so, 2);
            }
            load(buf[k], t + dir * kD);
            __builtin_amdgcn_sched_barrier(0);  // steps stay apart, as in K4
        }
    }
    if (acc == 0x9E3779B9u) p.sink[0] = acc + hold[lane];  // never: the planes hold 1s
}

#define CK(x)                                                              \
    do {                                                                   \
        hipError_t e_ = (x);                                               \
        if (e_ != hipSuccess) {                                            \
            printf("%s: %s\n", #x, hipGetErrorString(e_));                 \
            return 1;                                                      \
        }                                                                  \
    } while (0)

int main(int argc, char **argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 7, reps = argc > 2 ? atoi(argv[2]) : 50;
    const size_t pl = kPx * kBatch * 4;  // one planar plane, all pairs
    unsigned *buf, *sink;
    CK(hipMalloc(&buf, 5 * pl));
    CK(hipMalloc(&sink, 256));
    CK(hipMemset(buf, 1, 5 * pl));
    unsigned *q[5];
    for (int i = 0; i < 5; ++i) q[i] = buf + i * (pl / 4);
    // (a): u, v, u2, v2, g;  (b): uv = planes 0-1, uv2 = planes 2-3, g
    Args A[2] = {{q[0], q[1], nullptr, q[4], q[2], q[3], nullptr, sink},
                 {q[2], q[3], nullptr, q[4], q[0], q[1], nullptr, sink}};
    Args B[2] = {{nullptr, nullptr, q[0], q[4], nullptr, nullptr, q[2], sink},
                 {nullptr, nullptr, q[2], q[4], nullptr, nullptr, q[0], sink}};
    const size_t lds = 20 * 1024;
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    auto run = [&](int form, int n, float *us) -> hipError_t {
        (void)hipEventRecord(e0, 0);
        for (int i = 0; i < n; ++i) {
            if (form == 1)
                hipLaunchKernelGGL(stream<1>, dim3(kWaves), dim3(64), lds, 0, B[i & 1]);
            else if (form == 2)
                hipLaunchKernelGGL(stream<2>, dim3(kWaves), dim3(64), lds, 0, A[i & 1]);
            else
                hipLaunchKernelGGL(stream<0>, dim3(kWaves), dim3(64), lds, 0, A[i & 1]);
        }
        (void)hipEventRecord(e1, 0);
        hipError_t e = hipEventSynchronize(e1);
        if (e != hipSuccess) return e;
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        *us = ms * 1000.f / n;
        return hipGetLastError();
    };
    float t;
    for (int f = 0; f < 3; ++f) CK(run(f, 10, &t));
    std::vector<float> tt[3];
    for (int r = 0; r < rounds; ++r)
        for (int f = 0; f < 3; ++f) {
            CK(run(f, reps, &t));
            tt[f].push_back(t);
        }
    printf("uv_width: %d waves x %d rows, %d rounds of %d launches, us per launch\n", kWaves,
           kSeg + 2 * kHaloR, rounds, reps);
    const char *name[3] = {"(a) five planes, 8 B     ", "(b) uv plane, 16 B       ",
                           "(c) uv in place, 16 B    "};
    const double bytes = 20.0 * kPx * kBatch;
    float med[3];
    for (int f = 0; f < 3; ++f) {
        printf("%s:", name[f]);
        for (float x : tt[f]) printf(" %.2f", x);
        std::sort(tt[f].begin(), tt[f].end());
        med[f] = tt[f][rounds / 2];
        printf("   median %.2f (%.2f TB/s on 20 B/px), range %.2f-%.2f\n", med[f],
               bytes / med[f] * 1e-6, tt[f].front(), tt[f].back());
    }
    printf("(a)/(b) %.3f   (a)/(c) %.3f\n", med[0] / med[1], med[0] / med[2]);
    (void)hipFree(buf);
    (void)hipFree(sink);
    return 0;
}
