// hsflow_median_net.h -- the selection networks of KM (hsflow_median.hip),
// written over an operation set O { mn(a, b), mx(a, b) } on a key type T so
// that the same text runs on the device (unsigned keys, v_min/v_max/v_min3/
// v_max3) and on the host, where scripts/median_network_check.cpp proves it by
// the 0-1 principle: a min/max network selects rank r of every input iff it
// does so for every 0/1 input, and with T = 64 inputs per word, mn = AND,
// mx = OR, all 2^9 and 2^25 of them take a fraction of a second.
//
// The includer defines HSFLOW_NET_FN (the function qualifiers).  Every index
// is a compile-time constant after unrolling, so the arrays live in registers.
#pragma once

namespace hsflow_net {

template <class O, class T>
HSFLOW_NET_FN void cswap(T &a, T &b) {
    const T lo = O::mn(a, b);
    b = O::mx(a, b);
    a = lo;
}

template <class O, class T>
HSFLOW_NET_FN T med3(T a, T b, T c) {
    return O::mx(O::mn(a, b), O::mn(O::mx(a, b), c));
}

// ascending sorts: 3 and 9 exchanges (optimal)
template <class O, class T>
HSFLOW_NET_FN void sort_line(T (&a)[3]) {
    cswap<O>(a[0], a[1]);
    cswap<O>(a[1], a[2]);
    cswap<O>(a[0], a[1]);
}

template <class O, class T>
HSFLOW_NET_FN void sort_line(T (&a)[5]) {
    cswap<O>(a[0], a[1]);
    cswap<O>(a[3], a[4]);
    cswap<O>(a[2], a[4]);
    cswap<O>(a[2], a[3]);
    cswap<O>(a[1], a[4]);
    cswap<O>(a[0], a[3]);
    cswap<O>(a[0], a[2]);
    cswap<O>(a[1], a[3]);
    cswap<O>(a[1], a[2]);
}

// min of a[0..M) into a[0], max into a[M-1]; the rest stays a permutation
template <class O, int M, class T>
HSFLOW_NET_FN void extremes_out(T (&a)[M]) {
#pragma unroll
    for (int i = 0; i < M / 2; ++i) cswap<O>(a[i], a[M - 1 - i]);
#pragma unroll
    for (int i = 1; i < (M + 1) / 2; ++i) cswap<O>(a[0], a[i]);
#pragma unroll
    for (int i = M / 2; i < M - 1; ++i) cswap<O>(a[i], a[M - 1]);
}

// Median of a[0..M) and the M - 3 elements rest[0..) (2 M - 3 in all) by
// forgetful selection: the smallest and the largest of M elements in hand
// have M - 1 elements on one side, more than the median of the 2 M - 3 has,
// so both go and one unseen element comes in, down to the median of three.
template <class O, int M, class T>
struct Forget {
    static HSFLOW_NET_FN T run(T (&a)[M], const T *rest) {
        extremes_out<O, M>(a);
        T b[M - 1];
#pragma unroll
        for (int i = 0; i < M - 2; ++i) b[i] = a[i + 1];
        b[M - 2] = rest[0];
        return Forget<O, M - 1, T>::run(b, rest + 1);
    }
};
template <class O, class T>
struct Forget<O, 3, T> {
    static HSFLOW_NET_FN T run(T (&a)[3], const T *) { return med3<O>(a[0], a[1], a[2]); }
};

// Median of the 9 elements of three ascending lines r[j][0..3): the largest
// of the minima, the median of the medians and the smallest of the maxima
// hold it (each other element has 5 elements on one side).
template <class O, class T>
HSFLOW_NET_FN T median_of_lines(const T (&r)[3][3]) {
    const T lo = O::mx(O::mx(r[0][0], r[1][0]), r[2][0]);
    const T mid = med3<O>(r[0][1], r[1][1], r[2][1]);
    const T hi = O::mn(O::mn(r[0][2], r[1][2]), r[2][2]);
    return med3<O>(lo, mid, hi);
}

// Median of the 25 elements of five ascending lines r[j][0..5).  Sorting rank
// i of every line across the lines gives m[i][b], ascending in i and in b:
// m[i][b] has (i + 1)(b + 1) - 1 elements below or equal and (5 - i)(5 - b) - 1
// above or equal, so only the 13 places with both products <= 13 can hold
// rank 12; 6 of the others lie below all of them and 6 above, and the median
// of the 13 is the median of the 25.  The exchanges of the five sorts whose
// results are not among the 13 are dead code.
template <class O, class T>
HSFLOW_NET_FN T median_of_lines(const T (&r)[5][5]) {
    T m[5][5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
#pragma unroll
        for (int j = 0; j < 5; ++j) m[i][j] = r[j][i];
        sort_line<O>(m[i]);
    }
    T a[8] = {m[0][3], m[4][1], m[0][4], m[4][0], m[1][2], m[3][2], m[1][3], m[3][1]};
    const T rest[5] = {m[2][2], m[1][4], m[3][0], m[2][1], m[2][3]};
    return Forget<O, 8, T>::run(a, rest);
}

}  // namespace hsflow_net
