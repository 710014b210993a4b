// median_network_check.cpp -- proves KM's selection networks
// (cpp-optical-flow_amd/csrc/hsflow_median_net.h) on the host and counts their
// operations.  Build: g++ -O2 -std=c++17 -I cpp-optical-flow_amd/csrc
// scripts/median_network_check.cpp -o median_network_check.
//
// 0-1 principle: a network of min/max selects rank r of every input iff it
// does for every 0/1 input.  64 inputs per word (bit b of word w of tap t is
// tap t of input 64 w + b), min = AND, max = OR; the expected output bit is
// popcount(input) > r, r = (k^2 - 1) / 2.  All 2^(k^2) inputs are run.
// The operation count is that of the expression DAG that reaches the result
// (what is left after dead-code elimination), per output pixel, with the
// line sorts counted once per line as the kernel shares them.
// Prints one line per size; exit status 0 iff both networks are right.
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#define HSFLOW_NET_FN inline
#include "hsflow_median_net.h"

struct BitOps {
    static uint64_t mn(uint64_t a, uint64_t b) { return a & b; }
    static uint64_t mx(uint64_t a, uint64_t b) { return a | b; }
};

// expression DAG: node 0.. are inputs, every mn/mx makes a node
struct Dag {
    std::vector<int> lhs, rhs;
    int node(int a, int b) {
        lhs.push_back(a);
        rhs.push_back(b);
        return (int)lhs.size() - 1;
    }
};
static Dag *g_dag;
struct Sym {
    int id;
};
struct SymOps {
    static Sym mn(Sym a, Sym b) { return {g_dag->node(a.id, b.id)}; }
    static Sym mx(Sym a, Sym b) { return {g_dag->node(a.id, b.id)}; }
};

template <class O, int K, class T>
static T median_of_taps(const T *taps) {
    T r[K][K];
    for (int j = 0; j < K; ++j) {
        for (int i = 0; i < K; ++i) r[j][i] = taps[j * K + i];
        hsflow_net::sort_line<O>(r[j]);
    }
    return hsflow_net::median_of_lines<O>(r);
}

template <int K>
static bool check() {
    constexpr int N = K * K, R = (N - 1) / 2;
    // taps 0..5 vary inside a word, the others with the word index
    static const uint64_t kLow[6] = {0xAAAAAAAAAAAAAAAAull, 0xCCCCCCCCCCCCCCCCull,
                                     0xF0F0F0F0F0F0F0F0ull, 0xFF00FF00FF00FF00ull,
                                     0xFFFF0000FFFF0000ull, 0xFFFFFFFF00000000ull};
    const uint64_t words = 1ull << (N - 6);
    uint64_t bad = 0;
    for (uint64_t w = 0; w < words; ++w) {
        uint64_t taps[N];
        for (int t = 0; t < N; ++t)
            taps[t] = t < 6 ? kLow[t] : ((w >> (t - 6)) & 1 ? ~0ull : 0ull);
        const uint64_t got = median_of_taps<BitOps, K>(taps);
        const int high = __builtin_popcountll(w);
        uint64_t want = 0;
        for (int b = 0; b < 64; ++b)
            if (high + __builtin_popcount(b) > R) want |= 1ull << b;
        bad += __builtin_popcountll(got ^ want);
    }
    // live operations: the whole window, and what the line sorts take of it
    Dag dag;
    g_dag = &dag;
    Sym taps[N];
    for (int t = 0; t < N; ++t) taps[t] = {dag.node(-1, -1)};
    const int after_inputs = (int)dag.lhs.size();
    Sym r[K][K];
    for (int j = 0; j < K; ++j) {
        for (int i = 0; i < K; ++i) r[j][i] = taps[j * K + i];
        hsflow_net::sort_line<SymOps>(r[j]);
    }
    const int after_sorts = (int)dag.lhs.size();
    const Sym out = hsflow_net::median_of_lines<SymOps>(r);
    std::set<int> live;
    std::vector<int> todo{out.id};
    while (!todo.empty()) {
        const int n = todo.back();
        todo.pop_back();
        if (n < after_inputs || !live.insert(n).second) continue;
        todo.push_back(dag.lhs[n]);
        todo.push_back(dag.rhs[n]);
    }
    int sort_ops = 0, select_ops = 0;
    for (int n : live) (n < after_sorts ? sort_ops : select_ops)++;
    std::printf("k %d inputs 2^%d wrong %llu ops_per_line_sort %d ops_select %d "
                "ops_per_pixel_shared %d ops_per_pixel_unshared %d\n",
                K, N, (unsigned long long)bad, sort_ops / K, select_ops,
                sort_ops / K + select_ops, sort_ops + select_ops);
    return bad == 0;
}

int main() {
    const bool ok3 = check<3>();
    const bool ok5 = check<5>();
    return ok3 && ok5 ? 0 : 1;
}
