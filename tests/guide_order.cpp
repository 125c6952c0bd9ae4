// CPU harness of tests/test_guide_order.py: the host half of the guide-tree read order (abpoa_amd/csrc/guide_order.cpp) -- flag decoding and the greedy order
// from a triangular hit matrix.  Stand-alone program, built with -fsanitize=undefined,address.  argv[1]: a text file of cases, each
//   n  hit[0 .. n(n+1)/2)  order[0 .. n)
// (the recorded matrices and orders of the reference); the cases below need no file.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "guide_order.h"

using namespace abpoa_hip;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

static std::vector<int32_t> order_of(int n, const std::vector<int32_t> &hit) {
    CHECK((int)hit.size() == n * (n + 1) / 2);
    std::vector<int32_t> o(n > 0 ? n : 1, -7);
    guide_greedy_order(n, hit.data(), o.data());
    o.resize(n);
    return o;
}
// triangular matrix of reads given as multisets of small values
static std::vector<int32_t> hits_of(const std::vector<std::vector<int>> &reads) {
    const int n = (int)reads.size();
    std::vector<int32_t> h(n * (n + 1) / 2, 0);
    for (int i = 0; i < n; ++i) {
        h[i * (i + 1) / 2 + i] = (int32_t)reads[i].size();
        for (int j = 0; j < i; ++j) {
            int c = 0;
            for (int v = 0; v < 64; ++v) { int a = 0, b = 0; for (int x : reads[i]) a += x == v; for (int x : reads[j]) b += x == v; c += a < b ? a : b; }
            h[i * (i + 1) / 2 + j] = c;
        }
    }
    return h;
}
typedef std::vector<int32_t> V;

int main(int argc, char **argv) {
    // flags
    GuideParams g;
    CHECK(guide_params(5, ABPOA_HIP_PROGRESSIVE, &g) == 0 && g.k == 19 && g.w == 10 && !g.aa && !g.both_strands);
    CHECK(guide_params(5, ABPOA_HIP_PROGRESSIVE | ABPOA_HIP_AMB_STRAND | ABPOA_HIP_GUIDE_KW(15, 5), &g) == 0 && g.k == 15 && g.w == 5 && g.both_strands);
    CHECK(ABPOA_HIP_GUIDE_KW(15, 5) == (15u << 8 | 5u << 16) && ABPOA_HIP_GUIDE_KW(0, 0) == 0 && ABPOA_HIP_PROGRESSIVE == 8u);
    CHECK(guide_params(27, ABPOA_HIP_AMB_STRAND, &g) == 0 && g.k == 7 && g.w == 4 && g.aa && !g.both_strands);      // amino acids: default 7 / 4, one strand
    CHECK(guide_params(27, ABPOA_HIP_GUIDE_KW(0, 9), &g) == 0 && g.k == 7 && g.w == 4);                             // (the reference resets both, abpoa_align.c:157-159)
    CHECK(guide_params(27, ABPOA_HIP_GUIDE_KW(11, 9), &g) == 0 && g.k == 11 && g.w == 9);
    CHECK(guide_params(27, ABPOA_HIP_GUIDE_KW(12, 9), &g) == ABPOA_HIP_EINVAL);
    CHECK(guide_params(5, ABPOA_HIP_GUIDE_KW(28, 255), &g) == 0 && g.k == 28 && g.w == 255);
    CHECK(guide_params(5, ABPOA_HIP_GUIDE_KW(29, 10), &g) == ABPOA_HIP_EINVAL && guide_params(5, ABPOA_HIP_GUIDE_KW(255, 10), &g) == ABPOA_HIP_EINVAL);
    CHECK(guide_params(5, ABPOA_HIP_GUIDE_KW(1, 1), &g) == 0 && g.k == 1 && g.w == 1);
    // fewer than three reads, no minimizer at all: the input order
    CHECK(order_of(0, V{}) == V{});
    CHECK(order_of(1, V{5}) == V{0});
    CHECK(order_of(2, V{5, 1, 5}) == (V{0, 1}));
    CHECK(order_of(4, V(10, 0)) == (V{0, 1, 2, 3}));
    // n = 3: the most similar pair (stored column first), then the rest
    CHECK(order_of(3, hits_of({{1, 2, 3}, {7, 8, 9}, {1, 2, 4}})) == (V{0, 2, 1}));
    CHECK(order_of(3, hits_of({{1, 2, 3}, {2, 3, 4}, {3, 4, 2}})) == (V{1, 2, 0}));
    // duplicate reads: exact ties go to the lowest index -- the first pair is the FIRST of the equal largest ones (rows ascending, then columns)
    CHECK(order_of(4, hits_of({{1, 2}, {1, 2}, {1, 2}, {1, 2}})) == (V{0, 1, 2, 3}));
    CHECK(order_of(5, hits_of({{9}, {1, 2}, {1, 2}, {5, 6}, {1, 2}})) == (V{1, 2, 4, 0, 3}));
    CHECK(order_of(5, hits_of({{5, 6}, {1, 2, 3}, {5, 6}, {1, 2, 3}, {1, 2}})) == (V{0, 2, 1, 3, 4}));
    // a read without minimizers: zero denominators against other empty reads count as similarity 0, no division
    CHECK(order_of(4, hits_of({{}, {}, {1, 2}, {1, 2}})) == (V{2, 3, 0, 1}));
    CHECK(order_of(4, hits_of({{1}, {}, {}, {2}})) == (V{0, 1, 2, 3}));
    CHECK(order_of(3, hits_of({{}, {4}, {}})) == (V{0, 1, 2}));
    // multiplicities: the smaller count of a repeated value
    CHECK(hits_of({{1, 1, 1, 2}, {1, 1, 3}})[1] == 2);
    int n_file = 0;
    if (argc > 1) {
        FILE *f = fopen(argv[1], "r");
        CHECK(f);
        int n;
        while (fscanf(f, "%d", &n) == 1) {
            V hit(n * (n + 1) / 2), want(n);
            for (auto &v : hit) CHECK(fscanf(f, "%d", &v) == 1);
            for (auto &v : want) CHECK(fscanf(f, "%d", &v) == 1);
            const V got = order_of(n, hit);
            if (got != want) { fprintf(stderr, "case %d (n = %d): order differs from the recorded one\n", n_file, n); return 1; }
            ++n_file;
        }
        fclose(f);
    }
    printf("guide order ok: %d recorded cases\n", n_file);
    return 0;
}
