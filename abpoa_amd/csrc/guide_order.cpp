// Host half of the guide-tree read order (guide_order.h): parameters, Jaccard similarity, greedy order.  Plain C++: no HIP headers, so that the
// stand-alone harness tests/guide_order.cpp can build it under host sanitizers.
#include "guide_order.h"

namespace abpoa_hip {

int guide_params(int m, unsigned flags, GuideParams *out) {
    int k = (int)((flags >> 8) & 0xffu), w = (int)((flags >> 16) & 0xffu);
    const bool aa = m > 5, k_given = k != 0;
    if (k == 0) k = 19;
    if (w == 0) w = 10;
    if (aa && k > 11) {
        if (k_given) return ABPOA_HIP_EINVAL;
        k = 7; w = 4;
    }
    if (k < 1 || k > 28 || w < 1 || w > 255) return ABPOA_HIP_EINVAL;
    out->k = k; out->w = w; out->aa = aa;
    out->both_strands = !aa && (flags & ABPOA_HIP_AMB_STRAND);
    return ABPOA_HIP_OK;
}

void guide_greedy_order(int n, const int32_t *hit, int32_t *order) {
    for (int i = 0; i < n; ++i) order[i] = i;
    if (n < 3) return;
    auto H = [&](int i, int j) { return hit[((int64_t)i * (i + 1)) / 2 + j]; };      // j <= i
    int64_t n_mm = 0;
    for (int i = 0; i < n; ++i) n_mm += H(i, i);
    if (n_mm == 0) return;
    // similarity of every pair, and the strictly largest one (rows ascending, then columns): the first two reads
    std::vector<double> jac((size_t)n * (n - 1) / 2);
    auto J = [&](int a, int b) -> double { return a > b ? jac[(size_t)a * (a - 1) / 2 + b] : jac[(size_t)b * (b - 1) / 2 + a]; };
    double best = -1.0; int bi = -1, bj = -1;
    for (int i = 1; i < n; ++i)
        for (int j = 0; j < i; ++j) {
            const int both = H(i, j), either = H(i, i) + H(j, j) - both;
            const double v = either == 0 ? 0.0 : (0.0 + both) / either;
            jac[(size_t)i * (i - 1) / 2 + j] = v;
            if (v > best) { best = v; bi = i; bj = j; }
        }
    order[0] = bj; order[1] = bi;
    // then always the read with the strictly largest similarity sum to the chosen ones; the sum of a candidate grows by one term per chosen read, in
    // the order they were chosen -- the additions of a sum taken afresh at every step, so the same double
    std::vector<double> sum(n, 0.0);
    std::vector<char> chosen(n, 0);
    chosen[bj] = chosen[bi] = 1;
    for (int c = 0; c < n; ++c) if (!chosen[c]) { sum[c] += J(c, bj); sum[c] += J(c, bi); }
    for (int r = 2; r < n; ++r) {
        int pick = -1; best = -1.0;
        for (int c = 0; c < n; ++c) if (!chosen[c] && sum[c] > best) { best = sum[c]; pick = c; }
        order[r] = pick; chosen[pick] = 1;
        for (int c = 0; c < n; ++c) if (!chosen[c]) sum[c] += J(c, pick);
    }
}

}  // namespace abpoa_hip
