// CPU property checks of abpoa_amd/csrc/wide_closed_forms.h, the integer closed forms of the all-chunks row body (rows_fast.h ilp_chunks), against
// literal restatements of what they replace.  Built by tests/test_wide_row_closed_forms.py with -fsanitize=undefined (signed overflow aborts).
//   usage: wide_row_closed_forms key16|key32|carry <seed> <iterations>
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "wide_closed_forms.h"
using namespace abpoa_hip;

static long long n_checks = 0, n_fails = 0;
#define CHECK(x, ...) do { ++n_checks; if (!(x)) { if (n_fails++ < 10) { printf("FAILED %s: ", #x); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// ---- literal max_in_row (reference src/simd_abpoa_align.c:1043-1057; oracle/abpoa_dp_oracle.c max_in_row): H holds the row's columns beg_sn * pn ..
static void literal_max_in_row(const std::vector<int> &H, int pn, int beg_sn, int end_sn, int qlen, int inf, int &mx, int &mi) {
    auto at = [&](int j) { return H[j - beg_sn * pn]; };
    int a[16], b[16];
    for (int l = 0; l < pn; ++l) {
        const int j = end_sn * pn + l;
        a[l] = at(j); b[l] = j <= qlen ? j : -1;
        if (end_sn == qlen / pn && 0 > b[l]) a[l] = inf;
    }
    for (int v = beg_sn; v < end_sn; ++v) for (int l = 0; l < pn; ++l) {
        const int j = v * pn + l;
        if (at(j) > a[l]) { a[l] = at(j); b[l] = j <= qlen ? j : -1; }
    }
    mx = inf; mi = -1;
    for (int l = 0; l < pn; ++l) if (a[l] > mx) { mx = a[l]; mi = b[l]; }
}

// ---- the arg-max keys: random rows of 1..11 chunks; every in-band lane of every chunk builds its key as ilp_chunks does, the keys are reduced with an
//      unsigned max in a shuffled order (the DPP reduction), the winner is decoded and compared with the literal max_in_row
static void check_keys(bool i16, std::mt19937_64 &rng, int iters) {
    const int PN = i16 ? 16 : 8, NV = 64 / PN;
    auto uni = [&](long long lo, long long hi) { return (long long)(lo + (long long)(rng() % (unsigned long long)(hi - lo + 1))); };
    const int lo_t = i16 ? INT16_MIN : INT32_MIN, hi_t = i16 ? INT16_MAX : INT32_MAX;
    long long n_declined = 0, n_wide = 0;
    for (int nch = 1; nch <= 11; ++nch) for (int it = 0; it < iters; ++it) {
        const int mis = (int)uni(1, 8), oe = (int)uni(2, 30), e = (int)uni(0, 4);
        const int inf = lo_t + std::max(mis, oe) + 31 * e;                        // the reference's inf_min
        const int nvr = (int)uni((nch - 1) * NV + 1, nch * NV), Wr = nvr * PN;    // vectors of the row: exactly nch chunks of 64 lanes
        if (nvr > 64) ++n_wide;
        const int max_vec = i16 ? 2047 : 4095;                                    // int16: qlen < 2^15; int32: 12-bit band geometry
        const int beg_sn = (int)uni(0, max_vec - nvr + 1), end_sn = beg_sn + nvr - 1;
        int qlen;
        if (it % 3 == 0 || (end_sn + 1) * PN + 1 > (i16 ? INT16_MAX : 1 << 20)) qlen = end_sn * PN + (int)uni(0, PN - 1);      // end_sn == qlen_sn: the mask
        else qlen = (int)std::min<long long>((i16 ? INT16_MAX : 1 << 20), (long long)(end_sn + 1) * PN + uni(0, 3000));
        const int qlen_sn = qlen / PN;
        // values: a walk around a base; inf and inf-like cells; int16 extremes; int32 windows around the floor
        int vfloor = 0;
        long long base;
        if (i16) base = uni(-30000, 32000);
        else { vfloor = (int)uni(-(1 << 22), 1 << 22) - (1 << 19); base = vfloor + uni(-3000, (1 << 21) + 3000); }
        std::vector<int> H(Wr);
        const int mode = (int)uni(0, 5);
        for (int x = 0; x < Wr; ++x) {
            long long v = base + uni(-40, 40) - (mode == 1 ? uni(0, 5000) : 0);
            const int r = (int)uni(0, 19);
            if (r == 0) v = inf; else if (r == 1) v = inf + uni(-oe, 1); else if (r == 2 && i16) v = uni(0, 1) ? hi_t : lo_t;
            v = std::max<long long>(std::min<long long>(v, hi_t), i16 ? lo_t : (long long)inf - 5000);
            H[x] = (int)v;
        }
        if (mode == 2) std::fill(H.begin(), H.end(), inf);                                 // a dead row
        // ties: plant the row's maximum again across lanes, across vectors, in the end vector
        int mx0 = INT_MIN; for (int x = 0; x < Wr; ++x) mx0 = std::max(mx0, H[x]);
        if (!i16 && mode == 3) {                                                           // the window's edges
            const int edge[6] = {vfloor, vfloor + 1, vfloor + ARGMAX32_TOP - 1, vfloor + ARGMAX32_TOP, vfloor + ARGMAX32_TOP + 7, vfloor - 3};
            mx0 = edge[uni(0, 5)];
            for (int x = 0; x < Wr; ++x) H[x] = std::min(H[x], mx0 - (int)uni(0, 2));
            H[uni(0, Wr - 1)] = mx0;
        }
        const int nt = (int)uni(0, 6);
        for (int t = 0; t < nt; ++t) {
            const int kind = (int)uni(0, 2);
            int x = (int)uni(0, Wr - 1);
            if (kind == 1) x = (int)(uni(0, nvr - 1) * PN + x % PN);                      // same lane residue, another vector
            if (kind == 2) x = (nvr - 1) * PN + (int)uni(0, PN - 1);                        // the end vector
            H[x] = mx0;
        }
        // the kernel: lane = vvl * PN + l, column colb + 64 c of chunk c
        std::vector<unsigned> keys;
        const int relv_end = end_sn - beg_sn;
        for (int cg = 0; cg < nch; ++cg) for (int lane = 0; lane < 64; ++lane) {
            const int l = lane % PN, vvl = lane / PN, col = beg_sn * PN + lane + 64 * cg;
            const bool in_band = cg * 64 + lane < Wr, is_end = cg * NV + vvl == relv_end;
            if (!in_band) continue;
            int cand = H[cg * 64 + lane];
            if (end_sn == qlen_sn) cand = (is_end && col > qlen) ? inf : cand;
            keys.push_back(i16 ? argmax_key16(cand, argmax_key16_const(PN, l, vvl), beg_sn + cg * NV, is_end)
                               : argmax_key32(cand, vfloor, argmax_tie32(PN, l, vvl), cg, NV, is_end));
        }
        std::shuffle(keys.begin(), keys.end(), rng);
        unsigned kbst = 0;
        for (unsigned k : keys) kbst = k > kbst ? k : kbst;
        int lmx, lmi; literal_max_in_row(H, PN, beg_sn, end_sn, qlen, inf, lmx, lmi);
        int rowmax, mi;
        if (i16) {
            argmax_decode16(kbst, PN, qlen, inf, rowmax, mi);
            CHECK(mi == lmi && (lmx == inf ? rowmax <= inf : rowmax == lmx), "int16 nch %d beg %d end %d qlen %d: key %08x -> (%d, %d), literal (%d, %d)", nch, beg_sn,
                  end_sn, qlen, kbst, rowmax, mi, lmx, lmi);
        } else {
            // declined <=> the true winner is outside the window (vfloor, vfloor + 2^21 - 1)
            const bool outside = (long long)lmx <= vfloor || (long long)lmx >= (long long)vfloor + ARGMAX32_TOP;
            const bool declined = argmax_declines32(kbst);
            n_declined += declined;
            CHECK(declined == outside, "int32 nch %d beg %d end %d: key %08x declined %d, literal max %d (floor %d)", nch, beg_sn, end_sn, kbst, (int)declined, lmx, vfloor);
            if (!declined) {
                argmax_decode32(kbst, PN, beg_sn, vfloor, qlen, inf, rowmax, mi);
                CHECK(rowmax == lmx && mi == lmi, "int32 nch %d beg %d end %d qlen %d: key %08x -> (%d, %d), literal (%d, %d)", nch, beg_sn, end_sn, qlen, kbst, rowmax,
                      mi, lmx, lmi);
            }
        }
    }
    printf("rows of more than 64 vectors %lld, declined %lld\n", n_wide, n_declined);
}

// ---- the carry chain: one row of nch chunks; the literal vector-by-vector F scan chained across the whole row (reference :868-875 / :988-997 with
//      SIMD_SET_F, as tests/test_affine_closed_form.py literal_vector) against per-chunk unseeded prefix maxima + the seed chain + the F of ilp_chunks
static const int INJ16[16] = {0, 0, 0, 0, 0, 0, 0, 0, 8, 8, 8, 8, 12, 12, 14, -1}, INJ8[8] = {0, 0, 0, 0, 4, 4, 6, -1};      // dp_common.h inj_dist
struct Row { int PN, nch, inf, o, e; long long first; std::vector<int> hs; };
static std::vector<long long> literal_f(const Row &r) {
    const int pn = r.PN, oe = r.o + r.e, nv = (int)r.hs.size() / pn;
    std::vector<long long> F(r.hs.size());
    long long first = r.first;
    for (int v = 0; v < nv; ++v) {
        long long f[16];
        f[0] = first - oe;
        for (int l = 1; l < pn; ++l) f[l] = (long long)r.hs[v * pn + l - 1] - oe;
        for (int s = 1; s < pn; s *= 2) {
            long long g[16];
            for (int l = 0; l < pn; ++l) g[l] = l >= s ? std::max(f[l], f[l - s] - (long long)s * r.e) : std::max(f[l], (long long)r.inf);
            memcpy(f, g, sizeof f);
        }
        for (int l = 0; l < pn; ++l) F[v * pn + l] = f[l];
        first = std::max<long long>(r.hs[v * pn + pn - 1], f[pn - 1] + r.o);
    }
    return F;
}
// prefix maxima of chunk c without a seed: s[lane] = max over lanes < lane of g = hs + lane e (lane 0: INT_MIN); total = max over all 64 lanes
static void chunk_scan(const Row &r, int c, int *s, int &total) {
    int run = INT_MIN;
    for (int lane = 0; lane < 64; ++lane) { s[lane] = run; run = std::max(run, r.hs[c * 64 + lane] + lane * r.e); }
    total = run;
}
static std::vector<int> seed_chain(const Row &r) {
    std::vector<int> seed(r.nch + 1);
    seed[0] = (int)r.first - r.e;
    for (int c = 0; c < r.nch; ++c) { int s[64], total; chunk_scan(r, c, s, total); seed[c + 1] = carry_next(total, seed[c], r.e); }
    return seed;
}
static Row random_row(std::mt19937_64 &rng, int PN, int nch, int e, bool i16) {
    auto uni = [&](long long lo, long long hi) { return (long long)(lo + (long long)(rng() % (unsigned long long)(hi - lo + 1))); };
    Row r; r.PN = PN; r.nch = nch; r.e = e; r.o = (int)uni(1, 24);
    const int mis = (int)uni(1, 8), lo_t = i16 ? INT16_MIN : INT32_MIN;
    r.inf = lo_t + std::max(mis, r.o + e) + 31 * e;
    const int fast_lo = lo_t + r.o + e + PN * e;                                    // rows_fast.h fast_lo: lower cells send the row to the exact bodies
    const int W = nch * 64;
    r.hs.resize(W);
    long long h = uni(-200, 800) + (i16 ? 0 : uni(-(1 << 20), 1 << 20));
    for (int x = 0; x < W; ++x) { h += uni(-15, 15); r.hs[x] = (int)h; }
    const int nstretch = (int)uni(0, 3);                                             // inf stretches (the band's dead ends, rows of padding)
    for (int t = 0; t < nstretch; ++t) { const int a = (int)uni(0, W - 1), b = (int)std::min<long long>(W, a + uni(1, 200)); for (int x = a; x < b; ++x) r.hs[x] = uni(0, 3) ? r.inf : r.inf - mis; }
    for (int x = 0; x < W; ++x) r.hs[x] = std::max(r.hs[x], fast_lo);
    r.first = uni(0, 3) == 0 ? r.inf : r.hs[0] + uni(-5, 5);
    return r;
}
static void check_carry(std::mt19937_64 &rng, int iters) {
    for (int pn : {16, 8}) for (int gap = 1; gap <= 2; ++gap) for (int nch = 1; nch <= 11; ++nch) for (int it = 0; it < iters; ++it) {
        // convex: the second plane is a scan of the same hs with its own (o2, e2); e = 0 included
        for (int plane = 0; plane < gap; ++plane) {
            const int e = (int)(rng() % 5);
            Row r = random_row(rng, pn, nch, e, pn == 16);
            const std::vector<long long> lit = literal_f(r);
            const std::vector<int> seed = seed_chain(r);
            const int *INJ = pn == 16 ? INJ16 : INJ8, oe = r.o + r.e;
            for (int c = 0; c < nch; ++c) {
                int s[64], total; chunk_scan(r, c, s, total);
                for (int lane = 0; lane < 64; ++lane) {
                    const int l = lane % pn, cf = oe - r.e + lane * r.e, inj = INJ[l] >= 0 ? r.inf - INJ[l] * r.e : INT_MIN;
                    const int F = std::max(std::max(s[lane], seed[c]) - cf, inj);      // ilp_chunks: S = max(s, seed), F = max(S - cf, inj)
                    CHECK(F == lit[c * 64 + lane], "carry pn %d gap %d nch %d e %d chunk %d lane %d: %d, literal %lld", pn, gap, nch, e, c, lane, F, lit[c * 64 + lane]);
                }
            }
        }
    }
}

int main(int argc, char **argv) {
    if (argc < 4) { printf("usage: %s key16|key32|carry <seed> <iterations>\n", argv[0]); return 2; }
    std::mt19937_64 rng(strtoull(argv[2], nullptr, 10));
    const int iters = atoi(argv[3]);
    if (!strcmp(argv[1], "key16")) check_keys(true, rng, iters);
    else if (!strcmp(argv[1], "key32")) check_keys(false, rng, iters);
    else if (!strcmp(argv[1], "carry")) check_carry(rng, iters);
    else return 2;
    printf("%s: %lld checks, %lld failed\n", argv[1], n_checks, n_fails);
    if (!n_fails) printf("closed forms ok\n");
    return n_fails ? 1 : 0;
}
