// CPU harness of tests/test_device_plan.py: the planning step of the device-resident driver (abpoa_amd/csrc/msa_device_plan.cpp) on synthetic read-length lists,
// and the typed switch accessors of engine_options.cpp.  No GPU, no HIP runtime call; built with -fsanitize=undefined,address.
// The expected routing is what DESIGN.md section 1 and section 4.7 document (w = b + f * length; wide row loop for 40 <= w <= 215 -- 343 in the long-read form
// --; local row loop up to 575 columns; ragged sets: spread over max(64, longest / 8) becomes extra columns; linear gaps on the narrow loop only ...).
// Only plan fields that do not depend on lds_fixed_bytes_dp / _bt are asserted: the two values below are stand-ins for the kernels' own.
#include <atomic>
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <thread>
#include <vector>
#include "engine_options.h"
#include "msa_device_plan.h"

// (the snapshot a set_option replaces is left alone on purpose -- engine_options.h -- so the leak check would report every switch this harness flips)
extern "C" const char *__asan_default_options() { return "detect_leaks=0"; }

namespace abpoa_hip {
int lds_fixed_bytes_dp() { return 1024; }
int lds_fixed_bytes_bt() { return 2048; }
}  // namespace abpoa_hip
using namespace abpoa_hip;

static int g_fail = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "FAILED %s:%d [%s] %s\n", __FILE__, __LINE__, g_case.c_str(), #cond); g_fail++; } } while (0)
static std::string g_case;

struct Sets {      // read-sets by lengths alone: the plan never looks at a base
    std::vector<std::vector<int32_t>> lens; std::vector<abpoa_hip_readset_t> rs;
    void add(std::vector<int32_t> l) { lens.push_back(std::move(l)); }
    void uniform(int n_sets, int n_reads, int len) { for (int s = 0; s < n_sets; ++s) add(std::vector<int32_t>((size_t)n_reads, len)); }
    const abpoa_hip_readset_t *get() {
        rs.resize(lens.size());
        for (size_t s = 0; s < lens.size(); ++s) { rs[s].n_reads = (int)lens[s].size(); rs[s].seqs = nullptr; rs[s].lens = lens[s].data(); rs[s].weights = nullptr; }
        return rs.data();
    }
    int n() const { return (int)lens.size(); }
};

static std::vector<int32_t> g_mat;
static abpoa_hip_scoring_t scoring(int gap_mode, int align_mode = ABPOA_HIP_GLOBAL_MODE, int m = 5) {      // the reference's defaults: 2 / -4, 4 + 2 k, 24 + k, -b 10 -f 0.01
    abpoa_hip_scoring_t sc;
    g_mat.assign((size_t)m * m, -4); for (int i = 0; i < m; ++i) g_mat[(size_t)i * m + i] = 2;
    sc.m = m; sc.mat = g_mat.data(); sc.max_mat = 2; sc.min_mis = 4;
    sc.gap_open1 = gap_mode == ABPOA_HIP_LINEAR_GAP ? 0 : 4; sc.gap_ext1 = 2;
    sc.gap_open2 = gap_mode == ABPOA_HIP_CONVEX_GAP ? 24 : 0; sc.gap_ext2 = gap_mode == ABPOA_HIP_CONVEX_GAP ? 1 : 0;
    sc.align_mode = align_mode; sc.gap_mode = gap_mode; sc.wb = 10; sc.wf = 0.01f; sc.zdrop = 0; sc.ret_cigar = 1; sc.rev_cigar = 0;
    return sc;
}

// One case: the plan's documented answer, then the same job with one switch set (what: 'd' NODIR -> no direction words, the choice of kernels untouched;
// 'w' NOWIDE -> empty wide range; 'l' WIDE_LO=30 -> the range starts at 30, for jobs that have a wide loop; 'g' DEVICE_GENERAL -> the general kernel), then
// the switch reset: the first answer must come back.  Every case names at least one switch.
template <typename F>
static void run_case(const char *name, const abpoa_hip_scoring_t &sc, Sets &S, double node_factor, unsigned flags, bool force_general, const char *what, F expect) {
    g_case = name;
    const DevicePlan B = plan_device_job(&sc, S.n(), S.get(), node_factor, flags, force_general); expect(B); CHECK((int)B.ps.size() == S.n());
    CHECK(*what != 0);
    for (const char *c = what; *c; ++c) {
        g_case = std::string(name) + " + switch " + *c;
        const char *sw = *c == 'd' ? "ABPOA_HIP_NODIR" : *c == 'w' ? "ABPOA_HIP_NOWIDE" : *c == 'l' ? "ABPOA_HIP_WIDE_LO" : "ABPOA_HIP_DEVICE_GENERAL";
        CHECK(set_option(sw, *c == 'l' ? "30" : "1") == 0);
        const DevicePlan P = plan_device_job(&sc, S.n(), S.get(), node_factor, flags, force_general);
        if (*c == 'd') CHECK(!P.dir && P.general == B.general && P.fast_local == B.fast_local && P.lin_fast == B.lin_fast);
        if (*c == 'w') CHECK(P.wide_hi < P.wide_lo && !P.any_wide_set && P.general == B.general && P.dir == B.dir);
        if (*c == 'l') CHECK(P.wide_lo == 30);
        if (*c == 'g') CHECK(P.general && !P.dir && !P.fast_local && !P.lin_fast && !P.rounds_possible);
        CHECK(set_option(sw, nullptr) == 0);
        g_case = std::string(name) + " after reset of switch " + *c;
        const DevicePlan Q = plan_device_job(&sc, S.n(), S.get(), node_factor, flags, force_general); expect(Q);
    }
}

static void plan_cases() {
    const unsigned CONS = ABPOA_HIP_OUT_CONS;
    {   Sets S; S.uniform(8, 6, 1000); const abpoa_hip_scoring_t sc = scoring(ABPOA_HIP_AFFINE_GAP);
        int32_t inf; CHECK(abpoa_hip_score_bits(&sc, 3 * 1000 + 1026, 1000, &inf) == 16);
        run_case("1 kb affine", sc, S, 3.0, CONS, false, "dg", [](const DevicePlan &P) {
            CHECK(P.w_max == 20 && !P.general && P.dir && P.rounds_possible && !P.any_wide_set && !P.lin_fast && !P.fast_local && P.max_extra == 0);
            CHECK(P.wide_lo == 40 && P.wide_hi == 215 && P.CW == 4 && P.DB == 2 && !P.roomy && P.in_cap == POA_IN_CAP && P.out_cap == POA_OUT_CAP); });
        run_case("1 kb affine -s", sc, S, 3.0, CONS | ABPOA_HIP_AMB_STRAND, false, "g", [](const DevicePlan &P) { CHECK(!P.general && !P.dir && !P.rounds_possible && P.amb); });
        const abpoa_hip_scoring_t se = scoring(ABPOA_HIP_AFFINE_GAP, ABPOA_HIP_EXTEND_MODE);
        run_case("1 kb affine extend", se, S, 3.0, CONS, false, "g", [](const DevicePlan &P) { CHECK(!P.general && !P.dir && !P.rounds_possible); });
        run_case("1 kb affine forced general", sc, S, 3.0, CONS, true, "dwg", [](const DevicePlan &P) {
            CHECK(P.general && !P.dir && !P.fast_local && !P.lin_fast && !P.rounds_possible && P.wide_hi < P.wide_lo && !P.any_wide_set && P.max_extra == 0); });
        abpoa_hip_scoring_t su = sc; su.wb = -1;
        run_case("1 kb affine no band", su, S, 3.0, CONS, false, "dw", [](const DevicePlan &P) { CHECK(P.general && P.unbanded && !P.dir); });
    }
    {   Sets S; S.uniform(4, 4, 10000); const abpoa_hip_scoring_t sc = scoring(ABPOA_HIP_AFFINE_GAP);
        run_case("10 kb affine", sc, S, 3.0, CONS, false, "wlg", [](const DevicePlan &P) {
            CHECK(P.w_max == 110 && !P.general && P.wide_lo == 40 && P.wide_hi == 215 && P.wfr_cols == 448 && P.any_wide_set && !P.rounds_possible);
            for (const PoaSet &s : P.ps) CHECK(s.band_extra == 0); });
    }
    {   Sets S; S.uniform(2, 3, 26000); const abpoa_hip_scoring_t sc = scoring(ABPOA_HIP_CONVEX_GAP);
        run_case("26 kb convex", sc, S, 3.0, CONS, false, "w", [](const DevicePlan &P) {
            CHECK(P.w_max == 270 && !P.general && P.wfr_cols == 704 && P.wide_hi == 343 && P.any_wide_set && P.CW == 8 && P.DB == 4); });
    }
    {   Sets S; S.uniform(8, 6, 1000); abpoa_hip_scoring_t sc = scoring(ABPOA_HIP_LINEAR_GAP);
        run_case("linear e 2", sc, S, 3.0, CONS, false, "g", [](const DevicePlan &P) { CHECK(!P.general && P.lin_fast && !P.dir && P.rounds_possible && P.CW == 2); });
        sc.gap_ext1 = 0;
        run_case("linear e 0", sc, S, 3.0, CONS, false, "wg", [](const DevicePlan &P) { CHECK(P.general && !P.lin_fast && !P.rounds_possible); });
        sc.gap_ext1 = 2; Sets L; L.uniform(4, 4, 4000);
        run_case("linear 4 kb", sc, L, 3.0, CONS, false, "wg", [](const DevicePlan &P) { CHECK(P.w_max == 50 && P.general && !P.lin_fast); });
    }
    {   Sets S; S.uniform(1, 30, 500); const abpoa_hip_scoring_t sc = scoring(ABPOA_HIP_AFFINE_GAP, ABPOA_HIP_LOCAL_MODE, 27);
        run_case("local 500 aa", sc, S, 3.0, CONS, false, "g", [](const DevicePlan &P) {
            CHECK(P.local && P.sc.wb == -1 && !P.general && P.fast_local && P.wide_on == 0 && P.wide_hi < P.wide_lo && !P.dir && !P.rounds_possible && P.aln_cap == 26); });
        Sets L; L.uniform(1, 30, 700);
        run_case("local 700 aa", sc, L, 3.0, CONS, false, "dg", [](const DevicePlan &P) { CHECK(P.general && !P.fast_local); });
    }
    {   Sets S; S.uniform(3, 3, 1000); S.add({1000, 1000, 600}); S.add({1000, 900}); const abpoa_hip_scoring_t sc = scoring(ABPOA_HIP_AFFINE_GAP);
        run_case("ragged set", sc, S, 3.0, CONS, false, "d", [](const DevicePlan &P) {
            CHECK(!P.general && P.extra[0] == 0 && P.extra[1] == 0 && P.extra[2] == 0 && P.extra[3] == 400 && P.extra[4] == 0 && P.max_extra == 400 && !P.rounds_possible);
            CHECK(P.ps[3].band_extra == 400 && P.ps[4].band_extra == 0); });
    }
    {   Sets S; S.uniform(2, 20, 1000); const abpoa_hip_scoring_t sc = scoring(ABPOA_HIP_AFFINE_GAP);
        run_case("last pass, 20 reads", sc, S, 4096.0, CONS, false, "dwg", [](const DevicePlan &P) { CHECK(P.roomy && P.in_cap == 21 && P.out_cap == 21 && !P.dir && !P.rounds_possible); });
        Sets T; T.uniform(2, 6, 1000);
        run_case("last pass, 6 reads", sc, T, 4096.0, CONS, false, "wg", [](const DevicePlan &P) { CHECK(P.roomy && P.in_cap == POA_IN_CAP && P.out_cap == POA_OUT_CAP); });
        Sets U; U.uniform(1, 400, 1000);
        run_case("last pass, 400 reads", sc, U, 4096.0, CONS, false, "wg", [](const DevicePlan &P) { CHECK(P.in_cap == 250 && P.out_cap == 250 && !P.dir); });
    }
}

static void accessor_cases() {
    g_case = "accessors";
    CHECK(!opt_set("ABPOA_HIP_NO_SUCH_SWITCH") && !opt_on("ABPOA_HIP_NO_SUCH_SWITCH") && opt_int("ABPOA_HIP_NO_SUCH_SWITCH", 7) == 7);
    CHECK(set_option("ABPOA_HIP_NO_SUCH_SWITCH", "1") != 0);
    CHECK(set_option("ABPOA_HIP_VERBOSE", "0") == 0);
    CHECK(opt_set("ABPOA_HIP_VERBOSE") && !opt_on("ABPOA_HIP_VERBOSE") && opt_int("ABPOA_HIP_VERBOSE", 7) == 0);
    CHECK(set_option("ABPOA_HIP_VERBOSE", nullptr) == 0 && !opt_set("ABPOA_HIP_VERBOSE") && opt_int("ABPOA_HIP_VERBOSE", 7) == 7);
    CHECK(set_option("ABPOA_HIP_WIDE_LO", "30") == 0 && opt_on("ABPOA_HIP_WIDE_LO") && opt_int("ABPOA_HIP_WIDE_LO", 0) == 30 && set_option("ABPOA_HIP_WIDE_LO", nullptr) == 0);
    // another thread sets and resets a switch while this one reads it: every read sees one snapshot -- unset (the default) or "5"
    std::atomic<bool> stop{false};
    std::thread flip([&] { for (int i = 0; !stop.load(); ++i) set_option("ABPOA_HIP_RING_ROWS", (i & 1) ? nullptr : "5"); });
    int bad = 0;
    for (int i = 0; i < 100000; ++i) { const int v = opt_int("ABPOA_HIP_RING_ROWS", -1); (void)opt_on("ABPOA_HIP_RING_ROWS"); if (v != -1 && v != 5) bad++; }
    stop.store(true); flip.join();
    CHECK(bad == 0);
    CHECK(set_option("ABPOA_HIP_RING_ROWS", nullptr) == 0 && !opt_set("ABPOA_HIP_RING_ROWS"));
}

int main() {
    // (the harness owns every switch it tests: nothing inherited from the environment)
    for (const char *sw : {"ABPOA_HIP_NODIR", "ABPOA_HIP_NOWIDE", "ABPOA_HIP_WIDE_LO", "ABPOA_HIP_DEVICE_GENERAL", "ABPOA_HIP_NOFAST", "ABPOA_HIP_NOXL",
                           "ABPOA_HIP_RING_ROWS", "ABPOA_HIP_DIR_WIDE", "ABPOA_HIP_EXTRA_ROUTE_MIN", "ABPOA_HIP_ARENA_PCT", "ABPOA_HIP_VERBOSE"}) unsetenv(sw);
    plan_cases();
    accessor_cases();
    if (g_fail) { fprintf(stderr, "%d checks failed\n", g_fail); return 1; }
    printf("device plan ok\n");
    return 0;
}
