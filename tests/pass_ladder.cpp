// CPU harness of tests/test_pass_ladder.py: the decisions of the batch entry (abpoa_amd/csrc/msa_passes.cpp) -- the node-slot pass ladder over a scripted
// runner, the hint store, the device list, the batches -- and the one mapping from device to host reasons (msa_device.h).  No GPU, no HIP header, no
// run_msa_device; built with -fsanitize=undefined,address and once more with -fsanitize=thread.  The expected behaviour is the rule list of DESIGN.md section 5.
#include <algorithm>
#include <set>
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <thread>
#include <utility>
#include <vector>
#include "engine_options.h"
#include "msa_passes.h"

// (the snapshot a set_option replaces is left alone on purpose -- engine_options.h -- so the leak check would report every switch this harness flips)
extern "C" const char *__asan_default_options() { return "detect_leaks=0"; }

using namespace abpoa_hip;

static int g_fail = 0;
static std::string g_case;
#define CHECK(...) do { if (!(__VA_ARGS__)) { fprintf(stderr, "FAILED %s:%d [%s] %s\n", __FILE__, __LINE__, g_case.c_str(), #__VA_ARGS__); g_fail++; } } while (0)

typedef std::vector<int> V;
typedef std::pair<double, V> Call;
typedef std::map<int, HostReason> Why;
static std::vector<Call> CL(std::initializer_list<Call> l) { return l; }
static std::vector<V> BL(std::initializer_list<V> l) { return l; }
static Why WL(std::initializer_list<Why::value_type> l) { return l; }
static V range(int lo, int hi) { V v; for (int i = lo; i < hi; ++i) v.push_back(i); return v; }

// The scripted runner: records (node factor, set indices) of every call and answers from a table -- `marks`: (pass, set) -> how the set leaves that pass;
// `rc_at`: call number -> the rc of that call (nothing runs then); `fit3x`: the sets that count for n_fit_3x when they finish.
struct Mark { HostReason why; bool edge; };
struct Script {
    std::map<std::pair<int, int>, Mark> marks; std::map<int, int> rc_at; std::set<int> fit3x;
    std::vector<Call> calls;
    int resident = 0;      // what the resident-sets query answers
    void leave(int pass, const V &sets, HostReason why, bool edge = false) { for (int s : sets) marks[{pass, s}] = Mark{why, edge}; }
    ChunkOut run(const V &chunk, int pass, double factor) {
        ChunkOut c;
        CHECK(pass >= 0 && pass < N_PASSES && factor == PASS_NODE_FACTOR[pass] && !chunk.empty());
        auto e = rc_at.find((int)calls.size());
        calls.push_back({factor, chunk});
        if (e != rc_at.end()) { c.rc = e->second; return c; }
        for (size_t i = 0; i < chunk.size(); ++i) {
            auto m = marks.find({pass, chunk[i]});
            if (m != marks.end()) c.left.push_back(SetFallback{(int)i, m->second.why, m->second.edge});
            else { c.n_done++; c.n_fit_3x += (int)fit3x.count(chunk[i]); }
        }
        return c;
    }
    LadderOut ladder(const V &idx, int key, PassHints &h) {
        calls.clear();
        return run_pass_ladder(idx, key, h, [this](const V &c, int p, double f) { return run(c, p, f); }, [this](const V &open) { CHECK(!open.empty()); return resident; });
    }
};
static bool no_hint(PassHints &h, int key) { int p = -1; return !h.find(key, &p) && p == -1; }
static bool hint_is(PassHints &h, int key, int want) { int p = -1; return h.find(key, &p) && p == want; }
static const int KEY = 10 * 1024 + 6;

static void ladder_cases() {
    const HostReason FUSE = HOST_WHY_NODES_IN_FUSE, GROW = HOST_WHY_GROWTH, INIT = HOST_WHY_NODES_AT_INIT, ARENA = HOST_WHY_DP_ARENA, EDGE = HOST_WHY_EDGE_SLOTS;
    {   g_case = "1: every set finishes at 3x";
        Script S; PassHints H; const LadderOut R = S.ladder(range(0, 6), KEY, H);
        CHECK(S.calls == CL({{3.0, range(0, 6)}}));
        CHECK(R.rc == ABPOA_HIP_OK && R.device_ok && R.left.empty() && R.why.empty() && no_hint(H, KEY));
    }
    {   g_case = "2: node-slot fall-backs climb the four passes";
        Script S; PassHints H;
        S.leave(0, {1, 3, 5, 7}, FUSE); S.leave(1, {3, 5, 7}, GROW); S.leave(2, {5, 7}, INIT); S.leave(3, {7}, ARENA);
        const LadderOut R = S.ladder(range(0, 8), KEY, H);
        CHECK(S.calls == CL({{3.0, range(0, 8)}, {4.5, {1, 3, 5, 7}}, {6.0, {3, 5, 7}}, {4096.0, {5, 7}}}));
        CHECK(R.rc == ABPOA_HIP_OK && R.device_ok && R.left == V{7} && R.why == WL({{1, FUSE}, {3, GROW}, {5, INIT}, {7, ARENA}}) && no_hint(H, KEY));
    }
    {   g_case = "3: an edge-slot set skips the middle passes and rejoins in index order";
        Script S; PassHints H;
        S.leave(0, {2}, EDGE, true); S.leave(0, {1, 4}, FUSE); S.leave(1, {4}, FUSE); S.leave(2, {4}, GROW);
        const LadderOut R = S.ladder(range(0, 6), KEY, H);
        CHECK(S.calls == CL({{3.0, range(0, 6)}, {4.5, {1, 4}}, {6.0, {4}}, {4096.0, {2, 4}}}));
        CHECK(R.rc == ABPOA_HIP_OK && R.device_ok && R.left.empty() && R.why == WL({{1, FUSE}, {2, EDGE}, {4, GROW}}) && no_hint(H, KEY));
    }
    {   g_case = "4: only the edge-slot set open: the next call is the last pass";
        Script S; PassHints H;
        S.leave(0, {2}, EDGE, true);
        const LadderOut R = S.ladder(range(0, 4), KEY, H);
        CHECK(S.calls == CL({{3.0, range(0, 4)}, {4096.0, {2}}}));
        CHECK(R.rc == ABPOA_HIP_OK && R.device_ok && R.left.empty() && R.why == WL({{2, EDGE}}) && no_hint(H, KEY));
    }
    {   g_case = "5: marked again in the last pass: returned";
        Script S; PassHints H;
        S.leave(0, {2}, EDGE, true); S.leave(3, {2}, EDGE, true);
        const LadderOut R = S.ladder(range(0, 4), KEY, H);
        CHECK(S.calls == CL({{3.0, range(0, 4)}, {4096.0, {2}}}));
        CHECK(R.rc == ABPOA_HIP_OK && R.device_ok && R.left == V{2} && R.why == WL({{2, EDGE}}) && no_hint(H, KEY));
    }
    {   g_case = "6: ENOMEM on a chunk of 5: pieces of 3 from the same position, no hint from the halved pass";
        Script S; PassHints H;
        S.leave(0, range(1, 6), FUSE); S.rc_at[1] = ABPOA_HIP_ENOMEM;
        const LadderOut R = S.ladder(range(0, 7), KEY, H);
        CHECK(S.calls == CL({{3.0, range(0, 7)}, {4.5, range(1, 6)}, {4.5, {1, 2, 3}}, {4.5, {4, 5}}}));
        CHECK(R.rc == ABPOA_HIP_OK && R.device_ok && R.left.empty() && R.why.size() == 5 && no_hint(H, KEY));
        // (the same job with room for the pass in one piece: the hint is learnt -- case 9)
    }
    {   g_case = "7a: ENOMEM on a single set: leftovers of this pass, the rest from there on, then the deferred sets";
        Script S; PassHints H; S.resident = 2;
        S.leave(0, {0}, EDGE, true); S.leave(0, {1}, FUSE); S.rc_at[1] = ABPOA_HIP_ENOMEM; S.rc_at[2] = ABPOA_HIP_ENOMEM;
        const LadderOut R = S.ladder(range(0, 6), KEY, H);
        CHECK(S.calls == CL({{3.0, {0, 1}}, {3.0, {2, 3}}, {3.0, {2}}}));
        CHECK(R.rc == ABPOA_HIP_OK && !R.device_ok && R.left == V{1, 2, 3, 4, 5, 0} && R.why == WL({{0, EDGE}, {1, FUSE}}) && no_hint(H, KEY));
    }
    {   g_case = "7b: EINVAL in the last pass: leftovers, the rest, then the hopeless sets";
        Script S; PassHints H; S.resident = 2;
        S.leave(0, range(0, 5), EDGE, true); S.leave(0, {5}, FUSE); S.leave(1, {5}, FUSE); S.leave(2, {5}, FUSE);
        S.leave(3, {0}, EDGE, true); S.leave(3, {1}, ARENA); S.rc_at[6] = ABPOA_HIP_EINVAL;
        const LadderOut R = S.ladder(range(0, 6), KEY, H);
        CHECK(S.calls == CL({{3.0, {0, 1}}, {3.0, {2, 3}}, {3.0, {4, 5}}, {4.5, {5}}, {6.0, {5}}, {4096.0, {0, 1}}, {4096.0, {2, 3}}}));
        CHECK(R.rc == ABPOA_HIP_OK && !R.device_ok && R.left == V{1, 2, 3, 4, 5, 0});
        CHECK(R.why == WL({{0, EDGE}, {1, ARENA}, {2, EDGE}, {3, EDGE}, {4, EDGE}, {5, FUSE}}) && no_hint(H, KEY));
    }
    {   g_case = "8: any other rc ends the ladder at once";
        Script S; PassHints H; S.rc_at[0] = ABPOA_HIP_ENODEV;
        const LadderOut R = S.ladder(range(0, 4), KEY, H);
        CHECK(S.calls.size() == 1 && R.rc == ABPOA_HIP_ENODEV && R.left.empty() && R.why.empty() && no_hint(H, KEY));
        Script T; T.leave(0, {1, 2, 3}, FUSE); T.rc_at[1] = ABPOA_HIP_ELAUNCH;
        const LadderOut Q = T.ladder(range(0, 4), KEY, H);
        CHECK(T.calls.size() == 2 && Q.rc == ABPOA_HIP_ELAUNCH && Q.left.empty() && no_hint(H, KEY));
    }
}

static void hint_cases() {
    const HostReason FUSE = HOST_WHY_NODES_IN_FUSE;
    PassHints H;      // (shared by 9 .. 12)
    {   g_case = "9: the hint is learnt: most sets outgrew 3x, 4.5x held them in one piece";
        Script S; S.leave(0, range(1, 7), FUSE);
        const LadderOut R = S.ladder(range(0, 8), KEY, H);
        CHECK(S.calls == CL({{3.0, range(0, 8)}, {4.5, range(1, 7)}}) && R.left.empty() && hint_is(H, KEY, 1) && no_hint(H, KEY + 1));
    }
    {   g_case = "9a: not learnt in the last pass";
        Script S; PassHints G; S.leave(0, range(1, 7), FUSE); S.leave(1, range(1, 7), FUSE); S.leave(2, range(1, 7), FUSE);
        const LadderOut R = S.ladder(range(0, 8), KEY, G);
        CHECK(S.calls.size() == 4 && S.calls[3] == Call({4096.0, range(1, 7)}) && R.left.empty() && no_hint(G, KEY));
    }
    {   g_case = "9b: not learnt when the previous pass left fewer than half";
        Script S; PassHints G; S.leave(0, {1, 2, 3}, FUSE);
        const LadderOut R = S.ladder(range(0, 8), KEY, G);
        CHECK(S.calls.size() == 2 && R.left.empty() && no_hint(G, KEY));
        Script T; T.leave(0, {1, 2, 3, 4}, FUSE);      // (exactly half counts as most)
        T.ladder(range(0, 8), KEY, G);
        CHECK(hint_is(G, KEY, 1));
    }
    {   g_case = "9c: not learnt while the pass still leaves half of its sets";
        Script S; PassHints G; S.leave(0, range(1, 7), FUSE); S.leave(1, {1, 2, 3}, FUSE); S.leave(2, {1, 2}, FUSE);
        const LadderOut R = S.ladder(range(0, 8), KEY, G);
        CHECK(S.calls.size() == 4 && R.left.empty() && no_hint(G, KEY));
        Script T; T.leave(0, range(1, 7), FUSE); T.leave(1, {1, 2, 3}, FUSE);      // (6x holds what 4.5x did not: jobs of this shape start at 6x)
        T.ladder(range(0, 8), KEY, G);
        CHECK(T.calls.size() == 3 && hint_is(G, KEY, 2));
    }
    {   g_case = "9d: not learnt from a pass that was halved";
        Script S; PassHints G; S.leave(0, range(1, 7), FUSE); S.rc_at[1] = ABPOA_HIP_ENOMEM;
        const LadderOut R = S.ladder(range(0, 8), KEY, G);
        CHECK(S.calls == CL({{3.0, range(0, 8)}, {4.5, range(1, 7)}, {4.5, {1, 2, 3}}, {4.5, {4, 5, 6}}}) && R.left.empty() && no_hint(G, KEY));
    }
    {   g_case = "9e: not learnt when the device path gave up";
        Script S; PassHints G; S.resident = 4; S.leave(0, range(1, 7), FUSE); S.rc_at[3] = ABPOA_HIP_EINVAL;
        const LadderOut R = S.ladder(range(0, 8), KEY, G);
        CHECK(S.calls == CL({{3.0, {0, 1, 2, 3}}, {3.0, {4, 5, 6, 7}}, {4.5, {1, 2, 3, 4}}, {4.5, {5, 6}}}));
        CHECK(!R.device_ok && R.rc == ABPOA_HIP_OK && R.left == V{5, 6} && no_hint(G, KEY));
    }
    {   g_case = "10: a second ladder of the same shape starts at the learnt pass";
        Script S;
        const LadderOut R = S.ladder(range(0, 8), KEY, H);
        CHECK(S.calls == CL({{4.5, range(0, 8)}}) && R.left.empty() && hint_is(H, KEY, 1));
        Script T; T.ladder(range(0, 8), KEY + 1, H);      // (another shape: from 3x)
        CHECK(T.calls == CL({{3.0, range(0, 8)}}));
    }
    {   g_case = "11: ABPOA_HIP_NO_PASS_HINT ignores the hint (reads only: it is still written)";
        CHECK(set_option("ABPOA_HIP_NO_PASS_HINT", "1") == 0);
        Script S; const LadderOut R = S.ladder(range(0, 8), KEY, H);
        CHECK(S.calls == CL({{3.0, range(0, 8)}}) && R.left.empty() && hint_is(H, KEY, 1));
        Script T; PassHints G; T.leave(0, range(1, 7), FUSE); T.ladder(range(0, 8), KEY, G);
        CHECK(hint_is(G, KEY, 1));
        CHECK(set_option("ABPOA_HIP_NO_PASS_HINT", nullptr) == 0);
        Script U; U.ladder(range(0, 8), KEY, H);
        CHECK(U.calls == CL({{4.5, range(0, 8)}}));
    }
    {   g_case = "12: the hint is forgotten when more than half of the finished sets fit 3x";
        Script S; S.fit3x = {0, 1, 2, 3}; S.leave(1, {7}, FUSE);      // 4 of the 7 finished sets
        S.ladder(range(0, 8), KEY, H);
        CHECK(S.calls == CL({{4.5, range(0, 8)}, {6.0, {7}}}) && no_hint(H, KEY));
        H.set(KEY, 1);
        Script T; T.fit3x = {0, 1, 2, 3};      // exactly half of 8: kept
        T.ladder(range(0, 8), KEY, H);
        CHECK(T.calls == CL({{4.5, range(0, 8)}}) && hint_is(H, KEY, 1));
        Script U; U.fit3x = {0, 1, 2, 3, 4}; U.leave(0, range(1, 7), FUSE);      // a ladder that started at 3x forgets nothing (and learns 1 again)
        PassHints G; G.set(KEY + 2, 2); U.ladder(range(0, 8), KEY, G);
        CHECK(hint_is(G, KEY, 1) && hint_is(G, KEY + 2, 2));
    }
}

static void switch_cases() {
    const HostReason FUSE = HOST_WHY_NODES_IN_FUSE;
    auto first_factor = [](PassHints &h) { Script S; S.ladder(range(0, 4), KEY, h); return S.calls.at(0).first; };
    auto sizes = [](int resident) { Script S; PassHints h; S.resident = resident; S.ladder(range(0, 7), KEY, h); V n; for (const Call &c : S.calls) n.push_back((int)c.second.size()); return n; };
    {   g_case = "13: ABPOA_HIP_FIRST_PASS";
        PassHints none, two; two.set(KEY, 2);
        CHECK(first_factor(none) == 3.0);
        for (const char *v : {"1", "2", "3"}) { CHECK(set_option("ABPOA_HIP_FIRST_PASS", v) == 0); CHECK(first_factor(none) == PASS_NODE_FACTOR[atoi(v)]); }
        CHECK(first_factor(two) == 6.0);      // (the stored hint overrides the switch)
        CHECK(set_option("ABPOA_HIP_NO_PASS_HINT", "1") == 0 && first_factor(two) == 4096.0 && set_option("ABPOA_HIP_NO_PASS_HINT", nullptr) == 0);
        for (const char *v : {"0", "4", "-1"}) { CHECK(set_option("ABPOA_HIP_FIRST_PASS", v) == 0); CHECK(first_factor(none) == 3.0); }
        {   // a ladder that starts at 6x: what it leaves goes on to the last pass, and the sets it finished count for forgetting
            CHECK(set_option("ABPOA_HIP_FIRST_PASS", "2") == 0);
            Script S; PassHints h; S.leave(2, {1}, FUSE); const LadderOut R = S.ladder(range(0, 4), KEY, h);
            CHECK(S.calls == CL({{6.0, range(0, 4)}, {4096.0, {1}}}) && R.left.empty());
        }
        CHECK(set_option("ABPOA_HIP_FIRST_PASS", nullptr) == 0 && first_factor(none) == 3.0);
    }
    {   g_case = "13: ABPOA_HIP_PASS_SETS and the resident-sets cap";
        CHECK(sizes(0) == V{7} && sizes(-1) == V{7} && sizes(100) == V{7});
        CHECK(sizes(2) == V{2, 2, 2, 1});
        CHECK(set_option("ABPOA_HIP_PASS_SETS", "3") == 0);
        CHECK(sizes(0) == V{3, 3, 1} && sizes(5) == V{3, 3, 1} && sizes(2) == V{2, 2, 2, 1});
        CHECK(set_option("ABPOA_HIP_PASS_SETS", "0") == 0 && sizes(0) == V{7});
        CHECK(set_option("ABPOA_HIP_PASS_SETS", nullptr) == 0 && sizes(0) == V{7} && sizes(4) == V{4, 3});
        // per pass: the cap applies to what is open in that pass
        CHECK(set_option("ABPOA_HIP_PASS_SETS", "3") == 0);
        Script S; PassHints h; S.leave(0, {0, 2, 4, 6}, FUSE); S.ladder(range(0, 7), KEY, h);
        CHECK(S.calls == CL({{3.0, {0, 1, 2}}, {3.0, {3, 4, 5}}, {3.0, {6}}, {4.5, {0, 2, 4}}, {4.5, {6}}}));
        CHECK(set_option("ABPOA_HIP_PASS_SETS", nullptr) == 0);
    }
}

struct Sets {      // read-sets by lengths alone: nothing here looks at a base
    std::vector<std::vector<int32_t>> lens; std::vector<abpoa_hip_readset_t> rs;
    void add(std::vector<int32_t> l) { lens.push_back(std::move(l)); }
    const abpoa_hip_readset_t *get() {
        rs.resize(lens.size());
        for (size_t s = 0; s < lens.size(); ++s) { rs[s].n_reads = (int)lens[s].size(); rs[s].seqs = nullptr; rs[s].lens = lens[s].data(); rs[s].weights = nullptr; }
        return rs.data();
    }
    int n() const { return (int)lens.size(); }
};
static abpoa_hip_scoring_t banded_global() {
    abpoa_hip_scoring_t sc = abpoa_hip_scoring_t();
    sc.align_mode = ABPOA_HIP_GLOBAL_MODE; sc.wb = 10; sc.wf = 0.01f;
    return sc;
}

static void dealing_cases() {
    const abpoa_hip_scoring_t sc = banded_global();
    {   g_case = "shape key";
        Sets S; S.add({1000, 900, 1000}); S.add({1024, 5}); S.add(std::vector<int32_t>(2000, 3)); S.add({1025});
        CHECK(job_shape_key(S.get(), {0}) == 10 * 1024 + 3 && job_shape_key(S.get(), {0, 1}) == 10 * 1024 + 3 && job_shape_key(S.get(), {3, 0}) == 11 * 1024 + 3);
        CHECK(job_shape_key(S.get(), {2}) == 2 * 1024 + 1023 && job_shape_key(S.get(), {}) == 0);
    }
    {   g_case = "14: one queue: one batch in caller order";
        Sets S; for (int s = 0; s < 9; ++s) S.add(std::vector<int32_t>((size_t)(2 + s % 3), 100 * (9 - s)));
        CHECK(deal_batches(&sc, S.get(), S.n(), 1) == BL({range(0, 9)}));
    }
    {   g_case = "15: 2 queues x 5000 sets of mixed cost";
        Sets S; std::vector<int64_t> cost;
        for (int s = 0; s < 5000; ++s) { const int nr = 2 + (s * 7) % 5, len = 200 + (s * 37) % 900; S.add(std::vector<int32_t>((size_t)nr, len)); cost.push_back((int64_t)nr * len * nr); }
        const std::vector<V> B = deal_batches(&sc, S.get(), S.n(), 2);
        CHECK(B.size() == 4);
        V where(5000, -1); int n_seen = 0;
        for (size_t b = 0; b < B.size(); ++b) { CHECK(std::is_sorted(B[b].begin(), B[b].end())); for (int s : B[b]) { CHECK(s >= 0 && s < 5000 && where[s] == -1); where[s] = (int)b; n_seen++; } }
        CHECK(n_seen == 5000 && B.size() == 4 && B[0].size() == 1250 && B[3].size() == 1250);
        V order = range(0, 5000);
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cost[a] > cost[b]; });
        int misdealt = 0; for (int i = 0; i < 5000; ++i) misdealt += where[order[i]] != i % 4;      // heaviest first, round-robin
        CHECK(misdealt == 0);
        CHECK(set_option("ABPOA_GPU_BATCHES_PER_DEVICE", "1") == 0 && deal_batches(&sc, S.get(), S.n(), 2).size() == 2);
        CHECK(set_option("ABPOA_GPU_BATCHES_PER_DEVICE", nullptr) == 0 && deal_batches(&sc, S.get(), S.n(), 2).size() == 4);
    }
    {   g_case = "16: fewer sets than queues";
        Sets S; S.add({100, 100}); S.add({300, 300});
        CHECK(deal_batches(&sc, S.get(), S.n(), 4) == BL({{1}, {0}}));
        CHECK(deal_batches(&sc, S.get(), 1, 4) == BL({{0}}));
    }
    {   g_case = "17: split_ragged";
        Sets S; S.add({1000, 1000, 1000}); S.add({1000, 600}); S.add({1000, 950}); S.add({1000, 1000, 100}); S.add({500});
        const std::vector<V> mixed = {{0, 1, 2, 3}, {0, 2, 4}, {1, 3}};
        auto split = [&](const abpoa_hip_scoring_t *sc_) { std::vector<V> b = mixed; split_ragged(b, sc_, S.get()); return b; };
        CHECK(split(&sc) == BL({{0, 2}, {1, 3}, {0, 2, 4}, {1, 3}}));      // only the mixed batch is split
        CHECK(deal_batches(&sc, S.get(), S.n(), 1) == BL({{0, 2, 4}, {1, 3}}));
        abpoa_hip_scoring_t nb = sc; nb.wb = -1; CHECK(split(&nb) == mixed);
        abpoa_hip_scoring_t lo = sc; lo.align_mode = ABPOA_HIP_LOCAL_MODE; CHECK(split(&lo) == mixed);
        CHECK(split(nullptr) == mixed);
        CHECK(set_option("ABPOA_HIP_NO_RAGGED_SPLIT", "1") == 0 && split(&sc) == mixed);
        CHECK(set_option("ABPOA_HIP_NO_RAGGED_SPLIT", nullptr) == 0 && split(&sc).size() == 4);
    }
    {   g_case = "18: parse_device_list";
        CHECK(parse_device_list("all", 3, 1) == V{0, 1, 2});
        CHECK(parse_device_list("0,0", 1, 0) == V{0, 0});
        CHECK(parse_device_list("1,x", 2, 0) == V{1});
        CHECK(parse_device_list("x", 2, 1) == V{1});
        CHECK(parse_device_list("5", 2, 1) == V{1} && parse_device_list("0,7,1", 2, 1) == V{0, 1} && parse_device_list("-1", 2, 0) == V{0});
        CHECK(parse_device_list("", 4, 2) == V{2} && parse_device_list(nullptr, 4, 2) == V{2} && parse_device_list("all", 0, 3) == V{3});
        CHECK(parse_device_list("0,1,0,1,0,1,0,1,0,1,0,1,0,1,0,1,0,1,0,1", 2, 0).size() == (size_t)MSA_DEVICE_SLOTS);
        CHECK(parse_device_list("all", MSA_DEVICE_SLOTS + 8, 0) == range(0, MSA_DEVICE_SLOTS));
    }
}

static void reason_cases() {
    g_case = "19: host_reason_of";
    const int dev[] = {POA_WHY_NONE, POA_WHY_NODES_AT_INIT, POA_WHY_PRED_SLOTS, POA_WHY_CIGAR_SLOTS, POA_WHY_NODES_IN_FUSE, POA_WHY_EDGE_SLOTS, POA_WHY_GROWTH,
                       POA_WHY_ORDER_WALK, POA_WHY_RANK_WALK};
    for (int i = 0; i < 9; ++i) CHECK(dev[i] == i && host_reason_of(dev[i]) == (HostReason)i);      // today's values, slot for slot
    CHECK(POA_WHY_DP_STATUS == 1000 && host_reason_of(1000 + ABPOA_HIP_STATUS_OVERFLOW) == HOST_WHY_DP_ARENA && HOST_WHY_DP_ARENA == 9);
    CHECK(host_reason_of(1000 + ABPOA_HIP_STATUS_NEED_SCORES) == HOST_WHY_DP_OTHER && host_reason_of(1000) == HOST_WHY_DP_OTHER && host_reason_of(1007) == HOST_WHY_DP_OTHER);
    CHECK(HOST_WHY_DP_OTHER == 10 && HOST_WHY_JOB == 11 && MSA_HOST_REASONS == 12);
    for (int r : {-1, -1000, 9, 10, 11, 12, 99, 999}) CHECK(host_reason_of(r) == HOST_WHY_OTHER);
    g_case = "count_host_reasons";
    LadderOut R; R.left = {1, 2, 3, 5}; R.why = {{1, HOST_WHY_EDGE_SLOTS}, {3, HOST_WHY_DP_ARENA}, {5, HOST_WHY_OTHER}, {9, HOST_WHY_GROWTH}};
    int32_t hist[MSA_HOST_REASONS] = {0}; hist[HOST_WHY_JOB] = 2;
    count_host_reasons(R, hist);
    for (int i = 0; i < MSA_HOST_REASONS; ++i) CHECK(hist[i] == (i == HOST_WHY_JOB ? 3 : (i == HOST_WHY_EDGE_SLOTS || i == HOST_WHY_DP_ARENA || i == HOST_WHY_OTHER) ? 1 : 0));
}

// 21: two threads, 200 ladders each, one shape key, one hint store: every second ladder learns the hint, the others forget it
static void thread_case() {
    g_case = "21: two threads on one hint store";
    PassHints H; int bad[2] = {0, 0};
    auto work = [&](int t) {
        for (int i = 0; i < 200; ++i) {
            Script S;
            if ((i + t) & 1) S.leave(0, range(1, 7), HOST_WHY_NODES_IN_FUSE); else S.fit3x = {0, 1, 2, 3, 4, 5};
            std::vector<Call> calls;
            const LadderOut R = run_pass_ladder(range(0, 8), KEY, H, [&](const V &c, int p, double f) { calls.push_back({f, c}); return S.run(c, p, f); }, [](const V &) { return 0; });
            const double f0 = calls.at(0).first;
            if (R.rc != ABPOA_HIP_OK || !R.device_ok || !R.left.empty() || (f0 != 3.0 && f0 != 4.5) || calls.size() > 2) bad[t]++;
        }
    };
    std::thread other(work, 1);
    work(0);
    other.join();
    int p = 1;
    H.find(KEY, &p);      // (learnt or forgotten last: either, but nothing else)
    CHECK(bad[0] == 0 && bad[1] == 0 && p == 1);
}

int main() {
    // (the harness owns every switch it tests: nothing inherited from the environment)
    for (const char *sw : {"ABPOA_HIP_FIRST_PASS", "ABPOA_HIP_NO_PASS_HINT", "ABPOA_HIP_PASS_SETS", "ABPOA_HIP_NO_RAGGED_SPLIT", "ABPOA_GPU_BATCHES_PER_DEVICE"}) unsetenv(sw);
    ladder_cases();
    hint_cases();
    switch_cases();
    dealing_cases();
    reason_cases();
    thread_case();
    printf("MSA_HOST_REASONS %d\n", MSA_HOST_REASONS);
    if (g_fail) { fprintf(stderr, "%d checks failed\n", g_fail); return 1; }
    printf("pass ladder ok\n");
    return 0;
}
