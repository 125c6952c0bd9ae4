// The batch entry's decisions (msa_passes.h): pass ladder, hint store, device list, batches.  Host logic only.
#include <algorithm>
#include <stdlib.h>
#include <string.h>
#include "engine_options.h"
#include "msa_passes.h"

namespace abpoa_hip {

bool PassHints::find(int key, int *pass) {
    std::lock_guard<std::mutex> lk(mu_);
    auto it = start_.find(key);
    if (it == start_.end()) return false;
    *pass = it->second;
    return true;
}
void PassHints::set(int key, int pass) { std::lock_guard<std::mutex> lk(mu_); start_[key] = pass; }
void PassHints::erase(int key) { std::lock_guard<std::mutex> lk(mu_); start_.erase(key); }

int job_shape_key(const abpoa_hip_readset_t *sets, const std::vector<int> &idx) {
    int mx = 1, nr = 0;
    for (int i : idx) {
        nr = std::max(nr, sets[i].n_reads);
        for (int r = 0; r < sets[i].n_reads; ++r) mx = std::max(mx, sets[i].lens[r]);
    }
    int lg = 0;
    while ((1 << lg) < mx) ++lg;
    return lg * 1024 + std::min(nr, 1023);
}

LadderOut run_pass_ladder(const std::vector<int> &idx, int key, PassHints &hints, const ChunkRunner &run, const ResidentSets &resident) {
    LadderOut R;
    constexpr int LAST = N_PASSES - 1;
    std::vector<int> todo = idx, left;
    std::vector<int> deferred, hopeless;      // out of edge slots before the last pass / in it
    int first_pass = 0;
    {   // (profiling runs of one step: start where a warmed-up process would)
        const int fp = opt_int("ABPOA_HIP_FIRST_PASS", 0);
        if (fp >= 1 && fp < N_PASSES) first_pass = fp;
    }
    if (!opt_on("ABPOA_HIP_NO_PASS_HINT")) hints.find(key, &first_pass);
    bool most_outgrew = false;        // (of the previous pass)
    int n_small = 0, n_done = 0;      // (sets that would also have fitted the 3x estimate / sets that finished)
    for (int pass = first_pass; pass < N_PASSES && (!todo.empty() || !deferred.empty()); ++pass) {
        if (todo.empty()) pass = LAST;
        if (pass == LAST) { todo.insert(todo.end(), deferred.begin(), deferred.end()); deferred.clear(); std::sort(todo.begin(), todo.end()); }
        left.clear();
        size_t chunk = todo.size();
        bool halved = false;          // (the pass did not fit the device memory in the pieces first tried)
        {   // wide-band jobs: passes of what the device holds at once (msa_device.h)
            const int res_ = resident(todo);
            if (res_ > 0 && chunk > (size_t)res_) chunk = (size_t)res_;
            const int ps_ = opt_int("ABPOA_HIP_PASS_SETS", 0);      // (tests: several passes on a small job)
            if (ps_ > 0 && chunk > (size_t)ps_) chunk = (size_t)ps_;
        }
        for (size_t at = 0; at < todo.size();) {
            const size_t nb = std::min(chunk, todo.size() - at);
            const std::vector<int> sub(todo.begin() + at, todo.begin() + at + nb);
            const ChunkOut c = run(sub, pass, PASS_NODE_FACTOR[pass]);
            if (c.rc == ABPOA_HIP_ENOMEM && nb > 1) { chunk = (nb + 1) / 2; halved = true; continue; }      // split and retry this chunk
            if (c.rc != ABPOA_HIP_OK) {
                if (c.rc != ABPOA_HIP_ENOMEM && c.rc != ABPOA_HIP_EINVAL) { R.rc = c.rc; return R; }
                // not a job for the device path (does not fit even alone / shape): what is still open -- the leftovers of the chunks
                // already done in this pass and everything from here on -- goes back to the caller
                R.device_ok = false;
                left.insert(left.end(), todo.begin() + at, todo.end());
                break;
            }
            for (const SetFallback &f : c.left) {
                const int s = sub[f.set];
                (!f.edge_slots ? left : pass < LAST ? deferred : hopeless).push_back(s);
                R.why[s] = f.why;
            }
            n_small += c.n_fit_3x;
            n_done += c.n_done;
            at += nb;
        }
        if (!R.device_ok) { todo.swap(left); break; }
        const bool outgrew_now = left.size() * 2 >= todo.size();
        if (pass > 0 && pass < LAST && most_outgrew && !outgrew_now && !halved) hints.set(key, pass);
        most_outgrew = outgrew_now;
        if (pass == first_pass && first_pass > 0 && n_done > 0 && n_small * 2 > n_done) hints.erase(key);
        todo.swap(left);
    }
    R.left = todo;
    R.left.insert(R.left.end(), deferred.begin(), deferred.end());      // (only when the device path gave up on the job)
    R.left.insert(R.left.end(), hopeless.begin(), hopeless.end());
    return R;
}

void count_host_reasons(const LadderOut &R, int32_t *hist) {
    for (int s : R.left) { auto it = R.why.find(s); hist[it == R.why.end() ? HOST_WHY_JOB : it->second]++; }
}

std::vector<int> parse_device_list(const char *text, int n_devices, int engine_device) {
    std::vector<int> d;
    if (text && *text) {
        if (!strcmp(text, "all")) { for (int i = 0; i < n_devices; ++i) d.push_back(i); }
        else for (const char *q = text; *q;) {
            char *end;
            const long v = strtol(q, &end, 10);
            if (end == q) break;
            if (v >= 0 && v < n_devices) d.push_back((int)v);
            if (*end && *end != ',') break;
            q = *end == ',' ? end + 1 : end;
        }
    }
    if (d.empty()) d.push_back(engine_device);
    if ((int)d.size() > MSA_DEVICE_SLOTS) d.resize(MSA_DEVICE_SLOTS);
    return d;
}

void split_ragged(std::vector<std::vector<int>> &batches, const abpoa_hip_scoring_t *sc, const abpoa_hip_readset_t *sets) {
    if (!sc || sc->wb < 0 || sc->align_mode == ABPOA_HIP_LOCAL_MODE || opt_on("ABPOA_HIP_NO_RAGGED_SPLIT")) return;
    std::vector<std::vector<int>> out_;
    for (auto &b_ : batches) {
        std::vector<int> uni, rag;
        for (int i : b_) (msa_device_set_is_ragged(sets[i]) ? rag : uni).push_back(i);
        if (uni.empty() || rag.empty()) { out_.push_back(std::move(b_)); continue; }
        out_.push_back(std::move(uni)); out_.push_back(std::move(rag));
    }
    batches.swap(out_);
}
std::vector<std::vector<int>> deal_batches(const abpoa_hip_scoring_t *sc, const abpoa_hip_readset_t *sets, int n_sets, int n_q) {
    std::vector<std::vector<int>> batches;
    if (n_q == 1) {
        batches.emplace_back(n_sets);
        for (int s = 0; s < n_sets; ++s) batches[0][s] = s;
        split_ragged(batches, sc, sets);
        return batches;
    }
    std::vector<int64_t> cost(n_sets);
    for (int s = 0; s < n_sets; ++s) {
        int64_t sum = 0;
        for (int r = 0; r < sets[s].n_reads; ++r) sum += sets[s].lens[r];
        cost[s] = sum * std::max(1, sets[s].n_reads);
    }
    std::vector<int> order(n_sets);
    for (int s = 0; s < n_sets; ++s) order[s] = s;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cost[a] > cost[b]; });
    const int per_q = std::max(1, opt_int("ABPOA_GPU_BATCHES_PER_DEVICE", 2));
    // a batch should hold >= 1024 sets when the job allows: the device kernels run one wavefront per read-set, a GPU has 1024 SIMDs, and the
    // all-rounds kernel of the narrow-band jobs is at its best with ~1000 resident sets; never fewer batches than queues
    int nb = std::max(n_q, std::min(n_q * per_q, n_sets / 1024));
    nb = std::max(1, std::min(nb, n_sets));
    batches.resize(nb);
    for (int i = 0; i < n_sets; ++i) batches[i % nb].push_back(order[i]);
    for (auto &b_ : batches) std::sort(b_.begin(), b_.end());        // (caller order inside a batch)
    split_ragged(batches, sc, sets);
    return batches;
}

}  // namespace abpoa_hip
