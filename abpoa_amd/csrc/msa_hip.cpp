// The product's binding of the read-set driver to the HIP engine: every group gets its own BatchStream.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <memory>
#include <thread>
#include <mutex>
#include "engine_options.h"
#include "batch_stream.h"
#include "msa_batch.h"
#include "msa_device.h"
#include "msa_passes.h"
#include "guide_order.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

namespace abpoa_hip {
namespace {
class HipGroupAligner : public GroupAligner {
  public:
    int init() { return bs_.open(engine_device()); }
    ~HipGroupAligner() override { add_global_stats(bs_.take_stats()); bs_.close(); }
    int prepare(const abpoa_hip_scoring_t *sc, int n, const BatchShape *shapes, int band) override {
        return bs_.prepare(sc, n, shapes, band == GA_BAND_FRESH ? BS_FRESH_BAND : (band == GA_BAND_KEEP ? (BS_FRESH_BAND | BS_WANT_BAND_STATE) : BS_WANT_BAND_STATE));
    }
    const int32_t *left(int i) override { return bs_.left(i); }
    const int32_t *right(int i) override { return bs_.right(i); }
    ProblemSlots slots(int i) override { return bs_.slots(i); }
    int run() override { return bs_.run(); }
    int status(int i) override { return bs_.rec(i).status; }
    int64_t n_cells(int i) override { return bs_.rec(i).n_cells; }
    int best_score(int i) override { return bs_.rec(i).best_score; }
    int n_cigar(int i) override { return bs_.rec(i).n_cigar; }
    const uint64_t *cigar(int i) override { return bs_.cigar(i); }
  private:
    BatchStream bs_;
};
GroupAligner *make_hip_aligner() {
    std::unique_ptr<HipGroupAligner> a(new HipGroupAligner());
    if (a->init() != 0) return nullptr;
    return a.release();
}
abpoa_hip_msa_timing_t g_timing;
abpoa_hip_gfa_timing_t g_gfa_timing;      // GFA output of the last batch call (process-wide, like g_timing)

bool strict_mode() { return opt_on("ABPOA_HIP_STRICT"); }
void free_all(abpoa_hip_msa_t *out, int n) { for (int s = 0; s < n; ++s) abpoa_hip_free_msa(&out[s]); }

void add_stats(DeviceRunStats &t, const DeviceRunStats &d) {
    t.prepare_ms += d.prepare_ms; t.rows_ms += d.rows_ms; t.tail_ms += d.tail_ms; t.fuse_ms += d.fuse_ms;
    t.device_s += d.device_s; t.cons_s += d.cons_s; t.total_s += d.total_s;
    t.n_cells += d.n_cells; t.algo_bytes += d.algo_bytes; t.n_alignments += d.n_alignments; t.n_rounds += d.n_rounds;
    t.rounds_ms += d.rounds_ms; t.rounds_launches += d.rounds_launches; t.rounds_algo_bytes += d.rounds_algo_bytes;
    t.gfa_walk_ms += d.gfa_walk_ms; t.gfa_fill_ms += d.gfa_fill_ms; t.gfa_d2h_bytes += d.gfa_d2h_bytes;
}

PassHints g_hints;      // start passes by job shape, for as long as the process lives (msa_passes.h)
// reasons of the read-sets that the last batch call handed to the host driver (abpoa_hip_get_host_reasons; index = msa_device.h HostReason)
std::mutex g_reason_mu;
int32_t g_host_reasons[MSA_HOST_REASONS];

// The device passes over the sets `idx` on ONE device queue (device, slot): msa_passes.h run_pass_ladder decides, the runner below runs one chunk of a pass
// through run_msa_device; whatever is left (listed in `left`) goes to the host driver.
struct PassOut : LadderOut { DeviceRunStats tot; };
PassOut device_passes(const abpoa_hip_scoring_t *sc, const abpoa_hip_readset_t *sets, abpoa_hip_msa_t *out, const std::vector<int> &idx,
                      int n_threads, int device, int slot, unsigned flags) {
    PassOut R;
    memset(&R.tot, 0, sizeof(R.tot));
    const bool verbose = opt_set("ABPOA_HIP_VERBOSE");
    auto gather = [&](const std::vector<int> &ix) { std::vector<abpoa_hip_readset_t> v(ix.size()); for (size_t i = 0; i < ix.size(); ++i) v[i] = sets[ix[i]]; return v; };
    auto run = [&](const std::vector<int> &chunk, int pass, double node_factor) {
        const size_t nb = chunk.size();
        const std::vector<abpoa_hip_readset_t> sub = gather(chunk);
        std::vector<abpoa_hip_msa_t> sub_out(nb);
        ChunkOut c;
        DeviceRunStats ds;
        c.rc = run_msa_device(sc, (int)nb, sub.data(), sub_out.data(), n_threads, DevicePass{node_factor, flags, device, slot}, &c.left, &ds);
        if (c.rc != ABPOA_HIP_OK) return c;
        for (size_t i = 0; i < nb; ++i) out[chunk[i]] = sub_out[i];
        add_stats(R.tot, ds);
        c.n_fit_3x = ds.n_fit_3x;
        c.n_done = (int)nb - (int)c.left.size();
        if (verbose)
            fprintf(stderr, "[abpoa-hip] device-resident driver (device %d, pass %d, node slots %gx): %zu sets, %d rounds: prepare %.1f ms, "
                            "dp rows %.1f ms, backtrack %.1f ms, fuse %.1f ms; device wall %.1f ms, results %.1f ms, total %.1f ms; "
                            "%zu sets outgrew a device capacity\n",
                    device, pass + 1, node_factor, nb, ds.n_rounds, ds.prepare_ms, ds.rows_ms, ds.tail_ms, ds.fuse_ms, ds.device_s * 1e3,
                    ds.cons_s * 1e3, ds.total_s * 1e3, c.left.size());
        if (verbose && ds.rounds_launches)
            fprintf(stderr, "[abpoa-hip]   all-rounds kernel: %.1f ms (the phase times above are its duration split by the sets' clock ticks); "
                            "mean set busy %.0f %% of it; mean set, 10^6 ticks: prepare %.1f, row loop %.1f, backtrack %.1f, fuse %.1f\n",
                    ds.rounds_ms, 100.0 * ds.rounds_mean_over_max, ds.rounds_mticks[0], ds.rounds_mticks[1], ds.rounds_mticks[2], ds.rounds_mticks[3]);
        return c;
    };
    auto resident = [&](const std::vector<int> &open) { const std::vector<abpoa_hip_readset_t> all_ = gather(open); return msa_device_resident_sets(sc, (int)all_.size(), all_.data()); };
    static_cast<LadderOut &>(R) = run_pass_ladder(idx, job_shape_key(sets, idx), g_hints, run, resident);
    return R;
}

std::vector<int> device_list() {
    int n = 0;
    (void)hipGetDeviceCount(&n);
    return parse_device_list(opt_env("ABPOA_GPU_DEVICES"), n, engine_device());
}
}  // namespace
}  // namespace abpoa_hip

// A context (include/abpoa_hip.h abpoa_hip_ctx_t): the per-caller state of the batch entry -- device, device queue (pool cache, stream, the
// all-rounds kernel's argument record), timing and last error of its own calls -- so that several host threads can run batches side by side.
struct abpoa_hip_ctx { int device; int slot; abpoa_hip_msa_timing_t timing; char err[512]; };
namespace abpoa_hip {
namespace {
std::mutex g_ctx_mu;
bool g_ctx_slot_used[MSA_DEVICE_SLOTS] = {false};
constexpr int CTX_SLOT_LO = MSA_DEVICE_SLOTS / 2;      // the upper half of the device queues belongs to contexts, the lower half to the process-wide entry

// ---- the steps of the batch entry, in the order msa_batch_impl runs them
int validate_sets(int n_sets, const abpoa_hip_readset_t *sets) {
    for (int s = 0; s < n_sets; ++s) {
        if (sets[s].n_reads < 0) return ABPOA_HIP_EINVAL;
        for (int r = 0; r < sets[s].n_reads; ++r)
            if (sets[s].lens[r] <= 0 || !sets[s].seqs[r]) { set_err("read-set %d: read %d is empty", s, r); return ABPOA_HIP_EINVAL; }
    }
    return ABPOA_HIP_OK;
}

// The device queues pull the batches from one shared counter, a host thread per queue; ctx_slot >= 0: one device queue, the context's, on ctx_device.
struct QueueRun { std::vector<int> devs; std::vector<std::vector<int>> batches; std::vector<PassOut> results; std::vector<double> busy; };
QueueRun run_device_queues(const abpoa_hip_scoring_t *sc, int n_sets, const abpoa_hip_readset_t *sets, abpoa_hip_msa_t *out, unsigned flags, int n_threads,
                           int ctx_device, int ctx_slot) {
    QueueRun Q;
    std::vector<int> &devs = Q.devs;
    devs = device_list();
    if ((int)devs.size() > CTX_SLOT_LO) devs.resize(CTX_SLOT_LO);
    if (ctx_slot >= 0) devs.assign(1, ctx_device);      // a context: its own device, its own queue
    int n_q = (int)devs.size();
    Q.batches = deal_batches(sc, sets, n_sets, n_q);
    const std::vector<std::vector<int>> &batches = Q.batches;
    // (experiment, ABPOA_HIP_RAGGED_CONCURRENT=1: the ragged batch of a mixed job on a second queue of the same device, beside the uniform batch's all-rounds kernel)
    if (n_q == 1 && ctx_slot < 0 && batches.size() == 2 && opt_on("ABPOA_HIP_RAGGED_CONCURRENT")) { devs.push_back(devs[0]); n_q = 2; }
    std::atomic<int> next{0};
    Q.results.resize(batches.size());
    Q.busy.assign(n_q, 0.0);
    auto worker = [&](int q) {
        const int thr = std::max(1, n_threads / n_q);
        for (int b_; (b_ = next.fetch_add(1)) < (int)batches.size();) {
            const auto t0 = std::chrono::steady_clock::now();
            Q.results[b_] = device_passes(sc, sets, out, batches[b_], thr, devs[q], ctx_slot >= 0 ? ctx_slot : q, flags);
            Q.busy[q] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (Q.results[b_].rc != ABPOA_HIP_OK) break;
        }
    };
    std::vector<std::thread> th;
    for (int q = 1; q < n_q; ++q) th.emplace_back(worker, q);
    worker(0);
    for (auto &t : th) t.join();
    (void)hipSetDevice(engine_device());
    return Q;
}

// Sums the batches' stats, lists the sets for the host driver (sorted) and publishes why they left; returns the first error of a batch
int merge_batches(const std::vector<PassOut> &results, DeviceRunStats &tot, std::vector<int> &todo) {
    memset(&tot, 0, sizeof(tot));
    int rc_dev = ABPOA_HIP_OK;
    for (const PassOut &R : results) {
        if (R.rc != ABPOA_HIP_OK && rc_dev == ABPOA_HIP_OK) rc_dev = R.rc;
        // a batch the device path could not take (it does not fit even alone, or its shape is not the device driver's): only THAT batch's
        // open sets go to the host driver -- R.left holds them -- the finished results of the other batches stay
        todo.insert(todo.end(), R.left.begin(), R.left.end());
        add_stats(tot, R.tot);
    }
    std::sort(todo.begin(), todo.end());
    std::lock_guard<std::mutex> lk(g_reason_mu);
    memset(g_host_reasons, 0, sizeof(g_host_reasons));
    for (const PassOut &R : results) count_host_reasons(R, g_host_reasons);
    return rc_dev;
}

void fill_timing(const QueueRun &Q, DeviceRunStats &tot, int n_threads, size_t n_host_sets, abpoa_hip_msa_timing_t &tm) {
    const int n_q = (int)Q.devs.size();
    if (n_q > 1) tot.device_s = tot.total_s = *std::max_element(Q.busy.begin(), Q.busy.end());      // queues ran side by side: the busiest one is the wall time
    if (n_q > 1 && opt_set("ABPOA_HIP_VERBOSE")) {
        fprintf(stderr, "[abpoa-hip] %d device queues, %zu batches; busy seconds per queue:", n_q, Q.batches.size());
        for (int q = 0; q < n_q; ++q) fprintf(stderr, " dev%d %.3f", Q.devs[q], Q.busy[q]);
        fprintf(stderr, "\n");
    }
    StreamStats ss;
    ss.n_launches = tot.n_rounds; ss.n_alignments = tot.n_alignments; ss.n_cells = tot.n_cells; ss.algo_bytes = tot.algo_bytes;
    ss.kernel_ms = tot.rows_ms; ss.tail_ms = tot.tail_ms;
    ss.rounds_ms = tot.rounds_ms; ss.rounds_launches = tot.rounds_launches; ss.rounds_algo_bytes = tot.rounds_algo_bytes;
    add_global_stats(ss);
    g_gfa_timing.walk_ms = tot.gfa_walk_ms; g_gfa_timing.fill_ms = tot.gfa_fill_ms; g_gfa_timing.d2h_bytes = tot.gfa_d2h_bytes;
    memset(&tm, 0, sizeof(tm));
    tm.engine_s = tot.device_s; tm.cons_s = tot.cons_s; tm.total_s = tot.total_s;
    tm.n_rounds = tot.n_rounds; tm.n_threads = n_threads; tm.n_groups = n_q;
    tm.host_sort_s = tot.prepare_ms / 1e3; tm.host_fuse_s = tot.fuse_ms / 1e3;      // device kernels now: graph -> rows, cigar -> graph
    tm.n_host_sets = (int32_t)n_host_sets;                                          // how many sets take the host driver
}

// the sets the device passes left, on the host driver
int host_leftovers(const abpoa_hip_scoring_t *sc, const abpoa_hip_readset_t *sets, abpoa_hip_msa_t *out, const std::vector<int> &todo, unsigned flags, int n_threads) {
    std::vector<abpoa_hip_readset_t> sub(todo.size());
    std::vector<abpoa_hip_msa_t> sub_out(todo.size());
    for (size_t i = 0; i < todo.size(); ++i) sub[i] = sets[todo[i]];
    abpoa_hip_msa_timing_t t2;
    const int rc = run_msa_batch(sc, (int)todo.size(), sub.data(), sub_out.data(), flags, n_threads, 0, make_hip_aligner, &t2);
    if (rc != ABPOA_HIP_OK) return rc;
    for (size_t i = 0; i < todo.size(); ++i) out[todo[i]] = sub_out[i];
    return ABPOA_HIP_OK;
}

// the whole job on the host driver: its options are not the device-resident driver's (linear gaps, extension mode, -s, no band in
// global mode, local reads beyond the local row loop)
int host_whole_job(const abpoa_hip_scoring_t *sc, int n_sets, const abpoa_hip_readset_t *sets, abpoa_hip_msa_t *out, unsigned flags, int n_threads,
                   abpoa_hip_msa_timing_t &tm) {
    if (strict_mode() && n_sets > 0) {
        set_err("ABPOA_HIP_STRICT: this job's options are the host driver's (see msa_device_eligible)");
        return ABPOA_HIP_ESTRICT;
    }
    const int rc_host = run_msa_batch(sc, n_sets, sets, out, flags, n_threads, 0, make_hip_aligner, &tm);
    tm.n_host_sets = n_sets;
    { std::lock_guard<std::mutex> lk(g_reason_mu); memset(g_host_reasons, 0, sizeof(g_host_reasons)); g_host_reasons[HOST_WHY_JOB] = n_sets; }
    return rc_host;
}

// The batch entry proper: device-resident driver first; sets that outgrow a device capacity (and whole jobs that do not fit) go to the host driver.
// `tm` receives the call's timing record; ctx_slot >= 0: one device queue, the context's, on ctx_device.
int msa_batch_impl(const abpoa_hip_scoring_t *sc_in, int n_sets, const abpoa_hip_readset_t *sets, abpoa_hip_msa_t *out, unsigned flags,
                   int n_threads, abpoa_hip_msa_timing_t &tm, int ctx_device, int ctx_slot) {
    if (engine_device() < 0) { const int rc = abpoa_hip_init(ctx_device >= 0 ? ctx_device : 0); if (rc) return rc; }
    abpoa_hip_scoring_t sc_norm;
    const abpoa_hip_scoring_t *sc = sc_in;
    if (sc_in && sc_in->align_mode == ABPOA_HIP_LOCAL_MODE) { sc_norm = *sc_in; sc_norm.wb = -1; sc = &sc_norm; }      // ref abpoa_align.c:150: local mode has no band
    if (!(n_sets > 0 && sc && sets && out && msa_device_eligible(sc, flags))) return host_whole_job(sc, n_sets, sets, out, flags, n_threads, tm);
    if (n_threads <= 0) n_threads = effective_host_cores();
    if (const int rc = validate_sets(n_sets, sets)) return rc;
    for (int s = 0; s < n_sets; ++s) memset(&out[s], 0, sizeof(out[s]));
    const QueueRun Q = run_device_queues(sc, n_sets, sets, out, flags, n_threads, ctx_device, ctx_slot);
    DeviceRunStats tot;
    std::vector<int> todo;
    const int rc_dev = merge_batches(Q.results, tot, todo);
    if (rc_dev != ABPOA_HIP_OK) { free_all(out, n_sets); return rc_dev; }
    fill_timing(Q, tot, n_threads, todo.size(), tm);
    if (todo.empty()) return ABPOA_HIP_OK;
    if (opt_set("ABPOA_HIP_VERBOSE"))
        fprintf(stderr, "[abpoa-hip] %zu of %d read-sets outgrew a device capacity: host driver for those\n", todo.size(), n_sets);
    if (strict_mode()) {
        free_all(out, n_sets);
        set_err("ABPOA_HIP_STRICT: %zu of %d read-sets would take the host driver (device capacities: node / edge / aligned slots, arena)",
                todo.size(), n_sets);
        return ABPOA_HIP_ESTRICT;
    }
    const int rc_host = host_leftovers(sc, sets, out, todo, flags, n_threads);
    if (rc_host != ABPOA_HIP_OK) free_all(out, n_sets);
    return rc_host;
}

// ---- guide-tree read order (ABPOA_HIP_PROGRESSIVE, the reference's -p): the device pre-pass orders the reads of every set, the drivers above run on a
// view of the sets in that order, and the MSA rows go back to input order.  Only the pointer arrays are permuted, no base is copied.
static_assert(GUIDE_QUEUES == MSA_DEVICE_SLOTS, "one pre-pass queue per device queue");
abpoa_hip_guide_timing_t g_guide_timing; std::mutex g_guide_timing_mu;
struct PermutedSets {
    std::vector<abpoa_hip_readset_t> sets;
    std::vector<std::vector<const uint8_t *>> seqs; std::vector<std::vector<int32_t>> lens; std::vector<std::vector<const int32_t *>> weights;
    PermutedSets(int n_sets, const abpoa_hip_readset_t *in, const GuideResult &G) : sets(n_sets), seqs(n_sets), lens(n_sets), weights(n_sets) {
        for (int s = 0; s < n_sets; ++s) {
            const int n = in[s].n_reads; const int32_t *order = G.order.data() + G.set_read0[s];
            seqs[s].resize(n); lens[s].resize(n); if (in[s].weights) weights[s].resize(n);
            for (int r = 0; r < n; ++r) { seqs[s][r] = in[s].seqs[order[r]]; lens[s][r] = in[s].lens[order[r]]; if (in[s].weights) weights[s][r] = in[s].weights[order[r]]; }
            sets[s].n_reads = n; sets[s].seqs = seqs[s].data(); sets[s].lens = lens[s].data(); sets[s].weights = in[s].weights ? weights[s].data() : nullptr;
        }
    }
};
// MSA row r of the ordered run is input read order[r]: row order[r] of what the caller gets; the consensus row stays last
// ... and GFA path r is the path of input read order[r] (the graph's read ids are positions in the guide order; P line i must be input read i)
int paths_to_input_order(abpoa_hip_msa_t &o, const int32_t *order) {
    abpoa_hip_gfa_t *g = o.gfa;
    if (o.status != ABPOA_HIP_OK || !g || g->n_path <= 0) return ABPOA_HIP_OK;
    const int n = g->n_path; const int64_t tot = g->path_off[n];
    int64_t *off = (int64_t *)calloc((size_t)n + 1, 8); int32_t *node = (int32_t *)calloc((size_t)tot + 1, 4);
    if (!off || !node) { free(off); free(node); return ABPOA_HIP_ENOMEM; }
    for (int r = 0; r < n; ++r) off[order[r] + 1] = g->path_off[r + 1] - g->path_off[r];
    for (int i = 0; i < n; ++i) off[i + 1] += off[i];
    for (int r = 0; r < n; ++r) memcpy(node + off[order[r]], g->path_node + g->path_off[r], 4 * (size_t)(g->path_off[r + 1] - g->path_off[r]));
    free(g->path_off); free(g->path_node); g->path_off = off; g->path_node = node;
    return ABPOA_HIP_OK;
}
int rows_to_input_order(abpoa_hip_msa_t &o, const int32_t *order) {
    if (const int rc = paths_to_input_order(o, order)) return rc;
    if (o.status != ABPOA_HIP_OK || !o.msa_base || o.msa_len <= 0 || o.msa_rows < o.n_reads) return ABPOA_HIP_OK;
    const size_t len = (size_t)o.msa_len;
    uint8_t *rows = (uint8_t *)malloc((size_t)o.msa_rows * len);
    if (!rows) return ABPOA_HIP_ENOMEM;
    memcpy(rows, o.msa_base, (size_t)o.msa_rows * len);
    for (int r = 0; r < o.n_reads; ++r) memcpy(rows + (size_t)order[r] * len, o.msa_base + (size_t)r * len, len);
    free(o.msa_base); o.msa_base = rows;
    return ABPOA_HIP_OK;
}
void note_guide_timing(const GuideResult &G) {
    std::lock_guard<std::mutex> lk(g_guide_timing_mu);
    g_guide_timing.sketch_ms = G.sketch_ms; g_guide_timing.pair_ms = G.pair_ms; g_guide_timing.total_s = G.total_s;
    g_guide_timing.n_minimizers = G.mm_off.empty() ? 0 : G.mm_off.back();
}

// The batch entry with the flags of include/abpoa_hip.h: without ABPOA_HIP_PROGRESSIVE, and with it outside global mode (reference abpoa_align.c:408),
// msa_batch_impl as it is.
int msa_batch_entry(const abpoa_hip_scoring_t *sc, int n_sets, const abpoa_hip_readset_t *sets, abpoa_hip_msa_t *out, unsigned flags,
                    int n_threads, abpoa_hip_msa_timing_t &tm, int ctx_device, int ctx_slot) {
    if (!(flags & ABPOA_HIP_PROGRESSIVE)) return msa_batch_impl(sc, n_sets, sets, out, flags & ~ABPOA_HIP_GUIDE_KW(0xff, 0xff), n_threads, tm, ctx_device, ctx_slot);      // (k / w mean nothing without the flag)
    const unsigned plain = flags & (ABPOA_HIP_OUT_CONS | ABPOA_HIP_OUT_MSA | ABPOA_HIP_OUT_GFA | ABPOA_HIP_AMB_STRAND);
    GuideParams gp;
    if (!sc || guide_params(sc->m, flags, &gp) != ABPOA_HIP_OK) { set_err("guide order: k-mer size / window outside 1..28 (amino acids 1..11) / 1..255"); return ABPOA_HIP_EINVAL; }
    if (sc->align_mode != ABPOA_HIP_GLOBAL_MODE || n_sets <= 0 || !sets || !out) return msa_batch_impl(sc, n_sets, sets, out, plain, n_threads, tm, ctx_device, ctx_slot);
    if (engine_device() < 0) { const int rc = abpoa_hip_init(ctx_device >= 0 ? ctx_device : 0); if (rc) return rc; }
    if (const int rc = validate_sets(n_sets, sets)) return rc;
    GuideResult G;
    if (const int rc = guide_prepass(gp, n_sets, sets, ctx_device, ctx_slot >= 0 ? ctx_slot : 0, false, G)) return rc;
    note_guide_timing(G);
    const PermutedSets P(n_sets, sets, G);
    // no strand retry under a guide order (the reference aligns every read forward there, abpoa_align.c:248-250): -s only chose the sketch's strands
    const int rc = msa_batch_impl(sc, n_sets, P.sets.data(), out, plain & ~ABPOA_HIP_AMB_STRAND, n_threads, tm, ctx_device, ctx_slot);
    if (rc != ABPOA_HIP_OK) return rc;
    for (int s = 0; s < n_sets; ++s) {
        int rc_s = rows_to_input_order(out[s], G.order.data() + G.set_read0[s]);
        if (rc_s == ABPOA_HIP_OK && (flags & ABPOA_HIP_AMB_STRAND) && !out[s].is_rc && !(out[s].is_rc = (uint8_t *)calloc((size_t)std::max(1, sets[s].n_reads), 1))) rc_s = ABPOA_HIP_ENOMEM;
        if (rc_s != ABPOA_HIP_OK) { free_all(out, n_sets); return rc_s; }
    }
    return ABPOA_HIP_OK;
}
}  // namespace
}  // namespace abpoa_hip

extern "C" {
int abpoa_hip_guide_order(const abpoa_hip_scoring_t *sc, int n_sets, const abpoa_hip_readset_t *sets, unsigned flags, abpoa_hip_guide_t *out) {
    using namespace abpoa_hip;
    refresh_options();
    GuideParams gp;
    if (!sc || n_sets < 0 || (n_sets > 0 && (!sets || !out))) return ABPOA_HIP_EINVAL;
    if (guide_params(sc->m, flags, &gp) != ABPOA_HIP_OK) { set_err("guide order: k-mer size / window outside 1..28 (amino acids 1..11) / 1..255"); return ABPOA_HIP_EINVAL; }
    if (engine_device() < 0) { const int rc = abpoa_hip_init(0); if (rc) return rc; }
    if (const int rc = validate_sets(n_sets, sets)) return rc;
    GuideResult G;
    if (const int rc = guide_prepass(gp, n_sets, sets, -1, 0, flags & ABPOA_HIP_GUIDE_SKETCH, G)) return rc;
    note_guide_timing(G);
    for (int s = 0; s < n_sets; ++s) memset(&out[s], 0, sizeof(out[s]));
    for (int s = 0; s < n_sets; ++s) {
        abpoa_hip_guide_t &o = out[s];
        const int64_t n = sets[s].n_reads, r0 = G.set_read0[s], n_hit = n * (n + 1) / 2, m0 = G.mm_off[r0], n_mm = G.mm_off[r0 + n] - m0;
        o.n_reads = (int32_t)n;
        o.order = (int32_t *)malloc(sizeof(int32_t) * (size_t)std::max<int64_t>(1, n));
        bool ok = o.order != nullptr;
        if (ok) memcpy(o.order, G.order.data() + r0, sizeof(int32_t) * (size_t)n);
        if (ok && (flags & ABPOA_HIP_GUIDE_HITS)) {
            ok = (o.hit = (int32_t *)malloc(sizeof(int32_t) * (size_t)std::max<int64_t>(1, n_hit))) != nullptr;
            if (ok) memcpy(o.hit, G.hit.data() + G.set_hit0[s], sizeof(int32_t) * (size_t)n_hit);
        }
        if (ok && (flags & ABPOA_HIP_GUIDE_SKETCH)) {
            o.mm_off = (int64_t *)malloc(sizeof(int64_t) * (size_t)(n + 1)); o.mm = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)std::max<int64_t>(1, n_mm));
            ok = o.mm_off && o.mm;
            if (ok) { for (int64_t r = 0; r <= n; ++r) o.mm_off[r] = G.mm_off[r0 + r] - m0; memcpy(o.mm, G.mm.data() + m0, sizeof(uint64_t) * (size_t)n_mm); }
        }
        if (!ok) { abpoa_hip_free_guide(out, n_sets); set_err("guide order: host memory for the results"); return ABPOA_HIP_ENOMEM; }
    }
    return ABPOA_HIP_OK;
}
void abpoa_hip_free_guide(abpoa_hip_guide_t *r, int n) {
    for (int i = 0; r && i < n; ++i) { free(r[i].order); free(r[i].hit); free(r[i].mm_off); free(r[i].mm); memset(&r[i], 0, sizeof(r[i])); }
}
void abpoa_hip_get_guide_timing(abpoa_hip_guide_timing_t *out) { std::lock_guard<std::mutex> lk(abpoa_hip::g_guide_timing_mu); if (out) *out = abpoa_hip::g_guide_timing; }
int abpoa_hip_guide_tile(void) { return abpoa_hip::guide_tile_length(); }
void abpoa_hip_get_host_reasons(int32_t *out12) {
    std::lock_guard<std::mutex> lk(abpoa_hip::g_reason_mu);
    for (int i = 0; i < abpoa_hip::MSA_HOST_REASONS; ++i) out12[i] = abpoa_hip::g_host_reasons[i];
}
int abpoa_hip_msa_batch(const abpoa_hip_scoring_t *sc, int n_sets, const abpoa_hip_readset_t *sets, abpoa_hip_msa_t *out, unsigned flags, int n_threads) {
    abpoa_hip::refresh_options();
    return abpoa_hip::msa_batch_entry(sc, n_sets, sets, out, flags, n_threads, abpoa_hip::g_timing, -1, -1);
}
void abpoa_hip_get_msa_timing(abpoa_hip_msa_timing_t *out) { *out = abpoa_hip::g_timing; }
void abpoa_hip_get_gfa_timing(abpoa_hip_gfa_timing_t *out) { if (out) *out = abpoa_hip::g_gfa_timing; }
// ---- contexts
abpoa_hip_ctx_t *abpoa_hip_ctx_create(int device) {
    using namespace abpoa_hip;
    if (engine_device() < 0) { if (abpoa_hip_init(device >= 0 ? device : 0) != ABPOA_HIP_OK) return nullptr; }
    int n = 0; (void)hipGetDeviceCount(&n);
    if (device < 0) device = engine_device();
    if (device >= n) { set_err("device %d out of range (0..%d)", device, n - 1); return nullptr; }
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    for (int s = MSA_DEVICE_SLOTS - 1; s >= CTX_SLOT_LO; --s) if (!g_ctx_slot_used[s]) {
        g_ctx_slot_used[s] = true;
        abpoa_hip_ctx *c = new abpoa_hip_ctx(); c->device = device; c->slot = s; memset(&c->timing, 0, sizeof(c->timing)); c->err[0] = 0;
        return c;
    }
    set_err("all %d batch contexts are in use", MSA_DEVICE_SLOTS - CTX_SLOT_LO);
    return nullptr;
}
void abpoa_hip_ctx_destroy(abpoa_hip_ctx_t *c) {
    if (!c) return;
    { std::lock_guard<std::mutex> lk(abpoa_hip::g_ctx_mu); abpoa_hip::g_ctx_slot_used[c->slot] = false; }
    delete c;      // (the queue's pools stay cached for the next context that takes the slot; abpoa_hip_trim releases them)
}
int abpoa_hip_msa_batch_ctx(abpoa_hip_ctx_t *c, const abpoa_hip_scoring_t *sc, int n_sets, const abpoa_hip_readset_t *sets, abpoa_hip_msa_t *out, unsigned flags, int n_threads) {
    abpoa_hip::refresh_options();
    if (!c) return ABPOA_HIP_EINVAL;
    abpoa_hip::clear_thread_error();
    const int rc = abpoa_hip::msa_batch_entry(sc, n_sets, sets, out, flags, n_threads, c->timing, c->device, c->slot);
    if (rc != ABPOA_HIP_OK) { const char *m = abpoa_hip::thread_last_error(); snprintf(c->err, sizeof(c->err), "%s", m[0] ? m : abpoa_hip_last_error()); } else c->err[0] = 0;
    return rc;
}
void abpoa_hip_ctx_get_msa_timing(const abpoa_hip_ctx_t *c, abpoa_hip_msa_timing_t *out) { if (c && out) *out = c->timing; }
const char *abpoa_hip_ctx_last_error(const abpoa_hip_ctx_t *c) { return c ? c->err : "null context"; }
void abpoa_hip_trim(void) { abpoa_hip::release_msa_device_caches(); abpoa_hip::release_guide_queues(); }
}
