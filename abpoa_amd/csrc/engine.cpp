// Host side of the engine: device binding, BatchStream (pinned staging + HBM pools + launch) and the flat
// batch API of include/abpoa_hip.h on top of it.  Compiled with hipcc.  Every HIP call of the flat driver is made
// here; its sizes, offsets and routing answers come from batch_plan.cpp.
//
// Replaces the per-alignment driver simd_abpoa_align_sequence_to_subgraph
// (reference src/simd_abpoa_align.c:1645-1712) and the scratch owner simd_abpoa_realloc (:1178-1208):
// instead of one strided rows x (qlen+1) matrix per abpoa_t, a batch shares three grow-only HBM pools
// (inputs, per-row outputs, band-compacted score-plane arenas).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdarg.h>
#include <limits.h>
#include <mutex>
#include <vector>
#include <algorithm>
#include "engine_options.h"
#include "batch_stream.h"

namespace abpoa_hip {

// Last error of the PROCESS (the batch calls run on worker threads; the caller reads the message from its own thread).  Readers get a
// per-thread copy taken under the lock.
static char g_err[512] = ""; static std::mutex g_err_mu;
static thread_local char g_err_copy[512] = "";
static thread_local char tl_err[512] = "";      // last error raised on THIS thread (a context's call copies it: abpoa_hip_ctx_last_error)
void set_err(const char *fmt, ...) {
    va_list ap; va_start(ap, fmt); vsnprintf(tl_err, sizeof(tl_err), fmt, ap); va_end(ap);
    std::lock_guard<std::mutex> lk(g_err_mu);
    memcpy(g_err, tl_err, sizeof(g_err));
}
const char *thread_last_error() { return tl_err; }
void clear_thread_error() { tl_err[0] = 0; }
#define HIP_TRY(expr, code)                                                                          \
    do { hipError_t e_ = (expr); if (e_ != hipSuccess) {                                             \
        set_err("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); return code; } } while (0)

int Blob::reserve(size_t n) {
    if (n <= cap) return 0;
    size_t want = std::max(n, cap + cap / 2);
    want = (want + 0xFFFFF) & ~(size_t)0xFFFFF;
    release();
    if (hipMalloc((void **)&dev, want) != hipSuccess) { dev = nullptr; set_err("hipMalloc(%zu) failed", want); return ABPOA_HIP_ENOMEM; }
    if (mirrored && hipHostMalloc((void **)&host, want, hipHostMallocDefault) != hipSuccess) {
        host = nullptr; set_err("hipHostMalloc(%zu) failed", want); return ABPOA_HIP_ENOMEM; }
    cap = want; return 0;
}
void Blob::release() { if (dev) (void)hipFree(dev); if (host) (void)hipHostFree(host); dev = host = nullptr; cap = 0; }

struct Engine {
    bool ready = false; int device = -1;
    BatchStream flat;                  // default stream of the flat C API
    abpoa_hip_stats_t stats{};
    std::mutex mu, stats_mu;
};
static Engine g;
long long g_dbg[CLK_SLOTS] = {0};      // (abpoa_hip__debug_clocks; slots: diag.h)
long long g_dir_counts[2] = {0, 0};      // alignments whose backtrack walked a direction plane; alignments redone with score records (NEED_SCORES)
long long g_row_launches[3] = {0, 0, 0}; // launches of the narrow row kernel, of dp_wide_kernel, of dp_xl_kernel (launch_dp_fast counts, abpoa_hip__row_launches reads)

int engine_device() { return g.ready ? g.device : -1; }
int device_cu_count(int device) {
    hipDeviceProp_t pr;
    if (device < 0 && hipGetDevice(&device) != hipSuccess) return 256;
    return (hipGetDeviceProperties(&pr, device) == hipSuccess && pr.multiProcessorCount > 0) ? pr.multiProcessorCount : 256;
}
void add_global_stats(const StreamStats &s) {
    std::lock_guard<std::mutex> lk(g.stats_mu);
    g.stats.n_launches += s.n_launches; g.stats.n_alignments += s.n_alignments; g.stats.n_cells += s.n_cells;
    g.stats.algo_bytes += s.algo_bytes; g.stats.kernel_ms += s.kernel_ms; g.stats.h2d_ms += s.h2d_ms; g.stats.d2h_ms += s.d2h_ms; g.stats.tail_ms += s.tail_ms; g.stats.rounds_ms += s.rounds_ms;
    g.stats.rounds_launches += s.rounds_launches; g.stats.rounds_algo_bytes += s.rounds_algo_bytes;
}

// ------------------------------------------------------------------------------------------------ BatchStream
int BatchStream::open(int device) {
    if (open_) return 0;
    HIP_TRY(hipSetDevice(device), ABPOA_HIP_ENODEV);
    HIP_TRY(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking), ABPOA_HIP_ENODEV);
    for (auto &e : ev_) HIP_TRY(hipEventCreate(&e), ABPOA_HIP_ENODEV);
    device_ = device; open_ = true; return 0;
}
void BatchStream::close() {
    if (!open_) return;
    (void)hipSetDevice(device_);
    (void)hipStreamSynchronize(stream_);
    in_.release(); out_.release(); planes_.release();
    for (auto &e : ev_) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(stream_);
    open_ = false;
}

int BatchStream::prepare(const abpoa_hip_scoring_t *sc, int n, const BatchShape *sh, unsigned flags) {
    if (!open_) { set_err("stream not open"); return ABPOA_HIP_ENODEV; }
    HIP_TRY(hipSetDevice(device_), ABPOA_HIP_ENODEV);
    sc_ = *sc; mat_.assign(sc->mat, sc->mat + sc->m * sc->m); sc_.mat = mat_.data();
    flags_ = flags; n_ = n;
    P_ = sc->gap_mode == ABPOA_HIP_LINEAR_GAP ? 1 : (sc->gap_mode == ABPOA_HIP_AFFINE_GAP ? 3 : 5);
    desc_.resize(n); recs_.resize(n); cells_.resize(n); trace_arena_.clear();
    tot_ = describe_batch(sc, n, sh, desc_.data(), cells_.data());
    I_ = layout_in(n, sc->m, tot_); O_ = layout_out(n, tot_);
    int rc;
    if ((rc = in_.reserve(I_.bytes)) || (rc = out_.reserve(O_.bytes))) return rc;
    memcpy(in_.host + I_.mat, sc->mat, sizeof(int32_t) * sc->m * sc->m);
    memset(in_.host + I_.act, 1, tot_.rows);
    return 0;
}

// stages of run(), host arithmetic in batch_plan.cpp: mark_fast_ok, fill_dir_tables, then per pass plan_pass -> assign_arenas -> bind_pools -> upload_pass ->
// launch -> download -> collect_pass.  Events: [0, 1] the uploads, [1, 2] the kernels ([4, 2] the tail kernel of a pure fast-path pass), [2, 3] the download
int BatchStream::run() {
    HIP_TRY(hipSetDevice(device_), ABPOA_HIP_ENODEV);
    const abpoa_hip_scoring_t *sc = &sc_;
    uint8_t *hi = in_.host, *ho = out_.host;
    mark_fast_ok(sc, flags_ & BS_FRESH_BAND, n_, desc_.data(), hi + I_.act, (const int32_t *)(ho + O_.left), (const int32_t *)(ho + O_.right));
    Pass ps; ps.dir = dir_words_for_run(sc, flags_);
    if (ps.dir) for (AlnDesc &d : desc_) {
        if (!(d.flags & ALN_FAST_OK)) continue;
        if (!fill_dir_tables(d.n_rows, (const int32_t *)(hi + I_.poff) + d.poff0, (const int32_t *)(hi + I_.pred) + d.pred0, hi + I_.sdist + d.row0,
                             (uint32_t *)(hi + I_.pd) + 2 * d.row0)) d.flags = 0;
    }
    ps.todo.resize(n_); for (int i = 0; i < n_; ++i) ps.todo[i] = i;
    std::vector<int32_t> saved_lr;              // caller's band state, needed again if an alignment is retried
    int rc;
    while (!ps.todo.empty()) {
        ps.descs.resize(ps.todo.size());
        plan_pass(sc, flags_, ps.dir, desc_.data(), ps.todo, ps.b);
        const int64_t plane_bytes = assign_arenas(ps.b, ps.first, cells_.data(), ps.todo, desc_.data(), ps.descs.data(), &ps.n_fast);
        if ((rc = planes_.reserve((size_t)plane_bytes))) return rc;
        memcpy(hi + I_.desc, ps.descs.data(), sizeof(AlnDesc) * ps.descs.size());
        bind_pools(ps.b, I_, O_, in_.dev, out_.dev, planes_.dev);
        HIP_TRY(hipEventRecord(ev_[0], stream_), ABPOA_HIP_ELAUNCH);
        if ((rc = upload_pass(ps, saved_lr))) return rc;
        HIP_TRY(hipEventRecord(ev_[1], stream_), ABPOA_HIP_ELAUNCH);
        HIP_TRY(launch_dp(ps.b, ps.n_fast, stream_, ev_[4]), ABPOA_HIP_ELAUNCH);
        HIP_TRY(hipEventRecord(ev_[2], stream_), ABPOA_HIP_ELAUNCH);
        HIP_TRY(hipMemcpyAsync(ho, out_.dev, O_.download_bytes(sc->wb >= 0, flags_), hipMemcpyDeviceToHost, stream_), ABPOA_HIP_ELAUNCH);
        HIP_TRY(hipEventRecord(ev_[3], stream_), ABPOA_HIP_ELAUNCH);
        HIP_TRY(hipStreamSynchronize(stream_), ABPOA_HIP_ELAUNCH);
        if ((rc = collect_pass(ps))) return rc;
    }
    return ABPOA_HIP_OK;
}

// inputs (a retry pass: only up to the matrix, i.e. the descriptors), the caller's band state where it is kept, "row never computed" in dp_beg_sn / dp_end_sn
int BatchStream::upload_pass(const Pass &ps, std::vector<int32_t> &saved_lr) {
    uint8_t *hi = in_.host, *ho = out_.host, *di = in_.dev, *dout = out_.dev;
    const bool banded = sc_.wb >= 0, fresh = flags_ & BS_FRESH_BAND, first_pass = ps.first;
    const size_t lr_words = (O_.right - O_.left) / 4 + tot_.rows;
    HIP_TRY(hipMemcpyAsync(di, hi, first_pass ? I_.bytes : I_.mat, hipMemcpyHostToDevice, stream_), ABPOA_HIP_ELAUNCH);
    if (banded && !fresh) {
        if (first_pass) {
            saved_lr.assign((const int32_t *)(ho + O_.left), (const int32_t *)(ho + O_.left) + lr_words);
            HIP_TRY(hipMemcpyAsync(dout + O_.left, ho + O_.left, lr_words * 4, hipMemcpyHostToDevice, stream_), ABPOA_HIP_ELAUNCH);
        } else for (int i : ps.todo) {      // only the retried alignments restart from the caller's band state
            const AlnDesc &d = desc_[i]; const size_t ro = (O_.right - O_.left) / 4;
            HIP_TRY(hipMemcpyAsync(dout + O_.left + 4 * d.row0, saved_lr.data() + d.row0, 4 * (size_t)d.n_rows, hipMemcpyHostToDevice, stream_), ABPOA_HIP_ELAUNCH);
            HIP_TRY(hipMemcpyAsync(dout + O_.right + 4 * d.row0, saved_lr.data() + ro + d.row0, 4 * (size_t)d.n_rows, hipMemcpyHostToDevice, stream_), ABPOA_HIP_ELAUNCH);
        }
    }
    // -1 = "row never computed" (inactive rows, rows behind a z-drop break)
    if (first_pass) HIP_TRY(hipMemsetAsync(dout + O_.bsn, 0xFF, (O_.esn - O_.bsn) + 4 * tot_.rows, stream_), ABPOA_HIP_ELAUNCH);
    else for (int i : ps.todo) {
        const AlnDesc &d = desc_[i];
        HIP_TRY(hipMemsetAsync(dout + O_.bsn + 4 * d.row0, 0xFF, 4 * (size_t)d.n_rows, stream_), ABPOA_HIP_ELAUNCH);
        HIP_TRY(hipMemsetAsync(dout + O_.esn + 4 * d.row0, 0xFF, 4 * (size_t)d.n_rows, stream_), ABPOA_HIP_ELAUNCH);
    }
    return 0;
}

// clocks and stats of the pass; then its records: which alignments run again (NEED_SCORES: the whole retry without words; OVERFLOW: at full width), the
// others' results, and in trace mode their arenas
int BatchStream::collect_pass(Pass &ps) {
    const bool trace = flags_ & BS_TRACE; const int P = P_;
    float ms_h2d = 0, ms_k = 0, ms_d2h = 0;
    (void)hipEventElapsedTime(&ms_h2d, ev_[0], ev_[1]); (void)hipEventElapsedTime(&ms_k, ev_[1], ev_[2]); (void)hipEventElapsedTime(&ms_d2h, ev_[2], ev_[3]);
    float ms_tail = 0;                    // pure fast-path batches: ev_[4] sits between the row-loop kernel and the tail kernel
    if (ps.n_fast == ps.b.n) { (void)hipEventElapsedTime(&ms_tail, ev_[4], ev_[2]); ms_k -= ms_tail; }
    stats_.n_launches += 1; stats_.kernel_ms += ms_k; stats_.tail_ms += ms_tail; stats_.h2d_ms += ms_h2d; stats_.d2h_ms += ms_d2h;

    // records are indexed by position in this pass; cigar / per-row slots by alignment, so a retry pass cannot
    // clobber the results of alignments that finished earlier
    const AlnOut *got = (const AlnOut *)(out_.host + O_.rec);
    std::vector<int> again; bool need_scores = false;
    for (size_t t = 0; t < ps.todo.size(); ++t) {
        const int i = ps.todo[t]; const AlnOut &r = got[t]; const AlnDesc &d = desc_[i];
        if (r.status == ABPOA_HIP_STATUS_NEED_SCORES && ps.dir) { need_scores = true; again.push_back(i); stats_.n_need_scores += 1; __atomic_fetch_add(&g_dir_counts[1], 1, __ATOMIC_RELAXED);
                continue; }
        if (r.status == ABPOA_HIP_STATUS_OVERFLOW) {
            if (!ps.first) { set_err("problem %d: arena overflow at full width (internal error)", i); return ABPOA_HIP_ELAUNCH; }
            again.push_back(i); continue;
        }
        recs_[i] = r;
        if (r.pad < 0) __atomic_fetch_add(&g_dir_counts[0], 1, __ATOMIC_RELAXED);
        // trace mode: the arena of a finished alignment is kept on the host now -- a retry pass of OTHER alignments re-uses the device arenas
        if (trace) {
            trace_arena_.resize(desc_.size());
            trace_arena_[i].resize((size_t)r.cells_used * (d.bits / 8));
            if (!trace_arena_[i].empty()) HIP_TRY(hipMemcpy(trace_arena_[i].data(), planes_.dev + d.plane_off, trace_arena_[i].size(), hipMemcpyDeviceToHost), ABPOA_HIP_ELAUNCH);
        }
        stats_.n_alignments += 1; stats_.n_cells += r.n_cells;
        stats_.algo_bytes += r.n_cells * (d.bits / 8) * (P == 1 ? 2 : (P == 3 ? 5 : 8));
        g_dbg[CLK_DP] += r.clk_dp; g_dbg[CLK_BT] += r.clk_bt; g_dbg[CLK_ROWS_DONE] += r.n_rows_done; g_dbg[CLK_BT_STEPS] += r.n_bt_steps;
        for (int q_ = 0; q_ < DIAG_SLOTS; ++q_) g_dbg[CLK_SEG0 + q_] += r.seg[q_];
    }
    ps.todo.swap(again); ps.first = false;
    if (need_scores) ps.dir = false;                 // the retry pass runs with score records (full width: simplest, and rare)
    return 0;
}

int BatchStream::fetch_trace(int i, abpoa_hip_trace_t *T) {
    if ((size_t)i >= trace_arena_.size()) { set_err("no trace kept for problem %d", i); return ABPOA_HIP_EINVAL; }
    const AlnDesc &d = desc_[i]; const uint8_t *ho = out_.host;
    // (the arena was saved when the alignment finished: collect_pass)
    unpack_trace(d, P_, sc_.wb >= 0, recs_[i].pad, (const int32_t *)(ho + O_.bsn) + d.row0, (const int32_t *)(ho + O_.esn) + d.row0,
                 (const int64_t *)(ho + O_.coff) + d.row0, (const int32_t *)(ho + O_.rmi) + d.row0, trace_arena_[i].data(), T);
    return 0;
}

}  // namespace abpoa_hip

using namespace abpoa_hip;

extern "C" {
int abpoa_hip_set_option(const char *name, const char *value) { return abpoa_hip::set_option(name, value) == 0 ? ABPOA_HIP_OK : ABPOA_HIP_EINVAL; }
int abpoa_hip_list_options(const char **names, const char **help, int cap) { return abpoa_hip::list_options(names, help, cap); }

int abpoa_hip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int abpoa_hip_init(int device) {
    abpoa_hip::refresh_options();
    std::lock_guard<std::mutex> lk(g.mu);
    if (g.ready && g.device == device) return ABPOA_HIP_OK;
    if (g.ready) { set_err("engine already bound to device %d", g.device); return ABPOA_HIP_EINVAL; }
    // the read-set driver runs one stream per group; give the runtime enough hardware queues for them to overlap
    setenv("GPU_MAX_HW_QUEUES", "16", 0);
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { set_err("no HIP device available (the DP has no CPU fallback)"); return ABPOA_HIP_ENODEV; }
    if (device < 0 || device >= n) { set_err("device %d out of range (0..%d)", device, n - 1); return ABPOA_HIP_ENODEV; }
    int rc = g.flat.open(device);
    if (rc) return rc;
    g.device = device; g.ready = true; memset(&g.stats, 0, sizeof(g.stats));
    return ABPOA_HIP_OK;
}

void abpoa_hip_shutdown(void) {
    std::lock_guard<std::mutex> lk(g.mu);
    if (!g.ready) return;
    g.flat.close();
    g.ready = false; g.device = -1;
}

const char *abpoa_hip_last_error(void) { std::lock_guard<std::mutex> lk(g_err_mu); memcpy(g_err_copy, g_err, sizeof(g_err)); return g_err_copy; }
void abpoa_hip_get_stats(abpoa_hip_stats_t *out) { std::lock_guard<std::mutex> lk(g.stats_mu); *out = g.stats; }
void abpoa_hip__dir_counts(long long *out) { out[0] = __atomic_exchange_n(&g_dir_counts[0], 0, __ATOMIC_RELAXED); out[1] = __atomic_exchange_n(&g_dir_counts[1], 0, __ATOMIC_RELAXED); }
// (test hook, host only: the LDS carve-up of the wide row loop for a launch of n_aln alignments -- out: wide_on, ring rows, LDS bytes per workgroup,
//  workgroups per CU by the 1280-byte allocation granule of gfx950, the wide kernels' phase offset, the band half-widths [lo, hi] that take it)
void abpoa_hip__wide_plan(const abpoa_hip_scoring_t *sc, int max_qlen, int max_bits, int n_aln, int *out) {
    abpoa_hip::LdsPlan L; abpoa_hip::hook_lds_plan(sc, max_qlen, max_bits, n_aln, &L);
    out[0] = L.wide_on; out[1] = L.wfr_rows; out[2] = L.total_wide; out[3] = L.total_wide > 0 ? abpoa_hip::wide_workgroups_per_cu(L.total_wide) : 0;
    out[4] = L.w_phase_off; out[5] = L.wide_w_lo; out[6] = L.wide_w_hi;
}
// (test hook, host only: the same plan's narrow row loop -- out: score-ring rows, score-ring columns (0: no fast loop), arena window of the tail kernel in bytes)
void abpoa_hip__narrow_plan(const abpoa_hip_scoring_t *sc, int max_qlen, int max_bits, int n_aln, int *out) {
    abpoa_hip::LdsPlan L; abpoa_hip::hook_lds_plan(sc, max_qlen, max_bits, n_aln, &L);
    out[0] = L.fr_rows; out[1] = L.fr_cols; out[2] = L.bt_bytes_tail;
}
// (test hook, host only, read-only for the engine: row-kernel launches since the last call -- narrow loop, 448-column wide loop, 704-column wide loop)
void abpoa_hip__row_launches(long long *out) { for (int i = 0; i < 3; ++i) out[i] = __atomic_exchange_n(&abpoa_hip::g_row_launches[i], 0, __ATOMIC_RELAXED); }
void abpoa_hip__debug_clocks(long long *out) { for (int i = 0; i < CLK_SLOTS; ++i) { out[i] = g_dbg[i]; g_dbg[i] = 0; } }
void abpoa_hip_reset_stats(void) { std::lock_guard<std::mutex> lk(g.stats_mu); memset(&g.stats, 0, sizeof(g.stats)); }

void abpoa_hip_free_result(abpoa_hip_result_t *r) {
    if (!r) return;
    free(r->cigar);
    if (r->trace) {
        abpoa_hip_trace_t *t = r->trace;
        free(t->dp_beg); free(t->dp_end); free(t->dp_beg_sn); free(t->dp_end_sn); free(t->row_off); free(t->planes); free(t->row_max_i); free(t);
    }
    memset(r, 0, sizeof(*r));
}

static int validate(const abpoa_hip_scoring_t *sc, const abpoa_hip_problem_t *p, int idx) {
    if (p->n_rows < 3 || p->qlen < 0) { set_err("problem %d: n_rows=%d qlen=%d", idx, p->n_rows, p->qlen); return ABPOA_HIP_EINVAL; }
    if (!p->row_base || !p->row_node_id || !p->pred_off || !p->pred_row || !p->out_off || !p->out_row || (p->qlen > 0 && !p->query)) {
        set_err("problem %d: NULL array", idx); return ABPOA_HIP_EINVAL; }
    if ((sc->wb >= 0 || sc->zdrop > 0) && !p->row_remain) { set_err("problem %d: row_remain required", idx); return ABPOA_HIP_EINVAL; }
    if (sc->wb >= 0 && (!p->max_pos_left || !p->max_pos_right)) { set_err("problem %d: max_pos_left/right required when banded", idx); return ABPOA_HIP_EINVAL; }
    const int gn = p->n_rows;
    if (p->pred_off[0] != 0 || p->out_off[0] != 0) { set_err("problem %d: CSR offsets must start at 0", idx); return ABPOA_HIP_EINVAL; }
    for (int r = 0; r < gn; ++r) {
        if (p->pred_off[r + 1] < p->pred_off[r] || p->out_off[r + 1] < p->out_off[r]) { set_err("problem %d: CSR offsets not monotone at row %d", idx, r); return ABPOA_HIP_EINVAL; }
        if (p->row_base[r] >= sc->m) { set_err("problem %d: base code %d >= m at row %d", idx, p->row_base[r], r); return ABPOA_HIP_EINVAL; }
        const bool act = !p->row_active || p->row_active[r];
        for (int k = p->pred_off[r]; k < p->pred_off[r + 1]; ++k) {
            int q = p->pred_row[k];
            if (q < 0 || q >= r || (p->row_active && !p->row_active[q])) { set_err("problem %d: row %d has predecessor %d (must be an active earlier row)", idx, r, q); return ABPOA_HIP_EINVAL; }
        }
        if (act && r > 0 && r < gn - 1 && p->pred_off[r + 1] == p->pred_off[r]) { set_err("problem %d: active row %d has no predecessor", idx, r); return ABPOA_HIP_EINVAL; }
        for (int k = p->out_off[r]; k < p->out_off[r + 1]; ++k) {
            int o = p->out_row[k];
            if (o != -1 && (o <= r || o >= gn)) { set_err("problem %d: row %d has successor %d", idx, r, o); return ABPOA_HIP_EINVAL; }
        }
    }
    for (int j = 0; j < p->qlen; ++j) if (p->query[j] >= sc->m) { set_err("problem %d: query code %d >= m", idx, p->query[j]); return ABPOA_HIP_EINVAL; }
    return 0;
}

int abpoa_hip_align_batch(const abpoa_hip_scoring_t *sc, int n, const abpoa_hip_problem_t *pb,
                          abpoa_hip_result_t *res, unsigned flags) {
    abpoa_hip::refresh_options();
    if (n < 0 || !sc || (n > 0 && (!pb || !res))) { set_err("bad arguments"); return ABPOA_HIP_EINVAL; }
    if (n == 0) return ABPOA_HIP_OK;
    for (int i = 0; i < n; ++i) memset(&res[i], 0, sizeof(res[i]));
    if (!g.ready) { int rc = abpoa_hip_init(0); if (rc) return rc; }
    if (sc->m <= 0 || !sc->mat || sc->gap_mode < 0 || sc->gap_mode > 2 || sc->align_mode < 0 || sc->align_mode > 2) { set_err("bad scoring"); return ABPOA_HIP_EINVAL; }
    for (int i = 0; i < n; ++i) { int rc = validate(sc, &pb[i], i); if (rc) return rc; }
    std::lock_guard<std::mutex> lk(g.mu);
    const bool banded = sc->wb >= 0, trace = flags & ABPOA_HIP_FLAG_TRACE;
    std::vector<BatchShape> sh(n);
    for (int i = 0; i < n; ++i) sh[i] = BatchShape{pb[i].n_rows, pb[i].qlen, pb[i].pred_off[pb[i].n_rows], pb[i].out_off[pb[i].n_rows]};
    BatchStream &S = g.flat;
    int rc = S.prepare(sc, n, sh.data(), (trace ? BS_TRACE : 0) | BS_WANT_BAND_STATE);
    if (rc) return rc;
    for (int i = 0; i < n; ++i) {
        const abpoa_hip_problem_t &p = pb[i]; const int gn = p.n_rows; ProblemSlots s = S.slots(i);
        if (p.qlen) memcpy(s.query, p.query, p.qlen);
        memcpy(s.row_base, p.row_base, gn); memcpy(s.row_node_id, p.row_node_id, 4 * gn);
        if (p.row_remain) memcpy(s.row_remain, p.row_remain, 4 * gn); else memset(s.row_remain, 0, 4 * gn);
        if (p.row_active) memcpy(s.row_active, p.row_active, gn);
        memcpy(s.pred_off, p.pred_off, 4 * (gn + 1)); memcpy(s.pred_row, p.pred_row, 4 * (size_t)p.pred_off[gn]);
        memcpy(s.out_off, p.out_off, 4 * (gn + 1)); memcpy(s.out_row, p.out_row, 4 * (size_t)p.out_off[gn]);
        if (banded) { memcpy(s.left, p.max_pos_left, 4 * gn); memcpy(s.right, p.max_pos_right, 4 * gn); }
    }
    rc = S.run();
    if (rc) return rc;
    for (int i = 0; i < n; ++i) {
        const AlnOut &r = S.rec(i); abpoa_hip_result_t &R = res[i]; const abpoa_hip_problem_t &p = pb[i];
        R.status = r.status; R.bits = S.desc(i).bits; R.best_score = r.best_score; R.best_row = r.best_row; R.best_col = r.best_col;
        R.node_s = r.node_s; R.node_e = r.node_e; R.query_s = r.query_s; R.query_e = r.query_e;
        R.n_aln_bases = r.n_aln_bases; R.n_matched_bases = r.n_matched_bases; R.n_cells = r.n_cells;
        R.n_cigar = r.status == 0 ? r.n_cigar : 0;
        if (R.n_cigar > 0) {
            R.cigar = (uint64_t *)malloc(sizeof(uint64_t) * R.n_cigar);
            if (!R.cigar) { set_err("malloc failed"); return ABPOA_HIP_ENOMEM; }
            memcpy(R.cigar, S.cigar(i), sizeof(uint64_t) * R.n_cigar);
        }
        if (banded) { memcpy(p.max_pos_left, S.left(i), 4 * p.n_rows); memcpy(p.max_pos_right, S.right(i), 4 * p.n_rows); }
        if (trace) {
            R.trace = (abpoa_hip_trace_t *)calloc(1, sizeof(abpoa_hip_trace_t));
            if ((rc = S.fetch_trace(i, R.trace))) return rc;
        }
    }
    add_global_stats(S.take_stats());
    return ABPOA_HIP_OK;
}

}  // extern "C"
