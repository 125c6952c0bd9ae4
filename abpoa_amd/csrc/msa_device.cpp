// Host side of the device-resident read-set driver (poa_device.h): pool allocation, one upload of the reads, the per-round
// kernel sequence (prepare -> DP rows -> backtrack -> fuse) queued back to back with NO host work or synchronisation in
// between, consensus / MSA kernels, one download of the results.  Sets that exceed a device capacity (nodes, edge slots of an
// inner node, arena) are reported back: redone in a pass with more node slots or by the host driver (msa_batch.cpp).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <limits.h>
#include <mutex>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <thread>
#include <vector>
#include <hip/hip_runtime.h>
#include "engine_options.h"
#include "batch_stream.h"
#include "msa_device.h"
#include "poa_device.h"
#include "poa_graph.h"
#include "dir_plane.h"
#include "msa_batch.h"
#include "msa_device_debug.h"
#include "msa_device_layout.h"
#include "msa_device_plan.h"
#include "routing.h"

namespace abpoa_hip {

namespace {
#define HIP_OK(expr, code) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { \
        set_err("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); return code; } } while (0)

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// [0, n) split into contiguous ranges, one per worker (the calling thread takes the last range)
template <typename F>
void parallel_ranges(int n_threads, int n, F fn) {
    const int T = std::max(1, std::min(n_threads, n / 64));
    if (T <= 1) { fn(0, n); return; }
    std::vector<std::thread> th; th.reserve(T - 1);
    for (int t = 0; t < T - 1; ++t) th.emplace_back(fn, (int)((int64_t)n * t / T), (int)((int64_t)n * (t + 1) / T));
    fn((int)((int64_t)n * (T - 1) / T), n);
    for (auto &x : th) x.join();
}

// ABPOA_HIP_DEVICE_AUDIT=1 (multi-GPU runs: SURVEY.md section 8e): every pool allocation of a device queue is looked up with hipPointerGetAttributes and must
//  sit
// on the device the queue serves -- and the calling thread's current device must be that one -- or the call fails with ABPOA_HIP_ENODEV; ABPOA_HIP_VERBOSE=1
// prints where each allocation landed.  (The HIP device is per host thread; a queue thread that forgot hipSetDevice would put its pools on device 0.)
thread_local int t_queue_device = -1;
int audit_allocation(const void *ptr, size_t bytes, const char *what) {
    static const bool on = opt_on("ABPOA_HIP_DEVICE_AUDIT");
    if (!on || t_queue_device < 0) return 0;
    int cur = -1; (void)hipGetDevice(&cur);
    hipPointerAttribute_t at; memset(&at, 0, sizeof(at));
    const hipError_t e = hipPointerGetAttributes(&at, ptr);
    if (opt_set("ABPOA_HIP_VERBOSE")) fprintf(stderr, "[abpoa-hip] audit: %s, %zu bytes: device %d (queue device %d, thread's current device %d)\n", what,
            bytes, e == hipSuccess ? at.device : -1, t_queue_device, cur);
    if (e != hipSuccess || cur != t_queue_device || (at.type == hipMemoryTypeDevice && at.device != t_queue_device)) {
        set_err("device audit: %s of %zu bytes on device %d, queue serves device %d, thread's current device %d", what, bytes,
                e == hipSuccess ? at.device : -1, t_queue_device, cur);
        return ABPOA_HIP_ENODEV;
    }
    return 0;
}

struct Arena {                 // grow-only device / pinned-host buffers kept across calls (one job at a time, see g_mu)
    uint8_t *dev = nullptr, *host = nullptr; size_t dev_cap = 0, host_cap = 0;
    int need_dev(size_t n) {
        if (n <= dev_cap) return 0;
        if (dev) (void)hipFree(dev);
        dev = nullptr; dev_cap = 0;
        HIP_OK(hipMalloc((void **)&dev, n), ABPOA_HIP_ENOMEM); dev_cap = n; return audit_allocation(dev, n, "device pool");
    }
    int need_host(size_t n) {
        if (n <= host_cap) return 0;
        if (host) (void)hipHostFree(host);
        host = nullptr; host_cap = 0;
        HIP_OK(hipHostMalloc((void **)&host, n, hipHostMallocDefault), ABPOA_HIP_ENOMEM); host_cap = n;
        return audit_allocation(host, n, "pinned staging buffer");
    }
};
struct Cache { Arena in, graph, rows, planes, out, msa, gfa; hipStream_t stream = nullptr, copy_stream = nullptr; hipEvent_t ev_copy = nullptr;
        std::vector<hipEvent_t> ev; int device = -1;
        // frees every pool (the caller has made `device` the current one)
        void release() { for (Arena *a : {&in, &graph, &rows, &planes, &out, &msa, &gfa}) { if (a->dev) (void)hipFree(a->dev); if (a->host) (void)hipHostFree(a->host);
                *a = Arena(); } } };
Cache g_cache[MSA_DEVICE_SLOTS]; std::mutex g_cache_mu[MSA_DEVICE_SLOTS];      // one per worker of the multi-device batch call

// What the stages of one job share (run_msa_device_body runs them in order)
struct Job {
    DevicePlan pl; const abpoa_hip_readset_t *sets; int n_sets, n_threads, device, slot;
    Cache *C; Layout L; EventSlots ev;
    bool any_w, rest_up; int64_t split_at;      // per-base weights given; the reads of the later rounds are on their way; where they start in the read pool
    PoaDev p; DevBatch b, b_rc, b_r;      // kernel arguments of the graph kernels and of the row loops (b_rc: the -s retry, b_r: the all-rounds kernel)
    bool dbg_sync, use_rounds; size_t rounds_lds;
    MsaLayout M;
    GfaDev g; GfaLayout G;      // GFA output: kernel arguments; where each set's record lies in the result pools of Cache.gfa
    double t_begin, t_queue, t_done;
    const PoaState *host_state() const { return (const PoaState *)(C->graph.host + L.o_state); }      // (downloaded by queue_job)
};

}  // namespace

void release_msa_device_caches() {
    int cur = -1; (void)hipGetDevice(&cur);
    for (int s = 0; s < MSA_DEVICE_SLOTS; ++s) {
        std::lock_guard<std::mutex> lk(g_cache_mu[s]);
        Cache &C = g_cache[s];
        if (C.device < 0) continue;
        (void)hipSetDevice(C.device);
        if (C.stream) (void)hipStreamSynchronize(C.stream);
        C.release();
    }
    if (cur >= 0) (void)hipSetDevice(cur);
}

int msa_device_resident_sets(const abpoa_hip_scoring_t *sc, int n_sets, const abpoa_hip_readset_t *sets) {
    const int per_cu = wide_sets_per_cu(sc, n_sets, sets);
    return per_cu > 0 ? per_cu * device_cu_count(-1) : 0;
}

namespace {
// ---- stage 1: the cache slot on this device (a slot that served another device gives its pools and stream back there first)
int acquire_cache_slot(Cache &C, int device) {
    HIP_OK(hipSetDevice(device), ABPOA_HIP_ENODEV);          // (the HIP device is per host thread)
    t_queue_device = device;
    if (C.device != device) {
        if (C.device >= 0) {      // the slot served another device before: its pools and stream live there
            (void)hipSetDevice(C.device);
            C.release();
            if (C.stream) (void)hipStreamDestroy(C.stream); if (C.copy_stream) (void)hipStreamDestroy(C.copy_stream);
            if (C.ev_copy) (void)hipEventDestroy(C.ev_copy);
            for (hipEvent_t e : C.ev) (void)hipEventDestroy(e);
            C = Cache();
            HIP_OK(hipSetDevice(device), ABPOA_HIP_ENODEV);
        }
        if (!C.stream) HIP_OK(hipStreamCreateWithFlags(&C.stream, hipStreamNonBlocking), ABPOA_HIP_ENODEV);
        C.device = device;
    }
    return 0;
}

// ---- stage 2, byte offsets of every pool inside the three device blobs: lay_out_device (msa_device_layout.h)
// ---- stage 3: the whole job must fit (the caller splits very large jobs): checked on the computed layout, before any cached buffer is given up; then the
//      pools grow to it
int fit_device(Job &J) {
    DevicePlan &pl = J.pl; Cache &C = *J.C; const Layout &L = J.L;
    size_t free_b = 0, total_b = 0; (void)hipMemGetInfo(&free_b, &total_b);
    const size_t want[4] = {L.in_dev_bytes, L.graph_bytes, L.rows_bytes, (size_t)pl.plane_tot}, have[4] = {C.in.dev_cap, C.graph.dev_cap, C.rows.dev_cap,
            C.planes.dev_cap};
    size_t need = 0, given_back = 0;
    for (int i = 0; i < 4; ++i) if (want[i] > have[i]) { need += want[i]; given_back += have[i]; }      // a buffer that must grow is freed first
    // the record arenas of the wide-band sets do not fit: direction words for them too
    if (need > free_b + given_back && pl.dir_wide_auto && pl.any_wide_set && !pl.dir_wide) {
        pl.dir_wide = true; pl.size_arenas(J.sets, true);
        need = 0; given_back = 0;
        const size_t want2[4] = {L.in_dev_bytes, L.graph_bytes, L.rows_bytes, (size_t)pl.plane_tot};
        for (int i = 0; i < 4; ++i) if (want2[i] > have[i]) { need += want2[i]; given_back += have[i]; }
        if (opt_set("ABPOA_HIP_VERBOSE")) fprintf(stderr,
                "[abpoa-hip] device %d: %d sets: score-record arenas do not fit, direction words for the wide-band sets " "too (arenas %.1f GB)\n", J.device,
                J.n_sets, pl.plane_tot / 1e9);
    }
    if (need > free_b + given_back) {
        if (opt_set("ABPOA_HIP_VERBOSE")) fprintf(stderr,
                "[abpoa-hip] device %d: %d sets need %.1f GB in growing buffers (arenas %.1f GB), %.1f GB free + %.1f " "GB given back: splitting\n",
                J.device, J.n_sets, need / 1e9, pl.plane_tot / 1e9, free_b / 1e9, given_back / 1e9);
        set_err("device-resident job needs %zu more bytes, %zu free", need, free_b + given_back); return ABPOA_HIP_ENOMEM;
    }
    int rc;
    if ((rc = C.in.need_dev(L.in_dev_bytes)) || (rc = C.in.need_host(L.in_bytes)) || (rc = C.graph.need_dev(L.graph_bytes)) || (rc =
            C.graph.need_host(L.dl_bytes)) ||
        (rc = C.rows.need_dev(L.rows_bytes)) || (rc = C.planes.need_dev((size_t)pl.plane_tot))) return rc;
    while ((int)C.ev.size() < J.ev.count()) { hipEvent_t e; HIP_OK(hipEventCreate(&e), ABPOA_HIP_ENODEV); C.ev.push_back(e); }
    return 0;
}

void stage_reads(const Job &J, int k_lo, int k_hi) {
    const DevicePlan &pl = J.pl; uint8_t *hi = J.C->in.host; const int64_t *roff = (const int64_t *)(hi + J.L.o_roff); uint8_t *rd = hi + J.L.o_reads;
    parallel_ranges(std::min(J.n_threads, 16), J.n_sets, [&](int lo, int hi_) {
        for (int s = lo; s < hi_; ++s) { const int64_t r0 = pl.ps[s].read0; const int ke = std::min(k_hi, J.sets[s].n_reads);
                for (int r = k_lo; r < ke; ++r) memcpy(rd + roff[r0 + r], J.sets[s].seqs[r], J.sets[s].lens[r]); }
    });
}

// ---- stage 4: set table, reads (already residue codes), score matrix into the pinned buffer; the first part goes up
int upload_reads(Job &J) {
    const DevicePlan &pl = J.pl; Cache &C = *J.C; const Layout &L = J.L; const abpoa_hip_scoring_t *sc = &pl.sc;
    uint8_t *hi = C.in.host;
    memcpy(hi + L.o_sets, pl.ps.data(), sizeof(PoaSet) * J.n_sets);
    // Reads are laid out round by round (read k of every set, then read k + 1 ...): the first two rounds go up at once, the rest is staged
    // and copied while the GPU already works on round 1 (config 2: 50 MB of residue codes, ~1 ms of staging + ~1 ms of PCIe)
    int64_t *roff = (int64_t *)(hi + L.o_roff); int32_t *rlen = (int32_t *)(hi + L.o_rlen); uint8_t *rd = hi + L.o_reads;
    J.split_at = fill_read_tables(pl, J.n_sets, J.sets, roff, rlen);
    stage_reads(J, 0, 2);
    if (J.any_w) {      // weights of every read, same offsets as the bases; a read (or a set) without weights counts 1 per base
        int32_t *wd = (int32_t *)(hi + L.o_wts);
        parallel_ranges(std::min(J.n_threads, 16), J.n_sets, [&](int lo, int hi_) {
            for (int s = lo; s < hi_; ++s) for (int r = 0; r < J.sets[s].n_reads; ++r) {
                int32_t *dst = wd + roff[pl.ps[s].read0 + r]; const int32_t *src = J.sets[s].weights ? J.sets[s].weights[r] : nullptr;
                if (src) memcpy(dst, src, 4 * (size_t)J.sets[s].lens[r]); else for (int j = 0; j < J.sets[s].lens[r]; ++j) dst[j] = 1;
            }
        });
    }
    memcpy(hi + L.o_mat, sc->mat, 4 * sc->m * sc->m);
    hipStream_t st = C.stream;
    if (!C.copy_stream) { HIP_OK(hipStreamCreateWithFlags(&C.copy_stream, hipStreamNonBlocking), ABPOA_HIP_ENODEV);
            HIP_OK(hipEventCreateWithFlags(&C.ev_copy, hipEventDisableTiming), ABPOA_HIP_ENODEV); }
    HIP_OK(hipMemcpyAsync(C.in.dev, hi, L.o_reads + (size_t)J.split_at, hipMemcpyHostToDevice, st), ABPOA_HIP_ELAUNCH);
    J.rest_up = J.split_at >= roff[pl.tot_reads];      // nothing left for the second part
    return 0;
}

// ---- stage 5, arguments of the graph kernels: bind_poa_dev (msa_device_layout.h)
// ---- stage 6: arguments of the row-loop kernels (b_rc: the -s retry in the general kernel)
int fill_dev_batch(Job &J, bool *want_general) {
    const DevicePlan &pl = J.pl; Cache &C = *J.C; DevBatch &b = J.b; int rc;
    memset(&b, 0, sizeof(b));
    b.n = J.n_sets; b.m = pl.sc.m;
    if ((rc = final_lds_plan(pl, J.n_sets, J.sets, b))) { set_err("local alignment outside the device row loop's range"); return rc; }
    // caller falls back to the host driver
    if (!pl.local && !pl.general && !fast_loop_fits(b.lds, pl.max_qlen)) { *want_general = true; set_err("band too wide for the fast row loop"); return ABPOA_HIP_EINVAL; }
    bind_dev_batch(b, J.b_rc, pl, J.L, J.p, C.in.dev, C.rows.dev, C.planes.dev);
    return 0;
}

// ---- stage 7: all-rounds kernel (poa_rounds.hip) for jobs whose reads all take the narrow row loop: round 1 runs as separate launches (the upload of the
//      later reads hides behind it), rounds 2 .. n in ONE launch in which every read-set advances on its own.  ABPOA_HIP_LOCKSTEP=1: one launch
//      per phase and round throughout (what the wide-band jobs use, and the per-round diagnostics below).
void plan_rounds(Job &J) {
    const DevicePlan &pl = J.pl; const abpoa_hip_scoring_t *sc = &pl.sc; const PoaDev &p = J.p; const DevBatch &b = J.b; DevBatch &b_r = J.b_r;
    bool &dbg_sync = J.dbg_sync, &use_rounds = J.use_rounds; size_t &rounds_lds = J.rounds_lds;
    dbg_sync = opt_on("ABPOA_HIP_DEVSYNC");
    use_rounds = !pl.local && pl.rounds_possible && !dbg_sync && b.lds.wide_on == 0 && !(b.dbg & DBG_NO_FAST_LOOPS) && pl.max_reads > 2 && !opt_on("ABPOA_HIP_LOCKSTEP");
    b_r = b; rounds_lds = 0;
    if (use_rounds) {
        // (prepare: 5 bytes per row; fuse: static LDS only)
        auto dyn_of = [&](const DevBatch &x) { return std::max<size_t>(std::max<size_t>((size_t)x.lds.total_rows, (size_t)x.lds.total_tail),
                (size_t)5 * (size_t)(p.lds_rows > 0 ? p.lds_rows : 0)); };
        rounds_lds = dyn_of(b_r);
        int st_lds = 0; int nb = poa_rounds_residency(sc->gap_mode, rounds_lds, &st_lds);
        // four workgroups per CU when the job has that many sets: the kernel's static LDS (graph phases) comes out of the backtrack window
        if (nb < 4 && J.n_sets > nb * 256) {
            const int budget = 160 * 1024 / 4 - st_lds - 512, excess = (int)rounds_lds - budget;
            if (excess > 0 && (size_t)b_r.lds.total_tail == rounds_lds && b_r.lds.bt_bytes_tail - ((excess + 15) & ~15) >= 8 * 1024) {
                b_r.lds.bt_bytes_tail -= (excess + 15) & ~15; b_r.lds.total_tail -= (excess + 15) & ~15;
                rounds_lds = dyn_of(b_r); nb = poa_rounds_residency(sc->gap_mode, rounds_lds, &st_lds);
            }
        }
        // Helpers of the backtrack that walk while the row loop still runs (backtrack_dir.h, EARLY START) need LDS of their own: the score ring -- or the main
        // walk's region, whichever is larger; the main walk comes after the rows and may alias the ring -- then three helper regions, then the tables, all inside
        // the dynamic LDS the launch has anyway, so the residency above is untouched.  Equal quarters when a quarter holds the ring (the late start's very
        // split); else the ring's bytes in front and a third of the rest per helper.  A helper region under SPEC_EARLY_MIN (6 KB: a 1.5 KB image and 18 whole
        // rows of a 1 kb int16 band, just above the 16 below which the windows fall back to column slices) keeps the late start, and so does
        // ABPOA_HIP_LATE_TAIL=1 (for comparison in one process).
        b_r.lds.te_on = 0;
        if (b_r.dir_mode && sc->gap_mode != ABPOA_HIP_LINEAR_GAP && !opt_on("ABPOA_HIP_LATE_TAIL")) {
            const int avail = (int)rounds_lds - b_r.lds.phase_off, tables = (SPEC_WK - 1) * SPEC_PM_ROWS * 4;
            const int ring = (b_r.lds.total_rows - b_r.lds.phase_off + 15) & ~15;
            int w_ = ((avail - tables) / SPEC_WK) & ~15, m_ = w_;
            if (w_ < ring) { m_ = ring; w_ = ((avail - tables - m_) / (SPEC_WK - 1)) & ~15; }
            if (w_ >= SPEC_EARLY_MIN) { b_r.lds.te_on = 1; b_r.lds.te_main = m_; b_r.lds.te_w = w_; }
        }
        // The kernel pays when every read-set of the job is resident at once (one workgroup each; 4 per CU): a larger job runs faster with one
        // launch per phase and round, whose single-wavefront row-loop kernel then has several alignments per SIMD to hide latency behind
        // (measured, 1 kb reads: 1000 sets 13.0 k vs 10.4 k read-sets/s; 2000 sets 12.9 k vs 13.6 k; 4000 sets 13.2 k vs 17.4 k)
        const int n_cu = device_cu_count(J.device);
        if (nb < 1 || J.n_sets > nb * n_cu) use_rounds = false;
        if (opt_set("ABPOA_HIP_VERBOSE")) fprintf(stderr,
                "[abpoa-hip] all-rounds kernel: %s, %zu B dynamic + %d B static LDS per workgroup, %d workgroups per CU, " "backtrack window %d B, helpers %s (%d + 3 x %d B)\n",
                use_rounds ? "on" : "off", rounds_lds, st_lds, nb, b_r.lds.bt_bytes_tail, b_r.lds.te_on ? "under the row loop" : "after the row loop", b_r.lds.te_main, b_r.lds.te_w);
    }
}

// ---- the two output tails of stage 8, the same steps each: lay out on the host what the device counted (the state block is down), grow the pools, upload the
//      offsets, fill on the device, download in one piece, synchronise
// MSA rows: rows x columns bytes per set, back to back
int queue_msa_output(Job &J, DeviceDebug &dbg) {
    Cache &C = *J.C; const Layout &L = J.L; hipStream_t st = C.stream; uint8_t *hi = C.in.host; int rc;
    J.M = lay_out_msa(J.pl, J.n_sets, J.sets, J.host_state());
    if (J.M.total <= 0) return 0;
    const size_t total = (size_t)J.M.total, off_bytes = 8 * (size_t)J.n_sets;
    if ((rc = C.msa.need_dev(total)) || (rc = C.msa.need_host(total))) return rc;
    memcpy(hi + L.o_msaoff_h, J.M.off.data(), off_bytes);
    HIP_OK(hipMemcpyAsync(C.graph.dev + L.o_msaoff, hi + L.o_msaoff_h, off_bytes, hipMemcpyHostToDevice, st), ABPOA_HIP_ELAUNCH);
    J.p.msa_out = C.msa.dev;
    HIP_OK(launch_poa_msa_fill(J.p, st), ABPOA_HIP_ELAUNCH);
    if (dbg.stage("msa fill", J.pl.max_reads)) return ABPOA_HIP_ELAUNCH;
    HIP_OK(hipMemcpyAsync(C.msa.host, C.msa.dev, total, hipMemcpyDeviceToHost, st), ABPOA_HIP_ELAUNCH);
    HIP_OK(hipStreamSynchronize(st), ABPOA_HIP_ELAUNCH);
    return 0;
}
// GFA output, phase 2: segment, link and path pools of the sets back to back (the walk's counts came down with the state block)
int queue_gfa_output(Job &J, DeviceDebug &dbg) {
    Cache &C = *J.C; const Layout &L = J.L; hipStream_t st = C.stream; uint8_t *hi = C.in.host, *hg = C.graph.host, *dg = C.graph.dev; int rc;
    J.G = lay_out_gfa(J.pl, J.n_sets, J.sets, J.host_state(), (const int32_t *)(hg + L.o_gcnt));
    if (!J.G.bytes) return 0;
    const size_t off_bytes = 32 * (size_t)J.n_sets; hipEvent_t *eg = C.ev.data() + J.ev.gfa();
    if ((rc = C.gfa.need_dev(J.G.bytes)) || (rc = C.gfa.need_host(J.G.bytes))) return rc;
    memcpy(hi + L.o_gfaoff_h, J.G.off.data(), off_bytes);
    HIP_OK(hipMemcpyAsync(dg + L.o_goff, hi + L.o_gfaoff_h, off_bytes, hipMemcpyHostToDevice, st), ABPOA_HIP_ELAUNCH);
    bind_gfa_pools(J.g, J.G, C.gfa.dev);
    HIP_OK(hipEventRecord(eg[2], st), ABPOA_HIP_ELAUNCH);
    HIP_OK(launch_poa_gfa_fill(J.p, J.g, st), ABPOA_HIP_ELAUNCH);
    HIP_OK(hipEventRecord(eg[3], st), ABPOA_HIP_ELAUNCH);
    if (dbg.stage("gfa fill", J.pl.max_reads)) return ABPOA_HIP_ELAUNCH;
    HIP_OK(hipMemcpyAsync(C.gfa.host, C.gfa.dev, J.G.o_cnt, hipMemcpyDeviceToHost, st), ABPOA_HIP_ELAUNCH);
    HIP_OK(hipMemcpyAsync(C.gfa.host + J.G.o_cnt, dg + L.o_gcnt, 12 * (size_t)J.n_sets, hipMemcpyDeviceToHost, st), ABPOA_HIP_ELAUNCH);      // (the fill kernel's flags)
    HIP_OK(hipStreamSynchronize(st), ABPOA_HIP_ELAUNCH);
    return 0;
}

// ---- stage 8: the whole progressive alignment, queued back to back (ABPOA_HIP_DEVSYNC=1: synchronise and report after every kernel), the downloads
int queue_job(Job &J, DeviceDebug &dbg) {
    const DevicePlan &pl = J.pl; Cache &C = *J.C; const Layout &L = J.L; PoaDev &p = J.p; const DevBatch &b = J.b;
    hipStream_t st = C.stream; uint8_t *hi = C.in.host, *hg = C.graph.host, *dg = C.graph.dev, *dr = C.rows.dev; int rc;
    const int64_t *roff = (const int64_t *)(hi + L.o_roff);
    auto stage = [&](const char *what, int k) { return dbg.stage(what, k); };
    // (all ones: no sub-graph alignments here; -s: no read is reverse-complemented yet -- on the stream behind the upload, before the first kernel)
    if (pl.gen_io()) HIP_OK(hipMemsetAsync(dr + L.o_act, 1, (size_t)pl.node_tot, st), ABPOA_HIP_ELAUNCH);
    if (pl.amb) HIP_OK(hipMemsetAsync(dg + L.o_isrc, 0, (size_t)pl.tot_reads, st), ABPOA_HIP_ELAUNCH);
    J.t_queue = now_s();
    HIP_OK(hipEventRecord(C.ev[J.ev.job_begin()], st), ABPOA_HIP_ELAUNCH);
    if (stage("upload", 0)) return ABPOA_HIP_ELAUNCH;
    HIP_OK(launch_poa_init(p, st), ABPOA_HIP_ELAUNCH);
    if (stage("init", 0)) return ABPOA_HIP_ELAUNCH;
    dbg.graph_check(0);
    HIP_OK(hipEventRecord(C.ev[J.ev.after_init()], st), ABPOA_HIP_ELAUNCH);
    for (int k = 1; k < pl.max_reads; ++k) {
        if (k == 2 && !J.rest_up) {      // round 1 is queued: stage and send the reads of the later rounds behind it
            stage_reads(J, 2, pl.max_reads);
            HIP_OK(hipMemcpyAsync(C.in.dev + L.o_reads + (size_t)J.split_at, hi + L.o_reads + (size_t)J.split_at, (size_t)(roff[pl.tot_reads] - J.split_at),
                    hipMemcpyHostToDevice, C.copy_stream), ABPOA_HIP_ELAUNCH);
            HIP_OK(hipEventRecord(C.ev_copy, C.copy_stream), ABPOA_HIP_ELAUNCH);
            HIP_OK(hipStreamWaitEvent(st, C.ev_copy, 0), ABPOA_HIP_ELAUNCH);
            J.rest_up = true;
        }
        if (J.use_rounds && k == 2) {      // rounds 2 .. n - 1 of every set in one launch
            HIP_OK(hipEventRecord(C.ev[J.ev.rounds_begin()], st), ABPOA_HIP_ELAUNCH);
            HIP_OK(launch_poa_rounds(p, J.b_r, (int32_t *)(dr + L.o_ticket), C.in.host + L.o_rargs, J.slot, 2, J.rounds_lds, st), ABPOA_HIP_ELAUNCH);
            HIP_OK(hipEventRecord(C.ev[J.ev.rounds_end()], st), ABPOA_HIP_ELAUNCH);
            break;
        }
        p.round = k;
        hipEvent_t *e = C.ev.data() + J.ev.round(k);
        if (p.order_mode) { HIP_OK(launch_poa_order(p, st), ABPOA_HIP_ELAUNCH); if (stage("row order", k)) return ABPOA_HIP_ELAUNCH; dbg.order_check(k); }
        HIP_OK(launch_poa_prepare(p, st), ABPOA_HIP_ELAUNCH);
        if (stage("prepare", k)) return ABPOA_HIP_ELAUNCH;
        dbg.prepare_check(k);
        HIP_OK(hipEventRecord(e[0], st), ABPOA_HIP_ELAUNCH);
        if (pl.general) { HIP_OK(launch_dp_general(b, st), ABPOA_HIP_ELAUNCH); HIP_OK(hipEventRecord(e[1], st), ABPOA_HIP_ELAUNCH); }
        else HIP_OK(launch_dp_fast(b, st, e[1]), ABPOA_HIP_ELAUNCH);
        if (stage("dp rows + tail", k)) return ABPOA_HIP_ELAUNCH;
        if (pl.amb) {
            HIP_OK(launch_poa_strand_check(p, st), ABPOA_HIP_ELAUNCH);
            HIP_OK(launch_dp_general(J.b_rc, st), ABPOA_HIP_ELAUNCH);
            HIP_OK(launch_poa_strand_pick(p, st), ABPOA_HIP_ELAUNCH);
            if (stage("strand retry", k)) return ABPOA_HIP_ELAUNCH;
        }
        dbg.balance_report(k, b, e[0], e[1]);
        HIP_OK(hipEventRecord(e[2], st), ABPOA_HIP_ELAUNCH);
        HIP_OK(launch_poa_fuse(p, st), ABPOA_HIP_ELAUNCH);
        if (stage("fuse", k)) return ABPOA_HIP_ELAUNCH;
        dbg.graph_check(k);
        HIP_OK(hipEventRecord(e[3], st), ABPOA_HIP_ELAUNCH);
    }
    // ---- consensus on the device, then one small download: per-set state + consensus (node ids, bases, coverage)
    if (pl.want_cons) { HIP_OK(launch_poa_consensus(p, st), ABPOA_HIP_ELAUNCH); if (stage("consensus", pl.max_reads)) return ABPOA_HIP_ELAUNCH; }
    if (pl.want_msa) { HIP_OK(launch_poa_msa_rank(p, st), ABPOA_HIP_ELAUNCH); if (stage("msa rank", pl.max_reads)) return ABPOA_HIP_ELAUNCH; }
    hipEvent_t *eg = C.ev.data() + J.ev.gfa();
    if (pl.want_gfa) {      // GFA output, phase 1: the walk order and the segment / link counts of every set (they come down with the state block)
        HIP_OK(hipEventRecord(eg[0], st), ABPOA_HIP_ELAUNCH);
        HIP_OK(launch_poa_gfa_walk(p, J.g, st), ABPOA_HIP_ELAUNCH);
        HIP_OK(hipEventRecord(eg[1], st), ABPOA_HIP_ELAUNCH);
        if (stage("gfa walk", pl.max_reads)) return ABPOA_HIP_ELAUNCH;
    }
    HIP_OK(hipMemcpyAsync(hg, dg, L.dl_bytes, hipMemcpyDeviceToHost, st), ABPOA_HIP_ELAUNCH);
    HIP_OK(hipStreamSynchronize(st), ABPOA_HIP_ELAUNCH);
    if (pl.want_msa && (rc = queue_msa_output(J, dbg))) return rc;
    if (pl.want_gfa && (rc = queue_gfa_output(J, dbg))) return rc;
    J.t_done = now_s();
    return 0;
}

// ---- stage 9: kernel durations from the events; the all-rounds kernel's split by the ticks its sets spent per phase
void fill_stats(const Job &J, DeviceRunStats *stats) {
    const DevicePlan &pl = J.pl; Cache &C = *J.C; const PoaDev &p = J.p; const PoaState *hs_ = J.host_state();
    // (library built with -DABPOA_HIP_ORDER_PROF: the order walk's passes and ticks per kind, mean per set)
    if (opt_set("ABPOA_HIP_ORDER_PROF") && p.order_mode) {
        double a_[4] = {0, 0, 0, 0};
        for (int s = 0; s < J.n_sets; ++s) for (int i = 0; i < 4; ++i) a_[i] += (double)hs_[s].t_phase[i];
        fprintf(stderr, "[abpoa-hip] order walk per set: %.0f single-node passes x %.0f ticks, %.0f parallel passes x %.0f ticks\n", a_[2] / J.n_sets,
                a_[2] > 0 ? a_[0] / a_[2] : 0.0, a_[3] / J.n_sets, a_[3] > 0 ? a_[1] / a_[3] : 0.0);
    }
    if (!stats) return;
    float ms = 0;
    hipEvent_t prev = C.ev[J.ev.after_init()];
    for (int k = 1; k < (J.use_rounds ? 2 : pl.max_reads); ++k) {
        hipEvent_t *e = C.ev.data() + J.ev.round(k);
        (void)hipEventElapsedTime(&ms, prev, e[0]); stats->prepare_ms += ms;
        (void)hipEventElapsedTime(&ms, e[0], e[1]); stats->rows_ms += ms;
        (void)hipEventElapsedTime(&ms, e[1], e[2]); stats->tail_ms += ms;
        (void)hipEventElapsedTime(&ms, e[2], e[3]); stats->fuse_ms += ms;
        prev = e[3];
    }
    if (J.use_rounds) {      // the all-rounds kernel: its duration, split by the shader-clock ticks the sets spent in each phase (PoaState.t_phase)
        (void)hipEventElapsedTime(&ms, C.ev[J.ev.rounds_begin()], C.ev[J.ev.rounds_end()]); stats->rounds_ms = ms; stats->rounds_launches = 1;
        double tp[4] = {0, 0, 0, 0}, tmax = 0; for (int s = 0; s < J.n_sets; ++s) { double t_ = 0;
                if (hs_[s].status == POA_ST_OK) stats->rounds_algo_bytes += hs_[s].algo_bytes - hs_[s].algo_bytes_before;
        for (int i = 0; i < 4; ++i) { tp[i] += (double)hs_[s].t_phase[i]; t_ += (double)hs_[s].t_phase[i]; } tmax = std::max(tmax, t_); }
        const double tall = tp[0] + tp[1] + tp[2] + tp[3];
        if (tall > 0) { stats->prepare_ms += ms * tp[0] / tall; stats->rows_ms += ms * tp[1] / tall; stats->tail_ms += ms * tp[2] / tall;
                stats->fuse_ms += ms * tp[3] / tall;
                        for (int i = 0; i < 4; ++i) stats->rounds_mticks[i] = tp[i] / J.n_sets * 1e-6; stats->rounds_rows_share = tp[1] / tall;
                        stats->rounds_mean_over_max = J.n_sets > 0 && tmax > 0 ? tall / J.n_sets / tmax : 0; }
        // how much of the kernel is its slowest set: per phase mean / p99 / max ticks of a set, and max over mean of the sets' totals
        if (opt_set("ABPOA_HIP_VERBOSE") && J.n_sets > 0 && tall > 0) {
            static const char *const ph_[4] = {"prepare", "rows", "backtrack", "fuse"};
            std::vector<double> v_((size_t)J.n_sets);
            for (int i = 0; i < 4; ++i) {
                for (int s = 0; s < J.n_sets; ++s) v_[s] = (double)hs_[s].t_phase[i];
                std::sort(v_.begin(), v_.end());
                fprintf(stderr, "[abpoa-hip] all-rounds kernel, M ticks per set, %-9s: mean %.3f  p99 %.3f  max %.3f\n", ph_[i], tp[i] / J.n_sets * 1e-6,
                        v_[(size_t)std::min<long long>(J.n_sets - 1, (long long)J.n_sets * 99 / 100)] * 1e-6, v_[(size_t)J.n_sets - 1] * 1e-6);
            }
            fprintf(stderr, "[abpoa-hip] all-rounds kernel, set totals: mean %.3f M ticks, max %.3f M ticks, max / mean %.3f\n", tall / J.n_sets * 1e-6, tmax * 1e-6,
                    tmax / (tall / J.n_sets));
        }
    }
    if (pl.want_gfa) {
        hipEvent_t *eg = C.ev.data() + J.ev.gfa();
        (void)hipEventElapsedTime(&ms, eg[0], eg[1]); stats->gfa_walk_ms = ms;
        if (J.G.bytes) { (void)hipEventElapsedTime(&ms, eg[2], eg[3]); stats->gfa_fill_ms = ms; }
        stats->gfa_d2h_bytes = (int64_t)J.G.bytes;
    }
    stats->n_rounds = pl.max_reads > 0 ? pl.max_reads - 1 : 0; stats->device_s = J.t_done - J.t_queue;
}

// ---- stage 10: the results of the sets that finished; the others into `fallback`
void collect_results(const Job &J, DeviceDebug &dbg, abpoa_hip_msa_t *out, std::vector<char> &need_fb, std::vector<SetFallback> *fallback) {
    const DevicePlan &pl = J.pl; Cache &C = *J.C; const PoaDev &p = J.p; const PoaState *hs = J.host_state();
    need_fb.assign(J.n_sets, 0);
    std::vector<AlnOut> h_out;      // (tests, with the cigar digests: the result record of every set's last alignment -- msa_batch.h last_aln_set)
    if (p.dig_on && J.n_sets > 0) { h_out.resize((size_t)J.n_sets);
            if (hipMemcpy(h_out.data(), p.out, sizeof(AlnOut) * (size_t)J.n_sets, hipMemcpyDeviceToHost) != hipSuccess) h_out.clear(); }
    parallel_ranges(std::min(J.n_threads, 8), J.n_sets, [&](int lo, int hi_) {
        for (int s = lo; s < hi_; ++s) {
            if (unpack_set(pl, J.L, J.M, J.G, J.sets[s], s, C.graph.host, C.msa.host, C.gfa.host, &out[s])) {
                need_fb[s] = 1;
                if (hs[s].status != POA_ST_OK && J.dbg_sync) fprintf(stderr, "[poa-device] set %d falls back to the host driver: reason %d, %d nodes of %d\n", s,
                        hs[s].reason, hs[s].n_nodes, pl.ps[s].node_cap);
                continue;
            }
            if (p.dig_on && J.sets[s].n_reads > 0) cigar_digest_set(J.sets[s].seqs[0], J.sets[s].lens[0], hs[s].cigar_dig);
            if (!h_out.empty() && J.sets[s].n_reads > 1) { const AlnOut &a_ = h_out[(size_t)s];
                    const int32_t v8[8] = {a_.n_matched_bases, a_.n_aln_bases, a_.node_s, a_.node_e, a_.query_s, a_.query_e, a_.n_cigar, a_.status};
                    last_aln_set(J.sets[s].seqs[0], J.sets[s].lens[0], v8); }
        }
    });
    dbg.msa_check(hs, out);
    dbg.gfa_check(hs, out);
    dbg.consensus_check(hs, out);
    // (a set with a node out of edge slots gains nothing from a pass with more node slots: the caller takes it to the last pass -- `roomy` above -- at once,
    //  and to the host driver if that was this one: a terminal with more than POA_TERM_MAX edges)
    for (int s = 0; s < J.n_sets; ++s) if (need_fb[s]) fallback->push_back({s, host_reason_of(hs[s].reason), hs[s].reason == POA_WHY_EDGE_SLOTS});
}

// ---- stage 11: ABPOA_HIP_VERBOSE: why sets left the pass
void report_fallbacks(const Job &J, const std::vector<SetFallback> &fallback) {
    const PoaState *hs = J.host_state();
    if (!opt_set("ABPOA_HIP_VERBOSE") || fallback.empty()) return;
    int n[MSA_HOST_REASONS] = {0};
    int dp_scores = 0;      // DP status: direction words could not decide (the arena too small for the rows' bands has a host reason of its own)
    for (const SetFallback &f : fallback) {
        const int r = hs[f.set].reason;
        n[f.why]++;
        if (r - POA_WHY_DP_STATUS == ABPOA_HIP_STATUS_NEED_SCORES) dp_scores++;
        if (f.why == HOST_WHY_ORDER_WALK || f.why == HOST_WHY_RANK_WALK || (f.why == HOST_WHY_OTHER && r != POA_WHY_NONE)) fprintf(stderr,
                "[abpoa-hip]   set %d: reason code %d (7: row order walk, 8: MSA rank walk, 1000 + a negative DP status: " "%d)\n", f.set, r, r - 1000);
    }
    const int n_dp = n[HOST_WHY_DP_ARENA] + n[HOST_WHY_DP_OTHER];
    if (n_dp) fprintf(stderr, "[abpoa-hip]   DP status: arena too small for the bands %d, direction words undecided %d, other %d\n", n[HOST_WHY_DP_ARENA],
            dp_scores, n[HOST_WHY_DP_OTHER] - dp_scores);
    fprintf(stderr, "[abpoa-hip] fallback reasons: node cap at init %d, pred CSR cap %d, cigar cap %d, node slots in the fuse "
            "phase %d, edge slots of a node full (redone in the last pass) %d, DP status %d, projected node growth "
            "(early exit at read 10) %d, other %d\n", n[HOST_WHY_NODES_AT_INIT], n[HOST_WHY_PRED_SLOTS], n[HOST_WHY_CIGAR_SLOTS], n[HOST_WHY_NODES_IN_FUSE],
            n[HOST_WHY_EDGE_SLOTS], n_dp, n[HOST_WHY_GROWTH], n[HOST_WHY_OTHER] + n[HOST_WHY_ORDER_WALK] + n[HOST_WHY_RANK_WALK]);
}

void finish_stats(const Job &J, const std::vector<char> &need_fb, DeviceRunStats *stats) {
    const PoaState *hs = J.host_state();
    stats->cons_s = now_s() - J.t_done; stats->total_s = now_s() - J.t_begin;
    for (int s = 0; s < J.n_sets; ++s) if (!need_fb[s]) {
        stats->n_cells += hs[s].n_cells; stats->algo_bytes += hs[s].algo_bytes; stats->n_alignments += std::max(0, J.sets[s].n_reads - 1);
        int mx = 0; for (int r = 0; r < J.sets[s].n_reads; ++r) mx = std::max(mx, J.sets[s].lens[r]);
        if ((int64_t)hs[s].n_nodes <= 2 + (int64_t)(3.0 * mx) + 1024) stats->n_fit_3x += 1;
    }
}
}  // namespace

// force_general: every alignment through the general kernel; *want_general: the final LDS plan has no fast row loop for this job although the first estimate had
// one (ragged sets: one node factor more, wider rows -- the score width can flip to 32 bits): the caller runs the job again with force_general
static int run_msa_device_body(const abpoa_hip_scoring_t *sc_in, int n_sets, const abpoa_hip_readset_t *sets, abpoa_hip_msa_t *out, int n_threads,
                               const DevicePass &pass, std::vector<SetFallback> *fallback, DeviceRunStats *stats, bool force_general, bool *want_general) {
    const int slot = pass.slot; int device = pass.device;
    if (slot < 0 || slot >= MSA_DEVICE_SLOTS) { set_err("bad device slot %d", slot); return ABPOA_HIP_EINVAL; }
    std::lock_guard<std::mutex> lk(g_cache_mu[slot]);
    if (device < 0) device = engine_device();
    if (device < 0) { set_err("engine not initialised"); return ABPOA_HIP_ENODEV; }
    Job J; int rc;
    J.sets = sets; J.n_sets = n_sets; J.n_threads = n_threads; J.device = device; J.slot = slot; J.C = &g_cache[slot];
    if ((rc = acquire_cache_slot(*J.C, device))) return rc;
    fallback->clear();
    if (stats) memset(stats, 0, sizeof(*stats));
    J.t_begin = now_s();
    J.pl = plan_device_job(sc_in, n_sets, sets, pass.node_factor, pass.flags, force_general);
    J.any_w = false; for (int s = 0; s < n_sets && !J.any_w; ++s) J.any_w = sets[s].weights != nullptr;
    J.L = lay_out_device(J.pl, n_sets, J.any_w); J.ev = EventSlots{J.pl.max_reads};
    if ((rc = fit_device(J)) || (rc = upload_reads(J))) return rc;
    bind_poa_dev(J.p, J.g, J.pl, J.L, n_sets, J.any_w, cigar_digest_on(), J.C->in.dev, J.C->graph.dev, J.C->rows.dev);
    if ((rc = fill_dev_batch(J, want_general))) return rc;
    plan_rounds(J);
    DeviceDebug dbg(&J.p, &J.pl.ps, sets, n_sets, J.pl.sc.m, J.pl.aln_cap, J.pl.max_reads, J.pl.want_msa, J.pl.amb, J.C->stream, J.pl.want_gfa);      // (ABPOA_HIP_DEVSYNC=1; msa_device_debug.h)
    if ((rc = queue_job(J, dbg))) return rc;
    fill_stats(J, stats);
    std::vector<char> need_fb;
    collect_results(J, dbg, out, need_fb, fallback);
    report_fallbacks(J, *fallback);
    if (stats) finish_stats(J, need_fb, stats);
    return ABPOA_HIP_OK;
}

int run_msa_device(const abpoa_hip_scoring_t *sc, int n_sets, const abpoa_hip_readset_t *sets, abpoa_hip_msa_t *out, int n_threads, const DevicePass &pass,
                   std::vector<SetFallback> *fallback, DeviceRunStats *stats) {
    bool want_general = false;
    const int rc = run_msa_device_body(sc, n_sets, sets, out, n_threads, pass, fallback, stats, false, &want_general);
    if (rc != ABPOA_HIP_EINVAL || !want_general) return rc;
    // the job stays on the device: the general kernel takes what the fast row loops' final plan could not (it used to leave for the host driver)
    want_general = false;
    return run_msa_device_body(sc, n_sets, sets, out, n_threads, pass, fallback, stats, true, &want_general);
}

}  // namespace abpoa_hip
