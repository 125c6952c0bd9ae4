// Planning step of the device-resident read-set driver and the LDS carve-up of a launch (msa_device_plan.h, engine.h LdsPlan): host arithmetic only, no call
// into the HIP runtime.  lds_fixed_bytes_dp / _bt come from the kernels' translation unit (dp_general.hip); a CPU harness links its own.
#include <algorithm>
#include <limits.h>
#include <string.h>
#include "engine_options.h"
#include "msa_device_plan.h"
#include "routing.h"

namespace abpoa_hip {

// LDS carve-up of one wavefront (engine.h LdsPlan) for a launch whose largest query is max_qlen, widest score type max_bits
// and widest expected band est_cols columns.
constexpr int WIDE_PER_CU_MAX = 8, WIDE_RING_MIN = 4;
void make_lds_plan(const abpoa_hip_scoring_t *sc, int max_qlen, int max_bits, int64_t est_cols, int n_aln, LdsPlan *Lp) {
    LdsPlan &L = *Lp;
    const int P = sc->gap_mode == ABPOA_HIP_LINEAR_GAP ? 1 : (sc->gap_mode == ABPOA_HIP_AFFINE_GAP ? 3 : 5);
    const int cell = max_bits / 8, npr = P == 1 ? 1 : (P == 3 ? 2 : 3);
    // query codes in LDS: up to 32000 bases keep the fast row loops (their per-row registers hold band vectors in 12 bits: 4095 x 8 columns);
    // longer reads take the general kernel.  Above 16 K bases the kernels may use up to 62 KB of LDS per wavefront instead of 36 - 38 KB.
    const bool longq = max_qlen + 1 > 16384;
    L.q_off = 0; L.q_cap = max_qlen + 1 <= 32000 ? (int)align_up(max_qlen + 1, 16) : 0;
    L.mat_off = L.q_cap; L.mx_off = L.mat_off + (int)align_up(4 * sc->m * sc->m, 16);
    L.phase_off = L.mx_off + (int)align_up(4 * sc->m * (sc->m + 1), 16);
    L.ring_off = lds_fixed_bytes_dp(); L.ring_rows = 16; L.ring_cols = (int)align_up((size_t)est_cols, 64);
    while ((int64_t)L.ring_rows * npr * L.ring_cols * cell > 40 * 1024 && L.ring_rows > 4) L.ring_rows /= 2;
    if ((int64_t)L.ring_rows * npr * L.ring_cols * cell > 40 * 1024) L.ring_cols = 0;     // rows too wide: HBM path only
    const int ring_bytes = L.ring_rows * npr * L.ring_cols * cell;
    L.bt_off = lds_fixed_bytes_bt();
    // staged arena window of the backtrack: 24 KB, less when a long query already takes much of the 40 KB a workgroup may use
    L.bt_bytes = std::max(std::max(8 * 1024, std::min(24 * 1024, (longq ? 62 : 38) * 1024 - L.phase_off - L.bt_off)), L.ring_off + ring_bytes - L.bt_off) & ~15;
    // fast row loop: packed score ring (words per cell: linear 1, int16 affine 1, int16 convex 2, int32 affine 2, int32 convex 3)
    const int fw = P == 1 ? 1 : (max_bits == 16 ? (P == 3 ? 1 : 2) : (P == 3 ? 2 : 3));      // (linear gaps: H alone)
    L.fr_off = 0; L.fr_rows = 16; L.fr_cols = fw ? std::max(128, (int)align_up((size_t)est_cols, 64)) : 0;      // >= 128: the turbo row pads one chunk unconditionally
    const int fr_budget = (longq ? 62 : 36) * 1024 - L.phase_off;
    while (L.fr_cols && (int64_t)L.fr_rows * fw * (L.fr_cols + 4) * 4 + 64 > fr_budget && L.fr_rows > 4) L.fr_rows /= 2;
    if (L.fr_cols && (int64_t)L.fr_rows * fw * (L.fr_cols + 4) * 4 + 64 > fr_budget) L.fr_cols = 0;
    if (L.q_cap == 0 || est_cols > 1024) L.fr_cols = 0;
    if (opt_on("ABPOA_HIP_NOFAST")) L.fr_cols = 0;
    const int fr_bytes = L.fr_cols ? L.fr_rows * fw * (L.fr_cols + 4) * 4 + 64 : 0;
    L.total = L.phase_off + std::max(std::max(L.ring_off + ring_bytes, L.bt_off + L.bt_bytes), L.fr_off + fr_bytes);
    // the fast path's tail kernel: its own window size -- 28 KB, less when a long query already takes much of the 38 (62) KB that let four (two) of
    // its workgroups share a CU; the general kernel's bt_bytes above also covers its score ring and would halve that residency
    L.bt_bytes_tail = std::max(8 * 1024, std::min(28 * 1024, (longq ? 62 : 38) * 1024 - L.phase_off - L.bt_off)) & ~15;
    // a launch with fewer alignments than 4 per CU can afford a larger window per workgroup (fewer window reloads on wide bands): 160 KB / CU
    // divided by the workgroups a CU has to hold, capped at 56 KB
    { const int per_cu = std::max(1, (n_aln + 255) / 256);
      if (per_cu < 4 && L.fr_cols > 128) L.bt_bytes_tail = std::max(L.bt_bytes_tail, std::min(56 * 1024, 160 * 1024 / per_cu - 2048 - L.phase_off - L.bt_off) & ~15); }
    // more alignments than a GPU holds tail workgroups at the 24 KB window (4 per CU): a 12 KB window doubles the residency, and the tail kernel of such
    // a launch runs in as many turns as it has workgroups per resident set (8000 x 1 kb alignments: tail 153 -> 127 ms per step)
    if (n_aln > 4 * 256 && L.fr_cols && L.fr_cols <= 128) L.bt_bytes_tail = std::min(L.bt_bytes_tail, 12 * 1024);
    { const int tb_ = opt_int("ABPOA_HIP_BT_BYTES", 0); if (tb_ >= 4096 && tb_ <= 65536) L.bt_bytes_tail = tb_ & ~15; }
    L.total_rows = L.phase_off + L.fr_off + fr_bytes; L.total_tail = L.phase_off + L.bt_off + L.bt_bytes_tail;
    L.te_on = L.te_main = L.te_w = 0;      // (the all-rounds kernel's split of the backtrack region: msa_device.cpp decides it where that kernel runs)
    L.bt_wc = 0; { const int wc_ = opt_int("ABPOA_HIP_BT_WC", 0); if (wc_ >= 8 && wc_ <= 64) L.bt_wc = wc_ & ~7; }
    // local row loop (rows_local.h): unbanded local alignments of at most 9 x 64 columns, int16; ring depth by what 60 KB hold
    L.loc_rows = L.loc_cols = L.total_local = 0;
    if (sc->align_mode == ABPOA_HIP_LOCAL_MODE && sc->wb < 0 && P != 1 && L.q_cap && !opt_on("ABPOA_HIP_NOFAST")) {
        const int lw = P == 3 ? 1 : 2;                 // ring words per column (int16: H | E1 packed, E2)
        L.loc_cols = 9 * 64; L.loc_rows = 16;
        while ((int64_t)L.loc_rows * lw * (L.loc_cols + 4) * 4 > 60 * 1024 - L.phase_off && L.loc_rows > 4) L.loc_rows /= 2;
        L.total_local = L.phase_off + L.fr_off + (int)align_up((size_t)L.loc_rows * lw * (L.loc_cols + 4) * 4, 16) + 256;      // (+ the team kernel's exchange slots: 2 x 4 x 16 bytes)
    }
    // wide row loop (dp_wide_rows.hip): alignments whose band half-width w is in [wide_w_lo, wide_w_hi] -- rows of 2..7 chunks of 64 columns --
    // go to the kernel that keeps every chunk of a row in registers; it has its own score ring (448 columns; depth by what fits:
    // predecessors up to 15 rows back are common in a graph of noisy reads).  ABPOA_HIP_NOWIDE=1 turns it off, ABPOA_HIP_RING_ROWS sets
    // the depth.
    L.wide_on = 0; L.wfr_rows = L.wfr_cols = L.wx_off = L.total_wide = 0; L.wide_w_lo = 1; L.wide_w_hi = 0; L.narrow_off = 0; L.w_mx_off = L.w_phase_off = 0;
    if (L.fr_cols && L.q_cap && !opt_on("ABPOA_HIP_NOWIDE")) {
        L.wide_on = 1;
        // (rows wider than the 448-column ring -- reads of 20 kb and more: w = 10 + 0.01 L -- take the kernel's long-read form: 704 columns, 8 - 11 chunks a row)
        L.wfr_cols = (est_cols > WIDE_RING_COLS && !opt_on("ABPOA_HIP_NOXL")) ? WIDE_RING_COLS_XL : WIDE_RING_COLS; L.wfr_rows = 16;
        if (sc->m > 16) L.wide_on = 0;      // (4-bit query codes)
        L.w_mx_off = (int)align_up((size_t)(max_qlen + 2) / 2, 16); L.w_phase_off = L.w_mx_off + (int)align_up(4 * sc->m * (sc->m + 1), 16);
        // ring words per column of the wide kernels: as the narrow loop's, but two instead of three for convex int32 (rows_fast.h EPACK: E as 16-bit
        // differences to H, which needs gap-open + extend <= 65535)
        const int fww = (P == 5 && max_bits == 32) ? 2 : fw;
        if (P == 5 && (sc->gap_open1 + sc->gap_ext1 >= 65535 || sc->gap_open2 + sc->gap_ext2 >= 65535)) L.wide_on = 0;      // (0xffff: "E is inf" in the compact spill records)
        L.wide_w_lo = 40; L.wide_w_hi = (L.wfr_cols - 2 * 8 - 1) / 2;
        { const int lo_ = opt_int("ABPOA_HIP_WIDE_LO", 0); if (lo_ > 0) L.wide_w_lo = lo_; }
        const int rr_ = opt_int("ABPOA_HIP_RING_ROWS", 0); const bool rr_env_ = rr_ >= 4;
        if (rr_env_) L.wfr_rows = rr_ >= 16 ? 16 : (rr_ >= 8 ? 8 : 4);
        // (up to 120 KB per wavefront: a convex int32 ring of 16 rows is 58 KB; above 64 KB the launch raises the kernel's dynamic-LDS limit)
        const int budget = 120 * 1024 - L.w_phase_off - 512;
        while ((int64_t)L.wfr_rows * fww * (L.wfr_cols + 4) * 4 > budget && L.wfr_rows > 4) L.wfr_rows /= 2;
        // One wavefront per alignment: LDS is what limits how many alignments a CU holds.  It is handed out in pieces of 1280 B, 128 per CU
        // (tools/probes/lds_granule.hip: 3 x 53760 B fit a CU, 3 x 54080 B do not, whatever the occupancy query says).  The deepest ring with which
        // the whole launch is resident, counting at most eight workgroups per CU -- two wavefronts per SIMD, which is what the registers allow and
        // what pays: a SIMD with two alignments to issue from does 1.6x the rows of one with a single wavefront (tools/two_waves_probe.py).  A
        // shallower ring sends more rows to the HBM gather (predecessor older than the ring: 0.5 % / 14 % / ~45 % of the rows of a 15 %-error
        // graph at depth 16 / 8 / 4; rows +1.6 % / +6.5 %).
        auto per_cu_ = [&](int rows_) { return std::min<int64_t>(WIDE_PER_CU_MAX, 128 / ((L.w_phase_off + (int64_t)rows_ * fww * (L.wfr_cols + 4) * 4 + 1279) / 1280)); };
        if (!(rr_env_)) {
            const int top_ = L.wfr_rows; int best_ = top_;
            for (int r_ = top_; r_ >= WIDE_RING_MIN; r_ /= 2) {
                if (per_cu_(r_) > per_cu_(best_)) best_ = r_;
                if (per_cu_(r_) * 256 >= std::min(n_aln, WIDE_PER_CU_MAX * 256)) { best_ = r_; break; }
            }
            L.wfr_rows = best_;
        }
        L.wx_off = L.fr_off + (int)align_up((size_t)L.wfr_rows * fww * (L.wfr_cols + 4) * 4, 16);
        L.total_wide = L.w_phase_off + L.wx_off;
        if (P == 1) L.wide_on = 0;      // (linear gaps: the narrow loop only -- routing.h fast_global_aln)
    }
}

int wide_workgroups_per_cu(int total_wide) { return std::min(WIDE_PER_CU_MAX, 128 / ((total_wide + 1279) / 1280)); }

namespace {
// The LDS plan of a job whose longest read is max_qlen, for the score width that n_rows graph rows would need and rows as wide as the band estimate
// (engine.h band_cols; banded = false: the whole query); returns that score width
int estimate_lds(const abpoa_hip_scoring_t *sc, int n_rows, int max_qlen, bool banded, int n_aln, LdsPlan *pl) {
    int32_t inf_d; const int mb = abpoa_hip_score_bits(sc, n_rows, max_qlen, &inf_d); const int pn = mb == 16 ? 16 : 8;
    const int w = sc->wb + (int)(sc->wf * (float)max_qlen);
    make_lds_plan(sc, max_qlen, mb, band_cols(padded_width(max_qlen, pn), w, pn, banded), n_aln, pl);
    return mb;
}
// jobs the fast row loops exist for: banded global / extension (rows_fast.h), local with affine / convex gaps (rows_local.h; the plan turns the band off)
bool global_loops_job(const abpoa_hip_scoring_t *sc) { return fast_global_job(sc->gap_mode, sc->align_mode, sc->wb, sc->gap_ext1); }
bool local_job(const abpoa_hip_scoring_t *sc) { return local_loop_job(sc->gap_mode, sc->align_mode, -1); }
int longest_read(const abpoa_hip_readset_t &S) { int mx = 0; for (int r = 0; r < S.n_reads; ++r) mx = std::max(mx, S.lens[r]); return mx; }
}  // namespace

// What the device-resident driver takes: every gap model and alignment mode (run_msa_device picks the fast row loops or the general kernel per job), any
// alphabet of up to 27 codes, consensus and / or MSA output, per-base weights, the strand retry.
bool msa_device_eligible(const abpoa_hip_scoring_t *sc, unsigned flags) {
    if (opt_on("ABPOA_HIP_HOSTGRAPH")) return false;
    if (sc->m - 1 > POA_ALN_MAX || sc->m < 2) return false;
    // (-s on the host driver, as before round 4)
    if ((flags & ABPOA_HIP_AMB_STRAND) && opt_on("ABPOA_HIP_NO_DEVICE_STRAND")) return false;
    if (sc->align_mode == ABPOA_HIP_LOCAL_MODE && opt_on("ABPOA_HIP_NO_DEVICE_LOCAL")) return false;
    // every gap model and alignment mode: the fast row loops where they apply (banded global, short local), the general kernel otherwise (linear gaps,
    // extension mode with or without z-drop, global mode without a band, long local reads).  ABPOA_HIP_NO_DEVICE_GENERAL=1 sends those back to the host driver.
    const bool fast = global_loops_job(sc) || local_job(sc);
    if (!fast && opt_on("ABPOA_HIP_NO_DEVICE_GENERAL")) return false;
    return true;
}

int wide_sets_per_cu(const abpoa_hip_scoring_t *sc, int n_sets, const abpoa_hip_readset_t *sets) {
    int max_qlen = 0; for (int s = 0; s < n_sets; ++s) max_qlen = std::max(max_qlen, longest_read(sets[s]));
    if (max_qlen <= 0) return 0;
    const int w_max = sc->wb + (int)(sc->wf * (float)max_qlen);
    LdsPlan pl; estimate_lds(sc, 3 * max_qlen + 1024, max_qlen, true, n_sets, &pl);
    if (!takes_wide_band(pl, w_max) || pl.total_wide <= 0) return 0;
    // (LDS is handed out in pieces of 1280 B, 128 per CU: tools/probes/lds_granule.hip; 166-192 VGPRs: two wavefronts per SIMD at most)
    return std::max(1, wide_workgroups_per_cu(pl.total_wide));
}

namespace {
// ---- sizes
void job_sizes(DevicePlan &P, int n_sets, const abpoa_hip_readset_t *sets, int64_t *max_cap0) {
    P.max_reads = P.max_qlen = 0; P.tot_reads = P.tot_bases = 0; *max_cap0 = 0;
    for (int s = 0; s < n_sets; ++s) {
        P.max_reads = std::max(P.max_reads, sets[s].n_reads); P.tot_reads += sets[s].n_reads;
        int64_t sum = 0; const int mx = longest_read(sets[s]);
        for (int r = 0; r < sets[s].n_reads; ++r) sum += sets[s].lens[r];
        P.max_qlen = std::max(P.max_qlen, mx);
        P.tot_bases += sum; *max_cap0 = std::max(*max_cap0, std::min<int64_t>(2 + sum, 2 + (int64_t)(P.node_factor * mx) + 1024));
    }
    P.w_max = P.sc.wb + (int)(P.sc.wf * (float)P.max_qlen);
    P.aln_cap = std::max(1, P.sc.m - 1); P.rid_words = (P.want_msa || P.want_gfa) ? std::max(1, (P.max_reads + 63) / 64) : 0;
}

// Which kernels: the fast row loops (rows_fast.h: banded global, affine / convex; rows_local.h: local, int16, up to 575 columns) or -- `general` -- the
// general kernel (rows_general.h: linear gaps, extension mode, global without a band, longer local reads), one launch per round like the wide-band jobs.
void choose_kernels(DevicePlan &P, int n_sets, const abpoa_hip_readset_t *sets, int64_t max_cap0, bool force_general) {
    const abpoa_hip_scoring_t *sc = &P.sc; const bool banded = !(P.local || P.unbanded);
    {   LdsPlan pl; const int mb = estimate_lds(sc, (int)max_cap0, P.max_qlen, banded, n_sets, &pl);
        // (extension mode, round 5: the same banded rows plus the running best cell / z-drop of reference :1018-1026 -- rows_fast.h commit_row)
        bool fast_global = global_loops_job(sc) && fast_loop_fits(pl, P.max_qlen);
        // (linear gaps, round 5: the narrow row loop only -- every alignment of the job must take it, routing.h takes_fast: band half-widths below the wide
        //  loop's, no read-set with ragged ends; anything else is the general kernel's as before)
        if (fast_global && sc->gap_mode == ABPOA_HIP_LINEAR_GAP) {
            if (!fast_global_aln(sc->gap_mode, P.w_max, 0)) fast_global = false;
            for (int s = 0; s < n_sets && fast_global; ++s) if (msa_device_set_is_ragged(sets[s])) fast_global = false;      // (the `extra` rule below)
        }
        P.fast_local = local_job(sc) && local_loop_fits(pl, mb, P.max_qlen);
        P.general = !(fast_global || P.fast_local);
        if (opt_on("ABPOA_HIP_DEVICE_GENERAL")) P.general = true;      // (tests: the general kernel for every job)
        if (force_general) P.general = true;
        if (P.general) P.fast_local = false;
    }
    // direction-plane arenas (dir_plane.h) whenever the penalties allow it: 2 / 4 bytes per cell instead of 8 - 32; ABPOA_HIP_NODIR=1 keeps the score records
    // the last pass of the ladder (msa_passes.cpp run_pass_ladder): edge slots for one edge per read at every node -- a node takes at most one new in-edge and one new
    // out-edge per read, so a set can no longer run out of them (the terminals keep their pools: reads that start / end on different nodes); score records
    // instead of direction words there (dir_plane.h names a predecessor by its list index in four bits)
    P.roomy = P.node_factor >= 4096.0;
    P.in_cap = P.roomy ? std::max((int)POA_IN_CAP, std::min(250, P.max_reads + 1)) : POA_IN_CAP;
    P.out_cap = P.roomy ? std::max((int)POA_OUT_CAP, std::min(250, P.max_reads + 1)) : POA_OUT_CAP;
    P.dir = !P.local && !P.extend && !P.general && !P.amb && P.in_cap <= POA_IN_CAP && dir_words_allowed(sc);
    // band half-widths that take the wide row loop (LdsPlan.wide_w_lo / hi; none when the wide kernels are off), depth of its score ring
    P.wide_lo = 1; P.wide_hi = 0; P.wide_ring_rows = 16; P.wide_on = P.wfr_cols = 0;
    { LdsPlan pl; estimate_lds(sc, 3 * P.max_qlen + 1024, P.max_qlen, banded, n_sets, &pl);
      if (pl.wide_on >= 1 && !P.local && !P.general) { P.wide_lo = pl.wide_w_lo; P.wide_hi = pl.wide_w_hi; P.wide_ring_rows = pl.wfr_rows; P.wide_on = pl.wide_on;
              P.wfr_cols = pl.wfr_cols; } }
}

// Reads of very different lengths (ends cut at different places; a short read against a long graph): the band is anchored at `qlen - remaining length`
// (reference abpoa_align.h:34-35), which then sits as far from the alignment's path as the lengths differ, and every row is that much wider than 2 w.
// Such a set gets `extra` columns in its arena and ring estimates, and its alignments take the wide row loop as if half of them were band half-width
// (AlnDesc.pad0, routing.h route_w). Lengths within an eighth of the longest read (at least 64 bases; indel noise: a 25 %-error 400-base set spreads 8
//  %) count as equal: the estimates' own slack
// (3 vectors + 32 columns) covers those.
// (route: the part of `extra` that counts for the choice of the row loop)
void ragged_columns(DevicePlan &P, int n_sets, const abpoa_hip_readset_t *sets) {
    const abpoa_hip_scoring_t *sc = &P.sc;
    P.extra.assign(n_sets, 0); P.route.assign(n_sets, 0); P.max_extra = 0; P.weff_lo = INT_MAX; P.weff_hi = 0;
    // (experiments: sets with less extra keep the narrow loop)
    const int route_min = opt_int("ABPOA_HIP_EXTRA_ROUTE_MIN", 0);
    if (!P.local && !P.general && sc->wb >= 0) for (int s = 0; s < n_sets; ++s) {
        int mx = 0, mn = INT_MAX; for (int r = 0; r < sets[s].n_reads; ++r) { mx = std::max(mx, sets[s].lens[r]); mn = std::min(mn, sets[s].lens[r]); }
        if (sets[s].n_reads < 2) continue;
        const int spread = mx - mn, tol = std::max(64, mx / 8);
        P.extra[s] = spread > tol ? std::min((spread + 15) & ~15, 2048) : 0;
        P.max_extra = std::max(P.max_extra, P.extra[s]);
        P.route[s] = P.extra[s] >= route_min ? P.extra[s] : 0;
        P.weff_lo = std::min(P.weff_lo, route_w(sc->wb + (int)(sc->wf * (float)mn), P.route[s]));
        P.weff_hi = std::max(P.weff_hi, route_w(sc->wb + (int)(sc->wf * (float)mx), P.route[s]));
    }
    if (P.weff_hi == 0) { P.weff_lo = 0; }
}

// the per-set table (poa_device.h PoaSet) with its offsets into the pools, and the pool totals
void set_table(DevicePlan &P, int n_sets, const abpoa_hip_readset_t *sets) {
    P.ps.assign(n_sets, PoaSet());
    P.node_tot = P.pred_tot = P.cig_tot = P.scr_tot = P.plane_tot = P.cons_tot = P.term_tot = 0; P.max_node_cap = 0;
    int64_t read_i = 0;
    for (int s = 0; s < n_sets; ++s) {
        PoaSet &S = P.ps[s]; memset(&S, 0, sizeof(S));
        int64_t sum = 0; int mx = 0;
        for (int r = 0; r < sets[s].n_reads; ++r) { sum += sets[s].lens[r]; mx = std::max(mx, sets[s].lens[r]); }
        // graph nodes this set may grow to on the device (a set with ragged ends gets one read length more: its reads reach beyond each other's ends, and a
        // straggler that needs a second pass costs the whole job that pass's latency -- 3 of 1024 such sets were 149 ms on top of 216)
        const int64_t cap = std::min<int64_t>(2 + sum, 2 + (int64_t)((P.node_factor + (P.extra[s] > 0 ? 1.0 : 0.0)) * mx) + 1024);
        S.n_reads = sets[s].n_reads; S.node_cap = (int)cap; S.pred_cap = (int)(4 * cap);
        S.read0 = read_i; read_i += sets[s].n_reads;
        S.term0 = P.term_tot; P.term_tot += sets[s].n_reads + 2;      // (source out-edges / sink in-edges beyond the per-node slots: at most one of each per read)
        S.node0 = P.node_tot; P.node_tot += cap + 1;
        S.pred0 = P.pred_tot; P.pred_tot += S.pred_cap;
        // cigar slots: four times the words of a backtrack where the all-rounds kernel's helper wavefronts write their parts (backtrack_dir.h SPEC_WK,
        //  dir_walk_pair)
        // (four times: parts 1-3 take the words of the helper wavefronts)
        S.cigar_cap = (int)(cap + mx + 8); S.cigar_off = P.cig_tot; P.cig_tot += ((P.rounds_possible && S.cigar_cap < 65536) ? 4 : 1) * (int64_t)S.cigar_cap;
        // (fuse: 3 x qlen + nodes; order / rank passes: up to four tables of one int per node)
        S.scratch0 = P.scr_tot; P.scr_tot += 3LL * P.max_qlen + 4 * cap + 8;
        S.cons_cap = (int)std::min<int64_t>(cap, 2LL * mx + 64); S.cons0 = P.cons_tot; P.cons_tot += S.cons_cap;
        S.band_extra = P.route[s];
        P.max_node_cap = std::max(P.max_node_cap, (int)cap);
    }
}
}  // namespace

// arenas: the widest score type a set can reach decides the cell size; columns per row as the band estimate of engine.cpp
void DevicePlan::size_arenas(const abpoa_hip_readset_t *sets, bool dw) {
    plane_tot = 0; set_wide.assign(ps.size(), 0); set_dir.assign(ps.size(), 0); any_wide_set = false;
    const int pct_ = opt_int("ABPOA_HIP_ARENA_PCT", 0);
    for (size_t s = 0; s < ps.size(); ++s) {
        PoaSet &S = ps[s]; const int mx = longest_read(sets[s]);
        const int64_t cap = S.node_cap;
        int32_t inf_dummy; const int bits = abpoa_hip_score_bits(&sc, (int)cap, mx, &inf_dummy); const int pn = bits == 16 ? 16 : 8;
        const int64_t width = padded_width(mx, pn);
        const int w = sc.wb + (int)(sc.wf * (float)mx);
        int64_t est = std::min<int64_t>(width, est_cols(width, w, pn) + extra[s]);
        // (a set comes back to a later pass also because its ROWS were wider than the estimate -- extension mode on reads that end early, the band pushed off
        //  its anchor -- and for a set of a few reads the node slots of every pass are the same number, the sum of its reads: the later passes grow the columns
        //  with the slots, the last one takes whole rows while that stays under 1 GB per set; found by tools/fuzz_device_vs_oracle.py seed 770500103)
        int64_t sum_len = 0; for (int r = 0; r < sets[s].n_reads; ++r) sum_len += sets[s].lens[r];
        const bool slots_fixed = 2 + sum_len <= 2 + (int64_t)(3.0 * mx) + 1024;      // (a few reads: the 3x estimate already is the bound, no pass has more node slots or rows)
        // (sets whose slots DO grow keep the plain estimate in passes 2 and 3: 10 kb reads at 15 % error start at 4.5x / 6x, and wider arenas would halve the
        //  read-sets a pass holds -- configs[2] 405 -> 281 read-sets/s when this first went in for every set)
        if (node_factor > 3.0 && (roomy || slots_fixed)) {
            const double cellb = dir ? (double)(DB + 8) : (double)CW * (bits / 8);
            int64_t e2 = roomy ? width : std::min<int64_t>(width, (int64_t)((double)est * node_factor / 3.0));
            if (roomy && (double)e2 * (double)cap * cellb > 1e9) e2 = std::min<int64_t>(width, est * 4);
            est = std::max(est, e2);
        }
        // (direction words for every row, score records for the first row and for about one row in four -- rows a successor beyond the score ring or the
        //  global best will read from HBM; half of the rows where the wide loop's ring is only four rows deep; a set that needs more is flagged and
        //  redone like any other capacity miss)
        // (which row loop and which arena format the set's alignments will take: routing.h takes_wide / takes_dir at the set's longest read)
        const bool wide_s = !local && in_wide_range(wide_lo, wide_hi, route_w(w, route[s]));
        const bool dir_s = dir_for(dir ? (dw ? 2 : 1) : 0, wide_s);
        set_wide[s] = wide_s; set_dir[s] = dir_s; any_wide_set |= wide_s;
        const int64_t rec_div = (wide_s && wide_ring_rows <= 4) ? 2 : 4;
        // (bytes per cell record of a row that keeps its scores: CW values -- the wide kernel's compact records: 4 B int16 affine, else 8 B; rows_fast.h
        //  CWR)
        const int64_t recb = wide_s ? ((bits == 16 && CW == 4) ? 4 : 8) : CW * (bits / 8);
        // (local row loop, rows_local.h: every row the whole query wide, cell records, 64 records of slack behind the last row)
        int64_t bytes = local ? (int64_t)align_up((size_t)((width * cap + 64) * CW * (bits / 8) + 64 * 8 * 4))
                            : dir_s ? (int64_t)align_up((size_t)(width * (DB + recb) + (est * DB + est * recb / rec_div + 32) * (cap - 1) + 64 * 8 * 4))
                                  : (int64_t)align_up((size_t)((width + est * (cap - 1)) * CW * (bits / 8) + 64 * 8 * 4));
        // (tests, as in the flat engine: under-sized arenas in the 3x pass -- room for the first rows, then the row loops of its sets end with the overflow
        //  status in mid-graph and a later pass redoes them)
        if (!local && node_factor <= 3.0 && pct_ > 0 && pct_ < 100)
            bytes = std::max<int64_t>((int64_t)align_up((size_t)(2 * width * (DB + recb) + 64 * 8 * 4)), (int64_t)align_up((size_t)(bytes * pct_ / 100)));
        S.plane_off = plane_tot; S.plane_cap = bytes - 64 * 8 * 4; plane_tot += bytes;
    }
}

DevicePlan plan_device_job(const abpoa_hip_scoring_t *sc_in, int n_sets, const abpoa_hip_readset_t *sets, double node_factor, unsigned flags, bool force_general) {
    DevicePlan P;
    P.sc = *sc_in; P.node_factor = node_factor;
    P.local = sc_in->align_mode == ABPOA_HIP_LOCAL_MODE; P.extend = sc_in->align_mode == ABPOA_HIP_EXTEND_MODE;
    if (P.local) P.sc.wb = -1;                                  // reference abpoa_post_set_para, src/abpoa_align.c:150
    const abpoa_hip_scoring_t *sc = &P.sc;
    // -s: low-scoring reads are aligned again as their reverse complement (poa_device.hip poa_strand_check_kernel)
    P.amb = flags & ABPOA_HIP_AMB_STRAND;
    P.want_msa = flags & ABPOA_HIP_OUT_MSA; P.want_gfa = flags & ABPOA_HIP_OUT_GFA; P.want_cons = (flags & ABPOA_HIP_OUT_CONS) || !(P.want_msa || P.want_gfa);
    // values per DP column in an arena of score records: one padded cell record of the fast loops (4 / 8 values) = the planes of the general kernel (engine.cpp
    //  pv)
    P.CW = record_values(sc->gap_mode);
    P.DB = sc->gap_mode == ABPOA_HIP_AFFINE_GAP ? 2 : 4;
    P.unbanded = sc->wb < 0;
    int64_t max_cap0 = 0;
    job_sizes(P, n_sets, sets, &max_cap0);
    choose_kernels(P, n_sets, sets, max_cap0, force_general);
    ragged_columns(P, n_sets, sets);
    // (linear gaps on the fast loops keep H records -- no direction words -- and take the all-rounds kernel with them)
    P.lin_fast = !P.general && !P.local && !P.extend && sc->gap_mode == ABPOA_HIP_LINEAR_GAP && !P.amb;      // (extension mode: the row order is rebuilt before every read)
    P.rounds_possible = (P.dir || P.lin_fast) && P.max_reads > 2 && !(P.w_max >= P.wide_lo && P.wide_hi >= P.wide_lo) && P.max_extra == 0;
    // Wide-band sets (10 kb reads) keep score records while the record arenas of the whole job fit the device -- their all-chunks row loop is 18-21 % slower
    // with the words, more than the backtrack gains -- and switch to direction words when they do not: an eighth of the bytes per cell, so twice the
    // read-sets are in flight instead of two passes with half the SIMDs idle.  ABPOA_HIP_DIR_WIDE=1 / 0: always / never.
    P.dir_wide = P.dir && opt_int("ABPOA_HIP_DIR_WIDE", 0) > 0;
    P.dir_wide_auto = P.dir && !opt_set("ABPOA_HIP_DIR_WIDE");
    // ... and whenever the pass is large enough for two wavefronts per SIMD (the LDS plan then takes a 4-row ring: eight workgroups per CU): the
    // backtrack over words is 2.5x faster there than over records (configs[3] x 2048: 243 vs 609 ms per step), more than the row loop loses (1910 vs 1670 ms)
    if (P.dir_wide_auto && P.wide_ring_rows <= 4 && P.wide_hi >= P.wide_lo) P.dir_wide = true;
    set_table(P, n_sets, sets);
    P.size_arenas(sets, P.dir_wide);
    return P;
}

int final_lds_plan(const DevicePlan &pl, int n_sets, const abpoa_hip_readset_t *sets, DevBatch &b) {
    const abpoa_hip_scoring_t *sc = &pl.sc;
    int32_t inf_dummy; const int max_bits = abpoa_hip_score_bits(sc, pl.max_node_cap, pl.max_qlen, &inf_dummy); const int pn = max_bits == 16 ? 16 : 8;
    const int64_t width = padded_width(pl.max_qlen, pn);
    // (the rings hold the widest rows expected -- up to 1024 columns: beyond that the plan has no fast row loop at all, and a few ragged sets must not send
    //  the whole job to the host driver; theirs overflow on their own)
    const int64_t est_plain = pl.est_cols(width, pl.w_max, pn), est_ragged = std::min<int64_t>(std::max<int64_t>(est_plain, std::min<int64_t>(1024, width)),
            est_plain + pl.max_extra);
    make_lds_plan(sc, pl.max_qlen, max_bits, est_ragged, n_sets, &b.lds);
    // (a ring that wide does not fit -- int32 scores, convex gaps: the plain estimate then, and the ragged sets' rows that outgrow it are theirs alone)
    if (pl.max_extra > 0 && b.lds.fr_cols == 0) make_lds_plan(sc, pl.max_qlen, max_bits, est_plain, n_sets, &b.lds);
    // (no fast row loop takes anything: routing.h takes_fast / takes_local)
    if (pl.general) { b.lds.wide_on = 0; b.lds.fr_cols = 0; b.lds.loc_cols = 0; }
    // the local row loop: anything it does not take is the general kernel's
    else if (pl.local) {
        b.lds.wide_on = 0;
        if (!local_loop_fits(b.lds, max_bits, pl.max_qlen)) return ABPOA_HIP_EINVAL;
    }
    // score widths the rounds can meet (the width grows with graph and read size): launch only the kernels that can have work
    int min_qlen = pl.max_qlen;
    for (int s = 0; s < n_sets; ++s) for (int r = 1; r < sets[s].n_reads; ++r) min_qlen = std::min(min_qlen, sets[s].lens[r]);
    const int min_bits = abpoa_hip_score_bits(sc, 3, min_qlen, &inf_dummy);
    b.bits_mask = (min_bits == 16 ? 1 : 0) | (max_bits == 32 ? 2 : 0);
    // which row-loop kernels can have work at all: band half-widths of the reads that get aligned (w = b + f * length), as routing.h route_w counts them
    const int w_min = std::min(sc->wb + (int)(sc->wf * (float)min_qlen), pl.max_extra ? pl.weff_lo : INT_MAX), w_top = std::max(pl.w_max, pl.weff_hi);
    const bool mixed = pl.max_extra > 0;      // (sets with and without extra columns: both loops may have work whatever the extremes say)
    if (!mixed && !wide_range_meets(b.lds.wide_w_lo, b.lds.wide_w_hi, w_min, w_top)) b.lds.wide_on = 0;             // no read takes the wide loop
    b.lds.narrow_off = (!mixed && takes_wide_band(b.lds, w_min) && takes_wide_band(b.lds, w_top)) ? 1 : 0;          // every read does (w_min <= w_top)
    return 0;
}

}  // namespace abpoa_hip

// reference src/simd_abpoa_align.c:1672-1683
extern "C" int abpoa_hip_score_bits(const abpoa_hip_scoring_t *sc, int n_rows, int qlen, int32_t *inf_min) {
    int oe1 = sc->gap_open1 + sc->gap_ext1, oe2 = sc->gap_open2 + sc->gap_ext2;
    int len = qlen > n_rows ? qlen : n_rows;
    int max_score = std::max(qlen * sc->max_mat, len * sc->gap_ext1 + sc->gap_open1);
    int bits, lo;
    if (max_score <= INT16_MAX - sc->min_mis - oe1 - oe2) { bits = 16; lo = INT16_MIN; } else { bits = 32; lo = INT32_MIN; }
    if (inf_min) *inf_min = std::max(std::max(lo + sc->min_mis, lo + oe1), lo + oe2) + 31 * std::max(sc->gap_ext1, sc->gap_ext2);
    return bits;
}
