// Byte arithmetic of the device-resident read-set driver: see msa_device_layout.h
#include <algorithm>
#include <stdlib.h>
#include <string.h>
#include "engine_options.h"
#include "msa_device_layout.h"
#include "poa_graph.h"
#include "routing.h"

namespace abpoa_hip {

Layout lay_out_device(const DevicePlan &pl, int n_sets, bool any_w) {
    const abpoa_hip_scoring_t *sc = &pl.sc; const bool gen_io = pl.gen_io();
    Layout L; int blob = BLOB_IN; size_t o = 0;
    auto take = [&](const char *name, size_t bytes) { size_t at = o; o = align_up(o + bytes); L.table.push_back({blob, name, at, bytes}); return at; };
#define TAKE(field, bytes) L.field = take(#field, (bytes))
    // (o_rargs, o_msaoff_h: host-side staging only)
    TAKE(o_sets, sizeof(PoaSet) * n_sets); TAKE(o_roff, 8 * (pl.tot_reads + 1)); TAKE(o_rlen, 4 * (pl.tot_reads + 1)); TAKE(o_mat, 4 * sc->m * sc->m);
    TAKE(o_rargs, poa_rounds_args_bytes()); TAKE(o_msaoff_h, pl.want_msa ? 8 * (size_t)n_sets : 0);
    TAKE(o_gfaoff_h, pl.want_gfa ? 32 * (size_t)n_sets : 0);
    TAKE(o_wts, any_w ? 4 * (size_t)(pl.tot_bases + 64) : 0);      // (per-base weights, -Q: in front of the reads, so that they go up with the first part)
    TAKE(o_reads, pl.tot_bases + 64); L.in_bytes = o;      // reads last: they go up in two parts
    // -s: reverse complements / reversed weights of the reads under retry
    TAKE(o_rc, pl.amb ? pl.tot_bases + 64 : 0); TAKE(o_wrc, pl.amb && any_w ? 4 * (size_t)(pl.tot_bases + 64) : 0); L.in_dev_bytes = o;
    blob = BLOB_GRAPH; o = 0;
    TAKE(o_state, sizeof(PoaState) * n_sets);
    // downloaded part first, contiguous: per-set state and the consensus results
    TAKE(o_cnode, 4 * pl.cons_tot); TAKE(o_ccov, 4 * pl.cons_tot); TAKE(o_cbase, pl.cons_tot); TAKE(o_isrc, pl.amb ? (size_t)pl.tot_reads : 0);
    TAKE(o_gcnt, pl.want_gfa ? 12 * (size_t)n_sets : 0);
    L.dl_bytes = o;
    TAKE(o_order0, 4 * pl.node_tot); TAKE(o_order1, 4 * pl.node_tot); TAKE(o_base, pl.node_tot); TAKE(o_nout, pl.node_tot);
    TAKE(o_out, 4 * pl.node_tot * POA_HOT); TAKE(o_outw, 4 * pl.node_tot * POA_HOT); TAKE(o_nread, 4 * pl.node_tot);
    TAKE(o_outx, 4 * pl.node_tot * (size_t)(pl.out_cap - POA_HOT)); TAKE(o_outwx, 4 * pl.node_tot * (size_t)(pl.out_cap - POA_HOT));
    TAKE(o_inx, 4 * pl.node_tot * (size_t)(pl.in_cap - POA_HOT));
    TAKE(o_nin, pl.node_tot); TAKE(o_naln, pl.node_tot); TAKE(o_in, 4 * pl.node_tot * POA_HOT); TAKE(o_aln, 4 * pl.node_tot * (size_t)pl.aln_cap);
    TAKE(o_row, 4 * pl.node_tot);
    TAKE(o_rid, 8 * pl.node_tot * (size_t)pl.out_cap * (size_t)pl.rid_words); TAKE(o_mrank, pl.want_msa ? 4 * pl.node_tot : 0);
    TAKE(o_msaoff, pl.want_msa ? 8 * (size_t)n_sets : 0);
    TAKE(o_gwalk, pl.want_gfa ? 4 * pl.node_tot : 0); TAKE(o_gorw, pl.want_gfa ? 8 * pl.node_tot * (size_t)pl.rid_words : 0); TAKE(o_goff, pl.want_gfa ? 32 * (size_t)n_sets : 0);
    TAKE(o_tout, 4 * pl.term_tot); TAKE(o_toutw, 4 * pl.term_tot); TAKE(o_tin, 4 * pl.term_tot);
    L.graph_bytes = o;
    blob = BLOB_ROWS; o = 0;
    TAKE(o_ticket, 4 * POA_CU_TICKETS);
    TAKE(o_aln_desc, sizeof(AlnDesc) * n_sets); TAKE(o_out_rec, sizeof(AlnOut) * n_sets);
    TAKE(o_rbase, pl.node_tot); TAKE(o_rsd, pl.node_tot); TAKE(o_rpd, 8 * pl.node_tot); TAKE(o_rnid, 4 * pl.node_tot); TAKE(o_rrem, 4 * pl.node_tot);
    TAKE(o_poff, 4 * pl.node_tot); TAKE(o_pred, 4 * (pl.pred_tot + 1));
    TAKE(o_bsn, 4 * pl.node_tot); TAKE(o_esn, 4 * pl.node_tot); TAKE(o_coff, 8 * pl.node_tot); TAKE(o_rmi, 4 * pl.node_tot);
    TAKE(o_cigar, 8 * pl.cig_tot); TAKE(o_scratch, 4 * pl.scr_tot);
    // general kernel (rows_general.h): successor CSR, band state per row, the "row is part of the alignment" bytes (all ones: no sub-graph alignments here)
    TAKE(o_ooff, gen_io ? 4 * pl.node_tot : 0); TAKE(o_orow, gen_io ? 4 * (pl.pred_tot + 1) : 0); TAKE(o_left, gen_io ? 4 * pl.node_tot : 0);
    TAKE(o_right, gen_io ? 4 * pl.node_tot : 0); TAKE(o_act, gen_io ? pl.node_tot : 0);
    TAKE(o_outfwd, pl.amb ? sizeof(AlnOut) * n_sets : 0); TAKE(o_cigfwd, pl.amb ? 8 * pl.cig_tot : 0); TAKE(o_retry, pl.amb ? (size_t)n_sets : 0);
    L.rows_bytes = o;
#undef TAKE
    return L;
}

int64_t fill_read_tables(const DevicePlan &pl, int n_sets, const abpoa_hip_readset_t *sets, int64_t *roff, int32_t *rlen) {
    int64_t at = 0, split_at = 0;
    for (int k = 0; k < pl.max_reads; ++k) {
        if (k == 2) split_at = at;
        for (int s = 0; s < n_sets; ++s) if (k < sets[s].n_reads) { const int64_t ri = pl.ps[s].read0 + k; roff[ri] = at; rlen[ri] = sets[s].lens[k]; at += sets[s].lens[k]; }
    }
    if (pl.max_reads <= 2) split_at = at;
    roff[pl.tot_reads] = at;
    return split_at;
}

namespace {
// LDS tables of the graph walks -- the order / rank kernels (two ints per node; the rank pass packs four tables into the same space: 52 KB, three workgroups
// per CU) and the GFA walk (counters and queue, 48 KB) --: graphs of up to 6000 nodes, larger ones keep the tables in memory.  nodes: that capacity for the
// job's largest set; capped: under ABPOA_HIP_ORDER_CAP (tests: graphs above this many nodes take the walks with tables in memory); on: ABPOA_HIP_ORDER_LDS
// (0: the general walk everywhere)
struct WalkLds { int nodes, capped; bool on; };
WalkLds walk_lds(int max_node_cap) {
    WalkLds w; w.nodes = std::min(((max_node_cap + 3) & ~3), 6000); w.capped = w.nodes; w.on = opt_int("ABPOA_HIP_ORDER_LDS", 1) != 0;
    const int cap_ = opt_int("ABPOA_HIP_ORDER_CAP", -1); if (cap_ >= 0) w.capped = std::min(w.capped, cap_ & ~3);
    return w;
}
}  // namespace

void bind_poa_dev(PoaDev &p, GfaDev &g, const DevicePlan &pl, const Layout &L, int n_sets, bool any_w, bool dig_on, uint8_t *di, uint8_t *dg, uint8_t *dr) {
    const abpoa_hip_scoring_t *sc = &pl.sc; const bool gen_io = pl.gen_io();
    memset(&p, 0, sizeof(p));
    p.n_sets = n_sets; p.m = sc->m; p.max_mat = sc->max_mat; p.min_mis = sc->min_mis; p.o1 = sc->gap_open1; p.e1 = sc->gap_ext1; p.o2 = sc->gap_open2;
    p.e2 = sc->gap_ext2;
    p.wb = sc->wb; p.wf = sc->wf; p.gap_mode = sc->gap_mode; p.max_qlen = pl.max_qlen;
    p.last_pass = pl.node_factor >= 6.0 ? 1 : 0;      // (msa_passes.cpp run_pass_ladder: 3x, 4.5x, 6x, 4096x; the 6x pass and the last)
    p.in_cap = pl.in_cap; p.out_cap = pl.out_cap;
    p.dig_on = dig_on ? 1 : 0;      // (tests: the fuse phase folds every graph cigar into PoaState.cigar_dig)
    // (the reference's own row order where the best cell is the FIRST row that reaches the maximum: local and extension mode, ref :1012-1026; the remaining
    //  length where something reads it: the adaptive band and the z-drop test)
    p.aln_cap = pl.aln_cap; p.rid_words = pl.rid_words; p.order_mode = (pl.local || pl.extend) ? 1 : 0; p.banded = (sc->wb >= 0 || sc->zdrop > 0) ? 1 : 0;
    p.general = pl.general ? 1 : 0; p.msa_rows = 0; p.msa_cons = (pl.want_msa && pl.want_cons) ? 1 : 0;
    const WalkLds w = walk_lds(pl.max_node_cap);
    p.order_lds = (p.order_mode || pl.want_msa) ? w.capped : 0;
    // (the all-in-LDS order walk: what is left of 40 KB -- four workgroups per CU -- after 13 bytes a node goes to aligned-list entries, 2 bytes each)
    p.order_ecap = p.order_mode && w.on ? std::max(1024, std::min(65535, (40 * 1024 - 128 - 13 * w.nodes) / 2)) : 0;
    // per-row records of the prepare kernel in LDS (5 bytes a row, 40 KB at most: four workgroups per CU still fit)
    p.lds_rows = pl.max_node_cap <= 8000 ? ((pl.max_node_cap + 3) & ~3) : 0;
    p.sets = (const PoaSet *)(di + L.o_sets); p.state = (PoaState *)(dg + L.o_state);
    p.read_off = (const int64_t *)(di + L.o_roff); p.read_len = (const int32_t *)(di + L.o_rlen); p.reads = di + L.o_reads;
    p.wts = any_w ? (const int32_t *)(di + L.o_wts) : nullptr;
    p.nd_base = dg + L.o_base; p.nd_nin = dg + L.o_nin; p.nd_nout = dg + L.o_nout; p.nd_naln = dg + L.o_naln;
    p.nd_in = (int32_t *)(dg + L.o_in); p.nd_out = (int32_t *)(dg + L.o_out); p.nd_outw = (int32_t *)(dg + L.o_outw); p.nd_aln = (int32_t *)(dg + L.o_aln);
    p.nd_inx = (int32_t *)(dg + L.o_inx); p.nd_outx = (int32_t *)(dg + L.o_outx); p.nd_outwx = (int32_t *)(dg + L.o_outwx);
    p.nd_nread = (int32_t *)(dg + L.o_nread); p.nd_row = (int32_t *)(dg + L.o_row);
    p.t_out = (int32_t *)(dg + L.o_tout); p.t_outw = (int32_t *)(dg + L.o_toutw); p.t_in = (int32_t *)(dg + L.o_tin);
    p.nd_rid = (uint64_t *)(dg + L.o_rid); p.msa_rank = (int32_t *)(dg + L.o_mrank); p.msa_off = (const int64_t *)(dg + L.o_msaoff); p.msa_out = nullptr;
    p.row_node[0] = (int32_t *)(dg + L.o_order0); p.row_node[1] = (int32_t *)(dg + L.o_order1);
    p.scratch = (int32_t *)(dr + L.o_scratch);
    p.aln = (AlnDesc *)(dr + L.o_aln_desc); p.out = (AlnOut *)(dr + L.o_out_rec);
    p.row_base = dr + L.o_rbase; p.row_sdist = dr + L.o_rsd; p.row_pd = (uint32_t *)(dr + L.o_rpd); p.row_node_id = (int32_t *)(dr + L.o_rnid);
    p.row_remain = (int32_t *)(dr + L.o_rrem);
    p.pred_off = (int32_t *)(dr + L.o_poff); p.pred_row = (int32_t *)(dr + L.o_pred); p.cigar = (uint64_t *)(dr + L.o_cigar);
    p.out_off = gen_io ? (int32_t *)(dr + L.o_ooff) : nullptr; p.out_row = gen_io ? (int32_t *)(dr + L.o_orow) : nullptr;
    if (pl.amb) {
        p.reads_rc = di + L.o_rc; p.wts_rc = any_w ? (int32_t *)(di + L.o_wrc) : nullptr; p.is_rc = dg + L.o_isrc; p.retry = dr + L.o_retry;
        p.out_fwd = (AlnOut *)(dr + L.o_outfwd); p.cigar_fwd = (uint64_t *)(dr + L.o_cigfwd);
    }
    p.cons_node = (int32_t *)(dg + L.o_cnode); p.cons_cov = (int32_t *)(dg + L.o_ccov); p.cons_base = dg + L.o_cbase;
    // GFA output: the result pools are laid out once the walk has counted (lay_out_gfa, bind_gfa_pools)
    memset(&g, 0, sizeof(g));
    if (pl.want_gfa) {
        g.lds_cap = w.on ? w.capped : 0;
        g.walk = (int32_t *)(dg + L.o_gwalk); g.cnt = (int32_t *)(dg + L.o_gcnt); g.orw = (uint64_t *)(dg + L.o_gorw); g.off = (const int64_t *)(dg + L.o_goff);
    }
}

void bind_dev_batch(DevBatch &b, DevBatch &b_rc, const DevicePlan &pl, const Layout &L, const PoaDev &p, uint8_t *di, uint8_t *dr, uint8_t *planes) {
    const abpoa_hip_scoring_t *sc = &pl.sc;
    set_job_fields(b, *sc); b.ret_cigar = 1; b.rev_cigar = 0;
    b.want_trace = 0; b.fresh_band = 1; b.want_lr = 0;
    b.dbg = opt_int("ABPOA_HIP_DBG", 0);      // (diag.h)
    b.mat = (const int32_t *)(di + L.o_mat); b.aln = p.aln; b.out = p.out;
    b.dir_mode = pl.dir ? (pl.dir_wide ? 2 : 1) : 0; b.row_sdist = p.row_sdist; b.row_pd = p.row_pd;
    b.query = p.reads; b.row_base = p.row_base; b.row_node_id = p.row_node_id; b.row_remain = p.row_remain; b.row_active = p.row_base;
    b.pred_off = p.pred_off; b.pred_row = p.pred_row; b.out_off = p.pred_off; b.out_row = p.pred_row;
    b.left = p.scratch; b.right = p.scratch;
    if (pl.gen_io()) {
        b.out_off = p.out_off; b.out_row = p.out_row; b.left = (int32_t *)(dr + L.o_left); b.right = (int32_t *)(dr + L.o_right); b.row_active = dr + L.o_act;
    }
    b.dp_beg_sn = (int32_t *)(dr + L.o_bsn); b.dp_end_sn = (int32_t *)(dr + L.o_esn); b.row_cell_off = (int64_t *)(dr + L.o_coff);
    b.row_max_i = (int32_t *)(dr + L.o_rmi);
    b.planes = planes; b.cigar = p.cigar;
    // -s: the forward run leaves max_pos_left/right behind (fast row loops: a post-pass, rows_fast.h; general kernel: its own arrays) and the retry starts
    // from them -- the reference sorts, and so resets them, only before the forward alignment (src/abpoa_align.c:329 calls the DP directly)
    b_rc = b;
    if (pl.amb) {
        b.want_lr = (sc->wb >= 0 && !pl.general) ? 1 : 0;
        b_rc = b; b_rc.want_lr = 0; b_rc.fresh_band = sc->wb >= 0 ? 0 : 1;
    }
}

// (reference abpoa_generate_rc_msa, src/abpoa_output.c:123-166: the rank pass left the column count of every set in its state)
MsaLayout lay_out_msa(const DevicePlan &pl, int n_sets, const abpoa_hip_readset_t *sets, const PoaState *hs) {
    MsaLayout M; M.off.resize(n_sets); M.total = 0;
    for (int s = 0; s < n_sets; ++s) { M.off[s] = M.total; if (hs[s].status == POA_ST_OK && hs[s].n_nodes > 2) M.total += (int64_t)(sets[s].n_reads
            + (pl.want_cons ? 1 : 0)) * std::max(0, hs[s].msa_len); }
    return M;
}

// (reference abpoa_generate_gfa, src/abpoa_output.c:168-268: a path has room for the bases of its set's reads, the fill kernel counts what it writes)
GfaLayout lay_out_gfa(const DevicePlan &pl, int n_sets, const abpoa_hip_readset_t *sets, const PoaState *hs, const int32_t *cnt) {
    GfaLayout G;
    G.off.assign(4 * (size_t)n_sets, 0);
    for (int s = 0; s < n_sets; ++s) {
        int64_t *o4 = G.off.data() + 4 * (size_t)s; o4[0] = G.seg_tot; o4[1] = G.link_tot; o4[2] = G.path_tot; o4[3] = 0;
        if (hs[s].status != POA_ST_OK || hs[s].n_nodes <= 2 || cnt[3 * s] <= 0) continue;
        for (int r = 0; r < sets[s].n_reads; ++r) o4[3] += sets[s].lens[r];
        G.seg_tot += cnt[3 * s]; G.link_tot += cnt[3 * s + 1]; G.path_tot += o4[3];
    }
    if (G.seg_tot <= 0) return G;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o = align_up(o + bytes); return at; };
    G.o_seg = take(4 * (size_t)G.seg_tot); G.o_loff = take(4 * (size_t)(G.seg_tot + n_sets)); G.o_lfrom = take(4 * (size_t)G.link_tot);
    G.o_poff = take(8 * (size_t)(pl.tot_reads + n_sets)); G.o_pnode = take(4 * (size_t)G.path_tot); G.o_base = take((size_t)G.seg_tot);
    G.o_cnt = take(12 * (size_t)n_sets); G.bytes = o;
    return G;
}

void bind_gfa_pools(GfaDev &g, const GfaLayout &G, uint8_t *dq) {
    g.seg_node = (int32_t *)(dq + G.o_seg); g.link_off = (int32_t *)(dq + G.o_loff); g.link_from = (int32_t *)(dq + G.o_lfrom);
    g.path_off = (int64_t *)(dq + G.o_poff); g.path_node = (int32_t *)(dq + G.o_pnode); g.seg_base = dq + G.o_base;
}

bool unpack_set(const DevicePlan &pl, const Layout &L, const MsaLayout &M, const GfaLayout &G, const abpoa_hip_readset_t &set, int s, const uint8_t *hg,
                const uint8_t *h_msa, const uint8_t *h_gfa, abpoa_hip_msa_t *o) {
    const PoaState &st = ((const PoaState *)(hg + L.o_state))[s]; const int nr = set.n_reads;
    memset(o, 0, sizeof(*o)); o->n_reads = nr;
    if (st.status != POA_ST_OK) return true;
    // (GFA output: the fill kernel's links or paths did not fit what the walk counted / the reads' bases: the set is redone like one whose walk failed)
    if (pl.want_gfa && G.bytes && ((const int32_t *)(h_gfa + G.o_cnt))[3 * s + 2] != 0) return true;
    // (only for a set that finished here: the record of a set that goes to another pass or to the host driver is overwritten there)
    if (pl.amb) { o->is_rc = (uint8_t *)calloc((size_t)std::max(1, nr), 1); if (o->is_rc) memcpy(o->is_rc, hg + L.o_isrc + pl.ps[s].read0, (size_t)nr); }
    o->n_cells = st.n_cells;
    if (pl.want_cons && st.n_nodes > 2) {
        const int len = st.cons_len; const int64_t c0 = pl.ps[s].cons0;
        o->cons_len = len;
        o->cons_base = (uint8_t *)malloc(len + 1); o->cons_cov = (int32_t *)malloc(4 * (len + 1)); o->cons_node_id = (int32_t *)malloc(4 * (len + 1));
        memcpy(o->cons_base, hg + L.o_cbase + c0, len); memcpy(o->cons_cov, (const int32_t *)(hg + L.o_ccov) + c0, 4 * (size_t)len);
        memcpy(o->cons_node_id, (const int32_t *)(hg + L.o_cnode) + c0, 4 * (size_t)len);
    }
    if (pl.want_gfa) {      // (an empty graph: a record with n_seg = 0, as the host driver leaves it)
        const int32_t *hc = (const int32_t *)(hg + L.o_gcnt);
        const bool any = st.n_nodes > 2 && G.bytes && hc[3 * s] > 0;
        const int n_seg = any ? hc[3 * s] : 0, n_link = any ? hc[3 * s + 1] : 0;
        const int64_t *o4 = G.off.data() + 4 * (size_t)s;
        const int64_t *poff = any ? (const int64_t *)(h_gfa + G.o_poff) + pl.ps[s].read0 + s : nullptr;
        const int64_t n_pn = any ? std::min<int64_t>(std::max<int64_t>(0, poff[nr]), o4[3]) : 0;
        o->gfa = gfa_alloc(n_seg, n_link, nr, n_pn);
        if (o->gfa && any) {
            memcpy(o->gfa->seg_node, (const int32_t *)(h_gfa + G.o_seg) + o4[0], 4 * (size_t)n_seg); memcpy(o->gfa->seg_base, h_gfa + G.o_base + o4[0], (size_t)n_seg);
            memcpy(o->gfa->link_off, (const int32_t *)(h_gfa + G.o_loff) + o4[0] + s, 4 * ((size_t)n_seg + 1));
            memcpy(o->gfa->link_from, (const int32_t *)(h_gfa + G.o_lfrom) + o4[1], 4 * (size_t)n_link);
            memcpy(o->gfa->path_off, poff, 8 * ((size_t)nr + 1)); memcpy(o->gfa->path_node, (const int32_t *)(h_gfa + G.o_pnode) + o4[2], 4 * (size_t)n_pn);
        }
        if (!o->gfa) o->status = ABPOA_HIP_ENOMEM;
    }
    if (pl.want_msa && st.n_nodes > 2) {      // (an empty graph has no MSA: the host driver leaves the record zeroed too)
        const int len = std::max(0, st.msa_len);
        o->msa_len = len; o->msa_rows = nr + (pl.want_cons ? 1 : 0);
        o->msa_base = (uint8_t *)malloc((size_t)o->msa_rows * (len > 0 ? len : 1));
        if (len > 0) memcpy(o->msa_base, h_msa + M.off[s], (size_t)o->msa_rows * len);
    }
    return false;
}

}  // namespace abpoa_hip
