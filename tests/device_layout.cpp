// CPU harness of tests/test_device_layout.py: the byte arithmetic of the device-resident driver (abpoa_amd/csrc/msa_device_layout.cpp) on plans of small
// synthetic read-sets -- the blob layout, the read tables, the kernel-argument bindings, the MSA / GFA result layouts, the unpacking of results and the event
// slots.  No GPU, no HIP runtime call; built with -fsanitize=undefined,address, and every "device" or "downloaded" buffer is a malloc of exactly the bytes
// the layout names, so that an index past a pool's end is the sanitizer's to report.  What a pool must hold is restated here from the plan totals and the
// kernels' indexing (poa_device.h), not taken from the layout.  lds_fixed_bytes_* and poa_rounds_args_bytes are stand-ins for the kernels' own.
#include <algorithm>
#include <map>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "engine_options.h"
#include "msa_device_layout.h"
#include "poa_graph.h"

// (the snapshot a set_option replaces is left alone on purpose -- engine_options.h -- so the leak check would report every switch this harness flips)
extern "C" const char *__asan_default_options() { return "detect_leaks=0"; }

namespace abpoa_hip {
int lds_fixed_bytes_dp() { return 1024; }
int lds_fixed_bytes_bt() { return 2048; }
size_t poa_rounds_args_bytes() { return 1000; }
}  // namespace abpoa_hip
using namespace abpoa_hip;

static int g_fail = 0, g_jobs = 0;
static std::string g_case;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "FAILED %s:%d [%s] %s\n", __FILE__, __LINE__, g_case.c_str(), #cond); g_fail++; } } while (0)

struct Sets {      // read-sets by lengths (the layout never looks at a base); w_set >= 0: that set alone has per-base weights, on its first read only
    std::vector<std::vector<int32_t>> lens; int w_set = -1;
    std::vector<abpoa_hip_readset_t> rs; std::vector<int32_t> w; std::vector<const int32_t *> wp;
    const abpoa_hip_readset_t *get() {
        rs.resize(lens.size());
        for (size_t s = 0; s < lens.size(); ++s) { rs[s].n_reads = (int)lens[s].size(); rs[s].seqs = nullptr; rs[s].lens = lens[s].data(); rs[s].weights = nullptr; }
        if (w_set >= 0) { w.assign((size_t)lens[w_set][0], 3); wp.assign(lens[w_set].size(), nullptr); wp[0] = w.data(); rs[w_set].weights = wp.data(); }
        return rs.data();
    }
    int n() const { return (int)lens.size(); }
};

static std::vector<int32_t> g_mat;
static abpoa_hip_scoring_t scoring(int gap_mode, int align_mode) {      // the reference's defaults: 2 / -4, 4 + 2 k, -b 10 -f 0.01
    abpoa_hip_scoring_t sc; const int m = 5;
    g_mat.assign((size_t)m * m, -4); for (int i = 0; i < m; ++i) g_mat[(size_t)i * m + i] = 2;
    sc.m = m; sc.mat = g_mat.data(); sc.max_mat = 2; sc.min_mis = 4;
    sc.gap_open1 = gap_mode == ABPOA_HIP_LINEAR_GAP ? 0 : 4; sc.gap_ext1 = 2; sc.gap_open2 = 0; sc.gap_ext2 = 0;
    sc.align_mode = align_mode; sc.gap_mode = gap_mode; sc.wb = 10; sc.wf = 0.01f; sc.zdrop = 0; sc.ret_cigar = 1; sc.rev_cigar = 0;
    return sc;
}

static const LayoutEntry &entry(const Layout &L, const char *name) {
    for (const LayoutEntry &e : L.table) if (!strcmp(e.name, name)) return e;
    fprintf(stderr, "no layout entry %s\n", name); exit(2);
}
static size_t blob_bytes(const Layout &L, int blob) { return blob == BLOB_IN ? L.in_dev_bytes : blob == BLOB_GRAPH ? L.graph_bytes : L.rows_bytes; }

// ---- the layout table
static void layout_checks(const DevicePlan &P, const Layout &L, int n_sets, bool any_w) {
    const bool gen_io = P.general || P.amb;
    CHECK(L.in_bytes <= L.in_dev_bytes && L.dl_bytes <= L.graph_bytes);
    for (size_t i = 0; i < L.table.size(); ++i) {
        const LayoutEntry &a = L.table[i];
        CHECK(a.off % 256 == 0 && a.off + a.bytes <= blob_bytes(L, a.blob));
        for (size_t j = 0; j < i; ++j) { const LayoutEntry &b = L.table[j];
            if (a.blob == b.blob) CHECK((a.off + a.bytes <= b.off || b.off + b.bytes <= a.off) && (a.off != b.off || !a.bytes || !b.bytes) && strcmp(a.name, b.name)); }
        // the uploaded part of the in blob: everything but the -s pools; the downloaded head of the graph blob: state, consensus pools, is_rc, GFA counts
        const bool late = !strcmp(a.name, "o_rc") || !strcmp(a.name, "o_wrc");
        if (a.blob == BLOB_IN) CHECK(late ? a.off >= L.in_bytes : a.off + a.bytes <= L.in_bytes);
        bool head = false; for (const char *h : {"o_state", "o_cnode", "o_ccov", "o_cbase", "o_isrc", "o_gcnt"}) head |= !strcmp(a.name, h);
        if (a.blob == BLOB_GRAPH) CHECK(head ? a.off + a.bytes <= L.dl_bytes : a.off >= L.dl_bytes);
    }
    // what the consumers index (poa_device.h, engine.h DevBatch), from the plan totals; 0: the job has no such pool
    const size_t N = (size_t)P.node_tot, S = (size_t)n_sets, R = (size_t)P.tot_reads, B = (size_t)P.tot_bases, W = (size_t)P.rid_words, PT = (size_t)P.pred_tot + 1;
    const std::map<std::string, size_t> need = {
        {"o_sets", sizeof(PoaSet) * S}, {"o_roff", 8 * (R + 1)}, {"o_rlen", 4 * R}, {"o_mat", 4 * (size_t)P.sc.m * P.sc.m}, {"o_rargs", poa_rounds_args_bytes()},
        {"o_msaoff_h", P.want_msa ? 8 * S : 0}, {"o_gfaoff_h", P.want_gfa ? 32 * S : 0}, {"o_wts", any_w ? 4 * B : 0}, {"o_reads", B},
        {"o_rc", P.amb ? B : 0}, {"o_wrc", P.amb && any_w ? 4 * B : 0},
        {"o_state", sizeof(PoaState) * S}, {"o_cnode", 4 * (size_t)P.cons_tot}, {"o_ccov", 4 * (size_t)P.cons_tot}, {"o_cbase", (size_t)P.cons_tot},
        {"o_isrc", P.amb ? R : 0}, {"o_gcnt", P.want_gfa ? 12 * S : 0},
        {"o_order0", 4 * N}, {"o_order1", 4 * N}, {"o_base", N}, {"o_nin", N}, {"o_nout", N}, {"o_naln", N}, {"o_nread", 4 * N}, {"o_row", 4 * N},
        {"o_in", 4 * N * POA_HOT}, {"o_out", 4 * N * POA_HOT}, {"o_outw", 4 * N * POA_HOT},
        {"o_inx", 4 * N * (size_t)(P.in_cap - POA_HOT)}, {"o_outx", 4 * N * (size_t)(P.out_cap - POA_HOT)}, {"o_outwx", 4 * N * (size_t)(P.out_cap - POA_HOT)},
        {"o_aln", 4 * N * (size_t)P.aln_cap}, {"o_rid", 8 * N * (size_t)P.out_cap * W}, {"o_mrank", P.want_msa ? 4 * N : 0}, {"o_msaoff", P.want_msa ? 8 * S : 0},
        {"o_gwalk", P.want_gfa ? 4 * N : 0}, {"o_gorw", P.want_gfa ? 8 * N * W : 0}, {"o_goff", P.want_gfa ? 32 * S : 0},
        {"o_tout", 4 * (size_t)P.term_tot}, {"o_toutw", 4 * (size_t)P.term_tot}, {"o_tin", 4 * (size_t)P.term_tot},
        {"o_ticket", 4 * (size_t)POA_CU_TICKETS}, {"o_aln_desc", sizeof(AlnDesc) * S}, {"o_out_rec", sizeof(AlnOut) * S},
        {"o_rbase", N}, {"o_rsd", N}, {"o_rpd", 8 * N}, {"o_rnid", 4 * N}, {"o_rrem", 4 * N}, {"o_poff", 4 * N}, {"o_pred", 4 * PT},
        {"o_bsn", 4 * N}, {"o_esn", 4 * N}, {"o_coff", 8 * N}, {"o_rmi", 4 * N}, {"o_cigar", 8 * (size_t)P.cig_tot}, {"o_scratch", 4 * (size_t)P.scr_tot},
        {"o_ooff", gen_io ? 4 * N : 0}, {"o_orow", gen_io ? 4 * PT : 0}, {"o_left", gen_io ? 4 * N : 0}, {"o_right", gen_io ? 4 * N : 0}, {"o_act", gen_io ? N : 0},
        {"o_outfwd", P.amb ? sizeof(AlnOut) * S : 0}, {"o_cigfwd", P.amb ? 8 * (size_t)P.cig_tot : 0}, {"o_retry", P.amb ? S : 0},
    };
    CHECK(need.size() == L.table.size());
    for (const LayoutEntry &e : L.table) {
        const auto it = need.find(e.name);
        CHECK(it != need.end());
        if (it != need.end()) CHECK(it->second ? e.bytes >= it->second : e.bytes == 0);
    }
    CHECK(P.rid_words > 0 || !(P.want_msa || P.want_gfa));
    CHECK(P.roomy ? P.in_cap >= POA_HOT && P.out_cap >= POA_HOT : P.in_cap == POA_IN_CAP && P.out_cap == POA_OUT_CAP);
}

// ---- the read tables
static void read_table_checks(const DevicePlan &P, Sets &S) {
    std::vector<int64_t> roff((size_t)P.tot_reads + 1, -1); std::vector<int32_t> rlen((size_t)P.tot_reads + 1, -1);
    const int64_t split = fill_read_tables(P, S.n(), S.get(), roff.data(), rlen.data());
    int64_t at = 0, first_r2 = -1; int max_reads = 0;
    for (auto &l : S.lens) max_reads = std::max(max_reads, (int)l.size());
    for (int k = 0; k < max_reads; ++k) for (int s = 0; s < S.n(); ++s) if (k < (int)S.lens[s].size()) {      // round-major: read k of every set before read k + 1
        const int64_t ri = P.ps[s].read0 + k;
        CHECK(roff[ri] == at && rlen[ri] == S.lens[s][k]);
        if (k == 2 && first_r2 < 0) first_r2 = at;
        at += S.lens[s][k];
    }
    CHECK(roff[P.tot_reads] == at && at == P.tot_bases);
    CHECK(split == (first_r2 >= 0 ? first_r2 : at));
    if (max_reads <= 2) CHECK(split == at);
    std::vector<uint8_t> hit((size_t)at, 0);      // every base of the pool belongs to exactly one read
    for (int64_t r = 0; r < P.tot_reads; ++r) for (int64_t j = roff[r]; j < roff[r] + rlen[r]; ++j) { CHECK(j >= 0 && j < at && !hit[j]); if (j >= 0 && j < at) hit[j] = 1; }
}

// ---- the bindings: three blobs of exactly the layout's bytes
struct Blobs {
    uint8_t *d[3], *planes;
    Blobs(const Layout &L) { for (int i = 0; i < 3; ++i) d[i] = (uint8_t *)malloc(std::max<size_t>(1, blob_bytes(L, i))); planes = (uint8_t *)malloc(16); }
    ~Blobs() { for (uint8_t *x : d) free(x); free(planes); }
};
static void at_entry(const Layout &L, const Blobs &D, const void *ptr, int blob, const char *name, bool wanted) {
    if (!wanted) { CHECK(ptr == nullptr); return; }
    const LayoutEntry &e = entry(L, name);
    CHECK(e.blob == blob && ptr == D.d[blob] + e.off && e.off + e.bytes <= blob_bytes(L, blob));
}
// the parent's two copies of the LDS-capacity rule, as they stood in fill_poa_dev
static void parent_caps(const DevicePlan &P, int *order_lds, int *order_ecap, int *gfa_lds) {
    const int order_mode = (P.local || P.extend) ? 1 : 0;
    *order_lds = (order_mode || P.want_msa) ? std::min(((P.max_node_cap + 3) & ~3), 6000) : 0;
    *order_ecap = order_mode ? std::max(1024, std::min(65535, (40 * 1024 - 128 - 13 * *order_lds) / 2)) : 0;
    if (!opt_int("ABPOA_HIP_ORDER_LDS", 1)) *order_ecap = 0;
    { const int cap_ = opt_int("ABPOA_HIP_ORDER_CAP", -1); if (cap_ >= 0) *order_lds = std::min(*order_lds, cap_ & ~3); }
    *gfa_lds = 0;
    if (P.want_gfa) {
        *gfa_lds = opt_int("ABPOA_HIP_ORDER_LDS", 1) ? std::min(((P.max_node_cap + 3) & ~3), 6000) : 0;
        { const int cap_ = opt_int("ABPOA_HIP_ORDER_CAP", -1); if (cap_ >= 0) *gfa_lds = std::min(*gfa_lds, cap_ & ~3); }
    }
}
static void binding_checks(const DevicePlan &P, const Layout &L, int n_sets, bool any_w) {
    const Blobs D(L); const bool gen_io = P.general || P.amb;
    PoaDev p; GfaDev g; DevBatch b, b_rc;
    bind_poa_dev(p, g, P, L, n_sets, any_w, true, D.d[BLOB_IN], D.d[BLOB_GRAPH], D.d[BLOB_ROWS]);
    memset(&b, 0, sizeof(b)); b.n = n_sets; b.m = P.sc.m;
    bind_dev_batch(b, b_rc, P, L, p, D.d[BLOB_IN], D.d[BLOB_ROWS], D.planes);
#define AT(ptr, blob, name, wanted) at_entry(L, D, ptr, blob, name, wanted)
    AT(p.sets, BLOB_IN, "o_sets", true); AT(p.read_off, BLOB_IN, "o_roff", true); AT(p.read_len, BLOB_IN, "o_rlen", true); AT(p.reads, BLOB_IN, "o_reads", true);
    AT(p.wts, BLOB_IN, "o_wts", any_w); AT(p.reads_rc, BLOB_IN, "o_rc", P.amb); AT(p.wts_rc, BLOB_IN, "o_wrc", P.amb && any_w); AT(b.mat, BLOB_IN, "o_mat", true);
    AT(p.state, BLOB_GRAPH, "o_state", true); AT(p.nd_base, BLOB_GRAPH, "o_base", true); AT(p.nd_nin, BLOB_GRAPH, "o_nin", true); AT(p.nd_nout, BLOB_GRAPH, "o_nout", true);
    AT(p.nd_naln, BLOB_GRAPH, "o_naln", true); AT(p.nd_in, BLOB_GRAPH, "o_in", true); AT(p.nd_out, BLOB_GRAPH, "o_out", true); AT(p.nd_outw, BLOB_GRAPH, "o_outw", true);
    AT(p.nd_inx, BLOB_GRAPH, "o_inx", true); AT(p.nd_outx, BLOB_GRAPH, "o_outx", true); AT(p.nd_outwx, BLOB_GRAPH, "o_outwx", true); AT(p.nd_aln, BLOB_GRAPH, "o_aln", true);
    AT(p.nd_nread, BLOB_GRAPH, "o_nread", true); AT(p.nd_row, BLOB_GRAPH, "o_row", true); AT(p.t_out, BLOB_GRAPH, "o_tout", true); AT(p.t_outw, BLOB_GRAPH, "o_toutw", true);
    AT(p.t_in, BLOB_GRAPH, "o_tin", true); AT(p.nd_rid, BLOB_GRAPH, "o_rid", true); AT(p.msa_rank, BLOB_GRAPH, "o_mrank", true); AT(p.msa_off, BLOB_GRAPH, "o_msaoff", true);
    AT(p.row_node[0], BLOB_GRAPH, "o_order0", true); AT(p.row_node[1], BLOB_GRAPH, "o_order1", true); AT(p.is_rc, BLOB_GRAPH, "o_isrc", P.amb);
    AT(p.cons_node, BLOB_GRAPH, "o_cnode", true); AT(p.cons_cov, BLOB_GRAPH, "o_ccov", true); AT(p.cons_base, BLOB_GRAPH, "o_cbase", true);
    AT(g.walk, BLOB_GRAPH, "o_gwalk", P.want_gfa); AT(g.cnt, BLOB_GRAPH, "o_gcnt", P.want_gfa); AT(g.orw, BLOB_GRAPH, "o_gorw", P.want_gfa); AT(g.off, BLOB_GRAPH, "o_goff", P.want_gfa);
    AT(p.scratch, BLOB_ROWS, "o_scratch", true); AT(p.aln, BLOB_ROWS, "o_aln_desc", true); AT(p.out, BLOB_ROWS, "o_out_rec", true); AT(p.row_base, BLOB_ROWS, "o_rbase", true);
    AT(p.row_sdist, BLOB_ROWS, "o_rsd", true); AT(p.row_pd, BLOB_ROWS, "o_rpd", true); AT(p.row_node_id, BLOB_ROWS, "o_rnid", true); AT(p.row_remain, BLOB_ROWS, "o_rrem", true);
    AT(p.pred_off, BLOB_ROWS, "o_poff", true); AT(p.pred_row, BLOB_ROWS, "o_pred", true); AT(p.cigar, BLOB_ROWS, "o_cigar", true);
    AT(p.out_off, BLOB_ROWS, "o_ooff", gen_io); AT(p.out_row, BLOB_ROWS, "o_orow", gen_io); AT(p.retry, BLOB_ROWS, "o_retry", P.amb);
    AT(p.out_fwd, BLOB_ROWS, "o_outfwd", P.amb); AT(p.cigar_fwd, BLOB_ROWS, "o_cigfwd", P.amb);
    AT(b.dp_beg_sn, BLOB_ROWS, "o_bsn", true); AT(b.dp_end_sn, BLOB_ROWS, "o_esn", true); AT(b.row_cell_off, BLOB_ROWS, "o_coff", true); AT(b.row_max_i, BLOB_ROWS, "o_rmi", true);
    if (gen_io) { AT(b.left, BLOB_ROWS, "o_left", true); AT(b.right, BLOB_ROWS, "o_right", true); AT(b.row_active, BLOB_ROWS, "o_act", true);
            CHECK(b.out_off == p.out_off && b.out_row == p.out_row); }
    else CHECK(b.left == p.scratch && b.right == p.scratch && b.row_active == p.row_base && b.out_off == p.pred_off && b.out_row == p.pred_row);
#undef AT
    CHECK(p.msa_out == nullptr && !g.seg_node && !g.seg_base && !g.link_off && !g.link_from && !g.path_off && !g.path_node);
    CHECK(b.aln == p.aln && b.out == p.out && b.query == p.reads && b.row_base == p.row_base && b.row_sdist == p.row_sdist && b.row_pd == p.row_pd &&
          b.row_node_id == p.row_node_id && b.row_remain == p.row_remain && b.pred_off == p.pred_off && b.pred_row == p.pred_row && b.cigar == p.cigar && b.planes == D.planes);
    CHECK(b.n == n_sets && b.ret_cigar == 1 && b.fresh_band == 1 && b.dir_mode == (P.dir ? (P.dir_wide ? 2 : 1) : 0));
    CHECK(b_rc.left == b.left && b_rc.row_active == b.row_active && b_rc.want_lr == 0 && b_rc.fresh_band == ((P.amb && P.sc.wb >= 0) ? 0 : 1));
    CHECK(b.want_lr == ((P.amb && P.sc.wb >= 0 && !P.general) ? 1 : 0));
    CHECK(p.n_sets == n_sets && p.in_cap == P.in_cap && p.out_cap == P.out_cap && p.aln_cap == P.aln_cap && p.rid_words == P.rid_words && p.dig_on == 1);
    CHECK(p.order_mode == ((P.local || P.extend) ? 1 : 0) && p.general == (P.general ? 1 : 0) && p.msa_cons == ((P.want_msa && P.want_cons) ? 1 : 0));
    CHECK(p.lds_rows == (P.max_node_cap <= 8000 ? ((P.max_node_cap + 3) & ~3) : 0));
    // the LDS capacities of the walks under the two switches, against the parent's two copies of the rule
    for (int sw = 0; sw < 4; ++sw) {
        CHECK(set_option("ABPOA_HIP_ORDER_LDS", (sw & 1) ? "0" : nullptr) == 0 && set_option("ABPOA_HIP_ORDER_CAP", (sw & 2) ? "8" : nullptr) == 0);
        int order_lds, order_ecap, gfa_lds; parent_caps(P, &order_lds, &order_ecap, &gfa_lds);
        PoaDev q; GfaDev h; bind_poa_dev(q, h, P, L, n_sets, any_w, false, D.d[BLOB_IN], D.d[BLOB_GRAPH], D.d[BLOB_ROWS]);
        CHECK(q.order_lds == order_lds && q.order_ecap == order_ecap && h.lds_cap == gfa_lds && q.dig_on == 0);
        if ((sw & 2) && (q.order_mode || P.want_msa)) CHECK(q.order_lds == 8);
        if ((sw & 1) && P.want_gfa) CHECK(h.lds_cap == 0);
    }
    CHECK(set_option("ABPOA_HIP_ORDER_LDS", nullptr) == 0 && set_option("ABPOA_HIP_ORDER_CAP", nullptr) == 0);
}

// ---- output layouts and unpacking, round trip.  Values are keyed by (set, pool, index): a slice shifted by a set's slack reads another key
static int32_t key(int set, int pool, int64_t i) { return (int32_t)(set * 1000003 + pool * 10007 + i * 7 + 1); }
enum { K_CNODE, K_CCOV, K_CBASE, K_ISRC, K_MSA, K_SEG, K_SBASE, K_LOFF, K_LFROM, K_PNODE };
// what the device would have left for set s: kind 0 finished, 1 POA_ST_FALLBACK, 2 finished with an empty graph, 3 finished with no segment, 4 finished but the
// fill kernel's flag is set, 5 finished and its last path offset lies past the set's path capacity
static void round_trip(const abpoa_hip_scoring_t &sc, Sets &S, unsigned flags, const std::vector<int> &kind) {
    const int n = S.n(); const abpoa_hip_readset_t *sets = S.get();
    const DevicePlan P = plan_device_job(&sc, n, sets, 3.0, flags, false);
    const Layout L = lay_out_device(P, n, false);
    uint8_t *hg = (uint8_t *)malloc(L.dl_bytes); memset(hg, 0xEE, L.dl_bytes);
    PoaState *hs = (PoaState *)(hg + L.o_state); int32_t *cnt = (int32_t *)(hg + L.o_gcnt);
    std::vector<int> n_seg(n, 0), n_link(n, 0); std::vector<int64_t> cap(n, 0), n_pn(n, 0);
    for (int s = 0; s < n; ++s) {
        memset(&hs[s], 0, sizeof(PoaState));
        hs[s].status = kind[s] == 1 ? POA_ST_FALLBACK : POA_ST_OK; hs[s].reason = kind[s] == 1 ? POA_WHY_NODES_IN_FUSE : 0; hs[s].n_nodes = kind[s] == 2 ? 2 : 9 + s;
        hs[s].cons_len = std::min(P.ps[s].cons_cap, 5 + s); hs[s].msa_len = 3 + s; hs[s].n_cells = 1000 + s;
        for (int i = 0; i < P.ps[s].cons_cap; ++i) { const int64_t c = P.ps[s].cons0 + i;
            ((int32_t *)(hg + L.o_cnode))[c] = key(s, K_CNODE, i); ((int32_t *)(hg + L.o_ccov))[c] = key(s, K_CCOV, i); (hg + L.o_cbase)[c] = (uint8_t)key(s, K_CBASE, i); }
        if (P.amb) for (int r = 0; r < sets[s].n_reads; ++r) (hg + L.o_isrc)[P.ps[s].read0 + r] = (uint8_t)key(s, K_ISRC, r);
        for (int l : S.lens[s]) cap[s] += l;
        if (kind[s] != 3) { n_seg[s] = 11 + s; n_link[s] = 6 + 2 * s; n_pn[s] = std::min<int64_t>(cap[s], 3 + s); }
        if (P.want_gfa) { cnt[3 * s] = n_seg[s]; cnt[3 * s + 1] = n_link[s]; cnt[3 * s + 2] = 0; }
    }
    auto done = [&](int s) { return hs[s].status == POA_ST_OK && hs[s].n_nodes > 2; };
    // MSA rows
    MsaLayout M; uint8_t *h_msa = nullptr;
    if (P.want_msa) {
        M = lay_out_msa(P, n, sets, hs);
        int64_t at = 0;
        for (int s = 0; s < n; ++s) { CHECK(M.off[s] == at); if (done(s)) at += (int64_t)(sets[s].n_reads + (P.want_cons ? 1 : 0)) * hs[s].msa_len; }
        CHECK(M.total == at && (int)M.off.size() == n);
        h_msa = (uint8_t *)malloc((size_t)M.total);
        for (int s = 0; s < n; ++s) if (done(s)) for (int64_t i = 0; i < (int64_t)(sets[s].n_reads + (P.want_cons ? 1 : 0)) * hs[s].msa_len; ++i) h_msa[M.off[s] + i] = (uint8_t)key(s, K_MSA, i);
    }
    // GFA pools
    GfaLayout G; uint8_t *h_gfa = nullptr;
    if (P.want_gfa) {
        G = lay_out_gfa(P, n, sets, hs, cnt);
        int64_t seg = 0, link = 0, path = 0;
        for (int s = 0; s < n; ++s) {
            const bool any = done(s) && n_seg[s] > 0;
            CHECK(G.off[4 * s] == seg && G.off[4 * s + 1] == link && G.off[4 * s + 2] == path && G.off[4 * s + 3] == (any ? cap[s] : 0));
            if (any) { seg += n_seg[s]; link += n_link[s]; path += cap[s]; }
        }
        CHECK(G.seg_tot == seg && G.link_tot == link && G.path_tot == path && (G.bytes != 0) == (seg > 0) && (int)G.off.size() == 4 * n);
        if (G.bytes) {
            // the seven pools: 256-aligned, disjoint, each at least what the fill kernel indexes (link_off: a slot more per set, path_off likewise)
            const size_t off[8] = {G.o_seg, G.o_loff, G.o_lfrom, G.o_poff, G.o_pnode, G.o_base, G.o_cnt, G.bytes};
            const size_t min_b[7] = {4 * (size_t)seg, 4 * (size_t)(seg + n), 4 * (size_t)link, 8 * (size_t)(P.tot_reads + n), 4 * (size_t)path, (size_t)seg, 12 * (size_t)n};
            for (int i = 0; i < 7; ++i) CHECK(off[i] % 256 == 0 && off[i] + min_b[i] <= off[i + 1]);
            uint8_t *dq = (uint8_t *)malloc(G.bytes); GfaDev g; memset(&g, 0, sizeof(g)); bind_gfa_pools(g, G, dq);
            CHECK((uint8_t *)g.seg_node == dq + G.o_seg && (uint8_t *)g.link_off == dq + G.o_loff && (uint8_t *)g.link_from == dq + G.o_lfrom &&
                  (uint8_t *)g.path_off == dq + G.o_poff && (uint8_t *)g.path_node == dq + G.o_pnode && g.seg_base == dq + G.o_base);
            free(dq);
            h_gfa = (uint8_t *)malloc(G.bytes); memset(h_gfa, 0xEE, G.bytes);
            for (int s = 0; s < n; ++s) {
                int32_t *c2 = (int32_t *)(h_gfa + G.o_cnt) + 3 * s; c2[0] = n_seg[s]; c2[1] = n_link[s]; c2[2] = kind[s] == 4 ? 1 : 0;
                if (!(done(s) && n_seg[s] > 0)) continue;
                const int64_t s0 = G.off[4 * s], l0 = G.off[4 * s + 1], p0 = G.off[4 * s + 2]; const int nr = sets[s].n_reads;
                for (int i = 0; i < n_seg[s]; ++i) { ((int32_t *)(h_gfa + G.o_seg))[s0 + i] = key(s, K_SEG, i); (h_gfa + G.o_base)[s0 + i] = (uint8_t)key(s, K_SBASE, i); }
                for (int i = 0; i <= n_seg[s]; ++i) ((int32_t *)(h_gfa + G.o_loff))[s0 + s + i] = key(s, K_LOFF, i);
                for (int i = 0; i < n_link[s]; ++i) ((int32_t *)(h_gfa + G.o_lfrom))[l0 + i] = key(s, K_LFROM, i);
                int64_t *po = (int64_t *)(h_gfa + G.o_poff) + P.ps[s].read0 + s;
                for (int r = 0; r <= nr; ++r) po[r] = n_pn[s] * r / nr;
                if (kind[s] == 5) po[nr] = cap[s] + 5;
                for (int64_t i = 0; i < cap[s]; ++i) ((int32_t *)(h_gfa + G.o_pnode))[p0 + i] = key(s, K_PNODE, i);
            }
        }
    }
    // unpack every set and hold every field against what was written
    for (int s = 0; s < n; ++s) {
        abpoa_hip_msa_t o; memset(&o, 0x55, sizeof(o));
        const bool redo = unpack_set(P, L, M, G, sets[s], s, hg, h_msa, h_gfa, &o);
        const int nr = sets[s].n_reads;
        CHECK(redo == (kind[s] == 1 || (kind[s] == 4 && P.want_gfa && G.bytes)));
        CHECK(o.n_reads == nr && o.status == 0);
        if (redo) { abpoa_hip_msa_t z; memset(&z, 0, sizeof(z)); z.n_reads = nr; CHECK(!memcmp(&o, &z, sizeof(o))); continue; }
        CHECK(o.n_cells == 1000 + s);
        CHECK((o.is_rc != nullptr) == P.amb);
        if (o.is_rc) for (int r = 0; r < nr; ++r) CHECK(o.is_rc[r] == (uint8_t)key(s, K_ISRC, r));
        if (P.want_cons && done(s)) {
            CHECK(o.cons_len == hs[s].cons_len && o.cons_base && o.cons_cov && o.cons_node_id);
            for (int i = 0; i < o.cons_len; ++i) CHECK(o.cons_node_id[i] == key(s, K_CNODE, i) && o.cons_cov[i] == key(s, K_CCOV, i) && o.cons_base[i] == (uint8_t)key(s, K_CBASE, i));
        } else CHECK(o.cons_len == 0 && !o.cons_base && !o.cons_cov && !o.cons_node_id);
        if (P.want_msa && done(s)) {
            CHECK(o.msa_len == hs[s].msa_len && o.msa_rows == nr + (P.want_cons ? 1 : 0) && o.msa_base);
            for (int64_t i = 0; i < (int64_t)o.msa_rows * o.msa_len; ++i) CHECK(o.msa_base[i] == (uint8_t)key(s, K_MSA, i));
        } else CHECK(o.msa_len == 0 && o.msa_rows == 0 && !o.msa_base);      // (an empty graph has no MSA buffer)
        if (P.want_gfa) {
            const bool any = done(s) && n_seg[s] > 0 && G.bytes; const abpoa_hip_gfa_t *g = o.gfa;
            CHECK(g != nullptr);
            if (g) {
                CHECK(g->n_seg == (any ? n_seg[s] : 0) && g->n_link == (any ? n_link[s] : 0) && g->n_path == nr);
                const int64_t want_pn = !any ? 0 : kind[s] == 5 ? cap[s] : n_pn[s];
                for (int i = 0; any && i < g->n_seg; ++i) CHECK(g->seg_node[i] == key(s, K_SEG, i) && g->seg_base[i] == (uint8_t)key(s, K_SBASE, i));
                for (int i = 0; any && i <= g->n_seg; ++i) CHECK(g->link_off[i] == key(s, K_LOFF, i));
                for (int i = 0; any && i < g->n_link; ++i) CHECK(g->link_from[i] == key(s, K_LFROM, i));
                for (int r = 0; r <= nr; ++r) CHECK(g->path_off[r] == (!any ? 0 : (r == nr && kind[s] == 5) ? cap[s] + 5 : n_pn[s] * r / nr));
                for (int64_t i = 0; i < want_pn; ++i) CHECK(g->path_node[i] == key(s, K_PNODE, i));
                CHECK(g->path_node[want_pn] == 0);      // (gfa_alloc's spare slot: nothing was copied past the clamp)
            }
        } else CHECK(o.gfa == nullptr);
        free(o.cons_base); free(o.cons_cov); free(o.cons_node_id); free(o.msa_base); free(o.is_rc); gfa_free(o.gfa);
    }
    free(hg); free(h_msa); free(h_gfa);
}

int main() {
    // (the harness owns every switch the layout reads: nothing inherited from the environment)
    for (const char *sw : {"ABPOA_HIP_ORDER_LDS", "ABPOA_HIP_ORDER_CAP", "ABPOA_HIP_DBG", "ABPOA_HIP_NODIR", "ABPOA_HIP_NOWIDE", "ABPOA_HIP_WIDE_LO", "ABPOA_HIP_DEVICE_GENERAL",
                           "ABPOA_HIP_NOFAST", "ABPOA_HIP_NOXL", "ABPOA_HIP_RING_ROWS", "ABPOA_HIP_DIR_WIDE", "ABPOA_HIP_EXTRA_ROUTE_MIN", "ABPOA_HIP_ARENA_PCT", "ABPOA_HIP_VERBOSE"}) unsetenv(sw);
    const unsigned CONS = ABPOA_HIP_OUT_CONS, MSA = ABPOA_HIP_OUT_MSA, GFA = ABPOA_HIP_OUT_GFA;
    const unsigned outputs[5] = {CONS, MSA, MSA | CONS, GFA, GFA | MSA | CONS};
    const char *const modes[6] = {"global", "local", "-s", "weights", "general", "linear"};
    // shapes: one set and three; reads of 1 to 40 bases; sets of one and of two reads; jobs of at most two rounds (the upload has no second part)
    const std::vector<std::vector<std::vector<int32_t>>> shapes = {
        {{7, 1, 40, 13, 22}}, {{5, 9, 40, 3}, {17}, {1, 33}}, {{12, 40}}, {{9}}, {{4, 8}, {6}, {40, 1}},
    };
    bool saw_few_rounds = false, saw_split = false;
    for (int f = 0; f < 2; ++f) for (size_t sh = 0; sh < shapes.size(); ++sh) for (int mo = 0; mo < 6; ++mo) for (int ou = 0; ou < 5; ++ou) {
        if (f == 1 && !(sh == 1 && ou == 4)) continue;      // the roomy pass (node_factor 4096: an edge slot per read) on one job per mode
        Sets S; S.lens = shapes[sh];
        // (... whose first set has 250 reads: more edge slots than POA_IN_CAP / POA_OUT_CAP, and more nodes than the LDS tables of the walks and of prepare hold)
        if (f) { S.lens[0].clear(); for (int r = 0; r < 250; ++r) S.lens[0].push_back(40 - r % 7); }
        if (mo == 3) S.w_set = (int)S.lens.size() - 1;
        const abpoa_hip_scoring_t sc = scoring(mo == 5 ? ABPOA_HIP_LINEAR_GAP : ABPOA_HIP_AFFINE_GAP, mo == 1 ? ABPOA_HIP_LOCAL_MODE : ABPOA_HIP_GLOBAL_MODE);
        const unsigned flags = outputs[ou] | (mo == 2 ? ABPOA_HIP_AMB_STRAND : 0u); const bool any_w = mo == 3;
        g_case = std::string(modes[mo]) + ", shape " + std::to_string(sh) + ", output " + std::to_string(ou) + (f ? ", roomy" : "");
        const DevicePlan P = plan_device_job(&sc, S.n(), S.get(), f ? 4096.0 : 3.0, flags, mo == 4);
        CHECK((int)P.ps.size() == S.n() && P.amb == (mo == 2) && P.local == (mo == 1) && (mo != 4 || P.general) && P.roomy == (f == 1));
        if (mo == 1) CHECK(P.local || P.extend);
        const Layout L = lay_out_device(P, S.n(), any_w);
        layout_checks(P, L, S.n(), any_w);
        binding_checks(P, L, S.n(), any_w);
        read_table_checks(P, S);
        saw_few_rounds |= P.max_reads <= 2; saw_split |= P.max_reads > 2;
        if (f) CHECK(P.in_cap > POA_IN_CAP && P.out_cap > POA_OUT_CAP && P.max_node_cap > 8000);
        g_jobs++;
    }
    CHECK(saw_few_rounds && saw_split);
    // round trips: seven sets of every kind, a set of one read and one of two among them; then a job in which no set has a segment (no GFA pools at all)
    for (int ou = 0; ou < 5; ++ou) for (int amb = 0; amb < 2; ++amb) {
        // (28 reads and, in the first round trip, 59 segments in 7 sets: the slack slots of path_off -- 8 x (28 + 7) bytes -- and of link_off -- 4 x (59 + 7) --
        //  reach into another 256 bytes, so a pool laid out without them is one alignment step short and fails the pool-size check below)
        Sets S; S.lens = {{9, 12, 7}, {30, 31}, {5}, {8, 40, 2, 6}, {11, 13}, {1, 2, 3}, {21, 20, 19, 18, 17, 5, 6, 7, 8, 9, 10, 11, 12}};
        const abpoa_hip_scoring_t sc = scoring(ABPOA_HIP_AFFINE_GAP, ABPOA_HIP_GLOBAL_MODE); const unsigned flags = outputs[ou] | (amb ? ABPOA_HIP_AMB_STRAND : 0u);
        g_case = "round trip, output " + std::to_string(ou) + (amb ? ", -s" : "");
        round_trip(sc, S, flags, {0, 1, 2, 3, 4, 5, 0});
        g_case += ", no segments"; round_trip(sc, S, flags, {3, 1, 2, 3, 3, 3, 2});
        Sets T; T.lens = {{6, 40, 1}}; g_case += ", one set"; round_trip(sc, T, flags, {5});
    }
    // event slots
    for (int max_reads : {1, 2, 3, 50}) {
        g_case = "event slots, " + std::to_string(max_reads) + " reads";
        const EventSlots E{max_reads}; std::vector<int> v = {E.job_begin(), E.after_init(), E.rounds_begin(), E.rounds_end()};
        for (int k = 1; k < max_reads; ++k) for (int i = 0; i < 4; ++i) v.push_back(E.round(k) + i);
        for (int i = 0; i < 4; ++i) v.push_back(E.gfa() + i);
        CHECK(E.count() == 4 * max_reads + 8);
        for (int x : v) CHECK(x >= 0 && x < E.count());
        std::sort(v.begin(), v.end()); CHECK(std::adjacent_find(v.begin(), v.end()) == v.end());
    }
    if (g_fail) { fprintf(stderr, "%d checks failed\n", g_fail); return 1; }
    printf("device layout ok (%d jobs)\n", g_jobs);
    return 0;
}
