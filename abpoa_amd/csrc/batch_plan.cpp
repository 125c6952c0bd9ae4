// Host arithmetic of the flat batch driver: see batch_plan.h.  No call into the HIP runtime.
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include "engine_options.h"
#include "batch_plan.h"
#include "routing.h"
#include "dir_plane.h"

namespace abpoa_hip {

PoolTotals describe_batch(const abpoa_hip_scoring_t *sc, int n, const BatchShape *sh, AlnDesc *desc, ArenaCells *cells) {
    const bool banded = sc->wb >= 0;
    PoolTotals T{0, 0, 0, 0, 0};
    for (int i = 0; i < n; ++i) {
        AlnDesc &d = desc[i]; ArenaCells &c = cells[i];
        d.n_rows = sh[i].n_rows; d.qlen = sh[i].qlen;
        d.bits = abpoa_hip_score_bits(sc, d.n_rows, d.qlen, &d.inf_min);
        d.w = sc->wb < 0 ? d.qlen : sc->wb + (int)(sc->wf * d.qlen);     // reference :445 (float32 product)
        d.cigar_cap = d.n_rows + d.qlen + 8;
        d.query_off = T.q; d.row0 = T.rows; d.poff0 = T.rows + i; d.pred0 = T.preds; d.out0 = T.outs; d.cigar_off = T.cig;
        T.q += d.qlen; T.rows += d.n_rows; T.preds += sh[i].n_pred; T.outs += sh[i].n_out; T.cig += d.cigar_cap;
        const int pn = d.bits == 16 ? 16 : 8;
        const int64_t width = padded_width(d.qlen, pn);
        // values per DP column in the arena: P planes (general kernel) or one padded cell record (fast loop: 4 / 8 values)
        // (linear gaps: one plane in the general kernel, {H, match flag} in the fast loops)
        const int pv = record_values(sc->gap_mode);
        c.full = width * pv * d.n_rows;
        int64_t est = band_cols(width, d.w, pn, banded);
        // (tests: force the overflow -> full-width retry path)
        { const int pct_ = opt_int("ABPOA_HIP_ARENA_PCT", 0); if (pct_ > 0 && pct_ < 100) est = std::max<int64_t>(pn, est * pct_ / 100); }
        d.plane_cap = std::min<int64_t>(c.full, width * pv + est * pv * (d.n_rows - 1));
        c.est = d.plane_cap;
        // direction-plane arenas (dir_plane.h; a pass decides whether it uses them): words of DB bytes per column for every row, score records for the
        // first row and about one row in four (cells of the score width: DB bytes = DB * 8 / bits cells); full = every row at full width with its records
        const int64_t dbc = (sc->gap_mode == ABPOA_HIP_AFFINE_GAP ? 2 : 4) * 8 / d.bits + 1;
        c.dir_full = width * (pv + dbc) * d.n_rows + 64;
        c.dir_est = std::min<int64_t>(c.dir_full, width * (pv + dbc) + (est * dbc + est * pv / 4 + 2 * pn) * (d.n_rows - 1));
    }
    return T;
}

InLayout layout_in(int n, int m, const PoolTotals &t) {
    InLayout I; size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o = align_up(o + bytes); return at; };
    I.desc = take(sizeof(AlnDesc) * n); I.mat = take(sizeof(int32_t) * m * m); I.query = take(t.q + 1);
    I.base = take(t.rows); I.sdist = take(t.rows); I.pd = take(8 * t.rows); I.nid = take(4 * t.rows); I.rem = take(4 * t.rows); I.act = take(t.rows);
    // slack: tile prefetch over-reads up to TP entries
    I.poff = take(4 * (t.rows + n)); I.pred = take(4 * (t.preds + 1)); I.ooff = take(4 * (t.rows + n)); I.out = take(4 * (t.outs + 1) + 4 * 512);
    I.bytes = o;
    return I;
}
OutLayout layout_out(int n, const PoolTotals &t) {
    OutLayout O; size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o = align_up(o + bytes); return at; };
    O.rec = take(sizeof(AlnOut) * n); O.cig = take(8 * t.cig); O.left = take(4 * t.rows); O.right = take(4 * t.rows);
    O.bsn = take(4 * t.rows); O.esn = take(4 * t.rows); O.coff = take(8 * t.rows); O.rmi = take(4 * t.rows);
    O.bytes = o;
    return O;
}

ProblemSlots problem_slots(const InLayout &I, const OutLayout &O, const AlnDesc &d, uint8_t *hi, uint8_t *ho) {
    ProblemSlots s;
    s.query = hi + I.query + d.query_off; s.row_base = hi + I.base + d.row0;
    s.row_node_id = (int32_t *)(hi + I.nid) + d.row0; s.row_remain = (int32_t *)(hi + I.rem) + d.row0; s.row_active = hi + I.act + d.row0;
    s.pred_off = (int32_t *)(hi + I.poff) + d.poff0; s.pred_row = (int32_t *)(hi + I.pred) + d.pred0;
    s.out_off = (int32_t *)(hi + I.ooff) + d.poff0; s.out_row = (int32_t *)(hi + I.out) + d.out0;
    s.left = (int32_t *)(ho + O.left) + d.row0; s.right = (int32_t *)(ho + O.right) + d.row0;
    return s;
}

void mark_fast_ok(const abpoa_hip_scoring_t *sc, bool fresh, int n, AlnDesc *desc, const uint8_t *row_active, const int32_t *left, const int32_t *right) {
    const bool banded = sc->wb >= 0;
    for (int i = 0; i < n; ++i) {
        AlnDesc &d = desc[i]; bool ok = banded || (sc->align_mode == ABPOA_HIP_LOCAL_MODE && sc->wb < 0);      // (unbanded local: the local row loop; band state is not used)
        if (ok && memchr(row_active + d.row0, 0, (size_t)d.n_rows)) ok = false;
        if (ok && banded && !fresh) {
            const int32_t *l = left + d.row0, *r = right + d.row0;
            for (int k = 0; k < d.n_rows && ok; ++k) ok = l[k] == d.n_rows && r[k] == 0;
        }
        d.flags = ok ? ALN_FAST_OK : 0; d.pad0 = 0;
    }
}

// how far down the row order every row's scores are still needed (DevBatch.row_sdist); a row with more predecessors than a word can name keeps the alignment off the fast loops
bool fill_dir_tables(int n_rows, const int32_t *po, const int32_t *pr, uint8_t *sd, uint32_t *pdw) {
    memset(sd, 0, (size_t)n_rows);
    bool ok = true;
    for (int r = 0; r < n_rows; ++r) {
        if (po[r + 1] - po[r] > DIR_K_MAX && r < n_rows - 1) ok = false;
        uint64_t pdv = ~0ull;       // a byte per predecessor, 255 = none / too far
        for (int k = po[r]; k < po[r + 1]; ++k) {
            const int p_ = pr[k], dist = r == n_rows - 1 ? 255 : std::min(255, r - p_); if (dist > sd[p_]) sd[p_] = (uint8_t)dist;
            const int t = k - po[r]; if (t < 8 && r - p_ <= 254) pdv = (pdv & ~(0xffull << (8 * t))) | ((uint64_t)(r - p_) << (8 * t));
        }
        pdw[2 * r] = (uint32_t)pdv; pdw[2 * r + 1] = (uint32_t)(pdv >> 32);      // row distances to the first eight predecessors, two dwords per row (DevBatch.row_pd)
    }
    return ok;
}

// direction-plane arenas for the fast row loops (dir_plane.h) unless the caller wants the score planes back (trace), the penalties do not fit the
// words, or ABPOA_HIP_NODIR=1; an alignment whose backtrack meets the one case the words cannot decide is redone with score records
// (tests: ABPOA_HIP_DIRTRACE=1 keeps the direction plane in trace mode; the trace then carries the WORDS of every cell in plane 0)
bool dir_words_for_run(const abpoa_hip_scoring_t *sc, unsigned flags) {
    const bool banded = sc->wb >= 0, trace = flags & BS_TRACE;
    const bool dirtrace = trace && opt_on("ABPOA_HIP_DIRTRACE");
    return (!trace || dirtrace) && banded && sc->align_mode == ABPOA_HIP_GLOBAL_MODE && dir_words_allowed(sc);
}

void plan_pass(const abpoa_hip_scoring_t *sc, unsigned flags, bool dir, const AlnDesc *desc, const std::vector<int> &todo, DevBatch &b) {
    const bool banded = sc->wb >= 0, trace = flags & BS_TRACE, fresh = flags & BS_FRESH_BAND;
    memset(&b, 0, sizeof(b));
    b.n = (int)todo.size(); b.m = sc->m;
    {   // ---- LDS plan (engine.h LdsPlan): sized for the widest expected band / largest query of this pass
        int max_qlen = 0, max_bits = 16; int64_t est_cols = 0;
        for (int i : todo) {
            const AlnDesc &d = desc[i];
            max_qlen = std::max(max_qlen, d.qlen); max_bits = std::max(max_bits, d.bits);
            const int pn = d.bits == 16 ? 16 : 8;
            est_cols = std::max<int64_t>(est_cols, band_cols(padded_width(d.qlen, pn), d.w, pn, banded));
        }
        make_lds_plan(sc, max_qlen, max_bits, est_cols, b.n, &b.lds);
        for (int i : todo) b.bits_mask |= desc[i].bits == 16 ? 1 : 2;
        bool any_wide = false, all_wide = true;
        for (int i : todo) { const bool wd = takes_wide_band(b.lds, desc[i].w); any_wide |= wd; all_wide &= wd; }
        if (!any_wide) b.lds.wide_on = 0;
        b.lds.narrow_off = (b.lds.wide_on >= 1 && all_wide) ? 1 : 0;
    }
    // (ABPOA_HIP_DIR_WIDE=1: words for the wide-band alignments too -- the device-resident driver does that by itself when the record arenas of a
    //  job do not fit the device; here it is a test switch)
    const bool dir_wide = dir && opt_int("ABPOA_HIP_DIR_WIDE", 0) > 0;
    set_job_fields(b, *sc); b.dbg = opt_int("ABPOA_HIP_DBG", 0); b.dir_mode = dir ? (dir_wide ? 2 : 1) : 0;      // (what the routing rules read: routing.h)
    b.ret_cigar = sc->ret_cigar; b.rev_cigar = sc->rev_cigar;
    b.want_trace = trace ? 1 : 0; b.fresh_band = fresh ? 1 : 0;
    b.want_lr = (trace || (flags & BS_WANT_BAND_STATE)) ? 1 : 0;
}

int64_t assign_arenas(const DevBatch &b, bool first_pass, const ArenaCells *cells, const std::vector<int> &todo, AlnDesc *desc, AlnDesc *pass, int *n_fast) {
    int64_t plane_bytes = 0;
    *n_fast = 0;       // alignments of the fast row loops; the general kernel has the rest
    for (size_t t = 0; t < todo.size(); ++t) {
        AlnDesc &d = desc[todo[t]]; const ArenaCells &c = cells[todo[t]];
        // direction-plane arenas for the narrow-band alignments of a dir pass; the wide-band ones keep score records (routing.h takes_dir)
        // (an alignment the general kernel will run -- seeded band of the -s retry, a row with more predecessors than a word names, no fast row loop in the
        //  plan -- stores its planes: the records' estimate, not the words')
        const bool dir_a = takes_fast(b, d) && takes_dir(b, d);
        *n_fast += for_tail_kernel(b, d) ? 1 : 0;
        d.plane_cap = dir_a ? (first_pass ? c.dir_est : c.dir_full) : (first_pass ? c.est : c.full);
        d.plane_off = plane_bytes; plane_bytes += (int64_t)align_up((size_t)d.plane_cap * (d.bits / 8) + 64 * 8 * 4);   // + 64 records of slack (fast loop stores whole 64-lane chunks)
        pass[t] = d;
    }
    return plane_bytes;
}

void bind_pools(DevBatch &b, const InLayout &I, const OutLayout &O, uint8_t *di, uint8_t *dout, uint8_t *planes) {
    b.row_sdist = di + I.sdist; b.row_pd = (const uint32_t *)(di + I.pd);
    b.mat = (const int32_t *)(di + I.mat); b.aln = (const AlnDesc *)(di + I.desc); b.out = (AlnOut *)(dout + O.rec);
    b.query = di + I.query; b.row_base = di + I.base; b.row_node_id = (const int32_t *)(di + I.nid); b.row_remain = (const int32_t *)(di + I.rem);
    b.row_active = di + I.act; b.pred_off = (const int32_t *)(di + I.poff); b.pred_row = (const int32_t *)(di + I.pred);
    b.out_off = (const int32_t *)(di + I.ooff); b.out_row = (const int32_t *)(di + I.out);
    b.left = (int32_t *)(dout + O.left); b.right = (int32_t *)(dout + O.right);
    b.dp_beg_sn = (int32_t *)(dout + O.bsn); b.dp_end_sn = (int32_t *)(dout + O.esn); b.row_cell_off = (int64_t *)(dout + O.coff);
    b.row_max_i = (int32_t *)(dout + O.rmi); b.planes = planes; b.cigar = (uint64_t *)(dout + O.cig);
}

void unpack_trace(const AlnDesc &d, int P, bool banded, int cw, const int32_t *bsn, const int32_t *esn, const int64_t *coff, const int32_t *rmi,
                  const uint8_t *arena, abpoa_hip_trace_t *T) {
    const int gn = d.n_rows; const int pn = d.bits == 16 ? 16 : 8;
    T->bits = d.bits; T->n_planes = P;
    T->dp_beg = (int32_t *)malloc(4 * gn); T->dp_end = (int32_t *)malloc(4 * gn); T->dp_beg_sn = (int32_t *)malloc(4 * gn); T->dp_end_sn = (int32_t *)malloc(4 * gn);
    T->row_off = (int64_t *)malloc(8 * (gn + 1)); T->row_max_i = (int32_t *)malloc(4 * gn);
    memcpy(T->row_max_i, rmi, 4 * gn);
    int64_t tot = 0;
    for (int rr = 0; rr < gn; ++rr) {
        T->row_off[rr] = tot;
        const bool computed = rr < gn - 1 && bsn[rr] >= 0;
        if (!computed) { T->dp_beg[rr] = T->dp_end[rr] = T->dp_beg_sn[rr] = T->dp_end_sn[rr] = -1; T->row_max_i[rr] = -2; continue; }
        T->dp_beg_sn[rr] = bsn[rr]; T->dp_end_sn[rr] = esn[rr]; T->dp_beg[rr] = bsn[rr] * pn;
        T->dp_end[rr] = (banded || rr == 0) ? (esn[rr] + 1) * pn - 1 : d.qlen;
        if (rr == 0) T->row_max_i[rr] = -2;
        tot += (int64_t)(esn[rr] - bsn[rr] + 1) * pn * P;
    }
    T->row_off[gn] = tot;
    T->planes = malloc((size_t)std::max<int64_t>(tot, 1) * (d.bits / 8));
    // cw, the arena cell stride: 0 = plane-major rows (general kernel), > 0 cell records (fast loop), < 0 direction words of -cw bytes
    for (int rr = 0; rr < gn; ++rr) {
        if (T->dp_beg_sn[rr] < 0) continue;
        const int64_t nv = T->row_off[rr + 1] - T->row_off[rr];
        if (cw < 0) {      // (ABPOA_HIP_DIRTRACE) plane 0 = the cell's direction word, the other planes 0; row 0 has no words
            const int64_t W = nv / P;
            for (int64_t x = 0; x < nv; ++x) { if (d.bits == 16) ((int16_t *)T->planes)[T->row_off[rr] + x] = 0; else ((int32_t *)T->planes)[T->row_off[rr] + x] = 0; }
            if (rr == 0) continue;
            const uint8_t *src = arena + coff[rr] * (d.bits / 8);
            for (int64_t x = 0; x < W; ++x) {
                const uint32_t wv = cw == -2 ? (uint32_t)((const uint16_t *)src)[x] : ((const uint32_t *)src)[x];
                // (32-bit words in 16-bit planes: low half in plane 0, high half in plane 1)
                if (d.bits == 16) { ((int16_t *)T->planes)[T->row_off[rr] + x] = (int16_t)wv; if (cw == -4) ((int16_t *)T->planes)[T->row_off[rr] + W + x] = (int16_t)(wv >> 16); }
                else ((int32_t *)T->planes)[T->row_off[rr] + x] = (int32_t)wv;
            }
            continue;
        }
        if (cw == 0) { memcpy((uint8_t *)T->planes + T->row_off[rr] * (d.bits / 8), arena + coff[rr] * (d.bits / 8), (size_t)nv * (d.bits / 8)); continue; }
        const int64_t W = nv / P;
        for (int pl = 0; pl < P; ++pl) for (int64_t x = 0; x < W; ++x) {
            const int64_t src = coff[rr] + x * cw + pl, dst = T->row_off[rr] + pl * W + x;
            if (d.bits == 16) ((int16_t *)T->planes)[dst] = ((const int16_t *)arena)[src];
            else ((int32_t *)T->planes)[dst] = ((const int32_t *)arena)[src];
        }
    }
}

void hook_lds_plan(const abpoa_hip_scoring_t *sc, int max_qlen, int max_bits, int n_aln, LdsPlan *L) {
    const int pn = max_bits == 16 ? 16 : 8; const int w = sc->wb + (int)(sc->wf * (float)max_qlen);
    make_lds_plan(sc, max_qlen, max_bits, band_cols(padded_width(max_qlen, pn), w, pn, true), n_aln, L);
}

}  // namespace abpoa_hip
