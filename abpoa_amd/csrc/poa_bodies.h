// Bodies of the per-round graph kernels of the device-resident driver (poa_device.h): graph -> DP rows before the alignment of read k
// (poa_prepare_body) and graph cigar -> graph after it (poa_fuse_body).  One workgroup of GT threads owns one read-set.  Two users:
// poa_device.hip wraps each body in a kernel of its own (lock-step rounds: one launch per phase and round for all sets), poa_rounds.hip
// calls them from the kernel that takes a read-set through ALL its rounds.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include <string.h>
#include "poa_device.h"
#include "../../include/abpoa_hip.h"

namespace abpoa_hip {

namespace {      // (internal linkage: every translation unit that includes this header has its own copy)

__device__ __forceinline__ int imin_(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imax_(int a, int b) { return a > b ? a : b; }
// loads of data that OTHER lanes of this wave stored earlier in the same kernel: agent scope = not served from this CU's L1
__device__ __forceinline__ int ld_fresh(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// slot t of a node's edge lists (X = node0 + node id): the first POA_HOT slots are in the hot arrays, the next ones in the cold arrays; slots from the
// capacity on exist for the source's out-edges and the sink's in-edges only (PoaSet.term0: the set's slice of the terminal pools)
constexpr int POA_TERM_MAX = 250;      // edges of the source / into the sink at most (the counts are bytes)
__device__ __forceinline__ int32_t &in_slot(const PoaDev &p, const PoaSet &S, int64_t X, int t) {
    return t < POA_HOT ? p.nd_in[X * POA_HOT + t] : (t < p.in_cap ? p.nd_inx[X * (p.in_cap - POA_HOT) + t - POA_HOT] : p.t_in[S.term0 + t - p.in_cap]);
}
__device__ __forceinline__ int32_t &out_slot(const PoaDev &p, const PoaSet &S, int64_t X, int t) {
    return t < POA_HOT ? p.nd_out[X * POA_HOT + t] : (t < p.out_cap ? p.nd_outx[X * (p.out_cap - POA_HOT) + t - POA_HOT] : p.t_out[S.term0 + t - p.out_cap]);
}
__device__ __forceinline__ int32_t &outw_slot(const PoaDev &p, const PoaSet &S, int64_t X, int t) {
    return t < POA_HOT ? p.nd_outw[X * POA_HOT + t] : (t < p.out_cap ? p.nd_outwx[X * (p.out_cap - POA_HOT) + t - POA_HOT] : p.t_outw[S.term0 + t - p.out_cap]);
}
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }      // a value that is the same in every lane -> scalar register
__device__ __forceinline__ int shfl(int v, int src_lane) { return __builtin_amdgcn_ds_bpermute(src_lane << 2, v); }

template <int CTRL> __device__ __forceinline__ int dpp_(int old, int src) { return __builtin_amdgcn_update_dpp(old, src, CTRL, 0xF, 0xF, false); }
// inclusive prefix sum / max over the 64 lanes
__device__ __forceinline__ int wave_scan_add(int x) {
    x += dpp_<0x111>(0, x); x += dpp_<0x112>(0, x); x += dpp_<0x114>(0, x); x += dpp_<0x118>(0, x);
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xA, 0xF, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xC, 0xF, false);
    return x;
}
__device__ __forceinline__ int wave_scan_max(int x) {
    x = imax_(x, dpp_<0x111>(x, x)); x = imax_(x, dpp_<0x112>(x, x)); x = imax_(x, dpp_<0x114>(x, x)); x = imax_(x, dpp_<0x118>(x, x));
    x = imax_(x, __builtin_amdgcn_update_dpp(x, x, 0x142, 0xA, 0xF, false));
    x = imax_(x, __builtin_amdgcn_update_dpp(x, x, 0x143, 0xC, 0xF, false));
    return x;
}
// value of lane-1, lane 0 receives `lane0`

// reference src/simd_abpoa_align.c:1672-1683 (same arithmetic as abpoa_hip_score_bits in engine.cpp)
__device__ __forceinline__ int score_bits(const PoaDev &p, int n_rows, int qlen, int *inf_min) {
    const int oe1 = p.o1 + p.e1, oe2 = p.o2 + p.e2;
    const int len = qlen > n_rows ? qlen : n_rows;
    const int max_score = imax_(qlen * p.max_mat, len * p.e1 + p.o1);
    int bits, lo;
    if (max_score <= INT16_MAX - p.min_mis - oe1 - oe2) { bits = 16; lo = INT16_MIN; } else { bits = 32; lo = INT32_MIN; }
    *inf_min = imax_(imax_(lo + p.min_mis, lo + oe1), lo + oe2) + 31 * imax_(p.e1, p.e2);
    return bits;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// before the DP of round k: remaining length, rows in order with their predecessor CSR, alignment descriptor
// Four wavefronts per read-set: the row-parallel parts (heaviest edge, CSR) are latency-bound gathers, and four waves per SIMD hide
// most of that latency; the reverse sweep of the remaining length is sequential over 64-row blocks and runs on wavefront 0.
// workgroup size of the row-parallel graph kernels: 4 wavefronts per read-set (8 measured slower: the serial parts on wavefront 0 and the barriers dominate)
constexpr int GT = 256, GW = GT / 64;

__device__ __forceinline__ void poa_prepare_body(const PoaDev &p, const int s, const int k) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const PoaSet S = p.sets[s];
    PoaState *st = p.state + s;
    const int status = uni(st->status), n = uni(st->n_nodes);      // (wave-uniform; after a vector load when the state was written in this very kernel)
    // Early exit for sets that will outgrow their node slots: new nodes per read stay close to constant over the first reads
    // (most errors are novel), so ten reads predict the final size well; failing at once saves the rest of a doomed pass.
    // Read 5: a clear miss only (linear extrapolation 25 % over).  Read 10: a saturating growth model -- the nodes a read adds fall off as a / (1 + b k),
    // because its errors are more and more often ones the graph already holds (15 %-error 10 kb reads: 981 new nodes at read 5, 828 at read 10, 272 at
    // read 49; 5 %: 338, 331, 230) -- fitted to the mean gain of reads 3-6 and 7-10, summed over the remaining reads, +10 %.  (The linear test of round 2
    // projected 50 k nodes for graphs that end at 38.7 k and so sent every 15 % job to 6x node slots, twice the arena memory it needs.)
    bool doomed = false;
    // (not for read-sets with ragged ends, band_extra > 0: their first reads add nodes in bursts -- ends that reach beyond the graph -- and the projection sent a
    //  quarter of them through two more passes although they fit the first)
    if (status == POA_ST_OK && S.n_reads > 20 && !p.last_pass && S.band_extra == 0) {
        if (k == 2 && tid == 0) st->grow_n2 = n;
        if (k == 6 && tid == 0) st->grow_n6 = n;
        if (k == 5) {
            const int n0 = p.read_len[S.read0] + 2;
            const long long projected = (long long)n + (long long)(n - n0) * (S.n_reads - k) * 8 / (10 * k);
            doomed = projected * 4 > (long long)S.node_cap * 5;
        } else if (k == 10) {
            const int n2 = uni(st->grow_n2), n6 = uni(st->grow_n6);
            const float A = (float)(n6 - n2) * 0.25f, B = (float)(n - n6) * 0.25f;      // mean gain per read around read 4.5 / 8.5
            const float den = 8.5f * B - 4.5f * A;
            float bq = (A > B && den > 0.f) ? (A - B) / den : 0.f; bq = bq > 0.2f ? 0.2f : bq;
            const float a = A * (1.f + 4.5f * bq), N = (float)S.n_reads;
            const float rem = bq > 1e-4f ? (a / bq) * __logf((1.f + (N + 0.5f) * bq) / (1.f + 10.5f * bq)) : (A > B ? A : B) * (N - 10.f);
            doomed = (float)n + 1.1f * rem > (float)S.node_cap;
        }
        if (doomed && tid == 0) { st->status = POA_ST_FALLBACK; st->reason = POA_WHY_GROWTH; }
    }
    if (status != POA_ST_OK || doomed || k >= S.n_reads) {          // nothing to align for this set in this round: both DP kernels skip it
        if (tid == 0) { AlnDesc d; memset(&d, 0, sizeof(d)); d.n_rows = 3; d.bits = 16; d.flags = ALN_SKIP; p.aln[s] = d; p.out[s].status = 0; p.out[s].n_cigar = 0; p.out[s].n_cells = 0; }
        return;
    }
    const int64_t N0 = S.node0;
    const int32_t *order = p.row_node[uni(st->order_buf)] + N0;
    int32_t *nxt = p.scratch + S.scratch0;                 // [n] row of the heaviest successor
    int32_t *remain = p.row_remain + N0;
    // (1) heaviest out-edge per row (first maximum wins, reference :262-268)
    extern __shared__ unsigned jump_lds[];                 // [n] remaining-length jump records (see (2)), when the launch provides them
    const bool in_lds = p.lds_rows > 0 && n <= p.lds_rows;
    uint8_t *np_lds = (uint8_t *)(jump_lds + p.lds_rows);       // [n] in-degree per row (row 0: none), for (3)
    {
        // four rows per thread and pass, every load level issued for all four before the next one: the chain order -> node -> edge
        // slots -> row of the successor is four dependent HBM/L2 round trips, and a thread owns ~10 rows (150 on a 10 kb graph)
        for (int r0 = tid; r0 < n; r0 += 4 * GT) {
            int u[4], no[4], ni[4], bs[4], best[4], nx[4]; int4 w4[4], o4[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) { const int r = r0 + j * GT; u[j] = order[r < n ? r : 0]; }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t X = N0 + u[j];
                no[j] = p.nd_nout[X]; ni[j] = p.nd_nin[X]; bs[j] = p.nd_base[X];
                w4[j] = *(const int4 *)(p.nd_outw + X * POA_HOT); o4[j] = *(const int4 *)(p.nd_out + X * POA_HOT);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                int bw = -1, bb = -1;
                if (no[j] > 0 && w4[j].x > bw) { bw = w4[j].x; bb = o4[j].x; }
                if (no[j] > 1 && w4[j].y > bw) { bw = w4[j].y; bb = o4[j].y; }
                if (no[j] > 2 && w4[j].z > bw) { bw = w4[j].z; bb = o4[j].z; }
                if (no[j] > 3 && w4[j].w > bw) { bw = w4[j].w; bb = o4[j].w; }
                for (int t = POA_HOT; t < no[j]; ++t) { const int w = outw_slot(p, S, N0 + u[j], t); if (w > bw) { bw = w; bb = out_slot(p, S, N0 + u[j], t); } }
                best[j] = bb;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) nx[j] = best[j] >= 0 ? p.nd_row[N0 + best[j]] : -1;
            // how far down the row order the row's scores are still needed (DevBatch.row_sdist): the row of every out-edge (one more load per edge, same level as nx)
            int sd[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r = r0 + j * GT; int far = 0;
                if (no[j] == 1) far = nx[j];
                else {
                    int rr[4] = {0, 0, 0, 0};
                    if (no[j] > 0) rr[0] = p.nd_row[N0 + o4[j].x]; if (no[j] > 1) rr[1] = p.nd_row[N0 + o4[j].y]; if (no[j] > 2) rr[2] = p.nd_row[N0 + o4[j].z];
                    if (no[j] > 3) rr[3] = p.nd_row[N0 + o4[j].w];
                    far = imax_(imax_(rr[0], rr[1]), imax_(rr[2], rr[3]));
                    for (int t = POA_HOT; t < no[j]; ++t) far = imax_(far, p.nd_row[N0 + out_slot(p, S, N0 + u[j], t)]);
                }
                sd[j] = far >= n - 1 ? 255 : imin_(imax_(far - r, 0), 255);      // (the sink is the last row)
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r = r0 + j * GT;
                if (r < n) {
                    p.row_sdist[N0 + r] = (uint8_t)sd[j];
                    if (in_lds) { jump_lds[r] = nx[j] >= 0 ? ((unsigned)nx[j] << 16) | 1u : ((unsigned)r << 16); np_lds[r] = (uint8_t)(r > 0 ? ni[j] : 0); }
                    else nxt[r] = nx[j];
                    p.row_base[N0 + r] = (uint8_t)bs[j]; p.row_node_id[N0 + r] = u[j];
                }
            }
        }
    }
    __syncthreads();
    // (2) remaining length = (edges to the sink along heaviest successors) - 1, reference :233-274 (only the adaptive band reads it: abpoa_graph.c:303-311)
    if (!p.banded) { for (int r = tid; r < n; r += GT) remain[r] = 0; }
    else if (in_lds) {
        // Pointer jumping over all rows at once in LDS.  A record "row of a later node on the chain << 16 | edges up to it" is one
        // 32-bit word, so a row may read a neighbour's record while that neighbour is being advanced: either version is a valid jump.
        for (int span = 1; span < n; span <<= 1) {
            for (int r = tid; r < n; r += GT) {
                const unsigned w = jump_lds[r]; const int t = (int)(w >> 16);
                if (t != r) { const unsigned wt = jump_lds[t]; jump_lds[r] = (wt & 0xffff0000u) | ((w & 0xffffu) + (wt & 0xffffu)); }
            }
            __syncthreads();
        }
        for (int r = tid; r < n; r += GT) remain[r] = (int)(jump_lds[r] & 0xffffu) - 1;
    } else
    // (graphs too large for the LDS records) reverse sweep over 64-row blocks; inside a block the chains are resolved by pointer jumping.  The sweep is a
    // chain over the blocks, so what a block costs is what counts (600 blocks for a 10 kb graph): the successor rows of the NEXT block are loaded while
    // this one is resolved, and the values of the block above stay in a register -- a heaviest successor is almost always within the next few rows -- so
    // that only a target further than 64 rows beyond the block goes to memory (and waits for this wave's stores).
    if (wave == 0) {
        int t0 = ((n - 1) >> 6) << 6;
        int tgt_next = t0 + lane < n ? ld_fresh(nxt + t0 + lane) : -1, above = 0;      // above: values of block t0 + 64 (lane = row - t0 - 64)
        for (; t0 >= 0; t0 -= 64) {
            const int r = t0 + lane;
            int tgt = tgt_next, dist = 1, val = 0; bool done = r >= n;
            if (t0 >= 64) tgt_next = ld_fresh(nxt + t0 - 64 + lane);
            if (!done && tgt < 0) { val = -1; done = true; }                         // the sink (reference :247)
            const bool far = !done && tgt >= t0 + 128;
            const int from_above = shfl(above, (tgt - t0 - 64) & 63);
            if (!done && tgt >= t0 + 64 && !far) { val = from_above + 1; done = true; }
            if (__any(far)) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // stores are write-through: once acknowledged, later blocks read them from L2 (ld_fresh)
                if (far) { val = ld_fresh(remain + tgt) + 1; done = true; }
            }
#pragma unroll
            for (int it = 0; it < 6; ++it) {
                const int src = (!done) ? tgt - t0 : lane;
                const int t_tgt = shfl(tgt, src), t_dist = shfl(dist, src), t_val = shfl(val, src), t_done = shfl((int)done, src);
                if (!done) {
                    if (t_done) { val = t_val + dist; done = true; }
                    else { tgt = t_tgt; dist += t_dist; }
                }
            }
            if (r < n) remain[r] = val;
            above = val;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    // (3) predecessor CSR in row order (in_id order kept, reference pre_index[][] :519-530)
    __shared__ int wtot[GW];
    int carry = 0; bool overflow = false;
    for (int t0 = 0; t0 < n; t0 += GT) {
        const int r = t0 + tid;
        const int u = (r < n && !in_lds) ? order[r] : 0;
        const int np = r < n ? (in_lds ? (int)np_lds[r] : (r > 0 ? (int)p.nd_nin[N0 + u] : 0)) : 0;
        const int incl = wave_scan_add(np);
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w_ = 0; w_ < GW; ++w_) { const int x_ = wtot[w_]; all += x_; before += w_ < wave ? x_ : 0; }
        const int off = carry + before + incl - np;
        if (r < n) p.pred_off[N0 + r] = off;
        if (off + np > S.pred_cap) overflow = true;
        carry += all;
        __syncthreads();
    }
    {      // the lists themselves, four rows per thread and pass (see (1)); pred_off is read back by the thread that wrote it
        for (int r0 = tid; r0 < n; r0 += 4 * GT) {
            int u[4], np[4], off[4]; int4 i4[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) { const int r = r0 + j * GT; const bool ok = r < n; u[j] = order[ok ? r : 0]; off[j] = p.pred_off[N0 + (ok ? r : 0)];
                                          np[j] = !ok ? 0 : (in_lds ? (int)np_lds[r] : (r > 0 ? (int)p.nd_nin[N0 + u[j]] : 0)); }
#pragma unroll
            for (int j = 0; j < 4; ++j) { if (off[j] + np[j] > S.pred_cap) np[j] = 0; i4[j] = *(const int4 *)(p.nd_in + (N0 + u[j]) * POA_HOT); }
            int pr[4][4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                pr[j][0] = np[j] > 0 ? p.nd_row[N0 + i4[j].x] : 0; pr[j][1] = np[j] > 1 ? p.nd_row[N0 + i4[j].y] : 0;
                pr[j][2] = np[j] > 2 ? p.nd_row[N0 + i4[j].z] : 0; pr[j][3] = np[j] > 3 ? p.nd_row[N0 + i4[j].w] : 0;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                int32_t *dst = p.pred_row + S.pred0 + off[j];
                const int r = r0 + j * GT;      // (np[j] is 0 for a row whose list does not fit: the set falls back anyway)
                unsigned long long pdv = ~0ull;      // a byte per predecessor (the first eight), 255 = none / further than 254 rows
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    if (t < np[j]) { dst[t] = pr[j][t]; if (r - pr[j][t] <= 254) pdv = (pdv & ~(0xffull << (8 * t))) | ((unsigned long long)(r - pr[j][t]) << (8 * t)); }
                }
                for (int t = POA_HOT; t < np[j]; ++t) { const int pr_ = p.nd_row[N0 + in_slot(p, S, N0 + u[j], t)]; dst[t] = pr_;
                        if (t < 8 && r - pr_ <= 254) pdv = (pdv & ~(0xffull << (8 * t))) | ((unsigned long long)(r - pr_) << (8 * t)); }
                if (r < n) { p.row_pd[2 * (N0 + r)] = (unsigned)pdv; p.row_pd[2 * (N0 + r) + 1] = (unsigned)(pdv >> 32); }
            }
        }
    }
    if (tid == 0) p.pred_off[N0 + n] = carry;
    if (p.out_off) {      // (3b) successor rows per row, out_id order: the general kernel hands a row's arg-max to its successors' band state (reference :1078-1091)
        int carry_o = 0;
        for (int t0 = 0; t0 < n; t0 += GT) {
            const int r = t0 + tid;
            const int u = r < n ? order[r] : 0;
            const int no = r < n ? (int)p.nd_nout[N0 + u] : 0;
            const int incl = wave_scan_add(no);
            __syncthreads();
            if (lane == 63) wtot[wave] = incl;
            __syncthreads();
            int before = 0, all = 0;
#pragma unroll
            for (int w_ = 0; w_ < GW; ++w_) { const int x_ = wtot[w_]; all += x_; before += w_ < wave ? x_ : 0; }
            const int off = carry_o + before + incl - no;
            if (r < n) {
                p.out_off[N0 + r] = off;
                if (off + no > S.pred_cap) overflow = true;
                else for (int t = 0; t < no; ++t) p.out_row[S.pred0 + off + t] = p.nd_row[N0 + out_slot(p, S, N0 + u, t)];
            }
            carry_o += all;
        }
        if (tid == 0) p.out_off[N0 + n] = carry_o;
    }
    overflow = __syncthreads_or(overflow);
    // (4) alignment descriptor of this round
    if (tid == 0) {
        AlnDesc d; memset(&d, 0, sizeof(d));
        const int qlen = p.read_len[S.read0 + k];
        d.n_rows = n; d.qlen = qlen;
        d.bits = score_bits(p, n, qlen, &d.inf_min);
        d.w = p.wb < 0 ? qlen : p.wb + (int)(p.wf * (float)qlen);            // reference :445 (float32 product)
        d.cigar_cap = S.cigar_cap; d.flags = (p.general & 1) ? 0 : ALN_FAST_OK; d.pad0 = S.band_extra;
        d.query_off = p.read_off[S.read0 + k]; d.row0 = N0; d.poff0 = N0; d.pred0 = S.pred0; d.out0 = S.pred0;
        d.plane_off = S.plane_off; d.plane_cap = S.plane_cap / (d.bits / 8); d.cigar_off = S.cigar_off;
        if (overflow || n + qlen + 8 > S.cigar_cap) { st->status = POA_ST_FALLBACK; st->reason = overflow ? POA_WHY_PRED_SLOTS : POA_WHY_CIGAR_SLOTS; d.flags = ALN_SKIP; d.n_rows = 3; }
        p.aln[s] = d;
        p.out[s].status = 0; p.out[s].n_cigar = 0; p.out[s].n_cells = 0;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// after the backtrack of round k: fuse the graph cigar of read k into the graph and extend the row order
// Four wavefronts per read-set; the walk over the query (F2) takes 4 GT positions per super-pass.
__device__ __forceinline__ void poa_fuse_body(const PoaDev &p, const int s, const int k) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ int wtot[GW];
    const PoaSet S = p.sets[s];
    PoaState *st = p.state + s;
    if (uni(st->status) != POA_ST_OK || k >= S.n_reads) return;
    AlnOut res = p.out[s]; res.status = uni(res.status); res.n_cigar = uni(res.n_cigar);
    if (res.status != 0) { if (tid == 0) { st->status = POA_ST_FALLBACK; st->reason = POA_WHY_DP_STATUS + res.status; } return; }
    const int64_t N0 = S.node0;
    const int n_old = uni(st->n_nodes), qlen = p.read_len[S.read0 + k], n_cigar = res.n_cigar;
    const bool rc_read = p.is_rc && uni((int)p.is_rc[S.read0 + k]) != 0;      // (-s: the reverse complement of this read won, reference :331-334)
    const uint8_t *seq = (rc_read ? p.reads_rc : p.reads) + p.read_off[S.read0 + k];
    const uint64_t *cg = p.cigar + S.cigar_off;
    const int cur = uni(st->order_buf);
    const int32_t *order_old = p.row_node[cur] + N0; int32_t *order_new = p.row_node[cur ^ 1] + N0;
    int32_t *cand = p.scratch + S.scratch0, *n_anchor = cand + p.max_qlen, *n_j = n_anchor + p.max_qlen, *addcnt = n_j + p.max_qlen;
    if (p.dig_on) {      // (tests) this alignment's cigar into the set's digest -- before the early return: an empty cigar is a cigar too
        __shared__ unsigned long long sh_dig;
        if (tid == 0) sh_dig = 0;
        __syncthreads();
        unsigned long long part = 0;
        for (int i = tid; i < n_cigar; i += GT) part += poa_cigar_word_mix(cg[i], i);
        if (part) atomicAdd(&sh_dig, part);
        __syncthreads();
        if (tid == 0) st->cigar_dig = poa_cigar_digest_round(st->cigar_dig, k, n_cigar, sh_dig);
    }
    if (n_cigar == 0) return;                                                   // reference :614-616
    // F0/F1: node every query base is aligned to (-1: inserted base)
    for (int q = tid; q < qlen; q += GT) cand[q] = -1;
    for (int r = tid; r < n_old; r += GT) addcnt[r] = 0;
    __syncthreads();
    for (int i = tid; i < n_cigar; i += GT) {
        const uint64_t w = cg[i];
        if ((int)(w & 0xf) == ABPOA_HIP_CMATCH) cand[(int)((w >> 4) & 0x3fffffff)] = (int)((w >> 34) & 0x3fffffff);
    }
    __syncthreads();
    // F2: walk the query in super-passes of FP * GT positions, thread t owning the FP consecutive positions q0 + FP t ...
    int n_nodes = n_old, prev_c = 0 /* source */, prev_new_c = 0, carry_ar = 0 /* row of the source */, carry_sq = -1;
    bool fail = false, fail_slots = false;      // (fail_slots: an edge / aligned list is full -- more node slots would not help, POA_WHY_EDGE_SLOTS)
    // per-base weights of this read (-Q), reference :634-667: an edge takes the weight of the base it leads to
    const int32_t *wq = p.wts ? (rc_read ? p.wts_rc : p.wts) + p.read_off[S.read0 + k] : nullptr;
    // (the source may have any number of out-edges, the sink of in-edges: reads that start / end on different nodes; PoaSet.term0)
    const int out_lim0 = imin_(POA_TERM_MAX, p.out_cap + S.n_reads + 2), in_lim1 = imin_(POA_TERM_MAX, p.in_cap + S.n_reads + 2);
    // The walk is a chain of dependent gathers (cigar -> node -> aligned group -> its members; edge lists of the previous node), each an L2 / HBM round trip
    // of ~2 k ticks, so as in poa_prepare_body every load level is issued for all FP positions of a thread before anything waits on the level above, and a
    // 1 kb read is one super-pass.  Per-position work is private to its thread (the nodes of a path, and their aligned groups, are distinct); what flows
    // along the path -- new-node ids, the previous node, the running maxima AR / sq -- is handed on inside the thread, then by a wave scan, then through
    // LDS: two workgroup barriers per super-pass.  A wavefront holds FP * 64 = 256 consecutive positions.
    constexpr int FP = 4, FA = 3;      // FA: members of an aligned group whose loads are batched (a full A/C/G/T group has three besides the node itself)
    __shared__ int sCnt[GW], sMax[GW], sSqm[GW], sPrev[2];
    int *const sLast = wtot;               // (wtot is F4's)
    for (int q0 = 0; q0 < qlen; q0 += FP * GT) {
        const int qb = q0 + FP * tid;
        bool act[FP]; int c[FP], b[FP], cb[FP], na[FP], gv[FP], am[FP][FA], ab[FP][FA], ar[FP][FA];
        // level 1: the node each position is aligned to, and its base
#pragma unroll
        for (int j = 0; j < FP; ++j) { act[j] = qb + j < qlen; c[j] = act[j] ? ld_fresh(cand + qb + j) : -1; b[j] = act[j] ? (int)seq[qb + j] : 0; }
        // level 2: that node's base, group size and row (positions without a node read the source's: no branch between the loads)
        bool any_grp = false;
#pragma unroll
        for (int j = 0; j < FP; ++j) {
            const bool h = c[j] >= 0; const int64_t X = N0 + (h ? c[j] : 0);
            cb[j] = p.nd_base[X]; na[j] = h ? (int)p.nd_naln[X] : 0; gv[j] = h ? p.nd_row[X] : -1;
            any_grp |= na[j] > 0;
        }
        // levels 3 and 4: the first FA members of its aligned group, then their bases and rows
        if (__any(any_grp)) {
#pragma unroll
            for (int j = 0; j < FP; ++j)
#pragma unroll
                for (int t = 0; t < FA; ++t) { const bool h = t < na[j]; am[j][t] = p.nd_aln[(N0 + (h ? c[j] : 0)) * p.aln_cap + (h ? t : 0)]; }
#pragma unroll
            for (int j = 0; j < FP; ++j)
#pragma unroll
                for (int t = 0; t < FA; ++t) { const int64_t X = N0 + (t < na[j] ? am[j][t] : 0); ab[j][t] = p.nd_base[X]; ar[j][t] = p.nd_row[X]; }
        } else {
#pragma unroll
            for (int j = 0; j < FP; ++j)
#pragma unroll
                for (int t = 0; t < FA; ++t) { am[j][t] = 0; ab[j][t] = 0; ar[j][t] = 0; }
        }
        // the node of every position: the aligned node or the first member of its group with the read's base (reference abpoa_get_aligned_id :377-386),
        // else a new one.  gv: the group-end row that places the position in the row order (see the bookkeeping below) -- the last row of the aligned
        // node's group, which is also the group of the member that matched; read before the group is extended.
        int node[FP]; bool isnew[FP];
#pragma unroll
        for (int j = 0; j < FP; ++j) {
            node[j] = -1; isnew[j] = act[j];
            if (act[j] && c[j] >= 0) {
                if (cb[j] == b[j]) { node[j] = c[j]; isnew[j] = false; }
#pragma unroll
                for (int t = 0; t < FA; ++t) if (t < na[j]) { if (isnew[j] && ab[j][t] == b[j]) { node[j] = am[j][t]; isnew[j] = false; } gv[j] = imax_(gv[j], ar[j][t]); }
                for (int t = FA; t < na[j]; ++t) {      // (alphabets with more than four letters)
                    const int a = p.nd_aln[(N0 + c[j]) * p.aln_cap + t];
                    if (isnew[j] && (int)p.nd_base[N0 + a] == b[j]) { node[j] = a; isnew[j] = false; }
                    gv[j] = imax_(gv[j], p.nd_row[N0 + a]);
                }
            }
        }
        // exchange 1: new nodes and group-end rows before this thread (ids of the new nodes in path order, running maximum AR), and the last
        // position of the thread before (an old node's id, -1 for a new node: its id follows from the counts)
        int cnt = 0, gm = -1;
#pragma unroll
        for (int j = 0; j < FP; ++j) { cnt += isnew[j] ? 1 : 0; gm = imax_(gm, gv[j]); }
        const int icnt = wave_scan_add(cnt), imax = wave_scan_max(gm), lastnode = isnew[FP - 1] ? -1 : node[FP - 1];
        const int pl = (lane - 1) & 63;
        const int p_node = shfl(lastnode, pl), p_icnt = shfl(icnt, pl), p_imax = shfl(imax, pl);
        if (lane == 63) { sCnt[wave] = icnt; sMax[wave] = imax; sLast[wave] = lastnode; }
        __syncthreads();
        // The node slots are tested per super-pass; a wavefront's 256 positions are what one pass of the walk used to be, and as then the positions up
        // to the first 256 that do not fit still put their nodes and edges in (an edge list that is full among them is the reason reported).
        int before_cnt = 0, n_new = 0, before_max = carry_ar, all_max = carry_ar, wfail = GW;
#pragma unroll
        for (int w_ = 0; w_ < GW; ++w_) {
            const int x_ = sCnt[w_], m_ = sMax[w_];
            if (w_ < wave) { before_cnt += x_; before_max = imax_(before_max, m_); }
            n_new += x_; all_max = imax_(all_max, m_);
            if (wfail == GW && n_nodes + n_new > S.node_cap) wfail = w_;
        }
        const bool live = wave < wfail;
        // row-order bookkeeping.  Invariant (the reference's Kahn walk keeps it too, abpoa_graph.c:213-224): the members of an
        // aligned group are contiguous in the row order.  A new node is therefore spliced in right after the END of a group:
        // the group of the node it mismatches (which it joins), or the group of the nearest old node before it on the path,
        // whichever comes later -- i.e. after row AR = running maximum along the path of "group-end row" (old nodes: their own
        // group; mismatch nodes: the group they join; inserted bases: none).  New nodes with the same AR form a run in path order.
        int AR[FP], pv[FP]; bool pvn[FP], start[FP];
        int sqt = -1;
        {
            const int ex_cnt = lane ? p_icnt : 0;
            int run = imax_(before_max, lane ? p_imax : -1), id = n_nodes + before_cnt + ex_cnt;
            int prv = tid == 0 ? prev_c : (lane ? p_node : sLast[wave ? wave - 1 : 0]);
            bool prvn = tid == 0 ? prev_new_c != 0 : prv < 0;
            if (tid != 0 && prvn) prv = id - 1;
#pragma unroll
            for (int j = 0; j < FP; ++j) {
                pv[j] = prv; pvn[j] = prvn;
                const int pAR = run;
                run = imax_(run, gv[j]); AR[j] = run;
                if (isnew[j]) node[j] = id++;
                start[j] = isnew[j] && (!prvn || pAR != run);      // a run of new nodes starts here
                if (start[j]) sqt = qb + j;
                prv = node[j]; prvn = isnew[j];
            }
        }
        const int isq = wave_scan_max(sqt), p_isq = shfl(isq, pl);
        if (lane == 63) sSqm[wave] = isq;
        {      // carries into the next super-pass: the last position
            const int qlast = imin_(q0 + FP * GT, qlen) - 1;
#pragma unroll
            for (int j = 0; j < FP; ++j) if (qb + j == qlast) { sPrev[0] = node[j]; sPrev[1] = (int)isnew[j]; }
        }
        // the new nodes; a mismatch node joins the group of the node it is aligned to, reference :393-401
#pragma unroll
        for (int j = 0; j < FP; ++j) if (live && isnew[j]) {
            const int64_t Y = N0 + node[j], C = N0 + c[j];
            p.nd_base[Y] = (uint8_t)b[j]; p.nd_nin[Y] = 0; p.nd_nout[Y] = 0; p.nd_naln[Y] = 0; p.nd_nread[Y] = 0;
            if (c[j] >= 0) {
                const int na_ = na[j];      // (every member of a group lists all the others: the same count in each)
                if (na_ + 1 > p.aln_cap) { fail = true; fail_slots = true; }
                else {
#pragma unroll
                    for (int t = 0; t < FA; ++t) if (t < na_) {
                        const int other = am[j][t];
                        p.nd_aln[(N0 + other) * p.aln_cap + na_] = node[j]; p.nd_naln[N0 + other] = (uint8_t)(na_ + 1); p.nd_aln[Y * p.aln_cap + t] = other;
                    }
                    for (int t = FA; t < na_; ++t) {
                        const int other = p.nd_aln[C * p.aln_cap + t];
                        p.nd_aln[(N0 + other) * p.aln_cap + na_] = node[j]; p.nd_naln[N0 + other] = (uint8_t)(na_ + 1); p.nd_aln[Y * p.aln_cap + t] = other;
                    }
                    p.nd_aln[C * p.aln_cap + na_] = node[j]; p.nd_naln[C] = (uint8_t)(na_ + 1);
                    p.nd_aln[Y * p.aln_cap + na_] = c[j]; p.nd_naln[Y] = (uint8_t)(na_ + 1);
                }
            }
        }
        // the edges previous node -> node (a node created by this read has no edges but the ones this very walk gives it, which is known without a
        // load): counts, hot out-slots and read count of the old nodes for all FP edges, issued here so that they travel with the stores above
        bool ea[FP]; int ew[FP], no[FP], ni[FP], nr[FP]; int4 o4[FP];
#pragma unroll
        for (int j = 0; j < FP; ++j) {
            ea[j] = live && act[j];
            const int64_t F = N0 + ((ea[j] && !pvn[j]) ? pv[j] : 0), T = N0 + ((ea[j] && !isnew[j]) ? node[j] : 0);
            ew[j] = (wq && act[j]) ? wq[qb + j] : 1;
            no[j] = p.nd_nout[F]; ni[j] = p.nd_nin[T]; nr[j] = p.nd_nread[F]; o4[j] = *(const int4 *)(p.nd_out + F * POA_HOT);
        }
        // exchange 2: where the run of new nodes a position is in began.  The barrier also orders the new nodes' initialisation above before the
        // edge updates below.
        __syncthreads();
        int sq = imax_(carry_sq, lane ? p_isq : -1), sq_all = carry_sq;
#pragma unroll
        for (int w_ = 0; w_ < GW; ++w_) { const int x_ = sSqm[w_]; sq_all = imax_(sq_all, x_); if (w_ < wave) sq = imax_(sq, x_); }
#pragma unroll
        for (int j = 0; j < FP; ++j) {
            if (start[j]) sq = qb + j;
            if (live && isnew[j]) { n_anchor[node[j] - n_old] = AR[j]; n_j[node[j] - n_old] = qb + j - sq + 1; atomicAdd(addcnt + AR[j], 1); }
        }
        // the edges: which exist (the cold slots only for a node with more than POA_HOT out-edges), then their weights, then the new ones
        int hit[FP], ow[FP]; int32_t *wp[FP];
#pragma unroll
        for (int j = 0; j < FP; ++j) {
            if (pvn[j]) { no[j] = 0; nr[j] = 0; }
            if (isnew[j]) ni[j] = 0;
            hit[j] = -1;
            if (ea[j] && !pvn[j] && !isnew[j]) {
                const int to = node[j];
                if (no[j] > 0 && o4[j].x == to) hit[j] = 0;
                else if (no[j] > 1 && o4[j].y == to) hit[j] = 1;
                else if (no[j] > 2 && o4[j].z == to) hit[j] = 2;
                else if (no[j] > 3 && o4[j].w == to) hit[j] = 3;
                else for (int t = POA_HOT; t < no[j]; ++t) if (out_slot(p, S, N0 + pv[j], t) == to) { hit[j] = t; break; }
            }
            wp[j] = hit[j] >= 0 ? &outw_slot(p, S, N0 + pv[j], hit[j]) : p.nd_outw + N0 * POA_HOT;
        }
#pragma unroll
        for (int j = 0; j < FP; ++j) ow[j] = *wp[j];
#pragma unroll
        for (int j = 0; j < FP; ++j) if (ea[j]) {
            const int from = pv[j], to = node[j];
            const int64_t F = N0 + from, T = N0 + to;
            if (hit[j] >= 0) *wp[j] = ow[j] + ew[j];
            else {
                if (no[j] >= (from == 0 ? out_lim0 : p.out_cap) || ni[j] >= (to == 1 ? in_lim1 : p.in_cap)) { fail = true; fail_slots = true; continue; }
                out_slot(p, S, F, no[j]) = to; outw_slot(p, S, F, no[j]) = ew[j]; p.nd_nout[F] = (uint8_t)(no[j] + 1);
                in_slot(p, S, T, ni[j]) = from; p.nd_nin[T] = (uint8_t)(ni[j] + 1);
                hit[j] = no[j];
                // (a new edge: no read went through it yet.  The source's edges beyond the capacity keep no read ids: nothing reads the source's -- the MSA rows
                //  come from the out-edges of nodes 2.., reference abpoa_output.c:142-150)
                if (hit[j] < p.out_cap) for (int w_ = 0; w_ < p.rid_words; ++w_) p.nd_rid[(F * p.out_cap + hit[j]) * p.rid_words + w_] = 0;
            }
            // read k went through this edge (reference :453-472; a node is the tail of at most one edge per read, so no other lane touches these words)
            if (p.rid_words && hit[j] < p.out_cap) p.nd_rid[(F * p.out_cap + hit[j]) * p.rid_words + (k >> 6)] |= 1ull << (k & 63);
            p.nd_nread[F] = nr[j] + 1;
        }
        if (wfail < GW) { fail = true; break; }                                  // (the same in every thread)
        prev_c = sPrev[0]; prev_new_c = sPrev[1]; carry_ar = all_max; carry_sq = sq_all; n_nodes += n_new;
    }
    // F3: last node -> sink (reference :667: the last base's weight), on thread 0.  Nothing in the walk touched the last node's out-list or the
    // sink's in-list, so their loads are issued ahead of the barrier that waits for the walk's stores.
    int f3_no = 0, f3_ni = 0, f3_nr = 0; int4 f3_o4 = make_int4(0, 0, 0, 0);
    if (tid == 0) {
        const int64_t F = N0 + (prev_new_c ? 0 : prev_c);
        f3_no = p.nd_nout[F]; f3_ni = p.nd_nin[N0 + 1]; f3_nr = p.nd_nread[F]; f3_o4 = *(const int4 *)(p.nd_out + F * POA_HOT);
    }
    bool any_fail = __syncthreads_or(fail);
    if (!any_fail) {
        if (tid == 0) {
            const int from = prev_c, w = wq ? wq[qlen - 1] : 1;
            const bool from_new = prev_new_c != 0;
            const int64_t F = N0 + from, T = N0 + 1;
            const int no = from_new ? 0 : f3_no, ni = f3_ni;
            int hit = -1;
            if (no > 0 && f3_o4.x == 1) hit = 0;
            else if (no > 1 && f3_o4.y == 1) hit = 1;
            else if (no > 2 && f3_o4.z == 1) hit = 2;
            else if (no > 3 && f3_o4.w == 1) hit = 3;
            else for (int t = POA_HOT; t < no; ++t) if (out_slot(p, S, F, t) == 1) { hit = t; break; }
            bool ok = true;
            if (hit >= 0) outw_slot(p, S, F, hit) += w;
            else if (no >= (from == 0 ? out_lim0 : p.out_cap) || ni >= in_lim1) { fail = true; fail_slots = true; ok = false; }
            else {
                out_slot(p, S, F, no) = 1; outw_slot(p, S, F, no) = w; p.nd_nout[F] = (uint8_t)(no + 1);
                in_slot(p, S, T, ni) = from; p.nd_nin[T] = (uint8_t)(ni + 1);
                hit = no;
                if (hit < p.out_cap) for (int w_ = 0; w_ < p.rid_words; ++w_) p.nd_rid[(F * p.out_cap + hit) * p.rid_words + w_] = 0;
            }
            if (ok) {
                if (p.rid_words && hit < p.out_cap) p.nd_rid[(F * p.out_cap + hit) * p.rid_words + (k >> 6)] |= 1ull << (k & 63);
                p.nd_nread[F] = (from_new ? 0 : f3_nr) + 1;
            }
        }
        any_fail = __syncthreads_or(fail);
    }
    const bool any_slots = __syncthreads_or(fail_slots);
    if (any_fail) { if (tid == 0) { st->status = POA_ST_FALLBACK; st->reason = any_slots ? POA_WHY_EDGE_SLOTS : POA_WHY_NODES_IN_FUSE; } return; }
    // F4: new row order = old order with every run of new nodes spliced in after its anchor.  FR consecutive rows per thread, their counts and nodes
    // loaded before the scan: one workgroup scan per FR * GT rows (the graph of a 1 kb read-set: one or two).  The anchors of the first GT new nodes
    // are loaded ahead of it: they wait for nothing F4 writes.
    constexpr int FR = 8;
    const int n_add = n_nodes - n_old;
    int pl_ar = 0, pl_j = 0;
    if (tid < n_add) { pl_ar = ld_fresh(n_anchor + tid); pl_j = ld_fresh(n_j + tid); }
    int carry = 0;
    for (int r0 = 0; r0 < n_old; r0 += FR * GT) {
        const int rb = r0 + FR * tid;
        int cn[FR], u[FR], tot = 0;
#pragma unroll
        for (int j = 0; j < FR; ++j) { const bool ok = rb + j < n_old; cn[j] = ok ? ld_fresh(addcnt + rb + j) : 0; u[j] = order_old[ok ? rb + j : 0]; }
#pragma unroll
        for (int j = 0; j < FR; ++j) tot += cn[j];
        const int incl = wave_scan_add(tot);
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w_ = 0; w_ < GW; ++w_) { const int x_ = wtot[w_]; all += x_; before += w_ < wave ? x_ : 0; }
        int shift = carry + before + incl - tot;            // new nodes anchored at earlier rows
#pragma unroll
        for (int j = 0; j < FR; ++j) {
            const int r = rb + j;
            if (r < n_old) { order_new[r + shift] = u[j]; p.nd_row[N0 + u[j]] = r + shift; addcnt[r] = shift; }
            shift += cn[j];
        }
        carry += all;
        __syncthreads();
    }
    for (int i = tid; i < n_add; i += GT) {
        const int ar = i < GT ? pl_ar : ld_fresh(n_anchor + i), j = i < GT ? pl_j : ld_fresh(n_j + i);
        const int nr = ar + ld_fresh(addcnt + ar) + j;
        order_new[nr] = n_old + i; p.nd_row[N0 + n_old + i] = nr;
    }
    if (tid == 0) {
        st->n_nodes = n_nodes; st->order_buf = cur ^ 1; st->n_cells += res.n_cells;
        st->algo_bytes += res.n_cells * (p.aln[s].bits / 8) * (p.gap_mode == ABPOA_HIP_AFFINE_GAP ? 5 : 8);
    }
}

}  // namespace abpoa_hip
