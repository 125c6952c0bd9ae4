// Which row loop takes an alignment -- narrow (dp_fast_rows.hip / poa_rounds.hip), wide (dp_wide_rows.hip / dp_xl_rows.hip), local (dp_local_rows.hip) or
// the general kernel -- and which arena format it writes.  Every routing condition is written here once: the kernels call the guards, the drivers and the plan
// (engine.cpp, msa_device.cpp, msa_device_plan.cpp) call the same functions on the host, and tests/device_plan.cpp ties the plan's job-level answers to the
// per-alignment rule.  Host and device code, no HIP runtime call.
#pragma once
#include "engine.h"

namespace abpoa_hip {

// ---- pieces: each condition appears in exactly one of them
// (Some are written as text, ROUTE_*, and the function of the same name wraps the text: the per-alignment rules and the kernels expand the text inside their one
//  && chain.  Called as functions there, the same conditions reach the optimizer grouped differently, and the kernels' code changes -- a few compares in another
//  order, then tens of thousands of lines of register allocation; the all-rounds kernel is sensitive to that, csrc/Makefile.  Host code calls the functions.)

// Which jobs / alignments the banded global row loops (rows_fast.h) take.
// (linear gaps, round 5: gap extension >= 1 -- the row arg-max is taken before the in-row scan -- and band half-widths of the narrow loop only: LINEAR_FAST_W; the
//  wide kernels have no linear form; local / band-less linear jobs stay with the general kernel)
constexpr int LINEAR_FAST_W = 40;      // = LdsPlan.wide_w_lo's default
__host__ __device__ inline bool fast_global_job(int gap_mode, int align_mode, int wb, int e1) {
    if (wb < 0) return false;
    if (gap_mode == ABPOA_HIP_LINEAR_GAP && e1 < 1) return false;
    return align_mode == ABPOA_HIP_GLOBAL_MODE || align_mode == ABPOA_HIP_EXTEND_MODE;
}
// band half-width for the choice of the row loop: half of a ragged set's extra columns (AlnDesc.pad0 = PoaSet.band_extra) counts as band; nothing else reads pad0
#define ROUTE_W(w, pad0) ((w) + ((pad0) >> 1))
__host__ __device__ inline int route_w(int w, int pad0) { return ROUTE_W(w, pad0); }
__host__ __device__ inline bool fast_global_aln(int gap_mode, int w, int pad0) { return gap_mode != ABPOA_HIP_LINEAR_GAP || ROUTE_W(w, pad0) < LINEAR_FAST_W; }
// the launch has a banded row loop and the query codes fit its LDS
#define ROUTE_FAST_LOOP_FITS(L, qlen) ((L).fr_cols > 0 && (qlen) <= (L).q_cap)
__host__ __device__ inline bool fast_loop_fits(const LdsPlan &L, int qlen) { return ROUTE_FAST_LOOP_FITS(L, qlen); }
// jobs of the local row loop (rows_local.h): local mode without a band, affine / convex gaps
#define ROUTE_LOCAL_LOOP_JOB(gap_mode, align_mode, wb) ((align_mode) == ABPOA_HIP_LOCAL_MODE && (wb) < 0 && (gap_mode) != ABPOA_HIP_LINEAR_GAP)
__host__ __device__ inline bool local_loop_job(int gap_mode, int align_mode, int wb) { return ROUTE_LOCAL_LOOP_JOB(gap_mode, align_mode, wb); }
// (int16 scores only: a local alignment of at most loc_cols columns cannot need more unless the matrix is extreme -- then the general kernel takes it)
#define ROUTE_LOCAL_LOOP_FITS(L, bits, qlen) ((L).loc_cols > 0 && (bits) == 16 && ((qlen) / 16 + 1) * 16 <= (L).loc_cols && (qlen) <= (L).q_cap)
__host__ __device__ inline bool local_loop_fits(const LdsPlan &L, int bits, int qlen) { return ROUTE_LOCAL_LOOP_FITS(L, bits, qlen); }
// band half-widths (route_w) of the wide row loop; wide_range_meets: some half-width of [w_min, w_top] is among them
#define ROUTE_IN_WIDE_RANGE(lo, hi, w) ((w) >= (lo) && (w) <= (hi))
__host__ __device__ inline bool in_wide_range(int lo, int hi, int w) { return ROUTE_IN_WIDE_RANGE(lo, hi, w); }
__host__ __device__ inline bool wide_range_meets(int lo, int hi, int w_min, int w_top) { return w_top >= lo && w_min <= hi; }
#define ROUTE_TAKES_WIDE_BAND(L, w) ((L).wide_on >= 1 && ROUTE_IN_WIDE_RANGE((L).wide_w_lo, (L).wide_w_hi, w))
__host__ __device__ inline bool takes_wide_band(const LdsPlan &L, int w) { return ROUTE_TAKES_WIDE_BAND(L, w); }
// direction words (dir_plane.h) instead of score records: dir_mode 1 = the narrow-band alignments of the launch, dir_mode 2 = the wide-band ones too
#define ROUTE_DIR_FOR(dir_mode, wide) ((dir_mode) == 2 || ((dir_mode) == 1 && !(wide)))
__host__ __device__ inline bool dir_for(int dir_mode, bool wide) { return ROUTE_DIR_FOR(dir_mode, wide); }

// ---- per alignment

__host__ __device__ __forceinline__ bool takes_fast(const DevBatch &b, const AlnDesc &d) {
    return fast_global_job(b.gap_mode, b.align_mode, b.wb, b.e1) && fast_global_aln(b.gap_mode, d.w, d.pad0) && (d.flags & ALN_FAST_OK) &&
           ROUTE_FAST_LOOP_FITS(b.lds, d.qlen) && !(b.dbg & DBG_NO_FAST_LOOPS);
}
// ... and among those, the ones whose rows are wide enough for the wide row loop (dp_wide_rows.hip); the rest take the narrow one
__host__ __device__ __forceinline__ bool takes_wide(const DevBatch &b, const AlnDesc &d) { return takes_wide_band(b.lds, ROUTE_W(d.w, d.pad0)); }
__host__ __device__ __forceinline__ bool takes_local(const DevBatch &b, const AlnDesc &d) {
    return ROUTE_LOCAL_LOOP_JOB(b.gap_mode, b.align_mode, b.wb) && (d.flags & ALN_FAST_OK) && ROUTE_LOCAL_LOOP_FITS(b.lds, d.bits, d.qlen) && !(b.dbg & DBG_NO_FAST_LOOPS);
}
// ... and which of the fast alignments write direction words instead of score records.
// (Measured on MI355X: on 1 kb reads the words cost the row loop 5-8 % and save 36-42 % of the backtrack, a net 8-11 %; on 10 kb reads the all-chunks
//  row loop loses 18-21 % -- more than the backtrack, a fifth of the time there, gains -- so wide-band alignments keep their records while the record
//  arenas of the job fit the device; the host picks mode 2 when they do not: an eighth of the arena bytes, twice the read-sets in flight.)
__host__ __device__ __forceinline__ bool takes_dir(const DevBatch &b, const AlnDesc &d) { return ROUTE_DIR_FOR(b.dir_mode, takes_wide(b, d)); }

// ---- one guard per kernel family (the kernels add their own test of the score width; where a guard has a text form the kernel expands that, see above)

#define ROUTE_FOR_WIDE_KERNEL(b, d) (takes_fast(b, d) && takes_wide(b, d))
#define ROUTE_FOR_TAIL_KERNEL(b, d) (takes_fast(b, d) || takes_local(b, d))
#define ROUTE_FOR_GENERAL_KERNEL(b, d) (!((d).flags & ALN_SKIP) && !takes_fast(b, d) && !takes_local(b, d))
__host__ __device__ inline bool for_narrow_kernel(const DevBatch &b, const AlnDesc &d) { return takes_fast(b, d) && !takes_wide(b, d); }
__host__ __device__ inline bool for_wide_kernel(const DevBatch &b, const AlnDesc &d) { return ROUTE_FOR_WIDE_KERNEL(b, d); }
__host__ __device__ __forceinline__ bool for_local_kernel(const DevBatch &b, const AlnDesc &d) { return takes_local(b, d); }
__host__ __device__ inline bool for_tail_kernel(const DevBatch &b, const AlnDesc &d) { return ROUTE_FOR_TAIL_KERNEL(b, d); }
__host__ __device__ inline bool for_general_kernel(const DevBatch &b, const AlnDesc &d) { return ROUTE_FOR_GENERAL_KERNEL(b, d); }
// the all-rounds kernel (poa_rounds.hip), whose jobs have no ragged set (pad0 = 0) and only reads of the narrow loop: anything else is flagged for the fall-back
#define ROUTE_ROUNDS_TAKES(b, flags, w) (((flags) & ALN_FAST_OK) && !ROUTE_TAKES_WIDE_BAND((b).lds, w))
__host__ __device__ inline bool rounds_takes(const DevBatch &b, int flags, int w) { return ROUTE_ROUNDS_TAKES(b, flags, w); }

// the job's scoring as the kernels read it
__host__ __device__ inline void set_job_fields(DevBatch &b, const abpoa_hip_scoring_t &sc) {
    b.o1 = sc.gap_open1; b.e1 = sc.gap_ext1; b.o2 = sc.gap_open2; b.e2 = sc.gap_ext2;
    b.align_mode = sc.align_mode; b.gap_mode = sc.gap_mode; b.wb = sc.wb; b.zdrop = sc.zdrop;
}

}  // namespace abpoa_hip
