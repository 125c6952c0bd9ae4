// The kernels' diagnostic channel, defined once for kernels, drivers and host-only test programs ("Diagnostics"):
//   * the bits of ABPOA_HIP_DBG (DevBatch.dbg),
//   * the macros of the diagnostic builds (`make prof`, `make census`, `make counters`, -DABPOA_HIP_PROFILE),
//   * the layouts of AlnOut.seg[] (and of the fseg[] that feeds it) with the packings of their words,
//   * the slots of abpoa_hip__debug_clocks.
// Plain C++: no HIP runtime call, usable without hipcc.  tools/kernel_bench.py, tools/phase_clocks.py and tests/test_gpu_device_msa.py restate slots in Python.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DIAG_HD __host__ __device__
#else
#define DIAG_HD
#endif

namespace abpoa_hip {

// ---- (a) ABPOA_HIP_DBG.  Bits 6-11 are test hooks and report selectors: every build honours them and none of them changes a result.
constexpr int DBG_NO_FAST_LOOPS = 64;         // every alignment takes the general kernel's general rows (routing.h, rows_general.h); no all-rounds kernel
constexpr int DBG_KEEP_ROW_SLOTS = 128;       // the tails leave AlnOut.seg as the row loop wrote it (placement, census, counters)
constexpr int DBG_WALK_REPORT = 256;          // the direction-word tail writes the walk report into AlnOut.seg
constexpr int DBG_WALK_GIVES_UP = 512;        // the direction-word walk ends in NEED_SCORES at its first insertion decided from the words (tests of the redo path)
constexpr int DBG_ONE_WAVE_BACKTRACK = 1024;  // all-rounds kernel: one wavefront per backtrack
constexpr int DBG_CXX_TIGHT_LOOP = 2048;      // narrow row loop: the compiler's tight loop instead of the hand-placed assembly
// Bits 0-5 are timing-only ablations: RESULTS ARE WRONG ON PURPOSE.  They exist only behind ABL(), i.e. in a library built with -DABPOA_HIP_ABLATE
// (`make prof`, tools/kernel_bench.py); the shipped library ignores them.  A bit switches off one thing in the fast row loops (rows_fast.h: ABL_FAST_*) and
// another in the general kernel's rows (rows_general.h: ABL_GEN_*).
constexpr int ABL_NO_ARENA_STORE = 1;         // both loops: no store of the row's cells into the arena
constexpr int ABL_FAST_NO_RING_STORE = 2,     ABL_GEN_FAKE_ARGMAX = 2;          // no store into the LDS score ring | the row arg-max is made up
constexpr int ABL_FAST_NO_ARGMAX = 4,         ABL_GEN_LITERAL_F_SCAN = 4;       // no arg-max candidates | the literal F scan instead of the closed form
constexpr int ABL_FAST_NO_F_CLOSED_FORM = 8,  ABL_GEN_NO_CHUNKS = 8;            // no closed-form F | a row computes no chunk at all
constexpr int ABL_FAST_NO_GATHER = 16,        ABL_GEN_FAKE_GATHER = 16;         // no predecessor gather from the ring | predecessors' scores are `col & 15`
constexpr int ABL_FAST_NO_SLOW_F = 32,        ABL_GEN_NO_QUERY_PROFILE = 32;    // no literal F scan of the slow vectors | no query profile
constexpr int DBG_ABLATION_BITS = 63;
struct DbgBit { int value; const char *what; };
constexpr DbgBit DBG_BITS[] = {      // (the help text of ABPOA_HIP_DBG is made from this table: engine_options.cpp)
    {DBG_ABLATION_BITS, "timing ablations of the row loops (1 .. 32: only in a `make prof` library, results wrong on purpose)"},
    {DBG_NO_FAST_LOOPS, "no fast row loops"}, {DBG_KEEP_ROW_SLOTS, "the tails keep the row loop's AlnOut.seg"}, {DBG_WALK_REPORT, "walk report in AlnOut.seg"},
    {DBG_WALK_GIVES_UP, "the direction-word walk gives up (NEED_SCORES)"}, {DBG_ONE_WAVE_BACKTRACK, "one wavefront per backtrack"},
    {DBG_CXX_TIGHT_LOOP, "the compiler's tight loop"},
};

// ---- (b) the macros of the diagnostic builds.  They expand where `fseg` (long long[DIAG_SLOTS]) is in scope, with `fseg_last` (FSTAMP), `I16` (WCOUNT_BODY)
// and the DevBatch `b` (ABL).  One build flag at a time (the census takes -DABPOA_HIP_ASM_CENSUS on top): the layouts share the six slots.
#ifdef ABPOA_HIP_PROFILE      // ticks per segment of a row (s_memtime stamps: they distort the loop they measure by ~25 %)
#define FSTAMP(I) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); long long t_ = (long long)__builtin_amdgcn_s_memtime(); fseg[I] += t_ - fseg_last; fseg_last = t_; }
#else
#define FSTAMP(I)
#endif
#ifdef ABPOA_HIP_ASM_CENSUS      // (the census WITH the assembly loop: it takes the slot of the one-predecessor body, whose C++ copy moves in with the two-predecessor one)
#define CENSUS_SLOT(I) ((I) == CEN_ONE_PRED ? CEN_CXX_TIGHT : (I))
#else
#define CENSUS_SLOT(I) (I)
#endif
#ifdef ABPOA_HIP_ROW_CENSUS      // rows and ticks per body of the narrow loop
#define CENSUS_T0() const long long cen_t0 = (long long)__builtin_amdgcn_s_memtime();
#define CENSUS(I) { fseg[CENSUS_SLOT(I)] += census_pack(1, (long long)__builtin_amdgcn_s_memtime() - cen_t0); }
#else
#define CENSUS_T0()
#define CENSUS(I)
#endif
#ifdef ABPOA_HIP_WIDE_COUNTERS      // rows per path of the wide loop
#define WCOUNT(I) { fseg[I] += 1; }
#define WCOUNT_BODY(NCH) { fseg[WC_BODY] += wide_body_pack(1, 0, 0) + ((NCH) >= 9 ? (I16 ? wide_body_pack(0, 0, 1) : wide_body_pack(0, 1, 0)) : 0); }
#else
#define WCOUNT(I) {}
#define WCOUNT_BODY(NCH) {}
#endif
#ifdef ABPOA_HIP_ABLATE
#define ABL(BIT) (b.dbg & (BIT))
#else
#define ABL(BIT) false
#endif

// ---- (c) AlnOut.seg[]: six words, one layout at a time.  The row loop writes its layout (which one: the build); the tail that follows overwrites it with its
// own unless DBG_KEEP_ROW_SLOTS is set; DBG_WALK_REPORT puts the walk report there instead.
constexpr int DIAG_SLOTS = 6;
// shipped build, fast row loops: where the wave ran (the ABPOA_HIP_IMBAL placement report); the other slots are 0
enum PlacementSlot { PLACE_KEY = 5 };
// -DABPOA_HIP_PROFILE: ticks per segment, in the order of a row (names: the general rows', as tools/phase_clocks.py prints them).  General rows: row set-up |
// gather | in-row part | stores | arg-max and hand-over | tile switch and window slide.  Fast loops: band and reserve | gather | F scans | carry chain of the
// all-chunk bodies, the exact bodies as a whole | stores, arg-max, commit | an all-chunk row of the wide loop.
enum ProfileSlot { PROF_HDR = 0, PROF_GATHER = 1, PROF_FCHAIN = 2, PROF_STORE = 3, PROF_ARGMAX = 4, PROF_TOP = 5 };
// -DABPOA_HIP_ROW_CENSUS: census_pack(rows, ticks) per body of the narrow loop -- one predecessor (tight loop), two (tight loop), three to eight (straight-line
// body), the all-chunks / exact bodies, tile switches -- and the census "why" word.  With -DABPOA_HIP_ASM_CENSUS slot 0 is the assembly loop's and slot 1 the
// C++ copies of the one- / two-predecessor body.
enum CensusSlot { CEN_ONE_PRED = 0, CEN_ASM_LOOP = 0, CEN_TWO_PRED = 1, CEN_CXX_TIGHT = 1, CEN_MANY_PRED = 2, CEN_EXACT = 3, CEN_TILE = 4, CEN_WHY = 5 };
// -DABPOA_HIP_WIDE_COUNTERS: rows per path of the wide loop -- the all-chunk bodies (a wide body word) | not eligible (predecessor count / distance) | ring /
// geometry | wider than the body's chunks | slow vectors span two wavefronts | the body declined (arg-max key window, wrap guard)
enum WideSlot { WC_BODY = 0, WC_NOT_ELIGIBLE = 1, WC_RING_GEOMETRY = 2, WC_TOO_WIDE = 3, WC_STRADDLE = 4, WC_DECLINED = 5 };
// the tails (every build): ticks, and counts scaled by 1000 (*_K) so that a mean over alignments keeps three decimals
enum DirTailSlot { DTAIL_ZERO = 0, DTAIL_WALK_TICKS = 1, DTAIL_STEPS_K = 2, DTAIL_GENERAL_STEPS_K = 3, DTAIL_WINDOWS_K = 4, DTAIL_WINDOW_TICKS = 5 };      // backtrack_dir.h
enum RecordTailSlot { RTAIL_SETUP_TICKS = 0, RTAIL_WALK_TICKS = 1, RTAIL_FLAG_STEPS_K = 2, RTAIL_SLOW_STEPS_K = 3, RTAIL_WINDOWS_K = 4, RTAIL_WINDOW_TICKS = 5 };      // backtrack.h
// DBG_WALK_REPORT (backtrack_dir.h): why the walk hit a dead end (0: it did not) and on what | two words of where | best_i << 32 | best_j | cigar entries | steps
enum WalkSlot { WALK_WHY = 0, WALK_A = 1, WALK_B = 2, WALK_BEST = 3, WALK_N_CIGAR = 4, WALK_STEPS = 5 };

// ---- (d) the packed words
constexpr int GETREG_HW_ID = 63492, GETREG_XCC_ID = 6164;      // s_getreg operands: all 32 bits of HW_ID (register 4) | the 4 bits of XCC_ID (register 20)
DIAG_HD constexpr long long placement_pack(long long hw_id, long long xcc_id) { return hw_id | (xcc_id << 32); }
// xcc | se, sh, cu | simd: equal for two waves iff they ran on the same SIMD
DIAG_HD constexpr unsigned long long placement_simd(long long key) { return (((unsigned long long)key >> 32) & 15) << 16 | ((unsigned long long)key & 0xff30); }
// census word: rows in bits 40-63, ticks in bits 0-39
DIAG_HD constexpr long long census_pack(long long rows, long long ticks) { return (long long)(((unsigned long long)rows << 40) + (unsigned long long)ticks); }
DIAG_HD constexpr long long census_rows(long long word) { return (long long)((unsigned long long)word >> 40); }
DIAG_HD constexpr long long census_ticks(long long word) { return word & ((1ll << 40) - 1); }
// census "why" word, 20 bits each: rows that went to the exact bodies with more than 4 predecessors | because the straight-line body declined | because a
// predecessor lies beyond the ring
DIAG_HD constexpr long long census_why_pack(long long many_preds, long long declined, long long beyond_ring) { return (many_preds << 40) | (declined << 20) | beyond_ring; }
DIAG_HD constexpr long long census_why_many_preds(long long word) { return (word >> 40) & 0xfffff; }
DIAG_HD constexpr long long census_why_declined(long long word) { return (word >> 20) & 0xfffff; }
DIAG_HD constexpr long long census_why_beyond_ring(long long word) { return word & 0xfffff; }
// wide body word: rows of the all-chunk bodies in bits 0-31, those of 9-11 chunks (the long-read form) among them in bits 32-47 (int32) / 48-62 (int16)
DIAG_HD constexpr long long wide_body_pack(long long rows, long long long32, long long long16) { return rows | (long32 << 32) | (long16 << 48); }
DIAG_HD constexpr long long wide_body_rows(long long word) { return word & 0xffffffffll; }
DIAG_HD constexpr long long wide_body_long32(long long word) { return (word >> 32) & 0xffff; }
DIAG_HD constexpr long long wide_body_long16(long long word) { return word >> 48; }

// ---- (e) abpoa_hip__debug_clocks: sums over the alignments of the flat API since the last call
enum ClockSlot { CLK_DP = 0, CLK_BT = 1, CLK_ROWS_DONE = 2, CLK_BT_STEPS = 3, CLK_SEG0 = 4, CLK_SLOTS = CLK_SEG0 + DIAG_SLOTS };

}  // namespace abpoa_hip
