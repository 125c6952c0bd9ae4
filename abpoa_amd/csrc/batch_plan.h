// Host arithmetic of the flat batch driver (engine.cpp BatchStream): descriptors and arena estimates, the layouts of the two blobs, eligibility for the fast row
// loops, the direction-word tables, the plan of a pass, its arenas, the DevBatch pointers and the unpacking of a saved arena into trace planes -- plain C++ on
// host arrays with no call into the HIP runtime, so that it runs and is tested without a GPU (tests/test_batch_plan.py).  engine.cpp makes every HIP call and
// takes these answers as input.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <vector>
#include "engine.h"
#include "batch_types.h"

namespace abpoa_hip {

enum : unsigned {
    BS_TRACE = 0x1,             // keep per-row arg-max, allow fetch_trace()
    BS_FRESH_BAND = 0x2,        // max_pos_left/right start as (n_rows, 0) for every row: initialised on the device
    BS_WANT_BAND_STATE = 0x4,   // copy max_pos_left/right back to the host
};

// arena capacities of one alignment (cells of its score width): score records full width / estimate, direction-plane arenas likewise
struct ArenaCells { int64_t full, est, dir_full, dir_est; };
struct PoolTotals { int64_t rows, preds, outs, q, cig; };
// desc[i] (everything but flags / plane_off, which a run decides; plane_cap = the records' estimate) and cells[i] of every alignment; the pool totals
PoolTotals describe_batch(const abpoa_hip_scoring_t *sc, int n, const BatchShape *sh, AlnDesc *desc, ArenaCells *cells);

// Byte offsets of the pools in the input blob and in the output blob, every one 256-aligned
struct InLayout { size_t desc, mat, query, base, sdist, pd, nid, rem, act, poff, pred, ooff, out, bytes; };
struct OutLayout {
    size_t rec, cig, left, right, bsn, esn, coff, rmi, bytes;
    // what a launch copies back: records + cigars are adjacent at the start of the blob; band state / trace arrays on demand
    size_t download_bytes(bool banded, unsigned flags) const { return (flags & BS_TRACE) ? bytes : (banded && (flags & BS_WANT_BAND_STATE)) ? bsn : left; }
};
InLayout layout_in(int n, int m, const PoolTotals &t);
OutLayout layout_out(int n, const PoolTotals &t);
ProblemSlots problem_slots(const InLayout &I, const OutLayout &O, const AlnDesc &d, uint8_t *hi, uint8_t *ho);

// alignment-level eligibility for the register-resident row loops (AlnDesc.flags = ALN_FAST_OK | 0, pad0 = 0): banded, or unbanded local; every row active;
// for a kept band, the state at its reset value in every row.  The three pools are the blobs' (indexed through AlnDesc.row0)
void mark_fast_ok(const abpoa_hip_scoring_t *sc, bool fresh, int n, AlnDesc *desc, const uint8_t *row_active, const int32_t *left, const int32_t *right);
// the direction-word tables of one alignment (DevBatch.row_sdist [n_rows], DevBatch.row_pd [2 * n_rows]) from its predecessor CSR; false: a non-sink row names
// more predecessors than a word can (DIR_K_MAX) -- the alignment stays off the fast loops, and nothing reads its tables
bool fill_dir_tables(int n_rows, const int32_t *pred_off, const int32_t *pred_row, uint8_t *row_sdist, uint32_t *row_pd);
// direction words for the passes of a run, until an alignment needs its scores: not in trace mode (ABPOA_HIP_DIRTRACE=1 keeps them), banded global, penalties
// that fit the words, no ABPOA_HIP_NODIR
bool dir_words_for_run(const abpoa_hip_scoring_t *sc, unsigned flags);
// the launch of one pass over desc[todo[..]], pointers aside: LDS plan trimmed to the row-loop kernels that have work, score widths, scoring, switches
void plan_pass(const abpoa_hip_scoring_t *sc, unsigned flags, bool dir, const AlnDesc *desc, const std::vector<int> &todo, DevBatch &b);
// arenas of the pass (desc[i].plane_cap / plane_off, copied to pass[t]): words where the alignment takes a fast loop with words, else records; the estimate on
// the first pass, full width on a retry.  Returns the bytes of the arena pool; *n_fast = alignments of the tail kernel
int64_t assign_arenas(const DevBatch &b, bool first_pass, const ArenaCells *cells, const std::vector<int> &todo, AlnDesc *desc, AlnDesc *pass, int *n_fast);
void bind_pools(DevBatch &b, const InLayout &I, const OutLayout &O, uint8_t *di, uint8_t *dout, uint8_t *planes);

// A saved arena as the caller's trace: the per-row arrays of one alignment (dp_beg_sn / dp_end_sn / row_cell_off / row_max_i at its row 0) and the arena's
// bytes in the format the record names (AlnOut.pad: 0 = plane-major rows, > 0 cell records of that stride, < 0 direction words of that many bytes).
// Allocates T's arrays with malloc (abpoa_hip_free_result)
void unpack_trace(const AlnDesc &d, int P, bool banded, int cw, const int32_t *bsn, const int32_t *esn, const int64_t *coff, const int32_t *rmi,
                  const uint8_t *arena, abpoa_hip_trace_t *T);

// (test hooks abpoa_hip__wide_plan / abpoa_hip__narrow_plan: the LDS plan of a banded launch of n_aln alignments like the largest one)
void hook_lds_plan(const abpoa_hip_scoring_t *sc, int max_qlen, int max_bits, int n_aln, LdsPlan *L);

}  // namespace abpoa_hip
