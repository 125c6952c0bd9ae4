// Guide-tree read order (the reference's -p, progressive_poa): minimizer sketch of every read, minimizer hits of every read pair of a set, and the
// greedy order built from their Jaccard similarities (reference src/abpoa_seed.c:84-324, :704-721).  The sketch and the pair counts are kernels
// (guide_sketch.hip); the similarity and the order are plain host C++ (guide_order.cpp, no HIP headers: tests/guide_order.cpp builds it alone).
#pragma once
#include <stdint.h>
#include <vector>
#include "../../include/abpoa_hip.h"

namespace abpoa_hip {

// k-mer size, window, alphabet and strands of the sketch
struct GuideParams { int k, w; bool aa, both_strands; };
// From the scoring block and the call's flags (ABPOA_HIP_GUIDE_KW, ABPOA_HIP_AMB_STRAND): defaults k = 19, w = 10; amino acids with k above 11 take
// k = 7, w = 4 (reference abpoa_align.c:157-159) when k was left to the default, and are refused when k was given.  ABPOA_HIP_EINVAL outside 1..28 / 1..11.
int guide_params(int m, unsigned flags, GuideParams *out);

// hit: the triangular matrix of one set, hit[i(i+1)/2 + j] for j <= i (diagonal: minimizers of read i; below it: minimizer hits of reads i and j).
// order[r] = the read aligned in round r.  Fewer than 3 reads, or no minimizer at all: the input order.
void guide_greedy_order(int n_reads, const int32_t *hit, int32_t *order);

// What the device pre-pass returns for all sets of a call: read r of set s is read set_read0[s] + r
struct GuideResult {
    std::vector<int64_t> set_read0;      // [n_sets + 1]
    std::vector<int64_t> set_hit0;       // [n_sets + 1] first entry of the set's triangular matrix in `hit`
    std::vector<int32_t> hit;
    std::vector<int32_t> order;          // [total reads], per set
    std::vector<int64_t> mm_off;         // [total reads + 1] first sketch value of the read in `mm`
    std::vector<uint64_t> mm;            // per read ascending; filled only when asked for
    double sketch_ms = 0, pair_ms = 0;   // kernel durations, hipEvents on the pre-pass's stream
    double total_s = 0;                  // wall time of the whole pre-pass: packing, copies, kernels, order
};
// Sketch + pair kernels for every set on `device` (< 0: the engine's), then the order on the host.  Returns ABPOA_HIP_OK or a negative code.
// slot: which of the pre-pass queues (stream, events, pools) to use -- the device queue of the calling batch entry, so that contexts do not wait for
// each other; a queue runs one pre-pass at a time.
constexpr int GUIDE_QUEUES = 16;
int guide_prepass(const GuideParams &gp, int n_sets, const abpoa_hip_readset_t *sets, int device, int slot, bool want_mm, GuideResult &R);
// frees the streams and the pools the pre-pass queues keep between calls (abpoa_hip_trim)
void release_guide_queues();
// positions per tile of the sketch kernel (tests place read lengths around it)
int guide_tile_length();

}  // namespace abpoa_hip
