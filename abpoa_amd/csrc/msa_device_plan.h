// Planning step of the device-resident read-set driver (msa_device.cpp): which kernels a job takes, whether its arenas hold direction words or score records,
// the per-set table and the pool totals -- plain host arithmetic on the read lengths, the scoring and the switches, with no call into the HIP runtime, so that it
// can be run and tested without a GPU (tests/test_device_plan.py).  What needs the device -- free memory, the all-rounds kernel's residency, the CU count --
// stays in msa_device.cpp and takes the plan as input.
#pragma once
#include <stdint.h>
#include <vector>
#include "engine.h"
#include "poa_device.h"
#include "msa_device.h"

namespace abpoa_hip {

struct DevicePlan {
    abpoa_hip_scoring_t sc;        // the job's scoring; local mode: wb = -1 (reference abpoa_post_set_para, src/abpoa_align.c:150)
    double node_factor;
    bool local, extend, unbanded, amb, want_msa, want_cons, want_gfa;      // want_gfa: ABPOA_HIP_OUT_GFA -- read ids per edge as for the MSA, walk / output pools
    int CW, DB;                    // values per cell record (engine.h record_values); bytes per direction word
    int max_reads, max_qlen, w_max, aln_cap, rid_words; int64_t tot_reads, tot_bases;
    // which kernels: the general kernel for every alignment / the local row loop / direction words / linear gaps on the narrow loop / the all-rounds kernel
    // may take the job (msa_device.cpp plan_rounds decides)
    bool general, fast_local, dir, lin_fast, rounds_possible;
    bool roomy; int in_cap, out_cap;      // the last pass of the ladder: an edge slot per read at every node
    // band half-widths that take the wide row loop (LdsPlan.wide_w_lo / hi; none when the wide kernels are off), depth of its score ring.  wide_on / wfr_cols:
    // the wide loop's switch and ring columns of the ESTIMATE the range comes from (0 where the job has no wide loop) -- kept for the CPU test alone; no
    // driver stage reads them, the launch's final values are DevBatch.lds.wide_on / wfr_cols (final_lds_plan)
    int wide_lo, wide_hi, wide_ring_rows, wide_on, wfr_cols;
    // ragged sets: extra columns per set, the part of them that counts for the choice of the row loop, the largest, the effective band half-widths
    std::vector<int> extra, route; int max_extra, weff_lo, weff_hi;
    bool dir_wide, dir_wide_auto, any_wide_set;      // direction words for the wide-band sets too / ABPOA_HIP_DIR_WIDE leaves that to the driver / a set takes the wide loop
    // per set, what size_arenas assumed of the alignment of its longest read: the wide row loop / direction words (routing.h takes_wide / takes_dir) -- kept for
    // the CPU test, which holds them against the per-alignment rule; any_wide_set is their summary
    std::vector<uint8_t> set_wide, set_dir;
    std::vector<PoaSet> ps;
    int64_t node_tot, pred_tot, cig_tot, scr_tot, cons_tot, term_tot, plane_tot; int max_node_cap;

    // general kernel (rows_general.h): successor CSR, band state per row, the "row is part of the alignment" bytes (all ones: no sub-graph alignments here)
    bool gen_io() const { return general || amb; }      // (-s: the retry runs in the general kernel)
    int64_t est_cols(int64_t width, int w, int pn) const { return band_cols(width, w, pn, !(local || unbanded)); }      // columns per row: the whole query without a band
    // arenas (PoaSet.plane_off / plane_cap, plane_tot) with direction words for the wide-band sets or without: redone when the record arenas do not fit
    void size_arenas(const abpoa_hip_readset_t *sets, bool dir_wide);
};

DevicePlan plan_device_job(const abpoa_hip_scoring_t *sc, int n_sets, const abpoa_hip_readset_t *sets, double node_factor, unsigned flags, bool force_general);
// the launch's LDS plan (b.lds) and score widths (b.bits_mask): sized for the widest rows expected, trimmed to the row-loop kernels that can have work (wide_on,
// narrow_off); ABPOA_HIP_EINVAL: a local job outside the local row loop's range
int final_lds_plan(const DevicePlan &pl, int n_sets, const abpoa_hip_readset_t *sets, DevBatch &b);
// the wide row loop's workgroups per CU for a job of these sets when all of them take it with one wavefront each; 0: they do not (msa_device_resident_sets)
int wide_sets_per_cu(const abpoa_hip_scoring_t *sc, int n_sets, const abpoa_hip_readset_t *sets);

}  // namespace abpoa_hip
