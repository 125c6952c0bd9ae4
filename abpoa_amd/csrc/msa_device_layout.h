// Byte arithmetic of the device-resident read-set driver (msa_device.cpp): the offsets of every pool in the three device blobs, the round-major read tables,
// the kernel-argument records bound to those offsets, the layouts of the MSA and GFA result pools, the unpacking of one set's results and the event slots --
// plain C++ on host arrays and a plan (msa_device_plan.h) with no call into the HIP runtime, so that it runs and is tested without a GPU
// (tests/test_device_layout.py).  msa_device.cpp makes every HIP call and takes these answers as input.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <vector>
#include "msa_device_plan.h"

namespace abpoa_hip {

enum : int { BLOB_IN = 0, BLOB_GRAPH = 1, BLOB_ROWS = 2 };
struct LayoutEntry { int blob; const char *name; size_t off, bytes; };      // name: the Layout field, "o_sets" ...
struct Layout {                // byte offsets inside the three device blobs, every one 256-aligned
    // in blob (uploaded): sets, read tables, reads, score matrix
    // (o_rc, o_wrc: device only, behind the uploaded part)
    size_t o_sets, o_roff, o_rlen, o_reads, o_mat, o_rargs, o_msaoff_h, o_gfaoff_h, o_wts, in_bytes, o_rc, o_wrc, in_dev_bytes;
    // graph blob (device only, the head of it -- dl_bytes -- downloaded at the end): per-node pools
    size_t o_cnode, o_ccov, o_cbase, o_isrc, o_gcnt, dl_bytes;
    size_t o_gwalk, o_gorw, o_goff;      // GFA output (GfaDev): walk order, ORed read bitsets, the host's offsets -- zero bytes unless the job asked for it
    size_t o_state, o_base, o_nin, o_nout, o_naln, o_in, o_out, o_outw, o_inx, o_outx, o_outwx, o_aln, o_nread, o_row, o_order0, o_order1, o_rid, o_mrank,
            o_msaoff, o_tout, o_toutw, o_tin, graph_bytes;
    // rows blob: DP inputs / outputs per row, descriptors, cigars, scratch
    size_t o_ticket, o_aln_desc, o_out_rec, o_rbase, o_rsd, o_rpd, o_rnid, o_rrem, o_poff, o_pred, o_bsn, o_esn, o_coff, o_rmi, o_cigar, o_scratch, o_ooff,
            o_orow, o_left, o_right, o_act, o_outfwd, o_cigfwd, o_retry, rows_bytes;
    std::vector<LayoutEntry> table;      // every pool in the order it was taken (the CPU test walks this)
};
Layout lay_out_device(const DevicePlan &pl, int n_sets, bool any_w);

// Reads are laid out round by round (read k of every set, then read k + 1 ...): roff [tot_reads + 1] / rlen [tot_reads] indexed PoaSet.read0 + k.  Returns
// where the reads of round 2 and later start in the read pool (the first two rounds go up at once): the pool's end when no set has a third read
int64_t fill_read_tables(const DevicePlan &pl, int n_sets, const abpoa_hip_readset_t *sets, int64_t *roff, int32_t *rlen);

// Arguments of the graph kernels (p, and g: zeroed unless the job wants GFA output; its result pools come with bind_gfa_pools) on the blobs at di / dg / dr;
// dig_on: cigar_digest_on()
void bind_poa_dev(PoaDev &p, GfaDev &g, const DevicePlan &pl, const Layout &L, int n_sets, bool any_w, bool dig_on, uint8_t *di, uint8_t *dg, uint8_t *dr);
// Arguments of the row-loop kernels behind b.n / b.m / b.lds (final_lds_plan); b_rc: the -s retry in the general kernel
void bind_dev_batch(DevBatch &b, DevBatch &b_rc, const DevicePlan &pl, const Layout &L, const PoaDev &p, uint8_t *di, uint8_t *dr, uint8_t *planes);

// MSA rows of the sets back to back (rows x columns bytes per set; nothing for a set that did not finish or has an empty graph), from the downloaded states
struct MsaLayout { std::vector<int64_t> off; int64_t total = 0; };
MsaLayout lay_out_msa(const DevicePlan &pl, int n_sets, const abpoa_hip_readset_t *sets, const PoaState *hs);
// GFA result pools (Cache.gfa) from the downloaded states and the walk's counts (GfaDev.cnt).  off: per set first segment, first link, first path entry,
// path capacity (the bases of its reads).  link_off has n_seg + 1 entries per set at first segment + set, path_off n_reads + 1 at read0 + set: hence the
// + n_sets of those two pools.  bytes = 0: no set has a segment, no pool and no fill kernel
struct GfaLayout {
    std::vector<int64_t> off; int64_t seg_tot = 0, link_tot = 0, path_tot = 0;
    size_t o_seg = 0, o_loff = 0, o_lfrom = 0, o_poff = 0, o_pnode = 0, o_base = 0, o_cnt = 0, bytes = 0;      // (o_cnt: the host's copy of GfaDev.cnt after the fill kernel, not a device pool)
};
GfaLayout lay_out_gfa(const DevicePlan &pl, int n_sets, const abpoa_hip_readset_t *sets, const PoaState *hs, const int32_t *cnt);
void bind_gfa_pools(GfaDev &g, const GfaLayout &G, uint8_t *dq);

// The result record of set s from the downloaded buffers: hg = the head of the graph blob (Layout.dl_bytes), h_msa = the MSA rows (MsaLayout.total), h_gfa =
// the GFA pools (GfaLayout.bytes); M / G are read only where the plan wants that output.  Allocates with malloc (abpoa_hip_free_msa).  true: the set must be
// redone (it did not finish, or its GFA record did not fit) and *o holds nothing but n_reads
bool unpack_set(const DevicePlan &pl, const Layout &L, const MsaLayout &M, const GfaLayout &G, const abpoa_hip_readset_t &set, int s, const uint8_t *hg,
                const uint8_t *h_msa, const uint8_t *h_gfa, abpoa_hip_msa_t *o);

// Events of a job on its stream (Cache.ev), by index
struct EventSlots {
    int max_reads;
    int job_begin() const { return 0; }
    int after_init() const { return 1; }
    int rounds_begin() const { return 2; }      // the all-rounds kernel
    int rounds_end() const { return 3; }
    int round(int k) const { return 4 * k; }      // four from here, rounds 1 .. max_reads - 1: after prepare, after the rows, after the backtrack, after fuse
    int gfa() const { return 4 * max_reads + 4; }      // four from here: the walk kernel's pair, the fill kernel's pair
    int count() const { return 4 * max_reads + 8; }
};

}  // namespace abpoa_hip
