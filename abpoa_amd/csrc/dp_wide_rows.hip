// Row-loop kernels for WIDE bands (10 kb reads: 240-300 columns = 4-5 chunks of 64 per row): every chunk of a row in registers at once
// (rows_fast.h, ilp_chunks), one wavefront per alignment.  Rows the all-chunk body cannot take are done with the general body.
#include <stdio.h>
#include <stdlib.h>
#include "engine_options.h"
#include "rows_fast.h"

namespace abpoa_hip {

template <int GAP, int BITS, bool DIR = false>
__global__ void __launch_bounds__(64) dp_wide_kernel(const DevBatch b) {
    const int a = blockIdx.x;
    if (a >= b.n) return;
    const AlnDesc d = b.aln[a];
    // (= !for_wide_kernel(b, d) of routing.h or the other width's; the width test between its two terms, as the kernel has always been compiled)
    if (!takes_fast(b, d) || (BITS != 0 && d.bits != BITS) || !takes_wide(b, d)) return;
    // BITS == 0: both score widths in one launch.  A job whose graphs outgrow int16 on the way has a few rounds in which some read-sets are still
    // int16 and the others already int32; two launches (one per width) would run one after the other, each with the other's SIMDs idle.
    if (BITS == 16 || (BITS == 0 && d.bits == 16)) align_fast_rows<int16_t, GAP, true, DIR>(b, d, b.out + a);
    else align_fast_rows<int32_t, GAP, true, DIR>(b, d, b.out + a);
}

template <int GAP, bool DIR = false>
static hipError_t launch_wide_gap(const DevBatch &b, hipStream_t stream) {
    const int mask = b.bits_mask ? b.bits_mask : 3;
    hipError_t e = hipSuccess;
    static bool told = false;
    if (!told && opt_set("ABPOA_HIP_VERBOSE")) {      // residency of the wide kernels on one CU
        told = true; int nb16 = 0, nb32 = 0;
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb16, dp_wide_kernel<GAP, 16>, 64, (size_t)b.lds.total_wide);
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb32, dp_wide_kernel<GAP, 32>, 64, (size_t)b.lds.total_wide);
        fprintf(stderr, "[abpoa-hip] wide row loop: 1 wavefronts per alignment, %d B of LDS per workgroup, ring %d rows x %d " "columns, workgroups per CU: %d (int16) %d (int32)\n",
                b.lds.total_wide, b.lds.wfr_rows, b.lds.wfr_cols, nb16, nb32);
    }
    if (mask == 3) return launch_one(dp_wide_kernel<GAP, 0, DIR>, b, stream, b.lds.total_wide);
    if (mask & 1) e = launch_one(dp_wide_kernel<GAP, 16, DIR>, b, stream, b.lds.total_wide);
    if (e == hipSuccess && (mask & 2)) e = launch_one(dp_wide_kernel<GAP, 32, DIR>, b, stream, b.lds.total_wide);
    return e;
}
hipError_t launch_xl_rows(const DevBatch &b, hipStream_t stream);      // dp_xl_rows.hip
hipError_t launch_wide_rows(const DevBatch &b, hipStream_t stream) {
    if (b.lds.wfr_cols == WIDE_RING_COLS_XL) return launch_xl_rows(b, stream);      // rows wider than 448 columns: the long-read form
    // (wide-band alignments keep their score records in dir_mode 1 and write direction words in dir_mode 2: routing.h takes_dir)
    if (b.dir_mode == 2) return b.gap_mode == ABPOA_HIP_AFFINE_GAP ? launch_wide_gap<1, true>(b, stream) : launch_wide_gap<2, true>(b, stream);
    return b.gap_mode == ABPOA_HIP_AFFINE_GAP ? launch_wide_gap<1>(b, stream) : launch_wide_gap<2>(b, stream);
}

}  // namespace abpoa_hip
