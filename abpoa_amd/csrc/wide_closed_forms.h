/* Integer closed forms of the all-chunks row body (rows_fast.h ilp_chunks), shared by the kernels and by the CPU property tests
 * (tests/test_wide_row_closed_forms.py): plain inline functions, host + device under hipcc, plain C++ under any other compiler.
 *
 *   arg-max key    one 32-bit key per cell whose unsigned order is the order of the reference's max_in_row (src/simd_abpoa_align.c:1043-1057):
 *                  the largest H of the row; ties go to the lowest lane residue l, then -- inside a lane -- to the end vector (it seeds the
 *                  lane's running maximum), then to the lowest vector.  One unsigned max over the row's keys, one decode to (rowmax, max_i).
 *   carry chain    F of the row is one 64-lane prefix-max scan per chunk of 64 columns; chunk c starts from seed[c] = "first - e" and
 *                  seed[c + 1] = max(total[c], seed[c]) - 64 e, total[c] = max over the chunk's lanes x of hs[x] + x e.
 */
#ifndef ABPOA_WIDE_CLOSED_FORMS_H
#define ABPOA_WIDE_CLOSED_FORMS_H
#include <climits>

#ifdef __HIPCC__
#define WCF_FN __host__ __device__ __forceinline__
#else
#define WCF_FN inline
#endif

namespace abpoa_hip {

WCF_FN int wcf_max(int a, int b) { return a > b ? a : b; }
WCF_FN int wcf_min(int a, int b) { return a < b ? a : b; }

// ---- arg-max key, int16 (PN = 16): value + 2^15 (bits 16-31) | PN - 1 - l (12-15) | end flag (11) | 2047 - absolute vector (0-10; qlen < 2^15)
WCF_FN int argmax_key16_const(int PN, int l, int vvl) { return (int)(0x80000000u | ((unsigned)(PN - 1 - l) << 12) | (unsigned)(2047 - vvl)); }
// vb = absolute index of the chunk's first vector
WCF_FN unsigned argmax_key16(int cand, int kconst, int vb, bool is_end) { return ((unsigned)cand << 16) + (unsigned)(kconst - vb) + (is_end ? 2048u : 0u); }
WCF_FN int argmax_value16(unsigned k) { return (int)(k >> 16) - 32768; }
WCF_FN int argmax_index16(unsigned k, int PN, int qlen) { int mi = (2047 - (int)(k & 0x7ff)) * PN + (PN - 1 - (int)((k >> 12) & 0xf)); if (mi > qlen) mi = -1; return mi; }
// the row's (maximum, max_i): max_i = -1 where the maximum is "inf" or lies beyond the query
WCF_FN void argmax_decode16(unsigned k, int PN, int qlen, int inf, int &rowmax, int &mi) { mi = -1; rowmax = argmax_value16(k); if (rowmax > inf) mi = argmax_index16(k, PN, qlen); }

// ---- arg-max key, int32 (PN = 8): the value relative to a floor (the first predecessor's row maximum - 2^19), clamped to [0, 2^21 - 1] (bits 11-31) |
//      PN - 1 - l (8-10) | end flag (7) | 127 - vector of the row (0-6: the long-read form's rows have up to 11 chunks = 88 vectors).  A winner at
//      either clamp is not representable: the row is declined (argmax_declines32) and takes the exact bodies.
constexpr int ARGMAX32_TOP = (1 << 21) - 1;
WCF_FN int argmax_tie32(int PN, int l, int vvl) { return ((PN - 1 - l) << 8) | (127 - vvl); }
// cg = chunk of the row, NV = vectors per chunk
WCF_FN unsigned argmax_key32(int cand, int vfloor, int ktie, int cg, int NV, bool is_end) {
    return ((unsigned)wcf_min(wcf_max(cand, vfloor) - vfloor, ARGMAX32_TOP) << 11) | (unsigned)(ktie - cg * NV) | (is_end ? 128u : 0u);      // (max first: inf - floor must not wrap)
}
WCF_FN bool argmax_declines32(unsigned k) { const unsigned tv = k >> 11; return tv == 0u || tv == (unsigned)ARGMAX32_TOP; }
WCF_FN int argmax_value32(unsigned k, int vfloor) { return vfloor + (int)(k >> 11); }
WCF_FN int argmax_index32(unsigned k, int PN, int beg_sn, int qlen) { int mi = (beg_sn + 127 - (int)(k & 127)) * PN + (PN - 1 - (int)((k >> 8) & 7)); if (mi > qlen) mi = -1; return mi; }
WCF_FN void argmax_decode32(unsigned k, int PN, int beg_sn, int vfloor, int qlen, int inf, int &rowmax, int &mi) { mi = -1; rowmax = argmax_value32(k, vfloor); if (rowmax > inf) mi = argmax_index32(k, PN, beg_sn, qlen); }

// ---- carry chain of the F scan: the seed of the next chunk from this chunk's total and seed
WCF_FN int carry_next(int total, int seed, int e) { return wcf_max(total, seed) - 64 * e; }

}  // namespace abpoa_hip
#endif
