"""The band table of the all-chunk row bodies (rows_fast.h ilp_chunks<NCH>, NCH = 3 .. 7 in dp_wide_kernel, 8 / 9 / 11 in dp_xl_kernel): the two 1 kb goldens
re-banded (wf = 0) so that their rows of 1358 / 1147 x <= 704 columns walk through every chunk count from 2 to 11 and one past each kernel's widest body, in
both score widths, with what the launch plan (msa_device_plan.cpp make_lds_plan, read through the host-only hook abpoa_hip__wide_plan) answers at every point
written down as data.  One table for the CPU test of the inputs (tests/test_wide_band_regimes.py: the oracle's chunk counts per row, the plan against the
hook) and the GPU tests (tests/test_gpu_wide_bodies.py: kernels against the oracle).  A plain module beside tests/scoring_points.py."""
import scoring_points as SP

GAPS = {"s1k_ag_gb": dict(gap_open1=4, gap_open2=0, gap_ext1=2), "s1k_cg_gb": dict()}      # the goldens' own penalties: affine 4,0 / 2 and the default convex
GOLDENS = tuple(GAPS)
WIDTHS = (16, 32)
COMBOS = [(g, b) for g in GOLDENS for b in WIDTHS]


def point(golden, bits, qlen):
    """The golden's own scoring at match 2 (16 bits), or at the first match score at which a query of qlen bases scores in 32 bits (33 for both goldens)."""
    if bits == 16:
        return SP.Point(f"{golden[4:6]}16_m2", "wide", match=2, **GAPS[golden])
    m32 = SP.width_gate_points(qlen)[1].kw["match"]
    return SP.Point(f"{golden[4:6]}32_m{m32}", "wide", match=m32, **GAPS[golden])


# What abpoa_hip__wide_plan answers for one alignment: (wide_on, wide_w_lo, wide_w_hi, score-ring rows).  wide_w_hi = (ring columns - 17) / 2.
R448, R704, OFF = (1, 40, 215, 16), (1, 40, 343, 16), (0, 1, 0, 0)
RING_COLS = {215: 448, 343: 704}
# per band half-width wb: the plan for (s1k_ag_gb, 16), (s1k_cg_gb, 16), (s1k_ag_gb, 32), (s1k_cg_gb, 32)
_ROWS = [
    # wb    ag16  cg16  ag32  cg32     chunk counts per row by the oracle (modal count first)
    (39,   R448, R448, R448, R448),  # 2 (and 1; int32 affine also 3-4): below wide_w_lo, the narrow kernel
    (40,   R448, R448, R448, R448),  # 2: the first band of the wide loop
    (70,   R448, R448, R448, R448),  # 3
    (100,  R448, R448, R448, R448),  # 4
    (130,  R448, R448, R448, R448),  # 5
    (165,  R448, R448, R448, R448),  # 6
    (184,  R448, R448, R448, R448),  # 6 and 7: the last band of the 448-column ring in int16
    (185,  R704, R704, R448, R448),  # ... and the first of the 704-column ring in int16
    (196,  R704, R704, R448, R448),  # 7: the last band of the 448-column ring in int32 (int32 affine: 250 rows of 8-11 chunks, declined by the 7-chunk kernel)
    (197,  R704, R704, R704, R704),  # ... and the first of the 704-column ring in int32
    (215,  R704, R704, R704, R704),  # 7 and 8; with ABPOA_HIP_NOXL=1 the last band of the 448-column kernel, whose 8-chunk rows it declines
    (216,  R704, R704, R704, R704),  # 7 and 8; with ABPOA_HIP_NOXL=1 one past wide_w_hi
    (250,  R704, R704, R704, R704),  # 8 and 9
    (290,  R704, R704, R704, R704),  # 10
    (324,  R704, R704, R704, R704),  # 11 (396-504 rows), 6-10 at 120-200 rows each: the last band at which int32 convex keeps the fast loops
    (325,  R704, R704, R704, OFF),   # int32 convex: the four-row narrow ring no longer fits, no fast loop at all (general kernel)
    (343,  R704, R704, R704, OFF),   # 11 and 12: wide_w_hi of the 704-column ring, 12-chunk rows declined by the 11-chunk kernel
    (344,  R704, R704, R704, OFF),   # one past it: the narrow kernel's chunk-by-chunk bodies
]
BANDS = tuple(r[0] for r in _ROWS)
PLAN = {(g, b): {r[0]: r[1 + 2 * WIDTHS.index(b) + GOLDENS.index(g)] for r in _ROWS} for g, b in COMBOS}
# the same under ABPOA_HIP_NOXL=1 (no long-read form: the 448-column kernel up to its wide_w_hi = 215), at the bands the GPU test runs that way
NOXL_BANDS = (196, 215, 216)
NOXL_PLAN = {c: {wb: R448 for wb in NOXL_BANDS} for c in COMBOS}
# ABPOA_HIP_RING_ROWS=4 (every predecessor more than three rows back is gathered from the arena in HBM, inside the body) at five bands: 5, 6, 7, 8-9, 11 chunks
RING4_BANDS = (130, 165, 196, 250, 324)
# the thresholds, as the hook reports them (found by scanning wb; tests/test_wide_band_regimes.py repeats the scan)
RING_704_FROM = {16: 185, 32: 197}      # first band half-width with the 704-column ring
CG32_FAST_OFF_FROM = 325                # int32 convex, 1 kb query: first band half-width without any fast row loop
# one past each kernel's widest body: (plan table, band) -> chunk count that must occur and that the kernel declines ("wider than the body")
ONE_PAST = [("noxl", 215, 8), ("default", 343, 12), ("default", 344, 12)]
# extension mode with z-drop (heter_cg_extz, both containers): rows of >= 5 chunks at wb = 100, of >= 8 chunks at wb = 250 (>= 100 rows each)
EXTZ_BANDS = ((100, 5), (250, 8))


# (point, variant) pairs the GPU tests do not run under direction words, with the reason -- from the plan or from dir_plane_usable, never from a result
NO_WORDS = {("s1k_cg_gb", 32, wb): "no fast row loop in the plan (fr_cols = 0): the general kernel stores score planes and writes no words" for wb in BANDS if wb >= CG32_FAST_OFF_FROM}


def plan(golden, bits, wb, noxl=False):
    return (NOXL_PLAN if noxl else PLAN)[(golden, bits)][wb]


def inside(golden, bits, wb, noxl=False):
    """The alignment takes the wide row loop: wide_on and wide_w_lo <= wb <= wide_w_hi (routing.h takes_wide_band)."""
    on, lo, hi, _ = plan(golden, bits, wb, noxl)
    return on == 1 and lo <= wb <= hi


def fast_loops(golden, bits, wb):
    """The plan keeps a fast row loop for the point (narrow or wide kernel).  For these scorings (5 codes, affine / convex) the hook's wide_on is 0 only where
    make_lds_plan set fr_cols = 0; the general kernel then runs, which writes no direction words."""
    return plan(golden, bits, wb)[0] == 1
