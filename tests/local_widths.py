"""The width table of the local row loops (rows_local.h: dp_local_kernel's straight-line bodies rows_local<T, GAP, 3 / 5 / 9>, dp_local_team_kernel's shapes
rows_local_team<T, GAP, 1 / 2 / 3, 4>): three local goldens re-queried (tests/helpers.py requeried: the golden's own query cut or tiled, skip edges added to
the graph) so that their rows walk through every chunk count from 1 to 9, both sides of every body and team-shape switch, the hand-over to the general kernel at
576 columns, rows with 1 .. 13 predecessors up to 33 rows back, and rows whose maximum is tied between chunks.  Everything is data, written down from the
kernels' arithmetic and not computed by them: one table for the CPU test of the inputs (tests/test_local_regimes.py, against the oracle) and for the GPU tests
(tests/test_gpu_local_bodies.py, kernels against the oracle).  A plain module beside tests/wide_bands.py and tests/scoring_points.py."""
import scoring_points as SP
from abpoa_amd import api

# first container of each: amino acids under BLOSUM62, convex, 654 rows x 494 residues; nucleotides affine (4,0 / 2) 323 x 218 and convex (default) 299 x 240
GOLDENS = ("aa_blosum_loc", "ragged_ag_loc", "ragged_cg_loc")
NUCLEOTIDE = GOLDENS[1:]
GAPS = {"aa_blosum_loc": dict(), "ragged_ag_loc": dict(gap_open1=4, gap_open2=0, gap_ext1=2), "ragged_cg_loc": dict()}
RING_ROWS = {"aa_blosum_loc": 8, "ragged_ag_loc": 16, "ragged_cg_loc": 8}      # LDS score ring of the local loops (make_lds_plan): 16 rows affine, 8 convex
N_ROWS = {"aa_blosum_loc": 654, "ragged_ag_loc": 323, "ragged_cg_loc": 299}

GENERAL = "general"
# qlen: (chunks of 64 columns in a row of (qlen / 16 + 1) * 16 columns,  single-wavefront body NCH,  team NCW,  chunks per wavefront of the team of four)
QLENS = {
    1:   (1, 3, 1, (1, 0, 0, 0)),
    15:  (1, 3, 1, (1, 0, 0, 0)),      # one vector of 16 columns: a row's chunk store runs 48 records past its end
    16:  (1, 3, 1, (1, 0, 0, 0)),      # two vectors
    47:  (1, 3, 1, (1, 0, 0, 0)),
    48:  (1, 3, 1, (1, 0, 0, 0)),      # the first full chunk (64 columns, column 48 the last real one)
    63:  (1, 3, 1, (1, 0, 0, 0)),
    64:  (2, 3, 1, (1, 1, 0, 0)),
    127: (2, 3, 1, (1, 1, 0, 0)),
    128: (3, 3, 1, (1, 1, 1, 0)),
    191: (3, 3, 1, (1, 1, 1, 0)),      # the last row width of rows_local<.., 3>
    192: (4, 5, 1, (1, 1, 1, 1)),      # ... and the first of <.., 5>
    255: (4, 5, 1, (1, 1, 1, 1)),      # the last of the team's NCW = 1
    256: (5, 5, 2, (2, 1, 1, 1)),      # ... and the first of NCW = 2
    319: (5, 5, 2, (2, 1, 1, 1)),      # the last of <.., 5>
    320: (6, 9, 2, (2, 2, 1, 1)),      # ... and the first of <.., 9>
    383: (6, 9, 2, (2, 2, 1, 1)),
    384: (7, 9, 2, (2, 2, 2, 1)),
    447: (7, 9, 2, (2, 2, 2, 1)),
    448: (8, 9, 2, (2, 2, 2, 2)),
    511: (8, 9, 2, (2, 2, 2, 2)),      # the last of NCW = 2
    512: (9, 9, 3, (3, 2, 2, 2)),      # ... and the first of NCW = 3
    575: (9, 9, 3, (3, 2, 2, 2)),      # the last query the local loops take: (575 / 16 + 1) * 16 = 576 = loc_cols
    576: (10, GENERAL, GENERAL, GENERAL),      # 592 columns > loc_cols: takes_local hands the alignment to the general kernel
}
LOC_COLS = 576

# (qlen, period): the golden's query cut to `period` residues and tiled -- a periodic query scores the same against a graph row at columns one period apart, so
# the row maximum is tied between chunks wherever two such columns are both in reach.  Rows (of n_rows - 2) whose maximum H lies in more than one chunk,
# without / with SKIPS, and in brackets the rows that reach the alignment's best score (the first must win), by the oracle:
#                 aa_blosum_loc            ragged_ag_loc            ragged_cg_loc
#   (575, 100)    607 [1] / 652 [1]        321 [1] / 321 [1]        297 [1] / 297 [3]
#   (448, 64)     465 [1] / 588 [1]        321 [2] / 321 [2]        297 [1] / 297 [3]
#   (320, 80)     298 [2] / 342 [3]        319 [2] / 321 [1]        297 [1] / 297 [3]
#   (130, None)     2 [1] /   2 [1]         13 [1] /  15 [2]          5 [1] /  13 [1]      (6 / 41, 28 / 57, 12 / 38 rows with the maximum in more than one column)
TILED = [(575, 100), (448, 64), (320, 80), (130, None)]
TIED_ROWS_AT_LEAST = 100      # at every tiled point of two or more periods
# rows reaching the best score, (golden, qlen, period) -> (without, with SKIPS), where either is two or more: tests/test_local_regimes.py holds the oracle to it
BEST_TIES = {("aa_blosum_loc", 320, 80): (2, 3), ("ragged_ag_loc", 448, 64): (2, 2), ("ragged_ag_loc", 320, 80): (2, 1), ("ragged_ag_loc", 130, None): (1, 2),
             ("ragged_cg_loc", 575, 100): (1, 3), ("ragged_cg_loc", 448, 64): (1, 3), ("ragged_cg_loc", 320, 80): (1, 3)}

# skip edges (every, start, distances back): rows of 9 .. 13 predecessors (the run-time loop behind the eight unrolled gathers), predecessors 9 .. 33 rows
# back (older than either ring: gathered from the arena) and 2 .. 15 back (older than the convex ring only)
SKIPS = [(7, 20, (9,)), (11, 40, (17, 33)), (50, 60, (2, 3, 4, 6, 10, 12, 18, 20, 30)), (97, 100, tuple(range(2, 14)))]
# SKIPS alone leaves no row of 7 or 8 predecessors in any of the three graphs and none of 6 in two (its first two entries add at most three to a row's own
# one to four, the last two nine and more): four more entries of four to seven edges for the unrolled fifth to eighth gather
FILL = [(73, 38, (2, 4, 7, 13)), (61, 30, (2, 3, 5, 7, 11)),(67, 45, (2, 4, 6, 8, 10, 14)), (71, 52, (3, 5, 6, 9, 12, 15, 21))]
SKIPS_FILLED = SKIPS + FILL
SKIP_QLENS = (63, 192, 320, 575)      # 1, 4, 6 and 9 chunks


def point(golden):
    """The golden's own scoring as a scoring point (what rescored takes), for the nucleotide goldens."""
    return SP.Point(f"{golden}_own", "local", **GAPS[golden])


def asym_point(golden):
    return SP.BY_NAME["asym_ag" if golden == "ragged_ag_loc" else "asym_cg"]


def gate_points(golden, qlen):
    """The last match score at which a query of qlen bases runs in 16 bits under the golden's own penalties and the first at which it does not (as
    scoring_points.width_gate_points: qlen * max_mat <= 32767 - min_mis - oe1 - oe2)."""
    p = api.Params(**GAPS[golden])
    m16 = (32767 - p.min_mis - (p.gap_open1 + p.gap_ext1) - (p.gap_open2 + p.gap_ext2)) // qlen
    return (SP.Point(f"{golden}_gate16_m{m16}", "gate", match=m16, **GAPS[golden]), SP.Point(f"{golden}_gate32_m{m16 + 1}", "gate", match=m16 + 1, **GAPS[golden]))


SCORING_QLENS = (192, 575)
