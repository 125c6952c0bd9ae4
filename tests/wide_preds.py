"""The predecessor table of the wide row loop (rows_fast.h ilp_chunks<NCH>, NCH = 3 .. 7 in dp_wide_kernel, 8 / 9 / 11 in dp_xl_kernel, band half-widths
40 .. 343): the skip-edge families of tests/narrow_preds.py (helpers.requeried) pointed at the bands of tests/wide_bands.py, so that rows of 1358 / 1147 x <= 704
columns reach what the two 1 kb goldens' own graphs never do at these bands -- the run-time gather loop `for (k = 2; k < np; ++k)` up to k = 7 with its tvk
selector, is_far / hbm_read_all from the default 16-row ring, spill rows under direction words, tile bit 19 false (general_body inside the wide kernels), and
the walks of backtrack_dir.h / backtrack.h over column-slice windows behind both rings, through predecessor index 8 and above and out of a slice to the left.
One table for the CPU test of the inputs (tests/test_wide_pred_regimes.py: the classes per row and body on the oracle, the plan against the host-only hook
abpoa_hip__wide_plan, the oracle against the word model) and the GPU tests (tests/test_gpu_wide_pred_bodies.py: kernels against the oracle).  It holds no
results: inputs, and what the plan answers.  A plain module beside tests/wide_bands.py and tests/narrow_preds.py, whose FAMILIES, JUMP and case_dict it reuses.

The oracle on these graphs is NOT pinned to the compiled reference: no read-set produces them (a skip edge joins rows that no read joins).  The counterweight
is the read-set part of tests/test_gpu_wide_pred_bodies.py (the read-sets of narrow_preds.read_sets at a band that takes the wide loop, READ_SET_BAND), whose
CPU shim is pinned to the reference's command-line tool at that band by tests/test_host_msa.py.

Which family drives which branch (every family of narrow_preds.py keeps its meaning; RR = the score ring's rows, 16 unless ABPOA_HIP_RING_ROWS=4):
  in_ring    3-8 predecessors inside the ring: the gather loop at k = 2 .. 7, tv_p4 .. tv_p7, merge(.., kidx) up to 8 (kM / kE of 6 .. 8 in the words);
             9-11 predecessors: bit 19 false by `np <= 8`, general_body inside the wide kernels, WCOUNT(1);
  exact      every count 1 .. 8 on in-ring rows (the selector returns a different register per k), rows of 15 predecessors;
  far        the farthest predecessor 16-63 rows back at 1-2, 3-4 and 5-8 predecessors: ilp_far != 0, hbm_read_all at k = 1 .. 7, its sources are spill rows
             (row_sdist >= RR, bit 21: under words hbm_read_all steps over the row's words to its records); 64 and 70 back: bit 19 false by `dk < 64`,
             geo_of's HBM branch; the first predecessor near and the second far (`ilp_far & 3` == 2);
  farfirst   `far`'s 16- and 21-row edges on rows whose list is then turned round, the far predecessor FIRST: `ilp_far & 3` == 1 (helpers.requeried appends
             behind a row's own predecessors, so no other family has it at RR = 16);
  edge       the farthest exactly 15 | 16 | 17 rows back (RR - 1, RR, RR + 1), and 64;
  edge4      the same for ABPOA_HIP_RING_ROWS=4: exactly 3 | 4 | 5 rows back at 1-2, 3-4 and 5-8 predecessors (5 = RR + 1 is the first distance whose ring slot
             holds another row);
  many       9-11 predecessors: not eligible, general_body;
  jump       the walk leaves rows through predecessor index 8 .. 10 (go_pred behind the eight distances of row_pd, the record walk's loop) on slice windows;
  farjump    steps of 16 .. 300 rows: behind the score ring, the geometry ring and the 254 rows a byte of row_pd names, each followed by a new slice window;
  ins        `far` with runs of INS_RUNS random bases inserted into the query: the walk leaves a column slice to the left (load_window's !narrow branch stages
             DIR_TRI_SLACK columns beyond the triangle, rounded down to 16 bytes of words) and the window is re-centred.
Measured on the oracle (tests/test_wide_pred_regimes.py prints every count): see MEASURED, NOT_ELIGIBLE, WALK_FLOOR, STEP_FLOOR, INS_FLOOR below."""
import numpy as np

import helpers as H
import narrow_preds as NP
import wide_bands as WB

GOLDENS, COMBOS = NP.GOLDENS, WB.COMBOS
VARIANT = {16: "own", 32: "i32"}
RR, RR4, GEO_ROWS = NP.RR, 4, NP.GEO_ROWS
BODIES = (3, 4, 5, 6, 7, 8, 9, 11)                       # the chunk counts ilp_chunks is instantiated for in the wide kernels

# new skip-edge families, each entry (every, start, dists) as helpers.requeried takes them
FAMILIES = {
    "edge4": ((7, 30, (3,)), (11, 31, (2, 3)), (13, 35, (4,)), (17, 41, (2, 3, 4)), (19, 47, (5,)), (23, 60, (2, 3, 5)),
              (29, 33, (2, 3, 4, 5)), (31, 37, (2, 3, 4, 6, 5)), (37, 39, (2, 3)), (41, 43, (2, 4)), (43, 45, (2, 3, 4)), (9, 32, (4,))),
    "farfirst": ((9, 30, (16,)), (13, 35, (2, 21)), (17, 41, (2, 3, 17)), (23, 50, (2, 3, 4, 5, 40))),
}
# `farfirst`: the predecessor lists of the rows these entries touch are turned round, so that the row's farthest predecessor leads its list
TURNED = {"farfirst": tuple((e, s) for e, s, _ in FAMILIES["farfirst"]), "edge4": ((13, 35), (19, 47))}
# `ins`: on top of `far`, runs of random bases (seed INS_SEED) inserted in front of these query positions.  Measured: see INS_FLOOR
INS_RUNS = ((120, 48), (260, 60), (400, 40), (540, 72), (680, 48), (820, 60))
INS_SEED = 1818
PRED_FAMILIES = ("in_ring", "far", "edge", "exact", "many", "farfirst")           # compared plane by plane at every band of BANDS
WALK_FAMILIES = ("jump", "farjump", "ins")                                        # the walks; cut / lengthened queries
ALL_FAMILIES = PRED_FAMILIES + ("edge4",) + WALK_FAMILIES


def case_dict(golden, family, bits, wb):
    """Input dict (what helpers.FlatCase takes) of one table point at band half-width wb, wf = 0."""
    v = VARIANT[bits]
    if family in NP.FAMILIES or not family:
        return NP.case_dict(golden, family, v, wb)
    if family == "ins":
        d = NP.case_dict(golden, "far", v, wb)
        rng = np.random.RandomState(INS_SEED)
        q, parts, at = d["query"], [], 0
        for pos, n in INS_RUNS:
            parts += [q[at:pos], rng.randint(0, 4, n).astype(np.uint8)]
            at = pos
        d["query"] = np.ascontiguousarray(np.concatenate(parts + [q[at:]]), np.uint8)
        d["qlen"] = np.array([len(d["query"])], np.int32)
        return d
    d = NP.case_dict(golden, None, v, wb)
    d = H.requeried(d, int(d["qlen"][0]), skips=FAMILIES[family])
    if family in TURNED:
        n, po = int(d["n_rows"][0]), d["pred_off"]
        for every, start in TURNED[family]:
            for r in range(start, n - 1, every):
                d["pred_row"][po[r]:po[r + 1]] = d["pred_row"][po[r]:po[r + 1]][::-1].copy()
    return d


def body_of(nch):
    """The instantiation the wide kernels' dispatch sends a row of nch chunks to (rows_fast.h: nch <= 3 -> 3, 4 .. 9 their own, 10 and 11 -> 11)."""
    return 3 if 2 <= nch <= 3 else (nch if 4 <= nch <= 9 else (11 if nch <= 11 and nch >= 10 else None))


class WRow:
    """np: predecessors; dist: row distances in list order; dmax: the farthest; nch: chunks of 64 columns; body: body_of(nch); eligible: tile bit 19
    (1 .. 8 predecessors, all fewer than 64 rows back); src_reach: successor_reach of each predecessor."""
    __slots__ = ("np", "dist", "dmax", "nch", "body", "eligible", "src_reach")


def wide_rows(case, o):
    """{row: WRow} of every computed row with predecessors, from the inputs and the oracle's bands alone."""
    reach = NP.successor_reach(case)
    pn = 16 if o.bits == 16 else 8
    out = {}
    for r in range(1, case.n_rows - 1):
        if o.dp_beg_sn[r] < 0 or case.pred_off[r + 1] <= case.pred_off[r]:
            continue
        preds = case.pred_row[case.pred_off[r]:case.pred_off[r + 1]].astype(np.int64)
        x = WRow()
        x.np, x.dist = len(preds), tuple(int(r - p) for p in preds)
        x.dmax = max(x.dist)
        x.nch = (int(o.dp_end_sn[r] - o.dp_beg_sn[r] + 1) * pn + 63) // 64
        x.body = body_of(x.nch)
        x.eligible = x.np <= 8 and x.dmax < GEO_ROWS
        x.src_reach = tuple(int(reach[p]) for p in preds)
        out[r] = x
    return out


def classes_of(x, rr=RR):
    """Names of the classes of part 2 an eligible row of a body belongs to, for a score ring of rr rows."""
    if not x.eligible or x.body is None:
        return ()
    out = []
    if x.dmax < rr:
        if 3 <= x.np <= 4: out.append("ring3_4")
        if 5 <= x.np <= 8: out.append("ring5_8")
        out.append("np%d" % x.np)
    nb = "1_2" if x.np <= 2 else ("3_4" if x.np <= 4 else "5_8")
    if rr == RR and RR <= x.dmax < GEO_ROWS:
        out.append("far" + nb)
    if x.dmax in (rr - 1, rr, rr + 1):
        out.append("d%d" % x.dmax)
        if rr == RR4:
            out.append("d%d_%s" % (x.dmax, nb))
    if x.np >= 2 and x.dist[0] >= rr > x.dist[1]: out.append("far0_near1")
    if x.np >= 2 and x.dist[1] >= rr > x.dist[0]: out.append("near0_far1")
    if any(d >= rr for d in x.dist[2:]): out.append("far_k2")
    if any(d >= rr and s >= rr for d, s in zip(x.dist, x.src_reach)): out.append("far_spill")
    return tuple(out)


def not_eligible(rows):
    """Rows with more than 8 predecessors or a predecessor 64 and more rows back: what WCOUNT(1) counts in the wide kernels."""
    return sum(1 for x in rows.values() if not x.eligible)


def insertion_runs(o):
    """Lengths of the insertion words of the oracle's cigar (op 1: the length sits above bit 4)."""
    return [int(w >> np.uint64(4)) & 0x3fffffff for w in o.cigar if int(w) & 15 == 1]


# ---- the points of the table
# Bands (wf = 0) per (golden, width): the same six for all four -- the modal chunk counts in int16 are 3, 5, 6, 7, 8-9 and 11 there, body 4 gets its rows at 130
# and 165 (180-200 rows each); in int32 the rows are wider and more spread (s1k_ag_gb at match 33: 3-6 chunks at wb 70, 5-13 at 250), and over these six bands
# every body still holds 50 and more rows of every class below (MEASURED), so no band below 70 is needed and no cell of PRED_FAMILIES is left out.
BANDS = {c: (70, 130, 165, 196, 250, 324) for c in COMBOS}
SWITCH = {16: (WB.RING_704_FROM[16] - 1, WB.RING_704_FROM[16]), 32: (WB.RING_704_FROM[32] - 1, WB.RING_704_FROM[32])}      # 184 | 185, 196 | 197: `far` and `in_ring`
SWITCH_FAMILIES = ("far", "in_ring")
ONE_PAST = (343, "far")                        # rows of 12 chunks, too wide for the ring: as predecessors they are far at any distance (!(g_ & GEO_RING))
RING4_FAMILIES = ("edge4", "in_ring", "far")   # ABPOA_HIP_RING_ROWS=4, at every band of BANDS
NOXL_BANDS, NOXL_FAMILIES = (196, 215), ("in_ring", "far")       # ABPOA_HIP_NOXL=1: the 7-chunk body of dp_wide_kernel
# the walks: cut queries are shorter than the graph, their rows wider (int32 `jump`: 11-14 chunks already at wb 70), so the int32 walks start at 40; the
# 365 bases of `farjump` on s1k_cg_gb keep the 448-column ring at any band (wide_w_hi = 215), so the int16 walks end at 196
WALK_BANDS = {16: (70, 130, 196), 32: (40, 165)}
BT_BYTES = ("4096", "6144")                    # small backtrack windows (the values of test_small_backtrack_windows_with_wide_rows) ...
BT_BAND = {16: 130, 32: 165}                   # ... at one band per width
EXTZ = ("extz6", 196, ("far", "farjump"))      # extension mode, z-drop 6, int16: `far` 520 / 1039 computed rows of 5 chunks and more (s1k_ag_gb stops behind row 598);
                                               # `farjump` stops behind row 70 / 77, behind its first step of 16 rows (LEFT_OUT)
MIXED = dict(wb=12, wf=0.16, short={"s1k_ag_gb": "seq_ag_gb", "s1k_cg_gb": "seq_cg_gb"})      # one launch: w = 20 (54 bases) beside w = 84 .. 223 (every family)
READ_SET_BAND = dict(extra_b=60, extra_f=0.0)  # narrow_preds.read_sets at a band of the wide loop (w = 60 for every read: no alignment takes the narrow kernel)
READ_SET_FORMS = {"default": {}, "dir_wide": {"ABPOA_HIP_DIR_WIDE": "1"}, "dir_wide_ring4": {"ABPOA_HIP_DIR_WIDE": "1", "ABPOA_HIP_RING_ROWS": "4"},
                  "nodir": {"ABPOA_HIP_NODIR": "1"}}
CONVEX = dict()                                # the default convex penalties (4, 2 / 24, 1)
# cells left out, with the reason -- from arithmetic, the oracle or the plan, never from a GPU result
LEFT_OUT = {
    ("edge4", "d3_5_8"): "a farthest predecessor 3 rows back leaves three distinct distances: no row of 5-8 predecessors exists (measured 0 at every band)",
    ("edge4", "d4_5_8"): "a farthest predecessor 4 rows back leaves four distinct distances: no row of 5-8 predecessors exists (measured 0 at every band)",
    ("farjump", "extz", "5 chunks"): "the z-drop ends the row loop behind 70 / 77 rows, which are 3-4 chunks wide at every band its 454 / 365 bases leave inside the "
                                     "wide loop (wide_w_hi = 215): measured 0 rows of 5 chunks at wb = 130 and 196; the point runs, on the 3- and 4-chunk bodies",
    ("far", 343, "s1k_cg_gb", 32): "no fast row loop in the plan from wb = 325 on (wide_bands.CG32_FAST_OFF_FROM): the general kernel runs",
}
# `edge4` at 5 rows back holds rows of exactly 5 predecessors (distances 1 .. 5) in its 5-8 class.


def pred_points(golden, bits):
    """[(family, wb)] compared plane by plane under the default plan: PRED_FAMILIES at every band, the ring switch, one past the widest body, the walks."""
    pts = [(f, wb) for wb in BANDS[(golden, bits)] for f in PRED_FAMILIES]
    pts += [(f, wb) for wb in SWITCH[bits] for f in SWITCH_FAMILIES if (f, wb) not in pts]
    if ("far", ONE_PAST[0], golden, bits) not in LEFT_OUT:
        pts.append((ONE_PAST[1], ONE_PAST[0]))
    return pts + [(f, wb) for wb in WALK_BANDS[bits] for f in WALK_FAMILIES]


def words_apply(family):
    """abpoa_oracle_dir_walk answers at every family here (global mode, affine / convex, at most 15 predecessors per row); the CPU test holds this to its return code."""
    return True


# ---- floors.  MEASURED: rows per class and body (3, 4, 5, 6, 7, 8, 9, 11 chunks: BODIES) on the oracle, summed over BANDS, per (golden, width); the floor of a
# cell is two thirds of its measured count (floor_of), 4 at the least.  Class names: classes_of.
AG16, AG32, CG16, CG32 = COMBOS
MEASURED = {
    ('in_ring', 'ring3_4'): {AG16: (229, 88, 212, 196, 163, 71, 85, 84), AG32: (189, 113, 180, 191, 159, 90, 99, 90), CG16: (167, 51, 163, 158, 131, 60, 72, 80), CG32: (166, 55, 165, 155, 132, 71, 60, 78)},
    ('in_ring', 'ring5_8'): {AG16: (214, 77, 215, 199, 169, 72, 91, 91), AG32: (160, 106, 176, 184, 170, 97, 104, 103), CG16: (179, 57, 185, 171, 144, 49, 91, 84), CG32: (176, 65, 182, 173, 140, 52, 90, 82)},
    ('exact', 'np1'): {AG16: (918, 309, 891, 847, 699, 342, 342, 392), AG32: (739, 396, 770, 796, 713, 418, 419, 421), CG16: (888, 264, 893, 837, 712, 390, 312, 408), CG32: (887, 282, 891, 836, 713, 494, 201, 400)},
    ('exact', 'np2'): {AG16: (332, 114, 337, 315, 267, 114, 136, 155), AG32: (248, 145, 276, 299, 260, 158, 166, 166), CG16: (194, 84, 201, 176, 146, 71, 62, 74), CG32: (195, 88, 198, 179, 141, 90, 43, 74)},
    ('exact', 'np3'): {AG16: (105, 44, 103, 92, 83, 37, 43, 39), AG32: (85, 53, 87, 94, 79, 50, 45, 42), CG16: (55, 16, 49, 47, 38, 19, 22, 24), CG32: (56, 17, 48, 47, 39, 20, 20, 23)},
    ('exact', 'np4'): {AG16: (52, 18, 43, 44, 35, 14, 19, 21), AG32: (44, 21, 40, 38, 34, 16, 22, 25), CG16: (35, 11, 31, 34, 27, 12, 14, 16), CG32: (34, 12, 33, 33, 27, 14, 13, 14)},
    ('exact', 'np5'): {AG16: (38, 9, 39, 39, 32, 14, 17, 16), AG32: (26, 14, 31, 36, 32, 20, 22, 19), CG16: (32, 9, 32, 30, 25, 9, 17, 14), CG32: (32, 9, 33, 30, 24, 11, 15, 14)},
    ('exact', 'np6'): {AG16: (41, 14, 38, 39, 31, 14, 15, 18), AG32: (31, 18, 34, 35, 31, 14, 21, 19), CG16: (31, 10, 34, 30, 27, 12, 15, 15), CG32: (31, 9, 34, 31, 26, 13, 15, 15)},
    ('exact', 'np7'): {AG16: (39, 18, 39, 36, 29, 14, 14, 15), AG32: (28, 26, 30, 32, 29, 18, 20, 16), CG16: (32, 12, 33, 31, 26, 10, 15, 15), CG32: (31, 13, 33, 31, 26, 9, 16, 15)},
    ('exact', 'np8'): {AG16: (30, 8, 33, 28, 26, 13, 14, 16), AG32: (19, 15, 24, 23, 28, 17, 19, 19), CG16: (26, 8, 29, 27, 24, 10, 13, 13), CG32: (25, 10, 29, 27, 23, 10, 13, 13)},
    ('far', 'far1_2'): {AG16: (98, 38, 99, 90, 80, 27, 48, 42), AG32: (80, 48, 82, 88, 82, 37, 54, 44), CG16: (89, 26, 98, 87, 84, 20, 59, 47), CG32: (90, 28, 97, 89, 82, 24, 53, 47)},
    ('far', 'far3_4'): {AG16: (107, 35, 113, 106, 93, 24, 65, 51), AG32: (78, 48, 91, 93, 86, 56, 53, 58), CG16: (75, 27, 80, 75, 61, 19, 42, 35), CG32: (73, 31, 82, 74, 59, 19, 42, 34)},
    ('far', 'far5_8'): {AG16: (43, 39, 64, 63, 65, 26, 43, 28), AG32: (23, 46, 42, 63, 60, 44, 37, 42), CG16: (19, 51, 34, 59, 57, 39, 37, 19), CG32: (25, 46, 44, 54, 59, 32, 36, 21)},
    ('far', 'near0_far1'): {AG16: (107, 42, 110, 102, 93, 29, 56, 49), AG32: (85, 53, 89, 97, 93, 46, 60, 53), CG16: (98, 32, 109, 101, 97, 26, 67, 51), CG32: (100, 33, 110, 103, 94, 30, 60, 51)},
    ('far', 'far_k2'): {AG16: (148, 74, 175, 167, 155, 50, 106, 78), AG32: (100, 93, 132, 154, 143, 98, 89, 99), CG16: (91, 78, 110, 131, 115, 56, 77, 53), CG32: (95, 77, 122, 125, 115, 49, 76, 54)},
    ('far', 'far_spill'): {AG16: (248, 112, 276, 259, 238, 77, 156, 121), AG32: (181, 142, 215, 244, 228, 137, 144, 144), CG16: (183, 104, 212, 221, 202, 78, 138, 101), CG32: (188, 105, 223, 217, 200, 75, 131, 102)},
    ('farfirst', 'far0_near1'): {AG16: (341, 114, 355, 334, 293, 91, 192, 158), AG32: (234, 174, 283, 304, 298, 171, 194, 177), CG16: (272, 92, 302, 279, 247, 76, 172, 137), CG32: (268, 102, 300, 279, 244, 83, 166, 135)},
    ('edge', 'd15'): {AG16: (35, 12, 36, 35, 28, 10, 20, 16), AG32: (22, 20, 26, 28, 29, 22, 20, 18), CG16: (29, 7, 30, 28, 26, 6, 17, 13), CG32: (27, 10, 29, 28, 25, 7, 17, 13)},
    ('edge', 'd16'): {AG16: (102, 34, 107, 100, 86, 28, 58, 49), AG32: (70, 53, 81, 93, 87, 53, 59, 51), CG16: (83, 22, 93, 84, 76, 20, 51, 45), CG32: (80, 27, 91, 86, 73, 23, 51, 43)},
    ('edge', 'd17'): {AG16: (246, 83, 255, 242, 207, 61, 140, 116), AG32: (170, 116, 204, 224, 200, 130, 148, 121), CG16: (203, 60, 218, 203, 177, 52, 126, 101), CG32: (197, 71, 219, 198, 178, 57, 121, 99)},
    ('edge4', 'd3'): {AG16: (320, 122, 302, 292, 239, 108, 118, 131), AG32: (246, 153, 254, 275, 235, 147, 147, 138), CG16: (208, 69, 218, 196, 169, 79, 85, 92), CG32: (202, 77, 215, 202, 165, 105, 60, 90)},
    ('edge4', 'd4'): {AG16: (354, 127, 361, 336, 286, 129, 150, 159), AG32: (270, 164, 294, 323, 288, 170, 186, 173), CG16: (283, 92, 294, 272, 237, 108, 121, 135), CG32: (284, 95, 297, 271, 236, 122, 108, 129)},
    ('edge4', 'd5'): {AG16: (190, 65, 191, 180, 156, 65, 82, 85), AG32: (144, 84, 161, 167, 151, 96, 93, 95), CG16: (149, 49, 157, 145, 130, 53, 68, 71), CG32: (147, 53, 159, 144, 128, 60, 62, 69)},
    ('edge4', 'd3_1_2'): {AG16: (164, 69, 150, 147, 115, 53, 52, 60), AG32: (130, 85, 123, 142, 115, 71, 69, 59), CG16: (98, 36, 103, 93, 80, 38, 36, 44), CG32: (97, 39, 103, 93, 80, 46, 26, 44)},
    ('edge4', 'd3_3_4'): {AG16: (156, 53, 152, 145, 124, 55, 66, 71), AG32: (116, 68, 131, 133, 120, 76, 78, 79), CG16: (110, 33, 115, 103, 89, 41, 49, 48), CG32: (105, 38, 112, 109, 85, 59, 34, 46)},
    ('edge4', 'd4_1_2'): {AG16: (123, 42, 126, 117, 100, 47, 55, 56), AG32: (97, 54, 107, 111, 101, 61, 64, 55), CG16: (114, 37, 117, 105, 93, 41, 52, 53), CG32: (113, 41, 115, 109, 92, 50, 41, 51)},
    ('edge4', 'd4_3_4'): {AG16: (231, 85, 235, 219, 186, 82, 95, 103), AG32: (173, 110, 187, 212, 187, 109, 122, 118), CG16: (169, 55, 177, 167, 144, 67, 69, 82), CG32: (171, 54, 182, 162, 144, 72, 67, 78)},
    ('edge4', 'd5_1_2'): {AG16: (29, 7, 33, 29, 28, 15, 12, 15), AG32: (21, 10, 26, 28, 29, 20, 13, 19), CG16: (28, 11, 30, 28, 24, 14, 8, 13), CG32: (28, 11, 31, 27, 24, 13, 10, 12)},
    ('edge4', 'd5_3_4'): {AG16: (86, 35, 83, 84, 67, 27, 37, 37), AG32: (66, 44, 72, 74, 64, 41, 42, 41), CG16: (67, 22, 71, 67, 59, 27, 30, 29), CG32: (66, 24, 73, 67, 57, 29, 28, 28)},
    ('edge4', 'd5_5_8'): {AG16: (75, 23, 75, 67, 61, 23, 33, 33), AG32: (57, 30, 63, 65, 58, 35, 38, 35), CG16: (54, 16, 56, 50, 47, 12, 30, 29), CG32: (53, 18, 55, 50, 47, 18, 24, 29)},
    ('edge4', 'far0_near1'): {AG16: (159, 55, 162, 151, 129, 64, 65, 73), AG32: (123, 65, 135, 140, 128, 82, 84, 84), CG16: (127, 41, 131, 124, 107, 49, 55, 62), CG32: (126, 45, 131, 124, 107, 53, 50, 60)},
    ('edge4', 'near0_far1'): {AG16: (90, 31, 89, 87, 73, 37, 35, 44), AG32: (74, 42, 77, 83, 74, 40, 47, 39), CG16: (75, 21, 77, 69, 62, 30, 31, 37), CG32: (75, 23, 76, 72, 60, 36, 25, 35)},
    ('edge4', 'far_k2'): {AG16: (352, 124, 355, 333, 282, 119, 150, 151), AG32: (261, 169, 286, 315, 284, 164, 184, 170), CG16: (271, 89, 289, 263, 238, 94, 126, 130), CG32: (271, 92, 294, 259, 234, 111, 113, 126)},
    ('edge4', 'far_spill'): {AG16: (593, 208, 602, 564, 482, 215, 250, 266), AG32: (447, 273, 495, 532, 482, 289, 309, 291), CG16: (471, 153, 494, 453, 402, 173, 209, 225), CG32: (470, 161, 498, 453, 397, 198, 186, 217)},
}


def floor_of(measured):
    return (2 * measured) // 3


CLASS_RR = {f: (RR4 if f == "edge4" else RR) for f, _ in MEASURED}
# rows with more than 8 predecessors or a predecessor 64 and more rows back (tile bit 19 false: WCOUNT(1)), per family, for (s1k_ag_gb, s1k_cg_gb); a property
# of the graph, the same at every band and width.  tests/test_wide_pred_regimes.py counts them on the inputs; the device's counter is held to that count
NOT_ELIGIBLE = {"in_ring": (30, 23), "far": (76, 63), "many": (109, 97), "edge": (56, 47), "exact": (8, 7), "farfirst": (0, 0), "edge4": (0, 0)}
# the walks (measured at every band of WALK_BANDS, the same at each): `jump` 18 / 17 steps through predecessor index 8 and above in int16, 17 / 14 in int32;
# `farjump` steps of 16-63 / 64-254 / 255+ rows 6 / 4 / 1 in int16 on both goldens, 3 / 3 / 1 and 2 / 2 / 0 in int32: narrow_preds' floors carry over unchanged
WALK_FLOOR, STEP_FLOOR = NP.WALK_FLOOR, NP.STEP_FLOOR
# `ins`: insertion runs of the oracle's cigar longer than DIR_TRI_SLACK (9) plus the slice's alignment padding (16 bytes of words: up to 7 columns).  Measured
# at every band: s1k_ag_gb int16 seven runs (18 .. 72), int32 three (18-28: the match score of 33 breaks the runs up; at wb = 100 and 130 one run and none stay that long, so the
# int32 walks take 40 and 165), s1k_cg_gb six (40 .. 72) and five (30 .. 69)
INS_FLOOR = 3
# words whose kM or kE names predecessor 6 .. 8 (oracle/dir_model.c) on `in_ring` at wb = 130, for (s1k_ag_gb, s1k_cg_gb) per width: see KM_FLOOR's comment
KM_BAND = 130
