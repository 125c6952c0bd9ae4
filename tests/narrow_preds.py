"""The predecessor table of the narrow row loop (rows_fast.h rows_fast<T, GAP, false, DIR>, band half-widths w < 40, inside dp_fast_kernel and
poa_rounds_kernel): the two 1 kb goldens with skip edges added at run time (helpers.requeried) so that their rows of 1358 / 1147 x <= 192 columns reach every
body the loop picks among -- by predecessor count (1 .. 17), by how far back the farthest predecessor lies (inside the 16-row score ring, inside the 64-row
geometry ring, beyond it), by row width (<= 64, 65-128, > 128 columns), with and without a vector beyond every predecessor's band (the literal-scan vector) and
with and without a successor that reads the row from HBM (a spill row of the direction-word jobs).  One table for the CPU test of the inputs
(tests/test_narrow_regimes.py: the classes per row on the oracle, the plan against the host-only hook abpoa_hip__narrow_plan, the oracle against the word model)
and the GPU tests (tests/test_gpu_narrow_bodies.py: kernels against the oracle).  It holds no results: inputs, and what the plan answers.  A plain module beside
tests/wide_bands.py.

The oracle on these graphs is NOT pinned to the compiled reference: no read-set produces them (a skip edge joins rows that no read joins).  The
counterweight is the read-set part of tests/test_gpu_narrow_bodies.py, whose graphs grow high in-degree by themselves (reads at 30 % error) and whose CPU shim
is pinned to the reference's command-line tool by tests/test_host_msa.py.

Which point drives which body (s1k_ag_gb: int16 affine 4,0/2, w = 19 -- with direction words the job of the assembly loop rows_tight_asm.h; s1k_cg_gb: int16
convex, w = 20 -- the compiler's loops; every family at the golden's own band unless a band is named):
  in_ring          3-4 predecessors: the assembly loop's three- / four-predecessor paths (words, ag) or turbo_body<4> (cg, records, ABPOA_HIP_DBG=2048);
                   5-8: turbo_body<8>; 9-11, all in the ring: fast_body / general_body.  Rows with the literal-scan vector at 3-4 and 5-8 predecessors.
  in_ring, w = 24  the last band with a 128-column ring in int16: rows of 65-128 columns with 3-8 predecessors take ilp_chunks<2> from the score ring;
  in_ring, w = 25  the first band with a 192-column ring: bits 17, 18, 20 and the assembly loop are off, every row takes ilp_chunks<2> or the exact bodies
                   (36 / 37 are the same pair in int32, lanes of 8);
  far              a farthest predecessor 16-63 rows back: ilp_chunks<2> with the arena gather in HBM (dk = 15 | 16 either side of `dk < RR` in switch_tile
                   and is_far); 64 and more rows back: general_body (63 | 64 either side of `dk < 64`); the sources of those edges are the spill rows:
                   the outside copies of turbo_body<1|2> (tile bit 22) and the record stores of turbo_body<4|8> and ilp_chunks<2>;
  many             9-11 predecessors, all in the ring: general_body (the oracle's walk passes these rows through one of their first five predecessors);
  edge             the farthest predecessor exactly 15 | 16 | 17 rows back at 5-8 predecessors (tile bit 20), 17 at 3-4 and at 1-2 (bits 16-18, is_far), 64
                   at 5-8 (bit 19).  A row 16 back still sits in the slot the current row is about to take, so 16 on the wrong side of `dk < RR` reads
                   right values all the same: 17, which shares its slot with row - 1, is the first distance at which a slip there shows;
  jump             rows of eleven predecessors whose best path arrives over the LAST of them: the queries of the other families follow the golden's own path
                   and never leave a row through a skip edge behind its fourth predecessor -- here the walks of backtrack_dir.h (go_pred behind the eight
                   distances of row_pd) and backtrack.h step through predecessor index 8 and above;
  farjump          the same cut in front of rows with one skip edge 16, 17, 63, 64, 70 and 300 rows back: the best path takes every one of them, so the walks
                   step behind the score ring, behind the geometry ring and past the 254 rows a byte of row_pd names (go_pred's `i -= dk ... restage`, its
                   CSR branch at dk == 255, the lane-parallel step's break there; the same steps of backtrack.h) and a small window is staged again behind
                   each.  At every other family the longest step of the oracle's walk is 11 rows (`jump`), else 4-6;
  exact            every predecessor count 1 .. 8 on in-ring rows (NPC = 1, 2, 4 with np = 3 | 4, 8 with np = 5 .. 8), and rows of exactly 15;
  exact16 / 17     ... and rows of exactly 16 / 17 predecessors: past the 4-bit kM / kE fields of a direction word (DIR_K_MAX = 15) -- the word plane does not
                   apply (abpoa_oracle_dir_walk answers EINVAL, read in the CPU test), such an alignment keeps score records in the general kernel;
  variants         i32: match 33, the compiler's loops in 32 bits; linear (ag graph, e1 = 2): rows_fast GAP = 0, no ilp_chunks<2>, records only;
                   extz6 / extz10: extension mode with z-drop 6 / 10, where asm_tight_on is off: the C++ tight loop with commit_row's z-drop test."""
import numpy as np

import helpers as H
import wide_bands as WB

GOLDENS = ("s1k_ag_gb", "s1k_cg_gb")
R = lambda a, b: tuple(range(a, b + 1))

# skip-edge families, each entry (every, start, dists) as helpers.requeried takes them
_EXACT = ((40, 4, (2,)), (40, 8, (2, 3)), (40, 14, R(2, 4)), (40, 21, R(2, 5)), (40, 28, R(2, 6)), (40, 34, R(2, 7)), (40, 41, R(2, 8)), (160, 137, R(2, 15)))
FAMILIES = {
    "in_ring": ((7, 5, (2, 3)), (11, 8, (2, 3, 4, 5, 6)), (13, 9, (2, 4, 7, 9, 11, 13, 15)), (29, 20, (3,))),
    "far": ((9, 30, (16,)), (17, 40, (2, 3, 21)), (23, 50, (2, 3, 4, 5, 63)), (31, 70, (64,)), (37, 90, (2, 70)), (41, 100, (15,))),
    "many": ((19, 20, R(2, 9)), (27, 33, R(2, 11))),
    "edge": ((11, 30, (2, 3, 4, 5, 16)), (13, 35, (2, 3, 4, 5, 17)), (17, 41, (2, 3, 17)), (19, 47, (17,)), (23, 60, (2, 3, 4, 5, 64)), (29, 71, (2, 3, 4, 5, 15))),
    "jump": ((67, 50, R(2, 11)),),
    "farjump": tuple((10000, st + blk, (d,)) for blk in (0, 440) for st, d in ((40, 16), (80, 17), (170, 63), (260, 64), (350, 70))) + ((10000, 1120, (300,)),),
    "exact": _EXACT,
    "exact16": _EXACT + ((160, 57, R(2, 16)),),
    "exact17": _EXACT + ((160, 97, R(2, 17)),),
}
# `jump`: the query also loses the bases that the golden's own alignment (its recorded cigar) matches to the rows r - 10 .. r - 1 in front of every row r the
# family gives eleven predecessors, so that the best path takes the edge from r - 11, the last of the row's list
# `farjump`: the same cut in front of rows with ONE skip edge, 16, 17, 63, 64 or 70 rows back (two rows per distance) and one 300 rows back (past the 254 a
# byte of row_pd holds): the walk steps over the score ring and over the geometry ring, and the window of the backtrack is staged again behind a far step
JUMP = {"jump": ((67, 50, 11),), "farjump": tuple((e, st, ds[0]) for e, st, ds in FAMILIES["farjump"])}
# scoring variants: name -> (golden graphs it runs on, score width)
VARIANTS = {"own": (GOLDENS, 16), "i32": (GOLDENS, 32), "linear": (("s1k_ag_gb",), 16), "extz6": (GOLDENS, 16), "extz10": (GOLDENS, 16)}
# extension mode with z-drop: at 6 the oracle ends the row loop of every s1k_ag_gb family behind row 598 / 599 of 1356 and runs s1k_cg_gb to the end; at 10
# it ends only the three `exact` families of s1k_ag_gb (row 599).  STOPS_EARLY is asserted against the oracle on the CPU.
ZDROP = {"extz6": 6, "extz10": 10}
OWN_W = {"s1k_ag_gb": 19, "s1k_cg_gb": 20}       # the goldens' own band (wb = 10, wf = 0.01) ...
CUT_W = {"jump": (18, 18), "farjump": (14, 13)}  # ... and with the cut queries (847 / 865 bases; 454 / 365), for (s1k_ag_gb, s1k_cg_gb)
# cut queries: the least cigar words of a run to the end; where a z-drop stops it (STOPS_EARLY), the least rows computed and cigar words
CUT_SIZES = {"jump": (850, 150, 100), "farjump": (350, 60, 30)}
# the width switch of the score ring: fr_cols = max(128, align64(min(width, 2 w + 3 pn + 32))) -- 128 up to W_128[bits], 192 from one past it
W_128 = {16: 24, 32: 36}
RR, GEO_ROWS = 16, 64               # score-ring rows, rows of the geometry ring
# fr_rows as the plan answers it: 16, but 8 for int32 convex with 192 ring columns (three ring words per column: sixteen rows pass the LDS budget of the
# row-loop kernel) -- there the predecessors 8 .. 15 rows back of `in_ring` are gathered from the arena too
RING_ROWS_192 = {("s1k_ag_gb", 16): 16, ("s1k_cg_gb", 16): 16, ("s1k_ag_gb", 32): 16, ("s1k_cg_gb", 32): 8}


def case_dict(golden, family, variant="own", wb=None):
    """Input dict (what helpers.FlatCase takes) of one table point; wb = None: the golden's own band, else that half-width at wf = 0."""
    g = H.first_golden(golden)
    qlen = int(g["qlen"][0])
    assert golden in VARIANTS[variant][0]
    keep = np.arange(qlen)
    if family in JUMP:
        row_of = {int(nid): r for r, nid in enumerate(g["row_node_id"])}
        q_at = {row_of[int(w) >> 34]: (int(w) >> 4) & 0x3fffffff for w in g["cigar"] if int(w) & 15 == 0}       # match words: node id above bit 34, query index above bit 4
        drop = {q_at[r - k] for every, start, dist in JUMP[family] for r in range(start, int(g["n_rows"][0]) - 1, every) for k in range(1, dist) if r - k in q_at}
        keep = np.array([i for i in range(qlen) if i not in drop])
    d = H.rescored(g, WB.point(golden, VARIANTS[variant][1], len(keep)), wb, None if wb is None else 0.0)      # (int32: the first match score at which THIS query leaves 16 bits)
    i32 = lambda v: np.array([v], np.int32)
    if variant == "linear":
        d.update(gap_mode=i32(0), gap_open1=i32(0), gap_open2=i32(0), gap_ext1=i32(2))
    if variant in ZDROP:
        d.update(align_mode=i32(2), zdrop=i32(ZDROP[variant]))
    if family:
        d = H.requeried(d, qlen, skips=FAMILIES[family])
        d["query"], d["qlen"] = np.ascontiguousarray(d["query"][keep]), i32(len(keep))
    return d


def half_width(case):
    return case.sc.wb + int(np.float32(case.sc.wf) * np.float32(case.qlen))


def successor_reach(case):
    """Per row min(255, largest row distance to a successor), 255 for a predecessor of the sink: DevBatch.row_sdist as engine.cpp fills it."""
    n = case.n_rows
    sd = np.zeros(n, np.int64)
    for r in range(n):
        for p in case.pred_row[case.pred_off[r]:case.pred_off[r + 1]] if case.pred_off[r + 1] > case.pred_off[r] else ():
            sd[p] = max(sd[p], 255 if r == n - 1 else min(255, r - int(p)))
    return sd


class RowClass:
    """np: predecessors; far: 0 | 1 | 2 = the farthest is < 16 | 16 .. 63 | >= 64 rows back; cols: 0 | 1 | 2 = <= 64 | 65 .. 128 | > 128 columns; slow: a vector
    beyond every predecessor's band (dp_end_sn[r] > max over the predecessors); spill: a successor 16 or more rows ahead, or the sink."""
    __slots__ = ("np", "far", "cols", "slow", "spill", "dmax", "ncols", "reach")

    def key(self):
        return self.np, self.far, self.cols, self.slow, self.spill


def row_class(case, o, r, reach=None):
    """Class of computed row r (1 <= r < n_rows - 1) from the inputs and the oracle's bands alone."""
    preds = case.pred_row[case.pred_off[r]:case.pred_off[r + 1]].astype(np.int64)
    pn = 16 if o.bits == 16 else 8
    c = RowClass()
    c.np = len(preds)
    c.dmax = int(r - preds.min())
    c.far = 0 if c.dmax < RR else (1 if c.dmax < GEO_ROWS else 2)
    c.ncols = int(o.dp_end_sn[r] - o.dp_beg_sn[r] + 1) * pn
    c.cols = 0 if c.ncols <= 64 else (1 if c.ncols <= 128 else 2)
    c.slow = bool(o.dp_end_sn[r] > o.dp_end_sn[preds].max())
    c.reach = int((successor_reach(case) if reach is None else reach)[r])
    c.spill = c.reach >= RR
    return c


def row_classes(case, o):
    """{row: RowClass} of every computed row with predecessors (rows behind a z-drop stop are not computed: dp_beg_sn < 0)."""
    reach = successor_reach(case)
    return {r: row_class(case, o, r, reach) for r in range(1, case.n_rows - 1) if o.dp_beg_sn[r] >= 0 and case.pred_off[r + 1] > case.pred_off[r]}


def predicted_body(c, fr_rows, fr_cols, bits=16, gap_mode=1, words=False, asm=False, extend=False):
    """The body switch_tile's bits and the dispatch behind them send a row of class c to (rows_fast.h, narrow kernel), for a score ring of fr_rows x fr_cols:
    'asm' | 'turbo1' | 'turbo2' (tight copies) | 'turbo1_out' | 'turbo2_out' (copies outside the tight loop: literal-scan vector, spill row) | 'turbo4' |
    'turbo8' | 'ilp2' | 'ilp2_hbm' (a predecessor behind the score ring, gathered from the arena) | 'fast' | 'general'.  words: direction-word job (DIR);
    asm: the assembly loop is on (int16 affine words, ABPOA_HIP_DBG bit 11 clear).  Static rules only: what a body declines at run time (wrap guards, arena
    room, a band whose first vector lies beyond every predecessor's) is not modelled."""
    in_ring = c.dmax < fr_rows                                   # (c.far and c.spill are relative to RR = 16, the plan's fr_rows at every point but one)
    ring128 = fr_cols <= 128
    fastrow = 1 <= c.np <= 4 and in_ring                         # bit 16
    b17 = fastrow and c.np <= 2 and ring128
    b18 = fastrow and c.np >= 3 and ring128
    b20 = 5 <= c.np <= 8 and in_ring and ring128
    b19 = 1 <= c.np <= 8 and c.dmax < GEO_ROWS
    spill = words and c.reach >= fr_rows                         # bit 21; with bit 17: bit 22 instead
    asm_on = asm and words and bits == 16 and gap_mode == 1 and fr_cols == 128 and not extend
    if c.cols == 0:                                              # the straight-line bodies hold one chunk: NV vectors = 64 columns
        if b17 or b18:
            if asm_on and not spill:
                return "asm"
            if b18:
                return "turbo4"
            if spill or c.slow:
                return "turbo%d_out" % c.np
            return "turbo%d" % c.np
        if b20:
            return "turbo8"
    if gap_mode != 0 and b19 and c.cols <= 1:
        return "ilp2" if in_ring else "ilp2_hbm"
    if fastrow and c.ncols <= fr_cols:
        return "fast"
    return "general"


# ---- the points of the table: (golden, family, variant, wb); wb = None: the golden's own band
FAMILY_NAMES = tuple(FAMILIES)
POINTS = [(g, f, v, None) for v in VARIANTS for g in VARIANTS[v][0] for f in FAMILY_NAMES]
# the width switch (in_ring): 24 | 25 in int16, 36 | 37 in int32
SWITCH = [(g, "in_ring", v, W_128[b] + k) for v, b in (("own", 16), ("i32", 32)) for g in GOLDENS for k in (0, 1)]
ALL_POINTS = POINTS + SWITCH


def point_id(pt):
    g, f, v, wb = pt
    return f"{g[4:6]}_{f}_{v}" + ("" if wb is None else f"_w{wb}")


def words_apply(golden, family, variant):
    """Whether abpoa_oracle_dir_walk answers for the point: affine / convex global jobs whose rows have at most DIR_K_MAX = 15 predecessors.  The CPU test
    holds this to the function's own return code; the GPU tests read it here, never from a GPU result."""
    return variant in ("own", "i32") and family not in ("exact16", "exact17")


# ---- floors: rows per class on the oracle, about two thirds of the measured counts (measured: ag / cg, written beside each floor)
def count(classes, **kw):
    """Rows of {row: RowClass} with np in kw['np'] (a range), far / cols in a tuple, dmax (rows back to the farthest predecessor) / slow / spill equal."""
    n = 0
    for c in classes.values():
        if "np" in kw and c.np not in kw["np"]: continue
        if "far" in kw and c.far not in kw["far"]: continue
        if "dmax" in kw and c.dmax != kw["dmax"]: continue
        if "cols" in kw and c.cols not in kw["cols"]: continue
        if "slow" in kw and c.slow != kw["slow"]: continue
        if "spill" in kw and c.spill != kw["spill"]: continue
        n += 1
    return n


STOPS_EARLY = {(g, f, v) for v in ZDROP for g in GOLDENS for f in FAMILY_NAMES if f in JUMP or (g == "s1k_ag_gb" and (v == "extz6" or f.startswith("exact")))}
# `jump`: steps of the oracle's alignment that leave a row through predecessor index 8 and above -- floors for (s1k_ag_gb, s1k_cg_gb); measured 18 / 17 and 17 / 14
WALK_FLOOR = {"own": (12, 11), "i32": (11, 9)}
# `farjump`: steps of the oracle's alignment by length in rows, (16 .. 63, 64 .. 254, 255 and more) -- floors for (s1k_ag_gb, s1k_cg_gb).  Measured at the
# own scoring 6 / 4 / 1 on both, every edge of the family; at the int32 match scores some jumps lose to the path through the graph: 3 / 3 / 1 and 2 / 2 / 0
STEP_FLOOR = {"own": ((4, 3, 1), (4, 3, 1)), "i32": ((2, 2, 1), (1, 1, 0))}
N3_4, N5_8, N1_2 = range(3, 5), range(5, 9), range(1, 3)
# (family, band or None) -> [(class as `count` takes it, floor on s1k_ag_gb, floor on s1k_cg_gb)], at the `own` variant unless the key names another
FLOORS = {
    ("in_ring", None, "own"): [
        (dict(np=N3_4, far=(0,)), 125, 98),                   # measured 188 / 147
        (dict(np=N5_8, far=(0,)), 125, 106),                  # 188 / 160
        (dict(np=range(9, 12), far=(0,)), 20, 15),            # 30 / 23
        (dict(np=N3_4, far=(0,), slow=True), 8, 4),           # 13 / 6
        (dict(np=N5_8, far=(0,), slow=True), 10, 5),          # 15 / 8
    ],
    ("far", None, "own"): [
        (dict(np=N1_2, far=(1,)), 58, 56),                    # 87 / 85      a farthest predecessor 16 .. 63 rows back
        (dict(np=N3_4, far=(1,)), 66, 46),                    # 99 / 69
        (dict(np=N5_8, far=(1,)), 42, 36),                    # 63 / 55
        (dict(np=N1_2, far=(2,)), 18, 14),                    # 27 / 21      ... 64 rows back and more
        (dict(np=N3_4, far=(2,)), 28, 24),                    # 42 / 36
        (dict(np=N5_8, far=(2,)), 4, 4),                      # 7 / 6
        (dict(np=N1_2, spill=True), 180, 159),                # 271 / 239    spill rows: a successor 16 and more rows ahead (270 / 239) or the sink (row_sdist = 255)
        (dict(np=N3_4, spill=True), 25, 14),                  # 38 / 22
        (dict(np=N5_8, spill=True), 10, 8),                   # 16 / 13
    ],
    ("many", None, "own"): [(dict(np=range(9, 12)), 72, 64)],                                                    # 109 / 97
    ("edge", None, "own"): [
        (dict(np=N5_8, dmax=15), 21, 17),                     # 32 / 26      either side of `dk < RR` in tile bit 20 ...
        (dict(np=N5_8, dmax=16), 62, 52),                     # 94 / 79
        (dict(np=N5_8, dmax=17), 76, 64),                     # 115 / 96     ... and the first distance whose ring slot holds another row
        (dict(np=N3_4, dmax=17), 50, 38),                     # 75 / 57
        (dict(np=N1_2, dmax=17), 23, 24),                     # 35 / 37
        (dict(np=N5_8, dmax=64), 37, 31),                     # 56 / 47      the first distance behind the geometry ring (bit 19)
    ],
    # (every count 1 .. 8 on at least 20 in-ring rows: the floor the table was designed to; measured 790 295 91 41 34 35 34 28 / 784 168 45 30 28 29 29 25)
    ("exact", None, "own"): [(dict(np=(k,), far=(0,)), 20, 20) for k in range(1, 9)] + [(dict(np=(15,)), 4, 4)],   # 15 predecessors: 7 / 6
    ("exact16", None, "own"): [(dict(np=(15,)), 4, 4), (dict(np=(16,)), 4, 4)],                                  # 16: 6 / 7
    ("exact17", None, "own"): [(dict(np=(15,)), 4, 4), (dict(np=(17,)), 4, 4)],                                  # 17: 7 / 7
    # the width switch: rows of 65-128 columns
    ("in_ring", 24, "own"): [(dict(np=N3_4, cols=(1,)), 51, 38), (dict(np=N5_8, cols=(1,)), 61, 73)],            # 77 / 58, 92 / 110
    ("in_ring", 25, "own"): [(dict(np=N3_4, cols=(1,)), 65, 49), (dict(np=N5_8, cols=(1,)), 70, 80)],            # 98 / 74, 105 / 121
    ("in_ring", 36, "i32"): [(dict(np=N3_4, cols=(1,)), 96, 90), (dict(np=N5_8, cols=(1,)), 93, 100)],           # 145 / 135, 140 / 150
    ("in_ring", 37, "i32"): [(dict(np=N3_4, cols=(1,)), 96, 90), (dict(np=N5_8, cols=(1,)), 92, 99)],            # 144 / 136, 139 / 149
}


# ---- read-sets whose graphs grow high in-degree by themselves (tests/test_gpu_narrow_bodies.py through the device-resident driver, tests/test_host_msa.py
#      against the reference's command-line tool): 50 x 300 at 30 % error, 50 x 300 at 4 / 4 / 16 % substitutions / deletions / insertions, 20 x 300 at 30 %
AFFINE = dict(gap_open1=4, gap_open2=0, gap_ext1=2)
KINDS = {"err30": dict(n_reads=50, err=0.30), "ins16": dict(n_reads=50, rates=(0.04, 0.04, 0.16)), "first_pass": dict(n_reads=20, err=0.30)}
N_SETS = {"err30": 4, "ins16": 4, "first_pass": 1}
SEED, LENGTH = 4242, 300
FORMS = {"all_rounds": {}, "lockstep": {"ABPOA_HIP_LOCKSTEP": "1"}, "dbg2048": {"ABPOA_HIP_DBG": "2048"}}      # forms of the device-resident driver, with their switches
EXTRA = {("err30", "devsync"): {"ABPOA_HIP_DEVSYNC": "1"}}      # one run of ONE set (the first of the kind)


def read_sets(kind):
    from abpoa_amd import synth
    return [synth.make_read_set(SEED, i, length=LENGTH, **KINDS[kind]) for i in range(N_SETS[kind])]


def walk_steps(case, o):
    """Row distance of every step of the oracle's alignment from one graph row to the next (cigar words of match and deletion carry the node id above bit 34)."""
    row_of = {int(nid): r for r, nid in enumerate(case.row_node_id)}
    rows = [row_of[int(w) >> 34] for w in o.cigar if int(w) & 15 in (0, 2)]
    return [abs(a - b) for a, b in zip(rows, rows[1:])]
