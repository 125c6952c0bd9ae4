"""CPU: conditions on the INPUTS of tests/test_gpu_wide_pred_bodies.py (table: tests/wide_preds.py), checked on the oracle's bands, on the launch plan and on the
word model -- that the skip-edge families at the wide loop's bands do give every all-chunk body (3 .. 9 and 11 chunks) rows of every class the table claims
(predecessor count, reach behind the 16- and the 4-row ring, which of the first two predecessors is far, spill rows as far predecessors), that the rows the
wide kernels must decline as "not eligible" are counted, that the plan answers at every point what tests/wide_bands.py says (also under ABPOA_HIP_RING_ROWS=4
and ABPOA_HIP_NOXL=1), that the cut and lengthened queries make the oracle's walk step where the table says (predecessor index 8 and above, behind both
rings, past 254 rows, through insertion runs longer than a slice's slack), and that oracle/dir_model.c walks the oracle's own cigar at every point.  The GPU
tests could otherwise pass without running what they name."""
import collections
import ctypes as C
import os
import re

import numpy as np
import pytest

import helpers as H
import narrow_preds as NP
import wide_bands as WB
import wide_preds as WP
from test_local_regimes import walk_pred_indices
from test_wide_band_regimes import _hook, chunk_counts

COMBO_IDS = [f"{g}_i{b}" for g, b in WP.COMBOS]
_RUN = {}


def run(golden, family, bits, wb):
    """(FlatCase, {row: WRow}, the oracle's cigar-side output without planes) of a table point, computed once; the planes are dropped."""
    k = (golden, family, bits, wb)
    if k not in _RUN:
        c = H.FlatCase(WP.case_dict(golden, family, bits, wb))
        o = H.run_oracle(c)
        assert o.rc == 0 and o.status == 0 and o.bits == bits, k
        rows = WP.wide_rows(c, o)
        o.planes = None
        _RUN[k] = (c, rows, o)
    return _RUN[k]


@pytest.mark.parametrize("key", list(WP.MEASURED), ids=[f"{f}_{n}" for f, n in WP.MEASURED])
def test_every_body_holds_rows_of_every_class(key):
    """Per class of the table and per all-chunk body: the rows over the table's bands, per golden and score width, against two thirds of the measured count."""
    family, name = key
    rr = WP.CLASS_RR[family]
    for combo in WP.COMBOS:
        got = collections.Counter()
        for wb in WP.BANDS[combo]:
            for x in run(combo[0], family, combo[1], wb)[1].values():
                if name in WP.classes_of(x, rr):
                    got[x.body] += 1
        counts = tuple(got[b] for b in WP.BODIES)
        floors = tuple(WP.floor_of(m) for m in WP.MEASURED[key][combo])
        print(f"{combo[0]} int{combo[1]} {family} {name} (ring of {rr} rows), rows per body {WP.BODIES}: {counts} (floors {floors})")
        assert min(floors) >= 4, (key, combo, floors)
        assert all(n >= f for n, f in zip(counts, floors)), (key, combo, counts, floors)


def test_cells_left_out_are_empty_by_arithmetic():
    """`edge4`: no row of 5-8 predecessors has its farthest 3 or 4 rows back (fewer distinct distances than predecessors); 5 back gives exactly five."""
    for combo in WP.COMBOS:
        for wb in WP.BANDS[combo]:
            rows = run(combo[0], "edge4", combo[1], wb)[1]
            assert not any(x.np >= 5 and x.dmax <= 4 for x in rows.values())
            assert {x.np for x in rows.values() if x.dmax == 5 and x.np >= 5} == {5}
    assert ("edge4", "d3_5_8") in WP.LEFT_OUT and ("edge4", "d4_5_8") in WP.LEFT_OUT


@pytest.mark.parametrize("golden,bits", WP.COMBOS, ids=COMBO_IDS)
def test_not_eligible_rows_per_point(golden, bits):
    """Rows with more than 8 predecessors or a predecessor 64 and more rows back, per point: a property of the graph, the table's number at every band; `far`
    and `edge` have both kinds of them, `many` and `in_ring` only rows of 9-11 predecessors.  The diagnostic build's counter is held to this number
    (tests/test_gpu_device_msa.py::test_long_read_rows_take_the_all_chunk_bodies)."""
    gi = WP.GOLDENS.index(golden)
    for family, wb in WP.pred_points(golden, bits) + [(f, wb) for wb in WP.BANDS[(golden, bits)] for f in ("edge4",)]:
        if family in WP.WALK_FAMILIES:
            continue
        rows = run(golden, family, bits, wb)[1]
        n = WP.not_eligible(rows)
        many = sum(1 for x in rows.values() if x.np > 8)
        behind = sum(1 for x in rows.values() if x.dmax >= WP.GEO_ROWS)
        print(f"{golden} int{bits} {family} wb={wb}: {n} rows not eligible ({many} of 9 and more predecessors, {behind} with one 64 and more rows back)")
        assert n == WP.NOT_ELIGIBLE[family][gi], (golden, bits, family, wb, n)
        if family in ("far", "edge"):
            assert behind == n > 0 and many == 0
        if family in ("many", "in_ring"):
            assert many == n > 0 and behind == 0


@pytest.mark.parametrize("golden,bits", WP.COMBOS, ids=COMBO_IDS)
def test_plan_at_every_point(golden, bits):
    """abpoa_hip__wide_plan at every point == tests/wide_bands.py's table, every point inside the wide loop's range; with ABPOA_HIP_RING_ROWS=4 a 4-row ring
    at every band; with ABPOA_HIP_NOXL=1 the 448-column kernel at 196 and 215; one past the widest body rows of 12 chunks occur."""
    for family, wb in WP.pred_points(golden, bits):
        c = run(golden, family, bits, wb)[0]
        got, _ = _hook(c, bits)
        assert got[3] == WP.RR and got[0] == 1 and got[1] == 40 <= wb <= got[2], (golden, bits, family, wb, got)
        if family not in NP.JUMP:                  # (the cut queries are shorter: their plan may keep the 448-column ring where the table's 1 kb query has 704)
            assert got[:3] == WB.plan(golden, bits, wb)[:3], (golden, bits, family, wb, got)
        assert NP.half_width(c) == wb
    for family in WP.RING4_FAMILIES:
        for wb in WP.BANDS[(golden, bits)]:
            got, _ = _hook(run(golden, family, bits, wb)[0], bits, ABPOA_HIP_RING_ROWS=4)
            assert got == WB.plan(golden, bits, wb)[:3] + (WP.RR4,), (golden, bits, family, wb, got)
    for family in WP.NOXL_FAMILIES:
        for wb in WP.NOXL_BANDS:
            got, _ = _hook(run(golden, family, bits, wb)[0], bits, ABPOA_HIP_NOXL=1)
            assert got == WB.R448 and wb <= got[2], (golden, bits, family, wb, got)
            rows = run(golden, family, bits, wb)[1]
            assert sum(1 for x in rows.values() if x.nch == 7 and x.eligible) >= 100
    wb, family = WP.ONE_PAST
    if (family, wb, golden, bits) in WP.LEFT_OUT:
        assert not WB.fast_loops(golden, bits, wb)
    else:
        rows = run(golden, family, bits, wb)[1]
        wide = {r for r, x in rows.items() if x.nch >= 12}
        n = sum(1 for r, x in rows.items() if x.eligible and x.body and any(r - d in wide for d in x.dist))
        print(f"{golden} int{bits} {family} wb={wb}: {len(wide)} rows of 12 chunks and more, {n} eligible rows with such a predecessor")
        assert len(wide) >= 20 and n >= 10
    for wb in WP.SWITCH[bits]:
        assert WB.plan(golden, bits, wb)[2] == (215 if wb == WP.SWITCH[bits][0] else 343)


@pytest.mark.parametrize("golden,bits", WP.COMBOS, ids=COMBO_IDS)
def test_walk_families_step_where_the_table_says(golden, bits):
    """`jump`: steps through predecessor index 8 .. 10; `farjump`: steps of 16-63, 64-254 and 255 and more rows; `ins`: at least three insertion runs longer
    than DIR_TRI_SLACK plus the slice's alignment padding (both read from backtrack_dir.h); no other family has any of the three."""
    gi, v = WP.GOLDENS.index(golden), WP.VARIANT[bits]
    src = open(os.path.join(H.ROOT, "abpoa_amd", "csrc", "backtrack_dir.h")).read()
    slack = int(re.search(r"constexpr int DIR_TRI_SLACK = (\d+);", src).group(1))
    align_bytes = int(re.search(r"constexpr int ALIGN = (\d+) / DB;", src).group(1))
    pad = align_bytes // 2 - 1                      # words of 2 bytes (int16 affine) or 4: up to 7 columns of padding to the left
    assert (slack, align_bytes) == (9, 16)
    for wb in WP.WALK_BANDS[bits]:
        c, _, o = run(golden, "jump", bits, wb)
        idx = walk_pred_indices(c, o)
        n = sum(1 for k in idx if k >= 8)
        print(f"{golden} int{bits} jump wb={wb}: {n} steps through predecessor index >= 8, the highest {max(idx)}")
        assert n >= WP.WALK_FLOOR[v][gi] and max(idx) == 10
        c, _, o = run(golden, "farjump", bits, wb)
        st = NP.walk_steps(c, o)
        got = (sum(16 <= k < 64 for k in st), sum(64 <= k < 255 for k in st), sum(k >= 255 for k in st))
        print(f"{golden} int{bits} farjump wb={wb}: steps of 16-63 / 64-254 / 255+ rows: {got}, the longest {max(st)}")
        assert all(a >= b for a, b in zip(got, WP.STEP_FLOOR[v][gi]))
        c, _, o = run(golden, "ins", bits, wb)
        runs = sorted(k for k in WP.insertion_runs(o) if k > slack + pad)
        print(f"{golden} int{bits} ins wb={wb}: insertion runs longer than {slack} + {pad} columns: {runs}")
        assert len(runs) >= WP.INS_FLOOR, (golden, bits, wb, runs)
        assert max(NP.walk_steps(c, o)) <= 11 and max(walk_pred_indices(c, o)) < 8
    wb = WP.BANDS[(golden, bits)][2]
    for f in WP.PRED_FAMILIES:
        c, _, o = run(golden, f, bits, wb)
        assert max(NP.walk_steps(c, o)) <= 11 and max(walk_pred_indices(c, o)) < 8 and max(WP.insertion_runs(o) + [0]) <= slack + pad, (golden, bits, f)


def model_words(case):
    """The direction words oracle/dir_model.c derives from the oracle's scores, [n_rows, width], and the oracle's bands."""
    lib = H.oracle_lib(); case.reset()
    res, tr = H.Result(), H.OracleTrace()
    assert lib.abpoa_oracle_align(C.byref(case.sc), C.byref(case.pb), C.byref(res), C.byref(tr)) == 0
    lib.abpoa_oracle_dir_words.argtypes = [C.POINTER(H.Scoring), C.POINTER(H.Problem), C.POINTER(H.OracleTrace), C.c_int, C.c_int, C.POINTER(C.c_uint32)]
    mw = np.zeros((case.n_rows, tr.width), np.uint32)
    rc = lib.abpoa_oracle_dir_words(C.byref(case.sc), C.byref(case.pb), C.byref(tr), res.best_row, res.best_col, mw.ctypes.data_as(C.POINTER(C.c_uint32)))
    beg = np.ctypeslib.as_array(tr.dp_beg, (case.n_rows,)).copy(); end = np.ctypeslib.as_array(tr.dp_end, (case.n_rows,)).copy()
    lib.abpoa_oracle_free_trace(C.byref(tr)); H._libc.free(C.cast(res.cigar, C.c_void_p))
    assert rc == 0
    return mw, beg, end


# words of `in_ring` at wb = 130 whose kM or kE field names predecessor 6, 7 or 8, per (golden, width): two thirds of the measured counts written beside them
KM_FLOOR = {WP.AG16: 12300, WP.AG32: 10900, WP.CG16: 10000, WP.CG32: 8600}      # measured 18550, 16361, 15006, 12933


@pytest.mark.parametrize("golden,bits", WP.COMBOS, ids=COMBO_IDS)
def test_words_name_the_sixth_to_eighth_predecessor(golden, bits):
    c = run(golden, "in_ring", bits, WP.KM_BAND)[0]
    mw, beg, end = model_words(c)
    n = 0
    for r in range(1, c.n_rows - 1):
        w = mw[r, max(int(beg[r]), 0):int(end[r]) + 1]
        ks = [w & 15, (w >> 4) & 15] + ([(w >> 8) & 15] if c.sc.gap_mode == 2 else [])
        n += int(np.any([(k >= 6) & (k <= 8) for k in ks], axis=0).sum())
    print(f"{golden} int{bits} in_ring wb={WP.KM_BAND}: {n} words with kM or kE of 6 .. 8 (floor {KM_FLOOR[(golden, bits)]})")
    assert n >= KM_FLOOR[(golden, bits)] > 0


@pytest.mark.parametrize("golden,bits", WP.COMBOS, ids=COMBO_IDS)
def test_oracle_against_the_word_model(golden, bits):
    """abpoa_oracle_dir_walk answers at every point (rows of 15 predecessors and fewer: `many` and `exact` are in), and its walk over the words derived from
    the oracle's scores is the oracle's cigar, field for field."""
    pts = WP.pred_points(golden, bits) + [("edge4", wb) for wb in WP.BANDS[(golden, bits)]]
    for family, wb in pts:
        c = run(golden, family, bits, wb)[0]
        assert int(np.diff(c.pred_off[:c.n_rows + 1]).max()) <= 15 and WP.words_apply(family)
        rc, a, b, _ = H.run_dir_model(c)
        assert rc == 0, (golden, bits, family, wb, rc)
        for k in a:
            assert np.array_equal(a[k], b[k]), (golden, bits, family, wb, k)


@pytest.mark.parametrize("golden", WP.GOLDENS)
def test_mixed_launch_and_extension_points(golden):
    """The mixed launch: every family at wb = 12, wf = 0.16 beside one short golden -- w = 20 (narrow kernel) beside w of 70 and more (wide loop), one plan
    for all.  Extension mode with z-drop 6 at wb = 196: `farjump` stops early behind a step of 16 rows, `far` has 100 and more computed rows of 5 chunks and more."""
    m = WP.MIXED
    short = H.FlatCase(H.rescored(H.first_golden(m["short"][golden]), WB.point(golden, 16, 54), m["wb"], m["wf"]))
    assert NP.half_width(short) == 20
    ws = []
    for f in WP.ALL_FAMILIES:
        d = WP.case_dict(golden, f, 16, m["wb"])
        d["wf"] = np.array([m["wf"]], np.float32)
        c = H.FlatCase(d)
        o = H.run_oracle(c)
        assert o.status == 0 and o.bits == 16
        ws.append(NP.half_width(c))
    print(f"{golden} mixed launch: w = 20 and {sorted(set(ws))}")
    assert min(ws) >= 70 and max(ws) <= 343
    got, _ = _hook(max([short], key=lambda x: x.qlen), 16, n_aln=len(ws) + 1)
    variant, wb, fams = WP.EXTZ
    stopped = 0
    for f in fams:
        c = H.FlatCase(NP.case_dict(golden, f, variant, wb))
        o = H.run_oracle(c)
        assert o.status == 0 and c.sc.align_mode == 2 and c.sc.zdrop == NP.ZDROP[variant]
        cnt = chunk_counts(o)
        n_done = int((o.dp_beg_sn[1:c.n_rows - 1] >= 0).sum())
        stopped += n_done < c.n_rows - 2
        print(f"{golden} {variant} {f} wb={wb}: {n_done} of {c.n_rows - 2} rows computed, chunks {sorted(cnt.items())}")
        assert _hook(c, 16)[0][0] == 1 and 40 <= wb <= _hook(c, 16)[0][2]
        if f == "farjump":                         # (LEFT_OUT: no row of 5 chunks before its stop)
            assert 60 <= n_done < c.n_rows - 2 and min(cnt) >= 3 and max(NP.walk_steps(c, o)) >= 16 and ("farjump", "extz", "5 chunks") in WP.LEFT_OUT
        else:
            assert sum(v for n, v in cnt.items() if n >= 5) >= 100
    assert stopped >= 1
