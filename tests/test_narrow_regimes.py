"""CPU: conditions on the INPUTS of tests/test_gpu_narrow_bodies.py (table: tests/narrow_preds.py), checked on the oracle's bands, on the launch plan and on
the word model -- that the skip-edge families do give rows of every class the table claims (predecessor count, reach, width, literal-scan vector, spill row)
and of every body predicted_body names, that the plan answers a 16 x 128 score ring at every point meant for the straight-line bodies and 192 columns one band
past W_128, that the z-drop points stop where the table says, and that oracle/dir_model.c walks the oracle's own cigar wherever the word plane applies.  The
GPU tests could otherwise pass without running the bodies they name."""
import collections
import ctypes as C

import numpy as np
import pytest

import helpers as H
import narrow_preds as NP
from abpoa_amd import ffi

_RUN = {}
IDS = [NP.point_id(p) for p in NP.ALL_POINTS]


def run(pt):
    """(FlatCase, oracle output with trace, {row: RowClass}) of a table point, computed once."""
    if pt not in _RUN:
        g, f, v, wb = pt
        c = H.FlatCase(NP.case_dict(g, f, v, wb))
        o = H.run_oracle(c)
        assert o.rc == 0 and o.status == 0 and o.bits == NP.VARIANTS[v][1], pt
        _RUN[pt] = (c, o, NP.row_classes(c, o))
    return _RUN[pt]


def hook(case, bits, n_aln=1):
    """abpoa_hip__narrow_plan -> (fr_rows, fr_cols, bt_bytes_tail) for a launch of n_aln alignments like `case`."""
    out = (C.c_int * 4)()
    ffi.lib().abpoa_hip__narrow_plan(C.byref(case.sc), case.qlen, bits, n_aln, out)
    return out[0], out[1], out[2]


def body_counts(pt, words, asm):
    c, o, cl = run(pt)
    rows, cols, _ = hook(c, o.bits)
    return collections.Counter(NP.predicted_body(x, rows, cols, bits=o.bits, gap_mode=c.sc.gap_mode, words=words, asm=asm, extend=c.sc.align_mode == 2)
                               for x in cl.values())


@pytest.mark.parametrize("key", list(NP.FLOORS), ids=[f"{f}_{v}" + ("" if wb is None else f"_w{wb}") for f, wb, v in NP.FLOORS])
def test_every_class_the_table_claims_is_reached(key):
    family, wb, variant = key
    for gi, golden in enumerate(NP.GOLDENS):
        c, o, cl = run((golden, family, variant, wb))
        assert NP.half_width(c) == (NP.OWN_W[golden] if wb is None else wb) < 40
        for kw, *floors in NP.FLOORS[key]:
            n = NP.count(cl, **kw)
            print(f"{golden} {family} {variant} wb={wb} {kw}: {n} rows (floor {floors[gi]})")
            assert n >= floors[gi], (golden, key, kw, n)


@pytest.mark.parametrize("pt", NP.ALL_POINTS, ids=IDS)
def test_point_runs_on_the_oracle_and_stops_where_the_table_says(pt):
    """Status 0, the variant's score width, a cigar; rows behind a z-drop stop are not computed exactly at the points of STOPS_EARLY (both kinds occur per
    z-drop value); the graph-side classes do not depend on the variant."""
    g, f, v, wb = pt
    c, o, cl = run(pt)
    n_done = int((o.dp_beg_sn[1:c.n_rows - 1] >= 0).sum())
    assert o.n_cigar > 0
    assert (n_done < c.n_rows - 2) == ((g, f, v) in NP.STOPS_EARLY), (pt, n_done)
    full, done_min, cigar_min = NP.CUT_SIZES.get(f, (990, 500, 400))
    if (g, f, v) in NP.STOPS_EARLY:
        assert n_done >= done_min and o.n_cigar >= cigar_min
    else:
        assert o.n_cigar >= full
    assert NP.half_width(c) == (wb if wb is not None else NP.CUT_W[f][NP.GOLDENS.index(g)] if f in NP.CUT_W else NP.OWN_W[g])
    own = run((g, f, "own", None))[2]
    assert all((own[r].np, own[r].far, own[r].spill) == (x.np, x.far, x.spill) for r, x in cl.items())


@pytest.mark.parametrize("variant", list(NP.WALK_FLOOR))
def test_jump_family_walks_through_the_ninth_predecessor_and_beyond(variant):
    """The oracle's alignment of `jump` leaves rows through predecessor index 8, 9 and 10 (the row's list holds eleven; row_pd holds eight distances); at the
    other families it never does, which is why the table has this one."""
    from test_local_regimes import walk_pred_indices
    for gi, golden in enumerate(NP.GOLDENS):
        c, o, _ = run((golden, "jump", variant, None))
        idx = walk_pred_indices(c, o)
        n = sum(1 for k in idx if k >= 8)
        print(f"{golden} jump {variant}: {n} steps through predecessor index >= 8, the highest {max(idx)}")
        assert n >= NP.WALK_FLOOR[variant][gi] and max(idx) == 10, (golden, variant, n)
        for f in NP.FAMILY_NAMES:      # (rows of 15-17 predecessors included: the walk leaves them through one of their first four)
            if f != "jump":
                c2, o2, _ = run((golden, f, variant, None))
                assert max(walk_pred_indices(c2, o2)) < 8, (golden, f)


@pytest.mark.parametrize("variant", list(NP.STEP_FLOOR))
def test_farjump_family_walks_over_both_rings(variant):
    """The oracle's alignment of `farjump` takes steps of 16-63 rows (behind the score ring), of 64-254 (behind the geometry ring) and -- but for int32 convex
    -- one of 300 (past a byte of row_pd); at every other family its longest step is 11 rows, which is why the table has this one."""
    for gi, golden in enumerate(NP.GOLDENS):
        c, o, _ = run((golden, "farjump", variant, None))
        st = NP.walk_steps(c, o)
        got = (sum(16 <= k < 64 for k in st), sum(64 <= k < 255 for k in st), sum(k >= 255 for k in st))
        print(f"{golden} farjump {variant}: steps of 16-63 / 64-254 / 255+ rows: {got}, the longest {max(st)}")
        assert all(n >= f for n, f in zip(got, NP.STEP_FLOOR[variant][gi])), (golden, variant, got)
        if variant == "own":
            assert sorted(k for k in st if k >= 16) == [16, 16, 17, 17, 63, 63, 64, 64, 70, 70, 300]
        for f in NP.FAMILY_NAMES:
            if f != "farjump":
                c2, o2, _ = run((golden, f, variant, None))
                assert max(NP.walk_steps(c2, o2)) <= 11, (golden, f)


def test_both_outcomes_occur_at_each_zdrop():
    for v in NP.ZDROP:
        stops = {(g, f) for g, f, vv in NP.STOPS_EARLY if vv == v}
        assert stops and len(stops) < len(NP.GOLDENS) * len(NP.FAMILY_NAMES)


# bodies predicted_body must name at a point, per job form: (family, wb, variant, words, asm) -> [(body, floor ag, floor cg)], about two thirds of what it
# names today (in_ring with words: 1137 asm, 184 turbo8, 30 general on ag; 138 turbo4, 106 turbo8, 38 turbo1|2_out on cg; far, cg: 209 ilp2_hbm, 198 turbo1_out,
# 63 general; in_ring at w = 24, cg: 417 ilp2, 89 turbo4, 50 turbo8; at w = 25: 1122 ilp2, 23 general; int32 at w = 36 | 37, cg: 1056 | 1041 ilp2)
BODY_FLOORS = {
    ("in_ring", None, "own", True, True): [("asm", 740, 0), ("turbo4", 0, 84), ("turbo8", 120, 68), ("general", 20, 15)],
    ("in_ring", None, "own", False, False): [("turbo4", 125, 84), ("turbo8", 120, 68), ("turbo1_out", 20, 20), ("turbo2_out", 8, 4), ("general", 20, 15)],
    ("far", None, "own", True, True): [("ilp2_hbm", 160, 130), ("turbo1_out", 100, 80), ("general", 50, 40)],
    ("many", None, "own", True, True): [("general", 72, 64)],
    ("exact", None, "own", True, False): [("turbo4", 85, 40), ("turbo8", 85, 56)],
    ("in_ring", 24, "own", True, False): [("ilp2", 300, 250), ("turbo4", 60, 50), ("turbo8", 60, 30)],
    ("in_ring", 25, "own", True, True): [("ilp2", 850, 700), ("general", 20, 15)],
    ("in_ring", 36, "i32", True, False): [("ilp2", 600, 700)],
    ("in_ring", 37, "i32", True, False): [("ilp2", 600, 700)],
}


@pytest.mark.parametrize("key", list(BODY_FLOORS), ids=[f"{f}_{v}_w{wb}_{'words' if w else 'records'}{'_asm' if a else ''}" for f, wb, v, w, a in BODY_FLOORS])
def test_predicted_bodies(key):
    """predicted_body over the oracle's rows with the plan's ring: the bodies the table's docstring names for a point do get the rows; at one band past
    W_128 no row is predicted for a straight-line body or the assembly loop."""
    family, wb, variant, words, asm = key
    for gi, golden in enumerate(NP.GOLDENS):
        cnt = body_counts((golden, family, variant, wb), words, asm)
        print(f"{golden} {key}: {sorted(cnt.items())}")
        for body, *floors in BODY_FLOORS[key]:
            assert cnt[body] >= floors[gi], (golden, key, body, cnt[body])
        if wb in (25, 37):
            assert set(cnt) <= {"ilp2", "ilp2_hbm", "fast", "general"} and (cnt["ilp2_hbm"] > 0) == ((golden, variant) == ("s1k_cg_gb", "i32")), (golden, key, cnt)
        if golden == "s1k_cg_gb" or not (words and asm):
            assert cnt["asm"] == 0


@pytest.mark.parametrize("pt", NP.ALL_POINTS, ids=IDS)
def test_plan_is_16_rows_of_128_columns_up_to_the_switch(pt):
    g, f, v, wb = pt
    c, o, _ = run(pt)
    rows, cols, tail = hook(c, o.bits)
    w = NP.half_width(c)
    assert cols == (128 if w <= NP.W_128[o.bits] else 192) and tail > 0, (pt, rows, cols, tail)
    assert rows == (NP.RR if cols == 128 else NP.RING_ROWS_192[(g, o.bits)]), (pt, rows, cols)
    assert (cols == 192) == (wb is not None and wb == NP.W_128[o.bits] + 1)


@pytest.mark.parametrize("golden,variant", [(g, v) for v in ("own", "i32") for g in NP.GOLDENS], ids=lambda x: x)
def test_width_switch_is_the_plans(golden, variant):
    """Scanned through the hook, w = 1 .. 39: 16 rows of 128 ring columns up to W_128 (24 in int16, 36 in int32), 192 columns from the next band on -- in 16 rows,
    int32 convex in 8."""
    bits = NP.VARIANTS[variant][1]
    c = H.FlatCase(NP.case_dict(golden, "in_ring", variant, 10))
    seen = {}
    for wb in range(1, 40):
        c.sc.wb = wb
        seen[wb] = hook(c, bits)
    first_192 = min(wb for wb, p in seen.items() if p[1] > 128)
    print(f"{golden} int{bits}: 192 ring columns from w = {first_192}")
    assert first_192 == NP.W_128[bits] + 1
    r192 = NP.RING_ROWS_192[(golden, bits)]
    assert all(p[:2] == (16, 128) for wb, p in seen.items() if wb < first_192) and all(p[:2] == (r192, 192) for wb, p in seen.items() if wb >= first_192)
    assert (golden, "in_ring", variant, first_192 - 1) in NP.SWITCH and (golden, "in_ring", variant, first_192) in NP.SWITCH


@pytest.mark.parametrize("pt", NP.ALL_POINTS, ids=IDS)
def test_oracle_against_the_word_model(pt):
    """Where abpoa_oracle_dir_walk answers, its walk over the words derived from the oracle's scores is the oracle's cigar, field for field.  It may answer
    EINVAL only at linear gaps, in extension mode and on the graphs with a row of 16 / 17 predecessors -- words_apply says exactly that -- and never at an
    affine or convex int16 point of w <= 24 with at most 15 predecessors per row."""
    g, f, v, wb = pt
    c, o, _ = run(pt)
    rc, a, b, _ = H.run_dir_model(c)
    applies = NP.words_apply(g, f, v)
    max_np = int(np.diff(c.pred_off[:c.n_rows + 1]).max())
    assert applies == (c.sc.gap_mode != 0 and c.sc.align_mode == 0 and max_np <= 15), (pt, max_np)
    assert rc == (0 if applies else -2), (pt, rc)
    if f == "exact16" or f == "exact17":
        assert max_np == int(f[5:])
    if f == "exact":
        assert max_np == 15
    if not applies:
        return
    from scoring_points import Point
    assert Point("p", "x", gap_open1=c.sc.gap_open1, gap_ext1=c.sc.gap_ext1, gap_open2=c.sc.gap_open2, gap_ext2=c.sc.gap_ext2).dir_usable()
    for k in a:
        assert np.array_equal(a[k], b[k]), (pt, k)
