"""CPU: conditions on the INPUTS of tests/test_gpu_local_bodies.py, checked on the oracle and the graphs -- that the re-queried local goldens of
tests/local_widths.py have the chunk counts, bodies and team shares the table names, rows with enough and old enough predecessors for the arena gather and
the loop behind the eighth predecessor, row maxima tied between chunks, and scoring points on both sides of the int16 gate.  No kernel result can satisfy any
of them for the GPU tests, which could otherwise pass without running the code they name.  Also the home of the shared case builder."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import local_widths as LW

_GOLD, _CASES = {}, {"golden": None, "items": {}}


def golden(name):
    if name not in _GOLD:
        _GOLD[name] = H.first_golden(name)
    return _GOLD[name]


def local_case(name, qlen, period=None, skips=(), pt=None):
    """(FlatCase, the oracle's output with planes) of golden `name` re-queried (and re-scored at point `pt`), computed once; one golden's are kept at a time."""
    if _CASES["golden"] != name:
        _CASES["golden"], _CASES["items"] = name, {}
    key = (qlen, period, tuple(skips), pt.name if pt else None)
    items = _CASES["items"]
    if key not in items:
        d = H.requeried(golden(name), qlen, period, skips)
        if pt is not None:
            d = H.rescored(d, pt)
        c = H.FlatCase(d)
        o = H.run_oracle(c)
        assert o.rc == 0 and o.status == 0
        items[key] = (c, o)
    return items[key]


def h_rows(c, o):
    """H of rows 1 .. n_rows - 2 over columns 0 .. qlen, from the oracle's compacted planes (unbanded local: every row starts at column 0)."""
    out = np.zeros((c.n_rows - 2, c.qlen + 1), np.int64)
    for r in range(1, c.n_rows - 1):
        assert o.dp_beg_sn[r] == 0
        out[r - 1] = o.planes[int(o.row_off[r]):int(o.row_off[r]) + c.qlen + 1]
    return out


def tie_counts(c, o):
    """(rows whose maximum H lies in more than one 64-column chunk, in more than one column, rows that reach the alignment's best score)"""
    h = h_rows(c, o)
    mx = h.max(1)
    cols = [np.nonzero(h[r] == mx[r])[0] for r in range(len(h))]
    return sum(len(set(x // 64)) > 1 for x in cols), sum(len(x) > 1 for x in cols), int((mx == o.best_score).sum())


def walk_pred_indices(c, o):
    """For every step of the oracle's alignment from one graph row to the next (cigar words of match and deletion carry the node id above bit 34): the
    position of the row stepped to in the predecessor list of the row stepped from."""
    row_of = {int(nid): r for r, nid in enumerate(c.row_node_id)}
    rows = [row_of[int(w >> np.uint64(34))] for w in o.cigar if int(w) & 15 in (0, 2)]
    out = []
    for a, b in zip(rows, rows[1:]):
        r, p = max(a, b), min(a, b)
        out.append(c.pred_row[c.pred_off[r]:c.pred_off[r + 1]].tolist().index(p))
    return out


def test_goldens_are_what_the_table_says():
    for name in LW.GOLDENS:
        g = golden(name)
        p = LW.point(name).params() if name in LW.NUCLEOTIDE else None
        assert int(g["n_rows"][0]) == LW.N_ROWS[name] and int(g["align_mode"][0]) == 1 and int(g["wb"][0]) < 0
        assert int(g["gap_mode"][0]) == (1 if name == "ragged_ag_loc" else 2)
        if p is not None:      # the nucleotide goldens' own scoring is what point() rebuilds: re-scoring with it changes nothing
            d = H.rescored(g, LW.point(name))
            assert all(np.array_equal(d[k], g[k]) for k in H._INPUT_KEYS)
    assert int(golden("aa_blosum_loc")["m"][0]) == 27


def test_requeried_leaves_the_golden_alone_and_composes_with_rescored():
    g = golden("ragged_cg_loc")
    n, q = int(g["n_rows"][0]), int(g["qlen"][0])
    same = H.requeried(g, q, skips=[(1, n + 5, (1,))])      # (a skip list that names no row: the CSR rebuild alone)
    assert all(np.array_equal(same[k], g[k]) for k in H._INPUT_KEYS)
    d = H.requeried(g, 575, 100, LW.SKIPS)
    assert len(d["query"]) == 575 and np.array_equal(d["query"][:100], g["query"][:100]) and np.array_equal(d["query"][100:200], g["query"][:100])
    po, pr, oo, orow = d["pred_off"], d["pred_row"], d["out_off"], d["out_row"]
    assert len(po) == len(g["pred_off"]) and po[-1] == len(pr) == len(orow) == oo[-1]
    for r in range(n):
        own = g["pred_row"][g["pred_off"][r]:g["pred_off"][r + 1]]
        mine = pr[po[r]:po[r + 1]]
        assert np.array_equal(mine[:len(own)], own) and len(set(mine.tolist())) == len(mine) and (r == 0 or (mine < r).all())
    edges = sorted((int(p), r) for r in range(n) for p in pr[po[r]:po[r + 1]])
    assert edges == sorted((p, int(r)) for p in range(n) for r in orow[oo[p]:oo[p + 1]])
    assert set(pr[po[60]:po[61]].tolist()) >= {58, 57, 56, 54, 50, 48, 42, 40, 30}
    a, b = H.rescored(H.requeried(g, 192, skips=LW.SKIPS), LW.asym_point("ragged_cg_loc")), H.requeried(H.rescored(g, LW.asym_point("ragged_cg_loc")), 192, skips=LW.SKIPS)
    assert all(np.array_equal(a[k], b[k]) for k in H._INPUT_KEYS)


@pytest.mark.parametrize("name", LW.GOLDENS)
def test_every_width_has_the_chunks_body_and_shares_of_the_table(name):
    """rc 0 and 16 bits at every point; the chunk count the oracle's rows have is the table's, and the table's body / NCW / shares follow from that count by
    the selection rules written out again here (dp_local_rows.hip: bodies of 3 / 5 / 9 chunks, NCW = ceil(chunks / 4); rows_local_team: chunks / 4 each, the
    first chunks % 4 wavefronts one more; routing.h takes_local: at most 576 columns)."""
    want = sorted({1, 63} | {64 * (n - 1) for n in range(2, 10)} | {64 * n - 1 for n in range(1, 10)} | {15, 16, 47, 48, 576})
    assert sorted(LW.QLENS) == want
    seen = set()
    for qlen, (nch, body, ncw, share) in LW.QLENS.items():
        c, o = local_case(name, qlen)
        assert o.bits == 16 and c.qlen == qlen
        act = np.arange(1, c.n_rows - 1)
        assert (o.dp_beg_sn[act] == 0).all() and (o.dp_end_sn[act] == qlen // 16).all()
        w = (qlen // 16 + 1) * 16
        assert (w + 63) // 64 == nch == qlen // 64 + 1
        if w > LW.LOC_COLS:
            assert (body, ncw, share) == (LW.GENERAL,) * 3 and qlen == 576
            continue
        assert body == min(b for b in (3, 5, 9) if b >= nch) and ncw == -(-nch // 4)
        assert share == tuple(nch // 4 + (1 if wv < nch % 4 else 0) for wv in range(4)) and sum(share) == nch and max(share) == ncw
        seen.add((nch, body, ncw, share))
    assert {s[0] for s in seen} == set(range(1, 10)) and {s[1] for s in seen} == {3, 5, 9} and {s[2] for s in seen} == {1, 2, 3}
    assert {s[3] for s in seen} >= {(1, 1, 1, 0), (2, 1, 1, 1), (2, 2, 1, 1), (2, 2, 2, 1), (1, 1, 0, 0), (3, 2, 2, 2)}


def _pred_stats(name, skips):
    d = H.requeried(golden(name), int(golden(name)["qlen"][0]), skips=skips)
    n, po, pr = int(d["n_rows"][0]), d["pred_off"], d["pred_row"]
    npred = np.diff(po)[1:n - 1]
    oldest = np.array([r - int(pr[po[r]:po[r + 1]].min()) for r in range(1, n - 1)])
    return npred, oldest


# floors per golden: (rows of more than 8 predecessors, rows with a predecessor 16 or more rows back, rows whose oldest predecessor is 8 .. 15 back).  The
# nucleotide graphs have half the rows: every row the last two SKIPS entries name (5 + 3) has 9 and more, every row of the second entry (24) reaches 17 back
FLOORS = {"aa_blosum_loc": (10, 40, 40), "ragged_ag_loc": (8, 24, 24), "ragged_cg_loc": (8, 24, 24)}


@pytest.mark.parametrize("name", LW.GOLDENS)
def test_skip_edges_make_rows_of_many_and_old_predecessors(name):
    npred, oldest = _pred_stats(name, LW.SKIPS)
    many, far, mid = int((npred > 8).sum()), int((oldest >= 16).sum()), int(((oldest >= 8) & (oldest < 16)).sum())
    print(f"{name} SKIPS: {many} rows of more than 8 predecessors (at most {npred.max()}), {far} with one 16+ rows back, {mid} with the oldest 8-15 back; counts {np.bincount(npred)}")
    f = FLOORS[name]
    assert many >= f[0] and far >= f[1] and mid >= f[2] and 9 <= npred.max() <= 13
    if name == "aa_blosum_loc":
        assert (many, int(npred.max())) == (18, 13)
    # every predecessor count from 1 to 8 (the eight unrolled gathers of rows_local) and 9 .. 13 (the loop behind them): SKIPS alone has no row of 7 or 8
    # in any of the three graphs (and none of 6 in two of them), SKIPS + FILL has; the GPU tests run both
    assert np.bincount(npred, minlength=9)[7:9].sum() == 0
    npf, oldf = _pred_stats(name, LW.SKIPS_FILLED)
    cnt = np.bincount(npf, minlength=14)
    print(f"{name} SKIPS + FILL: counts {cnt}")
    assert (cnt[1:9] > 0).all() and (cnt[9:14] > 0).sum() >= 3 and int((npf > 8).sum()) >= f[0]
    assert int((oldf >= 16).sum()) >= f[1] and int(((oldf >= 8) & (oldf < 16)).sum()) >= f[2]
    # the arena gather of each kernel: predecessors at least a ring's depth back, first and later ones
    d = H.requeried(golden(name), 63, skips=LW.SKIPS_FILLED)
    po, pr, rr = d["pred_off"], d["pred_row"], LW.RING_ROWS[name]
    first_old = sum(1 for r in range(1, len(po) - 2) if r - pr[po[r]] >= rr)
    later_old = sum(1 for r in range(1, len(po) - 2) if (r - pr[po[r] + 1:po[r + 1]] >= rr).any())
    assert later_old >= f[1] and first_old >= 0


@pytest.mark.parametrize("name", LW.GOLDENS)
def test_tiled_queries_tie_the_row_maximum_between_chunks(name):
    ninth = 0      # tiled points with SKIPS at which the oracle's walk leaves a row through its ninth or a later predecessor (the match flags of the loop behind the eighth)
    for qlen, period in LW.TILED:
        got = []
        for skips in ((), LW.SKIPS):
            c, o = local_case(name, qlen, period, skips)
            chunks, cols, at_best = tie_counts(c, o)
            print(f"{name} ({qlen}, {period}) {'SKIPS' if skips else 'plain'}: maximum in more than one chunk on {chunks} rows, in more than one column on {cols}, {at_best} rows at the best score")
            assert o.bits == 16 and LW.QLENS.get(qlen, (qlen // 64 + 1,))[0] == qlen // 64 + 1
            if period is not None:
                assert qlen >= 2 * period and chunks >= LW.TIED_ROWS_AT_LEAST
            else:
                assert cols >= 1
            got.append(at_best)
            if skips:
                idx = walk_pred_indices(c, o)
                print(f"   the walk's steps by predecessor position: {np.bincount(idx)}")
                ninth += max(idx) >= 8
        assert tuple(got) == LW.BEST_TIES.get((name, qlen, period), (1, 1))
    assert ninth >= 1


@pytest.mark.parametrize("name", LW.NUCLEOTIDE)
def test_scoring_points_sit_where_the_table_says(name):
    lib = H.oracle_lib()
    for qlen in LW.SCORING_QLENS:
        for pt, bits in zip(LW.gate_points(name, qlen), (16, 32)):
            c, o = local_case(name, qlen, pt=pt)
            assert lib.abpoa_oracle_score_bits(C.byref(c.sc), c.n_rows, c.qlen, None) == bits == o.bits, (pt.name, qlen)
            assert c.sc.gap_mode == int(golden(name)["gap_mode"][0])
        c, o = local_case(name, qlen, pt=LW.asym_point(name))
        assert o.bits == 16 and c.sc.gap_mode == int(golden(name)["gap_mode"][0]) and o.n_cigar > 0
