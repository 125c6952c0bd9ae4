"""GPU (-m gpu): the narrow row loop (rows_fast.h rows_fast<T, GAP, false, DIR>, band half-widths w < 40) at every predecessor count, per body it picks among --
the assembly loop (rows_tight_asm.h) and its compiler twins turbo_body<1|2>, turbo_body<4>, turbo_body<8>, ilp_chunks<2> from the score ring and with the arena
gather in HBM, fast_body / general_body --, per arena format (score records / direction words), score width and gap model, against the C oracle, bit for bit,
through the flat C-ABI.  The inputs are the two 1 kb goldens with the skip-edge families of tests/narrow_preds.py, whose docstring says which point drives
which body; tests/test_narrow_regimes.py asserts on the CPU that the rows of every class are there, that the plan is the one the bodies need and where the
word plane applies.  The oracle on skip-edge graphs is not pinned to the compiled reference (no read-set produces them); the last part is the counterweight:
read-sets at 30 % error, whose graphs grow 100 and more nodes of 5-8 predecessors by themselves, through both forms of the device-resident driver against the
CPU build of the host layer (tests/cpu_shim.cpp, pinned to the reference's command-line tool by tests/test_host_msa.py).  Nothing here depends on timing."""
import numpy as np
import pytest

import helpers as H
import narrow_preds as NP
from gpu_harness import dir_counts, engine, launch, narrow_plan  # noqa: F401  (engine: the fixture)
from readset_worker import run_report

pytestmark = pytest.mark.gpu


# one launch per group of points that share every Scoring field: (golden, variant, wb, tag) -> families (`jump` and `farjump` in int32 have match scores of their
# own: their queries are shorter, and the table takes the first score at which each leaves 16 bits)
GROUPS = {}
for _g, _f, _v, _wb in NP.ALL_POINTS:
    GROUPS.setdefault((_g, _v, _wb, _f if (_f in NP.JUMP and _v == "i32") else ""), []).append(_f)
GROUP_IDS = [f"{g[4:6]}_{v}" + ("" if wb is None else f"_w{wb}") + ("_" + tag if tag else "") for g, v, wb, tag in GROUPS]
WORD_GROUPS = [k for k in GROUPS if k[1] in ("own", "i32")]                 # jobs that write direction words without the trace: global mode, affine / convex
WORD_IDS = [GROUP_IDS[list(GROUPS).index(k)] for k in WORD_GROUPS]
_CASES = {}


def _case(golden, family, variant, wb):
    """(FlatCase, its input dict, the oracle's output with planes), computed once per module; family None: the golden as recorded, under the variant's scoring."""
    k = (golden, family, variant, wb)
    if k not in _CASES:
        d = NP.case_dict(golden, family, variant, wb)
        c = H.FlatCase(d)
        o = H.run_oracle(c)
        assert o.rc == 0 and o.status == 0 and o.bits == NP.VARIANTS[variant][1], k
        _CASES[k] = (c, d, o)
    return _CASES[k]


def _group(key):
    golden, variant, wb = key[:3]
    return [(f, *_case(golden, f, variant, wb)) for f in GROUPS[key]]


@pytest.mark.parametrize("key", list(GROUPS), ids=GROUP_IDS)
def test_records_with_trace(engine, key):
    """Score records, trace kept: bands, every plane cell, row arg-max, best cell (extension mode: the running best), cigar, result fields, band state -- every
    family x golden x band x variant; the int32, linear and extension points take the compiler's loops."""
    launch(_group(key), True, f"records {key}")


@pytest.mark.parametrize("key", list(GROUPS), ids=GROUP_IDS)
@pytest.mark.parametrize("loop", ["asm", "dbg2048"])
def test_without_trace(engine, monkeypatch, key, loop):
    """No trace: the job writes direction words where the engine allows them (global mode, affine / convex, at most 15 predecessors per row) and score records
    elsewhere.  Cigar, best cell and result fields against the oracle; the plane was walked and nothing redone at exactly the points the CPU test marks
    usable (narrow_preds.words_apply).  With the assembly loop, and with the compiler's twins (ABPOA_HIP_DBG=2048)."""
    if loop == "dbg2048":
        monkeypatch.setenv("ABPOA_HIP_DBG", "2048")
    items = _group(key)
    dir_counts(engine)
    launch(items, False, f"no trace {loop} {key}")
    walked, redone = dir_counts(engine)
    assert (walked, redone) == (sum(NP.words_apply(key[0], f, key[1]) for f in GROUPS[key]), 0), (key, loop, walked, redone)


def _word_plane(case):
    """The direction words as the row loops wrote them (trace mode with ABPOA_HIP_DIRTRACE=1: the trace's planes carry the words), cut to the columns a walk can
    read (up to the query's end)."""
    h = H.run_hip([case], want_trace=True)[0]
    assert h.status == 0
    pn = 16 if h.bits == 16 else 8
    rows = []
    for r in range(1, case.n_rows - 1):
        if h.dp_beg_sn[r] < 0:
            continue
        W = int(h.dp_end_sn[r] - h.dp_beg_sn[r] + 1) * pn
        n = min(W, case.qlen + 1 - int(h.dp_beg_sn[r]) * pn)
        o = int(h.row_off[r])
        k = 2 if (case.sc.gap_mode == 2 and h.bits == 16) else 1          # plane 0 carries the words; int16 convex: plane 1 their upper halves
        rows.append(h.planes[o:o + k * W].reshape(k, W)[:, :n].copy())
    return rows


@pytest.mark.parametrize("key", WORD_GROUPS, ids=WORD_IDS)
def test_direction_words_match_the_model(engine, monkeypatch, key):
    """Every direction word the bodies write against the words oracle/dir_model.c derives from the oracle's scores (H.dir_words_mismatches == []), at every
    usable point, with the assembly loop and with the compiler's twins; and the two loops' word planes equal each other, word for word."""
    golden, variant, wb = key[:3]
    n = 0
    for f, c, d, o in _group(key):
        if not NP.words_apply(golden, f, variant):
            continue
        planes = {}
        for loop in ("asm", "dbg2048"):
            if loop == "dbg2048":
                monkeypatch.setenv("ABPOA_HIP_DBG", "2048")
            else:
                monkeypatch.delenv("ABPOA_HIP_DBG", raising=False)
            bad = H.dir_words_mismatches(c, d)
            assert bad is not None and bad == [], (key, f, loop, bad[:5] if bad else bad)
            monkeypatch.setenv("ABPOA_HIP_DIRTRACE", "1")
            planes[loop] = _word_plane(c)
            monkeypatch.delenv("ABPOA_HIP_DIRTRACE")
        assert len(planes["asm"]) == len(planes["dbg2048"]) > 0
        diff = [i for i, (a, b) in enumerate(zip(planes["asm"], planes["dbg2048"])) if not np.array_equal(a, b)]
        assert diff == [], (key, f, "word planes of the two loops differ at computed rows", diff[:8])
        n += 1
    assert n == sum(NP.words_apply(golden, f, variant) for f in GROUPS[key]) >= 1


@pytest.mark.parametrize("key", list(GROUPS), ids=GROUP_IDS)
def test_record_walk_without_trace(engine, monkeypatch, key):
    """ABPOA_HIP_NODIR=1 without the trace: the record walk of backtrack.h at every point -- through graphs with rows of up to 17 predecessors, which the
    walk leaves through one of their first four; behind the eighth predecessor on `jump`, over steps of 16 to 300 rows on `farjump`; no plane is walked."""
    monkeypatch.setenv("ABPOA_HIP_NODIR", "1")
    dir_counts(engine)
    launch(_group(key), False, f"records, no trace {key}")
    assert dir_counts(engine) == (0, 0)


@pytest.mark.parametrize("golden", NP.GOLDENS)
@pytest.mark.parametrize("wc", [None, "8"], ids=["bt8192", "bt8192_wc8"])
def test_small_backtrack_windows(engine, monkeypatch, golden, wc):
    """ABPOA_HIP_BT_BYTES=8192, and ABPOA_HIP_BT_WC=8 with it, on `far`, `many`, `jump` and `farjump`: the window staging of both walks (direction words,
    then score records with ABPOA_HIP_NODIR=1) when a step jumps 16, 17, 63, 64, 70 and 300 rows (`farjump`: eleven such steps per alignment, asserted on the
    oracle's cigar by tests/test_narrow_regimes.py; the walks over `far` and `many` take no step longer than six rows) and the loop behind the eighth
    predecessor (`jump`: 17-18 steps through it)."""
    monkeypatch.setenv("ABPOA_HIP_BT_BYTES", "8192")
    if wc:
        monkeypatch.setenv("ABPOA_HIP_BT_WC", wc)
    items = [(f, *_case(golden, f, "own", None)) for f in ("far", "many", "jump", "farjump")]
    dir_counts(engine)
    launch(items, False, f"small windows, words {golden}")
    assert dir_counts(engine) == (len(items), 0)
    monkeypatch.setenv("ABPOA_HIP_NODIR", "1")
    launch(items, False, f"small windows, records {golden}")
    assert dir_counts(engine) == (0, 0)
    launch(items, True, f"small windows, trace {golden}")


@pytest.mark.parametrize("golden", NP.GOLDENS)
def test_one_launch_mixing_every_family(engine, golden):
    """Every family of a golden in ONE launch, the golden as recorded between them, in both orders, with and without the trace: streaks of straight-line
    rows and declined rows alternate across the alignments of a launch; without the trace the two graphs with 16 / 17 predecessors keep records beside
    the eight alignments that walk their planes."""
    fams = list(NP.FAMILY_NAMES)
    order = fams[:3] + [None] + fams[3:]
    for names in (order, order[::-1]):
        items = [(str(f), *_case(golden, f, "own", None)) for f in names]
        launch(items, True, f"mixed launch {golden}")
        dir_counts(engine)
        launch(items, False, f"mixed launch {golden}")
        assert dir_counts(engine) == (len(items) - 2, 0)


@pytest.mark.parametrize("key", [k for k in GROUPS if k[1] in NP.ZDROP], ids=[i for i, k in zip(GROUP_IDS, GROUPS) if k[1] in NP.ZDROP])
def test_extension_mode_with_zdrop(engine, key):
    """Extension mode, z-drop 6 / 10 (asm_tight_on is off: the C++ tight loop, commit_row's z-drop test under many predecessors): planes, running best and
    cigar with the trace, best cell and cigar without it; the rows behind the oracle's stop are not computed on the device either (compare_outs: bands)."""
    items = _group(key)
    stopped = [f for f, c, _, o in items if (o.dp_beg_sn[1:c.n_rows - 1] < 0).any()]
    assert stopped == [f for f in GROUPS[key] if (key[0], f, key[1]) in NP.STOPS_EARLY]
    outs = launch(items, True, f"extension z-drop {key}")
    for (f, c, _, o), h in zip(items, outs):
        assert (h.best_score, h.best_row, h.best_col) == (o.best_score, o.best_row, o.best_col)
        assert np.array_equal(h.dp_beg_sn < 0, o.dp_beg_sn < 0), (key, f)
    launch(items, False, f"extension z-drop {key}")


@pytest.mark.parametrize("pt", NP.SWITCH, ids=[NP.point_id(p) for p in NP.SWITCH])
def test_width_switch(engine, monkeypatch, pt):
    """`in_ring` on either side of the switch from 128 to 192 ring columns (w = 24 | 25 in int16, 36 | 37 in int32), the plan taken from the hook: up to W_128
    the straight-line bodies and ilp_chunks<2> share the rows, one past it every row takes ilp_chunks<2> or the exact bodies (int32 convex: from an 8-row
    ring).  Records with the trace, then the walk over the words; test_direction_words_match_the_model holds the words of both bands to the model."""
    g, f, v, wb = pt
    c, d, o = _case(g, f, v, wb)
    bits = NP.VARIANTS[v][1]
    past = wb == NP.W_128[bits] + 1
    assert narrow_plan(c, bits) == ((NP.RING_ROWS_192[(g, bits)], 192) if past else (16, 128))
    launch([(f, c, d, o)], True, f"width switch {pt}")
    dir_counts(engine)
    launch([(f, c, d, o)], False, f"width switch {pt}")
    assert dir_counts(engine) == (1, 0)


# ---------------------------------------------------------------- real graphs through both forms of the device-resident driver
AFFINE, KINDS, N_SETS, FORMS, EXTRA = NP.AFFINE, NP.KINDS, NP.N_SETS, NP.FORMS, NP.EXTRA      # (the read-sets: tests/narrow_preds.py)


def high_in_degree(msa_rows):
    """(nodes with 5-8 distinct predecessors, nodes with 9 and more) of the graph rebuilt from MSA rows: a node is a (column, base) pair, an edge joins
    consecutive non-gap entries of a read."""
    preds = {}
    for row in msa_rows:
        prev = None
        for col, ch in enumerate(row):
            if ch == "-":
                continue
            preds.setdefault((col, ch), set())
            if prev is not None:
                preds[(col, ch)].add(prev)
            prev = (col, ch)
    return sum(1 for s in preds.values() if 5 <= len(s) <= 8), sum(1 for s in preds.values() if len(s) >= 9)


def make_jobs():
    """{kind: spec} for tests/readset_worker.py: every kind of read-set in every form of the driver, `devsync` on the first set of err30 only."""
    jobs = {}
    for kind in KINDS:
        extra = {f: e for (k, f), e in EXTRA.items() if k == kind}
        jobs[kind] = dict(params=AFFINE, sets=NP.read_sets(kind), forms=dict(FORMS, **extra), first_set_forms=tuple(extra), ref_first=True,
                          record=("n_cells", "msa", "dig", "n_host_sets", "host_reasons"), ref_record=("n_cells", "msa", "dig"))
    return jobs


@pytest.fixture(scope="module")
def report():
    return run_report("test_gpu_narrow_bodies", set_env={"ABPOA_HIP_CIGAR_DIGEST": "1"}, timeout=300,
                      clear_env=("ABPOA_HIP_DBG", "ABPOA_HIP_LOCKSTEP", "ABPOA_HIP_DEVSYNC", "ABPOA_HIP_NODIR", "ABPOA_HIP_VERBOSE"))


@pytest.mark.parametrize("kind", ["err30", "ins16"])
def test_read_sets_grow_high_in_degree(report, kind):
    """On the shim's output (CPU side): the final graph of every set, rebuilt from its MSA rows, has 100 and more nodes of 5-8 distinct predecessors
    (measured 148-169 at 30 % error, 143-153 at the insertion-heavy rates; the 1 kb benchmark sets at 5 % have about 55), some of 9 and more."""
    ref = report[kind]["ref"]
    n_reads = KINDS[kind]["n_reads"]
    counts = [high_in_degree(rows[:n_reads]) for rows in ref["msa"]]
    print(kind, counts)
    assert len(counts) == 4 and all(s == 0 for s in ref["status"])
    assert all(n58 >= 100 for n58, _ in counts), counts
    assert sum(n9 for _, n9 in counts) >= 1, counts


@pytest.mark.parametrize("kind", list(KINDS))
def test_device_driver_on_divergent_read_sets(report, kind):
    """The all-rounds kernel, the step-by-step driver (ABPOA_HIP_LOCKSTEP=1) and the compiler's row loop (ABPOA_HIP_DBG=2048): consensus, coverage, MSA rows
    and n_cells equal the shim's, the cigar digests are equal across the forms (and to the shim's), no set leaves the device.  The 50-read sets climb the
    node-slot ladder (graphs of five read lengths), the 20-read set stays in the first pass; one set once more under ABPOA_HIP_DEVSYNC=1."""
    rep = report[kind]
    ref = rep["ref"]
    assert all(s == 0 for s in ref["status"]) and all(d != 0 for d in ref["dig"])
    forms = [f for f in rep if f != "ref"]
    assert set(FORMS) <= set(forms) and (("devsync" in forms) == (kind == "err30"))
    for form in forms:
        got = rep[form]
        n = len(got["status"])
        assert n == (1 if (kind, form) in EXTRA else N_SETS[kind])
        assert got["n_host_sets"] == 0, f"{kind} / {form}: sets left the device: {got['host_reasons']}"
        for k in ("status", "cons", "cov", "msa", "n_cells", "dig"):
            assert got[k] == ref[k][:n], f"{kind} / {form}: {k} differs from the oracle-backed host run"
    for form in FORMS:
        assert rep[form]["dig"] == rep["all_rounds"]["dig"]
