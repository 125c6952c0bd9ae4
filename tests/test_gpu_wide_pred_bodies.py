"""GPU (-m gpu): the wide row loop (rows_fast.h ilp_chunks<NCH>, NCH = 3 .. 7 in dp_wide_kernel, 8 / 9 / 11 in dp_xl_kernel) at every predecessor count and
reach -- the run-time gather loop up to eight predecessors, predecessors gathered from the arena behind the 16-row and the 4-row ring (is_far, hbm_read_all, spill
rows under direction words), rows the wide kernels hand to general_body (9 and more predecessors, one 64 and more rows back) -- and the two walks over rows
staged as column slices (backtrack_dir.h, backtrack.h) behind both rings, through predecessor index 8 and above, past 254 rows and out of a slice to the
left, against the C oracle, bit for bit, through the flat C-ABI.  The inputs are the skip-edge families of tests/wide_preds.py, whose docstring says which
family drives which branch; tests/test_wide_pred_regimes.py asserts on the CPU that every body holds rows of every class and that the walks step where the
table says; the diagnostic build's counters (tests/test_gpu_device_msa.py::test_long_read_rows_take_the_all_chunk_bodies) tie the classes to what the device
dispatches.  The oracle on skip-edge graphs is not pinned to the compiled reference (no read-set produces them); the last part is the counterweight:
read-sets at 30 % error at a band of the wide loop through the device-resident driver against the CPU build of the host layer (tests/cpu_shim.cpp, pinned to
the reference's command-line tool at that band by tests/test_host_msa.py).  One launch per group of alignments that share a scoring; the oracle's planes of
one (golden, width, band) are alive at a time (a convex alignment's planes at 704 columns are 16 MB).  Nothing here depends on timing."""
import numpy as np
import pytest

import helpers as H
import narrow_preds as NP
import wide_bands as WB
import wide_preds as WP
from gpu_harness import dir_counts, engine, launch, words_match  # noqa: F401  (engine: the fixture)
from readset_worker import run_report

pytestmark = pytest.mark.gpu


def _points():
    """{(golden, bits, wb): families} of the default plan, in table order."""
    out = {}
    for g, b in WP.COMBOS:
        for f, wb in WP.pred_points(g, b):
            out.setdefault((g, b, wb), []).append(f)
    return out


POINTS = _points()
POINT_IDS = [f"{g[4:6]}{b}_w{wb}" for g, b, wb in POINTS]
BAND_POINTS = [(g, b, wb) for g, b in WP.COMBOS for wb in WP.BANDS[(g, b)]]
BAND_IDS = [f"{g[4:6]}{b}_w{wb}" for g, b, wb in BAND_POINTS]
COMBO_IDS = [f"{g}_i{b}" for g, b in WP.COMBOS]
_ALIVE = {"key": None, "items": {}}


def _case(golden, bits, wb, family, tag=""):
    """(family, FlatCase, input dict, oracle output with planes); the outputs of one (golden, width, band, tag) are kept at a time."""
    key = (golden, bits, wb, tag)
    if _ALIVE["key"] != key:
        _ALIVE["key"], _ALIVE["items"] = key, {}
    items = _ALIVE["items"]
    if family not in items:
        d = WP.case_dict(golden, family, bits, wb)
        c = H.FlatCase(d)
        o = H.run_oracle(c)
        assert o.rc == 0 and o.status == 0 and o.bits == bits, (key, family)
        items[family] = (family, c, d, o)
    return items[family]


def _launches(items):
    """Groups of [(family, case, dict, oracle)] that share every Scoring field (in int32 the cut queries of `jump` and `farjump` have match scores of their own)."""
    groups = {}
    for it in items:
        sc = it[1].sc
        groups.setdefault((sc.max_mat, sc.min_mis, tuple(it[1].mat.tolist())), []).append(it)
    return list(groups.values())


def _run(items, trace, label):
    """Every alignment against the oracle -- with the trace every plane cell, band and row arg-max too; one launch per scoring."""
    for group in _launches(items):
        launch(group, trace, label)


def _point_items(key):
    g, b, wb = key
    return [_case(g, b, wb, f) for f in POINTS[key]]


@pytest.mark.parametrize("key", list(POINTS), ids=POINT_IDS)
def test_records_with_trace(engine, key):
    """Score records, trace kept: bands, every plane cell (the packed E differences of convex int32 included), row arg-max, best cell, cigar, result fields,
    band state -- every family at every band of the table, the ring switch and one past the widest body."""
    _run(_point_items(key), True, f"records {key}")


@pytest.mark.parametrize("key", list(POINTS), ids=POINT_IDS)
def test_record_walk_without_trace(engine, monkeypatch, key):
    """ABPOA_HIP_NODIR=1: the record walk (backtrack.h) over the slice windows of rows this wide -- behind the eighth predecessor on `jump`, over steps of 16 to
    300 rows on `farjump`, through the insertion runs of `ins`; no plane is walked."""
    monkeypatch.setenv("ABPOA_HIP_NODIR", "1")
    dir_counts(engine)
    _run(_point_items(key), False, f"records, no trace {key}")
    assert dir_counts(engine) == (0, 0)


@pytest.mark.parametrize("key", list(POINTS), ids=POINT_IDS)
def test_direction_words(engine, monkeypatch, key):
    """ABPOA_HIP_DIR_WIDE=1: the bodies write direction words and the backtrack walks them (the column-slice triangle of backtrack_dir.h); every alignment
    walks the plane and none is redone with records."""
    monkeypatch.setenv("ABPOA_HIP_DIR_WIDE", "1")
    items = _point_items(key)
    dir_counts(engine)
    _run(items, False, f"words {key}")
    assert dir_counts(engine) == (len(items), 0), key


@pytest.mark.parametrize("key", list(POINTS), ids=POINT_IDS)
def test_direction_words_match_the_model(engine, monkeypatch, key):
    """Every direction word the bodies write (trace mode with ABPOA_HIP_DIRTRACE=1) against the words oracle/dir_model.c derives from the oracle's scores: kM and
    kE up to 8 on the rows of five to eight predecessors, up to 11 on the rows general_body takes."""
    monkeypatch.setenv("ABPOA_HIP_DIR_WIDE", "1")
    words_match(_point_items(key), f"words against the model {key}")


@pytest.mark.parametrize("key", BAND_POINTS, ids=BAND_IDS)
def test_four_row_ring(engine, monkeypatch, key):
    """ABPOA_HIP_RING_ROWS=4 on `edge4`, `in_ring` and `far`: a predecessor exactly 3 | 4 | 5 rows back either side of `row - p >= RR`, the first or the second
    predecessor far and the other near, far predecessors at k >= 2, all gathered from the arena inside the body; records with the trace, then direction words
    (the gather steps over a spill row's words to its records) walked and compared with the model."""
    g, b, wb = key
    monkeypatch.setenv("ABPOA_HIP_RING_ROWS", "4")
    items = [_case(g, b, wb, f, "ring4") for f in WP.RING4_FAMILIES]
    _run(items, True, f"4-row ring {key}")
    monkeypatch.setenv("ABPOA_HIP_DIR_WIDE", "1")
    dir_counts(engine)
    _run(items, False, f"4-row ring, words {key}")
    assert dir_counts(engine) == (len(items), 0)
    words_match(items, f"4-row ring, words against the model {key}")


@pytest.mark.parametrize("golden,bits", WP.COMBOS, ids=COMBO_IDS)
def test_448_column_kernel(engine, monkeypatch, golden, bits):
    """ABPOA_HIP_NOXL=1 at 196 and 215: `in_ring` and `far` on dp_wide_kernel's 7-chunk body; records with the trace, then words walked and against the model."""
    monkeypatch.setenv("ABPOA_HIP_NOXL", "1")
    for wb in WP.NOXL_BANDS:
        monkeypatch.delenv("ABPOA_HIP_DIR_WIDE", raising=False)
        items = [_case(golden, bits, wb, f, "noxl") for f in WP.NOXL_FAMILIES]
        _run(items, True, f"no long-read form wb={wb}")
        monkeypatch.setenv("ABPOA_HIP_DIR_WIDE", "1")
        dir_counts(engine)
        _run(items, False, f"no long-read form, words wb={wb}")
        assert dir_counts(engine) == (len(items), 0)
        words_match(items, f"no long-read form, words against the model wb={wb}")


@pytest.mark.parametrize("bt_bytes", WP.BT_BYTES)
@pytest.mark.parametrize("golden,bits", WP.COMBOS, ids=COMBO_IDS)
def test_small_backtrack_windows(engine, monkeypatch, golden, bits, bt_bytes):
    """ABPOA_HIP_BT_BYTES=4096 / 6144 on `farjump`, `jump` and `ins`: a window holds a few slices, so every far step and every long insertion run is followed by
    a new slice window -- the word walk (go_pred, restage, the re-centring when a walk leaves a slice to the left), then the record walk."""
    monkeypatch.setenv("ABPOA_HIP_BT_BYTES", bt_bytes)
    wb = WP.BT_BAND[bits]
    items = [_case(golden, bits, wb, f, "bt") for f in WP.WALK_FAMILIES]
    monkeypatch.setenv("ABPOA_HIP_DIR_WIDE", "1")
    dir_counts(engine)
    _run(items, False, f"small windows, words {golden} int{bits}")
    assert dir_counts(engine) == (len(items), 0)
    monkeypatch.delenv("ABPOA_HIP_DIR_WIDE")
    monkeypatch.setenv("ABPOA_HIP_NODIR", "1")
    _run(items, False, f"small windows, records {golden} int{bits}")
    assert dir_counts(engine) == (0, 0)


@pytest.mark.parametrize("golden", WP.GOLDENS)
def test_mixed_launch(engine, monkeypatch, golden):
    """Every family of a golden at wb = 12, wf = 0.16 (w = 84 .. 223) and one short golden (w = 20: the narrow kernel) in ONE launch, in both orders: with the
    trace, then with direction words."""
    m = WP.MIXED
    items = [("short", H.FlatCase(H.rescored(H.first_golden(m["short"][golden]), WB.point(golden, 16, 54), m["wb"], m["wf"])))]
    for f in WP.ALL_FAMILIES:
        d = WP.case_dict(golden, f, 16, m["wb"])
        d["wf"] = np.array([m["wf"]], np.float32)
        items.append((f, H.FlatCase(d)))
    items = items[3:] + items[:3]                  # (the short one in the middle)
    items = [(name, c, H.run_oracle(c)) for name, c in items]
    assert all(o.status == 0 and o.bits == 16 for _, _, o in items)
    for order in (items, items[::-1]):
        launch(order, True, f"mixed launch {golden}")
    for _, _, o in items:
        o.planes = None
    monkeypatch.setenv("ABPOA_HIP_DIR_WIDE", "1")
    dir_counts(engine)
    launch(items, False, f"mixed launch, words {golden}")
    assert dir_counts(engine) == (len(items), 0)


@pytest.mark.parametrize("golden", WP.GOLDENS)
def test_extension_mode_with_zdrop(engine, golden):
    """Extension mode, z-drop 6, wb = 196 on `far` (rows of 5-8 chunks) and `farjump` (stops behind its first far step): planes, running best and cigar with the
    trace, best cell and cigar without; the rows behind the oracle's stop are not computed on the device either."""
    variant, wb, fams = WP.EXTZ
    for f in fams:
        c = H.FlatCase(NP.case_dict(golden, f, variant, wb))
        o = H.run_oracle(c)
        assert o.status == 0
        for trace in (True, False):
            h = launch([(f, c, o)], trace, f"extension z-drop {golden}")[0]
            assert (h.best_score, h.best_row, h.best_col) == (o.best_score, o.best_row, o.best_col)
            if trace:
                assert np.array_equal(h.dp_beg_sn < 0, o.dp_beg_sn < 0), (golden, f)


# ---------------------------------------------------------------- read-sets at a band of the wide loop through the device-resident driver
def make_jobs():
    """{"<gaps>/<kind>": spec} for tests/readset_worker.py: the read-sets of tests/narrow_preds.py at READ_SET_BAND, affine and convex, in every form."""
    fields = ("n_cells", "msa", "dig")
    return {f"{gaps}/{kind}": dict(params=dict(kw, **WP.READ_SET_BAND), sets=NP.read_sets(kind), forms=WP.READ_SET_FORMS, ref_first=True,
                                   record=fields + ("launches", "n_host_sets", "host_reasons"), ref_record=fields)
            for gaps, kw in (("affine", NP.AFFINE), ("convex", WP.CONVEX)) for kind in NP.KINDS}


@pytest.fixture(scope="module")
def report():
    return run_report("test_gpu_wide_pred_bodies", set_env={"ABPOA_HIP_CIGAR_DIGEST": "1"}, timeout=600,
                      clear_env=("ABPOA_HIP_DBG", "ABPOA_HIP_LOCKSTEP", "ABPOA_HIP_DEVSYNC", "ABPOA_HIP_NODIR", "ABPOA_HIP_VERBOSE", "ABPOA_HIP_DIR_WIDE",
                                 "ABPOA_HIP_RING_ROWS"))


@pytest.mark.parametrize("kind", list(NP.KINDS))
@pytest.mark.parametrize("gaps", ["affine", "convex"])
def test_device_driver_on_divergent_read_sets_at_a_wide_band(report, gaps, kind):
    """The read-sets of tests/narrow_preds.py (30 % error, insertion-heavy, first pass) at -b 60 -f 0, where every alignment takes the wide loop: score records
    (the default), direction words (ABPOA_HIP_DIR_WIDE=1), words from a 4-row ring, records without any plane (ABPOA_HIP_NODIR=1).  Consensus, coverage, MSA
    rows, n_cells and cigar digests equal the CPU shim's; no set leaves the device; the wide row kernels were launched and the narrow one never was
    (abpoa_hip__row_launches, counted where the kernels are launched)."""
    rep = report[f"{gaps}/{kind}"]
    ref = rep["ref"]
    assert all(s == 0 for s in ref["status"]) and all(d != 0 for d in ref["dig"]) and len(ref["status"]) == NP.N_SETS[kind]
    for form in WP.READ_SET_FORMS:
        got = rep[form]
        assert got["n_host_sets"] == 0, f"{gaps} / {kind} / {form}: sets left the device: {got['host_reasons']}"
        narrow, wide448, wide704 = got["launches"]
        print(f"{gaps} / {kind} / {form}: row-kernel launches narrow {narrow}, 448-column wide {wide448}, 704-column wide {wide704}")
        assert narrow == 0 and wide448 > 0 and wide704 == 0, (gaps, kind, form, got["launches"])
        for k in ("status", "cons", "cov", "msa", "n_cells", "dig"):
            assert got[k] == ref[k], f"{gaps} / {kind} / {form}: {k} differs from the oracle-backed host run"
