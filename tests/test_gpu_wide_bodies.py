"""GPU (-m gpu): the all-chunk row bodies (rows_fast.h ilp_chunks<NCH>) at every chunk count they are instantiated for -- 3 .. 7 in dp_wide_kernel, 8 / 9 / 11 in
dp_xl_kernel --, per score width (int16 / int32, the packed E differences of convex int32), gap model (affine / convex), arena format (score records /
direction words) and ring reach (score ring / HBM gather inside the body), against the C oracle, bit for bit, through the flat C-ABI.  The inputs are the two
1 kb goldens re-banded over the table of tests/wide_bands.py (wf = 0): rows of 1358 / 1147 x <= 704 columns with at least 100 rows of every chunk count from 2
to 11 per golden and width, both ends of the wide loop's range (wide_w_lo = 40, the switch from the 448- to the 704-column ring, wide_w_hi = 215 / 343 and one
past each, the bodies' "wider than my chunks" decline at 8 / 12 chunks, the plan turning the fast loops off).  tests/test_wide_band_regimes.py asserts those
properties of the inputs and the plan on the CPU, tests/test_oracle_vs_reference.py pins the oracle to the compiled reference at three of the bands, and the
diagnostic build's row counters (tests/test_gpu_device_msa.py::test_long_read_rows_take_the_all_chunk_bodies) show on the device that the rows took the bodies."""
import numpy as np
import pytest

import helpers as H
import wide_bands as WB
from gpu_harness import dir_counts, engine, launch  # noqa: F401  (engine: the fixture)
from test_wide_band_regimes import mixed_cases

pytestmark = pytest.mark.gpu
IDS = [f"{g}_i{b}" for g, b in WB.COMBOS]


_GOLD, _CASES = {}, {"combo": None, "items": {}}


def _case(golden, bits, wb):
    """(re-banded FlatCase, its input dict, the oracle's output with planes), computed once; the outputs of one (golden, width) are kept at a time (a convex
    alignment's planes at 704 columns are 16 MB)."""
    if _CASES["combo"] != (golden, bits):
        _CASES["combo"], _CASES["items"] = (golden, bits), {}
    items = _CASES["items"]
    if wb not in items:
        if golden not in _GOLD:
            _GOLD[golden] = H.first_golden(golden)
        g = _GOLD[golden]
        d = H.rescored(g, WB.point(golden, bits, int(g["qlen"][0])), wb, 0.0)
        c = H.FlatCase(d)
        o = H.run_oracle(c)
        assert o.status == 0 and o.bits == bits
        items[wb] = (c, d, o)
    return items[wb]


def _with_trace(golden, bits, bands, label, trace=True):
    """One launch per band.  Score records, trace kept: bands, every plane cell, row arg-max, best cell, cigar, result fields, band state."""
    for wb in bands:
        launch([(f"wb={wb}", *_case(golden, bits, wb))], trace, f"{label} {golden} int{bits}", bits=bits)


def _without_trace(golden, bits, bands, label):
    """No trace: best cell, cigar, result fields, band state."""
    _with_trace(golden, bits, bands, label, trace=False)


NO_WORDS = WB.NO_WORDS      # (point, words variant) pairs that are not run, each with its reason; tests/test_wide_band_regimes.py holds the table to the plan


@pytest.mark.parametrize("golden,bits", WB.COMBOS, ids=IDS)
def test_records_with_trace(engine, golden, bits):
    _with_trace(golden, bits, WB.BANDS, "records")


@pytest.mark.parametrize("golden,bits", WB.COMBOS, ids=IDS)
def test_records_without_trace(engine, monkeypatch, golden, bits):
    """ABPOA_HIP_NODIR=1: the record walk (backtrack.h) over the column-slice windows of rows this wide."""
    monkeypatch.setenv("ABPOA_HIP_NODIR", "1")
    dir_counts(engine)
    _without_trace(golden, bits, WB.BANDS, "records, no trace")
    assert dir_counts(engine) == (0, 0)


@pytest.mark.parametrize("golden,bits", WB.COMBOS, ids=IDS)
def test_direction_words(engine, monkeypatch, golden, bits):
    """ABPOA_HIP_DIR_WIDE=1: the bodies write direction words (DIR = true) and the backtrack walks them; every alignment whose point has a fast row loop walks
    the plane and none is redone with records (dir_plane_usable holds at both scorings)."""
    monkeypatch.setenv("ABPOA_HIP_DIR_WIDE", "1")
    for wb in WB.BANDS:
        dir_counts(engine)
        _without_trace(golden, bits, [wb], "words")
        walked, redone = dir_counts(engine)
        assert (walked, redone) == ((0, 0) if (golden, bits, wb) in NO_WORDS else (1, 0)), (golden, bits, wb, walked, redone)


def _words_against_the_model(golden, bits, bands):
    n = 0
    for wb in bands:
        if (golden, bits, wb) in NO_WORDS:
            continue
        c, d, _ = _case(golden, bits, wb)
        bad = H.dir_words_mismatches(c, d)
        assert bad is not None and bad == [], (golden, bits, wb, bad[:5] if bad else bad)
        n += 1
    return n


@pytest.mark.parametrize("golden,bits", WB.COMBOS, ids=IDS)
def test_direction_words_match_the_model(engine, monkeypatch, golden, bits):
    """Every direction word the bodies write (trace mode with ABPOA_HIP_DIRTRACE=1) against the words oracle/dir_model.c derives from the oracle's scores."""
    monkeypatch.setenv("ABPOA_HIP_DIR_WIDE", "1")
    assert _words_against_the_model(golden, bits, WB.BANDS) == len(WB.BANDS) - sum(1 for k in NO_WORDS if k[:2] == (golden, bits))


@pytest.mark.parametrize("golden,bits", WB.COMBOS, ids=IDS)
def test_four_row_ring(engine, monkeypatch, golden, bits):
    """ABPOA_HIP_RING_ROWS=4: a predecessor four rows back or more is gathered from the arena in HBM inside the body (hbm_read_all), at 5, 6, 7, 8-9 and 11
    chunks; records with trace, then direction words against the model."""
    monkeypatch.setenv("ABPOA_HIP_RING_ROWS", "4")
    _with_trace(golden, bits, WB.RING4_BANDS, "4-row ring")
    monkeypatch.setenv("ABPOA_HIP_DIR_WIDE", "1")
    assert _words_against_the_model(golden, bits, WB.RING4_BANDS) == len(WB.RING4_BANDS)


@pytest.mark.parametrize("golden,bits", WB.COMBOS, ids=IDS)
def test_448_column_kernel_up_to_its_last_band(engine, monkeypatch, golden, bits):
    """ABPOA_HIP_NOXL=1 at 196, 215 and 216: dp_wide_kernel's 7-chunk body up to wide_w_hi = 215, where the rows of 8 chunks (54-374 of them) come back
    exact from the general body; at 216 no alignment takes the wide loop."""
    monkeypatch.setenv("ABPOA_HIP_NOXL", "1")
    _with_trace(golden, bits, WB.NOXL_BANDS, "no long-read form")


@pytest.mark.parametrize("bits32", [False, True], ids=["m2", "m_gate32"])
def test_mixed_launch(engine, bits32):
    """seq_ag_gb, heter_ag_gb, ragged_ag_gb and s1k_ag_gb in ONE launch at wb = 10, wf = 0.2: w = 20 (narrow kernel) beside w = 163 .. 209 (long-read kernel, rows
    of 3-8 chunks and, at the gate point, up to 15); at match = the int32 gate point of the longest query that query runs in 32 bits beside six in 16.  Every
    alignment against the oracle, planes included, order preserved; then without the trace."""
    cases = mixed_cases(bits32)
    items = [(label, c, H.run_oracle(c)) for label, c in cases]
    assert {o.bits for _, _, o in items} == ({16, 32} if bits32 else {16})
    for trace in (True, False):
        launch(items, trace, "mixed launch")


@pytest.mark.parametrize("wb,at_least", WB.EXTZ_BANDS, ids=[f"wb{w}" for w, _ in WB.EXTZ_BANDS])
def test_extension_mode_with_zdrop(engine, wb, at_least):
    """heter_cg_extz (both containers; extension mode, z-drop 5) on rows of >= 5 chunks (wb = 100) and >= 8 (wb = 250): the row loop's z-drop break and the
    best-cell bookkeeping of extension mode in the all-chunk bodies; records with and without the trace."""
    n = 0
    for label, path in H.golden_cases():
        if not label.startswith("heter_cg_extz/"):
            continue
        g = H.read_abpg(path)
        d = {k: np.array(g[k], copy=True) for k in H._INPUT_KEYS}
        d["wb"], d["wf"] = np.array([wb], np.int32), np.array([0.0], np.float32)
        c = H.FlatCase(d)
        o = H.run_oracle(c)
        for trace in (True, False):
            launch([(label, c, o)], trace, f"extension z-drop wb={wb}")
        n += 1
    assert n == 2
