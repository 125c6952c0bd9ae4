"""CPU: conditions on the INPUTS of tests/test_gpu_scoring.py, checked on the oracle's planes -- that the re-scored goldens do enter the regimes the GPU
tests are there for (the wrap guards of the fast row loops, the clamps of the int32 arg-max key, both sides of the int16 / int32 gate), and that the
fixtures are what the table says they are.  The GPU tests could otherwise pass without running the code they name."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import scoring_points as SP

GB = ["s1k_ag_gb", "s1k_cg_gb", "seq_ag_gb", "heter_cg_gb", "ragged_ag_gb"]


def test_matrix_fixtures_are_asymmetric():
    a = SP.BY_NAME["asym_cg"].params().mat.reshape(5, 5)
    off = ~np.eye(4, dtype=bool)
    assert (a[:4, :4] != a[:4, :4].T)[off].all(), "ASYM5: every mirrored pair of A/C/G/T differs, so any transposed index changes a score"
    assert len(set(np.diag(a).tolist())) == 5
    h = SP.BY_NAME["hox_cg"].params().mat.reshape(5, 5)
    assert h[2, 3] == -114 and h[3, 2] == -144
    p = SP.BY_NAME["hox_cg"].params()
    assert (p.max_mat, p.min_mis) == (100, 144) and (SP.BY_NAME["asym_cg"].params().max_mat, SP.BY_NAME["asym_cg"].params().min_mis) == (7, 10)


@pytest.mark.parametrize("band", ["adaptive", "b3"])
@pytest.mark.parametrize("outside,inside", SP.GUARD_PAIRS, ids=[b for _, b in SP.GUARD_PAIRS])
def test_guard_pairs_enter_and_stay_out_of_the_wrap_regime(outside, inside, band):
    """The inside point of each guard pair has at least a quarter of its active rows below fast_lo by the M + q criterion (H.wrap_regime_rows), the
    outside point none, on every banded global golden the GPU tests re-score."""
    kw = dict(wb=3, wf=0.0) if band == "b3" else {}
    for name in GB:
        g = H.first_golden(name)
        c = H.FlatCase(H.rescored(g, SP.BY_NAME[inside], **kw))
        share = H.wrap_regime_rows(c, H.run_oracle(c))
        print(f"{inside} {band} {name}: {share:.2f} of the rows in the regime")
        assert share >= 0.25, (inside, name, share)
        if outside:
            c = H.FlatCase(H.rescored(g, SP.BY_NAME[outside], **kw))
            assert H.wrap_regime_rows(c, H.run_oracle(c)) == 0.0, (outside, name)


def test_default_matrix_and_cap_points_stay_out_of_the_wrap_regime():
    for pt in [SP.Point("default", "default")] + SP.group("matrix", "cap"):
        c = H.FlatCase(H.rescored(H.first_golden("s1k_cg_gb"), pt))
        assert H.wrap_regime_rows(c, H.run_oracle(c)) == 0.0, pt.name


@pytest.mark.parametrize("name", ["s1k_ag_gb", "s1k_cg_gb"])
def test_key_clamp_points_lie_outside_and_inside_the_int32_key_window(name):
    g = H.first_golden(name)
    out_pt, in_pt = SP.CLAMP_POINTS
    c = H.FlatCase(H.rescored(g, out_pt, wb=45, wf=0.0))
    o = H.run_oracle(c)
    share = H.key_window_rows(c, o)
    print(f"{out_pt.name} {name}: {share:.2f} of the rows outside the key's window")
    assert o.bits == 32 and share >= 0.5
    c = H.FlatCase(H.rescored(g, in_pt, wb=45, wf=0.0))
    o = H.run_oracle(c)
    assert o.bits == 32 and H.key_window_rows(c, o) == 0.0


@pytest.mark.parametrize("name", GB)
def test_width_gate_points_sit_on_both_sides_of_the_gate(name):
    g = H.first_golden(name)
    p16, p32 = SP.width_gate_points(int(g["qlen"][0]))
    lib = H.oracle_lib()
    for pt, bits in ((p16, 16), (p32, 32)):
        c = H.FlatCase(H.rescored(g, pt))
        assert lib.abpoa_oracle_score_bits(C.byref(c.sc), c.n_rows, c.qlen, None) == bits, (pt.name, name)
        o = H.run_oracle(c, want_trace=False)
        assert o.status == 0 and o.bits == bits
    # the 16-bit point runs scores near the top of the range
    c = H.FlatCase(H.rescored(g, p16))
    o = H.run_oracle(c, want_trace=False)
    print(f"{p16.name} {name}: best score {o.best_score}")
    # three quarters of the int16 range and more: a golden whose 16-bit run stays far from +32767 does not serve the GPU test of the key value + 2^15
    assert o.best_score >= 24000, (p16.name, name, o.best_score)
