"""CPU: conditions on the INPUTS of tests/test_gpu_wide_bodies.py (table: tests/wide_bands.py), checked on the oracle's bands and on the launch plan -- that
the re-banded 1 kb goldens do give rows of every chunk count the all-chunk bodies are instantiated for (and one past each kernel's widest body), that the plan
answers at every point what the table says (which ring, which bands take the wide loop, where the fast loops end), and that the thresholds the table's bands
straddle are the plan's.  The GPU tests could otherwise pass without running the bodies they name."""
import collections
import ctypes as C

import numpy as np
import pytest

import helpers as H
import wide_bands as WB
from abpoa_amd import ffi

_ORACLE = {}


def chunk_counts(o):
    """Counter: chunks of 64 columns per computed row of oracle output o (the row loops' own count: ceil((dp_end_sn - dp_beg_sn + 1) * PN / 64))."""
    pn = 16 if o.bits == 16 else 8
    act = o.dp_beg_sn >= 0
    return collections.Counter((((o.dp_end_sn[act] - o.dp_beg_sn[act] + 1) * pn + 63) // 64).tolist())


def _run(golden, bits, wb):
    k = (golden, bits, wb)
    if k not in _ORACLE:
        g = H.first_golden(golden)
        c = H.FlatCase(H.rescored(g, WB.point(golden, bits, int(g["qlen"][0])), wb, 0.0))
        o = H.run_oracle(c)
        assert o.status == 0 and o.bits == bits, k
        _ORACLE[k] = (c, chunk_counts(o))
    return _ORACLE[k]


def _hook(case, bits, n_aln=1, **switches):
    """abpoa_hip__wide_plan for one launch of n_aln alignments like `case` -> ((wide_on, lo, hi, ring rows), LDS bytes of the wide kernels' ring)."""
    lib = ffi.lib()
    lib.abpoa_hip_set_option.argtypes = [C.c_char_p, C.c_char_p]
    out = (C.c_int * 8)()
    for k, v in switches.items():
        assert lib.abpoa_hip_set_option(k.encode(), str(v).encode()) == 0
    try:
        lib.abpoa_hip__wide_plan(C.byref(case.sc), case.qlen, bits, n_aln, out)
    finally:
        for k in switches:
            lib.abpoa_hip_set_option(k.encode(), None)
    return (out[0], out[5], out[6], out[1]), out[2] - out[4]


@pytest.mark.parametrize("golden,bits", WB.COMBOS, ids=[f"{g}_i{b}" for g, b in WB.COMBOS])
def test_bands_give_rows_of_every_chunk_count(golden, bits):
    """Over the table's bands: at least 100 rows of every chunk count from 2 to 11; the bands one past a kernel's widest body hold rows of 8 chunks (215 with
    the 448-column kernel), respectively 12 (343 / 344)."""
    union = collections.Counter()
    for wb in WB.BANDS:
        cnt = _run(golden, bits, wb)[1]
        print(f"{golden} int{bits} wb={wb}: {sorted(cnt.items())}")
        union.update(cnt)
    for n in range(2, 12):
        assert union[n] >= 100, (golden, bits, n, union[n])
    for _, wb, n in WB.ONE_PAST:
        assert _run(golden, bits, wb)[1][n] >= 1, (golden, bits, wb, n)
    # the 4-row ring's five bands: 5, 6, 7, 8 or 9, and 11 chunks, a hundred rows and more each
    n_at ={wb: _run(golden, bits, wb)[1] for wb in WB.RING4_BANDS}
    assert n_at[130][5] >= 100 and n_at[165][6] >= 100 and n_at[196][7] >= 100 and n_at[250][8] + n_at[250][9] >= 100 and n_at[324][11] >= 100, (golden, bits)


@pytest.mark.parametrize("golden,bits", WB.COMBOS, ids=[f"{g}_i{b}" for g, b in WB.COMBOS])
def test_plan_table_is_what_the_hook_answers(golden, bits):
    """(wide_on, wide_w_lo, wide_w_hi, ring rows) per band as data in the table == the hook; the ring's columns follow from wide_w_hi and are what the plan's
    LDS bytes hold; `inside` is 40 <= wb <= hi; the same under ABPOA_HIP_NOXL=1 and with a 4-row ring."""
    fww = 1 if (bits == 16 and golden == "s1k_ag_gb") else 2      # ring words per column of the wide kernels (int32 convex: H and one word of differences)
    for wb in WB.BANDS:
        case = _run(golden, bits, wb)[0]
        got, ring_bytes = _hook(case, bits)
        assert got == WB.plan(golden, bits, wb), (golden, bits, wb, got)
        on, lo, hi, rows = got
        assert WB.inside(golden, bits, wb) == (on == 1 and 40 <= wb <= hi) == (wb not in (39, 344) and got != WB.OFF), (golden, bits, wb)
        if on:
            cols = WB.RING_COLS[hi]
            assert hi == (cols - 17) // 2 and ring_bytes == rows * fww * (cols + 4) * 4, (golden, bits, wb, got, ring_bytes)
        else:
            assert (golden, bits) == ("s1k_cg_gb", 32) and wb >= WB.CG32_FAST_OFF_FROM and not WB.fast_loops(golden, bits, wb)
    for wb in WB.NOXL_BANDS:
        got, ring_bytes = _hook(_run(golden, bits, wb)[0], bits, ABPOA_HIP_NOXL=1)
        assert got == WB.plan(golden, bits, wb, noxl=True) == WB.R448 and ring_bytes == 16 * fww * 452 * 4, (golden, bits, wb, got)
        assert WB.inside(golden, bits, wb, noxl=True) == (wb <= 215)
    for wb in WB.RING4_BANDS:
        got, _ = _hook(_run(golden, bits, wb)[0], bits, ABPOA_HIP_RING_ROWS=4)
        assert got == WB.plan(golden, bits, wb)[:3] + (4,) and WB.inside(golden, bits, wb), (golden, bits, wb, got)


@pytest.mark.parametrize("golden,bits", WB.COMBOS, ids=[f"{g}_i{b}" for g, b in WB.COMBOS])
def test_thresholds_are_the_plans(golden, bits):
    """Scanned through the hook, band by band: the first band half-width with the 704-column ring (185 in int16, 197 in int32) and -- int32 convex at a 1 kb
    query only -- the first without any fast row loop (325); the table holds the band on either side of each."""
    case = _run(golden, bits, 100)[0]
    seen = {}
    for wb in range(40, 400):
        case.sc.wb = wb
        seen[wb] = _hook(case, bits)[0]
    case.sc.wb = 100
    first_704 = min(wb for wb, p in seen.items() if p[2] == 343)
    off = [wb for wb, p in seen.items() if p[0] == 0]
    print(f"{golden} int{bits}: 704-column ring from w = {first_704}, fast loops off from {min(off) if off else None}")
    assert first_704 == WB.RING_704_FROM[bits] and all(p[2] == 215 for wb, p in seen.items() if wb < first_704)
    assert first_704 - 1 in WB.BANDS and first_704 in WB.BANDS
    if (golden, bits) == ("s1k_cg_gb", 32):
        assert off == list(range(WB.CG32_FAST_OFF_FROM, 400)) and WB.CG32_FAST_OFF_FROM - 1 in WB.BANDS and WB.CG32_FAST_OFF_FROM in WB.BANDS
    else:
        assert off == []


def test_skip_table_of_the_words_variants_is_the_plans():
    """A (point, words variant) is left out exactly where the plan keeps no fast row loop; dir_plane_usable holds at all four scorings."""
    for golden, bits in WB.COMBOS:
        assert WB.point(golden, bits, int(H.first_golden(golden)["qlen"][0])).dir_usable()
        for wb in WB.BANDS:
            assert ((golden, bits, wb) in WB.NO_WORDS) == (not WB.fast_loops(golden, bits, wb)) == (_hook(_run(golden, bits, wb)[0], bits)[0][0] == 0)


def _golden_cases(*names):
    return [(label, H.read_abpg(path)) for label, path in H.golden_cases() if label.split("/")[0] in names]


def test_extension_goldens_give_the_rows_the_zdrop_test_names():
    """heter_cg_extz (both containers, z-drop 5) at wb = 100 / 250: at least 100 computed rows of 5 chunks and more, respectively 8 and more, in the wide loop's bands."""
    items = _golden_cases("heter_cg_extz")
    assert len(items) == 2
    for label, g in items:
        assert int(g["align_mode"][0]) == 2 and int(g["zdrop"][0]) > 0
        for wb, at_least in WB.EXTZ_BANDS:
            d = {k: np.array(g[k], copy=True) for k in H._INPUT_KEYS}
            d["wb"], d["wf"] = np.array([wb], np.int32), np.array([0.0], np.float32)
            c = H.FlatCase(d)
            o = H.run_oracle(c)
            cnt = chunk_counts(o)
            got, _ = _hook(c, o.bits)
            print(f"{label} wb={wb}: int{o.bits} {sorted(cnt.items())} plan {got}")
            assert sum(v for n, v in cnt.items() if n >= at_least) >= 100 and got[0] == 1 and got[1] <= wb <= got[2], (label, wb, cnt, got)


MIXED = ("seq_ag_gb", "heter_ag_gb", "ragged_ag_gb", "s1k_ag_gb")


def mixed_cases(bits32):
    """The affine goldens under one scoring at wb = 10, wf = 0.2: [(label, FlatCase)] in the order of the launch.  bits32: match = the int32 gate point of the
    longest query instead of 2."""
    import scoring_points as SP
    items = _golden_cases(*MIXED)
    qmax = max(int(g["qlen"][0]) for _, g in items)
    pt = SP.Point("mixed", "wide", match=SP.width_gate_points(qmax)[1].kw["match"] if bits32 else 2, **WB.GAPS["s1k_ag_gb"])
    return [(label, H.FlatCase(H.rescored(g, pt, 10, 0.2))) for label, g in items]


@pytest.mark.parametrize("bits32", [False, True], ids=["m2", "m_gate32"])
def test_mixed_launch_holds_narrow_and_wide_alignments(bits32):
    """One launch: band half-widths of 20 (narrow kernel) and 163-209 (the 704-column ring: w_max >= 185), rows of 3 to 8 chunks and more; at the gate point of
    the longest query that query alone scores in 32 bits -- the shorter ones stay in 16 --, so both widths share the launch."""
    cases = mixed_cases(bits32)
    assert len(cases) == 7
    ws, widths, union = [], set(), collections.Counter()
    for label, c in cases:
        o = H.run_oracle(c)
        assert o.status == 0
        w = c.sc.wb + int(np.float32(c.sc.wf) * np.float32(c.qlen))
        ws.append(w); widths.add(o.bits)
        if w >= 40:
            union.update(chunk_counts(o))
        print(f"{label}: w = {w}, int{o.bits}, {sorted(chunk_counts(o).items())}")
    assert sorted(set(ws)) == [20, 163, 191, 194, 209]
    widest = max(cases, key=lambda lc: lc[1].qlen)[1]
    got, _ = _hook(widest, 32 if bits32 else 16, n_aln=len(cases))
    assert got[:3] == (1, 40, 343)
    assert widths == ({16, 32} if bits32 else {16})
    for n in range(3, 12 if bits32 else 9):
        assert union[n] >= 30, (n, union[n])
