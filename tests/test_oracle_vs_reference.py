"""CPU, development container only: diff the oracle against the compiled reference (oracle/_ref/ref_dump,
built by oracle/Makefile) on a matrix of gap modes x align modes x band on/off x score width, cell for cell.
Inputs are the reference's own data files as committed under tests/golden/data/.  Skipped where the reference
build is absent."""
import glob
import os

import pytest

import helpers as H
import scoring_points as SP
import wide_bands as WB
from abpoa_amd import synth

pytestmark = pytest.mark.skipif(not H.have_ref(), reason="reference build not available")
DATA = os.path.join(H.GOLDEN_DIR, "data")

AG, CG, LG = ["-O", "4,0", "-E", "2"], [], ["-O", "0,0", "-E", "2"]
MODES = {"gb": [], "gu": ["-b", "-1"], "loc": ["-m", "1"], "ext": ["-m", "2"], "extz": ["-m", "2", "-z", "5"]}


def _check(tmp_path, name, fa, opts, reads, sub=None):
    d = str(tmp_path / name)
    H.run_ref_dump(fa, d, opts, reads, planes=1, sub=sub)
    files = sorted(glob.glob(d + "/*.abpg"))
    assert files
    for f in files:
        g = H.read_abpg(f)
        o = H.run_oracle(H.FlatCase(g))
        H.compare_with_golden(o, g, label=name + "/" + os.path.basename(f))


@pytest.mark.parametrize("gap", ["ag", "cg", "lg"])
@pytest.mark.parametrize("mode", list(MODES))
def test_reference_test_data(tmp_path, gap, mode):
    g = {"ag": AG, "cg": CG, "lg": LG}[gap]
    _check(tmp_path, "seq", os.path.join(DATA, "seq.fa"), g + MODES[mode], "all")
    _check(tmp_path, "het", os.path.join(DATA, "heter.fa"), g + MODES[mode], "2,7,14")


@pytest.mark.parametrize("gap", ["ag", "cg", "lg"])
def test_synthetic_1kb(tmp_path, gap):
    fa = str(tmp_path / "s.fa")
    synth.write_fasta(fa, synth.make_read_set(7, 3, 10, 1000, 0.05))
    g = {"ag": AG, "cg": CG, "lg": LG}[gap]
    _check(tmp_path, "b", fa, g, "1,9")
    _check(tmp_path, "u", fa, g + ["-b", "-1"], "4")


@pytest.mark.parametrize("e1,wb", [(2, 10), (1, 3), (4, 2), (3, 6)], ids=["e2_b10", "e1_b3", "e4_b2", "e3_b6"])
def test_linear_gaps_with_narrow_bands(tmp_path, e1, wb):
    """Linear gaps with bands of -b 2 .. 10 -f 0: rows with stretches no real score reaches (the reference clamps those lanes at `inf`, src/simd_abpoa_align.c:773-775) --
    the regime of tests/test_gpu_parity.py::test_linear_rows_plane_level_on_the_golden_graphs, which compares the fast row loops with this oracle."""
    g = ["-O", "0,0", "-E", str(e1), "-b", str(wb), "-f", "0"]
    _check(tmp_path, "seq", os.path.join(DATA, "seq.fa"), g, "all")
    _check(tmp_path, "het", os.path.join(DATA, "heter.fa"), g, "2,7,14")
    fa = str(tmp_path / "s.fa")
    synth.write_fasta(fa, synth.make_read_set(17, 2, 8, 700, 0.12))
    _check(tmp_path, "syn", fa, g, "3,7")


def test_synthetic_10kb_int32(tmp_path):
    fa = str(tmp_path / "s.fa")
    synth.write_fasta(fa, synth.make_read_set(11, 0, 9, 10000, 0.15))
    _check(tmp_path, "cg", fa, CG, "8")
    _check(tmp_path, "ag", fa, AG, "8")


def test_amino_acid_blosum62(tmp_path):
    fa = str(tmp_path / "aa.fa")
    synth.write_fasta(fa, synth.make_read_set(13, 1, 8, 500, alphabet=synth.AA, rates=(0.05, 0.03, 0.03)))
    mtx = os.path.join(DATA, "BLOSUM62.mtx")
    _check(tmp_path, "loc", fa, ["-m", "1", "-c", "-t", mtx], "2,7")
    _check(tmp_path, "glob", fa, ["-c", "-t", mtx], "5")


def test_subgraph(tmp_path):
    _check(tmp_path, "s1", os.path.join(DATA, "seq.fa"), AG, "3,5,8", sub=(10, 40))
    _check(tmp_path, "s2", os.path.join(DATA, "heter.fa"), CG, "4,9", sub=(100, 500))


_SCORING_MODES = {"gb": [], "b3": ["-b", "3", "-f", "0"], "b45": ["-b", "45", "-f", "0"], "gu": ["-b", "-1"], "loc": ["-m", "1"], "ext": ["-m", "2"]}
_SCORING_POINTS = SP.POINTS + SP.CLAMP_POINTS + list(SP.width_gate_points(300))


@pytest.fixture(scope="module")
def scoring_fasta(tmp_path_factory):
    fa = str(tmp_path_factory.mktemp("scoring") / "s.fa")
    synth.write_fasta(fa, synth.make_read_set(23, 1, 8, 300, 0.10))
    return fa


@pytest.mark.parametrize("point", _SCORING_POINTS, ids=[p.name for p in _SCORING_POINTS])
def test_scoring_points(tmp_path, scoring_fasta, point):
    """The table of tests/scoring_points.py -- asymmetric matrices (ASYM5, HOXD70 as committed), the guard pairs of the fast row loops, the direction
    plane's field caps, the clamps of the int32 arg-max key, both sides of the int16 / int32 gate -- on 8 x 300 bases in every band (adaptive, 3, 45 -- the wide-loop tests' --, none) / alignment mode: the
    record behind "the oracle is the reference" for tests/test_gpu_scoring.py, which compares the kernels with the oracle at these points."""
    for mode, mo in _SCORING_MODES.items():
        _check(tmp_path, point.name + "_" + mode, scoring_fasta, point.ref_opts() + mo, "all")


LOCAL_READ_LENGTHS = (63, 64, 191, 192, 319, 320, 575, 576)


@pytest.mark.parametrize("gap", ["ag", "cg"])
@pytest.mark.parametrize("alphabet", ["aa", "nt"])
def test_local_mode_at_the_chunk_edges(tmp_path, alphabet, gap):
    """Local mode (-m 1), affine and convex, on amino-acid (BLOSUM62) and nucleotide reads of exactly 63, 64, 191, 192, 319, 320, 575 and 576 residues -- both
    sides of the body switches of the local row loops and of their hand-over to the general kernel -- against a graph one of whose reads carries a 20-residue
    insertion, so that later rows have a predecessor more than 16 rows back: the oracle that tests/test_gpu_local_bodies.py compares the kernels with is cell
    for cell the compiled reference there."""
    import numpy as np
    rng = np.random.default_rng(20260 + (alphabet == "aa"))
    letters = np.array(list(synth.AA if alphabet == "aa" else synth.NT))

    def noisy(codes, rate=0.06):
        out = codes.copy()
        hit = rng.random(len(out)) < rate
        out[hit] = rng.integers(0, len(letters), int(hit.sum()))
        return out
    base = rng.integers(0, len(letters), 640)
    reads = [base, noisy(base), np.concatenate([noisy(base[:40]), rng.integers(0, len(letters), 20), noisy(base[40:])])]
    reads += [noisy(base[7 * i:7 * i + n]) for i, n in enumerate(LOCAL_READ_LENGTHS)]
    fa = str(tmp_path / "loc.fa")
    synth.write_fasta(fa, ["".join(letters[r]) for r in reads])
    opts = ["-m", "1"] + (AG if gap == "ag" else CG) + (["-c", "-t", os.path.join(DATA, "BLOSUM62.mtx")] if alphabet == "aa" else [])
    d = str(tmp_path / "loc")
    H.run_ref_dump(fa, d, opts, "all", planes=1)
    files = sorted(glob.glob(d + "/*.abpg"))
    qlens, far = [], 0
    for f in files:
        g = H.read_abpg(f)
        assert int(g["align_mode"][0]) == 1 and int(g["wb"][0]) < 0 and int(g["gap_mode"][0]) == (1 if gap == "ag" else 2) and int(g["bits"][0]) == 16
        qlens.append(int(g["qlen"][0]))
        po, pr, n = g["pred_off"], g["pred_row"], int(g["n_rows"][0])
        far += any(r - int(pr[po[r]:po[r + 1]].min()) > 16 for r in range(1, n - 1)) and qlens[-1] in LOCAL_READ_LENGTHS
        H.compare_with_golden(H.run_oracle(H.FlatCase(g)), g, label=f"local {alphabet} {gap} " + os.path.basename(f))
    assert tuple(qlens[-len(LOCAL_READ_LENGTHS):]) == LOCAL_READ_LENGTHS and far == len(LOCAL_READ_LENGTHS)


@pytest.mark.parametrize("wb", [184, 250, 324])
@pytest.mark.parametrize("golden,bits", WB.COMBOS, ids=[f"{g}_i{b}" for g, b in WB.COMBOS])
def test_wide_bands_on_short_reads(tmp_path, golden, bits, wb):
    """Three bands of tests/wide_bands.py (-b 184 / 250 / 324 -f 0: rows of 6-7, 8-9 and 11 chunks of 64 columns) on the read-sets of the 1 kb goldens, affine
    and convex, at match 2 (16 bits) and at the first 32-bit match score: the oracle that tests/test_gpu_wide_bodies.py compares the all-chunk row bodies with
    is itself cell for cell the compiled reference at wide bands on short reads."""
    fa = os.path.join(H.GOLDEN_DIR, golden, "input.fa")
    pt = WB.point(golden, bits, int(H.first_golden(golden)["qlen"][0]))
    d = str(tmp_path / "w")
    H.run_ref_dump(fa, d, pt.ref_opts() + ["-b", str(wb), "-f", "0"], "5,11", planes=1)
    files = sorted(glob.glob(d + "/*.abpg"))
    assert len(files) == 2
    for f in files:
        g = H.read_abpg(f)
        assert int(g["bits"][0]) == bits and int(g["wb"][0]) == wb
        pn = 16 if bits == 16 else 8
        act = g["dp_beg_sn"] >= 0
        assert int(((g["dp_end_sn"][act] - g["dp_beg_sn"][act] + 1) * pn).max()) > 6 * 64      # rows of seven chunks and more
        H.compare_with_golden(H.run_oracle(H.FlatCase(g)), g, label=f"{golden} int{bits} wb={wb} " + os.path.basename(f))
