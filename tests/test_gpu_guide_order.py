"""GPU (-m gpu): the guide-tree read order (-p, ABPOA_HIP_PROGRESSIVE) against what the reference recorded (tests/golden/guide_order/, written by
tools/make_guide_order_golden.py from the reference's own abpoa_collect_mm / abpoa_build_guide_tree and from `abpoa_ref -p`).

* the sketch kernel, value for value through abpoa_hip_guide_order: read lengths around every edge of the walk (k-1, k, w+k-2 .. w+k, the last k-mer at lanes
  63 / 64 / 65, the kernel's tile +-1, 1 kb, more than two tiles), read content (ambiguous bases at the start, in the middle, at the end, as a run;
  homopolymers; period-2 and period-3 repeats; both strands over k-mers equal to their own reverse complement), parameters at their limits, amino acids;
* the pair kernel's hit matrix and the order: n = 2, 3, 64, 65, 50 x 1 kb, duplicate reads, reads shorter than k, four sets in one call;
* the batch entry end to end, byte for byte against the recorded output of `abpoa_ref -p` (and against the binary itself where it was built), through both
  drivers, and each against an independent route: the reads permuted by the recorded order through the unflagged path, rows put back."""
import ctypes as C
import glob
import io
import json
import os
import subprocess

import numpy as np
import pytest

from gpu_harness import engine  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "guide_order")
GOLDEN = os.path.join(ROOT, "tests", "golden")
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "abpoa_ref")


def _names(prefix):
    return sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLD, prefix + "*.npz")))


def _load(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    ro, mo = np.concatenate([[0], np.cumsum(z["lens"])]), np.concatenate([[0], np.cumsum(z["mm_len"])])
    reads = [np.ascontiguousarray(z["reads"][ro[r]:ro[r + 1]]) for r in range(len(z["lens"]))]
    sketch = [z["mm"][mo[r]:mo[r + 1]] for r in range(len(z["lens"]))]
    return dict(name=name, tile=int(z["tile"]), m=int(z["m"]), k=int(z["k"]), w=int(z["w"]), both=bool(z["both"]), reads=reads, sketch=sketch, hit=z["hit"].tolist(), order=z["order"].tolist())


E2E = {c["name"]: c for c in json.load(open(os.path.join(GOLD, "e2e.json")))["cases"]}


def _check_sets(cases):
    """One abpoa_hip_guide_order call for `cases` (same alphabet and parameters): sketch, hit matrix and order of every set."""
    from abpoa_amd import api
    c0 = cases[0]
    assert all((c["m"], c["k"], c["w"], c["both"]) == (c0["m"], c0["k"], c0["w"], c0["both"]) for c in cases)
    got = api.guide_order([c["reads"] for c in cases], api.Params(is_aa=c0["m"] > 5), mm_k=c0["k"], mm_w=c0["w"], both_strands=c0["both"], hits=True, sketch=True)
    for c, g in zip(cases, got):
        for r, (a, b) in enumerate(zip(g.sketch, c["sketch"])):
            assert a.tolist() == b.tolist(), f"{c['name']}: sketch of read {r} (length {len(c['reads'][r])}): {len(a)} values, the reference {len(b)}"
        assert g.hit == c["hit"], f"{c['name']}: hit matrix"
        assert g.order == c["order"], f"{c['name']}: order"


@pytest.mark.parametrize("name", _names("sketch_"))
def test_sketch_kernel_matches_the_reference(engine, name):
    c = _load(name)
    if name == "sketch_lengths":      # the edges the fixture must hold: nothing, one value, the first full window, the tile of THIS library's kernel
        engine.abpoa_hip_guide_tile.restype = C.c_int
        tile = engine.abpoa_hip_guide_tile()
        assert c["tile"] == tile, "the fixture was written for another tile length: rerun tools/make_guide_order_golden.py"
        lens, n_mm, k, w = [len(r) for r in c["reads"]], [len(s) for s in c["sketch"]], c["k"], c["w"]
        assert dict(zip(lens, n_mm))[k - 1] == 0 and dict(zip(lens, n_mm))[k] == 1 and dict(zip(lens, n_mm))[w + k - 2] == 1
        assert {tile - 1, tile, tile + 1, 1000, w + k - 1, w + k, 63 + k, 64 + k, 65 + k} <= set(lens) and max(lens) > 2 * tile
    if name.startswith("sketch_long_"):      # sketches beyond what the kernel sorts in the LDS (2 048 values): sorted in place
        assert max(len(s) for s in c["sketch"]) > 2048
    _check_sets([c])


@pytest.mark.parametrize("name", _names("pairs_"))
def test_pair_kernel_and_order_match_the_reference(engine, name):
    c = _load(name)
    if name in ("pairs_n2", "pairs_all_short", "pairs_test"):
        assert c["order"] == list(range(len(c["reads"])))
    _check_sets([c])


def test_four_sets_of_different_size_in_one_call(engine):
    _check_sets([_load(n) for n in ("pairs_n65", "pairs_n2", "pairs_duplicates", "pairs_all_short", "pairs_n50x1k", "pairs_n3", "pairs_seq")])


def test_parameters_outside_their_range_are_refused(engine):
    from abpoa_amd import api
    api._bind_msa(engine)
    enc, out = api.EncodedSets([["ACGTACGTACGT"] * 3], 5), (api.Msa * 1)()
    for m, k, w in ((5, 29, 10), (5, 200, 10), (27, 12, 4)):
        sc = api.Params(is_aa=m > 5).scoring()
        assert engine.abpoa_hip_msa_batch(C.byref(sc), 1, enc.sets, out, api.OUT_CONS | api.PROGRESSIVE | api.guide_kw(k, w), 1) == -2, (m, k, w)


def test_cli_refuses_parameters_outside_their_range(engine, capsys):
    from abpoa_amd import cli
    seq = os.path.join(GOLDEN, "data", "seq.fa")
    for bad in (["-k", "29"], ["-w", "256"], ["-k", "-3"], ["-c", "-k", "12"]):
        assert cli.main(["-p", *bad, seq], out=io.StringIO()) == 2
        assert "guide order" in capsys.readouterr().err


# ---- end to end
def _cli(args, path):
    from abpoa_amd import cli
    buf = io.StringIO()
    assert cli.main([*args, path], out=buf) == 0
    return buf.getvalue()


def _input_of(case, tmp_path):
    if case["file"]:
        return os.path.join(GOLDEN, case["file"])
    path = tmp_path / (case["name"] + ".fa")
    path.write_text("".join(f">r{i}\n{r}\n" for i, r in enumerate(case["reads"])))
    return str(path)


FILE_CASES = [n for n, c in E2E.items() if c["file"]]


@pytest.mark.parametrize("name", FILE_CASES)
def test_batch_entry_reproduces_abpoa_ref_p(engine, tmp_path, name):
    """seq.fa / heter.fa at -r 0 / 1 / 2, with and without -s (no row may come back as a reverse complement), -k 15 -w 5, FASTQ weights (-Q), linear gaps,
    local mode (the flag changes nothing there)."""
    from abpoa_amd import api
    case = E2E[name]
    path = _input_of(case, tmp_path)
    got = _cli(["-p", *case["args"]], path)
    assert got == case["output"], f"{name}: differs from the recorded `abpoa_ref -p {' '.join(case['args'])}`"
    assert "_reverse_complement" not in got
    if name == "heter_affine_r0":
        assert api.msa_timing()["n_host_sets"] == 0, "affine gaps, consensus: the device-resident driver"
    if name == "heter_local_r2":
        assert got == _cli(case["args"], path), "local mode: the flag must change nothing"
    if name in ("seq_r2", "heter_r2"):
        assert case["differs_from_input_order"] and got != _cli(case["args"], path), "the guide order changes these outputs"
    if os.path.exists(REF_BIN):
        p = subprocess.run([REF_BIN, "-p", *case["args"], path], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and got == p.stdout, f"{name}: differs from abpoa_ref run here"


@pytest.mark.parametrize("name", ["heter_r2", "heter_r2_s", "seq_r0", "heter_affine_r0", "fastq_Q_r2", "heter_k15w5_r2"])
def test_batch_entry_reproduces_abpoa_ref_p_on_the_host_driver(engine, tmp_path, monkeypatch, name):
    """The same jobs with the host driver forced (ABPOA_HIP_HOSTGRAPH=1: host graph, one launch per round)."""
    from abpoa_amd import api
    monkeypatch.setenv("ABPOA_HIP_HOSTGRAPH", "1")
    case = E2E[name]
    assert _cli(["-p", *case["args"]], _input_of(case, tmp_path)) == case["output"]
    assert api.msa_timing()["n_host_sets"] == 1, "the host driver was asked for"


@pytest.mark.parametrize("group", ["mixed_", "mixed_cons_", "ragged_r2", "ragged_cons"])
def test_mixed_and_ragged_jobs_in_one_call(engine, tmp_path, group):
    """One job of several sets (-l): 2-read sets beside larger ones; sets whose read lengths lie far apart."""
    cases = [c for n, c in E2E.items() if n.startswith(group) and (group != "mixed_" or n[len(group):].isdigit())]
    assert cases and all(c["args"] == cases[0]["args"] for c in cases)
    if group.startswith("mixed"):
        assert {len(c["reads"]) for c in cases} >= {2} and max(len(c["reads"]) for c in cases) > 4
    lst = tmp_path / "list.txt"
    lst.write_text("".join(_input_of(c, tmp_path) + "\n" for c in cases))
    assert _cli(["-p", "-l", *cases[0]["args"]], str(lst)) == "".join(c["output"] for c in cases)


def _rows(res):
    return [(r.status, r.cons_seq, r.cons_cov, r.msa_seq, r.is_rc) for r in res]


@pytest.mark.parametrize("name,kw,amb,use_q", [("pairs_heter", dict(), False, False), ("pairs_heter_both", dict(), True, False), ("pairs_seq", dict(), False, False),
                                              ("pairs_heter", dict(gap_open1=0, gap_open2=0, gap_ext1=2, gap_ext2=0), False, False),
                                              ("pairs_heter", dict(gap_open1=4, gap_open2=0, gap_ext1=2), False, True), ("pairs_n50x1k", dict(gap_open1=4, gap_open2=0, gap_ext1=2), False, False)])
def test_flag_equals_permuted_reads_through_the_unflagged_path(engine, name, kw, amb, use_q):
    """The independent route: reads (and their per-base weights) permuted by the RECORDED order, the unflagged entry, MSA rows moved back to input order."""
    from abpoa_amd import api
    c = _load(name)
    order, n = c["order"], len(c["reads"])
    assert sorted(order) == list(range(n)) and order != list(range(n))
    p = api.Params(**kw)
    wts = [[(np.arange(len(r)) * (i + 3) % 7 + 1).astype(np.int32) for i, r in enumerate(c["reads"])]] if use_q else None
    for out_msa in (True, False):
        got = api.msa_batch([c["reads"]], p, out_cons=True, out_msa=out_msa, weights=wts, amb_strand=amb, progressive=True)[0]
        ref = api.msa_batch([[c["reads"][i] for i in order]], p, out_cons=True, out_msa=out_msa, weights=[[wts[0][i] for i in order]] if use_q else None)[0]
        assert got.status == 0 and ref.status == 0
        assert got.cons_seq == ref.cons_seq and got.cons_cov == ref.cons_cov
        assert got.is_rc == [False] * n and (not amb or bool(got._o.is_rc)), "no read is reverse-complemented under the flag; -s still returns the array"
        if out_msa:
            back = [None] * n
            for r, i in enumerate(order):
                back[i] = ref.msa_seq[r]
            assert got.msa_seq == back + [ref.msa_seq[-1]]
            same = api.msa_batch([c["reads"]], p, out_cons=True, out_msa=True, weights=wts)[0]
            assert kw or same.msa_seq != got.msa_seq, "the flag did nothing"


def test_context_entry_honours_the_flag(engine):
    from abpoa_amd import api
    sets = [_load(n)["reads"] for n in ("pairs_heter", "pairs_n2", "pairs_duplicates", "pairs_seq")]
    for kw in (dict(), dict(gap_open1=4, gap_open2=0, gap_ext1=2)):
        p = api.Params(**kw)
        ctx = api.BatchContext()
        try:
            a = ctx.msa_batch(sets, p, out_cons=True, out_msa=True, progressive=True)
            b = api.msa_batch(sets, p, out_cons=True, out_msa=True, progressive=True)
            plain = ctx.msa_batch(sets, p, out_cons=True, out_msa=True)
            assert _rows(a) == _rows(b) and _rows(a) != _rows(plain)
            a = ctx.msa_batch(sets, p, progressive=True, mm_k=15, mm_w=5)
            b = api.msa_batch(sets, p, progressive=True, mm_k=15, mm_w=5)
            assert _rows(a) == _rows(b)
            a = ctx.msa_batch(sets, p, out_cons=True, out_msa=True, amb_strand=True, progressive=True)      # -p -s: the both-strand sketch
            b = api.msa_batch(sets, p, out_cons=True, out_msa=True, amb_strand=True, progressive=True)
            assert _rows(a) == _rows(b) and all(bool(r._o.is_rc) and not any(r.is_rc) for r in a)
            assert kw or a[0].msa_seq == E2E["heter_r2_s"]["output"].split("\n")[1::2]
            # k / w without the flag mean nothing
            api._bind_msa(engine)
            enc, out = api.EncodedSets(sets, 5), (api.Msa * len(sets))()
            sc = p.scoring()
            assert engine.abpoa_hip_msa_batch(C.byref(sc), len(sets), enc.sets, out, api.OUT_CONS | api.OUT_MSA | api.guide_kw(200, 5), 1) == 0
            assert _rows(api.BatchResults(api._BatchOut(engine, out, len(sets)), 5)) == _rows(plain)
        finally:
            ctx.close()


def test_pyabpoa_batch_method_takes_the_flag(engine):
    from abpoa_amd import pyabpoa, seqio
    c = _load("pairs_heter")
    reads = [seqio.decode(r, 5) for r in c["reads"]]
    a = pyabpoa.msa_aligner()
    got = a.msa_batch([reads], out_cons=True, out_msa=True, progressive=True)[0]
    assert got.msa_seq == E2E["heter_r2"]["output"].split("\n")[1::2]      # the rows of the recorded output (its names are the file's)
