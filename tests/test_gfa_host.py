"""GFA output (ABPOA_HIP_OUT_GFA; the reference's -r 3 / -r 4, abpoa_generate_gfa src/abpoa_output.c:168-268) of the host layer, on the CPU: the batch driver,
PoaGraph::gfa, the formatter and the front ends through the oracle-backed build of the host layer (tests/_build/libcpu_shim.so), byte for byte against the
reference's recorded output (tests/golden/gfa/, tools/make_gfa_golden.py) and, where the compiled reference is present, against a run of it."""
import io
import os
import re
import subprocess

import numpy as np
import pytest

import gfa_cases as GC
import helpers as H
from abpoa_amd import api, cli, seqio

D = H.GOLDEN_DIR


def _cli_text(args):
    out = io.StringIO()
    assert cli.main(args, lib=H.cpu_shim_lib(), out=out) == 0, args
    return out.getvalue()


def _cpu_binary():
    """the C front end against the CPU build of the host layer, built as tests/test_c_frontend.py builds it"""
    H.cpu_shim_lib()
    bdir = os.path.join(H.ROOT, "tests", "_build")
    exe, src = os.path.join(bdir, "abpoa_batch_cpu"), os.path.join(H.ROOT, "abpoa_amd", "host", "abpoa_batch.c")
    shim = os.path.join(bdir, "libcpu_shim.so")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(shim)):
        subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-Wall", "-I" + os.path.join(H.ROOT, "include"), "-o", exe, src, "-L" + bdir, "-lcpu_shim", "-lz", "-lpthread", "-lm",
                               "-Wl,-rpath," + bdir])
    return exe


@pytest.mark.parametrize("name", GC.PLAIN)
def test_format_gfa_equals_the_reference(name, tmp_path):
    """api.msa_batch(out_gfa=True) + api.format_gfa (through cli.main: the reference's arguments, --gfa / --gfa-cons for -r 3 / -r 4): -s with reversed '-'
    paths, amino acids, local and extension mode, a one-read set, two identical reads.  Invariants from the record itself: NL of the header is n_link and the
    number of L lines; every read's path is as long as the read."""
    case = GC.CASES[name]
    path = GC.case_input(case, tmp_path)
    text = _cli_text(GC.front_end_args(case, path))
    GC.assert_matches(case, text, "cli.main on the CPU build")
    head = re.match(r"H\tVN:Z:1.0\tNS:i:(\d+)\tNL:i:(\d+)\tNP:i:(\d+)\n", text)
    lines = text.splitlines()
    assert int(head.group(1)) == sum(ln.startswith("S\t") for ln in lines) and int(head.group(2)) == sum(ln.startswith("L\t") for ln in lines)
    names, reads, _ = seqio.read_fastx(path)
    out_cons = "--gfa-cons" in GC.front_end_args(case, path)
    assert int(head.group(3)) == len(reads) + (1 if out_cons else 0)
    paths = [ln.split("\t") for ln in lines if ln.startswith("P\t")]
    for i, r in enumerate(reads):
        assert paths[i][1] == (names[i] or str(i + 1)) and len(paths[i][2].split(",")) == len(r) and paths[i][3] == "*", (name, i)
    if os.path.exists(GC.REF):
        ref = subprocess.run([GC.REF] + GC.ref_args(case, path), capture_output=True, text=True, timeout=600)
        assert ref.returncode == 0 and ref.stdout == text, name


def test_record_and_flag_semantics():
    """OUT_GFA alone computes no consensus; OUT_GFA | OUT_MSA fills both, the MSA rows those of an OUT_MSA run; the record's arrays hold together; a run
    without the flag carries no record."""
    shim = H.cpu_shim_lib()
    _, reads, _ = seqio.read_fastx(os.path.join(D, "data", "heter.fa"))
    p = api.Params()
    g = api.msa_batch([reads], p, out_cons=False, out_gfa=True, lib=shim)[0]
    assert g.status == 0 and g.cons_len == 0 and g.cons_seq == "" and g.msa_len == 0
    rec = g.gfa
    assert rec is not None and rec.n_path == len(reads) and rec.n_seg == len(rec.seg_node) == len(rec.seg_base) and rec.n_link == len(rec.link_from) == int(rec.link_off[-1])
    assert sorted(rec.seg_node.tolist()) == list(range(1, rec.n_seg + 1)), "every inner node once, printed as id - 1"
    assert np.array_equal(np.diff(rec.path_off), [len(r) for r in reads]) and int(rec.path_off[-1]) == len(rec.path_node)
    letters = np.frombuffer(seqio.NT_DECODE.encode(), np.uint8)
    pos = np.empty(rec.n_seg + 2, np.int64); pos[rec.seg_node] = np.arange(rec.n_seg)
    for i, r in enumerate(reads):      # a path spells its read
        nodes = rec.path_node[rec.path_off[i]:rec.path_off[i + 1]]
        assert bytes(letters[rec.seg_base[pos[nodes]]]).decode() == r.upper(), i
    both = api.msa_batch([reads], p, out_cons=True, out_msa=True, out_gfa=True, lib=shim)[0]
    msa = api.msa_batch([reads], p, out_cons=True, out_msa=True, lib=shim)[0]
    assert both.msa_seq == msa.msa_seq and both.cons_seq == msa.cons_seq and msa.gfa is None
    GC.same_record(both.gfa, rec, "OUT_GFA | OUT_MSA | OUT_CONS against OUT_GFA")
    assert api.format_gfa(msa) == "" and api.format_gfa(both, out_cons=True).endswith("\t*\n")


def test_pyabpoa_batch_carries_the_record():
    from abpoa_amd import pyabpoa as pa
    _, reads, _ = seqio.read_fastx(os.path.join(D, "data", "test.fa"))
    a = pa.msa_aligner(_lib=H.cpu_shim_lib())
    r = a.msa_batch([reads], out_cons=True, out_gfa=True)[0]
    assert r.gfa is not None and r.gfa.n_path == len(reads) and r.cons_len[0] > 0
    assert a.msa_batch([reads], out_cons=True)[0].gfa is None


def test_c_front_end_prints_the_reference_text(tmp_path):
    """abpoa_batch --gfa / --gfa-cons (abpoa_hip_format_gfa) on the fixture inputs, a `-l` list in pieces included"""
    exe = _cpu_binary()
    for name in ("test_r3", "test_r4", "seq_affine_r4", "aa_blosum_local_r4", "rc_long_s_r4", "rc_s_r3", "one_read_r4", "ragged_ext_r4", "list6_r4"):
        case = GC.CASES[name]
        args = GC.front_end_args(case, GC.case_input(case, tmp_path))
        p = subprocess.run([exe] + (["--piece", "4"] if case.get("list") else []) + args, capture_output=True, timeout=600)
        assert p.returncode == 0, (name, p.stderr[-1000:])
        GC.assert_matches(case, p.stdout, "abpoa_batch on the CPU build")


def test_python_front_end_list(tmp_path):
    case = GC.CASES["list6_r4"]
    GC.assert_matches(case, _cli_text(GC.front_end_args(case, GC.case_input(case, tmp_path))), "cli.main -l on the CPU build")


def test_front_ends_refuse_gfa_beside_another_output():
    seq = os.path.join(D, "data", "seq.fa")
    for bad in (["--gfa", "-r", "1"], ["--gfa-cons", "-r", "2"], ["--gfa", "-r", "5"], ["--gfa", "--gfa-cons"]):
        assert cli.main(bad + [seq], lib=H.cpu_shim_lib(), out=io.StringIO()) == 2, bad
        p = subprocess.run([_cpu_binary()] + bad + [seq], capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and p.stdout == "", bad
