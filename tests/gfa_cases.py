"""What the GFA tests (tests/test_gfa_host.py, tests/test_gpu_gfa.py) share: the fixture cases of tests/golden/gfa/ (tools/make_gfa_golden.py), their
inputs as files, and the comparison of a text with the recorded one (the text itself where it is committed, else its byte count and sha256).  A plain module."""
import hashlib
import json
import os

import numpy as np

import helpers as H
from abpoa_amd import synth

GFA_DIR = os.path.join(H.GOLDEN_DIR, "gfa")
REF = os.path.join(H.ROOT, "oracle", "_ref", "abpoa_ref")
CASES = {c["name"]: c for c in json.load(open(os.path.join(GFA_DIR, "cases.json")))["cases"]}
PLAIN = [n for n, c in CASES.items() if "-p" not in c["args"] and not c.get("list")]      # what the CPU build of the host layer can run: no guide order


def case_input(case, tmp_path):
    """the case's input file (a `list` case: the list of its files), written under tmp_path where the case does not name a committed file"""
    if case.get("file"):
        return os.path.join(H.GOLDEN_DIR, case["file"])
    if case.get("list"):
        files = []
        for i, kw in enumerate(case["list"]):
            fn = str(tmp_path / f"s{i}.fa")
            with open(fn, "w") as f:
                for j, r in enumerate(synth.make_read_set(**kw)):
                    f.write((f">r{j}\n" if (i + j) % 4 else ">\n") + r + "\n")
            files.append(fn)
        lst = str(tmp_path / "list.txt")
        open(lst, "w").write("\n".join(files) + "\n")
        return lst
    fn = str(tmp_path / (case["name"] + ".fa"))
    synth.write_fasta(fn, case["reads"] if case.get("reads") else synth.make_read_set(**case["synth"]))
    return fn


def front_end_args(case, path):
    """the case's reference arguments as this project's front ends take them: --gfa / --gfa-cons for -r 3 / -r 4"""
    a = [os.path.join(H.GOLDEN_DIR, "data", "BLOSUM62.mtx") if x == "@BLOSUM62" else x for x in case["args"]]
    i = a.index("-r")
    long_opt = {"3": "--gfa", "4": "--gfa-cons"}[a[i + 1]]
    return a[:i] + a[i + 2:] + [long_opt] + (["-l"] if case.get("list") else []) + [path]


def ref_args(case, path):
    return [os.path.join(H.GOLDEN_DIR, "data", "BLOSUM62.mtx") if x == "@BLOSUM62" else x for x in case["args"]] + (["-l"] if case.get("list") else []) + [path]


def assert_matches(case, text, what):
    data = text.encode() if isinstance(text, str) else text
    if case["text"]:
        want = open(os.path.join(GFA_DIR, case["name"] + ".gfa"), "rb").read()
        assert data == want, f"{what}: {case['name']}: text differs from the reference's"
    assert len(data) == case["bytes"], f"{what}: {case['name']}: {len(data)} bytes, the reference printed {case['bytes']}"
    assert hashlib.sha256(data).hexdigest() == case["sha256"], f"{what}: {case['name']}: sha256 differs from the reference's"


def same_record(a, b, what):
    """two SetResult.gfa records, array for array"""
    assert (a is None) == (b is None), what
    if a is None:
        return
    assert (a.n_seg, a.n_link, a.n_path) == (b.n_seg, b.n_link, b.n_path), f"{what}: counts {(a.n_seg, a.n_link, a.n_path)} vs {(b.n_seg, b.n_link, b.n_path)}"
    for k in ("seg_node", "seg_base", "link_off", "link_from", "path_off", "path_node"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), f"{what}: {k} differs"
