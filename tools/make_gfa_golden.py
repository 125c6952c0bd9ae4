"""Records the reference's GFA output (-r 3 / -r 4) as fixtures under tests/golden/gfa/ (needs oracle/_ref/abpoa_ref: the compiled reference).

  cases.json   per case: name, the reference's arguments, the input -- `file` (a path under tests/golden/), `reads` (the reads themselves), `synth`
               (keywords of synth.make_read_set; FASTA names r0, r1, ...) or `list` (several synth sets, one file each, run with -l; record j of file i is
               named r<j>, or has no name where (i + j) % 4 == 0) -- and the byte count and sha256 of the reference's stdout
  <name>.gfa   that stdout itself where it is under 16 KB

    python tools/make_gfa_golden.py            # rewrites every fixture (deterministic)
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from abpoa_amd import synth  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "abpoa_ref")
GOLDEN = os.path.join(ROOT, "tests", "golden")
OUT_DIR = os.path.join(GOLDEN, "gfa")
TEXT_LIMIT = 16 * 1024
BLOSUM = "data/BLOSUM62.mtx"      # (written "@BLOSUM62" in a case's arguments)


def write_list(td, specs):
    """the files of a `list` case and the list itself; returns the list's path"""
    files = []
    for i, kw in enumerate(specs):
        fn = os.path.join(td, f"s{i}.fa")
        with open(fn, "w") as f:
            for j, r in enumerate(synth.make_read_set(**kw)):
                f.write((f">r{j}\n" if (i + j) % 4 else ">\n") + r + "\n")
        files.append(fn)
    lst = os.path.join(td, "list.txt")
    with open(lst, "w") as f:
        f.write("\n".join(files) + "\n")
    return lst


def input_path(case, td):
    if case.get("file"):
        return os.path.join(GOLDEN, case["file"])
    if case.get("list"):
        return write_list(td, case["list"])
    reads = case["reads"] if case.get("reads") else synth.make_read_set(**case["synth"])
    fn = os.path.join(td, "in.fa")
    synth.write_fasta(fn, reads)
    return fn


def ref_args(case):
    return [os.path.join(GOLDEN, BLOSUM) if a == "@BLOSUM62" else a for a in case["args"]] + (["-l"] if case.get("list") else [])


def run_ref(case):
    with tempfile.TemporaryDirectory() as td:
        p = subprocess.run([REF] + ref_args(case) + [input_path(case, td)], capture_output=True, timeout=600)
    assert p.returncode == 0, (case["name"], p.stderr[-1000:])
    return p.stdout


CASES = [
    dict(name="test_r3", args=["-r", "3"], file="data/test.fa"),
    dict(name="test_r4", args=["-r", "4"], file="data/test.fa"),
    dict(name="seq_affine_r4", args=["-O", "4,0", "-E", "2", "-r", "4"], file="data/seq.fa"),
    dict(name="heter_r4", args=["-r", "4"], file="data/heter.fa"),
    dict(name="s1k_affine_r4", args=["-O", "4,0", "-E", "2", "-r", "4"], file="out_s1k_cons/input.fa"),
    dict(name="ragged_ext_r4", args=["-m", "2", "-r", "4"], file="out_ragged_ext_cons/input.fa"),
    dict(name="ragged_local_r3", args=["-m", "1", "-r", "3"], file="out_ragged_ext_cons/input.fa"),
    dict(name="aa_blosum_local_r4", args=["-m", "1", "-c", "-t", "@BLOSUM62", "-r", "4"], file="aa_blosum_loc/input.fa"),
    dict(name="rc_long_s_r4", args=["-s", "-r", "4"], file="out_rc_long_msa/input.fa"),
    dict(name="rc_s_r3", args=["-s", "-r", "3"], file="out_rc_cons/input.fa"),
    dict(name="one_read_r4", args=["-r", "4"], reads=["ACGTTGCAAGGCTTAACG"]),
    dict(name="two_identical_r3", args=["-r", "3"], reads=["ACGTTGCAAGGCTTAACGGATC"] * 2),
    # guide-tree order (-p): the CPU build of the host layer has none, the GPU tests compare with these
    dict(name="test_p_r4", args=["-p", "-r", "4"], file="data/test.fa"),
    dict(name="seq_p_r4", args=["-p", "-r", "4"], file="data/seq.fa"),
    dict(name="heter_p_r4", args=["-p", "-r", "4"], file="data/heter.fa"),
    dict(name="synth12x400_p_r4", args=["-p", "-r", "4"], synth=dict(seed=53, set_index=0, n_reads=12, length=400, err=0.10)),
    # a list of files, for the front ends' -l
    dict(name="list6_r4", args=["-r", "4"], list=[dict(seed=9, set_index=i, n_reads=4 + i, length=150 + 40 * i, err=0.06) for i in range(6)]),
]


if __name__ == "__main__":
    os.makedirs(OUT_DIR, exist_ok=True)
    out = []
    for case in CASES:
        text = run_ref(case)
        rec = dict(case, bytes=len(text), sha256=hashlib.sha256(text).hexdigest(), text=len(text) < TEXT_LIMIT)
        if rec["text"]:
            with open(os.path.join(OUT_DIR, case["name"] + ".gfa"), "wb") as f:
                f.write(text)
        out.append(rec)
        print(f"{case['name']}: {len(text)} bytes{'' if rec['text'] else ' (sha256 only)'}")
    with open(os.path.join(OUT_DIR, "cases.json"), "w") as f:
        json.dump(dict(cases=out), f, indent=1)
