"""CPU (-m "not gpu"): the integer closed forms of the all-chunks row body (abpoa_amd/csrc/wide_closed_forms.h, called by rows_fast.h ilp_chunks) against
literal restatements, in a C++ harness (tests/wide_row_closed_forms.cpp) built against the kernels' own header with -fsanitize=undefined:

  * the packed arg-max keys (int16: absolute vector order; int32: value relative to a floor, vector order within the row) of random rows of 1-11 chunks --
    rows of more than 64 vectors, ties across lanes / vectors / in the end vector, the end_sn == qlen_sn mask, inf cells, int16 extremes, int32 winners at
    and beyond the window's edges -- reduced with an unsigned max in a shuffled order and decoded, against the reference's max_in_row; int32 rows are
    declined exactly when the true maximum lies outside the window;
  * the chunk carry chain (seed[c + 1] = max(total[c], seed[c]) - 64 e) with the per-chunk unseeded prefix maxima, against the literal vector-by-vector
    F scan chained across the row (affine and convex planes, e = 0, inf stretches)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "abpoa_amd", "csrc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path_factory.mktemp("wcf") / "wide_row_closed_forms"
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-I" + CSRC, "-o", str(exe),
                    os.path.join(ROOT, "tests", "wide_row_closed_forms.cpp")], check=True, timeout=300, capture_output=True)
    return str(exe)


@pytest.mark.parametrize("what,seed,iters", [("key16", 11, 400), ("key32", 12, 400), ("key32", 13, 400), ("carry", 14, 12)])
def test_wide_row_closed_forms(harness, what, seed, iters):
    p = subprocess.run([harness, what, str(seed), str(iters)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "closed forms ok" in p.stdout and "runtime error" not in p.stderr, (p.stdout[-3000:], p.stderr[-3000:])


@pytest.mark.parametrize("label,bits", [("s3k_ag_i32_b300", 32), ("s3k_cg_i32_b300", 32), ("s3k_ag_b300", 16)])
def test_long_row_goldens_reach_9_to_11_chunks(label, bits):
    """The goldens of the long-read form's bodies (tests/test_gpu_parity.py runs them plane-exact) keep rows of 9, 10 and 11 chunks in their score width."""
    import sys
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import helpers as H
    paths = [p for lab, p in H.golden_cases() if lab.split("/")[0] == label]
    assert len(paths) == 1, paths
    g = H.read_abpg(paths[0])
    assert int(np.asarray(g["bits"]).ravel()[0]) == bits
    pn = 16 if bits == 16 else 8
    nch = ((np.asarray(g["dp_end_sn"]) - np.asarray(g["dp_beg_sn"]) + 1) * pn + 63) // 64
    for c in (9, 10, 11):
        assert (nch == c).sum() >= 100, (label, c, np.bincount(nch))
