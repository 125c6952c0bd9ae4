"""CPU (-m "not gpu"): the host half of the guide-tree read order (-p) and its way through the front ends.

* the greedy order (abpoa_amd/csrc/guide_order.cpp) in a stand-alone harness (tests/guide_order.cpp) under -fsanitize=undefined,address: every hit matrix
  recorded from the reference (tests/golden/guide_order/*.npz, tools/make_guide_order_golden.py) must give the recorded order -- seq.fa and heter.fa
  among them -- plus duplicate reads (exact ties), reads without minimizers (zero denominators) and n = 3 inside the harness;
* ABPOA_HIP_GUIDE_KW: packing and validation through api; the flag of api.msa_batch;
* the command line's -p -k -w."""
import glob
import os
import shutil
import subprocess

import numpy as np
import pytest

from abpoa_amd import api, cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "abpoa_amd", "csrc")
GOLD = os.path.join(ROOT, "tests", "golden", "guide_order")


def _cases():
    return [(os.path.basename(f)[:-4], np.load(f)) for f in sorted(glob.glob(os.path.join(GOLD, "*.npz")))]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path_factory.mktemp("guide") / "guide_order"
    p = subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-fsanitize=undefined,address", "-fno-sanitize-recover=undefined", "-I" + CSRC, "-o", str(exe),
                        os.path.join(ROOT, "tests", "guide_order.cpp"), os.path.join(CSRC, "guide_order.cpp")], timeout=300, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    return str(exe)


def test_greedy_order_reproduces_every_recorded_order(harness, tmp_path):
    cases = _cases()
    assert len(cases) >= 30
    named = dict(cases)
    assert named["pairs_seq"]["order"].tolist() == [7, 8, 0, 3, 1, 2, 4, 5, 6, 9]
    assert named["pairs_heter"]["order"].tolist() == [0, 3, 4, 13, 14, 10, 2, 8, 11, 1, 7, 9, 5, 6, 12]
    assert named["pairs_test"]["order"].tolist() == [0, 1, 2, 3] and int(named["pairs_test"]["mm_len"].sum()) == 0
    assert int(named["pairs_seq"]["mm_len"].sum()) == 54 and int(named["pairs_heter"]["mm_len"].sum()) == 1897
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        for _, z in cases:
            n = len(z["lens"])
            assert len(z["hit"]) == n * (n + 1) // 2 and len(z["order"]) == n
            f.write("%d\n%s\n%s\n" % (n, " ".join(map(str, z["hit"].tolist())), " ".join(map(str, z["order"].tolist()))))
    p = subprocess.run([harness, str(path)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "guide order ok: %d recorded cases" % len(cases) in p.stdout, (p.stdout[-2000:], p.stderr[-3000:])
    assert "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr[-3000:]


def test_guide_kw_packing_and_validation():
    assert api.PROGRESSIVE == 8
    assert api.guide_kw() == 0 and api.guide_kw(19, 10) == 19 << 8 | 10 << 16 and api.guide_kw(28, 255) == 28 << 8 | 255 << 16
    p, aa = api.Params(), api.Params(is_aa=True)
    assert api._batch_flags(p, True, False, False, False, 15, 5) == api.OUT_CONS                                   # k / w mean nothing without the flag
    assert api._batch_flags(p, True, True, True, True, 15, 5) == 1 | 2 | 4 | 8 | 15 << 8 | 5 << 16
    assert api._batch_flags(aa, True, False, False, True, 11, 0) == 1 | 8 | 11 << 8
    for k, w, params in ((29, 10, p), (-1, 10, p), (19, 256, p), (19, -1, p), (12, 4, aa), (256, 1, p)):
        with pytest.raises(ValueError):
            api._batch_flags(params, True, False, False, True, k, w)
    # the C header says the same
    hdr = open(os.path.join(ROOT, "include", "abpoa_hip.h")).read()
    assert "#define ABPOA_HIP_PROGRESSIVE 0x8u" in hdr and "ABPOA_HIP_GUIDE_KW(k, w)" in hdr
    for s in ("abpoa_hip_guide_order", "abpoa_hip_free_guide", "abpoa_hip_get_guide_timing"):
        assert hasattr(__import__("abpoa_amd.ffi", fromlist=["lib"]).lib(), s)


def test_cli_refuses_k_and_w_outside_their_range(capsys):
    """An error exit with a message, before any file is read or the engine is touched -- not a traceback."""
    for bad in (["-k", "29"], ["-w", "256"], ["-w", "-1"], ["-c", "-k", "12"]):
        assert cli.main(["-p", *bad, "no_such_file.fa"]) == 2
        assert "guide order" in capsys.readouterr().err


def test_tile_fixture_matches_the_kernel():
    """The read lengths of sketch_lengths.npz sit around the tile length the built kernel reports."""
    import ctypes as C
    from abpoa_amd import ffi
    lib = ffi.lib()
    lib.abpoa_hip_guide_tile.restype = C.c_int
    tile = lib.abpoa_hip_guide_tile()
    z = np.load(os.path.join(GOLD, "sketch_lengths.npz"))
    assert int(z["tile"]) == tile and {tile - 1, tile, tile + 1} <= set(z["lens"].tolist()) and int(z["lens"].max()) > 2 * tile
    longest = max(int(np.load(f)["mm_len"].max()) for f in glob.glob(os.path.join(GOLD, "sketch_long_*.npz")))
    assert longest > 2048, "no fixture reaches the in-place sort of the sketch kernel"


def test_cli_parser_knows_the_reference_letters():
    a = cli.build_parser().parse_args(["-p", "-k", "15", "-w", "5", "x.fa"])
    assert a.progressive and a.k_mer == 15 and a.window == 5
    a = cli.build_parser().parse_args(["--progressive", "--k-mer", "7", "--window", "4", "x.fa"])
    assert a.progressive and a.k_mer == 7 and a.window == 4
    a = cli.build_parser().parse_args(["x.fa"])
    assert not a.progressive and a.k_mer == 0 and a.window == 0
