"""CPU (-m "not gpu"): the start rows of the backtrack's helper walks (abpoa_amd/csrc/tail_schedule.h, the function the kernels call) for every graph of 768 to
70 000 rows: strictly decreasing, inside the graph, each the last row of a 64-row tile (the row loop's progress word moves at tile switches only, so such a row
is released by the very switch that completes it), a main walk of 64 .. 127 rows, the late start's quarters unchanged, and every helper done in time by the
header's own arithmetic.  The harness (tests/tail_schedule.cpp) is a stand-alone program built with -fsanitize=undefined,address."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "abpoa_amd", "csrc")


def build_harness(out_dir):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = os.path.join(str(out_dir), "tail_schedule")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-fsanitize=undefined,address", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
                    "-I/opt/rocm/include", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "tail_schedule.cpp")], check=True, timeout=300, capture_output=True)
    return exe


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("tail"))


def test_start_rows_of_every_graph(harness):
    p = subprocess.run([harness], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "tail schedule ok" in p.stdout and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, (p.stdout[-3000:], p.stderr[-3000:])


def test_start_rows_at_the_sizes_the_gpu_test_uses(harness):
    """The row counts tests/test_gpu_tail_final_pass.py aims at: either side of a tile boundary helper 1's start row moves by a whole tile."""
    p = subprocess.run([harness, "768", "831", "832", "895", "896", "1087", "1088", "1151", "1152", "2100"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = {int(a[0]): tuple(map(int, a[1:])) for a in (ln.split() for ln in p.stdout.splitlines())}
    assert rows[768][0] == 703 and rows[831][0] == 703 and rows[832][0] == 767 and rows[895][0] == 767 and rows[896][0] == 831
    assert rows[1087][0] == 959 and rows[1088][0] == 1023 and rows[1151][0] == 1023 and rows[1152][0] == 1087
    for n, (r1, r2, r3) in rows.items():
        assert n - 2 >= r1 > r2 > r3 >= 1 and all((r + 1) % 64 == 0 for r in (r1, r2, r3)), (n, r1, r2, r3)
