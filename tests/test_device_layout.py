"""CPU (-m "not gpu"): the byte arithmetic of the device-resident driver (abpoa_amd/csrc/msa_device_layout.cpp: the offsets of every pool in the three device
blobs, the round-major read tables, the kernel-argument bindings, the MSA / GFA result layouts, the unpacking of one set's results, the event slots) on plans
of small synthetic read-sets: every pool aligned, disjoint and at least as large as its consumer indexes, every pointer at its table entry inside a buffer of
exactly the blob's bytes, and a keyed round trip through the result pools.  The harness (tests/device_layout.cpp) is a stand-alone program built with
-fsanitize=undefined,address against that source, the plan, the switches, poa_graph.cpp (gfa_alloc) and its own stand-ins for the kernels' constants."""
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
    exe = tmp_path_factory.mktemp("layout") / "device_layout"
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-pthread", "-fsanitize=undefined,address", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
                    "-I/opt/rocm/include", "-I" + CSRC, "-o", str(exe), os.path.join(ROOT, "tests", "device_layout.cpp"), os.path.join(CSRC, "msa_device_layout.cpp"),
                    os.path.join(CSRC, "msa_device_plan.cpp"), os.path.join(CSRC, "engine_options.cpp"), os.path.join(CSRC, "poa_graph.cpp")],
                   check=True, timeout=300, capture_output=True)
    return str(exe)


def test_device_layout_bindings_and_unpacking(harness):
    p = subprocess.run([harness], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "device layout ok" in p.stdout and p.stderr == "", (p.stdout[-3000:], p.stderr[-3000:])
