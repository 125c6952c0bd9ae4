"""CPU (-m "not gpu"): the host arithmetic of the flat batch driver (abpoa_amd/csrc/batch_plan.cpp: alignment descriptors and arena estimates, the two blob
layouts and the download prefixes, eligibility for the fast row loops, the direction-word tables row_sdist / row_pd, the plan and the arenas of a first pass
and of a retry, the DevBatch pointers, the unpacking of a saved arena into trace planes) on synthetic shapes: the tables against a naive double loop, every
planned pass against the kernels' per-alignment routing rule (routing.h), each launch again in trace mode and with ABPOA_HIP_DIR_WIDE / ABPOA_HIP_NODIR set
through set_option.  The harness (tests/batch_plan.cpp) is a stand-alone program built with -fsanitize=undefined,address against the three sources and its
own lds_fixed_bytes_*."""
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
    exe = tmp_path_factory.mktemp("plan") / "batch_plan"
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-pthread", "-fsanitize=undefined,address", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
                    "-I/opt/rocm/include", "-I" + CSRC, "-o", str(exe), os.path.join(ROOT, "tests", "batch_plan.cpp"), os.path.join(CSRC, "batch_plan.cpp"),
                    os.path.join(CSRC, "msa_device_plan.cpp"), os.path.join(CSRC, "engine_options.cpp")], check=True, timeout=300, capture_output=True)
    return str(exe)


def test_batch_plan(harness):
    p = subprocess.run([harness], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "batch plan ok" in p.stdout and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, (p.stdout[-3000:], p.stderr[-3000:])
