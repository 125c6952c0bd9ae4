"""CPU (-m "not gpu"): the planning step of the device-resident driver (abpoa_amd/csrc/msa_device_plan.cpp: which kernels a job takes, direction words or
score records, the wide row loop's range, the extra columns of ragged sets, the last pass's edge slots) on synthetic read-length lists, against the routing
that DESIGN.md sections 1 and 4.7 document, each case again with one switch set through set_option and once more after its reset; and the typed switch
accessors of engine_options.cpp (unknown names, "0" is set but not on, reads while another thread sets and resets the switch).  The harness
(tests/device_plan.cpp) is a stand-alone program built with -fsanitize=undefined,address against the two sources and its own lds_fixed_bytes_*."""
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
    exe = tmp_path_factory.mktemp("plan") / "device_plan"
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-pthread", "-fsanitize=undefined,address", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
                    "-I/opt/rocm/include", "-I" + CSRC, "-o", str(exe), os.path.join(ROOT, "tests", "device_plan.cpp"), os.path.join(CSRC, "msa_device_plan.cpp"),
                    os.path.join(CSRC, "engine_options.cpp")], check=True, timeout=300, capture_output=True)
    return str(exe)


def test_device_plan_and_switch_accessors(harness):
    p = subprocess.run([harness], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "device plan ok" in p.stdout and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, (p.stdout[-3000:], p.stderr[-3000:])
