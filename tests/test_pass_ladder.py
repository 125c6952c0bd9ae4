"""CPU (-m "not gpu"): the decisions of the batch entry above run_msa_device (abpoa_amd/csrc/msa_passes.cpp): the node-slot pass ladder -- start pass, chunk
sizes, ENOMEM halving, the hand-back on ENOMEM of one set / EINVAL, any other rc, edge-slot sets deferred to the last pass, learning and forgetting the start
hint, ABPOA_HIP_FIRST_PASS / _PASS_SETS / _NO_PASS_HINT set through set_option and reset -- over a scripted runner that records every call; deal_batches,
split_ragged, parse_device_list; host_reason_of over every device reason code.  The harness (tests/pass_ladder.cpp) is a stand-alone program built with
-fsanitize=undefined,address from msa_passes.cpp and engine_options.cpp; its two-thread case on one hint store runs once more in a -fsanitize=thread build."""
import os
import re
import shutil
import subprocess

import pytest

from abpoa_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "abpoa_amd", "csrc")


def _build(tmp_path_factory, name, sanitize):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path_factory.mktemp(name) / "pass_ladder"
    p = subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-pthread", *sanitize, "-I" + CSRC, "-o", str(exe), os.path.join(ROOT, "tests", "pass_ladder.cpp"),
                        os.path.join(CSRC, "msa_passes.cpp"), os.path.join(CSRC, "engine_options.cpp")], timeout=300, capture_output=True, text=True)
    return p, str(exe)


def _run_clean(exe):
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "pass ladder ok" in p.stdout and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, (p.stdout[-3000:], p.stderr[-3000:])
    return p.stdout


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    p, exe = _build(tmp_path_factory, "ladder", ["-fsanitize=undefined,address", "-fno-sanitize-recover=undefined"])
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def test_pass_ladder_dealing_and_reasons(harness):
    out = _run_clean(harness)
    # the harness prints the engine's number of host reason slots: the names api.host_reasons() reports are one per slot
    assert int(re.search(r"MSA_HOST_REASONS (\d+)", out).group(1)) == len(api.HOST_REASONS)


def test_hint_store_under_thread_sanitizer(tmp_path_factory):
    p, exe = _build(tmp_path_factory, "ladder_tsan", ["-fsanitize=thread"])
    if p.returncode != 0:
        pytest.skip("no -fsanitize=thread build here: " + p.stderr.strip()[-300:])
    _run_clean(exe)
