"""CPU: the harness the GPU tests stand on (tests/gpu_harness.py, tests/readset_worker.py) does bite.  compare_launch is held to the oracle's own output
of one small golden, altered one word at a time; the worker runs end to end with the CPU shim standing in for the device library (a switch of the worker
that exists for this file), so that the protocol -- jobs from the test module, forms with their environments, markers, report, the parent's assertion when
the child dies -- is tested where no GPU is."""
import copy
import os

import pytest

import helpers as H
from gpu_harness import compare_launch
from readset_worker import SHIM_AS_DEVICE, run_report, split_log

VARS = ("HARNESS_TEST_FIRST", "HARNESS_TEST_SECOND")


@pytest.fixture(scope="module")
def golden_item():
    """(name, FlatCase, the oracle's output with the trace) of one small golden"""
    case = H.FlatCase(H.first_golden("seq_ag_gb"))
    o = H.run_oracle(case)
    assert o.rc == 0 and o.status == 0 and o.n_cigar > 0 and len(o.planes) > 0
    return ("seq_ag_gb", case, o)


def _untraced(o):
    h = copy.deepcopy(o)
    for k in ("dp_beg", "dp_end", "dp_beg_sn", "dp_end_sn", "row_max_i", "row_off", "planes"):
        delattr(h, k)
    return h


def test_compare_launch_passes_on_equal_copies(golden_item):
    o = golden_item[-1]
    compare_launch([golden_item], [copy.deepcopy(o)], True, "equal")
    compare_launch([golden_item], [_untraced(o)], False, "equal")
    compare_launch([golden_item, golden_item], [copy.deepcopy(o), copy.deepcopy(o)], True, "equal", bits=o.bits)


def test_compare_launch_raises_on_one_cigar_word(golden_item):
    h = copy.deepcopy(golden_item[-1])
    h.cigar[len(h.cigar) // 2] ^= 1 << 4
    with pytest.raises(AssertionError, match="label seq_ag_gb trace=True: cigar differs"):
        compare_launch([golden_item], [h], True, "label")
    with pytest.raises(AssertionError, match="seq_ag_gb trace=False: cigar differs"):
        compare_launch([golden_item], [_untraced(h)], False, "label")


def test_compare_launch_raises_on_one_plane_cell(golden_item):
    h = copy.deepcopy(golden_item[-1])
    h.planes[len(h.planes) // 2] += 1
    with pytest.raises(AssertionError, match="seq_ag_gb trace=True: plane cell differs: row"):
        compare_launch([golden_item], [h], True, "label")


def test_compare_launch_raises_on_a_missing_or_unasked_trace(golden_item):
    o = golden_item[-1]
    with pytest.raises(AssertionError, match="seq_ag_gb"):
        compare_launch([golden_item], [_untraced(o)], True, "label")
    with pytest.raises(AssertionError, match="seq_ag_gb"):
        compare_launch([golden_item], [copy.deepcopy(o)], False, "label")


def test_compare_launch_raises_on_status_width_and_length(golden_item):
    o = golden_item[-1]
    with pytest.raises(AssertionError):
        compare_launch([golden_item, golden_item], [copy.deepcopy(o)], True, "label")
    with pytest.raises(AssertionError):
        compare_launch([golden_item], [], True, "label")
    h = copy.deepcopy(o)
    h.status = 3
    with pytest.raises(AssertionError, match="seq_ag_gb"):
        compare_launch([golden_item], [h], True, "label")
    with pytest.raises(AssertionError, match="seq_ag_gb"):
        compare_launch([golden_item], [copy.deepcopy(o)], True, "label", bits=48 - o.bits)


def test_split_log():
    text = "before any run\n[job] a plain\nline 1\nline 2\n[job] a other\n[job] b/x plain\nline 3\n"
    assert split_log(text) == {("a", "plain"): "line 1\nline 2", ("a", "other"): "", ("b/x", "plain"): "line 3"}


def make_jobs(only=None):
    """{job: spec} for tests/readset_worker.py: two sets of three 60-base reads in two forms, each with a variable of its own."""
    from abpoa_amd import synth
    sets = [synth.make_read_set(7, i, 3, 60, 0.05) for i in range(2)]
    jobs = {"small": dict(params=dict(gap_open1=4, gap_open2=0, gap_ext1=2), sets=sets, forms={"first": {VARS[0]: "1"}, "second": {VARS[1]: "2"}},
                          env={"HARNESS_TEST_JOB": "j"}, first_set_forms=("second",), record=("n_cells", "msa", "dig", "n_host_sets"), ref_record=("dig",),
                          env_seen=VARS + ("HARNESS_TEST_JOB", "HARNESS_TEST_PARENT", "HARNESS_TEST_CLEARED"))}
    return jobs if only is None else {k: v for k, v in jobs.items() if k == only}


def test_worker_end_to_end_on_the_cpu_shim(monkeypatch):
    monkeypatch.setenv("HARNESS_TEST_CLEARED", "x")
    before = dict(os.environ)
    rep, log = run_report("test_gpu_harness", "small", set_env={SHIM_AS_DEVICE: "1", "ABPOA_HIP_CIGAR_DIGEST": "1", "HARNESS_TEST_PARENT": "p"},
                          clear_env=("HARNESS_TEST_CLEARED",), timeout=120, want_log=True)
    assert dict(os.environ) == before, "the parent's environment is untouched"
    assert list(rep) == ["small"] and list(rep["small"]) == ["first", "second", "ref"]
    assert list(log) == [("small", "first"), ("small", "second")] and all(isinstance(v, str) for v in log.values())
    first, second, ref = (rep["small"][k] for k in ("first", "second", "ref"))
    assert len(first["status"]) == 2 and len(second["status"]) == 1 and len(ref["status"]) == 2, "`second` runs the first set only"
    assert first["status"] == ref["status"] == [0, 0] and second["status"] == [0]
    assert all(d != 0 for d in ref["dig"]) and first["dig"] == ref["dig"] and second["dig"] == ref["dig"][:1]
    assert first["cons"] == ref["cons"] and first["cov"] == ref["cov"] and all(len(c) > 40 for c in ref["cons"])
    assert set(first) == {"status", "cons", "cov", "n_cells", "msa", "dig", "n_host_sets", "env"} and set(ref) == {"status", "cons", "cov", "dig", "env"}
    assert all(len(rows) == 4 and len(set(map(len, rows))) == 1 for rows in first["msa"]), "three reads and the consensus row per set"
    # a form's variables are there for its run and gone for the next; the job's are there for every device run; set_env and clear_env reached the child
    common = {"HARNESS_TEST_PARENT": "p", "HARNESS_TEST_CLEARED": None}
    assert first["env"] == dict(common, HARNESS_TEST_FIRST="1", HARNESS_TEST_SECOND=None, HARNESS_TEST_JOB="j")
    assert second["env"] == dict(common, HARNESS_TEST_FIRST=None, HARNESS_TEST_SECOND="2", HARNESS_TEST_JOB="j")
    assert ref["env"] == dict(common, HARNESS_TEST_FIRST=None, HARNESS_TEST_SECOND=None, HARNESS_TEST_JOB=None)


def test_a_child_that_dies_fails_the_parent_with_its_stderr():
    with pytest.raises(AssertionError, match="ModuleNotFoundError.*no_such_jobs_module"):
        run_report("no_such_jobs_module", set_env={SHIM_AS_DEVICE: "1"}, clear_env=(), timeout=120)
