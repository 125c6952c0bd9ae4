"""GPU (-m gpu): the all-rounds kernel's backtrack helpers start while the row loop still runs (abpoa_amd/csrc/backtrack_dir.h, EARLY START).  Whatever the
schedule, the results are the same: for every job below the cigar digests (ABPOA_HIP_CIGAR_DIGEST: every graph cigar of a set folded into 64 bits on the
device), the consensus records and the per-set status are identical in three forms -- the default, the late start (ABPOA_HIP_LATE_TAIL=1) and one wavefront
per backtrack (ABPOA_HIP_DBG bit 10) -- and equal to the CPU build of the host layer whose aligner is the plain-C oracle (tests/cpu_shim.cpp).

The digest switch is read once per process, so ONE child process (tests/readset_worker.py) runs every job of make_jobs() in every form and reports; the tests
below look at its report.  Nothing here depends on timing: a helper that starts early, late or not at all leaves the same cigar."""
import re

import pytest

from readset_worker import run_report

pytestmark = pytest.mark.gpu

AFFINE = dict(gap_open1=4, gap_open2=0, gap_ext1=2)
FORMS = {"default": {}, "late_start": {"ABPOA_HIP_LATE_TAIL": "1"}, "one_wavefront": {"ABPOA_HIP_DBG": "1024"}}
# job -> (Params keywords, [(reads, length)], index of the read replaced by an unrelated one or None, extra environment of the device runs)
# The helpers engage at graphs of 768 rows: reads of about 800 bases are the smallest that get there (int16 scores, 5 % errors).
JOBS = {
    "plain": (AFFINE, [(6, 800 + 13 * i) for i in range(8)], None, {}),
    # graphs that stay under 768 rows, cross it in a late round, or start above it: both schedules in one launch
    "threshold": (AFFINE, [(6, ln) for ln in (640, 690, 700, 715, 730, 745, 760, 820)], None, {}),
    # one read of the set has nothing to do with the graph: the helpers of its alignment start on branches the real path never touches
    "no_splice": (AFFINE, [(6, 820 + 11 * i) for i in range(4)], 3, {}),
    # arenas of the 3x pass at 6 % of the estimate (enough for the first rounds of these sets, not for the last): the row loops end with the overflow status in mid-graph (the helpers abandon, or finish a walk nobody
    # reads), the sets leave the pass and a later one redoes them
    "capacity": (AFFINE, [(6, 800 + 17 * i) for i in range(4)], None, {"ABPOA_HIP_ARENA_PCT": "6", "ABPOA_HIP_NO_PASS_HINT": "1"}),
    # extension mode with z-drop (a row loop that may stop before a helper's start row; today such jobs keep score records and one launch per phase)
    "extend_zdrop": (dict(aln_mode=2, zdrop=200), [(6, 800 + 19 * i) for i in range(4)], None, {}),
    # linear gaps: poa_rounds_kernel<0>, no direction words, no helpers
    "linear": (dict(gap_open1=0, gap_open2=0, gap_ext1=2), [(6, 800 + 23 * i) for i in range(4)], None, {}),
}


def make_jobs():
    """{job: spec} for tests/readset_worker.py."""
    from abpoa_amd import synth
    jobs = {}
    for job, (kw, shapes, stranger, env) in JOBS.items():
        sets = [synth.make_read_set(61, i, n, ln, 0.05) for i, (n, ln) in enumerate(shapes)]
        if stranger is not None:
            for i, (n, ln) in enumerate(shapes):
                sets[i][stranger] = synth.make_read_set(977, i, 1, ln, 0.0)[0]
        jobs[job] = dict(params=kw, sets=sets, forms=FORMS, env=env, record=("dig", "rounds_launches", "n_host_sets"), ref_record=("dig",))
    return jobs


@pytest.fixture(scope="module")
def report():
    """(the report, {(job, form): what the library said on stderr during that run})"""
    return run_report("test_gpu_overlap_tail", set_env={"ABPOA_HIP_CIGAR_DIGEST": "1", "ABPOA_HIP_VERBOSE": "1"}, timeout=600, want_log=True,
                      clear_env=("ABPOA_HIP_LATE_TAIL", "ABPOA_HIP_DBG", "ABPOA_HIP_LOCKSTEP", "ABPOA_HIP_ARENA_PCT"))


@pytest.mark.parametrize("job", list(JOBS))
def test_three_schedules_one_result(report, job):
    rep, log = report
    r = rep[job]
    ref = r["ref"]
    assert all(s == 0 for s in ref["status"]) and all(d != 0 for d in ref["dig"])
    for form in FORMS:
        got = r[form]
        assert got["status"] == ref["status"], f"{job} / {form}: per-set status"
        assert got["dig"] == ref["dig"], f"{job} / {form}: cigar digests differ from the oracle-backed run"
        assert got["cons"] == ref["cons"] and got["cov"] == ref["cov"], f"{job} / {form}: consensus records differ from the oracle-backed run"
    for form in ("late_start", "one_wavefront"):
        assert r[form]["dig"] == r["default"]["dig"] and r[form]["cons"] == r["default"]["cons"] and r[form]["cov"] == r["default"]["cov"]


def test_the_jobs_take_the_paths_they_are_about(report):
    """The all-rounds kernel ran wherever it can (not in extension mode), its helpers started under the row loop by default and after it with the switch,
    four workgroups per CU either way; and the capacity job's sets did leave the 3x pass with the row loop's overflow status."""
    rep, log = report
    for job in JOBS:
        for form in FORMS:
            assert rep[job][form]["n_host_sets"] == 0, f"{job} / {form}: sets on the host driver"
            assert (rep[job][form]["rounds_launches"] > 0) == (job != "extend_zdrop"), f"{job} / {form}"
    for job in ("plain", "threshold", "no_splice", "capacity"):
        assert "helpers under the row loop" in log[(job, "default")], log[(job, "default")][-2000:]
        assert "helpers after the row loop" in log[(job, "late_start")], log[(job, "late_start")][-2000:]
        assert "helpers under the row loop" not in log[(job, "late_start")]
    assert "helpers after the row loop" in log[("linear", "default")]
    for form in FORMS:
        assert re.search(r"arena too small for the bands [1-4]", log[("capacity", form)]), log[("capacity", form)][-2000:]
