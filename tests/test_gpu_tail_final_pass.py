"""GPU (-m gpu): the all-rounds kernel's backtrack with helper start rows on tile boundaries next to the sink (abpoa_amd/csrc/tail_schedule.h) and the final
pass over the cigar shared by the workgroup's four wavefronts (backtrack_dir.h, helper_final_pass).  Whatever the schedule and however many wavefronts take the
pass, the results are the same: for every job below the cigar digests (ABPOA_HIP_CIGAR_DIGEST), the consensus records, the coverage and the per-set status are
identical in three forms -- the default, the late start (ABPOA_HIP_LATE_TAIL=1) and one wavefront per backtrack (ABPOA_HIP_DBG bit 10, which also keeps the
final pass on one wavefront) -- and equal to the CPU build of the host layer whose aligner is the plain-C oracle (tests/cpu_shim.cpp).  The result record of
each set's last alignment (abpoa_hip__last_aln: matched bases, aligned bases, node and query ends, cigar words) is the same in the three forms; the matched-base
count is the only place where the wavefronts' partial sums of the final pass show.

Read lengths (sets of 6 reads at 5 % error; a set's five graphs grow by about 3 % per read, so one set sweeps a range of row counts):
  700 .. 775    graphs that cross dir_walk_pair's 768 rows and stay within a few rows of it;
  745 .. 826    row counts on either side of 832 and 896, 1000 .. 1075 on either side of 1088 and 1152: there helper 1's start row moves by a whole tile
                (tests/test_tail_schedule.py pins the rows at those counts);
  2100          graphs of 2100 .. 2400 rows, as in the late rounds of the 1 kb benchmark sets: cigars of more than 2048 words, so every wavefront has
                more than one block of the final pass.
"no_splice": one read of the set has nothing to do with the graph (the main walk meets no helper: one segment, and helpers that come to the pass late);
"capacity": arenas that run out in mid-graph (the row loop ends with a status: the main wavefront's "no pass" word).
One child process (tests/readset_worker.py) runs every job of make_jobs() in every form.  Nothing here depends on timing, and nothing provokes a fault or a hang."""
import pytest

from readset_worker import run_report

pytestmark = pytest.mark.gpu

AFFINE = dict(gap_open1=4, gap_open2=0, gap_ext1=2)
FORMS = {"default": {}, "late_start": {"ABPOA_HIP_LATE_TAIL": "1"}, "one_wavefront": {"ABPOA_HIP_DBG": "1024"}}
# job -> ([(reads, length)], index of the read replaced by an unrelated one or None, extra environment of the device runs)
JOBS = {
    "threshold_768": ([(6, ln) for ln in (700, 715, 730, 745, 760, 775)], None, {}),
    "tiles_832_896": ([(6, ln) for ln in (790, 800, 808, 815, 820, 826, 850, 870)], None, {}),
    "tiles_1088_1152": ([(6, ln) for ln in (1000, 1020, 1040, 1060, 1075, 1100, 1130)], None, {}),
    "rows_2100": ([(6, 2100), (6, 2111)], None, {}),
    "no_splice": ([(6, 820 + 11 * i) for i in range(3)] + [(6, 2100)], 5, {}),
    "capacity": ([(6, 800 + 17 * i) for i in range(4)], None, {"ABPOA_HIP_ARENA_PCT": "6", "ABPOA_HIP_NO_PASS_HINT": "1"}),
}


def make_jobs():
    """{job: spec} for tests/readset_worker.py."""
    from abpoa_amd import synth
    jobs = {}
    for job, (shapes, stranger, env) in JOBS.items():
        sets = [synth.make_read_set(73, i, n, ln, 0.05) for i, (n, ln) in enumerate(shapes)]
        if stranger is not None:
            for i, (n, ln) in enumerate(shapes):
                sets[i][stranger] = synth.make_read_set(977, i, 1, ln, 0.0)[0]
        jobs[job] = dict(params=AFFINE, sets=sets, forms=FORMS, env=env, record=("dig", "last", "rounds_launches", "n_host_sets"), ref_record=("dig",))
    return jobs


@pytest.fixture(scope="module")
def report():
    return run_report("test_gpu_tail_final_pass", set_env={"ABPOA_HIP_CIGAR_DIGEST": "1"}, timeout=600,
                      clear_env=("ABPOA_HIP_LATE_TAIL", "ABPOA_HIP_DBG", "ABPOA_HIP_LOCKSTEP", "ABPOA_HIP_ARENA_PCT", "ABPOA_HIP_VERBOSE"))


@pytest.mark.parametrize("job", list(JOBS))
def test_three_forms_and_the_oracle(report, job):
    r = report[job]
    ref = r["ref"]
    assert all(s == 0 for s in ref["status"]) and all(d != 0 for d in ref["dig"])
    for form in FORMS:
        got = r[form]
        assert got["n_host_sets"] == 0 and got["rounds_launches"] > 0, f"{job} / {form}: the all-rounds kernel did not take the job"
        assert got["status"] == ref["status"], f"{job} / {form}: per-set status"
        assert got["dig"] == ref["dig"], f"{job} / {form}: cigar digests differ from the oracle-backed run"
        assert got["cons"] == ref["cons"], f"{job} / {form}: consensus differs from the oracle-backed run"
        assert got["cov"] == ref["cov"], f"{job} / {form}: coverage differs from the oracle-backed run"


@pytest.mark.parametrize("job", list(JOBS))
def test_result_record_of_the_last_alignment(report, job):
    """n_matched_bases, n_aln_bases, node_s / node_e, query_s / query_e (and the cigar's words, status 0) of each set's last alignment: one record in the three forms."""
    r = report[job]
    base = r["one_wavefront"]["last"]
    assert all(v is not None and v[7] == 0 and v[6] > 0 and 0 < v[0] <= v[1] for v in base), base
    for form in ("default", "late_start"):
        assert r[form]["last"] == base, f"{job} / {form}: result records differ from the one-wavefront form"
