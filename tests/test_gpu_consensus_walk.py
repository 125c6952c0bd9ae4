"""GPU (-m gpu): the consensus kernel (abpoa_amd/csrc/poa_device.hip, poa_consensus_kernel) at the shapes where its three parts can go wrong -- the loads
that run three 64-row blocks ahead, the pointer jumping over rows with one heaviest edge, and the path walk that emits a block's rows lane-parallel.

Every set is compared with the CPU build of the host layer whose aligner is the plain-C oracle (tests/cpu_shim.cpp): status, consensus, per-base coverage.
Every job also runs under ABPOA_HIP_DEVSYNC=1, where the library recomputes the consensus of a job's first four sets on the host from the downloaded graph
(DeviceDebug::consensus_check) -- so no job has more than four sets.  ONE child process (tests/readset_worker.py) runs every job of make_jobs() in both forms
and reports."""
import numpy as np
import pytest

from readset_worker import run_report

pytestmark = pytest.mark.gpu

AFFINE = dict(gap_open1=4, gap_open2=0, gap_ext1=2)
NT = "ACGT"


def _template(rng, n, alphabet=NT):
    return "".join(alphabet[i] for i in rng.integers(0, len(alphabet), n))


def _deleted(rng, s, rate):
    """s without a few of its bases: no read adds a node, so the graph keeps the first read's row count"""
    keep = rng.random(len(s)) >= rate
    keep[0] = keep[-1] = True
    return "".join(c for c, k in zip(s, keep) if k)


def _substituted(rng, s, rate, alphabet=NT):
    out = list(s)
    for i in np.flatnonzero(rng.random(len(s)) < rate):
        out[i] = alphabet[(alphabet.index(out[i]) + 1 + int(rng.integers(0, len(alphabet) - 1))) % len(alphabet)]
    return "".join(out)


def _chain_sets(lengths, seed):
    """first read of L bases, four more that only lack bases: graphs of exactly L + 2 rows"""
    rng = np.random.default_rng(seed)
    sets = []
    for ln in lengths:
        t = _template(rng, ln)
        sets.append([t] + [_deleted(rng, t, 0.06) for _ in range(4)])
    return sets


def _skip_sets(seed):
    """3 of 5 reads lack a stretch: the heaviest path leaves the backbone and comes back 70 / 150 rows later, from the middle of a block and from its last rows"""
    rng = np.random.default_rng(seed)
    sets = []
    for start, gap in ((150, 70), (150, 150), (61, 70), (60, 150)):
        t = _template(rng, 400)
        short = t[:start] + t[start + gap:]
        sets.append([t, _substituted(rng, short, 0.01), _substituted(rng, t, 0.01), _substituted(rng, short, 0.01), _substituted(rng, short, 0.01)])
    return sets


def _ragged_set(seed, n_reads, span):
    """reads that start and end at different places of one template: the source gets an out-edge and the sink an in-edge per distinct end"""
    rng = np.random.default_rng(seed)
    t = _template(rng, 300)
    return [t] + [_substituted(rng, t[7 * i + 3:len(t) - (span - 7 * i)], 0.01) for i in range(1, n_reads)]


FORMS = {"default": {}, "devsync": {"ABPOA_HIP_DEVSYNC": "1", "ABPOA_HIP_HOSTGRAPH": "0"}}


def make_jobs():
    """{job: spec} for tests/readset_worker.py."""
    from abpoa_amd import synth, workloads
    rng = np.random.default_rng(16)
    table = {
        # graphs of 63, 64, 65 and of 127, 128, 129 rows: the sink is the last row of a block, the first of the next, and one further
        "rows_63_65": (AFFINE, _chain_sets((61, 62, 63), 1)),
        "rows_127_129": (AFFINE, _chain_sets((125, 126, 127), 2)),
        "skip_blocks": (AFFINE, _skip_sets(3)),
        # two reads: every edge weight is 1 wherever they differ, and the tie rules decide each step (last edge; for the source the first)
        "ties": (AFFINE, [synth.make_read_set(71, i, 2, ln, 0.15) for i, ln in enumerate((40, 70, 130, 200))]),
        "ties_convex": ({}, [synth.make_read_set(73, i, 2, ln, 0.2) for i, ln in enumerate((63, 64, 129, 260))]),
        "ragged": (AFFINE, [_ragged_set(4, 6, 60), _ragged_set(5, 14, 110)]),
        "protein": (dict(is_aa=True, score_matrix=workloads.BLOSUM62), [synth.make_read_set(75, i, 6, 90 + 45 * i, alphabet=synth.AA, rates=(0.06, 0.03, 0.03)) for i in range(3)]),
        "degenerate": (AFFINE, [[_template(rng, 150)], [], synth.make_read_set(77, 0, 5, 100, 0.05), [_template(rng, 1)]]),
    }
    return {job: dict(params=kw, sets=sets, forms=FORMS, record=("n_host_sets",), ref_record=("msa",)) for job, (kw, sets) in table.items()}


@pytest.fixture(scope="module")
def report():
    """(the report, {(job, form): what the library said on stderr during that run})"""
    return run_report("test_gpu_consensus_walk", set_env={}, timeout=600, want_log=True,
                      clear_env=("ABPOA_HIP_DEVSYNC", "ABPOA_HIP_HOSTGRAPH", "ABPOA_HIP_LOCKSTEP", "ABPOA_HIP_DBG"))


JOBS = ["rows_63_65", "rows_127_129", "skip_blocks", "ties", "ties_convex", "ragged", "protein", "degenerate"]


def test_the_job_list_is_the_workers():
    assert list(make_jobs()) == JOBS


@pytest.mark.parametrize("job", JOBS)
def test_consensus_equals_the_oracle_backed_run(report, job):
    rep, log = report
    r = rep[job]
    ref = r["ref"]
    assert all(s == 0 for s in ref["status"])
    for form in ("default", "devsync"):
        got = r[form]
        assert got["n_host_sets"] == 0, f"{job} / {form}: sets on the host driver"
        assert got["status"] == ref["status"], f"{job} / {form}: per-set status"
        assert got["cons"] == ref["cons"], f"{job} / {form}: consensus differs from the oracle-backed run"
        assert got["cov"] == ref["cov"], f"{job} / {form}: coverage differs from the oracle-backed run"


@pytest.mark.parametrize("job", JOBS)
def test_host_recomputation_from_the_device_graph(report, job):
    """ABPOA_HIP_DEVSYNC=1: node ids, bases and coverage of every set's consensus equal the host routine's on the downloaded graph"""
    rep, log = report
    text = log[(job, "devsync")]
    n_sets = len(rep[job]["ref"]["status"])
    assert "FAILED" not in text, text[-3000:]
    assert text.count("consensus check ok") == n_sets, text[-3000:]


def test_the_sets_are_what_they_are_meant_to_be(report):
    """from the oracle-backed run alone: the chain graphs have the row counts aimed at, the heaviest path does skip the stretch, the ragged reads do start apart"""
    rep, log = report
    jobs = make_jobs()
    for job, lengths in (("rows_63_65", (61, 62, 63)), ("rows_127_129", (125, 126, 127))):
        for msa, ln in zip(rep[job]["ref"]["msa"], lengths):
            assert len(msa[0]) == ln, f"{job}: a read added a node ({len(msa[0])} columns for a first read of {ln})"
    for cons, reads, gap in zip(rep["skip_blocks"]["ref"]["cons"], jobs["skip_blocks"]["sets"], (70, 150, 70, 150)):
        assert len(cons) == len(reads[0]) - gap
    for msa, reads in zip(rep["ragged"]["ref"]["msa"], jobs["ragged"]["sets"]):
        starts = {next(i for i, c in enumerate(row) if c != "-") for row in msa[:len(reads)]}
        assert len(starts) >= 5, "the source needs more than four out-edges of weight 1"
    deg = rep["degenerate"]["ref"]["cons"]
    assert deg[0] == jobs["degenerate"]["sets"][0][0] and deg[1] == "" and len(deg[3]) == 1
