"""GPU (-m gpu): the tables the prepare phase writes for the DP (abpoa_amd/csrc/poa_bodies.h, poa_prepare_body): row_base, row_node_id, the remaining length of
the adaptive band (pointer jumping over all rows in LDS; the reverse sweep in global memory for graphs beyond the LDS records), pred_off / pred_row in in_id
order, row_pd, row_sdist and, for general-kernel jobs, out_off / out_row.

A wrong remaining length only moves a band, a wrong row_sdist only changes which rows keep their records, and the order of a predecessor list only breaks ties:
none has to change a consensus, so the tables themselves are checked.  Under ABPOA_HIP_DEVSYNC=1 the library downloads them after every prepare launch and
compares them with a plain serial recomputation from the host graph (DeviceDebug::prepare_check; the first four sets of a job, so no job here has more).  The same jobs also run in the default form (the all-rounds kernel where it applies) and with ABPOA_HIP_LOCKSTEP=1 against the
CPU build of the host layer whose aligner is the plain-C oracle: status, cigar digests (every graph cigar of a set folded into 64 bits), consensus, coverage.  ONE child process
(tests/readset_worker.py) runs every job of make_jobs() in every form and reports."""
import re

import numpy as np
import pytest

from readset_worker import run_report

pytestmark = pytest.mark.gpu

AFFINE = dict(gap_open1=4, gap_open2=0, gap_ext1=2)


def _grow(seed, lengths, n_reads=5):
    """sets whose first read has the given length; 5 % errors add a few rows per read, so the graphs start at and grow across the edges aimed at"""
    from abpoa_amd import synth
    return [synth.make_read_set(seed, i, n_reads, ln, 0.05) for i, ln in enumerate(lengths)]


def _template(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


DEGREES = (5, 9, 12)      # in-degree of one node and out-degree of another in the hand-made sets: cold slots (> POA_HOT = 4), and more predecessors than row_pd's eight


def _degree_set(seed, degree):
    """Two copies of a template and reads that lack 1 .. degree - 1 bases in front of base 80 (every deletion ends at the same base: that node collects
    `degree` in-edges) and 1 .. degree - 1 bases behind base 30 (that node collects `degree` out-edges).  Bases 30 and 80 are the only A within 14 bases of
    themselves and no two neighbouring bases are equal, so every deletion has one place to go."""
    rng = np.random.default_rng(seed)
    t = []
    while len(t) < 120:
        i = len(t)
        c = 0 if i in (30, 80) else int(rng.integers(1, 4) if min(abs(i - 30), abs(i - 80)) <= 14 else rng.integers(0, 4))
        if i in (30, 80) or ((not t or c != t[-1]) and (len(t) < 2 or c != t[-2])):
            t.append(c)
    t = "".join("ACGT"[c] for c in t)
    return [t, t] + [t[:80 - k] + t[80:] for k in range(1, degree)] + [t[:31] + t[31 + k:] for k in range(1, degree)]


def _ragged_set(seed, n_reads):
    """reads that start and end at different places of one template: the source gets an out-edge and the sink an in-edge per distinct end (terminal pools)"""
    rng = np.random.default_rng(seed)
    t = _template(rng, 400)
    return [t] + [t[7 * i + 3:len(t) - 5 * (n_reads - i)] for i in range(1, n_reads)]


def degrees_from_msa(msa, n_reads):
    """largest in-degree and out-degree of a node of the graph whose row-column MSA this is: a node is (column, base), an edge joins a read's neighbouring bases"""
    ins, outs = {}, {}
    for row in msa[:n_reads]:
        cells = [(c, b) for c, b in enumerate(row) if b != "-"]
        for a, b in zip(cells, cells[1:]):
            outs.setdefault(a, set()).add(b); ins.setdefault(b, set()).add(a)
    return max(len(v) for v in ins.values()), max(len(v) for v in outs.values())


FORMS = {"default": {}, "lockstep": {"ABPOA_HIP_LOCKSTEP": "1"}, "devsync": {"ABPOA_HIP_DEVSYNC": "1", "ABPOA_HIP_HOSTGRAPH": "0"}}


def make_jobs():
    """{job: spec} for tests/readset_worker.py."""
    from abpoa_amd import synth
    table = {
        # rows = first read + 2, then more: the 64-row edge of a lane's records, the 256-row edge of a thread's next row, the 1 024- and 2 048-row edges that
        # four and eight rows of a thread lie across
        "tiny": (AFFINE, [synth.make_read_set(31, i, 4, ln, 0.0) for i, ln in enumerate((1, 2, 3))]),
        "edge_64": (AFFINE, _grow(32, (60, 61, 62, 63))),
        "edge_256": (AFFINE, _grow(33, (253, 254, 255))),
        "edge_1024": (AFFINE, _grow(34, (1021, 1022, 1023), 4)),
        "edge_2048": (AFFINE, _grow(35, (2045, 2046, 2047), 4)),
        "convex_2048": ({}, _grow(36, (2000,), 6)),
        # more rows than the LDS records of a small job hold
        "long_2700": (AFFINE, [synth.make_read_set(37, 0, 3, 2700, 0.05)]),
        # cold slots, predecessors beyond the eight of row_pd
        "degrees": (AFFINE, [_degree_set(41 + d, d) for d in DEGREES]),
        # the terminal pools of source and sink (more ends than edge slots of a node)
        "ragged_20": (AFFINE, [_ragged_set(45, 20)]),
        # unbanded, the reference's row order rebuilt before every read
        "local": (dict(aln_mode=1), [synth.make_read_set(46, i, 6, 150 + 40 * i, 0.06) for i in range(3)]),
        # linear gaps without a band: the general kernel, which reads the successor lists
        "general": (dict(gap_open1=0, gap_open2=0, gap_ext1=2, extra_b=-1), [synth.make_read_set(47, i, 6, 120 + 70 * i, 0.06) for i in range(3)]),
        # linear gaps with the band: no direction words, so the DP does not read row_sdist
        "linear": (dict(gap_open1=0, gap_open2=0, gap_ext1=2), [synth.make_read_set(48, i, 6, 300, 0.05) for i in range(2)]),
    }
    return {job: dict(params=kw, sets=sets, forms=FORMS, record=("dig", "n_host_sets"), ref_record=("dig", "msa")) for job, (kw, sets) in table.items()}


@pytest.fixture(scope="module")
def report():
    """(the report, {(job, form): what the library said on stderr during that run})"""
    return run_report("test_gpu_prepare_tables", set_env={"ABPOA_HIP_CIGAR_DIGEST": "1"}, timeout=600, want_log=True,
                      clear_env=("ABPOA_HIP_DEVSYNC", "ABPOA_HIP_HOSTGRAPH", "ABPOA_HIP_LOCKSTEP", "ABPOA_HIP_DBG"))


JOBS = ["tiny", "edge_64", "edge_256", "edge_1024", "edge_2048", "convex_2048", "long_2700", "degrees", "ragged_20", "local", "general", "linear"]


def test_the_job_list_is_the_workers():
    assert list(make_jobs()) == JOBS


@pytest.mark.parametrize("job", JOBS)
def test_tables_equal_the_host_recomputation(report, job):
    """one "prepare check ok" per set and round with something to align, no difference anywhere"""
    rep, log = report
    text = log[(job, "devsync")]
    assert "FAILED" not in text, "\n".join(ln for ln in text.splitlines() if "FAILED" in ln or "remaining length" in ln)[:3000]
    checks = re.findall(r"set (\d+) round (\d+): prepare check ok \((\d+) rows, 0 differences\)", text)
    assert len(checks) == sum(len(s) - 1 for s in make_jobs()[job]["sets"]), text[-2000:]


def test_the_graphs_cross_the_edges_aimed_at(report):
    rep, log = report
    def rows(job):
        return [int(n) for _, _, n in re.findall(r"set (\d+) round (\d+): prepare check ok \((\d+) rows", log[(job, "devsync")])]
    for job, edge in (("edge_64", 64), ("edge_256", 256), ("edge_1024", 1024), ("edge_2048", 2048), ("convex_2048", 2048)):
        r = rows(job)
        assert min(r) <= edge < max(r), (job, min(r), max(r))
    assert min(rows("long_2700")) > 2600


def test_the_jobs_take_the_paths_they_are_about(report):
    """the successor lists are written and checked in the general-kernel job only; the hand-made sets have the degrees they are meant to have and the ragged reads
    more distinct ends than a node has edge slots (from the oracle-backed run's MSA alone)"""
    rep, log = report
    for job in JOBS:
        assert ("successor rows too" in log[(job, "devsync")]) == (job == "general"), job
    for msa, reads, d in zip(rep["degrees"]["ref"]["msa"], make_jobs()["degrees"]["sets"], DEGREES):
        assert degrees_from_msa(msa, len(reads)) == (d, d)
    msa = rep["ragged_20"]["ref"]["msa"][0]
    starts = {next(i for i, c in enumerate(row) if c != "-") for row in msa[:20]}
    ends = {max(i for i, c in enumerate(row) if c != "-") for row in msa[:20]}
    assert len(starts) == 20 and len(ends) == 20


@pytest.mark.parametrize("job", JOBS)
def test_results_equal_the_oracle_backed_run(report, job):
    rep, log = report
    r = rep[job]
    ref = r["ref"]
    assert all(s == 0 for s in ref["status"])
    for form in FORMS:
        got = r[form]
        assert got["n_host_sets"] == 0, f"{job} / {form}: sets on the host driver"
        assert (got["status"], got["cons"], got["cov"]) == (ref["status"], ref["cons"], ref["cov"]), f"{job} / {form}: differs from the oracle-backed run"
        assert got["dig"] == ref["dig"] and all(d != 0 for d in ref["dig"]), f"{job} / {form}: cigar digests differ from the oracle-backed run"
