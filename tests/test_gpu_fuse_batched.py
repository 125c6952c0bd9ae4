"""GPU (-m gpu): the fuse phase of the device-resident driver (poa_bodies.h poa_fuse_body) walks a read in super-passes of 4 x 256
positions -- four consecutive positions per thread, 256 per wavefront, every load level issued for all four before the next -- and takes the
old rows of the row order eight per thread.  What flows along the path (ids of the new nodes, the previous node, the running group-end row, the
start of a run of new nodes) is handed on inside a thread, across lanes, across wavefronts and across super-passes, so the shapes here sit on
those edges: read lengths of 1 .. 2049 bases, runs of new nodes of 6 / 300 / 1 100 bases in the middle, at the source and at the sink, aligned
groups of four (and of up to 20 residues), per-base weights, both strands, and the ways out of the phase (node slots, edge slots).
Every job runs in both forms of the driver (all-rounds kernel, ABPOA_HIP_LOCKSTEP=1) and is compared with the oracle-backed run of the host
layer (tests/cpu_shim.cpp): consensus, coverage, DP cell counts and, where asked for, the MSA rows."""
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_harness import engine  # noqa: F401  (the fixture)
from readset_worker import run_report

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AFFINE = dict(gap_open1=4, gap_open2=0, gap_ext1=2)
EDGE_LENGTHS = [255, 256, 257, 1023, 1024, 1025, 2049]      # thread / wavefront (256 positions) / super-pass (1024) edges
TINY_LENGTHS = [1, 3, 4, 5]


def _seq(rng, n, alphabet="ACGT"):
    return "".join(alphabet[i] for i in rng.integers(0, len(alphabet), n))


def _noisy(rng, s, sub=0.02, dele=0.02, ins=0.0, alphabet="ACGT"):
    out = []
    for ch in s:
        u = rng.random()
        if u < dele:
            continue
        out.append(alphabet[rng.integers(0, len(alphabet))] if u < dele + sub else ch)
        if rng.random() < ins:
            out.append(alphabet[rng.integers(0, len(alphabet))])
    return "".join(out) or s[:1]


def _subs_only(rng, s, rate=0.03, alphabet="ACGT"):
    return "".join(alphabet[rng.integers(0, len(alphabet))] if rng.random() < rate else ch for ch in s)


def _run_both_forms(monkeypatch, sets, params, what, msa=False, weights=None, amb=False):
    """Both forms of the device driver against the oracle-backed run; returns the oracle-backed results."""
    import helpers as H
    from abpoa_amd import api
    ref = api.msa_batch(sets, params, out_cons=True, out_msa=msa, n_threads=4, weights=weights, amb_strand=amb, lib=H.cpu_shim_lib())
    for lockstep in ("0", "1"):
        monkeypatch.setenv("ABPOA_HIP_LOCKSTEP", lockstep)
        dev = api.msa_batch(sets, params, out_cons=True, out_msa=msa, n_threads=4, weights=weights, amb_strand=amb)
        assert api.msa_timing()["n_host_sets"] == 0, f"{what} lockstep={lockstep}: sets left the device: {api.host_reasons()}"
        for i, (a, b) in enumerate(zip(dev, ref)):
            tag = f"{what} lockstep={lockstep}: set {i}"
            assert a.status == 0 and b.status == 0, f"{tag}: status {a.status} / {b.status}"
            assert a.cons_seq == b.cons_seq, f"{tag}: consensus differs from the oracle-backed run"
            assert a.cons_cov == b.cons_cov, f"{tag}: coverage differs"
            assert a.n_cells == b.n_cells, f"{tag}: DP cell count {a.n_cells} / {b.n_cells}"
            if msa:
                assert a.msa_len == b.msa_len and a.msa_seq == b.msa_seq, f"{tag}: MSA rows differ"
            if amb:
                assert list(a.is_rc) == list(b.is_rc), f"{tag}: strand flags differ"
    return ref


def _longest_sets(lengths, seed):
    """the read of exactly `length` bases is the longest of its set: as the first read and, substitutions only, as the third"""
    rng = np.random.default_rng(seed)
    sets = []
    for ln in lengths:
        t = _seq(rng, ln)
        sets.append([t, _noisy(rng, t), _subs_only(rng, t), _noisy(rng, t, 0.03, 0.04), _noisy(rng, t)])
        assert max(len(r) for r in sets[-1]) == ln == len(sets[-1][2])
    return sets


def _shorter_sets(lengths, seed):
    """a read of exactly `length` bases as a later, shorter read: a piece of the set's template, which the first read carries whole"""
    rng = np.random.default_rng(seed)
    sets = []
    for ln in lengths:
        full = max(ln + 60 + ln // 8, 240)
        t = _seq(rng, full)
        a = (full - ln) // 2
        piece = _subs_only(rng, t[a:a + ln], 0.03 if ln > 5 else 0.0)
        sets.append([t, _noisy(rng, t), piece, _noisy(rng, t, ins=0.01), t[a:a + ln]])
        assert len(sets[-1][2]) == ln == len(sets[-1][4]) and len(t) > ln
    return sets


@pytest.mark.parametrize("name,lengths,builder", [("longest", EDGE_LENGTHS, _longest_sets), ("shorter_to_257", TINY_LENGTHS + EDGE_LENGTHS[:3], _shorter_sets),
                                                  ("shorter_from_1023", EDGE_LENGTHS[3:], _shorter_sets)])
def test_read_lengths_at_thread_wave_and_super_pass_edges(engine, monkeypatch, name, lengths, builder):
    """Reads of exactly 1 .. 2049 bases, as the longest read of their set and as a later read shorter than the graph (reads of up to five bases: against a
    graph of 240)."""
    from abpoa_amd import api
    _run_both_forms(monkeypatch, builder(lengths, 1009), api.Params(**AFFINE), name)


def _longest_private_stretch(rows, who):
    """longest run of MSA columns in which only read `who` has a base"""
    best = cur = 0
    for col in range(len(rows[who])):
        alone = rows[who][col] != "-" and all(r[col] == "-" for j, r in enumerate(rows) if j != who)
        cur = cur + 1 if alone else 0
        best = max(best, cur)
    return best


@pytest.mark.parametrize("n_ins,at_mid,need", [(6, 253, 5), (300, 300, 257), (1100, 300, 1025)])
def test_runs_of_new_nodes_across_the_edges(engine, monkeypatch, n_ins, at_mid, need):
    """Reads that carry `n_ins` foreign bases (T, in a template of A / C / G: nothing for them to align to) in the middle -- across position 256, 512 or
    1024 of the read --, in front of the first base (previous node = source) and behind the last (last node -> sink); the fourth read of five carries
    them.  Unbanded, they are aligned as one insertion: a run of new nodes with one anchor row, ids in path order.  The oracle-backed MSA must show it."""
    from abpoa_amd import api
    rng = np.random.default_rng(77 + n_ins)
    sets, who = [], 3
    for place in ("middle", "start", "end", "middle"):
        t = _seq(rng, 600, "ACG")
        at = {"middle": at_mid, "start": 0, "end": len(t)}[place]
        reads = [t, _noisy(rng, t, alphabet="ACG"), _noisy(rng, t, alphabet="ACG"), t[:at] + "T" * n_ins + t[at:], _noisy(rng, t, alphabet="ACG")]
        sets.append(reads)
    for kw in (dict(AFFINE, extra_b=-1), dict(extra_b=-1), dict(AFFINE), dict()):
        ref = _run_both_forms(monkeypatch, sets, api.Params(**kw), f"insertion of {n_ins} {kw}", msa=True)
        if kw.get("extra_b") == -1:
            for i, r in enumerate(ref):
                got = _longest_private_stretch(r.msa_seq[:5], who)
                assert got >= need, f"insertion of {n_ins}, set {i}, {kw}: the oracle-backed MSA has only {got} columns of read {who} alone"


def test_aligned_groups_of_four(engine, monkeypatch):
    """Four reads with four different bases at the same 20 positions: every such column becomes an aligned group of four nodes; later reads find their base
    as the aligned node itself or as the first / second / third member of its group.  MSA rows (read-id bitsets of the edges) included."""
    from abpoa_amd import api
    rng = np.random.default_rng(4242)
    sets = []
    for s in range(5):
        t = _seq(rng, 300 + 7 * s)
        pos = set(int(x) for x in rng.choice(np.arange(5, len(t) - 5), 20, replace=False))
        four = ["".join("ACGT"[("ACGT".index(ch) + k) % 4] if i in pos else ch for i, ch in enumerate(t)) for k in range(4)]
        sets.append(four + [four[2], _noisy(rng, four[3]), four[1], _noisy(rng, four[0])])
    for kw in (AFFINE, dict()):
        ref = _run_both_forms(monkeypatch, sets, api.Params(**kw), f"groups of four {kw}", msa=True)
        for i, r in enumerate(ref):      # reached: at least 20 columns in which the first four reads show four different bases
            rows = r.msa_seq[:4]
            n4 = sum(1 for col in range(len(rows[0])) if len({x[col] for x in rows} - {"-"}) == 4)
            assert n4 >= 20, f"set {i} {kw}: only {n4} columns with four different bases in the oracle-backed MSA"


def test_amino_acid_groups_with_msa_rows(engine, monkeypatch):
    """27-code alphabet, BLOSUM62, 15 % substitutions: aligned groups beyond the three members whose loads are batched; local convex as the cfg5 workload, and
    global convex so that the all-rounds kernel runs them too."""
    from abpoa_amd import api, synth, workloads
    sets = [synth.make_read_set(83, i, 10, 140 + 30 * i, alphabet=synth.AA, rates=(0.15, 0.01, 0.01)) for i in range(6)]
    for kw in (dict(aln_mode=1), dict()):
        ref = _run_both_forms(monkeypatch, sets, api.Params(is_aa=True, score_matrix=workloads.BLOSUM62, **kw), f"amino acids {kw}", msa=True)
        deep = max(len({x[col] for x in r.msa_seq[:10]} - {"-"}) for r in ref for col in range(r.msa_len))
        assert deep >= 5, f"{kw}: no MSA column with five or more different residues ({deep})"


@pytest.mark.parametrize("amb", [False, True], ids=["forward_only", "strand_retry"])
def test_per_base_weights(engine, monkeypatch, amb):
    """-Q: an edge takes the weight of the base it leads to, the sink edge the last base's; with -s the reverse complement of a read (and its reversed
    weights) goes into the graph."""
    from abpoa_amd import api, synth
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    rng = np.random.default_rng(31)
    sets = [list(synth.make_read_set(89, i, 7, 250 + 260 * i, 0.08)) for i in range(4)]      # 250 .. 1030 bases: the last set crosses a super-pass
    if amb:
        sets = [[("".join(comp[c] for c in reversed(r)) if j in (2, 5) else r) for j, r in enumerate(s)] for s in sets]
    weights = [[rng.integers(1, 41, len(r)).astype(np.int32) for r in s] for s in sets]
    ref = _run_both_forms(monkeypatch, sets, api.Params(**AFFINE), f"weights amb={amb}", msa=True, weights=weights, amb=amb)
    if amb:
        assert sum(sum(r.is_rc) for r in ref) >= 6, "the inputs were meant to have reverse-complemented reads"


_CHILD_HEAD = ("import os, sys, ctypes; sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))\n"
               "import numpy as np\n"
               "import helpers as H\n"
               "from abpoa_amd import api, ffi, synth, seqio\n"
               "lib = ffi.lib(); ffi.check(lib.abpoa_hip_init(0))\n" % (ROOT, ROOT))


def test_node_slots_run_out_inside_the_fuse_phase():
    """Six sets of 20 amino-acid reads x 600 residues at 30 % substitutions (BLOSUM62, global convex) outgrow the 3x node slots of the first pass while a read
    is being fused -- 20 reads are too few for the growth projection of the prepare phase -- and are redone with 4.5x and 6x: nothing leaves the device, results
    equal to the oracle-backed run, in both forms of the driver.  Counted from the oracle-backed MSA (one node per column and residue): 2 600 nodes after 10 reads,
    3 450 after 15, 4 250 at the end, against 3 x 630 + 1024 = 2 900 slots in the first pass, 3 830 in the second, 4 760 in the third.
    (Nucleotide sets of this size do not get there -- 12 or 20 reads x 600 bases at 30 % error, the recipe of test_job_shape_hint_skips_the_doomed_pass made
    smaller, nor 30 % insertions, nor 200 random bases of its own in every read: a column holds four nodes at most and the slots are 3 x the longest read + 1024;
    measured for all three: "0 sets outgrew a device capacity".  Twenty residues per column do not saturate.)
    Child process: the passes are reported on stderr; ABPOA_HIP_NO_PASS_HINT lets the second job start at 3x again."""
    code = (_CHILD_HEAD +
            "from abpoa_amd import workloads\n"
            "sets = [synth.make_read_set(5, i, 20, 600, alphabet=synth.AA, rates=(0.30, 0.03, 0.05)) for i in range(6)]\n"
            "p = api.Params(is_aa=True, score_matrix=workloads.BLOSUM62)\n"
            "ref = api.msa_batch(sets, p, n_threads=4, lib=H.cpu_shim_lib())\n"
            "for form in ('0', '1'):\n"
            "    os.environ['ABPOA_HIP_LOCKSTEP'] = form\n"
            "    sys.stderr.write('FORM %s\\n' % form); sys.stderr.flush()\n"
            "    dev = api.msa_batch(sets, p, n_threads=4)\n"
            "    assert api.msa_timing()['n_host_sets'] == 0, api.host_reasons()\n"
            "    assert all(a.status == 0 and a.cons_seq == b.cons_seq and a.cons_cov == b.cons_cov and a.n_cells == b.n_cells for a, b in zip(dev, ref)), form\n"
            "print('OK')\n")
    env = dict(os.environ, ABPOA_HIP_VERBOSE="1", ABPOA_HIP_HOSTGRAPH="0", ABPOA_HIP_NO_PASS_HINT="1")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "OK" in p.stdout, (p.stdout[-500:], p.stderr[-3000:])
    forms = p.stderr.split("FORM ")[1:]
    assert len(forms) == 2
    for f in forms:
        assert "pass 1, node slots 3x" in f and "pass 2, node slots 4.5x" in f, f[-2500:]
        first = [ln for ln in f.splitlines() if "fallback reasons:" in ln][0]
        n_fuse = int(first.split("node slots in the fuse phase ")[1].split(",")[0])
        assert n_fuse > 0, first


def test_edge_slots_run_out_inside_the_fuse_phase(engine, monkeypatch):
    """The job of test_gpu_device_general.py::test_inner_nodes_with_more_edges_than_the_edge_slots: one node collects 26 out-edges (in-edges), more than the
    16 (15) slots of the regular passes; the pass that finds the list full sends the set to the last pass of the ladder.  Same results, and the same histogram
    of sets handed to the host driver as before the super-passes: none."""
    from abpoa_amd import api, synth
    base = synth.make_read_set(211, 0, 1, 420, 0.0)[0]
    fan_out = [base] + [base[:200] + base[200 + k:] for k in range(1, 26)]
    fan_in = [base] + [base[:200 - k] + base[200:] for k in range(1, 26)]
    sets = [fan_out, fan_in, fan_out + fan_in[1:], list(synth.make_read_set(211, 1, 12, 300, 0.05))]
    expected_host_reasons = {}
    for kw in (AFFINE, dict()):
        _run_both_forms(monkeypatch, sets, api.Params(**kw), f"fan of edges {kw}", msa=True)
        assert api.host_reasons() == expected_host_reasons, (kw, api.host_reasons())


def make_jobs():
    """{job: spec} for tests/readset_worker.py: reads around a super-pass, in the form the child's own environment selects."""
    from abpoa_amd import synth
    sets = [synth.make_read_set(29, i, 6, 1000 + 12 * i, 0.06) for i in range(5)]
    return {"super_pass": dict(params=AFFINE, sets=sets, forms={"device": {}}, record=("dig", "rounds_launches", "n_host_sets"), ref_record=("dig",), ref_threads=8)}


@pytest.mark.parametrize("lockstep", ["0", "1"], ids=["all_rounds_kernel", "lockstep_rounds"])
def test_cigars_of_reads_around_a_super_pass(lockstep):
    """ABPOA_HIP_CIGAR_DIGEST=1 (as test_gpu_device_msa.py::test_device_driver_cigars_equal_the_oracle_backed_run): the fuse phase folds every graph cigar
    into a digest per read-set before it walks it; reads of 990 - 1060 bases, equal digests = equal cigars, word for word."""
    rep = run_report("test_gpu_fuse_batched", set_env={"ABPOA_HIP_CIGAR_DIGEST": "1", "ABPOA_HIP_LOCKSTEP": lockstep}, clear_env=(), timeout=300)["super_pass"]
    dev, ref = rep["device"], rep["ref"]
    assert all(s == 0 for s in dev["status"]) and dev["n_host_sets"] == 0, dev
    assert all(d != 0 for d in dev["dig"]) and dev["dig"] == ref["dig"], (dev["dig"], ref["dig"])
    assert dev["cons"] == ref["cons"] and dev["cov"] == ref["cov"]
    assert (dev["rounds_launches"] != 0) == (lockstep == "0"), dev["rounds_launches"]
def test_device_graph_node_by_node_after_every_read():
    """ABPOA_HIP_DEVSYNC=1 ABPOA_HIP_HOSTGRAPH=0 (child process): after every read the library compares the device graph with the host graph node by node --
    bases, edge lists in slot order, weights, aligned groups, read counts -- and the row order.  Reads of 257 / 1024 / 1025 bases, a 300-base insertion,
    groups of four."""
    code = (_CHILD_HEAD +
            "rng = np.random.default_rng(5)\n"
            "sq = lambda n, al='ACGT': ''.join(al[i] for i in rng.integers(0, len(al), n))\n"
            "sets = [list(synth.make_read_set(3, i, 6, ln, 0.08)) for i, ln in enumerate((257, 1024, 1025))]\n"
            "t = sq(600, 'ACG'); sets.append([t, t[:100] + t[104:], t[:300] + 'T' * 300 + t[300:], t[:500] + 'A' + t[500:], t])\n"
            "t = sq(320); four = [''.join('ACGT'[('ACGT'.index(c) + k) % 4] if i % 16 == 5 else c for i, c in enumerate(t)) for k in range(4)]\n"
            "sets.append(four + [four[3], four[1]])\n"
            "r = api.msa_batch(sets, api.Params(gap_open1=4, gap_open2=0, gap_ext1=2), n_threads=4)\n"
            "print('OK', all(x.status == 0 for x in r), api.msa_timing()['n_host_sets'])\n")
    env = dict(os.environ, ABPOA_HIP_DEVSYNC="1", ABPOA_HIP_HOSTGRAPH="0")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "OK True 0" in p.stdout, (p.stdout, p.stderr[-2000:])
    assert "graph check ok" in p.stderr and "consensus check ok" in p.stderr and "FAILED" not in p.stderr, p.stderr[-3000:]
