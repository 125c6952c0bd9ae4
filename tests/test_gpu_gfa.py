"""GFA output of the device-resident driver (poa_gfa.hip: poa_gfa_walk_kernel, poa_gfa_fill_kernel; ABPOA_HIP_OUT_GFA): the record a job brings back from the
graphs in HBM against the host layer's (PoaGraph::gfa through the oracle-backed CPU build), array for array and text for text, and against the reference's
recorded output (tests/golden/gfa/).  n_host_sets == 0 wherever the device path is the subject."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import gfa_cases as GC
import helpers as H
from gpu_harness import engine  # noqa: F401

pytestmark = pytest.mark.gpu
D = H.GOLDEN_DIR


def _same(dev, ref, what, names=None, out_cons=False, device_only=True):
    from abpoa_amd import api
    if device_only:
        assert api.msa_timing()["n_host_sets"] == 0, f"{what}: device driver not used for every set"
    assert len(dev) == len(ref)
    for i, (a, b) in enumerate(zip(dev, ref)):
        assert a.status == 0 and b.status == 0, (what, i, a.status, b.status)
        GC.same_record(a.gfa, b.gfa, f"{what}: set {i}")
        assert a.is_rc == b.is_rc, (what, i)
        assert a.cons_seq == b.cons_seq and (out_cons or a.cons_len == 0), (what, i)
        assert api.format_gfa(a, names, out_cons) == api.format_gfa(b, names, out_cons), (what, i)


def _both(sets, p, what, out_cons=True, device_only=True, **kw):
    from abpoa_amd import api
    dev = api.msa_batch(sets, p, out_cons=out_cons, out_gfa=True, n_threads=4, **kw)
    tm = api.msa_timing()
    ref = api.msa_batch(sets, p, out_cons=out_cons, out_gfa=True, n_threads=4, lib=H.cpu_shim_lib(), **kw)
    if device_only:
        assert tm["n_host_sets"] == 0, f"{what}: device driver not used for every set"
    _same(dev, ref, what, out_cons=out_cons, device_only=False)
    return dev, ref


@pytest.mark.parametrize("lockstep", [0, 1])
@pytest.mark.parametrize("out_cons", [False, True])
def test_global_gfa_on_the_device(engine, monkeypatch, lockstep, out_cons):
    """Nucleotide reads, global banded alignment, affine and convex gaps, through the all-rounds kernel and the lock-step launches: 3-40 reads of 120-800 bases
    at 2-18 % errors, and sets of 64, 65 and 70 reads (the last bit of word 0 of the read ids, the first of word 1, two words)."""
    from abpoa_amd import api, synth
    monkeypatch.setenv("ABPOA_HIP_LOCKSTEP", str(lockstep))
    for kw, shapes in ((dict(gap_open1=4, gap_open2=0, gap_ext1=2), [(3 + (5 * i) % 38, 120 + 61 * i, 0.02 + 0.02 * (i % 8)) for i in range(12)] + [(64, 131, 0.06), (65, 150, 0.08), (70, 143, 0.08)]),
                       (dict(), [(6 + i, 300 + 90 * i, 0.12) for i in range(6)] + [(65, 139, 0.10)])):
        sets = [synth.make_read_set(31, i, n, ln, err) for i, (n, ln, err) in enumerate(shapes)]
        dev, _ = _both(sets, api.Params(**kw), f"{kw} lockstep={lockstep} out_cons={out_cons}", out_cons=out_cons)
        assert any(r.gfa.n_seg % 64 for r in dev)


def test_protein_and_local_gfa_on_the_device(engine):
    """Protein global with BLOSUM62; nucleotide and protein local (the jobs whose row order is rebuilt before every read)."""
    from abpoa_amd import api, synth, workloads
    aa = [synth.make_read_set(37, i, 12 + i % 9, 150 + 40 * i, alphabet=synth.AA, rates=(0.10 + 0.02 * (i % 4), 0.02, 0.02)) for i in range(6)]
    nt = [synth.make_read_set(41, i, 5 + 2 * i, 140 + 50 * i, 0.08) for i in range(6)]
    _both(aa, api.Params(is_aa=True, score_matrix=workloads.BLOSUM62), "protein global")
    _both(aa, api.Params(aln_mode=api.LOCAL, is_aa=True, score_matrix=workloads.BLOSUM62), "protein local")
    _both(nt, api.Params(aln_mode=api.LOCAL), "nucleotide local", out_cons=False)


def _ragged_set(seed, n=28, tlen=600):
    from abpoa_amd import synth
    rng = np.random.default_rng(seed)
    reads = []
    for r in synth.make_read_set(71, seed, n, tlen, 0.06):
        a, b = int(rng.integers(0, tlen // 2 - 60)), int(rng.integers(tlen // 2 + 60, len(r)))
        reads.append(r[a:b])
    return reads


@pytest.mark.parametrize("mode", [0, 2])
def test_ragged_reads_spill_into_the_terminal_pools(engine, mode):
    """28 reads, each a random substring of a noisy 600-base template, global and extension mode: the source has more out-edges than an inner node has slots
    (POA_OUT_CAP 16) and the sink more in-edges (POA_IN_CAP 15), both reached through the terminal pools -- asserted from the host layer's record."""
    from abpoa_amd import api
    sets = [_ragged_set(2), _ragged_set(5, 24)]
    _, ref = _both(sets, api.Params(aln_mode=mode), f"ragged mode {mode}")
    g = ref[0].gfa
    first = {int(g.path_node[g.path_off[i]]) for i in range(g.n_path)}
    last = {int(g.path_node[g.path_off[i + 1] - 1]) for i in range(g.n_path)}
    assert len(first) > 16 and len(last) > 15, (len(first), len(last))


def test_ambiguous_strand_paths(engine):
    """-s: reads that went into the graph as their reverse complement (is_rc; the formatter reverses their paths)."""
    from abpoa_amd import api, seqio, synth
    _, rc_reads, _ = seqio.read_fastx(os.path.join(D, "out_rc_cons", "input.fa"))
    comp = str.maketrans("ACGT", "TGCA")
    long_set = [r if i % 3 else r.translate(comp)[::-1] for i, r in enumerate(synth.make_read_set(43, 0, 8, 2500, 0.08))]
    dev, _ = _both([rc_reads, long_set], api.Params(), "-s", amb_strand=True)
    assert any(dev[0].is_rc) and any(dev[1].is_rc)


@pytest.mark.parametrize("name", ["heter_p_r4", "synth12x400_p_r4", "test_p_r4"])
def test_guide_order_against_the_reference(engine, name, tmp_path):
    """-p (the CPU build has no guide order): the text against the reference's; P line i is input read i."""
    from abpoa_amd import api, cli
    case = GC.CASES[name]
    out = io.StringIO()
    assert cli.main(GC.front_end_args(case, GC.case_input(case, tmp_path)), out=out) == 0
    assert api.msa_timing()["n_host_sets"] == 0
    GC.assert_matches(case, out.getvalue(), "cli.main -p on the device")


def _variant_sets():
    from abpoa_amd import synth
    return [synth.make_read_set(47, i, 6 + 3 * i, 200 + 130 * i, 0.04 + 0.03 * i) for i in range(5)]


@pytest.mark.parametrize("env,device_only", [({"ABPOA_HIP_FIRST_PASS": "3"}, True), ({"ABPOA_HIP_ORDER_LDS": "0"}, True), ({"ABPOA_HIP_ORDER_CAP": "600"}, True),
                                             ({"ABPOA_HIP_HOSTGRAPH": "1"}, False)])
def test_driver_variants(engine, monkeypatch, env, device_only):
    """The last pass of the ladder (other edge-slot counts, no direction words); the walk's tables in memory for every graph, and for the larger graphs of the
    job only; the host driver with the HIP aligner (PoaGraph::gfa)."""
    from abpoa_amd import api
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _both(_variant_sets(), api.Params(), str(env), device_only=device_only)
    if not device_only:
        assert api.msa_timing()["n_host_sets"] == 5


def test_both_sides_of_the_walk_lds_capacity(engine):
    """16 x 3 kb reads at 15 % errors: more than the 6000 nodes whose counters and queue the walk keeps in LDS; 12 x 1 kb reads stay below."""
    from abpoa_amd import api, synth
    sets = [synth.make_read_set(59, 0, 16, 3000, 0.15), synth.make_read_set(59, 1, 12, 1000, 0.05)]
    dev, _ = _both(sets, api.Params(), "walk tables in memory / in LDS")
    assert dev[0].gfa.n_seg > 6000 > dev[1].gfa.n_seg


@pytest.mark.parametrize("name", ["test_r3", "test_r4", "seq_affine_r4", "s1k_affine_r4"])
def test_reference_texts_through_the_device(engine, name, tmp_path):
    from abpoa_amd import api, cli
    case = GC.CASES[name]
    out = io.StringIO()
    assert cli.main(GC.front_end_args(case, GC.case_input(case, tmp_path)), out=out) == 0
    assert api.msa_timing()["n_host_sets"] == 0
    GC.assert_matches(case, out.getvalue(), "cli.main on the device")


def test_gfa_and_msa_together(engine):
    """OUT_GFA | OUT_MSA fills both, the MSA rows those of an OUT_MSA run; a job without the flag carries no record."""
    from abpoa_amd import api
    sets = _variant_sets()
    p = api.Params()
    both = api.msa_batch(sets, p, out_cons=True, out_msa=True, out_gfa=True, n_threads=4)
    assert api.msa_timing()["n_host_sets"] == 0
    msa = api.msa_batch(sets, p, out_cons=True, out_msa=True, n_threads=4)
    ref = api.msa_batch(sets, p, out_cons=True, out_msa=True, out_gfa=True, n_threads=4, lib=H.cpu_shim_lib())
    for a, b, c in zip(both, msa, ref):
        assert a.msa_seq == b.msa_seq == c.msa_seq and b.gfa is None
        GC.same_record(a.gfa, c.gfa, "OUT_GFA | OUT_MSA")


def test_shipped_front_ends(engine, tmp_path):
    """abpoa_batch --gfa-cons -l, the list in pieces of 4 files, against the reference binary where it is present, else the recorded sha; python -m abpoa_amd.cli
    --gfa on one file."""
    exe = os.path.join(H.ROOT, "abpoa_amd", "abpoa_batch")
    assert os.path.exists(exe), "abpoa_amd/abpoa_batch not built (make -C abpoa_amd/csrc)"
    case = GC.CASES["list6_r4"]
    lst = GC.case_input(case, tmp_path)
    p = subprocess.run([exe, "--piece", "4"] + GC.front_end_args(case, lst), capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr[-1500:]
    if os.path.exists(GC.REF):
        ref = subprocess.run([GC.REF] + GC.ref_args(case, lst), capture_output=True, timeout=300)
        assert ref.returncode == 0 and ref.stdout == p.stdout
    GC.assert_matches(case, p.stdout, "abpoa_batch -l on the device")
    case = GC.CASES["test_r3"]
    p = subprocess.run([sys.executable, "-m", "abpoa_amd.cli"] + GC.front_end_args(case, GC.case_input(case, tmp_path)), capture_output=True, timeout=300, cwd=H.ROOT)
    assert p.returncode == 0, p.stderr[-1500:]
    GC.assert_matches(case, p.stdout, "python -m abpoa_amd.cli on the device")


def test_devsync_gfa_check(engine, tmp_path):
    """ABPOA_HIP_DEVSYNC=1 (a child process: the library talks on stderr): the device record of the mirrored sets equals PoaGraph::gfa on the host graph fed
    the same cigars."""
    case = GC.CASES["seq_affine_r4"]
    env = dict(os.environ, ABPOA_HIP_DEVSYNC="1")
    p = subprocess.run([sys.executable, "-m", "abpoa_amd.cli"] + GC.front_end_args(case, GC.case_input(case, tmp_path)), capture_output=True, text=True, timeout=300,
                       cwd=H.ROOT, env=env)
    assert p.returncode == 0, p.stderr[-1500:]
    assert "gfa check ok" in p.stderr and "FAILED" not in p.stderr, p.stderr[-3000:]
    GC.assert_matches(case, p.stdout, "cli.main under ABPOA_HIP_DEVSYNC")
