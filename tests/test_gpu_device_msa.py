"""GPU (-m gpu): the device-resident read-set driver (graph, fusion, row order, remaining length on the GPU;
abpoa_amd/csrc/poa_device.hip) must give exactly what the host driver gives (which keeps the reference's graph code
and row order, and is itself pinned to the reference's outputs in test_gpu_msa.py / test_host_msa.py):
consensus, per-base coverage and DP cell counts of every set; and, with ABPOA_HIP_DEVSYNC=1, the device graph must
equal the host graph node for node after every read (the library checks that itself and reports on stderr)."""
import os
import subprocess
import sys

import pytest

from gpu_harness import engine  # noqa: F401  (the fixture)
from readset_worker import run_report

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _both(sets, params, n_threads=8):
    from abpoa_amd import api
    os.environ["ABPOA_HIP_HOSTGRAPH"] = "1"
    try:
        host = api.msa_batch(sets, params, n_threads=n_threads)
    finally:
        os.environ["ABPOA_HIP_HOSTGRAPH"] = "0"
    dev = api.msa_batch(sets, params, n_threads=n_threads)
    tm = api.msa_timing()
    return host, dev, tm


@pytest.mark.parametrize("name,kw,shape", [
    ("affine_5pct", dict(gap_open1=4, gap_open2=0, gap_ext1=2), (48, 16, 400, 0.05)),
    ("affine_15pct", dict(gap_open1=4, gap_open2=0, gap_ext1=2), (24, 20, 300, 0.15)),
    ("convex_default", dict(), (24, 12, 500, 0.10)),
    ("ragged_tiny", dict(gap_open1=4, gap_open2=0, gap_ext1=2), (16, 5, 40, 0.05)),
    # graphs of 1000+ rows: in the all-rounds kernel two wavefronts share the backtrack (backtrack_dir.h)
    ("affine_1kb", dict(gap_open1=4, gap_open2=0, gap_ext1=2), (24, 14, 1000, 0.06)),
    ("convex_1kb_noisy", dict(), (16, 12, 1100, 0.14)),
])
@pytest.mark.parametrize("lockstep", [0, 1], ids=["all_rounds_kernel", "lockstep_rounds"])
def test_device_driver_equals_host_driver(engine, monkeypatch, name, kw, shape, lockstep):
    """Both forms of the device driver: every set through all its rounds in one kernel (poa_rounds.hip; ragged sets: the sets of a batch
    have different numbers of reads), and one launch per phase and round (ABPOA_HIP_LOCKSTEP=1)."""
    from abpoa_amd import api, ffi, synth
    monkeypatch.setenv("ABPOA_HIP_LOCKSTEP", str(lockstep))
    n_sets, n_reads, ln, err = shape
    sets = [synth.make_read_set(11, i, n_reads if i % 5 else max(2, n_reads // 2), ln, err) for i in range(n_sets)]
    engine.abpoa_hip_reset_stats()
    host, dev, tm = _both(sets, api.Params(**kw))
    assert tm["n_groups"] == 1 and tm["n_host_sets"] == 0, f"device driver not used for every set: {tm}"
    assert (ffi.stats()["rounds_launches"] > 0) == (lockstep == 0), ffi.stats()
    for i, (a, b) in enumerate(zip(dev, host)):
        assert a.status == 0 and b.status == 0
        assert a.cons_seq == b.cons_seq, f"{name}: consensus of set {i} differs"
        assert a.cons_cov == b.cons_cov, f"{name}: coverage of set {i} differs"
        assert a.n_cells == b.n_cells, f"{name}: DP cell count of set {i} differs"


@pytest.mark.parametrize("env", [{}, {"ABPOA_HIP_PASS_SETS": "3"}, {"ABPOA_HIP_DIR_WIDE": "1"}, {"ABPOA_HIP_DIR_WIDE": "1", "ABPOA_HIP_RING_ROWS": "4"},
                                 {"ABPOA_HIP_DIR_WIDE": "0", "ABPOA_HIP_RING_ROWS": "4"}],
                         ids=["default", "three_passes", "direction_words", "direction_words_ring4", "records_ring4"])
@pytest.mark.parametrize("kw", [dict(), dict(gap_open1=4, gap_open2=0, gap_ext1=2)], ids=["convex", "affine"])
def test_wide_band_jobs_passes_and_arena_formats(engine, monkeypatch, env, kw):
    """Wide-band read-sets (4.5 kb reads: band half-width 55, rows of 3 chunks) through the device-resident driver in the forms the driver picks by
    job size and free memory on big jobs: one pass or several (passes of the resident number of sets), score-record or direction-word arenas, the
    8-row or the 4-row score ring (packed E differences in the convex int32 ring, 4-bit query codes).  All equal to the host driver."""
    from abpoa_amd import api, synth
    sets = [synth.make_read_set(23, i, 6, 4500, 0.08) for i in range(8)]
    host, dev, tm = _both(sets, api.Params(**kw))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    dev2 = api.msa_batch(sets, api.Params(**kw), n_threads=8)
    assert api.msa_timing()["n_host_sets"] == 0
    for i, (a, b, c) in enumerate(zip(dev, host, dev2)):
        assert a.status == 0 and b.status == 0 and c.status == 0
        assert a.cons_seq == b.cons_seq == c.cons_seq, f"{env}: consensus of set {i} differs"
        assert a.cons_cov == b.cons_cov == c.cons_cov, f"{env}: coverage of set {i} differs"
        assert a.n_cells == b.n_cells == c.n_cells, f"{env}: DP cell count of set {i} differs"


@pytest.mark.parametrize("env", [{}, {"ABPOA_HIP_DIR_WIDE": "1"}, {"ABPOA_HIP_DIR_WIDE": "1", "ABPOA_HIP_RING_ROWS": "4"}, {"ABPOA_HIP_NODIR": "1"}],
                         ids=["default", "direction_words", "direction_words_ring4", "records_only"])
@pytest.mark.parametrize("kw", [dict(), dict(gap_open1=4, gap_open2=0, gap_ext1=2)], ids=["convex", "affine"])
def test_mixed_band_widths_in_one_job(engine, monkeypatch, env, kw):
    """One job whose read-sets take different row loops -- 1.5 kb reads (narrow band, one chunk), 3.9 kb (band half-width 49: the wide loop's
    smallest), 7 kb (4 chunks), 11 kb with 12 % error (5-6 chunks, odd read lengths: the 4-bit query packing's last nibble) -- so that narrow and
    wide kernels, both score widths and both arena formats meet in the same launches.  Equal to the host driver."""
    from abpoa_amd import api, synth
    shapes = [(5, 1500, 0.05), (4, 3901, 0.08), (4, 7003, 0.05), (3, 11001, 0.12), (6, 1203, 0.10), (3, 9999, 0.15)]
    sets = [synth.make_read_set(29, i, *shapes[i % len(shapes)]) for i in range(9)]
    host, dev, tm = _both(sets, api.Params(**kw))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    dev2 = api.msa_batch(sets, api.Params(**kw), n_threads=8)
    assert api.msa_timing()["n_host_sets"] == 0
    for i, (a, b, c) in enumerate(zip(dev, host, dev2)):
        assert a.status == 0 and b.status == 0 and c.status == 0
        assert a.cons_seq == b.cons_seq == c.cons_seq, f"{env}: consensus of set {i} differs"
        assert a.cons_cov == b.cons_cov == c.cons_cov, f"{env}: coverage of set {i} differs"
        assert a.n_cells == b.n_cells == c.n_cells, f"{env}: DP cell count of set {i} differs"


@pytest.mark.parametrize("kw", [dict(), dict(gap_open1=4, gap_open2=0, gap_ext1=2)], ids=["convex", "affine"])
def test_two_wavefronts_on_a_backtrack_change_nothing(engine, monkeypatch, kw):
    """All-rounds kernel, graphs of 800-3000 rows: the backtrack shared by two wavefronts (the helper starts mid-graph and the main walk takes over its
    cigar where the two meet, backtrack_dir.h) against one wavefront per backtrack (ABPOA_HIP_DBG bit 10) and against the host driver: consensus,
    coverage and DP cell counts of 64 read-sets with 3-20 % errors, deletion- and insertion-heavy mixes, 8-25 reads."""
    from abpoa_amd import api, ffi, synth
    shapes = [(8 + (7 * i) % 18, 800 + 137 * (i % 13), 0.03 + 0.017 * (i % 11), None if i % 3 == 0 else ((0.02, 0.09, 0.02) if i % 3 == 1 else (0.02, 0.02, 0.09))) for i in range(64)]
    sets = [synth.make_read_set(41, i, n, ln, err, rates=rt) for i, (n, ln, err, rt) in enumerate(shapes)]
    p = api.Params(**kw)
    engine.abpoa_hip_reset_stats()
    host, two, tm = _both(sets, p)
    assert tm["n_host_sets"] == 0 and ffi.stats()["rounds_launches"] > 0
    monkeypatch.setenv("ABPOA_HIP_DBG", "1024")
    one = api.msa_batch(sets, p, n_threads=8)
    for i, (a, b, c) in enumerate(zip(two, one, host)):
        assert a.status == 0 and b.status == 0 and c.status == 0
        assert a.cons_seq == b.cons_seq == c.cons_seq and a.cons_cov == b.cons_cov == c.cons_cov and a.n_cells == b.n_cells == c.n_cells, f"set {i} {shapes[i]}"


@pytest.mark.parametrize("bt_bytes", ["4096", "6144"])
def test_small_backtrack_windows_with_wide_rows(engine, monkeypatch, bt_bytes):
    """The backtrack's LDS window at its smallest (ABPOA_HIP_BT_BYTES; in the all-rounds kernel four wavefronts share it: about 1 KB each) against noisy
    reads whose bands open to 100+ columns and whose rows keep score records beside their direction words: the window that was copied ahead of the geometry
    loads can then hold no complete row, and the walk has to drop that copy and size the window anew (backtrack_dir.h load_window).  Both forms of the
    driver, equal to the host driver."""
    from abpoa_amd import api, synth
    monkeypatch.setenv("ABPOA_HIP_BT_BYTES", bt_bytes)
    shapes = [(10 + i % 6, 700 + 90 * i, 0.20 + 0.02 * (i % 4), (0.05, 0.10, 0.05) if i % 2 else (0.05, 0.05, 0.10)) for i in range(12)]
    sets = [synth.make_read_set(47, i, n, ln, err, rates=rt) for i, (n, ln, err, rt) in enumerate(shapes)]
    for kw in (dict(gap_open1=4, gap_open2=0, gap_ext1=2), dict()):
        for lockstep in ("0", "1"):
            monkeypatch.setenv("ABPOA_HIP_LOCKSTEP", lockstep)
            host, dev, tm = _both(sets, api.Params(**kw))
            for i, (a, b) in enumerate(zip(dev, host)):
                assert a.status == 0 and b.status == 0, (kw, lockstep, i, a.status, b.status)
                assert a.cons_seq == b.cons_seq and a.cons_cov == b.cons_cov and a.n_cells == b.n_cells, f"{kw} lockstep={lockstep}: set {i} differs"


def test_device_graph_equals_host_graph_after_every_read(engine):
    """Runs in a child process because the check mode is chosen by an environment variable at call time and prints to stderr."""
    code = ("import os,sys; sys.path.insert(0, %r)\n"
            "from abpoa_amd import api, ffi, synth\n"
            "lib = ffi.lib(); ffi.check(lib.abpoa_hip_init(0))\n"
            "sets = [synth.make_read_set(3, i, 10, 250, 0.08) for i in range(6)]\n"
            "r = api.msa_batch(sets, api.Params(gap_open1=4, gap_open2=0, gap_ext1=2), n_threads=4)\n"
            "print('OK', all(x.status == 0 for x in r), api.msa_timing()['n_host_sets'])\n" % ROOT)
    env = dict(os.environ, ABPOA_HIP_DEVSYNC="1", ABPOA_HIP_HOSTGRAPH="0")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "OK True 0" in p.stdout
    assert "graph check ok" in p.stderr and "consensus check ok" in p.stderr and "FAILED" not in p.stderr, p.stderr[-3000:]


def test_device_audit_mode_reports_where_every_pool_landed():
    """ABPOA_HIP_DEVICE_AUDIT=1 (child process: the switch is read once): every pool and staging allocation of every device queue is looked up with
    hipPointerGetAttributes and must sit on the device its queue serves, with the queue thread's current device set to it -- a call fails with ENODEV
    otherwise.  Two queues on device 0 here (the pool has one GPU per box); on a multi-GPU node the same switch checks the distinct-ordinal path."""
    code = ("import os,sys; sys.path.insert(0, %r)\n"
            "from abpoa_amd import api, ffi, synth\n"
            "lib = ffi.lib(); ffi.check(lib.abpoa_hip_init(0))\n"
            "sets = [synth.make_read_set(13, i, 5 + i %% 4, 150 + 30 * (i %% 5), 0.06) for i in range(600)]\n"
            "r = api.msa_batch(sets, api.Params(gap_open1=4, gap_open2=0, gap_ext1=2), n_threads=8)\n"
            "print('OK', all(x.status == 0 for x in r), api.msa_timing()['n_groups'], api.msa_timing()['n_host_sets'])\n" % ROOT)
    env = dict(os.environ, ABPOA_HIP_DEVICE_AUDIT="1", ABPOA_HIP_VERBOSE="1", ABPOA_GPU_DEVICES="0,0", ABPOA_GPU_BATCHES_PER_DEVICE="1")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "OK True 2 0" in p.stdout, (p.stdout, p.stderr[-2000:])
    lines = [ln for ln in p.stderr.splitlines() if "audit:" in ln]
    assert len(lines) >= 8, p.stderr[-2000:]      # (two queues x at least four pools)
    assert all("device 0 (queue device 0, thread's current device 0)" in ln for ln in lines), lines


def test_multi_queue_batch_call_matches_single_queue(engine):
    """abpoa_hip_msa_batch with ABPOA_GPU_DEVICES: cost-sorted batches dealt to per-device queues on worker threads, results in caller
    order.  One GPU here, so the list names device 0 twice (two queues, two pool caches, two streams): same records as the single queue.
    The read-sets are ragged (different read counts and lengths) so that the cost sort really permutes them.
    NOT covered here or anywhere: two DIFFERENT device ordinals (per-device __constant__ argument records of the all-rounds kernel, pool caches on
    several devices) -- the test boxes of this pool have one GPU; the multi-GPU bench of the build driver is the first run of that path."""
    from abpoa_amd import api, synth
    sets = [synth.make_read_set(11, i, 4 + i % 7, 120 + 40 * (i % 5), 0.06) for i in range(600)]
    p = api.Params(gap_open1=4, gap_open2=0, gap_ext1=2)
    one = api.msa_batch(sets, p, n_threads=8)
    os.environ["ABPOA_GPU_DEVICES"] = "0,0"
    os.environ["ABPOA_GPU_BATCHES_PER_DEVICE"] = "2"
    try:
        two = api.msa_batch(sets, p, n_threads=8)
        assert api.msa_timing()["n_groups"] == 2
    finally:
        del os.environ["ABPOA_GPU_DEVICES"], os.environ["ABPOA_GPU_BATCHES_PER_DEVICE"]
    for a, b in zip(one, two):
        assert (a.status, a.cons_seq, a.cons_cov, a.n_cells) == (0, b.cons_seq, b.cons_cov, b.n_cells)


def test_job_shape_hint_skips_the_doomed_pass(engine):
    """Noisy reads outgrow the 3x node estimate of the first device pass; the second such job of the process starts at the factor that held them (4.5x or 6x).  Same results either
    way, equal to the host driver's.  (Child process: the hint is process-wide state and the passes are reported on stderr.)"""
    code = ("import os,sys; sys.path.insert(0, %r)\n"
            "from abpoa_amd import api, ffi, synth\n"
            "lib = ffi.lib(); ffi.check(lib.abpoa_hip_init(0))\n"
            "sets = [synth.make_read_set(5, i, 30, 2000, 0.30) for i in range(6)]\n"
            "p = api.Params(gap_open1=4, gap_open2=0, gap_ext1=2)\n"
            "a = api.msa_batch(sets, p, n_threads=4); sys.stderr.write('SECOND CALL\\n'); b = api.msa_batch(sets, p, n_threads=4)\n"
            "os.environ['ABPOA_HIP_HOSTGRAPH'] = '1'; h = api.msa_batch(sets, p, n_threads=4)\n"
            "print('OK', all(x.status == 0 and x.cons_seq == y.cons_seq == z.cons_seq and x.cons_cov == y.cons_cov == z.cons_cov for x, y, z in zip(a, b, h)))\n" % ROOT)
    env = dict(os.environ, ABPOA_HIP_VERBOSE="1", ABPOA_HIP_HOSTGRAPH="0")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "OK True" in p.stdout, p.stdout
    first, second = p.stderr.split("SECOND CALL")
    assert "pass 1, node slots 3x" in first and ("pass 2, node slots 4.5x" in first), first[-1500:]
    assert "node slots 3x" not in second and ("node slots 4.5x" in second or "node slots 6x" in second), second[-1500:]


@pytest.mark.parametrize("lockstep", [0, 1], ids=["all_rounds_kernel", "lockstep_rounds"])
def test_device_driver_equals_oracle_backed_host_run(engine, monkeypatch, lockstep):
    """An independent check of the device-resident driver and its row-loop bodies (straight-line copies for 1-8 predecessors and for vectors beyond
    the predecessors' bands, the two-chunk body, the exact bodies): the same read-sets through the CPU build of the host layer whose aligner is the
    plain-C oracle (tests/cpu_shim.cpp).  Shapes chosen to leave the common path: narrow and wide extra bands (-b / -f), 2-25 % errors with
    deletion- and insertion-heavy mixes, convex and affine gaps, ragged read counts, reads of 150-1400 bases."""
    import helpers as H
    from abpoa_amd import api, ffi, synth
    monkeypatch.setenv("ABPOA_HIP_LOCKSTEP", str(lockstep))
    shim = H.cpu_shim_lib()
    cases = [
        (dict(gap_open1=4, gap_open2=0, gap_ext1=2), [(12 + i % 9, 150 + 97 * i, 0.02 + 0.02 * (i % 6), None) for i in range(10)]),
        (dict(), [(10 + i % 7, 300 + 130 * i, 0.12, (0.02, 0.08, 0.02) if i % 2 else (0.02, 0.02, 0.08)) for i in range(8)]),
        (dict(gap_open1=4, gap_open2=0, gap_ext1=2, extra_b=5, extra_f=0.02), [(16, 400 + 150 * i, 0.25, None) for i in range(6)]),
        (dict(gap_open1=6, gap_open2=30, gap_ext1=3, gap_ext2=1, extra_b=30, extra_f=0.03, match=3, mismatch=5), [(9 + i, 500 + 60 * i, 0.10, None) for i in range(6)]),
        # penalties outside the direction words' range (o1 > 7): score-record arenas, on wide bands
        (dict(gap_open1=20, gap_open2=60, gap_ext1=3, gap_ext2=1, extra_b=35, extra_f=0.02), [(7 + i, 600 + 90 * i, 0.12, None) for i in range(5)]),
        (dict(gap_open1=9, gap_open2=0, gap_ext1=4, extra_b=40, extra_f=0.01), [(8, 700 + 50 * i, 0.08, (0.02, 0.03, 0.03)) for i in range(5)]),
    ]
    for kw, shapes in cases:
        sets = [synth.make_read_set(23, i, n, ln, err, rates=rt) for i, (n, ln, err, rt) in enumerate(shapes)]
        p = api.Params(**kw)
        engine.abpoa_hip_reset_stats()
        dev = api.msa_batch(sets, p, n_threads=4)
        assert api.msa_timing()["n_host_sets"] == 0, "device driver not used for every set"
        w_max = p.wb + int(p.wf * max(ln for _, ln, _, _ in shapes))      # (a band half-width of 40 or more takes the wide row loop: one launch per phase and round)
        assert (ffi.stats()["rounds_launches"] > 0) == (lockstep == 0 and w_max < 40)
        ref = api.msa_batch(sets, p, n_threads=4, lib=shim)
        for i, (a, b) in enumerate(zip(dev, ref)):
            assert a.status == 0 and b.status == 0
            assert a.cons_seq == b.cons_seq and a.cons_cov == b.cons_cov, f"{kw}: set {i} differs from the oracle-backed run"


CIGAR_JOBS = {
    # narrow bands, graphs of 700-2500 rows: in the all-rounds kernel four wavefronts share every backtrack (helper parts, merged cigars)
    "narrow_affine": (dict(gap_open1=4, gap_open2=0, gap_ext1=2), [(12, 700 + 60 * i, 0.08) for i in range(8)]),
    "narrow_convex_noisy": (dict(), [(10, 900 + 90 * i, 0.15) for i in range(6)]),
    "narrow_1500": (dict(gap_open1=4, gap_open2=0, gap_ext1=2), [(9, 1500 + 100 * i, 0.05 + 0.02 * i) for i in range(5)]),
    # wide bands (10 kb reads: the all-chunks row loop, column-slice backtrack windows), 5 % and 15 % errors
    "wide_affine_5": (dict(gap_open1=4, gap_open2=0, gap_ext1=2), [(8, 10000 + 17 * i, 0.05) for i in range(4)]),
    "wide_convex_15": (dict(), [(8, 10000 - 23 * i, 0.15) for i in range(4)]),
    # long reads (the long-read form of the wide row loop, dp_xl_rows.hip: rows of 9-11 chunks): 26 kb reads score in int32 (2 x 26 000 > 32 767)
    # (test_long_read_rows_take_the_all_chunk_bodies pins it).  The int16 8 kb and the int32 3 kb jobs under a wide band (-b 200 / 300) are cigar checks of
    # their own: the device-resident driver does not give them the wide row loop (its row counters show no all-chunk body rows there)
    "long_reads_i32": (dict(), [(4, 26000 + 37 * i, 0.05) for i in range(4)]),
    "long_reads_i32_affine": (dict(gap_open1=4, gap_open2=0, gap_ext1=2), [(4, 26000 + 37 * i, 0.05) for i in range(4)]),
    "long_reads_i16": (dict(extra_b=200), [(4, 8000 + 37 * i, 0.05) for i in range(4)]),
    "xl_i32_b300": (dict(match=12, extra_b=300), [(6, 3000 + 41 * i, 0.08) for i in range(4)]),
    "xl_i32_b300_affine": (dict(gap_open1=4, gap_open2=0, gap_ext1=2, match=12, extra_b=300), [(6, 3000 + 41 * i, 0.08) for i in range(4)]),
    # the general kernel's own jobs on the device-resident driver (tests/test_gpu_device_general.py): linear gaps, extension mode, no band
    "linear_banded": (dict(gap_open1=0, gap_open2=0, gap_ext1=2), [(9, 400 + 90 * i, 0.06) for i in range(6)]),
    "extend_convex": (dict(aln_mode=2), [(9, 500 + 70 * i, 0.10) for i in range(6)]),
    "affine_unbanded": (dict(gap_open1=4, gap_open2=0, gap_ext1=2, extra_b=-1), [(8, 300 + 60 * i, 0.08) for i in range(6)]),
}


def make_jobs(job):
    """{job: spec} for tests/readset_worker.py: one of CIGAR_JOBS in the form the child's own environment selects, and through the oracle-backed host layer."""
    from abpoa_amd import synth
    kw, shapes = CIGAR_JOBS[job]
    sets = [synth.make_read_set(23, i, n, ln, err) for i, (n, ln, err) in enumerate(shapes)]
    return {job: dict(params=kw, sets=sets, forms={"device": {}}, record=("dig", "rounds_launches", "n_host_sets"), ref_record=("dig",), ref_threads=8)}


@pytest.mark.parametrize("job,env", [("narrow_affine", {}), ("narrow_affine", {"ABPOA_HIP_LOCKSTEP": "1"}), ("narrow_convex_noisy", {}), ("narrow_convex_noisy", {"ABPOA_HIP_LOCKSTEP": "1"}),
                                     ("narrow_affine", {"ABPOA_HIP_DBG": "2048"}),
                                     ("narrow_1500", {}), ("narrow_1500", {"ABPOA_HIP_DBG": "1024"}), ("narrow_1500", {"ABPOA_HIP_DBG": "2048"}), ("narrow_1500", {"ABPOA_HIP_DEVICE_GENERAL": "1"}),
                                     ("linear_banded", {}), ("linear_banded", {"ABPOA_HIP_LOCKSTEP": "1"}), ("linear_banded", {"ABPOA_HIP_DEVICE_GENERAL": "1"}), ("extend_convex", {}), ("affine_unbanded", {}),
                                     ("wide_affine_5", {"ABPOA_HIP_DIR_WIDE": "0"}), ("wide_affine_5", {"ABPOA_HIP_DIR_WIDE": "1"}), ("wide_affine_5", {"ABPOA_HIP_DIR_WIDE": "1", "ABPOA_HIP_RING_ROWS": "4"}),
                                     ("wide_convex_15", {"ABPOA_HIP_DIR_WIDE": "0"}), ("wide_convex_15", {"ABPOA_HIP_DIR_WIDE": "1"}), ("wide_convex_15", {"ABPOA_HIP_DIR_WIDE": "1", "ABPOA_HIP_RING_ROWS": "4"}),
                                     ("long_reads_i32", {}), ("long_reads_i32", {"ABPOA_HIP_DIR_WIDE": "0"}), ("long_reads_i32", {"ABPOA_HIP_DIR_WIDE": "1"}),
                                     ("long_reads_i32_affine", {"ABPOA_HIP_DIR_WIDE": "0"}), ("long_reads_i32_affine", {"ABPOA_HIP_DIR_WIDE": "1"}),
                                     ("long_reads_i16", {}), ("xl_i32_b300", {}), ("xl_i32_b300_affine", {"ABPOA_HIP_DIR_WIDE": "0"}),
                                     ("xl_i32_b300_affine", {"ABPOA_HIP_DIR_WIDE": "1"})],
                         ids=lambda v: v if isinstance(v, str) else ("default" if not v else "_".join(f"{k[10:].lower()}{x}" for k, x in v.items())))
def test_device_driver_cigars_equal_the_oracle_backed_run(engine, job, env):
    """Direct cigar comparison (not only consensus / coverage).  With ABPOA_HIP_CIGAR_DIGEST=1 the fuse phase of the device-resident driver folds the graph
    cigar of every alignment into a 64-bit digest per read-set ON THE DEVICE (poa_bodies.h, poa_device.h poa_cigar_digest_round) -- so both of its forms are
    covered: the all-rounds kernel, whose backtrack is shared by four wavefronts (helper cigar parts, merged at the cells where the walks meet), and the
    lock-step launches; narrow bands and 10 kb wide bands in both arena formats (score records / direction words, 8- and 4-row score ring).  The CPU build of
    the host driver, whose aligner is the plain-C oracle, folds the same function over its cigars (msa_batch.cpp): equal digests = equal cigars, word for word."""
    rep = run_report("test_gpu_device_msa", job, set_env=dict(env, ABPOA_HIP_CIGAR_DIGEST="1"), clear_env=(), timeout=900)[job]
    dev, ref = rep["device"], rep["ref"]
    assert all(s == 0 for s in dev["status"]) and dev["n_host_sets"] == 0, dev
    assert all(d != 0 for d in dev["dig"]) and dev["dig"] == ref["dig"], (dev["dig"], ref["dig"])
    assert dev["cons"] == ref["cons"]
    # (banded linear jobs: the fast row loops and the all-rounds kernel since round 5 -- H records, lane-parallel linear backtrack steps)
    narrow_all_rounds = (job.startswith("narrow") or job == "linear_banded") and "ABPOA_HIP_LOCKSTEP" not in env and "ABPOA_HIP_DEVICE_GENERAL" not in env
    assert (dev["rounds_launches"] != 0) == narrow_all_rounds, dev["rounds_launches"]


def test_assembly_row_loop_equals_the_compiler_loop():
    """The headline workload's narrow rows run the hand-placed assembly loop (rows_tight_asm.h); ABPOA_HIP_DBG=2048 runs the compiler's loop of the same
    body instead (rows_fast.h asm_tight_on).  cfg2 sets with and without it: identical consensus, and both hash to the committed reference digests
    (tests/golden/bench_digests/cfg2.json)."""
    import json
    import subprocess
    import sys
    idx = [0, 1, 2, 3, 999]
    code = ("import sys, json; sys.path.insert(0, %r)\n"
            "from abpoa_amd import api, ffi, synth, workloads as W\n"
            "ffi.check(ffi.lib().abpoa_hip_init(0))\n"
            "w = W.WORKLOADS['cfg2']; idx = %r\n"
            "sets = [synth.make_read_set(1, i, **synth.CONFIGS[w['cfg']]) for i in idx]\n"
            "res = api.msa_batch(sets, api.Params(**w['params']), out_cons=True, out_msa=False)\n"
            "assert all(r.status == 0 for r in res)\n"
            "print('SHA', json.dumps([W.output_sha(api.format_output(r, ['r%%d' %% j for j in range(len(sets[0]))], True, False)) for r in res]))\n" % (ROOT, idx))
    outs = []
    for env in ({}, {"ABPOA_HIP_DBG": "2048"}):
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, **env), timeout=600)
        assert r.returncode == 0, (env, r.stdout[-1500:], r.stderr[-3000:])
        outs.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("SHA ")][-1][4:]))
    from abpoa_amd import workloads as W
    ref = W.load_digests("cfg2")
    assert outs[0] == outs[1] == [ref[i] for i in idx]


# the long-read jobs above and the score width their rows of 9-11 chunks run in
LONG_ROW_JOBS = {"long_reads_i32": 32, "long_reads_i32_affine": 32}


@pytest.mark.slow
def test_long_read_rows_take_the_all_chunk_bodies(tmp_path):
    """The long-read jobs of CIGAR_JOBS do test what they are there for: the diagnostic build's row counters (Makefile `counters`,
    -DABPOA_HIP_WIDE_COUNTERS) report rows completed by the 9-11-chunk bodies of the long-read form in the job's score width (and none in the other),
    and no row declined by the arg-max key window or the wrap guard.  (With a 6-bit vector order in the int32 key, vector 64 of every such row wrapped
    into the key's value bits and declined nearly every row.)  Then, with the same library through the flat API, the re-banded 1 kb goldens of
    tests/test_gpu_wide_bodies.py at 6, 7, 8-9 and 11 chunks and at the last band of the 448-column kernel: rows declined as "wider than the body" = the
    oracle's count of such rows, 9-11-chunk rows in the run's own width only, at most 10 % of the rows declined for any other reason (measured: 1.3 % at most,
    LOG.md round 12 -- a condition on the inputs: move a band that fails it, do not raise the cap).  The same on the skip-edge families `far`, `many` and
    `in_ring` of tests/wide_preds.py at wb = 130 and 250: the rows declined as "not eligible" (slot 1) == the rows with more than 8 predecessors or a predecessor
    64 and more rows back, counted on the inputs -- so tile bit 19 is false on exactly those rows and the eligible ones reached the bodies."""
    import re
    import subprocess
    import sys
    csrc = os.path.join(ROOT, "abpoa_amd", "csrc")
    lib = str(tmp_path / "libabpoa_hip_wc.so")
    b = subprocess.run(["make", "-C", csrc, "counters", "WC_OBJDIR=" + str(tmp_path / "obj"), "WC_OUT=" + lib], capture_output=True, text=True, timeout=1500)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ABPOA_HIP_LIB=lib, ABPOA_HIP_WIDE_COUNTERS="1", ABPOA_HIP_DBG="128", ABPOA_HIP_DEVSYNC="1", ABPOA_HIP_IMBAL="1")
    for job, bits in LONG_ROW_JOBS.items():
        kw, shapes = CIGAR_JOBS[job]
        code = ("import sys; sys.path.insert(0, %r)\n"
                "from abpoa_amd import api, ffi, synth\n"
                "ffi.check(ffi.lib().abpoa_hip_init(0))\n"
                "sets = [synth.make_read_set(23, i, n, ln, err) for i, (n, ln, err) in enumerate(%r)]\n"
                "res = api.msa_batch(sets, api.Params(**%r), n_threads=4)\n"
                "assert all(r.status == 0 for r in res) and api.msa_timing()['n_host_sets'] == 0\n"
                "print('DONE')\n" % (ROOT, shapes, kw))
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0 and "DONE" in r.stdout, (job, r.stdout[-1500:], r.stderr[-3000:])
        rows = re.findall(r"wide-loop rows per alignment \(diagnostic build\): all-chunk body ([\d.]+) .*key window / wrap ([\d.]+) \| "
                          r"9-11-chunk bodies int32 ([\d.]+) int16 ([\d.]+)", r.stderr)
        assert len(rows) == max(n for n, _, _ in shapes) - 1, (job, r.stderr[-3000:])          # one line per alignment round
        declined = sum(float(x[1]) for x in rows)
        long32, long16 = sum(float(x[2]) for x in rows), sum(float(x[3]) for x in rows)
        assert declined == 0, (job, rows)
        assert (long32 > 0 and long16 == 0) if bits == 32 else (long16 > 0 and long32 == 0), (job, rows)
    # The same library on the inputs of tests/test_gpu_wide_bodies.py (table: tests/wide_bands.py), through the flat API: the rows those tests compare with the
    # oracle did take the all-chunk bodies.  abpoa_hip__debug_clocks slots 4 .. 9 = AlnOut.seg[0 .. 5] = rows per path (abpoa_amd/csrc/diag.h WideSlot): 0 all-chunk body
    # (a row of 9-11 chunks also in bits 32-47 / 48-62 for int32 / int16), 1 not eligible, 2 ring / geometry, 3 wider than the body's chunks, 4 vectors beyond
    # every predecessor's band outside the last chunk, 5 the body declined (arg-max key window, wrap guard).
    import json
    points = WIDE_BODY_POINTS + WIDE_PRED_POINTS
    r = subprocess.run([sys.executable, "-c", _WIDE_BODY_COUNTERS % dict(root=ROOT, points=points)], capture_output=True, text=True,
                       env=dict(os.environ, ABPOA_HIP_LIB=lib, ABPOA_HIP_DBG="128"), timeout=600)
    assert r.returncode == 0 and "DONE" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    recs = [json.loads(ln[4:]) for ln in r.stdout.splitlines() if ln.startswith("ROW ")]
    assert len(recs) == len(points)
    import wide_preds as WP
    for rec in recs:
        print("wide-body counters", json.dumps(rec))
        golden, bits, wb, noxl, family = rec["point"]
        # slot 1 ("not eligible": more than 8 predecessors, or one 64 and more rows back) == the count tests/test_wide_pred_regimes.py takes from the inputs
        assert rec["seg"][1] == rec["not_eligible"] == (WP.NOT_ELIGIBLE[family][("s1k_ag_gb", "s1k_cg_gb").index(golden)] if family else 0), rec
        seg, chunks = rec["seg"], {int(k): v for k, v in rec["chunks"].items()}      # chunks: per count, the oracle's rows 1 .. n - 2 (the rows a body may take)
        widest = 7 if rec["ring_cols"] == 448 else 11
        body, long32, long16 = seg[0] & 0xffffffff, (seg[0] >> 32) & 0xffff, seg[0] >> 48
        assert seg[3] == sum(v for n, v in chunks.items() if n > widest), rec
        n_long = sum(v for n, v in chunks.items() if 9 <= n <= widest)
        own, other = (long32, long16) if bits == 32 else (long16, long32)
        assert other == 0 and (own > 0) == (n_long > 0) and own <= n_long, rec
        assert 10 * (seg[1] + seg[2] + seg[4] + seg[5]) <= rec["rows"], rec
        assert body + seg[1] + seg[2] + seg[3] + seg[4] + seg[5] <= rec["rows"] and body >= sum(v for n, v in chunks.items() if 2 <= n <= widest) - (seg[1] + seg[2] + seg[4] + seg[5]), rec


# both goldens x both widths at 6, 7, 8-9 and 11 chunks, and the last band of the 448-column kernel (ABPOA_HIP_NOXL=1), whose 8-chunk rows it declines
WIDE_BODY_POINTS = [(g, b, wb, 0, None) for g in ("s1k_ag_gb", "s1k_cg_gb") for b in (16, 32) for wb in (165, 196, 250, 324)] + \
                   [(g, b, 215, 1, None) for g in ("s1k_ag_gb", "s1k_cg_gb") for b in (16, 32)]
# ... and the skip-edge families of tests/wide_preds.py whose rows the wide kernels must decline as "not eligible" (`many` and `in_ring`: 9-11 predecessors;
# `far`: a predecessor 64 and more rows back), at two bands per width
WIDE_PRED_POINTS = [(g, b, wb, 0, f) for g in ("s1k_ag_gb", "s1k_cg_gb") for b in (16, 32) for wb in (130, 250) for f in ("far", "many", "in_ring")]
_WIDE_BODY_COUNTERS = r"""
import ctypes, json, os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + '/tests')
import helpers as H, wide_bands as WB, wide_preds as WP
from abpoa_amd import ffi
lib = ffi.lib(); ffi.check(lib.abpoa_hip_init(0))
clk = (ctypes.c_longlong * 10)()
for golden, bits, wb, noxl, family in %(points)r:
    g = H.first_golden(golden)
    c = H.FlatCase(WP.case_dict(golden, family, bits, wb) if family else H.rescored(g, WB.point(golden, bits, int(g['qlen'][0])), wb, 0.0))
    o = H.run_oracle(c)
    pn = 16 if o.bits == 16 else 8
    rows = WP.wide_rows(c, o)
    chunks = {}
    for r in range(1, c.n_rows - 1):
        if o.dp_beg_sn[r] >= 0 and rows[r].eligible:      # (a row that is not eligible never reaches the body's width test)
            n = ((int(o.dp_end_sn[r]) - int(o.dp_beg_sn[r]) + 1) * pn + 63) // 64
            chunks[n] = chunks.get(n, 0) + 1
    if noxl: os.environ['ABPOA_HIP_NOXL'] = '1'
    else: os.environ.pop('ABPOA_HIP_NOXL', None)
    lib.abpoa_hip__debug_clocks(clk)
    h = H.run_hip([c], want_trace=False)[0]
    lib.abpoa_hip__debug_clocks(clk)
    assert h.status == 0 and o.bits == bits and WB.inside(golden, bits, wb, bool(noxl))
    H.compare_outs(h, o, label='counters build %%s %%s int%%d wb=%%d' %% (golden, family, bits, wb))
    print('ROW ' + json.dumps(dict(point=[golden, bits, wb, noxl, family], ring_cols=WB.RING_COLS[WB.plan(golden, bits, wb, bool(noxl))[2]], rows=len(rows),
                                   not_eligible=WP.not_eligible(rows), chunks=chunks, seg=[int(clk[4 + i]) for i in range(6)])))
print('DONE')
"""
