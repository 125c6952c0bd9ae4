"""GPU (-m gpu): bench.py's auxiliary modes on small jobs (the default line is the build driver's own run)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stream_mode_generates_and_checks_piece_by_piece():
    """--stream: the job is generated PIECE read-sets at a time in the generator pool (already as residue codes) while the engine works on the piece before;
    at most three pieces are in host memory (in the engine, laid out, being generated); every set with a committed reference digest is checked."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "cfg2", "--sets", "96", "--stream", "32", "--threads", "8"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    assert rec["mode"] == "stream" and rec["parity_sets_total"] == 96 and rec["parity_sets_checked"] == 96
    assert rec["config"]["pieces_rank0"] == 3 and rec["config"]["peak_read_sets_in_host_memory_rank0"] == 96
    assert rec["value"] > 0 and rec["value_engine_only"] >= rec["value"]


def test_plain_run_times_its_steps_and_dumps_the_last_one(tmp_path):
    """A plain run (no --full): the headline only, --steps timed steps, and --dump-outputs writes what the last step returned -- every dumped consensus
    must be the reference's for that set (committed digests), and a second run over the same arguments must dump the same arrays."""
    import numpy as np
    from abpoa_amd.workloads import load_digests, output_sha
    dumps = []
    for k in range(2):
        d = tmp_path / f"dump{k}"
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "cfg2", "--sets", "64", "--steps", "3", "--warmup", "1", "--threads", "8",
                            "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert p.returncode == 0, p.stderr[-3000:]
        rec = json.loads(p.stdout.strip().splitlines()[-1])
        assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["ms_per_step"] > 0 and rec["value"] > 0
        assert "secondary" not in rec and "cpu_baseline" not in rec
        arrs = {f.name[:-4]: np.load(f) for f in sorted(d.iterdir())}
        assert all(a.dtype in (np.float32, np.float64) for a in arrs.values()) and sum(a.nbytes for a in arrs.values()) <= 64 << 20
        dumps.append(arrs)
    a = dumps[0]
    assert a["set_index"].tolist() == list(range(64)) and not a["status"].any()
    ends = np.cumsum(a["cons_len"].astype(np.int64))
    assert ends[-1] == len(a["cons_seq"]) == len(a["cons_cov"])
    ref = load_digests("cfg2")
    for i, (s, e) in enumerate(zip(np.r_[0, ends[:-1]], ends)):
        seq = a["cons_seq"][s:e].astype(np.uint8).tobytes().decode()
        assert output_sha(">Consensus_sequence\n" + seq + "\n") == ref[i], f"set {i}: dumped consensus differs from the reference's"
    assert dumps[0].keys() == dumps[1].keys() and all(np.array_equal(dumps[0][k], dumps[1][k]) for k in dumps[0])
