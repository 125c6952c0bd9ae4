"""What the GFA output (ABPOA_HIP_OUT_GFA) costs, and how it compares with the reference's -r 4.

    python tools/gfa_bench.py [--shapes 1000x50x1000,256x50x10000] [--steps 3] [--ref-sets 64] [--out profiles/gfa.txt]

Per shape (read-sets x reads x bases; synth.make_read_set at the headline's error rates): (1) the wall time of an OUT_GFA | OUT_CONS job of abpoa_hip_msa_batch
beside an OUT_MSA | OUT_CONS job of the same build (median of --steps after one warm-up each); (2) the durations of poa_gfa_walk_kernel and
poa_gfa_fill_kernel by hipEvents and the bytes of the result download (abpoa_hip_get_gfa_timing); (3) `abpoa_ref -r 4` (oracle/_ref, where it was built) on the
first --ref-sets sets, one file each, in 16 processes at a time, as read-sets per second."""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CORES = 16
REF = os.path.join(ROOT, "oracle", "_ref", "abpoa_ref")


class GfaTiming(C.Structure):
    _fields_ = [("walk_ms", C.c_double), ("fill_ms", C.c_double), ("d2h_bytes", C.c_int64)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="1000x50x1000,256x50x10000")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--ref-sets", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from abpoa_amd import api, ffi, synth
    lib = ffi.lib()
    ffi.check(lib.abpoa_hip_init(0))
    lib.abpoa_hip_get_gfa_timing.argtypes, lib.abpoa_hip_get_gfa_timing.restype = [C.POINTER(GfaTiming)], None
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for shape in a.shapes.split(","):
        n_sets, n_reads, length = (int(x) for x in shape.split("x"))
        err = 0.05 if length <= 1000 else 0.15
        p = api.Params(gap_open1=4, gap_open2=0, gap_ext1=2) if length <= 1000 else api.Params()
        sets = [synth.make_read_set(1, i, n_reads, length, err) for i in range(n_sets)]
        enc = api.EncodedSets(sets, p.m)

        def step(**kw):
            ts = []
            for i in range(a.steps + 1):
                t0 = time.perf_counter()
                res = api.msa_batch(None, p, out_cons=True, encoded=enc, **kw)
                ts.append(time.perf_counter() - t0)
                assert all(r.status == 0 for r in res)
            return statistics.median(ts[1:]), api.msa_timing()["n_host_sets"]
        t_msa, h_msa = step(out_msa=True)
        t_gfa, h_gfa = step(out_gfa=True)
        gt = GfaTiming()
        lib.abpoa_hip_get_gfa_timing(C.byref(gt))
        say(f"{shape}: OUT_MSA|OUT_CONS {t_msa * 1e3:.1f} ms/step ({n_sets / t_msa:.0f} sets/s, {h_msa} host sets); OUT_GFA|OUT_CONS {t_gfa * 1e3:.1f} ms/step "
            f"({n_sets / t_gfa:.0f} sets/s, {h_gfa} host sets)")
        say(f"{shape}: poa_gfa_walk_kernel {gt.walk_ms:.2f} ms, poa_gfa_fill_kernel {gt.fill_ms:.2f} ms, result download {gt.d2h_bytes / 1e6:.1f} MB")
        if os.path.exists(REF):
            n_ref = min(a.ref_sets, n_sets)
            with tempfile.TemporaryDirectory() as td:
                files = []
                for i in range(n_ref):
                    files.append(os.path.join(td, f"s{i}.fa"))
                    synth.write_fasta(files[-1], sets[i])
                args = (["-O", "4,0", "-E", "2"] if length <= 1000 else []) + ["-r", "4"]
                t0 = time.perf_counter()
                with ThreadPoolExecutor(CORES) as ex:
                    rcs = list(ex.map(lambda f: subprocess.run([REF] + args + [f], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode, files))
                t_ref = time.perf_counter() - t0
            assert not any(rcs)
            say(f"{shape}: abpoa_ref -r 4, {n_ref} sets in {CORES} processes: {t_ref:.2f} s = {n_ref / t_ref:.1f} sets/s; the GFA job is {n_sets / t_gfa / (n_ref / t_ref):.1f}x that")
        else:
            say(f"{shape}: oracle/_ref/abpoa_ref not built: no reference figure")
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
