"""What the guide-tree order (-p) costs on the headline job: BASELINE.json configs[1]-shaped, N read-sets x 50 reads x 1 kb, global affine.

    python tools/guide_order_bench.py [--sets 1000] [--steps 5] [--out profiles/guide_order.txt]

Reports (1) the device pre-pass: sketch kernel (both passes) and pair kernel by hipEvents on the pre-pass's queue, and its wall time with packing,
copies and the host's greedy order; (2) the step time of abpoa_hip_msa_batch with and without ABPOA_HIP_PROGRESSIVE (wall, median of --steps after
one warm-up each); (3) the same order built by the reference's own abpoa_collect_mm + abpoa_build_guide_tree (oracle/_ref/libabpoa_ref.so, where it was
built) in 16 processes, each timing only its calls into the library -- the slowest process is the 16-core time -- and checks that both give the same
order for every set."""
import argparse
import ctypes as C
import multiprocessing as mp
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
CORES = 16


def _gen(idx):
    from abpoa_amd import seqio, synth
    return [seqio.encode(r, 5) for r in synth.make_read_set(1, idx, **synth.CONFIGS[2])]


def _ref_share(sets):
    """The reference's order of every set of `sets`; returns (orders, seconds inside the library)."""
    import numpy as np
    import make_guide_order_golden as G
    L = G.ref()
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    para = L.abpoa_init_para()
    para.contents.m, para.contents.k, para.contents.w, para.contents.amb_strand, para.contents.progressive_poa = 5, 19, 10, 0, 1
    prepared = []
    for codes in sets:
        n = len(codes)
        arrs = [np.ascontiguousarray(c, np.uint8) for c in codes]
        prepared.append((n, arrs, (C.POINTER(C.c_uint8) * n)(*[a.ctypes.data_as(C.POINTER(C.c_uint8)) for a in arrs]), (C.c_int * n)(*[len(a) for a in arrs])))
    orders, spent = [], 0.0
    for n, arrs, ptrs, lens in prepared:
        mm, mm_c, order = G.U128V(0, 0, None), (C.c_int * (n + 1))(), (C.c_int * n)(*range(n))
        t0 = time.perf_counter()
        L.abpoa_collect_mm(None, ptrs, lens, n, para, C.byref(mm), mm_c)
        if n > 2:
            L.abpoa_build_guide_tree(para, n, C.byref(mm), order)
        spent += time.perf_counter() - t0
        libc.free(C.cast(mm.a, C.c_void_p))
        orders.append(list(order))
    return orders, spent


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sets", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from abpoa_amd import api, ffi, workloads
    # Everything that forks happens BEFORE the engine library is loaded and the GPU opened: the worker processes generate the reads and time the
    # reference on the host, and are gone when the parent initialises the device -- no child ever holds the GPU.
    have_ref = os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libabpoa_ref.so"))
    ref_got, ref_wall = None, 0.0
    with mp.Pool(CORES) as pool:
        sets = pool.map(_gen, range(a.sets), chunksize=8)
        if have_ref:
            share = [sets[i::CORES] for i in range(CORES)]
            pool.map(_ref_share, [s[:2] for s in share], chunksize=1)      # (load the library in every process)
            t0 = time.perf_counter()
            ref_got = pool.map(_ref_share, share, chunksize=1)
            ref_wall = time.perf_counter() - t0
    params = api.Params(**workloads.WORKLOADS["cfg2"]["params"])
    enc = api.EncodedSets(sets, params.m)
    ffi.check(ffi.lib().abpoa_hip_init(0))
    lines = [f"guide-tree order (-p) on {a.sets} read-sets x 50 reads x 1 kb (BASELINE.json configs[1] shape), global affine -O 4,0 -E 2, k = 19, w = 10",
             f"wall times: time.perf_counter around the call, median of {a.steps} steps after one warm-up step of each kind; kernel times: hipEvents on the pre-pass's queue"]

    def steps(progressive):
        api.msa_batch(None, params, encoded=enc, progressive=progressive)
        ts, gts = [], []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            res = api.msa_batch(None, params, encoded=enc, progressive=progressive)
            ts.append(time.perf_counter() - t0)
            assert all(r.status == 0 for r in res)
            gts.append(api.guide_timing())
        return ts, gts, api.msa_timing()["n_host_sets"]

    plain, _, host_plain = steps(False)
    flagged, gts, host_flag = steps(True)
    med = statistics.median
    sk, pr, tot = med(g["sketch_ms"] for g in gts), med(g["pair_ms"] for g in gts), med(g["total_s"] for g in gts) * 1e3
    lines += [f"step without the flag: median {med(plain) * 1e3:.1f} ms (min {min(plain) * 1e3:.1f}, max {max(plain) * 1e3:.1f}); sets on the host driver: {host_plain}",
              f"step with the flag:    median {med(flagged) * 1e3:.1f} ms (min {min(flagged) * 1e3:.1f}, max {max(flagged) * 1e3:.1f}); sets on the host driver: {host_flag}",
              f"ratio flagged / unflagged: {med(flagged) / med(plain):.3f}",
              f"device pre-pass inside the flagged step (medians): sketch kernel {sk:.2f} ms (count pass + write-and-sort pass), pair kernel {pr:.2f} ms, "
              f"whole pre-pass {tot:.1f} ms wall (packing the reads, copies, both kernels, hit matrices back, greedy order on the host); "
              f"{gts[-1]['n_minimizers']} minimizers"]
    t0 = time.perf_counter()
    dev = api.guide_order(None, params, encoded=enc)
    lines.append(f"abpoa_hip_guide_order alone: {(time.perf_counter() - t0) * 1e3:.1f} ms wall (pre-pass {api.guide_timing()['total_s'] * 1e3:.1f} ms)")
    changed = sum(g.order != list(range(len(g.order))) for g in dev)
    lines.append(f"sets whose order differs from the input order: {changed} of {a.sets}")
    if have_ref:
        got, wall = ref_got, ref_wall
        worst, total = max(s for _, s in got), sum(s for _, s in got)
        same = all(got[i % CORES][0][i // CORES] == dev[i].order for i in range(a.sets))
        lines += [f"reference on the host (abpoa_collect_mm + abpoa_build_guide_tree of libabpoa_ref.so, {CORES} processes, time inside the library only): "
                  f"slowest process {worst * 1e3:.1f} ms, all processes together {total * 1e3:.1f} ms = {total / a.sets * 1e3:.3f} ms per set on one core "
                  f"(wall of the pool with argument marshalling: {wall * 1e3:.0f} ms)",
                  f"orders identical to the reference's for every set: {same}",
                  f"condition (device pre-pass faster than the {CORES}-core host time): pre-pass {tot:.1f} ms vs {worst * 1e3:.1f} ms: {'met' if tot < worst * 1e3 else 'NOT met'}"]
        assert same, "device order differs from the reference's"
    else:
        lines.append("reference library not built here: no host comparison")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
