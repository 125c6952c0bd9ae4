"""Records the reference's guide-tree order (-p) as fixtures under tests/golden/guide_order/ (needs oracle/_ref: the compiled reference).

  sketch_*.npz / pairs_*.npz   one read-set each: the reads (residue codes), k, w, alphabet, strands; per read the sketch values the
                               reference's abpoa_collect_mm emits, sorted ascending; the triangular hit matrix counted from those values
                               (abpoa_seed.c:239-278: per distinct value the smaller multiplicity); the order of abpoa_build_guide_tree
  e2e.json                     printed outputs of `abpoa_ref -p ...` per read-set, with the arguments and the reads

    python tools/make_guide_order_golden.py            # rewrites every fixture (deterministic)
"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from abpoa_amd import seqio  # noqa: E402

REF_DIR = os.path.join(ROOT, "oracle", "_ref")
OUT_DIR = os.path.join(ROOT, "tests", "golden", "guide_order")
DATA = os.path.join(ROOT, "tests", "golden", "data")


def kernel_tile():
    """Positions per tile of the sketch kernel, from the built library (needs no GPU): the read lengths below are placed around it."""
    from abpoa_amd import ffi
    L = ffi.lib()
    L.abpoa_hip_guide_tile.restype = C.c_int
    return int(L.abpoa_hip_guide_tile())


class U128(C.Structure):
    _fields_ = [("x", C.c_uint64), ("y", C.c_uint64)]


class U128V(C.Structure):
    _fields_ = [("n", C.c_size_t), ("m", C.c_size_t), ("a", C.POINTER(U128))]


class Para(C.Structure):      # the head of abpoa_para_t (include/abpoa.h), up to the option bits
    _fields_ = [("m", C.c_int), ("mat", C.c_void_p), ("mat_fn", C.c_void_p), ("use_score_matrix", C.c_int),
                ("match", C.c_int), ("max_mat", C.c_int), ("mismatch", C.c_int), ("min_mis", C.c_int), ("gap_open1", C.c_int), ("gap_open2", C.c_int),
                ("gap_ext1", C.c_int), ("gap_ext2", C.c_int), ("inf_min", C.c_int), ("k", C.c_int), ("w", C.c_int), ("min_w", C.c_int),
                ("wb", C.c_int), ("wf", C.c_float), ("zdrop", C.c_int), ("end_bonus", C.c_int),
                ("ret_cigar", C.c_uint8, 1), ("rev_cigar", C.c_uint8, 1), ("out_msa", C.c_uint8, 1), ("out_cons", C.c_uint8, 1), ("out_gfa", C.c_uint8, 1),
                ("out_fq", C.c_uint8, 1), ("use_read_ids", C.c_uint8, 1), ("amb_strand", C.c_uint8, 1),
                ("use_qv", C.c_uint8, 1), ("disable_seeding", C.c_uint8, 1), ("progressive_poa", C.c_uint8, 1)]


_ref = None


def ref():
    global _ref
    if _ref is None:
        L = C.CDLL(os.path.join(REF_DIR, "libabpoa_ref.so"))
        L.abpoa_init_para.restype = C.POINTER(Para)
        L.abpoa_collect_mm.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_int), C.c_int, C.POINTER(Para), C.POINTER(U128V), C.POINTER(C.c_int)]
        L.abpoa_build_guide_tree.argtypes = [C.POINTER(Para), C.c_int, C.POINTER(U128V), C.POINTER(C.c_int)]
        _ref = L
    return _ref


def reference_guide(codes, m, k, w, both):
    """(per-read sorted sketch values, order) by the reference's own functions."""
    L = ref()
    n = len(codes)
    para = L.abpoa_init_para()
    para.contents.m, para.contents.k, para.contents.w, para.contents.amb_strand, para.contents.progressive_poa = m, k, w, int(both), 1
    arrs = [np.ascontiguousarray(c, np.uint8) for c in codes]
    ptrs = (C.POINTER(C.c_uint8) * n)(*[a.ctypes.data_as(C.POINTER(C.c_uint8)) for a in arrs])
    lens = (C.c_int * n)(*[len(a) for a in arrs])
    mm, mm_c = U128V(0, 0, None), (C.c_int * (n + 1))()
    L.abpoa_collect_mm(None, ptrs, lens, n, para, C.byref(mm), mm_c)
    xs = np.array([mm.a[i].x for i in range(mm.n)], np.uint64)
    for i in range(mm.n):
        assert mm.a[i].y >> 32 == next(r for r in range(n) if mm_c[r] <= i < mm_c[r + 1])
    sketch = [np.sort(xs[mm_c[r]:mm_c[r + 1]]) for r in range(n)]
    order = (C.c_int * n)(*range(n))
    if n > 2:
        L.abpoa_build_guide_tree(para, n, C.byref(mm), order)      # (sorts mm in place: the sketches were taken before)
    return sketch, list(order)


def hit_matrix(sketch):
    n = len(sketch)
    hit = np.zeros(n * (n + 1) // 2, np.int32)
    cnt = [dict(zip(*np.unique(s, return_counts=True))) for s in sketch]
    for i in range(n):
        hit[i * (i + 1) // 2 + i] = len(sketch[i])
        for j in range(i):
            a, b = (cnt[i], cnt[j]) if len(cnt[i]) <= len(cnt[j]) else (cnt[j], cnt[i])
            hit[i * (i + 1) // 2 + j] = sum(min(c, b[x]) for x, c in a.items() if x in b)
    return hit


def save_case(name, codes, m=5, k=19, w=10, both=False, tile=0, min_longest=0):
    """tile: the kernel's tile length the read lengths were placed around (0: not such a case); min_longest: what the longest sketch must exceed."""
    sketch, order = reference_guide(codes, m, k, w, both)
    assert not min_longest or max(len(s) for s in sketch) > min_longest, (name, max(len(s) for s in sketch))
    lens = np.array([len(c) for c in codes], np.int32)
    np.savez_compressed(os.path.join(OUT_DIR, name + ".npz"), m=m, k=k, w=w, both=int(both), tile=tile, lens=lens,
                        reads=np.concatenate([np.asarray(c, np.uint8) for c in codes]) if codes else np.zeros(0, np.uint8),
                        mm_len=np.array([len(s) for s in sketch], np.int64), mm=np.concatenate(sketch) if sketch else np.zeros(0, np.uint64),
                        hit=hit_matrix(sketch), order=np.array(order, np.int32))
    print(f"{name}: {len(codes)} reads, {sum(len(s) for s in sketch)} minimizers, order {order[:12]}{'...' if len(order) > 12 else ''}")


def family(rng, n, length, err=0.08, n_codes=4, clusters=1):
    """n noisy copies of `clusters` random ancestors (substitutions, insertions, deletions), lengths cut to `length` (an int or a list)."""
    roots = [rng.integers(0, n_codes, 2 * (max(length) if isinstance(length, list) else length) + 64).astype(np.uint8) for _ in range(clusters)]
    reads = []
    for i in range(n):
        want = length[i] if isinstance(length, list) else length
        src, out = roots[int(rng.integers(0, clusters))], []
        for b in src:
            u = rng.random()
            if u < err / 3:
                continue
            if u < 2 * err / 3:
                out.append(int(rng.integers(0, n_codes)))
            out.append(int(rng.integers(0, n_codes)) if u > 1 - err / 3 else int(b))
        reads.append(np.array(out[:want], np.uint8))
        assert len(reads[-1]) == want
    return reads


def sketch_cases():
    rng = np.random.default_rng(20240521)
    k, w = 19, 10
    TILE = kernel_tile()
    # read lengths around every edge of the walk: nothing / one value / the first full window; the last k-mer at lanes 63, 64, 65; the tile +-1; 1 kb; 2+ tiles
    lens = [k - 1, k, w + k - 2, w + k - 1, w + k, 63 + 1, 64 + 1, 65 + 1, 63 + k, 64 + k, 65 + k, TILE - 1, TILE, TILE + 1, TILE + k - 1, TILE + w + k, 1000, 2 * TILE + 200]
    save_case("sketch_lengths", family(rng, len(lens), lens, err=0.05), tile=TILE)
    # read content
    base = family(rng, 1, 150, err=0.0)[0]

    def with_n(at):
        r = base.copy(); r[at] = 4; return r
    content = [with_n([0]), with_n([75]), with_n([149]), with_n(list(range(60, 67))), with_n([0, 1, 2, 30, 31, 90, 148, 149]), with_n(list(range(40, 40 + 19))),
               np.zeros(150, np.uint8), np.full(300, 2, np.uint8), np.tile(np.array([0, 1], np.uint8), 80), np.tile(np.array([2, 3, 0], np.uint8), 60),
               np.tile(np.array([0, 1], np.uint8), 200)[:TILE + 37], np.concatenate([np.zeros(40, np.uint8), base[:50], np.zeros(40, np.uint8)]), base.copy()]
    save_case("sketch_content", content)
    save_case("sketch_content_k4w3", content, k=4, w=3)
    save_case("sketch_content_k6w12", content, k=6, w=12)
    # both strands, k-mers equal to their own reverse complement (ACGT, GAATTC): those positions never reach the ring
    acgt, gaattc = seqio.encode("ACGT", 5), seqio.encode("GAATTC", 5)
    pal = []
    for i in range(10):
        r = family(rng, 1, 120 + 37 * i, err=0.0)[0]
        for at in range(5 + i, len(r) - 8, 17 + i):
            r[at:at + 4] = acgt
        for at in range(11, len(r) - 8, 29 + i):
            r[at:at + 6] = gaattc
        if i % 3 == 0:
            r[50] = 4
        pal.append(r)
    pal += [np.tile(acgt, 40), np.tile(gaattc, 30), np.tile(np.array([0, 3], np.uint8), 150), seqio.encode("ACGT", 5), seqio.encode("GAATTCGAATTC", 5)]
    for kk, ww in ((4, 3), (4, 10), (6, 3), (6, 10), (19, 10)):
        save_case(f"sketch_both_k{kk}w{ww}", pal, k=kk, w=ww, both=True)
    # parameters at their limits
    par = family(rng, 6, [40, 300, 600, 1000, 275, 273], err=0.06) + [with_n([3, 77]), np.zeros(700, np.uint8)]
    for kk, ww in ((1, 10), (28, 10), (19, 1), (19, 255), (1, 1), (28, 255)):
        save_case(f"sketch_k{kk}w{ww}", par, k=kk, w=ww)
        if (kk, ww) in ((1, 10), (28, 10)):
            save_case(f"sketch_both_k{kk}w{ww}", par, k=kk, w=ww, both=True)
    aa = family(rng, 8, [6, 7, 10, 11, 60, 300, 257, 600], err=0.06, n_codes=20)
    aa[4][10] = 26; aa[5][0] = 26; aa[5][100:104] = 26; aa[6][256] = 26
    aa.append(np.full(100, 7, np.uint8))
    save_case("sketch_aa_k7w4", aa, m=27, k=7, w=4)
    save_case("sketch_aa_k11w10", aa, m=27, k=11, w=10)
    save_case("sketch_aa_k1w255", aa, m=27, k=1, w=255)


def long_cases():
    """Sketches of more than 2 048 values (the kernel sorts those in place instead of in the LDS): 12 / 15 kb at the defaults, 3 kb at w = 1."""
    rng = np.random.default_rng(3301)
    reads = family(rng, 3, [15000, 12000, 3000], err=0.05)
    reads[0][7000:7003] = 4
    save_case("sketch_long_k19w10", reads, min_longest=2048)
    save_case("sketch_long_both_k19w10", reads[:2], both=True, min_longest=2048)
    save_case("sketch_long_k19w1", [reads[2], reads[1][:2500]], w=1, min_longest=2048)
    save_case("sketch_long_k4w1", [reads[2], np.tile(np.array([0, 1, 2], np.uint8), 1200)], k=4, w=1, min_longest=2048)


def pair_cases():
    rng = np.random.default_rng(977)
    save_case("pairs_n2", family(rng, 2, 200))
    save_case("pairs_n3", family(rng, 3, 200, clusters=2))
    save_case("pairs_n64", family(rng, 64, 120, err=0.06, clusters=3))
    save_case("pairs_n65", family(rng, 65, 120, err=0.06, clusters=3))
    save_case("pairs_n50x1k", family(rng, 50, 1000, err=0.08, clusters=2))
    d = family(rng, 6, 300, err=0.08, clusters=2)
    save_case("pairs_duplicates", [d[0], d[1], d[0].copy(), d[2], d[1].copy(), d[0].copy(), d[3], d[4], d[5]])
    s = family(rng, 5, 250, err=0.05)
    save_case("pairs_short_read", [s[0], s[1][:12], s[2], s[3], s[4][:18]])
    save_case("pairs_all_short", [x[:n] for x, n in zip(family(rng, 5, 18), (18, 5, 12, 1, 17))])
    save_case("pairs_no_minimizer_read", [s[0], np.full(90, 4, np.uint8), s[1], s[2]])
    for nm in ("seq", "heter", "test"):
        _, reads, _ = seqio.read_fastx(os.path.join(DATA, nm + ".fa"))
        save_case("pairs_" + nm, [seqio.encode(r, 5) for r in reads])
    _, reads, _ = seqio.read_fastx(os.path.join(DATA, "heter.fa"))
    save_case("pairs_heter_k15w5", [seqio.encode(r, 5) for r in reads], k=15, w=5)
    save_case("pairs_heter_both", [seqio.encode(r, 5) for r in reads], both=True)


def run_ref(args, path):
    p = subprocess.run([os.path.join(REF_DIR, "abpoa_ref"), *args, path], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (args, p.stderr[-2000:])
    return p.stdout


def e2e_cases():
    rng = np.random.default_rng(4242)
    cases = []

    def add(name, args, file=None, reads=None, fastq=None):
        with tempfile.TemporaryDirectory() as td:
            path = os.path.join(ROOT, "tests", "golden", file) if file else os.path.join(td, "in.fa")
            if reads is not None:
                with open(path, "w") as f:
                    for i, r in enumerate(reads):
                        f.write(f">r{i}\n{r}\n")
            out = run_ref(["-p", *args], path)
            plain = run_ref(args, path)
        cases.append(dict(name=name, args=args, file=file, reads=reads, output=out, differs_from_input_order=out != plain))

    for nm in ("seq", "heter"):
        for r in ("0", "1", "2"):
            add(f"{nm}_r{r}", ["-r", r], file=f"data/{nm}.fa")
            add(f"{nm}_r{r}_s", ["-r", r, "-s"], file=f"data/{nm}.fa")
    add("test_r2", ["-r", "2"], file="data/test.fa")
    add("heter_k15w5_r2", ["-r", "2", "-k", "15", "-w", "5"], file="data/heter.fa")
    add("heter_affine_r0", ["-r", "0", "-O", "4,0", "-E", "2"], file="data/heter.fa")
    add("fastq_Q_r2", ["-r", "2", "-Q"], file="out_qv_cons/input.fq")
    add("fastq_Q_r0", ["-r", "0", "-Q", "-O", "4,0", "-E", "2"], file="out_qv_cons/input.fq")
    add("heter_linear_r2", ["-r", "2", "-O", "0,0", "-E", "2,0"], file="data/heter.fa")
    add("heter_local_r2", ["-r", "2", "-m", "1"], file="data/heter.fa")
    dec = lambda rs: [seqio.decode(r, 5) for r in rs]      # noqa: E731
    # one job of the test: 2-read sets beside larger ones
    for i, n in enumerate((2, 7, 2, 12)):
        add(f"mixed_{i}", ["-r", "2"], reads=dec(family(rng, n, 160 + 10 * i, err=0.08, clusters=2)))
    for i, n in enumerate((2, 9, 5)):
        add(f"mixed_cons_{i}", ["-r", "0", "-O", "4,0", "-E", "2"], reads=dec(family(rng, n, 220, err=0.08, clusters=2)))
    # ragged sets: read lengths far apart
    add("ragged_r2", ["-r", "2"], reads=dec(family(rng, 8, [600, 250, 580, 300, 610, 200, 590, 420], err=0.06)))
    add("ragged_cons", ["-r", "0", "-O", "4,0", "-E", "2"], reads=dec(family(rng, 8, [600, 250, 580, 300, 610, 200, 590, 420], err=0.06)))
    with open(os.path.join(OUT_DIR, "e2e.json"), "w") as f:
        json.dump(dict(cases=cases), f, indent=0)
    print("e2e:", len(cases), "cases;", sum(c["differs_from_input_order"] for c in cases), "differ from the input-order run")


if __name__ == "__main__":
    os.makedirs(OUT_DIR, exist_ok=True)
    sketch_cases()
    long_cases()
    pair_cases()
    e2e_cases()
