"""Host-side mirror of the reference's parameter block and thin wrappers over the C-ABI.

`Params` mirrors abpoa_para_t (ref src/abpoa.h:62-81) with the defaults of abpoa_init_para
(src/abpoa_align.c:93-141) and the derived fields of abpoa_post_set_para (:143-168)."""
import ctypes as C
from collections.abc import Sequence

import numpy as np

from . import ffi, seqio

GLOBAL, LOCAL, EXTEND = 0, 1, 2
LINEAR, AFFINE, CONVEX = 0, 1, 2
OUT_CONS, OUT_MSA, AMB_STRAND, PROGRESSIVE, OUT_GFA = 1, 2, 4, 8, 0x10
GUIDE_HITS, GUIDE_SKETCH = 0x01000000, 0x02000000


def guide_kw(k=0, w=0):
    """ABPOA_HIP_GUIDE_KW: the sketch's k-mer size in flag bits 8-15, its window in bits 16-23 (0: the reference's default)."""
    if not (0 <= int(k) <= 255 and 0 <= int(w) <= 255):
        raise ValueError("guide order: k and w are 8-bit fields (valid: k 1..28, amino acids 1..11; w 1..255; 0 = default)")
    return int(k) << 8 | int(w) << 16


def check_guide_kw(k, w, is_aa=False):
    """What the library accepts (abpoa_hip_msa_batch returns ABPOA_HIP_EINVAL for the rest): k 0 or 1..28 (amino acids 1..11), w 0 or 1..255."""
    if not (k == 0 or 1 <= k <= (11 if is_aa else 28)) or not (0 <= w <= 255):
        raise ValueError(f"guide order: k = {k}, w = {w} outside k 1..{11 if is_aa else 28}, w 1..255")
    return guide_kw(k, w)


def _batch_flags(params, out_cons, out_msa, amb_strand, progressive, mm_k, mm_w, out_gfa=False):
    flags = (OUT_CONS if out_cons else 0) | (OUT_MSA if out_msa else 0) | (AMB_STRAND if amb_strand else 0) | (OUT_GFA if out_gfa else 0)
    if progressive:
        flags |= PROGRESSIVE | check_guide_kw(mm_k, mm_w, params.m > 5)
    return flags


class ReadSet(C.Structure):          # abpoa_hip_readset_t
    _fields_ = [("n_reads", C.c_int32), ("seqs", C.POINTER(C.POINTER(C.c_uint8))), ("lens", C.POINTER(C.c_int32)),
                ("weights", C.POINTER(C.POINTER(C.c_int32)))]


class Guide(C.Structure):            # abpoa_hip_guide_t
    _fields_ = [("status", C.c_int32), ("n_reads", C.c_int32), ("order", C.POINTER(C.c_int32)), ("hit", C.POINTER(C.c_int32)),
                ("mm_off", C.POINTER(C.c_int64)), ("mm", C.POINTER(C.c_uint64))]


class GuideTiming(C.Structure):      # abpoa_hip_guide_timing_t
    _fields_ = [("sketch_ms", C.c_double), ("pair_ms", C.c_double), ("total_s", C.c_double), ("n_minimizers", C.c_int64)]


class Gfa(C.Structure):              # abpoa_hip_gfa_t
    _fields_ = [("n_seg", C.c_int32), ("n_link", C.c_int32), ("n_path", C.c_int32), ("seg_node", C.POINTER(C.c_int32)), ("seg_base", C.POINTER(C.c_uint8)),
                ("link_off", C.POINTER(C.c_int32)), ("link_from", C.POINTER(C.c_int32)), ("path_off", C.POINTER(C.c_int64)), ("path_node", C.POINTER(C.c_int32))]


class Msa(C.Structure):              # abpoa_hip_msa_t
    _fields_ = [("status", C.c_int32), ("n_reads", C.c_int32), ("cons_len", C.c_int32),
                ("cons_base", C.POINTER(C.c_uint8)), ("cons_cov", C.POINTER(C.c_int32)), ("cons_node_id", C.POINTER(C.c_int32)),
                ("msa_len", C.c_int32), ("msa_rows", C.c_int32), ("msa_base", C.POINTER(C.c_uint8)), ("n_cells", C.c_int64),
                ("is_rc", C.POINTER(C.c_uint8)), ("gfa", C.POINTER(Gfa))]


class MsaTiming(C.Structure):        # abpoa_hip_msa_timing_t
    _fields_ = [("host_sort_s", C.c_double), ("host_fuse_s", C.c_double), ("engine_s", C.c_double), ("cons_s", C.c_double),
                ("total_s", C.c_double), ("n_rounds", C.c_int32), ("n_threads", C.c_int32), ("n_groups", C.c_int32), ("n_host_sets", C.c_int32)]


class Params:
    def __init__(self, aln_mode=GLOBAL, is_aa=False, match=2, mismatch=4, score_matrix=None, gap_open1=4, gap_open2=24,
                 gap_ext1=2, gap_ext2=1, extra_b=10, extra_f=0.01, zdrop=-1):
        self.align_mode, self.m = aln_mode, (27 if is_aa else 5)
        self.match, self.mismatch, self.mat_fn = match, mismatch, score_matrix
        self.gap_open1, self.gap_open2, self.gap_ext1, self.gap_ext2 = gap_open1, gap_open2, gap_ext1, gap_ext2
        self.wb, self.wf, self.zdrop = extra_b, extra_f, zdrop
        self.finalize()

    def finalize(self):
        """abpoa_post_set_para: gap mode from the open penalties, LOCAL disables the band, matrix."""
        if self.gap_open1 == 0:
            self.gap_mode = LINEAR
        elif self.gap_open1 > 0 and self.gap_open2 == 0:
            self.gap_mode = AFFINE
        else:
            self.gap_mode = CONVEX
        if self.align_mode == LOCAL:
            self.wb = -1
        if self.mat_fn:
            self.mat, self.max_mat, self.min_mis = seqio.matrix_from_file(self.mat_fn, self.m)
        else:
            self.mat, self.max_mat, self.min_mis = seqio.simple_matrix(self.m, self.match, self.mismatch)
        self.mat = np.ascontiguousarray(self.mat, np.int32)
        return self

    def scoring(self):
        return ffi.Scoring(self.m, self.mat.ctypes.data_as(C.POINTER(C.c_int32)), self.max_mat, self.min_mis, self.gap_open1,
                           self.gap_ext1, self.gap_open2, self.gap_ext2, self.align_mode, self.gap_mode, self.wb,
                           float(self.wf), self.zdrop, 1, 0)


class GfaView:
    """The arrays of one abpoa_hip_gfa_t (include/abpoa_hip.h): ids are the printed ones, node id - 1."""
    __slots__ = ("n_seg", "n_link", "n_path", "seg_node", "seg_base", "link_off", "link_from", "path_off", "path_node")

    def __init__(self, *v):
        for k, x in zip(self.__slots__, v):
            setattr(self, k, x)


class _BatchOut:
    """Owns the result records of one abpoa_hip_msa_batch call; the library's arrays are released when the last SetResult goes."""
    __slots__ = ("lib", "out", "n")

    def __init__(self, lib, out, n):
        self.lib, self.out, self.n = lib, out, n

    def __del__(self):
        try:
            if hasattr(self.lib, "abpoa_hip_free_msa_array"):
                self.lib.abpoa_hip_free_msa_array(self.out, self.n)
            else:
                free_msa, out = self.lib.abpoa_hip_free_msa, self.out
                for i in range(self.n):
                    free_msa(C.byref(out[i]))
        except Exception:      # interpreter shutdown: the library may already be gone
            pass


class SetResult:
    """Result of one read-set: a view of the library's record.  Strings / lists are built on first access (building 1000 Python
    strings and coverage lists eagerly costs more than the whole GPU job of a batch)."""
    __slots__ = ("_o", "_owner", "_m", "_cons_seq", "_cov_list", "_msa_seq", "_gfa")

    def __init__(self, owner, rec, m):
        self._owner, self._o, self._m = owner, rec, m
        self._cons_seq = self._cov_list = self._msa_seq = self._gfa = None

    status = property(lambda self: self._o.status)
    is_rc = property(lambda self: [bool(self._o.is_rc[i]) for i in range(self._o.n_reads)] if self._o.is_rc else [False] * self._o.n_reads)
    n_cells = property(lambda self: self._o.n_cells)
    cons_len = property(lambda self: self._o.cons_len)
    msa_len = property(lambda self: self._o.msa_len)

    @property
    def cons_seq(self):
        if self._cons_seq is None:
            n = self._o.cons_len
            self._cons_seq = seqio.decode(np.frombuffer(C.string_at(self._o.cons_base, n), dtype=np.uint8), self._m) if n > 0 else ""
        return self._cons_seq

    @property
    def cons_cov(self):
        if self._cov_list is None:
            n = self._o.cons_len
            self._cov_list = np.frombuffer(C.string_at(self._o.cons_cov, 4 * n), dtype=np.int32).tolist() if n > 0 else []
        return self._cov_list

    @property
    def cons_node_id(self):
        n = self._o.cons_len
        return np.frombuffer(C.string_at(self._o.cons_node_id, 4 * n), dtype=np.int32) if n > 0 else np.zeros(0, np.int32)

    @property
    def gfa(self):
        """abpoa_hip_gfa_t as numpy arrays (out_gfa=True), else None: n_seg, n_link, n_path, seg_node, seg_base, link_off, link_from, path_off, path_node."""
        if self._gfa is None and self._o.gfa:
            g = self._o.gfa.contents

            def arr(ptr, n, dt):
                return np.frombuffer(C.string_at(ptr, n * np.dtype(dt).itemsize), dtype=dt) if n > 0 else np.zeros(0, dt)
            n_pn = int(g.path_off[g.n_path]) if g.n_path > 0 else 0
            self._gfa = GfaView(g.n_seg, g.n_link, g.n_path, arr(g.seg_node, g.n_seg, np.int32), arr(g.seg_base, g.n_seg, np.uint8),
                                arr(g.link_off, g.n_seg + 1, np.int32), arr(g.link_from, g.n_link, np.int32), arr(g.path_off, g.n_path + 1, np.int64),
                                arr(g.path_node, n_pn, np.int32))
        return self._gfa

    @property
    def msa_seq(self):
        if self._msa_seq is None:
            o = self._o
            if o.msa_len > 0:
                rows = np.frombuffer(C.string_at(o.msa_base, o.msa_rows * o.msa_len), dtype=np.uint8).reshape(o.msa_rows, o.msa_len)
                self._msa_seq = [seqio.decode(row, self._m) for row in rows]
            else:
                self._msa_seq = []
        return self._msa_seq


class BatchResults(Sequence):
    """The results of one batch call as a read-only sequence of SetResult; the objects are made on first access (1000 of them cost
    more Python time than the call's own host work)."""
    __slots__ = ("_owner", "_m", "_items")

    def __init__(self, owner, m):
        self._owner, self._m, self._items = owner, m, [None] * owner.n

    def __len__(self):
        return len(self._items)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self._items)))]
        r = self._items[i]
        if r is None:
            if i < 0:
                i += len(self._items)
            r = self._items[i] = SetResult(self._owner, self._owner.out[i], self._m)
        return r


def _bind_msa(lib):
    if not getattr(lib, "_msa_bound", False):
        lib.abpoa_hip_msa_batch.argtypes = [C.POINTER(ffi.Scoring), C.c_int, C.POINTER(ReadSet), C.POINTER(Msa), C.c_uint, C.c_int]
        lib.abpoa_hip_msa_batch.restype = C.c_int
        lib.abpoa_hip_free_msa.argtypes = [C.POINTER(Msa)]
        if hasattr(lib, "abpoa_hip_free_msa_array"):
            lib.abpoa_hip_free_msa_array.argtypes = [C.POINTER(Msa), C.c_int]
            lib.abpoa_hip_free_msa_array.restype = None
        lib.abpoa_hip_get_msa_timing.argtypes = [C.POINTER(MsaTiming)]
        lib._msa_bound = True


class EncodedSets:
    """Read-sets encoded once into residue codes and laid out for abpoa_hip_msa_batch (kept alive on self)."""

    def __init__(self, read_sets, m=5, weights=None):
        """weights: None, or per set a list of per-read integer sequences (the reference's qv weights with -Q: seqio.qv_weights).
        A read given as a numpy uint8 array is taken as residue codes already (seqio.encode done elsewhere, e.g. in a generator process)."""
        self.n = len(read_sets)
        self.codes = [[np.ascontiguousarray(r if isinstance(r, np.ndarray) and r.dtype == np.uint8 else seqio.encode(r, m)) for r in rs] for rs in read_sets]
        self.sets = (ReadSet * self.n)()
        self._keep = []
        for i, rs in enumerate(self.codes):
            ptrs = (C.POINTER(C.c_uint8) * len(rs))(*[a.ctypes.data_as(C.POINTER(C.c_uint8)) for a in rs])
            lens = (C.c_int32 * len(rs))(*[len(a) for a in rs])
            wptrs = None
            if weights is not None and weights[i] is not None:
                ws = [np.ascontiguousarray(w, np.int32) for w in weights[i]]
                assert all(len(w) == len(a) for w, a in zip(ws, rs)), "one weight per base"
                wptrs = (C.POINTER(C.c_int32) * len(rs))(*[w.ctypes.data_as(C.POINTER(C.c_int32)) for w in ws])
                self._keep.append(ws)
            self._keep.append((ptrs, lens, wptrs))
            self.sets[i] = ReadSet(len(rs), ptrs, lens, wptrs)


def msa_batch(read_sets, params, out_cons=True, out_msa=False, n_threads=0, lib=None, encoded=None, weights=None, amb_strand=False,
              progressive=False, mm_k=0, mm_w=0, out_gfa=False):
    """Consensus / MSA of many independent read-sets (lists of strings) in one call.
    Returns a list of SetResult.  `lib` defaults to the HIP engine (tests may pass the CPU shim).
    weights: per set, per read, per base edge weights (the reference's -Q); amb_strand: the reference's -s;
    progressive: the reference's -p, reads aligned in guide-tree order (mm_k / mm_w: its -k / -w, 0 = default);
    out_gfa: the graph as the reference's GFA output walks it (SetResult.gfa, format_gfa); the consensus then only with out_cons."""
    lib = lib or ffi.lib()
    _bind_msa(lib)
    enc = encoded or EncodedSets(read_sets, params.m, weights)
    out = (Msa * enc.n)()
    sc = params.scoring()
    flags = _batch_flags(params, out_cons, out_msa, amb_strand, progressive, mm_k, mm_w, out_gfa)
    rc = lib.abpoa_hip_msa_batch(C.byref(sc), enc.n, enc.sets, out, flags, n_threads)
    if rc != 0:
        raise ffi.EngineError(f"abpoa_hip_msa_batch failed ({rc}): {lib.abpoa_hip_last_error().decode() if hasattr(lib, 'abpoa_hip_last_error') else ''}")
    res = BatchResults(_BatchOut(lib, out, enc.n), params.m)
    return res


class BatchContext:
    """abpoa_hip_ctx_t: the batch entry with per-caller state (own device queue, timing, last error): one host thread per context may call while others do."""

    def __init__(self, device=-1, lib=None):
        self.lib = lib or ffi.lib()
        _bind_msa(self.lib)
        self.lib.abpoa_hip_ctx_create.restype = C.c_void_p
        self.lib.abpoa_hip_ctx_create.argtypes = [C.c_int]
        self.lib.abpoa_hip_ctx_destroy.argtypes = [C.c_void_p]
        self.lib.abpoa_hip_msa_batch_ctx.argtypes = [C.c_void_p, C.POINTER(ffi.Scoring), C.c_int, C.POINTER(ReadSet), C.POINTER(Msa), C.c_uint, C.c_int]
        self.lib.abpoa_hip_msa_batch_ctx.restype = C.c_int
        self.lib.abpoa_hip_ctx_get_msa_timing.argtypes = [C.c_void_p, C.POINTER(MsaTiming)]
        self.lib.abpoa_hip_ctx_last_error.restype = C.c_char_p
        self.lib.abpoa_hip_ctx_last_error.argtypes = [C.c_void_p]
        self.h = self.lib.abpoa_hip_ctx_create(device)
        if not self.h:
            raise ffi.EngineError("abpoa_hip_ctx_create failed: " + self.lib.abpoa_hip_last_error().decode())

    def close(self):
        if self.h:
            self.lib.abpoa_hip_ctx_destroy(self.h)
            self.h = None

    __del__ = close

    def msa_batch(self, read_sets, params, out_cons=True, out_msa=False, n_threads=0, encoded=None, weights=None, amb_strand=False, progressive=False,
                  mm_k=0, mm_w=0, out_gfa=False):
        enc = encoded or EncodedSets(read_sets, params.m, weights)
        out = (Msa * enc.n)()
        sc = params.scoring()
        flags = _batch_flags(params, out_cons, out_msa, amb_strand, progressive, mm_k, mm_w, out_gfa)
        rc = self.lib.abpoa_hip_msa_batch_ctx(self.h, C.byref(sc), enc.n, enc.sets, out, flags, n_threads)
        if rc != 0:
            raise ffi.EngineError(f"abpoa_hip_msa_batch_ctx failed ({rc}): {self.lib.abpoa_hip_ctx_last_error(self.h).decode()}")
        return BatchResults(_BatchOut(self.lib, out, enc.n), params.m)

    def timing(self):
        t = MsaTiming()
        self.lib.abpoa_hip_ctx_get_msa_timing(self.h, C.byref(t))
        return {k: getattr(t, k) for k, _ in MsaTiming._fields_}


def msa_timing(lib=None):
    lib = lib or ffi.lib()
    _bind_msa(lib)
    t = MsaTiming()
    lib.abpoa_hip_get_msa_timing(C.byref(t))
    d = {k: getattr(t, k) for k, _ in MsaTiming._fields_}
    d["pad"] = d["n_host_sets"]          # (the field's name before round 4)
    return d


class GuideOrder:
    """The pre-pass's result for one read-set: order[r] = read aligned in round r; hit = the triangular matrix as a list (or None);
    sketch = per read the ascending minimizer values as numpy uint64 arrays (or None)."""
    __slots__ = ("order", "hit", "sketch")

    def __init__(self, order, hit, sketch):
        self.order, self.hit, self.sketch = order, hit, sketch


def guide_order(read_sets, params, mm_k=0, mm_w=0, both_strands=False, hits=False, sketch=False, lib=None, encoded=None):
    """abpoa_hip_guide_order: the guide-tree order (-p) of every read-set alone, computed by the device pre-pass."""
    lib = lib or ffi.lib()
    lib.abpoa_hip_guide_order.argtypes = [C.POINTER(ffi.Scoring), C.c_int, C.POINTER(ReadSet), C.c_uint, C.POINTER(Guide)]
    lib.abpoa_hip_guide_order.restype = C.c_int
    lib.abpoa_hip_free_guide.argtypes = [C.POINTER(Guide), C.c_int]
    lib.abpoa_hip_free_guide.restype = None
    enc = encoded or EncodedSets(read_sets, params.m)
    out = (Guide * enc.n)()
    sc = params.scoring()
    flags = check_guide_kw(mm_k, mm_w, params.m > 5) | (AMB_STRAND if both_strands else 0) | (GUIDE_HITS if hits else 0) | (GUIDE_SKETCH if sketch else 0)
    rc = lib.abpoa_hip_guide_order(C.byref(sc), enc.n, enc.sets, flags, out)
    if rc != 0:
        raise ffi.EngineError(f"abpoa_hip_guide_order failed ({rc}): {lib.abpoa_hip_last_error().decode()}")
    try:
        res = []
        for i in range(enc.n):
            o, n = out[i], out[i].n_reads
            order = [o.order[r] for r in range(n)]
            hit = np.ctypeslib.as_array(o.hit, (n * (n + 1) // 2,)).tolist() if hits and n else ([] if hits else None)
            sk = None
            if sketch:
                off = [o.mm_off[r] for r in range(n + 1)]
                vals = np.ctypeslib.as_array(o.mm, (max(1, off[-1]),)).copy()
                sk = [vals[off[r]:off[r + 1]] for r in range(n)]
            res.append(GuideOrder(order, hit, sk))
        return res
    finally:
        lib.abpoa_hip_free_guide(out, enc.n)


def guide_timing(lib=None):
    """Kernel durations (ms), wall time (s) and minimizer count of the last guide-order pre-pass."""
    lib = lib or ffi.lib()
    t = GuideTiming()
    lib.abpoa_hip_get_guide_timing.argtypes = [C.POINTER(GuideTiming)]
    lib.abpoa_hip_get_guide_timing.restype = None
    lib.abpoa_hip_get_guide_timing(C.byref(t))
    return {k: getattr(t, k) for k, _ in GuideTiming._fields_}


HOST_REASONS = ["other", "node slots at the first read", "predecessor-list slots", "cigar slots", "node slots while fusing", "edge / aligned slots of a node",
                "projected graph growth", "row-order walk", "MSA rank walk", "DP arena too small for the bands", "other DP status", "job options / pass did not fit"]


def host_reasons(lib=None):
    """{reason: sets} for the read-sets the last msa_batch call handed to the host driver (abpoa_hip_get_host_reasons)."""
    lib = lib or ffi.lib()
    a = (C.c_int32 * len(HOST_REASONS))()
    lib.abpoa_hip_get_host_reasons.argtypes = [C.POINTER(C.c_int32)]
    lib.abpoa_hip_get_host_reasons.restype = None
    lib.abpoa_hip_get_host_reasons(a)
    return {HOST_REASONS[i]: int(a[i]) for i in range(len(HOST_REASONS)) if a[i]}


def format_output(result, names=None, out_cons=True, out_msa=False):
    """Text exactly as the reference prints it: abpoa_output_rc_msa (src/abpoa_output.c:70-101) when MSA is
    requested, else abpoa_output_fx_consensus (:495-512), single consensus."""
    lines = []
    if out_msa:
        if result.msa_len <= 0:
            return ""
        n_reads = len(result.msa_seq) - (1 if out_cons else 0)
        rc = result.is_rc
        for i in range(n_reads):
            nm = names[i] if names and i < len(names) and names[i] else None
            lines.append((f">{nm}" if nm else f">Seq_{i + 1}") + ("_reverse_complement" if rc[i] else ""))      # src/abpoa_output.c:77
            lines.append(result.msa_seq[i])
        if out_cons:
            lines.append(">Consensus_sequence")
            lines.append(result.msa_seq[-1])
    elif out_cons:
        lines.append(">Consensus_sequence")
        lines.append(result.cons_seq)
    return "\n".join(lines) + "\n"


def format_gfa(result, names=None, out_cons=False):
    """Text exactly as the reference prints a graph as GFA (abpoa_generate_gfa, src/abpoa_output.c:168-268; -r 3, with out_cons -r 4) from
    SetResult.gfa: header, S / L lines in walk order, a P line per read (reversed with '-' where the read went in as its reverse complement)
    and with out_cons the consensus path.  "" for an empty graph."""
    g = result.gfa
    if g is None or g.n_seg <= 0:
        return ""
    letters = seqio.AA_DECODE if result._m > 5 else seqio.NT_DECODE
    out = ["H\tVN:Z:1.0\tNS:i:%d\tNL:i:%d\tNP:i:%d\n" % (g.n_seg, g.n_link, g.n_path + (1 if out_cons else 0))]
    seg, base, lo, lf = g.seg_node.tolist(), g.seg_base.tolist(), g.link_off.tolist(), g.link_from.tolist()
    for i, u in enumerate(seg):
        out.append("S\t%d\t%s\n" % (u, letters[base[i]]))
        for k in range(lo[i], lo[i + 1]):
            out.append("L\t%d\t+\t%d\t+\t0M\n" % (lf[k], u))
    po, rc = g.path_off.tolist(), result.is_rc
    for i in range(g.n_path):
        nm = names[i] if names and i < len(names) and names[i] else str(i + 1)
        p = g.path_node[po[i]:po[i + 1]].tolist()
        if rc[i]:
            body = ",".join("%d-" % x for x in reversed(p))
        else:
            body = ",".join("%d+" % x for x in p)
        out.append("P\t%s\t%s" % (nm, body + "\t*\n" if p else ""))
    if out_cons:
        ids = result.cons_node_id.tolist()
        out.append("P\tConsensus_sequence\t" + (",".join("%d+" % (x - 1) for x in ids) + "\t*\n" if ids else ""))
    return "".join(out)
