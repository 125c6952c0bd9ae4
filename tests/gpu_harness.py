"""What the GPU tests (tests/test_gpu_*.py) share: the `engine` fixture, wrappers of the library's test hooks that own their ctypes prototypes, and the one
way to send a launch through the flat C-ABI and hold every alignment to the oracle.  helpers.py has the plumbing both the CPU and the GPU tests use; the child
process of the read-set tests is tests/readset_worker.py.  A plain module: a test module takes what it needs with `from gpu_harness import engine, ...`."""
import ctypes as C

import numpy as np
import pytest

import helpers as H


@pytest.fixture(scope="module")
def engine():
    from abpoa_amd import ffi
    lib = ffi.lib()
    assert lib.abpoa_hip_device_count() >= 1, "no HIP device: the engine has no fallback"
    ffi.check(lib.abpoa_hip_init(0))
    return lib


# ---------------------------------------------------------------- test hooks (abpoa_hip__*: exported for the tests, not part of include/abpoa_hip.h)
_U8P = C.POINTER(C.c_uint8)


def dir_counts(lib):
    """(alignments whose backtrack walked the direction plane, alignments redone with score records) since the last call; the call zeroes both."""
    out = (C.c_longlong * 2)()
    lib.abpoa_hip__dir_counts.argtypes, lib.abpoa_hip__dir_counts.restype = [C.POINTER(C.c_longlong)], None
    lib.abpoa_hip__dir_counts(out)
    return out[0], out[1]


def row_launches(lib):
    """[launches of the narrow row kernel, of dp_wide_kernel, of dp_xl_kernel] since the last call; the call zeroes them."""
    out = (C.c_longlong * 3)()
    lib.abpoa_hip__row_launches.argtypes, lib.abpoa_hip__row_launches.restype = [C.POINTER(C.c_longlong)], None
    lib.abpoa_hip__row_launches(out)
    return [int(x) for x in out]


def narrow_plan(case, bits):
    """(score-ring rows, ring columns) of the launch plan for one alignment like `case` on the narrow row loop."""
    from abpoa_amd import ffi
    out = (C.c_int * 4)()
    f = ffi.lib().abpoa_hip__narrow_plan
    f.argtypes, f.restype = [C.POINTER(H.Scoring), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)], None
    f(C.byref(case.sc), case.qlen, bits, 1, out)
    return out[0], out[1]


def _first_read(reads, m):
    from abpoa_amd import seqio
    a = np.ascontiguousarray(seqio.encode(reads[0], m), np.uint8)
    return a, a.ctypes.data_as(_U8P)


def cigar_digests(lib, sets, m):
    """Under ABPOA_HIP_CIGAR_DIGEST=1 (read once per process): every graph cigar of a read-set folded into 64 bits, looked up by the set's first read, for
    each of `sets` (0: nothing folded); the table is released afterwards.  `lib`: the engine or the CPU shim."""
    f = lib.abpoa_hip__cigar_digest
    f.argtypes, f.restype = [_U8P, C.c_int, C.c_int], C.c_ulonglong
    out = []
    for s in sets:
        a, pa = _first_read(s, m)
        out.append(int(f(pa, len(a), 0)))
    f(None, 0, 1)
    return out


def last_alignments(lib, sets, m):
    """Under the same switch: the result record of each set's last alignment (eight ints: matched bases, aligned bases, node and query ends, cigar words,
    status), None where the library noted none; the table is released afterwards."""
    f = lib.abpoa_hip__last_aln
    f.argtypes, f.restype = [_U8P, C.c_int, C.POINTER(C.c_int), C.c_int], C.c_int
    out = []
    for s in sets:
        a, pa = _first_read(s, m)
        v = (C.c_int * 8)()
        out.append(list(v) if f(pa, len(a), v, 0) else None)
    f(None, 0, None, 1)
    return out


# ---------------------------------------------------------------- one launch through the flat C-ABI, every alignment against the oracle
def compare_launch(items, outs, trace, label, bits=None):
    """items: [(name, FlatCase, ..., oracle output)] of one launch, outs: what H.run_hip returned for it.  Every alignment ended with status 0, carries the
    trace exactly when one was asked for, ran in the oracle's score width (in `bits` where given) and equals the oracle: best cell, cigar, result fields, band
    state and -- with the trace -- bands, every plane cell and the row arg-max (H.compare_outs)."""
    assert len(outs) == len(items), (label, len(outs), len(items))
    for it, h in zip(items, outs):
        name, o = it[0], it[-1]
        assert h.status == 0 and hasattr(h, "dp_beg") == trace and h.bits == (bits or o.bits), (label, name, h.status, h.bits)
        H.compare_outs(h, o, label=f"{label} {name} trace={trace}")


def launch(items, trace, label, bits=None):
    """ONE launch of items' cases, compared with compare_launch; returns the device's outputs."""
    outs = H.run_hip([it[1] for it in items], want_trace=trace)
    compare_launch(items, outs, trace, label, bits)
    return outs


def words_match(items, label):
    """Every direction word the row loops write for items' (name, FlatCase, input dict, ...) equals the word oracle/dir_model.c derives from the oracle's scores."""
    for it in items:
        bad = H.dir_words_mismatches(it[1], it[2])
        assert bad is not None and bad == [], (label, it[0], bad[:5] if bad else bad)
