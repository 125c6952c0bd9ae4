"""Named scoring points away from `match 2 / mismatch 4` and the default gap penalties: asymmetric matrices, the wrap guards of the fast row loops,
the field caps of the direction plane, the int16 / int32 gate and the clamps of the int32 arg-max key.  One table for the CPU tests (oracle against the
compiled reference) and the GPU tests (kernels against the oracle).  A plain module: imported by name from the tests and from tools/."""
import os

import numpy as np

from abpoa_amd import api

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")
ASYM5 = os.path.join(DATA, "ASYM5.mtx")        # no two mirrored entries equal: a transposed matrix index changes scores
HOXD70 = os.path.join(DATA, "HOXD70.mtx")      # as committed G/T = -114, T/G = -144; penalties in the hundreds


class Point:
    """name; kw: api.Params keywords; group: matrix / guard / cap / clamp / gate; inside: for a guard pair, whether the point is in the wrap regime."""

    def __init__(self, name, group, inside=None, **kw):
        self.name, self.group, self.inside, self.kw = name, group, inside, kw

    def params(self, **more):
        return api.Params(**dict(self.kw, **more))

    def ref_opts(self):
        """The reference's command-line options for this point."""
        p = self.params()
        o = ["-O", f"{p.gap_open1},{p.gap_open2}", "-E", f"{p.gap_ext1},{p.gap_ext2}"]
        if p.mat_fn:
            return o + ["-t", p.mat_fn]
        return o + ["-M", str(p.match), "-X", str(p.mismatch)]

    def fields(self):
        """What to overwrite in a golden container's input section (max_mat / min_mis / gap_mode as the reference derives them: abpoa_post_set_para)."""
        p = self.params()
        i32 = lambda v: np.array([v], np.int32)
        return dict(mat=p.mat.copy(), m=i32(p.m), max_mat=i32(p.max_mat), min_mis=i32(p.min_mis), gap_open1=i32(p.gap_open1), gap_ext1=i32(p.gap_ext1),
                    gap_open2=i32(p.gap_open2), gap_ext2=i32(p.gap_ext2), gap_mode=i32(p.gap_mode))

    def dir_usable(self):
        """dir_plane_usable (abpoa_amd/csrc/dir_plane.h) spelled out again: 1 <= o1 <= 7, convex also 1 <= o2 <= 31 and e1 >= e2."""
        p = self.params()
        if p.gap_mode == api.AFFINE:
            return 1 <= p.gap_open1 <= 7
        return p.gap_mode == api.CONVEX and 1 <= p.gap_open1 <= 7 and 1 <= p.gap_open2 <= 31 and p.gap_ext1 >= p.gap_ext2

    def __repr__(self):
        return self.name


def _g(o1, o2, e1, e2=1):
    return dict(gap_open1=o1, gap_open2=o2, gap_ext1=e1, gap_ext2=e2)


POINTS = [
    # matrices
    Point("asym_cg", "matrix", score_matrix=ASYM5, **_g(4, 24, 2, 1)),
    Point("asym_ag", "matrix", score_matrix=ASYM5, **_g(6, 0, 2)),
    Point("asym_lg", "matrix", score_matrix=ASYM5, **_g(0, 0, 3)),
    Point("asym_ag_o7", "matrix", score_matrix=ASYM5, **_g(7, 0, 2)),      # affine at the direction plane's cap: the job of the assembly row loop
    Point("hox_cg", "matrix", score_matrix=HOXD70, **_g(400, 1200, 30, 1)),
    Point("hox_ag", "matrix", score_matrix=HOXD70, **_g(400, 0, 30)),
    Point("hox_lg", "matrix", score_matrix=HOXD70, **_g(0, 0, 60)),
    # guard pairs: the first of each pair keeps M + q at or above fast_lo, the second does not
    Point("guard_rec_x30", "guard", False, mismatch=30, **_g(4, 44, 2, 1)),
    Point("guard_rec_x31", "guard", True, mismatch=31, **_g(4, 44, 2, 1)),
    Point("guard_dir_x15", "guard", False, mismatch=15, **_g(7, 31, 1, 1)),
    Point("guard_dir_x16", "guard", True, mismatch=16, **_g(7, 31, 1, 1)),
    Point("guard_ag_x40", "guard", True, mismatch=40, **_g(40, 0, 2)),
    Point("guard_i32_x200", "guard", True, match=120, mismatch=200, **_g(4, 60, 2, 1)),
    # direction-plane field caps and the switch to score records
    Point("cap_o7_31", "cap", **_g(7, 31, 2, 1)),
    Point("cap_o8_31", "cap", **_g(8, 31, 2, 1)),
    Point("cap_o7_32", "cap", **_g(7, 32, 2, 1)),
    Point("cap_e2_2", "cap", **_g(4, 24, 2, 2)),
    Point("cap_e1_2", "cap", **_g(4, 24, 1, 2)),
    Point("cap_o6_3_e1_2", "cap", **_g(6, 3, 1, 2)),
    Point("cap_ag_o7", "cap", **_g(7, 0, 1)),
    Point("cap_ag_o8", "cap", **_g(8, 0, 1)),
]
# the int32 arg-max key's window (argmax_declines32, wide_closed_forms.h), run at wb = 45, wf = 0 on rows of 2-4 chunks: at -M 2000000 a matching row
# rises by more than the window's 2^21 - 2^19 above its first predecessor's maximum; at -M 500000 every row of the 1 kb goldens stays inside (at
# -M 1500000 4-7 % of their rows -- those whose first predecessor is not their best one -- still leave it: tests/test_scoring_regimes.py measures both)
CLAMP_POINTS = [
    Point("clamp_m2000000", "clamp", True, match=2000000, mismatch=2),
    Point("clamp_m500000", "clamp", False, match=500000, mismatch=2),
]
BY_NAME = {p.name: p for p in POINTS + CLAMP_POINTS}
GUARD_PAIRS = [("guard_rec_x30", "guard_rec_x31"), ("guard_dir_x15", "guard_dir_x16"), (None, "guard_ag_x40"), (None, "guard_i32_x200")]


def group(*names):
    return [p for p in POINTS if p.group in names]


def width_gate_points(qlen):
    """The last match score at which an alignment of `qlen` bases still runs in 16 bits under the default penalties, and the first at which it does not
    (reference src/simd_abpoa_align.c:1672-1683: qlen * max_mat <= 32767 - min_mis - oe1 - oe2)."""
    d = api.Params()
    m16 = (32767 - d.min_mis - (d.gap_open1 + d.gap_ext1) - (d.gap_open2 + d.gap_ext2)) // qlen
    return Point(f"gate16_m{m16}", "gate", match=m16), Point(f"gate32_m{m16 + 1}", "gate", match=m16 + 1)
