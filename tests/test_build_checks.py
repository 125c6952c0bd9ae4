"""CPU (-m "not gpu"): static checks of the device code hipcc generates for the kernels that run under a register cap.

The engine issues global loads from inline assembly and waits for them later (`gld_async` ... `gld_wait`, dp_common.h); to the compiler
the loaded register is defined at the load.  If it spills such a register between the load and the wait, it saves a value that has not
arrived yet -- the all-rounds kernel (128 vector registers per wavefront) did exactly that in its int32 / convex backtrack until its
staging batches were made smaller, and faulted on the GPU.  tools/check_async_spans.py finds the pattern in the assembly."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "abpoa_amd", "csrc")


_ASM = {}


def _device_asm(unit, tmp_path_factory):
    """(assembly path, resource-usage remarks) of one kernel translation unit, compiled once per session."""
    if unit not in _ASM:
        asm = tmp_path_factory.mktemp("asm") / (unit + ".s")
        cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-variable", "-Wno-unused-function", "-Wno-inline-asm", "--offload-arch=gfx950",
               "-I" + os.path.join(ROOT, "include"), "-S", "--cuda-device-only", "-o", str(asm), os.path.join(CSRC, unit + ".hip"),
               "-Rpass-analysis=kernel-resource-usage"]
        if unit == "poa_rounds":
            cmd.append("-falign-loops=32")                                 # (as the Makefile builds it)
        r = subprocess.run(cmd, check=True, cwd=CSRC, timeout=900, capture_output=True, text=True)
        _ASM[unit] = (str(asm), r.stderr)
    return _ASM[unit]


@pytest.mark.parametrize("unit", ["poa_rounds", "dp_fast_tail", "dp_wide_rows", "dp_xl_rows"])
def test_no_spill_between_async_load_and_wait(unit, tmp_path_factory):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    asm, _ = _device_asm(unit, tmp_path_factory)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_async_spans.py"), asm], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-3000:]


def test_assembly_row_loop_kernels_own_its_registers(tmp_path_factory):
    """The hand-placed assembly row loop (rows_tight_asm.h) lists v92-v127 as clobbered: the all-rounds kernels that hold it (affine, convex) must be
    allocated all 128 VGPRs, or the compiler would be free to keep live values there."""
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    _, remarks = _device_asm("poa_rounds", tmp_path_factory)
    vgprs, cur = {}, None
    for ln in remarks.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = m.group(1)
        m = re.search(r"remark:\s+VGPRs: (\d+)", ln)
        if m and cur:
            vgprs[cur] = int(m.group(1))
    for gap in (1, 2):
        name = "_ZN9abpoa_hip17poa_rounds_kernelILi%dEEEvii" % gap
        assert vgprs.get(name, 0) >= 128, (name, vgprs)


HOST_RULES = r"""
// the pieces of the kernels' routing rules (routing.h) and msa_device.h msa_device_set_is_ragged: plain functions, checked on the CPU
#include <stdio.h>
#include <vector>
#include "engine.h"
#include "routing.h"
#include "msa_device.h"
using namespace abpoa_hip;
static int fails = 0;
#define CHECK(x) do { if (!(x)) { printf("FAILED: %s\n", #x); ++fails; } } while (0)
static bool ragged(std::vector<int> lens) {
    std::vector<const uint8_t *> seqs(lens.size(), nullptr);
    abpoa_hip_readset_t S; S.n_reads = (int)lens.size(); S.seqs = seqs.data(); S.lens = lens.data(); S.weights = nullptr;
    return msa_device_set_is_ragged(S);
}
int main() {
    const int G = ABPOA_HIP_GLOBAL_MODE, L = ABPOA_HIP_LOCAL_MODE, X = ABPOA_HIP_EXTEND_MODE, LIN = ABPOA_HIP_LINEAR_GAP, AFF = ABPOA_HIP_AFFINE_GAP, CVX = ABPOA_HIP_CONVEX_GAP;
    // which jobs the banded global row loops take: a band, global or extension mode; linear gaps only with an extension penalty (the row arg-max is read before the in-row scan)
    CHECK(fast_global_job(AFF, G, 10, 2) && fast_global_job(CVX, X, 10, 2) && fast_global_job(AFF, G, 0, 0));
    CHECK(!fast_global_job(AFF, G, -1, 2) && !fast_global_job(CVX, L, 10, 2) && !fast_global_job(LIN, L, 10, 2));
    CHECK(fast_global_job(LIN, G, 10, 1) && fast_global_job(LIN, X, 10, 3) && !fast_global_job(LIN, G, 10, 0) && !fast_global_job(LIN, G, -1, 2));
    // ... and which of their alignments: linear gaps below the wide loop's band half-widths only (a ragged set's extra columns count half)
    CHECK(fast_global_aln(LIN, 39, 0) && !fast_global_aln(LIN, 40, 0) && !fast_global_aln(LIN, 20, 40) && fast_global_aln(LIN, 20, 38));
    CHECK(fast_global_aln(AFF, 400, 0) && fast_global_aln(CVX, 40, 512));
    // half of the extra columns counts as band half-width, rounded down
    CHECK(route_w(20, 0) == 20 && route_w(20, 1) == 20 && route_w(20, 39) == 39 && route_w(20, 41) == 40 && route_w(0, 401) == 200);
    // the local row loop: local mode without a band, affine / convex gaps; int16 scores, at most loc_cols columns (575 bases: 576 columns), query codes in LDS
    CHECK(local_loop_job(AFF, L, -1) && local_loop_job(CVX, L, -1) && !local_loop_job(LIN, L, -1) && !local_loop_job(AFF, L, 10) && !local_loop_job(AFF, G, -1) && !local_loop_job(CVX, X, -1));
    { LdsPlan P; P.loc_cols = 576; P.q_cap = 576; P.fr_cols = 128;
      CHECK(local_loop_fits(P, 16, 575) && !local_loop_fits(P, 16, 576) && !local_loop_fits(P, 32, 575) && !local_loop_fits(P, 32, 576) && local_loop_fits(P, 16, 1));
      CHECK(fast_loop_fits(P, 576) && !fast_loop_fits(P, 577));
      P.q_cap = 512; CHECK(local_loop_fits(P, 16, 512) && !local_loop_fits(P, 16, 513) && fast_loop_fits(P, 512) && !fast_loop_fits(P, 513));
      P.loc_cols = 0; P.fr_cols = 0; CHECK(!local_loop_fits(P, 16, 100) && !fast_loop_fits(P, 100)); }
    // the wide row loop's band half-widths; direction words: mode 1 narrow alignments only, mode 2 all, mode 0 none
    CHECK(in_wide_range(40, 215, 40) && in_wide_range(40, 215, 215) && !in_wide_range(40, 215, 39) && !in_wide_range(40, 215, 216) && !in_wide_range(1, 0, 0) && !in_wide_range(1, 0, 1));
    CHECK(wide_range_meets(40, 215, 20, 40) && wide_range_meets(40, 215, 215, 300) && !wide_range_meets(40, 215, 20, 39) && !wide_range_meets(40, 215, 216, 300));
    CHECK(!dir_for(0, false) && !dir_for(0, true) && dir_for(1, false) && !dir_for(1, true) && dir_for(2, false) && dir_for(2, true));
    // read-sets with ragged read ends: lengths differ by more than an eighth of the longest read, at least 64 bases
    CHECK(!ragged({1000}) && !ragged({1000, 1000, 990}) && !ragged({1000, 875}) && ragged({1000, 874}));
    CHECK(!ragged({300, 236}) && ragged({300, 235}) && ragged({10000, 10000, 8000}) && !ragged({10000, 8750, 9999}));
    printf(fails ? "host rules: %d failed\n" : "host rules ok\n", fails);
    return fails ? 1 : 0;
}
"""


def test_host_routing_rules(tmp_path):
    """The pieces of routing.h (fast_global_job, fast_global_aln, route_w, local_loop_job, local_loop_fits, fast_loop_fits, the wide range, dir_for: shared by
    the kernels' takes_* rules, engine.cpp and the device-resident driver's plan) and
    msa_device_set_is_ragged (msa_device.h: which read-sets abpoa_hip_msa_batch runs as a batch of their own) on their truth tables -- host code, no GPU."""
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    src = tmp_path / "host_rules.cpp"; src.write_text(HOST_RULES)
    exe = tmp_path / "host_rules"
    subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True, timeout=600,
                   capture_output=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "host rules ok" in p.stdout, p.stdout
