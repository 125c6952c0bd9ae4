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


DIAG_RULES = r"""
// diag.h alone (no HIP header): the packed words of AlnOut.seg at their field limits, the bits of ABPOA_HIP_DBG, and their help text
#include <stdio.h>
#include <string.h>
#include <string>
#include "diag.h"
#include "engine_options.h"
using namespace abpoa_hip;
static int fails = 0;
#define CHECK(x) do { if (!(x)) { printf("FAILED: %s\n", #x); ++fails; } } while (0)
int main() {
    // census word: 24 bits of rows over 40 bits of ticks; what the kernels add per row is one row and its ticks
    const long long R = (1ll << 24) - 1, T = (1ll << 40) - 1;
    for (long long r : {0ll, 1ll, R}) for (long long t : {0ll, 1ll, T}) { const long long w = census_pack(r, t); CHECK(census_rows(w) == r && census_ticks(w) == t); }
    { long long w = 0; for (int i = 0; i < 1000; ++i) w += census_pack(1, 12345); CHECK(census_rows(w) == 1000 && census_ticks(w) == 12345000); }
    // census "why" word: three counts of 20 bits
    const long long Y = (1ll << 20) - 1;
    for (long long a : {0ll, 1ll, Y}) for (long long b : {0ll, 1ll, Y}) for (long long c : {0ll, 1ll, Y}) {
        const long long w = census_why_pack(a, b, c); CHECK(census_why_many_preds(w) == a && census_why_declined(w) == b && census_why_beyond_ring(w) == c); }
    CHECK(census_why_pack(1, 0, 0) + census_why_pack(0, 1, 0) + census_why_pack(0, 0, 1) == census_why_pack(1, 1, 1));
    // wide body word: 32 bits of rows, 16 of int32 long-read rows, 15 of int16 ones
    for (long long a : {0ll, 1ll, (1ll << 32) - 1}) for (long long b : {0ll, 1ll, (1ll << 16) - 1}) for (long long c : {0ll, 1ll, (1ll << 15) - 1}) {
        const long long w = wide_body_pack(a, b, c); CHECK(w >= 0 && wide_body_rows(w) == a && wide_body_long32(w) == b && wide_body_long16(w) == c); }
    // placement key: HW_ID (wave 0-3, simd 4-5, cu 8-11, sh 12, se 13-15) under XCC_ID; two waves share a SIMD iff xcc, se, sh, cu and simd agree
    { const long long k = placement_pack(0xffffffffll, 15); CHECK((k & 0xffffffffll) == 0xffffffffll && (k >> 32) == 15);
      CHECK(placement_simd(placement_pack(0x1234, 3)) == placement_simd(placement_pack(0x123f, 3)));          // another wave slot of the same SIMD
      CHECK(placement_simd(placement_pack(0x1234, 3)) != placement_simd(placement_pack(0x1224, 3)));          // another SIMD
      CHECK(placement_simd(placement_pack(0x1234, 3)) != placement_simd(placement_pack(0x1334, 3)));          // another CU
      CHECK(placement_simd(placement_pack(0x1234, 3)) != placement_simd(placement_pack(0x1234, 4))); }        // another XCC
    // the test hooks are 64 .. 2048, one bit each, and none of them is an ablation bit; the ablation names cover bits 0-5 in both loops
    const int hooks[] = {DBG_NO_FAST_LOOPS, DBG_KEEP_ROW_SLOTS, DBG_WALK_REPORT, DBG_WALK_GIVES_UP, DBG_ONE_WAVE_BACKTRACK, DBG_CXX_TIGHT_LOOP};
    int all = 0; for (int i = 0; i < 6; ++i) { CHECK(hooks[i] == 64 << i); CHECK(!(hooks[i] & DBG_ABLATION_BITS)); all |= hooks[i]; }
    CHECK(all == 4032 && DBG_ABLATION_BITS == 63);
    CHECK((ABL_NO_ARENA_STORE | ABL_FAST_NO_RING_STORE | ABL_FAST_NO_ARGMAX | ABL_FAST_NO_F_CLOSED_FORM | ABL_FAST_NO_GATHER | ABL_FAST_NO_SLOW_F) == DBG_ABLATION_BITS);
    CHECK((ABL_NO_ARENA_STORE | ABL_GEN_FAKE_ARGMAX | ABL_GEN_LITERAL_F_SCAN | ABL_GEN_NO_CHUNKS | ABL_GEN_FAKE_GATHER | ABL_GEN_NO_QUERY_PROFILE) == DBG_ABLATION_BITS);
    // every slot of every layout is one of the six; the clocks are four sums and the six slots
    CHECK(DIAG_SLOTS == 6 && PLACE_KEY < DIAG_SLOTS && PROF_TOP == 5 && CEN_WHY == 5 && WC_DECLINED == 5 && DTAIL_WINDOW_TICKS == 5 && RTAIL_WINDOW_TICKS == 5 && WALK_STEPS == 5);
    CHECK(CLK_SEG0 == 4 && CLK_SLOTS == 10);
    // the help of ABPOA_HIP_DBG names every bit: each hook by its value, the ablations as a group
    const char *names[128], *help[128]; const int n = list_options(names, help, 128); const char *h = nullptr;
    for (int i = 0; i < n && i < 128; ++i) if (strcmp(names[i], "ABPOA_HIP_DBG") == 0) h = help[i];
    CHECK(h != nullptr);
    if (h) { int covered = 0;
             for (const DbgBit &d : DBG_BITS) { const std::string tok = " " + std::to_string(d.value) + " "; CHECK(strstr(h, tok.c_str()) != nullptr); CHECK(strstr(h, d.what) != nullptr);
                                                CHECK(!(covered & d.value)); covered |= d.value; }
             CHECK(covered == (all | DBG_ABLATION_BITS)); printf("%s\n", h); }
    printf(fails ? "diag rules: %d failed\n" : "diag rules ok\n", fails);
    return fails ? 1 : 0;
}
"""


def test_diag_words_bits_and_help(tmp_path):
    """diag.h, the one definition of the kernels' diagnostic channel, as a stand-alone host program built with -fsanitize=undefined,address (as
    tests/test_pass_ladder.py builds its own): the packed words of AlnOut.seg round-trip at their field limits (a census word of 2^24 - 1 rows has its top
    bit set), the test-hook bits of ABPOA_HIP_DBG are 64 .. 2048 and disjoint from the ablation bits, and list_options' help names every bit."""
    import shutil
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    src = tmp_path / "diag_rules.cpp"; src.write_text(DIAG_RULES)
    exe = tmp_path / "diag_rules"
    b = subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-fsanitize=undefined,address", "-fno-sanitize-recover=undefined", "-I" + CSRC, "-o", str(exe), str(src),
                        os.path.join(CSRC, "engine_options.cpp")], timeout=300, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "diag rules ok" in p.stdout and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, (p.stdout[-3000:], p.stderr[-3000:])
