"""GPU (-m gpu): the local row loops (rows_local.h) at plane level at every chunk count -- dp_local_kernel's straight-line bodies of 3 / 5 / 9 chunks and
dp_local_team_kernel's shapes of 1 / 2 / 3 chunks per wavefront with every uneven share -- against the C oracle, bit for bit, through the flat C-ABI: bands,
every plane cell, row arg-max, best cell, cigar, result fields.  The inputs are the table of tests/local_widths.py: three local goldens (amino acids under
BLOSUM62 convex, nucleotides affine and convex) re-queried at 1 .. 576 residues, with skip edges (rows of up to 13 predecessors up to 33 rows back: the arena
gather behind the LDS ring, the loop behind the eighth predecessor) and with periodic queries (row maxima tied between chunks: the packed arg-max key and its
trip through the team's LDS exchange).  All widths of a golden run in ONE launch, in both orders, so alignments of different widths lie side by side in the
arena and every row's chunk store that runs past its end has a neighbour to hit.  tests/test_local_regimes.py asserts the properties of the inputs on the CPU
and tests/test_oracle_vs_reference.py pins the oracle to the compiled reference at these read lengths."""
import pytest

import local_widths as LW
from gpu_harness import engine, launch  # noqa: F401  (engine: the fixture)
from test_local_regimes import local_case

pytestmark = pytest.mark.gpu
TEAM = pytest.mark.parametrize("team", ["0", "1"], ids=["one_wavefront", "team_of_four"])
GOLDEN = pytest.mark.parametrize("golden", LW.GOLDENS)


def _launch(items, label, orders=(1,), bits=None):
    """items: [(name, FlatCase, oracle output)] in ONE launch per trace mode and order; everything against the oracle."""
    for trace in (True, False):
        for step in orders:
            launch(items[::step], trace, f"{label} order={step}", bits=bits or 16)


def _widths(golden):
    return [(f"qlen={q}", *local_case(golden, q)) for q in LW.QLENS]


@TEAM
@GOLDEN
def test_every_width_in_one_launch(engine, monkeypatch, team, golden):
    """Every QLENS point, 1 .. 9 chunks and the 592-column alignment that the general kernel takes, in one launch; then in reverse order, so every alignment has
    had a narrower and a wider neighbour on either side; with and without the trace."""
    monkeypatch.setenv("ABPOA_HIP_LOCAL_TEAM", team)
    _launch(_widths(golden), f"widths team={team} {golden}", orders=(1, -1))


@GOLDEN
def test_every_width_through_the_general_kernel(engine, monkeypatch, golden):
    """ABPOA_HIP_DBG=64: the same launch with the general kernel for all -- the kernel the local loops hand over to."""
    monkeypatch.setenv("ABPOA_HIP_DBG", "64")
    _launch(_widths(golden), f"widths general {golden}")


@TEAM
@GOLDEN
def test_skip_edges(engine, monkeypatch, team, golden):
    """SKIPS, and SKIPS + FILL, at 1, 4, 6 and 9 chunks: predecessors older than the ring from the arena (first and later ones, lane 0's zero, the clamps at
    the row's end), rows of every predecessor count from 1 to 13; without the trace the record walk steps through the rows of 9 - 13 predecessors."""
    monkeypatch.setenv("ABPOA_HIP_LOCAL_TEAM", team)
    items = [(f"qlen={q} {tag}", *local_case(golden, q, skips=sk)) for q in LW.SKIP_QLENS for tag, sk in (("SKIPS", LW.SKIPS), ("SKIPS+FILL", LW.SKIPS_FILLED))]
    _launch(items, f"skip edges team={team} {golden}")


@TEAM
@GOLDEN
def test_tiled_queries(engine, monkeypatch, team, golden):
    """Periodic queries, with and without SKIPS: the row arg-max of every row, the best cell (the first row that reaches the best score wins) and the cigar."""
    monkeypatch.setenv("ABPOA_HIP_LOCAL_TEAM", team)
    items = [(f"({q}, {p}) {tag}", *local_case(golden, q, p, sk)) for q, p in LW.TILED for tag, sk in (("plain", ()), ("SKIPS", LW.SKIPS))]
    _launch(items, f"tiled team={team} {golden}")


@TEAM
@pytest.mark.parametrize("golden", LW.NUCLEOTIDE)
def test_non_default_scoring(engine, monkeypatch, team, golden):
    """An asymmetric matrix (ASYM5) at 4 and 9 chunks, and both sides of the int16 gate: at match = M16 the local loops run scores near the top of the range,
    at M16 + 1 the alignment scores in 32 bits, leaves the local loops (takes_local) and must still equal the oracle."""
    monkeypatch.setenv("ABPOA_HIP_LOCAL_TEAM", team)
    pt = LW.asym_point(golden)
    _launch([(f"{pt.name} qlen={q}", *local_case(golden, q, pt=pt)) for q in LW.SCORING_QLENS], f"scoring team={team} {golden}")
    for q in LW.SCORING_QLENS:
        for pt, bits in zip(LW.gate_points(golden, q), (16, 32)):
            _launch([(f"{pt.name} qlen={q}", *local_case(golden, q, pt=pt))], f"gate team={team} {golden}", bits=bits)
