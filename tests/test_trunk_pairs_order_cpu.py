"""The order rule of the trunk kernel's growth pairs (csrc/trunk_pairs.h pairs_allowed), no GPU: a
host-only program (tests/trunk_pairs_order_sim.cpp) includes the rule header and simulates the G
workgroup streams with blocking neighbourhood waits over a sweep of (n, nbx, nby, G).  Every
geometry the rule accepts must run to completion pair-major, and unpaired as well; and some geometry
the rule refuses must deadlock when paired (the rule is not vacuous).  The program is built plain and with the address and undefined-behaviour
sanitizers; both must agree (tests/host_program.py)."""
from pathlib import Path

import pytest

import host_program

SRC = Path(__file__).resolve().parent / "trunk_pairs_order_sim.cpp"


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    if host_program.GXX is None:
        pytest.skip("needs g++")
    (out,) = host_program.run_plain_and_sanitized(SRC, tmp_path_factory.mktemp("pairs_order"), timeout=600)
    rows = [tuple(int(v) for v in line.split()) for line in out.splitlines()]
    assert rows and all(len(row) == 7 for row in rows)
    return rows


def test_accepted_geometries_complete_and_a_refused_one_deadlocks(sweep):
    plain = sweep
    accepted = [r for r in plain if r[4]]
    refused = [r for r in plain if not r[4]]
    print(f"{len(plain)} geometries: {len(accepted)} accepted, {len(refused)} refused, "
          f"{sum(1 for r in refused if not r[6])} of the refused deadlock when paired")
    assert accepted and refused
    # the unpaired stream completes wherever the rule accepts, and wherever a tile row plus two fits
    # the grid.  (Below that, with more tiles than workgroups, the simulation finds launches whose
    # unpaired stream deadlocks as well: the last tiles of two workgroups each wait, before they
    # publish, for the other's to finish the layer, e.g. 7 x 2 tiles on 5 workgroups.  On 512
    # workgroups that takes tile rows of 510 tiles or more, 16,320 pixels; the kernel's bounded spin
    # then gives the launch up and the host raises.)
    stuck_unpaired = [r[:4] for r in plain if not r[5]]
    bad = [g for g in stuck_unpaired if g[0] * g[1] * g[2] <= g[3] or g[3] >= g[1] + 2]
    assert not bad, f"the unpaired stream must complete here: {bad[:5]}"
    assert not [r[:4] for r in accepted if not r[5]]
    stuck = [r[:4] for r in accepted if not r[6]]
    assert not stuck, f"accepted by pairs_allowed but the paired streams deadlock (n, nbx, nby, G): {stuck[:5]}"
    assert any(not r[6] for r in refused), "no refused geometry deadlocks: the rule would be vacuous"
    # more tiles than workgroups on both sides of the rule
    assert any(r[0] * r[1] * r[2] > r[3] for r in accepted)
    # the cases the GPU tests rely on: 546 tiles on 512 workgroups pair, the 768-tile row of 256 does not
    by_geo = {r[:4]: r for r in plain}
    assert by_geo[(3, 13, 14, 512)][4:] == (1, 1, 1)
    assert by_geo[(1, 256, 3, 512)][4] == 0
    # a 1080p frame: refused one workgroup below the rule's edge, and a real deadlock at G = nbx + 1
    assert by_geo[(1, 60, 68, 124)][4] == 1 and by_geo[(1, 60, 68, 123)][4] == 0
    assert (by_geo[(1, 60, 68, 61)][4], by_geo[(1, 60, 68, 61)][6]) == (0, 0)
