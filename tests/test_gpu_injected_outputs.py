"""The tree kernels against the oracle on net outputs no net emits: every round's (p, v) and every mirror row is
made up by tests/adversarial_outputs.py and injected (omok_round_inject / omok_mirror_inject), so k_scatter_policy, the mirror step's
masked_policy_row, the noise over such roots, the PUCT of k_round and the sampling kernels meet exact ties, zero and denormal rows,
legal sums at and one ulp below 2^-23, p = 0 on legal cells and v = +-1, +-0, the smallest denormal.  Everything is compared in
every bit (helpers.compare_trees, request boards, moves, status, replay tuples); there is no tolerance.

All inputs are finite.  NaN and +-inf are out of scope: f32::total_cmp orders NaNs by sign and payload and the sign of an arithmetic
NaN differs between x86 and gfx950, so no yardstick exists; a net with finite weights emits none.  (In the no-noise case the rows that can
become a searched root -- mirror rows and requests at even depth -- are therefore kept above 2^-24 of legal mass, since the root's
renormalisation is unguarded; requests at odd depth keep zero and denormal rows.)  The three cases of a few plies open with external moves
that fill the board until a ply has more simulations than empty cells (CASES' "opening"): PUCT between visited children then runs at
HW = 225, at K = 1 and without noise as well.

tests/test_adversarial_outputs.py checks the same configurations on the two oracles alone, and that they reach the branches
(coverage floors); this file asserts the floors again on what the device run actually contained, and prints the counts."""
import pytest

import adversarial_outputs as AO
from omok_ai_amd import binding as B
from helpers import drive_injected_vs_oracle

pytestmark = pytest.mark.gpu

MODE = B.NET_F16X3_MIXED  # (a set operand format: no probe at commit; the net only supplies the reset's root row)


@pytest.mark.parametrize("case", AO.CASES, ids=[c[0] for c in AO.CASES])
def test_injected_outputs_match_the_oracle(case):
    """n9_whole_games: HW = 81 (two lane sweeps, pad cells 81..127), 8 siblings per pass, zero-row roots under the noise, PUCT between
    tied children once the board has fewer empty cells than simulations; n15_k16: HW = 225 (four sweeps, four board words, pad cells
    225..255), 16 siblings = one full win-check pass; n9_k1: every simulation its own round; n9_no_noise: epsilon = 0, T = 0.5,
    Best and Boltzmann sampling on visit counts that tie."""
    name, n, games, count, k, plies, st = case
    settings = {key: st[key] for key in ("epsilon", "temperature", "threshold", "seed", "opening") if key in st}
    counts = drive_injected_vs_oracle(n, games, count, k, plies, MODE, st["kind_seed"], **settings)
    print(f"{name}: coverage {counts}")
    for key in AO.floor_keys(n, count, plies, st.get("epsilon", 0.25), st.get("opening", 0)):
        assert counts[key] >= AO.FLOOR, f"{name}: {key} = {counts[key]}"
