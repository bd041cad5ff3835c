"""The tree kernels (csrc/azg_kernels.h: best_child, leaf_policy / masked_sum, backup_path, root_probs, k_root_stats) held to the
REFERENCE at its edges (pytest -m gpu): tests/golden/{c4,tm,br,ot,gb,tt}_edge.npz, made by running the reference's MCTS.pyx /
SelfPlayAgent.pyx on the tests/edge_eval.py rows -- exact PUCT ties, zero and denormal priors, both forms of the seen-policy
sum, exact draw values, cpuct 0 / 50, fpu_reduction -1 / 0, noise_frac 1, root temperatures 0.5 / 2 / 1.1, roots with 1, 2,
63, 64 and 65 children, paths of 24 and more actions.  The device is compared with the fixtures directly, not with the oracle
(tests/test_oracle_golden.py pins the oracle to the same fixtures on the CPU).

gb_edge is the four-chunk family (best_child<G, 4>, leaf_policy<G, 4>, the four-chunk add_children and the per-node switch to
the one-chunk templates at k <= 64): roots of 225, 193, 192, 191, 129, 128, 127, 66, 65, 64, 63, 2 and 1 legal moves, 241
simulations each (and, as `gbr`, four random prefixes of 201 to 220 legal moves, 48 simulations each), so that under the first-play bonus the first maximum sweeps every chunk out of ties that span chunks, zero
priors are chosen among more than 64 children, the serial seen-sum runs over more than 128, and descents cross from wide
nodes into k <= 64.  Its noisy configs hold the device to the reference's arithmetic with only numpy's underflow trap off
(the float32 cast of a 225-way Dirichlet draw underflows).  ot_edge adds othello roots of one and two legal moves, tt_edge
tic-tac-toe's (one move from a full board, and two), on random roots of up to nine.  All three are
replayed on the host envs (tests/test_edge_fixtures_cpu.py pins that replay, and checks every recorded action legal on the
host rules; here the path is replayed only where the evaluator row depends on the leaf, the `onehot` family); gb_edge stores
a crc of the counts row per simulation where the other fixtures store the root's n row.

Every config runs (tests/fixture_checks.py: check_tree with the EDGE tier, check_agent) on two engines fed the same rows: one per launch form, azg_select + azg_backup (one launch per phase) and
azg_backup_select (k_backup_select2: backup k and select k + 1 in one launch, two wavefronts per tree).  Checked: every root's
leaf path at every simulation, the root visit counts after every simulation, the final root children (a / n / q / p / v),
root n and max depth, root_probs at every recorded temperature, root_value, tape counters.  The edge agent (temperature 0 from
the first move: np.argmax ties over visit counts) goes through select / backup / advance (k_play, k_emit_samples) in both forms.

Where the reference raised FloatingPointError (probs at T = 0.01: (counts / n) ** 100 underflows under its
np.seterr(all='raise')), the device returns the untrapped IEEE value of the same expression and that is
what is asserted.  The persistent search launches (azg_search_*) compute their own network, so they cannot take these injected
rows; they reach the same select_tree / backup_path code and stay tied to it through the launch-equals-phase tests."""
import numpy as np
import pytest

import edge_eval as ee
import fixture_checks as FC

pytestmark = pytest.mark.gpu
NAMES = ('c4', 'tm', 'br', 'ot', 'gb', 'tt')
EDGE_CASES = [(n, c) for n in NAMES + ('gbr',) for c in ee.CONFIGS]      # gbr: the random-prefix roots gb_edge.npz holds under rnd_


@pytest.mark.parametrize('name,cname', EDGE_CASES)
def test_edge_tree_vs_reference_goldens(name, cname):
    d = FC.load(name + '_edge')
    gid = ee.GAMES[name]
    A, NV = ee.game_sizes(gid)
    fam, seed = str(d[cname + '_family']), int(d[cname + '_seed'])
    roots = ee.roots(d, gid)
    if name == 'tt':                                         # random roots, and roots with one legal move (one move from a full board) and two
        ks = sorted(int(g.valid_moves().sum()) for g in roots)
        assert 4 <= len(roots) <= 16 and 8 <= int(d[cname + '_cfg'][4]) <= 30 and ks[:4] == [1, 1, 2, 2] and ks[-1] == 9

    def rows(s):
        """the rows the generator fed at simulation s (`onehot` looks at the leaf: the root played along the fixture's path)"""
        pol = np.zeros((len(roots), A), np.float32); val = np.zeros((len(roots), NV), np.float32)
        for r, g in enumerate(roots):
            ref = d[cname + '_paths'][r, s][:int(d[cname + '_depth'][r, s])]
            pol[r], val[r] = ee.leaf_row(fam, seed, g, r, s, ref, A, NV)
            assert ee.row_crc(pol[r], val[r]) == d[cname + '_row_crc'][r, s], (name, cname, 'row_crc', r, s)
        return pol, val
    FC.check_tree(gid, d, cname, [ee.root_state(g) for g in roots], FC.EDGE, name, rows, obs=False)


def _zero_temp(cur_temp, turns, const_max_turns):
    return 0


@pytest.mark.parametrize('launch', FC.LAUNCHES)
@pytest.mark.parametrize('name', NAMES)
def test_edge_agent_vs_reference_goldens(name, launch):
    """SelfPlayAgent.run on the engine with the edge agent's rows (uniform priors, draw-heavy values) at temperature 0 from the
    first move (np.argmax ties over the visit counts), symmetric samples on: counts, moves, games, every sample and result as the
    reference made them"""
    d = FC.load(name + '_edge')
    B, seed = int(d['agent_B']), int(d['agent_seed'])
    A, NV = ee.game_sizes(ee.GAMES[name])
    assert name != 'tt' or 4 <= B <= 8

    def rows(step):
        r = [ee.agent_row(seed, i, step, A, NV) for i in range(B)]
        return np.array([p for p, _ in r]), np.array([v for _, v in r])
    rec = FC.check_agent(ee.GAMES[name], d, 'agent_', launch, name, rows,
                         engine_kw=dict(example_capacity=20000, start_temp=0.0, temp_fn=_zero_temp))
    assert rec['games_played'][-1] == int(d['agent_games']) and (rec['games_played'][:-1] < int(d['agent_games'])).all()
