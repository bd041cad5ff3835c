"""Generate the othello golden vectors under tests/golden/ from the ACTUAL reference implementation (alphazero/envs/othello).

Run in the build container only:   PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_othello_goldens.py [which ...]
Outputs (small .npz fixtures, committed):
  ot_rules.npz          random playouts of the reference's othello.Game: every position's cells, player, turns, valid_moves, win_state,
                        observation CRC and the move played next; the 8 symmetries of a subset; coverage counts of every terminal kind
  ot_tree.npz           single-tree MCTS traces (make_goldens.gen_tree): default, cpuct 4 / fpu 0.4, noise + temperature
  ot_agent.npz          SelfPlayAgent lock-step traces (make_goldens.gen_agent): plain, noisy, fastmix (symmetricSamples=False + probFastSim)
  ot_mt19937_agent.npz  a whole SelfPlayAgent under np.random.seed(s), every draw observed (make_goldens.gen_c4_mt19937_agent)
  ot_edge.npz           the tree edge family (make_goldens.gen_edge, asked for by name: `ot_edge`): 12 random roots plus roots whose side
                        to move has exactly one and exactly two legal moves
The tree / agent helpers of make_goldens.py ask the oracle for the game's sizes (oracle_lib.game_info); the oracle has no othello, so
this script answers that one call for game id 3 in-process and hands every other id through.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as mg  # noqa: E402
import refharness as rh  # noqa: E402
from refharness import ol  # noqa: E402

GAME_OTHELLO = 3
_oracle_game_info = ol.game_info


def game_info(game):
    if game != GAME_OTHELLO:
        return _oracle_game_info(game)
    gi = ol.GameInfo()
    (gi.action_size, gi.obs_c, gi.obs_h, gi.obs_w, gi.num_players, gi.has_draw, gi.max_turns, gi.num_symmetries, gi.cells,
     gi.max_children) = 64, 1, 8, 8, 2, 1, 64, 8, 64, 60
    return gi


ol.game_info = game_info

# coverage floors of ot_rules.npz, per terminal kind (win_state from the mover's view, othello.pyx:83-96)
RULE_FLOORS = dict(positions=10000, mover_wins=20, other_wins=20, draws=3, early_end=40)


def ref_game():
    from alphazero.envs.othello.othello import Game
    return Game


def cells_of(g):
    return np.asarray(g._board.pieces, dtype=np.int8).reshape(-1)


def gen_rules(out_dir, seed=2468, n_sym=256, verbose=True):
    Game = ref_game()
    rng = np.random.RandomState(seed)
    cols = {k: [] for k in ('cells', 'player', 'turns', 'valids', 'ws', 'obs_crc', 'next', 'lens', 'moves')}
    cov = dict(mover_wins=0, other_wins=0, draws=0, early_end=0)
    games = 0
    while len(cols['lens']) < RULE_FLOORS['positions'] or any(cov[k] < RULE_FLOORS[k] for k in cov):
        g, seq = Game(), []
        while True:
            v = np.asarray(g.valid_moves()).astype(np.uint8)
            w = np.asarray(g.win_state()).astype(np.uint8)
            o = np.asarray(g.observation())
            assert o.shape == (1, 8, 8)
            cols['cells'].append(cells_of(g)); cols['player'].append(g.player); cols['turns'].append(g.turns)
            cols['valids'].append(v); cols['ws'].append(w); cols['obs_crc'].append(rh.crc(o.astype(np.float32)))
            m = np.full(60, -1, np.int8); m[:len(seq)] = seq
            cols['moves'].append(m); cols['lens'].append(len(seq))
            if w.any():
                cols['next'].append(-1)
                mover = g.player
                if w[2]:
                    cov['draws'] += 1
                elif w[mover]:
                    cov['mover_wins'] += 1
                else:
                    cov['other_wins'] += 1
                if (cells_of(g) == 0).any():
                    cov['early_end'] += 1
                break
            a = int(rng.choice(np.flatnonzero(v)))
            cols['next'].append(a)
            g.play_action(a); seq.append(a)
        games += 1
    n = len(cols['lens'])
    # the 8 symmetries of a subset (othello.pyx:101-120), pi = the action index itself so that the permutation is recorded
    pick = np.sort(rng.choice(n, n_sym, replace=False))
    sym_cells = np.zeros((n_sym, 8, 64), np.int8); sym_pi = np.zeros((n_sym, 8, 64), np.int8)
    for j, i in enumerate(pick):
        g = Game()
        g._board.pieces = np.asarray(cols['cells'][i], np.intc).reshape(8, 8).copy()
        g._player, g._turns = int(cols['player'][i]), int(cols['turns'][i])
        syms = g.symmetries(np.arange(64, dtype=np.float32))
        assert len(syms) == 8
        for k, (gs, pi) in enumerate(syms):
            sym_cells[j, k] = cells_of(gs); sym_pi[j, k] = np.asarray(pi).astype(np.int8)
        assert (sym_cells[j, 7] == cols['cells'][i]).all() and (sym_pi[j, 7] == np.arange(64)).all()   # the identity is the last entry
    counts = np.array([n, cov['mover_wins'], cov['other_wins'], cov['draws'], cov['early_end']], np.int32)
    for k, c in zip(('positions', 'mover_wins', 'other_wins', 'draws', 'early_end'), counts):
        assert c >= RULE_FLOORS[k], (k, c)
    np.savez_compressed(os.path.join(out_dir, 'ot_rules.npz'), cells=np.array(cols['cells']), player=np.array(cols['player'], np.int8),
                        turns=np.array(cols['turns'], np.int8), valids=np.array(cols['valids']), ws=np.array(cols['ws']),
                        obs_crc=np.array(cols['obs_crc'], np.uint32), next=np.array(cols['next'], np.int8), lens=np.array(cols['lens'], np.int16),
                        moves=np.array(cols['moves']), sym_index=pick.astype(np.int32), sym_cells=sym_cells, sym_pi=sym_pi,
                        coverage=counts, coverage_names=np.array(['positions', 'mover_wins', 'other_wins', 'draws', 'early_end']))
    if verbose:
        print('ot_rules: %d positions of %d games, coverage %s' % (n, games, dict(zip(('mover_wins', 'other_wins', 'draws', 'early_end'), counts[1:].tolist()))))


TREE_CONFIGS = [('default', 1.25, 0.2, False, False, 100), ('cpuct4', 4.0, 0.4, False, False, 100), ('noise_temp', 4.0, 0.4, True, True, 60)]
AGENT_CONFIGS = [
    ('plain', 4, 16, 4, dict()),
    ('noisy', 4, 12, 4, dict(add_root_noise=True, add_root_temp=True, cpuct=4.0, fpu_reduction=0.4)),
    ('fastmix', 4, 12, 4, dict(probFastSim=0.5, numFastSims=4, symmetricSamples=False)),   # raw samples: symmetries()[7] is the identity
]


def edge_roots(Game, seed, n_random=12, ks=(1, 2)):
    """reference games at the edge roots: random legal prefixes, then positions whose side to move has exactly k moves (the first
    ones random playouts meet).  The reference's othello has no pass: a side without a move ends the game (othello.pyx:83-96), so
    one legal move is the smallest root there is."""
    rng = np.random.RandomState(seed)
    roots, kinds = [], []
    for r in range(n_random):
        g = Game()
        for _ in range(0 if r == 0 else rng.randint(0, 50)):
            g2 = g.clone(); g2.play_action(int(rng.choice(np.flatnonzero(np.asarray(g.valid_moves())))))
            if np.asarray(g2.win_state()).any():
                break
            g = g2
        roots.append(g); kinds.append(0)
    for k in ks:
        found = None
        while found is None:
            g = Game()
            while not np.asarray(g.win_state()).any():
                v = np.flatnonzero(np.asarray(g.valid_moves()))
                if len(v) == k:
                    found = g
                    break
                g.play_action(int(rng.choice(v)))
        roots.append(found); kinds.append(k)
    return roots, kinds


mg.EDGE_HOOKS['ot'] = dict(gid=GAME_OTHELLO, sims=60, game_cls=ref_game, roots=edge_roots, cells=cells_of, agent=(4, 12, 4),
                           cov=[], floors={}, compact=False)


def main(which=None, out_dir=HERE, verbose=True):
    which = which or ['ot_rules', 'ot_tree', 'ot_agent', 'ot_mt19937_agent']
    rh.import_reference()
    mg.OUT = out_dir
    Game = ref_game()
    if 'ot_rules' in which:
        gen_rules(out_dir, verbose=verbose)
    if 'ot_tree' in which:
        mg.gen_tree(Game, GAME_OTHELLO, 'ot', n_roots=16, seed=37, configs=TREE_CONFIGS, max_prefix=40)
    if 'ot_agent' in which:
        mg.gen_agent(Game, GAME_OTHELLO, 'ot', configs=AGENT_CONFIGS, seed=515)
    if 'ot_mt19937_agent' in which:
        mg.gen_c4_mt19937_agent(B=4, sims=12, games=4, seed=20261015, eval_seed=97, Game=Game, gid=GAME_OTHELLO, name='ot')
    if 'ot_edge' in which:
        mg.gen_edge('ot', out_dir=out_dir, verbose=verbose)


if __name__ == '__main__':
    main(sys.argv[1:] or None)
