"""Generate the tic-tac-toe golden vectors under tests/golden/ from the ACTUAL reference implementation (alphazero/envs/tictactoe).

Run in the build container only:   PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_tictactoe_goldens.py [which ...]
Outputs (small .npz fixtures, committed):
  tt_rules.npz          EXHAUSTIVE: all 3^9 = 19 683 assignments of the nine cells x both movers (39 366 records, unreachable boards
                        included -- azg_set_states accepts any board, and a board on which both colours hold a line only exists there).
                        Record r = 2 * board + player, board = sum (cell_i + 1) 3^i, turns = the number of stones.  Per record: cells,
                        valid_moves, win_state, the observation (its values: small integers in float32, kept as int8) and, for every legal action, the record the
                        reference's play_action leads to (board, player and turns of the successor are checked against that record); the
                        8 symmetries of 1024 boards and the policy permutation of each (checked on every board)
  tt_tree.npz           single-tree MCTS traces (make_goldens.gen_tree): the empty board and mid-game roots; random priors (default,
                        cpuct2 = train.py's cpuct, noise, noise_temp) and UNIFORM priors (uniform, uniform_noise_temp: every PUCT comparison
                        at a fresh node is an exact tie); root probabilities at temperatures 1, .5, .25, .2, 0
  tt_edge.npz           the tree edge family (make_goldens.gen_edge): uniform, dyadic, one-hot (zero priors) and spread (denormal priors)
                        rows on random roots and on roots with exactly one legal move (one move from a full board) and two
  tt_agent.npz          SelfPlayAgent lock-step traces (make_goldens.gen_agent): plain (raw samples), symmetric (symmetricSamples),
                        fastmix (probFastSim 0.5) and a warm-up agent.  max_turns() is None for this env, so the temperature stays at
                        startTemp for the whole game (utils.py:19-23); the generator ASSERTS that, and that the plain and symmetric
                        agents' sampled moves differ from a run whose temp_scaling_fn halves the temperature after every move (what a
                        max_turns of 9 would do: int(0.15 * 9) == 1), so the fixture tells the two schedules apart
  tt_mt19937_agent.npz  a whole SelfPlayAgent under np.random.seed(s), every draw observed (make_goldens.gen_c4_mt19937_agent)
The tree / agent helpers of make_goldens.py ask the oracle for the game's sizes (oracle_lib.game_info); the oracle has no tic-tac-toe, so
this script answers that one call for game id 5 in-process and hands every other id through.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as mg  # noqa: E402
import refharness as rh  # noqa: E402
from refharness import ol  # noqa: E402

GAME_TICTACTOE = 5
_oracle_game_info = ol.game_info


def game_info(game):
    if game != GAME_TICTACTOE:
        return _oracle_game_info(game)
    gi = ol.GameInfo()
    (gi.action_size, gi.obs_c, gi.obs_h, gi.obs_w, gi.num_players, gi.has_draw, gi.max_turns, gi.num_symmetries, gi.cells,
     gi.max_children) = 9, 1, 3, 3, 2, 1, 9, 8, 9, 9
    return gi


ol.game_info = game_info


def ref_game():
    from alphazero.envs.tictactoe.tictactoe import Game
    return Game


def cells_of(g):
    return np.asarray(g._board.pieces, dtype=np.int8).reshape(-1)


def board_index(cells):
    return int(sum((int(c) + 1) * 3 ** i for i, c in enumerate(cells)))


def built(Game, cells, player):
    """the reference's Game on an arbitrary board: pieces as the list of lists Board.__init__ makes (TicTacToeLogic.py:31-37)"""
    g = Game()
    g._board.pieces = [[int(cells[3 * x + y]) for y in range(3)] for x in range(3)]
    g._player, g._turns = int(player), int((np.asarray(cells) != 0).sum())
    return g


def gen_rules(out_dir, verbose=True):
    Game = ref_game()
    N = 2 * 3 ** 9
    cells = np.zeros((N, 9), np.int8); player = np.zeros(N, np.int8); turns = np.zeros(N, np.int8)
    valids = np.zeros((N, 9), np.uint8); ws = np.zeros((N, 3), np.uint8); obs = np.zeros((N, 9), np.int8)
    succ = np.full((N, 9), -1, np.int32)
    sym_board = np.sort(np.random.RandomState(8642).choice(3 ** 9, 1024, replace=False)).astype(np.int32)
    sym_cells = np.zeros((len(sym_board), 8, 9), np.int8); sym_pi = np.zeros((8, 9), np.int8)
    both = 0
    for b in range(3 ** 9):
        c = np.array([(b // 3 ** i) % 3 - 1 for i in range(9)], np.int8)
        assert board_index(c) == b
        for p in (0, 1):
            r = 2 * b + p
            g = built(Game, c, p)
            cells[r], player[r], turns[r] = cells_of(g), g.player, g.turns
            valids[r] = np.asarray(g.valid_moves()).astype(np.uint8)
            ws[r] = np.asarray(g.win_state()).astype(np.uint8)
            o = np.asarray(g.observation())
            assert o.shape == (1, 3, 3) and o.dtype == np.float32 and (o == o.astype(np.int8)).all()
            obs[r] = o.reshape(-1).astype(np.int8)
            both += int(g._board.is_win(1) and g._board.is_win(-1))
            for a in np.flatnonzero(valids[r]):
                h = built(Game, c, p)
                h.play_action(int(a))
                s = 2 * board_index(cells_of(h)) + h.player
                assert h.player == 1 - p and h.turns == g.turns + 1
                succ[r, a] = s
        g = built(Game, c, b & 1)
        syms = g.symmetries(np.arange(9, dtype=np.float32))
        assert len(syms) == 8
        j = int(np.searchsorted(sym_board, b))
        keep = j < len(sym_board) and sym_board[j] == b
        for k, (gs, pi) in enumerate(syms):
            if keep:
                sym_cells[j, k] = cells_of(gs)
            if b == 0:
                sym_pi[k] = np.asarray(pi).astype(np.int8)
            # (on every board: the policy permutation is the same, and the board is permuted as the policy is)
            assert (np.asarray(pi).astype(np.int8) == sym_pi[k]).all() and gs.player == g.player and gs.turns == g.turns
            assert (cells_of(gs) == c[sym_pi[k]]).all()
        assert (sym_pi[7] == np.arange(9)).all()                 # the identity is the last entry
    # the successor records hold what the fixture says about them: the board with the mover's colour on cell a, the other mover, one more turn
    for r in range(N):
        for a in np.flatnonzero(valids[r]):
            s = succ[r, a]
            want = cells[r].copy(); want[a] = (1, -1)[player[r]]
            assert (cells[s] == want).all() and player[s] == 1 - player[r] and turns[s] == turns[r] + 1
    assert both > 0 and (valids == (cells == 0)).all()        # every empty cell is legal, also at a won position
    cov = np.array([N, int(ws[:, 0].sum()), int(ws[:, 1].sum()), int(ws[:, 2].sum()), both], np.int32)
    # (stored as succ - own record number: a constant per (action, mover), 2 * (+-3^a) + 1 - 2 * player, so it compresses to nothing)
    delta = np.where(succ >= 0, succ - np.arange(N, dtype=np.int32)[:, None], 0).astype(np.int32)
    np.savez_compressed(os.path.join(out_dir, 'tt_rules.npz'), cells=cells, player=player, turns=turns, valids=valids, ws=ws, obs=obs,
                        succ_delta=delta, sym_board=sym_board, sym_cells=sym_cells, sym_pi=sym_pi, coverage=cov,
                        coverage_names=np.array(['records', 'player0_wins', 'player1_wins', 'draws', 'both_lines']))
    if verbose:
        print('tt_rules: %d records, coverage %s' % (N, cov.tolist()))


# name, cpuct, fpu, noise, temp, sims; the `uniform*` configs are evaluated with uniform priors (gen_tree reads ol.fake_eval per call)
TREE_CONFIGS = [('default', 1.25, 0.2, False, False, 30), ('cpuct2', 2.0, 0.2, False, False, 30), ('noise', 1.25, 0.2, True, False, 24),
                ('noise_temp', 4.0, 0.4, True, True, 24)]
UNIFORM_CONFIGS = [('uniform', 1.25, 0.2, False, False, 30), ('uniform_noise_temp', 2.0, 0.0, True, True, 24)]
AGENT_CONFIGS = [
    ('plain', 4, 16, 8, dict(symmetricSamples=False)),       # raw samples: symmetries()[7] is the identity
    ('symmetric', 8, 12, 10, dict(add_root_noise=True, add_root_temp=True, cpuct=2.0)),
    ('fastmix', 4, 12, 8, dict(probFastSim=0.5, numFastSims=4, symmetricSamples=False)),
    ('warmup', 6, 10, 8, dict(numWarmupSims=5)),
]


def uniform_eval(seed, stream, step, A, NV):
    """uniform priors float32(1 / A) with the random value row of oracle_lib.fake_eval"""
    p, v = _fake_eval(seed, stream, step, A, NV)
    return np.full(A, np.float32(1.0) / np.float32(A), np.float32), v


_fake_eval = ol.fake_eval


def halving(cur_temp, turns, const_max_turns):
    """default_temp_scaling as a max_turns of 9 would make it: int(0.15 * 9) == 1, so every turn halves (utils.py:19-27)"""
    return max(0.2, cur_temp / 2)


def gen_tree(Game):
    mg.gen_tree(Game, GAME_TICTACTOE, 'tt', n_roots=8, seed=53, configs=TREE_CONFIGS, max_prefix=7)
    path = os.path.join(mg.OUT, 'tt_tree.npz')
    out = dict(np.load(path))
    ol.fake_eval = uniform_eval
    try:
        mg.gen_tree(Game, GAME_TICTACTOE, 'tt_uniform', n_roots=8, seed=53, configs=UNIFORM_CONFIGS, max_prefix=7)
    finally:
        ol.fake_eval = _fake_eval
    upath = os.path.join(mg.OUT, 'tt_uniform_tree.npz')
    u = dict(np.load(upath))
    os.remove(upath)
    assert (u['prefix'] == out['prefix']).all() and (u['prob_temps'] == out['prob_temps']).all()      # same seed: the same roots
    out.update({k: v for k, v in u.items() if k.startswith('uniform')})
    assert (out['prefix'][0] < 0).all() and (out['prefix'][1:] >= 0).any()                                # the empty board and mid-game roots
    np.savez_compressed(path, **out)


def gen_agent(Game):
    mg.gen_agent(Game, GAME_TICTACTOE, 'tt', configs=AGENT_CONFIGS, seed=717)
    path = os.path.join(mg.OUT, 'tt_agent.npz')
    out = dict(np.load(path))
    from alphazero.utils import default_temp_scaling
    assert Game.max_turns() is None
    t = 1.0
    for turn in range(12):                                    # SelfPlayAgent.playMoves (:156-157) on this env: the schedule never steps
        t = default_temp_scaling(t, turn, Game.max_turns())
        assert t == 1.0
    for ci, (cname, B, sims, games, kw) in enumerate(AGENT_CONFIGS):
        if cname not in ('plain', 'symmetric'):
            continue
        o, _ = mg.run_ref_agent(Game, GAME_TICTACTOE, cname, B, sims, games, dict(kw, temp_scaling_fn=halving), 717 + ci,
                                slot_base=0 if ci % 2 == 0 else 1000)
        a, b = out[cname + '_actions'], o['actions']
        n = min(len(a), len(b))
        assert a.shape != b.shape or (a != b).any(), cname
        out[cname + '_halving_differs_at'] = np.int32(next((r for r in range(n) if (a[r] != b[r]).any()), n))
        print('  tt/%s: a temperature halved after every move first changes a sampled move in round %d' % (cname, out[cname + '_halving_differs_at']))
    np.savez_compressed(path, **out)


def edge_roots(Game, seed, n_random=10, ks=(1, 2)):
    """reference games at the edge roots: random legal prefixes (the first is the empty board), then positions that are not decided and
    whose side to move has exactly k moves -- k = 1 is one move from a full board"""
    rng = np.random.RandomState(seed)
    roots, kinds = [], []
    for r in range(n_random):
        g = Game()
        for _ in range(0 if r == 0 else rng.randint(0, 7)):
            g2 = g.clone(); g2.play_action(int(rng.choice(np.flatnonzero(np.asarray(g.valid_moves())))))
            if np.asarray(g2.win_state()).any():
                break
            g = g2
        roots.append(g); kinds.append(0)
    for k in ks:
        for _ in range(2):                                    # two roots of each kind
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


# (coverage: the floors of make_goldens.EDGE_FLOORS, as the other games)
mg.EDGE_HOOKS['tt'] = dict(gid=GAME_TICTACTOE, sims=30, game_cls=ref_game, roots=edge_roots, cells=cells_of, agent=(4, 12, 8),
                           cov=[], floors={}, compact=False)


def main(which=None, out_dir=HERE, verbose=True):
    which = which or ['tt_rules', 'tt_tree', 'tt_edge', 'tt_agent', 'tt_mt19937_agent']
    rh.import_reference()
    mg.OUT = out_dir
    Game = ref_game()
    if 'tt_rules' in which:
        gen_rules(out_dir, verbose=verbose)
    if 'tt_tree' in which:
        gen_tree(Game)
    if 'tt_edge' in which:
        mg.gen_edge('tt', out_dir=out_dir, verbose=verbose)
    if 'tt_agent' in which:
        gen_agent(Game)
    if 'tt_mt19937_agent' in which:
        mg.gen_c4_mt19937_agent(B=4, sims=12, games=6, seed=20261019, eval_seed=101, Game=Game, gid=GAME_TICTACTOE, name='tt')


if __name__ == '__main__':
    main(sys.argv[1:] or None)
