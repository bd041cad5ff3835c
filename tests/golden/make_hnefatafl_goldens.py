"""Generate the hnefatafl golden vectors under tests/golden/ from the ACTUAL reference implementation (alphazero/envs/hnefatafl/fastafl.pyx on
fastafl/cengine.pyx, variants.hnefatafl_args).

Run in the build container only:   PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_hnefatafl_goldens.py [which ...]
Outputs (small .npz fixtures, committed; there is no C oracle for this game -- the host env and these fixtures are the checkers):
  hn_rules.npz   records in sequences: record i + 1 is the position the reference reaches from record i by `next[i]` wherever next[i] >= 0.
                 Random playouts (kind 0; whole games until the position floor is met, of the later ones the last TAIL positions) and king-hunting playouts
                 (kind 1: with probability 0.9 black moves next to the king when it can -- they end in a player-0 win), then boards built
                 through Game(Board(text, False)) (kind >= 2, names in `kind_names`), each in all eight symmetries and placed so that one
                 instance straddles cells 63 | 64 and rows 5 | 6: custodian captures by each side, against the throne and a corner, the
                 king NOT taken by two-sided capture, the five king-capture cases, group surround on an edge with and without the king, a
                 side without legal moves, the king on an escape square, slides across and beside the empty throne, a board at turn 512
                 with the king on a corner (a draw), and the board with the most legal moves a hill climb from sparse boards found
                 (`max_moves`).  Per record: cells, player, turns, aux0 (Board._king_captured), a CRC of valid_moves and the move count,
                 win_state, a CRC of the observation, next.  The 8 symmetries of a subset with an asymmetric pi.  Coverage floors
                 (RULE_FLOORS) are asserted here and again by tests/test_hnefatafl_cpu.py.
  hn_tree.npz    single-tree MCTS traces (make_goldens.gen_tree): default, cpuct 4 / fpu 0.4, root temperature; the 2420-wide per-simulation
                 rows are kept as CRCs
  hn_edge.npz    the same traces at edge roots: exactly 64 | 65, 128 | 129, 192 | 193 and 256 | 257 legal moves (every chunk boundary of the
                 child list), and undecided positions at turns 508..511, whose leaves meet the turn-512 draw inside the tree; a default and
                 a noisy config (root noise + temperature, run with only the float32 underflow trap off, underflowed casts counted)
  hn_agent.npz   SelfPlayAgent lock-step traces (make_goldens.run_ref_agent): plain, symmetric with root temperature, fastmix, warm-up
                 and `long` (B = 2, 2 simulations per move, raw samples, run until a game ends in the turn-512 draw); counts, sample
                 observations and sample policies are kept as CRCs plus the policies' non-zero entries
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as mg  # noqa: E402
import refharness as rh  # noqa: E402
from refharness import ol  # noqa: E402

GAME_HNEFATAFL, N, A, MT = 6, 11, 2420, 20
_oracle_game_info = ol.game_info


def game_info(game):
    if game != GAME_HNEFATAFL:
        return _oracle_game_info(game)
    gi = ol.GameInfo()
    (gi.action_size, gi.obs_c, gi.obs_h, gi.obs_w, gi.num_players, gi.has_draw, gi.max_turns, gi.num_symmetries, gi.cells,
     gi.max_children) = A, 5, N, N, 2, 1, 512, 8, N * N, 448
    return gi


ol.game_info = game_info

RULE_FLOORS = dict(positions=10000, wins_0=20, wins_1=20, draws=20, band_1_64=50, band_65_128=50, band_129_192=50, band_over_192=50)
TAIL = 40


def ref_game():
    """the reference's Game is a cdef class without has_draw() / max_turns(): the harness adds the two static methods"""
    from alphazero.envs.hnefatafl.fastafl import Game

    class HGame(Game):
        @staticmethod
        def has_draw():
            return True

        @staticmethod
        def max_turns():
            return 512
    return HGame


def cells_of(g):
    return np.asarray(g._board._state, dtype=np.int8).reshape(-1)


def build(Game, cells, turns=0, kc=0):
    """the reference's Game on an arbitrary board"""
    from fastafl.cengine import Board
    c = np.asarray(cells).reshape(N, N)
    g = Game(Board('\n'.join(''.join(str(int(v)) for v in row) for row in c), False))
    g._board.num_turns = int(turns)
    g._board._king_captured = bool(kc)
    g._player, g._turns = int(turns) % 2, int(turns)
    return g


def action_of(src, dst):
    (x, y), (nx, ny) = src, dst
    mt = (ny if ny < y else ny - 1) if x == nx else (N - 1 + nx - (1 if nx >= x else 0))
    return MT * (x + y * N) + mt


def record(cols, g, kind):
    v = np.asarray(g.valid_moves()).astype(np.uint8)
    w = np.asarray(g.win_state()).astype(np.uint8)
    o = np.asarray(g.observation())
    assert o.shape == (5, N, N) and o.dtype == np.float32 and v.shape == (A,)
    cols['cells'].append(cells_of(g)); cols['player'].append(g.player); cols['turns'].append(g.turns)
    cols['aux0'].append(int(g._board._king_captured))
    cols['valid_crc'].append(rh.crc(v)); cols['nvalid'].append(int(v.sum())); cols['ws'].append(w)
    cols['obs_crc'].append(rh.crc(o)); cols['kind'].append(kind); cols['next'].append(-1)
    return v, w


def playout(Game, rng, hunt):
    """one game of the reference: [(game clone, valid, win_state, move played or -1)]"""
    g, out = Game(), []
    while True:
        v = np.asarray(g.valid_moves()).astype(np.uint8); w = np.asarray(g.win_state()).astype(np.uint8)
        if w.any():
            out.append((g.clone(), -1))
            return out, w
        legal = np.flatnonzero(v)
        pick = legal
        if hunt and g.player == 0 and rng.rand() < 0.9:        # black moves next to the king when it can
            s = np.asarray(g._board._state)
            ky, kx = [int(t[0]) for t in np.nonzero(np.isin(s, (3, 7, 8)))]
            near = []
            for a in legal:
                mt, c = a % MT, a // MT
                x, y = c % N, c // N
                nx, ny = (x, mt + (1 if mt >= y else 0)) if mt < N - 1 else ((mt - N + 1) + (1 if mt - N + 1 >= x else 0), y)
                if abs(nx - kx) + abs(ny - ky) == 1:
                    near.append(a)
            if near:
                pick = np.array(near)
        a = int(pick[rng.randint(len(pick))])
        out.append((g.clone(), a))
        g.play_action(a)


def base_board():
    b = np.zeros((N, N), np.int8)
    b[5, 5] = 4
    b[0, 0] = b[0, N - 1] = b[N - 1, 0] = b[N - 1, N - 1] = 5
    return b


def scenarios():
    """(name, board [y, x], turns, move ((x, y), (nx, ny)) or None) built by hand; the reference decides what they are.  Black = code 2 moves
    at even turns, white = code 1 and the king at odd ones."""
    out = []

    def add(name, pieces, turns, move=None, extra=True):
        b = base_board()
        for (x, y), v in pieces.items():
            b[y, x] = v
        if extra:                                          # a free piece of each side far away, so that nobody is out of moves
            for (x, y), v in (((1, 9), 2), ((2, 8), 1)):
                if b[y, x] == 0:
                    b[y, x] = v
        out.append((name, b, turns, move))
    # custodian captures across cells 63 | 64 (row 5, x = 8 | 9) and across rows 5 | 6
    add('custodian_black', {(9, 5): 1, (10, 5): 2, (8, 8): 2}, 0, ((8, 8), (8, 5)))
    add('custodian_white', {(9, 5): 2, (10, 5): 1, (8, 8): 1}, 1, ((8, 8), (8, 5)))
    add('custodian_white_king_partner', {(9, 5): 2, (10, 5): 3, (8, 8): 1}, 1, ((8, 8), (8, 5)))
    add('custodian_king_moves', {(9, 5): 2, (10, 5): 1, (8, 8): 3}, 1, ((8, 8), (8, 5)))
    add('custodian_black_rows', {(3, 6): 1, (3, 7): 2, (0, 5): 2}, 0, ((0, 5), (3, 5)))
    add('custodian_white_rows', {(3, 6): 2, (3, 7): 1, (0, 5): 1}, 1, ((0, 5), (3, 5)))
    add('custodian_double', {(9, 5): 1, (10, 5): 2, (8, 4): 1, (8, 3): 2, (8, 6): 1, (8, 7): 2, (4, 5): 2}, 0, ((4, 5), (8, 5)))
    add('throne_black', {(6, 5): 1, (7, 8): 2}, 0, ((7, 8), (7, 5)))
    add('throne_white', {(6, 5): 2, (7, 8): 1}, 1, ((7, 8), (7, 5)))
    add('throne_rows', {(5, 6): 1, (8, 7): 2}, 0, ((8, 7), (5, 7)))
    add('corner_black', {(1, 0): 1, (2, 4): 2}, 0, ((2, 4), (2, 0)))
    add('corner_white', {(1, 0): 2, (2, 4): 1}, 1, ((2, 4), (2, 0)))
    add('king_not_two_sided', {(9, 5): 3, (10, 5): 2, (8, 8): 2}, 0, ((8, 8), (8, 5)))
    add('king_not_two_sided_rows', {(3, 6): 3, (3, 7): 2, (0, 5): 2}, 0, ((0, 5), (3, 5)))
    # the five king-capture cases (static), and the fourth defender arriving by a move
    add('kingcap_edge_3', {(5, 0): 3, (4, 0): 2, (6, 0): 2, (5, 1): 2}, 1)
    add('kingcap_edge_3_right', {(10, 5): 3, (10, 4): 2, (10, 6): 2, (9, 5): 2}, 1)
    add('kingcap_throne_3', {(5, 4): 3, (5, 3): 2, (4, 4): 2, (6, 4): 2}, 1)
    add('kingcap_throne_3_rows', {(5, 6): 3, (5, 7): 2, (4, 6): 2, (6, 6): 2}, 0)
    add('kingcap_corner_2', {(1, 0): 3, (2, 0): 2, (1, 1): 2}, 1)
    add('kingcap_open_3_not', {(8, 5): 3, (7, 5): 2, (9, 5): 2, (8, 4): 2}, 1)
    add('kingcap_open_4', {(8, 5): 3, (7, 5): 2, (9, 5): 2, (8, 4): 2, (8, 6): 2}, 1)
    add('kingcap_open_4_by_move', {(8, 5): 3, (7, 5): 2, (9, 5): 2, (8, 4): 2, (8, 9): 2}, 0, ((8, 9), (8, 6)))
    add('kingcap_open_3_white_beside', {(8, 5): 3, (7, 5): 2, (9, 5): 2, (8, 4): 2, (8, 6): 1}, 0)
    # group surround on an edge, with and without the king in the group
    add('surround_black_takes', {(10, 5): 1, (10, 6): 1, (10, 4): 2, (10, 7): 2, (9, 5): 2, (9, 9): 2}, 0, ((9, 9), (9, 6)))
    add('surround_white_takes', {(10, 5): 2, (10, 6): 2, (10, 4): 1, (10, 7): 1, (9, 5): 1, (9, 9): 1}, 1, ((9, 9), (9, 6)))
    add('surround_with_king', {(10, 5): 3, (10, 6): 1, (10, 4): 2, (10, 7): 2, (9, 5): 2, (9, 9): 2}, 0, ((9, 9), (9, 6)))
    add('surround_top', {(4, 0): 1, (5, 0): 1, (3, 0): 2, (6, 0): 2, (4, 1): 2, (5, 4): 2}, 0, ((5, 4), (5, 1)))
    add('surround_top_king', {(4, 0): 1, (5, 0): 3, (3, 0): 2, (6, 0): 2, (4, 1): 2, (5, 4): 2}, 0, ((5, 4), (5, 1)))
    add('surround_open_not', {(10, 5): 1, (10, 6): 1, (10, 4): 2, (9, 5): 2, (9, 9): 2}, 0, ((9, 9), (9, 6)))
    add('surround_two_groups', {(10, 5): 1, (10, 6): 1, (10, 4): 2, (10, 7): 2, (9, 5): 2, (8, 6): 1, (7, 6): 2, (8, 5): 2, (8, 7): 2, (9, 9): 2},
        0, ((9, 9), (9, 6)))
    # a side without legal moves
    add('black_no_moves', {(1, 0): 2, (2, 0): 1, (1, 1): 1, (7, 7): 3}, 0, extra=False)
    add('white_no_moves', {(1, 0): 1, (2, 0): 2, (1, 1): 2}, 1, extra=False)
    add('white_no_moves_king', {(1, 0): 1, (2, 0): 2, (1, 1): 2, (10, 5): 3, (10, 4): 2, (10, 6): 2, (9, 5): 1, (8, 5): 2, (9, 4): 2, (9, 6): 2}, 1,
        extra=False)
    add('black_only_over_throne', {(4, 5): 2, (3, 5): 1, (4, 4): 1, (4, 6): 1, (8, 8): 3}, 0, extra=False)
    # the king on an escape square, reaching one, leaving the throne; slides across and beside the empty throne
    add('king_on_escape', {(0, 0): 8}, 0)
    add('king_escapes', {(3, 0): 3}, 1, ((3, 0), (0, 0)))
    add('king_escapes_right', {(10, 5): 3}, 1, ((10, 5), (10, 10)))
    add('king_leaves_throne', {(5, 5): 7}, 1, ((5, 5), (5, 3)))
    add('king_beside_throne', {(5, 4): 3, (4, 5): 1, (6, 5): 2}, 1)
    add('slide_over_throne', {(2, 5): 1}, 1, ((2, 5), (8, 5)))
    add('slide_over_throne_black', {(5, 9): 2, (9, 5): 2}, 0, ((5, 9), (5, 2)))
    add('slide_beside_throne', {(4, 2): 1, (6, 8): 2}, 1, ((4, 2), (4, 8)))
    add('throne_blocked_by_king', {(5, 5): 7, (2, 5): 1, (5, 8): 2}, 1)
    add('turn_512_king_on_corner', {(10, 10): 8}, 512)
    add('turn_511_last_move', {(3, 0): 3}, 511, ((3, 0), (0, 0)))
    return out


def transform(b, move, k):
    """symmetry k = 2 (i - 1) + flip of a board [y, x] and a move, as Game.symmetries orders them"""
    i, flip = k // 2 + 1, k & 1
    b2 = np.rot90(b, i)
    if flip:
        b2 = np.fliplr(b2)

    def pt(p):
        x, y = p
        for _ in range(i):
            x, y = y, N - 1 - x                            # np.rot90: old [r][c] -> new [N - 1 - c][r]
        if flip:
            x = N - 1 - x
        return x, y
    return np.ascontiguousarray(b2), (None if move is None else (pt(move[0]), pt(move[1])))


def hill_climb(Game, rng, steps=2500):
    """the board with the most legal moves found by moving one piece at a time, from sparse boards of 20 movers"""
    best_k, best = -1, None
    for start in range(3):
        b = base_board()
        free = [(y, x) for y in range(N) for x in range(N) if b[y, x] == 0]
        idx = rng.permutation(len(free))
        for j in idx[:20]:
            b[free[j]] = 2
        b[free[idx[20]]] = 3; b[free[idx[21]]] = 1
        k = int(np.asarray(build(Game, b).valid_moves()).sum())
        for _ in range(steps // 3):
            movers = np.argwhere(b == 2); empt = np.argwhere(b == 0)
            m, e = movers[rng.randint(len(movers))], empt[rng.randint(len(empt))]
            b2 = b.copy(); b2[tuple(m)] = 0; b2[tuple(e)] = 2
            k2 = int(np.asarray(build(Game, b2).valid_moves()).sum())
            if k2 >= k:
                b, k = b2, k2
        if k > best_k:
            best_k, best = k, b
    return best, best_k


def gen_rules(out_dir, seed=1357, n_sym=48, verbose=True):
    Game = ref_game()
    rng = np.random.RandomState(seed)
    cols = {k: [] for k in ('cells', 'player', 'turns', 'aux0', 'valid_crc', 'nvalid', 'ws', 'obs_crc', 'kind', 'next')}
    cov = {k: 0 for k in RULE_FLOORS}
    games = [0, 0]

    def covered():
        return all(cov[k] >= RULE_FLOORS[k] for k in cov)
    while not covered():
        hunt = cov['wins_0'] < RULE_FLOORS['wins_0'] and (games[0] + games[1]) % 2 == 1
        seq, w = playout(Game, rng, hunt)
        keep = seq if cov['positions'] < RULE_FLOORS['positions'] else seq[-TAIL:]
        for g, a in keep:
            v, w2 = record(cols, g, int(hunt))
            cols['next'][-1] = a
            k = int(v.sum())
            cov['positions'] += 1
            cov['band_1_64' if k <= 64 else 'band_65_128' if k <= 128 else 'band_129_192' if k <= 192 else 'band_over_192'] += int(k > 0)
        cov['wins_0'] += int(w[0]); cov['wins_1'] += int(w[1]); cov['draws'] += int(w[2])
        games[int(hunt)] += 1
        if verbose:
            print('  game %d (%s): %d turns, ws %s, coverage %s' % (sum(games), 'hunt' if hunt else 'random', len(seq) - 1, w.tolist(), cov), flush=True)
    n_play = len(cols['kind'])
    names = ['random', 'hunt']
    seen_straddle = set()
    for name, b, turns, move in scenarios():
        names.append(name)
        for k in range(8):
            b2, mv = transform(b, move, k)
            g = build(Game, b2, turns)
            v, w = record(cols, g, len(names) - 1)
            if mv is not None:
                a = action_of(*mv)
                assert v[a], (name, k, mv)
                cols['next'][-1] = a
                g.play_action(a)
                record(cols, g, len(names) - 1)
                for c in ((mv[1][0] + N * mv[1][1]),):
                    seen_straddle.add(c)
    assert 63 in seen_straddle and 64 in seen_straddle
    top, max_moves = hill_climb(Game, rng)
    names.append('max_moves')
    for k in range(8):
        b2, _ = transform(top, None, k)
        v, w = record(cols, build(Game, b2, 0), len(names) - 1)
        assert int(v.sum()) == max_moves
    n = len(cols['kind'])
    for k, c in cov.items():
        assert c >= RULE_FLOORS[k], (k, c)
    # the 8 symmetries of a subset (fastafl.pyx:216-259) with an asymmetric pi: pi[a] = a + 1 on the legal moves, so the permutation shows
    pick = np.sort(np.concatenate([rng.choice(n_play, n_sym - 8, replace=False), n_play + rng.choice(n - n_play, 8, replace=False)]))
    sym_cells = np.zeros((n_sym, 8, N * N), np.int8); sym_pi_crc = np.zeros((n_sym, 8), np.uint32)
    for j, i in enumerate(pick):
        g = build(Game, cols['cells'][i], cols['turns'][i], cols['aux0'][i])
        pi = (np.arange(A, dtype=np.float32) + 1) * np.asarray(g.valid_moves()).astype(np.float32)
        syms = g.symmetries(pi)
        assert len(syms) == 8
        for k, (gs, p) in enumerate(syms):
            sym_cells[j, k] = np.asarray(gs._board._state).astype(np.int8).reshape(-1); sym_pi_crc[j, k] = rh.crc(np.asarray(p, np.float32))
            assert gs.player == g.player and gs.turns == g.turns
        assert (sym_cells[j, 6] == cols['cells'][i]).all() and sym_pi_crc[j, 6] == rh.crc(pi)        # the identity is entry 6
    np.savez_compressed(os.path.join(out_dir, 'hn_rules.npz'), cells=np.array(cols['cells'], np.int8), player=np.array(cols['player'], np.int8),
                        turns=np.array(cols['turns'], np.int16), aux0=np.array(cols['aux0'], np.int8),
                        valid_crc=np.array(cols['valid_crc'], np.uint32), nvalid=np.array(cols['nvalid'], np.int16), ws=np.array(cols['ws'], np.uint8),
                        obs_crc=np.array(cols['obs_crc'], np.uint32), next=np.array(cols['next'], np.int16), kind=np.array(cols['kind'], np.int16),
                        kind_names=np.array(names), n_play=np.int32(n_play), max_moves=np.int32(max_moves),
                        sym_index=pick.astype(np.int32), sym_cells=sym_cells, sym_pi_crc=sym_pi_crc,
                        coverage=np.array([cov[k] for k in RULE_FLOORS], np.int32), coverage_names=np.array(list(RULE_FLOORS)))
    if verbose:
        print('hn_rules: %d playout positions of %d random + %d hunting games, %d built records, most legal moves built %d, coverage %s'
              % (n_play, games[0], games[1], n - n_play, max_moves, cov))


TREE_CONFIGS = [('default', 1.25, 0.2, False, False, 40), ('cpuct4', 4.0, 0.4, False, False, 40), ('temp', 4.0, 0.4, False, True, 30)]
# name, B, sims, games, max_rounds, kwargs
AGENT_CONFIGS = [
    ('plain', 2, 4, 1, 1100, dict(symmetricSamples=False)),                                      # raw samples: symmetries()[6] is the identity
    ('symmetric', 2, 3, 1, 1100, dict(add_root_temp=True, cpuct=4.0, fpu_reduction=0.4)),
    ('fastmix', 2, 5, 1, 1100, dict(probFastSim=0.5, numFastSims=3, symmetricSamples=False)),
    ('warmup', 2, 0, 1, 1100, dict(numWarmupSims=5)),
    ('long', 2, 2, 2, 2200, dict(symmetricSamples=False)),
]
EDGE_KS = (64, 65, 128, 129, 192, 193, 256, 257)
EDGE_TURNS = (508, 509, 510, 511)
EDGE_CONFIGS = [('default', 1.25, 0.2, False, False, 24), ('noise_temp', 4.0, 0.4, True, True, 24)]


def crc_rows(a):
    a = np.ascontiguousarray(a)
    return np.array([rh.crc(r) for r in a.reshape(-1, a.shape[-1])], np.uint32).reshape(a.shape[:-1])


def gen_tree(Game):
    mg.gen_tree(Game, GAME_HNEFATAFL, 'hn', n_roots=6, seed=61, configs=TREE_CONFIGS, max_prefix=80)
    path = os.path.join(mg.OUT, 'hn_tree.npz')
    out = dict(np.load(path))
    for cname in [c[0] for c in TREE_CONFIGS]:                # the 2420-wide rows as CRCs (rootn: int16 rows, probs / counts: whole)
        out[cname + '_rootn_crc'] = crc_rows(out.pop(cname + '_rootn'))
        out[cname + '_rootq_crc'] = crc_rows(out.pop(cname + '_rootq'))
        out[cname + '_counts_crc'] = crc_rows(out.pop(cname + '_counts'))
        out[cname + '_probs_crc'] = crc_rows(out.pop(cname + '_probs'))
    np.savez_compressed(path, **out)


def gen_agent(Game):
    out = {}
    for ci, (cname, B, sims, games, max_rounds, kw) in enumerate(AGENT_CONFIGS):
        slot_base = 0 if ci % 2 == 0 else 1000
        o, args = mg.run_ref_agent(Game, GAME_HNEFATAFL, cname, B, sims, games, kw, 919 + ci, slot_base=slot_base, max_rounds=max_rounds)
        assert o['games_played'][-1] >= games, (cname, 'max_rounds too small')
        if cname == 'long':
            assert (o['r_ws'][:, 2] == 1).any() and (o['r_turns'][o['r_ws'][:, 2] == 1] == 512).all(), 'no game of `long` ended in the turn-512 draw'
        cnt = o.pop('counts')                                  # [rounds, B, A]: as CRCs, and its few non-zero entries (action, visits)
        o['counts_crc'] = crc_rows(cnt)
        S = int((cnt != 0).sum(axis=2).max())
        nz_a = np.full(cnt.shape[:2] + (S,), -1, np.int16); nz_n = np.zeros(cnt.shape[:2] + (S,), np.int16)
        for r in range(cnt.shape[0]):
            for i in range(cnt.shape[1]):
                a = np.flatnonzero(cnt[r, i])
                nz_a[r, i, :len(a)] = a; nz_n[r, i, :len(a)] = cnt[r, i, a]
        o['counts_a'], o['counts_n'] = nz_a, nz_n
        o['s_obs_crc'] = crc_rows(o.pop('s_obs').reshape(len(o['s_z']), -1))
        pi = o.pop('s_pi')
        o['s_pi_crc'] = crc_rows(pi)
        o['s_pi_nnz'] = (pi != 0).sum(axis=1).astype(np.int16)
        o['s_pi_sum'] = pi.sum(axis=1, dtype=np.float64)
        for k, v in o.items():
            out[cname + '_' + k] = v
        out[cname + '_slot_base'] = slot_base
        print('  hn/%s: rounds=%d samples=%d results=%s turns=%s' % (cname, len(o['actions']), len(o['s_z']), o['r_ws'].tolist(), o['r_turns'].tolist()), flush=True)
    np.savez_compressed(os.path.join(mg.OUT, 'hn_agent.npz'), **out)


def edge_roots(Game, out_dir, seed=77):
    """(state, kind) roots: positions of hn_rules.npz's playouts with exactly k legal moves for the k of EDGE_KS below 225, boards one
    piece move away from the hill climb's best for the larger ones, and undecided playout positions at turns 508..511"""
    d = dict(np.load(os.path.join(out_dir, 'hn_rules.npz')))
    rng = np.random.RandomState(seed)
    n_play = int(d['n_play'])
    roots = []
    for k in EDGE_KS:
        hit = np.flatnonzero((d['nvalid'][:n_play] == k) & (d['next'][:n_play] >= 0))
        if len(hit):
            i = int(hit[rng.randint(len(hit))])
            roots.append(((d['cells'][i], int(d['player'][i]), int(d['turns'][i]), int(d['aux0'][i])), k))
    top = d['cells'][int(np.flatnonzero(d['kind'] == len(d['kind_names']) - 1)[0])].reshape(N, N)
    want = {k for k in EDGE_KS if k > 224 and k <= int(d['max_moves'])}
    b = top.copy()
    for _ in range(6000):
        if not want:
            break
        movers = np.argwhere(b == 2); empt = np.argwhere(b == 0)
        b2 = b.copy(); b2[tuple(movers[rng.randint(len(movers))])] = 0; b2[tuple(empt[rng.randint(len(empt))])] = 2
        g = build(Game, b2, 0)
        k = int(np.asarray(g.valid_moves()).sum())
        if k in want and not np.asarray(g.win_state()).any():
            want.discard(k)
            roots.append(((b2.reshape(-1).astype(np.int8), 0, 0, 0), k))
        if k >= 250:
            b = b2
    for t in EDGE_TURNS:
        hit = np.flatnonzero((d['turns'][:n_play] == t) & (d['next'][:n_play] >= 0))
        i = int(hit[rng.randint(len(hit))])
        roots.append(((d['cells'][i], int(d['player'][i]), int(d['turns'][i]), int(d['aux0'][i])), -t))
    return roots


def gen_edge(Game, out_dir, verbose=True):
    """single-tree traces (as make_goldens.gen_tree records them, the wide rows as CRCs) at the edge roots; the noisy config runs with only
    the float32 underflow trap off (alpha = 10.83 / k underflows the reference's cast now and then), the roots where it did counted apart"""
    from alphazero.MCTS import MCTS
    roots = edge_roots(Game, out_dir)
    R = len(roots)
    out = dict(cells=np.array([r[0][0] for r in roots], np.int8), player=np.array([r[0][1] for r in roots], np.int8),
               turns=np.array([r[0][2] for r in roots], np.int16), aux0=np.array([r[0][3] for r in roots], np.int8),
               kind=np.array([r[1] for r in roots], np.int16))
    NV = 3
    for (cname, cpuct, fpu, noise, temp, sims) in EDGE_CONFIGS:
        tape = rh.Tape(31000 + rh.crc(np.frombuffer(cname.encode(), np.uint8)) % 997)
        under = [0]
        real_dirichlet = tape.dirichlet

        def dirichlet(alpha):
            o = real_dirichlet(alpha)
            under[0] += int((o.astype(np.float32) < np.finfo(np.float32).tiny).any())
            return o
        tape.dirichlet = dirichlet
        tape.install()
        try:
            args = rh.ref_args(Game, cpuct=cpuct, fpu_reduction=fpu)
            depth = np.zeros((R, sims), np.int16); rootn_crc = np.zeros((R, sims), np.uint32); paths = np.full((R, sims, 8), -1, np.int16)
            leaf_e = np.zeros((R, sims), np.int8)
            fin = {k: [] for k in ('a', 'n', 'q', 'p', 'v', 'counts_crc', 'probs_crc', 'vmax', 'vavg', 'root_n', 'maxdepth', 'ctr', 'k')}
            with np.errstate(under='ignore'):
                for r, (st, kind) in enumerate(roots):
                    g = build(Game, st[0], st[2], st[3])
                    m = MCTS(args)
                    tape.stream = r
                    for s in range(sims):
                        leaf = m.find_leaf(g)
                        acts = [n.a for n in m._path[1:]] + ([m._curnode.a] if m._path else [])
                        depth[r, s] = m.depth; paths[r, s, :min(len(acts), 8)] = acts[:8]
                        e = np.asarray(m._curnode.e)
                        leaf_e[r, s] = int(e[0]) + 2 * int(e[1]) + 4 * int(e[2])
                        p, v = ol.fake_eval(tape.seed, r, s, A, NV)
                        m.process_results(leaf, v, p, noise, temp)
                        rootn_crc[r, s] = rh.crc(np.asarray(m.counts(g)).astype(np.int32))
                    ch = m._root._children
                    pad = 448 - len(ch)
                    fin['k'].append(len(ch))
                    fin['a'].append(np.array([c.a for c in ch] + [-1] * pad, np.int16))
                    fin['n'].append(np.array([c.n for c in ch] + [0] * pad, np.int32))
                    for f in ('q', 'p', 'v'):
                        fin[f].append(np.array([getattr(c, f) for c in ch] + [0] * pad, np.float32))
                    fin['counts_crc'].append(rh.crc(np.asarray(m.counts(g)).astype(np.int32)))
                    fin['probs_crc'].append([rh.crc(np.asarray(m.probs(g, t), np.float32)) for t in mg.PROB_TEMPS])
                    fin['vmax'].append(m.value(False)); fin['vavg'].append(m.value(True))
                    fin['root_n'].append(m._root.n); fin['maxdepth'].append(m.max_depth); fin['ctr'].append(tape.ctr[r])
            out[cname + '_seed'] = np.uint64(tape.seed)
            out[cname + '_cfg'] = np.array([cpuct, fpu, float(noise), float(temp), sims], np.float64)
            out[cname + '_depth'] = depth; out[cname + '_paths'] = paths; out[cname + '_rootn_crc'] = rootn_crc; out[cname + '_leaf_e'] = leaf_e
            out[cname + '_noise_cast_underflows'] = np.int32(under[0])
            for k, v in fin.items():
                out[cname + '_' + k] = np.array(v)
        finally:
            tape.uninstall()
        if verbose:
            print('  hn_edge/%s: %d roots, k %s, draws met inside the tree %d, noise casts that underflowed %d'
                  % (cname, R, fin['k'], int((leaf_e == 4).sum()), under[0]), flush=True)
    assert set(EDGE_KS) <= set(out['kind'].tolist()) | {k for k in EDGE_KS if k > int(np.load(os.path.join(out_dir, 'hn_rules.npz'))['max_moves'])}
    assert (out['default_leaf_e'][out['kind'] < 0] == 4).any()
    np.savez_compressed(os.path.join(out_dir, 'hn_edge.npz'), **out)


def main(which=None, out_dir=HERE, verbose=True):
    which = which or ['hn_rules', 'hn_tree', 'hn_edge', 'hn_agent']
    rh.import_reference()
    mg.OUT = out_dir
    Game = ref_game()
    if 'hn_rules' in which:
        gen_rules(out_dir, verbose=verbose)
    if 'hn_tree' in which:
        gen_tree(Game)
    if 'hn_edge' in which:
        gen_edge(Game, out_dir, verbose=verbose)
    if 'hn_agent' in which:
        gen_agent(Game)


if __name__ == '__main__':
    main(sys.argv[1:] or None)
