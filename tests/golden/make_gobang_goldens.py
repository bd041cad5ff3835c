"""Generate the gobang golden vectors under tests/golden/ from the ACTUAL reference implementation (alphazero/envs/gobang).

Run in the build container only:   PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_gobang_goldens.py [which ...]
Outputs (small .npz fixtures, committed):
  gb_rules.npz          random playouts of the reference's gobang.Game: every position's cells, player, turns, a CRC of valid_moves,
                        win_state, observation CRC and the move played next; the 8 symmetries of a subset; boards built through
                        Board(_pieces=...) -- overlines, fives touching every edge and corner in all four directions, full-board draws,
                        both colours holding a five, runs of four that must not count (also across a row end) -- with the reference's
                        valid_moves CRC, win_state and observation CRC; coverage counts
  gb_tree.npz           single-tree MCTS traces (make_goldens.gen_tree): default, cpuct 4 / fpu 0.4, root temperature
  gb_agent.npz          SelfPlayAgent lock-step traces (make_goldens.gen_agent): plain, root temperature, fastmix (symmetricSamples=False +
                        probFastSim)
gb_tree and gb_agent have no root noise: with 225 children the Dirichlet alpha is 10.83 / 225, some draws lie below float32's normal
range, and the reference's cast of the noise to float32 raises FloatingPointError (underflow, MCTS.pyx:198-200 under
np.seterr(all='raise')) at the first noisy root.  gb_noise_tree.npz is the one noisy trace: make_goldens.gen_tree with root noise and
temperature, run inside np.errstate(under='ignore') -- the reference's own arithmetic, with only the underflow trap turned off (the tiny
draws become float32 denormals or zeros, as the cast rounds them).  There is no MT19937 whole-agent trace (that helper always adds noise).
  gb_edge.npz           the tree edge family (make_goldens.gen_edge, asked for by name: `gb_edge`): roots of 225 down to 1 legal moves
                        on both sides of every chunk of 64 children, 241 simulations each, and (under `rnd_`) four random prefixes of 1 to 29
                        stones, 48 simulations each; per simulation a crc of the counts row, the
                        full child arrays for the final tree.  Its noisy configs run, like gb_noise_tree, with only the underflow trap
                        off, and the roots whose noise cast underflowed are counted apart (noise_cast_underflows)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as mg  # noqa: E402
import refharness as rh  # noqa: E402
from refharness import ol  # noqa: E402

GAME_GOBANG, N = 4, 15
_oracle_game_info = ol.game_info


def game_info(game):
    if game != GAME_GOBANG:
        return _oracle_game_info(game)
    gi = ol.GameInfo()
    (gi.action_size, gi.obs_c, gi.obs_h, gi.obs_w, gi.num_players, gi.has_draw, gi.max_turns, gi.num_symmetries, gi.cells,
     gi.max_children) = 225, 4, 15, 15, 2, 1, 225, 8, 225, 225
    return gi


ol.game_info = game_info

# coverage floors of gb_rules.npz
RULE_FLOORS = dict(positions=10000, wins_0=20, wins_1=20, built=250, built_draws=4, built_both=8, built_overlines=8, built_short=40)
STEPS = ((1, 0), (0, 1), (1, 1), (1, -1))


def pack(cells):
    """225 int8 cells -> 64 bytes (include/azg.h gobang layout)"""
    b = np.asarray(cells, np.int8).reshape(N, N)
    out = np.zeros(64, np.uint8)
    for i, colour in enumerate((1, -1)):
        bits = np.zeros((16, 16), np.uint8)
        bits[:N, :N] = b == colour
        out[32 * i:32 * (i + 1)] = np.packbits(bits.reshape(-1), bitorder='little')
    return out


def ref_game():
    from alphazero.envs.gobang.gobang import Game
    return Game


def cells_of(g):
    return np.asarray(g._board.pieces, dtype=np.int8).reshape(-1)


def ref_from(Game, cells, player, turns):
    g = Game(_board=Game._get_board(_pieces=np.asarray(cells, np.intc).reshape(N, N).copy()))
    g._player, g._turns = int(player), int(turns)
    return g


def record(cols, g):
    v = np.asarray(g.valid_moves()).astype(np.uint8)
    w = np.asarray(g.win_state()).astype(np.uint8)
    o = np.asarray(g.observation())
    assert o.shape == (4, N, N)
    cols['cells'].append(pack(cells_of(g))); cols['player'].append(g.player); cols['turns'].append(g.turns)
    cols['valid_crc'].append(rh.crc(v)); cols['ws'].append(w); cols['obs_crc'].append(rh.crc(o.astype(np.float32)))
    return v, w


def line(b, x, y, dx, dy, n, c):
    for k in range(n):
        b[x + dx * k, y + dy * k] = c


def fits(x, y, dx, dy, n):
    return all(0 <= x + dx * k < N and 0 <= y + dy * k < N for k in range(n))


def built_boards(rng):
    """(kind, board) pairs built by hand; the reference decides what they are"""
    out = []
    for dx, dy in STEPS:                                  # fives starting on every border cell, both colours alternating
        for x in range(N):
            for y in range(N):
                if (x in (0, N - 1) or y in (0, N - 1) or (x + dx * 4) in (0, N - 1) or (y + dy * 4) in (0, N - 1)) and fits(x, y, dx, dy, 5):
                    b = np.zeros((N, N), np.int8)
                    line(b, x, y, dx, dy, 5, 1 if (x + y) % 2 == 0 else -1)
                    out.append(('edge', b))
    for dx, dy in STEPS:                                  # overlines of six and seven
        for n in (6, 7):
            for c in (1, -1):
                while True:
                    x, y = rng.randint(N), rng.randint(N)
                    if fits(x, y, dx, dy, n):
                        break
                b = np.zeros((N, N), np.int8)
                line(b, x, y, dx, dy, n, c)
                out.append(('overline', b))
    for dx, dy in STEPS:                                  # fours: in the open, blocked, and bent over a row end of the flat cell order
        for t in range(6):
            while True:
                x, y = rng.randint(N), rng.randint(N)
                if fits(x, y, dx, dy, 4):
                    break
            b = np.zeros((N, N), np.int8)
            line(b, x, y, dx, dy, 4, 1 if t % 2 == 0 else -1)
            if fits(x, y, dx, dy, 5):
                b[x + dx * 4, y + dy * 4] = -b[x, y]
            out.append(('short', b))
        for x in range(N - 4):                            # the 5th stone where a flat (15x + y) shift would wrap to
            b = np.zeros((N, N), np.int8)
            if (dx, dy) == (0, 1):
                line(b, x, N - 4, 0, 1, 4, 1); b[x + 1, 0] = 1
            elif (dx, dy) == (1, 0):
                line(b, N - 4, x, 1, 0, 4, -1); b[0, x + 1] = -1
            elif (dx, dy) == (1, 1):
                line(b, x, N - 4, 1, 1, 4, 1); b[x + 4, 0] = 1
            else:
                line(b, x, 3, 1, -1, 4, -1); b[x + 3, N - 1] = -1
            out.append(('short', b))
    for t in range(16):                                   # both colours hold a five: the scan's first start cell decides
        b = np.zeros((N, N), np.int8)
        d1, d2 = STEPS[t % 4], STEPS[(t // 4) % 4]
        while True:
            x1, y1, x2, y2 = rng.randint(N, size=4)
            if fits(x1, y1, *d1, 5) and fits(x2, y2, *d2, 5):
                c1 = [(x1 + d1[0] * k, y1 + d1[1] * k) for k in range(5)]
                c2 = [(x2 + d2[0] * k, y2 + d2[1] * k) for k in range(5)]
                if not set(c1) & set(c2):
                    break
        for p in c1:
            b[p] = 1 if t % 2 == 0 else -1
        for p in c2:
            b[p] = -1 if t % 2 == 0 else 1
        out.append(('both', b))
    # full boards: rows of a two-on two-off pattern, shifted so that no line of five forms -- draws; then one stone changed to make a five
    x, y = np.meshgrid(np.arange(N), np.arange(N), indexing='ij')
    for s in range(4):
        full = np.where(((y + s) // 2 + x) % 2 == 0, 1, -1).astype(np.int8)
        out.append(('full', full))
        full2 = full.T.copy()
        out.append(('full', full2))
        won = full.copy(); won[s:s + 5, 3] = 1
        out.append(('full', won))
        hole = full.copy(); hole[7, 7 + s] = 0
        out.append(('full', hole))
    return out


def gen_rules(out_dir, seed=2468, n_sym=128, n_games=None, verbose=True):
    Game = ref_game()
    rng = np.random.RandomState(seed)
    cols = {k: [] for k in ('cells', 'player', 'turns', 'valid_crc', 'ws', 'obs_crc', 'next', 'lens', 'kind')}
    cov = dict(wins_0=0, wins_1=0)
    games = 0
    while len(cols['lens']) < RULE_FLOORS['positions'] or any(cov[k] < RULE_FLOORS[k] for k in cov):
        g, L = Game(), 0
        while True:
            v, w = record(cols, g)
            cols['lens'].append(L); cols['kind'].append(0)
            if w.any():
                cols['next'].append(-1)
                if w[0]:
                    cov['wins_0'] += 1
                elif w[1]:
                    cov['wins_1'] += 1
                break
            a = int(rng.choice(np.flatnonzero(v)))
            cols['next'].append(a)
            g.play_action(a); L += 1
        games += 1
    n_play = len(cols['lens'])
    kinds = {'edge': 1, 'overline': 2, 'short': 3, 'both': 4, 'full': 5}
    bcov = dict(built=0, built_draws=0, built_both=0, built_overlines=0, built_short=0)
    for kind, b in built_boards(rng):
        turns = int((b != 0).sum())
        g = ref_from(Game, b.reshape(-1), turns % 2, turns)
        v, w = record(cols, g)
        cols['lens'].append(-1); cols['next'].append(-1); cols['kind'].append(kinds[kind])
        bcov['built'] += 1
        bcov['built_draws'] += int(w[2])
        bcov['built_both'] += int(kind == 'both')
        bcov['built_overlines'] += int(kind == 'overline' and bool(w[:2].any()))
        bcov['built_short'] += int(kind == 'short' and not w.any())
        assert kind != 'short' or not w.any(), 'a run of four counted'
        assert kind not in ('edge', 'overline', 'both') or w[:2].any(), kind
    n = len(cols['lens'])
    # the 8 symmetries of a subset of the playouts (gobang.pyx:159-182), pi = the action index so that the permutation is recorded
    pick = np.sort(rng.choice(n_play, n_sym, replace=False))
    sym_cells = np.zeros((n_sym, 8, 64), np.uint8); sym_pi = np.zeros((n_sym, 8, 225), np.uint8)
    for j, i in enumerate(pick):
        g = ref_from(Game, unpack(cols['cells'][i]), cols['player'][i], cols['turns'][i])
        syms = g.symmetries(np.arange(225, dtype=np.float32))
        assert len(syms) == 8
        for k, (gs, pi) in enumerate(syms):
            sym_cells[j, k] = pack(cells_of(gs)); sym_pi[j, k] = np.asarray(pi).astype(np.uint8)
            assert gs.player == g.player and gs.turns == g.turns
        assert (sym_cells[j, 7] == cols['cells'][i]).all() and (sym_pi[j, 7] == np.arange(225)).all()   # the identity is the last entry
    names = ['positions', 'wins_0', 'wins_1'] + list(bcov)
    counts = np.array([n_play, cov['wins_0'], cov['wins_1']] + list(bcov.values()), np.int32)
    for k, c in zip(names, counts):
        assert c >= RULE_FLOORS[k], (k, c)
    np.savez_compressed(os.path.join(out_dir, 'gb_rules.npz'), cells=np.array(cols['cells']), player=np.array(cols['player'], np.int8),
                        turns=np.array(cols['turns'], np.uint8), valid_crc=np.array(cols['valid_crc'], np.uint32), ws=np.array(cols['ws']),
                        obs_crc=np.array(cols['obs_crc'], np.uint32), next=np.array(cols['next'], np.int16), lens=np.array(cols['lens'], np.int16),
                        kind=np.array(cols['kind'], np.int8), sym_index=pick.astype(np.int32), sym_cells=sym_cells, sym_pi=sym_pi,
                        coverage=counts, coverage_names=np.array(names))
    if verbose:
        print('gb_rules: %d playout positions of %d games + %d built boards, coverage %s' % (n_play, games, n - n_play, dict(zip(names, counts.tolist()))))


def unpack(raw):
    raw = np.asarray(raw, np.uint8)
    out = np.zeros((N, N), np.int8)
    for i, colour in enumerate((1, -1)):
        bits = np.unpackbits(raw[32 * i:32 * (i + 1)], bitorder='little').reshape(16, 16)[:N, :N]
        out[bits != 0] = colour
    return out.reshape(-1)


TREE_CONFIGS = [('default', 1.25, 0.2, False, False, 60), ('cpuct4', 4.0, 0.4, False, False, 60), ('temp', 4.0, 0.4, False, True, 40)]
NOISE_CONFIGS = [('noise_temp', 4.0, 0.4, True, True, 40)]
AGENT_CONFIGS = [
    ('plain', 2, 8, 2, dict()),
    ('temp', 2, 6, 2, dict(add_root_temp=True, cpuct=4.0, fpu_reduction=0.4)),
    ('fastmix', 2, 6, 2, dict(probFastSim=0.5, numFastSims=3, symmetricSamples=False)),   # raw samples: symmetries()[7] is the identity
]


EDGE_KS = (193, 192, 191, 129, 128, 127, 66, 65, 64, 63, 2, 1)
EDGE_FLOORS = dict(chosen_chunk1=100, chosen_chunk2=100, chosen_chunk3=100, tie_spans_chunks=500, nc_switch=50,
                   zero_prior_selected_wide=20, seen_sum_serial_over128=50)


def edge_roots(Game, seed, n_random=1, exact=True):
    """reference games at the edge roots: random legal prefixes (the first one empty: 225 children), then one root per k of EDGE_KS
    with exactly k = 225 - stones legal moves -- random legal playouts that reject a move completing a five, and for k = 2 and 1 a
    full-board draw pattern of built_boards with two stones and one stone taken off"""
    rng = np.random.RandomState(seed)
    roots, kinds = [], []

    def playout(n):
        g = Game()
        for a in rng.permutation(N * N):
            if g.turns == n:
                break
            g2 = g.clone(); g2.play_action(int(a))
            if not np.asarray(g2.win_state()).any():
                g = g2
        assert g.turns == n
        return g
    for r in range(n_random):
        roots.append(playout(0 if r == 0 and exact else rng.randint(1, 30))); kinds.append(0)
    if not exact:
        return roots, kinds
    full = next(b for kind, b in built_boards(np.random.RandomState(seed)) if kind == 'full' and (b != 0).all())
    for k in EDGE_KS:
        if k > 2:
            g = playout(N * N - k)
        else:
            b = full.copy()
            b.reshape(-1)[rng.choice(N * N, k, replace=False)] = 0
            g = ref_from(Game, b.reshape(-1), (N * N - k) % 2, N * N - k)
        roots.append(g); kinds.append(k)
    return roots, kinds


mg.EDGE_HOOKS['gb'] = dict(gid=GAME_GOBANG, sims=241, game_cls=ref_game, roots=edge_roots, cells=lambda g: pack(cells_of(g)),
                           agent=(2, 8, 2), cov=mg.EDGE_COV_WIDE, floors=EDGE_FLOORS, compact=True,
                           extra=dict(prefix='rnd_', sims=48, roots=lambda Game, seed: edge_roots(Game, seed, 4, exact=False)))


def main(which=None, out_dir=HERE, verbose=True):
    which = which or ['gb_rules', 'gb_tree', 'gb_noise_tree', 'gb_agent']
    rh.import_reference()
    mg.OUT = out_dir
    Game = ref_game()
    if 'gb_rules' in which:
        gen_rules(out_dir, verbose=verbose)
    if 'gb_tree' in which:
        mg.gen_tree(Game, GAME_GOBANG, 'gb', n_roots=8, seed=41, configs=TREE_CONFIGS, max_prefix=60)
    if 'gb_noise_tree' in which:
        with np.errstate(under='ignore'):                 # (only the underflow trap: see the module docstring)
            mg.gen_tree(Game, GAME_GOBANG, 'gb_noise', n_roots=8, seed=43, configs=NOISE_CONFIGS, max_prefix=60)
    if 'gb_agent' in which:
        mg.gen_agent(Game, GAME_GOBANG, 'gb', configs=AGENT_CONFIGS, seed=717)
    if 'gb_edge' in which:
        mg.gen_edge('gb', out_dir=out_dir, verbose=verbose)


if __name__ == '__main__':
    main(sys.argv[1:] or None)
