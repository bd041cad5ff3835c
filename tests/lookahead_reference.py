"""One ply on GameState objects, restated: the children of a position, perft, and the reference's three scripted baseline players
(OneStepLookaheadConnect4Player, envs/connect4/players.py:26-69; GreedyOthelloPlayer, envs/othello/OthelloPlayers.py:27-40;
GreedyGobangPlayer, envs/gobang/GobangPlayers.py:27-40) -- what azg_game_lookahead / azg_game_choose_scripted are held to.  Everything
here works on any GameState class (this package's host envs or the reference's own): clone / play_action / win_state / valid_moves.
tests/test_lookahead_cpu.py holds it to tests/golden/lookahead.npz, which tests/golden/make_lookahead_goldens.py made from the
reference's own player objects."""
import functools
import os

import numpy as np

C4, BR, TM, OT, GB, TT, HN = range(7)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'lookahead.npz')
SHORT = {C4: 'c4', BR: 'br', TM: 'tm', OT: 'ot', GB: 'gb', TT: 'tt', HN: 'hn'}
PERFT_DEPTH = {C4: 5, TT: 5, OT: 5, BR: 3, GB: 2, HN: 2, TM: 3}     # the largest depth whose frontier stays under about 50 000 nodes
SCRIPTED = {C4: 'OneStepLookaheadConnect4Player', OT: 'GreedyOthelloPlayer', GB: 'GreedyGobangPlayer'}
N_POS = 256


def children(g):
    """[(action, child)] over valid_moves() in ascending action order: clone + play_action; win_state of g is not consulted"""
    out = []
    for a in np.flatnonzero(np.asarray(g.valid_moves())):
        c = g.clone()
        c.play_action(int(a))
        out.append((int(a), c))
    return out


def perft(root, depth):
    """(nodes int64 [depth], wins int64 [depth, P + 1]): at ply d + 1 the children of every unfinished position of ply d, and how many
    of them have each win_state entry set; a child with a non-zero win_state is not expanded"""
    frontier, nodes, wins = [root], [], []
    nv = len(np.asarray(root.win_state()))
    for _ in range(depth):
        nxt, w = [], np.zeros(nv, np.int64)
        n = 0
        for g in frontier:
            for _, c in children(g):
                ws = np.asarray(c.win_state()).astype(np.int64)
                n += 1
                w += ws
                if not ws.any():
                    nxt.append(c)
        nodes.append(n); wins.append(w)
        frontier = nxt
    return np.array(nodes, np.int64), np.stack(wins)


# ---------------------------------------------------------------------------------------------------------------- the three players
def connect4_sets(g):
    """players.py:38-49: (win, stop-loss, fallback) as ascending lists"""
    sets = ([], [], [])
    for a, c in children(g):
        ws = c.win_state()
        sets[0 if ws[g.player] else 1 if ws[c.player] else 2].append(a)
    return sets


def connect4_index(m, u):
    """the device's stand-in for np.random.choice(list) without p (numpy: randint(0, m)): min(m - 1, int(u * m)) in double"""
    return min(m - 1, int(np.float64(u) * np.float64(m)))


def connect4_move(g, u):
    """(move, chosen list) or (None, []) where the reference raises (players.py:51-67)"""
    for s in connect4_sets(g):
        if s:
            return s[connect4_index(len(s), u)], s
    return None, []


def othello_key(child):
    """-count_diff(child.player): count_diff(color) sums pieces * color (OthelloLogic.pyx:59-69) and is handed the player INDEX"""
    return -int(np.asarray(child._board.pieces, np.int64).sum() * int(child.player))


def gobang_key(child):
    return int(child.win_state()[child.player])


def greedy_move(g, key):
    """candidates.sort(); candidates[0][1] -- None where the reference raises IndexError"""
    cand = sorted((key(c), a) for a, c in children(g))
    return cand[0][1] if cand else None


def scripted_move(gid, g, u=0.0):
    """the scripted player's move on g (None: it raises)"""
    if gid == C4:
        return connect4_move(g, u)[0]
    return greedy_move(g, othello_key if gid == OT else gobang_key)


# ---------------------------------------------------------------------------------------------------------------- fixed inputs, shared
@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLDEN))


def positions(gid):
    """the 256 rule-table positions of choose_reference (what DeviceGames.pack takes)"""
    import choose_reference as R
    return R.inputs(gid)['items']


def built_states(gid):
    """the hand-built boards of the fixture for a game with a scripted player: [(cells, player, turns)]"""
    d, s = golden(), SHORT[gid]
    return [(np.asarray(c, np.int8), int(p), int(t)) for c, p, t in zip(d[s + '_built_cells'], d[s + '_built_player'], d[s + '_built_turns'])]


def host(gid, st):
    """the host env's GameState of a position as DeviceGames.pack takes it: a (cells, player, turns[, aux0]) tuple or a GameState"""
    import test_gpu_device_games as T
    if not isinstance(st, (tuple, list)):
        return st.clone()
    return T._host(gid, tuple(st) + (0,) * (4 - len(st)))
