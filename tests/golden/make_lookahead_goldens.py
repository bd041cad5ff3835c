"""tests/golden/lookahead.npz from the REFERENCE's own classes (build container only; never imported by a test):

  perft      for the six reference games, from the opening: <g>_perft_nodes [D] the children generated at ply 1..D (positions with a
             non-zero win_state are not expanded), <g>_perft_wins [D, P + 1] how many of them have each win_state entry set
  players    OneStepLookaheadConnect4Player / GreedyOthelloPlayer / GreedyGobangPlayer on the 256 rule-table positions of
             tests/choose_reference.py: <g>_move [256] what player.play(state) returned; for connect4 <g>_list [256, 7] the list
             np.random.choice was handed (recorded by wrapping it; -1 padded) and <g>_idx its index in that list
  built      hand-built boards where the players' quirks bite: <g>_built_cells / _player / _turns, <g>_built_move (-1: it raised),
             <g>_built_raised (the exception's class name, '' otherwise), and for connect4 <g>_built_list / <g>_built_idx

    python tests/golden/make_lookahead_goldens.py [out_dir]

The file is written with fixed zip timestamps, so a second run gives the same bytes."""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # the repository root: alphazero_general_amd
import refharness as rh  # noqa: E402  (puts tests/ on sys.path)
import lookahead_reference as LR  # noqa: E402

FRONTIER_CAP = 50000


def ref_classes():
    from alphazero.envs.brandubh.fastafl import Game as BRG
    from alphazero.envs.connect4.connect4 import Game as C4G
    from alphazero.envs.gobang.gobang import Game as GBG
    from alphazero.envs.hnefatafl.fastafl import Game as HNG
    from alphazero.envs.othello.othello import Game as OTG
    from alphazero.envs.tictactoe.tictactoe import Game as TTG
    return {LR.C4: C4G, LR.BR: BRG, LR.OT: OTG, LR.GB: GBG, LR.TT: TTG, LR.HN: HNG}


def ref_players():
    from alphazero.envs.connect4.players import OneStepLookaheadConnect4Player
    from alphazero.envs.gobang.GobangPlayers import GreedyGobangPlayer
    from alphazero.envs.othello.OthelloPlayers import GreedyOthelloPlayer
    return {LR.C4: OneStepLookaheadConnect4Player(), LR.OT: GreedyOthelloPlayer(), LR.GB: GreedyGobangPlayer()}


class ChoiceLog:
    """np.random.choice observed: the real function is called, what it was handed and what it returned are kept"""

    def __init__(self):
        self.calls = []

    def __enter__(self):
        self.real = np.random.choice
        np.random.choice = self.choice
        return self

    def __exit__(self, *exc):
        np.random.choice = self.real

    def choice(self, a, *args, **kw):
        assert not args and not kw, 'the player draws without p'
        r = self.real(a)
        self.calls.append(([int(x) for x in a], int(r)))
        return r


def play(player, g, seed):
    """(move or -1, exception class name or '', choice list, index in it)"""
    np.random.seed(seed)
    with ChoiceLog() as log:
        try:
            move, raised = int(player.play(g)), ''
        except Exception as e:                                       # recorded, not hidden: what the reference does on this board
            move, raised = -1, type(e).__name__
    assert len(log.calls) <= 1
    lst, got = log.calls[0] if log.calls else ([], -1)
    assert not lst or got == move
    return move, raised, lst, (lst.index(got) if lst else -1)


def built_boards():
    """{game: [(cells, player, turns)]}: see the module docstring; cells as Python callers hold them"""
    out = {}
    # connect4 (6 x 7, row 5 the bottom): colour -1 (player 1) already has four in the bottom row and player 0 is to move -- every move
    # leaves ws[child's mover] set: the stop-loss set is everything; then the same with a four of player 0's own to complete (the win
    # set takes precedence); both with the colours and the mover swapped; a full board for each mover
    b = np.zeros((6, 7), np.int8)
    b[5, 0:4] = -1
    b[4, 0:3] = 1
    b[5, 4] = 1
    c4 = [(b.copy(), 0, 8)]
    b2 = b.copy(); b2[5, 5] = 1; b2[5, 6] = -1; b2[4, 4] = 1; b2[4, 5] = -1; b2[3, 0] = 1; b2[3, 1] = -1   # player 0: 4,0..2 + 4,4 -- (4, 3) completes a row
    c4.append((b2.copy(), 0, 14))
    c4 += [(-c, 1 - p, t) for c, p, t in list(c4)]
    full = np.array([[1, 1, -1, -1, 1, 1, -1], [-1, -1, 1, 1, -1, -1, 1], [1, 1, -1, -1, 1, 1, -1], [1, 1, -1, -1, 1, 1, -1],
                     [-1, -1, 1, 1, -1, -1, 1], [1, 1, -1, -1, 1, 1, -1]], np.int8)
    c4 += [(full, 0, 42), (full, 1, 42)]
    out[LR.C4] = [(c.reshape(-1), p, t) for c, p, t in c4]
    # othello: the opening (player 0 to move: the child's mover is player 1 and the key is the stone difference) and the position after
    # its first move (player 1 to move: every key is 0), a board with one colour only and a full board for each mover (no valid move)
    op = np.zeros((8, 8), np.int8)
    op[3, 4] = op[4, 3] = 1; op[3, 3] = op[4, 4] = -1
    one = np.zeros((8, 8), np.int8); one[2:5, 2:5] = 1
    fullo = np.where(np.add.outer(np.arange(8), np.arange(8)) % 3 == 0, -1, 1).astype(np.int8)
    ot = [(op, 0, 0), (op, 1, 0), (one, 0, 9), (one, 1, 9), (fullo, 0, 60), (fullo, 1, 60)]
    mid = np.zeros((8, 8), np.int8)                                   # several flips of different sizes for either colour
    mid[3, 2:6] = -1; mid[3, 1] = 1; mid[4, 3] = 1; mid[2, 3] = -1; mid[5, 3] = -1; mid[4, 4] = -1; mid[2, 5] = 1
    ot += [(mid, 0, 8), (mid, 1, 8)]
    out[LR.OT] = [(c.reshape(-1), p, t) for c, p, t in ot]
    # gobang (cell 15x + y): the child's mover already holds a five -- every key is 1, except where the mover completes a five of its own
    # that the scan meets first; the same with the five only; colours and mover swapped; a full board for each mover
    g = np.zeros((15, 15), np.int8)
    g[10, 0:5] = -1
    g[2, 0:4] = 1
    g5 = np.zeros((15, 15), np.int8); g5[10, 0:5] = -1; g5[0, 0] = 1; g5[1, 1] = 1; g5[3, 7] = 1; g5[8, 8] = 1
    gb = [(g, 0, 9), (g5, 0, 9), (-g, 1, 9), (-g5, 1, 9)]
    fullg = np.where((np.add.outer(np.arange(15), 2 * np.arange(15)) // 2) % 2 == 0, 1, -1).astype(np.int8)
    gb += [(fullg, 0, 225), (fullg, 1, 225)]
    out[LR.GB] = [(c.reshape(-1), p, t) for c, p, t in gb]
    return out


def write_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            zi = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(zi, buf.getvalue())


def main(out_dir=HERE, verbose=True):
    rh.import_reference()
    from alphazero_general_amd.MCTS import decode_state
    classes, players = ref_classes(), ref_players()
    out = {}
    for gid, Game in classes.items():
        depth = LR.PERFT_DEPTH[gid]
        nodes, wins = LR.perft(Game(), depth)
        live = nodes - wins.sum(1)
        assert (live[:-1] <= FRONTIER_CAP).all(), (gid, nodes)
        out[LR.SHORT[gid] + '_perft_nodes'], out[LR.SHORT[gid] + '_perft_wins'] = nodes, wins
        if verbose:
            print(LR.SHORT[gid], 'perft', nodes.tolist(), wins.tolist(), flush=True)
    built = built_boards()
    for gid, player in players.items():
        s, Game = LR.SHORT[gid], classes[gid]
        for tag, states in (('', LR.positions(gid)), ('_built', built[gid])):
            rows = [play(player, decode_state(Game(), *st), 5000 + 1000 * gid + i) for i, st in enumerate(states)]
            out[s + tag + '_move'] = np.array([r[0] for r in rows], np.int32)
            if tag:
                out[s + '_built_cells'] = np.stack([np.asarray(st[0], np.int8) for st in states])
                out[s + '_built_player'] = np.array([st[1] for st in states], np.int8)
                out[s + '_built_turns'] = np.array([st[2] for st in states], np.int32)
                out[s + '_built_raised'] = np.array([r[1] for r in rows], 'U16')
            else:
                assert len(states) == LR.N_POS and not any(r[1] for r in rows)
            if gid == LR.C4:
                lst = np.full((len(rows), 7), -1, np.int8)
                for i, r in enumerate(rows):
                    lst[i, :len(r[2])] = r[2]
                out[s + tag + '_list'], out[s + tag + '_idx'] = lst, np.array([r[3] for r in rows], np.int8)
            if verbose:
                print(s + tag, 'moves', out[s + tag + '_move'][:24].tolist(), [r[1] for r in rows if r[1]], flush=True)
    path = os.path.join(out_dir, 'lookahead.npz')
    write_npz(path, out)
    if verbose:
        print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main(*sys.argv[1:2])
