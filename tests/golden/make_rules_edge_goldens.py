"""Rule fixtures of the two oldest games on BUILT and DENSE boards, recorded from the REFERENCE (make_goldens.py holds the random
playouts, br_rules.npz / c4_rules.npz; those stay as they are):

  br_rules_edge.npz   fastafl/cengine.pyx + envs/brandubh/fastafl.pyx on hand-built scenarios in all eight symmetries (custodian
                      capture, two-sided king capture, group surround, moves, win states), dense random boards and
                      capture-greedy playouts
  c4_rules_edge.npz   envs/connect4 on every winning line, long lines, wrapped non-lines, boards with a four of both colours,
                      full-board draws, the 42nd stone and every column at every height

Run in the build container only:   PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_rules_edge_goldens.py [br] [c4]

A record is a position (cells, player, turns, king flag) with the reference's valid_moves (packed bits), win_state and observation
crc, and optionally one action with `succ`, the index of the record that holds the successor position: every successor is a record
of its own (one per position, de-duplicated), so its move list and win state are checked as a root too.  The builder only decides
which boards are asked; every recorded value is the reference's answer.  A built scenario carries what it is meant to trigger (pieces
removed, king flag, win state, legal / illegal moves, cells) and the generator asserts that against the reference, so a scenario that
does not fire fails here instead of testing nothing.  Coverage counts are stored by name, per family, and their floors asserted."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import refharness as rh  # noqa: E402
from refharness import ol  # noqa: E402
import rules_edge as RE  # noqa: E402  (tests/rules_edge.py: the coverage floors, shared with the tests)

OUT = HERE
MAX_RECORDS, SIZE_LIMIT = RE.MAX_RECORDS, RE.SIZE_LIMIT


# ============================================================================================================= the record table
class Table:
    def __init__(self, ncells, make, state_of, families, cov_names):
        self.ncells, self.make, self.state_of = ncells, make, state_of
        self.families, self.cov_names = list(families), list(cov_names)
        self.rows, self.by_state, self.by_move = [], {}, {}
        self.cov = np.zeros((len(self.families), len(self.cov_names)), np.int64)

    def count(self, fam, name, n=1, mx=False):
        f, c = self.families.index(fam), self.cov_names.index(name)
        self.cov[f, c] = max(self.cov[f, c], n) if mx else self.cov[f, c] + n

    def _root(self, state, fam):
        g = self.make(state)
        v, w, o = np.asarray(g.valid_moves(), np.uint8), np.asarray(g.win_state(), np.uint8), g.observation()
        assert self.state_of(g) == state, 'the reference holds another state than it was given'
        return dict(state=state, valid=v, ws=w, obs_crc=rh.crc(o), action=-1, succ=-1, removed=0, fam=self.families.index(fam)), g

    def add(self, state, fam, action=None):
        """state = (cells bytes, player, turns, kc).  Returns (row index, successor state or None); new positions are classified
        into the coverage counts by self.on_position."""
        new = state not in self.by_state
        if action is None:
            if new:
                row, g = self._root(state, fam)
                self.by_state[state] = len(self.rows); self.rows.append(row)
                self.on_position(row, fam)
            return self.by_state[state], None
        if (state, action) in self.by_move:
            i = self.by_move[(state, action)]
            return i, self.rows[self.rows[i]['succ']]['state']
        first = self.by_state.get(state)
        if first is not None and self.rows[first]['action'] < 0:
            i, row = first, self.rows[first]                   # the position is there without an action: give it this one
            g = self.make(state)
        else:
            row, g = self._root(state, fam)
            i = len(self.rows); self.rows.append(row)
            if new:
                self.by_state[state] = i
                self.on_position(row, fam)
        assert not row['ws'].any() and row['valid'][action] == 1, ('the action must be legal at a live position', state, action)
        g.play_action(int(action))
        succ = self.state_of(g)
        row['action'] = int(action)
        self.by_move[(state, action)] = i
        row['succ'], _ = self.add(succ, fam)
        self.on_move(row, self.rows[row['succ']], fam)
        return i, succ

    def arrays(self):
        n = len(self.rows)
        assert n <= MAX_RECORDS, n
        cells = np.array([np.frombuffer(r['state'][0], np.int8) for r in self.rows])
        d = dict(cells=cells, player=np.array([r['state'][1] for r in self.rows], np.int8),
                 turns=np.array([r['state'][2] for r in self.rows], np.int16), kc=np.array([r['state'][3] for r in self.rows], np.int8),
                 ws=np.array([r['ws'] for r in self.rows], np.uint8), obs_crc=np.array([r['obs_crc'] for r in self.rows], np.uint32),
                 action=np.array([r['action'] for r in self.rows], np.int16), succ=np.array([r['succ'] for r in self.rows], np.int16),
                 removed=np.array([r['removed'] for r in self.rows], np.int8), family=np.array([r['fam'] for r in self.rows], np.uint8),
                 family_names=np.array(self.families), cov_names=np.array(self.cov_names), cov=self.cov)
        return d, np.array([r['valid'] for r in self.rows], np.uint8)


def save(name, d, out_dir, verbose, floors, table):
    path = os.path.join(out_dir or OUT, name + '.npz')
    np.savez_compressed(path, **d)
    size = os.path.getsize(path)
    tot = cov_total(d)
    if verbose:
        print('%s: %d records, %d with an action, %d bytes' % (name, len(d['action']), int((d['action'] >= 0).sum()), size))
        for f, fam in enumerate(table.families):
            print('  %-10s %s' % (fam, ' '.join('%s=%d' % (k, v) for k, v in zip(table.cov_names, d['cov'][f]) if v)))
        print('  total      %s' % ' '.join('%s=%d' % kv for kv in tot.items()))
    assert size <= SIZE_LIMIT, size
    for (fam, k), floor in floors.items():
        got = tot[k] if fam is None else int(d['cov'][table.families.index(fam), table.cov_names.index(k)])
        assert got >= floor, ('coverage floor missed', fam, k, got, floor)


cov_total = RE.cov_total


# ==================================================================================================================== brandubh
BR_FAMILIES = ['custodian', 'kingcap', 'surround', 'moves', 'win', 'dense', 'greedy']
BR_COV = ['scenarios', 'positions', 'moves', 'rm1', 'rm2', 'rm3p', 'kc_set', 'term_escape', 'term_capture', 'term_turn100',
          'term_nomove_def', 'term_nomove_att', 'over_with_moves', 'max_k', 'k_over_64']
# the eight symmetries of the square on (x, y)
SYMS = [lambda x, y: (x, y), lambda x, y: (6 - y, x), lambda x, y: (6 - x, 6 - y), lambda x, y: (y, 6 - x),
        lambda x, y: (6 - x, y), lambda x, y: (y, x), lambda x, y: (x, 6 - y), lambda x, y: (6 - y, 6 - x)]
CORNERS = {(0, 0), (6, 0), (0, 6), (6, 6)}

def br_cells(pieces):
    """{(x, y): 1 | 2 | 3} -> the 49 Board._state values (cengine.pyx:24-32: corners 5, throne 4, king + tile on both)"""
    c = np.zeros((7, 7), np.int8)
    for x, y in CORNERS:
        c[y, x] = 5
    c[3, 3] = 4
    for (x, y), v in pieces.items():
        assert 0 <= x < 7 and 0 <= y < 7 and v in (1, 2, 3)
        assert v == 3 or c[y, x] == 0, 'only the king stands on the throne or a corner'
        c[y, x] = v + c[y, x]
    return c.reshape(-1)


def br_action(sx, sy, nx, ny):                                 # fastafl.pyx:66-79
    mt = (ny if ny < sy else ny - 1) if sx == nx else (6 + nx - (1 if nx >= sx else 0))
    return 12 * (sx + sy * 7) + mt


def br_table():
    from make_goldens import br_game_cls
    G = br_game_cls()

    def make(state):
        cells, player, turns, kc = state
        g = G()
        g._board._state = np.frombuffer(cells, np.int8).astype(np.uint8).reshape(7, 7).copy()
        g._board.num_turns, g._turns, g._player, g._board._king_captured = int(turns), int(turns), int(player), bool(kc)
        return g

    def state_of(g):
        return (np.asarray(g._board._state, np.int8).tobytes(), int(g.player), int(g.turns), int(g._board._king_captured))

    t = Table(49, make, state_of, BR_FAMILIES, BR_COV)

    def on_position(row, fam):
        cells, player, turns, kc = row['state']
        c = np.frombuffer(cells, np.int8)
        k = int(row['valid'].sum())
        t.count(fam, 'positions'); t.count(fam, 'max_k', k, mx=True)
        if k > 64:
            t.count(fam, 'k_over_64')
        ws = row['ws']
        if ws.any():
            cause = ('term_turn100' if turns >= 100 else 'term_escape' if (c == 8).any() else 'term_nomove_def' if ws[1]
                     else 'term_capture' if kc else 'term_nomove_att')
            assert ws[2] == (turns >= 100) and (ws[1] if cause in ('term_escape', 'term_nomove_def') else True)
            t.count(fam, cause)
            if k > 0:
                t.count(fam, 'over_with_moves')
    t.on_position = on_position

    def on_move(row, srow, fam):
        a, b = np.frombuffer(row['state'][0], np.int8), np.frombuffer(srow['state'][0], np.int8)
        rm = int(np.isin(a, (1, 2)).sum() - np.isin(b, (1, 2)).sum())
        assert rm >= 0 and np.isin(a, (3, 7, 8)).sum() == np.isin(b, (3, 7, 8)).sum()        # the king is never lifted
        row['removed'] = rm
        t.count(fam, 'moves')
        if rm:
            t.count(fam, 'rm1' if rm == 1 else 'rm2' if rm == 2 else 'rm3p')
        if srow['state'][3] and not row['state'][3]:
            t.count(fam, 'kc_set')
    t.on_move = on_move
    return t


def br_state_of(pieces, turns, kc=0):
    return (br_cells(pieces).tobytes(), turns % 2, turns, kc)


def br_scenarios():
    """(kind, name, pieces, move or None, turns, expectation).  Canonical orientation; gen_br builds all eight symmetries, which
    gives every capture its four directions (DIRECTIONS order is visible in the surround step).  expectation keys: removed, kc,
    ws (after the move, or of the position when there is no move), ws0 (before the move, default live), k (legal moves of the
    position), legal / illegal: moves ((sx, sy), (nx, ny)) of the position, cells: {(x, y): value} after the move."""
    S = []

    def add(kind, name, pieces, move, turns=None, **exp):
        if turns is None:                                       # 2 (black) moves on even turns, 1 and the king on odd ones
            v = pieces[move[0]] if move else 2
            turns = 10 if v == 2 else 11
        S.append((kind, name, dict(pieces), move, turns, exp))
    K7 = {(3, 3): 3}                                            # the king at home

    # ---- custodian capture: mover m takes enemy e against far square f
    for m, e, f in ((1, 2, 1), (1, 2, 3), (2, 1, 2), (3, 2, 1)):
        far_king = f == 3
        king = {} if m == 3 or far_king else {(5, 5): 3}        # a king somewhere, away from the capture
        tag = 'm%de%df%d' % (m, e, f)
        add('custodian', 'friendly_' + tag, {(2, 2): m, (3, 1): e, (4, 1): f, **king}, ((2, 2), (2, 1)), removed=1, kc=0)
        if not far_king:
            add('custodian', 'empty_throne_' + tag, {(1, 1): m, (3, 2): e, **king}, ((1, 1), (3, 1)), removed=1, kc=0, cells={(3, 3): 4})
            add('custodian', 'corner_' + tag, {(2, 2): m, (1, 0): e, **king}, ((2, 2), (2, 0)), removed=1, kc=0, cells={(0, 0): 5})
            add('custodian', 'off_board_' + tag, {(1, 1): m, (3, 0): e, **king}, ((1, 1), (3, 1)), removed=0, kc=0)
            add('custodian', 'between_' + tag, {(3, 2): m, (2, 1): e, (4, 1): e, **king}, ((3, 2), (3, 1)), removed=0, kc=0)
            add('custodian', 'double_' + tag, {(2, 4): m, (1, 2): e, (0, 2): f, (2, 1): e, (2, 0): f, **king}, ((2, 4), (2, 2)), removed=2, kc=0)
            add('custodian', 'triple_' + tag, {(2, 4): m, (1, 2): e, (0, 2): f, (2, 1): e, (2, 0): f, (3, 2): e, (4, 2): f, **king},
                ((2, 4), (2, 2)), removed=3, kc=0)
    # against the OCCUPIED throne (7): the king is an attacker, so white captures against it and black does not
    add('custodian', 'king_at_home_m1', {(1, 1): 1, (3, 2): 2, **K7}, ((1, 1), (3, 1)), removed=1, kc=0, cells={(3, 3): 7})
    add('custodian', 'king_at_home_m2', {(1, 1): 2, (3, 2): 1, **K7}, ((1, 1), (3, 1)), removed=0, kc=0, cells={(3, 3): 7})
    # (7 per (m, e, f) with a non-king far piece x 3 + 1 + 2 = 24 ... counted in BR_FLOORS)

    # ---- two-sided king capture (fires for any mover)
    add('kingcap', 'by_black', {(2, 2): 2, (3, 1): 3, (4, 1): 2, (5, 5): 1}, ((2, 2), (2, 1)), removed=0, kc=1, ws=(1, 0, 0))
    add('kingcap', 'by_white', {(2, 2): 1, (3, 1): 3, (4, 1): 1, (5, 5): 2}, ((2, 2), (2, 1)), removed=0, kc=1, ws=(1, 0, 0))
    add('kingcap', 'black_vs_throne', {(1, 1): 2, (3, 2): 3}, ((1, 1), (3, 1)), removed=0, kc=1, ws=(1, 0, 0))
    add('kingcap', 'white_vs_throne', {(1, 1): 1, (3, 2): 3, (5, 5): 2}, ((1, 1), (3, 1)), removed=0, kc=1, ws=(1, 0, 0))
    add('kingcap', 'black_vs_corner', {(2, 2): 2, (1, 0): 3}, ((2, 2), (2, 0)), removed=0, kc=1, ws=(1, 0, 0))
    add('kingcap', 'white_vs_corner', {(2, 2): 1, (1, 0): 3, (5, 5): 2}, ((2, 2), (2, 0)), removed=0, kc=1, ws=(1, 0, 0))
    add('kingcap', 'black_one_side_only', {(2, 2): 2, (3, 1): 3, (5, 5): 1}, ((2, 2), (2, 1)), removed=0, kc=0, ws=(0, 0, 0))
    # the king at home (7) is not the value custodian capture looks for: two blacks on opposite sides do nothing
    add('kingcap', 'king_at_home_untouched', {(2, 1): 2, (4, 3): 2, **K7}, ((2, 1), (2, 3)), removed=0, kc=0, ws=(0, 0, 0))
    add('kingcap', 'king_off_board_side', {(1, 1): 2, (3, 0): 3}, ((1, 1), (3, 1)), removed=0, kc=0, ws=(0, 0, 0))

    # ---- group surround.  Blocked groups, then the same with exactly one liberty.  `sw` swaps the colours (white surrounds black)
    def surround(name, group, blockers, move, liberty, king=None, kc=0, extra=None):
        for sw in (False, True):
            a, b = (2, 1) if not sw else (1, 2)                 # a surrounds b
            base = {p: b for p in group}
            base.update({p: a for p in blockers})
            base[move[0]] = a
            base.update(extra or {})
            kp = dict(base)
            if king is not None:                                # the king is a member of the (white) group: only black surrounds it
                if sw:
                    continue
                kp[king] = 3
            else:
                kp[(5, 5) if (5, 5) not in kp else (5, 3)] = 3
            n = len(group) - (1 if king in group else 0)
            add('surround', '%s_%s' % (name, 'wb'[sw]), kp, move, removed=n, kc=kc)
            if liberty is not None:
                lp = dict(kp); del lp[liberty]
                add('surround', '%s_liberty_%s' % (name, 'wb'[sw]), lp, move, removed=0, kc=0)
    surround('g1_edge', [(3, 0)], [(2, 0), (4, 0)], ((3, 2), (3, 1)), (4, 0))
    surround('g1_corner', [(1, 0)], [(2, 0)], ((1, 3), (1, 1)), (2, 0))
    surround('g2_throne', [(3, 2), (3, 1)], [(2, 2), (4, 2), (2, 1), (4, 1)], ((1, 0), (3, 0)), (4, 2), extra=None)
    surround('g3_edge', [(2, 0), (3, 0), (4, 0)], [(1, 0), (5, 0), (2, 1), (4, 1)], ((3, 2), (3, 1)), (5, 0))
    surround('g4_block_corner', [(1, 0), (2, 0), (1, 1), (2, 1)], [(3, 0), (0, 1), (3, 1), (1, 2)], ((2, 4), (2, 2)), (0, 1))
    # a group that holds the king: the flag is set, the king stays, the others are lifted
    surround('king_in_group_mid', [(2, 0), (3, 0), (4, 0)], [(1, 0), (5, 0), (2, 1), (4, 1)], ((3, 2), (3, 1)), (5, 0), king=(3, 0), kc=1)
    surround('king_in_group_far', [(2, 0), (3, 0), (4, 0)], [(1, 0), (5, 0), (3, 1), (4, 1)], ((2, 2), (2, 1)), (5, 0), king=(4, 0), kc=1)
    # the king at home inside a blocked group (value 7)
    add('surround', 'king_at_home_in_group', {(3, 2): 1, (2, 2): 2, (4, 2): 2, (2, 3): 2, (4, 3): 2, (3, 4): 2, (1, 1): 2, **K7},
        ((1, 1), (3, 1)), removed=1, kc=1, cells={(3, 3): 7})
    # two groups next to the moved piece: the one on the edge is taken, the one with a liberty is not
    add('surround', 'two_groups_one_taken', {(3, 2): 2, (3, 0): 1, (2, 0): 2, (4, 0): 2, (2, 1): 1, (5, 5): 3}, ((3, 2), (3, 1)), removed=1, kc=0,
        cells={(2, 1): 1, (3, 0): 0})
    add('surround', 'two_groups_both_taken', {(3, 2): 2, (3, 0): 1, (2, 0): 2, (4, 0): 2, (2, 1): 1, (1, 1): 2, (2, 2): 2, (5, 5): 3},
        ((3, 2), (3, 1)), removed=2, kc=0)
    # the custodian step comes first: it lifts (4, 1), which opens a liberty for the rest of a group that was blocked before the move
    add('surround', 'custodian_opens_group', {(3, 2): 2, (4, 1): 1, (5, 1): 2, (4, 2): 2, (4, 0): 1, (3, 0): 2, (5, 0): 2, (5, 5): 3},
        ((3, 2), (3, 1)), removed=1, kc=0, cells={(4, 0): 1, (4, 1): 0})

    # ---- moves
    add('moves', 'king_leaves_home', {(0, 3): 2, (5, 5): 1, **K7}, ((3, 3), (3, 2)), cells={(3, 3): 4, (3, 2): 3},
        legal=[((3, 3), (3, 0)), ((5, 5), (3, 5))])
    for v in (1, 2, 3):
        other = {(5, 5): 3, (5, 1): 2} if v == 1 else {(5, 5): 3, (5, 1): 1} if v == 2 else {(5, 1): 2, (5, 5): 1}
        add('moves', 'over_empty_throne_v%d' % v, {(3, 1): v, **other}, ((3, 1), (3, 5)), removed=0,
            legal=[((3, 1), (3, 2)), ((3, 1), (3, 4)), ((3, 1), (3, 6))], illegal=[((3, 1), (3, 3))])
    for v in (1, 2):
        add('moves', 'home_king_blocks_v%d' % v, {(3, 1): v, (5, 1): 3 - v, **K7}, ((3, 1), (3, 2)), legal=[((3, 1), (3, 0))],
            illegal=[((3, 1), (3, 3)), ((3, 1), (3, 4)), ((3, 1), (3, 5))])
    add('moves', 'king_reaches_corner', {(0, 3): 3, (5, 1): 2, (5, 5): 1}, ((0, 3), (0, 0)), cells={(0, 0): 8, (0, 3): 0}, ws=(0, 1, 0),
        legal=[((0, 3), (0, 6))])
    for v in (1, 2):
        add('moves', 'corner_closed_v%d' % v, {(0, 3): v, (5, 1): 3 - v, (5, 5): 3}, ((0, 3), (0, 1)), legal=[((0, 3), (0, 5))],
            illegal=[((0, 3), (0, 0)), ((0, 3), (0, 6))])
    for v in (1, 2, 3):
        other = {(5, 5): 3, (4, 4): 2} if v == 1 else {(5, 5): 3, (4, 4): 1} if v == 2 else {(4, 4): 2, (5, 5): 1}
        add('moves', 'twelve_destinations_v%d' % v, {(1, 1): v, **other}, ((1, 1), (1, 6)), k12=(1, 1))
    return S


def br_wide_boards(n, seed=77, rounds=40, steps=700):
    """positions with as many legal moves as the builder can reach: hill climbing on the oracle's count (the search only proposes
    boards; the recorded move lists are the reference's).  Eight blacks to move, the king and nothing else."""
    rng = np.random.RandomState(seed)
    free = [(x, y) for y in range(7) for x in range(7) if (x, y) not in CORNERS and (x, y) != (3, 3)]

    def k_of(pl):
        st = ol.State()
        for i, v in enumerate(br_cells(pl)):
            st.cells[i] = int(v)
        st.turns = 10
        return int(ol.OGame(ol.GAME_BRANDUBH, st).valid_moves().sum())
    best = {}
    for _ in range(rounds):
        idx = rng.choice(len(free), 9, replace=False)
        sq = [free[i] for i in idx]
        cur = k_of({**{p: 2 for p in sq[:8]}, sq[8]: 3})
        for _ in range(steps):
            j, p = rng.randint(9), free[rng.randint(len(free))]
            if p in sq:
                continue
            cand = list(sq); cand[j] = p
            k = k_of({**{q: 2 for q in cand[:8]}, cand[8]: 3})
            if k >= cur:
                sq, cur = cand, k
        best[tuple(sorted(sq[:8])) + (sq[8],)] = cur
    top = sorted(best.items(), key=lambda kv: (-kv[1], kv[0]))[:n]
    return [({**{p: 2 for p in key[:8]}, key[8]: 3}, k) for key, k in top]


def br_win_scenarios():
    S = []

    def add(name, pieces, move, turns, **exp):
        S.append(('win', name, dict(pieces), move, turns, exp))
    # black (2) cannot move: attackers (1) win, on black's turn and on white's
    nm_def = {(1, 0): 2, (2, 0): 1, (1, 1): 1, (5, 5): 3}
    add('no_move_def_own_turn', nm_def, None, 10, ws=(0, 1, 0), k=0)
    add('no_move_def_other_turn', nm_def, None, 11, ws=(0, 1, 0))
    nm_def2 = {(3, 0): 2, (2, 0): 1, (4, 0): 1, (3, 1): 1, (0, 2): 2, (0, 1): 1, (0, 3): 1, (1, 2): 3}
    add('no_move_def2_own_turn', nm_def2, None, 10, ws=(0, 1, 0), k=0)
    add('no_move_def2_other_turn', nm_def2, None, 11, ws=(0, 1, 0))
    # white (1 and the king) cannot move: defenders (2) win
    nm_att = {(1, 0): 1, (2, 0): 2, (1, 1): 2, (3, 0): 3, (4, 0): 2, (3, 1): 2}
    add('no_move_att_own_turn', nm_att, None, 11, ws=(1, 0, 0), k=0)
    add('no_move_att_other_turn', nm_att, None, 10, ws=(1, 0, 0))
    nm_att2 = {(2, 2): 2, (4, 2): 2, (3, 2): 2, (2, 3): 2, (4, 3): 2, (3, 4): 2, (3, 3): 3}              # the king shut in at home
    add('no_move_king_home_own_turn', nm_att2, None, 11, ws=(1, 0, 0), k=0)
    add('no_move_king_home_other_turn', nm_att2, None, 10, ws=(1, 0, 0))
    # the only moves run over the empty throne: legal_moves lists them, _has_legals_check sees no free neighbour -> the game is over
    over_def = {(3, 2): 2, (2, 2): 1, (4, 2): 1, (3, 1): 1, (5, 5): 3}
    add('only_over_throne_def_own_turn', over_def, None, 10, ws=(0, 1, 0), k=3)
    add('only_over_throne_def_other_turn', over_def, None, 11, ws=(0, 1, 0))
    over_att = {(3, 2): 3, (2, 2): 2, (4, 2): 2, (3, 1): 2}
    add('only_over_throne_king_own_turn', over_att, None, 11, ws=(1, 0, 0), k=3)
    add('only_over_throne_king_other_turn', over_att, None, 10, ws=(1, 0, 0))
    # a king whose only open neighbour is a corner keeps white alive, and the one move wins
    add('king_only_corner_open', {(1, 0): 3, (2, 0): 2, (1, 1): 2}, ((1, 0), (0, 0)), 11, ws0=(0, 0, 0), k=1, ws=(0, 1, 0), cells={(0, 0): 8})
    add('king_only_corner_open_black_to_move', {(1, 0): 3, (2, 0): 2, (1, 1): 2}, None, 10, ws=(0, 0, 0))
    # escape and capture true together: the escape is tested first
    add('escaped_and_captured', {(0, 0): 3, (3, 1): 2, (4, 4): 1}, None, 10, kc0=1, ws=(0, 1, 0))
    add('captured_only', {(1, 2): 3, (3, 1): 2, (4, 4): 1}, None, 10, kc0=1, ws=(1, 0, 0))
    # the move that makes turns 100: the draw is tested first (fastafl.pyx:196)
    add('escape_on_turn_100', {(0, 3): 3, (5, 1): 2, (5, 5): 1}, ((0, 3), (0, 0)), 99, ws=(0, 0, 1), cells={(0, 0): 8})
    add('capture_on_turn_100', {(2, 2): 1, (3, 1): 3, (4, 1): 1, (5, 5): 2}, ((2, 2), (2, 1)), 99, kc=1, ws=(0, 0, 1))
    add('escape_on_turn_98', {(0, 3): 3, (5, 1): 2, (5, 5): 1}, ((0, 3), (0, 0)), 97, ws=(0, 1, 0))
    add('capture_on_turn_99', {(2, 2): 2, (3, 1): 3, (4, 1): 2, (5, 5): 1}, ((2, 2), (2, 1)), 98, kc=1, ws=(1, 0, 0))
    add('plain_move_to_turn_100', {(2, 2): 1, (5, 5): 2, (1, 5): 3}, ((2, 2), (2, 1)), 99, kc=0, ws=(0, 0, 1))
    return S


def br_build(t, scenario):
    kind, name, pieces, move, turns, exp = scenario
    made = set()
    for sym in SYMS:
        pl = {sym(x, y): v for (x, y), v in pieces.items()}
        state = br_state_of(pl, turns, exp.get('kc0', 0))
        mv = None if move is None else (sym(*move[0]), sym(*move[1]))
        key = (state, mv)
        if key in made:
            continue
        made.add(key)
        i, succ = t.add(state, kind, None if mv is None else br_action(*mv[0], *mv[1]))
        row = t.rows[i]
        what = (kind, name, pl, mv)
        if 'k' in exp:
            assert int(row['valid'].sum()) == exp['k'], what
        for s, d in exp.get('legal', []):
            assert row['valid'][br_action(*sym(*s), *sym(*d))] == 1, what
        for s, d in exp.get('illegal', []):
            assert row['valid'][br_action(*sym(*s), *sym(*d))] == 0, what
        if 'k12' in exp:
            x, y = sym(*exp['k12'])
            assert int(row['valid'][12 * (x + 7 * y):12 * (x + 7 * y) + 12].sum()) == 12, what
        if mv is None:
            if 'ws' in exp:
                assert tuple(row['ws']) == exp['ws'], (what, row['ws'])
            continue
        assert tuple(row['ws']) == exp.get('ws0', (0, 0, 0)), what
        srow = t.rows[row['succ']]
        after = np.frombuffer(succ[0], np.int8).reshape(7, 7)
        if 'removed' in exp:
            assert row['removed'] == exp['removed'], (what, row['removed'])
        if 'kc' in exp:
            assert succ[3] == exp['kc'], (what, succ[3])
        if 'ws' in exp:
            assert tuple(srow['ws']) == exp['ws'], (what, srow['ws'])
        for (x, y), v in exp.get('cells', {}).items():
            sx, sy = sym(x, y)
            assert after[sy, sx] == v, (what, (x, y), after)
    t.count(kind, 'scenarios')


def br_dense(t, n_boards=8000, seed=2024, filler=300, keep_terminal=220, keep_rm1=0.08):
    """Dense random boards: corners and throne fixed, the king at home or on a free square, 0-4 attackers and 0-8 defenders (40 % of the
    boards with all twelve), turns uniform in 0..98, up to six random legal moves per board.  All boards are asked and what the run
    met is stored as `dense_met`; the fixture keeps the first `keep_terminal` terminal boards, every move that removes two or more
    pieces or sets the king flag, every board with more than 64 moves, a share of the single removals and `filler` of the plain moves
    (the record budget does not hold all 45 000 moves)."""
    rng = np.random.RandomState(seed)
    free = [(x, y) for y in range(7) for x in range(7) if (x, y) not in CORNERS and (x, y) != (3, 3)]
    met = dict(terminal=0, nomove=0, rm2=0, rm3p=0, kc=0, max_k=0, moves=0)
    plain = []
    for b in range(n_boards):
        full = rng.rand() < 0.4
        na, nd = (4, 8) if full else (rng.randint(0, 5), rng.randint(0, 9))
        home = rng.rand() < 0.5
        idx = rng.permutation(len(free))[:na + nd + 1]
        sq = [free[i] for i in idx]
        pl = {(3, 3) if home else sq[0]: 3}
        pl.update({p: 1 for p in sq[1:1 + na]}); pl.update({p: 2 for p in sq[1 + na:1 + na + nd]})
        turns = int(rng.randint(0, 99))
        state = br_state_of(pl, turns)
        g = t.make(state)
        v, w = np.asarray(g.valid_moves()), np.asarray(g.win_state())
        k = int(v.sum())
        met['max_k'] = max(met['max_k'], k)
        if w.any():
            met['terminal'] += 1
            if not (np.frombuffer(state[0], np.int8) == 8).any():
                met['nomove'] += 1
            if met['terminal'] <= keep_terminal:
                t.add(state, 'dense')
            continue
        if k > 64:
            t.add(state, 'dense')
        legal = np.flatnonzero(v)
        for a in rng.permutation(legal)[:6]:
            h = t.make(state); h.play_action(int(a))
            s2 = t.state_of(h)
            c0, c1 = np.frombuffer(state[0], np.int8), np.frombuffer(s2[0], np.int8)
            rm = int(np.isin(c0, (1, 2)).sum() - np.isin(c1, (1, 2)).sum())
            met['moves'] += 1
            met['rm2'] += rm == 2; met['rm3p'] += rm >= 3; met['kc'] += s2[3]
            if rm >= 2 or s2[3] or (rm == 1 and rng.rand() < keep_rm1):
                t.add(state, 'dense', int(a))
            else:
                plain.append((state, int(a)))
    for j in rng.permutation(len(plain))[:filler]:
        t.add(plain[j][0], 'dense', plain[j][1])
    return met


def br_greedy(t, n_games=8, seed=99):
    """Capture-greedy playouts from the start position: a move that removes a piece is preferred when there is one (multi-removals
    first), so removals come up in reachable positions."""
    rng = np.random.RandomState(seed)
    from make_goldens import br_game_cls
    G = br_game_cls()
    for _ in range(n_games):
        g = G()
        state = t.state_of(g)
        while True:
            g = t.make(state)
            v, w = np.asarray(g.valid_moves()), np.asarray(g.win_state())
            if w.any():
                t.add(state, 'greedy')
                break
            legal = rng.permutation(np.flatnonzero(v))
            n0 = int(np.isin(np.frombuffer(state[0], np.int8), (1, 2)).sum())
            best, best_rm = int(legal[0]), 0
            for a in legal:
                h = t.make(state); h.play_action(int(a))
                rm = n0 - int(np.isin(np.asarray(h._board._state), (1, 2)).sum())
                if rm > best_rm:
                    best, best_rm = int(a), rm
            if best_rm == 0 or rng.rand() < 0.1:
                best = int(legal[0])
            _, state = t.add(state, 'greedy', best)


def gen_br(out_dir=None, verbose=True):
    t = br_table()
    scen = br_scenarios() + br_win_scenarios()
    for s in scen:
        br_build(t, s)
    for pl, k in br_wide_boards(6):                             # more than 64 legal moves (MAXK is 96): the widest the search reaches
        state = br_state_of(pl, 10)
        i, _ = t.add(state, 'moves')
        assert int(t.rows[i]['valid'].sum()) == k > 64, (k, pl)
        a = int(np.flatnonzero(t.rows[i]['valid'])[-1])         # the last move of the list lies in its second 64-lane chunk
        t.add(state, 'moves', a)
        t.count('moves', 'scenarios')
    n_built = len(t.rows)
    met = br_dense(t)
    br_greedy(t)
    d, valid = t.arrays()
    d['valid_bits'] = np.packbits(valid, axis=1)
    d['dense_met'] = np.array([met[k] for k in ('terminal', 'nomove', 'rm2', 'rm3p', 'kc', 'max_k', 'moves')], np.int64)
    d['dense_met_names'] = np.array(['terminal', 'nomove', 'rm2', 'rm3p', 'kc', 'max_k', 'moves'])
    if verbose:
        print('br_rules_edge: %d scenarios -> %d built records; dense run met %s' % (len(scen), n_built, met))
    di = t.families.index('dense')
    nomove = int(d['cov'][di, t.cov_names.index('term_nomove_def')] + d['cov'][di, t.cov_names.index('term_nomove_att')])
    assert nomove >= RE.BR_DENSE_NOMOVE, nomove
    save('br_rules_edge', d, out_dir, verbose, RE.BR_FLOORS, t)


# ==================================================================================================================== connect4
C4_FAMILIES = ['lines', 'floating', 'long', 'wrapped', 'both', 'draws', 'last', 'columns']
C4_COV = ['positions', 'moves', 'win_p0', 'win_p1', 'draws', 'win_on_42nd', 'draw_on_42nd', 'lines_row', 'lines_col', 'lines_diag',
          'lines_anti', 'isolated', 'both_colours', 'wrapped_flat', 'wrapped_stride', 'wrapped_mod7', 'col_heights', 'full_columns']
DIRS4 = (('row', 0, 1), ('col', 1, 0), ('diag', 1, 1), ('anti', 1, -1))


def c4_lines(length=4):
    out = []
    for name, dr, dc in DIRS4:
        for r in range(6):
            for c in range(7):
                cells = [(r + i * dr, c + i * dc) for i in range(length)]
                if all(0 <= rr < 6 and 0 <= cc < 7 for rr, cc in cells):
                    out.append((name, cells))
    return out


LINES4 = c4_lines()
assert len(LINES4) == 69


def c4_fours(b, colour):
    return [i for i, (_, cells) in enumerate(LINES4) if all(b[r, c] == colour for r, c in cells)]


def c4_pattern(k):
    """full boards without a four: vertical runs of two, alternating columns; k picks the phase, the colours and the mirror"""
    r, c = np.mgrid[0:6, 0:7]
    p = np.where((((r + (k & 1)) // 2) + c) % 2 == 0, 1, -1).astype(np.int8)
    if k & 2:
        p = -p
    if k & 4:
        p = p[:, ::-1].copy()
    return p


def c4_supported(cells, pat):
    """the cells of a line in one colour resting on filler from the pattern: every cell below a line cell is filled"""
    b = np.zeros((6, 7), np.int8)
    for r, c in cells:
        b[r + 1:, c] = pat[r + 1:, c]
    return b


def c4_table():
    from alphazero.envs.connect4.connect4 import Game

    def make(state):
        cells, player, turns, _ = state
        g = Game()
        g._board.pieces = np.frombuffer(cells, np.int8).astype(np.intc).reshape(6, 7).copy()
        g._player, g._turns = int(player), int(turns)
        return g

    def state_of(g):
        return (np.asarray(g._board.pieces, np.int8).tobytes(), int(g.player), int(g.turns), 0)
    t = Table(42, make, state_of, C4_FAMILIES, C4_COV)

    def on_position(row, fam):
        t.count(fam, 'positions')
        ws = row['ws']
        b = np.frombuffer(row['state'][0], np.int8).reshape(6, 7)
        if ws[0]:
            t.count(fam, 'win_p0')
        if ws[1]:
            t.count(fam, 'win_p1')
        if ws[2]:
            t.count(fam, 'draws')
        if c4_fours(b, 1) and c4_fours(b, -1):
            assert ws[0] and not ws[1]                          # the reference scans colour 1 first
            t.count(fam, 'both_colours')
    t.on_position = on_position

    def on_move(row, srow, fam):
        t.count(fam, 'moves')
        if row['state'][2] == 41:
            t.count(fam, 'draw_on_42nd' if srow['ws'][2] else 'win_on_42nd')
            assert srow['ws'].any()
    t.on_move = on_move
    return t


def c4_state(b, player=None):
    n = int(np.count_nonzero(b))
    return (np.asarray(b, np.int8).tobytes(), n % 2 if player is None else player, n, 0)


def c4_gravity(b):
    return all(not (b[r, c] != 0 and b[r + 1, c] == 0) for r in range(5) for c in range(7))


def c4_fix_parity(b, mover, avoid_col):
    """the board with one more filler stone when its stone count does not give `mover` the turn; no four may appear"""
    if int(np.count_nonzero(b)) % 2 == mover:
        return b
    for c in range(7):
        if c == avoid_col or b[0, c] != 0:
            continue
        r = int(np.flatnonzero(b[:, c] == 0).max())
        for colour in (1, -1):
            nb = b.copy(); nb[r, c] = colour
            if not c4_fours(nb, 1) and not c4_fours(nb, -1):
                return nb
    return None


def c4_line_boards(t, fam, lines, count_dir):
    """every line in both colours on a gravity board (filler below it from a no-four pattern), as a terminal record and as the
    move that completes it: the last stone is the line's highest cell (top of its column)"""
    for li, (name, cells) in enumerate(lines):
        for colour in (1, -1):
            done, alone = False, None
            for k in range(8):
                b = c4_supported(cells, c4_pattern(k))
                for r, c in cells:
                    b[r, c] = colour
                if c4_fours(b, -colour) or not c4_gravity(b):
                    continue
                alone = b if alone is None else alone
                mover = 0 if colour == 1 else 1
                mid = (len(cells) - 1) / 2.0                     # the last stone: the cell nearest the middle that lies on top of its
                for last in sorted(cells, key=lambda rc: (abs(cells.index(rc) - mid), rc)):   # column and leaves no four behind
                    pre = b.copy(); pre[last] = 0
                    if pre[:last[0], last[1]].any() or c4_fours(pre, colour):
                        continue
                    pre = c4_fix_parity(pre, mover, last[1])
                    if pre is None:
                        continue
                    i, succ = t.add(c4_state(pre), fam, last[1])
                    after = np.frombuffer(succ[0], np.int8).reshape(6, 7)
                    assert all(after[rc] == colour for rc in cells) and (after != pre).sum() == 1
                    i, done = t.rows[i]['succ'], True
                    break
                if done:
                    break
            if not done:                                        # a column of five or six: no stone can come last.  The end board alone
                assert len(cells) > 4 and alone is not None, ('no gravity board for the line', name, cells, colour)
                i, _ = t.add(c4_state(alone), fam)
            assert tuple(t.rows[i]['ws']) == ((1, 0, 0) if colour == 1 else (0, 1, 0)), (name, cells, colour)
            if count_dir:
                t.count(fam, 'lines_' + name)


def gen_c4(out_dir=None, verbose=True):
    t = c4_table()
    # all 69 lines, each colour, resting on filler; and floating alone on an empty board (no gravity: recorded without an action)
    c4_line_boards(t, 'lines', LINES4, True)
    for name, cells in LINES4:
        for colour in (1, -1):
            b = np.zeros((6, 7), np.int8)
            for r, c in cells:
                b[r, c] = colour
            i, _ = t.add(c4_state(b), 'floating')
            assert tuple(t.rows[i]['ws']) == ((1, 0, 0) if colour == 1 else (0, 1, 0))
            t.count('floating', 'isolated')
    # lines of 5, 6 and 7
    for n in (5, 6, 7):
        c4_line_boards(t, 'long', c4_lines(n), False)
    # wrapped runs that must not count: four cells consecutive in flat order (index 7r + c, steps 1 / 8 / 6), in the bit order of
    # the device's boards (index 8r + c, steps 1 / 9 / 7, column 7 being padding) or with the column taken modulo 7, that are no line
    def wrapped(idx_of, steps, cname):
        seen = set()
        for step in steps:
            for r in range(6):
                for c in range(7):
                    cells = []
                    for i in range(4):
                        cell = idx_of(r, c, i, step)
                        if cell is None:
                            break
                        cells.append(cell)
                    if len(cells) < 4 or len(set(cells)) < 4 or any(sorted(cells) == sorted(l) for _, l in LINES4):
                        continue
                    if tuple(sorted(cells)) in seen:
                        continue
                    seen.add(tuple(sorted(cells)))
                    for colour in (1, -1):
                        for k in range(8):
                            b = c4_supported(cells, c4_pattern(k))
                            for rr, cc in cells:
                                b[rr, cc] = colour
                            if not c4_fours(b, 1) and not c4_fours(b, -1) and c4_gravity(b):
                                i, _ = t.add(c4_state(b), 'wrapped')
                                assert not t.rows[i]['ws'].any(), cells
                                t.count('wrapped', cname)
                                break

    def flat(r, c, i, step):
        j = 7 * r + c + i * step
        return (j // 7, j % 7) if j < 42 else None

    def stride(r, c, i, step):
        j = 8 * r + c + i * step
        return (j // 8, j % 8) if j < 48 and j % 8 != 7 else None

    def mod7(r, c, i, step):
        dr, dc = {1: (0, 1), 8: (1, 1), 6: (1, -1)}[step]
        return (r + i * dr, (c + i * dc) % 7) if r + i * dr < 6 else None
    wrapped(flat, (1, 8, 6), 'wrapped_flat')
    wrapped(stride, (1, 9, 7), 'wrapped_stride')
    wrapped(mod7, (1, 8, 6), 'wrapped_mod7')
    # both colours hold a four: the reference scans colour 1 first, wherever the fours lie
    both = []
    for a, b_ in ((0, 1), (1, 0), (6, 5), (2, 4), (3, 0)):
        b = np.zeros((6, 7), np.int8); b[2:, a] = 1; b[2:, b_] = -1
        both.append(b)
    for c0 in (0, 3):
        b = np.zeros((6, 7), np.int8); b[5, c0:c0 + 4] = -1; b[4, c0:c0 + 4] = 1
        both.append(b)
        b = np.zeros((6, 7), np.int8); b[5, c0:c0 + 4] = 1; b[4, c0:c0 + 4] = -1
        both.append(b)
    for b in both:
        assert c4_fours(b, 1) and c4_fours(b, -1) and c4_gravity(b)
        i, _ = t.add(c4_state(b), 'both')
        assert tuple(t.rows[i]['ws']) == (1, 0, 0)
    # full boards without a four
    for k in range(8):
        i, _ = t.add(c4_state(c4_pattern(k)), 'draws')
        assert tuple(t.rows[i]['ws']) == (0, 0, 1)
    # the 42nd stone (player 1, colour -1): a draw, or a win that comes before the draw
    rng = np.random.RandomState(4242)
    for k in range(8):
        p = c4_pattern(k)
        for c in np.flatnonzero(p[0] == -1)[:2]:
            pre = p.copy(); pre[0, c] = 0
            i, _ = t.add(c4_state(pre), 'last', int(c))
            assert tuple(t.rows[t.rows[i]['succ']]['ws']) == (0, 0, 1)
    wins = 0
    for _ in range(200000):
        if wins >= 12:
            break
        p = c4_pattern(int(rng.randint(8))).copy()
        for _f in range(int(rng.randint(1, 4))):
            p[rng.randint(6), rng.randint(7)] *= -1
        c = int(rng.randint(7))
        full = p.copy(); full[0, c] = -1
        pre = full.copy(); pre[0, c] = 0
        if c4_fours(pre, 1) or c4_fours(pre, -1) or not c4_fours(full, -1):
            continue
        if (c4_state(pre), c) in t.by_move:
            continue
        i, _ = t.add(c4_state(pre), 'last', c)
        assert tuple(t.rows[t.rows[i]['succ']]['ws']) == (0, 1, 0)
        wins += 1
    # every column at every height: play lands on the lowest free cell, a full column leaves the valid mask
    for c in range(7):
        for h in range(7):
            p = c4_pattern((c + h) % 8)
            b = np.zeros((6, 7), np.int8)
            for cc in range(7):
                hh = h if cc == c else (cc * 2 + h + c) % 7
                if hh:
                    b[6 - hh:, cc] = p[6 - hh:, cc]
            assert not c4_fours(b, 1) and not c4_fours(b, -1)
            state = c4_state(b)
            if h < 6:
                i, succ = t.add(state, 'columns', c)
                after = np.frombuffer(succ[0], np.int8).reshape(6, 7)
                assert after[5 - h, c] == (1, -1)[state[1]] and (after != b).sum() == 1
            else:
                i, _ = t.add(state, 'columns')
                assert t.rows[i]['valid'][c] == 0
                t.count('columns', 'full_columns')
            assert (t.rows[i]['valid'] == (b[0] == 0)).all()
            t.count('columns', 'col_heights')
    d, valid = t.arrays()
    d['valids'] = valid
    del d['kc']
    save('c4_rules_edge', d, out_dir, verbose, RE.C4_FLOORS, t)


def main(which=None, out_dir=None, verbose=True):
    which = which or ['br', 'c4']
    rh.import_reference()
    if 'br' in which:
        gen_br(out_dir, verbose)
    if 'c4' in which:
        gen_c4(out_dir, verbose)


if __name__ == '__main__':
    main(sys.argv[1:])
