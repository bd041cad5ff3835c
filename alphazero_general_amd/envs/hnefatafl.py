"""hnefatafl (11x11 tafl) GameState -- host-side plugin with the API of alphazero/envs/hnefatafl/fastafl.pyx:122-259 (which at
the reference snapshot lacks has_draw()/max_turns(), SURVEY.md Q19: both are provided here).  Rules follow
fastafl/cengine.pyx with variants.hnefatafl_args: NO two-sided king capture -- the king is never taken by custodian capture;
it is captured when every in-bounds neighbour holds a piece of code 2, the empty throne or a corner, recomputed from the board
at every win test (Board.king_captured), or when the group-surround check meets it -- moves over the empty throne, king cannot
re-enter the throne.  Device rule kernels for the search: csrc/azg_games.h struct HN; this class is the Python object callers
hold (Arena.play_game, GenericPlayers, GUI-style code)."""
from typing import List, Tuple

import numpy as np

from ..Game import GameState

W = H = 11
NUM_PLAYERS, NUM_CHANNELS, DRAW_MOVE_COUNT = 2, 5, 512
MOVE_TYPES = W + H - 2
ACTION_SIZE = W * H * MOVE_TYPES
ATT, DEF, KING, THRONE, ESCAPE, KING_THRONE, KING_ESCAPE = 1, 2, 3, 4, 5, 7, 8
_KINGS = (KING, KING_THRONE, KING_ESCAPE)
_ATTACKERS = (ATT,) + _KINGS
_DIRS = ((0, 1), (1, 0), (0, -1), (-1, 0))
_KING_CAPTURE = (DEF, THRONE, ESCAPE)                          # cengine.pyx:44


def _start():
    """the standard 11x11 opening: corners, the king on the throne, its twelve men in the diamond around it, six men of code 2 in a T
    on the middle of every edge"""
    s = np.zeros((H, W), np.int8)
    for y in range(H):
        for x in range(W):
            dx, dy = abs(x - 5), abs(y - 5)
            if dx == 5 and dy == 5:
                s[y, x] = ESCAPE
            elif dx == 0 and dy == 0:
                s[y, x] = KING_THRONE
            elif dx + dy <= 2:
                s[y, x] = ATT
            elif (dy == 5 and dx <= 2) or (dx == 5 and dy <= 2) or (dy == 4 and dx == 0) or (dx == 4 and dy == 0):
                s[y, x] = DEF
    return s


_START = _start()


def get_move(action):
    """action -> ((x, y), (new_x, new_y))   (fastafl.pyx:46-63)"""
    mt, a = action % MOVE_TYPES, action // MOVE_TYPES
    x, y = a % W, a // W
    if mt < H - 1:
        return (x, y), (x, mt + (1 if mt >= y else 0))
    nx = mt - H + 1
    return (x, y), (nx + (1 if nx >= x else 0), y)


def get_action(src, dst):
    """fastafl.pyx:66-79"""
    (x, y), (nx, ny) = src, dst
    mt = (ny if ny < y else ny - 1) if x == nx else (H + nx - 1 - (1 if nx >= x else 0))
    return MOVE_TYPES * (x + y * W) + mt


_SYM_ACTIONS = {}


def _sym_actions(i, flip):
    """where every action goes under rot90^i then fliplr^flip: the reference's coordinate loop (fastafl.pyx:234-253), worked out once"""
    if (i, flip) not in _SYM_ACTIONS:
        out = np.zeros(ACTION_SIZE, np.int64)
        for a in range(ACTION_SIZE):
            (x, y), (nx, ny) = get_move(a)
            for _ in range(i):
                x, nx, y, ny = W - 1 - y, W - 1 - ny, x, nx
            if flip:
                x, nx = W - 1 - x, W - 1 - nx
            out[a] = get_action((x, y), (nx, ny))
        _SYM_ACTIONS[(i, flip)] = out
    return _SYM_ACTIONS[(i, flip)]


class Board:
    def __init__(self):
        self._state = _START.copy()
        self.num_turns = 0
        self._king_captured = False

    def copy(self):
        b = Board.__new__(Board)
        b._state, b.num_turns, b._king_captured = self._state.copy(), self.num_turns, self._king_captured
        return b

    def to_play(self):
        return 2 - self.num_turns % 2

    def _ok(self, x, y):
        return 0 <= x < W and 0 <= y < H

    def _valid(self, x, y, king):
        if not self._ok(x, y):
            return False
        v = self._state[y, x]
        return v == 0 or (v == ESCAPE and king)

    def legal_moves(self, team):
        s, out = self._state, []
        for y in range(H):
            for x in range(W):
                v = s[y, x]
                if not (v in _ATTACKERS if team == ATT else v == DEF):
                    continue
                king = v in _KINGS
                for dx, dy in _DIRS:
                    cx, cy = x + dx, y + dy
                    thr = self._ok(cx, cy) and s[cy, cx] == THRONE
                    while thr or self._valid(cx, cy, king):
                        if not thr:
                            out.append(((x, y), (cx, cy)))
                        cx, cy = cx + dx, cy + dy
                        thr = self._ok(cx, cy) and s[cy, cx] == THRONE
        return out

    def _group_blocked(self, start, enemy):
        s, group, stack = self._state, {start}, [start]
        while stack:
            x, y = stack.pop()
            for dx, dy in _DIRS:
                nx, ny = x + dx, y + dy
                if not self._ok(nx, ny):
                    continue
                v = s[ny, nx]
                if v == 0:
                    return None
                if v in enemy and (nx, ny) not in group:
                    group.add((nx, ny)); stack.append((nx, ny))
        return group

    def move(self, src, dst):
        s = self._state
        (x, y), (nx, ny) = src, dst
        v = s[y, x]
        piece = KING if v in (KING_THRONE, KING_ESCAPE) else v
        s[y, x] = THRONE if v == KING_THRONE else ESCAPE if v == KING_ESCAPE else 0
        d = s[ny, nx]
        s[ny, nx] = piece + d if d in (THRONE, ESCAPE) else piece
        pv = s[ny, nx]
        friendly = _ATTACKERS if pv in _ATTACKERS else (pv,)
        enemy = 3 - pv if pv != KING else DEF
        for dx, dy in _DIRS:                                  # custodian capture (cengine.pyx:174-199)
            ex, ey = nx + dx, ny + dy
            if not self._ok(ex, ey):
                continue
            if s[ey, ex] == enemy:                            # (king_two_sided_capture is off: a king is never the enemy here)
                fx, fy = ex + dx, ey + dy
                if self._ok(fx, fy) and (s[fy, fx] in friendly or s[fy, fx] in (THRONE, ESCAPE)):
                    s[ey, ex] = 0
        enemy_set = _ATTACKERS if s[ny, nx] == DEF else (DEF,)   # group surround (cengine.pyx:204-247)
        seen = set()
        for dx, dy in _DIRS:
            ex, ey = nx + dx, ny + dy
            if not self._ok(ex, ey) or s[ey, ex] not in enemy_set or (ex, ey) in seen:
                continue
            grp = self._group_blocked((ex, ey), enemy_set)
            if grp is None:
                continue
            seen |= grp
            for gx, gy in grp:
                if s[gy, gx] in _KINGS:
                    self._king_captured = True
                else:
                    s[gy, gx] = 0
        self.num_turns += 1

    def _has_legals(self, team):
        s = self._state
        for y in range(H):
            for x in range(W):
                v = s[y, x]
                if v in _ATTACKERS if team == ATT else v == DEF:
                    if any(self._valid(x + dx, y + dy, v in _KINGS) for dx, dy in _DIRS):
                        return True
        return False

    def king_captured(self):
        """cengine.pyx:154-161: the flag the group-surround check left, or a king whose in-bounds neighbours all hold 2 / throne / corner"""
        if self._king_captured:
            return True
        s = self._state
        for y, x in zip(*np.nonzero(np.isin(s, _KINGS))):
            if all(s[y + dy, x + dx] in _KING_CAPTURE for dx, dy in _DIRS if self._ok(x + dx, y + dy)):
                return True
        return False

    def get_winner(self):
        if (self._state == KING_ESCAPE).any() or not self._has_legals(DEF):
            return ATT
        if self.king_captured() or not self._has_legals(ATT):
            return DEF
        return 0

    def __str__(self):
        return '\n'.join(' '.join(str(v) for v in row) for row in self._state)


class Game(GameState):
    AZG_GAME_ID = 6

    def __init__(self, _board=None):
        super().__init__(_board or Board())
        self.last_action = -1

    def __eq__(self, other):
        return (self._board._state == other._board._state).all() and self._player == other._player and self._turns == other._turns

    def clone(self):
        g = Game(self._board.copy())
        g._player, g._turns, g.last_action = self._player, self._turns, self.last_action
        return g

    @staticmethod
    def num_players():
        return NUM_PLAYERS

    @staticmethod
    def action_size():
        return ACTION_SIZE

    @staticmethod
    def observation_size() -> Tuple[int, int, int]:
        return NUM_CHANNELS, W, H

    @staticmethod
    def has_draw():
        return True

    @staticmethod
    def max_turns():
        return DRAW_MOVE_COUNT

    def valid_moves(self):
        v = np.zeros(ACTION_SIZE, dtype=np.uint8)
        for src, dst in self._board.legal_moves(self._board.to_play()):
            v[get_action(src, dst)] = 1
        return v

    def play_action(self, action: int) -> None:
        self.last_action = action
        src, dst = get_move(int(action))
        self._board.move(src, dst)
        self._update_turn()

    def win_state(self) -> np.ndarray:
        r = np.zeros(NUM_PLAYERS + 1, dtype=np.uint8)
        if self.turns >= DRAW_MOVE_COUNT:
            r[NUM_PLAYERS] = 1
        else:
            w = self._board.get_winner()
            if w:
                r[2 - w] = 1
        return r

    def observation(self):
        s = self._board._state
        return np.array([s == DEF, s == ATT, np.isin(s, _KINGS), np.full(s.shape, self._board.num_turns % 2),
                         np.full(s.shape, self._board.num_turns // DRAW_MOVE_COUNT)], dtype=np.float32)

    def symmetries(self, pi) -> List[Tuple['Game', np.ndarray]]:
        syms = []
        for i in range(1, 5):
            for flip in (False, True):
                st = np.rot90(self._board._state, i)
                if flip:
                    st = np.fliplr(st)
                new_pi = np.zeros(ACTION_SIZE, dtype=np.float32)
                new_pi[_sym_actions(i, flip)] = pi
                g = self.clone()
                g._board._state = np.ascontiguousarray(st)
                syms.append((g, new_pi))
        return syms

    def to_azg_state(self):
        return self._board._state.reshape(-1).astype(np.int8), self._player, self._turns, int(self._board._king_captured)

    @classmethod
    def from_azg_state(cls, cells, player, turns, king_captured=0):
        g = cls()
        g._board._state = np.asarray(cells, np.int8).reshape(H, W).copy()
        g._board.num_turns = int(turns)
        g._board._king_captured = bool(king_captured)
        g._player, g._turns = int(player), int(turns)
        return g
