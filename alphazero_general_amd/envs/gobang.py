"""gobang GameState (host-side plugin; API of alphazero/envs/gobang/gobang.pyx:41-182 + GobangLogic.pyx).
Device rules for the search live in csrc/azg_games.h (struct GB); this class is the Python object callers hold.

15x15, five in a row, every empty cell is legal.  win_state is absolute (index 0 when colour 1 holds a five, 1 for colour -1),
overlines count, and a full board without a five is a draw.  Of two colours that both hold a five (a position play never reaches,
but one a caller can load) the one whose run the reference's scan meets first wins: start cells in [x][y] order."""
from typing import List, Tuple

import numpy as np

from ..Game import GameState

BOARD_SIZE, NUM_PLAYERS, NUM_CHANNELS, NUM_IN_ROW = 15, 2, 4, 5
MAX_TURNS = BOARD_SIZE * BOARD_SIZE
ACTION_SIZE = BOARD_SIZE * BOARD_SIZE
STEPS = ((1, 0), (0, 1), (1, 1), (1, -1))           # get_win_state's four tests at a start cell, in its order (GobangLogic.pyx:66-86)


class Board:
    """`pieces` int32[15,15] indexed [x][y], 1 / -1 / 0, as GobangLogic.pyx; action a plays pieces.flat[a]."""

    def __init__(self, pieces=None):
        self.pieces = np.zeros((BOARD_SIZE, BOARD_SIZE), np.intc) if pieces is None else np.asarray(pieces, np.intc)

    def five_at(self, x, y):
        """the colour of a run of five that starts at (x, y) in one of the four directions, or 0"""
        c = self.pieces[x, y]
        if c == 0:
            return 0
        for dx, dy in STEPS:
            ex, ey = x + dx * (NUM_IN_ROW - 1), y + dy * (NUM_IN_ROW - 1)
            if 0 <= ex < BOARD_SIZE and 0 <= ey < BOARD_SIZE and all(self.pieces[x + dx * k, y + dy * k] == c for k in range(NUM_IN_ROW)):
                return int(c)
        return 0

    def fives(self, colour):
        """[15, 15] bool: (x, y) starts a run of five of `colour` in one of the four directions"""
        m = np.pad(self.pieces == colour, ((0, NUM_IN_ROW), (NUM_IN_ROW, NUM_IN_ROW)))
        n, o = BOARD_SIZE, NUM_IN_ROW
        out = np.zeros((n, n), bool)
        for dx, dy in STEPS:
            r = np.ones((n, n), bool)
            for k in range(NUM_IN_ROW):
                r &= m[dx * k:dx * k + n, o + dy * k:o + dy * k + n]
            out |= r
        return out

    def win_state(self):                                # get_win_state: (game over, colour); the first start cell in [x][y] order decides
        f0, f1 = self.fives(1).reshape(-1), self.fives(-1).reshape(-1)
        if f0.any() or f1.any():
            i0 = int(np.argmax(f0)) if f0.any() else ACTION_SIZE
            i1 = int(np.argmax(f1)) if f1.any() else ACTION_SIZE
            return True, 1 if i0 < i1 else -1
        return not (self.pieces == 0).any(), 0

    def __str__(self):
        return str(self.pieces)


class Game(GameState):
    AZG_GAME_ID = 4

    def __init__(self):
        super().__init__(Board())

    def __hash__(self):
        return hash(self._board.pieces.tobytes() + bytes([self.turns]) + bytes([self._player]))

    def __eq__(self, other):
        return (self._board.pieces == other._board.pieces).all() and self._player == other._player and self.turns == other.turns

    def clone(self):
        g = Game()
        g._board.pieces = np.copy(self._board.pieces)
        g._player, g._turns, g.last_action = self._player, self._turns, self.last_action
        return g

    @staticmethod
    def max_turns():
        return MAX_TURNS

    @staticmethod
    def has_draw():
        return True

    @staticmethod
    def num_players():
        return NUM_PLAYERS

    @staticmethod
    def action_size():
        return ACTION_SIZE

    @staticmethod
    def observation_size() -> Tuple[int, int, int]:
        return NUM_CHANNELS, BOARD_SIZE, BOARD_SIZE

    def valid_moves(self):
        return (self._board.pieces.reshape(-1) == 0).astype(np.uint8)

    def play_action(self, action: int) -> None:
        super().play_action(action)
        x, y = divmod(int(action), BOARD_SIZE)
        if self._board.pieces[x, y] != 0:
            raise ValueError('invalid move (%d, %d)' % (x, y))
        self._board.pieces[x, y] = (1, -1)[self.player]
        self._update_turn()

    def win_state(self) -> np.ndarray:
        result = np.zeros(NUM_PLAYERS + 1, np.uint8)
        over, c = self._board.win_state()
        if over:
            result[0 if c == 1 else 1 if c == -1 else NUM_PLAYERS] = 1
        return result

    def observation(self):
        p = self._board.pieces
        return np.array([p == 1, p == -1, np.full_like(p, self.player), np.full(p.shape, self.turns / MAX_TURNS, np.float32)], np.float32)

    def symmetries(self, pi) -> List[Tuple['Game', np.ndarray]]:
        """the reference's order (gobang.pyx:159-182): entry 2(i-1) + (0 if mirrored else 1) is fliplr^mirrored(rot90^i), i = 1..4 --
        the identity is the LAST entry"""
        pi_board = np.reshape(pi, (BOARD_SIZE, BOARD_SIZE))
        out = []
        for i in range(1, 5):
            for flip in (True, False):
                b, p = np.rot90(self._board.pieces, i), np.rot90(pi_board, i)
                if flip:
                    b, p = np.fliplr(b), np.fliplr(p)
                g = self.clone()
                g._board.pieces = np.ascontiguousarray(b)
                out.append((g, p.ravel()))
        return out

    # ---- device-engine conversion (cells[15x + y] = pieces[x][y]; engine.py packs them into include/azg.h azg_state) ----
    def to_azg_state(self):
        return np.asarray(self._board.pieces, np.int8).reshape(-1), self._player, self._turns

    @classmethod
    def from_azg_state(cls, cells, player, turns):
        g = cls()
        g._board.pieces = np.asarray(cells, np.intc).reshape(BOARD_SIZE, BOARD_SIZE).copy()
        g._player, g._turns = int(player), int(turns)
        return g
