"""othello GameState (host-side plugin; API of alphazero/envs/othello/othello.pyx:17-120 + OthelloLogic.pyx).
Device rules for the search live in csrc/azg_games.h (struct OT); this class is the Python object callers hold.

As in the reference there is no pass action: the game ends as soon as the player to move has no legal move, even if the
opponent still has one, and the disc difference from the mover's colour decides it (othello.pyx:83-96)."""
from typing import List, Tuple

import numpy as np

from ..Game import GameState

BOARD_SIZE, NUM_PLAYERS, NUM_CHANNELS = 8, 2, 1
MAX_TURNS = BOARD_SIZE * BOARD_SIZE
ACTION_SIZE = BOARD_SIZE * BOARD_SIZE
DIRECTIONS = ((1, 1), (1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1), (0, 1))      # OthelloLogic.pyx:24


class Board:
    """`pieces` int32[8,8] indexed [x][y], 1 / -1 / 0, as OthelloLogic.pyx:31-46; action a plays pieces.flat[a]."""

    def __init__(self, pieces=None):
        if pieces is not None:
            self.pieces = np.asarray(pieces, np.intc)
            return
        n = BOARD_SIZE
        self.pieces = np.zeros((n, n), dtype=np.intc)
        self.pieces[n // 2 - 1, n // 2] = self.pieces[n // 2, n // 2 - 1] = 1
        self.pieces[n // 2 - 1, n // 2 - 1] = self.pieces[n // 2, n // 2] = -1

    def _run(self, x, y, dx, dy, color):
        """the opponent stones a stone of `color` at (x, y) closes in direction (dx, dy), or [] (_get_flips :162-176)"""
        run = []
        x, y = x + dx, y + dy
        while 0 <= x < BOARD_SIZE and 0 <= y < BOARD_SIZE:
            v = self.pieces[x, y]
            if v == -color:
                run.append((x, y))
            elif v == color:
                return run
            else:
                return []
            x, y = x + dx, y + dy
        return []

    def legal_mask(self, color):                              # get_legal_moves (:67-78) as a mask over x*8 + y
        m = np.zeros(ACTION_SIZE, np.intc)
        for x in range(BOARD_SIZE):
            for y in range(BOARD_SIZE):
                if self.pieces[x, y] == 0 and any(self._run(x, y, dx, dy, color) for dx, dy in DIRECTIONS):
                    m[x * BOARD_SIZE + y] = 1
        return m

    def execute_move(self, x, y, color):                      # :121-142
        flips = [p for dx, dy in DIRECTIONS for p in self._run(x, y, dx, dy, color)]
        if not flips:
            raise ValueError('illegal move (%d, %d) for colour %d' % (x, y, color))
        self.pieces[x, y] = color
        for fx, fy in flips:
            self.pieces[fx, fy] = color

    def count_diff(self, color):                              # :60-65
        return int((self.pieces * color).sum())

    def __str__(self):
        return str(self.pieces)


class Game(GameState):
    AZG_GAME_ID = 3

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

    def _color(self):                                          # _player_range (othello.pyx:65-66)
        return (1, -1)[self.player]

    def valid_moves(self):
        return self._board.legal_mask(self._color())

    def play_action(self, action: int) -> None:
        super().play_action(action)
        self._board.execute_move(action // BOARD_SIZE, action % BOARD_SIZE, self._color())
        self._update_turn()

    def win_state(self) -> np.ndarray:
        result = np.zeros(NUM_PLAYERS + 1, np.uint8)
        if not self.valid_moves().any():
            diff = self._board.count_diff(self._color())
            result[self.player if diff > 0 else 1 - self.player if diff < 0 else NUM_PLAYERS] = 1
        return result

    def observation(self):
        return self._board.pieces[None].astype(np.float32)

    def symmetries(self, pi) -> List[Tuple['Game', np.ndarray]]:
        """the reference's order (othello.pyx:101-120): entry 2(i-1) + (0 if mirrored else 1) is fliplr^mirrored(rot90^i), i = 1..4 --
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

    # ---- device-engine conversion (include/azg.h azg_state: cells[8x + y] = pieces[x][y]) ----
    def to_azg_state(self):
        return np.asarray(self._board.pieces, np.int8).reshape(-1), self._player, self._turns

    @classmethod
    def from_azg_state(cls, cells, player, turns):
        g = cls()
        g._board.pieces = np.asarray(cells, np.intc).reshape(BOARD_SIZE, BOARD_SIZE).copy()
        g._player, g._turns = int(player), int(turns)
        return g
