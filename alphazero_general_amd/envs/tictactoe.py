"""tic-tac-toe GameState (host-side plugin; API of alphazero/envs/tictactoe/tictactoe.py:15-102 + TicTacToeLogic.py).
Device rules for the search live in csrc/azg_games.h (struct TT); this class is the Python object callers hold.

As in the reference every empty cell is a legal move, also at a position that is already won; win_state looks at the
mover's lines first, then the opponent's, then the full board (tictactoe.py:67-78), and turns never decide anything:
max_turns() is None (Game.py:56-58), so the default temperature schedule never steps (utils.py:19-23)."""
from typing import List, Tuple

import numpy as np

from ..Game import GameState

BOARD_SIZE, NUM_PLAYERS, NUM_CHANNELS = 3, 2, 1
ACTION_SIZE = BOARD_SIZE * BOARD_SIZE


class Board:
    """`pieces` int32[3,3] indexed [x][y], 1 / -1 / 0, as TicTacToeLogic.py:20-37; action a plays pieces.flat[a]."""

    def __init__(self, pieces=None):
        n = BOARD_SIZE
        self.n = n
        self.pieces = np.zeros((n, n), dtype=np.intc) if pieces is None else np.asarray(pieces, np.intc)

    def legal_mask(self):                                     # get_legal_moves (:39-52) as a mask over x*3 + y
        return (self.pieces == 0).astype(np.uint8).reshape(-1)

    def is_win(self, color):
        """:61-105: the count along a strip is never reset, so a strip wins iff all three of its cells hold the colour"""
        m = self.pieces == color
        return bool(m.all(0).any() or m.all(1).any() or m.diagonal().all() or np.fliplr(m).diagonal().all())

    def execute_move(self, x, y, color):                      # :107-116
        if self.pieces[x, y] != 0:
            raise ValueError('illegal move (%d, %d): the cell is taken' % (x, y))
        self.pieces[x, y] = color

    def __str__(self):
        return str(self.pieces)


class Game(GameState):
    AZG_GAME_ID = 5

    def __init__(self):
        super().__init__(Board())

    def __hash__(self):
        return hash(self._board.pieces.tobytes() + bytes([self.turns & 255]) + bytes([self._player]))

    def __eq__(self, other):
        return (self._board.pieces == other._board.pieces).all() and self._player == other._player and self.turns == other.turns

    def clone(self):
        g = Game()
        g._board.pieces = np.copy(self._board.pieces)
        g._player, g._turns, g.last_action = self._player, self._turns, self.last_action
        return g

    @staticmethod
    def max_turns():
        return None                                           # the reference's default (Game.py:56-58): tictactoe.py does not override it

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

    def _color(self):                                         # _player_range (tictactoe.py:50-51)
        return (1, -1)[self.player]

    def valid_moves(self):
        return self._board.legal_mask()

    def play_action(self, action: int) -> None:
        super().play_action(action)
        self._board.execute_move(action // BOARD_SIZE, action % BOARD_SIZE, self._color())
        self._update_turn()

    def win_state(self) -> np.ndarray:
        result = np.zeros(NUM_PLAYERS + 1, np.uint8)
        color = self._color()
        if self._board.is_win(color):
            result[self.player] = 1
        elif self._board.is_win(-color):
            result[1 - self.player] = 1
        elif not (self._board.pieces == 0).any():
            result[NUM_PLAYERS] = 1
        return result

    def observation(self):
        return self._board.pieces[None].astype(np.float32)

    def symmetries(self, pi) -> List[Tuple['Game', np.ndarray]]:
        """the reference's order (tictactoe.py:83-102): entry 2(i-1) + (0 if mirrored else 1) is fliplr^mirrored(rot90^i), i = 1..4 --
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

    # ---- device-engine conversion (include/azg.h azg_state: cells[3x + y] = pieces[x][y]) ----
    def to_azg_state(self):
        return np.asarray(self._board.pieces, np.int8).reshape(-1), self._player, self._turns

    @classmethod
    def from_azg_state(cls, cells, player, turns):
        g = cls()
        g._board.pieces = np.asarray(cells, np.intc).reshape(BOARD_SIZE, BOARD_SIZE).copy()
        g._player, g._turns = int(player), int(turns)
        return g
