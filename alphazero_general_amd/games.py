"""DeviceGames: the rules of a device game on tensors of positions, without an engine or a tree -- the batched form of the reference's
GameState plugin (alphazero/Game.py:7-113: valid_moves, play_action, win_state, observation, symmetries) over azg_game_step /
azg_game_symmetries (include/azg.h).  What it is for: evaluating a net on a batch of positions, policy-only play (NNPlayer,
GenericPlayers.py:55-97), expanding stored (state, pi) samples into their symmetries at training time, writing another search.

A position is one row of a uint8 tensor [n, 80]: the bytes of an azg_state.  `pack` / `unpack` / `to_games` convert from and to host
objects (this package's envs, the reference's own classes, or (cells, player, turns[, aux0]) tuples); `step`, `symmetries`, `choose`
(the move of a player without a tree: RandomPlayer, NNPlayer), `lookahead` (the children of every position, one ply) and
`choose_scripted` (the reference's scripted baseline player of the game) are one kernel launch each on torch's current stream, read nothing back and, given `out=`, allocate nothing -- so a play loop can be captured
in a graph.  There is no CPU path for the rules themselves: `step` / `symmetries` need a HIP device."""
import collections
import ctypes as C

import numpy as np
import torch

from . import _abi
from ._abi import ptr as _ptr, stream as _stream
from .Game import azg_game_id

STATE_BYTES = C.sizeof(_abi.State)                              # 80
Step = collections.namedtuple('Step', 'next valid win obs status')
Symmetries = collections.namedtuple('Symmetries', 'states obs pi')
Choice = collections.namedtuple('Choice', 'actions status')
Lookahead = collections.namedtuple('Lookahead', 'num actions win children obs')
_OBS_FORMS = {torch.float32: 0, torch.float16: 1, 'nhwc8': 2}


class DeviceGames:
    def __init__(self, game_cls, device=None):
        """game_cls: a GameState class (or instance) with device rules -- this package's envs or the reference's own classes (Game.azg_game_id).
        device: where the tensors live; default the current HIP device, or the CPU where there is none (pack / unpack only)."""
        self.L = _abi.lib()
        self.game_cls = game_cls if isinstance(game_cls, type) else type(game_cls)
        self.game = int(azg_game_id(game_cls))
        gi = self.gi = _abi.game_info(self.game)
        self.A, self.P, self.NV, self.NSYM = gi.action_size, gi.num_players, gi.num_players + 1, gi.num_symmetries
        self.obs_shape = (gi.obs_c, gi.obs_h, gi.obs_w)
        self.cells = gi.cells
        self.max_children = gi.max_children
        name = self.L.azg_game_scripted_player(self.game)
        self.scripted_player = None if name is None else name.decode()   # the reference's scripted baseline player (class name), or None
        if device is None:
            device = torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else torch.device('cpu')
        self.device = torch.device(device)

    # ---- host <-> azg_state rows ------------------------------------------------------------------------------
    def pack(self, games_or_tuples):
        """GameState objects or (cells, player, turns[, aux0]) tuples (cells as Python callers hold them: gobang's 225, hnefatafl's 121
        int8 cells) -> uint8 tensor [n, 80] of azg_state rows on the device"""
        from .MCTS import encode_state
        items = list(games_or_tuples)
        raw = np.zeros((len(items), STATE_BYTES), np.uint8)
        words = raw[:, 64:].view('<i4')                          # player, turns, aux[0], aux[1]
        for i, it in enumerate(items):
            st = tuple(it) if isinstance(it, (tuple, list)) else encode_state(it)
            c = np.ascontiguousarray(_abi.cells_to_state(self.game, st[0])).view(np.uint8)
            assert c.size <= 64, 'a board of %d cells does not fit azg_state.cells' % c.size
            raw[i, :c.size] = c
            words[i, 0], words[i, 1] = int(st[1]), int(st[2])
            words[i, 2] = int(st[3]) if len(st) > 3 else 0
        return torch.from_numpy(raw).to(self.device)

    def unpack(self, states):
        """uint8 [n, 80] -> list of (cells int8, player, turns, aux0), cells as Python callers hold them"""
        raw = self._rows(states, need_device=False).cpu().numpy()
        out = []
        for row in raw:
            s = _abi.State.from_buffer_copy(row.tobytes())
            out.append((_abi.state_cells(s, self.game, self.cells), int(s.player), int(s.turns), int(s.aux[0])))
        return out

    def to_games(self, states, template=None):
        """GameState objects of template's class (default: an object of the class this DeviceGames was made for)"""
        from .MCTS import decode_state
        template = self.game_cls() if template is None else template
        return [decode_state(template, *st) for st in self.unpack(states)]

    def initial(self, n):
        """n copies of the opening position"""
        return self.pack([self.game_cls()]).repeat(int(n), 1).contiguous()

    # ---- argument checks ----------------------------------------------------------------------------------------
    def _rows(self, states, need_device=True):
        assert isinstance(states, torch.Tensor) and states.dtype == torch.uint8, 'states: a uint8 tensor [n, 80]'
        assert states.dim() == 2 and states.shape[1] == STATE_BYTES and states.is_contiguous(), 'states: contiguous [n, 80]'
        if need_device:
            assert states.is_cuda and states.device == self.device, 'states must live on %s (there is no CPU path for the rules)' % (self.device,)
        return states

    def _buf(self, given, want, name, n, tail, dtype):
        """the output `name`: None when not wanted, the caller's buffer (checked; it may hold more rows than n) or a new one"""
        if not want:
            return None
        if given is None:
            return torch.zeros((n,) + tail, dtype=dtype, device=self.device)
        assert isinstance(given, torch.Tensor) and given.dtype == dtype and given.device == self.device and given.is_contiguous(), \
            'out.%s: a contiguous %s tensor on %s' % (name, dtype, self.device)
        assert given.dim() == 1 + len(tail) and tuple(given.shape[1:]) == tail and given.shape[0] >= n, \
            'out.%s: shape [>= %d]%s, got %s' % (name, n, list(tail), list(given.shape))
        return given

    def obs_tail(self, form):
        """shape of one observation in format `form` (torch.float32 / torch.float16: NCHW planes; 'nhwc8': fp16 rows of 8 channels)"""
        c, h, w = self.obs_shape
        return (h * w, 8) if form == 'nhwc8' else (c, h, w)

    # ---- the launches ---------------------------------------------------------------------------------------
    def step(self, states, actions=None, *, next=True, valid=True, win=True, obs=None, out=None):
        """play actions[i] on states[i] where it is legal (GameState.play_action; an illegal or out-of-range action leaves the position
        as it is and sets status 1; -1 or actions=None: no move), then of the resulting positions return a Step record:
          next   uint8 [n, 80]     the positions                       valid  uint8 [n, A]      GameState.valid_moves
          win    uint8 [n, P + 1]  GameState.win_state                 status int32 [n]         1: the action was refused (None without actions)
          obs    GameState.observation: None, torch.float32 / torch.float16 ([n, C, H, W]) or 'nhwc8' (fp16 [n, H*W, 8])
        An output whose flag is false is None.  out: a Step whose tensors are written instead of new ones (they may hold more than n rows;
        rows from n on are left alone, and the record returned holds the first n); out.next may be `states` itself.  A non-zero status is
        returned, never raised."""
        states = self._rows(states)
        n = states.shape[0]
        assert obs is None or obs in _OBS_FORMS, 'obs: None, torch.float32, torch.float16 or \'nhwc8\''
        o = out if out is not None else Step(None, None, None, None, None)
        if actions is not None:
            assert isinstance(actions, torch.Tensor) and actions.dtype == torch.int32 and actions.device == self.device, 'actions: int32 on the device'
            assert actions.dim() == 1 and actions.shape[0] == n and actions.is_contiguous(), 'actions: contiguous [n]'
        b_next = self._buf(o.next, next, 'next', n, (STATE_BYTES,), torch.uint8)
        b_valid = self._buf(o.valid, valid, 'valid', n, (self.A,), torch.uint8)
        b_win = self._buf(o.win, win, 'win', n, (self.NV,), torch.uint8)
        b_obs = self._buf(o.obs, obs is not None, 'obs', n, self.obs_tail(obs), torch.float32 if obs == torch.float32 else torch.float16)
        b_status = self._buf(o.status, actions is not None, 'status', n, (), torch.int32)
        with torch.cuda.device(self.device):
            _abi.check(self.L.azg_game_step(_stream(), self.game, n, _ptr(states), _ptr(actions), _ptr(b_next), _ptr(b_valid), _ptr(b_win),
                                            _ptr(b_obs), _OBS_FORMS.get(obs, 0), _ptr(b_status)))
        return Step(*[None if b is None else b[:n] for b in (b_next, b_valid, b_win, b_obs, b_status)])

    def symmetries(self, states, pi=None, *, obs=True, states_out=True, out=None):
        """GameState.symmetries(pi) of every position, all NSYM entries in the reference's list order: a Symmetries record of
        states uint8 [n, NSYM, 80], obs float32 [n, NSYM, C, H, W] and pi float32 [n, NSYM, A] (None without pi: nothing is written to
        out.pi then).  out: a Symmetries whose tensors are written instead of new ones."""
        states = self._rows(states)
        n = states.shape[0]
        o = out if out is not None else Symmetries(None, None, None)
        if pi is not None:
            assert isinstance(pi, torch.Tensor) and pi.dtype == torch.float32 and pi.device == self.device, 'pi: float32 on the device'
            assert tuple(pi.shape) == (n, self.A) and pi.is_contiguous(), 'pi: contiguous [n, A]'
        b_states = self._buf(o.states, states_out, 'states', n, (self.NSYM, STATE_BYTES), torch.uint8)
        b_obs = self._buf(o.obs, obs, 'obs', n, (self.NSYM,) + self.obs_shape, torch.float32)
        b_pi = self._buf(o.pi, pi is not None, 'pi', n, (self.NSYM, self.A), torch.float32)
        with torch.cuda.device(self.device):
            _abi.check(self.L.azg_game_symmetries(_stream(), self.game, n, _ptr(states), _ptr(pi), _ptr(b_states), _ptr(b_obs), _ptr(b_pi)))
        return Symmetries(*[None if b is None else b[:n] for b in (b_states, b_obs, b_pi)])

    def choose(self, states, policy=None, temp=None, u=None, out=None):
        """the move of a player without a tree on every position (azg_game_choose), as a Choice record (actions int32 [n], status int32 [n]):
          policy=None          RandomPlayer.play (GenericPlayers.py:47-52): uniform over the valid moves
          policy float32 [n, A] NNPlayer.play (:69-94) with row i as the network's policy: masked, raised to 1 / temp[i] (temp float32 [n];
                               None: 1; an entry 0: the first maximum), normalised
        then np.random.choice given u[i], float64 [n] in [0, 1), the uniform that call draws; u=None draws torch.rand on the device.
        status 1 with action -1 where the reference would divide by zero (no valid move, options that sum to 0); returned, never raised.
        out: a Choice whose tensors are written instead of new ones (they may hold more than n rows)."""
        states = self._rows(states)
        n = states.shape[0]
        o = out if out is not None else Choice(None, None)
        if policy is not None:
            assert isinstance(policy, torch.Tensor) and policy.dtype == torch.float32 and policy.device == self.device, 'policy: float32 on the device'
            assert tuple(policy.shape) == (n, self.A) and policy.is_contiguous(), 'policy: contiguous [n, A]'
        if temp is not None:
            assert policy is not None, 'temp goes with a policy (RandomPlayer has no temperature)'
            assert isinstance(temp, torch.Tensor) and temp.dtype == torch.float32 and temp.device == self.device, 'temp: float32 on the device'
            assert tuple(temp.shape) == (n,) and temp.is_contiguous(), 'temp: contiguous [n]'
        if u is None:
            u = torch.rand(n, dtype=torch.float64, device=self.device)
        assert isinstance(u, torch.Tensor) and u.dtype == torch.float64 and u.device == self.device, 'u: float64 on the device'
        assert tuple(u.shape) == (n,) and u.is_contiguous(), 'u: contiguous [n]'
        b_actions = self._buf(o.actions, True, 'actions', n, (), torch.int32)
        b_status = self._buf(o.status, True, 'status', n, (), torch.int32)
        with torch.cuda.device(self.device):
            _abi.check(self.L.azg_game_choose(_stream(), self.game, n, _ptr(states), _ptr(policy), _ptr(temp), _ptr(u), _ptr(b_actions),
                                              _ptr(b_status)))
        return Choice(b_actions[:n], b_status[:n])

    def lookahead(self, states, *, win=True, children=False, obs=None, out=None):
        """the children of every position, one ply (azg_game_lookahead): the position's own move list -- valid_moves in ascending action
        order, k <= K = max_children entries -- played entry by entry with play_action on a copy, as a Lookahead record:
          num      int32 [n]           k                                actions  int32 [n, K]        the action of child j; -1 for j >= k
          win      uint8 [n, K, P + 1] win_state of child j             children uint8 [n, K, 80]    the child positions
          obs      observation of child j in the formats of `step`: [n, K, C, H, W] or, 'nhwc8', [n, K, H*W, 8]
        Rows j >= k of win / children / obs are left as they were (zero in a new tensor); an output whose flag is false is None.  The
        parent's win_state is not consulted: a finished position that still has moves has children.  out: a Lookahead whose tensors are
        written instead of new ones (they may hold more than n rows); none of them may be `states`.  perft is a loop of it:
            frontier = dg.initial(1)
            for depth in range(d):
                la = dg.lookahead(frontier, children=True)
                live = (la.actions >= 0) & (la.win.sum(2) == 0)        # children that exist and are not finished
                frontier = la.children[live]"""
        states = self._rows(states)
        n, K = states.shape[0], self.max_children
        assert obs is None or obs in _OBS_FORMS, 'obs: None, torch.float32, torch.float16 or \'nhwc8\''
        o = out if out is not None else Lookahead(None, None, None, None, None)
        b_num = self._buf(o.num, True, 'num', n, (), torch.int32)
        b_act = self._buf(o.actions, True, 'actions', n, (K,), torch.int32)
        b_win = self._buf(o.win, win, 'win', n, (K, self.NV), torch.uint8)
        b_ch = self._buf(o.children, children, 'children', n, (K, STATE_BYTES), torch.uint8)
        b_obs = self._buf(o.obs, obs is not None, 'obs', n, (K,) + self.obs_tail(obs), torch.float32 if obs == torch.float32 else torch.float16)
        assert b_ch is None or b_ch.data_ptr() != states.data_ptr(), 'out.children must not be `states`'
        with torch.cuda.device(self.device):
            _abi.check(self.L.azg_game_lookahead(_stream(), self.game, n, _ptr(states), _ptr(b_num), _ptr(b_act), _ptr(b_win), _ptr(b_ch),
                                                 _ptr(b_obs), _OBS_FORMS.get(obs, 0)))
        return Lookahead(*[None if b is None else b[:n] for b in (b_num, b_act, b_win, b_ch, b_obs)])

    def choose_scripted(self, states, u=None, out=None):
        """the move of the reference's scripted baseline player of this game (`scripted_player`: OneStepLookaheadConnect4Player,
        GreedyOthelloPlayer, GreedyGobangPlayer; azg_game_choose_scripted, include/azg.h for each player's rule) on every position, as a
        Choice record.  u float64 [n] in [0, 1): connect4 plays element min(m - 1, int(u[i] * m)) of the m moves of its chosen set in
        ascending order; the other two consume none; u=None draws torch.rand on the device.  status 1 with action -1 where there is no
        valid move (the reference raises); a game without a scripted player raises AzgError (AZG_E_UNSUPPORTED)."""
        states = self._rows(states)
        n = states.shape[0]
        o = out if out is not None else Choice(None, None)
        if u is None:
            u = torch.rand(n, dtype=torch.float64, device=self.device)
        assert isinstance(u, torch.Tensor) and u.dtype == torch.float64 and u.device == self.device, 'u: float64 on the device'
        assert tuple(u.shape) == (n,) and u.is_contiguous(), 'u: contiguous [n]'
        b_actions = self._buf(o.actions, True, 'actions', n, (), torch.int32)
        b_status = self._buf(o.status, True, 'status', n, (), torch.int32)
        with torch.cuda.device(self.device):
            _abi.check(self.L.azg_game_choose_scripted(_stream(), self.game, n, _ptr(states), _ptr(u), _ptr(b_actions), _ptr(b_status)))
        return Choice(b_actions[:n], b_status[:n])
