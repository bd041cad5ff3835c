"""Tree-free players without a GPU: the argument contract of azg_game_choose, the numpy restatement of RandomPlayer.play / NNPlayer.play
(tests/choose_reference.py) held to the reference's own classes, the margin rule the GPU test applies -- asserted here on the GPU test's
fixed inputs, before a GPU sees them -- and the per-player temperature table of a policy seat against a literal loop."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import choose_reference as R

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, 'golden')
REF = '/root/reference'
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, 'alphazero')), reason='needs the reference checkout (build container only)')


# ------------------------------------------------------------------------------------------------------------- the C entry point
def test_choose_argument_errors_without_a_device():
    """every argument is judged before the device is touched: the calls below never reach a launch (the pointers are not device memory)"""
    from alphazero_general_amd import _abi
    L = _abi.lib()
    assert L.azg_abi_version() == 7 == _abi.ABI_VERSION
    buf = (C.c_char * 4096)()
    p, null = C.cast(buf, C.c_void_p), C.c_void_p(0)
    ok = dict(game=_abi.GAME_CONNECT4, count=4, states=p, policy=null, temp=null, u=p, actions=p, status=p)

    def call(**kw):
        a = dict(ok, **kw)
        return L.azg_game_choose(null, a['game'], a['count'], a['states'], a['policy'], a['temp'], a['u'], a['actions'], a['status'])
    for bad in (dict(game=-1), dict(game=7), dict(count=-1), dict(states=null), dict(u=null), dict(actions=null), dict(status=null)):
        assert call(**bad) == _abi.E_INVALID_ARG, bad
        assert L.azg_last_error()
    for game in range(7):
        assert call(game=game, count=0) == 0                             # nothing launched
    assert call(count=0, policy=p, temp=p) == 0
    assert call(count=0, states=null) == _abi.E_INVALID_ARG              # (judged before the count)


def test_engine_entry_points_refuse_null_arguments():
    from alphazero_general_amd import _abi
    L = _abi.lib()
    null = C.c_void_p(0)
    out = C.c_void_p()
    assert L.azg_advance_actions(null, null, null, 0) == _abi.E_INVALID_ARG
    assert L.azg_states_dev(null, C.byref(out)) == _abi.E_INVALID_ARG


# ------------------------------------------------------------------------------------------------------------- the helper itself
def test_exactly_representable_boundaries_fall_to_the_right():
    """searchsorted(side='right'): a u that EQUALS a cdf entry belongs to the next move.  RandomPlayer with 2 or 4 valid moves has the
    exactly representable boundaries 0.5 and 0.25, 0.5, 0.75"""
    v2 = np.array([0, 1, 0, 0, 1, 0, 0, 0, 0], np.uint8)
    v4 = np.array([1, 0, 1, 0, 0, 1, 0, 0, 1], np.uint8)
    assert R.choose(v2, None, None, 0.5)[0] == 4 and R.choose(v2, None, None, np.nextafter(0.5, 0))[0] == 1
    assert R.choose(v4, None, None, 0.25)[0] == 2 and R.choose(v4, None, None, 0.5)[0] == 5 and R.choose(v4, None, None, 0.75)[0] == 8
    assert R.choose(v4, None, None, 0.0)[0] == 0 and R.choose(v4, None, None, np.nextafter(1.0, 0))[0] == 8
    cdf = R.choose(v4, None, None, 0.25)[1]
    assert cdf.dtype == np.float64 and R.near_boundary(cdf, 0.25) and not R.near_boundary(cdf, 0.3)


def test_helper_keeps_numpy2_float32():
    """what the device restates: the NNPlayer list holds float32 powers and np.sum of it stays float32"""
    opts = np.array([0.25, 0.5, 0.0], np.float32)
    probs = [x ** (1. / 0.2) for x in opts]
    assert all(type(x) is np.float32 for x in probs) and np.sum(probs).dtype == np.float32
    assert R.nn_probs(np.ones(3, np.uint8), opts, 0.2).dtype == np.float32
    assert R.random_probs(np.array([1, 0, 1], np.uint8)).dtype == np.float64


# ------------------------------------------------------------------------------------------------------------- against the reference
def reference_players_check():
    """(child process) the reference's RandomPlayer and NNPlayer under np.random.seed(s) against the helper fed RandomState(s)'s first
    uniform: the same action at every position"""
    sys.path.insert(0, G)
    sys.path.insert(0, os.path.dirname(HERE))
    import refharness as rh
    rh.import_reference()
    from alphazero.GenericPlayers import NNPlayer, RandomPlayer
    from alphazero.utils import dotdict
    from alphazero_general_amd.envs import brandubh, connect4
    rng = np.random.RandomState(7)
    checked = 0
    for Game in (connect4.Game, brandubh.Game):
        positions = []
        while len(positions) < 220:
            g = Game()
            while not g.win_state().any() and len(positions) < 220:
                positions.append(g.clone())
                g.play_action(int(rng.choice(np.flatnonzero(g.valid_moves()))))
        A = Game.action_size()
        rp = RandomPlayer(Game, dotdict())
        for s, g in enumerate(positions):
            valids = np.asarray(g.valid_moves())
            u = np.random.RandomState(s).random_sample()
            np.random.seed(s)
            assert int(rp.play(g)) == R.choose(valids, None, None, u)[0], ('RandomPlayer', Game.__module__, s)
            policy = (0.05 + 0.95 * rng.random_sample(A) ** 3).astype(np.float32)   # (no float32 underflow: np.seterr(all='raise'), MCTS.pyx:23)
            policy[rng.random_sample(A) < 0.2] = 0
            if (policy * valids).sum() == 0:
                policy[np.flatnonzero(valids)[0]] = 0.5
            policy /= policy.sum(dtype=np.float32)

            class Net:
                def predict(self, obs, policy=policy):
                    return policy, None
            for temp in R.TEMPS:
                player = NNPlayer(Net(), Game, dotdict(startTemp=temp, temp_scaling_fn=lambda t, *a: t))
                np.random.seed(s)
                got = int(player.play(g))
                assert got == R.choose(valids, policy, temp, u)[0], ('NNPlayer', Game.__module__, s, temp)
                checked += 1
    assert checked >= 2 * 200 * len(R.TEMPS)


@needs_reference
def test_helper_is_the_reference_players():
    code = 'import sys; sys.path.insert(0, %r); import test_choose_cpu as t; t.reference_players_check()' % HERE
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=900, env=env, cwd=os.path.dirname(HERE))
    assert r.returncode == 0, r.stderr[-3000:]


# ------------------------------------------------------------------------------------------------------------- the margin rule
@pytest.mark.parametrize('gid', range(7), ids=R.GAME_NAMES)
def test_gpu_inputs_keep_clear_of_the_boundaries(gid):
    """np_pow_f32 is a 1-ulp tier against powf, so the GPU test compares only the draws with no |cdf_j - u| < 1e-6.  The fixed inputs must
    leave at most 1 % of a game's draws that near a boundary -- and every expected action a valid move"""
    d = R.inputs(gid)
    act, near = R.expected(gid)
    assert act.shape == near.shape == (len(R.SETTINGS), R.N_POS) and d['valids'].shape[0] == R.N_POS
    assert near.sum() <= 0.01 * near.size and near.any(0).sum() <= 0.01 * R.N_POS, near.sum()
    assert (np.take_along_axis(d['valids'], act.T, 1) == 1).all()
    pol_on_valid = d['policy'] * d['valids']
    assert (pol_on_valid.sum(1) > 0).all() and ((d['policy'] == 0) & (d['valids'] == 1)).any(), 'exact zeros on valid moves'
    if gid == 6:
        nv = d['valids'].sum(1)
        assert nv[0] > 320 and nv[1] > 64, 'several chunks of the move list carry options'


# ------------------------------------------------------------------------------------------------------------- the seat's temperature
@pytest.mark.parametrize('game', ['connect4', 'hnefatafl'])
def test_seat_temp_table_is_the_players_own_loop(game):
    """NNPlayer.play :73 steps self.temp only on the player's OWN moves: a literal two-player game loop against the table"""
    import importlib
    from alphazero_general_amd.utils import default_temp_scaling, seat_temp_table
    Game = importlib.import_module('alphazero_general_amd.envs.' + game).Game
    mt, P = Game.max_turns(), Game.num_players()
    assert mt == dict(connect4=42, hnefatafl=512)[game]
    for start in (1.0, 0.8):
        tab = seat_temp_table(default_temp_scaling, start, mt, P)
        assert tab.shape == (P, mt + 2) and tab.dtype == np.float32
        temps = [start] * P                                              # one player object per seat, each with its own self.temp
        for turn in range(mt + 2):
            mover = turn % P
            temps[mover] = default_temp_scaling(temps[mover], turn, mt)
            assert tab[mover, turn] == np.float32(temps[mover]), (start, turn)
        assert tab.min() >= np.float32(0.2) and tab[:, -1].min() < start  # the schedule did step (connect4: on odd turns only)
    # (the self-play table steps on EVERY turn: the two differ, which is why a policy seat has its own)
    from alphazero_general_amd.utils import temp_table
    assert not np.array_equal(temp_table(default_temp_scaling, 1.0, mt), seat_temp_table(default_temp_scaling, 1.0, mt, P)[0])


def test_seat_values_pickle():
    import pickle
    from alphazero_general_amd.selfplay import RANDOM_SEAT, PolicySeat, is_tree_free
    assert pickle.loads(pickle.dumps(RANDOM_SEAT)) is RANDOM_SEAT and is_tree_free(RANDOM_SEAT)
    s = pickle.loads(pickle.dumps(PolicySeat(None, 0.5, None, [[1.0, 0.5], [1.0, 1.0]])))
    assert is_tree_free(s) and s.start_temp == 0.5 and s.temp_table == [[1.0, 0.5], [1.0, 1.0]]
    assert not is_tree_free(None) and not is_tree_free(object())
