"""Rules without a tree, the part that needs no GPU (include/azg.h azg_game_step / azg_game_symmetries, alphazero_general_amd/games.py):
the two symbols are declared, bound with the declared arity and exported; every precondition is decided before anything touches the
device (so it is answered on a machine without one); DeviceGames.pack / unpack carry the cells of every reference-made rule table
through the azg_state bytes and back, gobang's bitboards and hnefatafl's nibbles included."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, 'tests', 'golden')
NEW = ('azg_game_step', 'azg_game_symmetries')
FAKE = C.c_void_p(0x1000)                                     # a non-null pointer that is never followed: every call here returns first
NULL = C.c_void_p(0)


@pytest.fixture(scope='module')
def L():
    from alphazero_general_amd import build, _abi
    build.build()
    return _abi.lib()


def _declared_arity(name):
    txt = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'azg.h')).read(), flags=re.S)
    m = re.search(r'\bint\s+%s\s*\(([^;]*?)\)\s*;' % name, txt, flags=re.S)
    assert m, '%s is not declared in include/azg.h' % name
    return len([a for a in m.group(1).split(',') if a.strip()])


def test_symbols_declared_bound_and_exported(L):
    from alphazero_general_amd import _abi, build
    raw = C.CDLL(build.OUT)
    for name, arity in zip(NEW, (11, 8)):
        assert _declared_arity(name) == arity
        res, args = _abi.SYMBOLS[name]
        assert res is C.c_int and len(args) == arity, name
        assert hasattr(raw, name), 'libazg_hip.so does not export %s' % name
        assert getattr(L, name).argtypes == args
    assert L.azg_abi_version() == _abi.ABI_VERSION == 7      # additive: no ABI bump
    import alphazero_general_amd as pkg
    from alphazero_general_amd import games
    assert pkg.games is games and pkg.DeviceGames is games.DeviceGames


def _refused(L, rc, what):
    from alphazero_general_amd import _abi
    assert rc == _abi.E_INVALID_ARG, (what, rc)
    assert len(L.azg_last_error()) > 0, what


def test_step_preconditions_precede_the_device(L):
    step = L.azg_game_step
    ok = dict(stream=NULL, game=0, count=4, states=FAKE, actions=NULL, next=FAKE, valid=FAKE, win=FAKE, obs=FAKE, dtype=0, status=NULL)
    order = ('stream', 'game', 'count', 'states', 'actions', 'next', 'valid', 'win', 'obs', 'dtype', 'status')
    call = lambda **kw: step(*[dict(ok, **kw)[k] for k in order])
    _refused(L, call(states=NULL), 'null states_dev')
    _refused(L, call(count=-1), 'count < 0')
    for dt in (-1, 3, 17):
        _refused(L, call(dtype=dt), ('obs_dtype', dt))
    _refused(L, call(actions=FAKE, status=NULL), 'actions_dev without status_dev')
    for game in (-1, 7, 1000):
        _refused(L, call(game=game), ('unknown game', game))
        _refused(L, call(game=game, count=0), ('unknown game at count 0', game))
    for game in range(7):                                     # count == 0: nothing is launched, whatever else is passed
        for dt in (0, 1, 2):
            assert call(game=game, count=0, dtype=dt) == 0, (game, dt)
        assert call(game=game, count=0, actions=FAKE, status=FAKE) == 0, game
        assert call(game=game, count=0, next=NULL, valid=NULL, win=NULL, obs=NULL) == 0, game
    _refused(L, call(count=0, states=NULL), 'null states_dev at count 0')


def test_symmetries_preconditions_precede_the_device(L):
    sym = L.azg_game_symmetries
    ok = dict(stream=NULL, game=1, count=4, states=FAKE, pi=NULL, sym_states=FAKE, sym_obs=FAKE, sym_pi=NULL)
    order = ('stream', 'game', 'count', 'states', 'pi', 'sym_states', 'sym_obs', 'sym_pi')
    call = lambda **kw: sym(*[dict(ok, **kw)[k] for k in order])
    _refused(L, call(states=NULL), 'null states_dev')
    _refused(L, call(count=-5), 'count < 0')
    _refused(L, call(pi=FAKE, sym_pi=NULL), 'pi_dev without sym_pi_dev')
    _refused(L, call(pi=NULL, sym_pi=FAKE), 'sym_pi_dev without pi_dev')
    for game in (-1, 7):
        _refused(L, call(game=game), ('unknown game', game))
    for game in range(7):
        assert call(game=game, count=0) == 0, game
        assert call(game=game, count=0, pi=FAKE, sym_pi=FAKE, sym_states=NULL, sym_obs=NULL) == 0, game


def _envs():
    from alphazero_general_amd.envs import brandubh, connect4, gobang, hnefatafl, othello, tictactoe, trimok
    return [connect4.Game, brandubh.Game, trimok.Game, othello.Game, gobang.Game, tictactoe.Game, hnefatafl.Game]


def _table_states(gid):
    """(cells as Python callers hold them, player, turns, aux0) of every record of the game's rule tables"""
    from alphazero_general_amd import _abi
    out = []
    for name in {0: ('c4_rules', 'c4_rules_edge'), 1: ('br_rules', 'br_rules_edge'), 3: ('ot_rules',), 4: ('gb_rules',), 5: ('tt_rules',),
                 6: ('hn_rules',)}.get(gid, ()):
        d = dict(np.load(os.path.join(G, name + '.npz')))
        n = len(d['cells'])
        player = d['player'] if 'player' in d else d['lens'] % 2
        turns = d['turns'] if 'turns' in d else d['lens']
        aux = d['kc'] if 'kc' in d else d['aux0'] if 'aux0' in d else np.zeros(n, np.int8)
        cells = [_abi.gobang_unpack(c.tobytes()) for c in d['cells']] if gid == 4 else d['cells']
        out += [(np.asarray(cells[i], np.int8), int(player[i]), int(turns[i]), int(aux[i])) for i in range(n)]
    return out


@pytest.mark.parametrize('gid', range(7))
def test_pack_unpack_round_trip(L, gid):
    import torch
    from alphazero_general_amd import _abi
    from alphazero_general_amd.games import DeviceGames, STATE_BYTES
    Game = _envs()[gid]
    dg = DeviceGames(Game, device='cpu')
    assert dg.game == gid and (dg.A, dg.P) == (Game.action_size(), Game.num_players()) and dg.obs_shape == tuple(Game.observation_size())
    states = _table_states(gid)
    if gid == 2:                                              # the 3-player env has no table: positions of a seeded host playout
        rng, g = np.random.RandomState(5), Game()
        while not g.win_state().any():
            states.append(g.to_azg_state() + (0,))
            g.play_action(int(rng.choice(np.flatnonzero(g.valid_moves()))))
        states.append(g.to_azg_state() + (0,))
    assert len(states) >= 9
    states = states[::max(1, len(states) // 1500)]            # (a stride through the tables: every kind of record, a second of work)
    t = dg.pack(states)
    assert t.dtype == torch.uint8 and tuple(t.shape) == (len(states), STATE_BYTES) and t.device.type == 'cpu' and t.is_contiguous()
    back = dg.unpack(t)
    assert len(back) == len(states)
    for (c0, p0, t0, a0), (c1, p1, t1, a1) in zip(states, back):
        assert c1.dtype == np.int8 and c1.shape == (dg.cells,) and (c0 == c1).all() and (p0, t0, a0) == (p1, t1, a1)
    # the bytes are the azg_state of include/azg.h: the cells as _abi.cells_to_state packs them, then player, turns, aux as int32
    raw = t.numpy()
    for i in (0, len(states) // 2, len(states) - 1):
        c = np.ascontiguousarray(_abi.cells_to_state(gid, states[i][0])).view(np.uint8)
        assert (raw[i, :c.size] == c).all() and (raw[i, c.size:64] == 0).all()
        assert raw[i, 64:].view('<i4').tolist() == [states[i][1], states[i][2], states[i][3], 0]
    # objects go through MCTS.encode_state and come back through MCTS.decode_state as the same positions
    objs = dg.to_games(t[:16])
    assert all(type(o) is Game for o in objs)
    assert torch.equal(dg.pack(objs), t[:16])
    assert torch.equal(dg.initial(3), dg.pack([Game(), Game(), Game()]))
    if gid == 4:                                              # gobang's table holds the packed bitboards themselves
        d = np.load(os.path.join(G, 'gb_rules.npz'))
        idx = np.arange(0, len(d['cells']), max(1, len(d['cells']) // 1500))
        assert (raw[:, :64] == d['cells'][idx]).all()


def test_rules_need_a_device(L):
    from alphazero_general_amd.games import DeviceGames
    dg = DeviceGames(_envs()[0], device='cpu')
    with pytest.raises(AssertionError):                       # no CPU path for the rules themselves: CPU tensors are refused
        dg.step(dg.initial(2))
    with pytest.raises(AssertionError):
        dg.symmetries(dg.initial(2))
