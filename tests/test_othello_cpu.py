"""Othello without a GPU: the host rules of envs/othello.py against the reference's own rule table (tests/golden/ot_rules.npz: random
playouts of alphazero/envs/othello with every terminal kind covered, the 8 symmetries of a subset), the ABI's game table and tower
layouts for game id 3, and -- where the reference checkout is present -- the fixtures regenerated array for array and the hand-over of the
reference's own othello.Game objects to the device encoding."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, 'golden')
REF = '/root/reference'
FIXTURES = ('ot_rules', 'ot_tree', 'ot_agent', 'ot_mt19937_agent')


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


def _game():
    from alphazero_general_amd.envs.othello import Game
    return Game


def test_host_rules_vs_reference_table():
    Game = _game()
    d = dict(np.load(os.path.join(G, 'ot_rules.npz')))
    n = len(d['lens'])
    cov = dict(zip([str(x) for x in d['coverage_names']], d['coverage'].tolist()))
    assert n >= 10000 and cov['positions'] == n
    assert cov['mover_wins'] >= 20 and cov['other_wins'] >= 20 and cov['draws'] >= 3 and cov['early_end'] >= 40
    g = None
    for i in range(n):
        if d['lens'][i] == 0:
            g = Game()
            assert (g.to_azg_state()[0] == d['cells'][i]).all()
        assert (g._board.pieces.reshape(-1) == d['cells'][i]).all() and g.player == d['player'][i] and g.turns == d['turns'][i], i
        assert (g.valid_moves() == d['valids'][i]).all(), i
        assert (g.win_state() == d['ws'][i]).all(), i
        assert crc(g.observation()) == d['obs_crc'][i], i
        if d['next'][i] >= 0:
            g.play_action(int(d['next'][i]))


def test_host_symmetries_vs_reference_table():
    Game = _game()
    d = dict(np.load(os.path.join(G, 'ot_rules.npz')))
    for j, i in enumerate(d['sym_index']):
        g = Game.from_azg_state(d['cells'][i], d['player'][i], d['turns'][i])
        syms = g.symmetries(np.arange(64, dtype=np.float32))
        assert len(syms) == 8
        for k, (gs, pi) in enumerate(syms):
            assert (gs._board.pieces.reshape(-1) == d['sym_cells'][j, k]).all(), (i, k)
            assert (np.asarray(pi) == d['sym_pi'][j, k]).all(), (i, k)
    assert (d['sym_pi'][:, 7] == np.arange(64)).all()                 # the identity is the last entry


def test_abi_game_table_and_tower_layouts():
    import ctypes as C
    from alphazero_general_amd import _abi
    assert _abi.GAME_OTHELLO == 3 and _abi.lib().azg_abi_version() == _abi.ABI_VERSION == 7
    gi = _abi.game_info(_abi.GAME_OTHELLO)
    assert (gi.action_size, gi.obs_c, gi.obs_h, gi.obs_w, gi.num_players, gi.has_draw, gi.max_turns, gi.num_symmetries, gi.cells,
            gi.max_children) == (64, 1, 8, 8, 2, 1, 64, 8, 64, 60)
    L = _abi.lib()
    for bt, ch in ((1, 32), (2, 32), (4, 32), (1, 64), (2, 64), (3, 64), (4, 64)):
        pix = (C.c_int16 * (bt * 64))()
        info = (C.c_int32 * 8)()
        assert L.azg_tower_layout(3, bt, ch, pix, None, info) == 0, (bt, ch)
        assert info[0] == 4 * bt                                       # four 16-pixel subtiles per board: no pad rows
        assert sorted(pix) == list(range(bt * 64)), (bt, ch)


def test_package_registration():
    from alphazero_general_amd import coach, nnet
    from alphazero_general_amd.Game import azg_game_id
    Game = _game()
    assert azg_game_id(Game) == 3 and coach._ours(Game) is Game
    a = nnet.OTHELLO_NET_ARGS
    assert (a.num_channels, a.depth, a.value_head_channels, a.policy_head_channels) == (64, 4, 16, 16)


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, 'alphazero')), reason='needs the reference checkout (build container only)')
def test_fixtures_regenerate_identically(tmp_path):
    """make_othello_goldens.py, run on the reference again into a temporary directory, writes the committed fixtures array for array"""
    code = ('import sys; sys.path.insert(0, %r); import make_othello_goldens as m; m.main(out_dir=%r, verbose=False)') % (G, str(tmp_path))
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=1800, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    for n in FIXTURES:
        new, old = np.load(os.path.join(str(tmp_path), n + '.npz')), np.load(os.path.join(G, n + '.npz'))
        assert sorted(new.files) == sorted(old.files), n
        for k in old.files:
            a, b = new[k], old[k]
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (n, k)


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, 'alphazero')), reason='needs the reference checkout (build container only)')
def test_reference_objects_encode_and_decode():
    """the reference's own othello.Game objects: azg_game_id maps them to 3, encode_state / decode_state round-trip them"""
    sys.path.insert(0, G)
    import refharness as rh
    rh.import_reference()
    from alphazero.envs.othello.othello import Game as RefGame
    from alphazero_general_amd.Game import azg_game_id
    from alphazero_general_amd.MCTS import decode_state, encode_state
    Ours = _game()
    assert azg_game_id(RefGame) == 3
    rng = np.random.RandomState(5)
    for _ in range(20):
        g, o = RefGame(), Ours()
        for _ in range(rng.randint(0, 50)):
            if np.asarray(g.win_state()).any():
                break
            a = int(rng.choice(np.flatnonzero(np.asarray(g.valid_moves()))))
            g.play_action(a); o.play_action(a)
        cells, player, turns = encode_state(g)
        assert (cells == o.to_azg_state()[0]).all() and player == o.player and turns == o.turns
        back = decode_state(g, cells, player, turns)
        assert type(back) is type(g) and (np.asarray(back._board.pieces) == np.asarray(g._board.pieces)).all()
        assert back.player == g.player and back.turns == g.turns
        assert (np.asarray(back.valid_moves()) == np.asarray(g.valid_moves())).all()
