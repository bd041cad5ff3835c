"""Gobang without a GPU: the host rules of envs/gobang.py against the reference's own rule table (tests/golden/gb_rules.npz: random
playouts of alphazero/envs/gobang plus hand-built boards -- overlines, fives on every edge and corner, full-board draws, both colours
holding a five, runs of four that must not count -- and the 8 symmetries of a subset), the packed azg_state layout, the ABI's game table
and tower layouts for game id 4, and -- where the reference checkout is present -- the fixtures regenerated array for array and the
hand-over of the reference's own gobang.Game objects to the device encoding."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, 'golden')
REF = '/root/reference'
FIXTURES = ('gb_rules', 'gb_tree', 'gb_noise_tree', 'gb_agent')


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


def _game():
    from alphazero_general_amd.envs.gobang import Game
    return Game


def _rules():
    from alphazero_general_amd import _abi
    d = dict(np.load(os.path.join(G, 'gb_rules.npz')))
    d['board'] = np.array([_abi.gobang_unpack(c.tobytes()) for c in d['cells']])
    return d


def _check_position(g, d, i):
    assert (g.valid_moves().astype(np.uint8) == g.valid_moves()).all()
    assert crc(g.valid_moves().astype(np.uint8)) == d['valid_crc'][i], i
    assert (g.win_state() == d['ws'][i]).all(), i
    assert crc(g.observation()) == d['obs_crc'][i], i


def test_host_rules_vs_reference_table():
    Game = _game()
    d = _rules()
    n = len(d['lens'])
    cov = dict(zip([str(x) for x in d['coverage_names']], d['coverage'].tolist()))
    assert cov['positions'] >= 10000 and cov['wins_0'] >= 20 and cov['wins_1'] >= 20
    assert cov['built'] >= 250 and cov['built_draws'] >= 4 and cov['built_both'] >= 8 and cov['built_overlines'] >= 8 and cov['built_short'] >= 40
    assert (d['lens'] >= 0).sum() == cov['positions'] and (d['lens'] < 0).sum() == cov['built']
    g = None
    for i in range(n):
        if d['lens'][i] < 0:                                  # a hand-built board, loaded as it is
            g = Game.from_azg_state(d['board'][i], d['player'][i], d['turns'][i])
        elif d['lens'][i] == 0:
            g = Game()
            assert (g.to_azg_state()[0] == d['board'][i]).all()
        assert (g._board.pieces.reshape(-1) == d['board'][i]).all() and g.player == d['player'][i] and g.turns == d['turns'][i], i
        _check_position(g, d, i)
        if d['next'][i] >= 0:
            g.play_action(int(d['next'][i]))


def test_built_boards_cover_the_scan_order():
    """both colours holding a five: the fixture has wins for either colour, and the reference's answer is the colour whose run starts
    first in [x][y] order -- the order struct GB uses (lowest start bit)"""
    from alphazero_general_amd.envs.gobang import Board
    d = _rules()
    both = np.flatnonzero(d['kind'] == 4)
    assert len(both) >= 8
    winners = set()
    for i in both:
        b = Board(d['board'][i].reshape(15, 15))
        first = next(b.five_at(x, y) for x in range(15) for y in range(15) if b.five_at(x, y))
        w = d['ws'][i]
        assert w[0 if first == 1 else 1] == 1 and w.sum() == 1, i
        winners.add(int(first))
    assert winners == {1, -1}


def test_host_symmetries_vs_reference_table():
    from alphazero_general_amd import _abi
    Game = _game()
    d = _rules()
    for j, i in enumerate(d['sym_index']):
        g = Game.from_azg_state(d['board'][i], d['player'][i], d['turns'][i])
        syms = g.symmetries(np.arange(225, dtype=np.float32))
        assert len(syms) == 8
        for k, (gs, pi) in enumerate(syms):
            assert (_abi.gobang_pack(gs._board.pieces.reshape(-1)).view(np.uint8) == d['sym_cells'][j, k]).all(), (i, k)
            assert (np.asarray(pi) == d['sym_pi'][j, k]).all(), (i, k)
            assert gs.player == g.player and gs.turns == g.turns
    assert (d['sym_pi'][:, 7] == np.arange(225)).all()                # the identity is the last entry


def test_packed_state_layout():
    """include/azg.h: colour 1's board in bytes 0..31, colour -1's in 32..63, bit 16x + y of four little-endian words"""
    from alphazero_general_amd import _abi
    rng = np.random.RandomState(3)
    for _ in range(50):
        cells = rng.choice([-1, 0, 1], 225).astype(np.int8)
        raw = _abi.gobang_pack(cells)
        assert raw.dtype == np.int8 and raw.shape == (64,)
        words = raw.view(np.uint8).view('<u8')
        for colour, base in ((1, 0), (-1, 4)):
            for i in range(225):
                x, y = divmod(i, 15)
                p = 16 * x + y
                assert ((int(words[base + p // 64]) >> (p % 64)) & 1) == (cells[i] == colour)
            pad = [16 * x + 15 for x in range(15)] + list(range(240, 256))
            assert all(((int(words[base + p // 64]) >> (p % 64)) & 1) == 0 for p in pad)
        assert (_abi.gobang_unpack(raw.tobytes()) == cells).all()
    # the engine's conversion: a python board in, the same board out, for gobang only
    st = _abi.states_array(1)[0]
    c = _abi.cells_to_state(_abi.GAME_GOBANG, cells)
    for i, v in enumerate(c):
        st.cells[i] = int(v)
    assert (_abi.state_cells(st, _abi.GAME_GOBANG, 225) == cells).all()
    assert (_abi.cells_to_state(_abi.GAME_OTHELLO, np.arange(64)) == np.arange(64)).all()


def test_abi_game_table_and_tower_layouts():
    import ctypes as C
    from alphazero_general_amd import _abi
    assert _abi.GAME_GOBANG == 4 and _abi.lib().azg_abi_version() == _abi.ABI_VERSION == 7
    gi = _abi.game_info(_abi.GAME_GOBANG)
    assert (gi.action_size, gi.obs_c, gi.obs_h, gi.obs_w, gi.num_players, gi.has_draw, gi.max_turns, gi.num_symmetries, gi.cells,
            gi.max_children) == (225, 4, 15, 15, 2, 1, 225, 8, 225, 225)
    L = _abi.lib()
    for bt, ch in ((1, 32), (1, 64), (1, 128)):
        info = (C.c_int32 * 8)()
        pix = (C.c_int16 * (16 * 16 * bt))()
        assert L.azg_tower_layout(4, bt, ch, pix, None, info) == 0, (bt, ch)
        assert info[0] == 15 * bt                                      # 15 pixel subtiles per board, 15 spare lanes
        p = list(pix)[:info[0] * 16]
        assert sorted(x for x in p if x >= 0) == list(range(225 * bt)) and p.count(-1) == 16 * info[0] - 225 * bt, (bt, ch)
    assert L.azg_tower_layout(4, 2, 64, None, None, (C.c_int32 * 8)()) != 0      # no two-board gobang tile


def test_package_registration():
    from alphazero_general_amd import coach, nnet
    from alphazero_general_amd.Game import _REFERENCE_ENVS, azg_game_id
    Game = _game()
    assert azg_game_id(Game) == 4 and coach._ours(Game) is Game and _REFERENCE_ENVS['envs.gobang.gobang'] == 4
    a = nnet.GOBANG_NET_ARGS
    assert (a.num_channels, a.depth, a.value_head_channels, a.policy_head_channels) == (128, 8, 16, 16)
    assert list(a.value_dense_layers) == [2048, 128] and list(a.policy_dense_layers) == [2048]
    g = Game()
    assert g.observation().shape == (4, 15, 15) and g.observation().dtype == np.float32
    g.play_action(112)
    with pytest.raises(ValueError):
        g.play_action(112)


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, 'alphazero')), reason='needs the reference checkout (build container only)')
def test_fixtures_regenerate_identically(tmp_path):
    """make_gobang_goldens.py, run on the reference again into a temporary directory, writes the committed fixtures array for array"""
    code = ('import sys; sys.path.insert(0, %r); import make_gobang_goldens as m; m.main(out_dir=%r, verbose=False)') % (G, str(tmp_path))
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
    """the reference's own gobang.Game objects: azg_game_id maps them to 4, encode_state / decode_state round-trip them (in a child
    process: importing the reference here would leave it in sys.modules for the modules that run later)"""
    code = 'import sys; sys.path.insert(0, %r); import test_gobang_cpu as t; t.reference_objects_check()' % HERE
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=900, env=env, cwd=os.path.dirname(HERE))
    assert r.returncode == 0, r.stderr[-3000:]


def reference_objects_check():
    sys.path.insert(0, G)
    import refharness as rh
    rh.import_reference()
    from alphazero.envs.gobang.gobang import Game as RefGame
    from alphazero_general_amd.Game import azg_game_id
    from alphazero_general_amd.MCTS import decode_state, encode_state
    Ours = _game()
    assert azg_game_id(RefGame) == 4
    rng = np.random.RandomState(5)
    for _ in range(20):
        g, o = RefGame(), Ours()
        for _ in range(rng.randint(0, 80)):
            if np.asarray(g.win_state()).any():
                break
            a = int(rng.choice(np.flatnonzero(np.asarray(g.valid_moves()))))
            g.play_action(a); o.play_action(a)
        cells, player, turns = encode_state(g)
        assert (cells == o.to_azg_state()[0]).all() and player == o.player and turns == o.turns
        assert (np.asarray(g.win_state()) == o.win_state()).all() and (np.asarray(g.observation()) == o.observation()).all()
        back = decode_state(g, cells, player, turns)
        assert type(back) is type(g) and (np.asarray(back._board.pieces) == np.asarray(g._board.pieces)).all()
        assert back.player == g.player and back.turns == g.turns
        assert (np.asarray(back.valid_moves()) == np.asarray(g.valid_moves())).all()
