"""Hnefatafl without a GPU: the host rules of envs/hnefatafl.py against what the reference produced (tests/golden/hn_rules.npz: random and
king-hunting playouts, built boards in all eight symmetries) at every position -- valid moves, win state, observation, the position after
the move played, symmetries -- the fixture's coverage floors, the hn_agent samples replayed through the host env, the two-cells-per-byte
packing of azg_state, the ABI's game table and launch answer for game id 6, the temperature table and, where the reference checkout is
present, the mapping of the reference's own class."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, 'golden')
REF = '/root/reference'
HN, A, N = 6, 2420, 11
RULE_FLOORS = dict(positions=10000, wins_0=20, wins_1=20, draws=20, band_1_64=50, band_65_128=50, band_129_192=50, band_over_192=50)
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, 'alphazero')), reason='needs the reference checkout (build container only)')


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


def _game():
    from alphazero_general_amd.envs.hnefatafl import Game
    return Game


def _at(Game, d, i):
    return Game.from_azg_state(d['cells'][i], int(d['player'][i]), int(d['turns'][i]), int(d['aux0'][i]))


@pytest.fixture(scope='module')
def rules():
    return dict(np.load(os.path.join(G, 'hn_rules.npz')))


# ------------------------------------------------------------------------------------------------------------------------- rules
def test_host_rules_vs_reference_at_every_position(rules):
    Game, d = _game(), rules
    n, n_play = len(d['player']), int(d['n_play'])
    names = [str(x) for x in d['kind_names']]
    moves = 0
    for i in range(n):
        g = _at(Game, d, i)
        v = g.valid_moves()
        assert v.dtype == np.uint8 and v.shape == (A,) and int(v.sum()) == d['nvalid'][i] and crc(v) == d['valid_crc'][i], ('valid_moves', i, names[d['kind'][i]])
        w = g.win_state()
        assert w.dtype == np.uint8 and (w == d['ws'][i]).all(), ('win_state', i, names[d['kind'][i]])
        o = g.observation()
        assert o.shape == (5, N, N) and o.dtype == np.float32 and crc(o) == d['obs_crc'][i], ('observation', i)
        if d['next'][i] >= 0:
            assert v[d['next'][i]] == 1
            g.play_action(int(d['next'][i]))
            c, p, t, kc = g.to_azg_state()
            assert (c == d['cells'][i + 1]).all() and p == d['player'][i + 1] and t == d['turns'][i + 1] and kc == d['aux0'][i + 1], \
                ('play_action', i, names[d['kind'][i]])
            moves += 1
    assert moves > n_play - 200
    # what the built boards are there to show (the reference decided; the names say what was built)
    first = {nm: int(np.flatnonzero(d['kind'] == k)[0]) for k, nm in enumerate(names) if (d['kind'] == k).any()}
    for nm in ('kingcap_edge_3', 'kingcap_throne_3', 'kingcap_corner_2', 'kingcap_open_4'):
        assert d['ws'][first[nm]].tolist() == [1, 0, 0], nm
    assert not d['ws'][first['kingcap_open_3_not']].any()
    i = first['king_not_two_sided']
    assert not d['ws'][i + 1].any() and d['aux0'][i + 1] == 0 and (np.isin(d['cells'][i + 1], (3, 7, 8))).sum() == 1
    i = first['surround_with_king']
    assert d['aux0'][i + 1] == 1 and d['ws'][i + 1].tolist() == [1, 0, 0] and (d['cells'][i + 1] == 1).sum() < (d['cells'][i] == 1).sum()
    i = first['custodian_black']
    assert (d['cells'][i + 1] == 1).sum() == (d['cells'][i] == 1).sum() - 1
    assert d['ws'][first['black_no_moves']].tolist() == [0, 1, 0] and d['nvalid'][first['black_no_moves']] == 0
    assert d['ws'][first['white_no_moves']].tolist() == [1, 0, 0]
    assert d['ws'][first['king_on_escape']].tolist() == [0, 1, 0]
    i = first['turn_512_king_on_corner']
    assert d['turns'][i] == 512 and d['ws'][i].tolist() == [0, 0, 1] and (d['cells'][i] == 8).any()
    assert d['max_moves'] == d['nvalid'][first['max_moves']] > 256
    # every built board comes in its eight symmetries; one instance of a capture lands on cell 63, one on cell 64 (the two mask words)
    built = d['kind'] >= 2
    dst = []
    for i in np.flatnonzero(built & (d['next'] >= 0)):
        from alphazero_general_amd.envs.hnefatafl import get_move
        (_, _), (nx, ny) = get_move(int(d['next'][i]))
        dst.append(nx + N * ny)
    assert {63, 64} <= set(dst) and {c // N for c in dst} >= {5, 6}


def test_fixture_coverage_floors(rules):
    d = rules
    n_play = int(d['n_play'])
    cov = dict(zip([str(x) for x in d['coverage_names']], d['coverage'].tolist()))
    ws, k, nxt = d['ws'][:n_play], d['nvalid'][:n_play], d['next'][:n_play]
    term = nxt < 0
    mine = dict(positions=n_play, wins_0=int((ws[:, 0] == 1).sum()), wins_1=int((ws[:, 1] == 1).sum()), draws=int((ws[:, 2] == 1).sum()),
                band_1_64=int(((k >= 1) & (k <= 64)).sum()), band_65_128=int(((k > 64) & (k <= 128)).sum()),
                band_129_192=int(((k > 128) & (k <= 192)).sum()), band_over_192=int((k > 192).sum()))
    assert mine == cov
    for name, floor in RULE_FLOORS.items():
        assert mine[name] >= floor, name
    assert (ws.any(axis=1) == term).all()                                    # a playout stops at its first decided position
    assert (d['turns'][:n_play][ws[:, 2] == 1] == 512).all() and set(d['kind'][:n_play].tolist()) == {0, 1}
    assert k.max() <= 448 and d['nvalid'].max() <= 448


def test_host_symmetries_vs_reference(rules):
    Game, d = _game(), rules
    assert len(d['sym_index']) >= 32
    for j, i in enumerate(d['sym_index']):
        g = _at(Game, d, i)
        pi = (np.arange(A, dtype=np.float32) + 1) * g.valid_moves().astype(np.float32)
        syms = g.symmetries(pi)
        assert len(syms) == 8
        for k, (gs, p) in enumerate(syms):
            assert (gs.to_azg_state()[0] == d['sym_cells'][j, k]).all() and crc(np.asarray(p, np.float32)) == d['sym_pi_crc'][j, k], (i, k)
            assert gs.player == g.player and gs.turns == g.turns
        assert (syms[6][0].to_azg_state()[0] == d['cells'][i]).all() and (syms[6][1] == pi).all()      # SYM_RAW = 6: the identity


def test_start_position_and_protocol():
    Game = _game()
    g = Game()
    rows = [''.join(str(v) for v in r) for r in g._board._state]
    assert rows[0] == '50022222005' and rows[1] == '00000200000' and rows[3] == '20000100002' and rows[5] == '22011711022'
    assert rows == rows[::-1] and all(r == r[::-1] for r in rows)
    assert Game.AZG_GAME_ID == HN and Game.action_size() == A and Game.observation_size() == (5, N, N) and Game.num_players() == 2
    assert Game.has_draw() is True and Game.max_turns() == 512 and int(g.valid_moves().sum()) == 116 and g.player == 0
    assert g == g.clone() and g._board.to_play() == 2


# ------------------------------------------------------------------------------------------------------------------------- samples
@pytest.mark.parametrize('cname,symmetric', [('plain', False), ('symmetric', True), ('fastmix', False), ('warmup', True), ('long', False)])
def test_agent_samples_replayed_on_the_host_env(cname, symmetric):
    """every hn_agent config: what the reference's agent searched and played (the non-zero visit counts and the moves of every round)
    replayed through SelfPlayAgent.playMoves restated on the host env (tests/sample_replay.py) gives the reference's samples, results and
    games_played -- so the fixture's samples are also the host env's own, symmetries included"""
    import sample_replay as sr
    d = dict(np.load(os.path.join(G, 'hn_agent.npz')))
    B, games = int(d[cname + '_B']), int(d[cname + '_games'])
    ca, cn = d[cname + '_counts_a'], d[cname + '_counts_n']
    R = len(ca)
    counts = np.zeros((R, B, A), np.int32)
    for r in range(R):
        for i in range(B):
            k = ca[r, i] >= 0
            counts[r, i, ca[r, i][k]] = cn[r, i][k]
    assert (np.array([[crc(counts[r, i]) for i in range(B)] for r in range(R)], np.uint32) == d[cname + '_counts_crc']).all()
    out = sr.replay(_game(), B, games, symmetric, counts, d[cname + '_actions'], fast=d[cname + '_fast'])
    n = len(d[cname + '_s_z'])
    assert len(out['s_z']) == n and (out['s_z'] == d[cname + '_s_z']).all()
    assert (np.array([crc(o) for o in out['s_obs']], np.uint32) == d[cname + '_s_obs_crc']).all()
    assert (np.array([crc(p) for p in out['s_pi']], np.uint32) == d[cname + '_s_pi_crc']).all()
    assert ((out['s_pi'] != 0).sum(axis=1) == d[cname + '_s_pi_nnz']).all()
    assert (out['r_ws'] == d[cname + '_r_ws']).all() and (out['r_turns'] == d[cname + '_r_turns']).all()
    assert (out['games_played'] == d[cname + '_games_played']).all()
    if cname == 'long':
        assert 512 in out['r_turns'].tolist() and n > 513                     # a 512-entry history, emitted whole


# ------------------------------------------------------------------------------------------------------------------------- ABI
def test_pack_unpack_round_trip(rules):
    from alphazero_general_amd import _abi
    d = rules
    rng = np.random.RandomState(5)
    boards = [d['cells'][i] for i in rng.choice(len(d['cells']), 200, replace=False)] + [rng.randint(0, 9, 121).astype(np.int8) for _ in range(50)]
    for c in boards:
        raw = _abi.hnefatafl_pack(c)
        assert raw.dtype == np.int8 and raw.shape == (64,) and (raw[61:] == 0).all()
        u = raw.view(np.uint8)
        for cell in (0, 1, 62, 63, 64, 65, 119, 120):
            assert (u[cell // 2] >> (4 * (cell & 1))) & 15 == c[cell]
        assert u[60] >> 4 == 0
        assert (_abi.hnefatafl_unpack(raw.tobytes()) == c).all()
        assert (_abi.cells_to_state(HN, c) == raw).all()
    s = _abi.State()
    for i, v in enumerate(_abi.hnefatafl_pack(boards[0])):
        s.cells[i] = int(v)
    assert (_abi.state_cells(s, HN, 121) == boards[0]).all()


def test_abi_game_table_and_launch_answer():
    from alphazero_general_amd import _abi
    assert _abi.GAME_HNEFATAFL == HN and _abi.lib().azg_abi_version() == _abi.ABI_VERSION == 7
    gi = _abi.game_info(HN)
    assert (gi.action_size, gi.obs_c, gi.obs_h, gi.obs_w, gi.num_players, gi.has_draw, gi.max_turns, gi.num_symmetries, gi.cells,
            gi.max_children) == (2420, 5, 11, 11, 2, 1, 512, 8, 121, 448)
    L = _abi.lib()
    for ch in (32, 64, 128):
        assert L.azg_launch_support(HN, ch) == _abi.E_INVALID_ARG and _abi.launch_support(HN, ch) == 0
    assert L.azg_launch_support(7, 32) == _abi.E_INVALID_ARG
    # the proven bound on the move list: n movers make at most min(20 n, 4 (121 - n)) moves
    assert max(min(20 * n, 4 * (121 - n)) for n in range(122)) == 400 <= 403 <= gi.max_children     # (403.3 where the two lines cross)


def test_temperature_table_halves_every_76_turns():
    from alphazero_general_amd.Game import UNBOUNDED_TURNS, schedule_turns
    from alphazero_general_amd.utils import default_temp_scaling, temp_table
    Game = _game()
    assert schedule_turns(Game) == 512 and HN not in UNBOUNDED_TURNS and int(0.15 * 512) == 76
    tt = temp_table(default_temp_scaling, 1.0, Game.max_turns(), schedule_turns(Game))
    assert tt.dtype == np.float32 and len(tt) == 514
    t, want = 1.0, []
    for turn in range(514):
        t = default_temp_scaling(t, turn, 512)
        want.append(t)
    assert tt.tobytes() == np.asarray(want, np.float32).tobytes()
    steps = [i for i in range(1, 514) if tt[i] != tt[i - 1]]
    assert steps == [75, 151, 227] and all((s + 1) % 76 == 0 for s in steps)          # (the move made at turn 75 is the 76th)
    assert tt[74] == 1.0 and tt[75] == 0.5 and tt[151] == 0.25 and tt[227] == np.float32(0.2)
    assert tt.min() == np.float32(0.2) == tt[-1]


def test_package_registration():
    from alphazero_general_amd import coach
    from alphazero_general_amd.Game import _REFERENCE_ENVS, azg_game_id, has_device_rules
    Game = _game()
    assert azg_game_id(Game) == HN and coach._ours(Game) is Game and has_device_rules(Game)
    assert _REFERENCE_ENVS['envs.hnefatafl.fastafl'] == HN


@needs_reference
def test_reference_class_maps_to_the_device_game():
    """the reference's own alphazero.envs.hnefatafl.fastafl.Game is recognised as game 6, and encode_state / decode_state carry its board,
    turn count and king-captured flag both ways, move for move against the host env (in a child process: importing the reference here
    would leave it in sys.modules for the modules that run later)"""
    code = 'import sys; sys.path.insert(0, %r); import test_hnefatafl_cpu as t; t.reference_objects_check()' % HERE
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=900, env=env, cwd=os.path.dirname(HERE))
    assert r.returncode == 0, r.stderr[-3000:]


def reference_objects_check():
    sys.path.insert(0, G)
    sys.path.insert(0, os.path.dirname(HERE))
    import refharness as rh
    rh.import_reference()
    from alphazero.envs.hnefatafl.fastafl import Game as RefGame
    from alphazero_general_amd.Game import azg_game_id
    from alphazero_general_amd.MCTS import decode_state, encode_state
    Game, d = _game(), dict(np.load(os.path.join(G, 'hn_rules.npz')))
    assert azg_game_id(RefGame) == HN and azg_game_id(RefGame()) == HN
    ref, ours = RefGame(), Game()
    for a in d['next'][:60]:                                                  # the first playout of the fixture, move for move
        st = encode_state(ref)
        mine = ours.to_azg_state()
        assert (st[0] == mine[0]).all() and tuple(st[1:]) == tuple(mine[1:])
        back = decode_state(ref, *st)
        assert type(back) is RefGame and (np.asarray(back.valid_moves()) == ours.valid_moves()).all()
        assert (np.asarray(back.win_state()) == ours.win_state()).all() and back.player == ours.player and back.turns == ours.turns
        if a < 0:
            break
        ref.play_action(int(a)); ours.play_action(int(a))


@needs_reference
def test_fixtures_regenerate_bit_for_bit(tmp_path):
    """make_hnefatafl_goldens.py, run on the reference again into a temporary directory, writes the committed fixtures array for array"""
    code = ('import sys; sys.path.insert(0, %r); import make_hnefatafl_goldens as m; m.main(out_dir=%r, verbose=False)') % (G, str(tmp_path))
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=1800, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    for n in ('hn_rules', 'hn_tree', 'hn_edge', 'hn_agent'):
        new, old = np.load(os.path.join(str(tmp_path), n + '.npz')), np.load(os.path.join(G, n + '.npz'))
        assert sorted(new.files) == sorted(old.files), n
        for k in old.files:
            a, b = new[k], old[k]
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (n, k)
        assert os.path.getsize(os.path.join(G, n + '.npz')) <= 393524            # no larger than the largest fixture committed before (gb_edge.npz)
