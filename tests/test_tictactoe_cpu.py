"""Tic-tac-toe without a GPU: the host rules of envs/tictactoe.py against the reference's own rule table (tests/golden/tt_rules.npz:
EXHAUSTIVE -- all 3^9 assignments of the nine cells x both movers, unreachable boards included, every legal move of every record), its
symmetries, the temperature schedule (the class has no turn limit: constant under default_temp_scaling, and the other games' tables
unchanged), the ABI's game table, launch mask and tower layouts for game id 5, the zero-padding of head channels below 16 in
HipResNet's packing, the package registration and -- where the reference checkout is present -- the fixtures regenerated array for array,
the reference's own tictactoe.Game against the host env move for move, and TICTACTOE_NET_ARGS against train.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, 'golden')
REF = '/root/reference'
TT = 5
FIXTURES = ('tt_rules', 'tt_tree', 'tt_edge', 'tt_agent', 'tt_mt19937_agent')
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, 'alphazero')), reason='needs the reference checkout (build container only)')


def _game():
    from alphazero_general_amd.envs.tictactoe import Game
    return Game


def rules():
    """tt_rules.npz with the successor records decoded: succ[r, a] = the record play_action(a) leads to from record r, -1 if illegal"""
    d = dict(np.load(os.path.join(G, 'tt_rules.npz')))
    n = len(d['player'])
    d['succ'] = np.where(d['valids'] != 0, np.arange(n, dtype=np.int64)[:, None] + d['succ_delta'], -1)
    return d


# ------------------------------------------------------------------------------------------------------------------------- rules
def test_host_rules_vs_reference_table_every_state_every_move():
    Game = _game()
    d = rules()
    n = len(d['player'])
    cov = dict(zip([str(x) for x in d['coverage_names']], d['coverage'].tolist()))
    assert n == 2 * 3 ** 9 == cov['records'] and cov['both_lines'] > 0 and cov['draws'] > 0
    idx = (d['cells'].astype(np.int64) + 1) @ (3 ** np.arange(9))
    assert (2 * idx + d['player'] == np.arange(n)).all()                     # every board, both movers, in order
    moves = 0
    for r in range(n):
        g = Game.from_azg_state(d['cells'][r], d['player'][r], d['turns'][r])
        assert (g.valid_moves() == d['valids'][r]).all() and g.valid_moves().dtype == np.uint8, r
        assert (g.win_state() == d['ws'][r]).all() and g.win_state().dtype == np.uint8, r
        o = g.observation()
        assert o.shape == (1, 3, 3) and o.dtype == np.float32 and (o.reshape(-1) == d['obs'][r]).all(), r
        for a in np.flatnonzero(d['valids'][r]):
            h = g.clone()
            h.play_action(int(a))
            s = d['succ'][r, a]
            assert (h.to_azg_state()[0] == d['cells'][s]).all() and h.player == d['player'][s] and h.turns == d['turns'][s], (r, a)
            moves += 1
    assert moves == int(d['valids'].sum()) == 2 * 3 ** 9 * 3                # a third of all cells are empty
    # on a built board where both colours hold a line the player to move wins (is_win(mover) is tested first)
    both = [r for r in range(n) if Game.from_azg_state(d['cells'][r], 0, 0)._board.is_win(1) and Game.from_azg_state(d['cells'][r], 0, 0)._board.is_win(-1)]
    assert len(both) == cov['both_lines'] and all(d['ws'][r][d['player'][r]] == 1 for r in both)
    g = Game()
    g.play_action(4)
    with pytest.raises(ValueError):
        g.play_action(4)


def test_host_symmetries_vs_reference_table():
    Game = _game()
    d = rules()
    assert (d['sym_pi'][7] == np.arange(9)).all()                            # SYM_RAW = 7: the identity is the last entry
    for j, b in enumerate(d['sym_board']):
        cells = d['cells'][2 * b + (b & 1)]
        g = Game.from_azg_state(cells, int(b & 1), int((cells != 0).sum()))
        syms = g.symmetries(np.arange(9, dtype=np.float32))
        assert len(syms) == 8
        for k, (gs, pi) in enumerate(syms):
            assert (gs.to_azg_state()[0] == d['sym_cells'][j, k]).all() and (np.asarray(pi) == d['sym_pi'][k]).all(), (b, k)
            assert gs.player == g.player and gs.turns == g.turns
    g = Game()
    g.play_action(2)
    assert hash(g) == hash(g.clone()) and g == g.clone() and not (g == Game())


# ------------------------------------------------------------------------------------------------------------------------- schedule
def test_temperature_schedule_follows_the_class():
    from alphazero_general_amd import envs  # noqa: F401
    from alphazero_general_amd.Game import UNBOUNDED_TURNS, schedule_turns
    from alphazero_general_amd.utils import default_temp_scaling, temp_table
    import importlib
    Game = _game()
    assert Game.max_turns() is None and schedule_turns(Game) == 9 and UNBOUNDED_TURNS == {TT: 9}
    # what DeviceEngine, SelfPlayAgent.py and iteration.py build for this game: constant at startTemp, one entry per turn of the longest game
    for start in (1.0, 0.7):
        tt = temp_table(default_temp_scaling, start, Game.max_turns(), schedule_turns(Game))
        assert tt.dtype == np.float32 and len(tt) == 11 and (tt == np.float32(start)).all()
    # (a max_turns of 9 as the schedule's argument would halve after every move: the trap the sizing number sets)
    assert temp_table(default_temp_scaling, 1.0, 9)[:3].tolist() == [0.5, 0.25, float(np.float32(0.2))]
    # a schedule of the caller's own still gets a table that covers every turn
    assert temp_table(lambda t, turn, mt: t * 0.5, 1.0, None, 9).tolist() == [0.5 ** (i + 1) for i in range(11)]
    # the other five games: the table is what it was (the class's max_turns() is the argument and the length)
    for name in ('connect4', 'brandubh', 'trimok', 'othello', 'gobang'):
        cls = importlib.import_module('alphazero_general_amd.envs.' + name).Game
        mt = cls.max_turns()
        assert mt and schedule_turns(cls) == mt and cls.AZG_GAME_ID not in UNBOUNDED_TURNS
        old = []
        t = 1.0
        for turn in range(max(int(mt or 0), 1) + 2):                         # (temp_table as it was before the `turns` argument)
            t = default_temp_scaling(t, turn, mt)
            old.append(t)
        assert temp_table(default_temp_scaling, 1.0, mt, schedule_turns(cls)).tobytes() == np.asarray(old, np.float32).tobytes() \
            == temp_table(default_temp_scaling, 1.0, mt).tobytes(), name


# ------------------------------------------------------------------------------------------------------------------------- ABI
def test_abi_game_table_and_launch_mask():
    from alphazero_general_amd import _abi
    assert _abi.GAME_TICTACTOE == TT and _abi.lib().azg_abi_version() == _abi.ABI_VERSION == 7
    gi = _abi.game_info(TT)
    assert (gi.action_size, gi.obs_c, gi.obs_h, gi.obs_w, gi.num_players, gi.has_draw, gi.max_turns, gi.num_symmetries, gi.cells,
            gi.max_children) == (9, 1, 3, 3, 2, 1, 9, 8, 9, 9)
    L = _abi.lib()
    # (TT, 32): stand-alone tower rows and persistent rows, exact heads only (has_sparse_heads excludes the game); no other width
    assert L.azg_launch_support(TT, 32) == _abi.SUPPORT_TOWER | _abi.SUPPORT_SEARCH_WIDE == _abi.launch_support(TT, 32)
    # (64- and 128-channel tiles are out of scope: the library refuses those widths for this game, the Python layer reads that as no launch)
    for ch in (64, 128, 96):
        assert L.azg_launch_support(TT, ch) == _abi.E_UNSUPPORTED and _abi.launch_support(TT, ch) == 0
    assert L.azg_launch_support(6, 32) == _abi.E_INVALID_ARG
    info = (C.c_int32 * 8)()
    found = {bt for bt in range(1, 33) if L.azg_tower_layout(TT, bt, 32, None, None, info) == 0}
    assert found == {1, 2, 5, 16}                                            # tower: 1, 5, 16 boards; persistent: 1 and 2 games
    assert not any(L.azg_tower_layout(TT, bt, ch, None, None, info) == 0 for bt in range(1, 33) for ch in (64, 128))


@pytest.mark.parametrize('bt', [1, 2, 5, 16])
def test_tower_layout_of_every_tile(bt):
    """the LDS image of every (TT, 32) tile: the generic invariants (tests/test_abi.py check_tower_layout: bijection, in-bounds taps, pad
    rows, strides with BSTRIDE == 2 (mod 8)), spare lanes -1, the bank rule, and the border classes -- sixteen boards are exactly nine
    subtiles without a spare lane in the five-class form (1 interior, 3 + 3 row, 1 + 1 column subtiles), five boards three subtiles in the
    three-class form"""
    import test_abi as TA
    from alphazero_general_amd import _abi
    L = _abi.lib()
    nsub, rows, tile, pm, q = TA.check_tower_layout(L, TT, bt, 32, 3, 3)
    assert rows == 9 * bt and nsub == (9 * bt + 15) // 16 and int((pm == -1).sum()) == nsub * 16 - rows and (pm >= -1).all()
    info = (C.c_int32 * 8)()
    assert L.azg_tower_layout(TT, bt, 32, None, None, info) == 0
    assert info[7] == 26 and info[5] == 5 and info[6] == 6 and info[2] == 96 and info[3] == 6 + 26 * bt
    # the bank rule: an 8-lane set reads rows of pairwise different residue mod 8 where its class has them.  On this board a class can hold
    # as few as four residues (PW = 5, BSTRIDE = 26: the interior pixel of board b sits at residue 2 b + const), so a set of eight lanes
    # takes each of them twice -- a two-way conflict at most, never three lanes on one residue
    setA, setB = (0, 1, 2, 3, 12, 13, 14, 15), (4, 5, 6, 7, 8, 9, 10, 11)
    for s in range(nsub):
        for lanes in (setA, setB):
            res = [int(q[pm[s * 16 + l]]) % 8 for l in lanes if pm[s * 16 + l] >= 0]
            assert max([res.count(r) for r in res] or [0]) <= 2, (s, sorted(res))
    counts = {16: [1, 3, 3, 1, 1], 5: [1, 1, 1]}.get(bt)
    if bt == 16:
        assert nsub == 9 and not (pm == -1).any()
    if counts:
        def pclass(p):
            y, x = divmod(p % 9, 3)
            if y == 0: return 1
            if y == 2: return 2
            if len(counts) == 3: return 0
            return 3 if x == 0 else 4 if x == 2 else 0
        first = np.cumsum([0] + counts)
        assert first[-1] == nsub
        for s in range(nsub):
            c = int(np.searchsorted(first, s, side='right') - 1)
            assert all(pclass(int(p)) == c for p in pm[s * 16:(s + 1) * 16] if p >= 0), (s, c)
        if bt == 16:                                                         # taps that remain: 9 interior + 6 x 6 row + 2 x 6 column = 57 of 81
            assert 9 * counts[0] + 6 * (counts[1] + counts[2]) + 6 * (counts[3] + counts[4]) == 57


# ------------------------------------------------------------------------------------------------------------------------- head padding
def _folded(vc, pc, seed=3):
    import torch
    from alphazero_general_amd import nnet as N
    from alphazero_general_amd.utils import dotdict
    torch.manual_seed(seed)
    a = dotdict(dict(N.TICTACTOE_NET_ARGS)); a['value_head_channels'] = vc; a['policy_head_channels'] = pc; a['depth'] = 1
    net = N.ResNet((1, 3, 3), 9, 3, a).eval()
    with torch.no_grad():
        for m in net.modules():                                              # BatchNorms away from the identity
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.uniform_(-0.3, 0.3); m.running_var.uniform_(0.6, 1.5); m.weight.uniform_(0.7, 1.3); m.bias.uniform_(-0.2, 0.2)
    return N.FoldedResNet(net)


def _unfrag(w, fk, osub):
    """inverse of HipResNet's `frag`: [fk/32][osub][g 4][i 16][j 8] fp16 -> [fk, osub * 16] float64"""
    return w.reshape(fk // 32, osub, 4, 16, 8).permute(0, 2, 4, 1, 3).reshape(fk, osub * 16).double()


@pytest.mark.parametrize('vc,pc', [(4, 4), (1, 16), (16, 16)])
def test_head_channels_below_16_are_zero_padded(vc, pc):
    """HipResNet's factorised-heads operands for (vc, pc) head channels, in plain torch on the CPU: the 1x1 head convolution padded to
    16 + 16 rows (zero rows, zero biases -> the padded features are exact zeros), the chain matrices with zero rows at the padded feature
    slots; the logits computed from the packed operands equal the unpadded computation on the same fp16-rounded values (float64 sums:
    equal up to the order of the additions, 1e-12 of a logit of order 1); (16, 16) packs byte for byte as the code before the padding"""
    import torch
    from alphazero_general_amd import nnet as N
    f = _folded(vc, pc)
    h = N.HipResNet(f, TT, 'cpu')
    assert h.fact_head and not h.fused_head and h.feat_k == 160 and h.A == 9 and h.NV == 3
    CH, HW, FK = 32, 9, 160
    w1 = h.head1_w.reshape(CH // 32, 2, 4, 16, 8).permute(1, 3, 0, 2, 4).reshape(32, CH).double()      # rows: 16 policy, 16 value
    b1 = h.head1_b.double()
    assert bool((w1[pc:16] == 0).all()) and bool((w1[16 + vc:] == 0).all()) and bool((b1[pc:16] == 0).all()) and bool((b1[16 + vc:] == 0).all())
    w2p, w2v = _unfrag(h.head2_wp, FK, 1), _unfrag(h.head2_wv, FK, 1)
    for w, c in ((w2p, pc), (w2v, vc)):
        assert bool((w[:HW * 16].reshape(HW, 16, 16)[:, c:] == 0).all()) and bool((w[HW * 16:] == 0).all())
    assert h.head_rows.shape == (12, FK) and bool((h.head_rows.double() == torch.cat([w2p[:, :9].t(), w2v[:, :3].t()])).all())
    assert bool((_unfrag(h.head2_wps, FK, 1) == w2p).all())                  # one policy subtile: subtile-major is the same order
    torch.manual_seed(11)
    s = torch.randn(7, CH, 3, 3).half().double()                             # a final stream
    feat = (torch.einsum('oc,bcyx->byxo', w1, s) + b1).half().double().reshape(7, HW, 32)   # [b, pos, 32]: the kernel's fp16 features
    assert bool((feat[:, :, pc:16] == 0).all()) and bool((feat[:, :, 16 + vc:] == 0).all())
    fp = torch.zeros(7, FK, dtype=torch.float64); fv = torch.zeros(7, FK, dtype=torch.float64)
    fp[:, :HW * 16] = feat[:, :, :16].reshape(7, -1); fv[:, :HW * 16] = feat[:, :, 16:].reshape(7, -1)
    b2 = h.head2_b.double()
    lp, lv = fp @ w2p[:, :9] + b2[:9], fv @ w2v[:, :3] + b2[9:12]
    # the unpadded computation: the head convolution's own rows, the Linear chains' own [out, c * HW + pos] matrices, same rounding points
    hw_, hb = f.head_w.float().reshape(-1, CH).half().double(), f.head_b.float().double()
    hu = (torch.einsum('oc,bcyx->boyx', hw_, s) + hb[None, :, None, None]).half().double()        # [b, vc + pc, 3, 3]: value channels first
    rv = hu[:, :vc].reshape(7, -1) @ f.v_fc.weight.float().half().double().t() + f.v_fc.bias.float().double()
    rp = hu[:, vc:].reshape(7, -1) @ f.pi_fc.weight.float().half().double().t() + f.pi_fc.bias.float().double()
    assert torch.allclose(lp, rp, rtol=0, atol=1e-12 * max(1.0, float(rp.abs().max())))
    assert torch.allclose(lv, rv, rtol=0, atol=1e-12 * max(1.0, float(rv.abs().max())))
    assert float(rp.std()) > 1e-3 and float(rv.std()) > 1e-3
    if (vc, pc) == (16, 16):                                                 # the packing as it was: no padding step at all
        hw32, hb32 = f.head_w.float().reshape(-1, CH), f.head_b.float()
        Wv, Wp = f.v_fc.weight.float(), f.pi_fc.weight.float()
        o1 = torch.cat([hw32[vc:], hw32[:vc]]).reshape(2, 16, CH // 32, 4, 8).permute(2, 0, 3, 1, 4).contiguous().reshape(-1).to(torch.float16)
        assert o1.numpy().tobytes() == h.head1_w.numpy().tobytes()
        assert torch.cat([hb32[vc:], hb32[:vc]]).numpy().tobytes() == h.head1_b.numpy().tobytes()
        o2p = torch.zeros((FK, 16)); o2p[:HW * 16, :9] = Wp.reshape(9, pc, HW).permute(2, 1, 0).reshape(HW * pc, 9)
        o2v = torch.zeros((FK, 16)); o2v[:HW * 16, :3] = Wv.reshape(3, vc, HW).permute(2, 1, 0).reshape(HW * vc, 3)
        frag = lambda w: w.reshape(FK // 32, 4, 8, 1, 16).permute(0, 3, 1, 4, 2).contiguous().reshape(-1).to(torch.float16)
        assert frag(o2p).numpy().tobytes() == h.head2_wp.numpy().tobytes() and frag(o2v).numpy().tobytes() == h.head2_wv.numpy().tobytes()


def test_more_than_16_head_channels_stay_collapsed():
    from alphazero_general_amd import nnet as N
    assert not N.HipResNet(_folded(17, 16), TT, 'cpu').fact_head and not N.HipResNet(_folded(16, 32), TT, 'cpu').fact_head


# ------------------------------------------------------------------------------------------------------------------------- package
def test_package_registration():
    from alphazero_general_amd import coach, nnet
    from alphazero_general_amd.Game import _REFERENCE_ENVS, azg_game_id, has_device_rules
    from alphazero_general_amd.MCTS import decode_state, encode_state
    Game = _game()
    assert azg_game_id(Game) == TT and coach._ours(Game) is Game and has_device_rules(Game)
    assert 'envs.tictactoe.tictactoe' not in _REFERENCE_ENVS                 # the reference's own class still falls through behind install()
    a = nnet.TICTACTOE_NET_ARGS
    assert (a.num_channels, a.depth, a.value_head_channels, a.policy_head_channels) == (32, 4, 4, 4)
    assert list(a.value_dense_layers) == [128, 64] and list(a.policy_dense_layers) == [128]
    g = Game()
    for a_ in (4, 0, 8):
        g.play_action(a_)
    cells, player, turns = encode_state(g)
    assert cells.dtype == np.int8 and cells.tolist() == [-1, 0, 0, 0, 1, 0, 0, 0, 1] and (player, turns) == (1, 3)
    back = decode_state(g, cells, player, turns)
    assert type(back) is Game and back == g


@needs_reference
def test_net_args_are_train_pys():
    """TICTACTOE_NET_ARGS against the reference's training script (envs/tictactoe/train.py:24-29), read from its source text"""
    from alphazero_general_amd.nnet import TICTACTOE_NET_ARGS as a
    src = open(os.path.join(REF, 'alphazero', 'envs', 'tictactoe', 'train.py')).read()
    for k in ('num_channels', 'depth', 'value_head_channels', 'policy_head_channels', 'value_dense_layers', 'policy_dense_layers'):
        m = re.search(r'\b%s=([^\n]*?),\n' % k, src)
        assert m, k
        want = eval(m.group(1), {})
        assert (list(a[k]) if isinstance(want, list) else a[k]) == want, k
    assert sorted(a) == sorted(['num_channels', 'depth', 'value_head_channels', 'policy_head_channels', 'value_dense_layers', 'policy_dense_layers'])


@needs_reference
def test_fixtures_regenerate_identically(tmp_path):
    """make_tictactoe_goldens.py, run on the reference again into a temporary directory, writes the committed fixtures array for array"""
    code = ('import sys; sys.path.insert(0, %r); import make_tictactoe_goldens as m; m.main(out_dir=%r, verbose=False)') % (G, str(tmp_path))
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=1800, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    for n in FIXTURES:
        new, old = np.load(os.path.join(str(tmp_path), n + '.npz')), np.load(os.path.join(G, n + '.npz'))
        assert sorted(new.files) == sorted(old.files), n
        for k in old.files:
            a, b = new[k], old[k]
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (n, k)
        assert os.path.getsize(os.path.join(G, n + '.npz')) <= 393524            # no larger than the largest fixture that was there (gb_edge.npz)


@needs_reference
def test_reference_tictactoe_and_host_env_agree_move_for_move():
    """the reference's own tictactoe.Game against envs/tictactoe.py on random playouts: the same azg_state, win state, valid moves and
    observation after the same moves, with the reference's `pieces` as the list of lists Board.__init__ makes and as the ndarray clone()
    leaves (in a child process: importing the reference here would leave it in sys.modules for the modules that run later)"""
    code = 'import sys; sys.path.insert(0, %r); import test_tictactoe_cpu as t; t.reference_objects_check()' % HERE
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=900, env=env, cwd=os.path.dirname(HERE))
    assert r.returncode == 0, r.stderr[-3000:]


def reference_objects_check():
    sys.path.insert(0, G)
    sys.path.insert(0, os.path.dirname(HERE))
    import refharness as rh
    rh.import_reference()
    from alphazero.envs.tictactoe.tictactoe import Game as RefGame
    from alphazero_general_amd.Game import has_device_rules
    Ours = _game()
    assert RefGame.max_turns() is None and not has_device_rules(RefGame)
    rng = np.random.RandomState(5)
    n = 0
    for game in range(40):
        g, o = RefGame(), Ours()
        for ply in range(10):
            for gg in (g, g.clone()):                                        # pieces: a list of lists, an ndarray after clone()
                cells = np.asarray(gg._board.pieces, np.int8).reshape(-1)
                assert (cells == o.to_azg_state()[0]).all() and gg.player == o.player and gg.turns == o.turns
                back = Ours.from_azg_state(cells, gg.player, gg.turns)
                assert back == o and (np.asarray(gg.valid_moves()) == back.valid_moves()).all()
                assert (np.asarray(gg.win_state()) == back.win_state()).all() and (np.asarray(gg.observation()) == back.observation()).all()
                n += 1
            if np.asarray(g.win_state()).any():
                break
            a = int(rng.choice(np.flatnonzero(np.asarray(g.valid_moves()))))
            g.play_action(a); o.play_action(a)
    assert n > 400
