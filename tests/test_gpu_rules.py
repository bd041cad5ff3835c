"""Device rule kernels (csrc/azg_games.h: struct C4, struct BR) against the rule tables the REFERENCE itself produced
(tests/golden/c4_rules.npz: 10 362 random-playout positions of alphazero/envs/connect4 + the data of the reference's own
envs/connect4/test_connect4.py:31-39,58-64,99-151; tests/golden/br_rules.npz: 10 773 positions of fastafl/cengine.pyx:109-272
through envs/brandubh/fastafl.pyx) -- every position, on the GPU, through the C ABI:

  * expanding a root exposes valid_moves (the child action set), win_state (Node.e) and observation (the leaf row);
  * a second simulation steered onto the playout's next move exposes play_action: the leaf state must be the table's next
    position (captures, surrounds, king flags, draw-by-turns), and so must its observation.

Connect4Logic.pyx:40-110, connect4.pyx:54-91; fastafl/cengine.pyx:109-272, envs/brandubh/fastafl.pyx:48-121,196-211."""
import os

import numpy as np
import pytest

from fixture_checks import crc

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
C4, BR = 0, 1


def _engine(game, B):
    from alphazero_general_amd.engine import DeviceEngine
    return DeviceEngine(game, B, seed=3, sims_hint=4, cpuct=1.25, fpu_reduction=0.2)


def _ebits(ws):
    return sum(int(w) << j for j, w in enumerate(ws))


def _check_records(torch, game, cells, player, turns, kc, valids, ws, obs_crc, action, succ):
    """One engine slot per record.  cells [n, CELLS] int8, player / turns [n], kc [n] or None, valids [n, A] 0/1, ws [n, P + 1],
    obs_crc [n]; action [n] (-1: none) is played from record i and succ [n] names the record that holds the position it leads to."""
    n, A, NV = len(turns), valids.shape[1], ws.shape[1]
    eng = _engine(game, n)
    eng.set_states([(cells[i], int(player[i]), int(turns[i])) + ((int(kc[i]),) if kc is not None else ()) for i in range(n)])
    obs = eng.new_obs()
    eng.select(obs)                                           # find_leaf at a fresh root: win_state, valid_moves, add_children, observation
    o = obs.cpu().numpy()
    bad = [i for i in range(n) if crc(o[i]) != obs_crc[i]]
    assert not bad, ('observation', bad[:5])
    for i in range(n):
        ch = eng.root_children(i)
        assert (np.sort(ch['a']) == np.flatnonzero(valids[i])).all(), ('valid_moves', i)
        assert eng.tree_info(i)['e'] == _ebits(ws[i]), ('win_state', i)
    # one backup with a policy peaked on the record's action (PUCT at root.n == 1 with no visited child picks the largest
    # prior), then the second simulation descends exactly that ply
    has_next = (np.asarray(action) >= 0) & ~ws.any(1)
    nxt = np.where(has_next, action, 0).astype(np.int64)
    pol = np.full((n, A), 1e-4, np.float32)
    pol[np.arange(n), nxt] = 0.9
    val = np.full((n, NV), 1.0 / NV, np.float32)
    eng.backup(torch.from_numpy(pol).to(eng.device), torch.from_numpy(val).to(eng.device))
    eng.select(obs)
    o = obs.cpu().numpy()
    leaves = eng.get_leaf_states(full=True)
    for i in range(n):
        lc, lp, lt, lk = leaves[i]
        if ws[i].any():                                       # terminal root: find_leaf stops at it (MCTS.pyx:213)
            assert len(eng.last_path(i)) == 0 and (lc == cells[i]).all(), ('terminal', i)
            continue
        if not has_next[i]:
            continue
        j = int(succ[i])
        assert list(eng.last_path(i)) == [nxt[i]], ('descent', i)
        assert (lc == cells[j]).all(), ('play_action: board', i)
        assert lp == player[j] and lt == turns[j], ('play_action: player / turns', i)
        if kc is not None:
            assert lk == kc[j], ('play_action: king flag', i)
        assert crc(o[i]) == obs_crc[j], ('observation after play_action', i)
    eng.counters()                                            # no sticky device error
    eng.close()
    return int(has_next.sum())


def _check_table(torch, game, cells, lens, kc, valids, ws, obs_crc, moves):
    """cells [n, CELLS] int8, lens [n] plies played, valids [n, A] 0/1, ws [n, 3], obs_crc [n], moves [n, maxlen] (the playout
    prefix of every position; positions of one playout are consecutive, so row i + 1 is row i + one move when lens grows by 1)"""
    n = len(lens)
    action, succ = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    for i in range(n - 1):
        if lens[i + 1] == lens[i] + 1 and not ws[i].any():
            assert (moves[i + 1][:lens[i]] == moves[i][:lens[i]]).all()
            action[i], succ[i] = int(moves[i + 1][lens[i]]), i + 1
    L = np.asarray(lens).astype(np.int64)
    return _check_records(torch, game, cells, L % 2, L, kc, valids, ws, obs_crc, action, succ)


def test_c4_rules_vs_reference_tables():
    import torch
    d = dict(np.load(os.path.join(G, 'c4_rules.npz')))
    n = _check_table(torch, C4, d['cells'], d['lens'], None, d['valids'], d['ws'], d['obs_crc'], d['moves'])
    assert len(d['lens']) >= 10000 and n > 9000


def test_c4_reference_test_data_on_device():
    """the reference's own test tables (envs/connect4/test_connect4.py:31-39 move list -> board, :58-64 valid-move table, :99-151
    ten end-state boards) through the device rules."""
    import torch
    d = dict(np.load(os.path.join(G, 'c4_rules.npz')))
    boards = d['end_boards']
    eng = _engine(C4, len(boards))
    eng.set_states([(b.reshape(-1), int(np.count_nonzero(b)) % 2, int(np.count_nonzero(b))) for b in boards])
    eng.select(None)
    for i, (b, ws, winner) in enumerate(zip(boards, d['end_ws'], d['end_winner'])):
        e = eng.tree_info(i)['e']
        assert e == _ebits(ws), i
        assert bool(e & 1) == (winner == 1) and bool(e & 2) == (winner == -1), i
        assert (np.sort(eng.root_children(i)['a']) == np.flatnonzero(b[0] == 0)).all(), i     # columns whose top cell is free
    eng.close()
    # :31-39 the move list [4, 5, 4, 3, 0, 6] played on the device (every prefix set as a root, the tree steered onto the next move, its
    # successor read back as the leaf) must give the reference's board
    eng = _engine(C4, 1)
    cells = np.zeros(42, np.int8)
    for t, a in enumerate([4, 5, 4, 3, 0, 6]):
        eng.set_states([(cells, t % 2, t)])
        eng.select(None)
        pol = np.full((1, 7), 1e-4, np.float32); pol[0, a] = 0.9
        eng.backup(torch.from_numpy(pol).to(eng.device), torch.full((1, 3), 1 / 3, device=eng.device))
        eng.select(None)
        assert list(eng.last_path(0)) == [a]
        cells = eng.get_leaf_states()[0][0].copy()
    assert (cells.reshape(6, 7) == d['moves_board']).all()
    eng.close()
    # :58-64 valid-move table.  The reference's test keeps dropping stones after a four-in-a-row (its Board does not stop), which a
    # search never does, so these boards are built on the host (a stone falls to the lowest free cell of its column, +1 / -1
    # alternating) and the device answers valid_moves for them
    lists = [[int(x) for x in mv[mv >= 0]] for mv in d['vm_moves']]
    boards = []
    for mv in lists:
        b = np.zeros((6, 7), np.int8)
        for t, a in enumerate(mv):
            b[np.flatnonzero(b[:, a] == 0).max(), a] = 1 if t % 2 == 0 else -1
        boards.append(b)
    eng = _engine(C4, len(boards))
    eng.set_states([(b.reshape(-1), len(mv) % 2, len(mv)) for b, mv in zip(boards, lists)])
    eng.select(None)
    for i, ev in enumerate(d['vm_expected']):
        v = np.zeros(7, np.uint8); v[eng.root_children(i)['a']] = 1
        assert (v == ev).all(), i
    eng.close()


def test_br_rules_vs_reference_tables():
    import torch
    d = dict(np.load(os.path.join(G, 'br_rules.npz')))
    valids = np.unpackbits(d['valid_bits'], axis=1)[:, :588]
    n = _check_table(torch, BR, d['cells'], d['lens'], d['kc'], valids, d['ws'], d['obs_crc'], d['moves'])
    assert len(d['lens']) >= 10000 and n > 9000
    assert int(valids.sum(1).max()) == int(d['max_k'])


# ------------------------------------------------------------------------------------------------ built and dense boards
def _check_fixture(name, game):
    import torch
    import rules_edge as RE
    d = RE.load(name)
    n = _check_records(torch, game, d['cells'], d['player'], d['turns'], d['kc'] if name == 'br' else None, d['valids'], d['ws'],
                       d['obs_crc'], d['action'], d['succ'])
    assert n == int((d['action'] >= 0).sum())
    return d, n


def test_br_rules_on_built_and_dense_boards():
    """tests/golden/br_rules_edge.npz (make_rules_edge_goldens.py): custodian capture, two-sided king capture, group surround, moves
    and win states built in all eight symmetries, dense random boards, capture-greedy playouts -- where BR::play's early exit, the
    flood fill, reach7 and the neighbour masks of BR::win_bits are equal to the reference only by argument"""
    d, n = _check_fixture('br', BR)
    assert n >= 1500 and int(d['valids'].sum(1).max()) > 64              # the second 64-lane chunk of BR::valid_list holds moves


def test_c4_rules_on_built_boards():
    """tests/golden/c4_rules_edge.npz: all 69 lines in both colours, lines of 5 to 7, wrapped runs, both colours holding a four,
    full-board draws, the 42nd stone, every column at every height"""
    d, n = _check_fixture('c4', C4)
    assert n >= 290 and int(d['ws'][:, 2].sum()) >= 4


def test_tm_rules_on_built_boards():
    """trimok has no reference: the boards of tests/rules_edge.py (every line of three per colour, the wrapped triples, several
    players holding a line, full-board draws, the 25th stone), answered by the host env that defines the game"""
    d, n = _check_fixture('tm', 2)
    assert n >= 500 and int(d['ws'][:, 3].sum()) >= 6


def _form_positions(name):
    """(game id, states, action to steer the second simulation onto (-1: terminal), obs crc of the root or None, engine options)"""
    import rules_edge as RE
    if name in ('br', 'c4', 'tm'):
        d = RE.load(name)
        n = len(d['action'])
        states = [(d['cells'][i], int(d['player'][i]), int(d['turns'][i]), int(d['kc'][i])) for i in range(n)]
        first = np.where(d['valids'].any(1), d['valids'].argmax(1), -1)
        act = np.where(d['ws'].any(1), -1, np.where(d['action'] >= 0, d['action'], first))
        return {'c4': C4, 'br': BR, 'tm': 2}[name], states, act.astype(np.int64), d['obs_crc'], {}
    if name == 'ot':
        d = dict(np.load(os.path.join(G, 'ot_rules.npz')))
        idx = np.arange(0, len(d['lens']), 5)
        states = [(d['cells'][i], int(d['lens'][i]) % 2, int(d['lens'][i])) for i in idx]
        act = np.where(d['ws'][idx].any(1), -1, d['valids'][idx].argmax(1))
        return 3, states, act.astype(np.int64), d['obs_crc'][idx], {}
    from alphazero_general_amd import _abi
    d = dict(np.load(os.path.join(G, 'gb_rules.npz')))
    live = (d['next'] >= 0) & (d['lens'] >= 0)
    live[-1] = False
    idx = np.flatnonzero(live | d['ws'].any(1))[::8]
    states = [(_abi.gobang_unpack(d['cells'][i].tobytes()), int(d['player'][i]), int(d['turns'][i])) for i in idx]
    act = np.where(d['ws'][idx].any(1), -1, d['next'][idx])
    return 4, states, act.astype(np.int64), d['obs_crc'][idx], dict(nodes_per_tree=1024)


@pytest.mark.parametrize('name', ['c4', 'br', 'tm', 'ot', 'gb'])
def test_observation_forms_agree(name):
    """azg_select writes the leaf observation in three forms: f32 NCHW, f16 NCHW and f16 NHWC with the channels padded to 8 (obs8 /
    write_obs_nhwc8, the form every network launch is fed).  At the root and one ply down, on the rule records of every game, all
    three must hold exactly the f32 planes cast to fp16 (the f32 planes being the reference's, by crc), channels beyond obs_c zero.
    Every buffer is filled with a sentinel first, so a cell the kernel leaves out shows."""
    import torch
    from alphazero_general_amd.engine import DeviceEngine
    game, states, act, root_crc, opts = _form_positions(name)
    n = len(states)
    assert n >= 800 and int((act >= 0).sum()) >= 200 and int((act < 0).sum()) >= 10
    eng = DeviceEngine(game, n, seed=3, sims_hint=4, cpuct=1.25, fpu_reduction=0.2, **opts)
    Cc, H, W = eng.obs_shape
    assert Cc <= 8
    pol = np.full((n, eng.A), 1e-4, np.float32)
    pol[np.arange(n), np.maximum(act, 0)] = 0.9
    pol_t = torch.from_numpy(pol).to(eng.device)
    val_t = torch.full((n, eng.NV), 1.0 / eng.NV, device=eng.device)
    got = {}
    for form in ('f32', 'f16', 'nhwc8'):
        obs = (torch.full((n, H * W, 8), 7.0, dtype=torch.float16, device=eng.device) if form == 'nhwc8' else
               torch.full((n, Cc, H, W), 7.0, dtype=torch.float32 if form == 'f32' else torch.float16, device=eng.device))
        eng.set_states(states)
        eng.select(obs)
        root = obs.cpu().numpy().copy()
        obs.fill_(7.0)
        eng.backup(pol_t, val_t)
        eng.select(obs)
        paths = [list(eng.last_path(i)) for i in range(n)]
        assert paths == [[int(a)] if a >= 0 else [] for a in act], form
        got[form] = (root, obs.cpu().numpy().copy())
    eng.counters()
    eng.close()
    for ply in (0, 1):
        f32, f16, n8 = got['f32'][ply], got['f16'][ply], got['nhwc8'][ply]
        if ply == 0:
            bad = [i for i in range(n) if crc(f32[i]) != root_crc[i]]
            assert not bad, ('f32 root observation against the reference', bad[:5])
        want = f32.astype(np.float16)
        assert (f16.view(np.uint16) == want.view(np.uint16)).all(), ('f16 NCHW', ply)
        planes = n8[:, :, :Cc].transpose(0, 2, 1).reshape(n, Cc, H, W)
        assert (np.ascontiguousarray(planes).view(np.uint16) == want.view(np.uint16)).all(), ('f16 NHWC', ply)
        assert (n8[:, :, Cc:].view(np.uint16) == 0).all(), ('padding channels', ply)
