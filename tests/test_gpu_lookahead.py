"""One ply on the GPU: azg_game_lookahead (csrc/azg_rules.h k_game_lookahead through DeviceGames.lookahead) against the host envs'
children on every game, perft as a torch loop of it against tests/golden/lookahead.npz, azg_game_choose_scripted against the
reference's recorded moves and the restated players (tests/lookahead_reference.py, held to the fixture in tests/test_lookahead_cpu.py),
and SCRIPTED_SEAT in ArenaRunner and over two ranks.  Every comparison is exact."""
import functools
import json
import os
import signal
import subprocess
import sys

import numpy as np
import pytest

import lookahead_reference as LR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('connect4', 'brandubh', 'trimok', 'othello', 'gobang', 'tictactoe', 'hnefatafl')
FILL = 0xAB


def _T():
    import test_gpu_device_games as T
    return T


def _dg(gid):
    return _T()._dg(gid)


# ------------------------------------------------------------------------------------------------------------------------- the inputs
def _no_move_state(gid):
    """a position of the game without a valid move"""
    if gid == LR.C4:
        return LR.built_states(LR.C4)[-1]
    if gid == LR.OT:
        return LR.built_states(LR.OT)[2]                              # stones of one colour only
    if gid == LR.GB:
        return LR.built_states(LR.GB)[-1]
    if gid == LR.TT:
        return (np.array([1, -1, 1, 1, -1, -1, -1, 1, 1], np.int8), 0, 9)
    if gid == LR.TM:
        g = _T()._envs()[gid]()
        while np.asarray(g.valid_moves()).any():                      # (fill the board: play_action does not consult win_state)
            g.play_action(int(np.flatnonzero(g.valid_moves())[0]))
        return tuple(g.to_azg_state()[:3])
    n = 7 if gid == LR.BR else 11                                     # tafl: one piece of code 1 and nobody else -- the other side has nothing to move
    cells = np.asarray(_T()._envs()[gid]().to_azg_state()[0]).copy()
    cells[(cells == 1) | (cells == 2) | (cells == 3)] = 0
    cells[1] = 1
    for player in (0, 1):
        if not np.asarray(LR.host(gid, (cells, player, 4, 0)).valid_moves()).any():
            return (cells, player, 4, 0)
    raise AssertionError('no side without a move on the %dx%d board' % (n, n))


def _finished_with_moves(gid):
    """a position whose win_state is set and that still has valid moves (othello has none: its game ends when the mover cannot move)"""
    T = _T()
    if gid == LR.OT:
        return None
    if gid == LR.TM:
        rng = np.random.RandomState(5)
        while True:
            g = T._envs()[gid]()
            while not np.asarray(g.win_state()).any():
                g.play_action(int(rng.choice(np.flatnonzero(g.valid_moves()))))
            if np.asarray(g.valid_moves()).any():
                return tuple(g.to_azg_state()[:3])
    t = T._table(T.MAIN_TABLE[gid])
    for i in np.flatnonzero(t['ws'].any(1)):
        if np.asarray(LR.host(gid, t['states'][i]).valid_moves()).any():
            return t['states'][i]
    raise AssertionError('no finished position with moves in the table')


@functools.lru_cache(maxsize=None)
def _inputs(gid):
    """(states, expected): the 256 table positions (hnefatafl_ring first for hnefatafl), a position without a move, a finished one that
    still has moves; expected[i] = [(action, child GameState)] from the host env -- computed once, shared, never written to"""
    states = list(LR.positions(gid)) + [_no_move_state(gid)]
    fin = _finished_with_moves(gid)
    if fin is not None:
        states.append(fin)
    hosts = [LR.host(gid, st) for st in states]
    exp = [LR.children(g) for g in hosts]
    n = len(LR.positions(gid))
    assert len(exp[n]) == 0 and (fin is None or (len(exp[n + 1]) > 0 and np.asarray(hosts[n + 1].win_state()).any()))
    if gid == LR.HN:
        assert len(exp[0]) == 321
    return states, exp


def _filled(shape, dtype, value, dev):
    import torch
    return torch.full(shape, value, dtype=dtype, device=dev)


# ------------------------------------------------------------------------------------------------------------------------- lookahead
@pytest.mark.parametrize('gid', range(7), ids=NAMES)
def test_lookahead_is_the_host_envs_children(gid):
    """num, actions, win and children byte for byte; rows j >= k and rows past n of a pre-filled out= untouched; obs in the three
    formats equal to step() on the same children; one captured-graph replay gives the same bytes"""
    import torch
    from alphazero_general_amd.games import Lookahead
    dg = _dg(gid)
    states, exp = _inputs(gid)
    st = dg.pack(states)
    n, K, NV, dev = len(states), dg.max_children, dg.NV, dg.device
    assert K == dg.gi.max_children and max(len(e) for e in exp) <= K

    def buffers():
        return Lookahead(_filled((n + 3,), torch.int32, -7, dev), _filled((n + 3, K), torch.int32, -7, dev),
                         _filled((n + 3, K, NV), torch.uint8, FILL, dev), _filled((n + 3, K, 80), torch.uint8, FILL, dev), None)
    out = buffers()
    la = dg.lookahead(st, win=True, children=True, out=out)
    assert la.obs is None and la.num.data_ptr() == out.num.data_ptr() and la.children.data_ptr() == out.children.data_ptr()
    num, act = la.num.cpu().numpy(), la.actions.cpu().numpy()
    win, ch = la.win.cpu().numpy(), la.children.cpu().numpy()
    assert num.tolist() == [len(e) for e in exp]
    want_act = np.full((n, K), -1, np.int32)
    want_win = np.full((n, K, NV), FILL, np.uint8)
    want_ch = np.full((n, K, 80), FILL, np.uint8)
    flat = dg.pack([c for e in exp for _, c in e]).cpu().numpy()
    pos = 0
    for i, e in enumerate(exp):
        want_act[i, :len(e)] = [a for a, _ in e]
        for j, (_, c) in enumerate(e):
            want_win[i, j] = np.asarray(c.win_state(), np.uint8)
        want_ch[i, :len(e)] = flat[pos:pos + len(e)]
        pos += len(e)
    assert (act == want_act).all(), np.argwhere(act != want_act)[:5]
    assert (win == want_win).all(), np.argwhere(win != want_win)[:5]
    assert (ch == want_ch).all(), np.argwhere((ch != want_ch).any(2))[:5]
    for b, v in ((out.num, -7), (out.actions, -7), (out.win, FILL), (out.children, FILL)):
        assert bool((b[n:] == v).all()), 'rows past n are left alone'
    # the observations: a new tensor (zeros) -- rows j < k are step()'s observation of that child, rows j >= k stay zero
    mask = la.actions >= 0
    kids = la.children[mask].contiguous()
    for form in (torch.float32, torch.float16, 'nhwc8'):
        o = dg.lookahead(st, win=False, children=False, obs=form)
        assert o.win is None and o.children is None and torch.equal(o.actions, la.actions) and torch.equal(o.num, la.num)
        ref = dg.step(kids, None, next=False, valid=False, win=False, obs=form).obs
        assert tuple(o.obs.shape) == (n, K) + dg.obs_tail(form) and o.obs.dtype == ref.dtype
        assert torch.equal(o.obs[mask], ref) and not bool(o.obs[~mask].any()), form
        del o, ref
    # one captured launch, replayed into fresh buffers
    gout = buffers()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dg.lookahead(st, win=True, children=True, out=gout)
    torch.cuda.current_stream().wait_stream(side)
    fresh = buffers()
    for b, f in zip(gout[:4], fresh[:4]):
        b.copy_(f)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dg.lookahead(st, win=True, children=True, out=gout)
    for b, f in zip(gout[:4], fresh[:4]):
        b.copy_(f)
    graph.replay()
    torch.cuda.synchronize()
    for b, e in zip(gout[:4], out[:4]):
        assert torch.equal(b, e)


def test_lookahead_argument_checks():
    import torch
    from alphazero_general_amd.games import Lookahead
    dg = _dg(LR.TT)
    st = dg.initial(4)
    e = dg.lookahead(st)
    assert tuple(e.num.shape) == (4,) and tuple(e.actions.shape) == (4, 9) and tuple(e.win.shape) == (4, 9, 3) and e.children is None
    assert e.num.tolist() == [9] * 4 and e.actions.tolist() == [list(range(9))] * 4 and not bool(e.win.any())
    with pytest.raises(AssertionError):
        dg.lookahead(st, obs='nchw')
    with pytest.raises(AssertionError):
        dg.lookahead(st, out=Lookahead(torch.zeros(3, dtype=torch.int32, device=dg.device), None, None, None, None))
    with pytest.raises(AssertionError):
        dg.lookahead(st.cpu())
    assert dg.scripted_player is None and _dg(LR.C4).scripted_player == 'OneStepLookaheadConnect4Player'
    from alphazero_general_amd import _abi
    with pytest.raises(_abi.AzgError) as ei:
        dg.choose_scripted(st)
    assert ei.value.code == _abi.E_UNSUPPORTED


# ------------------------------------------------------------------------------------------------------------------------- perft
@pytest.mark.parametrize('gid', range(7), ids=NAMES)
def test_perft_on_the_device(gid):
    """lookahead(children=True) + a boolean gather per ply: the fixture's node and win_state counts at every depth (the 3-player env:
    the counts tests/test_lookahead_cpu.py records from the host env)"""
    dg = _dg(gid)
    if gid == LR.TM:
        want_nodes, want_wins = [25, 600, 13800], [[0, 0, 0, 0]] * 3
    else:
        d = LR.golden()
        want_nodes, want_wins = d[LR.SHORT[gid] + '_perft_nodes'].tolist(), d[LR.SHORT[gid] + '_perft_wins'].tolist()
    frontier, nodes, wins = dg.initial(1), [], []
    for _ in range(LR.PERFT_DEPTH[gid]):
        la = dg.lookahead(frontier, children=True)
        exists = la.actions >= 0
        nodes.append(int(la.num.sum()))
        assert int(exists.sum()) == nodes[-1]
        wins.append(la.win[exists].long().sum(0).cpu().tolist())
        frontier = la.children[exists & (la.win.sum(2) == 0)].contiguous()
    assert nodes == want_nodes and wins == want_wins


# ------------------------------------------------------------------------------------------------------------------------- choose_scripted
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0')


@pytest.mark.parametrize('gid', sorted(LR.SCRIPTED), ids=[NAMES[g] for g in sorted(LR.SCRIPTED)])
def test_choose_scripted_is_the_reference_players(gid):
    """the fixture's moves on the 256 table positions and the built boards; status 1 and action -1 where the reference raised; for
    connect4 the sweep u = (j + 0.5) / m recovers exactly the recorded list in ascending order, and u = 0 / the largest double below 1
    are its first / last element"""
    import torch
    from alphazero_general_amd.games import Choice
    dg, d, s = _dg(gid), LR.golden(), LR.SHORT[gid]
    assert dg.scripted_player == LR.SCRIPTED[gid]
    for tag, states in (('', LR.positions(gid)), ('_built', LR.built_states(gid))):
        st, n = dg.pack(states), len(states)
        move = d[s + tag + '_move'].astype(np.int64)
        raised = np.array([bool(r) for r in d[s + '_built_raised']]) if tag else np.zeros(n, bool)
        if gid != LR.C4:
            for u in (0.0, 0.5, float(np.nextafter(1.0, 0))):         # (no u is consumed)
                c = dg.choose_scripted(st, torch.full((n,), u, dtype=torch.float64, device=dg.device))
                assert c.actions.cpu().tolist() == move.tolist() and c.status.cpu().tolist() == raised.astype(int).tolist(), (tag, u)
            continue
        lists = [[int(a) for a in row if a >= 0] for row in d[s + tag + '_list']]
        idx = d[s + tag + '_idx'].astype(np.int64)
        m = np.array([max(len(x), 1) for x in lists])
        c = dg.choose_scripted(st, _dev((idx.clip(0) + 0.5) / m))
        assert c.actions.cpu().tolist() == move.tolist() and c.status.cpu().tolist() == raised.astype(int).tolist(), tag
        got = [[] for _ in range(n)]
        for j in range(7):                                            # the sweep: j-th element wherever the list has one
            a = dg.choose_scripted(st, _dev((np.minimum(j, m - 1) + 0.5) / m)).actions.cpu().tolist()
            for i in range(n):
                if j < len(lists[i]):
                    got[i].append(a[i])
        assert got == lists and all(x == sorted(x) for x in lists)
        for u, pick in ((0.0, 0), (float(np.nextafter(1.0, 0)), -1)):
            a = dg.choose_scripted(st, torch.full((n,), u, dtype=torch.float64, device=dg.device)).actions.cpu().tolist()
            assert a == [x[pick] if x else -1 for x in lists], u
    # out= longer than n, u=None: the caller's tensors, rows past n untouched, a move of the position
    st = dg.pack(LR.positions(gid)[:5])
    out = Choice(torch.full((8,), 77, dtype=torch.int32, device=dg.device), torch.full((8,), 77, dtype=torch.int32, device=dg.device))
    c = dg.choose_scripted(st, out=out)
    assert c.actions.data_ptr() == out.actions.data_ptr() and out.actions[5:].cpu().tolist() == [77] * 3 == out.status[5:].cpu().tolist()
    valid = dg.step(st, next=False, win=False).valid.cpu().numpy()
    assert c.status.cpu().tolist() == [0] * 5 and all(valid[i, a] for i, a in enumerate(c.actions.cpu().tolist()))


# ------------------------------------------------------------------------------------------------------------------------- seats
@pytest.mark.parametrize('game,rounds', [('connect4', 44), ('othello', 30)])
def test_arena_with_the_scripted_seat(game, rounds):
    """[net, SCRIPTED_SEAT] on 16 slots: in every round each slot whose mover sits on the scripted seat played the restated player's
    move for that round's uniform, and everybody's moves are those of a twin runner with a raw seat in its place that is handed the
    recorded actions through advance(actions=...); the tallies add up"""
    import torch
    import test_gpu_choose as TC
    from alphazero_general_amd.selfplay import SCRIPTED_SEAT, ArenaRunner
    gid = LR.C4 if game == 'connect4' else LR.OT
    Game, nets = TC._nets(game)
    args = TC._arena_args(gamesPerIteration=1 << 30)
    r = ArenaRunner(Game, [nets[0], SCRIPTED_SEAT], args, num_slots=16, seed=31, seats='slot', result_capacity=4096)
    twin = ArenaRunner(Game, [nets[0], None], args, num_slots=16, seed=31, seats='slot', result_capacity=4096, use_graph=False)
    assert r._tf_scripted == [1] and r.nnets[1] is None and twin._graph is None and r.wide_search == twin.wide_search
    sims, played = int(args.numMCTSSims), 0
    none = torch.full((16,), -1, dtype=torch.int32, device=r.engine.device)
    for rnd in range(rounds):
        before = r.games.unpack(r.engine.states_dev().clone())
        u = r._tree_free_uniforms().cpu().numpy().copy()
        seat = r._tf_seat.cpu().numpy()
        r.play_round()
        acts = r.engine.last_actions().cpu().numpy()
        mine = np.array([seat[s, before[s][1]] == 1 for s in range(16)])
        for s in np.flatnonzero(mine):
            assert acts[s] == LR.scripted_move(gid, LR.host(gid, before[s]), u[s]), (rnd, s)
        played += int(mine.sum())
        if twin.wide_search:
            twin._search_wide(sims)
        else:
            for _ in range(sims):
                twin.step()
        given = none.clone()
        given[torch.from_numpy(mine).to(given.device)] = torch.from_numpy(acts[mine].astype(np.int32)).to(given.device)
        twin.engine.advance(False, given)
        assert twin.engine.last_actions().cpu().tolist() == acts.tolist(), rnd
        assert torch.equal(twin.engine.states_dev(), r.engine.states_dev()), rnd
    assert played >= 4 * rounds
    c = r.engine.counters()
    wins, draws, _ = r.results()
    assert sum(wins) + draws == c['num_results'] == twin.engine.counters()['num_results'] and c['games_played'] == twin.engine.counters()['games_played']
    assert c['num_results'] >= (16 if game == 'connect4' else 0)       # (42 plies end every connect4 game; an othello game takes up to 60)
    r.engine.close(); twin.engine.close()


def test_scripted_seat_reaches_a_serving_rank(tmp_path):
    """two ranks on one GPU (tests/lookahead_rig.py): [net, SCRIPTED_SEAT] through iteration.lead / serve plays the comparison two ranks
    play when each holds the net and the seat"""
    import lookahead_rig as R
    from alphazero_general_amd import iteration as I
    out = str(tmp_path / 'scripted.json')
    env = dict(os.environ, AZG_DIST_BACKEND='gloo', AZG_SINGLE_DEVICE='1')
    env.pop('WORLD_SIZE', None); env.pop('RANK', None)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1', '--master-port', '29658',
           os.path.join(ROOT, 'tests', 'lookahead_rig.py'), out]
    p = subprocess.Popen(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, start_new_session=True)
    try:
        log, _ = p.communicate(timeout=300)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)
        raise
    assert p.returncode == 0, log.decode(errors='replace')[-3000:]
    rec = json.load(open(out))
    assert json.load(open(out + '.rank1'))['served'] == 1              # the arena command; then 'stop'
    d, c = rec['direct'], rec['coach']
    assert d == c
    assert d['games'] == R.GAMES and d['ranks'] == 2 and sum(d['wins']) + d['draws'] == d['num_results'] >= R.GAMES
    assert d['winrates'] == I.winrates(d['wins'], d['draws'], True)
