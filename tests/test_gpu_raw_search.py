"""The network-free search launch (azg_search_raw: `sims` x [find_leaf, constant policy / value rows, process_results] of every slot
in ONE launch) and its callers -- MCTS.raw_search, the warm-up rounds of SelfPlayRunner and of the compat SelfPlayAgent.

  * against the CPU oracle's MCTS.raw_search (oracle/azg_mcts_ref.c:257-269, pinned to the reference's goldens) on one tree,
  * against the launch-per-phase loop (azg_select(NULL) + azg_backup with the same constant rows) on all five games, whole games,
  * the warm-up runner against the oracle's warm-up agent, the captured round graph against plain launches,
  * the reported error conditions, and the MCTS class / compat agent paths.
Every comparison is exact equality."""
import os
import queue

import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
C4, BR, TM, OT, GB = 0, 1, 2, 3, 4
RAW = 'raw'            # MCTS.raw_search's rows (MCTS.pyx:176-177): p = ones(A), v = zeros(P + 1)
WARM = 'warm'          # a warm-up agent's (SelfPlayAgent.pyx:48-52): p = full(1 / A), v = full(1 / NV)


def _engine(game, B, **kw):
    from alphazero_general_amd.engine import DeviceEngine
    return DeviceEngine(game, B, **kw)


def _rows(e, consts):
    if consts == RAW:
        return 1.0, np.zeros(e.NV, np.float32)
    return float(np.float32(1 / e.A)), np.full(e.NV, 1 / e.NV, np.float32)


def _ostate(game, g):
    return (g.cells(), g.player, g.turns, g.s.aux[0]) if game == BR else (g.cells(), g.player, g.turns)


def _midgame(game, plies, seed):
    """a position `plies` random legal moves into a game (oracle rules), not finished"""
    rng = np.random.RandomState(seed)
    while True:
        g = ol.OGame(game)
        for _ in range(plies):
            g.play(int(rng.choice(np.flatnonzero(g.valid_moves()))))
            if g.win_state().any():
                break
        if not g.win_state().any():
            return g


# ---------------------------------------------------------------------------------------- 1. one tree against the oracle
@pytest.mark.parametrize('noise,temp', [(0, 0), (1, 1)])
@pytest.mark.parametrize('game', [C4, BR, TM])
def test_search_raw_single_tree_vs_oracle(game, noise, temp):
    seed = 77 + game
    e = _engine(game, 1, seed=seed, sims_hint=25)
    e.set_search_flags(noise, temp)
    try:
        for start in ('initial', 'mid'):
            og = ol.OGame(game) if start == 'initial' else _midgame(game, 6, 5 + game)
            for s in (1, 2, 25):
                e.set_states([_ostate(game, og)])
                e.set_tape_counters([0])
                e.reset_max_depth()
                om = ol.OMCTS(game, seed=seed, stream=0)
                e.search_raw(s, 1.0, np.zeros(e.NV, np.float32))
                om.raw_search(og, s, noise, temp)
                ch, och = e.root_children(0), om.root_children()
                for f in ('a', 'n', 'q', 'p', 'v'):
                    assert ch[f].shape == och[f].shape and (ch[f] == och[f]).all(), (start, s, f)
                n, q, v, player = ol.C.c_int32(), ol.C.c_float(), ol.C.c_float(), ol.C.c_int32()
                eb = np.zeros(ol.MAX_PLAYERS + 1, np.uint8)
                ol.lib().azo_mcts_root_header(om.h, ol.C.byref(n), ol.C.byref(q), ol.C.byref(v), ol.C.byref(player), eb)
                info = e.tree_info(0)
                assert (info['n'], np.float32(info['q']), np.float32(info['v']), info['player']) == (n.value, np.float32(q.value), np.float32(v.value), player.value), (start, s)
                assert info['n'] == s and info['e'] == sum(int(b) << j for j, b in enumerate(eb)), (start, s)
                assert info['max_depth'] == om.max_depth and info['depth'] == ol.lib().azo_mcts_depth(om.h), (start, s)
                assert (e.last_path(0) == om.last_path()).all(), (start, s)
                assert int(e.tape_counters()[0]) == ol.lib().azo_mcts_tape_ctr(om.h), (start, s)
                c = e.counters()
        assert c['sims'] == 2 * (1 + 2 + 25)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------- 2. launch == per-phase loop, all games
def _snapshot(e):
    out = []
    for i in range(e.B):
        ch = e.root_children(i)
        out.append((tuple(ch[f].tobytes() for f in ('a', 'n', 'q', 'p', 'v')), tuple(sorted(e.tree_info(i).items())), e.last_path(i).tobytes()))
    leaves = [(c.tobytes(), p, t, a) for c, p, t, a in e.get_leaf_states(full=True)]
    return out, leaves, e.tape_counters().tobytes(), e.counters()


PAIR_CASES = [
    # game, B, sims, rounds, engine keywords
    (C4, 1, 40, 12, {}), (C4, 5, 40, 12, {}), (C4, 37, 40, 45, {}),
    (GB, 3, 12, 4, {}),                                            # 225 children: four chunks of 64
    (BR, 5, 20, 8, {}), (BR, 37, 20, 3, {}),                       # more than 64 children
    (OT, 5, 20, 8, {}),
    (TM, 37, 10, 30, dict(mcts_reset_threshold=3)), (TM, 5, 10, 30, {}),
]


@pytest.mark.parametrize('consts', [RAW, WARM])
@pytest.mark.parametrize('game,B,sims,rounds,kw', PAIR_CASES)
def test_search_raw_equals_per_phase_loop(game, B, sims, rounds, kw, consts):
    import torch
    from alphazero_general_amd import _abi
    gi = _abi.game_info(game)
    mk = lambda: _engine(game, B, seed=31 + game, sims_hint=sims, add_root_noise=True, add_root_temp=True, cpuct=4.0, fpu_reduction=0.4,
                         example_capacity=B * (rounds + 1) * gi.num_symmetries, **kw)
    ea, eb = mk(), mk()
    try:
        fill, vrow = _rows(ea, consts)
        pol = torch.full((B, ea.A), fill, dtype=torch.float32, device=eb.device)
        val = torch.from_numpy(np.tile(vrow, (B, 1))).to(eb.device)
        for rnd in range(rounds):
            ea.search_raw(sims, fill, vrow)
            for _ in range(sims):
                eb.select(None)
                eb.backup(pol, val)
            assert _snapshot(ea) == _snapshot(eb), rnd                 # every slot, every field
            ea.advance(True); eb.advance(True)
            assert torch.equal(ea.last_actions(), eb.last_actions()), rnd
        ca, cb = ea.counters(), eb.counters()
        assert ca == cb and ca['sims'] == B * sims * rounds
        if (game, B) == (C4, 37):
            assert ca['games_played'] > B                          # games ended and restarted: terminal leaves, terminal roots
        for x, y in zip(ea.examples(), eb.examples()):
            assert torch.equal(x, y)
        for x, y in zip(ea.results(), eb.results()):
            assert (x == y).all()
    finally:
        ea.close(); eb.close()


# ---------------------------------------------------------------------------------------- 3. warm-up runner against the oracle
def _args(**kw):
    from alphazero_general_amd.utils import dotdict, default_temp_scaling
    a = dotdict(numMCTSSims=25, numFastSims=20, numWarmupSims=5, probFastSim=0.0, gamesPerIteration=1 << 30, cpuct=1.25, fpu_reduction=0.2,
                root_noise_frac=0.1, root_policy_temp=1.1, min_discount=1.0, add_root_noise=True, add_root_temp=True,
                symmetricSamples=True, mctsResetThreshold=0, startTemp=1.0, arenaTemp=0.25, temp_scaling_fn=default_temp_scaling)
    a.update(kw)
    return a


@pytest.mark.parametrize('game,B,games', [('connect4', 16, 24), ('brandubh', 8, 10)])
def test_warmup_runner_raw_launch_vs_oracle_agent(game, B, games):
    import importlib
    from alphazero_general_amd.selfplay import SelfPlayRunner
    Game = importlib.import_module('alphazero_general_amd.envs.' + game).Game
    seed = 41
    r = SelfPlayRunner(Game, None, _args(gamesPerIteration=games), num_slots=B, seed=seed, warmup=True, fused_search=True)
    assert r.fused_search and r.round_graph and r.warmup
    ag = ol.OAgent(Game.AZG_GAME_ID, B, games_per_iteration=games, seed=seed, add_root_noise=True, add_root_temp=True, is_warmup=True, warmup_sims=5)
    rounds = 0
    pol = np.zeros((B, ag.gi.action_size), np.float32); val = np.zeros((B, ag.gi.num_players + 1), np.float32)
    while ag.games_played < games:
        ns = ag.begin_round()
        assert ns == 5
        for _ in range(ns):
            ag.generate_batch()
            ag.process_batch(pol, val)                             # (ignored: the oracle's warm-up agent makes its own constant rows)
        ag.play_moves()
        assert r.play_round() == ns
        assert (r.engine.last_actions().cpu().numpy() == ag.last_actions()).all(), rounds
        rounds += 1
    assert r.lanes[0].round_graphs                                # the rounds were graph replays of the raw launch
    c = r.counters()
    assert c['games_played'] == ag.games_played == games and c['sims'] == ag.sims_done and c['expansions'] == ag.expansions
    oo, op, oz = ag.samples()
    eo, ep, ez = [t.cpu().numpy() for t in r.samples()]
    assert eo.shape == oo.shape and eo.shape[0] > 0
    assert (eo == oo).all() and (ep == op).all() and (ez == oz).all()
    for x, y in zip(r.results(), ag.results()):
        assert (x == y).all()


# ---------------------------------------------------------------------------------------- 4. a captured graph keeps its constants
def test_search_raw_graph_replays_captured_constants():
    """the launch's rows are kernel arguments copied at the call: a captured graph replays them after the host arrays are gone"""
    import torch
    B, sims = 24, 7
    mk = lambda: _engine(C4, B, seed=9, sims_hint=sims, add_root_noise=True, add_root_temp=True, example_capacity=4096)
    ea, eb = mk(), mk()
    try:
        fill = np.float32(1 / 7)
        vrow = np.full(3, 1 / 3, np.float32)
        keep = vrow.copy()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):                                  # (capture executes nothing)
            ea.search_raw(sims, fill, vrow)
            ea.advance(True)
        vrow[:] = np.nan                                           # the caller's array is overwritten, then freed
        del vrow
        junk = [np.full(3, -7.0, np.float32) for _ in range(64)]   # (whatever reuses its memory)
        for rnd in range(3):
            g.replay()
            eb.search_raw(sims, float(fill), keep)
            eb.advance(True)
            assert torch.equal(ea.last_actions(), eb.last_actions()), rnd
            assert _snapshot(ea) == _snapshot(eb), rnd
        assert ea.counters()['sims'] == 3 * sims * B and len(junk) == 64
    finally:
        ea.close(); eb.close()


# ---------------------------------------------------------------------------------------- 5. errors
def test_search_raw_tree_store_overflow_is_reported():
    """a node store that is too small: the launch stops expanding, ends, and leaves the sticky error for the next counter read"""
    from alphazero_general_amd import _abi
    e = _engine(C4, 37, cpuct=4.0, fpu_reduction=0.4, seed=1, sims_hint=4, nodes_per_tree=48)
    e.search_raw(60, 1.0, np.zeros(3, np.float32))
    with pytest.raises(_abi.AzgError) as ei:
        e.counters()
    assert ei.value.code == _abi.E_TREE_FULL
    # ... and with the error standing the launch leaves the trees alone
    before = [(e.tree_info(i), e.root_children(i)['n'].tobytes()) for i in range(e.B)]
    ctr = e.tape_counters().copy()
    e.search_raw(5, 1.0, np.zeros(3, np.float32))
    assert [(e.tree_info(i), e.root_children(i)['n'].tobytes()) for i in range(e.B)] == before and (e.tape_counters() == ctr).all()
    e.close()
    e2 = _engine(C4, 37, cpuct=4.0, fpu_reduction=0.4, seed=1, sims_hint=60)      # the device is fine afterwards
    e2.search_raw(60, 1.0, np.zeros(3, np.float32))
    assert e2.counters()['sims'] == 37 * 60
    e2.close()


def test_search_raw_argument_errors():
    import ctypes as C
    from alphazero_general_amd import _abi
    e = _engine(C4, 4, seed=3, sims_hint=8)
    z = np.zeros(3, np.float32)
    e.search_raw(3, 1.0, z)
    before = _snapshot(e)
    e.search_raw(0, 1.0, z)                                        # nothing is launched, nothing changes
    assert _snapshot(e) == before
    for sims, row in ((-1, z), (2, None)):
        with pytest.raises(_abi.AzgError) as ei:
            e.search_raw(sims, 1.0, row)
        assert ei.value.code == _abi.E_INVALID_ARG
    assert _abi.lib().azg_search_raw(None, None, 1.0, z.ctypes.data_as(C.POINTER(C.c_float)), 1) == _abi.E_INVALID_ARG
    assert _snapshot(e) == before
    e.close()
    ar = _engine(C4, 4, arena=True, seed=3, sims_hint=8)
    with pytest.raises(_abi.AzgError) as ei:
        ar.search_raw(2, 1.0, z)
    assert ei.value.code == _abi.E_UNSUPPORTED
    ar.close()


def test_search_raw_zero_policy_is_a_floating_point_error():
    """policy_fill = 0: the masked policy sums to 0, what the reference turns into FloatingPointError (MCTS.pyx:23,245)"""
    e = _engine(C4, 5, seed=3, sims_hint=8)
    e.search_raw(4, 0.0, np.zeros(3, np.float32))
    with pytest.raises(FloatingPointError):
        e.counters()
    e.close()


# ---------------------------------------------------------------------------------------- 6. MCTS.raw_search, compat agent
def _margs(**kw):
    from alphazero_general_amd.utils import dotdict
    a = dotdict(cpuct=1.25, fpu_reduction=0.2, root_noise_frac=0.1, root_policy_temp=1.1, min_discount=1, _num_players=3, numMCTSSims=30,
                _azg_seed=515)
    a.update(kw)
    return a


# columns 0, 1, 5 and 6 filled, colours alternating upwards: nobody has won, three columns are left
FOUR_FULL_COLUMNS = [c for c in (0, 1, 5, 6) for _ in range(6)]


@pytest.mark.parametrize('nodes_per_tree,prefix', [(0, []), (200, FOUR_FULL_COLUMNS)])
def test_mcts_class_raw_search_vs_oracle_over_a_game(nodes_per_tree, prefix):
    """MCTS.raw_search move after move with update_root in between, against the oracle's.  The second case runs the chunking and
    _make_room: a store of 200 nodes is less than the 30 x 7 nodes the class must assume a move adds, so every move takes a forced
    compaction and more than one launch -- while the trees themselves fit, because with four columns full an expansion adds at
    most 3 nodes (a move's tree at most 90, the subtree kept from the move before less than that)."""
    from alphazero_general_amd.envs.connect4 import Game
    from alphazero_general_amd.MCTS import MCTS
    m = MCTS(_margs(_azg_nodes_per_tree=nodes_per_tree))
    om = ol.OMCTS(C4, seed=515, stream=0)
    g, og = Game(), ol.OGame(C4)
    for a in prefix:
        g.play_action(a); og.play(a)
    assert not og.win_state().any()
    launches = []
    for move in range(12):
        flags = (move % 2 == 1, move % 3 == 2)
        if move == 0:
            m._ensure(g)
            real = m._engine.search_raw
            m._engine.search_raw = lambda n, *a: (launches.append(n), real(n, *a))[1]
        m.raw_search(g, 30, *flags)
        om.raw_search(og, 30, *flags)
        assert (m.counts(g) == om.counts()).all(), move
        assert (m.probs(g, 1.0) == om.probs(1.0)).all(), move
        assert m.value() == om.value(False) and m.value(True) == om.value(True), move
        assert m.max_depth == om.max_depth and m.depth == ol.lib().azo_mcts_depth(om.h), move
        a = m.best_action(g)
        m.update_root(g, a); om.update_root(og, a)
        g.play_action(a); og.play(a)
        if og.win_state().any():
            break
    assert move >= (2 if prefix else 6) and sum(launches) == 30 * (move + 1)     # (three columns left: a short game)
    assert len(launches) == move + 1 if not nodes_per_tree else len(launches) >= 2 * (move + 1)
    m._engine.counters()                                          # no sticky error


def test_compat_warmup_agent_through_its_worker_vs_reference_golden():
    """the compat SelfPlayAgent in warm-up mode -- one `search_raw` worker call per round -- reproduces the reference's warm-up agent
    (tests/golden/c4_agent.npz 'warmup': samples in output_queue order, results in result_queue order)"""
    import threading
    import time
    import torch
    import torch.multiprocessing as mp
    from alphazero_general_amd.SelfPlayAgent import SelfPlayAgent
    from alphazero_general_amd.envs.connect4 import Game
    from alphazero_general_amd.utils import dotdict, default_temp_scaling
    d = dict(np.load(os.path.join(G, 'c4_agent.npz')))
    B, games, seed = int(d['warmup_B']), int(d['warmup_games']), int(d['warmup_seed'])
    assert int(d['warmup_slot_base']) == 0 and (d['warmup_round_sims'] == 5).all()
    torch.zeros(1, device='cuda:0')                               # the parent owns a HIP context before forking, like Coach
    args = dotdict(cpuct=1.25, fpu_reduction=0.2, root_noise_frac=0.1, root_policy_temp=1.1, min_discount=1, _num_players=3,
                   numMCTSSims=int(d['warmup_sims']), numFastSims=20, numWarmupSims=5, probFastSim=0.0, gamesPerIteration=games,
                   add_root_noise=False, add_root_temp=False, symmetricSamples=True, mctsResetThreshold=None, startTemp=1, arenaTemp=0.25,
                   temp_scaling_fn=default_temp_scaling, _azg_seed=seed)
    ready_queue, file_queue, result_queue = mp.Queue(), mp.Queue(), mp.Queue()
    completed, games_played = mp.Value('i', 0), mp.Value('i', 0)
    stop, pause = mp.Event(), mp.Event()
    inp, pol, val, ev = torch.zeros([B, 4, 6, 7]).share_memory_(), torch.zeros([B, 7]).share_memory_(), torch.zeros([B, 3]).share_memory_(), mp.Event()
    ag = SelfPlayAgent(0, Game, ready_queue, ev, inp, pol, val, file_queue, result_queue, completed, games_played, stop, pause, args,
                       _is_warmup=True)
    ag.daemon = True; ag.start()
    got, res = [], []
    done = threading.Event()

    def drainer():                                                # (both queues emptied on every pass; ends once told to and nothing is left)
        while True:
            idle = True
            for q_, out in ((file_queue, got), (result_queue, res)):
                try:
                    while True:
                        out.append(q_.get_nowait())
                        idle = False
                except queue.Empty:
                    pass
            if idle:
                if done.is_set():
                    return
                done.wait(0.02)
    th = threading.Thread(target=drainer); th.start()
    t0 = time.time()
    try:
        while completed.value != 1:                               # (a warm-up agent never asks the parent for an evaluation)
            assert time.time() - t0 < 300, 'the agent did not finish'
            time.sleep(0.02)
    finally:
        stop.set(); ag.join(30)                                   # (the agent flushes its queues before it exits)
        done.set(); th.join()
    assert games_played.value == games
    assert len(got) == d['warmup_s_obs'].shape[0]
    assert all((g_[0] == d['warmup_s_obs'][i]).all() and (g_[1] == d['warmup_s_pi'][i]).all() and (g_[2] == d['warmup_s_z'][i]).all()
               for i, g_ in enumerate(got))
    assert len(res) == len(d['warmup_r_ws'])
    assert all((ws == d['warmup_r_ws'][i]).all() and st.turns == d['warmup_r_turns'][i] and aid == 0 for i, (st, ws, aid) in enumerate(res))
