"""Gobang on the device (csrc/azg_games.h struct GB, game id 4: the first board of more than 64 cells) against fixtures the REFERENCE
produced (tests/golden/gb_*.npz, written by tests/golden/make_gobang_goldens.py from alphazero/envs/gobang) and the 15x15 network kernels
against the fp64 reference of tests/net_reference.py:

  * every gb_rules position through the engine ABI -- random playouts and the hand-built boards (overlines, fives on every edge and
    corner, full-board draws, both colours holding a five, fours that must not count): valid moves, win state, observation, and
    play_action by a steered second simulation;
  * the reference's MCTS (gb_tree: a root with up to 225 children, four chunks of 64) and SelfPlayAgent (gb_agent: plain, root
    temperature, fastmix -- raw samples with symmetricSamples=False are symmetries()[7]), per-phase and fused launches;
  * the MCTS class API on envs.gobang.Game against gb_tree;
  * the tower, head features, logits and probabilities of the 32-, 64- and 128-channel nets, every border class, depths 0 to 6;
  * NNetWrapper.process on the HIP tower driving the per-phase search; the persistent and sparse-head launches refuse gobang."""
import os

import numpy as np
import pytest
import torch

import fixture_checks as FC
import test_gpu_net_fp64 as F
import test_gpu_parity as P
from fixture_checks import crc

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
GB, DEV, A, NV = 4, 'cuda:0', 225, 3
NETS = ['gobang_32x4', 'gobang_64x4', 'gobang_128x8']   # test_gpu_net_fp64.GAME_NETS: reference / wrapper / check_network there


def _game():
    from alphazero_general_amd.envs.gobang import Game
    return Game


# ------------------------------------------------------------------------------------------------------------------------- rules
def test_gb_rules_vs_reference_tables():
    from alphazero_general_amd import _abi
    from alphazero_general_amd.engine import DeviceEngine
    d = dict(np.load(os.path.join(G, 'gb_rules.npz')))
    board = np.array([_abi.gobang_unpack(c.tobytes()) for c in d['cells']])
    n, lens, ws = len(d['lens']), d['lens'], d['ws']
    assert n >= 10250 and (lens < 0).sum() >= 250
    eng = DeviceEngine(GB, n, seed=3, sims_hint=4, cpuct=1.25, fpu_reduction=0.2, nodes_per_tree=1024)
    eng.set_states([(board[i], int(d['player'][i]), int(d['turns'][i])) for i in range(n)])
    back = eng.get_states()
    assert all((back[i][0] == board[i]).all() and back[i][1] == d['player'][i] and back[i][2] == d['turns'][i] for i in range(n))
    obs = eng.new_obs()
    eng.select(obs)                                           # find_leaf at a fresh root: win_state, valid_moves, add_children, observation
    o = obs.cpu().numpy()
    bad = [i for i in range(n) if crc(o[i]) != d['obs_crc'][i]]
    assert not bad, ('observation', bad[:5])
    for i in range(n):
        ch = eng.root_children(i)
        v = np.zeros(A, np.uint8); v[ch['a']] = 1
        assert len(ch['a']) == v.sum() and crc(v) == d['valid_crc'][i], ('valid_moves', i)
        e = eng.tree_info(i)['e']
        assert e == int(ws[i][0]) + 2 * int(ws[i][1]) + 4 * int(ws[i][2]), ('win_state', i, e, ws[i])
    # one backup with a policy peaked on the playout's next move, then the second simulation descends exactly that ply
    nxt = d['next'].astype(np.int64)
    has_next = (nxt >= 0) & (lens >= 0)
    has_next[-1] = False
    pol = np.full((n, A), 1e-4, np.float32)
    pol[np.arange(n), np.where(has_next, nxt, 0)] = 0.9
    val = np.full((n, NV), 1.0 / 3, np.float32)
    eng.backup(torch.from_numpy(pol).to(eng.device), torch.from_numpy(val).to(eng.device))
    eng.select(obs)
    o = obs.cpu().numpy()
    leaves = eng.get_leaf_states()
    for i in range(n):
        lc, lp, lt = leaves[i]
        if ws[i].any():                                       # terminal root: find_leaf stops at it
            assert len(eng.last_path(i)) == 0 and (lc == board[i]).all(), ('terminal', i)
            continue
        if not has_next[i]:
            continue
        assert list(eng.last_path(i)) == [nxt[i]], ('descent', i)
        assert (lc == board[i + 1]).all(), ('play_action: board', i)
        assert lp == d['player'][i + 1] and lt == d['turns'][i + 1], ('play_action: player / turns', i)
        assert crc(o[i]) == d['obs_crc'][i + 1], ('observation after play_action', i)
    eng.close()


# ------------------------------------------------------------------------------------------------------------------------- tree / agent
@pytest.mark.parametrize('fixture,cname', [('gb_tree', 'default'), ('gb_tree', 'cpuct4'), ('gb_tree', 'temp'), ('gb_noise_tree', 'noise_temp')])
def test_gb_tree_vs_reference_goldens(fixture, cname):
    """gb_noise_tree: root noise over 225 children (four chunks), the reference run with its float32 underflow trap off"""
    d = FC.load(fixture)
    traces = FC.check_tree(GB, d, cname, FC.states_from_prefix(_game(), d['prefix']), FC.TREE, 'gb')
    assert all(len(a) > 64 for t in traces for a in t['a'])  # (the fixture keeps the first 128 children of a root in list order)


AGENT = {'plain': (dict(), dict()),
         'temp': (dict(add_root_temp=True, cpuct=4.0, fpu_reduction=0.4), dict()),
         'fastmix': (dict(symmetric_samples=False), dict(prob_fast=0.5, fast_sims=3))}


@pytest.mark.parametrize('launch', P.LAUNCHES)
@pytest.mark.parametrize('cname', list(AGENT))
def test_gb_agent_vs_reference_goldens(cname, launch):
    kw, rnd = AGENT[cname]
    FC.check_agent(GB, FC.load('gb_agent'), cname + '_', launch, 'gb', engine_kw=dict(kw, example_capacity=8192), **rnd)


def test_gb_mcts_class_api_vs_reference_goldens():
    """alphazero_general_amd.MCTS on an envs.gobang.Game object (one slot: the tape stream of gb_tree's root 0), find_leaf /
    process_results fed the fixture's evaluations, must build the reference's tree: depths, counts, values, probabilities"""
    FC.check_mcts_class(_game(), FC.load('gb_tree'), A, NV, game='gb')


# ------------------------------------------------------------------------------------------------------------------------- network
@pytest.mark.parametrize('key', list(NETS))
def test_gb_network_vs_fp64(key):
    args, sd, ref, x, o = F.reference(key)
    F.check_network(key, key, args, sd, ref, x, o, [1, 37, 301, 2 * F._cus() + 1])   # (one board per tile at every batch size)


@pytest.mark.parametrize('depth', [0, 1, 2, 6])
@pytest.mark.parametrize('key', ['gobang_32x4', 'gobang_64x4'])
def test_gb_network_depths_vs_fp64(key, depth):
    args, sd, ref, x, o = F.reference(key, depth=depth)
    F.check_network('%s_depth%d' % (key, depth), key, args, sd, ref, x, o, [37, 301])


# ------------------------------------------------------------------------------------------------------------------------- search
def _net(key, salt=7):
    args, sd, ref, x, o = F.reference(key, salt=salt)
    return F.wrapper(key, args, sd)


@pytest.mark.parametrize('key', ['gobang_32x4', 'gobang_64x4'])
def test_gb_phase_search_on_the_hip_tower(key):
    """NNetWrapper.process (the HIP tower) drives select / backup / advance for a few moves; the engine's leaf observations are the
    host env's, and every move played is legal and lands where the host env puts it.  The sparse heads refuse gobang cleanly."""
    from alphazero_general_amd.engine import DeviceEngine
    net = _net(key)
    assert net._hip.can_search
    Game = _game()
    B, sims, moves = 256, 24, 3
    eng = DeviceEngine(GB, B, cpuct=2.0, fpu_reduction=0.1, add_root_temp=True, seed=41, games_per_iteration=1 << 30,
                       example_capacity=B * (moves + 1) * 8, sims_hint=sims)
    oc = eng.new_obs(torch.float32)
    for mv in range(moves):
        before = [Game.from_azg_state(*s) for s in eng.get_states()]
        for s in range(sims):
            eng.select(oc)
            if s == 0:
                for i, lf in enumerate(eng.get_leaf_states()[:16]):
                    assert (oc[i].cpu().numpy() == Game.from_azg_state(*lf).observation()).all()
            p, v = net.process(oc)
            eng.backup(p.contiguous(), v.contiguous())
        eng.advance(True)
        acts = eng.last_actions().cpu().numpy()
        after = eng.get_states()
        for i in range(B):
            g = before[i]
            assert g.valid_moves()[acts[i]] == 1
            g.play_action(int(acts[i]))
            assert (after[i][0] == g._board.pieces.reshape(-1)).all() and after[i][1] == g.player and after[i][2] == g.turns
    obs, pi, z = eng.examples()
    assert obs.shape[1:] == (4, 15, 15) and pi.shape[1] == A and obs.shape[0] == 0 == eng.counters()['games_played']   # (samples: at game end)
    hip = net._hip
    feat = hip.forward_features_nhwc8(hip.to_nhwc8(oc))
    with pytest.raises(Exception) as ei:
        eng.backup_select_features(feat, hip.head_rows, hip.head2_b, oc, select=True)
    assert 'UNSUPPORTED' in str(ei.value) or 'sparse' in str(ei.value)
    with pytest.raises(Exception) as ei:
        hip.search(eng, sims, exact=False)                   # the sparse persistent launch
    assert 'UNSUPPORTED' in str(ei.value) or 'sparse' in str(ei.value)
    eng.close()


@pytest.mark.parametrize('key,B,sims,moves', [('gobang_32x4', 768, 60, 3), ('gobang_64x4', 768, 60, 3), ('gobang_64x4', 40, 30, 4)])
def test_gb_wide_exact_search_vs_phase_loop(key, B, sims, moves):
    """azg_search_wide_exact_f16 (one game per workgroup; 227-level paths through the game-sized walk mailbox) against select ->
    NNetWrapper.process -> backup on a twin engine with the same seeds: counts, probabilities, values, moves, samples, results"""
    net = _net(key)
    FC.twin_moves(GB, B, lambda ea: net._hip.search(ea, sims, exact=True), lambda ec, oc: net.process(oc), sims, moves,
                  cpuct=4.0, fpu_reduction=0.4, add_root_noise=True, add_root_temp=True, seed=41)


def _deep_path(net):
    """64 positions 180 or more plies in, 120 simulations: the persistent launch's root counts and deepest path equal the per-phase loop's"""
    Game = _game()
    rng = np.random.RandomState(11)
    states = []
    while len(states) < 64:
        g = Game()
        for a in rng.permutation(A)[:200]:
            g2 = g.clone(); g2.play_action(int(a))
            if g2.win_state().any():
                continue
            g = g2
        if g.turns >= 180:
            states.append(g.to_azg_state())
    from alphazero_general_amd.engine import DeviceEngine
    sims = 120
    kw = dict(cpuct=4.0, fpu_reduction=0.4, seed=17, games_per_iteration=1 << 30, example_capacity=1 << 14, sims_hint=sims)
    ea, ec = DeviceEngine(GB, 64, **kw), DeviceEngine(GB, 64, **kw)
    ea.set_states(states); ec.set_states(states)
    net._hip.search(ea, sims, exact=True)
    FC.phase_loop(ec, lambda ec, oc: net.process(oc), sims, ec.new_obs(torch.float32))
    FC.assert_engines_equal(ea, ec, ('counts',))             # (one search, no move: this test is about the walk)
    depth = max(ea.tree_info(i)['max_depth'] for i in range(64))
    assert depth >= 3 and depth == max(ec.tree_info(i)['max_depth'] for i in range(64))
    ea.close(); ec.close()


def test_gb_wide_search_deep_path():
    """positions about 200 plies in: the walks of the persistent launch reach terminal leaves and full boards (wins, draws at turn 225)
    through the game-sized walk mailbox, still equal to the per-phase loop"""
    _deep_path(_net('gobang_64x4'))


def _flat_net(key, salt=7):
    """the trained weights with the last Linear of both heads zeroed: every logit is 0, so every prior is the same after
    masking and every value row is uniform -- PUCT ties at every node"""
    args, sd, ref, x, o = F.reference(key, salt=salt)
    sd = {k: (torch.zeros_like(v) if k.rsplit('.', 1)[0] in ('pi_fc.4', 'v_fc.4') else v) for k, v in sd.items()}
    assert sum(1 for k in sd if k.rsplit('.', 1)[0] in ('pi_fc.4', 'v_fc.4')) == 4
    return F.wrapper(key, args, sd)


def _sparse_draw_states(ks, per_k, seed):
    """per k, `per_k` positions with exactly k legal moves and no five: a full board of the two-on two-off draw pattern
    (make_gobang_goldens.built_boards) with k random stones taken off -- taking stones off cannot make a five"""
    Game = _game()
    rng = np.random.RandomState(seed)
    x, y = np.meshgrid(np.arange(15), np.arange(15), indexing='ij')
    full = np.where((y // 2 + x) % 2 == 0, 1, -1).astype(np.int8).reshape(-1)
    out = []
    for k in ks:
        for _ in range(per_k):
            c = full.copy()
            c[rng.choice(A, k, replace=False)] = 0
            g = Game.from_azg_state(c, (A - k) % 2, A - k)
            assert not g.win_state().any() and int(g.valid_moves().sum()) == k
            out.append(g.to_azg_state())
    return out


def test_gb_wide_exact_search_at_exact_ties():
    """the persistent launch (azg_search_wide_exact_f16) where every PUCT comparison ties: a flat network (all logits 0) on roots
    of 225, 193, 129, 128, 66, 65, 64 and 30 legal moves -- first maxima out of ties that span chunks of 64 children, the switch
    to the one-chunk templates inside a descent -- against the per-phase loop on a twin engine (which tests/test_gpu_tree_edges.py
    holds to the reference at the same edges).  Root noise and temperature off."""
    from alphazero_general_amd.engine import DeviceEngine
    net = _flat_net('gobang_64x4')
    ks, per_k, sims, moves = (225, 193, 129, 128, 66, 65, 64, 30), 6, 80, 2
    B = len(ks) * per_k
    assert B == 48
    states = _sparse_draw_states(ks, per_k, 23)
    ep = DeviceEngine(GB, B, seed=43)                       # (an engine of its own: the twins' tapes stay in step)
    ep.set_states(states)
    oc = ep.new_obs(torch.float32)
    ep.select(oc)
    p, v = net.process(oc)                                  # the network really ties: every row's entries are equal bit for bit
    ep.close()
    assert p.shape == (B, A) and v.shape == (B, NV)
    assert bool((p == p[:, :1]).all()) and bool((v == v[:, :1]).all()) and bool((p > 0).all())
    wide = []

    def spread(ea, ec, mv):
        assert mv > 0 or int(ea.root_counts().sum()) == B * (sims - 1)         # (later moves search on in the kept subtree)
        wide.extend(int((ea.root_children(i)['n'][64:] > 0).sum()) for i in range(B))    # visits landed on list indices past the first chunk
    FC.twin_moves(GB, B, lambda ea: net._hip.search(ea, sims, exact=True), lambda ec, oc: net.process(oc), sims, moves, states,
                  each_move=spread, cpuct=1.25, fpu_reduction=-1.0, seed=43)
    assert sum(wide) > 0


# ------------------------------------------------------------------------------------------------------------------------- arena
def _arena_nets(width, n, seed0=20):
    from alphazero_general_amd import nnet as N
    from alphazero_general_amd.utils import dotdict
    na = dotdict(dict(N.DEFAULT_NET_ARGS, num_channels=width))
    out = []
    for m in range(n):
        torch.manual_seed(seed0 + m)
        w = N.NNetWrapper(_game(), na, device=DEV, dtype=torch.float16)
        w.refresh()
        out.append(w)
    return out


def _arena_replay(runs, B):
    """every slot's games replayed on envs.gobang from the actions of every round: each move legal, each finished game's win state and
    length the engine's result record"""
    Game = _game()
    acts, _, (ws, turns, slot), _ = runs
    games = [Game() for _ in range(B)]
    done = [[] for _ in range(B)]
    for row in acts:
        for i, a in enumerate(row):
            if a < 0:
                continue
            g = games[i]
            assert g.valid_moves()[a] == 1, (i, a)
            g.play_action(int(a))
            w = g.win_state()
            if w.any():
                done[i].append((tuple(int(x) for x in w), g.turns))
                games[i] = Game()
    for i in range(B):
        rec = [(tuple(int(x) for x in ws[j]), int(turns[j])) for j in range(len(slot)) if slot[j] == i]
        assert rec == done[i][:len(rec)] and len(rec) >= len(done[i]) - 1, i
    assert sum(len(d) for d in done) > 0


@pytest.mark.parametrize('raw', [False, True])
@pytest.mark.parametrize('width', [32, 64])
def test_gb_persistent_arena_equals_host_split(width, raw):
    """two differently seeded nets, or a net against a raw seat (RawMCTSPlayer: policy float32(1 / 225), value zeros): the persistent
    arena launch, captured and eager, plays exactly the games of the host-split path, and the games replay on the host env"""
    import test_gpu_arena_wide as W
    nets = _arena_nets(width, 1 if raw else 2)
    seats = nets + [None] if raw else nets
    B = 24
    runs = W._forms(_game(), seats, W._args(), B, 7 if raw else 5, 'slot' if raw else 'agent', 150)
    W._same(runs)
    _arena_replay(runs[0], B)


def test_gb_default_routing_takes_the_faster_form():
    """fused_search=None: gobang's persistent launch measured slower than the per-phase loop (profiles/gobang_throughput.json), so the
    self-play and arena runners take the per-phase form by default and the persistent one only when asked"""
    from alphazero_general_amd.selfplay import ArenaRunner, SelfPlayRunner
    import test_gpu_arena_wide as W
    nets = _arena_nets(32, 2)
    assert nets[0]._hip.can_search and not nets[0]._hip.search_preferred
    args = W._args()
    r = SelfPlayRunner(_game(), nets[0], args, num_slots=8, seed=3)
    assert not r.fused_search
    r.engine.close()
    r = SelfPlayRunner(_game(), nets[0], args, num_slots=8, seed=3, fused_search=True)
    assert r.fused_search
    r.engine.close()
    a = ArenaRunner(_game(), nets, args, num_slots=8, seed=3, use_graph=False)
    assert not a.wide_search
    a.engine.close()
