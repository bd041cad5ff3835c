"""Tic-tac-toe on the device (csrc/azg_games.h struct TT, game id 5) against fixtures the REFERENCE produced (tests/golden/tt_*.npz, written
by tests/golden/make_tictactoe_goldens.py from alphazero/envs/tictactoe) and the 3x3 network kernels against the fp64 reference of
tests/net_reference.py:

  * ALL 39 366 records of tt_rules (every board x both movers, unreachable ones included) through the engine ABI: valid moves, win state,
    observation, and EVERY legal move of every undecided record by a steered second simulation (test_gpu_rules._check_records);
  * the reference's MCTS (tt_tree: random and uniform priors; tt_edge -- exact ties, zero and denormal priors, roots of one and two legal
    moves -- is the `tt` name of tests/test_gpu_tree_edges.py), both per-phase launch forms; SelfPlayAgent (tt_agent: raw and symmetric
    samples, fast rounds, warm-up -- at a temperature that never steps: max_turns() is None) and a whole agent under np.random.seed(s)
    (tt_mt19937_agent) -- all through tests/fixture_checks.py;
  * the tower, head features with their zero padding, logits and probabilities of the default 32 x 4 net (16 + 16 head channels) and of
    TICTACTOE_NET_ARGS (4 + 4, padded) at every tower tile -- one, five and sixteen boards -- and their ragged last tiles;
  * azg_search_wide_exact_f16, azg_search_arena_wide_exact_f16 and azg_search_raw against the launch-per-phase loops, bit for bit;
  * the MCTS class API with pickling, the launch mask against the launches, one self-play iteration and one arena through the runners."""
import ctypes as C

import numpy as np
import pytest
import torch

import edge_eval as ee
import fixture_checks as FC
import net_reference as R
import test_gpu_arena_wide as AW
import test_gpu_net_fp64 as F
import test_gpu_parity as P
import test_gpu_raw_search as RS
import test_gpu_rules as GR

pytestmark = pytest.mark.gpu
TT, DEV, A, NV = 5, 'cuda:0', 9, 3
NETS = ['tictactoe_32x4_h4', 'tictactoe_32x4']       # test_gpu_net_fp64.GAME_NETS: reference / wrapper / check_network there


def _game():
    from alphazero_general_amd.envs.tictactoe import Game
    return Game


# ------------------------------------------------------------------------------------------------------------------------- rules
@pytest.mark.parametrize('mover', [0, 1])
@pytest.mark.parametrize('k', range(9))
def test_tt_rules_every_state_every_move(k, mover):
    """pass k plays the k-th legal move of every undecided record of `mover` that has one (pass 0 also holds every record's valid moves,
    win state and observation: all 19 683 boards per mover); the successor of (record, action) is the record the reference's
    play_action led to"""
    import test_tictactoe_cpu as TC
    d = TC.rules()
    n = len(d['player'])
    crc = np.array([GR.crc(o.astype(np.float32).reshape(1, 3, 3)) for o in d['obs']], np.uint32)
    nleg = d['valids'].sum(1)
    live = ~d['ws'].any(1) & (nleg > k) & (d['player'] == mover)
    rec = np.flatnonzero(d['player'] == mover) if k == 0 else np.flatnonzero(live)
    action = np.full(len(rec), -1, np.int64)
    for j, r in enumerate(rec):
        if live[r]:
            action[j] = np.flatnonzero(d['valids'][r])[k]
    succ_rec = np.array([d['succ'][r, a] if a >= 0 else -1 for r, a in zip(rec, action)])
    extra = np.unique(succ_rec[succ_rec >= 0])
    allrec = np.concatenate([rec, extra])
    pos = {int(r): len(rec) + j for j, r in enumerate(extra)}
    succ = np.array([pos[int(s)] if s >= 0 else -1 for s in succ_rec] + [-1] * len(extra))
    action = np.concatenate([action, np.full(len(extra), -1, np.int64)])
    got = GR._check_records(torch, TT, d['cells'][allrec], d['player'][allrec], d['turns'][allrec], None, d['valids'][allrec], d['ws'][allrec],
                            crc[allrec], action, succ)
    assert got == int(live.sum()) and (k > 0 or len(rec) == 3 ** 9)
    assert k >= 8 or got > 0


# ------------------------------------------------------------------------------------------------------------------------- tree
TREE_CONFIGS = ['default', 'cpuct2', 'noise', 'noise_temp', 'uniform', 'uniform_noise_temp']


@pytest.mark.parametrize('cname', TREE_CONFIGS)
def test_tt_tree_vs_reference_goldens(cname):
    d = FC.load('tt_tree')
    R_, sims, seed = d['prefix'].shape[0], int(d[cname + '_cfg'][4]), int(d[cname + '_seed'])
    assert 4 <= R_ <= 16 and 8 <= sims <= 30 and d['prob_temps'].tolist() == [1.0, 0.5, 0.25, float(np.float32(0.2)), 0.0]

    def uniform_rows(s):                                       # (make_tictactoe_goldens.uniform_eval: float32(1) / float32(9), the random value row)
        return np.full((R_, A), np.float32(1.0) / np.float32(A), np.float32), FC.fake_rows(seed, range(R_), s, A, NV)[1]
    FC.check_tree(TT, d, cname, FC.states_from_prefix(_game(), d['prefix']), FC.TREE, 'tt', uniform_rows if cname.startswith('uniform') else None)


def _edge_roots():
    return ee.roots(FC.load('tt_edge'), TT)


# ------------------------------------------------------------------------------------------------------------------------- agent
AGENT = {'plain': (dict(symmetric_samples=False), dict()),
         'symmetric': (dict(add_root_noise=True, add_root_temp=True, cpuct=2.0), dict()),
         'fastmix': (dict(symmetric_samples=False), dict(prob_fast=0.5, fast_sims=4)),
         'warmup': (dict(), dict(warmup=True, warmup_sims=5))}


@pytest.mark.parametrize('launch', P.LAUNCHES)
@pytest.mark.parametrize('cname', list(AGENT))
def test_tt_agent_vs_reference_goldens(cname, launch):
    """whole reference SelfPlayAgent runs, move for move and sample for sample.  The engine's DEFAULT temperature schedule is used: the
    fixture's moves are those of a temperature that stays at startTemp (the generator asserted that a schedule halving after every move
    -- what azg_game_info.max_turns = 9 would give -- samples other moves from round `<config>_halving_differs_at` on)"""
    d = FC.load('tt_agent')
    kw, rnd = AGENT[cname]

    def default_schedule(eng):
        assert 4 <= eng.B <= 8 and (eng._tt == np.float32(1.0)).all() and len(eng._tt) == 11
    rec = FC.check_agent(TT, d, cname + '_', launch, 'tt', engine_kw=dict(kw, example_capacity=4096), before=default_schedule, **rnd)
    if cname in ('plain', 'symmetric'):
        assert int(d[cname + '_halving_differs_at']) < len(rec['actions'])


@pytest.mark.parametrize('launch', P.LAUNCHES)
def test_tt_selfplay_agent_under_numpys_mt19937_seed(launch):
    FC.check_mt19937_agent(TT, FC.load('tt_mt19937_agent'), launch, 'tt')


def test_tt_mcts_class_api_vs_reference_goldens_with_pickling():
    """alphazero_general_amd.MCTS on an envs.tictactoe.Game object (one slot: the tape stream of tt_tree's root 0 -- the empty board),
    find_leaf / process_results fed the fixture's evaluations, pickled and restored half way, must build the reference's tree"""
    d = FC.load('tt_tree')
    m, g = FC.check_mcts_class(_game(), d, A, NV, pickle_at=int(d['default_cfg'][4]) // 2, game='tt')
    a = m.best_action(g)
    m.update_root(g, a)
    g.play_action(a)
    assert int(np.asarray(m.counts(g)).sum()) > 0


# ------------------------------------------------------------------------------------------------------------------------- network
@pytest.mark.parametrize('key', list(NETS))
def test_tt_network_every_tile_vs_fp64(key):
    """the one-board tile at 1, 2, 16, 17, 33 boards; the five-board tile from 8 boards per CU + 1 (a ragged last tile, as + 2 ... + 5 are
    whole or ragged in turn); the sixteen-board tile from 80 per CU + 1 and at + 17, + 33 (one and two whole tiles more, ragged)"""
    args, sd, ref, x, o = F.reference(key)
    cus = F._cus()
    sizes = [1, 2, 16, 17, 33, 8 * cus, 8 * cus + 1, 8 * cus + 5, 8 * cus + 6, 80 * cus, 80 * cus + 1, 80 * cus + 16, 80 * cus + 17, 80 * cus + 33]
    assert {F.tile_boards('tictactoe', 32, n, cus) for n in sizes} == {1, 5, 16}
    F.check_network(key, key, args, sd, ref, x, o, sizes)


@pytest.mark.parametrize('depth', [1, 6])
@pytest.mark.parametrize('key', list(NETS))
def test_tt_network_depths_vs_fp64(key, depth):
    args, sd, ref, x, o = F.reference(key, depth=depth)
    cus = F._cus()
    F.check_network('%s_depth%d' % (key, depth), key, args, sd, ref, x, o, [17, 8 * cus + 1, 80 * cus + 17])


# ------------------------------------------------------------------------------------------------------------------------- search launches
def _net(key, salt=7):
    args, sd, ref, x, o = F.reference(key, salt=salt)
    return F.wrapper(key, args, sd)


def _twin_search(net, B, sims, moves, states=None, **kw):
    """azg_search_wide_exact_f16 against select -> NNetWrapper.process -> backup on a twin engine with the same seeds: every slot's counts,
    probabilities, values, moves, samples and results identical"""
    tile = []
    ca, _ = FC.twin_moves(TT, B, lambda ea: net._hip.search(ea, sims, exact=True), lambda ec, oc: net.process(oc), sims, moves, states,
                          each_move=lambda ea, ec, mv: tile.append(net._hip.search_tile(ea, exact=True)), **dict(dict(seed=41), **kw))
    assert ca['sims'] == B * sims * moves
    return tile[-1]


@pytest.mark.parametrize('B', [1, 2, 3, 'wide'])
@pytest.mark.parametrize('key', list(NETS))
def test_tt_wide_exact_search_vs_phase_loop(key, B, capsys):
    """slots = 1, the tile sizes 1 and 2 and one more than each (1, 2, 3): the one-game tile's helper wavefront and pixel groups 2, 3 of
    the two-game tile own no subtile, and an odd engine leaves the last two-game tile one game short.  Which tile a launch takes is the
    set-up's choice (azg_search_wide_tile_info); 'wide' is an odd engine past two games per CU, where the tile model's prior is the
    two-game tile"""
    n = 2 * F._cus() + 3 if B == 'wide' else B
    tile = _twin_search(_net(key), n, 16, 3, cpuct=2.0, fpu_reduction=0.2, add_root_noise=True, add_root_temp=True)
    assert tile is not None and tile['games_per_workgroup'] in (1, 2)
    with capsys.disabled():
        print('tictactoe %s, %d slots: %d game(s) per workgroup (%s)' % (key, n, tile['games_per_workgroup'], tile['source']))


@pytest.mark.parametrize('key', list(NETS))
def test_tt_wide_exact_search_at_exact_ties_from_the_edge_roots(key):
    """the persistent launch where every PUCT comparison ties: the trained fill with the last Linear of both heads zeroed, so every logit
    is 0, every prior the same after masking and every value row uniform -- on the roots of tt_edge.npz (one and two legal moves among
    them), against the per-phase loop on a twin engine.  Root noise and temperature off."""
    from alphazero_general_amd.engine import DeviceEngine
    args, sd, ref, x, o = F.reference(key, salt=7)
    last = ['%s.%d' % (h, max(int(k.split('.')[1]) for k in sd if k.startswith(h + '.'))) for h in ('pi_fc', 'v_fc')]
    sd = {k: (torch.zeros_like(v) if k.rsplit('.', 1)[0] in last else v) for k, v in sd.items()}
    assert sum(1 for k in sd if k.rsplit('.', 1)[0] in last) == 4
    net = F.wrapper(key, args, sd)
    roots = _edge_roots()
    states = [g.to_azg_state() for g in roots]
    ep = DeviceEngine(TT, len(states), seed=47)
    ep.set_states(states)
    oc = ep.new_obs(torch.float32)
    ep.select(oc)
    p, v = net.process(oc)                                  # the network really ties: every row's entries are equal bit for bit
    ep.close()
    assert p.shape == (len(states), A) and bool((p == p[:, :1]).all()) and bool((v == v[:, :1]).all()) and bool((p > 0).all())
    _twin_search(net, len(states), 16, 3, states=states, seed=47, cpuct=1.25, fpu_reduction=-1.0)


def _tt_nets(n, key='tictactoe_32x4_h4', seed0=20):
    from alphazero_general_amd import nnet as N
    na = R.net_args(F.GAME_NETS[key][1])
    out = []
    for m in range(n):
        torch.manual_seed(seed0 + m)
        w = N.NNetWrapper(_game(), na, device=DEV, dtype=torch.float16)
        w.refresh()
        out.append(w)
    return out


@pytest.mark.parametrize('raw', [False, True])
@pytest.mark.parametrize('B', [2, 5])
def test_tt_wide_arena_equals_host_split(B, raw):
    """azg_search_arena_wide_exact_f16 (graph-captured and eager) plays exactly the games the host-split arena plays, two nets or a net
    and a raw seat; slot 0's first game is replayed on the host env: every move legal, the game over exactly at its last move, the
    recorded result the host's win state"""
    nets = _tt_nets(1 if raw else 2)
    seats = nets + [None] if raw else nets
    runs = AW._forms(_game(), seats, AW._args(), B, 5 + B, 'slot', 15)
    AW._same(runs)
    acts, _, (ws, turns, slot), _ = runs[0]
    first = int(np.flatnonzero(slot == 0)[0])
    g = _game()()
    for rnd in range(int(turns[first])):
        a = int(acts[rnd][0])
        assert not g.win_state().any() and g.valid_moves()[a] == 1, rnd
        g.play_action(a)
    assert g.turns == turns[first] and g.win_state().any() and (g.win_state() == ws[first]).all()


@pytest.mark.parametrize('consts', [RS.RAW, RS.WARM])
@pytest.mark.parametrize('B', [1, 3, 64])
def test_tt_search_raw_equals_per_phase_loop(B, consts):
    sims, rounds = 20, 12
    mk = lambda: RS._engine(TT, B, seed=36, sims_hint=sims, add_root_noise=True, add_root_temp=True, cpuct=4.0, fpu_reduction=0.4,
                            example_capacity=B * (rounds + 1) * 8)
    ea, eb = mk(), mk()
    try:
        fill, vrow = RS._rows(ea, consts)
        pol = torch.full((B, A), fill, dtype=torch.float32, device=eb.device)
        val = torch.from_numpy(np.tile(vrow, (B, 1))).to(eb.device)
        for rnd in range(rounds):
            ea.search_raw(sims, fill, vrow)
            for _ in range(sims):
                eb.select(None)
                eb.backup(pol, val)
            assert RS._snapshot(ea) == RS._snapshot(eb), rnd
            ea.advance(True); eb.advance(True)
            assert torch.equal(ea.last_actions(), eb.last_actions()), rnd
        ca, cb = ea.counters(), eb.counters()
        assert ca == cb and ca['sims'] == B * sims * rounds and ca['games_played'] >= B      # games ended and restarted
        for x, y in zip(ea.examples(), eb.examples()):
            assert torch.equal(x, y)
        for x, y in zip(ea.results(), eb.results()):
            assert (x == y).all()
    finally:
        ea.close(); eb.close()


@pytest.mark.parametrize('ch', [32, 64, 128])
def test_tt_launches_exist_exactly_where_the_mask_says(ch):
    """tests/test_gpu_launch_support.py's check for game id 5: the set-up call of the persistent launch (exact; sparse: never -- the mask
    has no sparse bit for this game) and a stand-alone tower launch succeed exactly where azg_launch_support has their bit"""
    from alphazero_general_amd import _abi, nnet as N
    from alphazero_general_amd.engine import DeviceEngine
    from alphazero_general_amd.utils import dotdict
    L = _abi.lib()
    mask = _abi.launch_support(TT, ch)                         # (the library refuses every width but 32 for this game: read as no launch)
    assert mask == (_abi.SUPPORT_TOWER | _abi.SUPPORT_SEARCH_WIDE if ch == 32 else 0)
    assert L.azg_launch_support(TT, ch) == (mask if ch == 32 else _abi.E_UNSUPPORTED)
    torch.manual_seed(3)
    na = dotdict(dict(N.TICTACTOE_NET_ARGS)); na['num_channels'] = ch; na['depth'] = 1
    w = N.NNetWrapper(_game(), na, device=DEV, dtype=torch.float16, backend='torch')
    h = N.HipResNet(N.FoldedResNet(w.nnet).to(DEV), TT, DEV)
    assert (h.fact_head and h.feat_k == 160) or (ch == 128 and h.fused_head)    # (12 outputs fuse behind a 128-channel tower: no factorised operands)
    dummy = torch.zeros(64, device=DEV)
    vp = lambda t: C.c_void_p(t.data_ptr())
    op = lambda a: vp(getattr(h, a, dummy))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    tower = (vp(h.tower_w), vp(h.tower_b), vp(h.tower_ps), vp(h.tower_pt))
    want = lambda bit: 0 if mask & bit else _abi.E_UNSUPPORTED
    e = DeviceEngine(TT, 2)
    try:
        assert L.azg_search_wide_exact_f16(e.h, st, *tower, 1, ch, op('head1_w'), op('head1_b'), op('head2_wps'), op('head2_wv'), op('head2_b'),
                                           160, 0) == want(_abi.SUPPORT_SEARCH_WIDE)
        assert L.azg_search_wide_f16(e.h, st, *tower, 1, ch, op('head1_w'), op('head1_b'), op('head_rows'), op('head2_b'), 160, 0) == _abi.E_UNSUPPORTED
        x = torch.zeros((2, 9, 8), dtype=torch.float16, device=DEV)
        y = torch.empty((2 * 9, ch), dtype=torch.float16, device=DEV)
        assert L.azg_resnet_tower_f16(st, TT, vp(x), *tower, vp(y), 2, 1, ch) == want(_abi.SUPPORT_TOWER)
        feat = torch.zeros((2, 2 * 160), dtype=torch.float16, device=DEV)
        lg = torch.zeros((2, 16), dtype=torch.float32, device=DEV)
        assert L.azg_leaf_heads_sparse_f16(e.h, st, vp(feat), 160, op('head_rows'), op('head2_b'), None, vp(lg), 16) == _abi.E_UNSUPPORTED
        torch.cuda.synchronize()
        e.counters()
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------------------------------- runners
def _run_args(**kw):
    from alphazero_general_amd.nnet import TICTACTOE_NET_ARGS
    from alphazero_general_amd.utils import dotdict, default_temp_scaling
    a = dotdict(TICTACTOE_NET_ARGS)
    a.update(numMCTSSims=12, numFastSims=4, numWarmupSims=5, probFastSim=0.5, gamesPerIteration=32, cpuct=2.0, fpu_reduction=0.2,
             root_noise_frac=0.25, root_policy_temp=1.1, min_discount=1.0, add_root_noise=True, add_root_temp=True, symmetricSamples=True,
             mctsResetThreshold=None, startTemp=1.0, arenaTemp=0.25, temp_scaling_fn=default_temp_scaling, use_draws_for_winrate=True,
             model_gating=False, workers=2, process_batch_size=16, arena_batch_size=16, arenaCompare=24, numIters=1, numWarmupIters=0,
             _azg_seed=9)
    a.update(kw)
    return a


def test_tt_one_iteration_and_one_arena_through_the_runners():
    """run_iteration (SelfPlayRunner, train.py's cpuct and probFastSim) and run_arena (ArenaRunner) on 16 slots: the games end, the
    samples are whole (8 symmetries of every recorded position, policies that sum to one over empty cells, one-hot results)"""
    from alphazero_general_amd import iteration as I
    args = _run_args()
    net = _tt_nets(1)[0]
    out = I.run_iteration(_game(), net, args, 1, num_slots=16)
    obs, pi, z = [t.cpu() for t in out['samples']]
    assert out['games'] >= 32 and sum(out['wins']) + out['draws'] == out['num_results'] >= 32
    assert obs.shape[1:] == (1, 3, 3) and obs.shape[0] == pi.shape[0] == z.shape[0] and obs.shape[0] % 8 == 0 and obs.shape[0] >= 64
    assert torch.allclose(pi.sum(1), torch.ones(pi.shape[0]), atol=1e-5) and bool((z.sum(1) == 1).all())
    assert bool((pi[obs.reshape(-1, 9) != 0] == 0).all())                                    # no mass on a taken cell
    assert bool(((obs == 0) | (obs == 1) | (obs == -1)).all())
    nets = _tt_nets(2)
    wins, draws, wr = I.run_arena(_game(), nets, args, 24, num_slots=16)
    assert len(wins) == 2 and sum(wins) + draws >= 24 and abs(sum(wr) - 1) < 1e-9


class _RefLikeNet:
    def __init__(self, seed, args):
        from alphazero_general_amd.nnet import ResNet
        from alphazero_general_amd.utils import dotdict
        torch.manual_seed(seed)
        self.args = dotdict(args)
        self.nnet = ResNet(_game().observation_size(), A, NV, self.args).cuda()


def test_tt_native_coach_round(tmp_path):
    """coach.native_coach on the stand-in Coach of tests/test_gpu_iteration.py: one network iteration of the game native_coach used to
    refuse ("has no device rules"), 16 slots, then the gating arena"""
    import test_gpu_iteration as TI
    from alphazero_general_amd.coach import native_coach
    args = _run_args(data=str(tmp_path / 'data'), run_name='tt', _azg_slots=16, _azg_arena_slots=16)
    Native = native_coach(TI._StandInCoach)
    coach = Native(_game(), _RefLikeNet(4, args), args)
    coach.past_net = _RefLikeNet(5, args)
    coach.learn()
    assert len(coach.loaded) == 1
    d, p, v = coach.loaded[0]
    assert d.shape[0] == p.shape[0] == v.shape[0] >= 64 and d.shape[1:] == (1, 3, 3) and not d.is_cuda
    assert torch.allclose(p.sum(1), torch.ones(p.shape[0]), atol=1e-5) and bool((v.sum(1) == 1).all())
    for wins, draws, wr in coach.arena_results:
        assert len(wins) == 2 and sum(wins) + draws >= 24 and len(wr) == 2 and abs(sum(wr) - 1) < 1e-9
