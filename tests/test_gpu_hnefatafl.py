"""Hnefatafl on the device (csrc/azg_games.h struct HN, game id 6: two cells per lane, 128-bit board masks, move lists of up to seven
chunks of 64 children) against fixtures the REFERENCE produced (tests/golden/hn_*.npz, written by tests/golden/make_hnefatafl_goldens.py
from alphazero/envs/hnefatafl/fastafl.pyx on fastafl/cengine.pyx).  There is no C oracle for this game: the fixtures and the host env are
the checkers, and every comparison is equality.

  * rules: every record of hn_rules.npz through the engine -- state round trip, observation in all three formats, root children = valid
    moves, terminal flags, play_action by a steered second simulation;
  * hn_tree / hn_edge / every hn_agent config bit for bit in the per-phase forms (select + backup, backup_select) and, where the config
    has no network (warm-up), through azg_search_raw;
  * azg_search_raw against sims x [azg_select(NULL), azg_backup] at 1, 3 and 64 slots; forced compaction; slot export / import;
  * the MCTS class on the host env; a SelfPlayRunner round with a PyTorch network (no tower is built for this game)."""
import numpy as np
import pytest
import torch

import fixture_checks as FC
import test_gpu_parity as P
import test_gpu_raw_search as RS
from fixture_checks import crc, crc_rows, load as _load

pytestmark = pytest.mark.gpu
HN, DEV, A, NV, CELLS = 6, 'cuda:0', 2420, 3, 121
PROB_TEMPS = [1.0, 0.5, 0.25, 0.2, 0.0]                       # (hn_edge.npz does not hold its probs columns' temperatures: make_goldens.PROB_TEMPS)
# This game's tier of fixture_checks.TREE.  The fixtures hold the 2420-wide rows as crcs, so MCTS.probs is compared where its power is exact
# on both sides: temperature 1 (x), 0.5 (x * x) and 0 (one-hot).  At 0.25 and 0.2 numpy calls the C library's float32 powf, which is within
# an ulp but not correctly rounded, and np_pow_f32 (csrc/azg_device.h, shared by every game) rounds a double pow: on hn_tree's `cpuct4` trace
# ONE of 14 520 entries differs by an ulp at 0.25 -- the tier a crc cannot carry.
# p_ulps: priors under ROOT TEMPERATURE are p ** (1 / 1.1) renormalised (MCTS.pyx:249-252): numpy's float32 powf again.  Both powers are
# within one ulp of the true value, so is their float32 sum (every term is), and the quotient rounds once more: the two priors are at most
# 4 ulps apart -- and must be, everything downstream of them (PUCT choices, counts, q, v) is compared exactly
HN_TREE = dict(FC.TREE, p_ulps=4)                             # (rootn crcs: of the fixture's int16 rows)
HN_EDGE = dict(HN_TREE, rootn_crc_dtype=np.int32, has_k=True)  # crcs of int32 rows; up to 448 children kept, and the root's child count


def _game():
    from alphazero_general_amd.envs.hnefatafl import Game
    return Game


def _edge_states(d, rows=None):
    rows = range(len(d['player'])) if rows is None else rows
    return [(d['cells'][i], int(d['player'][i]), int(d['turns'][i]), int(d['aux0'][i])) for i in rows]


# ------------------------------------------------------------------------------------------------------------------------- rules
def test_hn_rules_vs_reference_tables():
    from alphazero_general_amd.engine import DeviceEngine
    d = _load('hn_rules')
    n, ws, nxt = len(d['player']), d['ws'], d['next'].astype(np.int64)
    assert n >= 10500 and int(d['n_play']) >= 10000 and (d['nvalid'] > 256).any()
    eng = DeviceEngine(HN, n, seed=3, sims_hint=4, cpuct=1.25, fpu_reduction=0.2, nodes_per_tree=1024)
    states = _edge_states(d)
    eng.set_states(states)
    back = eng.get_states_full()
    assert all((back[i][0] == states[i][0]).all() and tuple(back[i][1:]) == tuple(states[i][1:]) for i in range(n))
    o32, o16, o8 = eng.new_obs(), eng.new_obs(torch.float16), torch.zeros((n, CELLS, 8), dtype=torch.float16, device=eng.device)
    eng.select(o32)                                           # find_leaf at a fresh root: win_state, valid_moves, add_children, observation
    for fmt in (o16, o8):                                     # (the other two formats from fresh trees of the same states)
        eng.set_states(states)
        eng.select(fmt)
    o = o32.cpu().numpy()
    assert (crc_rows(o.reshape(n, -1)) == d['obs_crc']).all()
    assert (o16.float().cpu().numpy() == o).all()
    h = o8.float().cpu().numpy()
    assert (h[:, :, 5:] == 0).all() and (h[:, :, :5].transpose(0, 2, 1).reshape(n, 5, 11, 11) == o).all()
    for i in range(n):
        ch = eng.root_children(i)
        v = np.zeros(A, np.uint8); v[ch['a']] = 1
        assert len(ch['a']) == v.sum() == d['nvalid'][i] and crc(v) == d['valid_crc'][i], ('valid_moves', i)
        e = eng.tree_info(i)['e']
        assert e == int(ws[i][0]) + 2 * int(ws[i][1]) + 4 * int(ws[i][2]), ('win_state', i, e, ws[i])
    # one backup with a policy peaked on the record's next move, then the second simulation descends exactly that ply
    has_next = nxt >= 0
    pol = np.full((n, A), 1e-4, np.float32)
    pol[np.arange(n), np.where(has_next, nxt, 0)] = 0.9
    val = np.full((n, NV), 1.0 / 3, np.float32)
    eng.backup(torch.from_numpy(pol).to(eng.device), torch.from_numpy(val).to(eng.device))
    eng.select(o32)
    o = o32.cpu().numpy()
    leaves = eng.get_leaf_states(full=True)
    oc = crc_rows(o.reshape(n, -1))
    for i in range(n):
        lc, lp, lt, lk = leaves[i]
        if ws[i].any():                                       # terminal root: find_leaf stops at it
            assert len(eng.last_path(i)) == 0 and (lc == d['cells'][i]).all(), ('terminal', i)
            continue
        if not has_next[i]:
            continue
        assert list(eng.last_path(i)) == [nxt[i]], ('descent', i)
        assert (lc == d['cells'][i + 1]).all(), ('play_action: board', i)
        assert lp == d['player'][i + 1] and lt == d['turns'][i + 1] and lk == d['aux0'][i + 1], ('play_action: player / turns / king captured', i)
        assert oc[i] == d['obs_crc'][i + 1], ('observation after play_action', i)
    eng.counters()
    eng.close()


# ------------------------------------------------------------------------------------------------------------------------- tree / edge
@pytest.mark.parametrize('launch', P.LAUNCHES)
@pytest.mark.parametrize('cname', ['default', 'cpuct4', 'temp'])
def test_hn_tree_vs_reference_goldens(cname, launch):
    d = _load('hn_tree')
    sims = int(d[cname + '_cfg'][4])
    tr, = FC.check_tree(HN, d, cname, FC.states_from_prefix(_game(), d['prefix']), HN_TREE, 'hn', None, [launch], nodes_per_tree=sims * 448 + 64)
    assert all(len(a) > 64 for a in tr['a'])


@pytest.mark.parametrize('launch', P.LAUNCHES)
@pytest.mark.parametrize('cname', ['default', 'noise_temp'])
def test_hn_edge_vs_reference_goldens(cname, launch):
    """roots with exactly 64 | 65, 128 | 129, 192 | 193, 256 | 257 legal moves -- both sides of every chunk boundary of the child list --
    and roots at turns 508..511, where leaves meet the turn-512 draw inside the tree; noise_temp: Dirichlet noise over up to 257 children
    (alpha = 10.83 / k: some draws are float32 denormals) and root temperature"""
    d = _load('hn_edge')
    sims = int(d[cname + '_cfg'][4])
    assert {64, 65, 128, 129, 192, 193, 256, 257, -508, -509, -510, -511} <= set(d['kind'].tolist())
    assert (d[cname + '_k'][:8] == d['kind'][:8]).all() and (d[cname + '_leaf_e'][d['kind'] < 0] == 4).any()
    FC.check_tree(HN, d, cname, _edge_states(d), HN_EDGE, 'hn_edge', None, [launch], prob_temps=PROB_TEMPS, nodes_per_tree=sims * 448 + 64)


# ------------------------------------------------------------------------------------------------------------------------- agent
AGENT = {'plain': (dict(symmetric_samples=False), dict()),
         'symmetric': (dict(add_root_temp=True, cpuct=4.0, fpu_reduction=0.4), dict()),
         'fastmix': (dict(symmetric_samples=False), dict(prob_fast=0.5, fast_sims=3)),
         'warmup': (dict(), dict(warmup=True, warmup_sims=5)),
         'long': (dict(symmetric_samples=False), dict())}


@pytest.mark.parametrize('cname,launch', [(c, l) for c in AGENT for l in P.LAUNCHES] + [('warmup', 'raw')])
def test_hn_agent_vs_reference_goldens(cname, launch):
    """whole reference SelfPlayAgent runs, move for move and sample for sample; `long` plays until a game ends in the turn-512 draw: a
    513-entry history and paths through turn 512; launch 'raw': a warm-up round as ONE azg_search_raw launch"""
    d = _load('hn_agent')
    kw, rnd = AGENT[cname]
    rec = FC.check_agent(HN, d, cname + '_', launch, 'hn', max_rounds=2200, **rnd,
                         engine_kw=dict(kw, example_capacity=8192, sims_hint=max(int(d[cname + '_sims']), 5), nodes_per_tree=16 * 5 * 448 + 64))
    if cname == 'long':
        ws, turns = rec['r_ws'], rec['r_turns']
        assert 512 in turns.tolist() and ws[turns.tolist().index(512)].tolist() == [0, 0, 1]


# ------------------------------------------------------------------------------------------------------------------------- raw search
def _raw_states(B):
    """edge roots first (257 and 256 children, turn 508, ...), the opening for the rest"""
    d = _load('hn_edge')
    order = [7, 8, 6, 0, 1, 2, 3, 4, 5, 9, 10, 11]
    st = _edge_states(d, order[:min(B - 1, len(order))])
    return st + [_game()().to_azg_state()] * (B - len(st))


@pytest.mark.parametrize('consts', [RS.RAW, RS.WARM])
@pytest.mark.parametrize('B', [1, 3, 64])
def test_hn_search_raw_equals_per_phase_loop(B, consts):
    """azg_search_raw against sims x [azg_select(NULL), azg_backup] from the same states: trees, counters, leaf states and last paths"""
    sims, rounds = 12, 5
    mk = lambda: RS._engine(HN, B, seed=36, sims_hint=sims, add_root_noise=True, add_root_temp=True, cpuct=4.0, fpu_reduction=0.4,
                            example_capacity=B * (rounds + 1) * 8, nodes_per_tree=4 * sims * 448 + 64)
    ea, eb = mk(), mk()
    try:
        st = _raw_states(B)
        ea.set_states(st); eb.set_states(st)
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
        assert ca == cb and ca['sims'] == B * sims * rounds
        if B > 1:
            assert ca['games_played'] >= 1                    # (the turn-508 root ran into the draw and restarted)
        for x, y in zip(ea.examples(), eb.examples()):
            assert torch.equal(x, y)
        for x, y in zip(ea.results(), eb.results()):
            assert (x == y).all()
    finally:
        ea.close(); eb.close()


def _trees(e):
    """every slot's root children, root record and last path -- not the store's fill, which is what a compaction changes"""
    out = []
    for i in range(e.B):
        ch, info = e.root_children(i), e.tree_info(i)
        out.append((tuple(ch[f].tobytes() for f in ('a', 'n', 'q', 'p', 'v')), tuple(sorted((k, v) for k, v in info.items() if k != 'nodes_used')),
                    e.last_path(i).tobytes()))
    return out


def test_hn_forced_compaction_changes_no_result():
    B, sims, rounds = 12, 10, 6
    mk = lambda: RS._engine(HN, B, seed=52, sims_hint=sims, add_root_noise=True, add_root_temp=True, example_capacity=B * (rounds + 1) * 8,
                            nodes_per_tree=rounds * sims * 448 + 64)
    ea, eb = mk(), mk()
    try:
        st = _raw_states(B)
        ea.set_states(st); eb.set_states(st)
        for rnd in range(rounds):
            for s in range(sims):
                pol, val = P.fake_batch(torch, 52, range(B), rnd * sims + s, A, NV, ea.device)
                for e in (ea, eb):
                    e.select(None)
                    e.backup(pol, val)
            assert _trees(ea) == _trees(eb) and torch.equal(ea.root_probs(1.0), eb.root_probs(1.0)), rnd
            ea.advance(True); eb.advance(True)
            eb.compact(force=True)                            # every tree copied into its other semi-space: the root's subtree only
            assert torch.equal(ea.last_actions(), eb.last_actions()), rnd
            assert torch.equal(ea.root_counts(), eb.root_counts()), rnd
            used = [(ea.tree_info(i)['nodes_used'], eb.tree_info(i)['nodes_used']) for i in range(B)]
            assert all(b <= a for a, b in used) and any(b < a for a, b in used), rnd
        for x, y in zip(ea.examples(), eb.examples()):
            assert torch.equal(x, y)
        assert ea.counters()['games_played'] == eb.counters()['games_played']
    finally:
        ea.close(); eb.close()


def test_hn_slot_export_import_continues_bit_for_bit():
    sims = 10
    mk = lambda: RS._engine(HN, 2, seed=58, sims_hint=sims, add_root_noise=True, add_root_temp=True, nodes_per_tree=8 * sims * 448 + 64)
    ea, eb = mk(), mk()
    try:
        st = _raw_states(2)
        ea.set_states(st)
        fill, vrow = RS._rows(ea, RS.WARM)
        for rnd in range(3):
            ea.search_raw(sims, fill, vrow)
            ea.advance(False)
        ea.search_raw(sims // 2, fill, vrow)                  # (in the middle of a move's search)
        for slot in range(2):
            eb.import_slot(ea.export_slot(slot), slot)
        assert RS._snapshot(ea)[:3] == RS._snapshot(eb)[:3]
        for rnd in range(3):
            for e in (ea, eb):
                e.search_raw(sims, fill, vrow)
            assert RS._snapshot(ea)[:3] == RS._snapshot(eb)[:3], rnd
            ea.advance(False); eb.advance(False)
            assert torch.equal(ea.last_actions(), eb.last_actions()), rnd
    finally:
        ea.close(); eb.close()


# ------------------------------------------------------------------------------------------------------------------------- Python layers
def test_hn_mcts_class_api_vs_reference_goldens():
    """alphazero_general_amd.MCTS on an envs.hnefatafl.Game object: search() with a callable network fed the fixture's evaluations builds
    hn_tree's root 0; raw_search() equals the per-phase loop of a one-slot engine; update_root / probs / counts follow the move"""
    from alphazero_general_amd.MCTS import MCTS, NODE_STORE_BUDGET
    from alphazero_general_amd.engine import DeviceEngine
    from alphazero_general_amd.utils import dotdict
    d = _load('hn_tree')
    cpuct, fpu, _, _, sims = d['default_cfg']
    seed, Game = int(d['default_seed']), _game()
    m, g = FC.check_mcts_class(Game, d, A, NV, search=True, tier=HN_TREE, game='hn')
    assert m._engine.nodes_per_tree * 64 <= NODE_STORE_BUDGET                               # (a default object: 256 MB, not max_turns moves' worth)
    args = dotdict(cpuct=float(cpuct), fpu_reduction=float(fpu), root_noise_frac=0.1, root_policy_temp=1.1, min_discount=1, _num_players=3,
                   numMCTSSims=int(sims), _azg_seed=seed)
    c0 = np.asarray(m.counts(g))
    a = m.best_action(g)
    m.update_root(g, a)
    g2 = g.clone(); g2.play_action(a)
    assert c0[a] == c0.max() > 1 and int(np.asarray(m.counts(g2)).sum()) == c0[a] - 1      # the played child's subtree is the tree now
    assert type(m.find_leaf(g2)) is Game
    # raw_search: ones / zeros rows, one launch; the same tree as the loop on a one-slot engine with the same tape
    m2 = MCTS(dotdict(dict(args), _azg_nodes_per_tree=40 * 448 + 64))
    m2.raw_search(g, 30, True, True)
    e = DeviceEngine(HN, 1, cpuct=float(cpuct), fpu_reduction=float(fpu), seed=seed, sims_hint=30, nodes_per_tree=40 * 448 + 64)
    e.set_states([g.to_azg_state()])
    pol, val = torch.ones((1, A), device=e.device), torch.zeros((1, NV), device=e.device)
    for _ in range(30):
        e.select(None)
        e.backup(pol, val, add_root_noise=True, add_root_temp=True)
    assert (np.asarray(m2.counts(g)) == e.root_counts()[0].cpu().numpy()).all() and np.asarray(m2.counts(g)).sum() == 29
    assert (np.asarray(m2.probs(g, 1.0), np.float32) == e.root_probs(1.0)[0].cpu().numpy()).all()
    e.close()


def test_hn_selfplay_runner_round_with_a_pytorch_network():
    """no tower is built for this game: NNetWrapper(backend='auto') runs PyTorch and the runner takes the per-phase form; whole games'
    samples come out whole and every policy sums to one over the legal moves of its position"""
    from alphazero_general_amd.nnet import DEFAULT_NET_ARGS, NNetWrapper
    from alphazero_general_amd.selfplay import SelfPlayRunner
    from alphazero_general_amd.utils import dotdict
    Game = _game()
    torch.manual_seed(11)
    net = NNetWrapper(Game, dotdict(dict(DEFAULT_NET_ARGS)), device=DEV)
    net.refresh()
    assert getattr(net, '_hip', None) is None or not net._hip.can_search
    B, sims = 4, 6
    args = dotdict(numMCTSSims=sims, gamesPerIteration=1 << 30, symmetricSamples=False, add_root_noise=True, add_root_temp=True, cpuct=1.25,
                   fpu_reduction=0.2, probFastSim=0.0, startTemp=1.0)
    r = SelfPlayRunner(Game, net, args, num_slots=B, seed=5, example_capacity=B * 2 * 513, nodes_per_tree=16 * sims * 448 + 64)
    assert not r.fused_search
    st = _edge_states(_load('hn_edge'), [8, 9, 10, 11])       # turns 508..511: the games end in a few rounds and restart
    r.engine.set_states(st)
    for _ in range(8):
        r.play_round()
    c = r.engine.counters()
    assert c['games_played'] >= B and c['sims'] == B * sims * 8
    obs, pi, z = [t.cpu().numpy() for t in r.engine.examples()]
    assert len(obs) == c['num_examples'] >= B and obs.shape[1:] == (5, 11, 11) and np.isfinite(pi).all()
    # (a policy is counts / sum of at most `sims` non-zero entries: each quotient is off by half an ulp at most, 2^-25 here)
    assert (np.abs(pi.sum(axis=1, dtype=np.float64) - 1.0) <= sims * 2.0 ** -25).all() and (z.sum(axis=1) == 1).all()
    # the first samples are the four start states' own observations, and their policies sit on those states' legal moves
    for i in range(B):
        g = Game.from_azg_state(*st[i])
        j = next(j for j in range(len(obs)) if (obs[j] == g.observation()).all())
        assert (pi[j][g.valid_moves() == 0] == 0).all()
