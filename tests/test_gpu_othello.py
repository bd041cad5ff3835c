"""Othello on the device (csrc/azg_games.h struct OT, game id 3) against fixtures the REFERENCE produced (tests/golden/ot_*.npz, written by
tests/golden/make_othello_goldens.py from alphazero/envs/othello) and the 8x8 network kernels against the fp64 reference of
tests/net_reference.py:

  * every ot_rules position through the engine ABI: valid moves, win state (no pass: the mover without a move ends the game), observation,
    and play_action by a steered second simulation (test_gpu_rules._check_table);
  * the reference's MCTS (ot_tree), SelfPlayAgent (ot_agent: plain, noisy, fastmix -- raw samples with symmetricSamples=False are
    symmetries()[7], the identity) and a whole agent under np.random.seed(s) (ot_mt19937_agent), per-phase and fused launches;
  * the tower, head features, logits and probabilities of the 32- and 64-channel nets at every tile threshold, every border class and
    depths 0 to 6; the sparse heads;
  * azg_search_wide_exact_f16 / azg_search_wide_f16 against the launch-per-phase loop fed NNetWrapper.process / the sparse heads;
  * the MCTS class API on envs.othello.Game against ot_tree."""
import os

import numpy as np
import pytest
import torch

import net_reference as R
import oracle_lib as ol
import test_gpu_net_fp64 as F
import test_gpu_parity as P
import test_gpu_rules as GR

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
OT, DEV = 3, 'cuda:0'
NETS = {'othello_64x4': ('OTHELLO_NET_ARGS', {}), 'othello_32x4': ('DEFAULT_NET_ARGS', {})}


def _game():
    from alphazero_general_amd.envs.othello import Game
    return Game


def _states(prefix):
    Game = _game()
    out = []
    for row in prefix:
        g = Game()
        for a in row:
            if a >= 0:
                g.play_action(int(a))
        out.append(g.to_azg_state())
    return out


# ------------------------------------------------------------------------------------------------------------------------- rules
def test_ot_rules_vs_reference_tables():
    d = dict(np.load(os.path.join(G, 'ot_rules.npz')))
    n = GR._check_table(torch, OT, d['cells'], d['lens'], None, d['valids'], d['ws'], d['obs_crc'], d['moves'])
    assert len(d['lens']) >= 10000 and n > 9500


# ------------------------------------------------------------------------------------------------------------------------- tree / agent
@pytest.mark.parametrize('cname', ['default', 'cpuct4', 'noise_temp'])
def test_ot_tree_vs_reference_goldens(cname):
    d = dict(np.load(os.path.join(G, 'ot_tree.npz')))
    cpuct, fpu, noise, temp, sims = d[cname + '_cfg']
    noise, temp, sims = bool(noise), bool(temp), int(sims)
    seed = int(d[cname + '_seed'])
    R_, A, NV = d['prefix'].shape[0], 64, 3
    exact = not temp
    eng = P.engine(game=OT, B=R_, cpuct=cpuct, fpu_reduction=fpu, add_root_noise=noise, add_root_temp=temp, seed=seed, sims_hint=sims)
    eng.set_states(_states(d['prefix']))
    obs = eng.new_obs()
    for s in range(sims):
        eng.select(obs)
        for r in range(R_):
            path = eng.last_path(r)
            assert len(path) == d[cname + '_depth'][r, s]
            assert (path[:24] == d[cname + '_paths'][r, s][:len(path)]).all(), (r, s)
        pol, val = P.fake_batch(torch, seed, range(R_), s, A, NV, eng.device)
        eng.backup(pol, val)
        assert (eng.root_counts().cpu().numpy() == d[cname + '_rootn'][:, s]).all(), s
    for r in range(R_):
        ch = eng.root_children(r)
        k = len(ch['a'])
        assert (ch['a'] == d[cname + '_a'][r][:k]).all() and (d[cname + '_a'][r][k:] == -1).all() and (ch['n'] == d[cname + '_n'][r][:k]).all()
        for f in ('q', 'p', 'v'):
            if exact:
                assert (ch[f] == d[cname + '_' + f][r][:k]).all(), (f, r)
            else:
                assert np.allclose(ch[f], d[cname + '_' + f][r][:k], atol=1e-5), (f, r)
        info = eng.tree_info(r)
        assert info['n'] == d[cname + '_root_n'][r] and info['max_depth'] == d[cname + '_maxdepth'][r]
    assert (eng.root_counts().cpu().numpy() == d[cname + '_counts']).all()
    assert (eng.root_probs(1.0).cpu().numpy() == d[cname + '_probs'][:, 0]).all()
    assert (eng.root_probs(0.0).cpu().numpy() == d[cname + '_probs'][:, 4]).all()
    assert (eng.root_value(False).cpu().numpy() == d[cname + '_vmax']).all()
    assert (eng.root_value(True).cpu().numpy() == d[cname + '_vavg']).all()
    assert (eng.tape_counters() == d[cname + '_ctr']).all()
    eng.counters()
    eng.close()


AGENT = {'plain': (dict(), dict()),
         'noisy': (dict(add_root_noise=True, add_root_temp=True, cpuct=4.0, fpu_reduction=0.4), dict()),
         'fastmix': (dict(symmetric_samples=False), dict(prob_fast=0.5, fast_sims=4))}


@pytest.mark.parametrize('launch', P.LAUNCHES)
@pytest.mark.parametrize('cname', list(AGENT))
def test_ot_agent_vs_reference_goldens(cname, launch):
    d = dict(np.load(os.path.join(G, 'ot_agent.npz')))
    B, sims, games = int(d[cname + '_B']), int(d[cname + '_sims']), int(d[cname + '_games'])
    seed, slot_base = int(d[cname + '_seed']), int(d[cname + '_slot_base'])
    kw, rnd = AGENT[cname]
    eng = P.engine(game=OT, B=B, seed=seed, slot_base=slot_base, games_per_iteration=games, example_capacity=8192, sims_hint=sims, **kw)
    rec = P.run_engine_agent(torch, eng, seed, slot_base, sims, games, launch=launch, **rnd)
    assert (np.array(rec['sims']) == d[cname + '_round_sims']).all()
    assert (np.array(rec['counts']) == d[cname + '_counts']).all()
    assert (np.array(rec['actions']) == d[cname + '_actions']).all()
    assert (np.array(rec['games_played']) == d[cname + '_games_played']).all()
    assert (np.array(rec['obs_crc'], np.uint32) == d[cname + '_obs_crc']).all()
    obs, pi, z = [t.cpu().numpy() for t in eng.examples()]
    assert obs.shape == d[cname + '_s_obs'].shape
    assert (obs == d[cname + '_s_obs']).all() and (pi == d[cname + '_s_pi']).all() and (z == d[cname + '_s_z']).all()
    ws, turns, _ = eng.results()
    assert (ws == d[cname + '_r_ws']).all() and (turns == d[cname + '_r_turns']).all()
    eng.close()


@pytest.mark.parametrize('launch', P.LAUNCHES)
def test_ot_selfplay_agent_under_numpys_mt19937_seed(launch):
    d = dict(np.load(os.path.join(G, 'ot_mt19937_agent.npz')))
    B, sims, games, eseed = int(d['B']), int(d['sims']), int(d['games']), int(d['eval_seed'])
    cpuct, fpu, nfrac, rtemp = [float(x) for x in d['cfg']]
    eng = P.engine(game=OT, B=B, cpuct=cpuct, fpu_reduction=fpu, root_noise_frac=nfrac, root_policy_temp=rtemp, add_root_noise=True,
                   add_root_temp=True, seed=987654321, games_per_iteration=games, example_capacity=4096, sims_hint=sims)
    eng.set_random_tape(d['tape_ranks'], d['tape_u'], d['tape_noise_off'], d['tape_noise_pool'])
    rec = P.run_engine_agent(torch, eng, eseed, 0, sims, games, launch=launch)
    n = len(d['actions'])
    assert len(rec['actions']) == n and (np.array(rec['games_played']) == d['games_played']).all()
    for r in range(n):
        assert (np.asarray(rec['counts'][r]) == d['counts'][r]).all(), (launch, r)
        assert (np.asarray(rec['actions'][r]) == d['actions'][r]).all(), (launch, r)
    eo, ep, ez = [t.cpu().numpy() for t in eng.examples()]
    assert eo.shape == d['s_obs'].shape and (eo == d['s_obs']).all() and (ez == d['s_z']).all() and (ep == d['s_pi']).all()
    ws, turns, _ = eng.results()
    assert (ws == d['r_ws']).all() and (turns == d['r_turns']).all()
    eng.set_shuffle_tape(None)
    eng.close()


def test_ot_mcts_class_api_vs_reference_goldens():
    """alphazero_general_amd.MCTS on an envs.othello.Game object (one slot: the tape stream of ot_tree's root 0), find_leaf /
    process_results fed the fixture's evaluations, must build the reference's tree: paths, root children, counts, values"""
    from alphazero_general_amd.MCTS import MCTS
    from alphazero_general_amd.utils import dotdict
    d = dict(np.load(os.path.join(G, 'ot_tree.npz')))
    cpuct, fpu, _, _, sims = d['default_cfg']
    seed, sims = int(d['default_seed']), int(sims)
    g = _states(d['prefix'][:1])[0]
    g = _game().from_azg_state(*g)
    m = MCTS(dotdict(cpuct=float(cpuct), fpu_reduction=float(fpu), root_noise_frac=0.1, root_policy_temp=1.1, min_discount=1,
                     _num_players=3, numMCTSSims=sims, _azg_seed=seed))
    for s in range(sims):
        leaf = m.find_leaf(g)
        assert m.depth == d['default_depth'][0, s]
        p, v = ol.fake_eval(seed, 0, s, 64, 3)
        m.process_results(leaf, v, p, False, False)
    assert (np.asarray(m.counts(g)) == d['default_counts'][0]).all()
    assert m.value(False) == d['default_vmax'][0] and m.value(True) == d['default_vavg'][0]
    assert (np.asarray(m.probs(g, 1.0), np.float32) == d['default_probs'][0, 0]).all()


# ------------------------------------------------------------------------------------------------------------------------- network
def _reference(key, salt=0, depth=None):
    argname, over = NETS[key]
    over = dict(over)
    if depth is not None:
        over['depth'] = depth
    args = R.net_args(argname, **over)
    x = torch.from_numpy(R.boards('othello'))
    sd, ref = R.make_state('othello', args, 'trained', salt, probe=x)
    return args, sd, ref, x, ref.forward(x)


def _wrapper(args, sd):
    from alphazero_general_amd.nnet import NNetWrapper
    net = NNetWrapper(_game(), args, device=DEV, backend='hip')
    net.adopt(sd)
    net.refresh()
    assert net._hip is not None and net._hip.fact_head
    return net


def _tile(ch, n, cus):
    """boards per workgroup tile dispatch_tower picks for othello"""
    if ch == 32:
        return 2 if n <= 4 * cus else 4
    return 1 if n <= 2 * cus else 2


def _check(name, args, sd, o, x, sizes):
    net = _wrapper(args, sd)
    hip = net._hip
    N = x.shape[0]
    xg = x.to(DEV)
    for B in sizes:
        idx = F._idx(N, B)
        xb = xg[idx.to(DEV)].contiguous()
        x8 = hip.to_nhwc8(xb)
        tag = '%s_B%d' % (name, B)
        F._stream_cmp(tag, hip, F.tower_stream(hip, x8), o, idx, _tile(hip.CH, B, F._cus()))
        feat = hip.forward_features_nhwc8(x8).float().cpu().reshape(B, 2, hip.feat_k)
        f = feat[:, :, :hip.HW * 16].reshape(B, 2, hip.HW, 16)
        got = torch.cat([f[:, 1], f[:, 0]], 2).permute(0, 2, 1).reshape(B, 32, *o['feat'].shape[2:])
        sel = F._sel(B)
        rep = R.stream_report(got[sel], o['feat'][idx[sel]], tile=1)
        F.record(dict(case=tag, what='head_features', **rep, tau=R.TAU_STREAM))
        assert rep['ratio'] <= 1.0, (tag, rep)
        lg = hip.forward_logits_nhwc8(x8).float().cpu()
        F._logits_cmp(tag + '_fact', lg[:, :hip.A], lg[:, hip.A:hip.A + hip.NV], o, idx)
        p, v = net.process(xb)
        F._probs_cmp(tag + '_process', p.cpu(), v.cpu(), o, idx)


@pytest.mark.parametrize('key', list(NETS))
def test_ot_network_every_tile_vs_fp64(key):
    args, sd, ref, x, o = _reference(key)
    cus = F._cus()
    th = [4 * cus] if args.num_channels == 32 else [2 * cus, 4 * cus]
    big = _tile(args.num_channels, 1 << 30, cus)
    sizes = sorted({1, 37, 301} | set(th) | {t + 1 for t in th} | {big * 16 * cus + 1})
    _check(key, args, sd, o, x, sizes)


@pytest.mark.parametrize('depth', [0, 1, 2, 6])
@pytest.mark.parametrize('key', list(NETS))
def test_ot_network_depths_vs_fp64(key, depth):
    args, sd, ref, x, o = _reference(key, depth=depth)
    cus = F._cus()
    _check('%s_depth%d' % (key, depth), args, sd, o, x, [37, 4 * cus + 1])


# ------------------------------------------------------------------------------------------------------------------------- search launches
def _net(key, salt=7):
    args, sd, ref, x, o = _reference(key, salt=salt)
    return _wrapper(args, sd)


@pytest.mark.parametrize('key,B,sims,moves', [('othello_64x4', 1024, 100, 3), ('othello_32x4', 1024, 100, 3), ('othello_64x4', 96, 30, 4)])
def test_ot_wide_exact_search_vs_phase_loop(key, B, sims, moves):
    """azg_search_wide_exact_f16 against select -> NNetWrapper.process -> backup on a twin engine with the same seeds: every slot's
    counts, moves, samples and results identical"""
    from alphazero_general_amd.engine import DeviceEngine
    net = _net(key)
    kw = dict(cpuct=4.0, fpu_reduction=0.4, add_root_noise=True, add_root_temp=True, seed=41, games_per_iteration=1 << 30,
              example_capacity=B * (moves + 1) * 8, sims_hint=sims)
    ea, ec = DeviceEngine(OT, B, **kw), DeviceEngine(OT, B, **kw)
    oc = ec.new_obs(torch.float32)
    for mv in range(moves):
        net._hip.search(ea, sims, exact=True)
        for _ in range(sims):
            ec.select(oc)
            p, v = net.process(oc)
            ec.backup(p.contiguous(), v.contiguous())
        assert torch.equal(ea.root_counts(), ec.root_counts()), mv
        assert torch.equal(ea.root_probs(1.0), ec.root_probs(1.0)) and torch.equal(ea.root_value(True), ec.root_value(True)), mv
        ea.advance(True); ec.advance(True)
        assert torch.equal(ea.last_actions(), ec.last_actions()), mv
    assert (ea.tape_counters() == ec.tape_counters()).all()
    assert ea.counters() == ec.counters()
    for t, u in zip(ea.examples(), ec.examples()):
        assert torch.equal(t, u)
    assert all((a == b).all() for a, b in zip(ea.results(), ec.results()))
    ea.close(); ec.close()


def test_ot_wide_exact_search_at_exact_ties():
    """the persistent launch (azg_search_wide_exact_f16) where every PUCT comparison ties: a flat network -- the trained weights with
    the last Linear of both heads zeroed, so every logit is 0, every prior the same after masking and every value row uniform -- on
    the roots of tests/golden/ot_edge.npz (openings to late middle games, and the reference's smallest roots: one and two legal moves;
    its othello has no pass action), four slots each, against the per-phase loop on a twin engine.  Root noise and temperature off."""
    import edge_eval as ee
    from alphazero_general_amd.engine import DeviceEngine
    args, sd, ref, x, o = _reference('othello_64x4', salt=7)
    last = ['%s.%d' % (h, max(int(k.split('.')[1]) for k in sd if k.startswith(h + '.'))) for h in ('pi_fc', 'v_fc')]
    sd = {k: (torch.zeros_like(v) if k.rsplit('.', 1)[0] in last else v) for k, v in sd.items()}
    assert sum(1 for k in sd if k.rsplit('.', 1)[0] in last) == 4 and sd[last[0] + '.weight'].shape[0] == 64
    net = _wrapper(args, sd)
    roots = ee.roots(dict(np.load(os.path.join(G, 'ot_edge.npz'))), OT)
    ks = [int(g.valid_moves().sum()) for g in roots]
    assert {1, 2} <= set(ks) and max(ks) >= 8
    states = [g.to_azg_state() for g in roots] * 4
    B, sims, moves = len(states), 60, 2
    kw = dict(cpuct=1.25, fpu_reduction=-1.0, seed=47, games_per_iteration=1 << 30, example_capacity=B * (moves + 1) * 8, sims_hint=sims)
    ea, ec, ep = DeviceEngine(OT, B, **kw), DeviceEngine(OT, B, **kw), DeviceEngine(OT, B, **kw)
    ea.set_states(states); ec.set_states(states); ep.set_states(states)
    oc = ec.new_obs(torch.float32)
    ep.select(oc)                                           # (a third engine: the twins' tapes stay in step)
    p, v = net.process(oc)                                  # the network really ties: every row's entries are equal bit for bit
    ep.close()
    assert p.shape == (B, 64) and bool((p == p[:, :1]).all()) and bool((v == v[:, :1]).all()) and bool((p > 0).all())
    for mv in range(moves):
        net._hip.search(ea, sims, exact=True)
        for _ in range(sims):
            ec.select(oc)
            p, v = net.process(oc)
            ec.backup(p.contiguous(), v.contiguous())
        assert torch.equal(ea.root_counts(), ec.root_counts()), mv
        assert torch.equal(ea.root_probs(1.0), ec.root_probs(1.0)) and torch.equal(ea.root_value(True), ec.root_value(True)), mv
        assert torch.equal(ea.root_value(False), ec.root_value(False)), mv
        ea.advance(True); ec.advance(True)
        assert torch.equal(ea.last_actions(), ec.last_actions()), mv
    assert (ea.tape_counters() == ec.tape_counters()).all()
    assert ea.counters() == ec.counters()
    for t, u in zip(ea.examples(), ec.examples()):
        assert torch.equal(t, u)
    assert all((a == b).all() for a, b in zip(ea.results(), ec.results()))
    ea.close(); ec.close()


@pytest.mark.parametrize('key', list(NETS))
def test_ot_wide_sparse_search_vs_phase_loop(key):
    """azg_search_wide_f16 (sparse heads) against select -> tower features -> azg_leaf_heads_sparse_f16 -> softmax -> backup"""
    from alphazero_general_amd.engine import DeviceEngine
    net = _net(key)
    hip = net._hip
    B, sims, moves = 512, 50, 3
    kw = dict(cpuct=1.25, fpu_reduction=0.2, add_root_noise=True, add_root_temp=True, seed=29, games_per_iteration=1 << 30,
              example_capacity=B * (moves + 1) * 8, sims_hint=sims)
    ea, ec = DeviceEngine(OT, B, **kw), DeviceEngine(OT, B, **kw)
    oc = ec.new_obs(torch.float32)
    for mv in range(moves):
        hip.search(ea, sims)
        for _ in range(sims):
            ec.select(oc)
            lg = ec.leaf_heads_sparse(hip.forward_features_nhwc8(hip.to_nhwc8(oc), key=2), hip.head_rows, hip.head2_b)
            p, v = ec.heads_softmax(lg)
            ec.backup(p, v)
        assert torch.equal(ea.root_counts(), ec.root_counts()), mv
        ea.advance(True); ec.advance(True)
        assert torch.equal(ea.last_actions(), ec.last_actions()), mv
    assert ea.counters() == ec.counters()
    ea.close(); ec.close()


def test_ot_sparse_heads_vs_fp64():
    """azg_leaf_heads_sparse_f16 on othello leaves: valid-action and value logits against the fp64 network, -inf elsewhere"""
    from alphazero_general_amd.engine import DeviceEngine
    args, sd, ref, x, o = _reference('othello_64x4')
    hip = _wrapper(args, sd)._hip
    Game = _game()
    B = 96
    e = DeviceEngine(OT, B, seed=5, cpuct=1.25, fpu_reduction=0.2, example_capacity=1 << 16, sims_hint=8, device=0)
    oc = e.new_obs(torch.float32)
    lgs, obs, valid = [], [], []
    for move in range(3):
        for s in range(8):
            e.select(oc)
            lg = e.leaf_heads_sparse(hip.forward_features_nhwc8(hip.to_nhwc8(oc)), hip.head_rows, hip.head2_b)
            for i, lf in enumerate(e.get_leaf_states(full=True)):
                g = Game.from_azg_state(*lf[:3])
                if g.win_state().any():
                    continue
                lgs.append(lg[i].cpu()); obs.append(oc[i].cpu()); valid.append(torch.from_numpy(np.asarray(g.valid_moves(), bool)))
            pol, val = e.heads_softmax(lg)
            e.backup(pol, val)
        e.advance(True)
    lg, xo, valid = torch.stack(lgs), torch.stack(obs), torch.stack(valid)
    r = ref.forward(xo)
    A, NV = ref.A, ref.NV
    assert bool(torch.isneginf(lg[:, :A][~valid]).all()) and bool(torch.isfinite(lg[:, :A][valid]).all())
    scale = R.row_std(r['pi'])
    cen = lambda t: t - (torch.where(valid, t, 0.0).sum(1, keepdim=True) / valid.sum(1, keepdim=True))
    gp, rp = torch.where(valid, lg[:, :A].double(), 0.0), torch.where(valid, r['pi'], 0.0)
    err_p = float(torch.where(valid, (cen(gp) - cen(rp)).abs(), 0.0).max())
    ev, sv, rv = R.logit_err(lg[:, A:A + NV], r['v'])
    assert err_p / (R.TAU * scale) <= 1.0 and rv <= 1.0, (err_p, scale, rv)
    e.close()
