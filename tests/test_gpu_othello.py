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

import fixture_checks as FC
import net_reference as R
import test_gpu_net_fp64 as F
import test_gpu_parity as P
import test_gpu_rules as GR

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
OT, DEV = 3, 'cuda:0'
NETS = ['othello_64x4', 'othello_32x4']             # test_gpu_net_fp64.GAME_NETS: reference / wrapper / check_network there


def _game():
    from alphazero_general_amd.envs.othello import Game
    return Game


# ------------------------------------------------------------------------------------------------------------------------- rules
def test_ot_rules_vs_reference_tables():
    d = dict(np.load(os.path.join(G, 'ot_rules.npz')))
    n = GR._check_table(torch, OT, d['cells'], d['lens'], None, d['valids'], d['ws'], d['obs_crc'], d['moves'])
    assert len(d['lens']) >= 10000 and n > 9500


# ------------------------------------------------------------------------------------------------------------------------- tree / agent
@pytest.mark.parametrize('cname', ['default', 'cpuct4', 'noise_temp'])
def test_ot_tree_vs_reference_goldens(cname):
    d = FC.load('ot_tree')
    FC.check_tree(OT, d, cname, FC.states_from_prefix(_game(), d['prefix']), FC.TREE, 'ot')


AGENT = {'plain': (dict(), dict()),
         'noisy': (dict(add_root_noise=True, add_root_temp=True, cpuct=4.0, fpu_reduction=0.4), dict()),
         'fastmix': (dict(symmetric_samples=False), dict(prob_fast=0.5, fast_sims=4))}


@pytest.mark.parametrize('launch', P.LAUNCHES)
@pytest.mark.parametrize('cname', list(AGENT))
def test_ot_agent_vs_reference_goldens(cname, launch):
    kw, rnd = AGENT[cname]
    FC.check_agent(OT, FC.load('ot_agent'), cname + '_', launch, 'ot', engine_kw=dict(kw, example_capacity=8192), **rnd)


@pytest.mark.parametrize('launch', P.LAUNCHES)
def test_ot_selfplay_agent_under_numpys_mt19937_seed(launch):
    FC.check_mt19937_agent(OT, FC.load('ot_mt19937_agent'), launch, 'ot')


def test_ot_mcts_class_api_vs_reference_goldens():
    """alphazero_general_amd.MCTS on an envs.othello.Game object (one slot: the tape stream of ot_tree's root 0), find_leaf /
    process_results fed the fixture's evaluations, must build the reference's tree: paths, root children, counts, values"""
    FC.check_mcts_class(_game(), FC.load('ot_tree'), 64, 3, game='ot')


# ------------------------------------------------------------------------------------------------------------------------- network
@pytest.mark.parametrize('key', list(NETS))
def test_ot_network_every_tile_vs_fp64(key):
    args, sd, ref, x, o = F.reference(key)
    cus = F._cus()
    th = [4 * cus] if args.num_channels == 32 else [2 * cus, 4 * cus]
    big = F.tile_boards('othello', args.num_channels, 1 << 30, cus)
    sizes = sorted({1, 37, 301} | set(th) | {t + 1 for t in th} | {big * 16 * cus + 1})
    F.check_network(key, key, args, sd, ref, x, o, sizes)


@pytest.mark.parametrize('depth', [0, 1, 2, 6])
@pytest.mark.parametrize('key', list(NETS))
def test_ot_network_depths_vs_fp64(key, depth):
    args, sd, ref, x, o = F.reference(key, depth=depth)
    cus = F._cus()
    F.check_network('%s_depth%d' % (key, depth), key, args, sd, ref, x, o, [37, 4 * cus + 1])


# ------------------------------------------------------------------------------------------------------------------------- search launches
def _net(key, salt=7):
    args, sd, ref, x, o = F.reference(key, salt=salt)
    return F.wrapper(key, args, sd)


@pytest.mark.parametrize('key,B,sims,moves', [('othello_64x4', 1024, 100, 3), ('othello_32x4', 1024, 100, 3), ('othello_64x4', 96, 30, 4)])
def test_ot_wide_exact_search_vs_phase_loop(key, B, sims, moves):
    """azg_search_wide_exact_f16 against select -> NNetWrapper.process -> backup on a twin engine with the same seeds: every slot's
    counts, moves, samples and results identical"""
    net = _net(key)
    FC.twin_moves(OT, B, lambda ea: net._hip.search(ea, sims, exact=True), lambda ec, oc: net.process(oc), sims, moves,
                  cpuct=4.0, fpu_reduction=0.4, add_root_noise=True, add_root_temp=True, seed=41)


def test_ot_wide_exact_search_at_exact_ties():
    """the persistent launch (azg_search_wide_exact_f16) where every PUCT comparison ties: a flat network -- the trained weights with
    the last Linear of both heads zeroed, so every logit is 0, every prior the same after masking and every value row uniform -- on
    the roots of tests/golden/ot_edge.npz (openings to late middle games, and the reference's smallest roots: one and two legal moves;
    its othello has no pass action), four slots each, against the per-phase loop on a twin engine.  Root noise and temperature off."""
    import edge_eval as ee
    from alphazero_general_amd.engine import DeviceEngine
    args, sd, ref, x, o = F.reference('othello_64x4', salt=7)
    last = ['%s.%d' % (h, max(int(k.split('.')[1]) for k in sd if k.startswith(h + '.'))) for h in ('pi_fc', 'v_fc')]
    sd = {k: (torch.zeros_like(v) if k.rsplit('.', 1)[0] in last else v) for k, v in sd.items()}
    assert sum(1 for k in sd if k.rsplit('.', 1)[0] in last) == 4 and sd[last[0] + '.weight'].shape[0] == 64
    net = F.wrapper('othello_64x4', args, sd)
    roots = ee.roots(FC.load('ot_edge'), OT)
    ks = [int(g.valid_moves().sum()) for g in roots]
    assert {1, 2} <= set(ks) and max(ks) >= 8
    states = [g.to_azg_state() for g in roots] * 4
    B, sims, moves = len(states), 60, 2
    ep = DeviceEngine(OT, B, seed=47)                       # (an engine of its own: the twins' tapes stay in step)
    ep.set_states(states)
    oc = ep.new_obs(torch.float32)
    ep.select(oc)
    p, v = net.process(oc)                                  # the network really ties: every row's entries are equal bit for bit
    ep.close()
    assert p.shape == (B, 64) and bool((p == p[:, :1]).all()) and bool((v == v[:, :1]).all()) and bool((p > 0).all())
    FC.twin_moves(OT, B, lambda ea: net._hip.search(ea, sims, exact=True), lambda ec, oc: net.process(oc), sims, moves, states,
                  cpuct=1.25, fpu_reduction=-1.0, seed=47)


@pytest.mark.parametrize('key', list(NETS))
def test_ot_wide_sparse_search_vs_phase_loop(key):
    """azg_search_wide_f16 (sparse heads) against select -> tower features -> azg_leaf_heads_sparse_f16 -> softmax -> backup"""
    from alphazero_general_amd.engine import DeviceEngine
    net = _net(key)
    hip = net._hip
    # counts, moves and counters: the comparisons this test has always made of the sparse-heads launch, passed by name -- widening it to
    # probabilities, values, samples and results is left to a change of its own
    FC.twin_moves(OT, 512, lambda ea: hip.search(ea, 50), lambda ec, oc: ec.heads_softmax(ec.leaf_heads_sparse(
        hip.forward_features_nhwc8(hip.to_nhwc8(oc), key=2), hip.head_rows, hip.head2_b)), 50, 3, searched=('counts',), finished=('counters',),
        cpuct=1.25, fpu_reduction=0.2, add_root_noise=True, add_root_temp=True, seed=29)


def test_ot_sparse_heads_vs_fp64():
    """azg_leaf_heads_sparse_f16 on othello leaves: valid-action and value logits against the fp64 network, -inf elsewhere"""
    from alphazero_general_amd.engine import DeviceEngine
    args, sd, ref, x, o = F.reference('othello_64x4')
    hip = F.wrapper('othello_64x4', args, sd)._hip
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
