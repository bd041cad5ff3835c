"""Gobang's own training net -- GOBANG_NET_ARGS, 128 channels x 8 blocks, envs/gobang/train.py -- in ONE persistent launch per move
(azg_search_wide_exact_f16 / azg_search_arena_wide_exact_f16 at (gobang, 128): a one-game tile of twelve wavefronts, the exact heads
streamed through a short register ring, csrc/azg_conv.h heads_full_stream).  Bit equality throughout, no tolerances:

  * the persistent search against select -> NNetWrapper.process -> backup on a twin engine with the same seeds, root noise and root
    temperature on, more games than CUs and a small engine, depth 8 and depth 1;
  * positions 180 or more plies in: terminal leaves and full boards through the game-sized walk mailbox;
  * the persistent arena, captured and eager, against the host-split arena at width 128 -- two nets, and a net against a raw seat --,
    the games replayed on envs.gobang;
  * routing: fused_search=True takes the persistent form, fused_search=None follows HipResNet.search_preferred, and the sparse
    persistent launch still refuses gobang."""
import pytest
import torch

import fixture_checks as FC
import test_gpu_arena_wide as W
import test_gpu_gobang as TG
import test_gpu_net_fp64 as F

pytestmark = pytest.mark.gpu
GB, DEV, A = TG.GB, TG.DEV, TG.A
KEY = 'gobang_128x8'


def _net(depth, salt=7):
    args, sd, ref, x, o = F.reference(KEY, salt=salt, depth=depth)
    net = F.wrapper(KEY, args, sd)
    assert net._hip.CH == 128 and len(net._hip.blocks) == depth and net._hip.feat_k == 3616
    return net


@pytest.mark.parametrize('B,sims,moves', [(320, 40, 3), (24, 30, 4)])
@pytest.mark.parametrize('depth', [8, 1])
def test_gb128_wide_exact_search_vs_phase_loop(depth, B, sims, moves):
    """one persistent launch per move against the per-phase loop on a twin engine: root counts, root_probs(1.0), both root values and
    the moves after every move; tape counters, counters, examples and results at the end"""
    net = _net(depth)
    assert net._hip.can_search
    FC.twin_moves(GB, B, lambda ea: net._hip.search(ea, sims, exact=True), lambda ec, oc: net.process(oc), sims, moves,
                  cpuct=4.0, fpu_reduction=0.4, add_root_noise=True, add_root_temp=True, seed=41)


def test_gb128_wide_search_deep_path():
    """64 positions 180 or more plies in (test_gpu_gobang._deep_path, on this net), 120 simulations: the
    persistent launch's walks reach terminal leaves and full boards, root counts and the deepest path equal the per-phase loop's"""
    TG._deep_path(_net(8))


@pytest.mark.parametrize('raw', [False, True])
def test_gb128_persistent_arena_equals_host_split(raw):
    """width 128: two differently seeded nets, or a net against a raw seat -- the persistent arena launch, captured and eager, plays
    exactly the games of the host-split path, and the games replay on the host env"""
    nets = TG._arena_nets(128, 1 if raw else 2)
    assert all(n._hip.CH == 128 and n._hip.fact_head for n in nets)
    seats = nets + [None] if raw else nets
    B = 24
    runs = W._forms(TG._game(), seats, W._args(), B, 7 if raw else 5, 'slot' if raw else 'agent', 150)
    W._same(runs)
    TG._arena_replay(runs[0], B)


def test_gb128_routing():
    """fused_search=True: the self-play and the arena runner take the persistent form for the 128-channel net; fused_search=None: what
    HipResNet.search_preferred says; the sparse persistent launch refuses gobang at this width too"""
    from alphazero_general_amd.engine import DeviceEngine
    from alphazero_general_amd.selfplay import ArenaRunner, SelfPlayRunner
    nets = TG._arena_nets(128, 2)
    hip = nets[0]._hip
    assert hip.can_search
    args = W._args()
    r = SelfPlayRunner(TG._game(), nets[0], args, num_slots=8, seed=3, fused_search=True)
    assert r.fused_search
    r.engine.close()
    r = SelfPlayRunner(TG._game(), nets[0], args, num_slots=8, seed=3)
    assert bool(r.fused_search) == bool(hip.search_preferred)
    r.engine.close()
    a = ArenaRunner(TG._game(), nets, args, num_slots=8, seed=3, use_graph=False, fused_search=True)
    assert a.wide_search
    a.engine.close()
    a = ArenaRunner(TG._game(), nets, args, num_slots=8, seed=3, use_graph=False)
    assert bool(a.wide_search) == bool(hip.search_preferred)
    a.engine.close()
    from alphazero_general_amd import _abi
    eng = DeviceEngine(GB, 8, cpuct=2.0, fpu_reduction=0.1, seed=5, sims_hint=8)
    with pytest.raises(_abi.AzgError) as ei:
        hip.search(eng, 8, exact=False)
    assert ei.value.code == _abi.E_UNSUPPORTED
    eng.close()


def test_gb128_tower_too_deep_is_refused():
    """LDS of the tile: image 88 704 B + search scratch 31 072 B + parameters (12 depth + 8) x 128 + 16 + 8 320 B against the 163 840 B of
    a CU -- 22 blocks fit (162 912 B), 23 do not (164 448 B) and are refused with AZG_E_INVALID_ARG at set-up"""
    from alphazero_general_amd import _abi, nnet as N
    from alphazero_general_amd.engine import DeviceEngine
    from alphazero_general_amd.utils import dotdict
    eng = DeviceEngine(GB, 8, cpuct=2.0, fpu_reduction=0.1, seed=5, sims_hint=8)
    for depth in (22, 23):
        torch.manual_seed(30 + depth)
        net = N.NNetWrapper(TG._game(), dotdict(dict(N.GOBANG_NET_ARGS, depth=depth)), device=DEV, dtype=torch.float16)
        net.refresh()
        hip = net._hip
        assert hip.CH == 128 and len(hip.blocks) == depth and hip.can_search
        if depth == 22:
            hip.search(eng, 0, exact=True)                       # one-time set-up: the tile fits
            hip.search(eng, 4, exact=True)
            assert int(eng.root_counts().sum()) > 0
        else:
            with pytest.raises(_abi.AzgError) as ei:
                hip.search(eng, 0, exact=True)
            assert ei.value.code == _abi.E_INVALID_ARG
    eng.close()
