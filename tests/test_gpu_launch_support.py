"""azg_launch_support against the launches themselves: for every (game, tower width) the set-up call of the persistent wide-head search
(exact and sparse heads) and a stand-alone tower launch succeed exactly where the mask has their bit and return AZG_E_UNSUPPORTED
elsewhere; and the wide arena launch, whose tile is the one-game row of the pair's persistent tiles, searches the trees the host-split
arena path searches -- on the k-split row (brandubh x 64) and the three-pixel-group row (gobang x 32)."""
import ctypes as C

import pytest

import test_gpu_arena_wide as aw

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('ch', [32, 64, 128])
@pytest.mark.parametrize('name', ['connect4', 'brandubh', 'trimok', 'othello', 'gobang'])
def test_launches_exist_exactly_where_the_mask_says(name, ch):
    import torch
    from alphazero_general_amd import _abi, nnet as N
    from alphazero_general_amd.engine import DeviceEngine
    from alphazero_general_amd.utils import dotdict
    Game = aw._game(name)
    gid = Game.AZG_GAME_ID
    L = _abi.lib()
    mask = L.azg_launch_support(gid, ch)
    assert mask >= 0
    torch.manual_seed(3)
    na = dotdict(dict(N.DEFAULT_NET_ARGS)); na['num_channels'] = ch; na['depth'] = 1
    w = N.NNetWrapper(Game, na, device='cuda:0', dtype=torch.float16, backend='torch')
    h = N.HipResNet(N.FoldedResNet(w.nnet).to('cuda:0'), gid, 'cuda:0')
    gi = _abi.game_info(gid)
    hw = gi.obs_h * gi.obs_w
    feat_k = (hw * 16 + 31) // 32 * 32
    assert h.fact_head or (name, ch) == ('connect4', 128)            # (fused heads there: no factorised operands, and no wide launch to read them)
    dummy = torch.zeros(64, device='cuda:0')
    vp = lambda t: C.c_void_p(t.data_ptr())
    op = lambda a: vp(getattr(h, a, dummy))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    tower = (vp(h.tower_w), vp(h.tower_b), vp(h.tower_ps), vp(h.tower_pt))
    want = lambda bit: 0 if mask & bit else _abi.E_UNSUPPORTED
    e = DeviceEngine(gid, 2)
    try:
        assert L.azg_search_wide_exact_f16(e.h, st, *tower, 1, ch, op('head1_w'), op('head1_b'), op('head2_wps'), op('head2_wv'), op('head2_b'),
                                           feat_k, 0) == want(_abi.SUPPORT_SEARCH_WIDE)
        assert L.azg_search_wide_f16(e.h, st, *tower, 1, ch, op('head1_w'), op('head1_b'), op('head_rows'), op('head2_b'),
                                     feat_k, 0) == want(_abi.SUPPORT_SEARCH_SPARSE)
        x = torch.zeros((2, hw, 8), dtype=torch.float16, device='cuda:0')
        y = torch.empty((2 * hw, ch), dtype=torch.float16, device='cuda:0')
        assert L.azg_resnet_tower_f16(st, gid, vp(x), *tower, vp(y), 2, 1, ch) == want(_abi.SUPPORT_TOWER)
        torch.cuda.synchronize()
        e.counters()                                                 # (raises on a device-side error)
    finally:
        e.close()


@pytest.mark.parametrize('name,width', [('brandubh', 64), ('gobang', 32)])
def test_wide_arena_one_game_row_equals_host_split(name, width):
    """one 4-simulation wide arena launch on 2 slots leaves the root visit counts of four host-split simulations"""
    from alphazero_general_amd.selfplay import ArenaRunner
    Game, nets = aw._nets(name, width, 2)
    counts = []
    for wide in (True, False):
        r = ArenaRunner(Game, nets, aw._args(numMCTSSims=4), num_slots=2, seed=5, use_graph=False, fused_search=wide)
        assert r.wide_search == wide
        if wide:
            r._search_wide(0)
            r._search_wide(4)
        else:
            for _ in range(4):
                r.step()
        counts.append(r.engine.root_counts().cpu().numpy())
        r.engine.counters()                                          # (raises on a device-side error)
        r.engine.close()
    assert counts[0].sum() > 0 and (counts[0] == counts[1]).all()
