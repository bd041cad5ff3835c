"""Every entry point of the hand-written network kernels (csrc/azg_conv.h) against the fp64 reference of tests/net_reference.py, in logit
space, at trained-scale weights: every (game, tower width) of csrc/azg_tiles.h that a BASELINE game has, every tile threshold of the device (derived from its
CU count), batches that are not a multiple of the tile and batches where workgroups loop over several tiles, depths 0 to BASELINE + 2,
the collapsed wide heads with a partial chunk, the multi-model arena launch with uneven and empty splits, and the sparse heads.  The bar
and the measure live in tests/net_reference.py (calibrated on the CPU by tests/test_net_reference_cpu.py); the measured errors go to
the network error log test_gpu_nnet.record_error keeps (nn_error.jsonl).

The persistent search launches (azg_search_f16, azg_search_wide_exact_f16, azg_search_wide_f16) need no test here: the oracle tests
(test_gpu_runner_oracle.py, test_gpu_benchsize_oracle.py, smoke()) already assert that they hand the tree exactly the bits of
NNetWrapper.process / DeviceEngine.leaf_heads_sparse, which this module holds to the fp64 reference.

The fp64 reference is computed once per network on 301 distinct boards (coprime to every tile size: a batch repeating them puts every
board in every slot of a tile) and cached for the module."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import net_reference as R

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
# (key, env, nnet args name, overrides): every (game, width) with tower rows of connect4, brandubh and trimok, plus the head paths that need their own shape
NETS = {
    'connect4_128x8': ('connect4', 'CONNECT4_NET_ARGS', {}),                          # fused heads
    'connect4_64x8': ('connect4', 'CONNECT4_NET_ARGS', dict(num_channels=64)),         # collapsed wide heads (32 head channels)
    'connect4_32x4': ('connect4', 'DEFAULT_NET_ARGS', {}),                             # factorised heads
    'brandubh_64x4': ('brandubh', 'BRANDUBH_NET_ARGS', {}),
    'brandubh_128x4': ('brandubh', 'BRANDUBH_NET_ARGS', dict(num_channels=128)),
    'brandubh_64x4_h32': ('brandubh', 'BRANDUBH_NET_ARGS', dict(value_head_channels=32, policy_head_channels=32)),   # 591 outputs: 37 subtiles
    'trimok_32x4': ('trimok', 'DEFAULT_NET_ARGS', {}),
}
# the nets of the games whose network tests live in their own modules (test_gpu_othello.py, test_gpu_gobang.py, test_gpu_gobang128.py,
# test_gpu_tictactoe.py) and run through reference / wrapper / check_network here: not parametrised in this module
GAME_NETS = {
    'othello_64x4': ('othello', 'OTHELLO_NET_ARGS', {}),
    'othello_32x4': ('othello', 'DEFAULT_NET_ARGS', {}),
    'gobang_32x4': ('gobang', 'DEFAULT_NET_ARGS', {}),
    'gobang_64x4': ('gobang', 'DEFAULT_NET_ARGS', dict(num_channels=64)),
    'gobang_128x8': ('gobang', 'GOBANG_NET_ARGS', {}),
    'tictactoe_32x4_h4': ('tictactoe', 'TICTACTOE_NET_ARGS', {}),          # 4 + 4 head channels, padded to 16 + 16
    'tictactoe_32x4': ('tictactoe', 'DEFAULT_NET_ARGS', {}),
}
# what wrapper() and check_network() hold for those games beyond the comparisons: flags of the HipResNet, its feature row and head sizes
HOLDS = {'othello': dict(flags=('fact_head',)),
         'gobang': dict(flags=('fact_head',), feat_k=3616, A=225, NV=3),
         'tictactoe': dict(flags=('fact_head', 'can_search', 'search_preferred'), feat_k=160)}
WIDTHS = {('connect4', 128): 'connect4_128x8', ('connect4', 64): 'connect4_64x8', ('connect4', 32): 'connect4_32x4',
          ('brandubh', 64): 'brandubh_64x4', ('brandubh', 128): 'brandubh_128x4', ('trimok', 32): 'trimok_32x4'}


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def net_spec(key):
    return NETS[key] if key in NETS else GAME_NETS[key]


def tile_boards(env, ch, n, cus):
    """boards per workgroup tile the stand-alone tower takes for n boards: the tests' own statement of the policy in the rows of
    csrc/azg_tiles.h, held to the library by tests/test_tile_policy_cpu.py and, for every batch run here, by check_network"""
    if env == 'connect4' and ch == 128:
        return 1 if 2 * n <= 5 * cus else 2 if n <= 5 * cus else 4
    if env in ('connect4', 'othello') and ch == 32:
        return 2 if n <= 4 * cus else 4
    if env in ('brandubh', 'othello') and ch == 64:
        return 1 if n <= 2 * cus else 2
    if env == 'trimok':
        return 2 if n <= 8 * cus else 5
    if env == 'tictactoe':
        return 1 if n <= 8 * cus else 5 if n <= 80 * cus else 16
    return {('connect4', 64): 4, ('brandubh', 128): 2, ('gobang', 32): 1, ('gobang', 64): 1, ('gobang', 128): 1}[env, ch]


def tictactoe_boards(n=301, seed=0):
    """n boards [n, 1, 3, 3] float32 (net_reference.boards needs a turn limit to size its playouts): the empty board, all ones, all
    minus ones, then records of tt_rules drawn without replacement -- full boards, won boards and unreachable ones among them"""
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'tt_rules.npz'))
    rng = np.random.RandomState(seed)
    pick = rng.choice(3 ** 9, n - 3, replace=False) * 2
    x = np.concatenate([np.zeros((1, 9)), np.ones((1, 9)), -np.ones((1, 9)), d['obs'][pick]]).astype(np.float32)
    return x.reshape(n, 1, 3, 3)


def batches(env, ch, cus):
    """B = 1, every tile threshold of this device and one board above it, a batch not a multiple of the tile, and one where the grid
    (capped at residency x CUs) loops: 16 tiles per CU of the largest tile"""
    th = {('connect4', 128): [5 * cus // 2, 5 * cus], ('connect4', 32): [4 * cus], ('brandubh', 64): [2 * cus, 4 * cus],
          ('trimok', 32): [8 * cus]}.get((env, ch), [])
    big = tile_boards(env, ch, 1 << 30, cus)
    out = {1, 37, 301} | {t for t in th} | {t + 1 for t in th} | {big * 16 * cus + 1}
    return sorted(out)


@functools.lru_cache(maxsize=None)
def reference(key, fill='trained', salt=0, depth=None):
    """(state_dict, Ref, boards [N, C, H, W] fp32, fp64 outputs) of one network"""
    env, argname, over = net_spec(key)
    over = dict(over)
    if depth is not None:
        over['depth'] = depth
    args = R.net_args(argname, **over)
    x = torch.from_numpy(tictactoe_boards() if env == 'tictactoe' else R.boards(env))
    sd, ref = R.make_state(env, args, fill, salt, probe=x)
    return args, sd, ref, x, ref.forward(x)


def wrapper(key, args, sd, fused=True):
    from alphazero_general_amd.nnet import NNetWrapper
    env = net_spec(key)[0]
    net = NNetWrapper(R.game_cls(env), args, device=DEV, backend='hip')
    net.adopt(sd)
    net.refresh()
    assert net._hip is not None
    for flag in HOLDS.get(env, {}).get('flags', ()):
        assert getattr(net._hip, flag), (key, flag)
    if not fused:
        net._hip.fused_head = False
    return net


def record(rec):
    from test_gpu_nnet import record_error
    print('NNERR64 ' + json.dumps(rec))
    record_error(rec)


def _idx(N, B):
    return torch.arange(B) % N


def _sel(B, n=602):
    """rows whose tower stream is compared: the first and the last n (the looping workgroups' tiles are at the end)"""
    return torch.unique(torch.cat([torch.arange(min(B, n)), torch.arange(max(0, B - n), B)]))


def tower_stream(hip, x8):
    """azg_resnet_tower_f16 as forward_nhwc8 calls it -> [B, CH, H, W] float32"""
    vp = lambda q: C.c_void_p(q.data_ptr())
    B = x8.shape[0]
    s = hip._buffers(B, key=77)
    hip._check(hip.L.azg_resnet_tower_f16(C.c_void_p(torch.cuda.current_stream().cuda_stream), hip.game, vp(x8), vp(hip.tower_w),
                                          vp(hip.tower_b), vp(hip.tower_ps), vp(hip.tower_pt), vp(s), int(B), len(hip.blocks), int(hip.CH)))
    return s


def _stream_cmp(name, hip, s, o, idx, tile):
    H, W = o['stream'].shape[2:]
    sel = _sel(idx.numel())
    got = s.reshape(-1, H, W, hip.CH)[sel].permute(0, 3, 1, 2).float().cpu()
    rep = R.stream_report(got, o['stream'][idx[sel]], tile=tile)
    # (slot of a selected row = row index mod tile: the rows are selected as absolute batch indices)
    slots = sel % tile
    per_px = ((got.double() - o['stream'][idx[sel]]).abs() / rep['rms']).amax(dim=(1, 2, 3))
    rep['by_slot'] = [float(per_px[slots == k].max()) if bool((slots == k).any()) else 0.0 for k in range(tile)]
    record(dict(case=name, what='tower_stream', tile=tile, **rep, tau=R.TAU_STREAM))
    assert rep['ratio'] <= 1.0, (name, rep)
    assert max(rep['by_slot']) <= R.TAU_STREAM, (name, rep)


def _logits_cmp(name, pi, v, o, idx):
    r = R.logits_bar(name, pi, v, {'pi': o['pi'][idx], 'v': o['v'][idx]})
    record(dict(what='logits', **r))
    assert r['ratio_policy'] <= 1.0 and r['ratio_value'] <= 1.0, r


def _probs_cmp(name, p, v, o, idx):
    ep, rp = R.logprob_err(p, o['P'][idx], R.row_std(o['pi'][idx]))
    ev, rv = R.logprob_err(v, o['V'][idx], R.row_std(o['v'][idx]))
    record(dict(case=name, what='probabilities', rows=int(idx.numel()), err_policy=ep, ratio_policy=rp, err_value=ev, ratio_value=rv, tau=R.TAU))
    assert rp <= 1.0 and rv <= 1.0, (name, rp, rv)
    assert float((p.double().sum(1) - 1).abs().max()) < 1e-4


def check_network(name, key, args, sd, ref, x, o, sizes, fused=True, stream=True):
    """every entry point a network of this shape reaches, at every batch size in `sizes`"""
    net = wrapper(key, args, sd, fused)
    hip = net._hip
    env = net_spec(key)[0]
    for k, want in HOLDS.get(env, {}).items():
        assert k == 'flags' or getattr(hip, k) == want, (key, k, want)
    N = x.shape[0]
    xg = x.to(DEV)
    for B in sizes:
        idx = _idx(N, B)
        xb = xg[idx.to(DEV)].contiguous()
        x8 = hip.to_nhwc8(xb)
        tile = tile_boards(env, hip.CH, B, _cus())
        tile3 = (C.c_int32 * 3)()
        assert hip.L.azg_tower_tile(hip.game, int(hip.CH), int(B), _cus(), tile3) == 0 and tile3[0] == tile, (key, B, list(tile3), tile)
        tag = '%s_B%d' % (name, B)
        if stream:
            _stream_cmp(tag, hip, tower_stream(hip, x8), o, idx, tile)
        if hip.fact_head:                                      # azg_resnet_tower_features_f16: head features and their zero padding
            feat = hip.forward_features_nhwc8(x8).float().cpu().reshape(B, 2, hip.feat_k)
            HW, vc, pc = hip.HW, ref.vc, ref.head_w.shape[0] - ref.vc
            assert float(feat[:, :, HW * 16:].abs().max() if hip.feat_k > HW * 16 else 0.0) == 0.0     # the rows' padding behind HW x 16 features
            f = feat[:, :, :HW * 16].reshape(B, 2, HW, 16)                                               # [B, policy | value, pos, 16]
            assert float(f[:, 0, :, pc:].abs().max() if pc < 16 else 0.0) == 0.0                         # the padded head channels: exact zeros
            assert float(f[:, 1, :, vc:].abs().max() if vc < 16 else 0.0) == 0.0
            got = torch.cat([f[:, 1, :, :vc], f[:, 0, :, :pc]], 2).permute(0, 2, 1).reshape(B, vc + pc, *o['feat'].shape[2:])   # value channels, then policy
            sel = _sel(B)
            rep = R.stream_report(got[sel], o['feat'][idx[sel]], tile=1)
            record(dict(case=tag, what='head_features', **rep, tau=R.TAU_STREAM))
            assert rep['ratio'] <= 1.0, (tag, rep)
        if hip.wide_head:                                      # the logits: factorised or collapsed wide heads
            lg = hip.forward_logits_nhwc8(x8).float().cpu()
            _logits_cmp(tag + ('_fact' if hip.fact_head else '_wide'), lg[:, :hip.A], lg[:, hip.A:hip.A + hip.NV], o, idx)
        p, v = net.process(xb)                                 # NNetWrapper.process: probabilities (fused heads: only these)
        _probs_cmp(tag + '_process', p.cpu(), v.cpu(), o, idx)


@pytest.mark.parametrize('key', list(NETS))
def test_every_network_shape_and_batch_vs_fp64(key):
    args, sd, ref, x, o = reference(key)
    env = NETS[key][0]
    sizes = batches(env, args.num_channels, _cus())
    check_network(key, key, args, sd, ref, x, o, sizes)


def test_connect4_128_wide_heads_vs_fp64():
    """connect4 x 128 with the heads unfused: azg_resnet_tower_f16 + azg_policy_value_heads_f16 (collapsed, one 16-output subtile)"""
    args, sd, ref, x, o = reference('connect4_128x8')
    check_network('connect4_128x8_unfused', 'connect4_128x8', args, sd, ref, x, o, [1, 301, 5 * _cus() + 1], fused=False)


@pytest.mark.parametrize('fill', ['low', 'large'])
@pytest.mark.parametrize('gw', sorted(WIDTHS))
def test_low_and_large_fills_vs_fp64(gw, fill):
    """one network per (game, width) at today's nearly flat scale and with tower activations of 2^11 .. 2^14 (no fp16 saturation)"""
    key = WIDTHS[gw]
    args, sd, ref, x, o = reference(key, fill)
    check_network('%s_%s' % (key, fill), key, args, sd, ref, x, o, [301])


@pytest.mark.parametrize('depth', [0, 1, 2, 'baseline+2'])
@pytest.mark.parametrize('key', ['connect4_128x8', 'brandubh_64x4', 'trimok_32x4'])
def test_depths_on_one_and_multi_board_tiles(key, depth):
    """depths 0, 1, 2 and BASELINE + 2 on a one-board (or the smallest) tile and a multi-board tile.  The ABI accepts nblocks >= 0;
    depth 0 is the stem alone."""
    env, argname, over = NETS[key]
    d = R.net_args(argname, **over).depth + 2 if depth == 'baseline+2' else depth
    args, sd, ref, x, o = reference(key, depth=d)
    cus = _cus()
    sizes = {'connect4': [37, 5 * cus + 1], 'brandubh': [37, 4 * cus + 1], 'trimok': [37, 8 * cus + 1]}[env]
    check_network('%s_depth%d' % (key, d), key, args, sd, ref, x, o, sizes)


@pytest.mark.parametrize('splits', [(0, 1, 300), (150, 151), (301, 0, 0, 0), (37, 0, 5, 259), (0, 0, 301), 'big'])
def test_multi_model_launch_vs_fp64(splits):
    """azg_resnet_policy_value_multi_f16 (HipResNet.forward_models): every row against ITS model's fp64 network; splits with empty
    models, a single row, counts that are not a multiple of the tile, one model holding everything"""
    from alphazero_general_amd.nnet import HipResNet
    if splits == 'big':
        n = 5 * _cus() + 3
        splits = (n // 3, 0, n - n // 3)
    refs = [reference('connect4_128x8', salt=m) for m in range(len(splits))]
    nets = [wrapper('connect4_128x8', r[0], r[1]) for r in refs]
    B = sum(splits)
    x = refs[0][3]
    idx = _idx(x.shape[0], B)
    x8 = nets[0]._hip.to_nhwc8(x.to(DEV)[idx.to(DEV)].contiguous())
    pol = torch.full((B, 7), float('nan'), dtype=torch.float32, device=DEV)
    val = torch.full((B, 3), float('nan'), dtype=torch.float32, device=DEV)
    rpm = torch.tensor(splits, dtype=torch.int32, device=DEV)
    HipResNet.forward_models([n._hip for n in nets], x8, pol, val, rpm)
    pol, val = pol.cpu(), val.cpu()
    r0 = 0
    for m, n in enumerate(splits):
        if n:
            _probs_cmp('multi_%s_model%d' % ('-'.join(map(str, splits)), m), pol[r0:r0 + n], val[r0:r0 + n], refs[m][4], idx[r0:r0 + n])
        r0 += n


@pytest.mark.parametrize('key', ['connect4_32x4', 'brandubh_64x4', 'trimok_32x4'])
def test_sparse_heads_vs_fp64(key):
    """azg_leaf_heads_sparse_f16 (DeviceEngine.leaf_heads_sparse): the valid-action and value logits of every slot's selected leaf against
    the fp64 network on that leaf's observation; invalid actions are -inf.  Valid moves come from the host rules of the leaf state."""
    from alphazero_general_amd.engine import DeviceEngine
    args, sd, ref, x, o = reference(key)
    net = wrapper(key, args, sd)
    hip = net._hip
    env = NETS[key][0]
    Gm = R.game_cls(env)
    gid, B = Gm.AZG_GAME_ID, 96
    e = DeviceEngine(gid, B, seed=5, cpuct=1.25, fpu_reduction=0.2, example_capacity=1 << 16, sims_hint=8, device=0)
    oc = e.new_obs(torch.float32)
    lgs, obs, valid = [], [], []
    for move in range(3):
        for s in range(8):
            e.select(oc)
            lg = e.leaf_heads_sparse(hip.forward_features_nhwc8(hip.to_nhwc8(oc)), hip.head_rows, hip.head2_b)
            leaves = e.get_leaf_states(full=True)
            for i, lf in enumerate(leaves):
                g = Gm.from_azg_state(*lf) if env == 'brandubh' else Gm.from_azg_state(*lf[:3])
                if g.win_state().any():
                    continue
                lgs.append(lg[i].cpu()); obs.append(oc[i].cpu()); valid.append(torch.from_numpy(np.asarray(g.valid_moves(), bool)))
            pol, val = e.heads_softmax(lg)
            e.backup(pol, val)
        e.advance(True)
    lg, xo, valid = torch.stack(lgs), torch.stack(obs), torch.stack(valid)
    r = ref.forward(xo)
    A, NV = ref.A, ref.NV
    assert bool(torch.isneginf(lg[:, :A][~valid]).all()), 'an invalid action has a finite logit'
    assert bool(torch.isfinite(lg[:, :A][valid]).all())
    scale = R.row_std(r['pi'])
    cen = lambda t: t - (torch.where(valid, t, 0.0).sum(1, keepdim=True) / valid.sum(1, keepdim=True))
    gp, rp = torch.where(valid, lg[:, :A].double(), 0.0), torch.where(valid, r['pi'], 0.0)
    err_p = float(torch.where(valid, (cen(gp) - cen(rp)).abs(), 0.0).max())
    ev, sv, rv = R.logit_err(lg[:, A:A + NV], r['v'])
    rec = dict(case='%s_sparse' % key, what='sparse_logits', rows=int(lg.shape[0]), err_policy=err_p, scale_policy=scale,
               ratio_policy=err_p / (R.TAU * scale), err_value=ev, scale_value=sv, ratio_value=rv, tau=R.TAU)
    record(rec)
    assert lg.shape[0] > B and rec['ratio_policy'] <= 1.0 and rv <= 1.0, rec
