"""The fp64 network reference (tests/net_reference.py) and the bar the GPU network tests hold the MFMA kernels to, checked on the CPU:
the reference equals the unfolded ResNet and the reference implementation's golden outputs; an ideal fp16 implementation with the kernels'
rounding points stays within a quarter of the bar on every BASELINE network; and a catalogue of simulated kernel bugs (a tap dropped for
one border class, a pixel read from its neighbour, a missing bias or shift, swapped or unwritten output subtiles, an off-by-one in the
value outputs, a 2 % scale error) each lands at three times the bar or more.  So the bar cannot drift into passing real bugs or failing
correct kernels without this module noticing."""
import functools
import os

import numpy as np
import pytest
import torch

import net_reference as R

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
NETS = [k for k, _, _ in R.BASELINE]


@functools.lru_cache(maxsize=None)
def _case(key):
    env, argname = {k: (e, a) for k, e, a in R.BASELINE}[key]
    sd, ref = R.make_state(env, R.net_args(argname), 'trained')
    x = torch.from_numpy(R.boards(env))
    return env, argname, sd, ref, x, ref.forward(x)


@pytest.mark.parametrize('key', NETS)
def test_reference_equals_unfolded_resnet_fp64(key):
    """FoldedResNet restated in fp64 == the architecture's own ResNet module run in fp64 (log-softmax outputs, 1e-9)"""
    from alphazero_general_amd.nnet import ResNet
    env, argname, sd, ref, x, o = _case(key)
    Gm = R.game_cls(env)
    net = ResNet(tuple(Gm.observation_size()), Gm.action_size(), Gm.num_players() + Gm.has_draw(), R.net_args(argname)).double().eval()
    net.load_state_dict({k: v.double() if v.dtype.is_floating_point else v for k, v in sd.items()})
    with torch.no_grad():
        lp, lv = net(x.double())
    assert float((torch.log_softmax(o['pi'], 1) - lp).abs().max()) <= 1e-9
    assert float((torch.log_softmax(o['v'], 1) - lv).abs().max()) <= 1e-9


@pytest.mark.parametrize('name,argname', [('default', 'DEFAULT_NET_ARGS'), ('c4train', 'CONNECT4_NET_ARGS')])
def test_reference_vs_reference_implementation_golden(name, argname):
    """the fp64 reference on the reference implementation's own outputs (tests/golden/c4_net.npz), at test_nnet_cpu.py's bar"""
    from test_nnet_cpu import fill_deterministic
    from alphazero_general_amd.nnet import ResNet
    d = dict(np.load(os.path.join(G, 'c4_net.npz')))
    Gm = R.game_cls('connect4')
    net = ResNet(tuple(Gm.observation_size()), Gm.action_size(), Gm.num_players() + Gm.has_draw(), R.net_args(argname))
    ref = R.Ref.from_state(net, fill_deterministic(net.state_dict()))
    o = ref.forward(torch.from_numpy(d['obs']))
    assert np.allclose(o['P'].numpy(), d[name + '_policy'], atol=2e-5) and np.allclose(o['V'].numpy(), d[name + '_value'], atol=2e-5)


@pytest.mark.parametrize('key', NETS)
def test_fills_meet_their_windows(key):
    """make_state asserts its own windows: trained (logit row std in [2, 8)), low (today's nearly flat scale), large (largest tower
    activation in [2^11, 2^14)); the large fill's logits are the trained fill's (the tower scale is exact and compensated)"""
    env, argname, sd, ref, x, o = _case(key)
    args = R.net_args(argname)
    _, low = R.make_state(env, args, 'low')
    assert R.row_std(low.forward(x)['pi']) < 0.25
    _, big = R.make_state(env, args, 'large')
    ob = big.forward(x)
    assert 2.0 ** 11 <= ob['act_max'] < 2.0 ** 14
    assert float((ob['pi'] - o['pi']).abs().max()) < 1e-9 * float(o['pi'].abs().max()) * 2 ** 14
    e = big.forward(x, emulate=R.kernel_head_path(big))              # fp16 storage at that scale: finite, and still within the bar
    assert all(torch.isfinite(e[k]).all() for k in ('stream', 'feat', 'pi', 'v'))
    r = R.logits_bar(key, e['pi'], e['v'], ob)
    assert r['ratio_policy'] <= 0.25 and r['ratio_value'] <= 0.25, r


@pytest.mark.parametrize('key', NETS)
def test_fp16_emulation_within_a_quarter_of_the_bar(key):
    """an ideal fp16 implementation (the kernels' rounding points, wide accumulation) on the kernel's head path: <= TAU / 4 on the
    logits, <= TAU_STREAM / 4 on the stream and the head features"""
    env, argname, sd, ref, x, o = _case(key)
    e = ref.forward(x, emulate=R.kernel_head_path(ref))
    r = R.logits_bar(key, e['pi'], e['v'], o)
    print('EMU', r)
    assert r['ratio_policy'] <= 0.25 and r['ratio_value'] <= 0.25, r
    for k in ('stream', 'feat'):
        s = R.stream_report(e[k], o[k])
        assert s['ratio'] <= 0.25, (k, s)


@pytest.mark.parametrize('key', NETS)
def test_catalogued_bugs_exceed_the_bar_threefold(key):
    env, argname, sd, ref, x, o = _case(key)
    names = []
    for name, bug in R.bugs(ref):
        ob = ref.forward(x, bug=bug)
        r = R.logits_bar(name, ob['pi'], ob['v'], o)
        assert max(r['ratio_policy'], r['ratio_value']) >= 3.0, r
        names.append(name)
    assert len([n for n in names if n.startswith('tap_')]) == 15                 # five border classes x first / middle / last layer
