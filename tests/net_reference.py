"""An fp64 reference of the network the MFMA kernels compute, and the error measure they are held to (test infrastructure, CPU only).

The kernels of csrc/azg_conv.h evaluate `FoldedResNet` (nnet.py): BatchNorms folded into the convolutions, the pre-activation affine of
every block, and both dense chains collapsed to one affine map each.  `Ref` restates that forward in float64 and returns every stage a
kernel can be compared at: the tower's final stream, the two 1x1 head convolutions (the factorised heads' features), the policy and value
LOGITS and their softmaxes.

Why logits.  A probability bar cannot see what matters on nearly flat policies (a swapped output subtile moves p by 1e-3), so the bar is
on centred logits:  err = max over rows and outputs of |c(hip) - c(ref)|, c() subtracting each row's mean, held to
err <= TAU * scale with scale = the mean over rows of the fp64 logits' row std, separately for policy and value.  The tower stream and
the head features are held per element relative to the fp64 tensor's RMS, reported per border class and per board slot of the
workgroup tile, so that a bug confined to a class or a slot shows where it lives.

Where the numbers come from.  `Ref.forward(..., emulate=...)` is an ideal fp16 implementation with the kernels' rounding points
(fp16 weights, input planes, pre-activation affine, every layer's output, the residual stream, the head features, the collapsed head
matrices; wide accumulation).  tests/test_net_reference_cpu.py holds the emulation to TAU / 4 and a catalogue of simulated kernel bugs
(`Ref.forward(..., bug=...)`) to >= 3 TAU on every BASELINE network, so the bar keeps headroom both ways on every CPU run.

Weights are filled by integer hashing (as tests/net_pins.det_fill: exact on every host, no RNG, no libm) at three scales: 'trained'
(policy and value logits spread like a trained network's: mean row std in [2, 8), asserted), 'low' (the scale of the suite's
torch-initialised networks, nearly flat policies) and 'large' (the largest tower activation in [2^11, 2^14): fp16 conversion neither
saturates nor overflows).  The scales are powers of two applied where the network is positively homogeneous, so they are exact."""
import importlib

import numpy as np
import torch
import torch.nn.functional as F

# Calibration (tests/test_net_reference_cpu.py, trained fill, 301 boards per BASELINE network): the fp16 emulation reaches at most 0.0044
# of the logit scale (trimok value head), so TAU >= 4 * 0.0044 = 0.0177; the smallest catalogued bug, every logit scaled by 1.02, reaches
# 0.056 on connect4 128 x 8, so TAU <= 0.056 / 3 = 0.0187.  The stream's emulated error is at most 0.0109 of its RMS (TAU_STREAM >= 0.044).
TAU = 0.018            # centred logits: err <= TAU * scale (policy and value separately)
TAU_STREAM = 0.05      # tower stream and head features: max |hip - ref| <= TAU_STREAM * rms(ref), per border class and per tile slot
P_FLOOR = 1e-30        # probabilities below this are compared as "underflowed", not in log space

CLASSES = ('interior', 'top', 'bottom', 'left', 'right')
# BASELINE.md's networks: (key, env module, nnet args name)
BASELINE = [('connect4_128x8', 'connect4', 'CONNECT4_NET_ARGS'), ('connect4_32x4', 'connect4', 'DEFAULT_NET_ARGS'),
            ('brandubh_64x4', 'brandubh', 'BRANDUBH_NET_ARGS'), ('trimok_32x4', 'trimok', 'DEFAULT_NET_ARGS')]


def game_cls(env):
    return importlib.import_module('alphazero_general_amd.envs.' + env).Game


def net_args(argname, **over):
    from alphazero_general_amd import nnet as N
    from alphazero_general_amd.utils import dotdict
    a = dotdict(dict(getattr(N, argname)))
    a.update(over)
    return a


# ------------------------------------------------------------------------------------------------------------ weights
def _hash_unit(n, salt):
    """n values in (-0.5, 0.5) with 16 bits each, from the element index and a salt by integer hashing"""
    j = np.arange(n, dtype=np.uint64)
    h = (j * np.uint64(2654435761) + np.uint64(salt) * np.uint64(40503) * np.uint64(65599)) & np.uint64(0xFFFFFFFF)
    h = ((h ^ (h >> np.uint64(15))) * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    h = ((h ^ (h >> np.uint64(13))) * np.uint64(3266489917)) & np.uint64(0xFFFFFFFF)
    return ((h >> np.uint64(8)) & np.uint64(0xFFFF)).astype(np.float64) / 65536.0 - 0.5


def hash_fill(sd, salt=0):
    """a ResNet state_dict of unit gain: He-like stem, head and Linear weights (a power of two times the uniform), residual branches at
    half that gain, BatchNorms with spread statistics"""
    out = {}
    for i, k in enumerate(sorted(sd)):
        t = sd[k]
        if not t.dtype.is_floating_point:
            out[k] = t.clone()
            continue
        u = _hash_unit(t.numel(), 1 + i + 977 * salt)
        if k.endswith('running_var'):
            x = np.abs(u) * 1.5 + 0.5
        elif k.endswith('running_mean') or k.endswith('.bias'):
            x = u * 0.5
        elif 'bn' in k and k.endswith('.weight'):
            x = u * 0.25 + 1.0
        else:
            fan = max(int(t[0].numel()), 1)
            x = u * 2.0 ** (2 - fan.bit_length() // 2)                         # uniform of std ~ 1.15 / sqrt(fan)
            if k.startswith('resnet.'):                                         # residual branches at half that: the stream stays
                x = x * 0.5                                                     # dominated by its identity path, as in trained towers
        out[k] = torch.from_numpy(x.reshape(tuple(t.shape))).to(t.dtype)
    return out


def _linears(prefix, sd):
    return sorted({int(k.split('.')[1]) for k in sd if k.startswith(prefix + '.') and k.endswith('.weight')})


def scale_fill(sd, tower=0, policy=0, value=0):
    """exact power-of-two rescaling of a ResNet state_dict: the tower stream (and head features) by 2^tower -- stem conv weights and every
    BN shift in the tower and the head convs (the network is positively homogeneous there) -- with the dense chains' inner biases following
    and their last weights compensating; then the policy / value logits by 2^policy / 2^value (last Linear weight and bias)."""
    out = {k: v.clone() for k, v in sd.items()}
    g = 2.0 ** tower
    out['conv1.weight'] *= g
    for k in out:
        if ('bn' in k) and (k.endswith('running_mean') or k.endswith('.bias')):
            out[k] *= g
    for pre, e in (('pi_fc', policy), ('v_fc', value)):
        idx = _linears(pre, out)
        for i in idx[:-1]:
            out['%s.%d.bias' % (pre, i)] *= g
        out['%s.%d.weight' % (pre, idx[-1])] *= 2.0 ** e / g
        out['%s.%d.bias' % (pre, idx[-1])] *= 2.0 ** e
    return out


FILLS = {'trained': (2.0, 8.0), 'low': (1 / 16, 1 / 4)}      # target window of the mean row std of the logits (a factor 4 wide: a power of two fits)
LARGE = (2.0 ** 11, 2.0 ** 14)                                 # 'large': window of the largest tower activation; logits as 'trained'


def make_state(env, args, fill='trained', salt=0, probe=None):
    """(ResNet state_dict float32, Ref) for a fill: the powers of two are chosen on the probe boards (default: `boards(env)`) and the
    resulting fp64 network is asserted to meet its window (the fixture cannot quietly go flat or saturate)."""
    from alphazero_general_amd.nnet import ResNet
    G = game_cls(env)
    net = ResNet(tuple(G.observation_size()), G.action_size(), G.num_players() + G.has_draw(), args)
    base = hash_fill(net.state_dict(), salt)
    x = torch.from_numpy(boards(env)) if probe is None else probe
    o = Ref.from_state(net, base).forward(x)
    lo, hi = FILLS['low' if fill == 'low' else 'trained']
    up = lambda target, have: int(np.ceil(np.log2(target / have)))          # the power of two that lifts `have` into [target, 2 target)
    sd = scale_fill(base, up(LARGE[0], o['act_max']) if fill == 'large' else 0, up(lo, row_std(o['pi'])), up(lo, row_std(o['v'])))
    ref = Ref.from_state(net, sd)
    o = ref.forward(x)
    for name in ('pi', 'v'):
        s = row_std(o[name])
        assert lo <= s < hi, (env, fill, name, s)
        if fill != 'low':
            assert 2.0 <= s < 8.0, (env, fill, name, s)
    if fill == 'large':
        assert LARGE[0] <= o['act_max'] < LARGE[1], (env, o['act_max'])
    return {k: v.float() for k, v in sd.items()}, ref


def kernel_head_path(ref):
    """the head path HipResNet takes for this network: 'fact' (factorised: 16 + 16 head channels, features then the dense chains) or
    'collapsed' (one [H*W*CH, A + NV] matrix: the fused heads and the wide-head kernel)"""
    fused = ref.A + ref.NV <= 16 and ref.CH == 128
    return 'fact' if not fused and ref.vc == 16 and ref.head_w.shape[0] - ref.vc == 16 else 'collapsed'


def row_std(logits):
    """mean over rows of the row std of a logits tensor: the `scale` of the bar"""
    return float(logits.double().std(dim=1, unbiased=False).mean())


# ------------------------------------------------------------------------------------------------------------ inputs
def boards(env, n=301, seed=0):
    """n boards of `env` ([n, C, H, W] float32): the empty board, all-ones planes, terminal positions of random playouts, random 0/1 planes
    in every input channel, and positions of random playouts.  The default n = 301 = 7 * 43 is coprime to every tile size (1, 2, 4, 5
    boards), so a batch that repeats the set puts every board in every slot of a tile."""
    G = game_cls(env)
    C, H, W = G.observation_size()
    rng = np.random.RandomState(seed)
    out = [G().observation(), np.ones((C, H, W), np.float32)]
    terminal = []
    while len(terminal) < 12:
        g = G()
        for _ in range(G.max_turns() + 1):
            v = np.flatnonzero(g.valid_moves())
            if g.win_state().any() or len(v) == 0:
                break
            g.play_action(int(rng.choice(v)))
        terminal.append(g.observation())
    out += terminal
    out += list(rng.randint(0, 2, size=(40, C, H, W)).astype(np.float32))
    while len(out) < n:
        g = G()
        for _ in range(rng.randint(0, G.max_turns())):
            v = np.flatnonzero(g.valid_moves())
            if g.win_state().any() or len(v) == 0:
                break
            g.play_action(int(rng.choice(v)))
        out.append(g.observation())
    return np.array(out[:n], np.float32)


def border_class(H, W):
    """[H, W] index into CLASSES, as the tower's five-class tiling (TowerGeom::pixel_class): rows own the corners"""
    c = np.zeros((H, W), np.int64)
    c[:, 0], c[:, W - 1] = 3, 4
    c[0, :], c[H - 1, :] = 1, 2
    return c


# ------------------------------------------------------------------------------------------------------------ the fp64 forward
def r16(t):
    return t.to(torch.float16).to(torch.float64)


class Ref:
    """FoldedResNet's parameters in float64 and its forward, optionally as an ideal fp16 implementation (`emulate` = 'fact' | 'collapsed':
    which head path) and optionally with one simulated kernel bug."""

    def __init__(self, folded):
        d = lambda t: t.detach().to(torch.float64).cpu()
        self.shape = folded.shape
        self.stem_w, self.stem_b = d(folded.stem_w), d(folded.stem_b)
        self.blocks = [(d(folded.pre_scale[i]), d(folded.pre_shift[i]), d(folded.w1[i]), d(folded.b1[i]), d(folded.w2[i]))
                       for i in range(len(folded.w1))]
        self.head_w, self.head_b, self.vc = d(folded.head_w), d(folded.head_b), folded.vc
        self.Wv, self.bv = d(folded.v_fc.weight), d(folded.v_fc.bias)
        self.Wp, self.bp = d(folded.pi_fc.weight), d(folded.pi_fc.bias)
        self.CH, self.A, self.NV = self.stem_w.shape[0], self.Wp.shape[0], self.Wv.shape[0]

    @classmethod
    def from_state(cls, net, sd):
        """fold a ResNet (module of the right architecture) loaded with `sd`, all in float64"""
        import copy
        from alphazero_general_amd.nnet import FoldedResNet
        m = copy.deepcopy(net).double().eval()
        m.load_state_dict({k: v.double() if v.dtype.is_floating_point else v for k, v in sd.items()})
        ref = cls(FoldedResNet(m))
        ref.Wv, ref.bv = cls._chain64(m.v_fc)          # (FoldedResNet collapses the dense chains into fp32 Linear modules)
        ref.Wp, ref.bp = cls._chain64(m.pi_fc)
        return ref

    @staticmethod
    def _chain64(seq):
        W, b = None, None
        for mod in seq:
            if isinstance(mod, torch.nn.Linear):
                w, c = mod.weight.detach().double(), mod.bias.detach().double()
                W, b = (w, c) if W is None else (w @ W, w @ b + c)
        return W, b

    @property
    def depth(self):
        return len(self.blocks)

    def _conv(self, x, w, b, layer, bug):
        y = F.conv2d(x, w, b, padding=1)
        if bug and bug[0] == 'tap' and bug[1] == layer:                  # the taps of one direction dropped for one border class
            H, W = self.shape[1:]
            cls = CLASSES.index(bug[2])
            dy, dx = {'interior': (-1, None), 'top': (1, None), 'bottom': (-1, None), 'left': (None, 1), 'right': (None, -1)}[bug[2]]
            wb = w.clone()
            if dy is not None:
                wb[:, :, dy + 1, :] = 0
            else:
                wb[:, :, :, dx + 1] = 0
            yb = F.conv2d(x, wb, b, padding=1)
            m = torch.from_numpy(border_class(H, W) == cls)
            y = torch.where(m, yb, y)
        return y

    def forward(self, x, emulate=None, bug=None):
        """x [B, C, H, W] -> dict(stream [B, CH, H, W], feat [B, vc + pc, H, W] (value channels, then policy), pi / v logits, P / V
        softmaxes, act_max = the largest |activation| of the tower).  emulate='fact' | 'collapsed': fp16 storage at the kernels'
        rounding points with that head path.  bug: a tuple naming one simulated kernel bug (see BUGS)."""
        em = emulate is not None
        q = r16 if em else (lambda t: t)
        x = q(torch.as_tensor(x).to(torch.float64))
        nodrop = lambda b, kind, layer: None if bug and bug[0] == kind and bug[1] == layer else b
        amax = 0.0
        s = F.relu(q(self._conv(x, q(self.stem_w), nodrop(self.stem_b, 'nobias', 0), 0, bug)))
        amax = max(amax, float(s.abs().max()))
        for i, (ps, pt, w1, b1, w2) in enumerate(self.blocks):
            if bug and bug[0] == 'pixel' and bug[1] == 2 * i:
                s = self._move_pixel(s, bug[2])
            pt_ = torch.zeros_like(pt) if bug and bug[0] == 'noshift' and bug[1] == i else pt
            t = F.relu(q(s * q(ps) + q(pt_)))
            u = F.relu(q(self._conv(t, q(w1), nodrop(b1, 'nobias', 2 * i + 1), 2 * i + 1, bug)))
            s = q(q(self._conv(u, q(w2), None, 2 * i + 2, bug)) + s)
            amax = max(amax, float(t.abs().max()), float(u.abs().max()), float(s.abs().max()))
        if bug and bug[0] == 'pixel' and bug[1] == 2 * self.depth:
            s = self._move_pixel(s, bug[2])
        B = s.shape[0]
        h = F.conv2d(s, q(self.head_w), self.head_b)
        if emulate == 'fact':
            feat = q(h)
            v = torch.flatten(feat[:, :self.vc], 1) @ q(self.Wv).t() + self.bv
            pi = torch.flatten(feat[:, self.vc:], 1) @ q(self.Wp).t() + self.bp
        elif emulate == 'collapsed':                      # the collapsed [H*W*CH, A + NV] matrix of the wide / fused heads, in fp16
            feat = h
            Wc, bc = self.collapsed()
            lg = s.permute(0, 2, 3, 1).reshape(B, -1) @ q(Wc) + bc
            pi, v = lg[:, :self.A], lg[:, self.A:]
        else:
            feat = h
            v = torch.flatten(h[:, :self.vc], 1) @ self.Wv.t() + self.bv
            pi = torch.flatten(h[:, self.vc:], 1) @ self.Wp.t() + self.bp
        pi, v = self._head_bug(pi, v, bug)
        return dict(stream=s, feat=feat, pi=pi, v=v, P=torch.softmax(pi, 1), V=torch.softmax(v, 1), act_max=amax)

    def collapsed(self):
        """the heads as ONE affine map of the final stream (nnet.HipResNet): W [H*W*CH (pos-major), A + NV], b [A + NV]"""
        HW, CH, vc = self.shape[1] * self.shape[2], self.CH, self.vc
        hw, hb = self.head_w.reshape(-1, CH), self.head_b
        fv = torch.einsum('ocp,ck->pko', self.Wv.reshape(self.NV, vc, HW), hw[:vc])
        fp = torch.einsum('ocp,ck->pko', self.Wp.reshape(self.A, -1, HW), hw[vc:])
        bv = self.bv + torch.einsum('ocp,c->o', self.Wv.reshape(self.NV, vc, HW), hb[:vc])
        bp = self.bp + torch.einsum('ocp,c->o', self.Wp.reshape(self.A, -1, HW), hb[vc:])
        return torch.cat([fp, fv], 2).reshape(HW * CH, -1), torch.cat([bp, bv])

    def _move_pixel(self, s, yx):
        y, x = yx
        W = s.shape[3]
        s = s.clone()
        s[:, :, y, x] = s[:, :, y, x + 1 if x + 1 < W else x - 1]
        return s

    def _head_bug(self, pi, v, bug):
        if not bug:
            return pi, v
        A = self.A
        if bug[0] == 'swap':                              # two 16-output subtiles exchanged
            a, b = bug[1], bug[2]
            pi = pi.clone()
            pi[:, a * 16:a * 16 + 16], pi[:, b * 16:b * 16 + 16] = pi[:, b * 16:b * 16 + 16].clone(), pi[:, a * 16:a * 16 + 16].clone()
        elif bug[0] == 'zero_last':                       # the last (partial) policy subtile never written
            pi = pi.clone()
            pi[:, (A - 1) // 16 * 16:] = 0
        elif bug[0] == 'value_off_by_one':                # the value outputs read one column early (the last policy logit first)
            v = torch.cat([pi[:, A - 1:], v[:, :-1]], 1)
        elif bug[0] == 'scale':                           # every logit off by a common factor (an epilogue scale, a wrong fold)
            pi, v = pi * bug[1], v * bug[1]
        return pi, v


def bugs(ref):
    """the catalogue of simulated kernel bugs for a network: (name, bug tuple)"""
    H, W = ref.shape[1:]
    L = 2 * ref.depth
    out = []
    for layer in sorted({0, L // 2 + (L // 2) % 2 - 1 if L > 1 else 0, L}):          # first, a middle conv1, last
        for c in CLASSES:
            out.append(('tap_%s_layer%d' % (c, layer), ('tap', layer, c)))
    out.append(('pixel_from_neighbour_mid', ('pixel', 2 * (ref.depth // 2), (H // 2, W // 2))))
    out.append(('pixel_from_neighbour_last', ('pixel', L, (H - 1, 0))))
    out.append(('no_stem_bias', ('nobias', 0)))
    if ref.depth:
        out.append(('no_conv1_bias_mid', ('nobias', 2 * (ref.depth // 2) + 1)))
        out.append(('no_pre_shift_mid', ('noshift', ref.depth // 2)))
    if ref.A >= 48:
        out.append(('swap_subtiles_1_2', ('swap', 1, 2)))
    out.append(('zero_last_subtile', ('zero_last',)))
    out.append(('value_off_by_one', ('value_off_by_one',)))
    out.append(('logit_scale_1.02', ('scale', 1.02)))
    return out


# ------------------------------------------------------------------------------------------------------------ the measure
def centred(t):
    t = t.double()
    return t - t.mean(dim=1, keepdim=True)


def logit_err(hip, ref):
    """(err, scale, err / (TAU * scale)) for one head: err = max |c(hip) - c(ref)|, scale = mean row std of the fp64 logits"""
    hip, ref = hip.detach().double().cpu(), ref.detach().double().cpu()
    assert hip.shape == ref.shape, (hip.shape, ref.shape)
    assert torch.isfinite(hip).all()
    err, scale = float((centred(hip) - centred(ref)).abs().max()), row_std(ref)
    return err, scale, err / (TAU * scale)


def logprob_err(p_hip, p_ref, scale):
    """probabilities against the fp64 softmax in log space: centred log p over the entries where p_ref > P_FLOOR (there the bar is the
    logits' bar: centring removes log-sum-exp); elsewhere p_hip must be <= P_FLOOR.  -> (err, err / (TAU * scale))"""
    p_hip, p_ref = p_hip.detach().double().cpu(), p_ref.detach().double().cpu()
    live = p_ref > P_FLOOR
    assert (p_hip[~live] <= P_FLOOR).all(), 'probabilities the fp64 network underflows are not small'
    assert (p_hip[live] > 0).all(), 'a probability the fp64 network keeps is zero'
    lh, lr = torch.where(live, p_hip.clamp_min(1e-300).log(), 0.0), torch.where(live, p_ref.log(), 0.0)
    n = live.sum(1, keepdim=True)
    ch = lh - (lh.sum(1, keepdim=True) / n)
    cr = lr - (lr.sum(1, keepdim=True) / n)
    err = float(torch.where(live, (ch - cr).abs(), 0.0).max())
    return err, err / (TAU * scale)


def logits_bar(name, pi_hip, v_hip, o):
    """dict of the logit errors of both heads against the fp64 output `o` (no assertion)"""
    ep, sp, rp = logit_err(pi_hip, o['pi'])
    ev, sv, rv = logit_err(v_hip, o['v'])
    return dict(case=name, rows=int(o['pi'].shape[0]), err_policy=ep, scale_policy=sp, ratio_policy=rp, err_value=ev, scale_value=sv,
                ratio_value=rv, tau=TAU)


def stream_report(hip, ref, tile=1):
    """hip, ref: [B, K, H, W] (any dtype).  Per-element |hip - ref| / rms(ref): max per border class and per tile slot (board index mod
    `tile`).  -> dict(rms, by_class {name: err}, by_slot [err], max, ratio = max / TAU_STREAM)"""
    hip, ref = hip.detach().double().cpu(), ref.detach().double().cpu()
    assert hip.shape == ref.shape, (hip.shape, ref.shape)
    assert torch.isfinite(hip).all()
    rms = float(ref.pow(2).mean().sqrt())
    e = (hip - ref).abs() / rms                                   # [B, K, H, W]
    cls = torch.from_numpy(border_class(*ref.shape[2:]))
    per_px = e.amax(dim=1)                                        # [B, H, W]
    by_class = {c: float(per_px[:, cls == i].max()) if bool((cls == i).any()) else 0.0 for i, c in enumerate(CLASSES)}
    slots = torch.arange(ref.shape[0]) % tile
    by_slot = [float(per_px[slots == k].max()) if bool((slots == k).any()) else 0.0 for k in range(tile)]
    m = float(per_px.max())
    return dict(rms=rms, by_class=by_class, by_slot=by_slot, max=m, ratio=m / TAU_STREAM)
