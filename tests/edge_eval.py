"""Synthetic evaluators for the tree edge goldens (tests/golden/{c4,br,tm}_edge.npz, made by make_goldens.py `edge`, and
{ot,gb}_edge.npz, made by the same gen_edge through make_othello_goldens.py `ot_edge` / make_gobang_goldens.py `gb_edge`).

Each returns one (policy row float32[A], value row float32[NV]) for (family, seed, stream, step), from seeded integer hashing
(splitmix64) and exact float constructions only -- no libm -- so the machine that replays a fixture computes the same rows
bit for bit without the reference.  The fixtures store crc32 of every row the generator fed, and the replayers check it.

  uniform  1 on every action: after masking and renormalising (MCTS.pyx:244-245) every valid move gets the same prior, so
           PUCT ties everywhere.  The value row is a constant draw (get_value = 0.5 exactly in the 2-player games).
  dyadic   powers of two 2^0 .. 2^-7 with repeats; values from {0, 0.25, 0.5, 1} per player, one row in four an outright
           draw.  Sums of the priors are exact and visited children get exactly equal q.
  onehot   all mass on one valid move (chosen by the hash), exact zeros on every other valid move.  Needs the leaf's valid
           moves.  Values as dyadic.
  spread   (1 + m / 2^23) * 2^-e with e uniform in [0, 137] (about exp(-U(0, 95))) on connect4 / brandubh rows and e in
           [0, 57] (about exp(-U(0, 40))) on 3-player rows: denormal priors, and exponent ranges on both sides of the 22
           binades that decide between the exact reduction tree and the serial sum in best_child.  24-bit uniform values.

The replay helpers below rebuild a fixture's roots and leaves: connect4, brandubh and the 3-player env on the C oracle's rules
(oracle_lib), othello and gobang -- which have no C oracle -- on the package's host envs (alphazero_general_amd/envs), which
test_othello_cpu.py / test_gobang_cpu.py pin to the reference's rule tables.
"""
import zlib

import numpy as np

FAMILIES = ('uniform', 'dyadic', 'onehot', 'spread')
_M64 = (1 << 64) - 1


def _mix(x):
    """splitmix64 finaliser over a uint64 array"""
    x = np.asarray(x, np.uint64)
    with np.errstate(over='ignore'):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def _hash(seed, stream, step, n, salt):
    base = (int(seed) * 0x100000001B3 ^ int(stream) * 0x9E3779B97F4A7C15 ^ int(step) * 0xC2B2AE3D27D4EB4F ^ int(salt) * 0x165667B19E3779F9) & _M64
    return _mix(_mix(np.uint64(base)) + np.arange(n, dtype=np.uint64))


def _dyadic_values(h, NV):
    v = np.array([0.0, 0.25, 0.5, 1.0], np.float32)[(h[:NV] & np.uint64(3)).astype(np.int64)]
    if int(h[NV] % np.uint64(4)) == 0:                       # an outright draw
        v[:] = 0.0
        v[NV - 1] = 1.0
    return v


def row(family, seed, stream, step, A, NV, valid=None):
    """(policy float32[A], value float32[NV]); `valid` (the leaf's valid-move mask) is needed by 'onehot' only"""
    h = _hash(seed, stream, step, A + NV + 1, FAMILIES.index(family) + 1)
    if family == 'uniform':
        p = np.ones(A, np.float32)
        v = np.zeros(NV, np.float32)
        v[NV - 1] = 1.0
    elif family == 'dyadic':
        p = np.ldexp(np.ones(A), -(h[:A] & np.uint64(7)).astype(np.int64)).astype(np.float32)
        v = _dyadic_values(h[A:], NV)
    elif family == 'onehot':
        p = np.zeros(A, np.float32)
        idx = np.flatnonzero(np.asarray(valid)) if valid is not None else np.zeros(0, np.int64)
        if len(idx):
            p[idx[int(h[0] % np.uint64(len(idx)))]] = 1.0
        v = _dyadic_values(h[A:], NV)
    elif family == 'spread':
        emax = 58 if NV == 4 else 138
        e = (h[:A] % np.uint64(emax)).astype(np.int64)
        m = ((h[:A] >> np.uint64(40)) & np.uint64((1 << 23) - 1)).astype(np.float64)
        with np.errstate(under='ignore'):
            p = np.ldexp(1.0 + m / float(1 << 23), -e).astype(np.float32)    # (float64 exact; one IEEE rounding to float32)
        v = ((h[A:A + NV] >> np.uint64(40)).astype(np.float64) / float(1 << 24)).astype(np.float32)
    else:
        raise ValueError(family)
    return p, v


def row_crc(p, v):
    return zlib.crc32(np.ascontiguousarray(v, np.float32).tobytes(), zlib.crc32(np.ascontiguousarray(p, np.float32).tobytes())) & 0xFFFFFFFF


def agent_row(seed, stream, step, A, NV):
    """the edge agent's evaluator: uniform priors, dyadic (draw-heavy) values"""
    p, _ = row('uniform', seed, stream, step, A, NV)
    _, v = row('dyadic', seed, stream, step, A, NV)
    return p, v


# ---- replay helpers (the oracle's rules, the host envs' for othello and gobang; used by the CPU and GPU replays of the edge fixtures) ----
CONFIGS = ['uniform_q', 'uniform_bonus', 'dyadic', 'dyadic_noise1', 'onehot', 'onehot_q', 'spread', 'spread_powf']
GAMES = {'c4': 0, 'br': 1, 'tm': 2, 'ot': 3, 'gb': 4, 'gbr': 4, 'tt': 5}
HOST_GAMES = (3, 4, 5)                                       # no C oracle: replayed on alphazero_general_amd.envs.{othello,gobang,tictactoe}


def game_sizes(gid):
    """(action size, value row length)"""
    if gid in HOST_GAMES:
        cls = host_game(gid)
        return cls.action_size(), cls.num_players() + 1
    import oracle_lib as ol
    gi = ol.game_info(gid)
    return gi.action_size, gi.num_players + 1


def host_game(gid):
    from alphazero_general_amd.envs import gobang, othello, tictactoe
    return {3: othello.Game, 4: gobang.Game, 5: tictactoe.Game}[gid]


def roots(d, gid):
    """the fixture's root positions: oracle games, or host env games for othello (64 cells) and gobang (the packed ABI layout)"""
    if gid in HOST_GAMES:
        from alphazero_general_amd import _abi
        cls = host_game(gid)
        unpack = (lambda c: _abi.gobang_unpack(c.tobytes())) if gid == 4 else (lambda c: c)
        return [cls.from_azg_state(unpack(d['cells'][r]), int(d['player'][r]), int(d['turns'][r])) for r in range(len(d['player']))]
    import oracle_lib as ol
    out = []
    for r in range(len(d['player'])):
        st = ol.State()
        for i, x in enumerate(d['cells'][r]):
            st.cells[i] = int(x)
        st.player, st.turns = int(d['player'][r]), int(d['turns'][r])
        st.aux[0] = int(d['aux0'][r])
        out.append(ol.OGame(gid, state=st))
    return out


def leaf_row(family, seed, root, r, s, path, A, NV):
    """the row the generator fed at (root r, simulation s): the leaf is the root played along the recorded path"""
    if family != 'onehot':                                   # (only 'onehot' looks at the leaf)
        return row(family, seed, r, s, A, NV)
    g = root.clone()
    play = g.play if hasattr(g, 'play') else g.play_action
    for a in path:
        play(int(a))
    term = np.asarray(g.win_state()).any()
    return row(family, seed, r, s, A, NV, None if term else np.asarray(g.valid_moves()))


def root_state(g):
    """a root of `roots` as DeviceEngine.set_states takes it (gobang: the 225 unpacked cells, engine.py packs them)"""
    if hasattr(g, 'to_azg_state'):
        return g.to_azg_state()
    return (g.cells(), g.player, g.turns, g.s.aux[0])


def pack_obs(obs, nbit=2):
    """gobang observations [n, 4, 15, 15] without loss in a fraction of the space: the first `nbit` planes hold 0 / 1 (kept as
    bits), every other plane is one constant (kept as that float32).  Checked here to decode to the same bytes."""
    obs = np.ascontiguousarray(obs, np.float32)
    n = len(obs)
    out = dict(agent_s_obs_bits=np.packbits(obs[:, :nbit].reshape(n, -1) != 0, axis=1),
               agent_s_obs_planes=np.ascontiguousarray(obs[:, nbit:, 0, 0]), agent_s_obs_shape=np.array(obs.shape, np.int32))
    assert unpack_obs(out).tobytes() == obs.tobytes()
    return out


def pack_pi(pi):
    """the agent's sample policies [n, A] (A < 256; a handful of non-zero entries per row) without loss: per row the count of
    non-zero entries, then their columns and values in row order.  Checked here to decode to the same bytes."""
    pi = np.ascontiguousarray(pi, np.float32)
    rows, cols = np.nonzero(pi)
    out = dict(agent_s_pi_nnz=np.bincount(rows, minlength=len(pi)).astype(np.uint8), agent_s_pi_col=cols.astype(np.uint8),
               agent_s_pi_val=pi[rows, cols], agent_s_pi_shape=np.array(pi.shape, np.int32))
    assert pi.shape[1] < 256 and unpack_pi(out).tobytes() == pi.tobytes()
    return out


def unpack_pi(d):
    """the agent's sample policies of a fixture: stored as they are, or as pack_pi wrote them"""
    if 'agent_s_pi' in d:
        return d['agent_s_pi']
    pi = np.zeros(tuple(int(x) for x in d['agent_s_pi_shape']), np.float32)
    pi[np.repeat(np.arange(len(pi)), d['agent_s_pi_nnz']), d['agent_s_pi_col']] = d['agent_s_pi_val']
    return pi


def stack_configs(d):
    """every `<config>_<key>` of a fixture dict stacked over the configs into one `cfgs_<key>` (paths padded with 255 to one
    length): gb_edge.npz has a few hundred small arrays otherwise, and a zip entry costs as much as many of them hold"""
    cfgs = [str(c) for c in d['configs']]
    pre = sorted(cfgs, key=len, reverse=True)
    out, per = {}, {}
    for k, v in d.items():
        c = next((c for c in pre if k.startswith(c + '_')), None)
        if c is None:
            out[k] = v
        else:
            per.setdefault(k[len(c) + 1:], {})[c] = np.asarray(v)
    for key, by in per.items():
        arrs = [by[c] for c in cfgs]
        if key == 'paths':
            L = max(a.shape[-1] for a in arrs)
            assert all(a.dtype == np.uint8 for a in arrs)
            arrs = [np.pad(a, ((0, 0), (0, 0), (0, L - a.shape[-1])), constant_values=255) for a in arrs]
        out['cfgs_' + key] = np.stack(arrs)
    return out


def unstack_configs(d):
    if not any(k.startswith('cfgs_') for k in d):
        return d
    out = {k: v for k, v in d.items() if not k.startswith('cfgs_')}
    for k, v in d.items():
        if k.startswith('cfgs_'):
            for i, c in enumerate(d['configs']):
                x = v[i]
                if k == 'cfgs_a' and x.dtype == np.uint8:   # (stored with 255 for "no child")
                    x = np.where(x == 255, -1, x.astype(np.int16)).astype(np.int16)
                out['%s_%s' % (c, k[5:])] = x
    return out


def load(golden_dir, name):
    """the arrays of fixture `name`, one `<config>_<key>` per config and key; 'gbr' is the group of random gobang roots that
    gb_edge.npz holds under `rnd_`"""
    import os
    if name == 'gbr':
        return unstack_configs({k[4:]: v for k, v in np.load(os.path.join(golden_dir, 'gb_edge.npz')).items() if k.startswith('rnd_')})
    d = dict(np.load(os.path.join(golden_dir, name + '_edge.npz')))
    return unstack_configs({k: v for k, v in d.items() if not k.startswith('rnd_')})


def unpack_obs(d):
    """the agent's sample observations of a fixture: stored as they are, or as pack_obs wrote them"""
    if 'agent_s_obs' in d:
        return d['agent_s_obs']
    n, C, H, W = [int(x) for x in d['agent_s_obs_shape']]
    nbit = C - d['agent_s_obs_planes'].shape[1]
    obs = np.empty((n, C, H, W), np.float32)
    obs[:, :nbit] = np.unpackbits(d['agent_s_obs_bits'], axis=1)[:, :nbit * H * W].reshape(n, nbit, H, W)
    obs[:, nbit:] = d['agent_s_obs_planes'][:, :, None, None]
    return obs


def probs_untrapped(counts, t):
    """MCTS.probs (:319-321) with numpy's underflow trap off: what the expression evaluates to where the reference's
    np.seterr(all='raise') turns an underflow into FloatingPointError"""
    c = np.asarray(counts, np.float32)
    with np.errstate(under='ignore', invalid='ignore'):
        p = (c / np.sum(c)) ** (1.0 / float(np.float32(t)))
        return p / np.sum(p)
