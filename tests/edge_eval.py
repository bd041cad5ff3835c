"""Synthetic evaluators for the tree edge goldens (tests/golden/{c4,br,tm}_edge.npz, made by make_goldens.py `edge`).

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


# ---- replay helpers (the oracle's rules; used by the CPU and GPU replays of the edge fixtures) ----
CONFIGS = ['uniform_q', 'uniform_bonus', 'dyadic', 'dyadic_noise1', 'onehot', 'onehot_q', 'spread', 'spread_powf']
GAMES = {'c4': 0, 'br': 1, 'tm': 2}


def roots(d, gid):
    """the fixture's root positions as oracle games"""
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
    g = root.clone()
    for a in path:
        g.play(int(a))
    term = g.win_state().any()
    return row(family, seed, r, s, A, NV, None if term else g.valid_moves())


def probs_untrapped(counts, t):
    """MCTS.probs (:319-321) with numpy's underflow trap off: what the expression evaluates to where the reference's
    np.seterr(all='raise') turns an underflow into FloatingPointError"""
    c = np.asarray(counts, np.float32)
    with np.errstate(under='ignore', invalid='ignore'):
        p = (c / np.sum(c)) ** (1.0 / float(np.float32(t)))
        return p / np.sum(p)
