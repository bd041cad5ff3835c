"""RandomPlayer.play and NNPlayer.play (alphazero/GenericPlayers.py:47-52, :69-94) restated in numpy, with np.random.choice's own
arithmetic written out so that the one uniform it draws is an argument: what azg_game_choose is held to.

np.random.choice(A, p=p) (numpy's legacy RandomState): cdf = p.cumsum() in float64; cdf /= cdf[-1]; uniform = random_sample();
index = cdf.searchsorted(uniform, side='right').  It draws exactly one double, so RandomState(s).random_sample() is the u of
np.random.seed(s); np.random.choice(...)."""
import numpy as np

NEAR = 1e-6          # |cdf_j - u| below this: the draw sits next to a boundary that a 1-ulp difference of a float32 pow could move


def random_probs(valids):
    """RandomPlayer.play :49-50"""
    valids = np.asarray(valids)
    return valids / np.sum(valids)


def nn_probs(valids, policy, temp):
    """NNPlayer.play :72-80 (float32 policy; temp as the Python float the player holds)"""
    options = np.asarray(policy, np.float32) * np.asarray(valids)
    if temp == 0:
        bestA = np.argmax(options)
        probs = [0] * len(options)
        probs[bestA] = 1
    else:
        probs = [x ** (1. / temp) for x in options]
        probs /= np.sum(probs)
    return probs


def choice(p, u):
    """(index, cdf) of np.random.choice(len(p), p=p) when its random_sample() returns u"""
    cdf = np.asarray(p, np.float64).cumsum() if not isinstance(p, np.ndarray) else p.astype(np.float64).cumsum()
    cdf /= cdf[-1]
    return int(cdf.searchsorted(u, side='right')), cdf


def choose(valids, policy, temp, u):
    """(action, cdf): policy None -> RandomPlayer, else NNPlayer at temperature temp"""
    p = random_probs(valids) if policy is None else nn_probs(valids, policy, 1.0 if temp is None else temp)
    return choice(p, u)


def near_boundary(cdf, u, tol=NEAR):
    return bool((np.abs(np.asarray(cdf) - u) < tol).any())


# ---------------------------------------------------------------------------------------------------- the fixed inputs of the GPU test
# 256 positions per game from the reference-made rule tables (the 3-player env, which has no table: seeded host playouts), a policy row
# with exact zeros on some valid moves and one uniform per (position, setting), all from fixed seeds -- so that tests/test_choose_cpu.py
# can hold the inputs to the margin rule before a GPU sees them.  A setting is None (RandomPlayer) or one of TEMPS (NNPlayer).
import functools  # noqa: E402

TEMPS = (1.0, 0.5, 1 / 3, 0.25, 0.2, 0.0)
SETTINGS = (None,) + TEMPS
N_POS = 256
GAME_NAMES = ('connect4', 'brandubh', 'trimok', 'othello', 'gobang', 'tictactoe', 'hnefatafl')


def hnefatafl_ring():
    """an 11x11 board of this game's piece codes with 321 valid moves (the move list reaches its sixth chunk of 64): pieces of code 1 on
    every border cell but the corners, the king at (1, 0) -- every interior cell but the throne is reached from four sides, the king
    also steps onto the corner next to it"""
    c = np.zeros((11, 11), np.int8)
    c[5, 5] = 4
    for y, x in ((0, 0), (0, 10), (10, 0), (10, 10)):
        c[y, x] = 5
    for i in range(1, 10):
        c[0, i] = c[10, i] = c[i, 0] = c[i, 10] = 1
    c[1, 0] = 3
    return (c.reshape(-1), 1, 11, 0)


@functools.lru_cache(maxsize=None)
def inputs(gid):
    """dict(items: what DeviceGames.pack takes, valids uint8 [N_POS, A], policy float32 [N_POS, A], u float64 [len(SETTINGS), N_POS])"""
    import test_gpu_device_games as T
    rng = np.random.RandomState(100 + gid)
    items, valids = [], []
    if gid == T.TM:
        Game = T._envs()[gid]
        while len(items) < N_POS:
            g = Game()
            while not g.win_state().any() and len(items) < N_POS:
                items.append(g.clone()); valids.append(np.asarray(g.valid_moves(), np.uint8))
                g.play_action(int(rng.choice(np.flatnonzero(g.valid_moves()))))
    else:
        t = T._table(T.MAIN_TABLE[gid])
        order = list(rng.permutation(t['n']))
        if gid == T.HN:                                              # several chunks of the move list: > 64 and > 320 valid moves
            nv = t['raw']['nvalid']
            order = [int(np.flatnonzero(nv > 64)[0])] + order
            items.append(hnefatafl_ring()); valids.append(np.asarray(T._host(gid, items[0]).valid_moves(), np.uint8))
            assert valids[0].sum() > 320
        for i in order:
            if len(items) == N_POS:
                break
            v = np.asarray(T._host(gid, t['states'][i]).valid_moves(), np.uint8)
            if v.any():
                items.append(t['states'][i]); valids.append(v)
        if gid == T.HN:
            assert valids[1].sum() > 64
    valids = np.stack(valids)
    A = valids.shape[1]
    # (no entry so small that its fifth power underflows float32: the reference runs under np.seterr(all='raise'), MCTS.pyx:23)
    policy = (0.05 + 0.95 * rng.random_sample((N_POS, A)) ** 3).astype(np.float32)
    policy[rng.random_sample((N_POS, A)) < 0.2] = 0                  # exact zeros, on valid moves too
    for i in np.flatnonzero((policy * valids).sum(1) == 0):          # (a row the reference would divide by zero on is an edge case, not here)
        policy[i, np.flatnonzero(valids[i])[0]] = 0.5
    policy /= policy.sum(1, keepdims=True, dtype=np.float32)
    u = np.stack([np.random.RandomState(1000 + 10 * gid + si).random_sample(N_POS) for si in range(len(SETTINGS))])
    return dict(items=items, valids=valids, policy=policy, u=u)


@functools.lru_cache(maxsize=None)
def expected(gid):
    """(actions int64 [len(SETTINGS), N_POS], near bool [len(SETTINGS), N_POS]) of the helper on inputs(gid): computed once, shared"""
    d = inputs(gid)
    act = np.zeros((len(SETTINGS), N_POS), np.int64)
    near = np.zeros((len(SETTINGS), N_POS), bool)
    for si, temp in enumerate(SETTINGS):
        for i in range(N_POS):
            a, cdf = choose(d['valids'][i], None if temp is None else d['policy'][i], temp, d['u'][si, i])
            act[si, i], near[si, i] = a, near_boundary(cdf, d['u'][si, i])
    return act, near
