"""The host replay of sample emission (tests/sample_replay.py) against the reference's own output.

Every config of the agent fixtures -- written by the reference's SelfPlayAgent (tests/golden/make_goldens.py gen_agent and
gen_c4_mt19937_agent) -- is replayed from its recorded fast flags, root counts and actions, and the replay must give the
fixture's samples and results bit for bit.  That pins the replay to the reference without a GPU, so the GPU tests can hold
the device to it at sizes no fixture reaches.  A second group checks the host envs' symmetries at positions after the
first move, where a symmetric start position cannot hide a wrong identity entry."""
import os
import zlib

import numpy as np
import pytest

import sample_replay as sr

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
C4, BR, TM, OT, GB = 0, 1, 2, 3, 4

# (fixture, game, config, symmetricSamples): every config of the lock-step agent fixtures
AGENT_FIXTURES = (
    [('c4_agent', C4, c, c != 'fastmix') for c in ('plain', 'noisy', 'fastmix', 'reset', 'warmup', 'config1')]
    + [('br_agent', BR, c, c != 'raw') for c in ('plain', 'noisy', 'wide', 'raw')]
    + [('tm_agent', TM, c, True) for c in ('plain', 'noisy', 'wide')]
    + [('ot_agent', OT, c, c != 'fastmix') for c in ('plain', 'noisy', 'fastmix')]
    + [('gb_agent', GB, c, c != 'fastmix') for c in ('plain', 'temp', 'fastmix')])
MT_FIXTURES = [('c4_mt19937_agent', C4), ('br_mt19937_agent', BR), ('ot_mt19937_agent', OT)]

_cache = {}


def load(name):
    if name not in _cache:
        _cache[name] = dict(np.load(os.path.join(G, name + '.npz')))   # (NpzFile decompresses an array on EVERY d[key])
    return _cache[name]


def check_replay(out, d, p):
    for k in ('s_obs', 's_pi', 's_z', 'r_ws', 'r_turns', 'games_played'):
        want = d[p + k]
        assert out[k].shape == want.shape, (k, out[k].shape, want.shape)
        assert out[k].dtype == want.dtype, (k, out[k].dtype, want.dtype)
        assert out[k].tobytes() == want.tobytes(), k


@pytest.mark.parametrize('fixture,game,cname,symmetric', AGENT_FIXTURES)
def test_replay_reproduces_agent_fixture(fixture, game, cname, symmetric):
    d = load(fixture)
    p = cname + '_'
    out = sr.replay(sr.GAMES[game], int(d[p + 'B']), int(d[p + 'games']), symmetric, d[p + 'counts'], d[p + 'actions'],
                    fast=d[p + 'fast'])
    check_replay(out, d, p)
    assert len(out['s_pi']) > 0


@pytest.mark.parametrize('fixture,game', MT_FIXTURES)
def test_replay_reproduces_mt19937_agent_fixture(fixture, game):
    """every round of these fixtures is a full search (no fast flag); symmetricSamples is on"""
    d = load(fixture)
    out = sr.replay(sr.GAMES[game], int(d['B']), int(d['games']), True, d['counts'], d['actions'])
    check_replay(out, d, '')


def test_raw_fixture_samples_positions_after_the_first_move():
    """the brandubh raw config is what exposes a wrong identity entry: it must hold samples of asymmetric positions"""
    d = load('br_agent')
    assert len(d['raw_r_turns']) == int(d['raw_games']) and (d['raw_r_turns'] > 1).all()
    obs = d['raw_s_obs']
    assert len(obs) > 4 * int(d['raw_games'])
    rot = np.rot90(obs[:, :3], 1, axes=(2, 3))                       # piece planes of a quarter turn
    assert (rot != obs[:, :3]).any(axis=(1, 2, 3)).sum() > len(obs) // 2


# ------------------------------------------------------------------------------------------------ the transforms themselves
IDENTITY = {C4: 0, BR: 6, OT: 7, GB: 7}          # the entry of symmetries() that is (state, pi) itself


def positions(game, n, seed):
    """n positions reached by 1 .. 20 random moves from the start"""
    cls = sr.GAMES[game]
    rng = np.random.RandomState(seed)
    out = []
    while len(out) < n:
        g = cls()
        for _ in range(rng.randint(1, 21)):
            v = np.flatnonzero(np.asarray(g.valid_moves()))
            if len(v) == 0 or np.asarray(g.win_state()).any():
                break
            g.play_action(int(rng.choice(v)))
        if g.turns > 0 and not np.asarray(g.win_state()).any():
            out.append(g)
    return out


def test_identity_entries_are_what_the_reference_fixtures_imply():
    # othello: the reference's own table (make_othello_goldens ot_rules), symmetries(arange(64)) per recorded position
    d = load('ot_rules')
    assert (d['sym_pi'][:, IDENTITY[OT]] == np.arange(64)).all()
    assert all((d['sym_pi'][:, k] != np.arange(64)).any(axis=1).all() for k in range(8) if k != IDENTITY[OT])
    d = load('gb_rules')                                   # gobang: the same table (make_gobang_goldens gb_rules), 225 actions
    assert (d['sym_pi'][:, IDENTITY[GB]] == np.arange(225)).all()
    assert all((d['sym_pi'][:, k] != np.arange(225)).any(axis=1).all() for k in range(8) if k != IDENTITY[GB])
    # brandubh: br_rules.sym_crc row = [position, crc(cells_k) ^ crc(pi_k) for the reference's 8 entries, crc(pi)]
    d = load('br_rules')
    crc = lambda a: zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF  # noqa: E731
    n_after = 0
    for row in d['sym_crc']:
        pos, ent, pi_crc = int(row[0]), row[1:9], int(row[9])
        ident = crc(d['cells'][pos].astype(np.int8)) ^ pi_crc
        hits = np.flatnonzero(ent == ident)
        assert list(hits) == [IDENTITY[BR]], (pos, hits)
        n_after += int(d['lens'][pos] > 0)
    assert n_after > 100
    # connect4: the reference lists (self, pi) first (connect4.pyx symmetries)
    g = positions(C4, 1, 5)[0]
    pi = np.arange(7, dtype=np.float32)
    s0, p0 = g.symmetries(pi)[0]
    assert (s0.observation() == g.observation()).all() and (p0 == pi).all()


@pytest.mark.parametrize('game,n', [(C4, 60), (BR, 12), (OT, 60), (GB, 60)])
def test_replay_symmetries_identity_once_and_only_once(game, n):
    """on positions after the first move, the replay's symmetric block holds (state, pi) at IDENTITY[game] and every other
    entry differs from it in observation or pi; with symmetricSamples off the replay writes exactly (state, pi)"""
    cls = sr.GAMES[game]
    rng = np.random.RandomState(100 + game)
    nsym = 0
    for g in positions(game, n, 200 + game):
        pi = (rng.rand(cls.action_size()) * np.asarray(g.valid_moves())).astype(np.float32)
        pi /= pi.sum()
        o = g.observation()
        block = sr.samples_of(g, pi, True)
        nsym = len(block)
        for k, (s2, p2) in enumerate(block):
            same = (np.asarray(s2.observation()) == o).all() and (np.asarray(p2) == pi).all()
            assert same == (k == IDENTITY[game]), k
        (s2, p2), = sr.samples_of(g, pi, False)
        assert (np.asarray(s2.observation()) == o).all() and (np.asarray(p2) == pi).all()
    assert nsym == {C4: 2, BR: 8, OT: 8, GB: 8}[game]
