"""Self-play samples at scale (pytest -m gpu): the device's examples() and results() against the host replay of the reference's
playMoves (tests/sample_replay.py, pinned to the reference's own fixtures by test_sample_replay_cpu.py).

Per game, thousands of history positions: a cheap deterministic evaluator (seeded tensors generated on the device), a few
simulations per move, a quarter of the rounds fast (no history entry), and enough rounds that at least 2B games finish.  Three
runs of the same search:
  commit  advance_begin + advance_commit, symmetricSamples off; every finished game is counted until 2B games have finished,
          then, in a round where two or more finish, the ones at even positions in slot order are skipped -- a mask the
          games_per_iteration cap cannot express -- and the run ends;
  on/off  eng.advance with symmetricSamples on and off, under a games_per_iteration cap that counts half of that last round's
          finished games.
All three must play the same counts and actions (symmetricSamples does not touch the search), and each run's samples and
results must be bit-identical to the replay of what it played."""
import time

import numpy as np
import pytest

import sample_replay as sr

pytestmark = pytest.mark.gpu

SIMS, FAST_SIMS, PROB_FAST = 4, 2, 0.25
SLOTS = {0: 64, 1: 32, 2: 96, 3: 32, 4: 16}              # connect4, brandubh, the 3-player env, othello, gobang
ROUNDS = {4: 340}                                        # gobang: this seeded run ends after 308 rounds; 3 * max_turns + 20 = 695 would size
                                                         # example_capacity (rounds x slots x 8 symmetries, 4.5 KB a sample) at twice the need


@pytest.fixture(scope='module')
def torch_mod():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return torch


class Evaluator:
    """a pool of seeded policy / value rows generated on the device; simulation `step` uses pool entry step % n"""

    def __init__(self, torch, eng, seed, n=8):
        g = torch.Generator(device=eng.device)
        g.manual_seed(seed)
        self.pol, self.val = [], []
        for _ in range(n):
            p = torch.rand((eng.B, eng.A), generator=g, device=eng.device) + 0.05
            v = torch.rand((eng.B, eng.NV), generator=g, device=eng.device) + 0.05
            self.pol.append((p / p.sum(1, keepdim=True)).contiguous())
            self.val.append((v / v.sum(1, keepdim=True)).contiguous())

    def __call__(self, step):
        return self.pol[step % len(self.pol)], self.val[step % len(self.val)]


def play(eng, ev, fast, cap=None, target=None):
    """SelfPlayAgent rounds (SelfPlayAgent.pyx:79-101) on the engine, in the phase form of fixture_checks.run_agent.
    cap: eng.advance until the engine's games_per_iteration cap is met.  target: advance_begin + advance_commit, every finished
    game counted until `target` games have finished; then the first round with two or more finished games skips the ones at
    even positions in slot order, and the run ends there."""
    rec = dict(counts=[], actions=[], fast=[], counted=[])
    nres, step = 0, 0
    for r in range(len(fast)):
        for _ in range(FAST_SIMS if fast[r] else SIMS):
            eng.select(None)
            eng.backup(*ev(step))
            step += 1
        rec['counts'].append(eng.root_counts().cpu().numpy())
        rec['fast'].append(bool(fast[r]))
        if cap is not None:
            eng.advance(record_history=not fast[r])
            rec['actions'].append(eng.last_actions().cpu().numpy())
            if eng.counters()['games_played'] >= cap:
                return rec
        else:
            fin = eng.advance_begin(record_history=not fast[r]) != 0
            idx = np.flatnonzero(fin)
            last = nres >= target and len(idx) >= 2
            counted = fin.copy()
            if last:
                counted[idx[0::2]] = False
            eng.advance_commit(counted)
            rec['actions'].append(eng.last_actions().cpu().numpy())
            rec['counted'].append(counted)
            nres += len(idx)
            if last:
                return rec
    raise AssertionError('the run did not end within %d rounds' % len(fast))


def rows_differing(a, b):
    return np.flatnonzero((a.reshape(len(a), -1) != b.reshape(len(b), -1)).any(1))[:8]


def check(eng, rec, game, symmetric, cap=1 << 30, counted=None):
    want = sr.replay(sr.GAMES[game], eng.B, cap, symmetric, rec['counts'], rec['actions'], fast=rec['fast'], counted=counted)
    c = eng.counters()
    obs, pi, z = [t.cpu().numpy() for t in eng.examples()]
    ws, turns, slot = eng.results()
    assert c['games_played'] == want['games_played'][-1] and c['num_results'] == len(want['r_turns'])
    assert obs.shape == want['s_obs'].shape, (obs.shape, want['s_obs'].shape)
    assert obs.tobytes() == want['s_obs'].tobytes(), ('observations differ', rows_differing(obs, want['s_obs']))
    assert pi.tobytes() == want['s_pi'].tobytes(), ('policies differ', rows_differing(pi, want['s_pi']))
    assert z.tobytes() == want['s_z'].tobytes(), ('winstates differ', rows_differing(z, want['s_z']))
    assert (ws == want['r_ws']).all() and (turns == want['r_turns']).all() and (slot == want['r_slot']).all(), 'results differ'
    return want


@pytest.mark.parametrize('game', [0, 1, 2, 3, 4])
def test_samples_vs_host_replay(torch_mod, game):
    torch = torch_mod
    from alphazero_general_amd import _abi
    from alphazero_general_amd.engine import DeviceEngine
    t0 = time.time()
    gi = _abi.game_info(game)
    B, nsym = SLOTS[game], gi.num_symmetries
    fast = np.random.RandomState(70 + game).random_sample(ROUNDS.get(game, 3 * gi.max_turns + 20)) < PROB_FAST
    ex_cap = int((~fast).sum()) * B * nsym                   # every round adds at most B history entries

    def run(symmetric, cap=None, target=None):
        eng = DeviceEngine(game, B, seed=500 + game, symmetric_samples=symmetric, games_per_iteration=cap or 1 << 30,
                           example_capacity=ex_cap, sims_hint=SIMS)
        rec = play(eng, Evaluator(torch, eng, 900 + game), fast, cap=cap, target=target)
        return eng, rec

    # advance_begin + advance_commit with a counted mask, symmetricSamples off
    eng, rc = run(False, target=2 * B)
    cm = np.array(rc['counted'])
    want = check(eng, rc, game, False, counted=cm)
    eng.close()
    before = int(want['games_played'][-2])                   # every game that finished before the last round was counted
    nfin_last = len(want['r_turns']) - before
    assert 1 <= int(cm[-1].sum()) < nfin_last, 'the last round must count some finished games and skip some'
    positions = len(want['s_pi'])                            # symmetricSamples off: one sample per history position
    assert len(want['r_turns']) >= 2 * B and positions >= 1000
    # eng.advance under a cap that cuts inside the same round, symmetricSamples on and off: the same search, the same cut
    cap = before + nfin_last // 2
    for symmetric in (True, False):
        eng, ra = run(symmetric, cap=cap)
        assert len(ra['actions']) == len(rc['actions'])
        assert (np.array(ra['counts']) == np.array(rc['counts'])).all(), 'symmetricSamples changed the search'
        assert (np.array(ra['actions']) == np.array(rc['actions'])).all(), 'symmetricSamples changed the moves'
        w = check(eng, ra, game, symmetric, cap=cap)
        assert int(w['games_played'][-1]) == cap < len(w['r_turns'])
        eng.close()
    print('\n  game %d: %d slots, %d rounds, %d results, %d history positions, %.1f s'
          % (game, B, len(rc['actions']), len(want['r_turns']), positions, time.time() - t0))
