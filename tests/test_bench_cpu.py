"""bench.py's host side without a GPU: --dump-outputs (what the timed path returned, within the size budget, a seeded subset above
it) and the argument checks that run before any device is touched."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


class _Engine:
    def __init__(self, actions):
        self.actions = torch.tensor(actions, dtype=torch.int32)

    def last_actions(self):
        return self.actions


def _selfplay(n):
    g = torch.Generator().manual_seed(5)
    obs, pi, z = torch.rand((n, 4, 6, 7), generator=g), torch.rand((n, 7), generator=g), torch.rand((n, 3), generator=g)
    c = SimpleNamespace(arena=False, engines=[_Engine([1, 2, 3]), _Engine([4, 5])])
    t = {'exchange': dict(samples=(obs, pi, z), wins=[3, 2], draws=1, num_results=6, games=6, expansions=100, sims=120, num_samples=n)}
    return c, t


def test_dump_outputs_writes_what_the_exchange_returned(tmp_path):
    c, t = _selfplay(50)
    shapes = bench.dump_outputs(c, t, str(tmp_path))
    assert sorted(shapes) == ['last_actions', 'samples_obs', 'samples_pi', 'samples_z', 'tallies']
    tal = np.load(tmp_path / 'tallies.npy')
    assert tal.dtype == np.float64 and tal.tolist() == [3, 2, 1, 6, 6, 100, 120, 50]
    la = np.load(tmp_path / 'last_actions.npy')
    assert la.dtype == np.float64 and la.tolist() == [1, 2, 3, 4, 5]
    for name, ref in zip(('obs', 'pi', 'z'), t['exchange']['samples']):
        a = np.load(tmp_path / ('samples_%s.npy' % name))
        assert a.dtype == np.float32 and np.array_equal(a, ref.numpy())


def test_dump_outputs_keeps_to_the_budget_with_a_fixed_subset(tmp_path):
    budget = 3 << 20
    c, t = _selfplay(10000)                                           # 7.1 MB of samples
    bench.dump_outputs(c, t, str(tmp_path / 'a'), budget=budget)
    bench.dump_outputs(c, t, str(tmp_path / 'b'), budget=budget)
    total = sum(os.path.getsize(tmp_path / 'a' / f) for f in os.listdir(tmp_path / 'a'))
    assert total <= budget
    rows = np.load(tmp_path / 'a' / 'samples_rows.npy').astype(np.int64)
    assert len(rows) > 1000 and (np.diff(rows) > 0).all()
    assert np.array_equal(np.load(tmp_path / 'a' / 'samples_obs.npy'), t['exchange']['samples'][0].numpy()[rows])
    for f in os.listdir(tmp_path / 'a'):
        assert np.array_equal(np.load(tmp_path / 'a' / f), np.load(tmp_path / 'b' / f)), f


def test_dump_outputs_arena_has_tallies_and_moves_only(tmp_path):
    c = SimpleNamespace(arena=True, engines=[_Engine([0, 6])])
    t = {'exchange': dict(wins=[4, 1], draws=0, winrates=[0.8, 0.2], num_results=5, games=5, expansions=70, sims=80)}
    assert sorted(bench.dump_outputs(c, t, str(tmp_path))) == ['last_actions', 'tallies']
    assert np.load(tmp_path / 'tallies.npy').tolist() == [4, 1, 0, 5, 5, 70, 80]


def test_steps_below_one_is_refused_before_the_device_is_touched():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '0'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and '--steps must be >= 1' in r.stderr, r.stderr[-2000:]
