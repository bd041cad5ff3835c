"""compareToBaseline in native mode (coach.native_arena): the reference's RawMCTSPlayer -- compareToBaseline's default baselineTester,
Coach.py:70,575-584 -- is a raw seat (None) of the device arena, whose evaluation is RawMCTSPlayer.process's constants
(GenericPlayers.py:198-200); every other non-model player still falls through to the reference's Arena.  The parts that need the reference
checkout skip where it is absent, like test_iteration_cpu.py."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from test_iteration_cpu import REF  # noqa: E402  (the reference checkout the build container has)


# ------------------------------------------------------------------------------------------------ stand-ins: the routing of play_games
def _routing(monkeypatch, players, *, batched=True, game=None, raw_seats=True):
    """NativeArena over a stand-in reference Arena: what play_games did -- ('device', seats) or ('reference',)"""
    from alphazero_general_amd import coach as AC
    from alphazero_general_amd import iteration as I
    from alphazero_general_amd.envs.connect4 import Game
    seen = []

    class RefArena:
        def __init__(self, players, game_cls, use_batched_mcts=True, args=None):
            self.players, self.game_cls, self.use_batched_mcts, self.args = players, game_cls, use_batched_mcts, args
            self.stop_event = types.SimpleNamespace(is_set=lambda: False)

        def play_games(self, num, verbose=False, shuffle_players=True):
            seen.append(('reference',))
            return [0] * len(self.players), 0, [0.0] * len(self.players)

    def lead(op, g, nnets, args, **kw):
        seen.append(('device', op, ['net' if n is not None else None for n in nnets], kw.get('num_games')))
        return dict(wins=[1] * len(nnets), draws=0, winrates=[0.5] * len(nnets), games=len(nnets))

    monkeypatch.setattr(I, 'lead', lead)
    monkeypatch.setattr(AC._NetCache, 'get', lambda self, n: n)
    A = AC.native_arena(RefArena, raw_seats=raw_seats)
    A(players, game or Game, use_batched_mcts=batched).play_games(8)
    return seen


def _raw_class(module='alphazero.GenericPlayers', name='RawMCTSPlayer'):
    def process(self, batch):
        raise AssertionError('a raw seat is never asked to evaluate')
    return type(name, (), {'__module__': module, 'nn': None, 'process': process})


def test_raw_player_is_a_raw_seat(monkeypatch):
    net = types.SimpleNamespace(nn=object())
    assert _routing(monkeypatch, [net, _raw_class()()]) == [('device', 'arena', ['net', None], 8)]


def test_other_players_fall_through(monkeypatch):
    net = types.SimpleNamespace(nn=object())
    Raw = _raw_class()
    random_player = _raw_class(name='RandomPlayer')()
    assert _routing(monkeypatch, [net, random_player]) == [('reference',)]                      # RandomPlayer
    assert _routing(monkeypatch, [net, Raw()], batched=False) == [('reference',)]               # unbatched arena
    assert _routing(monkeypatch, [net, Raw()], game=type('NoRules', (), {})) == [('reference',)]    # a game without device rules
    assert _routing(monkeypatch, [net, Raw()], raw_seats=False) == [('reference',)]             # the opt-out keyword
    assert _routing(monkeypatch, [Raw(), Raw()]) == [('reference',)]                            # no network at all
    sub = type('MyRaw', (Raw,), {})()                                                          # a subclass, an own process
    assert _routing(monkeypatch, [net, sub]) == [('reference',)]
    own = Raw()
    own.process = lambda batch: None
    assert _routing(monkeypatch, [net, own]) == [('reference',)]
    assert _routing(monkeypatch, [net, _raw_class(module='mine.players')()]) == [('reference',)]


def test_native_coach_passes_the_opt_out_on():
    from alphazero_general_amd.coach import native_arena, native_coach
    mod = types.ModuleType('azg_stand_in_coach')

    class Arena:
        pass

    class Coach:
        pass
    Coach.__module__ = mod.__name__
    mod.Arena, mod.Coach = Arena, Coach
    sys.modules[mod.__name__] = mod
    try:
        native_coach(Coach, raw_seats=False)
        assert mod.Arena._azg_native and mod.Arena._azg_raw_seats is False and mod.Arena._azg_base is Arena
        again = native_arena(mod.Arena)                              # the other choice wraps the reference's class afresh
        assert again._azg_raw_seats is True and again._azg_base is Arena and native_arena(again) is again
    finally:
        del sys.modules[mod.__name__]


# ------------------------------------------------------------------------------------------------ against the real reference
_PROBE = r'''
import json, os, sys, threading, types
sys.dont_write_bytecode = True
sys.path.insert(0, %(root)r); sys.path.insert(1, %(ref)r)
import numpy as np, torch
tbx = types.ModuleType('tensorboardX')
class _W:
    def __init__(self, *a, **k): self.scalars = []
    def add_scalar(self, *a, **k): self.scalars.append(a)
    def __getattr__(self, n): return lambda *a, **k: None
tbx.SummaryWriter = _W
sys.modules.setdefault('tensorboardX', tbx)
import pyximport
os.makedirs('/tmp/pyxbld', exist_ok=True)
pyximport.install(setup_args={'include_dirs': np.get_include()}, build_dir='/tmp/pyxbld', language_level=3)
import alphazero_general_amd as azg
azg.install()
import alphazero.Coach as CM
from alphazero.GenericPlayers import RawMCTSPlayer
from alphazero.utils import dotdict
from alphazero_general_amd import coach as AC, iteration as I
from alphazero_general_amd.envs.connect4 import Game
out = {}
calls = []
def lead(op, g, nnets, args, **kw):
    calls.append([op, g.__name__, [None if n is None else 'net' for n in nnets], kw.get('num_games')])
    return dict(wins=[3, 1], draws=0, winrates=[0.75, 0.25], games=4)
I.lead = lead
AC._NetCache.get = lambda self, n: n
Native = AC.native_coach(CM.Coach)
coach = object.__new__(Native)
coach.args = dotdict(CM.DEFAULT_ARGS)
coach.game_cls, coach.train_net, coach.writer, coach.stop_train = Game, object(), _W(), threading.Event()
out['defaults'] = [coach.args.compareWithBaseline, coach.args.baselineCompareFreq, coach.args.baselineTester.__name__, coach.args.arenaBatched]
coach.compareToBaseline(1)
out['calls'] = calls
out['scalar'] = [list(a[:2]) for a in coach.writer.scalars]
# RawMCTSPlayer.process against the engine's constants: float32(1 / A) (C++ (float)(1.0 / A)), zeros
raw = RawMCTSPlayer(Game, coach.args)
p, v = raw.process(torch.zeros((5,) + tuple(Game.observation_size())))
A = Game.action_size()
out['raw'] = dict(p_dtype=str(p.dtype), v_dtype=str(v.dtype), p_shape=list(p.shape), v_shape=list(v.shape),
                  p_bits=(p.numpy().view(np.uint32) == np.full((5, A), np.float32(1.0 / A)).view(np.uint32)).all().item(),
                  host_split_bits=(p.numpy().view(np.uint32) == torch.zeros((5, A)).fill_(1 / A).numpy().view(np.uint32)).all().item(),
                  v_zero=(v.numpy().view(np.uint32) == 0).all().item())
print(json.dumps(out))
'''


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, 'alphazero')), reason='needs the reference checkout (build container only)')
def test_compare_to_baseline_reaches_the_device_arena_with_a_raw_seat(tmp_path):
    """the real Coach.compareToBaseline with its default args plays [train net, None] through iteration.lead('arena', ...), and
    RawMCTSPlayer.process returns, bit for bit, the rows the engine's raw seat uses (kernel constant and host-split fill)"""
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
    r = subprocess.run([sys.executable, '-c', _PROBE % dict(root=ROOT, ref=REF)], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d['defaults'] == [True, 1, 'RawMCTSPlayer', True], d
    assert d['calls'] == [['arena', 'Game', ['net', None], 128]], d
    assert d['scalar'] == [['win_rate/baseline', 0.75]], d
    raw = d['raw']
    assert raw['p_dtype'] == raw['v_dtype'] == 'torch.float32' and raw['p_shape'] == [5, 7] and raw['v_shape'] == [5, 3], raw
    assert raw['p_bits'] and raw['host_split_bits'] and raw['v_zero'], raw
