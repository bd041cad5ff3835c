"""Rules without a tree on one GPU: positions/s of DeviceGames.step (a move played, then every output: the position, the valid mask, the
win state, the float32 observation) and of DeviceGames.symmetries (states, observations, policies of all NSYM entries), per game, at
1 k and 64 k positions -- next to the host env classes doing the same work position by position.

The positions are mid-game: `--plies` random legal plies from the opening, played on the device (the finished ones stay in: the kernels
treat them like any other).  A timed window is about `--window` seconds of launches between two device synchronises (their number
comes from a short pilot window, which also warms), every buffer allocated before it (out=); `--reps` windows, median with min / max.  The host figure is the same calls on `--host` positions taken
from the same set: clone + play_action + valid_moves + win_state + observation, and symmetries(pi) + observation() of each entry.

No number here is a pass bar.  The result goes to `--out` (default profiles/device_games_throughput.json) with the device named."""
import argparse
import importlib
import json
import os
import platform
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from alphazero_general_amd.games import DeviceGames  # noqa: E402

GAMES = ('connect4', 'brandubh', 'trimok', 'othello', 'gobang', 'tictactoe', 'hnefatafl')
PLIES = dict(connect4=12, brandubh=20, trimok=6, othello=20, gobang=40, tictactoe=3, hnefatafl=20)


def med(xs):
    xs = sorted(xs)
    return dict(median=int(statistics.median(xs)), min=int(xs[0]), max=int(xs[-1]))


def midgame(dg, n, plies, seed):
    gen = torch.Generator(device=dg.device)
    gen.manual_seed(seed)
    r = dg.step(dg.initial(n), next=True, win=True)
    for _ in range(plies):
        done = (r.win != 0).any(1) | ~(r.valid != 0).any(1)
        w = r.valid.float()
        w[done] = 1.0
        acts = torch.multinomial(w, 1, generator=gen).flatten().to(torch.int32)
        acts[done] = -1
        r = dg.step(r.next, acts)
    first = torch.where((r.valid != 0).any(1), r.valid.argmax(1).to(torch.int32), torch.full((n,), -1, dtype=torch.int32, device=dg.device))
    return r.next.contiguous(), first


def windows(fn, n, seconds, reps):
    """positions/s over `reps` windows of about `seconds` each; the launches of a window are counted from a short pilot window, which
    also warms (code objects, caches)"""
    def window(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    window(20)
    iters = max(20, int(seconds / (window(20) / 20)))
    return dict(med([n * iters / window(iters) for _ in range(reps)]), launches_per_window=iters)


def host_rates(dg, states, acts, pi, reps):
    games = dg.to_games(states)
    acts = acts.cpu().tolist()
    step, sym = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        for g, a in zip(games, acts):
            h = g.clone()
            if a >= 0:
                h.play_action(int(a))
            h.valid_moves(); h.win_state(); h.observation()
        step.append(len(games) / (time.perf_counter() - t0))
        t0 = time.perf_counter()
        for g, p in zip(games, pi):
            for gs, _ in g.symmetries(p):
                gs.observation()
        sym.append(len(games) / (time.perf_counter() - t0))
    return med(step), med(sym)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--games', nargs='*', default=list(GAMES))
    ap.add_argument('--sizes', nargs='*', type=int, default=[1024, 65536])
    ap.add_argument('--window', type=float, default=0.25, help='seconds of launches per timed window')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host', type=int, default=64)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'device_games_throughput.json'))
    a = ap.parse_args()
    rows = []
    for name in a.games:
        dg = DeviceGames(importlib.import_module('alphazero_general_amd.envs.' + name).Game)
        for n in a.sizes:
            states, acts = midgame(dg, n, PLIES[name], seed=n + len(name))
            pi = torch.rand((n, dg.A), device=dg.device)
            out = dg.step(states, acts, obs=torch.float32)
            step = windows(lambda: dg.step(states, acts, obs=torch.float32, out=out), n, a.window, a.reps)
            del out
            sout = dg.symmetries(states, pi)
            sym = windows(lambda: dg.symmetries(states, pi, out=sout), n, a.window, a.reps)
            del sout
            row = dict(game=name, positions=n, window_s=a.window, reps=a.reps, finished=int((dg.step(states, next=False, valid=False).win != 0).any(1).sum()),
                       step_positions_per_s=step, symmetries_positions_per_s=sym)
            if n == a.sizes[0]:
                hs, hy = host_rates(dg, states[:a.host].contiguous(), acts[:a.host], pi[:a.host].cpu().numpy(), 3)
                row.update(host_positions=a.host, host_step_positions_per_s=hs, host_symmetries_positions_per_s=hy)
            rows.append(row)
            print(json.dumps(row), flush=True)
            torch.cuda.empty_cache()
    res = dict(device=torch.cuda.get_device_name(), arch=getattr(torch.cuda.get_device_properties(0), 'gcnArchName', ''), torch=torch.__version__,
               hip=torch.version.hip, host_cpu=platform.processor() or platform.machine(), unit='positions per second; median, min, max over the windows',
               rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
