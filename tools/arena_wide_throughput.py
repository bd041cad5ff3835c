"""Arena throughput on one GPU for the factorised-head networks: the persistent wide arena launch (azg_search_arena_wide_exact_f16, one
graph-captured launch per move) against the host-split form (ArenaRunner.step: per simulation one select, one evaluation per model's
slice after a host read of the split, one backup), for every (game, tower width) the launch has, at 128 / 256 / 512 games with the env's
usual numMCTSSims; two networks, and one network against a raw seat ([net, None]: RawMCTSPlayer's constants).  The two forms alternate
in one process, `--reps` times each; the row reports the median and the spread (min / max) of the moves per second.  Prints one JSON line
per case and writes them all to profiles/arena_wide_throughput.json.  Kernel averages: run it under the profiler on its own, e.g.

    rocprofv3 --kernel-trace --stats --output-format csv -d profiles/arena_wide_rocprof -o arena -- python tools/arena_wide_throughput.py --quick
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from alphazero_general_amd import nnet as N  # noqa: E402
from alphazero_general_amd.selfplay import ArenaRunner  # noqa: E402
from alphazero_general_amd.utils import dotdict, default_temp_scaling  # noqa: E402

# (game, width, numMCTSSims of the env's training script)
PAIRS = [('connect4', 32, 100), ('connect4', 64, 100), ('brandubh', 64, 100), ('trimok', 32, 50), ('othello', 32, 100), ('othello', 64, 100)]


def nets(name, width, n):
    Game = importlib.import_module('alphazero_general_amd.envs.' + name).Game
    na = dotdict(dict(N.BRANDUBH_NET_ARGS if name == 'brandubh' else N.DEFAULT_NET_ARGS))
    na['num_channels'] = width
    out = []
    for m in range(n):
        torch.manual_seed(m)
        out.append(N.NNetWrapper(Game, na, device='cuda:0').refresh())
    return Game, out


def rate(r, moves):
    r.play_round()                                                   # (warm)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(moves):
        r.play_round()
    torch.cuda.synchronize()
    return moves / (time.perf_counter() - t)


def case(name, width, sims, B, raw, moves, reps):
    Game, ns = nets(name, width, 1 if raw else _players(name))
    seats = ns + [None] * (Game.num_players() - 1) if raw else ns
    args = dotdict(numMCTSSims=sims, gamesPerIteration=1 << 30, cpuct=4.0, fpu_reduction=0.4, arenaTemp=0.25, startTemp=1.0,
                   temp_scaling_fn=default_temp_scaling)
    runners = {f: ArenaRunner(Game, seats, args, num_slots=B, seed=1, fused_search=f == 'persistent') for f in ('persistent', 'host_split')}
    got = {f: [] for f in runners}
    for _ in range(reps):                                            # (alternating: drift of clocks / temperature hits both forms)
        for f, r in runners.items():
            got[f].append(rate(r, moves))
    for r in runners.values():
        r.engine.close()
    row = dict(game=name, channels=width, games=B, sims=sims, seats='net+raw' if raw else 'nets', moves_per_rep=moves, reps=reps)
    for f, v in got.items():
        row[f] = dict(moves_per_s_median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3),
                      spread_pct=round(100 * (max(v) - min(v)) / statistics.median(v), 1))
    row['speedup_median'] = round(row['persistent']['moves_per_s_median'] / row['host_split']['moves_per_s_median'], 2)
    return row


def _players(name):
    return importlib.import_module('alphazero_general_amd.envs.' + name).Game.num_players()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--games', type=int, nargs='+', default=[128, 256, 512])
    ap.add_argument('--moves', type=int, default=3)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--quick', action='store_true', help='connect4 x 32 at 128 games only (a profiler run)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'arena_wide_throughput.json'))
    a = ap.parse_args()
    rows = []
    pairs = PAIRS[:1] if a.quick else PAIRS
    for name, width, sims in pairs:
        for B in ([128] if a.quick else a.games):
            for raw in (False, True):
                r = case(name, width, sims, B, raw, a.moves, a.reps)
                rows.append(r)
                print(json.dumps(r), flush=True)
    if not a.quick:
        with open(a.out, 'w') as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), fh, indent=1)


if __name__ == '__main__':
    main()
