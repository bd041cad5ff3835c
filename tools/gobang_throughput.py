"""Gobang self-play throughput on one GPU: the persistent search launch (azg_search_wide_exact_f16, one launch per move) against the
launch-per-phase loop (azg_select -> NNetWrapper.process on the 15x15 HIP tower -> azg_backup per simulation) at the same size, for the
reference's default 32 x 4 net, a 64 x 4 net and envs/gobang/train.py's 128 x 8 net, at several game counts (`--nets` picks some of
them).  Each case is measured `--reps` times, the two forms alternating, and the median kept with the spread (min, max).
Prints one JSON line per case and writes them all to `--out` (default profiles/gobang_throughput.json, the record of the 32 x 4 and
64 x 4 A/B and of the 128 x 8 per-phase baseline; the 128 x 8 net's A/B of its persistent launch is meant to go to
profiles/gobang128_throughput.json: --nets gobang_128x8 --out profiles/gobang128_throughput.json).  Kernel averages: run it under the
profiler, e.g.

    rocprofv3 --kernel-trace --stats --output-format csv -d profiles/gobang_rocprof -o gobang -- python tools/gobang_throughput.py
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from alphazero_general_amd.engine import DeviceEngine  # noqa: E402
from alphazero_general_amd.envs.gobang import Game  # noqa: E402
from alphazero_general_amd.nnet import DEFAULT_NET_ARGS, GOBANG_NET_ARGS, NNetWrapper  # noqa: E402
from alphazero_general_amd.utils import dotdict  # noqa: E402

NETS = (('default_32x4', DEFAULT_NET_ARGS), ('gobang_64x4', dotdict(dict(DEFAULT_NET_ARGS, num_channels=64))), ('gobang_128x8', GOBANG_NET_ARGS))


def one(net, path, B, sims, moves):
    eng = DeviceEngine(4, B, cpuct=2.0, fpu_reduction=0.1, add_root_temp=True, seed=3, sims_hint=sims)
    obs = eng.new_obs(torch.float16) if path == 'phase' else None

    def move():
        if path == 'persistent':
            net._hip.search(eng, sims, exact=True)
        else:
            for _ in range(sims):
                eng.select(obs)
                p, v = net.process(obs)
                eng.backup(p.contiguous(), v.contiguous())
        eng.advance(True)

    if path == 'persistent':
        net._hip.search(eng, 0, exact=True)                  # one-time set-up

    move()                                                   # warm
    torch.cuda.synchronize()
    e0 = eng.counters()['expansions']
    t0 = time.perf_counter()
    for _ in range(moves):
        move()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    c = eng.counters()
    eng.close()
    return dt, c['expansions'] - e0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--moves', type=int, default=2)
    ap.add_argument('--sims', type=int, default=50)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--games', type=int, nargs='+', default=[128, 512, 2048])
    ap.add_argument('--nets', nargs='+', default=[n for n, _ in NETS], choices=[n for n, _ in NETS])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gobang_throughput.json'))
    a = ap.parse_args()
    rows = []
    for net_name, args in NETS:
        if net_name not in a.nets:
            continue
        torch.manual_seed(0)
        net = NNetWrapper(Game, args, device='cuda:0').refresh()
        assert net._hip is not None
        paths = ('persistent', 'phase') if net._hip.can_search else ('phase',)
        for B in a.games:
            runs = {p: [] for p in paths}
            for _ in range(a.reps):
                for p in paths:
                    runs[p].append(one(net, p, B, a.sims, a.moves))
            for p in paths:
                rates = sorted(x / dt for dt, x in runs[p])
                r = dict(net=net_name, path=p, games=B, sims=a.sims, moves=a.moves, reps=a.reps,
                         expansions_per_s=round(statistics.median(rates)), min=round(rates[0]), max=round(rates[-1]))
                print(json.dumps(r), flush=True)
                rows.append(r)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(rows, fh, indent=1)


if __name__ == '__main__':
    main()
