"""Othello self-play throughput on one GPU: the persistent search launch (azg_search_wide_exact_f16, one launch per move) against the
launch-per-phase loop (azg_select -> NNetWrapper.process -> azg_backup per simulation) at the same size, for envs/othello/train.py's
64 x 4 net and the 32 x 4 default net, at 512 and 2048 games x 100 simulations.  Prints one JSON line per case and writes them all to
profiles/othello_throughput.json.  Kernel averages: run it under the profiler, e.g.

    rocprofv3 --kernel-trace --stats --output-format csv -d profiles/othello_rocprof -o othello -- python tools/othello_throughput.py
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from alphazero_general_amd.engine import DeviceEngine  # noqa: E402
from alphazero_general_amd.envs.othello import Game  # noqa: E402
from alphazero_general_amd.nnet import DEFAULT_NET_ARGS, OTHELLO_NET_ARGS, NNetWrapper  # noqa: E402


def one(net_name, args, B, sims, moves, path):
    torch.manual_seed(0)
    net = NNetWrapper(Game, args, device='cuda:0').refresh()
    assert net._hip is not None and net._hip.can_search
    eng = DeviceEngine(3, B, cpuct=4.0, fpu_reduction=0.4, add_root_noise=True, add_root_temp=True, seed=3, sims_hint=sims)
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
        net._hip.search(eng, 0, exact=True)                  # one-time set-up (tile trial)
    move()                                                   # warm
    torch.cuda.synchronize()
    e0 = eng.counters()['expansions']
    t0 = time.perf_counter()
    for _ in range(moves):
        move()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    c = eng.counters()
    rec = dict(net=net_name, path=path, games=B, sims=sims, moves=moves, seconds=round(dt, 4),
               expansions_per_s=round((c['expansions'] - e0) / dt), tile=net._hip.search_tile(eng, exact=True) if path == 'persistent' else None)
    eng.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--moves', type=int, default=3)
    ap.add_argument('--sims', type=int, default=100)
    ap.add_argument('--games', type=int, nargs='+', default=[512, 2048])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'othello_throughput.json'))
    a = ap.parse_args()
    rows = []
    for net_name, args in (('othello_64x4', OTHELLO_NET_ARGS), ('default_32x4', DEFAULT_NET_ARGS)):
        for B in a.games:
            for path in ('persistent', 'phase'):
                r = one(net_name, args, B, a.sims, a.moves, path)
                print(json.dumps(r), flush=True)
                rows.append(r)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(rows, fh, indent=1)


if __name__ == '__main__':
    main()
