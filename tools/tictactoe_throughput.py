"""Tic-tac-toe self-play throughput on one GPU: the persistent search launch (azg_search_wide_exact_f16, one launch per move) against the
launch-per-phase loop (azg_select -> NNetWrapper.process -> azg_backup per simulation) at the same size, for envs/tictactoe/train.py's
32 x 4 net with 4 + 4 head channels (zero-padded to the factorised path) and the 32 x 4 default net (16 + 16), at 128, 512 and 2048
games x 100 simulations (train.py: numMCTSSims=100, arenaBatchSize=2048).  The two forms ALTERNATE, three repeats each; a case reports
the median and the spread (max - min) of its repeats.  The rate is SIMULATIONS per second (games x simulations x moves / seconds): both
forms run the same simulations on the same positions (same seeds; the launches are bit-identical), while the expansions of a repeat depend
on how far its games have got -- a game lasts five to nine moves, and a simulation that ends in a decided position expands nothing -- so
expansions per second, reported beside it, swing by a factor of two between repeats whose times agree to a few per cent.  Prints one JSON line per case and per verdict and writes them all to
profiles/tictactoe_throughput.json.  HipResNet.search_preferred for (tictactoe, 32) may turn true only if this file shows the persistent
form faster at ALL three sizes by more than the spread, for both nets.  Kernel averages: run it under the profiler, e.g.

    rocprofv3 --kernel-trace --stats --output-format csv -d profiles/tictactoe_rocprof -o tictactoe -- python tools/tictactoe_throughput.py
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
from alphazero_general_amd.envs.tictactoe import Game  # noqa: E402
from alphazero_general_amd.nnet import DEFAULT_NET_ARGS, TICTACTOE_NET_ARGS, NNetWrapper  # noqa: E402

PATHS = ('persistent', 'phase')


class Case:
    """one (net, games, form): its engine lives across the repeats, so that the forms can take turns"""

    def __init__(self, net, B, sims, path):
        self.net, self.B, self.sims, self.path = net, B, sims, path
        self.eng = DeviceEngine(Game.AZG_GAME_ID, B, cpuct=2.0, fpu_reduction=0.2, add_root_noise=True, add_root_temp=True, seed=3, sims_hint=sims)
        self.obs = self.eng.new_obs(torch.float16) if path == 'phase' else None
        if path == 'persistent':
            net._hip.search(self.eng, 0, exact=True)             # one-time set-up (tile trial)
        self.move()                                              # warm
        torch.cuda.synchronize()

    def move(self):
        if self.path == 'persistent':
            self.net._hip.search(self.eng, self.sims, exact=True)
        else:
            for _ in range(self.sims):
                self.eng.select(self.obs)
                p, v = self.net.process(self.obs)
                self.eng.backup(p.contiguous(), v.contiguous())
        self.eng.advance(True)

    def timed(self, moves):
        e0 = self.eng.counters()['expansions']
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(moves):
            self.move()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return self.B * self.sims * moves / dt, dt, (self.eng.counters()['expansions'] - e0) / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--moves', type=int, default=3)
    ap.add_argument('--sims', type=int, default=100)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--games', type=int, nargs='+', default=[128, 512, 2048])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tictactoe_throughput.json'))
    a = ap.parse_args()
    rows = []
    for net_name, args in (('tictactoe_32x4_h4', TICTACTOE_NET_ARGS), ('default_32x4', DEFAULT_NET_ARGS)):
        torch.manual_seed(0)
        net = NNetWrapper(Game, args, device='cuda:0').refresh()
        assert net._hip is not None and net._hip.fact_head and net._hip.can_search
        faster = []
        for B in a.games:
            cases = {p: Case(net, B, a.sims, p) for p in PATHS}
            rates = {p: [] for p in PATHS}
            secs = {p: [] for p in PATHS}
            exps = {p: [] for p in PATHS}
            for _ in range(a.repeats):                           # the forms alternate
                for p in PATHS:
                    r, dt, ex = cases[p].timed(a.moves)
                    rates[p].append(r); secs[p].append(dt); exps[p].append(ex)
            for p in PATHS:
                rec = dict(net=net_name, path=p, games=B, sims=a.sims, moves=a.moves, repeats=a.repeats,
                           simulations_per_s=round(statistics.median(rates[p])), spread=round(max(rates[p]) - min(rates[p])),
                           all_simulations_per_s=[round(x) for x in rates[p]], seconds=[round(x, 5) for x in secs[p]],
                           expansions_per_s=[round(x) for x in exps[p]],
                           tile=net._hip.search_tile(cases[p].eng, exact=True) if p == 'persistent' else None)
                print(json.dumps(rec), flush=True)
                rows.append(rec)
                cases[p].eng.close()
            gap = statistics.median(rates['persistent']) - statistics.median(rates['phase'])
            spread = max(max(rates[p]) - min(rates[p]) for p in PATHS)
            faster.append(bool(gap > spread))
        verdict = dict(net=net_name, verdict='persistent faster at every size by more than the spread' if all(faster)
                       else 'not shown faster at every size', persistent_faster_beyond_spread=dict(zip([str(b) for b in a.games], faster)))
        print(json.dumps(verdict), flush=True)
        rows.append(verdict)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(rows, fh, indent=1)


if __name__ == '__main__':
    main()
