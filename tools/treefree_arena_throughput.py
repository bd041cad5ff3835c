"""Tree-free players on one GPU: positions/s of DeviceGames.choose (RandomPlayer: policy=None; NNPlayer: a policy row at temperature
0.25) per game at 1 k and 64 k mid-game positions, and an arena comparison -- 128 connect4 games of the default net, 100 simulations
per move, against a random seat: once as ONE 128-slot engine (selfplay.ArenaRunner([net, RANDOM_SEAT])), once in the form an
unbatched Arena takes today (Arena.pyx:139-186 with a RandomPlayer: the games one after another, every MCTS move a search on one
tree): a ONE-slot engine played 128 times in sequence, the random side's moves drawn on the host and handed over with
advance(actions=...).

Timed windows as tools/device_games_throughput.py takes them (a pilot window sizes and warms; `--reps` windows, median with min / max).
No number here is a pass bar.  The result goes to `--out` (default profiles/treefree_arena_throughput.json) with the device named."""
import argparse
import importlib
import json
import os
import platform
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from device_games_throughput import GAMES, PLIES, midgame, windows  # noqa: E402
from alphazero_general_amd.games import DeviceGames  # noqa: E402


def choose_rows(a):
    rows = []
    for name in a.games:
        dg = DeviceGames(importlib.import_module('alphazero_general_amd.envs.' + name).Game)
        for n in a.sizes:
            states, _ = midgame(dg, n, PLIES[name], seed=n + len(name))
            policy = torch.rand((n, dg.A), device=dg.device)
            policy /= policy.sum(1, keepdim=True)
            temp = torch.full((n,), 0.25, dtype=torch.float32, device=dg.device)
            u = torch.rand(n, dtype=torch.float64, device=dg.device)
            out = dg.choose(states, u=u)
            rnd = windows(lambda: dg.choose(states, u=u, out=out), n, a.window, a.reps)
            nn = windows(lambda: dg.choose(states, policy, temp, u, out=out), n, a.window, a.reps)
            row = dict(game=name, positions=n, window_s=a.window, reps=a.reps, no_move=int(dg.choose(states, u=u).status.sum()),
                       choose_random_positions_per_s=rnd, choose_policy_temp025_positions_per_s=nn)
            rows.append(row)
            print(json.dumps(row), flush=True)
            torch.cuda.empty_cache()
    return rows


def arena_rows(a):
    from alphazero_general_amd import nnet as N
    from alphazero_general_amd.envs.connect4 import Game
    from alphazero_general_amd.selfplay import RANDOM_SEAT, ArenaRunner
    from alphazero_general_amd.utils import dotdict
    torch.manual_seed(0)
    net = N.NNetWrapper(Game, N.DEFAULT_NET_ARGS, device='cuda:0', dtype=torch.float16)
    net.refresh()
    args = dotdict(numMCTSSims=a.sims, gamesPerIteration=a.arena_games, cpuct=1.25, fpu_reduction=0.2, arenaTemp=0.25, use_draws_for_winrate=True)
    out = {}
    # (a) every game side by side
    r = ArenaRunner(Game, [net, RANDOM_SEAT], args, num_slots=a.arena_games, seed=1, seats='slot')
    r.play_round(); r.engine.reset(); r.engine.clear_outputs(); r.rounds = 0          # warm: code objects, scratch
    torch.cuda.synchronize(); t0 = time.perf_counter()
    c = r.run(a.arena_games)
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    wins, draws, _ = r.results()
    out['one_engine'] = dict(slots=a.arena_games, games=int(c['games_played']), seconds=round(dt, 4), games_per_s=round(c['games_played'] / dt, 1),
                             persistent_launch=bool(r.wide_search), net_wins=int(wins[0]), random_wins=int(wins[1]), draws=int(draws))
    r.engine.close()
    # (b) one game at a time on a one-slot engine, the random side's move from the host
    r = ArenaRunner(Game, [net, RANDOM_SEAT], dotdict(args, gamesPerIteration=1 << 30), num_slots=1, seed=1, seats='agent', result_capacity=4 * a.arena_games)
    e, rng = r.engine, np.random.RandomState(1)
    act = torch.zeros(1, dtype=torch.int32, device=e.device)

    def search():
        if r.wide_search:
            r._search_wide(a.sims)
        else:
            for _ in range(a.sims):
                r.step()
    search(); e.reset(); e.clear_outputs()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    games = moves = 0
    while games < a.arena_games:
        cells, player, turns = e.get_states()[0]
        if r.tree_free[r.player_to_index[player]]:                   # RandomPlayer.play on the host (GenericPlayers.py:47-52)
            g = Game.from_azg_state(cells, player, turns)
            valids = g.valid_moves()
            act[0] = int(rng.choice(len(valids), p=valids / np.sum(valids)))
        else:
            search()
            act[0] = -1
        e.advance(False, act)
        moves += 1
        games = e.counters()['num_results']
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    out['one_slot_in_sequence'] = dict(slots=1, games=int(games), moves=int(moves), seconds=round(dt, 4), games_per_s=round(games / dt, 1),
                                       persistent_launch=bool(r.wide_search))
    e.close()
    out['speedup'] = round(out['one_engine']['games_per_s'] / out['one_slot_in_sequence']['games_per_s'], 1)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--games', nargs='*', default=list(GAMES))
    ap.add_argument('--sizes', nargs='*', type=int, default=[1024, 65536])
    ap.add_argument('--window', type=float, default=0.25, help='seconds of launches per timed window')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--arena-games', type=int, default=128)
    ap.add_argument('--sims', type=int, default=100)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'treefree_arena_throughput.json'))
    a = ap.parse_args()
    res = dict(device=torch.cuda.get_device_name(), arch=getattr(torch.cuda.get_device_properties(0), 'gcnArchName', ''), torch=torch.__version__,
               hip=torch.version.hip, host_cpu=platform.processor() or platform.machine(),
               unit='choose: positions per second; median, min, max over the windows.  arena: connect4, default net, one run each',
               choose=choose_rows(a), arena=arena_rows(a))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
