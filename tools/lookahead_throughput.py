"""One ply on one GPU: positions/s of DeviceGames.lookahead -- `win` (num, actions, the children's win states) and `full` (children=True,
obs='nhwc8': the children themselves and their observations as the MFMA tower reads them) -- per game at 1 k and 64 k mid-game
positions, next to the composition a caller had before the dedicated launch: step(valid=True), torch's nonzero (a host read), step on
the repeated (position, action) rows.  Both sides run here, in the same session, on the same positions (tools/device_games_throughput.py
makes them: `PLIES` random legal plies from the opening).  Beside it, choose_scripted next to choose (RandomPlayer) for the games with a
scripted player.

A count is cut down where the outputs of `full` would not fit `--max-bytes` (max_children * (80 + H*W*16) bytes per position: hnefatafl's
448 children, gobang's 225); the row says how many positions were timed.  A timed window is about `--window` seconds of calls between
two device synchronises, every output of the dedicated launch allocated before it (out=); `--reps` windows, median with min / max.

No number here is a pass bar.  The result goes to `--out` (default profiles/lookahead_throughput.json) with the device named."""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import torch  # noqa: E402

from alphazero_general_amd.games import DeviceGames  # noqa: E402
from device_games_throughput import GAMES, PLIES, midgame, windows  # noqa: E402


def composed(dg, states, children, obs):
    """what lookahead replaces: the valid mask, its nonzero on the host side of torch, one step per (position, action) row"""
    valid = dg.step(states, next=False, win=False).valid
    idx = valid.nonzero()
    rows = states[idx[:, 0]]
    return dg.step(rows, idx[:, 1].to(torch.int32), next=children, valid=False, win=True, obs=obs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--games', nargs='*', default=list(GAMES))
    ap.add_argument('--sizes', nargs='*', type=int, default=[1024, 65536])
    ap.add_argument('--window', type=float, default=0.25, help='seconds of calls per timed window')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--max-bytes', type=float, default=8e9, help='cap on the outputs of one full lookahead')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lookahead_throughput.json'))
    a = ap.parse_args()
    rows = []
    for name in a.games:
        dg = DeviceGames(importlib.import_module('alphazero_general_amd.envs.' + name).Game)
        per_position = dg.max_children * (80 + dg.obs_shape[1] * dg.obs_shape[2] * 16 + dg.NV + 4) + 4
        for size in a.sizes:
            n = max(64, min(size, int(a.max_bytes // per_position)))
            states, _ = midgame(dg, n, PLIES[name], seed=size + len(name))
            row = dict(game=name, positions=n, asked=size, window_s=a.window, reps=a.reps, max_children=dg.max_children,
                       mean_children=round(float(dg.lookahead(states, win=False).num.float().mean()), 2))
            for tag, kw in (('win', dict(win=True)), ('full', dict(win=True, children=True, obs='nhwc8'))):
                out = dg.lookahead(states, **kw)
                row['lookahead_%s_positions_per_s' % tag] = windows(lambda: dg.lookahead(states, out=out, **kw), n, a.window, a.reps)
                del out
                torch.cuda.empty_cache()
                row['composed_%s_positions_per_s' % tag] = windows(lambda: composed(dg, states, 'children' in kw, kw.get('obs')), n, a.window, a.reps)
                torch.cuda.empty_cache()
            u = torch.rand(n, dtype=torch.float64, device=dg.device)
            cout = dg.choose(states, u=u)
            row['choose_random_positions_per_s'] = windows(lambda: dg.choose(states, u=u, out=cout), n, a.window, a.reps)
            if dg.scripted_player is not None:
                row['choose_scripted_positions_per_s'] = windows(lambda: dg.choose_scripted(states, u, out=cout), n, a.window, a.reps)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del states
            torch.cuda.empty_cache()
    res = dict(device=torch.cuda.get_device_name(), arch=getattr(torch.cuda.get_device_properties(0), 'gcnArchName', ''), torch=torch.__version__,
               hip=torch.version.hip, unit='positions per second; median, min, max over the windows', rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
