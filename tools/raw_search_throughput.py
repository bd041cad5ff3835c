"""Network-free searches on one GPU: MCTS.raw_search (RawMCTSPlayer's move) and warm-up self-play rounds, as ONE launch per move
(azg_search_raw) against the launch-per-phase forms.  The form is picked by `hasattr(engine, 'search_raw')`, so the same file also
runs on a commit that has no such launch (it then measures only the forms that commit has).

  (a) ms per MCTS.raw_search(g, 100, False, False) move, one tree, connect4 and brandubh: `--moves` moves of a game, median.
  (b) ms per warm-up round of SelfPlayRunner(warmup=True, numWarmupSims=5) at 128 / 512 / 2048 slots, connect4 and brandubh: graph replay
      of the launch-per-phase form and of the raw launch, alternating, `--reps` times `--rounds` rounds each; median with min / max.
  (c) tree-only expansions/s of the raw launch itself at 2048 connect4 slots x 100 simulations per move (no network anywhere).
  (d) `--hnefatafl`: 128 / 512 / 2048 hnefatafl games x 100 simulations per move (the widest move lists: up to seven chunks of 64
      children), the raw launch against `sims` x [azg_select(NULL), azg_backup] of the same build, alternating: expansions/s and ms per
      move, median of `--reps` repetitions with the spread.  Written to profiles/hnefatafl_raw_throughput.json.  A record, not a bar.

Every timed window ends in a device synchronise.  One JSON line per case; all of them go to `--out` under `--label` (the file keeps the
other labels it holds: run it on the commit before and on this one, profiles/raw_search_throughput.json holds both)."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from alphazero_general_amd.engine import DeviceEngine  # noqa: E402
from alphazero_general_amd.MCTS import MCTS  # noqa: E402
from alphazero_general_amd.selfplay import SelfPlayRunner  # noqa: E402
from alphazero_general_amd.utils import default_temp_scaling, dotdict  # noqa: E402

HAS_RAW = hasattr(DeviceEngine, 'search_raw')


def game_cls(name):
    return importlib.import_module('alphazero_general_amd.envs.' + name).Game


def med(xs):
    xs = sorted(xs)
    return dict(median=round(statistics.median(xs), 4), min=round(xs[0], 4), max=round(xs[-1], 4))


def raw_search_moves(name, moves, reps):
    """(a): the time of MCTS.raw_search alone (it ends in a blocking read of the tree), move after move of one game per repeat"""
    Game = game_cls(name)
    args = dotdict(cpuct=1.25, fpu_reduction=0.2, root_noise_frac=0.1, root_policy_temp=1.1, min_discount=1, _num_players=Game.num_players() + 1,
                   numMCTSSims=100, _azg_seed=7)
    per_rep = []
    for rep in range(reps + 1):                                 # (the first repeat warms: code objects, allocations)
        m, g, ms = MCTS(args), Game(), []
        for _ in range(moves):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.raw_search(g, 100, False, False)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
            a = m.best_action(g)
            m.update_root(g, a); g.play_action(a)
            if np.asarray(g.win_state()).any():
                break
        if rep:
            per_rep.append(statistics.median(ms))
        m._engine.close()
    return dict(case='raw_search_move', game=name, sims=100, moves=moves, reps=reps, form='launch' if HAS_RAW else 'phase', ms_per_move=med(per_rep))


def warmup_rounds(name, B, rounds, reps):
    """(b): graph replays of a whole warm-up round (numWarmupSims = 5 simulations + playMoves), the forms alternating"""
    Game = game_cls(name)
    a = dotdict(numMCTSSims=25, numFastSims=20, numWarmupSims=5, probFastSim=0.0, gamesPerIteration=1 << 30, cpuct=1.25, fpu_reduction=0.2,
                root_noise_frac=0.1, root_policy_temp=1.1, min_discount=1.0, add_root_noise=True, add_root_temp=True, symmetricSamples=True,
                mctsResetThreshold=0, startTemp=1.0, arenaTemp=0.25, temp_scaling_fn=default_temp_scaling)
    from alphazero_general_amd import _abi
    gi = _abi.game_info(Game.AZG_GAME_ID)
    cap = B * (rounds * reps + 8) * gi.num_symmetries
    forms = ('phase', 'launch') if HAS_RAW else ('phase',)
    runners = {}
    for f in forms:
        r = SelfPlayRunner(Game, None, a, num_slots=B, seed=5, warmup=True, example_capacity=cap, fused_search=(f == 'launch'))
        assert r.round_graph and bool(r.fused_search) == (f == 'launch')
        r.prepare()
        for _ in range(3):
            r.play_round()
        runners[f] = r
    ms = {f: [] for f in forms}
    for _ in range(reps):
        for f in forms:
            r = runners[f]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(rounds):
                r.play_round()
            torch.cuda.synchronize()
            ms[f].append((time.perf_counter() - t0) * 1e3 / rounds)
    out = []
    for f in forms:
        c = runners[f].counters()                               # (raises on a sticky device error)
        out.append(dict(case='warmup_round', game=name, slots=B, sims=5, rounds=rounds, reps=reps, form=f, ms_per_round=med(ms[f]),
                        games_played=c['games_played'], sims_done=c['sims']))
        for ln in runners[f].lanes:
            ln.engine.close()
    return out


def tree_only(B, sims, moves, reps):
    """(c): the launch by itself -- every slot's `sims` simulations, then playMoves -- in expansions per second"""
    rates = []
    for _ in range(reps):
        e = DeviceEngine(0, B, seed=3, sims_hint=sims, add_root_noise=True, add_root_temp=True)
        fill, vrow = float(np.float32(1 / e.A)), np.full(e.NV, 1 / e.NV, np.float32)

        def move():
            e.search_raw(sims, fill, vrow)
            e.advance(True)
        move()
        torch.cuda.synchronize()
        x0 = e.counters()['expansions']
        t0 = time.perf_counter()
        for _ in range(moves):
            move()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        rates.append((e.counters()['expansions'] - x0) / dt)
        e.close()
    return dict(case='tree_only', game='connect4', slots=B, sims=sims, moves=moves, reps=reps, form='launch', expansions_per_s=med(rates))


def hnefatafl_moves(B, sims, moves, reps):
    """(d): whole moves (`sims` simulations + playMoves, no samples kept) of B hnefatafl games from the opening, the two forms alternating"""
    Game = game_cls('hnefatafl')
    gid = Game.AZG_GAME_ID
    # (the library's default store holds 16 moves' worth of 448-child expansions: 46 MB a tree; three moves' worth is plenty here -- a
    #  move adds about sims x 120 nodes and the played child's subtree is compacted once less than a move's worth is free)
    mk = lambda: DeviceEngine(gid, B, seed=3, sims_hint=sims, add_root_noise=True, add_root_temp=True, nodes_per_tree=3 * sims * 448 + 64)
    eng = dict(launch=mk(), phase=mk())
    fill, vrow = float(np.float32(1 / eng['phase'].A)), np.full(eng['phase'].NV, 1 / eng['phase'].NV, np.float32)
    pol = torch.full((B, eng['phase'].A), fill, dtype=torch.float32, device=eng['phase'].device)
    val = torch.from_numpy(np.tile(vrow, (B, 1))).to(eng['phase'].device)

    def move(f):
        e = eng[f]
        if f == 'launch':
            e.search_raw(sims, fill, vrow)
        else:
            for _ in range(sims):
                e.select(None)
                e.backup(pol, val)
        e.advance(False)
    ms, rate = {f: [] for f in eng}, {f: [] for f in eng}
    for f in eng:
        move(f)
    for _ in range(reps):
        for f in eng:
            torch.cuda.synchronize()
            x0 = eng[f].counters()['expansions']
            t0 = time.perf_counter()
            for _ in range(moves):
                move(f)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            ms[f].append(dt * 1e3 / moves)
            rate[f].append((eng[f].counters()['expansions'] - x0) / dt)
    same = bool(torch.equal(eng['launch'].root_counts(), eng['phase'].root_counts()))
    out = [dict(case='hnefatafl_move', game='hnefatafl', slots=B, sims=sims, moves=moves, reps=reps, form=f, ms_per_move=med(ms[f]),
                expansions_per_s=med(rate[f]), max_nodes_used=eng[f].counters()['max_nodes_used'], forms_agree=same) for f in eng]
    for e in eng.values():
        e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--label', required=True, help="which commit this is, e.g. 'parent' or 'branch'")
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'raw_search_throughput.json'))
    ap.add_argument('--games', nargs='+', default=['connect4', 'brandubh'])
    ap.add_argument('--slots', type=int, nargs='+', default=[128, 512, 2048])
    ap.add_argument('--moves', type=int, default=8)
    ap.add_argument('--rounds', type=int, default=30)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--hnefatafl', action='store_true', help='case (d) only, into profiles/hnefatafl_raw_throughput.json')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    rows = []

    def emit(r):
        print(json.dumps(r), flush=True)
        rows.append(r)
    if a.hnefatafl:
        if a.out == ap.get_default('out'):
            a.out = os.path.join(ROOT, 'profiles', 'hnefatafl_raw_throughput.json')
        for B in a.slots:
            for r in hnefatafl_moves(B, 100, a.moves, a.reps):
                emit(r)
        a.games = []
    for g in a.games:
        emit(raw_search_moves(g, a.moves, a.reps))
    for g in a.games:
        for B in a.slots:
            for r in warmup_rounds(g, B, a.rounds, a.reps):
                emit(r)
    if HAS_RAW and not a.hnefatafl:
        emit(tree_only(2048, 100, 10, a.reps))
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            doc = json.load(fh)
    doc[a.label] = rows
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(doc, fh, indent=1)


if __name__ == '__main__':
    main()
