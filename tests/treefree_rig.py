"""Rig for tests/test_gpu_treefree_ranks.py: started under torch.distributed.run with two ranks that share GPU 0 (as tests/iteration_rig.py).
One arena comparison per tree-free seat kind, [net, RANDOM_SEAT] and [net, PolicySeat(net2)], played twice: `direct` -- every rank calls
iteration.run_arena itself -- and `coach` -- rank 0 hands its live nets and the seats to iteration.lead, rank 1 sits in iteration.serve
and builds nothing itself.  Rank 0 writes the records as JSON (argv[1]), rank 1 the number of commands it served (argv[1] + '.rank1')."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from alphazero_general_amd import distributed as D  # noqa: E402
from alphazero_general_amd import iteration as I  # noqa: E402
from alphazero_general_amd.envs.tictactoe import Game  # noqa: E402
from alphazero_general_amd.nnet import TICTACTOE_NET_ARGS, NNetWrapper  # noqa: E402
from alphazero_general_amd.selfplay import RANDOM_SEAT, PolicySeat  # noqa: E402
from alphazero_general_amd.utils import dotdict, default_temp_scaling  # noqa: E402

GAMES, SLOTS = 24, 8
KEEP = ('wins', 'draws', 'winrates', 'num_results', 'games', 'ranks', 'sims', 'expansions', 'rounds')


def args():
    return dotdict(numMCTSSims=8, cpuct=2.0, fpu_reduction=0.2, startTemp=1.0, arenaTemp=0.25, temp_scaling_fn=default_temp_scaling,
                   use_draws_for_winrate=True, _azg_seed=9)


def net(seed):
    torch.manual_seed(seed)
    return NNetWrapper(Game, TICTACTOE_NET_ARGS, device='cuda:0', dtype=torch.float16)


def seats(kind, nets):
    return [nets[0], RANDOM_SEAT if kind == 'random' else PolicySeat(nets[1], 0.5, default_temp_scaling)]


def main():
    out_json = sys.argv[1]
    rank, local_rank, world = D.init_from_env()
    torch.cuda.set_device(local_rank)
    rec = {}
    nets = [net(1), net(2)]
    for kind in ('random', 'policy'):                                # collective: every rank holds the nets
        r = I.run_arena(Game, seats(kind, nets), args(), GAMES, num_slots=SLOTS, details=True)
        rec['direct_' + kind] = {k: r[k] for k in KEEP}
    if rank == 0:
        for kind in ('random', 'policy'):
            r = I.lead('arena', Game, seats(kind, nets), args(), num_games=GAMES, num_slots=SLOTS, details=True)
            rec['coach_' + kind] = {k: r[k] for k in KEEP}
        I.lead('stop', Game, [], args())
        with open(out_json, 'w') as f:
            json.dump(rec, f)
    else:
        del nets
        torch.manual_seed(12345)                                     # (nothing this rank could build by itself equals rank 0's nets)
        with open(out_json + '.rank1', 'w') as f:
            json.dump({'served': I.serve(Game)}, f)
    D.barrier()
    D.shutdown()


if __name__ == '__main__':
    main()
