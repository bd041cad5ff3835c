"""Rig for tests/test_gpu_lookahead.py: started under torch.distributed.run with two ranks that share GPU 0 (as tests/treefree_rig.py).
One connect4 arena comparison [net, SCRIPTED_SEAT], played twice: `direct` -- every rank calls iteration.run_arena itself -- and `coach`
-- rank 0 hands its live net and the seat to iteration.lead, rank 1 sits in iteration.serve and builds nothing itself.  Rank 0 writes
the records as JSON (argv[1]), rank 1 the number of commands it served (argv[1] + '.rank1')."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from alphazero_general_amd import distributed as D  # noqa: E402
from alphazero_general_amd import iteration as I  # noqa: E402
from alphazero_general_amd.envs.connect4 import Game  # noqa: E402
from alphazero_general_amd.nnet import DEFAULT_NET_ARGS, NNetWrapper  # noqa: E402
from alphazero_general_amd.selfplay import SCRIPTED_SEAT  # noqa: E402
from alphazero_general_amd.utils import dotdict, default_temp_scaling  # noqa: E402

GAMES, SLOTS = 16, 8
KEEP = ('wins', 'draws', 'winrates', 'num_results', 'games', 'ranks', 'sims', 'expansions', 'rounds')


def args():
    return dotdict(numMCTSSims=8, cpuct=2.0, fpu_reduction=0.2, startTemp=1.0, arenaTemp=0.25, temp_scaling_fn=default_temp_scaling,
                   use_draws_for_winrate=True, _azg_seed=9)


def main():
    out_json = sys.argv[1]
    rank, local_rank, world = D.init_from_env()
    torch.cuda.set_device(local_rank)
    torch.manual_seed(1)
    net = NNetWrapper(Game, DEFAULT_NET_ARGS, device='cuda:0', dtype=torch.float16)
    r = I.run_arena(Game, [net, SCRIPTED_SEAT], args(), GAMES, num_slots=SLOTS, details=True)     # collective: every rank holds the net
    rec = {'direct': {k: r[k] for k in KEEP}}
    if rank == 0:
        r = I.lead('arena', Game, [net, SCRIPTED_SEAT], args(), num_games=GAMES, num_slots=SLOTS, details=True)
        rec['coach'] = {k: r[k] for k in KEEP}
        I.lead('stop', Game, [], args())
        with open(out_json, 'w') as f:
            json.dump(rec, f)
    else:
        del net
        torch.manual_seed(12345)                                     # (nothing this rank could build by itself equals rank 0's net)
        with open(out_json + '.rank1', 'w') as f:
            json.dump({'served': I.serve(Game)}, f)
    D.barrier()
    D.shutdown()


if __name__ == '__main__':
    main()
