"""Tree-free arena seats over two ranks (tests/treefree_rig.py: two ranks share GPU 0 over gloo): the seats travel with iteration.lead's
command -- RANDOM_SEAT as it is, a PolicySeat as its start temperature and iterated schedule, its network with the broadcast weights --
and the comparison a serving rank helps to play is the one two ranks play when each holds the nets and the seats."""
import json
import os
import signal
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tree_free_seats_reach_a_serving_rank(tmp_path):
    import treefree_rig as R
    from alphazero_general_amd import iteration as I
    out = str(tmp_path / 'treefree.json')
    env = dict(os.environ, AZG_DIST_BACKEND='gloo', AZG_SINGLE_DEVICE='1')
    env.pop('WORLD_SIZE', None); env.pop('RANK', None)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1', '--master-port', '29657',
           os.path.join(ROOT, 'tests', 'treefree_rig.py'), out]
    p = subprocess.Popen(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, start_new_session=True)
    try:
        log, _ = p.communicate(timeout=300)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)
        raise
    assert p.returncode == 0, log.decode(errors='replace')[-3000:]
    rec = json.load(open(out))
    assert json.load(open(out + '.rank1'))['served'] == 2            # the two arena commands; then 'stop'
    for kind in ('random', 'policy'):
        d, c = rec['direct_' + kind], rec['coach_' + kind]
        assert d == c, kind
        assert d['games'] == R.GAMES and d['ranks'] == 2 and sum(d['wins']) + d['draws'] == d['num_results'] >= R.GAMES
        assert d['winrates'] == I.winrates(d['wins'], d['draws'], True)
    assert rec['direct_random'] != rec['direct_policy']
