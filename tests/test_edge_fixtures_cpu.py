"""The edge fixtures of the two games without a C oracle, othello and gobang (tests/golden/{ot,gb}_edge.npz: the reference's
MCTS.pyx / SelfPlayAgent.pyx on the tests/edge_eval.py rows, written by make_goldens.gen_edge through make_othello_goldens.py /
make_gobang_goldens.py), checked without a GPU:

  * the fixtures reach their edges: the config list, the exact root sizes, every coverage floor the generator asserts (the
    shared ones and gobang's chunk / tie / template-switch floors), paths of 24 and more actions, probs the reference raised
    on, argmax ties at temperature 0;
  * the replay tests/test_gpu_tree_edges.py depends on: every recorded path of every (config, root, simulation) is played on
    the host env (alphazero_general_amd/envs, pinned to the reference's rule tables by test_othello_cpu.py / test_gobang_cpu.py),
    every action must be legal where it is played, no position before the leaf may be terminal, and the evaluator row
    recomputed at the leaf must have the recorded crc;
  * what a fixture says twice agrees: the final counts with the final children and, for gobang, with the last per-simulation
    crc; root n with the simulation count (`gbr` is the group of random gobang prefixes that gb_edge.npz holds under `rnd_`);
  * with the reference checkout present, the generators write both files again array for array.

The reference's othello has no pass action (a side without a move ends the game, othello.pyx:83-96; 64 actions), so the
smallest othello root is one with a single legal move."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import edge_eval as ee

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, 'golden')
REF = '/root/reference'
NAMES = ('ot', 'gb')
EDGE_FLOORS = {'tied_max': 500, 'zero_prior_selected': 50, 'seen_sum_tree': 100, 'seen_sum_serial_wide': 50, 'draw_backups': 100}
GB_FLOORS = {'chosen_chunk1': 100, 'chosen_chunk2': 100, 'chosen_chunk3': 100, 'tie_spans_chunks': 500, 'nc_switch': 50,
             'zero_prior_selected_wide': 20, 'seen_sum_serial_over128': 50}
GB_KS = [193, 192, 191, 129, 128, 127, 66, 65, 64, 63, 2, 1]
NOISY = ('dyadic_noise1', 'onehot', 'spread_powf')
_cache = {}


def _edge(name):
    if name not in _cache:
        _cache[name] = ee.load(G, name)
    return _cache[name]


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


@pytest.mark.parametrize('name', NAMES)
def test_edge_fixture_reaches_its_edges(name):
    d = _edge(name)
    assert os.path.getsize(os.path.join(G, name + '_edge.npz')) <= 400 * 1000
    assert list(d['configs']) == ee.CONFIGS
    assert (d['prob_temps'] == np.array([1.0, 2.0, 0.5, 0.1, 0.0, 0.01], np.float32)).all()
    names = list(d['cov_names'])
    tot = dict(zip(names, sum(d[c + '_cov'] for c in ee.CONFIGS).tolist()))
    for k, floor in dict(EDGE_FLOORS, **(GB_FLOORS if name == 'gb' else {})).items():
        assert tot[k] >= floor, (k, tot[k])
    roots = ee.roots(d, ee.GAMES[name])
    ks = [int(np.asarray(g.valid_moves()).sum()) for g in roots]
    assert all(not g.win_state().any() for g in roots)
    kind = d['root_kind'].tolist()
    assert all(kd == 0 or kd == k for kd, k in zip(kind, ks))
    if name == 'gb':
        assert [k for kd, k in zip(kind, ks) if kd] == GB_KS and kind.count(0) == 1 and ks[0] == 225
        assert int(d['sims']) >= 240
        dr = _edge('gbr')                                                         # the other random prefixes: mid-opening roots
        kr = [int(g.valid_moves().sum()) for g in ee.roots(dr, 4)]
        assert len(kr) == 4 and all(195 < k < 225 for k in kr) and (dr['root_kind'] == 0).all() and int(dr['sims']) == 48
        assert list(dr['configs']) == ee.CONFIGS and (dr['prob_temps'] == d['prob_temps']).all()
        assert (d['cells'].dtype, d['cells'].shape[1]) == (np.uint8, 64)       # the packed ABI layout
        for c in ee.CONFIGS:                                                      # only the noisy configs reach the cast
            assert (d[c + '_cov'][names.index('noise_cast_underflows')] > 0) == (c in NOISY), c
            assert d[c + '_a'].shape[1] == 225 and c + '_rootn' not in d          # all k children; crcs per simulation
    else:
        assert [k for kd, k in zip(kind, ks) if kd] == [1, 2] and kind.count(0) == 12
        assert int(d['sims']) == 60 and d['cells'].shape[1] == 64
    for c in ee.CONFIGS:
        fam = str(d[c + '_family'])
        if fam != 'spread':                                                       # "only spread rows underflow" holds apart from the cast
            assert d[c + '_cov'][names.index('underflows')] == 0, c
    assert tot['underflows'] > 0
    assert max(int(d[c + '_depth'].max()) for c in ee.CONFIGS) >= 24
    assert sum(int(d[c + '_probs_raised'].sum()) for c in ee.CONFIGS) > 0
    tied0 = sum(int(((d[c + '_counts'] == d[c + '_counts'].max(1, keepdims=True)).sum(1) > 1).sum()) for c in ee.CONFIGS)
    assert tied0 > 0                                                              # argmax ties at temperature 0: final trees ...
    ac = d['agent_counts']
    assert int(((ac == ac.max(-1, keepdims=True)).sum(-1) > 1).sum()) >= 20      # ... and the agent's moves (k_play)
    B, sims, games = (2, 8, 2) if name == 'gb' else (4, 12, 4)
    assert (int(d['agent_B']), int(d['agent_sims']), int(d['agent_games'])) == (B, sims, games)
    assert len(d['agent_r_turns']) >= games and len(ee.unpack_pi(d)) > 0


@pytest.mark.parametrize('name,cname', [(n, c) for n in NAMES + ('gbr',) for c in ee.CONFIGS])
def test_edge_rows_replay_on_the_host_env(name, cname):
    d = _edge(name)
    gid = ee.GAMES[name]
    A, NV = ee.game_sizes(gid)
    fam, seed, sims = str(d[cname + '_family']), int(d[cname + '_seed']), int(d[cname + '_cfg'][4])
    roots = ee.roots(d, gid)
    assert sims == int(d['sims']) and d[cname + '_row_crc'].shape == (len(roots), sims)
    for r, root in enumerate(roots):
        for s in range(sims):
            dep = int(d[cname + '_depth'][r, s])
            path = d[cname + '_paths'][r, s]
            pad = 255 if path.dtype == np.uint8 else -1                          # (gb_edge: uint8 paths)
            assert (path[:dep] != pad).all() and (path[dep:] == pad).all(), (r, s)
            g = root.clone()
            for a in path[:dep]:
                assert not g.win_state().any() and g.valid_moves()[a] == 1, (r, s, int(a))
                g.play_action(int(a))
            term = g.win_state().any()
            p, v = ee.row(fam, seed, r, s, A, NV, None if term else np.asarray(g.valid_moves()))
            assert ee.row_crc(p, v) == d[cname + '_row_crc'][r, s], (r, s)
            q, w = ee.leaf_row(fam, seed, root, r, s, path[:dep], A, NV)           # the helper the GPU replay calls
            assert q.tobytes() == p.tobytes() and w.tobytes() == v.tobytes(), (r, s)
        assert d[cname + '_depth'][r, 0] == 0                                     # the first simulation expands the root


@pytest.mark.parametrize('name,cname', [(n, c) for n in NAMES + ('gbr',) for c in ee.CONFIGS])
def test_edge_final_records_agree(name, cname):
    d = _edge(name)
    roots = ee.roots(d, ee.GAMES[name])
    sims = int(d['sims'])
    for r, root in enumerate(roots):
        valid = np.asarray(root.valid_moves())
        k = int(valid.sum())
        a, n = d[cname + '_a'][r], d[cname + '_n'][r]
        assert sorted(a[:k].tolist()) == np.flatnonzero(valid).tolist() and (a[k:] == -1).all() and (n[k:] == 0).all(), r
        counts = np.zeros(len(valid), np.int32)
        counts[a[:k]] = n[:k]
        assert (counts == d[cname + '_counts'][r]).all() and d[cname + '_counts'].dtype == np.int32
        assert d[cname + '_root_n'][r] == sims and counts.sum() == sims - 1
        assert (d[cname + '_rootN'][r] == np.arange(1, sims + 1)).all()
        if cname + '_counts_crc' in d:
            assert d[cname + '_counts_crc'][r, sims - 1] == crc(counts), r
            assert d[cname + '_counts_crc'][r, 0] == crc(np.zeros_like(counts)), r
        else:
            assert (d[cname + '_rootn'][r, sims - 1][:k] == n[:k]).all(), r


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, 'alphazero')), reason='needs the reference checkout (build container only)')
@pytest.mark.parametrize('name', NAMES)
def test_edge_fixtures_regenerate_identically(tmp_path, name):
    """the generator, run on the reference again into a temporary directory, writes the committed fixture array for array"""
    mod = {'ot': 'make_othello_goldens', 'gb': 'make_gobang_goldens'}[name]
    code = 'import sys; sys.path.insert(0, %r); import %s as m; m.main([%r], out_dir=%r, verbose=False)' % (G, mod, name + '_edge', str(tmp_path))
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=1800, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    new, old = np.load(os.path.join(str(tmp_path), name + '_edge.npz')), np.load(os.path.join(G, name + '_edge.npz'))
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        a, b = new[k], old[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (name, k)
