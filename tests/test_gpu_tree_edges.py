"""The tree kernels (csrc/azg_kernels.h: best_child, leaf_policy / masked_sum, backup_path, root_probs, k_root_stats) held to the
REFERENCE at its edges (pytest -m gpu): tests/golden/{c4,tm,br,ot,gb}_edge.npz, made by running the reference's MCTS.pyx /
SelfPlayAgent.pyx on the tests/edge_eval.py rows -- exact PUCT ties, zero and denormal priors, both forms of the seen-policy
sum, exact draw values, cpuct 0 / 50, fpu_reduction -1 / 0, noise_frac 1, root temperatures 0.5 / 2 / 1.1, roots with 1, 2,
63, 64 and 65 children, paths of 24 and more actions.  The device is compared with the fixtures directly, not with the oracle
(tests/test_oracle_golden.py pins the oracle to the same fixtures on the CPU).

gb_edge is the four-chunk family (best_child<G, 4>, leaf_policy<G, 4>, the four-chunk add_children and the per-node switch to
the one-chunk templates at k <= 64): roots of 225, 193, 192, 191, 129, 128, 127, 66, 65, 64, 63, 2 and 1 legal moves, 241
simulations each (and, as `gbr`, four random prefixes of 201 to 220 legal moves, 48 simulations each), so that under the first-play bonus the first maximum sweeps every chunk out of ties that span chunks, zero
priors are chosen among more than 64 children, the serial seen-sum runs over more than 128, and descents cross from wide
nodes into k <= 64.  Its noisy configs hold the device to the reference's arithmetic with only numpy's underflow trap off
(the float32 cast of a 225-way Dirichlet draw underflows).  ot_edge adds othello roots of one and two legal moves.  Both are
replayed on the host envs (tests/test_edge_fixtures_cpu.py pins that replay, and checks every recorded action legal on the
host rules; here the path is replayed only where the evaluator row depends on the leaf, the `onehot` family); gb_edge stores
a crc of the counts row per simulation where the other fixtures store the root's n row.

Every config runs on two engines fed the same rows: one per launch form, azg_select + azg_backup (one launch per phase) and
azg_backup_select (k_backup_select2: backup k and select k + 1 in one launch, two wavefronts per tree).  Checked: every root's
leaf path at every simulation, the root visit counts after every simulation, the final root children (a / n / q / p / v),
root n and max depth, root_probs at every recorded temperature, root_value, tape counters.  The edge agent (temperature 0 from
the first move: np.argmax ties over visit counts) goes through select / backup / advance (k_play, k_emit_samples) in both forms.

Where the reference raised FloatingPointError (probs at T = 0.01: (counts / n) ** 100 underflows under its
np.seterr(all='raise')), the device returns the untrapped IEEE value of the same expression and that is
what is asserted.  The persistent search launches (azg_search_*) compute their own network, so they cannot take these injected
rows; they reach the same select_tree / backup_path code and stay tied to it through the launch-equals-phase tests."""
import os
import zlib

import numpy as np
import pytest

import edge_eval as ee

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
NAMES = ('c4', 'tm', 'br', 'ot', 'gb')
EDGE_CASES = [(n, c) for n in NAMES + ('gbr',) for c in ee.CONFIGS]      # gbr: the random-prefix roots gb_edge.npz holds under rnd_


@pytest.fixture(scope='module')
def torch_mod():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return torch


def _edge(name):
    return ee.load(G, name)


def _set_roots(eng, name, roots):
    if ee.GAMES[name] in ee.HOST_GAMES:                      # host env games (gobang: 225 unpacked cells, engine.py packs them)
        eng.set_states([g.to_azg_state() for g in roots])
        return
    eng.set_states([(g.cells(), g.player, g.turns, g.s.aux[0]) if name == 'br' else (g.cells(), g.player, g.turns) for g in roots])


def _check_probs(pr, d, cname, ti, t):
    for r in range(len(pr)):
        ref = d[cname + '_probs'][r][ti]
        if d[cname + '_probs_raised'][r][ti]:
            assert np.allclose(pr[r], ee.probs_untrapped(d[cname + '_counts'][r], t), rtol=3e-7, atol=1e-12, equal_nan=True), (r, t)
        elif t in (1.0, 2.0, 0.5, 0.0):
            assert (pr[r] == ref).all(), (r, t)
        else:
            assert np.allclose(pr[r], ref, rtol=3e-7, atol=1e-12), (r, t)


@pytest.mark.parametrize('name,cname', EDGE_CASES)
def test_edge_tree_vs_reference_goldens(torch_mod, name, cname):
    from alphazero_general_amd.engine import DeviceEngine
    torch = torch_mod
    d = _edge(name)
    gid = ee.GAMES[name]
    A, NV = ee.game_sizes(gid)
    cpuct, fpu, nfrac, rtemp, sims = d[cname + '_cfg']
    noise, temp, sims = bool(nfrac > 0), bool(rtemp > 0), int(sims)
    fam, seed = str(d[cname + '_family']), int(d[cname + '_seed'])
    exact = not temp or rtemp in (2.0, 0.5)
    compact = cname + '_counts_crc' in d                     # (gb_edge: a crc of the counts row per simulation)
    roots = ee.roots(d, gid)
    R = len(roots)
    a_of = d[cname + '_a']                                   # root children in list order (fixed from the root's expansion on)
    engs = [DeviceEngine(gid, R, cpuct=float(cpuct), fpu_reduction=float(fpu), root_noise_frac=float(nfrac) if noise else 0.1,
                         root_policy_temp=float(rtemp) if temp else 1.1, add_root_noise=noise, add_root_temp=temp, seed=seed,
                         sims_hint=sims) for _ in range(2)]                   # [0]: select + backup, [1]: backup_select
    try:
        for e in engs:
            _set_roots(e, name, roots)
        engs[1].select(None)
        for s in range(sims):
            engs[0].select(None)
            pol = np.zeros((R, A), np.float32); val = np.zeros((R, NV), np.float32)
            for r in range(R):
                dep = int(d[cname + '_depth'][r, s])
                ref = d[cname + '_paths'][r, s][:dep]
                for e in engs:
                    path = e.last_path(r)
                    assert len(path) == dep and (path == ref).all(), (r, s)
                pol[r], val[r] = ee.leaf_row(fam, seed, roots[r], r, s, ref, A, NV)
                assert ee.row_crc(pol[r], val[r]) == d[cname + '_row_crc'][r, s], (r, s)
            tp, tv = torch.from_numpy(pol).to(engs[0].device), torch.from_numpy(val).to(engs[0].device)
            engs[0].backup(tp, tv)
            if s + 1 < sims:
                engs[1].backup_select(tp, tv, None)
            else:
                engs[1].backup(tp, tv)
            if compact:
                for e in engs:
                    got = e.root_counts().cpu().numpy()
                    assert got.dtype == np.int32 and got.shape == (R, A)
                    assert [zlib.crc32(row.tobytes()) & 0xFFFFFFFF for row in got] == d[cname + '_counts_crc'][:, s].tolist(), s
                continue
            want = np.zeros((R, A), np.int32)
            for r in range(R):
                k = int((a_of[r] >= 0).sum())
                want[r, a_of[r][:k]] = d[cname + '_rootn'][r, s][:k]
            for e in engs:
                assert (e.root_counts().cpu().numpy() == want).all(), s
        for e in engs:
            for r in range(R):
                ch = e.root_children(r)
                k = len(ch['a'])
                assert (ch['a'] == a_of[r][:k]).all() and (a_of[r][k:] == -1).all()
                assert (ch['n'] == d[cname + '_n'][r][:k]).all()
                for f in ('q', 'p', 'v'):
                    if exact:
                        assert (ch[f] == d[cname + '_' + f][r][:k]).all(), (f, r)
                    else:
                        assert np.allclose(ch[f], d[cname + '_' + f][r][:k], atol=1e-5), (f, r)
                info = e.tree_info(r)
                assert info['n'] == d[cname + '_root_n'][r] and info['max_depth'] == d[cname + '_maxdepth'][r], r
            assert (e.root_counts().cpu().numpy() == d[cname + '_counts']).all()
            for ti, t in enumerate(d['prob_temps']):
                _check_probs(e.root_probs(float(t)).cpu().numpy(), d, cname, ti, float(t))
            assert (e.root_value(False).cpu().numpy() == d[cname + '_vmax']).all()
            assert (e.root_value(True).cpu().numpy() == d[cname + '_vavg']).all()
            assert (e.tape_counters() == d[cname + '_ctr']).all()
            e.counters()                                                     # (raises a sticky device error, if any)
    finally:
        for e in engs:
            e.close()


def _zero_temp(cur_temp, turns, const_max_turns):
    return 0


@pytest.mark.parametrize('launch', ['phase', 'fused'])
@pytest.mark.parametrize('name', NAMES)
def test_edge_agent_vs_reference_goldens(torch_mod, name, launch):
    """SelfPlayAgent.run on the engine with the edge agent's rows (uniform priors, draw-heavy values) at temperature 0 from the
    first move, symmetric samples on: counts, moves, games, every sample and result as the reference made them"""
    from alphazero_general_amd.engine import DeviceEngine
    torch = torch_mod
    d = _edge(name)
    gid = ee.GAMES[name]
    B, sims, games, seed = int(d['agent_B']), int(d['agent_sims']), int(d['agent_games']), int(d['agent_seed'])
    eng = DeviceEngine(gid, B, seed=seed, games_per_iteration=games, example_capacity=20000, sims_hint=sims, start_temp=0.0,
                       temp_fn=_zero_temp)
    try:
        A, NV = eng.A, eng.NV
        rec = dict(actions=[], counts=[], games_played=[], sims=[], obs_crc=[])
        step, gp = 0, 0
        obs = eng.new_obs()
        for _ in range(len(d['agent_actions'])):                       # (probFastSim 0: every round is a full search)
            assert gp < games
            rec['sims'].append(sims)
            if launch == 'fused':
                eng.select(obs)
            for s in range(sims):
                if launch == 'phase':
                    eng.select(obs)
                o = obs.cpu().numpy()
                rec['obs_crc'].append([zlib.crc32(np.ascontiguousarray(o[i]).tobytes()) & 0xFFFFFFFF for i in range(B)])
                pol = np.zeros((B, A), np.float32); val = np.zeros((B, NV), np.float32)
                for i in range(B):
                    pol[i], val[i] = ee.agent_row(seed, i, step, A, NV)
                tp, tv = torch.from_numpy(pol).to(eng.device), torch.from_numpy(val).to(eng.device)
                if launch == 'fused' and s + 1 < sims:
                    eng.backup_select(tp, tv, obs)
                else:
                    eng.backup(tp, tv)
                step += 1
            rec['counts'].append(eng.root_counts().cpu().numpy())
            eng.advance(record_history=True)
            rec['actions'].append(eng.last_actions().cpu().numpy())
            gp = eng.counters()['games_played']
            rec['games_played'].append(gp)
        assert gp == games
        assert (np.array(rec['sims']) == d['agent_round_sims']).all()
        assert (np.array(rec['counts']) == d['agent_counts']).all()
        assert (np.array(rec['actions']) == d['agent_actions']).all()
        assert (np.array(rec['games_played']) == d['agent_games_played']).all()
        assert (np.array(rec['obs_crc'], np.uint32) == d['agent_obs_crc']).all()
        o, pi, z = [t.cpu().numpy() for t in eng.examples()]
        want = ee.unpack_obs(d)
        assert o.shape == want.shape
        assert (o == want).all() and (pi == ee.unpack_pi(d)).all() and (z == d['agent_s_z']).all()
        ws, turns, slot = eng.results()
        assert (ws == d['agent_r_ws']).all() and (turns == d['agent_r_turns']).all()
    finally:
        eng.close()
