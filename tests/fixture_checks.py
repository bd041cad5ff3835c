"""One record-and-compare module for the reference fixtures every game shares (tests/golden/<g>_tree.npz, <g>_agent.npz,
<g>_mt19937_agent.npz, <g>_edge.npz; imported by the tests like edge_eval and oracle_lib, not collected by pytest).

RECORDING drives an engine with a fixture's rows and keeps what it did (record_tree, run_agent: they need a GPU); COMPARING holds such a
record to the fixture (compare_tree, compare_agent, compare_mt19937_agent: pure numpy, so tests/test_fixture_checks_cpu.py can show on a
CPU that every comparison bites).  The rules, stated once:

  * a fixture holds a wide field in full (`<cfg>_rootn`, `_counts`, `_probs`, `_s_obs`, `_s_pi`) or as one crc32 per row (`_rootn_crc`,
    ... as hn_* do); the comparison takes whichever key is there, and a record may hold either form too;
  * a key that is there in neither form is a failure, never a skipped check; so is a field the record lacks, or one it has that no
    comparison reads.  The exceptions are the `not_recorded` a game's test names, with the reason;
  * root children q, p, v: exact without root temperature (and at root temperature 2.0 / 0.5 in the edge fixtures, powers numpy takes
    exactly); under root temperature within np.allclose(atol=1e-5) -- or, for a tier with `p_ulps` (hnefatafl), q and v exact and p within
    that many ulps;
  * root_probs: exact at the temperatures where numpy's power is exact (1, 0.5, 0; 2.0 too in the edge fixtures), rtol 3e-7 / atol 1e-12
    elsewhere -- float32 powf, within an ulp but not correctly rounded.  A CRC cannot carry a tolerance: a fixture that holds probs as
    CRCs is compared at the exact temperatures only.  Where the reference raised (edge fixtures, `_probs_raised`) the device returns the
    untrapped IEEE value of the same expression (edge_eval.probs_untrapped);
  * everything else -- paths, depths, counts, actions, samples, results, values, tape counters -- is equality.

The shared default is the strictest form the fixtures carry: every root's path at every simulation, every prob_temps column, both
per-phase launch forms, the tape counters of an mt19937 replay.  A weaker form is a named argument at the call, with its reason.

Every assert carries (game / fixture, config, field, row, simulation or round, ...): this module gets no assertion rewriting."""
import functools
import os
import zlib

import numpy as np

import edge_eval as ee
import oracle_lib as ol

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
LAUNCHES = ['phase', 'fused']                                # azg_select + azg_backup | azg_backup_select (backup k and select k + 1 in one launch)

# what a tier of fixtures can be held to.  exact_root_temps: the root temperatures (cfg[3]; 0: off, the tree fixtures keep a flag there)
# under which the root children's q / p / v are exact; rootn: the per-simulation root counts row is indexed by action or by child in list
# order; rootn_crc, rootn_crc_dtype: the key that holds those rows as crcs (gb_edge calls it `_counts_crc`, [R, sims]; hn_tree's
# `_counts_crc` is the final counts', [R]) and what a row was cast to before its crc was taken; raised: the fixture marks the probs the
# reference raised at; has_k: it holds the root's child count (where it keeps fewer children than a root can have)
TREE = dict(exact_root_temps=(0.0,), exact_temps=(1.0, 0.5, 0.0), rootn='action', rootn_crc='rootn_crc', rootn_crc_dtype=np.int16,
            p_ulps=None, raised=False, has_k=False)
EDGE = dict(TREE, exact_root_temps=(0.0, 2.0, 0.5), exact_temps=(1.0, 2.0, 0.5, 0.0), rootn='child', rootn_crc='counts_crc',
            rootn_crc_dtype=np.int32, raised=True)

SEARCHED = ('counts', 'probs', 'vavg', 'vmax')               # assert_engines_equal: after a move's search,
PLAYED = ('actions',)                                        # after advance,
FINISHED = ('tapes', 'counters', 'examples', 'results')      # and at the end


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


def crc_rows(a):
    """one crc per row (last axis) of a"""
    a = np.ascontiguousarray(a)
    return np.array([crc(r) for r in a.reshape(-1, a.shape[-1])], np.uint32).reshape(a.shape[:-1])


@functools.lru_cache(maxsize=None)
def load(name):
    """the arrays of tests/golden/<name>.npz, read once (NpzFile decompresses an array on EVERY d[key]): shared, never written to.
    '<g>_edge' of the games of edge_eval.GAMES comes unstacked as edge_eval.load gives it"""
    if name.endswith('_edge') and name[:-5] in ee.GAMES:
        return ee.load(G, name[:-5])
    return dict(np.load(os.path.join(G, name + '.npz')))


def states_from_prefix(Game, prefix):
    """the host env's states after each row of opening moves (-1: padding)"""
    out = []
    for row in prefix:
        g = Game()
        for a in row:
            if a >= 0:
                g.play_action(int(a))
        out.append(g.to_azg_state())
    return out


def oracle_states_from_prefix(game, prefix):
    """the same on the C oracle's rules, for the games that have them (connect4, brandubh, the 3-player env)"""
    out = []
    for row in prefix:
        g = ol.OGame(game)
        for a in row:
            if a >= 0:
                g.play(a)
        out.append(ee.root_state(g) if game == ol.GAME_BRANDUBH else (g.cells(), g.player, g.turns))
    return out


def fake_rows(seed, slots, step, A, NV):
    """the goldens' stand-in network: one oracle_lib.fake_eval row per slot"""
    pol = np.zeros((len(slots), A), np.float32); val = np.zeros((len(slots), NV), np.float32)
    for r, s in enumerate(slots):
        pol[r], val[r] = ol.fake_eval(seed, int(s), step, A, NV)
    return pol, val


def _to_device(eng, rows):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(eng.device) for x in rows]


def sim_step(eng, launch, s, sims, pol, val, obs):
    """simulation s's backup (and, fused, simulation s + 1's select); simulation 0's select is the caller's"""
    if launch == 'fused' and s + 1 < sims:
        eng.backup_select(pol, val, obs)
    else:
        eng.backup(pol, val)
        if launch == 'phase' and s + 1 < sims:
            eng.select(obs)


# ------------------------------------------------------------------------------------------------------------------------- comparing
def _same(got, want, where):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, where + ('shape', got.shape, want.shape)
    bad = np.argwhere(np.atleast_1d(got != want))
    assert len(bad) == 0, where + ('first of %d at' % len(bad), tuple(bad[0]) if len(bad) else ())


def _close(got, want, where, **tol):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, where + ('shape', got.shape, want.shape)
    bad = np.argwhere(np.atleast_1d(~np.isclose(got, want, **tol)))
    assert len(bad) == 0, where + (tol, 'first of %d at' % len(bad), tuple(bad[0]) if len(bad) else ())


def _has(rec, key, where):
    assert key in rec, where + (key, 'missing from the record')
    return rec[key]


def _fixture(d, prefix, key, where):
    """('full' | 'crc', array) of one wide fixture field"""
    if prefix + key in d:
        return 'full', d[prefix + key]
    if prefix + key + '_crc' in d:
        return 'crc', d[prefix + key + '_crc']
    if prefix == 'agent_' and key == 's_obs' and 'agent_s_obs_bits' in d:
        return 'full', ee.unpack_obs(d)                      # (gb_edge keeps its samples packed: edge_eval.pack_obs / pack_pi)
    if prefix == 'agent_' and key == 's_pi' and 'agent_s_pi_nnz' in d:
        return 'full', ee.unpack_pi(d)
    raise AssertionError(where + (prefix + key, 'in the fixture neither in full nor as _crc'))


def _recorded(rec, key, form, where, rows=lambda a: a):
    """the record's field in the fixture's form; rows: the full array as the rows whose crcs the fixture holds"""
    if form == 'full':
        return _has(rec, key, where)
    if key + '_crc' in rec:
        return rec[key + '_crc']
    return crc_rows(rows(np.asarray(_has(rec, key, where))))


def _wide(rec, d, prefix, key, where, rows=lambda a: a, pick=lambda a: a):
    """one wide field, record against fixture, in the form the fixture holds; pick: the part of both that is compared"""
    form, want = _fixture(d, prefix, key, where)
    _same(pick(np.asarray(_recorded(rec, key, form, where, rows))), pick(want), where + (key, form))
    return form


def _no_strays(rec, known, where):
    stray = sorted(set(rec) - set(known) - {k + '_crc' for k in known})
    assert not stray, where + ('fields no comparison reads', stray)


def _check_probs(got, form, want, temps, d, pre, tier, where):
    """root_probs [R, T, A] (crc form: [R, T]) at every recorded temperature, by the rules of the module docstring"""
    got = np.asarray(got)
    assert got.shape == want.shape, where + ('probs', 'shape', got.shape, want.shape)
    for ti, t in enumerate(temps):
        t = float(t)
        for r in range(len(want)):
            w = where + ('probs', 'root', r, 'temperature', t)
            if tier['raised'] and d[pre + 'probs_raised'][r][ti]:
                _close(got[r, ti], ee.probs_untrapped(d[pre + 'counts'][r], t), w + ('untrapped',), rtol=3e-7, atol=1e-12, equal_nan=True)
            elif t in tier['exact_temps']:
                _same(got[r, ti], want[r, ti], w + (form,))
            elif form == 'full':
                _close(got[r, ti], want[r, ti], w, rtol=3e-7, atol=1e-12)


TREE_FIELDS = ('paths', 'rootn', 'a', 'n', 'q', 'p', 'v', 'root_n', 'maxdepth', 'counts', 'probs', 'vmax', 'vavg', 'ctr')


def compare_tree(trace, d, cname, tier, game='', prob_temps=None):
    """one engine's record_tree trace against config `cname` of a tree or edge fixture (prob_temps: for a fixture that does not hold the
    temperatures of its probs columns itself)"""
    pre = cname + '_'
    where = (game, cname, trace.get('launch', ''))
    d = d if prob_temps is None else dict(d, prob_temps=np.asarray(prob_temps, np.float32))
    _no_strays(trace, TREE_FIELDS + ('launch',), where)
    for k in ('cfg', 'depth', 'paths', 'a', 'n', 'q', 'p', 'v', 'root_n', 'maxdepth', 'vmax', 'vavg', 'ctr') + \
            ('probs_raised', 'counts') * tier['raised'] + ('k',) * tier['has_k']:
        assert pre + k in d, where + (pre + k, 'missing from the fixture')
    assert 'prob_temps' in d, where + ('prob_temps', 'missing from the fixture')
    depth, ref_paths, a_of = d[pre + 'depth'], d[pre + 'paths'], d[pre + 'a']
    R, sims = depth.shape
    assert int(d[pre + 'cfg'][4]) == sims, where + ('cfg', 'sims')
    # every recorded leaf path: its length, and its actions as far as the fixture keeps them
    paths = _has(trace, 'paths', where)
    assert len(paths) == sims and all(len(p) == R for p in paths), where + ('paths', 'shape')
    assert any(p is not None for row in paths for p in row), where + ('paths', 'none recorded')
    for s in range(sims):
        for r in range(R):
            path = paths[s][r]
            if path is None:                                 # (a declared path_stride)
                continue
            assert len(path) == depth[r, s], where + ('depth', 'root', r, 'sim', s, len(path), int(depth[r, s]))
            keep = ref_paths.shape[-1]
            assert (np.asarray(path[:keep]) == ref_paths[r, s][:len(path)]).all(), where + ('paths', 'root', r, 'sim', s)
    # the root's visit counts after every simulation
    if pre + 'rootn' not in d:                               # ([R, sims] crcs of the counts rows)
        assert pre + tier['rootn_crc'] in d, where + (pre + 'rootn', 'in the fixture neither in full nor as _' + tier['rootn_crc'])
        got = _recorded(trace, 'rootn', 'crc', where, lambda x: x.astype(tier['rootn_crc_dtype']))
        _same(got, d[pre + tier['rootn_crc']], where + ('rootn', 'crc', 'root, sim'))
    else:
        want = d[pre + 'rootn']
        got = np.asarray(_has(trace, 'rootn', where))
        if tier['rootn'] == 'child':                         # (the fixture's row is n of the root's children in list order)
            byaction = np.zeros(got.shape, np.int32)
            for r in range(R):
                k = int((a_of[r] >= 0).sum())
                byaction[r][:, a_of[r][:k]] = want[r][:, :k]
            want = byaction
        _same(got, want, where + ('rootn', 'root, sim, action'))
    # the root's children at the end, in list order (the fixture may keep the first kmax of them only)
    exact = float(d[pre + 'cfg'][3]) in tier['exact_root_temps']
    ch = {f: _has(trace, f, where) for f in ('a', 'n', 'q', 'p', 'v')}
    assert all(len(ch[f]) == R for f in ch), where + ('root children', 'rows')
    for r in range(R):
        k = len(ch['a'][r])
        kk = min(k, a_of.shape[1])
        if tier['has_k']:
            assert k == d[pre + 'k'][r], where + ('k', 'root', r, k)
        assert all(len(ch[f][r]) == k for f in ch), where + ('root children', 'root', r, 'lengths')
        assert (a_of[r][kk:] == -1).all(), where + ('a', 'root', r, 'the fixture has more children')
        _same(ch['a'][r][:kk], a_of[r][:kk], where + ('a', 'root', r))
        _same(ch['n'][r][:kk], d[pre + 'n'][r][:kk], where + ('n', 'root', r))
        for f in ('q', 'p', 'v'):
            got, want = np.asarray(ch[f][r][:kk]), d[pre + f][r][:kk]
            if exact or (tier['p_ulps'] and f != 'p'):
                _same(got, want, where + (f, 'root', r))
            elif tier['p_ulps']:
                ok = np.abs(got.astype(np.float64) - want) <= tier['p_ulps'] * np.spacing(np.maximum(got, want))
                assert got.shape == want.shape and ok.all(), where + (f, 'root', r, 'ulps', tier['p_ulps'])
            else:
                assert got.shape == want.shape and np.allclose(got, want, atol=1e-5), where + (f, 'root', r, 'atol 1e-5')
    _same(_has(trace, 'root_n', where), d[pre + 'root_n'], where + ('root_n',))
    _same(_has(trace, 'maxdepth', where), d[pre + 'maxdepth'], where + ('maxdepth',))
    _wide(trace, d, pre, 'counts', where)
    form, want = _fixture(d, pre, 'probs', where)
    _check_probs(_recorded(trace, 'probs', form, where), form, want, d['prob_temps'], d, pre, tier, where)
    _same(_has(trace, 'vmax', where), d[pre + 'vmax'], where + ('vmax',))
    _same(_has(trace, 'vavg', where), d[pre + 'vavg'], where + ('vavg',))
    _same(_has(trace, 'ctr', where), d[pre + 'ctr'], where + ('ctr',))


AGENT_FIELDS = ('round_sims', 'counts', 'actions', 'games_played', 'obs_crc', 's_obs', 's_pi', 's_z', 'r_ws', 'r_turns')


def compare_agent(rec, d, prefix, game='', not_recorded=()):
    """a run_agent record against `<prefix>*` of an agent fixture ('plain_', 'agent_'); not_recorded: the fields this fixture does not
    hold, named (with the reason) by the test that passes them"""
    where = (game, prefix)
    _no_strays(rec, AGENT_FIELDS + ('ctr',), where)
    B = np.asarray(_has(rec, 'actions', where)).shape[-1]
    for key in ('round_sims', 'actions', 'games_played', 's_z', 'r_ws', 'r_turns'):
        if key not in not_recorded:
            assert prefix + key in d, where + (prefix + key, 'missing from the fixture')
            _same(_has(rec, key, where), d[prefix + key], where + (key,))
    _wide(rec, d, prefix, 'counts', where + ('round, slot',))
    if 'obs_crc' not in not_recorded:                         # one row per evaluated simulation (none in a warm-up round)
        assert prefix + 'obs_crc' in d, where + (prefix + 'obs_crc', 'missing from the fixture')
        _same(np.asarray(_has(rec, 'obs_crc', where), np.uint32).reshape(-1, B), d[prefix + 'obs_crc'].reshape(-1, B), where + ('obs_crc', 'step, slot'))
    n = len(d[prefix + 's_z'])
    _wide(rec, d, prefix, 's_obs', where + ('sample',), rows=lambda x: x.reshape(n, -1))
    _wide(rec, d, prefix, 's_pi', where + ('sample',))


def compare_mt19937_agent(rec, d, game=''):
    """a run_agent record against a whole reference agent under np.random.seed(s) (<g>_mt19937_agent.npz: no prefix; every round a full
    search, so `sims` stands for round_sims; the observations were not recorded), and the engine's tape counters at the end against the
    end of each slot's recorded draws: call_order rows are (kind, slot, n) -- a shuffle (kind 0) takes n ranks, every other draw one"""
    where = (game, 'mt19937')
    for k in ('sims', 'B', 'call_order'):
        assert k in d, where + (k, 'missing from the fixture')
    compare_agent({k: v for k, v in rec.items() if k != 'obs_crc'}, d, '', game, not_recorded=('round_sims', 'obs_crc'))
    _same(_has(rec, 'round_sims', where), np.full(len(d['actions']), int(d['sims'])), where + ('round_sims',))
    co = d['call_order']
    used = [int(co[(co[:, 1] == sl) & (co[:, 0] == 0), 2].sum() + ((co[:, 1] == sl) & (co[:, 0] > 0)).sum()) for sl in range(int(d['B']))]
    _same(_has(rec, 'ctr', where), np.array(used, np.uint64), where + ('ctr', 'slot'))


# ------------------------------------------------------------------------------------------------------------------------- recording
def tree_engines(gid, d, cname, tier, launches=LAUNCHES, **kw):
    """one engine per launch form with config `cname`'s search constants: cfg = (cpuct, fpu_reduction, noise, root temperature, sims) --
    flags in the tree fixtures, the noise fraction and the temperature themselves (0: off) in the edge fixtures"""
    from alphazero_general_amd.engine import DeviceEngine
    cpuct, fpu, noise, temp, sims = [float(x) for x in d[cname + '_cfg']]
    if tier['rootn'] == 'child':
        kw = dict(dict(root_noise_frac=noise if noise > 0 else 0.1, root_policy_temp=temp if temp > 0 else 1.1), **kw)
    R = len(d['prefix'] if 'prefix' in d else d['player'])
    return [DeviceEngine(gid, R, **dict(dict(cpuct=cpuct, fpu_reduction=fpu, add_root_noise=noise > 0, add_root_temp=temp > 0,
                                             seed=int(d[cname + '_seed']), sims_hint=int(sims)), **kw)) for _ in launches]


def check_tree(gid, d, cname, states, tier=TREE, game='', rows=None, launches=LAUNCHES, path_stride=1, obs=True, prob_temps=None, **kw):
    """config `cname` of a tree or edge fixture from the roots `states` on one engine per launch form (kw: further engine arguments):
    record_tree, then compare_tree of every trace.  Returns the traces"""
    engs = tree_engines(gid, d, cname, tier, launches, **kw)
    try:
        for e in engs:
            e.set_states(states)
        traces = record_tree(engs, d, cname, rows, launches, path_stride, obs, prob_temps)
    finally:
        for e in engs:
            e.close()
    for t in traces:
        compare_tree(t, d, cname, tier, game, prob_temps)
    return traces


def record_tree(engs, d, cname, rows=None, launches=LAUNCHES, path_stride=1, obs=True, prob_temps=None):
    """drive one engine per launch form (their roots set, nothing selected yet) through config `cname`'s simulations in step, feeding
    rows(s) -> (policy [R, A], value [R, NV]) (default: the goldens' fake_eval rows under the config's seed), and return one trace per
    engine.  path_stride: read the leaf path of every path_stride-th root only -- a weaker form, for the test to name with its reason"""
    sims, seed = int(d[cname + '_cfg'][4]), int(d[cname + '_seed'])
    prob_temps = d['prob_temps'] if prob_temps is None else prob_temps
    R, A, NV = engs[0].B, engs[0].A, engs[0].NV
    rows = rows or (lambda s: fake_rows(seed, range(R), s, A, NV))
    assert len(engs) == len(launches)
    buf = [e.new_obs() if obs else None for e in engs]
    traces = [dict(launch=l, paths=[], rootn=[]) for l in launches]
    for e, o in zip(engs, buf):
        e.select(o)
    for s in range(sims):
        for e, t in zip(engs, traces):
            t['paths'].append([e.last_path(r) if r % path_stride == 0 else None for r in range(R)])
        if obs:
            assert all((buf[0] == o).all() for o in buf[1:]), (cname, 'leaf observations differ between the launch forms', 'sim', s)
        pol, val = rows(s)
        for e, o, t in zip(engs, buf, traces):
            sim_step(e, t['launch'], s, sims, *_to_device(e, (pol, val)), o)
            t['rootn'].append(e.root_counts().cpu().numpy())
    for e, t in zip(engs, traces):
        t['rootn'] = np.stack(t['rootn'], axis=1)
        ch = [e.root_children(r) for r in range(R)]
        for f in ('a', 'n', 'q', 'p', 'v'):
            t[f] = [c[f] for c in ch]
        info = [e.tree_info(r) for r in range(R)]
        t['root_n'] = np.array([i['n'] for i in info])
        t['maxdepth'] = np.array([i['max_depth'] for i in info])
        t['counts'] = e.root_counts().cpu().numpy()
        t['probs'] = np.stack([e.root_probs(float(x)).cpu().numpy() for x in prob_temps], axis=1)
        t['vmax'], t['vavg'] = e.root_value(False).cpu().numpy(), e.root_value(True).cpu().numpy()
        t['ctr'] = e.tape_counters()
        e.counters()                                         # (raises a sticky device error, if any)
    return traces


def run_agent(eng, seed, slot_base, sims, games, launch='phase', rows=None, prob_fast=0.0, fast_sims=20, warmup=False, warmup_sims=5,
              max_rounds=500):
    """SelfPlayAgent.run (SelfPlayAgent.pyx:79-101) on the engine: rounds of `sims` simulations (fast_sims in a fast round, drawn as the
    reference draws it; warmup_sims of uniform rows without observations in a warm-up) and a move, until `games` games are done.
    launch 'phase': generateBatch / processBatch as azg_select / azg_backup; 'fused': backup k and select k + 1 share a launch
    (azg_backup_select), the form every runner uses; 'raw' (warm-up only): a round is ONE azg_search_raw launch.  rows(step) -> (policy
    [B, A], value [B, NV]); default: the goldens' fake_eval rows of slots slot_base ..  The record holds every field compare_agent reads"""
    from alphazero_general_amd import _abi
    from alphazero_general_amd.utils import AGENT_STREAM
    L = _abi.lib()
    B, A, NV = eng.B, eng.A, eng.NV
    assert launch in LAUNCHES or (launch == 'raw' and warmup), launch
    rows = rows or (lambda step: fake_rows(seed, [slot_base + i for i in range(B)], step, A, NV))
    rec = dict(round_sims=[], counts=[], actions=[], games_played=[], obs_crc=[])
    obs = None if warmup else eng.new_obs()
    uniform = _to_device(eng, (np.full((B, A), 1 / A), np.full((B, NV), 1 / NV)))
    step, gp = 0, 0
    for actr in range(max_rounds):
        if gp >= games:
            break
        fast = L.azg_tape_uniform(seed, AGENT_STREAM + slot_base, actr) < prob_fast
        ns = fast_sims if fast else (warmup_sims if warmup else sims)
        rec['round_sims'].append(ns)
        if launch == 'raw':
            eng.search_raw(ns, float(np.float32(1 / A)), np.full(NV, 1 / NV, np.float32))
        else:
            eng.select(obs)
            for s in range(ns):
                if warmup:
                    pol, val = uniform
                else:
                    rec['obs_crc'].append(crc_rows(obs.cpu().numpy().reshape(B, -1)))
                    pol, val = _to_device(eng, rows(step))
                sim_step(eng, launch, s, ns, pol, val, obs)
                step += 1
        rec['counts'].append(eng.root_counts().cpu().numpy())
        eng.advance(record_history=not fast)
        rec['actions'].append(eng.last_actions().cpu().numpy())
        gp = eng.counters()['games_played']
        rec['games_played'].append(gp)
    rec = {k: np.array(v) for k, v in rec.items()}
    rec['s_obs'], rec['s_pi'], rec['s_z'] = [t.cpu().numpy() for t in eng.examples()]
    rec['r_ws'], rec['r_turns'], _ = eng.results()
    rec['ctr'] = eng.tape_counters()
    return rec


def check_agent(gid, d, prefix, launch, game='', rows=None, engine_kw={}, before=None, **rnd):
    """`<prefix>*` of an agent fixture: an engine with the fixture's B, seed, slot_base, games and sims (engine_kw: the rest; before(eng):
    what a game checks on the fresh engine), run_agent (rnd: its round arguments), compare_agent.  Returns the record"""
    from alphazero_general_amd.engine import DeviceEngine
    B, sims, games, seed = [int(d[prefix + k]) for k in ('B', 'sims', 'games', 'seed')]
    slot_base = int(d[prefix + 'slot_base'])
    eng = DeviceEngine(gid, B, **dict(dict(seed=seed, slot_base=slot_base, games_per_iteration=games, sims_hint=sims), **engine_kw))
    try:
        if before is not None:
            before(eng)
        rec = run_agent(eng, seed, slot_base, sims, games, launch, rows, **rnd)
    finally:
        eng.close()
    compare_agent(rec, d, prefix, game)
    return rec


def check_mt19937_agent(gid, d, launch, game=''):
    """A whole SelfPlayAgent under np.random.seed(s), move for move: <g>_mt19937_agent.npz is the REFERENCE's agent -- root noise and root
    temperature on -- on numpy's own MT19937 stream with shuffle / dirichlet / choice observed per game slot (tests/test_oracle_golden.py
    re-derives every draw from the seed alone).  The engine replays all three (azg_set_random_tape) and must reproduce the counts and the
    sampled action of every slot in every round, the games_played trajectory, the samples incl. symmetries and the results in queue
    order, and end with its tape counters at the end of each slot's recorded draws"""
    from alphazero_general_amd.engine import DeviceEngine
    cpuct, fpu, nfrac, rtemp = [float(x) for x in d['cfg']]
    eng = DeviceEngine(gid, int(d['B']), cpuct=cpuct, fpu_reduction=fpu, root_noise_frac=nfrac, root_policy_temp=rtemp, add_root_noise=True,
                       add_root_temp=True, seed=987654321, games_per_iteration=int(d['games']), example_capacity=4096, sims_hint=int(d['sims']))
    try:
        eng.set_random_tape(d['tape_ranks'], d['tape_u'], d['tape_noise_off'], d['tape_noise_pool'])
        rec = run_agent(eng, int(d['eval_seed']), 0, int(d['sims']), int(d['games']), launch)
        eng.set_shuffle_tape(None)
    finally:
        eng.close()
    compare_mt19937_agent(rec, d, game)


# ------------------------------------------------------------------------------------------------------------------------- other checks
def check_mcts_class(Game, d, A, NV, pickle_at=None, search=False, tier=TREE, game=''):
    """alphazero_general_amd.MCTS on a host env object (one slot: the tape stream of the tree fixture's root 0) fed config `default`'s
    evaluations must build the reference's tree: the depth of every simulation, then counts, both values, max depth and probs at every
    recorded temperature.  search: through MCTS.search with a callable network, not find_leaf / process_results; pickle_at: the object
    is pickled and restored before that simulation.  Returns (mcts, game object) for what a game checks on top"""
    import pickle
    from alphazero_general_amd.MCTS import MCTS
    from alphazero_general_amd.utils import dotdict
    where = (game, 'MCTS class')
    cpuct, fpu, _, _, sims = d['default_cfg']
    seed, sims = int(d['default_seed']), int(sims)
    g = Game.from_azg_state(*states_from_prefix(Game, d['prefix'][:1])[0])
    m = MCTS(dotdict(cpuct=float(cpuct), fpu_reduction=float(fpu), root_noise_frac=0.1, root_policy_temp=1.1, min_discount=1, _num_players=3,
                     numMCTSSims=sims, _azg_seed=seed))
    if search:
        calls = []

        def nn(o):
            assert o.shape == tuple(Game.observation_size()), where + ('observation', o.shape)
            calls.append(1)
            return ol.fake_eval(seed, 0, len(calls) - 1, A, NV)
        m.search(g, nn, sims, False, False)
        assert len(calls) == sims, where + ('network calls', len(calls))
    else:
        for s in range(sims):
            if s == pickle_at:
                m = pickle.loads(pickle.dumps(m))
            leaf = m.find_leaf(g)
            assert m.depth == d['default_depth'][0, s] and type(leaf) is Game, where + ('depth', 'sim', s, m.depth)
            p, v = ol.fake_eval(seed, 0, s, A, NV)
            m.process_results(leaf, v, p, False, False)
    got = dict(counts=np.asarray(m.counts(g)).astype(np.int32)[None],
               probs=np.array([np.asarray(m.probs(g, float(t)), np.float32) for t in d['prob_temps']])[None])
    form, want = _fixture(d, 'default_', 'counts', where)
    _same(_recorded(got, 'counts', form, where), want[:1], where + ('counts', form))
    form, want = _fixture(d, 'default_', 'probs', where)
    _check_probs(_recorded(got, 'probs', form, where), form, want[:1], d['prob_temps'], d, 'default_', tier, where)
    assert m.value(False) == d['default_vmax'][0] and m.value(True) == d['default_vavg'][0], where + ('values', m.value(False), m.value(True))
    assert m.max_depth == d['default_maxdepth'][0], where + ('max_depth', m.max_depth)
    return m, g


def phase_loop(ec, evaluate, sims, obs):
    """the per-phase side of a launch-equals-loop test: sims x [select, evaluate(ec, obs) -> (policy, value), backup]"""
    for _ in range(sims):
        ec.select(obs)
        p, v = evaluate(ec, obs)
        ec.backup(p.contiguous(), v.contiguous())


def twin_moves(gid, B, search, evaluate, sims, moves, states=None, searched=SEARCHED, finished=FINISHED, each_move=None, **kw):
    """`moves` moves of search(ea) -- a persistent launch -- against phase_loop(ec, evaluate) on a twin engine with the same seeds (kw: the
    engines' arguments), from `states` if given: `searched` after every search, the moves after every advance, `finished` at the end.
    each_move(ea, ec, mv): what a test looks at besides, before the move is played.  Returns the two engines' counters (equal if
    `finished` says so)"""
    import torch
    from alphazero_general_amd.engine import DeviceEngine
    kw = dict(dict(games_per_iteration=1 << 30, example_capacity=B * (moves + 1) * 8, sims_hint=sims), **kw)
    ea, ec = DeviceEngine(gid, B, **kw), DeviceEngine(gid, B, **kw)
    try:
        if states is not None:
            ea.set_states(states); ec.set_states(states)
        oc = ec.new_obs(torch.float32)
        for mv in range(moves):
            search(ea)
            phase_loop(ec, evaluate, sims, oc)
            assert_engines_equal(ea, ec, searched, 'move', mv)
            if each_move is not None:
                each_move(ea, ec, mv)
            ea.advance(True); ec.advance(True)
            assert_engines_equal(ea, ec, PLAYED, 'move', mv)
        assert_engines_equal(ea, ec, finished, 'end')
        return ea.counters(), ec.counters()
    finally:
        ea.close(); ec.close()


def assert_engines_equal(ea, ec, what, *where):
    """twin engines (a persistent launch on one, the per-phase loop on the other) hold the same, bit for bit: `what` names the
    comparisons -- SEARCHED after a move's search, PLAYED after advance, FINISHED at the end, or a subset the test gives a reason for"""
    import torch
    unknown = set(what) - set(SEARCHED + PLAYED + FINISHED)
    assert not unknown, where + ('unknown comparisons', sorted(unknown))
    tensors = dict(counts=lambda e: e.root_counts(), probs=lambda e: e.root_probs(1.0), vavg=lambda e: e.root_value(True),
                   vmax=lambda e: e.root_value(False), actions=lambda e: e.last_actions())
    for k in what:
        if k in tensors:
            assert torch.equal(tensors[k](ea), tensors[k](ec)), where + (k,)
    if 'tapes' in what:
        assert (ea.tape_counters() == ec.tape_counters()).all(), where + ('tapes',)
    if 'counters' in what:
        ca, cc = ea.counters(), ec.counters()
        assert ca == cc, where + ('counters', ca, cc)
    if 'examples' in what:
        for i, (t, u) in enumerate(zip(ea.examples(), ec.examples())):
            assert torch.equal(t, u), where + ('examples', ('obs', 'pi', 'z')[i])
    if 'results' in what:
        for i, (t, u) in enumerate(zip(ea.results(), ec.results())):
            assert (t == u).all(), where + ('results', ('ws', 'turns', 'slot')[i])
