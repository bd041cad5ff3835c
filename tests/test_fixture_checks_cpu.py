"""The comparisons of tests/fixture_checks.py bite (no GPU: they are pure numpy).  On the smallest fixtures -- tt_tree `default` (8 roots x
30 simulations; `noise_temp` for the root-temperature tier), tt_agent `plain`, tt_mt19937_agent, and hn_tree `default` for the CRC form
(6 roots x 40 simulations) -- a record built from the fixture itself passes; one altered entry in any field a comparison reads fails it;
so does a fixture with any one key deleted, a record with a field missing, and a record with a field nothing reads.  The tolerances are
pinned where they are: 4 float32 ulps are caught in the exact tier and at probs in the powf tier (rtol 3e-7 is under 3 ulps); under root
temperature a q off by 2e-5 is caught and one off by 1e-6 is not.  The exceptions the game files declare are pinned by name."""
import copy
import glob
import inspect
import os
import re

import numpy as np
import pytest

import fixture_checks as FC
import test_gpu_hnefatafl as HN

HERE = os.path.dirname(os.path.abspath(__file__))


def tree_record(d, cname):
    """what record_tree would return of an engine that did exactly what the fixture holds (wide fields in the fixture's form; a path the
    fixture keeps the head of is padded to its depth)"""
    pre = cname + '_'
    R, sims = d[pre + 'depth'].shape
    keep = d[pre + 'paths'].shape[-1]
    rec = dict(launch='fixture')
    rec['paths'] = [[np.concatenate([d[pre + 'paths'][r, s][:min(int(d[pre + 'depth'][r, s]), keep)],
                                     np.zeros(max(int(d[pre + 'depth'][r, s]) - keep, 0), np.int16)]) for r in range(R)] for s in range(sims)]
    k = (d[pre + 'a'] >= 0).sum(1)
    for f in ('a', 'n', 'q', 'p', 'v'):
        rec[f] = [d[pre + f][r][:k[r]].copy() for r in range(R)]
    for f in ('root_n', 'maxdepth', 'vmax', 'vavg', 'ctr'):
        rec[f] = d[pre + f].copy()
    for f in ('rootn', 'counts', 'probs'):
        key = f if pre + f in d else f + '_crc'
        rec[key] = d[pre + key].copy()
    return rec


def agent_record(d, prefix):
    return {k: d[prefix + k].copy() for k in FC.AGENT_FIELDS if prefix + k in d}


def ulps(x, n=4):
    x = np.float32(x)
    return np.float32(x + n * np.spacing(x))


def fails(compare, *a, **kw):
    with pytest.raises(AssertionError):
        compare(*a, **kw)


def first_leaf(d, pre):
    """(root, simulation) of a path with an action in it"""
    r, s = np.argwhere(d[pre + 'depth'] > 0)[0]
    return int(r), int(s)


# ------------------------------------------------------------------------------------------------------------------------- tree
TREES = [('tt_tree', 'default', FC.TREE), ('hn_tree', 'default', HN.HN_TREE)]


def tree_alterations(d, cname):
    """{field: function altering one entry of a record in place}"""
    pre = cname + '_'
    r, s = first_leaf(d, pre)
    full = pre + 'rootn' in d
    a0 = int(np.argmax(d[pre + 'counts'][0])) if full else 0

    def entry(f, delta=1):
        def alter(rec):
            rec[f][1] = rec[f][1] + delta
        return alter

    def child(f, exact_step):
        def alter(rec):
            rec[f][0][0] = exact_step(rec[f][0][0])
        return alter

    def path(rec):
        rec['paths'][s][r] = rec['paths'][s][r].copy()
        rec['paths'][s][r][0] += 1

    def depth(rec):
        rec['paths'][s][r] = np.append(rec['paths'][s][r], 0)

    def wide(f, idx, step):
        def alter(rec):
            if f in rec:
                rec[f][idx] = step(rec[f][idx])
            else:
                rec[f + '_crc'][idx[:-1]] ^= 1
        return alter
    alts = dict(paths=path, depth=depth, rootn=wide('rootn', (0, 3, a0), lambda x: x + 1), a=child('a', lambda x: x + 1),
                n=child('n', lambda x: x + 1), q=child('q', ulps), p=child('p', ulps), v=child('v', ulps),
                counts=wide('counts', (0, a0), lambda x: x + 1), probs_exact=wide('probs', (0, 0, a0), ulps),
                vmax=entry('vmax', 1e-7), vavg=entry('vavg', 1e-7), root_n=entry('root_n'), maxdepth=entry('maxdepth'), ctr=entry('ctr'))
    if full:
        alts['probs_powf'] = wide('probs', (0, 2, a0), ulps)
    return alts


@pytest.mark.parametrize('name,cname,tier', TREES, ids=[t[0] for t in TREES])
def test_compare_tree_passes_on_the_fixture_and_bites_everywhere(name, cname, tier):
    d = FC.load(name)
    pre = cname + '_'
    assert d[pre + 'depth'].shape == ((8, 30) if name == 'tt_tree' else (6, 40)) and float(d[pre + 'cfg'][3]) == 0.0
    rec = tree_record(d, cname)
    assert (pre + 'rootn_crc' in d) == (name == 'hn_tree') and set(rec) - {'launch'} in (set(FC.TREE_FIELDS), {f + '_crc' if f in ('rootn', 'counts', 'probs') else f for f in FC.TREE_FIELDS})
    FC.compare_tree(rec, d, cname, tier, name)
    for field, alter in tree_alterations(d, cname).items():
        bad = copy.deepcopy(rec)
        alter(bad)
        with pytest.raises(AssertionError) as ei:
            FC.compare_tree(bad, d, cname, tier, name)
        assert field.split('_')[0] in [str(x) for x in ei.value.args[0]] or field == 'root_n', (field, ei.value.args)
        assert ei.value.args[0][:2] == (name, cname), ei.value.args                             # game and config lead every message
    read = [pre + k for k in ('cfg', 'depth', 'paths', 'a', 'n', 'q', 'p', 'v', 'vmax', 'vavg', 'root_n', 'maxdepth', 'ctr')] + ['prob_temps'] + \
           [pre + f + ('' if pre + f in d else '_crc') for f in ('rootn', 'counts', 'probs')]
    for key in read:
        fails(FC.compare_tree, rec, {k: v for k, v in d.items() if k != key}, cname, tier, name)
    for f in set(rec) - {'launch'}:
        fails(FC.compare_tree, {k: v for k, v in rec.items() if k != f}, d, cname, tier, name)
    fails(FC.compare_tree, dict(rec, rootq=0), d, cname, tier, name)
    none = dict(rec, paths=[[None] * len(row) for row in rec['paths']])                          # (a stride past the last root)
    fails(FC.compare_tree, none, d, cname, tier, name)


def test_a_crc_fixture_is_held_at_the_exact_temperatures_only():
    """hn_tree keeps probs as one crc per (root, temperature): the columns of 0.25 and 0.2 cannot be read through a tolerance, and are not"""
    d = FC.load('hn_tree')
    assert [float(t) for t in d['prob_temps']] == [1.0, 0.5, 0.25, float(np.float32(0.2)), 0.0]
    for ti, caught in enumerate([True, True, False, False, True]):
        rec = tree_record(d, 'default')
        rec['probs_crc'][0, ti] ^= 1
        if caught:
            fails(FC.compare_tree, rec, d, 'default', HN.HN_TREE, 'hn')
        else:
            FC.compare_tree(rec, d, 'default', HN.HN_TREE, 'hn')


def test_root_temperature_tiers_stay_where_they_are():
    d = FC.load('tt_tree')
    assert float(d['noise_temp_cfg'][3]) == 1.0
    rec = tree_record(d, 'noise_temp')
    FC.compare_tree(rec, d, 'noise_temp', FC.TREE, 'tt')
    r, j = [(r, j) for r in range(len(rec['q'])) for j in range(len(rec['q'][r])) if 0.05 < abs(rec['q'][r][j]) < 0.5][0]
    for f in ('q', 'p', 'v'):
        for delta, caught in ((2e-5, True), (1e-6, False)):
            bad = copy.deepcopy(rec)
            bad[f][r][j] = np.float32(bad[f][r][j] + delta)
            assert bad[f][r][j] != rec[f][r][j]
            if caught:
                fails(FC.compare_tree, bad, d, 'noise_temp', FC.TREE, 'tt')
            else:
                FC.compare_tree(bad, d, 'noise_temp', FC.TREE, 'tt')
    # hnefatafl's form of the same tier: q and v exact, p within 4 ulps
    d = FC.load('hn_tree')
    assert float(d['temp_cfg'][3]) == 1.0
    rec = tree_record(d, 'temp')
    FC.compare_tree(rec, d, 'temp', HN.HN_TREE, 'hn')
    for f, n, caught in (('q', 1, True), ('v', 1, True), ('p', 4, False), ('p', 6, True)):
        bad = copy.deepcopy(rec)
        j = int(np.argmax(np.abs(bad[f][0])))
        bad[f][0][j] = ulps(bad[f][0][j], n)
        if caught:
            fails(FC.compare_tree, bad, d, 'temp', HN.HN_TREE, 'hn')
        else:
            FC.compare_tree(bad, d, 'temp', HN.HN_TREE, 'hn')


# ------------------------------------------------------------------------------------------------------------------------- agents
def agent_alterations(rec):
    def at(f, idx, step=lambda x: x + 1):
        def alter(bad):
            bad[f][idx] = step(bad[f][idx])
        return alter
    a0 = int(np.argmax(rec['counts'][0, 0]))
    s0 = tuple(np.argwhere(rec['s_pi'] > 0)[0])
    alts = dict(round_sims=at('round_sims', 1), counts=at('counts', (0, 0, a0)), actions=at('actions', (1, 0)), games_played=at('games_played', 2),
                s_obs=at('s_obs', (0, 0, 0, 0)), s_pi=at('s_pi', s0, ulps), s_z=at('s_z', (0, 0), lambda x: 1 - x), r_ws=at('r_ws', (0, 0), lambda x: 1 - x),
                r_turns=at('r_turns', 0))
    if 'obs_crc' in rec:
        alts['obs_crc'] = at('obs_crc', (0, 0), lambda x: x ^ 1)
    return alts


def test_compare_agent_passes_on_the_fixture_and_bites_everywhere():
    d = FC.load('tt_agent')
    rec = agent_record(d, 'plain_')
    assert set(rec) == set(FC.AGENT_FIELDS) and rec['actions'].shape[1] == 4
    FC.compare_agent(rec, d, 'plain_', 'tt')
    FC.compare_agent(dict(rec, ctr=np.zeros(4, np.uint64)), d, 'plain_', 'tt')                   # (run_agent records it; an agent fixture has none)
    alts = agent_alterations(rec)
    assert set(alts) == set(FC.AGENT_FIELDS)
    for field, alter in alts.items():
        bad = copy.deepcopy(rec)
        alter(bad)
        with pytest.raises(AssertionError) as ei:
            FC.compare_agent(bad, d, 'plain_', 'tt')
        assert field in ei.value.args[0] and ei.value.args[0][:2] == ('tt', 'plain_'), (field, ei.value.args)
    for f in FC.AGENT_FIELDS:
        fails(FC.compare_agent, rec, {k: v for k, v in d.items() if k != 'plain_' + f}, 'plain_', 'tt')
        fails(FC.compare_agent, {k: v for k, v in rec.items() if k != f}, d, 'plain_', 'tt')
    fails(FC.compare_agent, dict(rec, fast=0), d, 'plain_', 'tt')


def test_compare_mt19937_agent_passes_on_the_fixture_and_bites_everywhere():
    d = FC.load('tt_mt19937_agent')
    B, rounds = int(d['B']), len(d['actions'])
    rec = agent_record(d, '')
    rec['round_sims'] = np.full(rounds, int(d['sims']))
    rec['obs_crc'] = np.zeros((rounds * int(d['sims']), B), np.uint32)                           # (recorded by run_agent; this fixture holds none)
    ctr = np.zeros(B, np.uint64)
    for kind, slot, n in d['call_order']:                    # a shuffle takes one rank per child, a dirichlet or a choice one entry;
        if slot >= 0:                                        # (the round's coin is no slot's)
            ctr[slot] += np.uint64(n if kind == 0 else 1)
    rec['ctr'] = ctr
    assert ctr.min() > 0 and set(rec) == set(FC.AGENT_FIELDS) | {'ctr'}
    FC.compare_mt19937_agent(rec, d, 'tt')
    alts = agent_alterations({k: v for k, v in rec.items() if k != 'obs_crc'})
    alts['ctr'] = lambda bad: bad['ctr'].__setitem__(1, bad['ctr'][1] + np.uint64(1))
    assert set(alts) == set(FC.AGENT_FIELDS) - {'obs_crc'} | {'ctr'}
    for field, alter in alts.items():
        bad = copy.deepcopy(rec)
        alter(bad)
        with pytest.raises(AssertionError) as ei:
            FC.compare_mt19937_agent(bad, d, 'tt')
        assert field in ei.value.args[0], (field, ei.value.args)
    for key in ('actions', 'counts', 'games_played', 's_obs', 's_pi', 's_z', 'r_ws', 'r_turns', 'sims', 'B', 'call_order'):
        fails(FC.compare_mt19937_agent, rec, {k: v for k, v in d.items() if k != key}, 'tt')
    for f in set(rec) - {'obs_crc'}:
        fails(FC.compare_mt19937_agent, {k: v for k, v in rec.items() if k != f}, d, 'tt')
    fails(FC.compare_mt19937_agent, dict(rec, fast=0), d, 'tt')


# ------------------------------------------------------------------------------------------------------------------------- declarations
def test_the_defaults_are_the_strictest_form_and_every_exception_is_one_listed_here():
    """the tiers and the recorders' defaults as the issue of this module set them, and every weaker form a game file asks for by name:
    a new one has to be added here, with its reason at the call"""
    assert FC.TREE == dict(exact_root_temps=(0.0,), exact_temps=(1.0, 0.5, 0.0), rootn='action', rootn_crc='rootn_crc', rootn_crc_dtype=np.int16,
                           p_ulps=None, raised=False, has_k=False)
    assert FC.EDGE == dict(exact_root_temps=(0.0, 2.0, 0.5), exact_temps=(1.0, 2.0, 0.5, 0.0), rootn='child', rootn_crc='counts_crc',
                           rootn_crc_dtype=np.int32, p_ulps=None, raised=True, has_k=False)
    assert HN.HN_TREE == dict(FC.TREE, p_ulps=4) and HN.HN_EDGE == dict(FC.TREE, p_ulps=4, rootn_crc_dtype=np.int32, has_k=True)
    sig = inspect.signature(FC.record_tree).parameters
    assert sig['path_stride'].default == 1 and sig['launches'].default == FC.LAUNCHES == ['phase', 'fused']
    assert inspect.signature(FC.compare_agent).parameters['not_recorded'].default == ()
    found = []
    for path in sorted(glob.glob(os.path.join(HERE, 'test_gpu_*.py'))):
        for m in re.finditer(r'\b(path_stride|not_recorded|launches)=([^,)]+(?:\([^)]*\))?)', open(path).read()):
            found.append((os.path.basename(path), m.group(1), m.group(2).strip()))
    assert found == [('test_gpu_parity.py', 'path_stride', '7'), ('test_gpu_parity.py', 'path_stride', '5')], found
