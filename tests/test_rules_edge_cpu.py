"""The built rule fixtures (tests/golden/{br,c4}_rules_edge.npz: the reference's brandubh and connect4 on hand-built scenarios, dense
boards and capture-greedy playouts, written by tests/golden/make_rules_edge_goldens.py) and trimok's boards (tests/rules_edge.py),
checked without a GPU:

  * every record replayed on the C oracle (oracle/azg_games_ref.c, azg_brandubh_ref.c, azg_trimok_ref.c) and on the host envs
    (alphazero_general_amd/envs): valid moves, win state, observation, and with an action the successor's cells, player, turns and
    king flag -- the two implementations the GPU parity tests lean on;
  * the coverage floors, again, from the counts stored beside the data, and the counts themselves from the records;
  * what a fixture says twice agrees: every action is legal where it is played, every successor is a record, no position is
    stored twice without need;
  * trimok has no reference, its host env is the definition: the oracle against the env on every line of three, the wrapped
    triples, two and three players holding a line, full-board draws and the 25th stone;
  * with the reference checkout present, the generator writes both files again byte for byte, and the old generators still
    write br_rules.npz / c4_rules.npz."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as ol
import rules_edge as RE

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, 'golden')
REF = '/root/reference'
GAMES = {'c4': RE.C4, 'br': RE.BR, 'tm': RE.TM}


def _env(name):
    import importlib
    return importlib.import_module('alphazero_general_amd.envs.' + {'c4': 'connect4', 'br': 'brandubh', 'tm': 'trimok'}[name]).Game


class _Oracle:
    """the C oracle behind the few calls the replay needs"""

    def __init__(self, game, cells, player, turns, kc):
        st = ol.State()
        for i, v in enumerate(cells):
            st.cells[i] = int(v)
        st.player, st.turns, st.aux[0] = int(player), int(turns), int(kc)
        self.g = ol.OGame(game, st)

    def valid_moves(self):
        return self.g.valid_moves()

    def win_state(self):
        return self.g.win_state()

    def observation(self):
        return self.g.observation()

    def play_action(self, a):
        self.g.play(a)

    def state(self):
        return self.g.cells(), self.g.player, self.g.turns, int(self.g.s.aux[0])


class _Host:
    def __init__(self, name, cells, player, turns, kc):
        Game = _env(name)
        self.g = Game.from_azg_state(cells, player, turns, kc) if name == 'br' else Game.from_azg_state(cells, player, turns)

    def valid_moves(self):
        return np.asarray(self.g.valid_moves())

    def win_state(self):
        return np.asarray(self.g.win_state())

    def observation(self):
        return np.asarray(self.g.observation(), np.float32)

    def play_action(self, a):
        self.g.play_action(int(a))

    def state(self):
        s = self.g.to_azg_state()
        return np.asarray(s[0], np.int8), s[1], s[2], (s[3] if len(s) > 3 else 0)


@pytest.mark.parametrize('impl', ['oracle', 'host'])
@pytest.mark.parametrize('name', ['br', 'c4', 'tm'])
def test_every_record_replays(name, impl):
    d = RE.load(name)
    n = len(d['action'])
    played = 0
    for i in range(n):
        args = (d['cells'][i], int(d['player'][i]), int(d['turns'][i]), int(d['kc'][i]))
        g = _Oracle(GAMES[name], *args) if impl == 'oracle' else _Host(name, *args)
        assert (np.asarray(g.valid_moves()) == d['valids'][i]).all(), ('valid_moves', i)
        assert (np.asarray(g.win_state()) == d['ws'][i]).all(), ('win_state', i, g.win_state(), d['ws'][i])
        assert RE.crc(g.observation()) == d['obs_crc'][i], ('observation', i)
        a, j = int(d['action'][i]), int(d['succ'][i])
        if a < 0:
            continue
        g.play_action(a)
        cells, player, turns, kc = g.state()
        assert (cells == d['cells'][j]).all(), ('play_action: board', i, a)
        assert (player, turns, kc) == (d['player'][j], d['turns'][j], d['kc'][j]), ('play_action: player / turns / king flag', i, a)
        assert RE.crc(g.observation()) == d['obs_crc'][j], ('observation after play_action', i)
        played += 1
    assert played == int((d['action'] >= 0).sum()) and played >= {'br': 1500, 'c4': 290, 'tm': 500}[name]


@pytest.mark.parametrize('name', ['br', 'c4', 'tm'])
def test_records_are_consistent(name):
    d = RE.load(name)
    n = len(d['action'])
    assert n <= RE.MAX_RECORDS
    act, succ = d['action'].astype(int), d['succ'].astype(int)
    has = act >= 0
    assert ((succ >= 0) == has).all() and (succ < n).all()                       # every successor is a record
    assert (d['valids'][np.flatnonzero(has), act[has]] == 1).all()               # every action is legal in its position ...
    assert not d['ws'][has].any()                                                # ... which is live
    assert (d['turns'][succ[has]] == d['turns'][has] + 1).all()
    P = d['ws'].shape[1] - 1
    assert (d['player'][succ[has]] == (d['player'][has] + 1) % P).all() and (d['player'] == d['turns'] % P).all()
    assert (d['ws'].sum(1) <= 1).all()
    states = [(d['cells'][i].tobytes(), int(d['turns'][i]), int(d['kc'][i])) for i in range(n)]
    moves = [(s, int(a)) for s, a in zip(states, act)]
    assert len(set(moves)) == n                                                  # no (position, action) twice
    first = {}
    for i, s in enumerate(states):
        first.setdefault(s, []).append(i)
    for s, rows in first.items():                                                # a position is repeated only to carry another action
        assert len(rows) == 1 or all(act[i] >= 0 for i in rows), rows
        for i in rows[1:]:
            assert (d['valids'][i] == d['valids'][rows[0]]).all() and (d['ws'][i] == d['ws'][rows[0]]).all() and d['obs_crc'][i] == d['obs_crc'][rows[0]]
    if name != 'tm':
        assert os.path.getsize(os.path.join(G, name + '_rules_edge.npz')) <= RE.SIZE_LIMIT
        assert RE.cov_total(d)['positions'] == len(first) and RE.cov_total(d)['moves'] == int(has.sum())


def test_br_fixture_reaches_its_edges():
    d = RE.load('br')
    RE.check_floors(d, RE.BR_FLOORS)
    assert RE.cov_of(d, 'dense', 'term_nomove_def') + RE.cov_of(d, 'dense', 'term_nomove_att') >= RE.BR_DENSE_NOMOVE
    met = dict(zip([str(x) for x in d['dense_met_names']], d['dense_met'].tolist()))     # what the whole dense run met, kept or not
    assert met['nomove'] >= 100 and met['rm2'] >= 8 and met['kc'] >= 100 and met['max_k'] >= 65
    # the stored counts, again, from the records themselves
    tot, has = RE.cov_total(d), d['action'] >= 0
    rm = d['removed'][has]
    assert ((rm == 1).sum(), (rm == 2).sum(), (rm >= 3).sum()) == (tot['rm1'], tot['rm2'], tot['rm3p']) and (d['removed'][~has] == 0).all()
    pieces = lambda c: np.isin(c, (1, 2)).sum(1)
    assert (pieces(d['cells'][has]) - pieces(d['cells'][d['succ'][has]]) == rm).all()
    assert int(((d['kc'][d['succ'][has]] == 1) & (d['kc'][has] == 0)).sum()) == tot['kc_set']
    k = d['valids'].sum(1)
    assert int(k.max()) == tot['max_k'] >= 65 and tot['max_k'] <= 96
    uniq = {}
    for i in range(len(k)):
        uniq.setdefault((d['cells'][i].tobytes(), int(d['turns'][i]), int(d['kc'][i])), i)
    u = np.array(sorted(uniq.values()))
    ws, turns, kc, esc = d['ws'][u], d['turns'][u], d['kc'][u], (d['cells'][u] == 8).any(1)
    over = ws.any(1)
    t100 = over & (turns >= 100)
    assert (ws[t100, 2] == 1).all() and int(t100.sum()) == tot['term_turn100'] and not ws[~t100, 2].any()
    assert int((over & ~t100 & esc).sum()) == tot['term_escape'] and (ws[over & ~t100 & esc, 1] == 1).all()
    assert int((over & ~t100 & ~esc & (ws[:, 1] == 1)).sum()) == tot['term_nomove_def']
    assert int((over & ~t100 & ~esc & (ws[:, 0] == 1) & (kc == 1)).sum()) == tot['term_capture']
    assert int((over & ~t100 & ~esc & (ws[:, 0] == 1) & (kc == 0)).sum()) == tot['term_nomove_att']
    assert int((over & (k[u] > 0)).sum()) == tot['over_with_moves'] and int((k[u] > 64).sum()) == tot['k_over_64']
    # a king is never lifted, and stands on a corner (8), the throne (7) or a plain square (3)
    assert (np.isin(d['cells'], (3, 7, 8)).sum(1) == 1).all()
    fam = [str(x) for x in d['family_names']]
    assert fam == ['custodian', 'kingcap', 'surround', 'moves', 'win', 'dense', 'greedy'] and int(d['family'].max()) == len(fam) - 1


def test_c4_fixture_reaches_its_edges():
    d = RE.load('c4')
    RE.check_floors(d, RE.C4_FLOORS)
    tot, has = RE.cov_total(d), d['action'] >= 0
    b = d['cells'].reshape(-1, 6, 7)
    full = (b != 0).all((1, 2))
    assert int((d['ws'][:, 2] == 1).sum()) == tot['draws'] >= 4 and (d['ws'][:, 2] == full & ~d['ws'][:, :2].any(1)).all()
    last = has & (d['turns'] == 41)
    ws_after = d['ws'][d['succ'][last]]
    assert int(ws_after[:, 2].sum()) == tot['draw_on_42nd'] and int(ws_after[:, :2].sum()) == tot['win_on_42nd'] and ws_after.any(1).all()
    assert (d['valids'] == (b[:, 0, :] == 0)).all()                               # the top row is the valid mask, win or not
    # every column at every height is played: the stone lands on the lowest free cell
    seen = set()
    for i in np.flatnonzero(has):
        a, after = int(d['action'][i]), b[d['succ'][i]]
        h = int((b[i][:, a] != 0).sum())
        assert after[5 - h, a] == (1, -1)[d['player'][i]] and ((after != b[i]).sum() == 1)
        seen.add((a, h))
    assert seen == {(c, h) for c in range(7) for h in range(6)}
    assert {int(c) for i in range(len(b)) for c in np.flatnonzero(b[i][0] != 0)} == set(range(7))


def test_tm_boards_reach_their_edges():
    d = RE.load('tm')
    lines, wrapped = RE.tm_lines(), RE.tm_wrapped()
    assert len(lines) == 48 and len(wrapped) == 8 + 4 + 8              # steps 1, 6, 4: the runs that cross a row end
    ws, cells = d['ws'], d['cells']
    for p in range(3):
        won = {tuple(np.flatnonzero(c == p + 1)) for c, w in zip(cells, ws) if w[p] and np.count_nonzero(c) == 3}
        assert won == {tuple(sorted(l)) for l in lines}, p                        # every line alone wins for every colour
        for tri in wrapped:
            i = [j for j, c in enumerate(cells) if np.count_nonzero(c) == 3 and (c[list(tri)] == p + 1).all()]
            assert len(i) == 1 and not ws[i[0]].any(), (p, tri)                 # and no wrapped triple does
    assert int(ws[:, 3].sum()) >= 6 and ((cells != 0).all(1) == (d['turns'] == 25)).all()
    both = [i for i, c in enumerate(cells) if sum(any((c[list(l)] == p + 1).all() for l in lines) for p in range(3)) >= 2]
    assert len(both) >= 16 and all(ws[i].argmax() == min(p for p in range(3) if any((cells[i][list(l)] == p + 1).all() for l in lines)) for i in both)
    last = (d['action'] >= 0) & (d['turns'] == 24)
    after = ws[d['succ'][last]]
    assert int(after[:, 3].sum()) >= 6 and int(after[:, 0].sum()) >= 4            # the 25th stone: a draw, or a win that comes first


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, 'alphazero')), reason='needs the reference checkout (build container only)')
def test_rule_fixtures_regenerate_identically(tmp_path):
    """the generator, run on the reference again into a temporary directory, writes both new fixtures byte for byte, and the
    generators of the old rule tables still write the committed br_rules.npz / c4_rules.npz"""
    code = ('import sys; sys.path.insert(0, %r); import make_rules_edge_goldens as m; m.main(["br", "c4"], out_dir=%r, verbose=False); '
            'import make_goldens as g; g.OUT = %r; g.gen_c4_rules(); g.gen_br_rules()') % (G, str(tmp_path), str(tmp_path))
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=1800, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    for f in ('br_rules_edge.npz', 'c4_rules_edge.npz', 'br_rules.npz', 'c4_rules.npz'):
        with open(os.path.join(str(tmp_path), f), 'rb') as a, open(os.path.join(G, f), 'rb') as b:
            assert a.read() == b.read(), f
