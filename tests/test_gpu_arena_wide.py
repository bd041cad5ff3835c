"""The batched Arena on the persistent wide launch (azg_search_arena_wide_exact_f16: one game per workgroup, the mover's tree, the mover's
model -- tower, 1x1 head convolutions and all A + P+1 logits --, or a raw seat's constants) for every (game, tower width) the persistent
self-play search supports, and raw seats (the reference's RawMCTSPlayer.process, GenericPlayers.py:198-200) on every path:

  * persistent (graph-captured round and eager) against the host-split path (ArenaRunner.step: select, NNetWrapper-equal evaluation of
    every model's slice, backup), bit for bit: actions of every round, counters, result records, tallies;
  * against the CPU oracle (OAgent(is_arena=True)) fed NNetWrapper.process for each model's rows and torch.full(1 / A) / zeros for a
    raw seat's rows, until every slot has restarted.

The oracle has no othello rules: othello is held to the host-split path, which the oracle tests hold to the reference on the other games."""
import importlib

import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu

PAIRS = [('connect4', 32), ('connect4', 64), ('brandubh', 64), ('trimok', 32), ('othello', 32), ('othello', 64)]


def _game(name):
    return importlib.import_module('alphazero_general_amd.envs.' + name).Game


def _nets(name, width, n, seed0=20):
    import torch
    from alphazero_general_amd import nnet as N
    from alphazero_general_amd.utils import dotdict
    Game = _game(name)
    na = dotdict(dict(N.CONNECT4_NET_ARGS if width == 128 else N.BRANDUBH_NET_ARGS if name == 'brandubh' else N.DEFAULT_NET_ARGS))
    na['num_channels'] = width
    out = []
    for m in range(n):
        torch.manual_seed(seed0 + m)
        w = N.NNetWrapper(Game, na, device='cuda:0', dtype=torch.float16)
        w.refresh()
        out.append(w)
    return Game, out


def _args(**kw):
    from alphazero_general_amd.utils import dotdict, default_temp_scaling
    a = dotdict(numMCTSSims=10, numFastSims=4, probFastSim=0.0, gamesPerIteration=1 << 30, cpuct=4.0, fpu_reduction=0.4,
                root_noise_frac=0.3, root_policy_temp=1.3, min_discount=1.0, add_root_noise=True, add_root_temp=True,
                symmetricSamples=True, mctsResetThreshold=0, startTemp=1.0, arenaTemp=0.25, temp_scaling_fn=default_temp_scaling,
                use_draws_for_winrate=True)
    a.update(kw)
    return a


def _play(r, rounds):
    acts = []
    for _ in range(rounds):
        r.play_round()
        acts.append(r.engine.last_actions().cpu().numpy().copy())
    ws, turns, slot = r.engine.results()
    return np.array(acts), r.engine.counters(), (np.asarray(ws), np.asarray(turns), np.asarray(slot)), r.results()


def _same(runs):
    a0, c0, rec0, res0 = runs[0]
    assert c0['games_played'] > 0 and (a0 >= 0).any()
    for a, c, rec, res in runs[1:]:
        assert (a == a0).all()
        assert all(c[k] == c0[k] for k in ('games_played', 'sims', 'expansions', 'num_results'))
        assert all(x.shape == y.shape and (x == y).all() for x, y in zip(rec, rec0))
        assert res == res0
    wins, draws, _ = res0
    assert sum(wins) + draws == len(rec0[0])


def _forms(Game, nets, args, B, seed, seats, rounds):
    """(graph, eager, host-split) runs of the same arena; the persistent ones must be the wide launch"""
    from alphazero_general_amd.selfplay import ArenaRunner
    runs = []
    for form in ('graph', 'eager', 'host'):
        r = ArenaRunner(Game, nets, args, num_slots=B, seed=seed, seats=seats, use_graph=form == 'graph',
                        fused_search=True if form != 'host' else False)
        assert r.wide_search == (form != 'host') and (r._graph is not None) == (form == 'graph')
        runs.append(_play(r, rounds))
        r.engine.close()
    return runs


@pytest.mark.parametrize('seats', ['agent', 'slot'])
@pytest.mark.parametrize('name,width', PAIRS)
def test_persistent_wide_arena_equals_host_split(name, width, seats):
    """two differently seeded nets (three on the 3-player env): the persistent launch, captured and eager, plays exactly the games the
    host-split path plays, past the first finished games (slots restart)"""
    Game, nets = _nets(name, width, _players(name))
    rounds = min(Game.max_turns(), 66) + 6
    _same(_forms(Game, nets, _args(), 24, 5, seats, rounds))


@pytest.mark.parametrize('name,width', PAIRS)
def test_raw_seat_persistent_equals_host_split(name, width):
    """[net, None] ([net, None, None] on the 3-player env): the raw seat's games run no network in the persistent launch and its rows
    are RawMCTSPlayer's constants on the host-split path -- the same games"""
    Game, nets = _nets(name, width, 1)
    seats = nets + [None] * (Game.num_players() - 1)
    rounds = min(Game.max_turns(), 66) + 6
    _same(_forms(Game, seats, _args(), 24, 7, 'slot', rounds))


def _players(name):
    return _game(name).num_players()


def _oracle_arena(Game, nets, B, sims, games, seed, **runner_kw):
    """the runner against the oracle fed each model's NNetWrapper.process rows (a raw seat: torch.full(1 / A) and zeros) until `games`
    games are done: actions every round, counters, result records, tallies"""
    import torch
    from alphazero_general_amd.selfplay import ArenaRunner
    gid = Game.AZG_GAME_ID
    gi = ol.game_info(gid)
    P = Game.num_players()
    r = ArenaRunner(Game, nets, _args(numMCTSSims=sims, gamesPerIteration=games), num_slots=B, seed=seed, seats='agent', **runner_kw)
    ag = ol.OAgent(gid, B, sims=sims, games_per_iteration=games, seed=seed, cpuct=4.0, fpu_reduction=0.4, is_arena=True, ref_misroute=False)
    assert ag.player_to_index() == r.player_to_index and sorted(r.player_to_index) == list(range(P))
    rounds = 0
    while ag.games_played < games:
        ag.begin_round()
        for _ in range(sims):
            oobs, rg, rm = ag.generate_batch()
            pol = np.zeros((B, gi.action_size), np.float32); val = np.zeros((B, gi.num_players + gi.has_draw), np.float32)
            for m, n in enumerate(nets):
                idx = np.flatnonzero(rm == m)
                if not len(idx):
                    continue
                if n is None:                                        # RawMCTSPlayer.process (GenericPlayers.py:198-200)
                    p, v = torch.full((len(idx), gi.action_size), 1 / gi.action_size), torch.zeros(len(idx), gi.num_players + 1)
                else:
                    p, v = n.process(torch.from_numpy(oobs[idx]))
                pol[idx], val[idx] = p.cpu().numpy(), v.cpu().numpy()
            ag.process_batch(pol, val)
        ag.play_moves()
        r.play_round()
        assert (r.engine.last_actions().cpu().numpy() == ag.last_actions()).all(), rounds
        rounds += 1
    c = r.engine.counters()
    assert c['games_played'] == ag.games_played == games and c['sims'] == ag.sims_done and c['expansions'] == ag.expansions
    ws, turns, slot = r.engine.results()
    ows, oturns, oslot = ag.results()
    assert (ws == ows).all() and (turns == oturns).all() and (slot == oslot).all() and len(ws) >= games
    wins, draws, rates = r.results()
    assert sum(wins) + draws == len(ws) and len(wins) == P
    return r


@pytest.mark.parametrize('name,B,sims,games', [('connect4', 32, 16, 40), ('trimok', 24, 16, 30)])
def test_persistent_wide_arena_vs_oracle(name, B, sims, games):
    """connect4 x 32 (two models) and the 3-player env x 32 (three models) on the persistent launch against the oracle"""
    Game, nets = _nets(name, 32, _players(name))
    r = _oracle_arena(Game, nets, B, sims, games, 13)
    assert r.wide_search and r._graph is not None


@pytest.mark.parametrize('form', ['persistent', 'phase'])
@pytest.mark.parametrize('name,width,B,sims,games', [('connect4', 32, 32, 16, 40), ('brandubh', 64, 16, 12, 18), ('trimok', 32, 24, 16, 30)])
def test_raw_seats_vs_oracle(name, width, B, sims, games, form):
    """[net, None] ([net, None, None] on the 3-player env) against the oracle fed RawMCTSPlayer's constants for the raw rows, on the
    persistent launch and on the per-simulation path"""
    Game, nets = _nets(name, width, 1)
    r = _oracle_arena(Game, nets + [None] * (Game.num_players() - 1), B, sims, games, 17, fused_search=form == 'persistent')
    assert r.wide_search == (form == 'persistent')


def test_raw_seat_with_fused_head_net_vs_oracle():
    """connect4 x 128 (fused heads) against a raw seat: no persistent launch takes raw seats there, the per-simulation path plays"""
    from alphazero_general_amd.selfplay import ArenaRunner
    Game, nets = _nets('connect4', 128, 1)
    with pytest.raises(NotImplementedError):
        ArenaRunner(Game, nets + [None], _args(), num_slots=8, seed=1, fused_search=True)
    r = _oracle_arena(Game, nets + [None], 32, 12, 40, 19)
    assert not r.wide_search and not r.fused_search and not r.device_split


@pytest.mark.parametrize('raw', [False, True])
def test_default_coach_size_persistent_equals_host_split(raw):
    """connect4 x 32 (the reference's default net) at the default Coach's arena size -- 128 games x 100 simulations --, 16 moves"""
    from alphazero_general_amd.selfplay import ArenaRunner
    Game, nets = _nets('connect4', 32, 2)
    seats = [nets[0], None] if raw else nets
    runs = []
    for fused in (True, False):
        r = ArenaRunner(Game, seats, _args(numMCTSSims=100), num_slots=128, seed=3, fused_search=fused)
        acts = []
        for _ in range(16):
            r.play_round()
            acts.append(r.engine.last_actions().cpu().numpy().copy())
        runs.append((np.array(acts), r.engine.counters(), r.engine.root_counts().cpu().numpy()))
        r.engine.close()
    (a0, c0, n0), (a1, c1, n1) = runs
    assert (a0 == a1).all() and (n0 == n1).all()
    assert all(c0[k] == c1[k] for k in ('games_played', 'sims', 'expansions'))


def test_run_arena_with_a_raw_seat():
    """iteration.run_arena with a None seat on one rank: every game is tallied, winrates follow Arena.__update_winrates"""
    from alphazero_general_amd import iteration as I
    Game, nets = _nets('connect4', 32, 1)
    out = I.run_arena(Game, [nets[0], None], _args(numMCTSSims=16), 40, num_slots=16, details=True)
    assert out['games'] >= 40 and sum(out['wins']) + out['draws'] == out['num_results'] >= 40
    n = sum(out['wins']) + out['draws']
    assert out['winrates'] == [(w + 0.5 * out['draws']) / n for w in out['wins']]
