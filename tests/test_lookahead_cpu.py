"""One-ply lookahead and the scripted players, without a GPU: the restatement of tests/lookahead_reference.py on this package's host
envs against tests/golden/lookahead.npz (made from the reference's own classes and player objects by
tests/golden/make_lookahead_goldens.py), the connect4 index rule, every refusal of azg_game_lookahead / azg_game_choose_scripted (all of
them come back before anything touches a device), SCRIPTED_SEAT and the class recognition of coach.native_arena."""
import ctypes as C
import pickle

import numpy as np
import pytest

import lookahead_reference as LR

REF_GAMES = (LR.C4, LR.BR, LR.OT, LR.GB, LR.TT, LR.HN)


def _envs():
    import test_gpu_device_games as T
    return T._envs()


# ------------------------------------------------------------------------------------------------------------------------- the fixture
@pytest.mark.parametrize('gid', REF_GAMES, ids=[LR.SHORT[g] for g in REF_GAMES])
def test_perft_on_the_host_envs_is_the_reference(gid):
    """node counts and win_state counts per ply from the opening: the host env's children are the reference's"""
    d, s = LR.golden(), LR.SHORT[gid]
    nodes, wins = LR.perft(_envs()[gid](), LR.PERFT_DEPTH[gid])
    assert len(nodes) == LR.PERFT_DEPTH[gid] == len(d[s + '_perft_nodes'])
    assert nodes.tolist() == d[s + '_perft_nodes'].tolist() and wins.tolist() == d[s + '_perft_wins'].tolist()


def test_perft_of_the_three_player_env():
    """no reference class: recorded here from the host env -- 25 * 24 * 23 placements, nobody can have won with one stone each"""
    nodes, wins = LR.perft(_envs()[LR.TM](), LR.PERFT_DEPTH[LR.TM])
    assert nodes.tolist() == [25, 600, 13800] and wins.tolist() == [[0, 0, 0, 0]] * 3


def _check_player(gid, states, tag):
    d, s = LR.golden(), LR.SHORT[gid]
    move = d[s + tag + '_move']
    raised = d[s + '_built_raised'] if tag else [''] * len(move)
    assert len(states) == len(move)
    for i, st in enumerate(states):
        g = LR.host(gid, st)
        if raised[i]:
            assert move[i] == -1 and LR.scripted_move(gid, g, 0.3) is None and not np.asarray(g.valid_moves()).any(), (tag, i)
            continue
        if gid == LR.C4:
            lst, idx = [int(a) for a in d[s + tag + '_list'][i] if a >= 0], int(d[s + tag + '_idx'][i])
            sets = LR.connect4_sets(g)
            chosen = next(x for x in sets if x)
            assert chosen == lst == sorted(lst), (tag, i, 'the list np.random.choice was handed, ascending', sets, lst)
            assert lst[idx] == move[i]
            assert LR.connect4_move(g, (idx + 0.5) / len(lst)) == (move[i], lst)
        else:
            assert LR.scripted_move(gid, g) == move[i], (tag, i)
    return raised


@pytest.mark.parametrize('gid', sorted(LR.SCRIPTED), ids=[LR.SHORT[g] for g in sorted(LR.SCRIPTED)])
def test_restated_players_are_the_reference(gid):
    """every entry of the fixture: the 256 table positions and the built boards, the boards the reference raises on included"""
    _check_player(gid, LR.positions(gid), '')
    raised = _check_player(gid, LR.built_states(gid), '_built')
    assert sorted(set(raised) - {''}) == (['Exception'] if gid == LR.C4 else ['IndexError']) and list(raised).count('') >= 4


def test_the_quirks_bite_in_the_fixture():
    """connect4: a non-empty stop-loss set was played from and a win set took precedence; othello: both movers, and a greedy move that
    is not the lowest valid one; gobang: a move that is not the lowest empty cell"""
    d = LR.golden()
    c4 = [LR.connect4_sets(LR.host(LR.C4, st)) for st in LR.built_states(LR.C4)[:4]]
    assert any(s[1] and not s[0] for s in c4) and any(s[0] and s[1] for s in c4)
    table_sets = [LR.connect4_sets(LR.host(LR.C4, st)) for st in LR.positions(LR.C4)]
    assert any(s[0] for s in table_sets) and any(not s[0] for s in table_sets)
    for gid in (LR.OT, LR.GB):
        movers, notlowest = set(), 0
        for st, mv in list(zip(LR.positions(gid), d[LR.SHORT[gid] + '_move'])) + list(zip(LR.built_states(gid), d[LR.SHORT[gid] + '_built_move'])):
            if mv >= 0:
                movers.add(int(st[1]))
                notlowest += int(mv != np.flatnonzero(np.asarray(LR.host(gid, st).valid_moves()))[0])
        assert movers == {0, 1} and notlowest > 0, (gid, movers, notlowest)


def test_connect4_index_rule():
    """u = (j + 0.5) / m is element j for every m a connect4 set can have; 0 is the first and the largest double below 1 the last"""
    for m in range(1, 8):
        assert [LR.connect4_index(m, (j + 0.5) / m) for j in range(m)] == list(range(m))
        assert LR.connect4_index(m, 0.0) == 0 and LR.connect4_index(m, float(np.nextafter(1.0, 0))) == m - 1


# ------------------------------------------------------------------------------------------------------------------------- refusals
@pytest.fixture(scope='module')
def lib():
    from alphazero_general_amd import _abi
    return _abi.lib()


def _err(lib):
    return lib.azg_last_error().decode()


def test_lookahead_refusals_come_before_any_launch(lib):
    from alphazero_general_amd import _abi
    buf = C.create_string_buffer(4096)
    p = C.addressof(buf)
    cases = [((7, 1, p, p, p, None, None, None, 0), 'unknown game id'), ((-1, 1, p, p, p, None, None, None, 0), 'unknown game id'),
             ((0, -1, p, p, p, None, None, None, 0), 'count < 0'), ((0, 1, None, p, p, None, None, None, 0), 'null states_dev'),
             ((0, 1, p, None, p, None, None, None, 0), 'null num_dev'), ((0, 1, p, p, None, None, None, None, 0), 'null actions_dev'),
             ((0, 1, p, p, p, None, None, p, 3), 'obs_dtype must be 0 (float32), 1 (float16) or 2 (float16 NHWC8)'),
             ((0, 1, p, p, p, None, None, None, -1), 'obs_dtype must be 0 (float32), 1 (float16) or 2 (float16 NHWC8)')]
    for args, text in cases:
        assert lib.azg_game_lookahead(None, *args) == _abi.E_INVALID_ARG and _err(lib) == text, args
    for game in range(7):
        assert lib.azg_game_lookahead(None, game, 0, p, p, p, p, p, p, 2) == 0      # count == 0: nothing launched, no device needed
    assert buf.raw == b'\0' * 4096


def test_choose_scripted_refusals_come_before_any_launch(lib):
    from alphazero_general_amd import _abi
    buf = C.create_string_buffer(4096)
    p = C.addressof(buf)
    cases = [((7, 1, p, p, p, p), 'unknown game id'), ((0, -1, p, p, p, p), 'count < 0'), ((0, 1, None, p, p, p), 'null states_dev'),
             ((3, 1, p, None, p, p), 'null u_dev'), ((4, 1, p, p, None, p), 'null actions_dev'), ((0, 1, p, p, p, None), 'null status_dev')]
    for args, text in cases:
        assert lib.azg_game_choose_scripted(None, *args) == _abi.E_INVALID_ARG and _err(lib) == text, args
    names = {0: b'OneStepLookaheadConnect4Player', 3: b'GreedyOthelloPlayer', 4: b'GreedyGobangPlayer'}
    for game in range(7):
        assert lib.azg_game_scripted_player(game) == names.get(game)
        for count in (0, 5):
            if game in names and count:
                continue                                             # (a launch: tests/test_gpu_lookahead.py)
            rc = lib.azg_game_choose_scripted(None, game, count, p, p, p, p)
            assert rc == (0 if game in names else _abi.E_UNSUPPORTED), (game, count)
            if game not in names:
                assert _err(lib).startswith('the reference has no scripted player for ')
    assert lib.azg_game_scripted_player(9) is None and _err(lib) == 'unknown game id'
    assert buf.raw == b'\0' * 4096
    assert {g: n.decode() for g, n in names.items()} == LR.SCRIPTED


# ------------------------------------------------------------------------------------------------------------------------- seats
def test_scripted_seat_pickles_to_itself():
    from alphazero_general_amd.selfplay import RANDOM_SEAT, SCRIPTED_SEAT, is_tree_free
    assert pickle.loads(pickle.dumps(SCRIPTED_SEAT)) is SCRIPTED_SEAT and pickle.loads(pickle.dumps([SCRIPTED_SEAT, None]))[0] is SCRIPTED_SEAT
    assert is_tree_free(SCRIPTED_SEAT) and SCRIPTED_SEAT != RANDOM_SEAT and repr(SCRIPTED_SEAT) == 'SCRIPTED_SEAT'
    assert len({SCRIPTED_SEAT, pickle.loads(pickle.dumps(SCRIPTED_SEAT)), RANDOM_SEAT}) == 2


def test_arena_runner_refuses_the_seat_for_a_game_without_a_player(lib):
    from alphazero_general_amd.selfplay import ArenaRunner, SCRIPTED_SEAT
    with pytest.raises(NotImplementedError, match='no scripted player'):
        ArenaRunner(_envs()[LR.TT], [object(), SCRIPTED_SEAT], {}, num_slots=4)      # (refused before an engine is made)


def _fake(module, name, **attrs):
    obj = type(name, (), {'__module__': module})()
    for k, v in attrs.items():
        setattr(obj, k, v)
    return obj


def test_coach_recognises_the_three_classes_and_nothing_else():
    from alphazero_general_amd import coach as AC
    envs = _envs()
    theirs = {LR.C4: ('alphazero.envs.connect4.players', 'OneStepLookaheadConnect4Player'),
              LR.OT: ('alphazero.envs.othello.OthelloPlayers', 'GreedyOthelloPlayer'),
              LR.GB: ('alphazero.envs.gobang.GobangPlayers', 'GreedyGobangPlayer')}
    for gid, (mod, name) in theirs.items():
        for other in range(7):
            assert AC.is_scripted_player(_fake(mod, name), envs[other]) == (other == gid), (name, other)
        assert not AC.is_scripted_player(_fake(mod, name, play=lambda state: 0), envs[gid]), 'an instance with its own play'
        assert not AC.is_scripted_player(_fake('elsewhere.' + mod.rsplit('.', 1)[-1], name), envs[gid]), 'another package'
        assert not AC.is_scripted_player(type(name, (type(_fake(mod, name)),), {'__module__': 'mine'})(), envs[gid]), 'a subclass'
        assert AC.tree_free_kind(_fake(mod, name)) is None
    for mod, name in (('alphazero.envs.connect4.players', 'HumanConnect4Player'), ('alphazero.envs.othello.OthelloPlayers', 'HumanOthelloPlayer'),
                      ('alphazero.envs.hnefatafl.players', 'GreedyTaflPlayer'), ('alphazero.envs.brandubh.players', 'GreedyTaflPlayer'),
                      ('alphazero.GenericPlayers', 'RandomPlayer'), ('alphazero.envs.tictactoe.TicTacToePlayers', 'GreedyTicTacToePlayer')):
        assert not any(AC.is_scripted_player(_fake(mod, name), g) for g in envs), name


def test_native_arena_seats_them_only_under_the_opt_in():
    """scripted_seats=False (the default): the arena falls through to the reference's play_games; True: the seats are [net, SCRIPTED_SEAT]"""
    import types
    from alphazero_general_amd import coach as AC
    from alphazero_general_amd.selfplay import SCRIPTED_SEAT
    Game = _envs()[LR.C4]
    reached, led = [], []

    class StandInArena:
        def __init__(self, players, game_cls, use_batched_mcts=True, args=None):
            self.players, self.game_cls, self.use_batched_mcts, self.args = players, game_cls, use_batched_mcts, args
            self.stop_event = types.SimpleNamespace(is_set=lambda: False)

        def play_games(self, num, verbose=False, shuffle_players=True):
            reached.append(num)
            return 'reference'
    mcts = _fake('alphazero.GenericPlayers', 'MCTSPlayer', nn='net')
    scripted = _fake('alphazero.envs.connect4.players', 'OneStepLookaheadConnect4Player')
    off = AC.native_arena(StandInArena)([mcts, scripted], Game, use_batched_mcts=False, args={})
    assert off.play_games(8) == 'reference' and reached == [8]
    only_tf = AC.native_arena(StandInArena, tree_free_seats=True)([mcts, scripted], Game, use_batched_mcts=False, args={})
    assert only_tf.play_games(8) == 'reference' and reached == [8, 8]
    On = AC.native_arena(StandInArena, scripted_seats=True)
    on = On([mcts, scripted], Game, use_batched_mcts=False, args={})
    on._azg_lead = lambda g, ours, num, shuffle: led.append((g, ours, num)) or 'device'
    real = AC._NetCache.get
    AC._NetCache.get = lambda self, nn: ('ours', nn)
    try:
        assert on.play_games(8) == 'device' and reached == [8, 8]
        assert led[0][0] is Game and led[0][1] == [('ours', 'net'), SCRIPTED_SEAT] and led[0][1][1] is SCRIPTED_SEAT
        wrong_game = On([mcts, scripted], _envs()[LR.OT], use_batched_mcts=False, args={})
        assert wrong_game.play_games(4) == 'reference' and reached == [8, 8, 4], 'a connect4 player in an othello arena'
        rnd = _fake('alphazero.GenericPlayers', 'RandomPlayer')
        assert On([scripted, rnd], Game, use_batched_mcts=False, args={}).play_games(2) == 'reference', 'RandomPlayer needs tree_free_seats'
    finally:
        AC._NetCache.get = real
    assert AC.native_arena(On, scripted_seats=True) is On and AC.native_arena(On) is not On
