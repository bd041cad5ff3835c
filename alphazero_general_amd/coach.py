"""NATIVE mode behind the reference's unchanged `Coach.learn()` (alphazero/Coach.py:225-288).

    from alphazero.Coach import Coach                      # the reference's own class, untouched
    from alphazero_general_amd.coach import native_coach
    coach = native_coach(Coach)(Game, nnet, args)          # `nnet`: the reference's NNetWrapper (it keeps training on it)
    coach.learn()

`native_coach` returns a subclass that overrides EXACTLY the five methods learn() calls for self-play -- generateSelfPlayAgents,
processSelfPlayBatches, saveIterationSamples, processGameResults, killSelfPlayAgents (Coach.py:291,326,364,389,401) -- and rebinds the
name `Arena` in the Coach's module to `native_arena(Arena)`, whose play_games takes the batched branch (Arena.pyx:223-328) to the
device when every player is a model player or the reference's RawMCTSPlayer (compareToBaseline's default baselineTester, Coach.py:70,
575-584: a raw seat, evaluated on the device with RawMCTSPlayer.process's constants) of a game with device rules.  Everything else --
train(), gating, checkpoints, the TensorBoard writer, compareToBaseline against other non-model players (RandomPlayer, unbatched
arenas) -- runs the reference's code; native_coach(..., raw_seats=False) sends RawMCTSPlayer arenas there too, and
native_coach(..., tree_free_seats=True) brings RandomPlayer / NNPlayer arenas, unbatched ones included, to the device, and
native_coach(..., scripted_seats=True) the games' scripted baseline players.  No agent processes, no shared
tensors, no queues: the games live on the GPU(s) (iteration.run_iteration / run_arena), the live net's weights are adopted in
memory (NNetWrapper.adopt), and the three sample files the unchanged Coach.train loads (:442-456) are written by rank 0.

Multi-GPU: start the training script under torch.distributed.run; rank 0 builds the Coach, the other ranks call
`alphazero_general_amd.iteration.serve(Game)`.
"""
import os
import sys
import time

from . import iteration as it_mod
from .Game import has_device_rules


def _ours(game_cls):
    """this package's GameState class for a game with device rules (the reference's own env classes are recognised by module name,
    Game.azg_game_id), or None: the runners read the static protocol (observation_size, max_turns, symmetries ...) from it -- the
    reference's brandubh class lacks has_draw / max_turns at this snapshot"""
    import importlib
    from .Game import azg_game_id
    if not has_device_rules(game_cls):
        return None
    return importlib.import_module(__package__ + '.envs.' + ('connect4', 'brandubh', 'trimok', 'othello', 'gobang', 'tictactoe', 'hnefatafl')[azg_game_id(game_cls)]).Game


class _NetCache:
    """this package's NNetWrapper per reference wrapper, re-adopting the live weights before every use"""

    def __init__(self, game_cls, device=None):
        self.game_cls, self.device, self.map = game_cls, device, {}

    def get(self, ref_net):
        from .nnet import NNetWrapper
        if isinstance(ref_net, NNetWrapper):
            return ref_net
        w = self.map.get(id(ref_net))
        if w is None:
            w = self.map[id(ref_net)] = NNetWrapper(self.game_cls, ref_net.args, device=self.device)
        return w.adopt(ref_net)


def native_coach(Coach, *, device=None, install_arena=True, raw_seats=True, tree_free_seats=False, scripted_seats=False):
    """class factory: the reference's Coach with its self-play phase on the device engine (see the module docstring).  tree_free_seats:
    native_arena's opt-in -- arenas against RandomPlayer / NNPlayer (compareToBaseline with such a baselineTester) on the device too; scripted_seats: the same for
    the scripted baseline players (is_scripted_player)."""
    cmod = sys.modules[Coach.__module__]
    TrainState = getattr(cmod, 'TrainState', None)

    def _state(self, name):
        if TrainState is not None and hasattr(TrainState, name):
            self.state = getattr(TrainState, name)

    class NativeCoach(Coach):
        __doc__ = 'native_coach(%s): self-play and batched gating on the MI355X engine' % Coach.__name__

        def _azg_setup(self):
            if getattr(self, '_azg_game', None) is None:
                g = _ours(self.game_cls)
                if g is None:
                    raise NotImplementedError('%r has no device rules (alphazero_general_amd.envs): native mode cannot play it' % (self.game_cls,))
                self._azg_game, self._azg_nets, self._azg_result = g, _NetCache(g, device), None
            return self._azg_game

        def generateSelfPlayAgents(self):                            # Coach.py:291-323
            _state(self, 'INIT_AGENTS')
            self._azg_setup()
            src = self.self_play_net if self.args.model_gating else self.train_net      # (:334)
            self._azg_net = None if self.warmup else self._azg_nets.get(src)
            self.agents = []                                         # (learn()'s final `if self.agents: killSelfPlayAgents()` :286-287)
            _state(self, 'STANDBY')

        def processSelfPlayBatches(self, iteration):                 # Coach.py:326-361
            _state(self, 'SELF_PLAY')
            t0 = time.time()
            folder = os.path.join(self.args.data, self.args.run_name)
            # (the sample files are written here, by rank 0 right behind the exchange step; saveIterationSamples reports them)
            self._azg_result = r = it_mod.lead('selfplay', self._azg_game, [self._azg_net], self.args, iteration=iteration, folder=folder,
                                               warmup=bool(self.warmup), keep_samples=False, stop=self.stop_train.is_set)
            self.sample_time = (time.time() - t0) / max(r['games'], 1)
            self.iter_time = time.time() - t0
            self.writer.add_scalar('loss/sample_time', self.sample_time, iteration)
            _state(self, 'STANDBY')

        def saveIterationSamples(self, iteration):                   # Coach.py:364-386
            _state(self, 'SAVE_SAMPLES')
            print('Saving %d samples' % self._azg_result['num_samples'])
            _state(self, 'STANDBY')

        def processGameResults(self, iteration):                     # Coach.py:389-398
            _state(self, 'PROCESS_RESULTS')
            r = self._azg_result
            n = max(r['num_results'], 1)
            for i, w in enumerate(r['wins']):
                self.writer.add_scalar('win_rate/player%d' % i, (w + (0.5 * r['draws'] if self.args.use_draws_for_winrate else 0)) / n, iteration)
            self.writer.add_scalar('win_rate/draws', r['draws'] / n, iteration)
            self.writer.add_scalar('win_rate/avg_game_length', r['avg_game_length'], iteration)
            _state(self, 'STANDBY')

        def killSelfPlayAgents(self):                                # Coach.py:401-435
            _state(self, 'KILL_AGENTS')
            self._azg_net = None
            self.agents = []
            _state(self, 'STANDBY')

        def learn(self):
            try:
                return Coach.learn(self)
            finally:
                it_mod.lead('stop', getattr(self, '_azg_game', None), [], self.args)   # the serving ranks return from serve()

    NativeCoach.__name__ = NativeCoach.__qualname__ = 'Native' + Coach.__name__
    if install_arena and hasattr(cmod, 'Arena'):
        cmod.Arena = native_arena(cmod.Arena, device=device, raw_seats=raw_seats, tree_free_seats=tree_free_seats, scripted_seats=scripted_seats)
    return NativeCoach


def is_raw_player(p):
    """the reference's RawMCTSPlayer itself (recognised by module and class name, like the env classes; a subclass or an instance with
    its own `process` is not): its batched evaluation is constant (GenericPlayers.py:198-200), so the engine plays it as a raw seat"""
    t = type(p)
    return t.__name__ == 'RawMCTSPlayer' and t.__module__.rsplit('.', 1)[-1] == 'GenericPlayers' and 'process' not in vars(p)


def tree_free_kind(p):
    """'random' / 'policy' for the reference's RandomPlayer / NNPlayer themselves (GenericPlayers.py:47-97; recognised like is_raw_player:
    module and class name, no `play` of the instance's own), else None: players whose move needs no tree, played on the device by
    games.DeviceGames.choose"""
    t = type(p)
    if t.__module__.rsplit('.', 1)[-1] != 'GenericPlayers' or 'play' in vars(p):
        return None
    return {'RandomPlayer': 'random', 'NNPlayer': 'policy'}.get(t.__name__)


# the reference's scripted baseline players: (env package, module, class) -> the game id they belong to
_SCRIPTED_PLAYERS = {('connect4', 'players', 'OneStepLookaheadConnect4Player'): 0, ('othello', 'OthelloPlayers', 'GreedyOthelloPlayer'): 3,
                     ('gobang', 'GobangPlayers', 'GreedyGobangPlayer'): 4}


def is_scripted_player(p, game_cls):
    """the reference's OneStepLookaheadConnect4Player / GreedyOthelloPlayer / GreedyGobangPlayer themselves (envs/connect4/players.py:26-69,
    envs/othello/OthelloPlayers.py:27-40, envs/gobang/GobangPlayers.py:27-40; recognised like tree_free_kind: module and class name, no
    `play` of the instance's own) in an arena of THEIR game: played on the device by games.DeviceGames.choose_scripted"""
    from .Game import azg_game_id
    t = type(p)
    gid = _SCRIPTED_PLAYERS.get(tuple(t.__module__.split('.')[-2:]) + (t.__name__,))
    return gid is not None and 'play' not in vars(p) and has_device_rules(game_cls) and azg_game_id(game_cls) == gid


def native_arena(Arena, *, device=None, raw_seats=True, tree_free_seats=False, scripted_seats=False):
    """class factory: the reference's Arena whose batched play_games runs on the device when it can (every player carries a model `.nn`
    or is a RawMCTSPlayer -- a raw seat; raw_seats=False: such arenas fall through --, Arena was built with use_batched_mcts, the game has
    device rules); anything else falls through to the reference's own code.
    tree_free_seats=True (opt-in) widens that: RandomPlayer and NNPlayer are seated too (selfplay.RANDOM_SEAT / PolicySeat) next to
    MCTSPlayer and RawMCTSPlayer, and an Arena built with use_batched_mcts=False -- what Coach.compareToBaseline builds for a
    RandomPlayer (Coach.py:577) -- takes the device path as well.  The MCTS seats then play with the BATCHED arena's settings
    (args.arenaTemp, no root noise / temperature, trees re-rooted every move), not MCTSPlayer.play's own startTemp schedule and
    args.add_root_*: INTEGRATION.md section 3a.
    scripted_seats=True (opt-in) seats the scripted baseline players of connect4, othello and gobang (is_scripted_player) as
    selfplay.SCRIPTED_SEAT under the same conditions; with it off such an arena falls through to the reference."""
    if getattr(Arena, '_azg_native', False):
        if (Arena._azg_raw_seats, Arena._azg_tree_free, Arena._azg_scripted) == (raw_seats, tree_free_seats, scripted_seats):
            return Arena
        Arena = Arena._azg_base                                      # (another choice of seats: wrap the reference's class afresh)

    class NativeArena(Arena):
        _azg_native = True
        _azg_raw_seats, _azg_tree_free, _azg_scripted, _azg_base = raw_seats, tree_free_seats, scripted_seats, Arena

        def _azg_seats(self, g):
            """the seats of an arena with RandomPlayer / NNPlayer / a scripted player in it, or None: not every player is one this path accepts"""
            from .selfplay import RANDOM_SEAT, SCRIPTED_SEAT, PolicySeat, is_tree_free
            cache, seats = _NetCache(g, device), []
            for p in self.players:
                kind, nn = tree_free_kind(p) if tree_free_seats else None, getattr(p, 'nn', None)
                if kind == 'random':
                    seats.append(RANDOM_SEAT)
                elif scripted_seats and is_scripted_player(p, self.game_cls):
                    seats.append(SCRIPTED_SEAT)
                elif kind == 'policy' and nn is not None:
                    a = getattr(p, 'args', None) or {}
                    seats.append(PolicySeat(cache.get(nn), a.get('startTemp'), a.get('temp_scaling_fn')))
                elif raw_seats and is_raw_player(p):
                    seats.append(None)
                elif nn is not None and type(p).__name__ == 'MCTSPlayer':
                    seats.append(cache.get(nn))
                else:
                    return None
            if not any(s is not None and not is_tree_free(s) for s in seats):
                return None                                          # (no network searched with MCTS: the engine has nothing to do)
            return seats

        def play_games(self, num, verbose=False, shuffle_players=True):          # Arena.pyx:188-376
            g = _ours(self.game_cls)
            if g is not None and (tree_free_seats and any(tree_free_kind(p) for p in self.players)
                                  or scripted_seats and any(is_scripted_player(p, self.game_cls) for p in self.players)):
                ours = self._azg_seats(g)
                if ours is None:
                    return Arena.play_games(self, num, verbose, shuffle_players)
                return self._azg_lead(g, ours, num, shuffle_players)
            nets = [getattr(p, 'nn', None) for p in self.players]
            raw = [n is None and raw_seats and is_raw_player(p) for p, n in zip(self.players, nets)]
            if not self.use_batched_mcts or g is None or all(raw) or any(n is None and not r for n, r in zip(nets, raw)):
                return Arena.play_games(self, num, verbose, shuffle_players)
            cache = _NetCache(g, device)
            ours = [None if r else cache.get(n) for n, r in zip(nets, raw)]     # (None: a raw seat)                      # (one wrapper per distinct reference net: [new] + [past] * (P - 1))
            return self._azg_lead(g, ours, num, shuffle_players)

        def _azg_lead(self, g, ours, num, shuffle_players):
            self.total_games = num
            r = it_mod.lead('arena', g, ours, self.args, num_games=num, details=True,
                            seats='slot' if shuffle_players else 'agent', stop=self.stop_event.is_set)
            self.draws, self.games_played = r['draws'], r['games']
            stats = getattr(self, '_Arena__player_stats', None)      # (so that wins() / winrates() answer afterwards, :133-137)
            if stats is not None:
                for s, w, wr in zip(stats, r['wins'], r['winrates']):
                    s.wins, s.winrate = w, wr
            return r['wins'], r['draws'], r['winrates']

    NativeArena.__name__ = NativeArena.__qualname__ = 'Native' + Arena.__name__
    return NativeArena
