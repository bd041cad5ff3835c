"""Host-side helpers mirroring alphazero/utils.py of the reference (dotdict, temperature schedules)."""
import numpy as np


class dotdict(dict):
    """alphazero/utils.py:1-12"""

    def __getattr__(self, name):
        if name.startswith('__'):
            raise AttributeError
        return self[name]

    def __setattr__(self, key, value):
        self[key] = value

    def copy(self):
        return self.__class__(super().copy())


def scale_temp(scale_factor, min_temp, cur_temp, turns, const_max_turns):
    """alphazero/utils.py:19-23: halve every int(scale_factor * max_turns) turns down to min_temp."""
    if const_max_turns and (turns + 1) % int(scale_factor * const_max_turns) == 0:
        return max(min_temp, cur_temp / 2)
    return cur_temp


def default_temp_scaling(*args, **kwargs):
    """alphazero/utils.py:26-27"""
    return scale_temp(0.15, 0.2, *args, **kwargs)


def const_temp_scaling(temp, *args, **kwargs):
    """alphazero/utils.py:30-31"""
    return temp


def temp_table(temp_fn, start_temp, max_turns, turns=None):
    """temp_by_turn[t]: the temperature SelfPlayAgent.playMoves uses for the move made at turn t, i.e.
    args.temp_scaling_fn iterated from args.startTemp (alphazero/SelfPlayAgent.pyx:156-157).  The callable is
    evaluated on the host once; the device indexes the table.  `max_turns` is what the game's CLASS reports and the
    callable receives -- None for a game without a turn limit, where the default schedule never steps; `turns`
    (default: max_turns) is how many turns the table covers."""
    out, t = [], float(start_temp)
    for turn in range(max(int(turns or max_turns or 0), 1) + 2):
        t = temp_fn(t, turn, max_turns)
        out.append(t)
    return np.asarray(out, dtype=np.float32)


def seat_temp_table(temp_fn, start_temp, max_turns, num_players, turns=None):
    """temp[p][t]: the temperature a PLAYER object seated as player p uses for a move it makes at turn t (NNPlayer.play,
    GenericPlayers.py:73: self.temp = temp_scaling_fn(self.temp, state.turns, max_turns) on ITS OWN moves only, from args.startTemp) --
    player p moves at the turns t with t % num_players == p; the entries of the other turns hold the value the player carries then.
    `max_turns` / `turns` as temp_table."""
    n = max(int(turns or max_turns or 0), 1) + 2
    out = np.zeros((int(num_players), n), np.float32)
    for p in range(int(num_players)):
        t = float(start_temp)
        for turn in range(n):
            if turn % int(num_players) == p:
                t = temp_fn(t, turn, max_turns)
            out[p, turn] = t
    return out


AGENT_STREAM = 0x4000000000000000   # tape stream of agent-level draws (fast coin, seat shuffle); DESIGN.md
TREEFREE_STREAM = 0x2000000000000000   # ... of the np.random.choice uniforms of tree-free arena seats: + global slot id, counter = round
TREEFREE_SEED_XOR = 0x7F4EE5EA7


# Searches that use no network -- MCTS.raw_search (RawMCTSPlayer) and the rounds of a warm-up agent -- can run their whole simulation
# loop as ONE launch (azg_search_raw).  A caller takes that form BY DEFAULT only where tools/raw_search_throughput.py measured it faster
# than the launch-per-phase form of the commit before it by more than the spread of the repeats, at EVERY (game, slots) size listed for
# that caller; otherwise it stays opt-in (SelfPlayRunner(fused_search=True)).  The numbers: profiles/raw_search_throughput.json,
# DESIGN.md "Network-free searches in one launch".
RAW_LAUNCH = {
    # (MCTS.raw_search has no other form left: the entry records that the rule was met, and at which sizes)
    'raw_search': dict(default=True, sizes=[('connect4', 1), ('brandubh', 1)]),                         # ms per MCTS.raw_search(g, 100) move
    'warmup': dict(default=False, sizes=[(g, b) for g in ('connect4', 'brandubh') for b in (128, 512, 2048)]),   # ms per round, numWarmupSims = 5
}


def raw_launch_default(caller):
    """does `caller` ('raw_search' or 'warmup') run its network-free simulations as one azg_search_raw launch unless told otherwise?"""
    return bool(RAW_LAUNCH[caller]['default'])
