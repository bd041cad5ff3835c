"""Host replay of self-play sample emission: SelfPlayAgent.playMoves (SelfPlayAgent.pyx:153-200) restated in plain numpy on
the package's host envs (alphazero_general_amd/envs/*).

Given what a self-play agent searched and played -- per round the `fast` flag, the root visit counts [B, A] and the sampled
actions [B] -- `replay` rebuilds the reference's output_queue (observation, pi, winstate) and result_queue (winstate, turns)
in order.  It never asks the engine, the C oracle or the device's symmetry tables: the samples are the host env's own
`symmetries(pi)` in list order, or the raw `(state, pi)` when symmetricSamples is off.
"""
import numpy as np

from alphazero_general_amd.envs import brandubh, connect4, gobang, othello, trimok

GAMES = {0: connect4.Game, 1: brandubh.Game, 2: trimok.Game, 3: othello.Game, 4: gobang.Game}     # include/azg.h game ids


def probs_t1(counts):
    """MCTS.probs(gs) at its default temperature 1 (MCTS.pyx:309,320-322), the float32 expression of the reference"""
    c = np.asarray(counts, np.float32)
    p = (c / np.sum(c)) ** 1.0
    p /= np.sum(p)
    return p


def samples_of(state, pi, symmetric):
    """the (state, pi) pairs one history entry contributes (SelfPlayAgent.pyx:186-190)"""
    return state.symmetries(pi) if symmetric else ((state, pi),)


def replay(game_cls, B, games_per_iteration, symmetric, counts, actions, fast=None, counted=None):
    """counts[r, i, :], actions[r, i]: round r of slot i; fast[r]: round r was a fast search (no history entry);
    counted[r, i]: the advance_commit form -- whether a game that finished in round r, slot i is counted, in place of the
    games_played < gamesPerIteration test.  Returns the two queues as arrays (r_slot: the slot of each result) plus
    games_played after every round."""
    R = len(actions)
    games = [game_cls() for _ in range(B)]
    hist = [[] for _ in range(B)]
    gp = 0
    s_obs, s_pi, s_z, r_ws, r_turns, r_slot, played = [], [], [], [], [], [], []
    for r in range(R):
        for i in range(B):                                                   # :154 slot order
            a = int(actions[r][i])
            if not (fast is not None and fast[r]):                           # :161-165
                hist[i].append((games[i].clone(), probs_t1(counts[r][i])))
            games[i].play_action(a)                                          # :171
            ws = np.asarray(games[i].win_state())                            # :176
            if not ws.any():
                continue
            r_ws.append(ws.astype(np.uint8)); r_turns.append(games[i].turns); r_slot.append(i)   # :178
            ok = bool(counted[r][i]) if counted is not None else gp < games_per_iteration
            if not ok:                                                       # :181-183
                continue
            gp += 1
            z = np.array(ws, dtype=np.float32)
            for st, pi in hist[i]:                                           # :184-196
                for s2, p2 in samples_of(st, pi, symmetric):
                    s_obs.append(np.asarray(s2.observation(), np.float32)); s_pi.append(np.asarray(p2, np.float32)); s_z.append(z)
            games[i] = game_cls()                                            # :197-200
            hist[i] = []
        played.append(gp)
    C, H, W = game_cls.observation_size()
    A, NV = game_cls.action_size(), game_cls.num_players() + 1
    return dict(s_obs=np.array(s_obs, np.float32).reshape(len(s_obs), C, H, W),
                s_pi=np.array(s_pi, np.float32).reshape(len(s_pi), A),
                s_z=np.array(s_z, np.float32).reshape(len(s_z), NV),
                r_ws=np.array(r_ws, np.uint8).reshape(len(r_ws), NV),
                r_turns=np.array(r_turns, np.int32), r_slot=np.array(r_slot, np.int32),
                games_played=np.array(played, np.int32))
