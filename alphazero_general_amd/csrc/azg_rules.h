// azg_rules.h -- the game rules of azg_games.h on plain arrays of positions, no engine and no tree: the batched form of the reference's
// GameState plugin (alphazero/Game.py:7-113: valid_moves, play_action, win_state, observation, symmetries).  One wavefront per position
// (k_game_step) or per (position, symmetry) (k_game_symmetries), one workgroup each, so a launch of `count` positions is a grid of `count`.
//
// Nothing a caller hands over becomes an address unchecked: an action is played only after it was found in the position's own move list
// (whose entries the rule structs form from lane and cell numbers, never from cell values), every scattered index is compared with A first,
// and every output row is addressed by the position's number alone.  A board outside the contract of azg_set_states gives a wrong answer.
#pragma once
#include "azg_games.h"

namespace azg {

// GameState.play_action (Game.py:82-85) of actions[i] on states[i] when the action is in valid_moves() -- status 1 and the position
// unchanged otherwise, -1: no move -- then, of the position that results: the azg_state, valid_moves() (Game.py:45-47) as a 0/1 row of A
// bytes, win_state() (Game.py:87-93) as P + 1 bytes, observation() (Game.py:96-98) in the format of k_select.  Null outputs are skipped.
template <class G, typename OT, bool NHWC8>
__global__ __launch_bounds__(64) void k_game_step(int count, const azg_state *states, const int32_t *actions, azg_state *next, uint8_t *valid,
                                                  uint8_t *win, OT *obs, int32_t *status) {
    constexpr int A = G::A, NV = G::P + 1, NCH = (G::MAXK + 63) / 64;
    __shared__ int act_lds[NCH * 64];
    __shared__ uint8_t mask_lds[(A + 63) / 64 * 64];
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= count) return;
    typename G::S s = G::load(&states[i], lane);
    if (actions) {
        const int a = __builtin_amdgcn_readfirstlane(actions[i]);
        int st = 0;
        if (a != -1) {
            bool hit = false;
            if (a >= 0 && a < A) {                                           // membership in the move list: play_action itself checks nothing
                int my_a[NCH];
                const int k = G::valid_list(s, lane, act_lds, my_a);
#pragma unroll
                for (int c = 0; c < NCH; c++) hit = hit || (c * 64 + lane < k && my_a[c] == a);
            }
            if (__ballot(hit) != 0) G::play(s, a); else st = 1;
        }
        if (status && lane == 0) status[i] = st;
    }
    if (next) G::store(s, &next[i], lane);                                   // (next may be states: the position is in registers)
    if (valid) {
        int my_a[NCH];
        const int k = G::valid_list(s, lane, act_lds, my_a);
        for (int e = lane; e < A; e += 64) mask_lds[e] = 0;
        wave_sync();
#pragma unroll
        for (int c = 0; c < NCH; c++) if (c * 64 + lane < k && (unsigned)my_a[c] < (unsigned)A) mask_lds[my_a[c]] = 1;
        wave_sync();
        uint8_t *row = valid + (size_t)i * A;
        for (int e = lane; e < A; e += 64) row[e] = mask_lds[e];
    }
    if (win) {
        const int ws = G::win_bits(s);                                       // (every lane: the tafl games ballot)
        if (lane < NV) win[(size_t)i * NV + lane] = (uint8_t)((ws >> lane) & 1);
    }
    if (obs) {
        if constexpr (NHWC8) G::write_obs_nhwc8(s, (_Float16 *)obs + (size_t)i * G::CELLS * 8, lane);
        else G::template write_obs<OT>(s, obs + (size_t)i * G::OBS, lane);
    }
}

// The move of a player without a tree on states[i] (alphazero/GenericPlayers.py), given the uniform u[i] its np.random.choice draws:
//   policy == NULL  RandomPlayer.play (:47-52): p = valids / np.sum(valids), uint8 / uint64 -> float64, so 1.0 / k in double on each of
//                   the k valid actions;
//   policy != NULL  NNPlayer.play (:69-94) on row i of policy[count, A] at temperature temp[i] (NULL: 1): options = policy * valids in
//                   float32 (:72), then the one-hot of np.argmax (:74-77) or x ** (1 / temp) / np.sum (:79-80) -- temper_probs, the
//                   arithmetic MCTS.probs ends with.
// Then np.random.choice (:51, :82): choice_draw, the draw of k_play.  status 0 and the action; status 1 and action -1 where the reference
// divides by zero or asserts: no valid move, options that sum to 0 or to no finite number, or -- outside the contract: negative or NaN
// policy entries, u outside [0, 1) -- a draw that did not land on a valid action with a positive option.  win_state is not consulted.
template <class G>
__global__ __launch_bounds__(64) void k_game_choose(int count, const azg_state *states, const float *policy, const float *temp, const double *u,
                                                    int32_t *actions, int32_t *status) {
    constexpr int A = G::A, NCH = (G::MAXK + 63) / 64, AL = A < 8 ? 8 : A;
    __shared__ int act_lds[NCH * 64];
    __shared__ float opt[AL], pr[AL], scr[64];
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= count) return;
    typename G::S s = G::load(&states[i], lane);
    int my_a[NCH];
    const int k = G::valid_list(s, lane, act_lds, my_a);
    for (int e = lane; e < A; e += 64) opt[e] = 0.f;
    wave_sync();
    const float *row = policy ? policy + (size_t)i * A : nullptr;           // (an action indexes the row and LDS only after it compared below A)
#pragma unroll
    for (int c = 0; c < NCH; c++)
        if (c * 64 + lane < k && (unsigned)my_a[c] < (unsigned)A) opt[my_a[c]] = row ? row[my_a[c]] : 1.f;
    wave_sync();
    const double ud = u[i];
    int action = -1;
    if (k > 0) {
        if (!policy) action = choice_draw<A, true>(opt, ud, 1.0 / (double)k);
        else {
            const float sum = temper_probs<A>(opt, temp ? temp[i] : 1.f, pr, scr, lane);
            if (sum > 0.f && sum <= 3.402823466e38f) action = choice_draw<A>(pr, ud);   // (0, a negative sum, inf, NaN: :80 divides by it)
        }
        if (action >= 0 && !(opt[action] > 0.f)) action = -1;
    }
    if (lane == 0) { actions[i] = action; status[i] = action < 0 ? 1 : 0; }
}

// The children of states[i]: entry j < k of the position's own move list (valid_list: ascending, k clamped to MAXK) played with
// G::play on a copy of the position, for j in the chunk blockIdx.y of 64 entries.  A position lives in the registers of one wavefront,
// so a wavefront plays its children one after the other and the grid spreads them: (position, chunk), every wavefront rebuilding the
// list (in act_lds, whatever the game's valid_list keeps there).  The games of at most 64 children are one wavefront per position.
// num[i] = k; child_actions[i, j] the action, -1 from k on; of child j < k, where the pointer is given: win[i, j, 0:P+1], children[i, j],
// obs[i, j] as k_game_step writes them.  Rows from k on are left alone.  The parent's win_state is not consulted (play_action does not).
// An entry of the list indexes nothing but a register compare: it is played only when it lies in [0, A).
template <class G, typename OT, bool NHWC8>
__global__ __launch_bounds__(64) void k_game_lookahead(int count, const azg_state *states, int32_t *num, int32_t *child_actions, uint8_t *win,
                                                       azg_state *children, OT *obs) {
    constexpr int A = G::A, NV = G::P + 1, MAXK = G::MAXK, NCH = (MAXK + 63) / 64;
    __shared__ int act_lds[NCH * 64];
    const int i = blockIdx.x, chunk = blockIdx.y, lane = threadIdx.x;
    if (i >= count || chunk >= NCH) return;
    const typename G::S s = G::load(&states[i], lane);
    int my_a[NCH];
    int k = G::valid_list(s, lane, act_lds, my_a);
    k = k < 0 ? 0 : k > MAXK ? MAXK : k;
    wave_sync();
#pragma unroll
    for (int c = 0; c < NCH; c++) act_lds[c * 64 + lane] = c * 64 + lane < k ? my_a[c] : -1;
    wave_sync();
    if (chunk == 0 && lane == 0) num[i] = k;
    const int j0 = chunk * 64;
    if (j0 + lane < MAXK) child_actions[(size_t)i * MAXK + j0 + lane] = act_lds[j0 + lane];
    const int j1 = k < j0 + 64 ? k : j0 + 64;
    for (int j = j0; j < j1; j++) {
        const int a = __builtin_amdgcn_readfirstlane(act_lds[j]);
        if ((unsigned)a >= (unsigned)A) continue;
        typename G::S t = s;
        G::play(t, a);
        const size_t o = (size_t)i * MAXK + j;
        if (children) G::store(t, &children[o], lane);
        if (win) {
            const int ws = G::win_bits(t);                                   // (every lane: the tafl games ballot)
            if (lane < NV) win[o * NV + lane] = (uint8_t)((ws >> lane) & 1);
        }
        if (obs) {
            if constexpr (NHWC8) G::write_obs_nhwc8(t, (_Float16 *)obs + o * G::CELLS * 8, lane);
            else G::template write_obs<OT>(t, obs + o * G::OBS, lane);
        }
    }
}

// The reference's scripted baseline player of the game (G::SCRIPTED) on states[i], one wavefront per position: every entry of the move
// list is played on a copy and given G::scripted_key(parent, child); the move is the lowest action of the smallest key, or -- with
// G::SCRIPTED_DRAWS, np.random.choice(list(set)) without p -- entry min(m - 1, (int)(u[i] * m)) of the m moves of the smallest key in
// ascending order.  status 1 and action -1 without a valid move (the reference raises).  win_state of the parent is not consulted.
template <class G>
__global__ __launch_bounds__(64) void k_game_choose_scripted(int count, const azg_state *states, const double *u, int32_t *actions,
                                                             int32_t *status) {
    constexpr int A = G::A, MAXK = G::MAXK, NCH = (MAXK + 63) / 64;
    __shared__ int act_lds[NCH * 64];
    __shared__ int key_lds[G::SCRIPTED_DRAWS ? NCH * 64 : 1];
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= count) return;
    const typename G::S s = G::load(&states[i], lane);
    int my_a[NCH];
    int k = G::valid_list(s, lane, act_lds, my_a);
    k = k < 0 ? 0 : k > MAXK ? MAXK : k;
    wave_sync();
#pragma unroll
    for (int c = 0; c < NCH; c++) act_lds[c * 64 + lane] = c * 64 + lane < k ? my_a[c] : -1;
    wave_sync();
    int best = 0x7fffffff, best_a = -1, m = 0;                               // (wave-uniform: the smallest key, its first action, its count)
    for (int j = 0; j < k; j++) {
        const int a = __builtin_amdgcn_readfirstlane(act_lds[j]);
        if ((unsigned)a >= (unsigned)A) continue;
        typename G::S t = s;
        G::play(t, a);
        const int key = __builtin_amdgcn_readfirstlane(G::scripted_key(s, t));
        if (key < best) { best = key; best_a = a; m = 0; }
        if (key == best) m++;
        if constexpr (G::SCRIPTED_DRAWS) { if (lane == 0) key_lds[j] = key; }
    }
    if constexpr (G::SCRIPTED_DRAWS) {
        wave_sync();
        if (m > 1) {
            int idx = (int)(u[i] * (double)m);
            idx = idx < 0 ? 0 : idx > m - 1 ? m - 1 : idx;                   // (u outside [0, 1) or NaN is outside the contract: still a move of the set)
            for (int j = 0, seen = 0; j < k; j++) {
                const int a = __builtin_amdgcn_readfirstlane(act_lds[j]);
                if ((unsigned)a >= (unsigned)A || key_lds[j] != best) continue;
                if (seen++ == idx) { best_a = a; break; }
            }
        }
    }
    if (lane == 0) { actions[i] = best_a; status[i] = best_a < 0 ? 1 : 0; }
}

// GameState.symmetries(pi) (Game.py:100-113) of states[i], entry k = blockIdx.y of the reference's list: the arithmetic of k_emit_samples.
template <class G>
__global__ __launch_bounds__(64) void k_game_symmetries(int count, const azg_state *states, const float *pi, azg_state *sym_states,
                                                        float *sym_obs, float *sym_pi) {
    constexpr int A = G::A;
    const int i = blockIdx.x, k = blockIdx.y, lane = threadIdx.x;
    if (i >= count || k >= G::NSYM) return;
    const typename G::S s = G::load(&states[i], lane);
    const typename G::S ss = G::symmetry(s, k);
    const size_t o = (size_t)i * G::NSYM + k;
    if (sym_states) G::store(ss, &sym_states[o], lane);
    if (sym_obs) G::template write_obs<float>(ss, sym_obs + o * G::OBS, lane);
    if (pi && sym_pi) {
        for (int a = lane; a < A; a += 64) {
            const int t = G::sym_action(a, k);
            if ((unsigned)t < (unsigned)A) sym_pi[o * A + t] = pi[(size_t)i * A + a];
        }
    }
}

}  // namespace azg
