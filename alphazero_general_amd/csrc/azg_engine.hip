// azg_engine.hip -- host side of libazg_hip.so: the C ABI of include/azg.h over the kernels of azg_kernels.h.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -shared -fPIC  (alphazero_general_amd/build.py)
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>
#include "azg_kernels.h"
#include "azg_rules.h"
#include "azg_conv.h"
#include "azg_tiles.h"

using namespace azg;

static thread_local std::string g_err;
static int fail(int code, const std::string &msg) { g_err = msg; return code; }
#define HIPCHK(x) do { hipError_t _e = (x); if (_e != hipSuccess) return fail(AZG_E_HIP, std::string(#x) + ": " + hipGetErrorString(_e)); } while (0)

struct EvPair { hipEvent_t a, b; bool ext; };

// Timing of ONE kernel: while a profile hook is armed (g_kev), the next AZG_LAUNCH goes through hipExtLaunchKernelGGL, which stamps
// the pair's events with the dispatch's own begin / end timestamps -- the kernel's execution time as rocprofv3 reports it, without
// the ~2 us of marker packets that hipEventRecord brackets add to a 10 us kernel.
static thread_local EvPair *g_kev = nullptr;
#define AZG_LAUNCH(kernel, grid, block, lds, stream, ...) do { \
    if (g_kev) { hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, g_kev->a, g_kev->b, 0, __VA_ARGS__); g_kev = nullptr; } \
    else hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__); } while (0)

// One profile record (every engine has one: azg_profile_*; the network launches share one: azg_profile_net_*): per launch family the
// event pairs still in flight, the milliseconds and launches counted so far, and the idle pairs
struct Prof {
    bool on = false;
    std::vector<EvPair> ev[3], pool;
    double ms[3] = {0, 0, 0};
    int64_t n[3] = {0, 0, 0};
    EvPair take() {
        EvPair p{};
        if (!pool.empty()) { p = pool.back(); pool.pop_back(); }
        else { (void)hipEventCreate(&p.a); (void)hipEventCreate(&p.b); }
        return p;
    }
    void done(int fam, const EvPair &p) { ev[fam].push_back(p); n[fam]++; }
    void drain() {
        for (int f = 0; f < 3; f++) {
            for (auto &p : ev[f]) {
                (void)hipEventSynchronize(p.b);
                float t = 0; (void)hipEventElapsedTime(&t, p.a, p.b);
                ms[f] += t;
                pool.push_back(p);
            }
            ev[f].clear();
        }
    }
    void enable(bool v) { drain(); on = v; if (v) for (int f = 0; f < 3; f++) { ms[f] = 0; n[f] = 0; } }
    void read(double *ms3, int64_t *launches3) { drain(); for (int f = 0; f < 3; f++) { ms3[f] = ms[f]; launches3[f] = n[f]; } }
};

// One timed region of family `fam`, open for as long as the object lives.  one_kernel: the region is ONE AZG_LAUNCH, timed through g_kev;
// otherwise a sequence of launches between two event records.  However the region is left, g_kev is clear afterwards and the pair goes
// back: to the family's list if a launch took it (AZG_LAUNCH resets g_kev), to the pool -- nothing counted -- if none did.
class ProfScope {
    Prof *prof = nullptr; std::mutex *mu; hipStream_t s; int fam; EvPair p{};
    std::unique_lock<std::mutex> lock() const { return mu ? std::unique_lock<std::mutex>(*mu) : std::unique_lock<std::mutex>(); }
public:
    ProfScope(Prof &pr, std::mutex *mu_, hipStream_t s_, int fam_, bool one_kernel = true, bool enabled = true) : mu(mu_), s(s_), fam(fam_) {
        if (!enabled) return;
        { auto lk = lock(); if (!pr.on) return; p = pr.take(); }
        prof = &pr; p.ext = one_kernel;
        if (p.ext) g_kev = &p; else (void)hipEventRecord(p.a, s);
    }
    ~ProfScope() {
        if (!prof) return;
        const bool launched = !p.ext || g_kev != &p;
        if (!p.ext) (void)hipEventRecord(p.b, s);
        g_kev = nullptr;
        auto lk = lock();
        if (launched) prof->done(fam, p); else prof->pool.push_back(p);
    }
    ProfScope(const ProfScope &) = delete;
    ProfScope &operator=(const ProfScope &) = delete;
};

struct azg_engine {
    azg_config cfg;
    azg_game_info gi;
    View v;
    std::vector<void *> allocs;
    int32_t *d_p2i = nullptr, *d_ok = nullptr;
    int16_t *d_perm = nullptr;                                 // azg_set_shuffle_tape / azg_set_random_tape
    double *d_utape = nullptr; int32_t *d_noff = nullptr; float *d_npool = nullptr;
    Prof prof;
};

// the game table and everything else per game below: expanded from the one list of rule structs (AZG_GAMES, azg_games.h)
#define AZG_GAME_INFO(G, ...) {G::A, G::OBS_C, G::H, G::W, G::P, G::HAS_DRAW, G::MAX_TURNS, G::NSYM, G::CELLS, G::MAXK},
static const azg_game_info k_info[] = {AZG_GAMES(AZG_GAME_INFO)};   // action_size, c,h,w, players, has_draw, max_turns, nsym, cells, max_children
#define AZG_GAME_ID(G, ...) G::ID,
static constexpr int k_game_ids[] = {AZG_GAMES(AZG_GAME_ID)};
static constexpr int k_num_games = sizeof(k_game_ids) / sizeof(k_game_ids[0]);
static constexpr bool game_ids_in_order() { for (int i = 0; i < k_num_games; i++) if (k_game_ids[i] != i) return false; return true; }
static_assert(game_ids_in_order(), "AZG_GAMES lists the rule structs in id order: each struct's ID is its position");

extern "C" int azg_abi_version(void) { return AZG_ABI_VERSION; }
#ifndef AZG_SRC_SHA
#define AZG_SRC_SHA "unstamped"
#endif
extern "C" const char *azg_source_sha(void) { return AZG_SRC_SHA; }
extern "C" const char *azg_last_error(void) { return g_err.c_str(); }
extern "C" int azg_game_info_get(int game, azg_game_info *out) {
    if (game < 0 || game >= k_num_games || !out) return fail(AZG_E_INVALID_ARG, "unknown game id");
    *out = k_info[game];
    return AZG_OK;
}
extern "C" int azg_device_count(void) { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) return 0; return n; }

extern "C" uint64_t azg_tape_u64(uint64_t seed, uint64_t stream, uint64_t ctr) { return tape_u64(seed, stream, ctr); }
extern "C" double azg_tape_uniform(uint64_t seed, uint64_t stream, uint64_t ctr) { return u53(tape_u64(seed, stream, ctr)); }
extern "C" void azg_tape_shuffle_pos(uint64_t seed, uint64_t stream, uint64_t ctr, int k, int32_t *pos) {
    std::vector<uint64_t> key((size_t)k);
    for (int i = 0; i < k; i++) key[i] = tape_u64(seed, stream, ctr + (uint64_t)i);
    for (int i = 0; i < k; i++) {
        int r = 0;
        for (int j = 0; j < k; j++) r += (key[j] < key[i]) || (key[j] == key[i] && j < i);
        pos[i] = r;
    }
}

template <typename T> static int dalloc(azg_engine *e, T **p, size_t count) {
    void *q = nullptr;
    size_t bytes = count * sizeof(T);
    if (bytes == 0) bytes = 16;
    HIPCHK(hipMalloc(&q, bytes));
    HIPCHK(hipMemset(q, 0, bytes));
    e->allocs.push_back(q);
    *p = (T *)q;
    return AZG_OK;
}
#define DALLOC(ptr, count) do { int _r = dalloc(e, &(ptr), (size_t)(count)); if (_r != AZG_OK) return _r; } while (0)

// dispatch a templated kernel launch on the game id: CALL sees the rule struct as G
#define AZG_GAME_CASE(G_, ...) case G_::ID: { using G = G_; __VA_ARGS__; } break;
#define GAME_SWITCH(e, ...) \
    switch ((e)->cfg.game) { AZG_GAMES(AZG_GAME_CASE, __VA_ARGS__) default: return fail(AZG_E_UNSUPPORTED, "game has no device rules"); }
// the same for the sparse heads (head features -> logits of the leaf's children only): the games without them (G::SPARSE_HEADS says
// why) are refused by name
#define AZG_SPARSE_CASE(G_, ...) case G_::ID: if constexpr (G_::SPARSE_HEADS) { using G = G_; __VA_ARGS__; } \
    else return fail(AZG_E_UNSUPPORTED, std::string("no sparse heads for ") + G_::NAME + " (use the dense heads)"); break;
#define SPARSE_GAME_SWITCH(e, ...) \
    switch ((e)->cfg.game) { AZG_GAMES(AZG_SPARSE_CASE, __VA_ARGS__) default: return fail(AZG_E_UNSUPPORTED, "game has no device rules"); }
// dispatch on the observation format the tree kernels write (obs_dtype 0: f32 planes, 1: f16 planes, 2: f16 NHWC8 rows): CALL sees the
// element type OBS, the flag NHWC8 and the buffer as OBS *o
#define OBS_SWITCH(obs_dtype, obs, CALL) \
    if ((obs_dtype) == 0) { using OBS = float; constexpr bool NHWC8 = false; OBS *const o = (OBS *)(obs); CALL; } \
    else if ((obs_dtype) == 1) { using OBS = _Float16; constexpr bool NHWC8 = false; OBS *const o = (OBS *)(obs); CALL; } \
    else { using OBS = _Float16; constexpr bool NHWC8 = true; OBS *const o = (OBS *)(obs); CALL; }

extern "C" int azg_engine_create(const azg_config *cfg, azg_engine **out) {
    if (!cfg || !out) return fail(AZG_E_INVALID_ARG, "null argument");
    if (cfg->abi_version != AZG_ABI_VERSION) return fail(AZG_E_INVALID_ARG, "ABI version mismatch");
    if (cfg->game < 0 || cfg->game >= k_num_games) return fail(AZG_E_UNSUPPORTED, "game has no device rules");
    if (cfg->num_slots <= 0) return fail(AZG_E_INVALID_ARG, "num_slots must be > 0");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(AZG_E_HIP, "no HIP device: libazg_hip has no CPU fallback");
    HIPCHK(hipSetDevice(cfg->device));
    azg_engine *e = new azg_engine();
    e->cfg = *cfg; e->gi = k_info[cfg->game];
    const azg_game_info &gi = e->gi;
    View &v = e->v;
    memset(&v, 0, sizeof(v));
    v.B = cfg->num_slots; v.arena = cfg->arena ? 1 : 0; v.T = v.arena ? gi.num_players : 1;
    // node store: two semi-spaces of `cap` nodes per tree (k_compact).  A move adds at most sims_per_move * max_children nodes to
    // the live space, and the space is compacted after a move once fewer than one move's worth of free nodes is left.  A search
    // that carries a fraction f of its visits into the played move keeps about f / (1 - f) moves' worth of nodes across moves:
    // the default capacity holds min(max_turns, 16) moves' worth (f up to 0.94 sustained; random-init nets keep 0.2-0.5 of ONE
    // move's worth), the worst case -- a game that never drops a sibling -- needs max_turns, which nodes_per_tree can ask for.
    // Overflow is loud: the sticky AZG_E_TREE_FULL
    const int sims = cfg->sims_per_move > 0 ? cfg->sims_per_move : 100;
    const long long per_move = (long long)sims * gi.max_children;
    const long long cap = cfg->nodes_per_tree > 0 ? cfg->nodes_per_tree : (long long)(gi.max_turns < 16 ? gi.max_turns : 16) * per_move + 64;
    if (cap >= (1 << 28)) { delete e; return fail(AZG_E_INVALID_ARG, "nodes_per_tree must be < 2^28"); }
    v.cap = (int)cap;
    v.compact_reserve = (int)(per_move < cap / 2 ? per_move : cap / 2);
    v.maxd = gi.max_turns + 2; v.max_hist = gi.max_turns + 1;
    v.ex_cap = cfg->example_capacity; v.res_cap = cfg->result_capacity > 0 ? cfg->result_capacity : 4 * v.B + 1024;
    v.add_noise = (cfg->add_root_noise && !v.arena) ? 1 : 0; v.add_temp = (cfg->add_root_temp && !v.arena) ? 1 : 0;
    v.symmetric = cfg->symmetric_samples; v.reset_thr = cfg->mcts_reset_threshold; v.games_cap = cfg->games_per_iteration;
    v.cpuct = cfg->cpuct; v.fpu_reduction = cfg->fpu_reduction; v.noise_frac = cfg->root_noise_frac;
    v.root_temp = cfg->root_policy_temp; v.arena_temp = cfg->arena_temp;
    v.seed = cfg->tape_seed; v.slot_base = cfg->slot_base;
    const size_t trees = (size_t)v.B * v.T;
    const int A = gi.action_size, NV = gi.num_players + 1, O = gi.obs_c * gi.obs_h * gi.obs_w;
    DALLOC(v.nodes, trees * 2 * (size_t)v.cap);
    DALLOC(v.hdr, trees);
    DALLOC(v.path, trees * (size_t)v.maxd);
    DALLOC(v.states, v.B); DALLOC(v.leaf_states, v.B);
    DALLOC(v.tape_ctr, v.B); DALLOC(v.next_reset, v.B); DALLOC(v.hist_len, v.B);
    const bool hist = !v.arena && v.ex_cap > 0;
    DALLOC(v.hist_state, hist ? (size_t)v.B * v.max_hist : 1);
    DALLOC(v.hist_pi, hist ? (size_t)v.B * v.max_hist * A : 1);
    if (!hist) v.max_hist = 0;
    DALLOC(v.last_action, v.B); DALLOC(v.fin_flag, v.B); DALLOC(v.fin_ridx, v.B); DALLOC(v.fin_counted, v.B); DALLOC(v.fin_soff, v.B);
    DALLOC(v.slot_sims, v.B); DALLOC(v.slot_exp, v.B);
    DALLOC(v.gcount, 8);
    DALLOC(v.ex_obs, (size_t)v.ex_cap * O); DALLOC(v.ex_pi, (size_t)v.ex_cap * A); DALLOC(v.ex_z, (size_t)v.ex_cap * NV);
    DALLOC(v.res_ws, (size_t)v.res_cap * NV); DALLOC(v.res_turns, v.res_cap); DALLOC(v.res_slot, v.res_cap);
    // temperature table (args.temp_scaling_fn iterated on the host)
    std::vector<float> tt;
    if (cfg->temp_table && cfg->temp_table_len > 0) tt.assign(cfg->temp_table, cfg->temp_table + cfg->temp_table_len);
    else tt.assign(1, cfg->start_temp);
    float *d_tt; DALLOC(d_tt, tt.size());
    HIPCHK(hipMemcpy(d_tt, tt.data(), tt.size() * sizeof(float), hipMemcpyHostToDevice));
    v.temp_table = d_tt; v.temp_len = (int)tt.size();
    DALLOC(e->d_p2i, 8); DALLOC(e->d_ok, 4);
#ifdef AZG_TREE_TIMING
    DALLOC(v.dbg, (size_t)v.B * 16);
#endif
    *out = e;
    int r = azg_engine_reset(e, nullptr);
    if (r != AZG_OK) { azg_engine_destroy(e); *out = nullptr; return r; }
    HIPCHK(hipDeviceSynchronize());
    return AZG_OK;
}

extern "C" int azg_engine_destroy(azg_engine *e) {
    if (!e) return AZG_OK;
    (void)hipDeviceSynchronize();
    e->prof.drain();
    for (auto &p : e->prof.pool) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
    for (void *p : e->allocs) (void)hipFree(p);
    if (e->d_perm) (void)hipFree(e->d_perm);
    if (e->d_utape) (void)hipFree(e->d_utape);
    if (e->d_noff) (void)hipFree(e->d_noff);
    if (e->d_npool) (void)hipFree(e->d_npool);
    delete e;
    return AZG_OK;
}

extern "C" int azg_engine_reset(azg_engine *e, void *stream) {
    if (!e) return fail(AZG_E_INVALID_ARG, "null engine");
    hipStream_t s = (hipStream_t)stream;
    GAME_SWITCH(e, hipLaunchKernelGGL((k_reset<G>), dim3(e->v.B), dim3(64), 0, s, e->v, 0, e->v.B, 1));
    HIPCHK(hipMemsetAsync(e->v.tape_ctr, 0, sizeof(uint64_t) * e->v.B, s));
    HIPCHK(hipMemsetAsync(e->v.gcount, 0, sizeof(int32_t) * 8, s));
    HIPCHK(hipMemsetAsync(e->v.slot_sims, 0, sizeof(int64_t) * e->v.B, s));
    HIPCHK(hipMemsetAsync(e->v.slot_exp, 0, sizeof(int64_t) * e->v.B, s));
    HIPCHK(hipGetLastError());
    return AZG_OK;
}

static int check_range(azg_engine *e, int first, int count) {
    if (!e) return fail(AZG_E_INVALID_ARG, "null engine");
    if (first < 0 || count < 0 || first + count > e->v.B) return fail(AZG_E_INVALID_ARG, "slot range out of bounds");
    return AZG_OK;
}

extern "C" int azg_set_states(azg_engine *e, void *stream, int first, int count, const azg_state *host, int reset_trees) {
    int r = check_range(e, first, count); if (r) return r;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemcpyAsync(e->v.states + first, host, sizeof(azg_state) * count, hipMemcpyHostToDevice, s));
    if (reset_trees) { GAME_SWITCH(e, hipLaunchKernelGGL((k_reset<G>), dim3(count), dim3(64), 0, s, e->v, first, count, 0)); }
    HIPCHK(hipStreamSynchronize(s));
    return AZG_OK;
}
extern "C" int azg_get_states(azg_engine *e, void *stream, int first, int count, azg_state *host) {
    int r = check_range(e, first, count); if (r) return r;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemcpyAsync(host, e->v.states + first, sizeof(azg_state) * count, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return AZG_OK;
}
extern "C" int azg_get_leaf_states(azg_engine *e, void *stream, int first, int count, azg_state *host) {
    int r = check_range(e, first, count); if (r) return r;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemcpyAsync(host, e->v.leaf_states + first, sizeof(azg_state) * count, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return AZG_OK;
}
extern "C" int azg_set_tape_counters(azg_engine *e, void *stream, int first, int count, const uint64_t *host) {
    int r = check_range(e, first, count); if (r) return r;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemcpyAsync(e->v.tape_ctr + first, host, sizeof(uint64_t) * count, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    return AZG_OK;
}
extern "C" int azg_get_tape_counters(azg_engine *e, void *stream, int first, int count, uint64_t *host) {
    int r = check_range(e, first, count); if (r) return r;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemcpyAsync(host, e->v.tape_ctr + first, sizeof(uint64_t) * count, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return AZG_OK;
}

extern "C" int azg_select(azg_engine *e, void *stream, void *obs, int obs_dtype, const int32_t *row_of_slot) {
    if (!e) return fail(AZG_E_INVALID_ARG, "null engine");
    if (obs_dtype < 0 || obs_dtype > 2) return fail(AZG_E_INVALID_ARG, "obs_dtype must be 0 (f32), 1 (f16) or 2 (f16 NHWC8)");
    hipStream_t s = (hipStream_t)stream;
    ProfScope timed(e->prof, nullptr, s, 0);
    OBS_SWITCH(obs_dtype, obs, GAME_SWITCH(e, AZG_LAUNCH((k_select<G, OBS, NHWC8>), dim3(e->v.B), dim3(64), 0, s, e->v, o, row_of_slot)));
    HIPCHK(hipGetLastError());
    return AZG_OK;
}

extern "C" int azg_arena_rows(azg_engine *e, void *stream, const int32_t *p2i_host, int32_t *row_of_slot, int32_t *rows_per_model) {
    if (!e || !p2i_host || !row_of_slot || !rows_per_model) return fail(AZG_E_INVALID_ARG, "null argument");
    hipStream_t s = (hipStream_t)stream;
    if (e->gi.num_players > 8) return fail(AZG_E_UNSUPPORTED, "more than 8 players");
    SeatMap seat{};
    for (int i = 0; i < e->gi.num_players; i++) seat.v[i] = p2i_host[i];
    hipLaunchKernelGGL(k_arena_rows, dim3(1), dim3(64), 0, s, e->v, seat, (const uint32_t *)nullptr, row_of_slot, rows_per_model);
    HIPCHK(hipGetLastError());
    return AZG_OK;
}

extern "C" int azg_arena_rows_seats(azg_engine *e, void *stream, const uint32_t *seat_of_slot, int32_t *row_of_slot, int32_t *rows_per_model) {
    if (!e || !seat_of_slot || !row_of_slot || !rows_per_model) return fail(AZG_E_INVALID_ARG, "null argument");
    if (e->gi.num_players > 8) return fail(AZG_E_UNSUPPORTED, "more than 8 players");
    hipLaunchKernelGGL(k_arena_rows, dim3(1), dim3(64), 0, (hipStream_t)stream, e->v, SeatMap{}, seat_of_slot, row_of_slot, rows_per_model);
    HIPCHK(hipGetLastError());
    return AZG_OK;
}

extern "C" int azg_backup(azg_engine *e, void *stream, const float *policy, const float *value, const int32_t *row_of_slot, int flags) {
    if (!e || !policy || !value) return fail(AZG_E_INVALID_ARG, "null argument");
    hipStream_t s = (hipStream_t)stream;
    View v = e->v;
    if (flags >= 0) { v.add_noise = (flags & AZG_FLAG_NOISE) ? 1 : 0; v.add_temp = (flags & AZG_FLAG_TEMP) ? 1 : 0; }
    ProfScope timed(e->prof, nullptr, s, 1);
    GAME_SWITCH(e, AZG_LAUNCH((k_backup<G>), dim3(e->v.B), dim3(64), 0, s, v, policy, value, row_of_slot));
    HIPCHK(hipGetLastError());
    return AZG_OK;
}

extern "C" int azg_search_raw(azg_engine *e, void *stream, float policy_fill, const float *value_host, int sims) {
    if (!e || !value_host || sims < 0) return fail(AZG_E_INVALID_ARG, "null or out-of-range argument");
    if (e->v.arena) return fail(AZG_E_UNSUPPORTED, "the network-free search launch is built for self-play engines (one tree per slot)");
    if (sims == 0) return AZG_OK;
    hipStream_t s = (hipStream_t)stream;
    GAME_SWITCH(e, {
        RawValueRow<G> vrow;                                    // both constant rows go by value: nothing of the caller's is read after the call
        for (int j = 0; j < G::P + 1; j++) vrow.v[j] = value_host[j];
        hipLaunchKernelGGL((k_search_raw<G>), dim3(e->v.B), dim3(64), 0, s, e->v, policy_fill, vrow, sims);
    });
    HIPCHK(hipGetLastError());
    return AZG_OK;
}

extern "C" int azg_backup_select(azg_engine *e, void *stream, const float *policy, const float *value, const int32_t *row_of_slot, int flags,
                                 void *obs, int obs_dtype) {
    if (!e || !policy || !value) return fail(AZG_E_INVALID_ARG, "null argument");
    if (obs_dtype < 0 || obs_dtype > 2) return fail(AZG_E_INVALID_ARG, "obs_dtype must be 0 (f32), 1 (f16) or 2 (f16 NHWC8)");
    hipStream_t s = (hipStream_t)stream;
    View v = e->v;
    if (flags >= 0) { v.add_noise = (flags & AZG_FLAG_NOISE) ? 1 : 0; v.add_temp = (flags & AZG_FLAG_TEMP) ? 1 : 0; }
    ProfScope timed(e->prof, nullptr, s, 1);
    const int A = e->gi.action_size;
    OBS_SWITCH(obs_dtype, obs, GAME_SWITCH(e, AZG_LAUNCH((k_backup_select2<G, OBS, NHWC8, IN_PROBS>), dim3(v.B), dim3(128), 0, s, v, policy, value, A, o, row_of_slot, 1, HeadRows{})));
    HIPCHK(hipGetLastError());
    return AZG_OK;
}

extern "C" int azg_backup_select_logits(azg_engine *e, void *stream, const float *logits, int logits_stride, const int32_t *row_of_slot,
                                        int flags, void *obs, int obs_dtype, int do_select) {
    if (!e || !logits) return fail(AZG_E_INVALID_ARG, "null argument");
    if (obs_dtype < 0 || obs_dtype > 2) return fail(AZG_E_INVALID_ARG, "obs_dtype must be 0 (f32), 1 (f16) or 2 (f16 NHWC8)");
    if (logits_stride < e->gi.action_size + e->gi.num_players + 1 || e->gi.action_size > 1024)
        return fail(AZG_E_INVALID_ARG, "logits_stride must hold A + P + 1 logits (A <= 1024)");
    hipStream_t s = (hipStream_t)stream;
    View v = e->v;
    if (flags >= 0) { v.add_noise = (flags & AZG_FLAG_NOISE) ? 1 : 0; v.add_temp = (flags & AZG_FLAG_TEMP) ? 1 : 0; }
    ProfScope timed(e->prof, nullptr, s, 1);
    const float *nov = nullptr;
    OBS_SWITCH(obs_dtype, obs, GAME_SWITCH(e, AZG_LAUNCH((k_backup_select2<G, OBS, NHWC8, IN_LOGITS>), dim3(v.B), dim3(128), 0, s, v, logits, nov, logits_stride, o, row_of_slot, do_select, HeadRows{})));
    HIPCHK(hipGetLastError());
    return AZG_OK;
}

extern "C" int azg_backup_select_features(azg_engine *e, void *stream, const void *feat, int feat_k, const void *head_rows, const float *head_b,
                                          const int32_t *row_of_slot, int flags, void *obs, int obs_dtype, int do_select) {
    if (!e || !feat || !head_rows || !head_b) return fail(AZG_E_INVALID_ARG, "null argument");
    if (obs_dtype < 0 || obs_dtype > 2) return fail(AZG_E_INVALID_ARG, "obs_dtype must be 0 (f32), 1 (f16) or 2 (f16 NHWC8)");
    if (e->gi.action_size > 1024) return fail(AZG_E_INVALID_ARG, "A <= 1024");
    hipStream_t s = (hipStream_t)stream;
    View v = e->v;
    if (flags >= 0) { v.add_noise = (flags & AZG_FLAG_NOISE) ? 1 : 0; v.add_temp = (flags & AZG_FLAG_TEMP) ? 1 : 0; }
    const HeadRows hd{(const _Float16 *)head_rows, head_b, feat_k};
    int want = 0;
    SPARSE_GAME_SWITCH(e, want = head_fk<G>());
    if (feat_k != want) return fail(AZG_E_INVALID_ARG, "feat_k must be cells x 16 rounded up to a multiple of 32 for this game");
    ProfScope timed(e->prof, nullptr, s, 1);
    const float *nov = nullptr, *f = (const float *)feat;
    OBS_SWITCH(obs_dtype, obs, SPARSE_GAME_SWITCH(e, AZG_LAUNCH((k_backup_select2<G, OBS, NHWC8, IN_FEATURES>), dim3(v.B), dim3(128), 0, s, v, f, nov, 0, o, row_of_slot, do_select, hd)));
    HIPCHK(hipGetLastError());
    return AZG_OK;
}

extern "C" int azg_leaf_heads_sparse_f16(azg_engine *e, void *stream, const void *feat, int feat_k, const void *head_rows, const float *head_b,
                                         const int32_t *row_of_slot, float *logits, int logits_stride) {
    if (!e || !feat || !head_rows || !head_b || !logits) return fail(AZG_E_INVALID_ARG, "null argument");
    if (logits_stride < e->gi.action_size + e->gi.num_players + 1 || e->gi.action_size > 1024)
        return fail(AZG_E_INVALID_ARG, "logits_stride must hold A + P + 1 logits (A <= 1024)");
    int want = 0;
    SPARSE_GAME_SWITCH(e, want = head_fk<G>());
    if (feat_k != want) return fail(AZG_E_INVALID_ARG, "feat_k must be cells x 16 rounded up to a multiple of 32 for this game");
    const HeadRows hd{(const _Float16 *)head_rows, head_b, feat_k};
    SPARSE_GAME_SWITCH(e, hipLaunchKernelGGL((k_leaf_heads_sparse<G>), dim3(e->v.B), dim3(64), 0, (hipStream_t)stream, e->v, (const _Float16 *)feat, hd,
                                      row_of_slot, logits, logits_stride));
    HIPCHK(hipGetLastError());
    return AZG_OK;
}

// playMoves and what follows it, for azg_advance (actions == nullptr: k_play<G>, every move from the trees) and azg_advance_actions
// (k_play<G, true>: the slots with an action >= 0 play it): one launch sequence, so that the two cannot drift apart
static int advance_launches(azg_engine *e, hipStream_t s, int record_history, const int32_t *actions) {
    ProfScope timed(e->prof, nullptr, s, 2, false);
    GAME_SWITCH(e, {
        if (actions) hipLaunchKernelGGL((k_play<G, true>), dim3(e->v.B), dim3(64), 0, s, e->v, record_history, actions);
        else hipLaunchKernelGGL((k_play<G>), dim3(e->v.B), dim3(64), 0, s, e->v, record_history, (const int32_t *)nullptr);
        hipLaunchKernelGGL((k_finalize<G>), dim3(1), dim3(64), 0, s, e->v, (const int32_t *)nullptr);
        hipLaunchKernelGGL((k_emit_samples<G>), dim3(e->v.B, G::NSYM), dim3(64), 0, s, e->v);
        hipLaunchKernelGGL((k_emit<G>), dim3(e->v.B), dim3(64), 0, s, e->v);
        hipLaunchKernelGGL((k_compact<G>), dim3(e->v.B * e->v.T), dim3(64), 0, s, e->v, 0, 0);
    });
    HIPCHK(hipGetLastError());
    return AZG_OK;
}

extern "C" int azg_advance(azg_engine *e, void *stream, int record_history) {
    if (!e) return fail(AZG_E_INVALID_ARG, "null engine");
    return advance_launches(e, (hipStream_t)stream, record_history, nullptr);
}

extern "C" int azg_advance_actions(azg_engine *e, void *stream, const int32_t *actions, int record_history) {
    if (!e) return fail(AZG_E_INVALID_ARG, "null engine");
    if (!actions) return fail(AZG_E_INVALID_ARG, "null actions_dev");
    return advance_launches(e, (hipStream_t)stream, record_history, actions);
}

extern "C" int azg_advance_begin(azg_engine *e, void *stream, int record_history, int32_t *fin_host) {
    if (!e || !fin_host) return fail(AZG_E_INVALID_ARG, "null argument");
    hipStream_t s = (hipStream_t)stream;
    GAME_SWITCH(e, hipLaunchKernelGGL((k_play<G>), dim3(e->v.B), dim3(64), 0, s, e->v, record_history, (const int32_t *)nullptr));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(fin_host, e->v.fin_flag, sizeof(int32_t) * e->v.B, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return AZG_OK;
}

extern "C" int azg_advance_commit(azg_engine *e, void *stream, const int32_t *counted_host) {
    if (!e || !counted_host) return fail(AZG_E_INVALID_ARG, "null argument");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemcpyAsync(e->v.fin_counted, counted_host, sizeof(int32_t) * e->v.B, hipMemcpyHostToDevice, s));
    GAME_SWITCH(e, {
        hipLaunchKernelGGL((k_finalize<G>), dim3(1), dim3(64), 0, s, e->v, (const int32_t *)e->v.fin_counted);
        hipLaunchKernelGGL((k_emit_samples<G>), dim3(e->v.B, G::NSYM), dim3(64), 0, s, e->v);
        hipLaunchKernelGGL((k_emit<G>), dim3(e->v.B), dim3(64), 0, s, e->v);
        hipLaunchKernelGGL((k_compact<G>), dim3(e->v.B * e->v.T), dim3(64), 0, s, e->v, 0, 0);
    });
    HIPCHK(hipGetLastError());
    return AZG_OK;
}

extern "C" int azg_root_counts(azg_engine *e, void *stream, int32_t *counts) {
    if (!e || !counts) return fail(AZG_E_INVALID_ARG, "null argument");
    hipStream_t s = (hipStream_t)stream;
    GAME_SWITCH(e, hipLaunchKernelGGL((k_root_stats<G>), dim3(e->v.B), dim3(64), 0, s, e->v, 0, 1.0f, 0, counts, (float *)nullptr, (float *)nullptr));
    HIPCHK(hipGetLastError());
    return AZG_OK;
}
extern "C" int azg_root_probs(azg_engine *e, void *stream, float temp, float *probs) {
    if (!e || !probs) return fail(AZG_E_INVALID_ARG, "null argument");
    hipStream_t s = (hipStream_t)stream;
    GAME_SWITCH(e, hipLaunchKernelGGL((k_root_stats<G>), dim3(e->v.B), dim3(64), 0, s, e->v, 1, temp, 0, (int32_t *)nullptr, probs, (float *)nullptr));
    HIPCHK(hipGetLastError());
    return AZG_OK;
}
extern "C" int azg_root_value(azg_engine *e, void *stream, int average, float *values) {
    if (!e || !values) return fail(AZG_E_INVALID_ARG, "null argument");
    hipStream_t s = (hipStream_t)stream;
    GAME_SWITCH(e, hipLaunchKernelGGL((k_root_stats<G>), dim3(e->v.B), dim3(64), 0, s, e->v, 2, 1.0f, average, (int32_t *)nullptr, (float *)nullptr, values));
    HIPCHK(hipGetLastError());
    return AZG_OK;
}

extern "C" int azg_update_root(azg_engine *e, void *stream, int slot, int action) {
    int r = check_range(e, slot, 1); if (r) return r;
    hipStream_t s = (hipStream_t)stream;
    GAME_SWITCH(e, hipLaunchKernelGGL((k_update_root<G>), dim3(1), dim3(64), 0, s, e->v, slot, action, e->d_ok));
    // (only this slot's trees: a compaction voids the tree's pending find_leaf, and another slot of a per-slot driven engine may
    //  sit between azg_select and azg_backup)
    GAME_SWITCH(e, hipLaunchKernelGGL((k_compact<G>), dim3(e->v.T), dim3(64), 0, s, e->v, 0, slot * e->v.T));
    int32_t ok = 0;
    HIPCHK(hipMemcpyAsync(&ok, e->d_ok, sizeof(ok), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (!ok) return fail(AZG_E_INVALID_ACTION, "Invalid action encountered while updating root: " + std::to_string(action));
    return AZG_OK;
}

extern "C" int azg_compact(azg_engine *e, void *stream, int slot, int force) {
    if (!e) return fail(AZG_E_INVALID_ARG, "null engine");
    if (slot >= e->v.B) return fail(AZG_E_INVALID_ARG, "slot out of range");
    hipStream_t s = (hipStream_t)stream;
    const int first = slot < 0 ? 0 : slot * e->v.T, count = slot < 0 ? e->v.B * e->v.T : e->v.T;
    GAME_SWITCH(e, hipLaunchKernelGGL((k_compact<G>), dim3(count), dim3(64), 0, s, e->v, force ? 1 : 0, first));
    HIPCHK(hipGetLastError());
    return AZG_OK;
}

extern "C" int azg_engine_info(azg_engine *e, int32_t *out8) {
    if (!e || !out8) return fail(AZG_E_INVALID_ARG, "null argument");
    out8[0] = e->v.cap; out8[1] = e->v.compact_reserve; out8[2] = e->v.T; out8[3] = e->v.maxd; out8[4] = e->v.B;
    out8[5] = e->v.ex_cap; out8[6] = e->v.res_cap; out8[7] = e->cfg.sims_per_move > 0 ? e->cfg.sims_per_move : 100;
    return AZG_OK;
}

extern "C" int azg_set_random_tape(azg_engine *e, void *stream, const int16_t *ranks_host, const double *u_host, const int32_t *noise_off_host,
                                   const float *noise_pool_host, int noise_len, int len) {
    (void)stream;
    if (!e || len < 0 || noise_len < 0) return fail(AZG_E_INVALID_ARG, "null engine or negative length");
    if ((u_host || noise_off_host) && !ranks_host) return fail(AZG_E_INVALID_ARG, "choice / noise tapes come with a shuffle tape (one counter indexes all three)");
    if ((noise_off_host != nullptr) != (noise_pool_host != nullptr)) return fail(AZG_E_INVALID_ARG, "noise offsets and noise pool come together");
    const size_t n = (size_t)e->v.B * (size_t)(len > 0 ? len : 0);
    // every rank is an offset into an expansion's block of k <= max_children nodes: refuse anything else here, on the host (the device
    // checks rank < k per expansion as well and raises the sticky AZG_E_INVALID_ARG)
    if (ranks_host) for (size_t i = 0; i < n; i++)
        if (ranks_host[i] < 0 || ranks_host[i] >= e->gi.max_children) return fail(AZG_E_INVALID_ARG, "shuffle tape: a rank is outside [0, max_children)");
    if (u_host) for (size_t i = 0; i < n; i++)
        if (!(u_host[i] >= 0.0 && u_host[i] < 1.0)) return fail(AZG_E_INVALID_ARG, "choice tape: a uniform is outside [0, 1)");
    if (noise_off_host) for (size_t i = 0; i < n; i++)
        if (noise_off_host[i] < -1 || noise_off_host[i] >= noise_len) return fail(AZG_E_INVALID_ARG, "noise tape: an offset is outside the pool");
    // the View -- and with it these pointers -- is passed BY VALUE to every launch, also to launches captured in a hipGraph: work of ANY
    // stream may still read the old tapes, so the whole device is drained before they are freed.  A graph captured while a tape was set
    // keeps replaying with the pointers it captured: re-capture after changing the tape
    HIPCHK(hipDeviceSynchronize());
    if (e->d_perm) { (void)hipFree(e->d_perm); e->d_perm = nullptr; }
    if (e->d_utape) { (void)hipFree(e->d_utape); e->d_utape = nullptr; }
    if (e->d_noff) { (void)hipFree(e->d_noff); e->d_noff = nullptr; }
    if (e->d_npool) { (void)hipFree(e->d_npool); e->d_npool = nullptr; }
    e->v.perm_tape = nullptr; e->v.perm_len = 0; e->v.u_tape = nullptr; e->v.noise_off = nullptr; e->v.noise_pool = nullptr; e->v.noise_len = 0;
    if (!ranks_host || len == 0) return AZG_OK;
    HIPCHK(hipMalloc((void **)&e->d_perm, n * sizeof(int16_t)));
    HIPCHK(hipMemcpy(e->d_perm, ranks_host, n * sizeof(int16_t), hipMemcpyHostToDevice));
    if (u_host) {
        HIPCHK(hipMalloc((void **)&e->d_utape, n * sizeof(double)));
        HIPCHK(hipMemcpy(e->d_utape, u_host, n * sizeof(double), hipMemcpyHostToDevice));
    }
    if (noise_off_host) {
        HIPCHK(hipMalloc((void **)&e->d_noff, n * sizeof(int32_t)));
        HIPCHK(hipMemcpy(e->d_noff, noise_off_host, n * sizeof(int32_t), hipMemcpyHostToDevice));
        HIPCHK(hipMalloc((void **)&e->d_npool, (size_t)(noise_len > 0 ? noise_len : 1) * sizeof(float)));
        HIPCHK(hipMemcpy(e->d_npool, noise_pool_host, (size_t)noise_len * sizeof(float), hipMemcpyHostToDevice));
    }
    e->v.perm_tape = e->d_perm; e->v.perm_len = len;
    e->v.u_tape = e->d_utape; e->v.noise_off = e->d_noff; e->v.noise_pool = e->d_npool; e->v.noise_len = noise_len;
    return AZG_OK;
}

extern "C" int azg_set_shuffle_tape(azg_engine *e, void *stream, const int16_t *ranks_host, int len) {
    return azg_set_random_tape(e, stream, ranks_host, nullptr, nullptr, nullptr, 0, len);
}

// bounds-checked builds (-DAZG_DEBUG_BOUNDS): the first check that failed (0: none; site numbers: csrc/azg_kernels.h AZG_BOUNDS_OK).
// *checked = 1 if this binary carries the checks at all.
extern "C" int azg_debug_bounds_site(azg_engine *e, void *stream, int32_t *site, int32_t *checked) {
    if (!e || !site || !checked) return fail(AZG_E_INVALID_ARG, "null argument");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemcpyAsync(site, e->v.gcount + GC_BOUNDS_SITE, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
#ifdef AZG_DEBUG_BOUNDS
    *checked = 1;
#else
    *checked = 0;
#endif
    return AZG_OK;
}

#ifdef AZG_DEBUG_BOUNDS
// bounds-checked builds only (not part of include/azg.h): overwrite the root's first_child of a slot's tree -- the positive control of
// tools/debug_soak.py (a child block outside the live allocation must be caught by the checks, not read)
extern "C" int azg_debug_poke_root_fc(azg_engine *e, void *stream, int slot, int32_t fc) {
    int r = check_range(e, slot, 1); if (r) return r;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemcpyAsync(reinterpret_cast<char *>(e->v.hdr + (size_t)slot * e->v.T) + 16, &fc, sizeof(fc), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    return AZG_OK;
}
#endif

extern "C" int azg_set_root_flags(azg_engine *e, int flags) {
    if (!e || flags < 0) return fail(AZG_E_INVALID_ARG, "null engine or negative flags");
    e->v.add_noise = ((flags & AZG_FLAG_NOISE) && !e->v.arena) ? 1 : 0; e->v.add_temp = ((flags & AZG_FLAG_TEMP) && !e->v.arena) ? 1 : 0;
    return AZG_OK;
}

// ---- snapshot of one slot's search state (pickling of the single-tree MCTS class: MCTS.pyx:8 auto_pickle) ----
// layout: int64 magic, int32 game, T, maxd, pad | azg_state root, leaf | uint64 tape_ctr | per tree: TreeHdr, PathEnt[maxd], Node[alloc]
static const int64_t k_snap_magic = 0x315A4E53475A41LL;     // "AZGSNZ1"
struct SnapHead { int64_t magic; int32_t game, T, maxd, layout; azg_state root, leaf; uint64_t ctr; };
// (layout: the record sizes and the ABI version the snapshot was written with -- a change of Node / TreeHdr / PathEnt invalidates old pickles)
static const int32_t k_snap_layout = (int32_t)(sizeof(Node) | (sizeof(TreeHdr) << 8) | (sizeof(PathEnt) << 16) | ((unsigned)AZG_ABI_VERSION << 24));

extern "C" int64_t azg_slot_export(azg_engine *e, void *stream, int slot, void *host_buf, int64_t nbytes) {
    int r = check_range(e, slot, 1); if (r) return r;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipStreamSynchronize(s));
    const int T = e->v.T, maxd = e->v.maxd;
    std::vector<TreeHdr> hdr((size_t)T);
    HIPCHK(hipMemcpy(hdr.data(), e->v.hdr + (size_t)slot * T, sizeof(TreeHdr) * T, hipMemcpyDeviceToHost));
    int64_t need = (int64_t)sizeof(SnapHead);
    for (int t = 0; t < T; t++) need += (int64_t)sizeof(TreeHdr) + (int64_t)sizeof(PathEnt) * maxd + (int64_t)sizeof(Node) * hdr[t].alloc;
    if (!host_buf) return need;                              // size query
    if (nbytes < need) return fail(AZG_E_INVALID_ARG, "snapshot buffer too small");
    char *o = (char *)host_buf;
    SnapHead sh; memset(&sh, 0, sizeof(sh));
    sh.magic = k_snap_magic; sh.game = e->cfg.game; sh.T = T; sh.maxd = maxd; sh.layout = k_snap_layout;
    HIPCHK(hipMemcpy(&sh.root, e->v.states + slot, sizeof(azg_state), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&sh.leaf, e->v.leaf_states + slot, sizeof(azg_state), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&sh.ctr, e->v.tape_ctr + slot, sizeof(uint64_t), hipMemcpyDeviceToHost));
    memcpy(o, &sh, sizeof(sh)); o += sizeof(sh);
    for (int t = 0; t < T; t++) {
        const size_t tt = (size_t)slot * T + t;
        memcpy(o, &hdr[t], sizeof(TreeHdr)); o += sizeof(TreeHdr);
        HIPCHK(hipMemcpy(o, e->v.path + tt * maxd, sizeof(PathEnt) * maxd, hipMemcpyDeviceToHost)); o += sizeof(PathEnt) * maxd;
        if (hdr[t].alloc > 0) HIPCHK(hipMemcpy(o, e->v.nodes + tt * 2 * e->v.cap + hdr[t].base, sizeof(Node) * hdr[t].alloc, hipMemcpyDeviceToHost));
        o += sizeof(Node) * hdr[t].alloc;
    }
    return need;
}

extern "C" int azg_slot_import(azg_engine *e, void *stream, int slot, const void *host_buf, int64_t nbytes) {
    int r = check_range(e, slot, 1); if (r) return r;
    if (!host_buf || nbytes < (int64_t)sizeof(SnapHead)) return fail(AZG_E_INVALID_ARG, "snapshot truncated");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipStreamSynchronize(s));
    const char *o = (const char *)host_buf, *end = o + nbytes;
    SnapHead sh; memcpy(&sh, o, sizeof(sh)); o += sizeof(sh);
    if (sh.magic != k_snap_magic || sh.game != e->cfg.game || sh.T != e->v.T || sh.maxd != e->v.maxd)
        return fail(AZG_E_INVALID_ARG, "snapshot does not belong to this kind of engine (game / arena mode)");
    if (sh.layout != k_snap_layout) return fail(AZG_E_INVALID_ARG, "snapshot was written by a library with another record layout / ABI version");
    {                                                        // validate the whole snapshot before anything is written
        const char *q = o;
        for (int t = 0; t < sh.T; t++) {
            if (end - q < (int64_t)(sizeof(TreeHdr) + sizeof(PathEnt) * sh.maxd)) return fail(AZG_E_INVALID_ARG, "snapshot truncated");
            TreeHdr h; memcpy(&h, q, sizeof(h));
            if (h.alloc < 0 || h.alloc > e->v.cap) return fail(AZG_E_TREE_FULL, "snapshot holds more nodes than this engine's nodes_per_tree");
            q += sizeof(TreeHdr) + sizeof(PathEnt) * sh.maxd;
            if (end - q < (int64_t)sizeof(Node) * h.alloc) return fail(AZG_E_INVALID_ARG, "snapshot truncated");
            // every index the kernels will follow must stay inside the live nodes: a corrupted or hand-made pickle must not become an
            // out-of-bounds device access on the next find_leaf / process_results
            const unsigned lk = h.leaf_info & 0xFFFFu;
            if (h.depth < 0 || h.depth > sh.maxd || h.max_depth < 0 || h.leaf < LEAF_IS_ROOT || h.leaf >= h.alloc || h.leaf_fc < -1 ||
                (h.leaf_fc >= 0 && (int64_t)h.leaf_fc + (int64_t)lk > h.alloc))
                return fail(AZG_E_INVALID_ARG, "snapshot header points outside its nodes");
            if (h.root.first_child < -1 || (h.root.first_child >= 0 && (int64_t)h.root.first_child + h.root.nchild > h.alloc))
                return fail(AZG_E_INVALID_ARG, "snapshot root points outside its nodes");
            const PathEnt *pe = reinterpret_cast<const PathEnt *>(q - sizeof(PathEnt) * sh.maxd);
            for (int d = 0; d < h.depth; d++) {
                PathEnt ent; memcpy(&ent, pe + d, sizeof(ent));
                if ((int)(ent.idx_mover & 0x0FFFFFFFu) >= h.alloc) return fail(AZG_E_INVALID_ARG, "snapshot path points outside its nodes");
            }
            for (int i = 0; i < h.alloc; i++) {
                Node nd; memcpy(&nd, q + sizeof(Node) * (size_t)i, sizeof(nd));
                if (nd.first_child < -1 || (nd.first_child >= 0 && (int64_t)nd.first_child + nd.nchild > h.alloc))
                    return fail(AZG_E_INVALID_ARG, "snapshot node points outside its nodes");
            }
            q += sizeof(Node) * h.alloc;
        }
    }
    HIPCHK(hipMemcpy(e->v.states + slot, &sh.root, sizeof(azg_state), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e->v.leaf_states + slot, &sh.leaf, sizeof(azg_state), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e->v.tape_ctr + slot, &sh.ctr, sizeof(uint64_t), hipMemcpyHostToDevice));
    for (int t = 0; t < sh.T; t++) {
        const size_t tt = (size_t)slot * sh.T + t;
        if (end - o < (int64_t)(sizeof(TreeHdr) + sizeof(PathEnt) * sh.maxd)) return fail(AZG_E_INVALID_ARG, "snapshot truncated");
        TreeHdr h; memcpy(&h, o, sizeof(h)); o += sizeof(h);
        if (h.alloc < 0 || h.alloc > e->v.cap) return fail(AZG_E_TREE_FULL, "snapshot holds more nodes than this engine's nodes_per_tree");
        h.base = 0;                                          // the live nodes land in semi-space 0 (indices are relative to the base)
        HIPCHK(hipMemcpy(e->v.hdr + tt, &h, sizeof(h), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(e->v.path + tt * sh.maxd, o, sizeof(PathEnt) * sh.maxd, hipMemcpyHostToDevice)); o += sizeof(PathEnt) * sh.maxd;
        if (end - o < (int64_t)sizeof(Node) * h.alloc) return fail(AZG_E_INVALID_ARG, "snapshot truncated");
        if (h.alloc > 0) HIPCHK(hipMemcpy(e->v.nodes + tt * 2 * e->v.cap, o, sizeof(Node) * h.alloc, hipMemcpyHostToDevice));
        o += sizeof(Node) * h.alloc;
    }
    return AZG_OK;
}

static int tree_of(azg_engine *e, int slot, int tree) { return slot * e->v.T + tree; }

// node `node` of a tree (AZG_NODE_ROOT = the root, which lives in the header) and the base of the tree's live semi-space
static int fetch_node(azg_engine *e, int t, int node, TreeHdr &h, Node &nd, Node *&base) {
    HIPCHK(hipMemcpy(&h, e->v.hdr + t, sizeof(h), hipMemcpyDeviceToHost));
    base = e->v.nodes + (size_t)t * 2 * e->v.cap + h.base;
    if (node < 0) { nd = h.root; return AZG_OK; }
    if (node >= h.alloc) return fail(AZG_E_INVALID_ARG, "node index out of range");
    HIPCHK(hipMemcpy(&nd, base + node, sizeof(Node), hipMemcpyDeviceToHost));
    return AZG_OK;
}

extern "C" int azg_root_children(azg_engine *e, void *stream, int slot, int tree, int max_k, int32_t *a, int32_t *n, float *q, float *p, float *vv) {
    int r = check_range(e, slot, 1); if (r) return r;
    if (tree < 0 || tree >= e->v.T) return fail(AZG_E_INVALID_ARG, "tree index out of range");
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    TreeHdr h; Node root; Node *base;
    r = fetch_node(e, tree_of(e, slot, tree), -1, h, root, base); if (r) return r;
    int k = root.nchild;
    if (k > max_k) return fail(AZG_E_INVALID_ARG, "max_k too small");
    if (k == 0) return 0;
    std::vector<Node> ch((size_t)k);
    HIPCHK(hipMemcpy(ch.data(), base + root.first_child, sizeof(Node) * k, hipMemcpyDeviceToHost));
    for (int i = 0; i < k; i++) { a[i] = ch[i].a; n[i] = ch[i].n; q[i] = ch[i].q; p[i] = ch[i].p; vv[i] = ch[i].v; }
    return k;
}

extern "C" int azg_node_children(azg_engine *e, void *stream, int slot, int tree, int node, int max_k, int32_t *idx, int32_t *a, int32_t *n, float *q, float *p, float *vv,
                                 int32_t *player, int32_t *e_bits) {
    int r = check_range(e, slot, 1); if (r) return r;
    if (tree < 0 || tree >= e->v.T) return fail(AZG_E_INVALID_ARG, "tree index out of range");
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    TreeHdr h; Node nd; Node *base;
    r = fetch_node(e, tree_of(e, slot, tree), node, h, nd, base); if (r) return r;
    int k = nd.nchild;
    if (k > max_k) return fail(AZG_E_INVALID_ARG, "max_k too small");
    if (k == 0) return 0;
    std::vector<Node> ch((size_t)k);
    HIPCHK(hipMemcpy(ch.data(), base + nd.first_child, sizeof(Node) * k, hipMemcpyDeviceToHost));
    for (int i = 0; i < k; i++) {
        idx[i] = nd.first_child + i; a[i] = ch[i].a; n[i] = ch[i].n; q[i] = ch[i].q; p[i] = ch[i].p; vv[i] = ch[i].v;
        if (player) player[i] = ch[i].player;
        if (e_bits) e_bits[i] = ch[i].e;
    }
    return k;
}

extern "C" int azg_reset_max_depth(azg_engine *e, void *stream) {
    if (!e) return fail(AZG_E_INVALID_ARG, "null engine");
    hipLaunchKernelGGL(k_reset_max_depth, dim3(((int)(e->v.B * e->v.T) + 63) / 64), dim3(64), 0, (hipStream_t)stream, e->v);
    HIPCHK(hipGetLastError());
    return AZG_OK;
}

extern "C" int azg_tree_info(azg_engine *e, void *stream, int slot, int tree, int32_t *out8) {
    int r = check_range(e, slot, 1); if (r) return r;
    if (tree < 0 || tree >= e->v.T) return fail(AZG_E_INVALID_ARG, "tree index out of range");
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    TreeHdr h;
    HIPCHK(hipMemcpy(&h, e->v.hdr + tree_of(e, slot, tree), sizeof(h), hipMemcpyDeviceToHost));
    const Node &root = h.root;
    out8[0] = root.n; memcpy(&out8[1], &root.q, 4); memcpy(&out8[2], &root.v, 4);
    out8[3] = root.player; out8[4] = root.e; out8[5] = h.depth; out8[6] = h.max_depth; out8[7] = h.alloc;
    return AZG_OK;
}

extern "C" int azg_last_path(azg_engine *e, void *stream, int slot, int tree, int max_len, int32_t *actions) {
    int r = check_range(e, slot, 1); if (r) return r;
    if (tree < 0 || tree >= e->v.T) return fail(AZG_E_INVALID_ARG, "tree index out of range");
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    const int t = tree_of(e, slot, tree);
    TreeHdr h;
    HIPCHK(hipMemcpy(&h, e->v.hdr + t, sizeof(h), hipMemcpyDeviceToHost));
    if (h.depth > max_len) return fail(AZG_E_INVALID_ARG, "max_len too small");
    std::vector<PathEnt> path((size_t)(h.depth > 0 ? h.depth : 1));
    if (h.depth > 0) HIPCHK(hipMemcpy(path.data(), e->v.path + (size_t)t * e->v.maxd, sizeof(PathEnt) * h.depth, hipMemcpyDeviceToHost));
    const Node *base = e->v.nodes + (size_t)t * 2 * e->v.cap + h.base;
    for (int d = 0; d < h.depth; d++) {
        Node nd;
        HIPCHK(hipMemcpy(&nd, base + (path[d].idx_mover & 0x0FFFFFFFu), sizeof(Node), hipMemcpyDeviceToHost));
        actions[d] = nd.a;
    }
    return h.depth;
}

extern "C" int azg_read_counters(azg_engine *e, void *stream, azg_counters *out) {
    if (!e || !out) return fail(AZG_E_INVALID_ARG, "null argument");
    hipStream_t s = (hipStream_t)stream;
    int32_t gc[8];
    std::vector<int64_t> sims((size_t)e->v.B), exps((size_t)e->v.B);
    hipLaunchKernelGGL(k_max_nodes, dim3(1), dim3(256), 0, s, e->v);
    HIPCHK(hipMemcpyAsync(gc, e->v.gcount, sizeof(gc), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(sims.data(), e->v.slot_sims, sizeof(int64_t) * e->v.B, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(exps.data(), e->v.slot_exp, sizeof(int64_t) * e->v.B, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    memset(out, 0, sizeof(*out));
    for (int i = 0; i < e->v.B; i++) { out->sims += sims[i]; out->expansions += exps[i]; }
    out->games_played = gc[GC_GAMES]; out->num_results = gc[GC_RESULTS]; out->num_examples = gc[GC_EXAMPLES];
    out->error = gc[GC_ERROR]; out->max_nodes_used = gc[GC_MAXNODES]; out->max_nodes_kept = gc[GC_MAXLIVE];
    return AZG_OK;
}

extern "C" int azg_examples_dev(azg_engine *e, float **obs, float **pi, float **z) {
    if (!e) return fail(AZG_E_INVALID_ARG, "null engine");
    if (obs) *obs = e->v.ex_obs; if (pi) *pi = e->v.ex_pi; if (z) *z = e->v.ex_z;
    return AZG_OK;
}

extern "C" int azg_copy_examples(azg_engine *e, void *stream, int first, int count, float *obs, float *pi, float *z) {
    if (!e) return fail(AZG_E_INVALID_ARG, "null engine");
    if (first < 0 || count < 0 || first + count > e->v.ex_cap) return fail(AZG_E_INVALID_ARG, "example range out of bounds");
    if (count == 0) return AZG_OK;
    hipStream_t s = (hipStream_t)stream;
    const size_t A = e->gi.action_size, NV = e->gi.num_players + 1, O = (size_t)e->gi.obs_c * e->gi.obs_h * e->gi.obs_w;
    if (obs) HIPCHK(hipMemcpyAsync(obs, e->v.ex_obs + (size_t)first * O, sizeof(float) * count * O, hipMemcpyDeviceToDevice, s));
    if (pi) HIPCHK(hipMemcpyAsync(pi, e->v.ex_pi + (size_t)first * A, sizeof(float) * count * A, hipMemcpyDeviceToDevice, s));
    if (z) HIPCHK(hipMemcpyAsync(z, e->v.ex_z + (size_t)first * NV, sizeof(float) * count * NV, hipMemcpyDeviceToDevice, s));
    return AZG_OK;
}

extern "C" int azg_read_results(azg_engine *e, void *stream, int first, int count, uint8_t *ws, int32_t *turns, int32_t *slot) {
    if (!e) return fail(AZG_E_INVALID_ARG, "null engine");
    if (first < 0 || count < 0 || first + count > e->v.res_cap) return fail(AZG_E_INVALID_ARG, "result range out of bounds");
    hipStream_t s = (hipStream_t)stream;
    const int NV = e->gi.num_players + 1;
    if (count == 0) return AZG_OK;
    HIPCHK(hipMemcpyAsync(ws, e->v.res_ws + (size_t)first * NV, (size_t)count * NV, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(turns, e->v.res_turns + first, sizeof(int32_t) * count, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(slot, e->v.res_slot + first, sizeof(int32_t) * count, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return AZG_OK;
}

extern "C" int azg_clear_outputs(azg_engine *e, void *stream) {
    if (!e) return fail(AZG_E_INVALID_ARG, "null engine");
    HIPCHK(hipMemsetAsync(e->v.gcount, 0, sizeof(int32_t) * 3, (hipStream_t)stream));
    return AZG_OK;
}

extern "C" int azg_last_actions_dev(azg_engine *e, int32_t **actions) {
    if (!e || !actions) return fail(AZG_E_INVALID_ARG, "null argument");
    *actions = e->v.last_action;
    return AZG_OK;
}

extern "C" int azg_states_dev(azg_engine *e, const azg_state **states) {
    if (!e || !states) return fail(AZG_E_INVALID_ARG, "null argument");
    *states = e->v.states;
    return AZG_OK;
}

#ifdef AZG_TOWER_TIMING
// measurement builds only: the stamp buffer of ONE k_tower2 instantiation and its dump to stderr -- a persistent wide-head launch after
// every launch (phase means over the workgroups, the helper wavefront, the layers of workgroup 0), any other tile after its 8th launch
// (the layers of workgroup 0, every workgroup's phases)
template <int H, int W, int BOARDS, int C, int PSPLIT, class SEARCH, int KSPLIT>
struct TowerTiming {
    static int stamps(unsigned long long **out) {
        if (!dbg()) { HIPCHK(hipMalloc((void **)&dbg(), (2048 + 4096 * 8) * 8)); HIPCHK(hipMemset(dbg(), 0, (2048 + 4096 * 8) * 8)); }
        *out = dbg();
        return AZG_OK;
    }
    static int dump(hipStream_t s, const TowerParams &P, const SEARCH &sa, int grid) {
        constexpr bool IS_SEARCH = !__is_same(SEARCH, NoSearch);
        unsigned long long *const dbg = TowerTiming::dbg();
        static int calls = 0;
        (void)sa;
        if constexpr (IS_SEARCH) if constexpr (SEARCH::WIDE) {
            static unsigned long long w[512 * 4];
            HIPCHK(hipStreamSynchronize(s)); HIPCHK(hipMemcpy(w, dbg + 2048 + 4096 * 4, sizeof(unsigned long long) * 4 * (grid < 512 ? grid : 512), hipMemcpyDeviceToHost));
            double ph[4] = {0, 0, 0, 0}; const int nb = grid < 512 ? grid : 512;
            for (int b = 0; b < nb; b++) for (int i = 0; i < 4; i++) ph[i] += (double)w[b * 4 + i];
            const double n = (double)nb * (sa.sims > 8 ? sa.sims - 8 : 1);
            fprintf(stderr, "wide search, cycles per simulation (mean over %d workgroups): tree %.0f tower %.0f headconv %.0f heads %.0f\n", nb, ph[0] / n, ph[1] / n, ph[2] / n, ph[3] / n);
            HIPCHK(hipMemset(dbg + 2048 + 4096 * 4, 0, sizeof(unsigned long long) * 4 * 512));
            static unsigned long long hw_[512 * 8];
            HIPCHK(hipMemcpy(hw_, dbg + 2048 + 4096 * 5, sizeof(unsigned long long) * 8 * nb, hipMemcpyDeviceToHost));
            double hp[5] = {0, 0, 0, 0, 0}, hn = 0;
            for (int b = 0; b < nb; b++) { for (int i = 0; i < 5; i++) hp[i] += (double)hw_[b * 8 + i]; hn += (double)hw_[b * 8 + 5]; }
            if (hn > 0) fprintf(stderr, "  helper wavefront (cycles per simulation with a policy backup): header %.0f masks %.0f logits %.0f softmax %.0f priors %.0f\n",
                                hp[0] / hn, hp[1] / hn, hp[2] / hn, hp[3] / hn, hp[4] / hn);
            HIPCHK(hipMemset(dbg + 2048 + 4096 * 5, 0, sizeof(unsigned long long) * 8 * 512));
            {                                                       // the layers of workgroup 0's last simulation (all wavefronts of the workgroup)
                unsigned long long h[64 * 4 * 5];
                HIPCHK(hipMemcpy(h, dbg, sizeof(h), hipMemcpyDeviceToHost));
                for (int l = 0; l <= 2 * P.nblocks; l++) for (int w = 0; w < C / 32 * PSPLIT * KSPLIT && w < 4; w++) {
                    unsigned long long *t = h + (l * 4 + w) * 5;
                    fprintf(stderr, "  layer %2d wave %d: main %6llu wait %6llu epi %6llu bar %6llu | start %llu\n", l, w, t[1] - t[0], t[2] - t[1], t[3] - t[2], t[4] - t[3], t[0] - h[0]);
                }
            }
            calls = 100;
        }
        if (++calls == 8) {
            unsigned long long h[64 * 4 * 5];
            HIPCHK(hipStreamSynchronize(s)); HIPCHK(hipMemcpy(h, dbg, sizeof(h), hipMemcpyDeviceToHost));
            for (int l = 0; l <= 2 * P.nblocks; l++) for (int w = 0; w < C / 32; w++) {
                unsigned long long *t = h + (l * 4 + w) * 5;
                fprintf(stderr, "layer %2d wave %d: main %6llu wait %6llu epi %6llu bar %6llu | start %llu\n", l, w, t[1] - t[0], t[2] - t[1], t[3] - t[2], t[4] - t[3], t[0] - h[0]);
            }
            static unsigned long long w[4096 * 8];
            HIPCHK(hipMemcpy(w, dbg + 2048, sizeof(unsigned long long) * 8 * grid, hipMemcpyDeviceToHost));
            unsigned long long x2[1024];
            HIPCHK(hipMemcpy(x2, dbg + 1024, sizeof(x2), hipMemcpyDeviceToHost));
            for (int b = 0; b < grid && b < 512; b++) fprintf(stderr, "wgx %4d xload+store %llu weights %llu\n", b, x2[b * 2] - w[b * 8], x2[b * 2 + 1] - x2[b * 2]);
            for (int b = 0; b < grid; b++) fprintf(stderr, "wg %4d xcc %llu hwid %08llx start %llu end %llu | prologue %llu layers %llu headmm %llu softmax %llu tail %llu\n", b, w[b * 8 + 3] & 15, w[b * 8 + 2], w[b * 8], w[b * 8 + 1],
                                                   w[b * 8 + 4] - w[b * 8], w[b * 8 + 5] - w[b * 8 + 4], w[b * 8 + 6] - w[b * 8 + 5], w[b * 8 + 7] - w[b * 8 + 6], w[b * 8 + 1] - w[b * 8 + 7]);
        }
        return AZG_OK;
    }
private:
    static unsigned long long *&dbg() { static unsigned long long *d = nullptr; return d; }
};
#endif

// occ (optional): the workgroups of THIS instantiation a CU of this device holds at once (the occupancy query with the launch's own LDS
// size) -- what the tile choice of the persistent launches is derived from instead of a constant for one chip
template <int H, int W, int BOARDS, int C, int PSPLIT = 1, class SEARCH = NoSearch, int KSPLIT = 1>
static int launch_tower(hipStream_t s, const TowerParams &P, SEARCH sa = SEARCH{}, bool init_only = false, int *occ = nullptr) {
    constexpr bool IS_SEARCH = !__is_same(SEARCH, NoSearch);
    using GEO = TowerGeom<H, W, BOARDS, C>;
    constexpr size_t LDS_IMG = []() {                          // the image (+ the wide search mode's scratch behind it)
        if constexpr (IS_SEARCH) { if constexpr (SEARCH::WIDE) return (size_t)GEO::TILE + (size_t)WideLds<typename SEARCH::Game, H * W, BOARDS, wide_solo<C, PSPLIT, KSPLIT, BOARDS>(),
                                                                                                             HeadsStreamedOf<SEARCH, H * W, C>::value>::BYTES; }
        return (size_t)GEO::TILE;
    }();
    // (+ the k-split exchange area: per wave one 1 KB accumulator tile for each of the 2 x NSUB / 2 tiles its partner finishes)
    constexpr size_t LDS_FIXED = LDS_IMG + (KSPLIT == 2 ? (size_t)(C / 32 * PSPLIT * 2) * ((GEO::NSUB + PSPLIT - 1) / PSPLIT) * 1024 : 0);
    // (+ the layers' biases and affines of one-board tiles, tower_param_bytes: sized by the network's depth)
    constexpr bool WSOLO = []() { if constexpr (IS_SEARCH) { if constexpr (SEARCH::WIDE) return wide_solo<C, PSPLIT, KSPLIT, BOARDS>(); } return false; }();
    constexpr bool DYN_PARAMS = BOARDS == 1 || WSOLO;          // (tower_param_bytes: sized by the network's depth)
    const size_t LDS_BYTES = LDS_FIXED + (size_t)tower_param_bytes<C, BOARDS, WSOLO>(P.nblocks);
    // per (instantiation, device): the pixel -> (subtile, lane) table, a few hundred bytes that live as long as the process
    // (the table is a pure function of the template arguments); first use is serialised
    static int16_t *d_map[16] = {nullptr};
    static int d_lds[16] = {0};
    static std::mutex d_map_mu;
    int dev = 0, cus = 256;
    HIPCHK(hipGetDevice(&dev));
    if (dev < 0 || dev >= 16) return fail(AZG_E_INVALID_ARG, "device ordinal out of range");
    {
        std::lock_guard<std::mutex> lk(d_map_mu);
        if (!d_map[dev]) {
            int16_t map[GEO::NSUB * 16];
            if (!tower_pixmap<GEO>(map)) return fail(AZG_E_INTERNAL, "tower pixel map does not fit its subtiles");
            int16_t *d = nullptr;
            HIPCHK(hipMalloc((void **)&d, sizeof(map)));
            HIPCHK(hipMemcpy(d, map, sizeof(map), hipMemcpyHostToDevice));
            // (the LDS a workgroup may take on THIS device -- 160 KB on gfx950 --, not a constant: a device with less refuses loudly below)
            int lds_limit = 0;
            HIPCHK(hipDeviceGetAttribute(&lds_limit, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
            if ((size_t)lds_limit < LDS_FIXED) return fail(AZG_E_UNSUPPORTED, "this tile shape needs more LDS per workgroup than the device has");
            HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_tower2<H, W, BOARDS, C, PSPLIT, SEARCH, KSPLIT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(DYN_PARAMS ? (size_t)lds_limit : LDS_FIXED)));
            d_lds[dev] = lds_limit;
            d_map[dev] = d;
        }
    }
    if (LDS_BYTES > (size_t)d_lds[dev]) return fail(AZG_E_INVALID_ARG, "this tower does not fit the LDS of its tile (too many residual blocks)");
    if (occ) {
        int n = 0;
        HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, reinterpret_cast<const void *>(&k_tower2<H, W, BOARDS, C, PSPLIT, SEARCH, KSPLIT>),
                                                            C * 2 * PSPLIT * KSPLIT, LDS_BYTES));
        *occ = n > 0 ? n : 1;
    }
    if (init_only) return AZG_OK;                            // (first-use allocations must not happen inside a stream capture)
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    const int ntiles = (P.boards + BOARDS - 1) / BOARDS + (P.rows_per_model ? P.nmodels - 1 : 0);
    {                                                        // one LDS image, residual stream in registers, >= 2 workgroups per CU
        const int per_cu = (int)((size_t)d_lds[dev] / LDS_BYTES) > 0 ? (int)((size_t)d_lds[dev] / LDS_BYTES) : 1;
        // (search mode: every tile is its own workgroup for the whole launch -- they never synchronise, later ones just start later)
        const int grid = IS_SEARCH || ntiles < per_cu * cus ? ntiles : per_cu * cus;
#ifdef AZG_TOWER_TIMING
        using TT = TowerTiming<H, W, BOARDS, C, PSPLIT, SEARCH, KSPLIT>;
        TowerParams Q = P;
        { const int r = TT::stamps(&Q.dbg); if (r != AZG_OK) return r; }
        AZG_LAUNCH((k_tower2<H, W, BOARDS, C, PSPLIT, SEARCH, KSPLIT>), dim3(grid), dim3(C * 2 * PSPLIT * KSPLIT), LDS_BYTES, s, Q, (const int16_t *)d_map[dev], sa);
        { const int r = TT::dump(s, P, sa, grid); if (r != AZG_OK) return r; }
#else
        AZG_LAUNCH((k_tower2<H, W, BOARDS, C, PSPLIT, SEARCH, KSPLIT>), dim3(grid), dim3(C * 2 * PSPLIT * KSPLIT), LDS_BYTES, s, P, (const int16_t *)d_map[dev], sa);
#endif
    }
    HIPCHK(hipGetLastError());
    return AZG_OK;
}

// ---- timing hooks for the network launches (no engine handle there: one record for the process, behind a mutex) -----------------
static struct { std::mutex mu; Prof prof; } g_netprof;
struct NetProfScope : ProfScope {
    NetProfScope(hipStream_t s, int fam, bool enabled = true) : ProfScope(g_netprof.prof, &g_netprof.mu, s, fam, true, enabled) {}
};
extern "C" int azg_profile_net_enable(int on) {
    std::lock_guard<std::mutex> lk(g_netprof.mu);
    g_netprof.prof.enable(on != 0);
    return AZG_OK;
}
extern "C" int azg_profile_net_read(double *ms3, int64_t *launches3) {
    if (!ms3 || !launches3) return fail(AZG_E_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> lk(g_netprof.mu);
    g_netprof.prof.read(ms3, launches3);
    return AZG_OK;
}

static int device_cus(int *cus) {
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    HIPCHK(hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, dev));
    if (*cus <= 0) *cus = 1;
    return AZG_OK;
}

// the launch half of dispatch_tower: the row of AZG_TOWER_TILES that is (game, channels, bt, psplit, ksplit)
static int tower_tile_launch(hipStream_t s, int game, int channels, int bt, int psplit, int ksplit, const TowerParams &P) {
#define AZG_ROW(G, C, BT, PS, KS, LIMIT) \
    if (game == G::ID && channels == C && bt == BT && psplit == PS && ksplit == KS) return launch_tower<G::H, G::W, BT, C, PS, NoSearch, KS>(s, P);
    AZG_TOWER_TILES(AZG_ROW)
#undef AZG_ROW
    return fail(AZG_E_UNSUPPORTED, "no MFMA tower for this game / channel count (azg_launch_support: the pairs with AZG_SUPPORT_TOWER)");
}

// The tile of a stand-alone tower launch: the policy is in the rows (tower_tile_pick, azg_tiles.h), in boards per CU of THIS device;
// tower_tile_launch launches the row.  Tuning builds (hipcc -DAZG_TUNING; tools/sweep_small.py, sweep_tower.py, sweep_arena.py) let the
// environment override the choice among the pair's rows: AZG_TOWER_BOARDS, AZG_TOWER_PSPLIT; the product library reads no environment.
static int dispatch_tower(hipStream_t s, int game, int channels, const TowerParams &P) {
#ifdef AZG_TUNING
    static const int forced = getenv("AZG_TOWER_BOARDS") ? atoi(getenv("AZG_TOWER_BOARDS")) : 0;
    static const int psplit = getenv("AZG_TOWER_PSPLIT") ? atoi(getenv("AZG_TOWER_PSPLIT")) : 0;
#else
    constexpr int forced = 0, psplit = 0;
#endif
    int cus = 1;
    { const int r = device_cus(&cus); if (r != AZG_OK) return r; }
    const TilePick t = tower_tile_pick(game, channels, P.boards, cus, forced, psplit);    // (bt == 0: a pair without a tower -- no row matches)
    return tower_tile_launch(s, game, channels, t.bt, t.ps, t.ks, P);
}

// TowerParams by name: the tower's own fields; a launch then sets the heads it has, everything else stays null / 0
static TowerParams tower_params(const void *x, const void *w, const float *bias, const float *pre_scale, const float *pre_shift, int boards, int nblocks) {
    TowerParams P{};
    P.x = x; P.w = w; P.bias = bias; P.pre_scale = pre_scale; P.pre_shift = pre_shift; P.boards = boards; P.nblocks = nblocks;
    return P;
}
static void set_fused_heads(TowerParams &P, const void *head_w, const float *head_b, float *policy, float *value, int A, int NV) {
    P.head_w = head_w; P.head_b = head_b; P.policy = policy; P.value = value; P.A = A; P.NV = NV;
}
static void set_fact_heads(TowerParams &P, const void *head1_w, const float *head1_b, void *feat, int feat_k) {
    P.head1_w = head1_w; P.head1_b = head1_b; P.feat = feat; P.feat_k = feat_k;
}

// ---- argument checks and fills the launches below share (`if (int r = ...) return r;`: AZG_OK is 0) ------------------------------------
// a tower with residual blocks needs their affines
static int check_affine(int nblocks, const void *pre_scale, const void *pre_shift) {
    return nblocks > 0 && (!pre_scale || !pre_shift) ? fail(AZG_E_INVALID_ARG, "pre_scale/pre_shift required") : AZG_OK;
}
// the head features of the persistent wide-head launches: 16 per cell
static int check_search_feat_k(const azg_engine *e, int feat_k) {
    const int hw = e->gi.obs_h * e->gi.obs_w;
    return feat_k != (hw * 16 + 31) / 32 * 32 ? fail(AZG_E_INVALID_ARG, "feat_k must be H*W*16 rounded up to 32") : AZG_OK;
}
// player -> model of an arena launch, from the host's player_to_index (null: the launch seats by slot, seat_of_slot)
static int seat_map(const azg_engine *e, const int32_t *p2i_host, int nmodels, SeatMap &seat) {
    if (p2i_host) for (int i = 0; i < e->gi.num_players && i < 8; i++) {
        if (p2i_host[i] < 0 || p2i_host[i] >= nmodels) return fail(AZG_E_INVALID_ARG, "player_to_index entry out of range");
        seat.v[i] = p2i_host[i];
    }
    return AZG_OK;
}
// TowerParams of a fused-heads launch of `nmodels` models (model 0: the tower's own fields, model m > 0: alt[m - 1]); every model brings
// all its parameters
static int fused_models_params(TowerParams &P, const void *x, int boards, float *policy, float *value, int A, int NV, int nmodels, const void *const *w,
                               const float *const *bias, const float *const *pre_scale, const float *const *pre_shift, int nblocks,
                               const void *const *head_w, const float *const *head_b) {
    for (int m = 0; m < nmodels; m++)
        if (!w[m] || !bias[m] || !head_w[m] || !head_b[m] || (nblocks > 0 && (!pre_scale || !pre_shift || !pre_scale[m] || !pre_shift[m])))
            return fail(AZG_E_INVALID_ARG, "null model parameter");
    const auto model = [&](int m) {
        return TowerParams::Model{w[m], bias[m], nblocks ? pre_scale[m] : nullptr, nblocks ? pre_shift[m] : nullptr, head_w[m], head_b[m]};
    };
    const TowerParams::Model m0 = model(0);
    P = tower_params(x, m0.w, m0.bias, m0.pre_scale, m0.pre_shift, boards, nblocks);
    set_fused_heads(P, m0.head_w, m0.head_b, policy, value, A, NV); P.nmodels = nmodels;
    for (int m = 1; m < nmodels; m++) P.alt[m - 1] = model(m);
    return AZG_OK;
}

// the end of every stand-alone tower entry point: the launch's tile for this device, timed as the tower family
static int run_tower(void *stream, int game, int channels, const TowerParams &P) {
    NetProfScope timed((hipStream_t)stream, 0);
    return dispatch_tower((hipStream_t)stream, game, channels, P);
}

// The fused search launches (azg_search_f16, azg_search_arena_f16) run on the rows of AZG_TOWER_TILES that is_fused_search_tile names
// (azg_tiles.h): SA's kernel on the row of bt games per workgroup.  The arena launch is built for one game per workgroup only.
template <class SA, class G, int C, int BT, int PS, int KS> constexpr bool fused_search_row = is_fused_search_tile<G, C, PS, KS> && (BT == 1 || !SA::ARENA);
template <class G, int C, int BT, int PS, int KS, class SA>
static int fused_search_tile_launch(hipStream_t s, const TowerParams &P, const SA &sa, bool init) {
    if constexpr (fused_search_row<SA, G, C, BT, PS, KS>) return launch_tower<G::H, G::W, BT, C, PS, SA, KS>(s, P, sa, init);
    else return AZG_E_UNSUPPORTED;
}
template <class SA>
static int fused_search_launch(hipStream_t s, const TowerParams &P, const SA &sa, int bt, bool init) {
#define AZG_ROW(G, C, BT, PS, KS, LIMIT) \
    if (fused_search_row<SA, G, C, BT, PS, KS> && bt == BT) return fused_search_tile_launch<G, C, BT, PS, KS>(s, P, sa, init);
    AZG_TOWER_TILES(AZG_ROW)
#undef AZG_ROW
    return fail(AZG_E_INTERNAL, "the fused search kernel has no tile of this many games per workgroup");
}

// [boards, C, H*W] f32 planes (what GameState.observation / the reference's batch tensors hold) -> the tower's input rows [boards * H*W][8] fp16
__global__ __launch_bounds__(256) void k_obs_to_nhwc8(const float *src, half8 *dst, int n, int C, int HW) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int b = i / HW, pos = i - b * HW;
    half8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int c = 0; c < C; c++) v[c] = (_Float16)src[((size_t)b * C + c) * HW + pos];
    dst[i] = v;
}
extern "C" int azg_obs_to_nhwc8_f16(void *stream, const float *obs, int boards, int channels, int hw, void *x) {
    if (!obs || !x || boards <= 0 || channels <= 0 || channels > 8 || hw <= 0) return fail(AZG_E_INVALID_ARG, "null or out-of-range argument (channels <= 8)");
    const int n = boards * hw;
    hipLaunchKernelGGL(k_obs_to_nhwc8, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, obs, (half8 *)x, n, channels, hw);
    HIPCHK(hipGetLastError());
    return AZG_OK;
}

extern "C" int azg_resnet_tower_f16(void *stream, int game, const void *x, const void *w, const float *bias, const float *pre_scale,
                                    const float *pre_shift, void *y, int boards, int nblocks, int channels) {
    if (!x || !w || !bias || !y || boards <= 0 || nblocks < 0) return fail(AZG_E_INVALID_ARG, "null argument");
    if (int r = check_affine(nblocks, pre_scale, pre_shift)) return r;
    TowerParams P = tower_params(x, w, bias, pre_scale, pre_shift, boards, nblocks); P.y = y;
    return run_tower(stream, game, channels, P);
}

extern "C" int azg_resnet_tower_features_f16(void *stream, int game, const void *x, const void *w, const float *bias, const float *pre_scale,
                                             const float *pre_shift, int boards, int nblocks, int channels, const void *head1_w, const float *head1_b,
                                             void *feat, int feat_k) {
    if (!x || !w || !bias || !head1_w || !head1_b || !feat || boards <= 0 || nblocks < 0) return fail(AZG_E_INVALID_ARG, "null argument");
    if (int r = check_affine(nblocks, pre_scale, pre_shift)) return r;
    if (feat_k <= 0 || (feat_k & 31)) return fail(AZG_E_INVALID_ARG, "feat_k must be a positive multiple of 32");
    TowerParams P = tower_params(x, w, bias, pre_scale, pre_shift, boards, nblocks);
    set_fact_heads(P, head1_w, head1_b, feat, feat_k);
    return run_tower(stream, game, channels, P);
}

extern "C" int azg_resnet_policy_value_f16(void *stream, int game, const void *x, const void *w, const float *bias, const float *pre_scale,
                                           const float *pre_shift, int boards, int nblocks, const void *head_w, const float *head_b,
                                           int A, int NV, float *policy, float *value) {
    if (!x || !w || !bias || !head_w || !head_b || !policy || !value || boards <= 0 || nblocks < 0) return fail(AZG_E_INVALID_ARG, "null argument");
    if (A <= 0 || NV <= 0 || A + NV > 16) return fail(AZG_E_UNSUPPORTED, "fused heads need A + NV <= 16");
    if (int r = check_affine(nblocks, pre_scale, pre_shift)) return r;
    TowerParams P = tower_params(x, w, bias, pre_scale, pre_shift, boards, nblocks);
    set_fused_heads(P, head_w, head_b, policy, value, A, NV);
    return run_tower(stream, game, 128, P);
}

extern "C" int azg_resnet_policy_value_multi_f16(void *stream, int game, const void *x, int nmodels, const void *const *w, const float *const *bias,
                                                 const float *const *pre_scale, const float *const *pre_shift, int max_boards, int nblocks,
                                                 const void *const *head_w, const float *const *head_b, int A, int NV, float *policy, float *value,
                                                 const int32_t *rows_per_model) {
    if (!x || !w || !bias || !head_w || !head_b || !policy || !value || !rows_per_model || max_boards <= 0 || nblocks < 0)
        return fail(AZG_E_INVALID_ARG, "null or out-of-range argument");
    if (nmodels < 1 || nmodels > 4) return fail(AZG_E_UNSUPPORTED, "1 to 4 models per launch");
    if (A <= 0 || NV <= 0 || A + NV > 16) return fail(AZG_E_UNSUPPORTED, "fused heads need A + NV <= 16");
    if (int r = check_affine(nblocks, pre_scale, pre_shift)) return r;
    // the grid is sized for max_boards rows plus one partial tile per extra model
    TowerParams P;
    if (int r = fused_models_params(P, x, max_boards, policy, value, A, NV, nmodels, w, bias, pre_scale, pre_shift, nblocks, head_w, head_b)) return r;
    P.rows_per_model = rows_per_model;
    return run_tower(stream, game, 128, P);
}

extern "C" int azg_search_f16(azg_engine *e, void *stream, const void *w, const float *bias, const float *pre_scale, const float *pre_shift,
                              int nblocks, const void *head_w, const float *head_b, int sims) {
    if (!e || !w || !bias || !head_w || !head_b || nblocks < 0 || sims < 0) return fail(AZG_E_INVALID_ARG, "null or out-of-range argument");
    if (int r = check_affine(nblocks, pre_scale, pre_shift)) return r;
    if (e->cfg.game != AZG_GAME_CONNECT4 || e->v.arena)
        return fail(AZG_E_UNSUPPORTED, "the fused search kernel is built for connect4 self-play with a 128-channel tower (use azg_select / network / azg_backup)");
    const int A = e->gi.action_size, NV = e->gi.num_players + 1;
    TowerParams P = tower_params(nullptr, w, bias, pre_scale, pre_shift, e->v.B, nblocks);
    set_fused_heads(P, head_w, head_b, nullptr, nullptr, A, NV);
    // games per workgroup: the stand-alone tower's tile for as many boards (tower_tile_pick).  Small engines -- the single-tree MCTS class, config 1's 32 games --
    // take one game per workgroup (a lone 4-board tile runs at the tower's latency for four boards: 170 us per simulation against ~60)
    int cus = 1;
    if (int r = device_cus(&cus)) return r;
    NetProfScope timed((hipStream_t)stream, 2, sims > 0);
    return fused_search_launch((hipStream_t)stream, P, SearchArgs<C4>{e->v, sims}, tower_tile_pick(AZG_GAME_CONNECT4, 128, e->v.B, cus).bt, sims == 0);   // sims == 0: set up only
}

extern "C" int azg_search_arena_f16(azg_engine *e, void *stream, int nmodels, const void *const *w, const float *const *bias, const float *const *pre_scale,
                                    const float *const *pre_shift, int nblocks, const void *const *head_w, const float *const *head_b,
                                    const int32_t *p2i_host, const uint32_t *seat_of_slot, int sims) {
    if (!e || !w || !bias || !head_w || !head_b || nblocks < 0 || sims < 0 || (!p2i_host && !seat_of_slot)) return fail(AZG_E_INVALID_ARG, "null or out-of-range argument");
    if (e->cfg.game != AZG_GAME_CONNECT4 || !e->v.arena)
        return fail(AZG_E_UNSUPPORTED, "the persistent arena launch is built for connect4 arena engines with 128-channel towers (use azg_select / network / azg_backup)");
    if (nmodels < 1 || nmodels > 4 || nmodels < e->gi.num_players) return fail(AZG_E_UNSUPPORTED, "one model per player, at most 4");
    TowerParams P;
    if (int r = fused_models_params(P, nullptr, e->v.B, nullptr, nullptr, e->gi.action_size, e->gi.num_players + 1, nmodels, w, bias, pre_scale, pre_shift,
                                    nblocks, head_w, head_b)) return r;
    SearchArena<C4> sa{e->v, sims, SeatMap{}, seat_of_slot};
    if (int r = seat_map(e, p2i_host, nmodels, sa.seat)) return r;
    NetProfScope timed((hipStream_t)stream, 2, sims > 0);
    return fused_search_launch((hipStream_t)stream, P, sa, 1, sims == 0);   // sims == 0: set up only
}

// ---- the persistent wide-head search launch: tiles, the device-derived tile model, the set-up autotune ----------------------------------
#ifdef AZG_TUNING
static int wide_forced_tile() { static const int f = getenv("AZG_WIDE_BOARDS") ? atoi(getenv("AZG_WIDE_BOARDS")) : 0; return f; }
#else
static constexpr int wide_forced_tile() { return 0; }
#endif

// ONE tile shape of the launch (bt games per workgroup) for (game, tower width): the row of AZG_WIDE_TILES; AZG_E_UNSUPPORTED: no such tile.
// sparse heads (EXACT = false: hd; the pairs with has_sparse_heads only) or full-width heads (EXACT = true: hf).  init: one-time set-up
// only.  occ: see launch_tower.
template <bool EXACT>
static int wide_tile_launch(azg_engine *e, hipStream_t s, const TowerParams &P, int channels, int bt, const HeadRows &hd, const HeadsFull &hf, int sims,
                            bool init, int *occ) {
    const int game = e->cfg.game;
#ifdef AZG_TUNING
    if (game == AZG_GAME_BRANDUBH && channels == 64) {             // AZG_WIDE_BOARDS codes: one workgroup per CU
        using SW = SearchWide<BR, 1, EXACT>;
        const SW sa{e->v, sims, hd, hf};
        if (bt == 8) return launch_tower<BR::H, BR::W, 8, 64, 4, SW>(s, P, sa, init, occ);         // one workgroup of eight wavefronts per CU
        if (bt == 12) return launch_tower<BR::H, BR::W, 2, 64, 2, SW, 2>(s, P, sa, init, occ);     // 2 games, 8 wavefronts (k-split), one workgroup per CU
        if (bt == 14) return launch_tower<BR::H, BR::W, 4, 64, 2, SW>(s, P, sa, init, occ);        // (what the spills cost: the 4-board tile with the whole register file)
    }
    if (game == AZG_GAME_TRIMOK && channels == 32 && bt == 4)
        return launch_tower<TM::H, TM::W, 4, 32, 4, SearchWide<TM, 2, EXACT>>(s, P, SearchWide<TM, 2, EXACT>{e->v, sims, hd, hf}, init, occ);
#endif
#define AZG_ROW(G, C, BT, PS, MINB, KS) \
    if constexpr (EXACT || has_sparse_heads<G>) if (game == G::ID && channels == C && bt == BT) { \
        using SW = SearchWide<G, MINB, EXACT>; \
        return launch_tower<G::H, G::W, BT, C, PS, SW, KS>(s, P, SW{e->v, sims, hd, hf}, init, occ); }
    AZG_WIDE_TILES(AZG_ROW)
#undef AZG_ROW
    return AZG_E_UNSUPPORTED;
}

// The tile model (used when no measurement exists: a launch that is being captured without a set-up call before it).  Nothing in it is
// a constant of one chip or one depth: a tile of t games gives n = ceil(B / t) workgroups; they run in rounds of cus x occ(t) (CU count of
// THIS device x the occupancy query of the tile's kernel with its LDS for THIS depth); a workgroup's chain per simulation is
// fixed(t) [tree phase + heads] + conv(t) x (2 nblocks + 1) [the tower], in k cycles, from the phase stamps of the measurement build
// (profiles/r05_phase_budget.json, r05_wide_tile_sweep.txt: brandubh 4-block chain exact 83 / 105 / 123 / 161, sparse 54 / 83 / 109 / 146 at
// 1 / 2 / 3 / 4 games per workgroup, of which the tower 37 / 62 / 78 / 100 -- i.e. per conv 4.1 / 6.9 / 8.7 / 11.1); a last round that
// fills at most half of the chip's slots runs without a neighbour on its CU (x 0.82: 70 vs 83 ... 124 vs 161 measured).
template <bool EXACT>
static int wide_tile_model(azg_engine *e, int channels, int nblocks, int cus, const int *occ) {
    const int game = e->cfg.game, B = e->v.B, tmax = wide_max_tile(game, channels);
    if (game != AZG_GAME_BRANDUBH) {
        // (othello has no phase budget of its own yet: this prior, and the set-up trial of every tile, decide)
        // one game per workgroup up to two games per CU (3-player env, M expansions/s at 256 / 512 / 1024 games on 256 CUs: one game per
        // workgroup 20.7 / 37.4 / 39.4, two 16.3 / 31.3 / 48.0: profiles/r05_wide_tile_sweep.txt); beyond that the shared weight stream wins
        return (occ[0] > 0 && B <= 2 * cus) || tmax < 2 || occ[1] <= 0 ? 1 : 2;
    }
    static const double fixed_exact[4] = {46, 43, 45, 61}, fixed_sparse[4] = {17, 21, 31, 46}, conv[4] = {4.1, 6.9, 8.7, 11.1};
    int bt = 1; double best = -1;
    for (int t = 1; t <= tmax; t++) {
        if (occ[t - 1] <= 0) continue;                          // this tile does not fit (LDS: too deep a tower)
        const long round = (long)cus * occ[t - 1], n = (B + t - 1) / t, full = n / round, rem = n % round;
        const double chain = (EXACT ? fixed_exact : fixed_sparse)[t - 1] + conv[t - 1] * (2 * nblocks + 1);
        const double cost = full * chain + (rem == 0 ? 0 : rem * 2 <= round ? 0.82 * chain : chain);
        if (best < 0 || cost < best) { best = cost; bt = t; }
    }
    return bt;
}

// what was decided for (device, game, width, heads, engine size, depth): tile, where it came from (0 model, 1 measured at set-up, 2 forced)
struct WideTileKey { int dev, game, channels, exact, B, nblocks; bool operator<(const WideTileKey &o) const { return memcmp(this, &o, sizeof(*this)) < 0; } };
struct WideTilePick { int bt, source, occ; float us[4]; };
static std::mutex g_tile_mu;
static std::map<WideTileKey, WideTilePick> g_tile;

// Set-up autotune (sims == 0, never inside a capture): every tile shape this (game, width) has is timed ONCE on a scratch engine of the same
// size -- fresh games, a node store for the trial only -- with THIS network: a warm launch, then two timed launches of 40 simulations, each
// from fresh trees (the shorter of the two counts); the fastest is the engine's tile for (B, nblocks) from then on.  Tile shape changes no
// result (every shape is bit-identical to the launch-per-phase form: tests/test_gpu_fullsize.py), so the measurement only decides speed.
// The model's tile is the prior: a trial has to beat it by more than 3 % to replace it.  Falls back to the model when the scratch engine
// cannot be had (memory).
static constexpr int TRIAL_SIMS = 40;                        // simulations per trial launch (reported by azg_search_wide_tile_info)

template <bool EXACT>
static int wide_tile_autotune(azg_engine *e, hipStream_t s, const TowerParams &P, int channels, const HeadRows &hd, const HeadsFull &hf, const int *occ,
                              WideTilePick &pick) {
    const int tmax = wide_max_tile(e->cfg.game, channels);
    // (8 simulations on fresh trees could not tell the 2- from the 3-game tile of an 8-block tower: 1 % apart in the trial, 20 % at 40
    //  simulations -- the solo tree phase slows down as the trees grow; and 24 simulations timed on trees already grown by 24 put the 1- and
    //  2-game tiles of a 4-block tower at 512 games 1-3 % apart, where launches of 40 simulations from fresh trees separate them by 7-9 %)
    constexpr int TRIAL_TIMED = 2;
    azg_config cfg = e->cfg;
    cfg.sims_per_move = TRIAL_SIMS; cfg.nodes_per_tree = (2 * TRIAL_SIMS + 2) * e->gi.max_children + 64;
    cfg.example_capacity = 0; cfg.result_capacity = 0; cfg.temp_table = nullptr; cfg.temp_table_len = 0; cfg.arena = 0;
    azg_engine *tmp = nullptr;
    if (azg_engine_create(&cfg, &tmp) != AZG_OK || !tmp) return AZG_E_HIP;
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { azg_engine_destroy(tmp); return AZG_E_HIP; }
    int best = 0; float best_ms = 0;
    for (int t = 1; t <= tmax; t++) {
        pick.us[t - 1] = 0;
        if (occ[t - 1] <= 0) continue;
        if (azg_engine_reset(tmp, s) != AZG_OK) continue;
        TowerParams Q = P; Q.boards = tmp->v.B;
        if (wide_tile_launch<EXACT>(tmp, s, Q, channels, t, hd, hf, TRIAL_SIMS, false, nullptr) != AZG_OK) continue;
        float tile_ms = 0;
        for (int k = 0; k < TRIAL_TIMED; k++) {
            if (azg_engine_reset(tmp, s) != AZG_OK) { tile_ms = 0; break; }
            (void)hipEventRecord(a, s);
            const int r = wide_tile_launch<EXACT>(tmp, s, Q, channels, t, hd, hf, TRIAL_SIMS, false, nullptr);
            (void)hipEventRecord(b, s);
            if (r != AZG_OK || hipEventSynchronize(b) != hipSuccess) { tile_ms = 0; break; }
            float ms = 0; (void)hipEventElapsedTime(&ms, a, b);
            if (k == 0 || ms < tile_ms) tile_ms = ms;
        }
        if (tile_ms <= 0) continue;
        pick.us[t - 1] = tile_ms * 1e3f;
        if (!best || tile_ms < best_ms) { best = t; best_ms = tile_ms; }
    }
    (void)hipEventDestroy(a); (void)hipEventDestroy(b);
    azg_engine_destroy(tmp);
    (void)hipGetLastError();
    if (!best) return AZG_E_HIP;
    // hysteresis: the model's tile (pick.bt on entry) stands unless the fastest trial beats ITS trial by more than 3 % -- near-ties (8 blocks x
    // 512 brandubh games: one and two games per workgroup are 2 % apart) would otherwise flip with the noise of a single timing, and under a
    // profiler, which serialises and slows the trials, the kernel a run is measured on must not depend on which pass it is
    const int prior = pick.bt;
    if (prior >= 1 && prior <= tmax && pick.us[prior - 1] > 0 && best_ms * 1e3f >= 0.97f * pick.us[prior - 1]) best = prior;
    pick.bt = best; pick.source = 1;
    return AZG_OK;
}

template <bool EXACT>
static int wide_tile_pick(azg_engine *e, hipStream_t s, const TowerParams &P, int channels, const HeadRows &hd, const HeadsFull &hf, bool setup, WideTilePick &out) {
    int dev = 0, cus = 1;
    HIPCHK(hipGetDevice(&dev));
    int r = device_cus(&cus); if (r != AZG_OK) return r;
    const WideTileKey key{dev, e->cfg.game, channels, EXACT ? 1 : 0, e->v.B, P.nblocks};
    {
        std::lock_guard<std::mutex> lk(g_tile_mu);
        auto it = g_tile.find(key);
        if (it != g_tile.end() && (it->second.source != 0 || !setup)) { out = it->second; return AZG_OK; }
    }
    WideTilePick pick{1, 0, 1, {0, 0, 0, 0}};
    const int tmax = wide_max_tile(e->cfg.game, channels);
    if (tmax == 0) return AZG_E_UNSUPPORTED;
    if (wide_forced_tile()) {
        pick.bt = wide_forced_tile(); pick.source = 2;
        r = wide_tile_launch<EXACT>(e, s, P, channels, pick.bt, hd, hf, 0, true, &pick.occ);
        if (r != AZG_OK) return r;
    } else {
        // (no first-use allocation inside a capture, so no tile can be set up there: the set-up call comes first)
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing(s, &cs);
        if (cs != hipStreamCaptureStatusNone)
            return fail(AZG_E_INVALID_ARG, "persistent wide-head search: call it once with sims == 0 (one-time set-up) before capturing it in a graph");
        int occ[4] = {0, 0, 0, 0};
        for (int t = 1; t <= tmax; t++) {                        // set up every tile this network fits; its occupancy on this device
            int o = 0;
            if (wide_tile_launch<EXACT>(e, s, P, channels, t, hd, hf, 0, true, &o) == AZG_OK) occ[t - 1] = o;
        }
        bool any = false;
        for (int t = 0; t < tmax; t++) any |= occ[t] > 0;
        if (!any) return fail(AZG_E_INVALID_ARG, "this tower does not fit the LDS of any tile of the persistent launch (too many residual blocks)");
        pick.bt = wide_tile_model<EXACT>(e, channels, P.nblocks, cus, occ);
        if (setup && !e->v.perm_tape) (void)wide_tile_autotune<EXACT>(e, s, P, channels, hd, hf, occ, pick);   // (failure: the model's pick stands)
        pick.occ = occ[pick.bt - 1];
    }
    std::lock_guard<std::mutex> lk(g_tile_mu);
    g_tile[key] = pick;
    out = pick;
    return AZG_OK;
}

template <bool EXACT>
static int search_wide(azg_engine *e, void *stream, const void *w, const float *bias, const float *pre_scale, const float *pre_shift, int nblocks, int channels,
                       const void *head1_w, const float *head1_b, const HeadRows &hd, const HeadsFull &hf, int feat_k, int sims) {
    if (!e || !w || !bias || !head1_w || !head1_b || nblocks < 0 || sims < 0) return fail(AZG_E_INVALID_ARG, "null or out-of-range argument");
    if (int r = check_affine(nblocks, pre_scale, pre_shift)) return r;
    if (e->v.arena) return fail(AZG_E_UNSUPPORTED, "the persistent search launches are built for self-play engines");
    const int A = e->gi.action_size, NV = e->gi.num_players + 1;
    if (int r = check_search_feat_k(e, feat_k)) return r;
    if (wide_max_tile(e->cfg.game, channels) == 0)
        return fail(AZG_E_UNSUPPORTED, "persistent wide-head search: built for the pairs azg_launch_support gives AZG_SUPPORT_SEARCH_WIDE (use azg_select / network / azg_backup)");
#define AZG_NO_SPARSE(G, ...) \
    if (!EXACT && !G::SPARSE_HEADS && e->cfg.game == G::ID) return fail(AZG_E_UNSUPPORTED, std::string("no sparse heads for ") + G::NAME + " (use the exact persistent launch)");
    AZG_GAMES(AZG_NO_SPARSE)
#undef AZG_NO_SPARSE
    TowerParams P = tower_params(nullptr, w, bias, pre_scale, pre_shift, e->v.B, nblocks);
    set_fact_heads(P, head1_w, head1_b, nullptr, feat_k); P.A = A; P.NV = NV;
    hipStream_t s = (hipStream_t)stream;
    // Games per workgroup by the engine's size (SelfPlayAgent.pyx:23-26: the batch is whatever the caller made it): measured at set-up
    // (sims == 0) on this device with this network, else the device-derived model above.  More boards per tile share every weight fragment
    // between the tile's boards, pad fewer pixel lanes (brandubh: 196 of 208 instead of 49 of 64) and have a main loop long enough to
    // amortise a layer's epilogue and barriers; fewer fill the chip at small engines.
    WideTilePick pick;
    int r = wide_tile_pick<EXACT>(e, s, P, channels, hd, hf, sims == 0, pick);
    if (r != AZG_OK) return r;
    if (sims == 0) return AZG_OK;                            // one-time set-up only
    NetProfScope timed(s, 2);
    r = wide_tile_launch<EXACT>(e, s, P, channels, pick.bt, hd, hf, sims, false, nullptr);
    if (r == AZG_E_UNSUPPORTED) return fail(r, "persistent wide-head search: no such tile for this game / width");
    return r;
}

// the tile a wide-head engine searches with: info12 = {games per workgroup, workgroups of a launch, workgroups a CU holds at once, CUs of the
// device, source (0 device-derived model, 1 measured at set-up, 2 forced by a tuning build), trial simulations, 0, 0, then the set-up
// measurement in ns per trial launch for 1 / 2 / 3 / 4 games per workgroup (0: not measured)}; AZG_E_INVALID_ARG before the first call of the
// launch for this (engine size, depth)
extern "C" int azg_search_wide_tile_info(azg_engine *e, int channels, int nblocks, int exact, int32_t *info12) {
    if (!e || !info12) return fail(AZG_E_INVALID_ARG, "null argument");
    int dev = 0, cus = 1;
    HIPCHK(hipGetDevice(&dev));
    int r = device_cus(&cus); if (r != AZG_OK) return r;
    std::lock_guard<std::mutex> lk(g_tile_mu);
    auto it = g_tile.find(WideTileKey{dev, e->cfg.game, channels, exact ? 1 : 0, e->v.B, nblocks});
    if (it == g_tile.end()) return fail(AZG_E_INVALID_ARG, "no persistent wide-head launch has been set up for this engine size and depth");
    const WideTilePick &p = it->second;
    info12[0] = p.bt; info12[1] = (e->v.B + p.bt - 1) / p.bt; info12[2] = p.occ; info12[3] = cus; info12[4] = p.source;
    info12[5] = TRIAL_SIMS; info12[6] = info12[7] = 0;
    for (int t = 0; t < 4; t++) info12[8 + t] = (int32_t)(p.us[t] * 1e3f);
    return AZG_OK;
}

extern "C" int azg_search_wide_f16(azg_engine *e, void *stream, const void *w, const float *bias, const float *pre_scale, const float *pre_shift,
                                   int nblocks, int channels, const void *head1_w, const float *head1_b, const void *head_rows, const float *head_b,
                                   int feat_k, int sims) {
    if (!head_rows || !head_b) return fail(AZG_E_INVALID_ARG, "null argument");
    return search_wide<false>(e, stream, w, bias, pre_scale, pre_shift, nblocks, channels, head1_w, head1_b, HeadRows{(const _Float16 *)head_rows, head_b, feat_k},
                              HeadsFull{}, feat_k, sims);
}

extern "C" int azg_search_wide_exact_f16(azg_engine *e, void *stream, const void *w, const float *bias, const float *pre_scale, const float *pre_shift,
                                         int nblocks, int channels, const void *head1_w, const float *head1_b, const void *wps_packed, const void *wv_packed,
                                         const float *head_b, int feat_k, int sims) {
    if (!e || !wps_packed || !wv_packed || !head_b) return fail(AZG_E_INVALID_ARG, "null argument");
    return search_wide<true>(e, stream, w, bias, pre_scale, pre_shift, nblocks, channels, head1_w, head1_b, HeadRows{nullptr, head_b, feat_k},
                             HeadsFull{(const half8 *)wps_packed, (const half8 *)wv_packed, head_b}, feat_k, sims);
}

// the wide arena launch: the one-game row of each (game, width) in AZG_WIDE_TILES -- the self-play launch's bt == 1 shape (arena shards
// are small: the default arenaCompare of 128 games is below the CU count), no tile autotune
template <class G, int C, int BT, int PSPLIT, int MINB, int KSPLIT>
static int wide_arena_tile(hipStream_t s, const TowerParams &P, const WideArenaArgs &a, bool init) {
    if constexpr (BT == 1) {
        SearchWideArena<G, MINB> sa;
        static_cast<WideArenaArgs &>(sa) = a;
        return launch_tower<G::H, G::W, 1, C, PSPLIT, SearchWideArena<G, MINB>, KSPLIT>(s, P, sa, init);
    }
    return AZG_E_UNSUPPORTED;
}

extern "C" int azg_search_arena_wide_exact_f16(azg_engine *e, void *stream, int nmodels, const void *const *w, const float *const *bias,
                                               const float *const *pre_scale, const float *const *pre_shift, int nblocks, int channels,
                                               const void *const *head1_w, const float *const *head1_b, const void *const *wps,
                                               const void *const *wv, const float *const *head_b, int feat_k, const int32_t *p2i_host,
                                               const uint32_t *seat_of_slot, int sims) {
    if (!e || !w || !bias || !pre_scale || !pre_shift || !head1_w || !head1_b || !wps || !wv || !head_b || nblocks < 0 || sims < 0 || (!p2i_host && !seat_of_slot))
        return fail(AZG_E_INVALID_ARG, "null or out-of-range argument");
    const int game = e->cfg.game;
    if (!e->v.arena || wide_max_tile(game, channels) == 0)
        return fail(AZG_E_UNSUPPORTED, "the persistent wide arena launch is built for arena engines on the pairs azg_launch_support gives "
                                       "AZG_SUPPORT_SEARCH_WIDE (use azg_select / network / azg_backup)");
    if (nmodels < e->gi.num_players || nmodels > 4) return fail(AZG_E_INVALID_ARG, "one model per player, at most 4");
    const int A = e->gi.action_size, NV = e->gi.num_players + 1;
    if (int r = check_search_feat_k(e, feat_k)) return r;
    WideArenaArgs sa0{};
    sa0.ev = e->v; sa0.sims = sims; sa0.hd = HeadRows{nullptr, nullptr, feat_k}; sa0.seat_of_slot = seat_of_slot; sa0.nmodels = nmodels;
    int real = -1;
    for (int m = 0; m < nmodels; m++) {
        const bool ps = nblocks == 0 || (pre_scale[m] && pre_shift[m]), ps_null = nblocks == 0 || (!pre_scale[m] && !pre_shift[m]);
        const bool all = w[m] && bias[m] && ps && head1_w[m] && head1_b[m] && wps[m] && wv[m] && head_b[m];
        const bool none = !w[m] && !bias[m] && ps_null && !head1_w[m] && !head1_b[m] && !wps[m] && !wv[m] && !head_b[m];
        if (!all && !none) return fail(AZG_E_INVALID_ARG, "a model's parameters must be all set (a network) or all null (a raw seat)");
        if (all) {
            sa0.m[m] = WideModel{w[m], bias[m], nblocks ? pre_scale[m] : nullptr, nblocks ? pre_shift[m] : nullptr, head1_w[m], head1_b[m],
                                 HeadsFull{(const half8 *)wps[m], (const half8 *)wv[m], head_b[m]}};
            if (real < 0) real = m;
        }
    }
    if (int r = seat_map(e, p2i_host, nmodels, sa0.seat)) return r;
    // (P: the shape of the launch -- boards, depth, heads form; the parameters every workgroup reads are its model's, sa.m)
    const WideModel &M0 = sa0.m[real < 0 ? 0 : real];
    TowerParams P = tower_params(nullptr, M0.w, M0.bias, M0.pre_scale, M0.pre_shift, e->v.B, nblocks);
    set_fact_heads(P, M0.head1_w, M0.head1_b, nullptr, feat_k); P.A = A; P.NV = NV;
    hipStream_t s = (hipStream_t)stream;
    const bool init = sims == 0;                                  // sims == 0: set up only
    NetProfScope timed(s, 2, !init);
    int r = AZG_E_UNSUPPORTED;
#define AZG_ROW(G, C, BT, PS, MINB, KS) if (BT == 1 && game == G::ID && channels == C) r = wide_arena_tile<G, C, BT, PS, MINB, KS>(s, P, sa0, init);
    AZG_WIDE_TILES(AZG_ROW)
#undef AZG_ROW
    if (r == AZG_E_UNSUPPORTED) return fail(r, "persistent wide arena launch: no tile for this game / width");
    return r;
}

extern "C" int azg_policy_value_heads_f16(void *stream, const void *y, const void *head_w_packed, const float *head_b, int boards, int k,
                                          int A, int NV, float *logits_ws, float *policy, float *value) {
    if (!y || !head_w_packed || !head_b || !logits_ws || (!policy != !value)) return fail(AZG_E_INVALID_ARG, "null argument");
    if (boards <= 0 || k <= 0 || (k & 31) || A <= 0 || A > 1024 || NV <= 0 || NV > 64) return fail(AZG_E_INVALID_ARG, "boards > 0, k a multiple of 32, 0 < A <= 1024, 0 < NV <= 64");
    const int osub = (A + NV + 15) / 16, nchunks = (osub + HEAD_NS - 1) / HEAD_NS, groups = (boards + 15) / 16;
    hipStream_t s = (hipStream_t)stream;
    {
        NetProfScope timed(s, 1);                            // (the GEMM alone: the softmax below is not timed)
        AZG_LAUNCH(k_heads, dim3(groups * nchunks), dim3(HEAD_WAVES * 64), 0, s, (const _Float16 *)y, (const half8 *)head_w_packed, head_b, logits_ws,
                           boards, k / 32, osub);
    }
    if (policy)                                              // (NULL: leave the logits for azg_backup_select_logits)
        AZG_LAUNCH(k_heads_softmax, dim3((boards + 3) / 4), dim3(256), 0, s, (const float *)logits_ws, policy, value, boards, osub * 16, A, NV);
    HIPCHK(hipGetLastError());
    return AZG_OK;
}

extern "C" int azg_policy_value_heads_fact_f16(void *stream, const void *feat, const void *wp_packed, const void *wv_packed, const float *head_b, int boards,
                                               int feat_k, int A, int NV, float *logits_ws, float *policy, float *value) {
    if (!feat || !wp_packed || !wv_packed || !head_b || !logits_ws || (!policy != !value)) return fail(AZG_E_INVALID_ARG, "null argument");
    if (boards <= 0 || feat_k <= 0 || (feat_k & 31) || A <= 0 || A > 1024 || NV <= 0 || NV > 16) return fail(AZG_E_INVALID_ARG, "boards > 0, feat_k a multiple of 32, 0 < A <= 1024, 0 < NV <= 16");
    const int osp = (A + 15) / 16, osub = (A + NV + 15) / 16, nchunks = (osp + HEADF_NS - 1) / HEADF_NS + 1, groups = (boards + 15) / 16;
    hipStream_t s = (hipStream_t)stream;
    const HeadsFact hf{(const half8 *)wp_packed, (const half8 *)wv_packed, head_b, feat_k, osp, A, NV};
    {
        NetProfScope timed(s, 1);                            // (the GEMM alone: the softmax below is not timed)
        AZG_LAUNCH(k_heads_fact, dim3(groups * nchunks), dim3(HEADF_Q * 64), 0, s, (const _Float16 *)feat, hf, logits_ws, boards, osub * 16);
    }
    if (policy)
        AZG_LAUNCH(k_heads_softmax, dim3((boards + 3) / 4), dim3(256), 0, s, (const float *)logits_ws, policy, value, boards, osub * 16, A, NV);
    HIPCHK(hipGetLastError());
    return AZG_OK;
}

extern "C" int azg_heads_softmax(void *stream, const float *logits, int boards, int logits_stride, int A, int NV, float *policy, float *value) {
    if (!logits || !policy || !value) return fail(AZG_E_INVALID_ARG, "null argument");
    if (boards <= 0 || A <= 0 || A > 1024 || NV <= 0 || NV > 64 || logits_stride < A + NV) return fail(AZG_E_INVALID_ARG, "boards > 0, 0 < A <= 1024, 0 < NV <= 64, stride >= A + NV");
    hipLaunchKernelGGL(k_heads_softmax, dim3((boards + 3) / 4), dim3(256), 0, (hipStream_t)stream, logits, policy, value, boards, logits_stride, A, NV);
    HIPCHK(hipGetLastError());
    return AZG_OK;
}

// halves of w_packed a tower launch may read: stem (3 k-steps) + 2 * nblocks convolutions (9 * C/32 k-steps each) + the slack the weight
// prefetch ring runs into behind the last layer.  The deepest ring is the k-split tile's (azg_conv.h conv_main2<..., WR = 9, KSTR = 2>):
// its last prefetch of the last layer is k-step 2 * (8 + 8) + 1 = 33 of an 18 k-step layer -- 16 k-steps past the end; 18 are required.
extern "C" int64_t azg_tower_weights_size(int channels, int nblocks) {
    if (channels <= 0 || (channels & 31) || nblocks < 0) return fail(AZG_E_INVALID_ARG, "channels must be a positive multiple of 32");
    const int64_t kstep = (int64_t)channels * 32;
    return ((int64_t)STEM_KSTEPS + (int64_t)2 * nblocks * 9 * (channels / 32) + AZG_TOWER_W_SLACK_KSTEPS) * kstep;
}

// host-side layout tables of one instantiated tile and the launches a (game, tower width) has: both straight from the tile lists (azg_tiles.h)
extern "C" int azg_tower_layout(int game, int boards_per_tile, int channels, int16_t *pixmap, int32_t *qrow, int32_t *info8) {
    if (!info8) return fail(AZG_E_INVALID_ARG, "null argument");
    const int r = tower_layout(game, boards_per_tile, channels, pixmap, qrow, info8);
    if (r == AZG_E_INTERNAL) return fail(r, "tower pixel map does not fit its subtiles");
    if (r == AZG_E_UNSUPPORTED) return fail(r, "no tower instantiation for this (game, boards per tile, channels)");
    return r;
}

// the stand-alone tower's default tile for `boards` boards on a device of `cus` CUs: tile3 = {boards per tile, PSPLIT, KSPLIT}
extern "C" int azg_tower_tile(int game, int channels, int boards, int cus, int32_t *tile3) {
    if (game < 0 || game >= k_num_games) return fail(AZG_E_INVALID_ARG, "unknown game id");
    if (boards <= 0 || cus <= 0 || !tile3) return fail(AZG_E_INVALID_ARG, "boards > 0, cus > 0, tile3 not null");
    const TilePick t = tower_tile_pick(game, channels, boards, cus);
    if (!t.bt) return fail(AZG_E_UNSUPPORTED, "no MFMA tower for this game / channel count (azg_launch_support: the pairs with AZG_SUPPORT_TOWER)");
    tile3[0] = t.bt; tile3[1] = t.ps; tile3[2] = t.ks;
    return AZG_OK;
}

extern "C" int azg_launch_support(int game, int channels) {
    if (game < 0 || game >= k_num_games) return fail(AZG_E_INVALID_ARG, "unknown game id");
    // tic-tac-toe is built for 32-channel towers only (both of its nets): any other width is refused, not answered with an empty mask
    if (game == AZG_GAME_TICTACTOE && channels != 32) return fail(AZG_E_UNSUPPORTED, "tic-tac-toe has 32-channel launches only");
    // hnefatafl has device rules and no tile row: its network runs outside the library
    if (game == AZG_GAME_HNEFATAFL) return fail(AZG_E_INVALID_ARG, "no network launch is built for this game");
    return tile_support(game, channels);
}

// ---- rules without a tree (csrc/azg_rules.h): the GameState plugin on arrays of positions ---------------------------------------------
#define RULES_SWITCH(game, ...) \
    switch (game) { AZG_GAMES(AZG_GAME_CASE, __VA_ARGS__) default: return fail(AZG_E_INVALID_ARG, "unknown game id"); }

// every argument is judged here, before anything touches the device
extern "C" int azg_game_step(void *stream, int game, int count, const azg_state *states, const int32_t *actions, azg_state *next,
                             uint8_t *valid, uint8_t *win, void *obs, int obs_dtype, int32_t *status) {
    if (game < 0 || game >= k_num_games) return fail(AZG_E_INVALID_ARG, "unknown game id");
    if (count < 0) return fail(AZG_E_INVALID_ARG, "count < 0");
    if (!states) return fail(AZG_E_INVALID_ARG, "null states_dev");
    if (obs_dtype < 0 || obs_dtype > 2) return fail(AZG_E_INVALID_ARG, "obs_dtype must be 0 (float32), 1 (float16) or 2 (float16 NHWC8)");
    if (actions && !status) return fail(AZG_E_INVALID_ARG, "status_dev is required when actions_dev is given");
    if (count == 0) return AZG_OK;
    RULES_SWITCH(game, OBS_SWITCH(obs_dtype, obs,
        hipLaunchKernelGGL((k_game_step<G, OBS, NHWC8>), dim3(count), dim3(64), 0, (hipStream_t)stream, count, states, actions, next, valid,
                           win, o, status)));
    HIPCHK(hipGetLastError());
    return AZG_OK;
}

extern "C" int azg_game_choose(void *stream, int game, int count, const azg_state *states, const float *policy, const float *temp,
                               const double *u, int32_t *actions, int32_t *status) {
    if (game < 0 || game >= k_num_games) return fail(AZG_E_INVALID_ARG, "unknown game id");
    if (count < 0) return fail(AZG_E_INVALID_ARG, "count < 0");
    if (!states) return fail(AZG_E_INVALID_ARG, "null states_dev");
    if (!u) return fail(AZG_E_INVALID_ARG, "null u_dev");
    if (!actions) return fail(AZG_E_INVALID_ARG, "null actions_dev");
    if (!status) return fail(AZG_E_INVALID_ARG, "null status_dev");
    if (count == 0) return AZG_OK;
    RULES_SWITCH(game,
        hipLaunchKernelGGL((k_game_choose<G>), dim3(count), dim3(64), 0, (hipStream_t)stream, count, states, policy, temp, u, actions, status));
    HIPCHK(hipGetLastError());
    return AZG_OK;
}

extern "C" int azg_game_lookahead(void *stream, int game, int count, const azg_state *states, int32_t *num, int32_t *child_actions,
                                  uint8_t *win, azg_state *children, void *obs, int obs_dtype) {
    if (game < 0 || game >= k_num_games) return fail(AZG_E_INVALID_ARG, "unknown game id");
    if (count < 0) return fail(AZG_E_INVALID_ARG, "count < 0");
    if (!states) return fail(AZG_E_INVALID_ARG, "null states_dev");
    if (!num) return fail(AZG_E_INVALID_ARG, "null num_dev");
    if (!child_actions) return fail(AZG_E_INVALID_ARG, "null actions_dev");
    if (obs_dtype < 0 || obs_dtype > 2) return fail(AZG_E_INVALID_ARG, "obs_dtype must be 0 (float32), 1 (float16) or 2 (float16 NHWC8)");
    if (count == 0) return AZG_OK;
    // grid (position, chunk of 64 children): connect4, tic-tac-toe, the 3-player env and othello are one wavefront per position
    RULES_SWITCH(game, OBS_SWITCH(obs_dtype, obs,
        hipLaunchKernelGGL((k_game_lookahead<G, OBS, NHWC8>), dim3(count, (G::MAXK + 63) / 64), dim3(64), 0, (hipStream_t)stream, count, states,
                           num, child_actions, win, children, o)));
    HIPCHK(hipGetLastError());
    return AZG_OK;
}

// G::SCRIPTED and G::NAME of every game, by game id
#define AZG_GAME_SCRIPTED(G_, ...) G_::SCRIPTED,
static constexpr const char *k_game_scripted[] = {AZG_GAMES(AZG_GAME_SCRIPTED)};
#define AZG_GAME_NAME(G_, ...) G_::NAME,
static constexpr const char *k_game_names[] = {AZG_GAMES(AZG_GAME_NAME)};

extern "C" const char *azg_game_scripted_player(int game) {
    if (game < 0 || game >= k_num_games) { fail(AZG_E_INVALID_ARG, "unknown game id"); return nullptr; }
    return k_game_scripted[game];
}

#define AZG_SCRIPTED_CASE(G_, ...) case G_::ID: if constexpr (G_::SCRIPTED != nullptr) { using G = G_; __VA_ARGS__; } break;
extern "C" int azg_game_choose_scripted(void *stream, int game, int count, const azg_state *states, const double *u, int32_t *actions,
                                        int32_t *status) {
    if (game < 0 || game >= k_num_games) return fail(AZG_E_INVALID_ARG, "unknown game id");
    if (count < 0) return fail(AZG_E_INVALID_ARG, "count < 0");
    if (!states) return fail(AZG_E_INVALID_ARG, "null states_dev");
    if (!u) return fail(AZG_E_INVALID_ARG, "null u_dev");
    if (!actions) return fail(AZG_E_INVALID_ARG, "null actions_dev");
    if (!status) return fail(AZG_E_INVALID_ARG, "null status_dev");
    if (!k_game_scripted[game]) return fail(AZG_E_UNSUPPORTED, std::string("the reference has no scripted player for ") + k_game_names[game]);
    if (count == 0) return AZG_OK;
    switch (game) {
        AZG_GAMES(AZG_SCRIPTED_CASE,
            hipLaunchKernelGGL((k_game_choose_scripted<G>), dim3(count), dim3(64), 0, (hipStream_t)stream, count, states, u, actions, status))
        default: break;
    }
    HIPCHK(hipGetLastError());
    return AZG_OK;
}

extern "C" int azg_game_symmetries(void *stream, int game, int count, const azg_state *states, const float *pi, azg_state *sym_states,
                                   float *sym_obs, float *sym_pi) {
    if (game < 0 || game >= k_num_games) return fail(AZG_E_INVALID_ARG, "unknown game id");
    if (count < 0) return fail(AZG_E_INVALID_ARG, "count < 0");
    if (!states) return fail(AZG_E_INVALID_ARG, "null states_dev");
    if ((pi != nullptr) != (sym_pi != nullptr)) return fail(AZG_E_INVALID_ARG, "pi_dev and sym_pi_dev go together: both or neither");
    if (count == 0) return AZG_OK;
    RULES_SWITCH(game,
        hipLaunchKernelGGL((k_game_symmetries<G>), dim3(count, G::NSYM), dim3(64), 0, (hipStream_t)stream, count, states, pi, sym_states,
                           sym_obs, sym_pi));
    HIPCHK(hipGetLastError());
    return AZG_OK;
}

#ifdef AZG_TREE_TIMING
// measurement builds only (not part of include/azg.h): the s_memtime stamps [B][16] of every slot's last simulation
extern "C" int azg_debug_tree_timing(azg_engine *e, unsigned long long *host) {
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(host, e->v.dbg, sizeof(unsigned long long) * 16 * (size_t)e->v.B, hipMemcpyDeviceToHost));
    return AZG_OK;
}
#endif

extern "C" int azg_profile_enable(azg_engine *e, int on) {
    if (!e) return fail(AZG_E_INVALID_ARG, "null engine");
    e->prof.enable(on != 0);
    return AZG_OK;
}
extern "C" int azg_profile_read(azg_engine *e, double *ms3, int64_t *launches3) {
    if (!e || !ms3 || !launches3) return fail(AZG_E_INVALID_ARG, "null argument");
    e->prof.read(ms3, launches3);
    return AZG_OK;
}
