// azg_tiles.h -- host code only (it needs the device headers for TowerGeom / tower_pixmap, but defines no kernel and runs without a
// device): THE declaration of every k_tower2 tile the library instantiates, one row per instantiation, and what follows from the rows
// alone: which launches a (game, tower width) has, which stand-alone tile a batch size takes, the largest persistent tile, the layout
// query.  azg_engine.hip expands the same rows into its launches, so adding a tile -- or a whole (game, width) pair -- is adding rows
// here and nothing else: a pair whose rows leave some batch size without a tile does not compile (tower_tiles_ok).
#pragma once
#include "azg_kernels.h"
#include "azg_conv.h"

namespace azg {

// ---- stand-alone tower tiles (azg_resnet_tower*_f16, azg_resnet_policy_value*_f16): X(game, channels, boards per tile, PSPLIT, KSPLIT,
// LIMIT).  LIMIT is the tile policy: a launch of n boards on a device of c CUs takes the first row of its pair, in the order written
// here, with 2 n <= LIMIT c -- LIMIT is TWICE the boards per CU up to which the row is the pair's tile (5: 2.5 boards per CU), in boards
// per CU of the device because that is what was measured (256 CUs: 640 / 1280 boards = 2.5 / 5 per CU).  The big tile has the least
// MFMA padding, small ones fill the chip at small batches (the arena, the single-tree API, brandubh's 512 games per GPU).  TILE_REST
// marks the pair's last default row (every larger batch); TILE_NEVER a row no batch size takes by default -- a measured alternative
// that an override of a tuning build reaches.  The rows is_fused_search_tile names are also the tiles of the fused search launches
// (azg_search_f16 at the same limits; azg_search_arena_f16: the one-board row).
constexpr int TILE_NEVER = 0, TILE_REST = 1 << 30;
template <class G, int C, int PS, int KS> constexpr bool is_fused_search_tile = G::ID == C4::ID && C == 128 && PS == 1 && KS == 1;   // connect4 x 128 without a split
#ifdef AZG_TUNING
#define AZG_TOWER_TILES_TUNING(X) \
    X(C4, 128, 2, 2, 1, TILE_NEVER)   /* (sweep only: profiles/r03_arena_tile_sweep.txt) */
#else
#define AZG_TOWER_TILES_TUNING(X)
#endif
#define AZG_TOWER_TILES(X) \
    X(C4, 128, 1, 1, 1, 5) \
    X(C4, 128, 1, 2, 1, TILE_NEVER)   /* 8 waves, 2 + 1 pixel subtiles: measured slower (101 vs 69 us) */ \
    X(C4, 128, 2, 1, 1, 2 * 5) \
    X(C4, 128, 4, 1, 1, TILE_REST) \
    X(C4,  64, 4, 1, 1, TILE_REST) \
    X(C4,  32, 2, 2, 1, 2 * 4)        /* the default net of Coach.py:108-116 (BASELINE config 1): one cout group, */ \
    X(C4,  32, 4, 2, 1, TILE_REST)    /* the tile's pixel subtiles dealt to two waves */ \
    /* brandubh x 64, measured (us per evaluation incl. heads, 256 / 512 / 1024 / 2048 boards on 256 CUs): 1 board, no split 39 / 47 / */ \
    /* 66 / 107; 1 board, pixels split 35 / 46 / 80 / 113; 2 boards, pixels split 39 / 43 / 63 / 113; round 3, the k-split 1-board tile */ \
    /* 28 / 36 / 64 / 114 -- the shape up to 512 boards */ \
    X(BR,  64, 1, 1, 2, 2 * 2)        /* k-split: 4 waves = (cout group, k group) */ \
    X(BR,  64, 1, 2, 1, TILE_NEVER)   /* two cout groups: split the pixels too at small batches */ \
    X(BR,  64, 1, 1, 1, TILE_NEVER) \
    X(BR,  64, 2, 2, 1, 2 * 4) \
    X(BR,  64, 2, 1, 1, TILE_REST) \
    X(BR, 128, 2, 1, 1, TILE_REST) \
    X(TM,  32, 2, 4, 1, TILE_NEVER)   /* one cout group */ \
    X(TM,  32, 2, 2, 1, 2 * 8)        /* (256 boards: 26 us unsplit, 23 us split in two) */ \
    X(TM,  32, 2, 1, 1, TILE_NEVER) \
    X(TM,  32, 5, 1, 1, TILE_REST) \
    /* othello: an 8x8 board is exactly four pixel subtiles, so no tile carries pad rows; the tiles of the widths it shares with */ \
    /* connect4's default net (32) and brandubh's (64) */ \
    X(OT,  32, 2, 2, 1, 2 * 4)        /* one cout group, the tile's pixel subtiles dealt to two waves */ \
    X(OT,  32, 4, 2, 1, TILE_REST) \
    X(OT,  64, 1, 1, 2, 2 * 2)        /* two cout groups: the k-split 1-board tile at small batches, as brandubh */ \
    X(OT,  64, 2, 2, 1, 2 * 4) \
    X(OT,  64, 2, 1, 1, TILE_REST) \
    /* gobang: a 15x15 board is 225 pixels, 15 pixel subtiles (15 spare lanes, five border classes) -- an odd count, so no k-split; */ \
    /* one board per tile, its subtiles dealt to three pixel groups of five (every width: 3, 6 or 12 waves) */ \
    X(GB,  32, 1, 3, 1, TILE_REST) \
    X(GB,  64, 1, 3, 1, TILE_REST) \
    X(GB, 128, 1, 3, 1, TILE_REST) \
    /* tic-tac-toe: a 3x3 board is 9 pixels, less than one pixel subtile.  One wavefront per workgroup in every shape: one board (one */ \
    /* subtile, 7 spare lanes) while that fills no more than 8 wavefronts per CU, five boards (45 pixels: three subtiles, one per border */ \
    /* class of the three-class form) up to 16 workgroups per CU, then sixteen (144 pixels: exactly nine subtiles and no spare lane; the */ \
    /* five-class form, 1 interior + 3 + 3 row + 1 + 1 column subtiles: 57 of 81 subtile-taps).  The limits are the occupancy argument */ \
    /* alone: nothing for this game has been measured */ \
    X(TT,  32, 1, 1, 1, 2 * 8) \
    X(TT,  32, 5, 1, 1, 2 * 80) \
    X(TT,  32, 16, 1, 1, TILE_REST) \
    AZG_TOWER_TILES_TUNING(X)

struct TowerTile { int game, channels, bt, ps, ks, limit; };
#define AZG_ROW(G, C, BT, PS, KS, LIMIT) {G::ID, C, BT, PS, KS, LIMIT},
constexpr TowerTile k_tower_tiles[] = {AZG_TOWER_TILES(AZG_ROW)};
#undef AZG_ROW
constexpr int k_num_tower_tiles = sizeof(k_tower_tiles) / sizeof(k_tower_tiles[0]);

// every pair's default rows have strictly ascending limits that end in its one TILE_REST row: every batch size has exactly one tile
constexpr bool tower_tiles_ok() {
    for (int i = 0; i < k_num_tower_tiles; i++) {
        const TowerTile &p = k_tower_tiles[i];
        int last = 0;
        for (int j = 0; j < k_num_tower_tiles; j++) {
            const TowerTile &t = k_tower_tiles[j];
            if (t.game != p.game || t.channels != p.channels || t.limit == TILE_NEVER) continue;
            if (t.limit <= last || t.limit > TILE_REST) return false;
            last = t.limit;
        }
        if (last != TILE_REST) return false;
    }
    return true;
}
static_assert(tower_tiles_ok(), "AZG_TOWER_TILES: the default rows of a (game, channels) pair need strictly ascending limits, the last of them TILE_REST");

// The tile policy, from the rows alone (no device call, no environment): the tile of `boards` boards on a device of `cus` CUs;
// bt == 0 for a pair without rows.  forced_bt / forced_ps (0: none) are the overrides of tuning builds: they select, among the pair's
// rows, the first with that many boards and / or that split -- PSPLIT 3 names a k-split row, as it always has for brandubh -- keeping
// the default pick's value for whichever of the two was not given where such a row exists; an override that names no row changes nothing.
struct TilePick { int bt, ps, ks; };
constexpr TilePick tower_tile_pick(int game, int channels, int boards, int cus, int forced_bt = 0, int forced_ps = 0) {
    TilePick d{0, 1, 1};
    for (const TowerTile &t : k_tower_tiles)
        if (t.game == game && t.channels == channels && t.limit != TILE_NEVER && (t.limit == TILE_REST || 2LL * boards <= (long long)t.limit * cus)) {
            d = TilePick{t.bt, t.ps, t.ks};
            break;
        }
    if (!forced_bt && !forced_ps) return d;
    const int d_split = d.ks == 2 ? 3 : d.ps;
    for (int keep = 1; keep >= 0; keep--)
        for (const TowerTile &t : k_tower_tiles) {
            const int split = t.ks == 2 ? 3 : t.ps;
            if (t.game != game || t.channels != channels || (forced_bt && t.bt != forced_bt) || (forced_ps && split != forced_ps)) continue;
            if (keep && ((!forced_bt && t.bt != d.bt) || (!forced_ps && split != d_split))) continue;
            return TilePick{t.bt, t.ps, t.ks};
        }
    return d;
}
#ifdef AZG_TUNING
// the shapes tools/sweep_arena.py forces (connect4 x 128, 256 rows) and the measured brandubh / trimok shapes quoted in the rows
constexpr bool tile_is(TilePick t, int bt, int ps, int ks) { return t.bt == bt && t.ps == ps && t.ks == ks; }
static_assert(tile_is(tower_tile_pick(C4::ID, 128, 256, 256, 1, 1), 1, 1, 1) && tile_is(tower_tile_pick(C4::ID, 128, 256, 256, 1, 2), 1, 2, 1) &&
              tile_is(tower_tile_pick(C4::ID, 128, 256, 256, 2, 1), 2, 1, 1) && tile_is(tower_tile_pick(C4::ID, 128, 256, 256, 2, 2), 2, 2, 1));
static_assert(tile_is(tower_tile_pick(BR::ID, 64, 2048, 256, 1, 1), 1, 1, 1) && tile_is(tower_tile_pick(BR::ID, 64, 2048, 256, 1, 2), 1, 2, 1) &&
              tile_is(tower_tile_pick(BR::ID, 64, 256, 256, 2, 2), 2, 2, 1) && tile_is(tower_tile_pick(BR::ID, 64, 2048, 256, 1, 3), 1, 1, 2) &&
              tile_is(tower_tile_pick(TM::ID, 32, 256, 256, 2, 1), 2, 1, 1) && tile_is(tower_tile_pick(TM::ID, 32, 256, 256, 0, 4), 2, 4, 1));
#endif

// ---- persistent wide-search tiles (azg_search_wide_f16, azg_search_wide_exact_f16): X(game, channels, games per workgroup, PSPLIT, MINB,
// KSPLIT); MINB = workgroups per CU the kernel is compiled for.  A pair's one-game row is also the tile of its arena launch
// (azg_search_arena_wide_exact_f16).  The extra tiles of tuning builds (AZG_WIDE_BOARDS codes) are hand-written in wide_tile_launch.
#define AZG_WIDE_TILES(X) \
    /* brandubh x 64: two workgroups of four wavefronts per CU in every shape */ \
    X(BR,  64, 1, 1, 2, 2)   /* four wavefronts per game (walk, priors, masks, rules), k-split tower */ \
    X(BR,  64, 2, 2, 2, 1)   /* walker + helper per game */ \
    X(BR,  64, 3, 2, 2, 1)   /* solo tree phase: one wavefront per game */ \
    X(BR,  64, 4, 2, 2, 1)   /* (two 4-game workgroups fill a CU's LDS with a 4-block tower's parameters beside them: a deeper */ \
                             /*  tower does not fit -> AZG_E_INVALID_ARG) */ \
    X(TM,  32, 1, 2, 1, 1) \
    X(TM,  32, 2, 4, 2, 1)   /* walker + helper per game */ \
    /* connect4 x 32: the reference's DEFAULT net (Coach.py:108-116: 32 channels x 4 blocks, 16 + 16 head channels -- BASELINE config 1's */ \
    /* network and what an unconfigured Coach trains): factorised heads, so the wide search mode; tiles like the 3-player env's */ \
    X(C4,  32, 1, 2, 1, 1) \
    X(C4,  32, 2, 4, 2, 1)   /* walker + helper per game */ \
    X(C4,  64, 1, 2, 2, 1)   /* four wavefronts per game */ \
    X(C4,  64, 2, 2, 2, 1)   /* walker + helper per game */ \
    /* othello x 32: the default net of an unconfigured Coach (32 x 4): connect4-32's shapes */ \
    X(OT,  32, 1, 2, 1, 1) \
    X(OT,  32, 2, 4, 2, 1)   /* walker + helper per game */ \
    /* othello x 64: envs/othello/train.py's net (64 x 4, 16 + 16 head channels): brandubh-64's shapes */ \
    X(OT,  64, 1, 1, 2, 2)   /* k-split tower */ \
    X(OT,  64, 2, 2, 2, 1) \
    X(OT,  64, 3, 2, 2, 1) \
    X(OT,  64, 4, 2, 2, 1) \
    /* gobang: the one-game tile of the stand-alone 15x15 towers (three pixel groups of five subtiles; walker, helper, mask wave and, */ \
    /* from 64 channels, the rules wave); exact heads only (has_sparse_heads).  128 channels (envs/gobang/train.py's 128 x 8 net): */ \
    /* twelve wavefronts, one workgroup per CU, the streamed heads loop (heads_full_stream) */ \
    X(GB,  32, 1, 3, 1, 1) \
    X(GB,  64, 1, 3, 1, 1) \
    X(GB, 128, 1, 3, 1, 1) \
    /* tic-tac-toe x 32 (envs/tictactoe/train.py's 32 x 4 net and the default net): connect4-32's shapes.  The board is ONE pixel subtile, */ \
    /* so the second pixel group of the one-game tile (the helper's wavefront) and groups 2, 3 of the two-game tile own no subtile: they */ \
    /* run the layers on the zero pad row and store nothing (k_tower2: gs < NSUBT); exact heads only (has_sparse_heads) */ \
    X(TT,  32, 1, 2, 1, 1) \
    X(TT,  32, 2, 4, 2, 1)   /* walker + helper per game */

// sparse heads (head features -> logits of the leaf's children only) are built for the games whose rules say so (azg_games.h)
template <class G> constexpr bool has_sparse_heads = G::SPARSE_HEADS;

// azg_launch_support: the AZG_SUPPORT_* mask of (game, tower width); 0 for a game id the lists do not know
inline int tile_support(int game, int channels) {
    int m = 0;
#define AZG_ROW(G, C, BT, PS, KS, LIMIT) \
    if (game == G::ID && channels == C) m |= AZG_SUPPORT_TOWER | (is_fused_search_tile<G, C, PS, KS> ? AZG_SUPPORT_SEARCH_FUSED : 0);
    AZG_TOWER_TILES(AZG_ROW)
#undef AZG_ROW
#define AZG_ROW(G, C, BT, PS, MINB, KS) \
    if (game == G::ID && channels == C) m |= AZG_SUPPORT_SEARCH_WIDE | (has_sparse_heads<G> ? AZG_SUPPORT_SEARCH_SPARSE : 0);
    AZG_WIDE_TILES(AZG_ROW)
#undef AZG_ROW
    return m;
}

// the most games per workgroup a pair's persistent launch has a tile for (0: no persistent launch)
inline int wide_max_tile(int game, int channels) {
    int m = 0;
#define AZG_ROW(G, C, BT, PS, MINB, KS) if (game == G::ID && channels == C && BT > m) m = BT;
    AZG_WIDE_TILES(AZG_ROW)
#undef AZG_ROW
    return m;
}

// host-side layout tables of the tower: the pixel -> (subtile, lane) map and the padded LDS row of every pixel
template <int H, int W, int BOARDS, int C>
inline int tower_layout_of(int16_t *map, int32_t *qrow, int32_t *info) {
    using GEO = TowerGeom<H, W, BOARDS, C>;
    if (map && !tower_pixmap<GEO>(map)) return AZG_E_INTERNAL;
    if (qrow) for (int p = 0; p < GEO::ROWS; p++) qrow[p] = GEO::qrow(p);
    info[0] = GEO::NSUB; info[1] = GEO::ROWS; info[2] = GEO::RSTRIDE; info[3] = GEO::TROWS; info[4] = GEO::TILE; info[5] = GEO::PW;
    info[6] = GEO::LEAD; info[7] = GEO::BSTRIDE;
    return AZG_OK;
}

// azg_tower_layout: every (game, boards, channels) of both lists; AZG_E_UNSUPPORTED for a shape no row instantiates
inline int tower_layout(int game, int boards_per_tile, int channels, int16_t *pixmap, int32_t *qrow, int32_t *info8) {
#define AZG_LAYOUT(G, C, BT) if (game == G::ID && boards_per_tile == BT && channels == C) return tower_layout_of<G::H, G::W, BT, C>(pixmap, qrow, info8);
#define AZG_ROW(G, C, BT, PS, KS, LIMIT) AZG_LAYOUT(G, C, BT)
    AZG_TOWER_TILES(AZG_ROW)
#undef AZG_ROW
#define AZG_ROW(G, C, BT, PS, MINB, KS) AZG_LAYOUT(G, C, BT)
    AZG_WIDE_TILES(AZG_ROW)
#undef AZG_ROW
#undef AZG_LAYOUT
    return AZG_E_UNSUPPORTED;
}

}  // namespace azg
