// azg_tiles.h -- host code only (it needs the device headers for TowerGeom / tower_pixmap, but defines no kernel and runs without a
// device): THE declaration of every k_tower2 tile the library instantiates, one row per instantiation, and what follows from the rows
// alone: which launches a (game, tower width) has, the largest persistent tile, the layout query.  azg_engine.hip expands the same rows
// into its launches, so adding a tile -- or a game's tiles -- is adding rows here.
#pragma once
#include "azg_kernels.h"
#include "azg_conv.h"

namespace azg {

// ---- stand-alone tower tiles (azg_resnet_tower*_f16, azg_resnet_policy_value*_f16): X(game, channels, boards per tile, PSPLIT, KSPLIT).
// Which row a launch takes is dispatch_tower's tile policy (azg_engine.hip): a NEW (game, channels) pair needs a branch there as well
// as its rows here -- without one no row is ever chosen and the launch returns AZG_E_UNSUPPORTED although azg_launch_support has the
// tower bit (tests/test_gpu_launch_support.py launches every pair).  The three connect4 x 128 rows without a split are also the tiles
// of the fused search launches (azg_search_f16, azg_search_arena_f16).
#ifdef AZG_TUNING
#define AZG_TOWER_TILES_TUNING(X) \
    X(C4, 128, 2, 2, 1)   /* (sweep only: profiles/r03_arena_tile_sweep.txt) */
#else
#define AZG_TOWER_TILES_TUNING(X)
#endif
#define AZG_TOWER_TILES(X) \
    X(C4, 128, 1, 1, 1) \
    X(C4, 128, 1, 2, 1)   /* 8 waves, 2 + 1 pixel subtiles: measured slower (101 vs 69 us) */ \
    X(C4, 128, 2, 1, 1) \
    X(C4, 128, 4, 1, 1) \
    X(C4,  64, 4, 1, 1) \
    X(C4,  32, 2, 2, 1)   /* the default net of Coach.py:108-116 (BASELINE config 1): one cout group, */ \
    X(C4,  32, 4, 2, 1)   /* the tile's pixel subtiles dealt to two waves */ \
    X(BR,  64, 1, 1, 2)   /* k-split: 4 waves = (cout group, k group) */ \
    X(BR,  64, 1, 2, 1)   /* two cout groups: split the pixels too at small batches */ \
    X(BR,  64, 1, 1, 1) \
    X(BR,  64, 2, 2, 1) \
    X(BR,  64, 2, 1, 1) \
    X(BR, 128, 2, 1, 1) \
    X(TM,  32, 2, 4, 1)   /* one cout group */ \
    X(TM,  32, 2, 2, 1)   /* (256 boards: 26 us unsplit, 23 us split in two) */ \
    X(TM,  32, 2, 1, 1) \
    X(TM,  32, 5, 1, 1) \
    /* othello: an 8x8 board is exactly four pixel subtiles, so no tile carries pad rows; the tiles of the widths it shares with */ \
    /* connect4's default net (32) and brandubh's (64) */ \
    X(OT,  32, 2, 2, 1)   /* one cout group, the tile's pixel subtiles dealt to two waves */ \
    X(OT,  32, 4, 2, 1) \
    X(OT,  64, 1, 1, 2)   /* two cout groups: the k-split 1-board tile at small batches, as brandubh */ \
    X(OT,  64, 2, 2, 1) \
    X(OT,  64, 2, 1, 1) \
    /* gobang: a 15x15 board is 225 pixels, 15 pixel subtiles (15 spare lanes, five border classes) -- an odd count, so no k-split; */ \
    /* one board per tile, its subtiles dealt to three pixel groups of five (every width: 3, 6 or 12 waves) */ \
    X(GB,  32, 1, 3, 1) \
    X(GB,  64, 1, 3, 1) \
    X(GB, 128, 1, 3, 1) \
    /* tic-tac-toe: a 3x3 board is 9 pixels, less than one pixel subtile.  One wavefront per workgroup in every shape: one board (one */ \
    /* subtile, 7 spare lanes), five boards (45 pixels: three subtiles, one per border class of the three-class form), sixteen boards */ \
    /* (144 pixels: exactly nine subtiles and no spare lane; the five-class form, 1 interior + 3 + 3 row + 1 + 1 column subtiles) */ \
    X(TT,  32, 1, 1, 1) \
    X(TT,  32, 5, 1, 1) \
    X(TT,  32, 16, 1, 1) \
    AZG_TOWER_TILES_TUNING(X)

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

// sparse heads (head features -> logits of the leaf's children only) are not built for gobang, where nearly every cell is a legal
// move: a sparse row saves little and the 3616-wide feature dot products would spill
// nor for tic-tac-toe: A = 9 is one output subtile, which the exact heads compute whole at the same cost
template <class G> constexpr bool has_sparse_heads = G::ID != AZG_GAME_GOBANG && G::ID != AZG_GAME_TICTACTOE && G::ID != AZG_GAME_HNEFATAFL;

// azg_launch_support: the AZG_SUPPORT_* mask of (game, tower width); 0 for a game id the lists do not know
inline int tile_support(int game, int channels) {
    int m = 0;
#define AZG_ROW(G, C, BT, PS, KS) if (game == G::ID && channels == C) m |= AZG_SUPPORT_TOWER;
    AZG_TOWER_TILES(AZG_ROW)
#undef AZG_ROW
#define AZG_ROW(G, C, BT, PS, MINB, KS) \
    if (game == G::ID && channels == C) m |= AZG_SUPPORT_SEARCH_WIDE | (has_sparse_heads<G> ? AZG_SUPPORT_SEARCH_SPARSE : 0);
    AZG_WIDE_TILES(AZG_ROW)
#undef AZG_ROW
    if (game == AZG_GAME_CONNECT4 && channels == 128) m |= AZG_SUPPORT_SEARCH_FUSED;   // azg_search_f16 / azg_search_arena_f16: one special case
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
#define AZG_ROW(G, C, BT, PS, KS) AZG_LAYOUT(G, C, BT)
    AZG_TOWER_TILES(AZG_ROW)
#undef AZG_ROW
#define AZG_ROW(G, C, BT, PS, MINB, KS) AZG_LAYOUT(G, C, BT)
    AZG_WIDE_TILES(AZG_ROW)
#undef AZG_ROW
#undef AZG_LAYOUT
    return AZG_E_UNSUPPORTED;
}

}  // namespace azg
