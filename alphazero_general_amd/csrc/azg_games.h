// azg_games.h -- device-side game rules ("rule kernels" registered per game; Game plugin API alphazero/Game.py:7-113).
//
// A game policy G provides, for one wavefront working on one game:
//   G::S                      wave-uniform register state
//   load(azg_state*, lane)    HBM -> registers         store(S, azg_state*, lane)  registers -> HBM
//   play(S&, action)          GameState.play_action    win_bits(S)   GameState.win_state as bit flags
//   valid_list(S, lane, act_lds, k)   GameState.valid_moves: lane i < k holds the i-th valid action (ascending)
//   write_obs<OT>(S, out, lane)       GameState.observation
//   symmetry(S, k, lane) / sym_action(a, k)   GameState.symmetries
#pragma once
#include "azg_device.h"

namespace azg {

// ================================================================================================ connect4
// alphazero/envs/connect4/connect4.pyx + Connect4Logic.pyx.  The reference scans an int board cell by cell;
// here the board is two 48-bit bitboards (bit r*8+c, column 7 = padding so shifts never wrap) held in SGPRs,
// built from the ABI's int8 cells with two wave ballots.
struct C4 {
    static constexpr int ID = AZG_GAME_CONNECT4;
    static constexpr const char *NAME = "connect4";
    static constexpr bool SPARSE_HEADS = true;                           // head features -> logits of the leaf's children only
    static constexpr int A = 7, H = 6, W = 7, CELLS = 42, P = 2, HAS_DRAW = 1, MAX_TURNS = 42, NSYM = 2;
    static constexpr int OBS_C = 4, OBS = OBS_C * CELLS, MAXK = 7;
    static constexpr int SYM_RAW = 0;                                    // symmetries()[SYM_RAW] is the position itself
    // The reference's scripted baseline player of this game (k_game_choose_scripted, azg_rules.h), or nullptr.  Such a game gives
    // scripted_key(parent, child), the sort key of one move; the player takes the smallest key, and of the moves that share it the lowest
    // action, or, with SCRIPTED_DRAWS, one drawn uniformly.
    static constexpr const char *SCRIPTED = "OneStepLookaheadConnect4Player";
    static constexpr bool SCRIPTED_DRAWS = true;
    struct S { uint64_t b0, b1; int player, turns; };

    static AZG_DEV S load(const azg_state *st, int lane) {
        int r = lane >> 3, c = lane & 7;
        int8_t v = (lane < 48 && c < 7) ? st->cells[r * 7 + c] : (int8_t)0;
        S s;
        s.b0 = __ballot(v == 1);                    // stone of player 0 = 1   (connect4.pyx:65)
        s.b1 = __ballot(v == -1);
        s.player = __builtin_amdgcn_readfirstlane(st->player);
        s.turns = __builtin_amdgcn_readfirstlane(st->turns);
        return s;
    }
    static AZG_DEV void init(S &s) { s.b0 = s.b1 = 0; s.player = 0; s.turns = 0; }
    static AZG_DEV int cell(const S &s, int i) {    // i = r*7+c
        int r = i / 7, c = i - r * 7; int b = r * 8 + c;
        return (int)((s.b0 >> b) & 1) - (int)((s.b1 >> b) & 1);
    }
    static AZG_DEV void store(const S &s, azg_state *st, int lane) {
        st->cells[lane] = lane < CELLS ? (int8_t)cell(s, lane) : (int8_t)0;
        if (lane == 0) { st->player = s.player; st->turns = s.turns; st->aux[0] = 0; st->aux[1] = 0; }
    }
    // Connect4Logic.pyx:40-47 add_stone (lowest empty row of the column) + Game.py:76-79 _update_turn
    static AZG_DEV void play(S &s, int a) {
        uint64_t occ = s.b0 | s.b1;
        int cnt = __popcll((occ >> a) & 0x0101010101010101ULL);
        uint64_t bit = 1ULL << ((5 - cnt) * 8 + a);
        if (s.player == 0) s.b0 |= bit; else s.b1 |= bit;
        s.player ^= 1; s.turns += 1;
    }
    static AZG_DEV uint64_t valid_mask(const S &s) { return ~(s.b0 | s.b1) & 0x7FULL; }   // :49-57 top row empty
    static AZG_DEV bool has4(uint64_t b) {
        uint64_t m;
        m = b & (b >> 1); if (m & (m >> 2)) return true;      // rows        :64-72
        m = b & (b >> 8); if (m & (m >> 16)) return true;     // columns     :74-82
        m = b & (b >> 9); if (m & (m >> 18)) return true;     // diagonal    :86-92
        m = b & (b >> 7); if (m & (m >> 14)) return true;     // anti-diag   :93-99
        return false;
    }
    // Connect4Logic.pyx:59-110 + connect4.pyx:68-81: bit0 = player 0 won, bit1 = player 1 won, bit2 = draw
    static AZG_DEV int win_bits(const S &s) {
        if (has4(s.b0)) return 1;
        if (has4(s.b1)) return 2;
        if (valid_mask(s) == 0) return 4;
        return 0;
    }
    // OneStepLookaheadConnect4Player.play (connect4/players.py:43-49): ws = win_state() of the child; ws[parent's mover]: the win set
    // (0), else ws[child's mover]: the stop-loss set (1), else the fallback set (2)
    static AZG_DEV int scripted_key(const S &parent, const S &child) {
        const int ws = win_bits(child);
        return (ws >> parent.player) & 1 ? 0 : (ws >> child.player) & 1 ? 1 : 2;
    }
    // lane i < k receives the i-th valid action in ascending order
    static AZG_DEV int valid_list(const S &s, int lane, int *act_lds, int (&my_a)[1]) {
        uint64_t vm = valid_mask(s);
        int k = __popcll(vm);
        // i-th set bit of vm: A <= 7, unrolled select
        int a = -1, cnt = 0;
#pragma unroll
        for (int c = 0; c < A; c++) { if ((vm >> c) & 1) { if (cnt == lane) a = c; cnt++; } }
        my_a[0] = a; (void)act_lds;
        return k;
    }
    // connect4.pyx:83-91: planes [pieces==1, pieces==-1, player, turns/42]
    template <typename OT> static AZG_DEV void write_obs(const S &s, OT *out, int lane) {
        float turn = (float)((double)s.turns / 42.0);
#pragma unroll
        for (int e0 = 0; e0 < OBS; e0 += 64) {
            int e = e0 + lane;
            if (e < OBS) {
                int plane = e / CELLS, i = e - plane * CELLS;
                int c = cell(s, i);
                float v = plane == 0 ? (c == 1 ? 1.f : 0.f) : plane == 1 ? (c == -1 ? 1.f : 0.f) : plane == 2 ? (float)s.player : turn;
                out[e] = (OT)v;
            }
        }
    }
    // the same four planes as NHWC fp16 rows with the channel dim padded to 8 (input format of the MFMA stem conv)
    typedef _Float16 h8 __attribute__((ext_vector_type(8)));
    static AZG_DEV h8 obs8(const S &s, int lane) {               // the four planes of cell `lane` (< CELLS), channels 4..7 zero
        const int c = cell(s, lane);
        return (h8){(_Float16)(c == 1 ? 1.f : 0.f), (_Float16)(c == -1 ? 1.f : 0.f), (_Float16)(float)s.player,
                    (_Float16)(float)((double)s.turns / 42.0), (_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f};
    }
    static AZG_DEV void write_obs_nhwc8(const S &s, _Float16 *out, int lane) {
        if (lane < CELLS) *reinterpret_cast<h8 *>(out + lane * 8) = obs8(s, lane);
    }
    // connect4.pyx:96-99: k = 1 mirrors the columns, pi -> pi[::-1]
    static AZG_DEV S symmetry(const S &s, int k) {
        if (k == 0) return s;
        S t = s; t.b0 = t.b1 = 0;
#pragma unroll
        for (int c = 0; c < 7; c++) {
            uint64_t col0 = (s.b0 >> c) & 0x0101010101010101ULL, col1 = (s.b1 >> c) & 0x0101010101010101ULL;
            t.b0 |= col0 << (6 - c); t.b1 |= col1 << (6 - c);
        }
        return t;
    }
    static AZG_DEV int sym_action(int a, int k) { return k == 0 ? a : 6 - a; }
};


// ================================================================================================ brandubh
// 7x7 tafl: alphazero/envs/brandubh/fastafl.pyx (Game) + fastafl/cengine.pyx (Board) + boardgame/board.pyx, board
// options of variants.brandubh_args (king_two_sided_capture, move_over_throne, king cannot re-enter the throne).
// The reference walks Python lists of Square objects; here lane i < 49 owns cell i = y*7+x (the Board._state value,
// cengine.pyx:24-32) and everything is expressed on 49-bit wave ballots: sliding moves by per-lane ray walks over
// the passable mask, custodian captures by uniform readlanes around the moved piece, the recursive group-surround
// check (cengine.pyx:204-247) as a bitboard flood fill ("no member of the connected enemy group touches an empty
// square"), win tests by neighbour masks.
struct BR {
    static constexpr int ID = AZG_GAME_BRANDUBH;
    static constexpr const char *NAME = "brandubh";
    static constexpr bool SPARSE_HEADS = true;
    static constexpr const char *SCRIPTED = nullptr;                     // no scripted baseline player (k_game_choose_scripted refuses the game)
    static constexpr int A = 588, H = 7, W = 7, CELLS = 49, P = 2, HAS_DRAW = 1, MAX_TURNS = 100, NSYM = 8;
    static constexpr int OBS_C = 5, OBS = OBS_C * CELLS, MAXK = 96;      // 8 attackers x 12 destinations bounds the move list
    static constexpr int SYM_RAW = 6;                                    // the identity: rot90^4 without flip (fastafl.pyx:213-256, k = 2*(4-1) + 0)
    static constexpr uint64_t ALL = (1ULL << 49) - 1;
    static constexpr uint64_t COL0 = 0x0040810204081ULL, COL6 = COL0 << 6;
    struct S { int cell; int player, turns, kc; };

    static AZG_DEV uint64_t nbr(uint64_t m) {       // squares orthogonally adjacent to the set m (board edges: nothing)
        return ((m << 7) | (m >> 7) | ((m & ~COL6) << 1) | ((m & ~COL0) >> 1)) & ALL;
    }
    static AZG_DEV uint64_t mask_eq(const S &s, int lane, int v) { return __ballot(lane < CELLS && s.cell == v); }
    static AZG_DEV bool is_king(int v) { return v == 3 || v == 7 || v == 8; }
    static AZG_DEV bool is_att(int v) { return v == 1 || is_king(v); }                       // ATTACKERS cengine.pyx:42
    static AZG_DEV int rd(const S &s, int idx) { return __builtin_amdgcn_readlane(s.cell, __builtin_amdgcn_readfirstlane(idx)); }

    static AZG_DEV S load(const azg_state *st, int lane) {
        S s;
        s.cell = lane < CELLS ? (int)st->cells[lane] : 0;
        s.player = __builtin_amdgcn_readfirstlane(st->player);
        s.turns = __builtin_amdgcn_readfirstlane(st->turns);
        s.kc = __builtin_amdgcn_readfirstlane(st->aux[0]);
        return s;
    }
    static AZG_DEV void init(S &s) {                // fastafl/variants.py:13-19
        const int lane = threadIdx.x & 63;
        const int y = lane / 7, x = lane - y * 7;
        int v = 0;
        if (lane < CELLS) {
            const bool corner = (x == 0 || x == 6) && (y == 0 || y == 6);
            if (corner) v = 5;
            else if (x == 3 && y == 3) v = 7;
            else if ((x == 3 && (y == 2 || y == 4)) || (y == 3 && (x == 2 || x == 4))) v = 1;
            else if ((x == 3 && (y <= 1 || y >= 5)) || (y == 3 && (x <= 1 || x >= 5))) v = 2;
        }
        s.cell = v; s.player = 0; s.turns = 0; s.kc = 0;
    }
    static AZG_DEV void store(const S &s, azg_state *st, int lane) {
        st->cells[lane] = lane < CELLS ? (int8_t)s.cell : (int8_t)0;
        if (lane == 0) { st->player = s.player; st->turns = s.turns; st->aux[0] = s.kc; st->aux[1] = 0; }
    }
    static AZG_DEV void decode(int a, int &src, int &dst) {          // fastafl.pyx:48-63 get_move
        const int mt = a % 12; src = a / 12;
        const int sx = src % 7, sy = src / 7;
        int nx, ny;
        if (mt < 6) { nx = sx; ny = mt + (mt >= sy ? 1 : 0); }
        else { nx = mt - 6; nx += (nx >= sx ? 1 : 0); ny = sy; }
        dst = ny * 7 + nx;
    }
    static AZG_DEV int encode(int x, int y, int nx, int ny) {        // fastafl.pyx:66-79 get_action
        const int mt = x == nx ? (ny < y ? ny : ny - 1) : (nx < x ? 6 + nx : 6 + nx - 1);
        return 12 * (x + y * 7) + mt;
    }
    // Board.move (cengine.pyx:249-272, no validity / win checks) + _check_capture (:172-197) + _check_surround (:228-247)
    static AZG_DEV void play(S &s, int a) {
        const int lane = threadIdx.x & 63;
        a = __builtin_amdgcn_readfirstlane(a);
        int src, dst; decode(a, src, dst);
        const int srcv = rd(s, src), dstv = rd(s, dst);
        const int piece = (srcv == 7 || srcv == 8) ? 3 : srcv;                               // remove_piece :311-326
        const int newsrc = srcv == 7 ? 4 : srcv == 8 ? 5 : 0;
        const int newdst = (dstv == 4 || dstv == 5) ? piece + dstv : piece;                  // add_piece :293-309
        if (lane == src) s.cell = newsrc;
        if (lane == dst) s.cell = newdst;
        // every capture below starts from a square next to the moved piece that holds an enemy or -- two-sided king capture fires
        // for any mover (Q20) -- the king: most moves have none, and are done here
        {
            const bool black = newdst == 2;                                                  // (the mover; a king on the throne / an escape counts as an attacker for black)
            const uint64_t relevant = __ballot(lane < CELLS && (black ? is_att(s.cell) : (s.cell == 2 || s.cell == 3)));
            if ((nbr(1ULL << dst) & relevant) == 0) { s.turns += 1; s.player ^= 1; return; }
        }
        const int dx4[4] = {0, 1, 0, -1}, dy4[4] = {1, 0, -1, 0};                            // DIRECTIONS :46
        const int mx = dst % 7, my = dst / 7;
        // ---- custodian capture around the moved piece ----
        const bool friendly_att = is_att(newdst);
        const int enemy = newdst != 3 ? 3 - newdst : 2;
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const int ex = mx + dx4[d], ey = my + dy4[d];
            if (ex < 0 || ex > 6 || ey < 0 || ey > 6) continue;
            const int ev = rd(s, ey * 7 + ex);
            const bool do_capture = ev == 3;                                                 // two-sided king capture (Q20)
            if (ev == enemy || do_capture) {
                const int fx = ex + dx4[d], fy = ey + dy4[d];
                if (fx < 0 || fx > 6 || fy < 0 || fy > 6) continue;
                const int fv = rd(s, fy * 7 + fx);
                const bool friendly = friendly_att ? is_att(fv) : fv == newdst;
                if (friendly || fv == 4 || fv == 5) {
                    if (do_capture) s.kc = 1;
                    else if (lane == ey * 7 + ex) s.cell = 0;
                }
            }
        }
        // ---- group surround: start squares in DIRECTIONS order, removals visible to the later ones ----
        const bool enemy_is_att = rd(s, dst) == 2;
        uint64_t checked = 0;
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const int ex = mx + dx4[d], ey = my + dy4[d];
            if (ex < 0 || ex > 6 || ey < 0 || ey > 6) continue;
            const int e = ey * 7 + ex;
            const uint64_t enemyM = enemy_is_att ? __ballot(lane < CELLS && is_att(s.cell)) : mask_eq(s, lane, 2);
            if (!((enemyM >> e) & 1) || ((checked >> e) & 1)) continue;
            uint64_t g = 1ULL << e;
            for (;;) { const uint64_t g2 = g | (nbr(g) & enemyM); if (g2 == g) break; g = g2; }
            checked |= g;
            const uint64_t empty = mask_eq(s, lane, 0);
            if ((nbr(g) & empty) == 0) {                                                     // every member fully blocked
                const uint64_t kings = __ballot(lane < CELLS && is_king(s.cell));
                if (g & kings) s.kc = 1;                                                     // a king is never lifted (:243-244)
                if (lane < CELLS && ((g >> lane) & 1) && !is_king(s.cell)) s.cell = 0;
            }
        }
        s.turns += 1; s.player ^= 1;
    }
    // Game.win_state (fastafl.pyx:186-199) + Board.get_winner (cengine.pyx:163-169) + _has_legals_check (:134-141)
    static AZG_DEV int win_bits(const S &s) {
        const int lane = threadIdx.x & 63;
        if (s.turns >= 100) return 4;
        const uint64_t esc = mask_eq(s, lane, 8);
        const uint64_t adjE = nbr(mask_eq(s, lane, 0)), adjX = nbr(mask_eq(s, lane, 5));
        const uint64_t kings = __ballot(lane < CELLS && is_king(s.cell));
        const bool def_has = (mask_eq(s, lane, 2) & adjE) != 0;
        const bool att_has = ((mask_eq(s, lane, 1) & adjE) | (kings & (adjE | adjX))) != 0;
        if (esc != 0 || !def_has) return 2;           // attackers (player 1) win: result[2 - 1]
        if (s.kc || !att_has) return 1;               // defenders (player 0) win: result[2 - 2]
        return 0;
    }
    // cells of a 7-cell line (bit p = the piece's own position) a sliding piece at p reaches: the runs of passable cells on
    // both sides of p (Board.legal_moves walks them square by square, cengine.pyx:109-132)
    static AZG_DEV unsigned reach7(unsigned line, int p) {
        const unsigned up = line >> (p + 1);                                  // cells above p, bit 0 = p + 1
        const unsigned run = (unsigned)__builtin_ctz(~up);                    // trailing ones (a 7-bit line: ~up is never 0)
        const unsigned reach_up = ((1u << run) - 1u) << (p + 1);
        const unsigned below = (1u << p) - 1u, blk = ~line & below;           // blockers below p
        const unsigned cut = blk ? (2u << (31 - __builtin_clz(blk))) : 1u;    // first bit above the highest blocker
        return reach_up | (line & below & ~(cut - 1u));
    }
    // Game.valid_moves (fastafl.pyx:171-178) + Board.legal_moves (cengine.pyx:109-132): ascending action list in LDS.
    // Branch-free per lane: the row of the passable mask and (through the transposed board) its column are 7-bit lines, the
    // reachable runs come from count-trailing-ones / count-leading-zeros, the move types from two shifts; the list offsets
    // from a DPP row scan of the per-lane move counts.
    static AZG_DEV int valid_list(const S &s, int lane, int *act_lds, int (&my_a)[2]) {
        const int team = 2 - (s.turns & 1);                                                  // Board.to_play :330-331
        const bool mine = lane < CELLS && (team == 1 ? is_att(s.cell) : s.cell == 2);
        const bool king = is_king(s.cell);
        const int x = lane % 7, y = lane / 7;
        const int cellT = __shfl(s.cell, lane < CELLS ? x * 7 + y : 0);                      // the transposed board
        const uint64_t E = mask_eq(s, lane, 0), T = mask_eq(s, lane, 4), X = mask_eq(s, lane, 5);
        const uint64_t Et = __ballot(lane < CELLS && cellT == 0), Tt = __ballot(lane < CELLS && cellT == 4), Xt = __ballot(lane < CELLS && cellT == 5);
        const uint64_t pass = E | T | (king ? X : 0ULL), passT = Et | Tt | (king ? Xt : 0ULL);     // the ray continues over these
        const unsigned row = (unsigned)(pass >> (7 * y)) & 0x7Fu, col = (unsigned)(passT >> (7 * x)) & 0x7Fu;
        const unsigned trow = (unsigned)(T >> (7 * y)) & 0x7Fu, tcol = (unsigned)(Tt >> (7 * x)) & 0x7Fu;
        const unsigned rx = reach7(row, x) & ~trow, ry = reach7(col, y) & ~tcol;             // nobody lands on the empty throne
        // move_type (fastafl.pyx:66-79): vertical ny -> ny or ny - 1, horizontal nx -> 6 + nx or 6 + nx - 1
        const unsigned mvy = (ry & ((1u << y) - 1u)) | ((ry >> (y + 1)) << y), mvx = (rx & ((1u << x) - 1u)) | ((rx >> (x + 1)) << x);
        const unsigned mv = mine ? (mvy | (mvx << 6)) : 0u;                                  // bit = move_type (0..11)
        // list offset of the lane = moves of the lanes below it: an inclusive scan of the per-lane counts inside each row of 16
        // (four DPP row shifts) + the totals of the rows below; then one predicated store per move type instead of a per-lane loop
        const int cnt = __popc(mv);
        int inc = cnt;
        inc += dpp_i<0x111>(inc); inc += dpp_i<0x112>(inc); inc += dpp_i<0x114>(inc); inc += dpp_i<0x118>(inc);   // row_shr:1, 2, 4, 8
        const int r0 = rl(inc, 15), r1 = rl(inc, 31), r2 = rl(inc, 47), r3 = rl(inc, 63);
        const int lrow = lane >> 4;
        const int off = inc - cnt + (lrow == 0 ? 0 : lrow == 1 ? r0 : lrow == 2 ? r0 + r1 : r0 + r1 + r2);
        const int k = r0 + r1 + r2 + r3;
#pragma unroll
        for (int b = 0; b < 12; b++) {
            const int pos = off + __popc(mv & ((1u << b) - 1u));
            if (((mv >> b) & 1u) && pos < MAXK) act_lds[pos] = 12 * lane + b;
        }
        wave_sync();
        my_a[0] = lane < k ? act_lds[lane] : -1;
        my_a[1] = 64 + lane < k ? act_lds[64 + lane] : -1;
        wave_sync();
        return k < MAXK ? k : MAXK;
    }
    // Game.observation (fastafl.pyx:84-121,205-211): planes [black(2), white(1), king, to-move colour, 0] (Q18)
    template <typename OT> static AZG_DEV void write_obs(const S &s, OT *out, int lane) {
        const float colour = (float)(s.turns & 1), turn_no = (float)(s.turns / 100);
        for (int e0 = 0; e0 < OBS; e0 += 64) {
            const int e = e0 + lane;
            const int plane = e / CELLS, i = e - plane * CELLS;
            const int c = __shfl(s.cell, i < CELLS ? i : 0);
            if (e < OBS) {
                const float v = plane == 0 ? (c == 2 ? 1.f : 0.f) : plane == 1 ? (c == 1 ? 1.f : 0.f)
                              : plane == 2 ? (is_king(c) ? 1.f : 0.f) : plane == 3 ? colour : turn_no;
                out[e] = (OT)v;
            }
        }
    }
    typedef _Float16 h8 __attribute__((ext_vector_type(8)));
    static AZG_DEV h8 obs8(const S &s, int lane) {               // the five planes of cell `lane` (< CELLS: the lane's own cell)
        const int c = s.cell; (void)lane;
        return (h8){(_Float16)(c == 2 ? 1.f : 0.f), (_Float16)(c == 1 ? 1.f : 0.f), (_Float16)(is_king(c) ? 1.f : 0.f),
                    (_Float16)(float)(s.turns & 1), (_Float16)(float)(s.turns / 100), (_Float16)0.f, (_Float16)0.f, (_Float16)0.f};
    }
    static AZG_DEV void write_obs_nhwc8(const S &s, _Float16 *out, int lane) {
        if (lane < CELLS) *reinterpret_cast<h8 *>(out + lane * 8) = obs8(s, lane);
    }
    // Game.symmetries (fastafl.pyx:213-256): k = (i-1)*2 + flip; state = fliplr^flip(rot90^i(state)); the policy index is
    // permuted by the reference's own coordinate loop (sym_action)
    static AZG_DEV S symmetry(const S &s, int k) {
        const int lane = threadIdx.x & 63;
        const int i = k / 2 + 1, flip = k & 1;
        int r = lane / 7, c = lane - (lane / 7) * 7;
        if (flip) c = 6 - c;                              // final[r][c] = rotated[r][6-c]
        for (int t = 0; t < i; t++) { const int nr = c, nc = 6 - r; r = nr; c = nc; }       // rot90: new[r][c] = old[c][6-r]
        S o = s;
        const int v = __shfl(s.cell, lane < CELLS ? r * 7 + c : 0);
        o.cell = lane < CELLS ? v : 0;
        return o;
    }
    static AZG_DEV int sym_action(int a, int k) {
        const int i = k / 2 + 1, flip = k & 1;
        int src, dst; decode(a, src, dst);
        int x = src % 7, y = src / 7, nx = dst % 7, ny = dst / 7;
        for (int t = 0; t < i; t++) { const int tx = x, tnx = nx; x = 6 - y; nx = 6 - ny; y = tx; ny = tnx; }   // :241-246
        if (flip) { x = 6 - x; nx = 6 - nx; }
        return encode(x, y, nx, ny);
    }
};


// ================================================================================================ trimok (3 players)
// Build-defined N-player env (BASELINE config 5; rules in alphazero_general_amd/envs/trimok.py): 5x5 board, three players
// place stones in turn, three in a row wins, full board draws.  One 25-bit bitboard per player in SGPRs.
struct TM {
    static constexpr int ID = AZG_GAME_TRIMOK;
    static constexpr const char *NAME = "trimok";
    static constexpr bool SPARSE_HEADS = true;
    static constexpr const char *SCRIPTED = nullptr;                     // no scripted baseline player (k_game_choose_scripted refuses the game)
    static constexpr int A = 25, H = 5, W = 5, CELLS = 25, P = 3, HAS_DRAW = 1, MAX_TURNS = 25, NSYM = 1;
    static constexpr int OBS_C = 5, OBS = OBS_C * CELLS, MAXK = 25;
    static constexpr int SYM_RAW = 0;
    struct S { uint32_t b[3]; int player, turns; };
    static AZG_DEV S load(const azg_state *st, int lane) {
        const int8_t v = lane < CELLS ? st->cells[lane] : (int8_t)0;
        S s;
        s.b[0] = (uint32_t)__ballot(v == 1); s.b[1] = (uint32_t)__ballot(v == 2); s.b[2] = (uint32_t)__ballot(v == 3);
        s.player = __builtin_amdgcn_readfirstlane(st->player);
        s.turns = __builtin_amdgcn_readfirstlane(st->turns);
        return s;
    }
    static AZG_DEV void init(S &s) { s.b[0] = s.b[1] = s.b[2] = 0; s.player = 0; s.turns = 0; }
    static AZG_DEV int cell(const S &s, int i) { return (int)((s.b[0] >> i) & 1) + 2 * (int)((s.b[1] >> i) & 1) + 3 * (int)((s.b[2] >> i) & 1); }
    static AZG_DEV void store(const S &s, azg_state *st, int lane) {
        st->cells[lane] = lane < CELLS ? (int8_t)cell(s, lane) : (int8_t)0;
        if (lane == 0) { st->player = s.player; st->turns = s.turns; st->aux[0] = 0; st->aux[1] = 0; }
    }
    static AZG_DEV void play(S &s, int a) {
        const uint32_t bit = 1u << a;
        if (s.player == 0) s.b[0] |= bit; else if (s.player == 1) s.b[1] |= bit; else s.b[2] |= bit;
        s.player = s.player == 2 ? 0 : s.player + 1; s.turns += 1;          // Game.py:73-79 (player + 1) % num_players
    }
    static AZG_DEV bool has3(uint32_t m) {
        constexpr uint32_t XLE2 = 0x00739CE7u;                               // cells with x <= 2 (line start, going right)
        constexpr uint32_t XGE2 = 0x01CE739Cu;                               // cells with x >= 2 (anti-diagonal start)
        if (m & (m >> 1) & (m >> 2) & XLE2) return true;                     // horizontal
        if (m & (m >> 5) & (m >> 10)) return true;                           // vertical
        if (m & (m >> 6) & (m >> 12) & XLE2) return true;                    // diagonal  (+1, +1)
        if (m & (m >> 4) & (m >> 8) & XGE2) return true;                     // diagonal  (-1, +1)
        return false;
    }
    static AZG_DEV int win_bits(const S &s) {
        if (has3(s.b[0])) return 1;
        if (has3(s.b[1])) return 2;
        if (has3(s.b[2])) return 4;
        if ((s.b[0] | s.b[1] | s.b[2]) == 0x1FFFFFFu) return 8;
        return 0;
    }
    static AZG_DEV int valid_list(const S &s, int lane, int *act_lds, int (&my_a)[1]) {
        const uint32_t vm = ~(s.b[0] | s.b[1] | s.b[2]) & 0x1FFFFFFu;
        const int k = __popc(vm);
        // lane i takes the i-th set bit: the lane of an empty cell pushes its index to the lane of its rank (one ds_permute; the
        // other lanes push to lane 63, which nobody reads: k <= 25)
        const bool empty = ((vm >> (lane & 31)) & 1u) != 0 && lane < CELLS;
        const int rank = __popc(vm & ((1u << (lane & 31)) - 1u));
        const int a = __builtin_amdgcn_ds_permute((empty ? rank : 63) << 2, lane);
        my_a[0] = lane < k ? a : -1; (void)act_lds;
        return k;
    }
    template <typename OT> static AZG_DEV void write_obs(const S &s, OT *out, int lane) {
        const float turn = (float)((double)s.turns / 25.0);
#pragma unroll
        for (int e0 = 0; e0 < OBS; e0 += 64) {
            const int e = e0 + lane;
            if (e < OBS) {
                const int plane = e / CELLS, i = e - plane * CELLS;
                const float v = plane < 3 ? (float)((s.b[plane == 0 ? 0 : plane == 1 ? 1 : 2] >> i) & 1) : plane == 3 ? (float)s.player : turn;
                out[e] = (OT)v;
            }
        }
    }
    typedef _Float16 h8 __attribute__((ext_vector_type(8)));
    static AZG_DEV h8 obs8(const S &s, int lane) {               // the five planes of cell `lane` (< CELLS)
        return (h8){(_Float16)(float)((s.b[0] >> lane) & 1), (_Float16)(float)((s.b[1] >> lane) & 1), (_Float16)(float)((s.b[2] >> lane) & 1),
                    (_Float16)(float)s.player, (_Float16)(float)((double)s.turns / 25.0), (_Float16)0.f, (_Float16)0.f, (_Float16)0.f};
    }
    static AZG_DEV void write_obs_nhwc8(const S &s, _Float16 *out, int lane) {
        if (lane < CELLS) *reinterpret_cast<h8 *>(out + lane * 8) = obs8(s, lane);
    }
    static AZG_DEV S symmetry(const S &s, int k) { (void)k; return s; }
    static AZG_DEV int sym_action(int a, int k) { (void)k; return a; }
};


// ================================================================================================ othello
// alphazero/envs/othello/othello.pyx + OthelloLogic.pyx.  Cell i = 8x + y of the reference's pieces[x][y] (action a = 8x + y places a
// stone on cell a), colour 1 for player 0 and -1 for player 1.  The board is two 64-bit bitboards in SGPRs: every bit is a cell, so
// there is no padding bit, and a shift that moves along y must clear the column it would wrap out of first.  No pass action: the game
// ends as soon as the player to move has no legal move (win_state, othello.pyx:83-96), scored by the disc difference from the mover.
struct OT {
    static constexpr int ID = AZG_GAME_OTHELLO;
    static constexpr const char *NAME = "othello";
    static constexpr bool SPARSE_HEADS = true;
    static constexpr int A = 64, H = 8, W = 8, CELLS = 64, P = 2, HAS_DRAW = 1, MAX_TURNS = 64, NSYM = 8;
    static constexpr int OBS_C = 1, OBS = OBS_C * CELLS, MAXK = 60;      // at most 60 empty squares: one wavefront holds the move list
    static constexpr int SYM_RAW = 7;                                    // the identity is the LAST entry of symmetries() (k = 2*(4-1) + 1)
    static constexpr uint64_t COL0 = 0x0101010101010101ULL, COL7 = 0x8080808080808080ULL;
    static constexpr const char *SCRIPTED = "GreedyOthelloPlayer";
    static constexpr bool SCRIPTED_DRAWS = false;
    struct S { uint64_t b0, b1; int player, turns; };                    // b0: colour 1 (player 0), b1: colour -1

    // one step of the 8 directions (OthelloLogic.pyx:24); d = 0..7, x = bit >> 3, y = bit & 7
    static AZG_DEV uint64_t step(uint64_t m, int d) {
        switch (d) {
        case 0: return (m & ~COL7) << 9;     // (+1, +1)
        case 1: return m << 8;               // (+1,  0)
        case 2: return (m & ~COL0) << 7;     // (+1, -1)
        case 3: return (m & ~COL0) >> 1;     // ( 0, -1)
        case 4: return (m & ~COL0) >> 9;     // (-1, -1)
        case 5: return m >> 8;               // (-1,  0)
        case 6: return (m & ~COL7) >> 7;     // (-1, +1)
        default: return (m & ~COL7) << 1;    // ( 0, +1)
        }
    }
    static AZG_DEV S load(const azg_state *st, int lane) {
        const int8_t v = st->cells[lane];
        S s;
        s.b0 = __ballot(v == 1);
        s.b1 = __ballot(v == -1);
        s.player = __builtin_amdgcn_readfirstlane(st->player);
        s.turns = __builtin_amdgcn_readfirstlane(st->turns);
        return s;
    }
    static AZG_DEV void init(S &s) {                                     // OthelloLogic.pyx Board.__init__: pieces[3][4] = pieces[4][3] = 1, [3][3] = [4][4] = -1
        s.b0 = (1ULL << 28) | (1ULL << 35); s.b1 = (1ULL << 27) | (1ULL << 36); s.player = 0; s.turns = 0;
    }
    static AZG_DEV int cell(const S &s, int i) { return (int)((s.b0 >> i) & 1) - (int)((s.b1 >> i) & 1); }
    static AZG_DEV void store(const S &s, azg_state *st, int lane) {
        st->cells[lane] = (int8_t)cell(s, lane);
        if (lane == 0) { st->player = s.player; st->turns = s.turns; st->aux[0] = 0; st->aux[1] = 0; }
    }
    // empty squares that close a run of the opponent's stones against one of `own` (get_legal_moves, OthelloLogic.pyx:67-78):
    // directional fills, a run is at most 6 stones long
    static AZG_DEV uint64_t moves(uint64_t own, uint64_t opp) {
        const uint64_t empty = ~(own | opp);
        uint64_t mv = 0;
#pragma unroll
        for (int d = 0; d < 8; d++) {
            uint64_t t = step(own, d) & opp;
#pragma unroll
            for (int i = 0; i < 5; i++) t |= step(t, d) & opp;
            mv |= step(t, d) & empty;
        }
        return mv;
    }
    static AZG_DEV uint64_t valid_mask(const S &s) { return s.player == 0 ? moves(s.b0, s.b1) : moves(s.b1, s.b0); }
    // execute_move (OthelloLogic.pyx:121-142, _get_flips :162-176): in each direction, the run of opponent stones the move closes
    static AZG_DEV void play(S &s, int a) {
        a = __builtin_amdgcn_readfirstlane(a) & 63;
        const uint64_t m = 1ULL << a;
        uint64_t own = s.player == 0 ? s.b0 : s.b1, opp = s.player == 0 ? s.b1 : s.b0;
        uint64_t flips = 0;
#pragma unroll
        for (int d = 0; d < 8; d++) {
            uint64_t run = 0, x = step(m, d);
            while (x & opp) { run |= x; x = step(x, d); }
            if (x & own) flips |= run;
        }
        own |= flips | m; opp &= ~flips;
        if (s.player == 0) { s.b0 = own; s.b1 = opp; } else { s.b0 = opp; s.b1 = own; }
        s.player ^= 1; s.turns += 1;
    }
    // win_state (othello.pyx:83-96): the player to move has no legal move -> count_diff from the mover's colour decides
    static AZG_DEV int win_bits(const S &s) {
        if (valid_mask(s) != 0) return 0;
        const int own = __popcll(s.player == 0 ? s.b0 : s.b1), opp = __popcll(s.player == 0 ? s.b1 : s.b0);
        return own > opp ? 1 << s.player : own < opp ? 1 << (s.player ^ 1) : 4;
    }
    // GreedyOthelloPlayer.play (OthelloPlayers.py:37): -child._board.count_diff(child.player).  count_diff(color) sums pieces * color
    // (OthelloLogic.pyx:59-69) and is handed the player INDEX, not the colour: 0 when the child's mover is player 0, the stones of
    // colour -1 minus those of colour 1 when it is player 1
    static AZG_DEV int scripted_key(const S &parent, const S &child) {
        (void)parent;
        return child.player == 0 ? 0 : __popcll(child.b1) - __popcll(child.b0);
    }
    // lane i < k receives the i-th legal move in ascending order: the lane of a legal square pushes its index to the lane of its rank
    // (the legal squares below it: mbcnt), one ds_permute; the others push to lane 63, which nobody reads (k <= 60)
    static AZG_DEV int valid_list(const S &s, int lane, int *act_lds, int (&my_a)[1]) {
        const uint64_t vm = valid_mask(s);
        const int k = __popcll(vm);
        const bool legal = ((vm >> lane) & 1) != 0;
        const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(vm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)vm, 0u));
        const int a = __builtin_amdgcn_ds_permute((legal ? rank : 63) << 2, lane);
        my_a[0] = lane < k ? a : -1; (void)act_lds;
        return k;
    }
    // observation (othello.pyx:98-99): one plane of the raw pieces, absolute colours
    template <typename OT_> static AZG_DEV void write_obs(const S &s, OT_ *out, int lane) { out[lane] = (OT_)(float)cell(s, lane); }
    typedef _Float16 h8 __attribute__((ext_vector_type(8)));
    static AZG_DEV h8 obs8(const S &s, int lane) {
        return (h8){(_Float16)(float)cell(s, lane), (_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f};
    }
    static AZG_DEV void write_obs_nhwc8(const S &s, _Float16 *out, int lane) { *reinterpret_cast<h8 *>(out + lane * 8) = obs8(s, lane); }
    // symmetries (othello.pyx:101-120): entry k = 2(i-1) + (0 if flipped else 1), i = 1..4: fliplr^flip(rot90^i(pieces)), so k = 7 is the
    // identity.  np.rot90: out[r][c] = in[c][7-r]; np.fliplr: out[r][c] = in[r][7-c]
    static AZG_DEV S symmetry(const S &s, int k) {
        const int lane = threadIdx.x & 63;
        const int i = k / 2 + 1;
        int r = lane >> 3, c = lane & 7;
        if ((k & 1) == 0) c = 7 - c;
        for (int t = 0; t < i; t++) { const int nr = c, nc = 7 - r; r = nr; c = nc; }
        const int src = r * 8 + c;
        S o = s;
        o.b0 = __ballot((s.b0 >> src) & 1);
        o.b1 = __ballot((s.b1 >> src) & 1);
        return o;
    }
    // where pi[a] lands under symmetry k (the forward maps: rot90 sends (r, c) to (7-c, r), fliplr (r, c) to (r, 7-c))
    static AZG_DEV int sym_action(int a, int k) {
        const int i = k / 2 + 1;
        int r = a >> 3, c = a & 7;
        for (int t = 0; t < i; t++) { const int nr = 7 - c, nc = r; r = nr; c = nc; }
        if ((k & 1) == 0) c = 7 - c;
        return r * 8 + c;
    }
};


// ================================================================================================ gobang
// alphazero/envs/gobang/gobang.pyx + GobangLogic.pyx: 15x15, five in a row.  Cell i = 15x + y of the reference's pieces[x][y] (action a
// places a stone on cell a, every empty cell is legal), colour 1 for player 0 and -1 for player 1.  The first board that one wavefront
// cannot hold a cell per lane: each colour is a 256-bit bitboard of four 64-bit words in SGPRs, 15 rows of 16 bits (bit 16x + y; bit 15
// of every row and the 16 bits behind row 14 stay zero), so a run shifted along any of the four directions never wraps onto the next
// row.  The observation, legal-move list and symmetries walk the cells in chunks of 64 (cell c = lane + 64 j).
struct GB {
    static constexpr int ID = AZG_GAME_GOBANG;
    static constexpr const char *NAME = "gobang";
    static constexpr bool SPARSE_HEADS = false;   // nearly every cell is a legal move: a sparse row saves little and the 3616-wide feature dot products would spill
    static constexpr int A = 225, H = 15, W = 15, CELLS = 225, P = 2, HAS_DRAW = 1, MAX_TURNS = 225, NSYM = 8;
    static constexpr int OBS_C = 4, OBS = OBS_C * CELLS, MAXK = 225;     // every empty cell is legal
    static constexpr int SYM_RAW = 7;                                    // the identity is the LAST entry of symmetries(), as othello
    static constexpr uint64_t ROWS4 = 0x7FFF7FFF7FFF7FFFULL, ROWS3 = 0x00007FFF7FFF7FFFULL;     // the board's bits of words 0-2 / 3
    static constexpr const char *SCRIPTED = "GreedyGobangPlayer";
    static constexpr bool SCRIPTED_DRAWS = false;
    struct S { uint64_t b0[4], b1[4]; int player, turns; };              // b0: colour 1 (player 0), b1: colour -1

    static AZG_DEV int bit_of(int i) { return (i / 15) * 16 + i % 15; }  // cell -> packed bit
    static AZG_DEV uint64_t word(const uint64_t (&b)[4], int w) { return w == 0 ? b[0] : w == 1 ? b[1] : w == 2 ? b[2] : b[3]; }
    static AZG_DEV int bit(const uint64_t (&b)[4], int p) { return (int)((word(b, p >> 6) >> (p & 63)) & 1); }
    static AZG_DEV uint64_t rows(int w) { return w == 3 ? ROWS3 : ROWS4; }
    static AZG_DEV S load(const azg_state *st, int lane) {               // (azg.h: two packed boards in cells[64])
        (void)lane;
        const uint32_t *q = reinterpret_cast<const uint32_t *>(st->cells);
        S s;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            s.b0[w] = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)q[2 * w + 1]) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)q[2 * w]);
            s.b1[w] = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)q[9 + 2 * w]) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)q[8 + 2 * w]);
        }
        s.player = __builtin_amdgcn_readfirstlane(st->player);
        s.turns = __builtin_amdgcn_readfirstlane(st->turns);
        return s;
    }
    static AZG_DEV void init(S &s) {
#pragma unroll
        for (int w = 0; w < 4; w++) { s.b0[w] = 0; s.b1[w] = 0; }
        s.player = 0; s.turns = 0;
    }
    static AZG_DEV int cell(const S &s, int i) { const int p = bit_of(i); return bit(s.b0, p) - bit(s.b1, p); }
    static AZG_DEV void store(const S &s, azg_state *st, int lane) {     // lane j < 16 writes 32-bit word j of the two boards
        if (lane < 16) {
            const int w = (lane >> 1) & 3;
            const uint64_t v = lane < 8 ? word(s.b0, w) : word(s.b1, w);
            reinterpret_cast<uint32_t *>(st->cells)[lane] = (lane & 1) ? (uint32_t)(v >> 32) : (uint32_t)v;
        }
        if (lane == 0) { st->player = s.player; st->turns = s.turns; st->aux[0] = 0; st->aux[1] = 0; }
    }
    static AZG_DEV void play(S &s, int a) {                              // execute_move (GobangLogic.pyx:94-99)
        const int p = bit_of(__builtin_amdgcn_readfirstlane(a));
        const uint64_t m = 1ULL << (p & 63);
#pragma unroll
        for (int w = 0; w < 4; w++) {
            if (w == (p >> 6)) { if (s.player == 0) s.b0[w] |= m; else s.b1[w] |= m; }
        }
        s.player ^= 1; s.turns += 1;
    }
    // the 256-bit board shifted towards bit 0 by d < 64 bits: bit q of the result is bit q + d of b
    static AZG_DEV void shr(const uint64_t (&b)[4], int d, uint64_t (&o)[4]) {
#pragma unroll
        for (int w = 0; w < 4; w++) o[w] = (b[w] >> d) | (w < 3 ? b[w + 1] << (64 - d) : 0ULL);
    }
    // start cells of a run of five of `b`: bit q is set iff q, q + d, ..., q + 4d all are, for the four steps of get_win_state
    // (GobangLogic.pyx:66-86): along the first index (+16), the second (+1), the diagonal (+17) and the anti-diagonal (w + l, h - l:
    // +15).  A run that would leave the board passes a padding bit or a bit behind row 14, which are zero.
    static AZG_DEV void fives(const uint64_t (&b)[4], uint64_t (&acc)[4]) {
#pragma unroll
        for (int w = 0; w < 4; w++) acc[w] = 0;
        const int steps[4] = {16, 1, 17, 15};
#pragma unroll
        for (int di = 0; di < 4; di++) {
            uint64_t r[4] = {b[0], b[1], b[2], b[3]}, t[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                shr(r, steps[di], t);
#pragma unroll
                for (int w = 0; w < 4; w++) r[w] = b[w] & t[w];
            }
#pragma unroll
            for (int w = 0; w < 4; w++) acc[w] |= r[w];
        }
    }
    // win_state (gobang.pyx:133-148, get_win_state): the scan visits start cells (w outer, h inner) in ascending packed-bit order and
    // the first run it meets decides, so of two colours that both hold a five the one whose earliest start cell is lower wins; no
    // run and no empty cell: a draw
    static AZG_DEV int win_bits(const S &s) {
        uint64_t f0[4], f1[4];
        fives(s.b0, f0); fives(s.b1, f1);
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const uint64_t m = f0[w] | f1[w];
            if (m) return (f0[w] & (m & (~m + 1))) ? 1 : 2;
        }
        bool full = true;
#pragma unroll
        for (int w = 0; w < 4; w++) full = full && (s.b0[w] | s.b1[w]) == rows(w);
        return full ? 4 : 0;
    }
    // GreedyGobangPlayer.play (GobangPlayers.py:37): int(child.win_state()[child.player]) -- 1 when the child's mover holds the five
    // that the scan meets first, which the move just played cannot have made
    static AZG_DEV int scripted_key(const S &parent, const S &child) {
        (void)parent;
        return (win_bits(child) >> child.player) & 1;
    }
    // child i < k of the list is the i-th empty cell (ascending): the lane of every empty cell stores its cell number at its rank (the
    // empty cells below it) in act_lds, then lane l reads child c * 64 + l back
    static AZG_DEV int valid_list(const S &s, int lane, int *act_lds, int (&my_a)[4]) {
        uint64_t e[4];
#pragma unroll
        for (int w = 0; w < 4; w++) e[w] = ~(s.b0[w] | s.b1[w]) & rows(w);
        const int c0 = __popcll(e[0]), c1 = __popcll(e[1]), c2 = __popcll(e[2]), k = c0 + c1 + c2 + __popcll(e[3]);
        wave_sync();                                                     // (an earlier list's reads are done)
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int i = c * 64 + lane;
            if (i < CELLS) {
                const int p = bit_of(i), w = p >> 6, b = p & 63;
                const uint64_t ew = word(e, w);
                if ((ew >> b) & 1)
                    act_lds[(w > 0 ? c0 : 0) + (w > 1 ? c1 : 0) + (w > 2 ? c2 : 0) + __popcll(ew & ((1ULL << b) - 1ULL))] = i;
            }
        }
        wave_sync();
#pragma unroll
        for (int c = 0; c < 4; c++) my_a[c] = c * 64 + lane < k ? act_lds[c * 64 + lane] : -1;
        return k;
    }
    // observation (gobang.pyx:150-157): pieces == 1, pieces == -1, a plane of `player`, a plane of float32(turns / 225)
    static AZG_DEV float turn_plane(const S &s) { return (float)((double)s.turns / 225.0); }
    template <typename OT_> static AZG_DEV void write_obs(const S &s, OT_ *out, int lane) {
        const float pl = (float)s.player, tn = turn_plane(s);
        for (int c = lane; c < CELLS; c += 64) {
            const int p = bit_of(c);
            out[c] = (OT_)(float)bit(s.b0, p);
            out[CELLS + c] = (OT_)(float)bit(s.b1, p);
            out[2 * CELLS + c] = (OT_)pl;
            out[3 * CELLS + c] = (OT_)tn;
        }
    }
    typedef _Float16 h8 __attribute__((ext_vector_type(8)));
    static AZG_DEV h8 obs8(const S &s, int c) {                          // the row of cell c (any cell, not only the lane's)
        const int p = bit_of(c);
        return (h8){(_Float16)(float)bit(s.b0, p), (_Float16)(float)bit(s.b1, p), (_Float16)(float)s.player, (_Float16)turn_plane(s),
                    (_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f};
    }
    static AZG_DEV void write_obs_nhwc8(const S &s, _Float16 *out, int lane) {
        for (int c = lane; c < CELLS; c += 64) *reinterpret_cast<h8 *>(out + c * 8) = obs8(s, c);
    }
    // symmetries (gobang.pyx:159-182): entry k = 2(i-1) + (0 if flipped else 1), i = 1..4: fliplr^flip(rot90^i(pieces)), so k = 7 is
    // the identity.  Word w of the result is built by one ballot: lane l looks up the source of packed bit 64 w + l
    static AZG_DEV S symmetry(const S &s, int k) {
        const int lane = threadIdx.x & 63;
        const int i = k / 2 + 1;
        S o = s;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const int p = w * 64 + lane;
            int r = p >> 4, c = p & 15;
            const bool on = r < 15 && c < 15;
            if ((k & 1) == 0) c = 14 - c;
            for (int t = 0; t < i; t++) { const int nr = c, nc = 14 - r; r = nr; c = nc; }
            const int src = on ? r * 16 + c : 0;
            o.b0[w] = __ballot(on && bit(s.b0, src));
            o.b1[w] = __ballot(on && bit(s.b1, src));
        }
        return o;
    }
    // where pi[a] lands under symmetry k (the forward maps: rot90 sends (r, c) to (14-c, r), fliplr (r, c) to (r, 14-c))
    static AZG_DEV int sym_action(int a, int k) {
        const int i = k / 2 + 1;
        int r = a / 15, c = a % 15;
        for (int t = 0; t < i; t++) { const int nr = 14 - c, nc = r; r = nr; c = nc; }
        if ((k & 1) == 0) c = 14 - c;
        return r * 15 + c;
    }
};


// ================================================================================================ tictactoe
// alphazero/envs/tictactoe/tictactoe.py + TicTacToeLogic.py: 3x3, three in a row.  Cell i = 3x + y of the reference's pieces[x][y] (action a
// places a stone on cell a, every empty cell is legal -- also at a position that is already won), colour 1 for player 0 and -1 for
// player 1.  One 9-bit bitboard per colour in SGPRs.  The reference's max_turns() is None (Game.py:56-58: turns never decide anything and
// the temperature schedule never steps, utils.py:19-23); MAX_TURNS = 9 here only sizes history, paths and the default node store.
struct TT {
    static constexpr int ID = AZG_GAME_TICTACTOE;
    static constexpr const char *NAME = "tic-tac-toe";
    static constexpr bool SPARSE_HEADS = false;   // A = 9 is one output subtile, which the exact heads compute whole at the same cost
    static constexpr const char *SCRIPTED = nullptr;                     // no scripted baseline player (k_game_choose_scripted refuses the game)
    static constexpr int A = 9, H = 3, W = 3, CELLS = 9, P = 2, HAS_DRAW = 1, MAX_TURNS = 9, NSYM = 8;
    static constexpr int OBS_C = 1, OBS = OBS_C * CELLS, MAXK = 9;
    static constexpr int SYM_RAW = 7;                                    // the identity is the LAST entry of symmetries(), as othello
    static constexpr uint32_t FULL = 0x1FFu;
    struct S { uint32_t b0, b1; int player, turns; };                    // b0: colour 1 (player 0), b1: colour -1

    static AZG_DEV S load(const azg_state *st, int lane) {
        const int8_t v = lane < CELLS ? st->cells[lane] : (int8_t)0;
        S s;
        s.b0 = (uint32_t)__ballot(v == 1);
        s.b1 = (uint32_t)__ballot(v == -1);
        s.player = __builtin_amdgcn_readfirstlane(st->player);
        s.turns = __builtin_amdgcn_readfirstlane(st->turns);
        return s;
    }
    static AZG_DEV void init(S &s) { s.b0 = s.b1 = 0; s.player = 0; s.turns = 0; }
    static AZG_DEV int cell(const S &s, int i) { return (int)((s.b0 >> i) & 1) - (int)((s.b1 >> i) & 1); }
    static AZG_DEV void store(const S &s, azg_state *st, int lane) {
        st->cells[lane] = lane < CELLS ? (int8_t)cell(s, lane) : (int8_t)0;
        if (lane == 0) { st->player = s.player; st->turns = s.turns; st->aux[0] = 0; st->aux[1] = 0; }
    }
    static AZG_DEV uint64_t valid_mask(const S &s) { return ~(s.b0 | s.b1) & FULL; }            // get_legal_moves (TicTacToeLogic.py:39-52)
    static AZG_DEV void play(S &s, int a) {                              // execute_move (TicTacToeLogic.py:107-116) + Game.py:76-79
        const uint32_t bit = 1u << (__builtin_amdgcn_readfirstlane(a) & 15);
        if (s.player == 0) s.b0 |= bit; else s.b1 |= bit;
        s.player ^= 1; s.turns += 1;
    }
    // is_win (TicTacToeLogic.py:61-105): the counts along a strip are never reset, so on a 3-wide board a strip wins iff all three of
    // its cells hold the colour: the three y-strips (bits y, 3 + y, 6 + y), the three x-strips, the two diagonals
    static AZG_DEV bool has3(uint32_t m) {
        return (m & 0x049u) == 0x049u || (m & 0x092u) == 0x092u || (m & 0x124u) == 0x124u ||
               (m & 0x007u) == 0x007u || (m & 0x038u) == 0x038u || (m & 0x1C0u) == 0x1C0u ||
               (m & 0x111u) == 0x111u || (m & 0x054u) == 0x054u;
    }
    // win_state (tictactoe.py:67-78): the mover's line first, then the opponent's, then a draw if no cell is empty -- on a built board
    // where both colours hold a line the player to move wins
    static AZG_DEV int win_bits(const S &s) {
        const uint32_t own = s.player == 0 ? s.b0 : s.b1, opp = s.player == 0 ? s.b1 : s.b0;
        if (has3(own)) return 1 << s.player;
        if (has3(opp)) return 1 << (s.player ^ 1);
        return (s.b0 | s.b1) == FULL ? 4 : 0;
    }
    // lane i < k receives the i-th empty cell in ascending order (A = 9: unrolled select, as connect4)
    static AZG_DEV int valid_list(const S &s, int lane, int *act_lds, int (&my_a)[1]) {
        const uint32_t vm = (uint32_t)valid_mask(s);
        const int k = __popc(vm);
        int a = -1, cnt = 0;
#pragma unroll
        for (int c = 0; c < A; c++) { if ((vm >> c) & 1) { if (cnt == lane) a = c; cnt++; } }
        my_a[0] = a; (void)act_lds;
        return k;
    }
    // observation (tictactoe.py:80-81): one plane of the raw pieces, absolute colours
    template <typename OT_> static AZG_DEV void write_obs(const S &s, OT_ *out, int lane) { if (lane < CELLS) out[lane] = (OT_)(float)cell(s, lane); }
    typedef _Float16 h8 __attribute__((ext_vector_type(8)));
    static AZG_DEV h8 obs8(const S &s, int lane) {
        return (h8){(_Float16)(float)cell(s, lane), (_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f};
    }
    static AZG_DEV void write_obs_nhwc8(const S &s, _Float16 *out, int lane) {
        if (lane < CELLS) *reinterpret_cast<h8 *>(out + lane * 8) = obs8(s, lane);
    }
    // symmetries (tictactoe.py:83-102): entry k = 2(i-1) + (0 if flipped else 1), i = 1..4: fliplr^flip(rot90^i(pieces)), so k = 7 is the
    // identity.  np.rot90: out[r][c] = in[c][2-r]; np.fliplr: out[r][c] = in[r][2-c]
    static AZG_DEV S symmetry(const S &s, int k) {
        const int lane = threadIdx.x & 63;
        const int i = k / 2 + 1;
        const int l9 = lane < CELLS ? lane : 0;
        int r = l9 / 3, c = l9 - (l9 / 3) * 3;
        if ((k & 1) == 0) c = 2 - c;
        for (int t = 0; t < i; t++) { const int nr = c, nc = 2 - r; r = nr; c = nc; }
        const int src = r * 3 + c;
        S o = s;
        o.b0 = (uint32_t)__ballot(lane < CELLS && ((s.b0 >> src) & 1));
        o.b1 = (uint32_t)__ballot(lane < CELLS && ((s.b1 >> src) & 1));
        return o;
    }
    // where pi[a] lands under symmetry k (the forward maps: rot90 sends (r, c) to (2-c, r), fliplr (r, c) to (r, 2-c))
    static AZG_DEV int sym_action(int a, int k) {
        const int i = k / 2 + 1;
        int r = a / 3, c = a - (a / 3) * 3;
        for (int t = 0; t < i; t++) { const int nr = 2 - c, nc = r; r = nr; c = nc; }
        if ((k & 1) == 0) c = 2 - c;
        return r * 3 + c;
    }
};

// ================================================================================================ hnefatafl
// 11x11 tafl: alphazero/envs/hnefatafl/fastafl.pyx (Game) + fastafl/cengine.pyx (Board), board options of variants.hnefatafl_args: NO
// two-sided king capture (the king is never taken by custodian capture; Board.king_captured() is recomputed from the board at every
// get_winner: every in-bounds neighbour of the king holds a defender-code piece 2, the empty throne or a corner), moves over the empty
// throne, the king cannot re-enter it.  Board codes and the action codec are brandubh's with 11 in place of 7: action = 20 (x + 11 y) +
// move_type.  121 cells are more than a wavefront has lanes: lane l owns cell l (c0) and cell 64 + l (c1, l < 57), and a set of cells
// is a 128-bit mask M of two wave ballots, bit c & 63 of word c >> 6 -- the word boundary falls inside row 5, between x = 8 and x = 9.
// Shifts by one row (11) and one column (1, with the wrapping column cleared first) carry between the words.  Everything else follows
// struct BR: sliding moves from the 11-bit row of the passable mask and, through the transposed board, its column; custodian captures
// by uniform reads around the moved piece; the group-surround check (cengine.pyx:204-247) as a flood fill on the masks.
struct HN {
    static constexpr int ID = AZG_GAME_HNEFATAFL;
    static constexpr const char *NAME = "hnefatafl";
    static constexpr bool SPARSE_HEADS = false;   // no network launch is built for this game at all
    static constexpr const char *SCRIPTED = nullptr;                     // no scripted baseline player (k_game_choose_scripted refuses the game)
    static constexpr int A = 2420, H = 11, W = 11, CELLS = 121, P = 2, HAS_DRAW = 1, MAX_TURNS = 512, NSYM = 8;
    // MAXK bounds the move list of ANY board azg_set_states can hand over: every move lands on a cell that holds no piece, and a cell is
    // reached by at most one mover piece from each of the four directions, so with n mover pieces k <= min(20 n, 4 (121 - n)) <= 403
    // (n = 20); 448 = seven chunks of 64.  valid_list clamps all the same.
    static constexpr int OBS_C = 5, OBS = OBS_C * CELLS, MAXK = 448;
    static constexpr int SYM_RAW = 6;                                    // the identity, as brandubh (fastafl.pyx:216-259, k = 2*(4-1) + 0)
    static constexpr int HI = CELLS - 64;                                // cells of the second word
    struct M { uint64_t lo, hi; };
    struct S { int c0, c1; int player, turns, kc; };                     // c1 == 0 in lanes >= HI, always

    static constexpr M colmask(int x) {
        M m{0, 0};
        for (int y = 0; y < 11; y++) { const int c = 11 * y + x; if (c < 64) m.lo |= 1ULL << c; else m.hi |= 1ULL << (c - 64); }
        return m;
    }
    static constexpr uint64_t HI_ALL = (1ULL << HI) - 1;
    static AZG_DEV M mor(M a, M b) { return M{a.lo | b.lo, a.hi | b.hi}; }
    static AZG_DEV M mand(M a, M b) { return M{a.lo & b.lo, a.hi & b.hi}; }
    static AZG_DEV M mandn(M a, M b) { return M{a.lo & ~b.lo, a.hi & ~b.hi}; }           // a without b
    static AZG_DEV bool any(M a) { return (a.lo | a.hi) != 0; }
    static AZG_DEV bool same(M a, M b) { return a.lo == b.lo && a.hi == b.hi; }
    static AZG_DEV M single(int c) { return c < 64 ? M{1ULL << (c & 63), 0ULL} : M{0ULL, 1ULL << (c & 63)}; }
    static AZG_DEV bool has(M a, int c) { return (((c < 64 ? a.lo : a.hi) >> (c & 63)) & 1) != 0; }
    static AZG_DEV M shl(M m, int d) { return M{m.lo << d, (m.hi << d) | (m.lo >> (64 - d))}; }      // 0 < d < 64
    static AZG_DEV M shr(M m, int d) { return M{(m.lo >> d) | (m.hi << (64 - d)), m.hi >> d}; }
    static AZG_DEV M nbr(M m) {                     // squares orthogonally adjacent to the set m (board edges: nothing)
        constexpr M C0 = colmask(0), C10 = colmask(10);
        const M a = shl(m, 11), b = shr(m, 11), c = shl(mandn(m, C10), 1), d = shr(mandn(m, C0), 1);
        return M{a.lo | b.lo | c.lo | d.lo, (a.hi | b.hi | c.hi | d.hi) & HI_ALL};
    }
    // the 11 bits of m from bit p (p = 11 j, per lane)
    static AZG_DEV unsigned line11(M m, int p) {
        const uint64_t v = p < 64 ? ((m.lo >> (p & 63)) | (p ? (m.hi << ((64 - p) & 63)) : 0ULL)) : (m.hi >> ((p - 64) & 63));
        return (unsigned)v & 0x7FFu;
    }
    static AZG_DEV bool is_king(int v) { return v == 3 || v == 7 || v == 8; }
    static AZG_DEV bool is_att(int v) { return v == 1 || is_king(v); }                       // ATTACKERS cengine.pyx:42
    template <class F> static AZG_DEV M mask(const S &s, int lane, F &&f) { return M{__ballot(f(s.c0)), __ballot(lane < HI && f(s.c1))}; }
    static AZG_DEV M mask_eq(const S &s, int lane, int v) { return M{__ballot(s.c0 == v), __ballot(lane < HI && s.c1 == v)}; }
    // the value of cell idx: a wave-uniform index / a per-lane one (every lane takes part)
    static AZG_DEV int rd(const S &s, int idx) {
        idx = __builtin_amdgcn_readfirstlane(idx);
        const int a = __builtin_amdgcn_readlane(s.c0, idx & 63), b = __builtin_amdgcn_readlane(s.c1, idx & 63);
        return idx < 64 ? a : b;
    }
    static AZG_DEV int get(const S &s, int idx) {
        const int a = __shfl(s.c0, idx & 63), b = __shfl(s.c1, idx & 63);
        return idx < 64 ? a : b;
    }
    static AZG_DEV void put(S &s, int lane, int idx, int v) {            // idx < CELLS, wave-uniform
        if (idx < 64) { if (lane == idx) s.c0 = v; } else if (lane == idx - 64) s.c1 = v;
    }

    static AZG_DEV S load(const azg_state *st, int lane) {               // (azg.h: two cells per byte, the even cell in the low nibble)
        const uint8_t *q = reinterpret_cast<const uint8_t *>(st->cells);
        const int c1 = 64 + lane;
        S s;
        s.c0 = (q[lane >> 1] >> ((lane & 1) * 4)) & 15;
        s.c1 = lane < HI ? (q[c1 >> 1] >> ((c1 & 1) * 4)) & 15 : 0;
        s.player = __builtin_amdgcn_readfirstlane(st->player);
        s.turns = __builtin_amdgcn_readfirstlane(st->turns);
        s.kc = __builtin_amdgcn_readfirstlane(st->aux[0]);
        return s;
    }
    static AZG_DEV int start_cell(int c) {          // fastafl/variants.py:1-11: the standard 11x11 opening
        const int y = c / 11, x = c - y * 11;
        const int dx = x < 5 ? 5 - x : x - 5, dy = y < 5 ? 5 - y : y - 5;
        if (dx == 5 && dy == 5) return 5;
        if (dx == 0 && dy == 0) return 7;
        if (dx + dy <= 2) return 1;
        if ((dy == 5 && dx <= 2) || (dx == 5 && dy <= 2) || (dy == 4 && dx == 0) || (dx == 4 && dy == 0)) return 2;
        return 0;
    }
    static AZG_DEV void init(S &s) {
        const int lane = threadIdx.x & 63;
        s.c0 = start_cell(lane); s.c1 = lane < HI ? start_cell(64 + lane) : 0;
        s.player = 0; s.turns = 0; s.kc = 0;
    }
    static AZG_DEV void store(const S &s, azg_state *st, int lane) {     // lane j writes byte j: cells 2j and 2j + 1 (cell 121 and bytes 61..63: zero)
        const int ve = get(s, 2 * lane), vo = get(s, 2 * lane + 1);
        st->cells[lane] = lane * 2 < CELLS ? (int8_t)(ve | (vo << 4)) : (int8_t)0;
        if (lane == 0) { st->player = s.player; st->turns = s.turns; st->aux[0] = s.kc; st->aux[1] = 0; }
    }
    static AZG_DEV void decode(int a, int &src, int &dst) {          // fastafl.pyx:46-63 get_move
        const int mt = a % 20; src = a / 20;
        const int sx = src % 11, sy = src / 11;
        int nx, ny;
        if (mt < 10) { nx = sx; ny = mt + (mt >= sy ? 1 : 0); }
        else { nx = mt - 10; nx += (nx >= sx ? 1 : 0); ny = sy; }
        dst = ny * 11 + nx;
    }
    static AZG_DEV int encode(int x, int y, int nx, int ny) {        // fastafl.pyx:66-79 get_action
        const int mt = x == nx ? (ny < y ? ny : ny - 1) : (nx < x ? 10 + nx : 10 + nx - 1);
        return 20 * (x + y * 11) + mt;
    }
    // Board.move (cengine.pyx:249-272, no validity / win checks) + _check_capture (:174-199) + _check_surround (:228-247)
    static AZG_DEV void play(S &s, int a) {
        const int lane = threadIdx.x & 63;
        a = __builtin_amdgcn_readfirstlane(a);
        int src, dst; decode(a, src, dst);
        const int srcv = rd(s, src), dstv = rd(s, dst);
        const int piece = (srcv == 7 || srcv == 8) ? 3 : srcv;                               // remove_piece :315-330
        const int newsrc = srcv == 7 ? 4 : srcv == 8 ? 5 : 0;
        const int newdst = (dstv == 4 || dstv == 5) ? piece + dstv : piece;                  // add_piece :294-313
        put(s, lane, src, newsrc);
        put(s, lane, dst, newdst);
        // every capture below starts from a square next to the moved piece that holds an enemy (custodian: 3 - mover, never a king;
        // surround: the enemy team, kings included for a black mover): most moves have none, and are done here
        {
            const bool black = newdst == 2;
            const M relevant = black ? mask(s, lane, [](int v) { return is_att(v); }) : mask_eq(s, lane, 2);
            if (!any(mand(nbr(single(dst)), relevant))) { s.turns += 1; s.player ^= 1; return; }
        }
        const int dx4[4] = {0, 1, 0, -1}, dy4[4] = {1, 0, -1, 0};                            // DIRECTIONS :46
        const int mx = dst % 11, my = dst / 11;
        // ---- custodian capture around the moved piece: against a friendly piece, the empty throne or a corner ----
        const bool friendly_att = is_att(newdst);
        const int enemy = newdst != 3 ? 3 - newdst : 2;
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const int ex = mx + dx4[d], ey = my + dy4[d];
            if (ex < 0 || ex > 10 || ey < 0 || ey > 10) continue;
            if (rd(s, ey * 11 + ex) != enemy) continue;
            const int fx = ex + dx4[d], fy = ey + dy4[d];
            if (fx < 0 || fx > 10 || fy < 0 || fy > 10) continue;
            const int fv = rd(s, fy * 11 + fx);
            const bool friendly = friendly_att ? is_att(fv) : fv == newdst;
            if (friendly || fv == 4 || fv == 5) put(s, lane, ey * 11 + ex, 0);
        }
        // ---- group surround: start squares in DIRECTIONS order, removals visible to the later ones ----
        const bool enemy_is_att = rd(s, dst) == 2;
        M checked{0, 0};
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const int ex = mx + dx4[d], ey = my + dy4[d];
            if (ex < 0 || ex > 10 || ey < 0 || ey > 10) continue;
            const int e = ey * 11 + ex;
            const M enemyM = enemy_is_att ? mask(s, lane, [](int v) { return is_att(v); }) : mask_eq(s, lane, 2);
            if (!has(enemyM, e) || has(checked, e)) continue;
            M g = single(e);
            for (;;) { const M g2 = mor(g, mand(nbr(g), enemyM)); if (same(g2, g)) break; g = g2; }
            checked = mor(checked, g);
            if (!any(mand(nbr(g), mask_eq(s, lane, 0)))) {                                   // every member fully blocked
                if (any(mand(g, mask(s, lane, [](int v) { return is_king(v); })))) s.kc = 1; // a king is never lifted (:242-243)
                if (((g.lo >> lane) & 1) && !is_king(s.c0)) s.c0 = 0;
                if (lane < HI && ((g.hi >> lane) & 1) && !is_king(s.c1)) s.c1 = 0;
            }
        }
        s.turns += 1; s.player ^= 1;
    }
    // Game.win_state (fastafl.pyx:194-206: the draw first) + Board.get_winner (cengine.pyx:163-169) + king_captured (:154-161) +
    // _has_legals_check (:134-141)
    static AZG_DEV int win_bits(const S &s) {
        const int lane = threadIdx.x & 63;
        if (s.turns >= MAX_TURNS) return 4;
        const M esc = mask_eq(s, lane, 8), m2 = mask_eq(s, lane, 2);
        const M adjE = nbr(mask_eq(s, lane, 0)), adjX = nbr(mask_eq(s, lane, 5));
        const M kings = mask(s, lane, [](int v) { return is_king(v); });
        const bool def_has = any(mand(m2, adjE));
        const bool att_has = any(mor(mand(mask_eq(s, lane, 1), adjE), mand(kings, mor(adjE, adjX))));
        if (any(esc) || !def_has) return 2;           // attackers (player 1) win: result[2 - 1]
        // a king all of whose in-bounds neighbours hold 2, the empty throne or a corner (KING_CAPTURE :44)
        const M holds = mask(s, lane, [](int v) { return v == 2 || v == 4 || v == 5; });
        const M open = M{~holds.lo, ~holds.hi & HI_ALL};
        const bool boxed = any(mandn(kings, nbr(open)));
        if (s.kc || boxed || !att_has) return 1;      // defenders (player 0) win: result[2 - 2]
        return 0;
    }
    // cells of an 11-cell line (bit p = the piece's own position) a sliding piece at p reaches: the runs of passable cells on both
    // sides of p (Board.legal_moves walks them square by square, cengine.pyx:109-132)
    static AZG_DEV unsigned reach11(unsigned line, int p) {
        const unsigned up = line >> (p + 1);                                  // cells above p, bit 0 = p + 1
        const unsigned run = (unsigned)__builtin_ctz(~up);                    // trailing ones (an 11-bit line: ~up is never 0)
        const unsigned reach_up = ((1u << run) - 1u) << (p + 1);
        const unsigned below = (1u << p) - 1u, blk = ~line & below;           // blockers below p
        const unsigned cut = blk ? (2u << (31 - __builtin_clz(blk))) : 1u;    // first bit above the highest blocker
        return reach_up | (line & below & ~(cut - 1u));
    }
    // the 20 move types of the piece on cell c (< CELLS) as a bit set: vertical ny -> ny or ny - 1, horizontal nx -> 10 + nx or 10 + nx - 1
    // (fastafl.pyx:66-79).  pass / passT: the cells a ray continues over, T / Tt the empty throne (nobody lands on it), both also transposed
    static AZG_DEV unsigned cell_moves(M pass, M passT, M T, M Tt, int c) {
        const int y = c / 11, x = c - y * 11;
        const unsigned row = line11(pass, 11 * y), col = line11(passT, 11 * x);
        const unsigned rx = reach11(row, x) & ~line11(T, 11 * y), ry = reach11(col, y) & ~line11(Tt, 11 * x);
        const unsigned mvy = (ry & ((1u << y) - 1u)) | ((ry >> (y + 1)) << y), mvx = (rx & ((1u << x) - 1u)) | ((rx >> (x + 1)) << x);
        return mvy | (mvx << 10);
    }
    // Game.valid_moves (fastafl.pyx:179-186) + Board.legal_moves (cengine.pyx:109-132): ascending action list in LDS -- cells in
    // ascending order (the lanes' first cells, then their second ones), the move types of a cell in ascending order.
    static AZG_DEV int valid_list(const S &s, int lane, int *act_lds, int (&my_a)[7]) {
        const int team = 2 - (s.turns & 1);                                                  // Board.to_play :332-333
        const int cA = lane, cB = lane < HI ? 64 + lane : CELLS - 1;
        const bool mineA = team == 1 ? is_att(s.c0) : s.c0 == 2, mineB = lane < HI && (team == 1 ? is_att(s.c1) : s.c1 == 2);
        // the transposed board: the cell (x, y) of the lane's cell (y, x)
        const int tA = get(s, (cA % 11) * 11 + cA / 11), tB = get(s, (cB % 11) * 11 + cB / 11);
        const M E = mask_eq(s, lane, 0), T = mask_eq(s, lane, 4), X = mask_eq(s, lane, 5);
        const M Et{__ballot(tA == 0), __ballot(lane < HI && tB == 0)}, Tt{__ballot(tA == 4), __ballot(lane < HI && tB == 4)},
                Xt{__ballot(tA == 5), __ballot(lane < HI && tB == 5)};
        const M ET = mor(E, T), ETt = mor(Et, Tt), ETX = mor(ET, X), ETXt = mor(ETt, Xt);    // (only the king's ray enters a corner)
        const bool kA = is_king(s.c0), kB = is_king(s.c1);
        const unsigned mvA = mineA ? cell_moves(kA ? ETX : ET, kA ? ETXt : ETt, T, Tt, cA) : 0u;
        const unsigned mvB = mineB ? cell_moves(kB ? ETX : ET, kB ? ETXt : ETt, T, Tt, cB) : 0u;
        const int cntA = __popc(mvA), cntB = __popc(mvB);
        const int totA = wave_sum_i(cntA), k = totA + wave_sum_i(cntB);
        const int offA = wave_excl_scan(cntA, lane), offB = totA + wave_excl_scan(cntB, lane);
        wave_sync();                                                     // (an earlier list's reads are done)
#pragma unroll
        for (int b = 0; b < 20; b++) {
            const int pa = offA + __popc(mvA & ((1u << b) - 1u)), pb = offB + __popc(mvB & ((1u << b) - 1u));
            if (((mvA >> b) & 1u) && pa < MAXK) act_lds[pa] = 20 * cA + b;
            if (((mvB >> b) & 1u) && pb < MAXK) act_lds[pb] = 20 * cB + b;
        }
        wave_sync();
        const int kk = k < MAXK ? k : MAXK;
#pragma unroll
        for (int c = 0; c < 7; c++) my_a[c] = c * 64 + lane < kk ? act_lds[c * 64 + lane] : -1;
        wave_sync();
        return kk;
    }
    // Game.observation (fastafl.pyx:82-119,208-214): planes [black(2), white(1), king, to-move colour, turns / 512 in integers]
    static AZG_DEV float plane(int p, int c, const S &s) {
        return p == 0 ? (c == 2 ? 1.f : 0.f) : p == 1 ? (c == 1 ? 1.f : 0.f) : p == 2 ? (is_king(c) ? 1.f : 0.f)
             : p == 3 ? (float)(s.turns & 1) : (float)(s.turns / MAX_TURNS);
    }
    template <typename OT_> static AZG_DEV void write_obs(const S &s, OT_ *out, int lane) {
#pragma unroll
        for (int p = 0; p < OBS_C; p++) {
            out[p * CELLS + lane] = (OT_)plane(p, s.c0, s);
            if (lane < HI) out[p * CELLS + 64 + lane] = (OT_)plane(p, s.c1, s);
        }
    }
    typedef _Float16 h8 __attribute__((ext_vector_type(8)));
    static AZG_DEV h8 obs8(const S &s, int c) {                  // the five planes of cell c, one of the calling lane's OWN two cells (lane or 64 + lane)
        const int v = c < 64 ? s.c0 : s.c1;
        return (h8){(_Float16)plane(0, v, s), (_Float16)plane(1, v, s), (_Float16)plane(2, v, s), (_Float16)plane(3, v, s),
                    (_Float16)plane(4, v, s), (_Float16)0.f, (_Float16)0.f, (_Float16)0.f};
    }
    static AZG_DEV void write_obs_nhwc8(const S &s, _Float16 *out, int lane) {
        *reinterpret_cast<h8 *>(out + lane * 8) = obs8(s, lane);
        if (lane < HI) *reinterpret_cast<h8 *>(out + (64 + lane) * 8) = obs8(s, 64 + lane);
    }
    // Game.symmetries (fastafl.pyx:216-259): k = (i-1)*2 + flip; state = fliplr^flip(rot90^i(state)); the policy index is permuted by
    // the reference's own coordinate loop (sym_action)
    static AZG_DEV int sym_source(int c, int i, int flip) {
        int r = c / 11, cc = c - (c / 11) * 11;
        if (flip) cc = 10 - cc;                            // final[r][c] = rotated[r][10-c]
        for (int t = 0; t < i; t++) { const int nr = cc, nc = 10 - r; r = nr; cc = nc; }    // rot90: new[r][c] = old[c][10-r]
        return r * 11 + cc;
    }
    static AZG_DEV S symmetry(const S &s, int k) {
        const int lane = threadIdx.x & 63;
        const int i = k / 2 + 1, flip = k & 1;
        S o = s;
        const int v0 = get(s, sym_source(lane, i, flip)), v1 = get(s, sym_source(lane < HI ? 64 + lane : 0, i, flip));
        o.c0 = v0; o.c1 = lane < HI ? v1 : 0;
        return o;
    }
    static AZG_DEV int sym_action(int a, int k) {
        const int i = k / 2 + 1, flip = k & 1;
        int src, dst; decode(a, src, dst);
        int x = src % 11, y = src / 11, nx = dst % 11, ny = dst / 11;
        for (int t = 0; t < i; t++) { const int tx = x, tnx = nx; x = 10 - y; nx = 10 - ny; y = tx; ny = tnx; }   // :241-247
        if (flip) { x = 10 - x; nx = 10 - nx; }
        return encode(x, y, nx, ny);
    }
};

// ================================================================================================ the list
// every game with device rules, in id order (azg_engine.hip holds each struct's ID to its place here): the game table, the switches
// on the game id and the sparse-heads refusals are all expanded from it, so a new game is a struct above and an entry here
#define AZG_GAMES(X, ...) X(C4, __VA_ARGS__) X(BR, __VA_ARGS__) X(TM, __VA_ARGS__) X(OT, __VA_ARGS__) X(GB, __VA_ARGS__) X(TT, __VA_ARGS__) X(HN, __VA_ARGS__)

}  // namespace azg
