"""The stand-alone tower's tile policy, the part that needs no GPU: azg_tower_tile (include/azg.h; the rows of csrc/azg_tiles.h) against the
policy written out HERE, per (game, tower width) and per interval of boards per CU, as the if-chain the rows replaced had it -- at one
board, at every limit and one board above it, and at 2^20 boards, for devices of 1 to 304 CUs.  The same points hold the tests' own
restatement (test_gpu_net_fp64.tile_boards, which decides which rows of a batch share a tile) and the games-per-workgroup rule bench.py
restates for azg_search_f16 to the library."""
import ctypes as C

import pytest

C4, BR, TM, OT, GB, TT, HN = range(7)
ENVS = {C4: 'connect4', BR: 'brandubh', TM: 'trimok', OT: 'othello', GB: 'gobang', TT: 'tictactoe'}
CUS = (1, 7, 80, 256, 304)
# (game, width): [(limit, (boards per tile, PSPLIT, KSPLIT)), ...] -- n boards on c CUs take the first entry with 2 n <= limit c; None: the rest
POLICY = {
    (C4, 128): [(5, (1, 1, 1)), (10, (2, 1, 1)), (None, (4, 1, 1))],
    (C4, 64): [(None, (4, 1, 1))],
    (C4, 32): [(8, (2, 2, 1)), (None, (4, 2, 1))],
    (BR, 64): [(4, (1, 1, 2)), (8, (2, 2, 1)), (None, (2, 1, 1))],
    (BR, 128): [(None, (2, 1, 1))],
    (TM, 32): [(16, (2, 2, 1)), (None, (5, 1, 1))],
    (OT, 32): [(8, (2, 2, 1)), (None, (4, 2, 1))],
    (OT, 64): [(4, (1, 1, 2)), (8, (2, 2, 1)), (None, (2, 1, 1))],
    (GB, 32): [(None, (1, 3, 1))],
    (GB, 64): [(None, (1, 3, 1))],
    (GB, 128): [(None, (1, 3, 1))],
    (TT, 32): [(16, (1, 1, 1)), (160, (5, 1, 1)), (None, (16, 1, 1))],
}


@pytest.fixture(scope='module')
def L():
    from alphazero_general_amd import build, _abi
    build.build()
    return _abi.lib()


def tile(L, game, ch, n, cus):
    t = (C.c_int32 * 3)()
    rc = L.azg_tower_tile(game, ch, n, cus, t)
    return tuple(t) if rc == 0 else rc


def points(rows, cus):
    """(n, the interval's tile): one board, every limit of the pair and one board above it, 2^20 boards"""
    ns = {1, 1 << 20}
    for lim, _ in rows:
        if lim is not None:
            ns |= {lim * cus // 2, lim * cus // 2 + 1}
    ns.discard(0)
    return [(n, next(t for lim, t in rows if lim is None or 2 * n <= lim * cus)) for n in sorted(ns)]


@pytest.mark.parametrize('cus', CUS)
@pytest.mark.parametrize('pair', sorted(POLICY))
def test_tile_at_every_limit(L, pair, cus):
    import test_gpu_net_fp64 as F
    game, ch = pair
    pts = points(POLICY[pair], cus)
    assert {t for _, t in pts} == {t for _, t in POLICY[pair]}            # the points reach every interval
    for n, want in pts:
        assert tile(L, game, ch, n, cus) == want, (pair, cus, n)
        assert F.tile_boards(ENVS[game], ch, n, cus) == want[0], (pair, cus, n)


def test_every_tower_pair_has_a_tile_and_no_other_pair(L):
    from alphazero_general_amd import _abi
    info = (C.c_int32 * 8)()
    for game in range(7):
        for ch in (32, 64, 128):
            has = bool(_abi.launch_support(game, ch) & _abi.SUPPORT_TOWER)
            assert has == ((game, ch) in POLICY), (game, ch)
            for n in (1, 37, 1000, 1 << 20):
                got = tile(L, game, ch, n, 256)
                if not has:
                    assert got == _abi.E_UNSUPPORTED, (game, ch, n, got)
                else:
                    assert isinstance(got, tuple) and L.azg_tower_layout(game, got[0], ch, None, None, info) == 0, (game, ch, n, got)
    assert tile(L, C4, 96, 8, 256) == _abi.E_UNSUPPORTED


def test_argument_errors_need_no_device(L):
    from alphazero_general_amd import _abi
    t = (C.c_int32 * 3)(-7, -7, -7)
    for game, ch, n, cus, out in ((C4, 128, 0, 256, t), (C4, 128, -1, 256, t), (C4, 128, 8, 0, t), (C4, 128, 8, -3, t), (C4, 128, 8, 256, None),
                                  (-1, 128, 8, 256, t), (7, 128, 8, 256, t), (HN, 128, 0, 256, t)):
        assert L.azg_tower_tile(game, ch, n, cus, out) == _abi.E_INVALID_ARG, (game, ch, n, cus)
    assert tuple(t) == (-7, -7, -7)
    assert L.azg_abi_version() == _abi.ABI_VERSION == 7                  # additive: no ABI bump


@pytest.mark.parametrize('cus', CUS)
def test_fused_search_games_per_workgroup_is_the_towers_tile(L, cus):
    """azg_search_f16 launches the connect4 x 128 tile of as many boards as the engine has games; bench.py restates that rule for its
    operand-stream bound"""
    for B in sorted({1, 32, 5 * cus // 2, 5 * cus // 2 + 1, 3 * cus, 5 * cus, 5 * cus + 1, 8192}):
        gpw = 1 if 2 * B <= 5 * cus else 2 if B <= 5 * cus else 4
        assert tile(L, C4, 128, B, cus)[0] == gpw, (B, cus)
