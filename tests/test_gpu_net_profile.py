"""The library's timing hooks (azg_profile_net_* behind HipResNet.profile / profile_read, which bench.py's profile rounds read, and
azg_profile_* behind DeviceEngine.profile): which launches each entry point counts, per family.  Two networks of depth 1 on engines of
8 games with 4 simulations per move: connect4 x 128 (fused heads: azg_resnet_policy_value_f16, azg_search_f16) and tic-tac-toe x 32
(factorised heads: tower + head convolutions, the heads GEMM, the persistent wide search).

Every successful call counts exactly the launches it counted before the hooks became one record type behind a scope object.  The one
difference: a call the library REFUSES without a launch (test_a_refused_call_counts_nothing) used to add 1 to tower_n and put an event
pair that no dispatch had stamped on the family's list, so the next successful launch read tower_n == 2; it now counts nothing."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV, B, SIMS = 'cuda:0', 8, 4


def _net(game_cls, args):
    from alphazero_general_amd.nnet import NNetWrapper
    from alphazero_general_amd.utils import dotdict
    torch.manual_seed(0)
    return NNetWrapper(game_cls, dotdict(dict(args, depth=1)), device=DEV).refresh()._hip


@pytest.fixture(scope='module')
def fused():
    from alphazero_general_amd.envs.connect4 import Game
    from alphazero_general_amd.nnet import CONNECT4_NET_ARGS
    hip = _net(Game, CONNECT4_NET_ARGS)
    assert hip.fused_head and hip.CH == 128 and len(hip.blocks) == 1 and hip.can_search
    return hip


@pytest.fixture(scope='module')
def fact():
    from alphazero_general_amd.envs.tictactoe import Game
    from alphazero_general_amd.nnet import DEFAULT_NET_ARGS
    hip = _net(Game, DEFAULT_NET_ARGS)
    assert hip.fact_head and hip.CH == 32 and len(hip.blocks) == 1 and hip.can_search
    return hip


@pytest.fixture(autouse=True)
def hooks_off_afterwards():
    yield
    from alphazero_general_amd.nnet import HipResNet
    HipResNet.profile(False)


def _engine(hip):
    from alphazero_general_amd.engine import DeviceEngine
    return DeviceEngine(hip.game, B, seed=3, sims_hint=SIMS, device=0)


def _boards(hip):
    return torch.zeros((B, hip.HW, 8), dtype=torch.float16, device=DEV)


def _counts(step):
    """the (tower, heads, search) launches `step` adds, with the milliseconds: the counters are cleared by switching the hooks on"""
    from alphazero_general_amd.nnet import HipResNet
    HipResNet.profile(True)
    step()
    r = HipResNet.profile_read()
    return (r['tower_n'], r['heads_n'], r['search_n']), r


def test_forward_fused_is_one_tower_launch(fused):
    x = _boards(fused)
    fused.forward_nhwc8(x)                                       # (scratch allocated before the counted call)
    n, r = _counts(lambda: fused.forward_nhwc8(x))
    assert n == (1, 0, 0) and r['tower_ms'] > 0 and r['heads_ms'] == 0 and r['search_ms'] == 0


def test_forward_factorised_times_the_tower_and_the_heads_gemm(fact):
    x = _boards(fact)
    n, r = _counts(lambda: fact.forward_nhwc8(x))
    assert n == (1, 1, 0)                                        # three launches ran: the softmax behind the heads' GEMM is not timed
    assert r['tower_ms'] > 0 and r['heads_ms'] > 0
    n, _ = _counts(lambda: fact.forward_logits_nhwc8(x))         # ... and stopping at the logits counts the same
    assert n == (1, 1, 0)


def test_forward_features_is_one_tower_launch(fact):
    x = _boards(fact)
    n, r = _counts(lambda: fact.forward_features_nhwc8(x))
    assert n == (1, 0, 0) and r['tower_ms'] > 0


@pytest.mark.parametrize('which', ['fused', 'fact'])
def test_search_set_up_counts_nothing_and_a_search_counts_one(which, request):
    hip = request.getfixturevalue(which)
    eng = _engine(hip)
    n, r = _counts(lambda: hip.search(eng, 0, exact=True))       # set-up only: the wide launch's autotune trials are not counted
    assert n == (0, 0, 0) and (r['tower_ms'], r['heads_ms'], r['search_ms']) == (0, 0, 0)
    n, r = _counts(lambda: hip.search(eng, SIMS, exact=True))
    assert n == (0, 0, 1) and r['search_ms'] > 0

    def moves():
        for _ in range(3):
            eng.advance(record_history=False)                    # (the engine's launches are not the network's)
            hip.search(eng, SIMS, exact=True)
    n, _ = _counts(moves)
    assert n == (0, 0, 3)


def test_a_refused_call_counts_nothing(fused):
    """a pair without a tower (hnefatafl, game 6: device rules, no tile row) is refused after the hook was armed and before any launch: the
    armed pair must be disarmed and handed back, so that the refused call counts nothing and the next launch is timed as itself"""
    from alphazero_general_amd import _abi
    from alphazero_general_amd.nnet import HipResNet
    x = _boards(fused)
    fused.forward_nhwc8(x)
    HipResNet.profile(True)
    game, fused.game = fused.game, _abi.GAME_HNEFATAFL
    try:
        with pytest.raises(_abi.AzgError) as err:
            fused.forward_nhwc8(x)
    finally:
        fused.game = game
    assert err.value.code == _abi.E_UNSUPPORTED
    r = HipResNet.profile_read()
    assert (r['tower_n'], r['heads_n'], r['search_n']) == (0, 0, 0)
    fused.forward_nhwc8(x)
    r = HipResNet.profile_read()
    assert (r['tower_n'], r['heads_n'], r['search_n']) == (1, 0, 0) and r['tower_ms'] > 0
    eng = _engine(fused)                                         # the engine's own hooks share g_kev: nothing is left armed for them either
    eng.profile(True)
    eng.select(eng.new_obs(torch.float16))
    assert eng.profile_read()['select_n'] == 1 and HipResNet.profile_read()['tower_n'] == 1


def test_engine_hooks_count_one_launch_per_phase(fused):
    eng = _engine(fused)
    obs = eng.new_obs(torch.float16)
    pol = torch.full((B, eng.A), 1.0 / eng.A, dtype=torch.float32, device=DEV)
    val = torch.zeros((B, eng.NV), dtype=torch.float32, device=DEV)
    for _ in range(SIMS - 1):                                    # (a move is played from a tree that has been searched)
        eng.select(obs)
        eng.backup(pol, val)
    eng.profile(True)
    eng.select(obs)
    eng.backup(pol, val)
    eng.advance(record_history=False)
    r = eng.profile_read()
    assert (r['select_n'], r['backup_n'], r['advance_n']) == (1, 1, 1)
    assert r['select_ms'] > 0 and r['backup_ms'] > 0 and r['advance_ms'] > 0
    eng.profile(False)
    eng.select(obs)
    assert eng.profile_read()['select_n'] == 1                   # off: nothing more is counted
