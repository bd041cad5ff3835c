"""The argument errors of the network entry points (include/azg.h: the stand-alone tower and heads launches, the persistent search
launches), the part that needs no GPU: every call below is refused before the library makes its first HIP call, so the return code and
the azg_last_error() text are a pure function of the arguments.  The table pins, per entry point, which code and which text a mistake
gets, and -- through the rows with two mistakes at once -- the ORDER of the checks.  Non-null pointers are the address of one host
buffer: nothing is dereferenced before the checks (the model arrays of the multi-model forms are host arrays and are read)."""
import ctypes as C

import pytest

INVALID, UNSUPPORTED = -1, -6
_BUF = C.create_string_buffer(64)
P = C.addressof(_BUF)                                            # "a pointer": any host address


def arr(*entries):
    return (C.c_void_p * len(entries))(*entries)


A4 = arr(P, P, P, P)                                             # a model array without a null entry
HOLE = arr(P, None, P, P)                                        # model 1 is missing

NULL_ARG = 'null argument'
NULL_RANGE = 'null or out-of-range argument'
AFFINE = 'pre_scale/pre_shift required'
FUSED16 = 'fused heads need A + NV <= 16'
MODELS = '1 to 4 models per launch'
NULL_MODEL = 'null model parameter'
FEAT32 = 'feat_k must be a positive multiple of 32'

# entry point -> its parameters in order, each with a value no check objects to
GOOD = {
    'azg_resnet_tower_f16': dict(stream=None, game=0, x=P, w=P, bias=P, pre_scale=P, pre_shift=P, y=P, boards=8, nblocks=1, channels=128),
    'azg_resnet_tower_features_f16': dict(stream=None, game=0, x=P, w=P, bias=P, pre_scale=P, pre_shift=P, boards=8, nblocks=1, channels=32,
                                          head1_w=P, head1_b=P, feat=P, feat_k=704),
    'azg_resnet_policy_value_f16': dict(stream=None, game=0, x=P, w=P, bias=P, pre_scale=P, pre_shift=P, boards=8, nblocks=1, head_w=P, head_b=P,
                                        A=7, NV=3, policy=P, value=P),
    'azg_resnet_policy_value_multi_f16': dict(stream=None, game=0, x=P, nmodels=2, w=A4, bias=A4, pre_scale=A4, pre_shift=A4, max_boards=8, nblocks=1,
                                              head_w=A4, head_b=A4, A=7, NV=3, policy=P, value=P, rows_per_model=P),
    'azg_search_f16': dict(e=P, stream=None, w=P, bias=P, pre_scale=P, pre_shift=P, nblocks=1, head_w=P, head_b=P, sims=4),
    'azg_search_arena_f16': dict(e=P, stream=None, nmodels=2, w=A4, bias=A4, pre_scale=A4, pre_shift=A4, nblocks=1, head_w=A4, head_b=A4,
                                 p2i=None, seats=P, sims=4),
    'azg_search_wide_f16': dict(e=P, stream=None, w=P, bias=P, pre_scale=P, pre_shift=P, nblocks=1, channels=32, head1_w=P, head1_b=P,
                                head_rows=P, head_b=P, feat_k=160, sims=4),
    'azg_search_wide_exact_f16': dict(e=P, stream=None, w=P, bias=P, pre_scale=P, pre_shift=P, nblocks=1, channels=32, head1_w=P, head1_b=P,
                                      wps=P, wv=P, head_b=P, feat_k=160, sims=4),
    'azg_search_arena_wide_exact_f16': dict(e=P, stream=None, nmodels=2, w=A4, bias=A4, pre_scale=A4, pre_shift=A4, nblocks=1, channels=32,
                                            head1_w=A4, head1_b=A4, wps=A4, wv=A4, head_b=A4, feat_k=160, p2i=None, seats=P, sims=4),
    'azg_policy_value_heads_f16': dict(stream=None, y=P, head_w=P, head_b=P, boards=8, k=64, A=7, NV=3, logits_ws=P, policy=P, value=P),
    'azg_policy_value_heads_fact_f16': dict(stream=None, feat=P, wp=P, wv=P, head_b=P, boards=8, feat_k=160, A=9, NV=3, logits_ws=P,
                                            policy=P, value=P),
    'azg_heads_softmax': dict(stream=None, logits=P, boards=8, stride=16, A=7, NV=3, policy=P, value=P),
    'azg_obs_to_nhwc8_f16': dict(stream=None, obs=P, boards=8, channels=3, hw=42, x=P),
}


def rows():
    """(entry point, the arguments that differ from GOOD, return code, azg_last_error text)"""
    out = []

    def row(fn, rc, text, **bad):
        assert set(bad) <= set(GOOD[fn]), (fn, bad)
        out.append((fn, bad, rc, text))

    # ---- the stand-alone tower launches: a null x / w / bias / output, residual blocks without their affines
    fn = 'azg_resnet_tower_f16'
    for name in ('x', 'w', 'bias', 'y'):
        row(fn, INVALID, NULL_ARG, **{name: None})
    row(fn, INVALID, NULL_ARG, boards=0)
    row(fn, INVALID, NULL_ARG, nblocks=-1)
    row(fn, INVALID, AFFINE, pre_scale=None)
    row(fn, INVALID, AFFINE, pre_shift=None)
    row(fn, INVALID, NULL_ARG, y=None, pre_scale=None)                       # the pointers before the affines
    fn = 'azg_resnet_tower_features_f16'
    for name in ('x', 'w', 'bias', 'head1_w', 'head1_b', 'feat'):
        row(fn, INVALID, NULL_ARG, **{name: None})
    row(fn, INVALID, AFFINE, pre_scale=None)
    row(fn, INVALID, AFFINE, pre_shift=None)
    row(fn, INVALID, FEAT32, feat_k=48)
    row(fn, INVALID, FEAT32, feat_k=0)
    row(fn, INVALID, AFFINE, pre_shift=None, feat_k=48)                      # the affines before feat_k
    row(fn, INVALID, NULL_ARG, feat=None, feat_k=0)
    fn = 'azg_resnet_policy_value_f16'
    for name in ('x', 'w', 'bias', 'head_w', 'head_b', 'policy', 'value'):
        row(fn, INVALID, NULL_ARG, **{name: None})
    row(fn, INVALID, AFFINE, pre_scale=None)
    row(fn, INVALID, AFFINE, pre_shift=None)
    row(fn, UNSUPPORTED, FUSED16, A=14, NV=3)
    row(fn, UNSUPPORTED, FUSED16, A=0)
    row(fn, UNSUPPORTED, FUSED16, A=14, NV=3, pre_scale=None)                # the heads' width before the affines
    row(fn, INVALID, NULL_ARG, A=14, NV=3, value=None)                       # the pointers before the heads' width
    fn = 'azg_resnet_policy_value_multi_f16'
    for name in ('x', 'w', 'bias', 'head_w', 'head_b', 'policy', 'value', 'rows_per_model'):
        row(fn, INVALID, NULL_RANGE, **{name: None})
    row(fn, INVALID, NULL_RANGE, max_boards=0)
    row(fn, UNSUPPORTED, MODELS, nmodels=0)
    row(fn, UNSUPPORTED, MODELS, nmodels=5)
    row(fn, UNSUPPORTED, FUSED16, A=14, NV=3)
    row(fn, INVALID, AFFINE, pre_scale=None)
    row(fn, INVALID, AFFINE, pre_shift=None)
    for name in ('w', 'bias', 'head_w', 'head_b', 'pre_scale', 'pre_shift'):
        row(fn, INVALID, NULL_MODEL, **{name: HOLE})
    row(fn, INVALID, NULL_RANGE, x=None, nmodels=0)                          # pointers, model count, heads' width, affines, models
    row(fn, UNSUPPORTED, MODELS, nmodels=5, A=14, NV=3)
    row(fn, UNSUPPORTED, FUSED16, A=14, NV=3, pre_scale=None)
    row(fn, INVALID, AFFINE, pre_shift=None, w=HOLE)
    # ---- the persistent search launches: a null engine, and the null head pointer each checks first
    fn = 'azg_search_f16'
    row(fn, INVALID, NULL_RANGE, e=None)
    for name in ('w', 'bias', 'head_w', 'head_b'):
        row(fn, INVALID, NULL_RANGE, **{name: None})
    row(fn, INVALID, NULL_RANGE, sims=-1)
    row(fn, INVALID, NULL_RANGE, e=None, pre_scale=None)                     # the engine before the affines
    fn = 'azg_search_arena_f16'
    row(fn, INVALID, NULL_RANGE, e=None)
    for name in ('w', 'bias', 'head_w', 'head_b'):
        row(fn, INVALID, NULL_RANGE, **{name: None})
    row(fn, INVALID, NULL_RANGE, seats=None)                                 # neither player_to_index nor seats
    row(fn, INVALID, NULL_RANGE, e=None, nmodels=5)
    fn = 'azg_search_wide_f16'                                               # its own heads first ("null argument"), then the common part
    row(fn, INVALID, NULL_RANGE, e=None)
    row(fn, INVALID, NULL_ARG, head_rows=None)
    row(fn, INVALID, NULL_ARG, head_b=None)
    row(fn, INVALID, NULL_ARG, e=None, head_rows=None)
    for name in ('w', 'bias', 'head1_w', 'head1_b'):
        row(fn, INVALID, NULL_RANGE, **{name: None})
    row(fn, INVALID, NULL_RANGE, sims=-1)
    row(fn, INVALID, NULL_RANGE, e=None, pre_scale=None)
    fn = 'azg_search_wide_exact_f16'                                         # the engine is among what it checks first
    row(fn, INVALID, NULL_ARG, e=None)
    for name in ('wps', 'wv', 'head_b'):
        row(fn, INVALID, NULL_ARG, **{name: None})
    for name in ('w', 'bias', 'head1_w', 'head1_b'):
        row(fn, INVALID, NULL_RANGE, **{name: None})
    row(fn, INVALID, NULL_ARG, e=None, w=None)
    row(fn, INVALID, NULL_RANGE, nblocks=-1)
    fn = 'azg_search_arena_wide_exact_f16'
    row(fn, INVALID, NULL_RANGE, e=None)
    for name in ('w', 'bias', 'pre_scale', 'pre_shift', 'head1_w', 'head1_b', 'wps', 'wv', 'head_b'):
        row(fn, INVALID, NULL_RANGE, **{name: None})
    row(fn, INVALID, NULL_RANGE, pre_scale=None, nblocks=0)                  # the affine arrays are required at any depth
    row(fn, INVALID, NULL_RANGE, seats=None)
    row(fn, INVALID, NULL_RANGE, e=None, nmodels=5, feat_k=48)
    # ---- the heads launches
    fn = 'azg_policy_value_heads_f16'
    HEADS = 'boards > 0, k a multiple of 32, 0 < A <= 1024, 0 < NV <= 64'
    for name in ('y', 'head_w', 'head_b', 'logits_ws'):
        row(fn, INVALID, NULL_ARG, **{name: None})
    row(fn, INVALID, NULL_ARG, policy=None)                                  # policy and value: both or neither
    row(fn, INVALID, NULL_ARG, value=None)
    row(fn, INVALID, HEADS, k=33)
    row(fn, INVALID, HEADS, k=0)
    row(fn, INVALID, HEADS, NV=65)
    row(fn, INVALID, HEADS, k=33, policy=None, value=None)                   # (neither: stops at the logits -- not an error)
    row(fn, INVALID, NULL_ARG, y=None, k=33)
    fn = 'azg_policy_value_heads_fact_f16'
    FACT = 'boards > 0, feat_k a multiple of 32, 0 < A <= 1024, 0 < NV <= 16'
    for name in ('feat', 'wp', 'wv', 'head_b', 'logits_ws'):
        row(fn, INVALID, NULL_ARG, **{name: None})
    row(fn, INVALID, NULL_ARG, value=None)
    row(fn, INVALID, FACT, NV=17)
    row(fn, INVALID, FACT, feat_k=48)
    row(fn, INVALID, FACT, A=1025)
    row(fn, INVALID, NULL_ARG, wv=None, NV=17)
    fn = 'azg_heads_softmax'
    SOFT = 'boards > 0, 0 < A <= 1024, 0 < NV <= 64, stride >= A + NV'
    for name in ('logits', 'policy', 'value'):
        row(fn, INVALID, NULL_ARG, **{name: None})
    row(fn, INVALID, SOFT, stride=9)
    row(fn, INVALID, SOFT, boards=0)
    row(fn, INVALID, NULL_ARG, logits=None, stride=9)
    fn = 'azg_obs_to_nhwc8_f16'
    OBS = 'null or out-of-range argument (channels <= 8)'
    row(fn, INVALID, OBS, channels=9)
    row(fn, INVALID, OBS, channels=0)
    row(fn, INVALID, OBS, obs=None)
    row(fn, INVALID, OBS, x=None, channels=9)
    return out


ROWS = rows()


@pytest.fixture(scope='module')
def L():
    from alphazero_general_amd import build, _abi
    build.build()
    return _abi.lib()


def test_the_table_covers_every_entry_point():
    assert {fn for fn, _, _, _ in ROWS} == set(GOOD)
    assert sum(1 for _, bad, _, _ in ROWS if len(bad) > 1) >= 20             # the rows that pin the order of the checks


def test_good_arguments_match_the_declared_signatures():
    from alphazero_general_amd import _abi
    for fn, args in GOOD.items():
        assert len(args) == len(_abi.SYMBOLS[fn][1]), fn


@pytest.mark.parametrize('fn', sorted(GOOD))
def test_bad_arguments_are_refused_by_code_and_text(L, fn):
    mine = [r for r in ROWS if r[0] == fn]
    assert mine
    for _, bad, rc, text in mine:
        args = dict(GOOD[fn], **bad)
        got = getattr(L, fn)(*args.values())
        assert (got, L.azg_last_error().decode()) == (rc, text), (fn, sorted(bad))


def test_codes_are_the_headers():
    from alphazero_general_amd import _abi
    assert (INVALID, UNSUPPORTED) == (_abi.E_INVALID_ARG, _abi.E_UNSUPPORTED)
