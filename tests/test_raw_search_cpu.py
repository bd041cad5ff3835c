"""CPU-side checks of the network-free search launch (azg_search_raw): it is declared, bound and exported; without a device it
fails on its arguments; and which form a warm-up SelfPlayRunner takes -- the launch or the launch-per-phase loop -- follows one
table (utils.RAW_LAUNCH), checked here with a stubbed engine."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def built():
    from alphazero_general_amd import build
    return build.build()


def test_search_raw_declared_bound_and_exported(built):
    from alphazero_general_amd import _abi
    txt = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'azg.h')).read(), flags=re.S)
    m = re.search(r'int\s+azg_search_raw\s*\(([^)]*)\)', txt)
    assert m and [a.strip() for a in m.group(1).split(',')] == ['azg_engine *e', 'void *stream', 'float policy_fill', 'const float *value_host', 'int sims']
    assert re.search(r'#define\s+AZG_ABI_VERSION\s+7\b', txt)                  # one added function: the ABI version stands
    res, args = _abi.SYMBOLS['azg_search_raw']
    assert res is C.c_int and args == [C.c_void_p, C.c_void_p, C.c_float, C.POINTER(C.c_float), C.c_int]
    assert hasattr(C.CDLL(built), 'azg_search_raw')


def test_search_raw_rejects_a_null_engine_without_a_device(built):
    from alphazero_general_amd import _abi
    L = _abi.lib()
    z = np.zeros(3, np.float32).ctypes.data_as(C.POINTER(C.c_float))
    assert L.azg_search_raw(None, None, 1.0, z, 5) == _abi.E_INVALID_ARG
    assert L.azg_search_raw(None, None, 1.0, z, 0) == _abi.E_INVALID_ARG       # (the null engine comes before sims == 0)
    assert b'null' in L.azg_last_error()


class _StubEngine:
    A, NV = 7, 3

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def rec(*a, **k):
            self.calls.append((name,) + tuple(x if isinstance(x, (int, float, bool)) else 'row' for x in a))
        return rec


def _stub_runner(fused_search):
    """a warm-up SelfPlayRunner around a stubbed engine (no device): only what _issue_round reads"""
    from alphazero_general_amd.selfplay import SelfPlayRunner, _Lane
    r = object.__new__(SelfPlayRunner)
    r.warmup, r.heads, r.nnet = True, None, None
    r.fused_search = SelfPlayRunner.warmup_raw_round(fused_search)
    e = _StubEngine()
    r._raw_fill, r._raw_value = float(np.float32(1 / e.A)), np.full(e.NV, 1 / e.NV, np.float32)
    ln = _Lane(e, None)
    ln.policy, ln.value = 'P', 'V'
    return r, ln, e


def test_warmup_round_form_follows_the_adoption_table():
    from alphazero_general_amd import utils
    from alphazero_general_amd.selfplay import SelfPlayRunner
    # one table holds the defaults and the sizes the adoption rule was measured at
    assert set(utils.RAW_LAUNCH) == {'raw_search', 'warmup'}
    assert utils.RAW_LAUNCH['warmup']['sizes'] == [(g, b) for g in ('connect4', 'brandubh') for b in (128, 512, 2048)]
    assert utils.RAW_LAUNCH['raw_search']['sizes'] == [('connect4', 1), ('brandubh', 1)]
    for caller in utils.RAW_LAUNCH:
        assert utils.raw_launch_default(caller) is bool(utils.RAW_LAUNCH[caller]['default'])
    assert SelfPlayRunner.warmup_raw_round(True) is True and SelfPlayRunner.warmup_raw_round(False) is False
    assert SelfPlayRunner.warmup_raw_round(None) is utils.raw_launch_default('warmup')
    # the default follows the table, whichever way it stands
    saved = utils.RAW_LAUNCH['warmup']['default']
    try:
        for d in (True, False):
            utils.RAW_LAUNCH['warmup']['default'] = d
            assert SelfPlayRunner.warmup_raw_round(None) is d
    finally:
        utils.RAW_LAUNCH['warmup']['default'] = saved


def test_warmup_round_launch_sequences():
    # fused_search=True: ONE launch with the warm-up constants, then advance
    r, ln, e = _stub_runner(True)
    r._issue_round(ln, 5, False)
    assert e.calls == [('search_raw', 5, float(np.float32(1 / 7)), 'row'), ('advance',)]
    # fused_search=False: the launch-per-phase loop, backup k and select k + 1 sharing a launch
    r, ln, e = _stub_runner(False)
    r._issue_round(ln, 3, True)
    assert [c[0] for c in e.calls] == ['select', 'backup_select', 'backup_select', 'backup', 'advance']
