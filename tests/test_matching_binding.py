"""The header's fslr_pair_matching / fslr_pair_matching_any / fslr_pair_matching_timings declarations against
their ctypes prototypes in fslr_amd/_lib.py (no device)."""
import ctypes
import os
import re

import pytest

from fslr_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'fslr_hip.h')

pytestmark = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason='libfslr_hip.so is not built')

C_TYPES = {'fslr_ctx *': ctypes.c_void_p, 'int64_t': ctypes.c_int64, 'int32_t': ctypes.c_int32,
           'const int32_t *': ctypes.c_void_p, 'int32_t *': ctypes.c_void_p, 'uint8_t *': ctypes.c_void_p,
           'const fslr_params *': ctypes.POINTER(_lib.Params), 'float *': ctypes.POINTER(ctypes.c_float)}
# row_off is an array, n_rows a single value returned by reference
BY_NAME = {'row_off': ctypes.c_void_p, 'n_rows': ctypes.POINTER(ctypes.c_int64)}
NAMES = ['fslr_pair_matching', 'fslr_pair_matching_any', 'fslr_pair_matching_timings']


def declared(name):
    """(return type, [(argument type, argument name)]) of ``name`` as the header declares it."""
    text = open(HEADER).read()
    m = re.search(r'^(\w+)\s+' + name + r'\(([^)]*)\);', text, re.M)
    assert m, f'{name} is not declared in fslr_hip.h'
    args = []
    for a in m.group(2).split(','):
        a = re.sub(r'/\*.*?\*/', '', a).strip()
        args.append((re.sub(r'\s*\w+$', '', a).strip(), re.search(r'(\w+)$', a).group(1)))
    return m.group(1), args


@pytest.mark.parametrize('name', NAMES)
def test_prototype_matches_the_header(name):
    L = _lib.load()
    ret, args = declared(name)
    fn = getattr(L, name)
    assert ret == 'int' and fn.restype is ctypes.c_int
    want = [BY_NAME[n] if t == 'int64_t *' else C_TYPES[t] for t, n in args]
    assert want == list(fn.argtypes), (name, args)
    assert name in _lib.EXPORTED


def test_the_calls_extend_the_score_calls():
    """The matching calls take fslr_score_pairs' (fslr_score_pairs_any's) arguments, then the row outputs."""
    L = _lib.load()
    tail = [ctypes.c_void_p] * 3 + [ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
    assert list(L.fslr_pair_matching.argtypes) == list(L.fslr_score_pairs.argtypes) + tail
    assert list(L.fslr_pair_matching_any.argtypes) == list(L.fslr_score_pairs_any.argtypes) + tail
    assert list(L.fslr_pair_matching_timings.argtypes) == list(L.fslr_score_timings.argtypes)
    assert [n for _, n in declared('fslr_pair_matching')[1]][-5:] == ['row_off', 'row', 'col', 'capacity', 'n_rows']


def test_null_context_is_refused_without_a_device():
    L = _lib.load()
    n = ctypes.c_int64(-7)
    assert L.fslr_pair_matching(None, None, 0, None, None, None, None, None, None, None, None, 0,
                                ctypes.byref(n)) == _lib.FSLR_ERR_INVALID
    assert L.fslr_pair_matching_any(None, None, None, 0, 0, None, None, None, None, None, None, None, None, 0,
                                    ctypes.byref(n)) == _lib.FSLR_ERR_INVALID
    assert L.fslr_pair_matching_timings(None, None) == _lib.FSLR_ERR_INVALID
    assert n.value == -7


def test_abi_version_is_unchanged():
    m = re.search(r'^#define\s+FSLR_ABI_VERSION\s+(\d+)', open(HEADER).read(), re.M)
    assert int(m.group(1)) == _lib.ABI_VERSION == 21 == _lib.load().fslr_abi_version()
