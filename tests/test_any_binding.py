"""The header's fslr_append_reads_any / fslr_remove_reads_any declarations against their ctypes prototypes in
fslr_amd/_lib.py (no device)."""
import ctypes
import os
import re

import pytest

from fslr_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'fslr_hip.h')

pytestmark = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason='libfslr_hip.so is not built')

C_TYPES = {'fslr_ctx *': ctypes.c_void_p, 'int64_t': ctypes.c_int64, 'const uint8_t *': ctypes.c_void_p,
           'int32_t *': ctypes.c_void_p, 'const fslr_reads *': ctypes.POINTER(_lib.Reads)}


def declared(name):
    """(return type, argument types) of ``name`` as the header declares it."""
    text = open(HEADER).read()
    m = re.search(r'^(\w+)\s+' + name + r'\(([^)]*)\);', text, re.M)
    assert m, f'{name} is not declared in fslr_hip.h'
    args = [re.sub(r'\s*\w+$', '', re.sub(r'/\*.*?\*/', '', a).strip()).strip() for a in m.group(2).split(',')]
    return m.group(1), args


@pytest.mark.parametrize('name', ['fslr_append_reads_any', 'fslr_remove_reads_any'])
def test_prototype_matches_the_header(name):
    L = _lib.load()
    ret, args = declared(name)
    fn = getattr(L, name)
    assert ret == 'int' and fn.restype is ctypes.c_int
    assert [C_TYPES[a] for a in args] == list(fn.argtypes), (name, args)
    assert name in _lib.EXPORTED


def test_the_any_calls_take_what_the_short_calls_take():
    L = _lib.load()
    assert list(L.fslr_append_reads_any.argtypes) == list(L.fslr_append_reads.argtypes)
    assert list(L.fslr_remove_reads_any.argtypes) == list(L.fslr_remove_reads.argtypes)


def test_length_limit_matches_the_header():
    m = re.search(r'^#define\s+FSLR_MAX_ANY_L\s+(\d+)', open(HEADER).read(), re.M)
    assert m and int(m.group(1)) == 4096


def test_abi_version_is_unchanged():
    m = re.search(r'^#define\s+FSLR_ABI_VERSION\s+(\d+)', open(HEADER).read(), re.M)
    assert int(m.group(1)) == _lib.ABI_VERSION == 21 == _lib.load().fslr_abi_version()
