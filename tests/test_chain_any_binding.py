"""The header's fslr_cluster_junctions_any / fslr_cluster_paths_any declarations against their ctypes prototypes in
fslr_amd/_lib.py, the wrappers' argument checks and the refusals that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest

import search_ref as sr
from fslr_amd import _lib, cluster

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'fslr_hip.h')

pytestmark = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason='libfslr_hip.so is not built')

C_TYPES = {'fslr_ctx *': ctypes.c_void_p, 'int64_t': ctypes.c_int64, 'const int32_t *': ctypes.c_void_p,
           'const uint8_t *': ctypes.c_void_p, 'int64_t *': ctypes.POINTER(ctypes.c_int64)}
NAMES = {'fslr_cluster_junctions_any': 'fslr_cluster_junctions', 'fslr_cluster_paths_any': 'fslr_cluster_paths'}


def declared(name):
    """(return type, [(argument type, argument name)]) of ``name`` as the header declares it."""
    text = open(HEADER).read()
    m = re.search(r'^(\w+)\s+' + name + r'\(([^)]*)\);', text, re.M)
    assert m, f'{name} is not declared in fslr_hip.h'
    args = []
    for a in re.sub(r'/\*.*?\*/', '', m.group(2)).split(','):
        a = a.strip()
        args.append((re.sub(r'\s*\w+$', '', a).strip(), re.search(r'(\w+)$', a).group(1)))
    return m.group(1), args


@pytest.mark.parametrize('name', sorted(NAMES))
def test_prototype_matches_the_header_and_the_plain_call(name):
    L = _lib.load()
    ret, args = declared(name)
    fn = getattr(L, name)
    assert ret == 'int' and fn.restype is ctypes.c_int
    assert [C_TYPES[t] for t, _ in args] == list(fn.argtypes), (name, args)
    assert name in _lib.EXPORTED
    assert (ret, args) == declared(NAMES[name])                   # the plain call's arguments, names included
    assert list(fn.argtypes) == list(getattr(L, NAMES[name]).argtypes)


def test_abi_version_is_unchanged():
    m = re.search(r'^#define\s+FSLR_ABI_VERSION\s+(\d+)', open(HEADER).read(), re.M)
    assert int(m.group(1)) == _lib.ABI_VERSION == 21 == _lib.load().fslr_abi_version()


def test_null_context_is_refused_without_a_device():
    L = _lib.load()
    nr, nt = ctypes.c_int64(-7), ctypes.c_int64(-7)
    key = np.zeros(4, np.int32)
    ptr = key.ctypes.data_as(ctypes.c_void_p)
    assert L.fslr_cluster_junctions_any(None, ptr, None, 4, ctypes.byref(nr)) == _lib.FSLR_ERR_INVALID
    assert L.fslr_cluster_paths_any(None, ptr, None, 4, ctypes.byref(nr), ctypes.byref(nt)) == _lib.FSLR_ERR_INVALID
    assert nr.value == -7 and nt.value == -7


class Recorder:
    """Stands for the loaded library: the two calls record their arguments and refuse."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return _lib.FSLR_ERR_STATE
        return call


def bare_context():
    c = object.__new__(_lib.Context)
    c._L, c._h, c.n_reads = Recorder(), None, 0
    c._check = lambda rc: (_ for _ in ()).throw(RuntimeError(f'rc {rc}')) if rc else None
    return c


@pytest.mark.parametrize('method', ['cluster_junctions_any', 'cluster_paths_any'])
def test_wrapper_argument_checks(method):
    c = bare_context()
    call = getattr(c, method)
    with pytest.raises(ValueError, match='one-dimensional'):
        call(np.zeros((2, 2), np.int32))
    with pytest.raises(ValueError, match='integers'):
        call(np.zeros(4, np.float64))
    with pytest.raises(ValueError, match='int32'):
        call(np.asarray([0, 1 << 31], np.int64))
    with pytest.raises(ValueError, match='int32'):
        call(np.asarray([-(1 << 31) - 1, 0], np.int64))
    with pytest.raises(ValueError, match='shape'):
        call(np.zeros(4, np.int32), np.zeros(3, np.uint8))
    assert c._L.calls == []                                       # nothing reached the library
    # the extremes of int32 pass, as int32, with the count and the strand bits as uint8
    with pytest.raises(RuntimeError, match=f'rc {_lib.FSLR_ERR_STATE}'):
        call(np.asarray([-(1 << 31), (1 << 31) - 1, 0], np.int64), [1, 0, 1])
    (name, args), = c._L.calls
    assert name == 'fslr_' + method and args[3] == 3


def test_multi_gpu_index_refuses():
    mg = cluster.MultiGpuIndex(sr.make_data([1, 1], [0, 5], [9, 9]), 2)
    with pytest.raises(NotImplementedError, match='n_gpus=1'):
        mg.cluster_junctions_any([0, 1])
    with pytest.raises(NotImplementedError, match='n_gpus=1'):
        mg.cluster_paths_any([0, 1])


def test_cli_declares_the_flag():
    from fslr_amd.main import pipeline
    opts = {o for p in pipeline.params for o in p.opts}
    assert '--cluster-long-reads' in opts
