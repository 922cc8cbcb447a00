"""The header's fslr_cluster_path_segments_any declaration against its ctypes prototype in fslr_amd/_lib.py and against
the plain call's, the wrappers' argument checks and the refusals that need no device."""
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
           'int64_t *': ctypes.POINTER(ctypes.c_int64)}
ANY, PLAIN = 'fslr_cluster_path_segments_any', 'fslr_cluster_path_segments'


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


def test_prototype_matches_the_header_and_the_plain_call():
    L = _lib.load()
    ret, args = declared(ANY)
    fn = getattr(L, ANY)
    assert ret == 'int' and fn.restype is ctypes.c_int
    assert [C_TYPES[t] for t, _ in args] == list(fn.argtypes), args
    assert ANY in _lib.EXPORTED
    assert (ret, args) == declared(PLAIN)                         # the plain call's arguments, names included
    assert [n for _, n in args] == ['ctx', 'iv_qkey', 'iv_qend', 'n_intervals', 'n_tokens']
    assert list(fn.argtypes) == list(getattr(L, PLAIN).argtypes)


def test_abi_version_is_unchanged():
    m = re.search(r'^#define\s+FSLR_ABI_VERSION\s+(\d+)', open(HEADER).read(), re.M)
    assert int(m.group(1)) == _lib.ABI_VERSION == 21 == _lib.load().fslr_abi_version()


def test_null_context_is_refused_without_a_device():
    L = _lib.load()
    nt = ctypes.c_int64(-7)
    key = np.zeros(4, np.int32)
    ptr = key.ctypes.data_as(ctypes.c_void_p)
    assert L.fslr_cluster_path_segments_any(None, ptr, ptr, 4, ctypes.byref(nt)) == _lib.FSLR_ERR_INVALID
    assert nt.value == -7


class Recorder:
    """Stands for the loaded library: every call records its arguments and refuses."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return _lib.FSLR_ERR_STATE
        return call


def test_context_wrapper_argument_checks():
    c = object.__new__(_lib.Context)
    c._L, c._h, c.n_reads = Recorder(), None, 0
    c._check = lambda rc: (_ for _ in ()).throw(RuntimeError(f'rc {rc}')) if rc else None
    with pytest.raises(ValueError, match='one-dimensional'):
        c.cluster_path_segments_any(np.zeros((2, 2), np.int32))
    with pytest.raises(ValueError, match='shape'):
        c.cluster_path_segments_any(np.zeros(4, np.int32), np.zeros(3, np.int32))
    assert c._L.calls == []                                       # nothing reached the library
    with pytest.raises(RuntimeError, match=f'rc {_lib.FSLR_ERR_STATE}'):
        c.cluster_path_segments_any(np.asarray([3, 1, 2], np.int64))
    (name, args), = c._L.calls
    assert name == ANY and args[2] is None and args[3] == 3
    # with the query ends: both columns go down, the plain wrapper's call is not used
    with pytest.raises(RuntimeError, match=f'rc {_lib.FSLR_ERR_STATE}'):
        c.cluster_path_segments_any([3, 1], [4, 2])
    assert [n for n, _ in c._L.calls] == [ANY, ANY] and c._L.calls[1][1][2] is not None and c._L.calls[1][1][3] == 2


def test_multi_gpu_index_refuses_and_a_long_read_index_is_taken():
    mg = cluster.MultiGpuIndex(sr.make_data([1, 1], [0, 5], [9, 9]), 2)
    with pytest.raises(NotImplementedError, match='n_gpus=1'):
        mg.cluster_path_segments_any([0, 1])
    # an index that holds reads of more than 64 intervals: the plain wrapper refuses by its length, the _any wrapper
    # goes on to its arguments (this bare index has no CSR to check them against)
    idx = object.__new__(cluster.DeviceIntervalIndex)
    idx.long = np.asarray([65, 1], np.int32)
    with pytest.raises(NotImplementedError, match='more than 64'):
        idx.cluster_path_segments([0, 1])
    with pytest.raises(AttributeError):
        idx.cluster_path_segments_any([0, 1])


def test_cli_declares_the_flag_and_refuses_several_gpus(tmp_path):
    """A usage error before any work: nothing is read, created or started."""
    from click.testing import CliRunner
    from fslr_amd.main import pipeline
    opts = {o for p in pipeline.params for o in p.opts}
    assert '--cluster-path-segments-any' in opts and '--cluster-path-segments' in opts and '--cluster-long-reads' in opts
    out = tmp_path / 'out'
    res = CliRunner().invoke(pipeline, ['--name', 'x', '--out', str(out), '--ref', 'unused.fa', '--primers', '21q1',
                                        '--skip-alignment', '--cluster-path-segments-any', '--gpus', '2'])
    assert res.exit_code == 2 and '--gpus 1' in res.output and '--cluster-path-segments-any' in res.output
    assert not out.exists()
