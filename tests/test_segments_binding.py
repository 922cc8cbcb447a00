"""The header's fslr_cluster_path_segments / fslr_get_cluster_path_segments / fslr_cluster_path_segments_timings
declarations against their ctypes prototypes in fslr_amd/_lib.py, the wrappers' refusals and the result class (no
device)."""
import ctypes
import os
import re

import numpy as np
import pytest

import search_ref as sr
from fslr_amd import _lib, cluster

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'fslr_hip.h')

pytestmark = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason='libfslr_hip.so is not built')

C_TYPES = {'fslr_ctx *': ctypes.c_void_p, 'int64_t': ctypes.c_int64, 'int32_t *': ctypes.c_void_p,
           'const int32_t *': ctypes.c_void_p, 'float *': ctypes.POINTER(ctypes.c_float),
           'int64_t *': ctypes.POINTER(ctypes.c_int64)}             # n_tokens: a single value returned by reference
NAMES = ['fslr_cluster_path_segments', 'fslr_get_cluster_path_segments', 'fslr_cluster_path_segments_timings']


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


@pytest.mark.parametrize('name', NAMES)
def test_prototype_matches_the_header(name):
    L = _lib.load()
    ret, args = declared(name)
    fn = getattr(L, name)
    assert ret == 'int' and fn.restype is ctypes.c_int
    assert [C_TYPES[t] for t, _ in args] == list(fn.argtypes), (name, args)
    assert name in _lib.EXPORTED


def test_the_argument_names():
    assert [n for _, n in declared(NAMES[0])[1]] == ['ctx', 'iv_qkey', 'iv_qend', 'n_intervals', 'n_tokens']
    assert [n for _, n in declared(NAMES[1])[1]] == ['ctx', 'start', 'end', 'gap', 'token_capacity']
    assert [n for _, n in declared(NAMES[2])[1]] == ['ctx', 'ms']


def test_null_context_is_refused_without_a_device():
    L = _lib.load()
    nt = ctypes.c_int64(-7)
    key = np.zeros(4, np.int32)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.fslr_cluster_path_segments(None, ptr(key), ptr(key), 4, ctypes.byref(nt)) == _lib.FSLR_ERR_INVALID
    assert nt.value == -7
    outs = [np.full(12, -7, np.int32) for _ in range(3)]
    assert L.fslr_get_cluster_path_segments(None, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), 4) == _lib.FSLR_ERR_INVALID
    assert all((a == -7).all() for a in outs)
    ms = (ctypes.c_float * 1)(-7.0)
    assert L.fslr_cluster_path_segments_timings(None, ms) == _lib.FSLR_ERR_INVALID
    assert ms[0] == -7.0


def test_abi_version_is_unchanged():
    m = re.search(r'^#define\s+FSLR_ABI_VERSION\s+(\d+)', open(HEADER).read(), re.M)
    assert int(m.group(1)) == _lib.ABI_VERSION == 21 == _lib.load().fslr_abi_version()


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
        c.cluster_path_segments(np.zeros((2, 2), np.int32))
    with pytest.raises(ValueError, match='shape'):
        c.cluster_path_segments(np.zeros(4, np.int32), np.zeros(3, np.int32))
    assert c._L.calls == []                                       # nothing reached the library
    with pytest.raises(RuntimeError, match=f'rc {_lib.FSLR_ERR_STATE}'):
        c.cluster_path_segments(np.asarray([3, 1, 2], np.int64))
    (name, args), = c._L.calls
    assert name == 'fslr_cluster_path_segments' and args[2] is None and args[3] == 3


def test_multi_gpu_and_long_read_indexes_refuse():
    mg = cluster.MultiGpuIndex(sr.make_data([1, 1], [0, 5], [9, 9]), 2)
    with pytest.raises(NotImplementedError, match='n_gpus=1'):
        mg.cluster_path_segments([0, 1])
    idx = object.__new__(cluster.DeviceIntervalIndex)             # an index that holds reads of more than 64 intervals
    idx.long = np.asarray([65, 1], np.int32)
    with pytest.raises(NotImplementedError, match='more than 64'):
        idx.cluster_path_segments([0, 1])


def test_cli_refuses_cluster_path_segments_on_several_gpus(tmp_path):
    """A usage error before any work: nothing is read, created or started."""
    from click.testing import CliRunner
    from fslr_amd.main import pipeline
    out = tmp_path / 'out'
    res = CliRunner().invoke(pipeline, ['--name', 'x', '--out', str(out), '--ref', 'unused.fa', '--primers', '21q1',
                                        '--skip-alignment', '--cluster-path-segments', '--gpus', '2'])
    assert res.exit_code == 2 and '--gpus 1' in res.output and '--cluster-path-segments' in res.output
    assert not out.exists()


def test_the_frame_and_the_structure_of_a_result():
    """ClusterPathSegments on hand-made arrays: two clusters, rows (0:+), (0:+, 1:-) | (2:+, 2:+)."""
    loci = cluster.ClusterLoci(np.asarray([0, 2, 3]), np.asarray(['chr4', 'chr21', 'chr4'], dtype=object),
                               np.asarray([100, 1000, 7000]), np.asarray([200, 1100, 7100]), np.asarray([2, 1, 4]),
                               np.asarray([2, 1, 2]), np.asarray([0, 1, 0]))
    p = cluster.ClusterPaths(np.asarray([0, 2, 3], np.int64), np.asarray([0, 1, 3, 5], np.int64),
                             np.asarray([1, 2, 2], np.int32), np.asarray([1, 0, 3], np.int32),
                             np.asarray([0, 0, 1, 2, 2], np.int32), np.asarray([0, 0, 1, 0, 0], np.uint8),
                             np.asarray([1, 0, 1, 2, -1, 2], np.int32), np.asarray([0, 0, 1, 0, 0, 1], np.uint8), loci,
                             np.asarray(['a', 'b', 'c', 'd', 'e', 'f'], dtype=object))
    i32 = lambda *v: np.asarray(v, np.int32)
    s = cluster.ClusterPathSegments(p, i32(120, 100, 1000, 7000, 7050), i32(120, 105, 1010, 7001, 7051), i32(120, 110, 1020, 7002, 7052),
                                    i32(180, 190, 1090, 7040, 7090), i32(180, 195, 1095, 7041, 7091), i32(180, 200, 1100, 7042, 7092),
                                    i32(0, -3, 0, 4, 0), i32(0, -1, 0, 5, 0), i32(0, 2, 0, 6, 0))
    assert len(s) == 5 and s.paths is p and [c.tolist() for c in s.columns()][1] == [120, 105, 1010, 7001, 7051]
    f = s.to_frame()
    assert list(f.columns) == ['cluster', 'path', 'piece', 'chrom', 'start', 'end', 'strand', 'n_reads', 'start_min',
                               'start_max', 'end_min', 'end_max', 'gap_min', 'gap', 'gap_max']
    assert f.values.tolist() == [[0, 0, 0, 'chr4', 120, 180, '+', 1, 120, 120, 180, 180, 0, 0, 0],
                                 [0, 1, 0, 'chr4', 105, 195, '+', 2, 100, 110, 190, 200, -3, -1, 2],
                                 [0, 1, 1, 'chr21', 1010, 1095, '-', 2, 1000, 1020, 1090, 1100, 0, 0, 0],
                                 [1, 0, 0, 'chr4', 7001, 7041, '+', 2, 7000, 7002, 7040, 7042, 4, 5, 6],
                                 [1, 0, 1, 'chr4', 7051, 7091, '+', 2, 7050, 7052, 7090, 7092, 0, 0, 0]]
    assert s.structure(0) == 'chr4:120-180:+' and s.structure(1) == 'chr4:105-195:+,chr21:1010-1095:-'
    assert s.structure(2) == 'chr4:7001-7041:+,chr4:7051-7091:+'
