"""The header's fslr_cluster_paths / fslr_get_cluster_paths / fslr_cluster_paths_timings declarations against their
ctypes prototypes in fslr_amd/_lib.py (no device)."""
import ctypes
import os
import re

import numpy as np
import pytest

from fslr_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'fslr_hip.h')

pytestmark = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason='libfslr_hip.so is not built')

C_TYPES = {'fslr_ctx *': ctypes.c_void_p, 'int64_t': ctypes.c_int64, 'int32_t *': ctypes.c_void_p,
           'const int32_t *': ctypes.c_void_p, 'const uint8_t *': ctypes.c_void_p, 'uint8_t *': ctypes.c_void_p,
           'float *': ctypes.POINTER(ctypes.c_float)}
# off and tok_off are arrays, n_rows and n_tokens single values returned by reference
BY_NAME = {'off': ctypes.c_void_p, 'tok_off': ctypes.c_void_p, 'n_rows': ctypes.POINTER(ctypes.c_int64),
           'n_tokens': ctypes.POINTER(ctypes.c_int64)}
NAMES = ['fslr_cluster_paths', 'fslr_get_cluster_paths', 'fslr_cluster_paths_timings']


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
    want = [BY_NAME[n] if t == 'int64_t *' else C_TYPES[t] for t, n in args]
    assert want == list(fn.argtypes), (name, args)
    assert name in _lib.EXPORTED


def test_the_argument_names():
    assert [n for _, n in declared('fslr_cluster_paths')[1]] == ['ctx', 'iv_qkey', 'iv_rev', 'n_intervals', 'n_rows',
                                                                 'n_tokens']
    assert [n for _, n in declared('fslr_get_cluster_paths')[1]] == [
        'ctx', 'off', 'tok_off', 'n_reads', 'first_read', 'locus', 'rev', 'path_of_read', 'flipped', 'row_capacity',
        'token_capacity']
    assert [n for _, n in declared('fslr_cluster_paths_timings')[1]] == ['ctx', 'ms']


def test_null_context_is_refused_without_a_device():
    L = _lib.load()
    nr, nt = ctypes.c_int64(-7), ctypes.c_int64(-7)
    key = np.zeros(4, np.int32)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.fslr_cluster_paths(None, ptr(key), None, 4, ctypes.byref(nr), ctypes.byref(nt)) == _lib.FSLR_ERR_INVALID
    assert nr.value == -7 and nt.value == -7
    wide = [np.full(4, -7, np.int64) for _ in range(2)]
    ints = [np.full(4, -7, np.int32) for _ in range(4)]
    bytes_ = [np.full(4, 249, np.uint8) for _ in range(2)]
    assert L.fslr_get_cluster_paths(None, ptr(wide[0]), ptr(wide[1]), ptr(ints[0]), ptr(ints[1]), ptr(ints[2]),
                                    ptr(bytes_[0]), ptr(ints[3]), ptr(bytes_[1]), 4, 4) == _lib.FSLR_ERR_INVALID
    assert all((a == -7).all() for a in wide + ints) and all((a == 249).all() for a in bytes_)
    ms = (ctypes.c_float * 1)(-7.0)
    assert L.fslr_cluster_paths_timings(None, ms) == _lib.FSLR_ERR_INVALID
    assert ms[0] == -7.0


def test_abi_version_is_unchanged():
    m = re.search(r'^#define\s+FSLR_ABI_VERSION\s+(\d+)', open(HEADER).read(), re.M)
    assert int(m.group(1)) == _lib.ABI_VERSION == 21 == _lib.load().fslr_abi_version()


def test_cli_refuses_cluster_paths_on_several_gpus(tmp_path):
    """A usage error before any work: nothing is read, created or started."""
    from click.testing import CliRunner
    from fslr_amd.main import pipeline
    out = tmp_path / 'out'
    res = CliRunner().invoke(pipeline, ['--name', 'x', '--out', str(out), '--ref', 'unused.fa', '--primers', '21q1',
                                        '--skip-alignment', '--cluster-paths', '--gpus', '2'])
    assert res.exit_code == 2 and '--gpus 1' in res.output and '--cluster-paths' in res.output
    assert not out.exists()


def test_the_frames_of_a_result():
    """ClusterPaths on hand-made arrays: two clusters, rows (0:+), (0:+, 1:-) | (2:+, 2:+); a read alone."""
    from fslr_amd import cluster
    loci = cluster.ClusterLoci(np.asarray([0, 2, 3]), np.asarray(['chr4', 'chr21', 'chr4'], dtype=object),
                               np.asarray([100, 1000, 7000]), np.asarray([200, 1100, 7100]), np.asarray([2, 1, 4]),
                               np.asarray([2, 1, 2]), np.asarray([0, 1, 0]))
    p = cluster.ClusterPaths(np.asarray([0, 2, 3], np.int64), np.asarray([0, 1, 3, 5], np.int64),
                             np.asarray([1, 2, 2], np.int32), np.asarray([1, 0, 3], np.int32),
                             np.asarray([0, 0, 1, 2, 2], np.int32), np.asarray([0, 0, 1, 0, 0], np.uint8),
                             np.asarray([1, 0, 1, 2, -1, 2], np.int32), np.asarray([0, 0, 1, 0, 0, 1], np.uint8), loci,
                             np.asarray(['a', 'b', 'c', 'd', 'e', 'f'], dtype=object))
    assert len(p) == 3 and p.cluster_of_row().tolist() == [0, 0, 1]
    assert [x.tolist() for x in p.tokens(1)] == [[0, 1], [0, 1]]
    f = p.to_frame()
    assert list(f.columns) == ['cluster', 'path', 'n_reads', 'n_loci', 'first_read', 'structure']
    assert f.values.tolist() == [[0, 0, 1, 1, 'b', 'chr4:100-200:+'],
                                 [0, 1, 2, 2, 'a', 'chr4:100-200:+,chr21:1000-1100:-'],
                                 [1, 0, 2, 2, 'd', 'chr4:7000-7100:+,chr4:7000-7100:+']]
    r = p.read_frame()
    assert list(r.columns) == ['qname', 'cluster', 'path', 'flipped']
    assert r.values.tolist() == [['a', 0, 1, 0], ['b', 0, 0, 0], ['c', 0, 1, 1], ['d', 1, 0, 0], ['e', -1, -1, 0],
                                 ['f', 1, 0, 1]]
    assert p.dominant().tolist() == [1, 2]
    p.n_reads = np.asarray([2, 2, 2], np.int32)
    assert p.dominant().tolist() == [0, 2]                 # a tie goes to the first row
