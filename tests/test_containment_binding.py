"""The header's fslr_cluster_path_containment / fslr_get_cluster_path_containment /
fslr_cluster_path_containment_timings declarations against their ctypes prototypes in fslr_amd/_lib.py, the
wrappers' refusals and the result class (no device)."""
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
           'uint8_t *': ctypes.c_void_p, 'float *': ctypes.POINTER(ctypes.c_float), 'int64_t *': ctypes.c_void_p}
NAMES = ['fslr_cluster_path_containment', 'fslr_get_cluster_path_containment', 'fslr_cluster_path_containment_timings']


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
    want = [C_TYPES[t] for t, _ in args]
    if name == NAMES[0]:
        want[1] = ctypes.POINTER(ctypes.c_int64)                  # n_pairs: a single value returned by reference
    assert want == list(fn.argtypes), (name, args)
    assert name in _lib.EXPORTED


def test_the_argument_names():
    assert [n for _, n in declared(NAMES[0])[1]] == ['ctx', 'n_pairs']
    assert [n for _, n in declared(NAMES[1])[1]] == ['ctx', 'coff', 'outer', 'offset', 'rev', 'n_occ', 'n_inner', 'support',
                                                     'collapse_to', 'collapsed_reads', 'row_capacity', 'pair_capacity']
    assert [n for _, n in declared(NAMES[2])[1]] == ['ctx', 'ms']


def test_null_context_is_refused_without_a_device():
    L = _lib.load()
    n = ctypes.c_int64(-7)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.fslr_cluster_path_containment(None, ctypes.byref(n)) == _lib.FSLR_ERR_INVALID
    assert n.value == -7
    outs = [np.full(8, -7, np.int64) for _ in range(9)]
    assert L.fslr_get_cluster_path_containment(None, *[ptr(a) for a in outs], 4, 4) == _lib.FSLR_ERR_INVALID
    assert all((a == -7).all() for a in outs)
    ms = (ctypes.c_float * 1)(-7.0)
    assert L.fslr_cluster_path_containment_timings(None, ms) == _lib.FSLR_ERR_INVALID
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


def test_context_wrapper_stops_at_the_library_s_refusal():
    c = object.__new__(_lib.Context)
    c._L, c._h, c.n_reads = Recorder(), None, 0
    c._check = lambda rc: (_ for _ in ()).throw(RuntimeError(f'rc {rc}')) if rc else None
    with pytest.raises(RuntimeError, match=f'rc {_lib.FSLR_ERR_STATE}'):
        c.cluster_path_containment()
    (name, args), = c._L.calls                                    # the getter was not reached
    assert name == 'fslr_cluster_path_containment' and len(args) == 2
    with pytest.raises(RuntimeError, match=f'rc {_lib.FSLR_ERR_STATE}'):
        c.cluster_path_containment_timings()


def test_multi_gpu_index_refuses():
    mg = cluster.MultiGpuIndex(sr.make_data([1, 1], [0, 5], [9, 9]), 2)
    with pytest.raises(NotImplementedError, match='n_gpus=1'):
        mg.cluster_path_containment([0, 1])


def test_cli_refuses_cluster_path_containment_on_several_gpus(tmp_path):
    """A usage error before any work: nothing is read, created or started."""
    from click.testing import CliRunner
    from fslr_amd.main import pipeline
    out = tmp_path / 'out'
    res = CliRunner().invoke(pipeline, ['--name', 'x', '--out', str(out), '--ref', 'unused.fa', '--primers', '21q1',
                                        '--skip-alignment', '--cluster-path-containment', '--gpus', '2'])
    assert res.exit_code == 2 and '--gpus 1' in res.output and '--cluster-path-containment' in res.output
    assert not out.exists()


def test_the_frames_of_a_result():
    """ClusterPathContainment on hand-made arrays: two clusters, rows (0:+), (0:+, 1:-) | (2:+, 2:+); row 0 lies in
    row 1 at offset 0."""
    loci = cluster.ClusterLoci(np.asarray([0, 2, 3]), np.asarray(['chr4', 'chr21', 'chr4'], dtype=object),
                               np.asarray([100, 1000, 7000]), np.asarray([200, 1100, 7100]), np.asarray([2, 1, 4]),
                               np.asarray([2, 1, 2]), np.asarray([0, 1, 0]))
    p = cluster.ClusterPaths(np.asarray([0, 2, 3], np.int64), np.asarray([0, 1, 3, 5], np.int64),
                             np.asarray([1, 2, 2], np.int32), np.asarray([1, 0, 3], np.int32),
                             np.asarray([0, 0, 1, 2, 2], np.int32), np.asarray([0, 0, 1, 0, 0], np.uint8),
                             np.asarray([1, 0, 1, 2, -1, 2], np.int32), np.asarray([0, 0, 1, 0, 0, 1], np.uint8), loci,
                             np.asarray(['a', 'b', 'c', 'd', 'e', 'f'], dtype=object))
    i32 = lambda *v: np.asarray(v, np.int32)
    i64 = lambda *v: np.asarray(v, np.int64)
    s = cluster.ClusterPathContainment(p, i64(0, 1, 1, 1), i32(1), i32(0), np.asarray([0], np.uint8), i32(1),
                                       i32(0, 1, 0), i64(1, 3, 2), i32(1, 1, 2), i64(0, 3, 2))
    assert len(s) == 1 and s.paths is p and s.maximal().tolist() == [False, True, True]
    f = s.to_frame()
    assert list(f.columns) == ['cluster', 'inner', 'outer', 'offset', 'rev', 'n_occ']
    assert f.values.tolist() == [[0, 0, 1, 0, 0, 1]]
    g = s.paths_frame()
    assert list(g.columns) == ['cluster', 'row', 'n_tokens', 'n_reads', 'n_inner', 'support', 'maximal', 'collapse_to',
                               'collapsed_reads']
    assert g.values.tolist() == [[0, 0, 1, 1, 0, 1, False, 1, 0], [0, 1, 2, 2, 1, 3, True, 1, 3], [1, 2, 2, 2, 0, 2, True, 2, 2]]


def test_the_writer_s_last_column_on_hand_made_pairs(tmp_path, monkeypatch):
    """main.write_cluster_path_containment on a hand-made result: row 0 lies in row 1 forward at offset 0 and in row 3
    reverse complemented at offset 2, row 2 lies in row 3 forward at offset 1 (twice); rows 1 and 3 are maximal."""
    from fslr_amd import main
    loci = cluster.ClusterLoci(np.asarray([0, 3]), np.asarray([4, 4, 21], dtype=object), np.asarray([100, 1000, 7000]),
                               np.asarray([200, 1100, 7100]), np.asarray([4, 5, 4]), np.asarray([4, 4, 3]), np.asarray([0, 0, 1]))
    i32 = lambda *v: np.asarray(v, np.int32)
    i64 = lambda *v: np.asarray(v, np.int64)
    p = cluster.ClusterPaths(i64(0, 4), i64(0, 1, 3, 5, 9), i32(2, 1, 3, 1), i32(0, 2, 3, 6),
                             i32(0, 0, 1, 1, 2, 2, 1, 2, 0), np.asarray([0, 0, 0, 0, 0, 0, 0, 0, 1], np.uint8),
                             i32(0, 0, 1, 2, 2, 2, 3), np.zeros(7, np.uint8), loci, np.asarray(list('abcdefg'), dtype=object))
    res = cluster.ClusterPathContainment(p, i64(0, 2, 2, 3, 3), i32(1, 3, 3), i32(0, 2, 1), np.asarray([0, 1, 0], np.uint8),
                                         i32(1, 1, 2), i32(0, 1, 0, 2), i64(2, 3, 3, 6), i32(3, 1, 3, 3), i64(0, 1, 0, 6))
    seen = {}

    class Trees:
        data = type('D', (), {'index': np.arange(9)})()

        def cluster_path_containment(self, qstart, rev, G):
            seen['args'] = (qstart, rev, G)
            return res

    monkeypatch.setattr(main, 'junction_inputs', lambda path, rows: ('Q', 'R'))
    out = tmp_path / 'c.bed'
    assert main.write_cluster_path_containment(str(out), 'unused.bed', Trees(), 'G')
    assert seen['args'] == ('Q', 'R', 'G')
    assert out.read_text().splitlines() == [
        'cluster\trow\tn_tokens\tn_reads\tn_inner\tsupport\tmaximal\tcollapse_to\tcollapsed_reads\tcontained_in',
        '0\t0\t1\t2\t0\t2\t0\t3\t0\t1:0:+,3:2:-',
        '0\t1\t2\t1\t1\t3\t1\t1\t1\t.',
        '0\t2\t2\t3\t0\t3\t0\t3\t0\t3:1:+',
        '0\t3\t4\t1\t2\t6\t1\t3\t6\t.']
