"""The header's fslr_cluster_collapsed_segments / fslr_cluster_collapsed_segments_any /
fslr_get_cluster_collapsed_segments / fslr_cluster_collapsed_segments_timings declarations against their ctypes
prototypes in fslr_amd/_lib.py, the wrappers' refusals, the result class on rows from the plain statement and the
command line's writer (no device)."""
import ctypes
import os
import re

import numpy as np
import pytest

import collapsed_ref as cl
import search_ref as sr
from fslr_amd import _lib, cluster
from test_collapsed_ref import run, three_loci

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'fslr_hip.h')

pytestmark = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason='libfslr_hip.so is not built')

C_TYPES = {'fslr_ctx *': ctypes.c_void_p, 'int64_t': ctypes.c_int64, 'int32_t *': ctypes.c_void_p,
           'const int32_t *': ctypes.c_void_p, 'float *': ctypes.POINTER(ctypes.c_float),
           'int64_t *': ctypes.POINTER(ctypes.c_int64)}
NAMES = ['fslr_cluster_collapsed_segments', 'fslr_cluster_collapsed_segments_any', 'fslr_get_cluster_collapsed_segments',
         'fslr_cluster_collapsed_segments_timings']


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
    run_args = ['ctx', 'iv_qkey', 'iv_qend', 'n_intervals', 'n_tokens']
    assert [n for _, n in declared(NAMES[0])[1]] == run_args == [n for _, n in declared(NAMES[1])[1]]
    assert [n for _, n in declared(NAMES[2])[1]] == ['ctx', 'n_cov', 'n_link', 'start', 'end', 'gap', 'token_capacity']
    assert [n for _, n in declared(NAMES[3])[1]] == ['ctx', 'ms']


def test_null_context_is_refused_without_a_device():
    L = _lib.load()
    n = ctypes.c_int64(-7)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    q = np.zeros(4, np.int32)
    for name in NAMES[:2]:
        assert getattr(L, name)(None, ptr(q), ptr(q), 4, ctypes.byref(n)) == _lib.FSLR_ERR_INVALID
    assert n.value == -7
    outs = [np.full(12, -7, np.int32) for _ in range(5)]
    assert L.fslr_get_cluster_collapsed_segments(None, *[ptr(a) for a in outs], 4) == _lib.FSLR_ERR_INVALID
    assert all((a == -7).all() for a in outs)
    ms = (ctypes.c_float * 1)(-7.0)
    assert L.fslr_cluster_collapsed_segments_timings(None, ms) == _lib.FSLR_ERR_INVALID
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


@pytest.mark.parametrize('method, symbol', [('cluster_collapsed_segments', NAMES[0]), ('cluster_collapsed_segments_any', NAMES[1])])
def test_context_wrapper_stops_at_the_library_s_refusal(method, symbol):
    c = object.__new__(_lib.Context)
    c._L, c._h, c.n_reads = Recorder(), None, 0
    c._check = lambda rc: (_ for _ in ()).throw(RuntimeError(f'rc {rc}')) if rc else None
    with pytest.raises(RuntimeError, match=f'rc {_lib.FSLR_ERR_STATE}'):
        getattr(c, method)(np.arange(5, dtype=np.int32))
    (name, args), = c._L.calls                                    # the getter was not reached
    assert name == symbol and len(args) == 5 and args[2] is None and args[3] == 5
    with pytest.raises(ValueError, match='shape'):
        getattr(c, method)(np.arange(5), np.arange(4))
    with pytest.raises(RuntimeError, match=f'rc {_lib.FSLR_ERR_STATE}'):
        c.cluster_collapsed_segments_timings()


def test_multi_gpu_index_refuses():
    mg = cluster.MultiGpuIndex(sr.make_data([1, 1], [0, 5], [9, 9]), 2)
    for method in ('cluster_collapsed_segments', 'cluster_collapsed_segments_any'):
        with pytest.raises(NotImplementedError, match='n_gpus=1'):
            getattr(mg, method)([0, 1])


def test_cli_refuses_cluster_collapsed_segments_on_several_gpus(tmp_path):
    """A usage error before any work: nothing is read, created or started."""
    from click.testing import CliRunner
    from fslr_amd.main import pipeline
    out = tmp_path / 'out'
    res = CliRunner().invoke(pipeline, ['--name', 'x', '--out', str(out), '--ref', 'unused.fa', '--primers', '21q1',
                                        '--skip-alignment', '--cluster-collapsed-segments', '--gpus', '2'])
    assert res.exit_code == 2 and '--gpus 1' in res.output and '--cluster-collapsed-segments' in res.output
    assert not out.exists()


def statement_result():
    """ClusterCollapsedSegments on the rows of the statement's first hand-worked cluster (tests/test_collapsed_ref.py):
    rows (L0+, L1+) | (L0+, L1+, L2+) | (L1+, L2+), the outer two collapse onto the middle one."""
    p, ct, got = run(three_loci())
    loci = cluster.ClusterLoci(np.asarray([0, 3]), np.asarray([4, 4, 4], dtype=object), np.asarray([0, 10000, 20000]),
                               np.asarray([106, 10106, 20104]), np.asarray([3, 4, 3]), np.asarray([3, 4, 3]), np.asarray([0, 0, 0]))
    paths = cluster.ClusterPaths(*[p[k] for k in ('off', 'tok_off', 'n_reads', 'first_read', 'locus', 'rev', 'path_of_read', 'flipped')],
                                 loci, np.asarray(list('abcd'), dtype=object))
    cont = cluster.ClusterPathContainment(paths, *[ct[k] for k in ('coff', 'outer', 'offset', 'rev', 'n_occ', 'n_inner', 'support',
                                                                    'collapse_to', 'collapsed_reads')])
    return cluster.ClusterCollapsedSegments(paths, cont, *[got[k] for k in cl.NAMES])


def test_the_frame_of_a_result_on_rows_from_the_statement():
    s = statement_result()
    assert cluster.ClusterCollapsedSegments.NAMES == cl.NAMES and len(s) == 7
    assert [c.tolist() for c in s.columns()][0] == [0, 0, 3, 4, 3, 0, 0]
    f = s.to_frame()
    assert list(f.columns) == ['cluster', 'path', 'piece', 'chrom', 'start', 'end', 'strand', 'n_cov', 'start_min',
                               'start_max', 'end_min', 'end_max', 'gap_min', 'gap', 'gap_max', 'n_link', 'collapsed_reads']
    # one line per piece of the maximal row alone (path 1 of cluster 0): all four reads collapse onto it
    assert f.values.tolist() == [
        [0, 1, 0, 4, 2, 102, '+', 3, 0, 6, 100, 106, 2, 4, 6, 3, 4],
        [0, 1, 1, 4, 10002, 10102, '+', 4, 10000, 10006, 10100, 10106, 1, 3, 5, 3, 4],
        [0, 1, 2, 4, 20002, 20102, '+', 3, 20000, 20004, 20100, 20104, 0, 0, 0, 0, 4]]


def test_the_writer_on_rows_from_the_statement(tmp_path, monkeypatch):
    from fslr_amd import main
    res, seen = statement_result(), {}

    class Trees:
        data = type('D', (), {'index': np.arange(10)})()

        def cluster_collapsed_segments_any(self, qstart, qend, rev, G):
            seen['args'] = (qstart, qend, rev, G)
            return res

    monkeypatch.setattr(main, 'junction_inputs', lambda path, rows, with_qend=False: ('Q', 'R', 'E'))
    out = tmp_path / 'c.bed'
    assert main.write_cluster_collapsed_segments(str(out), 'unused.bed', Trees(), 'G', {'chr4': 4})
    assert seen['args'] == ('Q', 'E', 'R', 'G')
    assert out.read_text().splitlines() == [
        'chrom\tstart\tend\tcluster\tpath\tpiece\tstrand\tn_cov\tstart_min\tstart_max\tend_min\tend_max\tgap_min\tgap\tgap_max'
        '\tn_link\tcollapsed_reads',
        'chr4\t2\t102\t0\t1\t0\t+\t3\t0\t6\t100\t106\t2\t4\t6\t3\t4',
        'chr4\t10002\t10102\t0\t1\t1\t+\t4\t10000\t10006\t10100\t10106\t1\t3\t5\t3\t4',
        'chr4\t20002\t20102\t0\t1\t2\t+\t3\t20000\t20004\t20100\t20104\t0\t0\t0\t0\t4']
