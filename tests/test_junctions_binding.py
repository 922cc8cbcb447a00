"""The header's fslr_cluster_junctions / fslr_get_cluster_junctions / fslr_cluster_junctions_timings declarations against their
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
# off is an array, n_rows a single value returned by reference
BY_NAME = {'off': ctypes.c_void_p, 'n_rows': ctypes.POINTER(ctypes.c_int64)}
NAMES = ['fslr_cluster_junctions', 'fslr_get_cluster_junctions', 'fslr_cluster_junctions_timings']


def declared(name):
    """(return type, [(argument type, argument name)]) of ``name`` as the header declares it."""
    text = open(HEADER).read()
    m = re.search(r'^(\w+)\s+' + name + r'\(([^)]*)\);', text, re.M)
    assert m, f'{name} is not declared in fslr_hip.h'
    args = []
    for a in re.sub(r'/\*.*?\*/', '', m.group(2)).split(','):     # the comments hold commas
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
    assert [n for _, n in declared('fslr_cluster_junctions')[1]] == ['ctx', 'iv_qkey', 'iv_rev', 'n_intervals', 'n_rows']
    assert [n for _, n in declared('fslr_get_cluster_junctions')[1]] == ['ctx', 'off', 'locus_a', 'locus_b', 'sides',
                                                                         'n_obs', 'n_reads', 'bp', 'capacity']
    assert [n for _, n in declared('fslr_cluster_junctions_timings')[1]] == ['ctx', 'ms']


def test_null_context_is_refused_without_a_device():
    L = _lib.load()
    n = ctypes.c_int64(-7)
    key = np.zeros(4, np.int32)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.fslr_cluster_junctions(None, ptr(key), None, 4, ctypes.byref(n)) == _lib.FSLR_ERR_INVALID
    assert n.value == -7
    off = np.full(3, -7, np.int64)
    cols = [np.full(4, -7, np.int32) for _ in range(4)]
    sides, bp = np.full(4, 249, np.uint8), np.full(16, -7, np.int32)
    assert L.fslr_get_cluster_junctions(None, ptr(off), ptr(cols[0]), ptr(cols[1]), ptr(sides), ptr(cols[2]),
                                        ptr(cols[3]), ptr(bp), 4) == _lib.FSLR_ERR_INVALID
    assert (off == -7).all() and all((c == -7).all() for c in cols) and (sides == 249).all() and (bp == -7).all()
    ms = (ctypes.c_float * 1)(-7.0)
    assert L.fslr_cluster_junctions_timings(None, ms) == _lib.FSLR_ERR_INVALID
    assert ms[0] == -7.0


def test_the_wrapper_parses_strands():
    from fslr_amd import cluster
    assert cluster._rev_bits(['+', '-', '-']).tolist() == [0, 1, 1]
    assert cluster._rev_bits(np.asarray([True, False])).tolist() == [1, 0]
    assert cluster._rev_bits([0, 1, 1, 0]).tolist() == [0, 1, 1, 0]
    assert cluster._rev_bits(np.asarray(['-', '+'], dtype=object)).dtype == np.uint8
    with pytest.raises(ValueError, match="'\\*'"):
        cluster._rev_bits(['+', '*'])


def test_the_cli_strand_rule(tmp_path):
    """rev = (strand == '-') xor (the primary row's strand == '-'); the primary row is the first with a sequence,
    and a read without one counts as forward."""
    from fslr_amd.main import junction_inputs
    rows = [('r1', 0, '-', 'ACGT'), ('r1', 4, '+', ''), ('r1', 9, '-', ''), ('r1', 12, '-', ''),
            ('r2', 0, '+', ''), ('r2', 5, '-', ''), ('r2', 7, '+', 'GG'), ('r2', 9, '-', 'TT'),
            ('r3', 0, '-', ''), ('r3', 3, '+', '')]
    path = tmp_path / 'x.mappings.bed'
    with open(path, 'w') as fh:
        fh.write('qname\tchrom\tqstart\tstrand\tseq\n')
        fh.writelines(f'{q}\tchr1\t{s}\t{st}\t{seq}\n' for q, s, st, seq in rows)
    qstart, rev = junction_inputs(str(path), np.arange(len(rows)))
    assert qstart.tolist() == [0, 4, 9, 12, 0, 5, 7, 9, 0, 3]
    assert rev.tolist() == [0, 1, 0, 0, 0, 1, 0, 1, 1, 0] and rev.dtype == np.uint8
    qstart, rev = junction_inputs(str(path), [9, 1])
    assert (qstart.tolist(), rev.tolist()) == ([3, 4], [0, 1])


def test_abi_version_is_unchanged():
    m = re.search(r'^#define\s+FSLR_ABI_VERSION\s+(\d+)', open(HEADER).read(), re.M)
    assert int(m.group(1)) == _lib.ABI_VERSION == 21 == _lib.load().fslr_abi_version()


def test_cli_refuses_cluster_junctions_on_several_gpus(tmp_path):
    """A usage error before any work: nothing is read, created or started."""
    from click.testing import CliRunner
    from fslr_amd.main import pipeline
    out = tmp_path / 'out'
    res = CliRunner().invoke(pipeline, ['--name', 'x', '--out', str(out), '--ref', 'unused.fa', '--primers', '21q1',
                                        '--skip-alignment', '--cluster-junctions', '--gpus', '2'])
    assert res.exit_code == 2 and '--gpus 1' in res.output
    assert not out.exists()
