"""The header's fslr_cluster_loci / fslr_get_cluster_loci / fslr_cluster_loci_timings declarations against their
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
           'float *': ctypes.POINTER(ctypes.c_float)}
# off is an array, n_rows a single value returned by reference
BY_NAME = {'off': ctypes.c_void_p, 'n_rows': ctypes.POINTER(ctypes.c_int64)}
NAMES = ['fslr_cluster_loci', 'fslr_get_cluster_loci', 'fslr_cluster_loci_timings']


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


def test_the_argument_names():
    assert [n for _, n in declared('fslr_cluster_loci')[1]] == ['ctx', 'n_rows']
    assert [n for _, n in declared('fslr_get_cluster_loci')[1]] == ['ctx', 'off', 'chrom', 'start', 'end',
                                                                    'n_intervals', 'n_reads', 'capacity']
    assert [n for _, n in declared('fslr_cluster_loci_timings')[1]] == ['ctx', 'ms']


def test_null_context_is_refused_without_a_device():
    L = _lib.load()
    n = ctypes.c_int64(-7)
    assert L.fslr_cluster_loci(None, ctypes.byref(n)) == _lib.FSLR_ERR_INVALID
    assert n.value == -7
    off = np.full(3, -7, np.int64)
    cols = [np.full(4, -7, np.int32) for _ in range(5)]
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.fslr_get_cluster_loci(None, ptr(off), *(ptr(c) for c in cols), 4) == _lib.FSLR_ERR_INVALID
    assert (off == -7).all() and all((c == -7).all() for c in cols)
    ms = (ctypes.c_float * 1)(-7.0)
    assert L.fslr_cluster_loci_timings(None, ms) == _lib.FSLR_ERR_INVALID
    assert ms[0] == -7.0


def test_abi_version_is_unchanged():
    m = re.search(r'^#define\s+FSLR_ABI_VERSION\s+(\d+)', open(HEADER).read(), re.M)
    assert int(m.group(1)) == _lib.ABI_VERSION == 21 == _lib.load().fslr_abi_version()


def test_cli_refuses_cluster_loci_on_several_gpus(tmp_path):
    """A usage error before any work: nothing is read, created or started."""
    from click.testing import CliRunner
    from fslr_amd.main import pipeline
    out = tmp_path / 'out'
    res = CliRunner().invoke(pipeline, ['--name', 'x', '--out', str(out), '--ref', 'unused.fa', '--primers', '21q1',
                                        '--skip-alignment', '--cluster-loci', '--gpus', '2'])
    assert res.exit_code == 2 and '--gpus 1' in res.output
    assert not out.exists()
