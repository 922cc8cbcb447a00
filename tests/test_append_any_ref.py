"""The contracts of fslr_append_reads_any / fslr_remove_reads_any on the host.

append_any_ref states the virtual layout after an append and after a removal with plain loops; here it is pinned to
prep.split_long_reads of the union / of the survivors, and fslr_amd/csrc/any_idx.hpp (the arithmetic the device
kernels and the host bookkeeping share) is compiled into a stand-alone program and compared with it."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import append_any_ref as aa
import append_ref as ar
from fslr_amd import prep
from fslr_amd.prep import CSR

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')

# (resident real lengths, batch real lengths): the seams of the append
APPEND_SHAPES = {
    'plain_plus_65': ([3, 1, 64, 2], [2, 65, 1]),
    'long_plus_short': ([5, 65, 1, 128, 129, 2, 4096, 64], [1, 7, 64, 3]),
    'long_both': ([65, 2, 200], [1, 130, 64, 65, 3]),
    'batch_64_and_4096': ([2, 70], [64, 4096]),
    'one_and_one': ([65], [65]),
    'plain_both': ([1, 2, 3], [4, 5]),
}
REMOVE_SHAPES = {
    'only_long_goes': ([3, 70, 2, 64], [1, 0, 1, 1]),
    'long_between_two': ([65, 1, 128, 2, 129, 3], [1, 1, 0, 1, 1, 0]),
    'only_short_go': ([1, 65, 2, 200, 3], [0, 1, 0, 1, 1]),
    'one_long_left': ([4, 4096, 65, 1], [0, 1, 0, 0]),
    'all_stay': ([65, 1, 130], [1, 1, 1]),
}


def csr_of(lens, seed, base=0):
    """A real CSR of the given read lengths whose iv_end names each real interval (base + its index)."""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.int64)
    ni = int(lens.sum())
    start = rng.integers(0, 50, ni).astype(np.int32)             # ties on purpose
    order = np.argsort(start, kind='stable')
    dp = np.empty(ni, np.int64)
    dp[order] = np.arange(ni)
    return CSR(read_off=np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), read_qlen2=np.arange(lens.size, dtype=np.int32) + 100,
               read_nal=np.full(lens.size, 3, np.int32), iv_chrom=np.zeros(ni, np.int32), iv_start=start,
               iv_end=base + np.arange(ni, dtype=np.int32), iv_aln=np.full(ni, 50, np.int64), n_chroms=1,
               read_qcode=np.arange(lens.size, dtype=np.int64), data_pos=dp, nal_varies=False)


@pytest.mark.parametrize('name', list(APPEND_SHAPES))
def test_append_layout_is_split_long_reads_of_the_union(name):
    res_l, new_l = APPEND_SHAPES[name]
    res, new = csr_of(res_l, 1), csr_of(new_l, 2, base=sum(res_l))
    u = ar.concat_csr(res, new)
    vu, vreal, vbase, rlen = prep.split_long_reads(u)
    lay = aa.append_layout(res_l, new_l)
    np.testing.assert_array_equal(vreal, lay['vreal'])
    np.testing.assert_array_equal(vbase, lay['vbase'])
    np.testing.assert_array_equal(rlen, lay['rlen'])
    np.testing.assert_array_equal(np.diff(vu.read_off), lay['vlen'])
    np.testing.assert_array_equal(vu.iv_end, lay['rows'])                       # iv_end names the real interval
    # every row and rank of the union comes from where the statement says, in the two sides' own virtual CSRs
    vr, vb = prep.split_long_reads(res)[0], prep.split_long_reads(new)[0]
    src = lay['row_src']
    want_end = np.where(src >= 0, vr.iv_end[np.maximum(src, 0)], vb.iv_end[np.maximum(~src, 0)])
    np.testing.assert_array_equal(vu.iv_end, want_end)
    pos_res, pos_new = ar.merged_positions(ar.data_starts(res), ar.data_starts(new))
    want_dp = np.where(src >= 0, pos_res[vr.data_pos[np.maximum(src, 0)]], pos_new[vb.data_pos[np.maximum(~src, 0)]])
    np.testing.assert_array_equal(vu.data_pos, want_dp)
    rs = lay['rank_src']
    np.testing.assert_array_equal(vu.read_qlen2, np.where(rs >= 0, vr.read_qlen2[np.maximum(rs, 0)], vb.read_qlen2[np.maximum(~rs, 0)]))
    # off2: the row of interval 64 of every long read
    for r in np.flatnonzero(lay['rlen'] > 64):
        first_further = np.flatnonzero((vreal == r) & (vbase == 64))[0]
        assert lay['off2'][r] == vu.read_off[first_further]
    assert (lay['off2'][lay['rlen'] <= 64] == -1).all()


@pytest.mark.parametrize('name', list(REMOVE_SHAPES))
def test_remove_layout_is_split_long_reads_of_the_survivors(name):
    res_l, keep = REMOVE_SHAPES[name]
    keep = np.asarray(keep, bool)
    res = csr_of(res_l, 3)
    left, ranks = prep.remove_reads_csr(res, keep)
    lay = aa.remove_layout(res_l, keep)
    np.testing.assert_array_equal(ranks, lay['new_rank'])
    vr = prep.split_long_reads(res)[0]
    if prep.has_long_reads(left):
        vl, vreal, vbase, rlen = prep.split_long_reads(left)
    else:                                                   # a plain context: the virtual CSR is the real one
        vl, vreal, vbase, rlen = left, np.arange(left.n_reads), np.zeros(left.n_reads, np.int64), np.diff(left.read_off)
    np.testing.assert_array_equal(vreal, lay['vreal'])
    np.testing.assert_array_equal(vbase, lay['vbase'])
    np.testing.assert_array_equal(rlen, lay['rlen'])
    np.testing.assert_array_equal(vl.iv_start, vr.iv_start[lay['row_src']])
    # the virtual keep flag is keep[vreal[v]] and the virtual compaction is stable
    _, old_vreal, _, _ = prep.split_long_reads(res) if prep.has_long_reads(res) else (None, np.arange(res.n_reads), None, None)
    kv = keep[old_vreal]
    np.testing.assert_array_equal(lay['new_vrank'], np.where(kv, np.cumsum(kv) - 1, -1))
    np.testing.assert_array_equal(lay['new_vrank'][:res.n_reads], lay['new_rank'])


def test_append_then_remove_is_the_identity():
    res_l, new_l = APPEND_SHAPES['long_both']
    keep = np.arange(len(res_l) + len(new_l)) < len(res_l)
    back = aa.remove_layout(list(res_l) + list(new_l), keep)
    own = aa.virtual_layout(res_l)
    for got, want in zip((back['vreal'], back['vbase'], back['vlen'], back['rows'], back['off2']), own):
        np.testing.assert_array_equal(got, want)


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++') or shutil.which('hipcc') or \
        next((p for p in ('/opt/rocm/bin/hipcc', '/opt/rocm/llvm/bin/clang++') if os.path.exists(p)), None)
    assert cxx is not None, 'no C++ compiler (g++, c++, clang++, hipcc): any_idx.hpp cannot be checked on the host'
    exe = str(tmp_path_factory.mktemp('anyidx') / 'any_idx_main')
    subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    '-I', os.path.join(ROOT, 'fslr_amd', 'csrc'), '-o', exe, os.path.join(ROOT, 'tests', 'any_idx_main.cpp')],
                   check=True)
    return exe


@pytest.mark.parametrize('name', list(APPEND_SHAPES))
def test_the_index_header_agrees_with_the_statement(program, name):
    res_l, new_l = APPEND_SHAPES[name]
    sh = aa.shape(res_l, new_l)
    lay = aa.append_layout(res_l, new_l)
    res_off2 = aa.virtual_layout(res_l)[4]
    n = len(res_l)
    long_res = [r for r in range(n) if res_l[r] > 64]
    long_new = [r for r in range(len(new_l)) if new_l[r] > 64]
    before = [int(sum(max(L - 64, 0) for L in new_l[:r])) for r in long_new]
    args = [str(sh[k]) for k in ('n', 'V', 'o1', 'ni', 'm', 'e', 'mi1', 'mi')]
    args += [f'r{int(res_off2[r])}' for r in long_res] + [f'b{x}' for x in before]
    out = subprocess.run([program] + args, check=True, capture_output=True, text=True).stdout
    tab = {ln.split()[0]: np.asarray(ln.split()[1:], np.int64) for ln in out.splitlines()}
    np.testing.assert_array_equal(tab['new_vrank'], lay['new_vrank'])
    np.testing.assert_array_equal(tab['new_row'], lay['new_row'])
    np.testing.assert_array_equal(tab['rank_source'], lay['rank_src'])
    np.testing.assert_array_equal(tab['row_source'], lay['row_src'])
    v = np.arange(sh['V'])
    np.testing.assert_array_equal(tab['retag'], (lay['new_vrank'] << 6) | (v & 63))
    np.testing.assert_array_equal(tab['off2'], np.concatenate([lay['off2'][long_res], lay['off2'][[n + r for r in long_new]]]).astype(np.int64))
    L = np.arange(1, 4097)
    np.testing.assert_array_equal(tab['extra_chunks'], (L + 63) // 64 - 1)
