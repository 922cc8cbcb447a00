"""Directed tests for the walk engine's deferred pairs (query.hip deferred_kernel) at the full lane width.

deferred_kernel puts list2's columns on the 64 lanes of a wavefront and steps list1's rows through the shared
first-fit (firstfit.hpp FirstFit::row<64>).  At overlap <= 0 the walk engine defers every pair that passes
the length gate (a kDefPair entry each), and so it does at any overlap for a pair with a read that holds an
aln_size == 0 interval.  The inputs put the work on the last lane, column 63:
  - two reads of 64 x 64 and of 64 x 63 intervals (long_ref.diagonal);
  - a long_ref.gadgets placement in the last two columns, (r0, r1, c0, c1) = (61, 63, 62, 63).  A gadget's
    contested column c0 has its alternative c1 behind it, so in a list of 64 columns the gadget that reaches
    column 63 has c0 = 62 and c1 = 63: at overlap 0.5 row 61 takes column 62, row 63 finds it taken and column
    63 must stay free (first-fit 1 where a maximum matching has 2); at overlap <= 0 every same-chromosome cell
    matches and row 63 must take column 63.  The run at 0.5 goes through deferred_kernel because read A's
    interval between its two gadget rows, on a chromosome of A's own, is given aln_size 0 (it is never a
    candidate, so nothing raises);
  - a pair whose row 0 meets its first same-chromosome free column at column 63, of aln_size 0: the
    reference raises ZeroDivisionError and the device lists the pair.
Edges with I and U, forward degrees and labels are compared exactly with tests/long_ref.py and the C oracle.
"""
import ctypes
import functools

import numpy as np
import pytest

import long_ref as R
from fslr_amd import _lib
from fslr_amd.prep import fold_overlap_threshold, pass_table
from oracle import oracle as O

gpu = pytest.mark.gpu
QCUT, NCUT = 1 - R.QLEN_DIFF, 1 - R.NAL_DIFF
CUTS = [0.3]
GADGET_PLACE = (61, 63, 62, 63)


@functools.lru_cache(maxsize=None)
def gadget_data():
    """gadgets(64, 64, [GADGET_PLACE]) with aln_size 0 on A's interval 62 (on the chromosome that A alone
    uses; the lists carry the CSR's dense chromosome ids)."""
    plain = R.gadgets(64, 64, [GADGET_PLACE])
    lists, rank = R.read_lists(plain.csr()), R.rank_of(plain)
    reads = [list(lists[rank[k]]) for k in range(len(lists))]
    c, s, e, _ = reads[0][62]
    assert all(x[0] != c for r in reads[1:] for x in r) and c not in (reads[0][61][0], reads[0][63][0])
    reads[0][62] = (c, s, e, 0)
    return R.reads_to_data(reads)


@functools.lru_cache(maxsize=None)
def zero_column_data():
    """A: row 0 on chromosome 1, spanning every start of B; B: 63 columns on a chromosome of its own, then
    column 63 on chromosome 1 with aln_size 0.  A begins first, so it is list1."""
    a = [(1, 0, 451_000, 1000)] + [(2, 1_000_000 + 100 * k, 1_000_010 + 100 * k, 10) for k in range(63)]
    b = [(3, 100 + 100 * k, 110 + 100 * k, 10) for k in range(63)] + [(1, 450_000, 451_000, 0)]
    return R.reads_to_data([a, b] + R.bystanders())


INPUTS = {'diag_64_64': functools.lru_cache(maxsize=None)(functools.partial(R.diagonal, 64, 64)),
          'diag_64_63': functools.lru_cache(maxsize=None)(functools.partial(R.diagonal, 64, 63)),
          'gadget_62_63': gadget_data}
# (input, overlap): every input at overlap 0.0 and -0.5, and the gadget at the overlap it is built for
RUNS = [(name, overlap) for name in INPUTS for overlap in (0.0, -0.5)] + [('gadget_62_63', 0.5)]


def ab_lists(data):
    """(rank of A, rank of B, A's list, B's list): reads r0 and r1 of the input."""
    lists, rank = R.read_lists(data.csr()), R.rank_of(data)
    return rank[0], rank[1], lists[rank[0]], lists[rank[1]]


# ------------------------------------------------------------------ the inputs' conditions (CPU)
def test_gadget_input_is_not_degenerate():
    """At 0.5 first-fit is below the maximum matching and leaves column 63 free; at overlap <= 0 it takes it."""
    data = gadget_data()
    ra, rb, la, lb = ab_lists(data)
    assert ra < rb and len(la) == 64 and len(lb) == 64             # A is list1, both fill the wavefront
    cells = R.matching_cells(la, lb, 0.5)
    r0, r1, c0, c1 = GADGET_PLACE
    assert {(r0, c0), (r0, c1), (r1, c0)} <= set(cells) and (r1, c1) not in cells
    ff = R.first_fit(la, lb, 0.5)
    assert ff == R.first_fit_cells(cells) == 62 and R.max_matching(cells) == 63 and ff < R.max_matching(cells)
    for overlap in (0.0, -0.5):
        dense = R.matching_cells(la, lb, overlap)
        assert (r1, c1) in dense and R.first_fit(la, lb, overlap) == R.max_matching(dense) == 63
    # the edge is the pair's, at every overlap of the runs
    for overlap in (0.5, 0.0, -0.5):
        want = R.long_ref(data.csr(), overlap, CUTS)
        assert (ra, rb, R.first_fit(la, lb, overlap), 128 - R.first_fit(la, lb, overlap)) in want.edges


def test_diagonal_inputs_fill_the_last_column():
    for name, (na, nb) in {'diag_64_64': (64, 64), 'diag_64_63': (64, 63)}.items():
        ra, rb, la, lb = ab_lists(INPUTS[name]())
        assert ra < rb and (len(la), len(lb)) == (na, nb)
        for overlap in (0.0, -0.5):
            assert R.first_fit(la, lb, overlap) == nb


def test_zero_column_input_raises_in_the_reference():
    data = zero_column_data()
    ra, rb, la, lb = ab_lists(data)
    assert (ra, rb) == (0, 1) and len(la) == len(lb) == 64
    assert [j for j, y in enumerate(lb) if y[0] == la[0][0]] == [63] and lb[63][3] == 0
    for overlap in (0.0, -0.5):
        with pytest.raises(ZeroDivisionError):
            R.first_fit(la, lb, overlap)
        with pytest.raises(ZeroDivisionError):
            R.long_ref(data.csr(), overlap, CUTS)
        with pytest.raises(O.OracleZeroDivision):
            O.run_core(R.oracle_from_csr(data.csr()), overlap, CUTS, R.QLEN_DIFF, R.NAL_DIFF, 10, use_cap=False)


# ------------------------------------------------------------------ the device (GPU)
@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def walk_query(c, csr, overlap):
    c.load_csr(csr, fold_overlap_threshold(csr.iv_aln, overlap))
    c.reserve_edges(1 << 12)
    c.build_index()
    c.query(QCUT, NCUT, pass_table(CUTS), 10, engine='walk')


@gpu
@pytest.mark.parametrize('name,overlap', RUNS)
def test_deferred_pairs_equal_the_reference(ctx, name, overlap):
    data = INPUTS[name]()
    csr = data.csr()
    want = R.long_ref(csr, overlap, CUTS)
    o = O.run_core(R.oracle_from_csr(csr), overlap, CUTS, R.QLEN_DIFF, R.NAL_DIFF, 10, use_cap=False)
    oe = sorted(zip(o['edge_a'].tolist(), o['edge_b'].tolist(), o['edge_I'].tolist(), o['edge_U'].tolist()))
    assert oe == want.edges
    ra, rb, la, lb = ab_lists(data)
    I = R.first_fit(la, lb, overlap)
    assert (ra, rb, I, len(la) + len(lb) - I) in want.edges
    walk_query(ctx, csr, overlap)
    ctx.components()
    st = ctx.stats()
    assert st['engine'] == 'walk'
    # the pair of r0 and r1 went through the deferred list: every gated pair at overlap <= 0, the pairs of
    # the read with the aln_size == 0 interval at 0.5; each entry is a kDefPair one, evaluated once
    assert st['gather_pairs'] == st['deferred'] >= 1
    if overlap <= 0:
        assert st['deferred'] == st['jaccard_evals']
    a, b, gI, gU = ctx.edges(st['n_edges'])
    assert sorted(zip(a.tolist(), b.tolist(), gI.tolist(), gU.tolist())) == want.edges
    np.testing.assert_array_equal(ctx.fwd_degree(), want.fwd)
    np.testing.assert_array_equal(ctx.labels(), want.labels)
    assert st['zd_pairs'] == 0


@gpu
@pytest.mark.parametrize('overlap', [0.0, -0.5])
def test_zero_aln_at_column_63_raises_with_the_pair(ctx, overlap):
    csr = zero_column_data().csr()
    walk_query(ctx, csr, overlap)
    with pytest.raises(ZeroDivisionError):
        ctx.stats()
    s = _lib.QueryStats()                                  # the struct whatever the return code
    assert ctx._L.fslr_read_stats(ctx._h, ctypes.byref(s)) == _lib.FSLR_ERR_ZERO_DIVISION
    st = s.as_dict()
    assert st['engine'] == 'walk' and st['zd_pairs'] == 1 and (st['err_a'], st['err_b']) == (0, 1)
