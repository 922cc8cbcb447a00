"""tests/paths_ref.py, the plain statement of fslr_cluster_paths, against cases worked by hand (no device).  Every
expectation below is written out as literals."""
import numpy as np

import junctions_ref as jr
import paths_ref as pr

# three loci on chromosome 0 for the cases below: 0 = [100, 2xx], 1 = [1000, 11xx], 2 = [5000, 51xx]
A, B, C = (0, 100, 200), (0, 1000, 1100), (0, 5000, 5100)


def make(reads, cid=None):
    """reads: per read a list of (chrom, start, end, qkey, rev).  All reads in cluster 0 unless ``cid`` says."""
    flat = [iv for r in reads for iv in r]
    off = np.cumsum([0] + [len(r) for r in reads])
    cols = [np.asarray([iv[k] for iv in flat], np.int64) for k in range(5)]
    cid = np.zeros(len(reads), np.int64) if cid is None else np.asarray(cid, np.int64)
    return off, cols, cid, int(cid.max()) + 1


def result(reads, cid=None, rev=True):
    off, (ch, s, e, key, rv), cid, nc = make(reads, cid)
    return pr.paths(off, ch, s, e, cid, nc, key, rv if rev else None)


def test_two_reads_with_identical_chains():
    # both walk locus 0 forward, locus 1 reversed, locus 2 forward: F = (0, 3, 4), B = (5, 2, 1)
    res = result([[A + (0, 0), B + (1, 1), C + (2, 0)], [A + (5, 0), B + (6, 1), C + (9, 0)]])
    assert pr.rows_of(res) == [((0, 3, 4), 2, 0)]
    assert res['off'].tolist() == [0, 1] and res['tok_off'].tolist() == [0, 3]
    assert res['locus'].tolist() == [0, 1, 2] and res['rev'].tolist() == [0, 1, 0]
    assert res['path_of_read'].tolist() == [0, 0] and res['flipped'].tolist() == [0, 0]
    assert {k: res[k].dtype for k in pr.NAMES} == pr.DTYPES


def test_one_read_reverse_complemented_gives_one_row_and_opposite_flipped():
    reads = [[A + (0, 0), B + (1, 1), C + (2, 0)], [A + (5, 0), B + (6, 1), C + (9, 0)]]
    off, (ch, s, e, key, rv), cid, nc = make(reads)
    k2, r2 = jr.reverse_complement(off, key, rv, [1])
    res = pr.paths(off, ch, s, e, cid, nc, k2, r2)
    # read 1 now walks locus 2 reversed, locus 1 forward, locus 0 reversed: F = (5, 2, 1), B = (0, 3, 4) < F
    assert pr.rows_of(res) == [((0, 3, 4), 2, 0)]
    assert res['path_of_read'].tolist() == [0, 0] and res['flipped'].tolist() == [0, 1]
    # written out without the helper: the same chain given directly
    direct = result([[A + (0, 0), B + (1, 1), C + (2, 0)], [C + (0, 1), B + (1, 0), A + (2, 1)]])
    assert pr.rows_of(direct) == [((0, 3, 4), 2, 0)] and direct['flipped'].tolist() == [0, 1]


def test_a_palindromic_chain_is_not_flipped():
    # [a:+, a:-]: F = (0, 1), B = (1 ^ 1, 0 ^ 1) = (0, 1) = F
    res = result([[(0, 100, 200, 0, 0), (0, 150, 250, 1, 1)], [(0, 120, 130, 0, 0)]])
    assert pr.rows_of(res) == [((0,), 1, 1), ((0, 1), 1, 0)]
    assert res['flipped'].tolist() == [0, 0] and res['path_of_read'].tolist() == [1, 0]
    # length 4: a:+ b:+ b:- a:-, F = (0, 2, 3, 1) = B
    res = result([[A + (0, 0), B + (1, 0), (0, 1010, 1090, 2, 1), (0, 110, 190, 3, 1)], [(0, 120, 130, 0, 0)]])
    assert pr.rows_of(res) == [((0,), 1, 1), ((0, 2, 3, 1), 1, 0)] and res['flipped'].tolist() == [0, 0]


def test_a_prefix_sorts_before_its_extension():
    res = result([[A + (0, 0), B + (1, 0), C + (2, 0)], [A + (0, 0), B + (1, 0)]])
    # (0, 2) is a proper prefix of (0, 2, 4): two rows, the prefix first
    assert pr.rows_of(res) == [((0, 2), 1, 1), ((0, 2, 4), 1, 0)]
    assert res['tok_off'].tolist() == [0, 2, 5] and res['path_of_read'].tolist() == [1, 0]


def test_equal_query_keys_fall_back_to_csr_order():
    other = [(0, 110, 120, 0, 0)]
    tied = result([[C + (5, 0), A + (5, 0), B + (5, 0)], other])        # CSR order: c, a, b; F = (4, 0, 2), B = (3, 1, 5)
    assert pr.rows_of(tied) == [((0,), 1, 1), ((3, 1, 5), 1, 0)] and tied['flipped'].tolist() == [1, 0]
    early = result([[C + (5, 0), A + (5, 0), B + (4, 0)], other])       # b, c, a: F = (2, 4, 0), B = (1, 5, 3)
    assert pr.rows_of(early) == [((0,), 1, 1), ((1, 5, 3), 1, 0)]
    # a reverse complement of tied keys does not reverse the order: its path differs from the original's
    off, (ch, s, e, key, rv), cid, nc = make([[C + (5, 0), A + (5, 0), B + (5, 0)], other])
    k2, r2 = jr.reverse_complement(off, key, rv, [0])
    rc = pr.paths(off, ch, s, e, cid, nc, k2, r2)                       # F = (5, 1, 3), B = (2, 0, 4)
    assert pr.rows_of(rc) == [((0,), 1, 1), ((2, 0, 4), 1, 0)]


def test_a_one_interval_read_has_rev_0_after_canonicalisation():
    res = result([[A + (0, 1)], [(0, 150, 250, 0, 0)]])                 # F = (1,), B = (0,): flipped
    assert pr.rows_of(res) == [((0,), 2, 0)]
    assert res['flipped'].tolist() == [1, 0] and res['rev'].tolist() == [0]


def test_an_unclustered_read_and_rev_none():
    res = result([[A + (0, 0), B + (1, 0)], [A + (0, 1), B + (1, 1)], [A + (1, 0), B + (0, 0)]], cid=[0, -1, 0], rev=False)
    # read 2 walks b then a: F = (2, 0), B = (1, 3) < F
    assert pr.rows_of(res) == [((0, 2), 1, 0), ((1, 3), 1, 2)]
    assert res['path_of_read'].tolist() == [0, -1, 1] and res['flipped'].tolist() == [0, 0, 1]


def test_no_clusters():
    res = result([[A + (0, 0)], [B + (0, 0)]], cid=[-1, -1])
    assert res['off'].tolist() == [0] and res['tok_off'].tolist() == [0]
    assert all(res[k].size == 0 for k in ('n_reads', 'first_read', 'locus', 'rev'))
    assert res['path_of_read'].tolist() == [-1, -1] and res['flipped'].tolist() == [0, 0]
    res = pr.paths([0], [], [], [], [], 0, [], [])
    assert res['off'].tolist() == [0] and res['path_of_read'].size == 0


def test_random_inputs_cluster_order_sums_and_reverse_complements():
    rng = np.random.default_rng(5)
    reads, cid = [], []
    for r in range(80):
        n = int(rng.integers(1, 7))
        reads.append([(int(rng.integers(0, 3)), int(s), int(s) + int(rng.integers(0, 80)), k, int(rng.integers(0, 2)))
                      for k, s in enumerate(rng.integers(0, 2000, n))])          # distinct keys within a read
        cid.append(int(rng.integers(-1, 4)))
    cid = np.asarray(cid)
    cid[:4] = [0, 1, 2, 3]
    off, (ch, s, e, key, rv), cid, nc = make(reads, cid)
    res = pr.paths(off, ch, s, e, cid, nc, key, rv)
    rows = pr.rows_of(res)
    assert [t for t, _, _ in rows] == sorted({t for t, _, _ in rows})
    loci = jr.loci_ref.loci(off, ch, s, e, cid, nc)
    of_locus = np.repeat(np.arange(nc), np.diff(loci['off']))
    for c in range(nc):
        a, b = int(res['off'][c]), int(res['off'][c + 1])
        assert int(res['n_reads'][a:b].sum()) == int((cid == c).sum())
        assert all((of_locus[[t >> 1 for t in rows[i][0]]] == c).all() for i in range(a, b))
    turned = np.flatnonzero(rng.integers(0, 2, len(reads)))
    k2, r2 = jr.reverse_complement(off, key, rv, turned)
    rc = pr.paths(off, ch, s, e, cid, nc, k2, r2)
    for k in pr.NAMES[:-1]:
        np.testing.assert_array_equal(rc[k], res[k], err_msg=k)
    pal = np.asarray([r >= 0 and rows[r][0] == tuple(t ^ 1 for t in reversed(rows[r][0])) for r in res['path_of_read']])
    is_turned = np.isin(np.arange(len(reads)), turned)
    change = (rc['flipped'] != res['flipped'])
    np.testing.assert_array_equal(change, is_turned & (cid >= 0) & ~pal)
