"""fslr_amd.prep.remove_reads_csr / kept_data_rows (the CSR without some of its reads, for a caller that uploads
what is left) and the numpy statement of that contract (remove_ref), both pinned three ways: to build_csr of the data
list without the removed reads' rows (the reference's own preparation of the smaller frame), to append's
reference (append then remove gives the resident set back), and at its two ends (everything, nothing)."""
import numpy as np
import pytest

import append_ref as ar
import match_ref as mr
import remove_ref as rr
from host_pipeline import host_prepare
from fslr_amd import prep
from fslr_amd.prep import build_csr

COLUMNS = ('read_off', 'read_qlen2', 'read_nal', 'iv_start', 'iv_end', 'iv_aln', 'read_qcode', 'data_pos')


def same_columns(got, want, chrom=True):
    for f in COLUMNS + (('iv_chrom',) if chrom else ()):
        np.testing.assert_array_equal(np.asarray(getattr(got, f), np.int64), np.asarray(getattr(want, f), np.int64), err_msg=f)


def against_build_csr(data, keep):
    """The product's remove_reads_csr and the reference's remove_csr of the whole list's CSR against build_csr
    of the list without the removed reads' rows."""
    csr = data.csr()
    got, dp, ranks = rr.remove_csr(csr, keep)
    rows = prep.kept_data_rows(csr, keep)
    np.testing.assert_array_equal(rows, rr.kept_rows(csr, keep))
    mine, my_ranks = prep.remove_reads_csr(csr, keep)
    same_columns(mine, got)
    np.testing.assert_array_equal(my_ranks, ranks)
    assert my_ranks.dtype == np.int32 and mine.n_chroms == csr.n_chroms and mine.start_sorted
    assert mine.read_off.dtype == np.int32 and mine.nal_varies == csr.nal_varies
    want = build_csr(data.select(rows))
    assert want.start_sorted and got.n_reads == want.n_reads == int(keep.sum())
    same_columns(got, want, chrom=False)
    np.testing.assert_array_equal(dp, want.data_pos)
    # the dense ids stay the resident ones: build_csr renumbers the chromosomes that are left, in the same order
    present, dense = np.unique(got.iv_chrom, return_inverse=True)
    np.testing.assert_array_equal(dense, want.iv_chrom)
    assert got.n_chroms == csr.n_chroms >= want.n_chroms == present.size
    # the rank map: first-appearance ranks of the smaller frame are the resident ranks with the gaps closed
    np.testing.assert_array_equal(np.flatnonzero(ranks >= 0), np.flatnonzero(keep))
    np.testing.assert_array_equal(ranks[keep], np.arange(want.n_reads))
    np.testing.assert_array_equal(np.asarray(csr.read_qcode)[keep], want.read_qcode)
    return got, want


@pytest.mark.parametrize('frac', [0.05, 1 / 3, 0.9])
def test_golden_fixture_equals_prepare_data_of_the_smaller_frame(frac):
    data, _, _ = host_prepare('ties_600')
    n = data.csr().n_reads
    keep = np.random.default_rng(int(frac * 100)).random(n) >= frac
    got, want = against_build_csr(data, keep)
    assert 0 < got.n_reads < n


def tie_run_data(seed=4):
    """120 reads of 1-5 intervals on two chromosomes with starts from 6 values: tie runs of ~50 elements."""
    rng = np.random.default_rng(seed)
    reads = [[(int(c), int(s) * 10, int(s) * 10 + 80, 80) for c, s in zip(rng.integers(1, 3, L), rng.integers(0, 6, L))]
             for L in rng.integers(1, 6, 120)]
    return mr.resident_data(reads, rng.integers(900, 1100, 120), rng.integers(1, 5, 120), shuffle_seed=seed)


@pytest.mark.parametrize('pattern', ['alternate', 'random', 'first_and_last', 'one_left', 'a_chromosome'])
def test_long_tie_runs_equal_prepare_data_of_the_smaller_frame(pattern):
    data = tie_run_data()
    csr = data.csr()
    n = csr.n_reads
    keep = np.ones(n, bool)
    if pattern == 'alternate':
        keep[1::2] = False
    elif pattern == 'random':
        keep = np.random.default_rng(1).random(n) < 0.5
    elif pattern == 'first_and_last':
        keep[[0, n - 1]] = False
    elif pattern == 'one_left':
        keep[:] = False
        keep[n // 2] = True
    else:                                         # every read that touches dense chromosome 0 goes
        on0 = np.repeat(np.arange(n), np.diff(csr.read_off))[csr.iv_chrom == 0]
        keep[on0] = False
        assert keep.any()
    got, want = against_build_csr(data, keep)
    if pattern == 'a_chromosome':
        assert want.n_chroms == 1 and got.n_chroms == 2 and (got.iv_chrom == 1).all()
    s = np.empty(got.n_intervals, np.int64)
    s[got.data_pos] = got.iv_start
    assert (np.diff(s) >= 0).all()


def test_append_then_remove_gives_the_resident_set_back():
    rng = np.random.default_rng(5)
    reads = [[(int(c), int(s), int(s) + 50, 50) for c, s in zip(rng.integers(1, 3, L), rng.integers(0, 40, L))]
             for L in rng.integers(1, 6, 60)]
    res = mr.resident_data(reads[:45], np.full(45, 1000), np.full(45, 3), shuffle_seed=1).csr()
    new = mr.resident_data(reads[45:], np.full(15, 1000), np.full(15, 3), shuffle_seed=2).csr()
    u = ar.concat_csr(res, new)
    keep = np.arange(u.n_reads) < res.n_reads
    back, dp, ranks = rr.remove_csr(u, keep)
    same_columns(back, res)
    assert back.n_chroms == u.n_chroms
    np.testing.assert_array_equal(ranks, np.where(keep, np.arange(u.n_reads), -1))
    mine, my_ranks = prep.remove_reads_csr(u, keep)
    same_columns(mine, res)
    np.testing.assert_array_equal(my_ranks, ranks)
    # and the other way round: removing the resident reads leaves the batch, its own order intact
    rest, _, _ = rr.remove_csr(u, ~keep)
    for f in ('read_off', 'read_qlen2', 'read_nal', 'iv_chrom', 'iv_start', 'iv_end', 'iv_aln', 'data_pos'):
        np.testing.assert_array_equal(np.asarray(getattr(rest, f), np.int64), np.asarray(getattr(new, f), np.int64), err_msg=f)


def test_everything_and_nothing():
    csr = tie_run_data(7).csr()
    n = csr.n_reads
    with pytest.raises(ValueError, match='would leave no reads'):
        rr.remove_csr(csr, np.zeros(n, bool))
    with pytest.raises(ValueError, match='one mask entry per read'):
        rr.remove_csr(csr, np.ones(n + 1, bool))
    same, dp, ranks = rr.remove_csr(csr, np.ones(n, bool))
    same_columns(same, csr)
    np.testing.assert_array_equal(dp, csr.data_pos)
    np.testing.assert_array_equal(ranks, np.arange(n))
    np.testing.assert_array_equal(rr.rank_map([True, False, False, True, True]), [0, -1, -1, 1, 2])
    with pytest.raises(ValueError, match='would leave no reads'):
        prep.remove_reads_csr(csr, np.zeros(n, bool))
    with pytest.raises(ValueError, match='one entry per read'):
        prep.remove_reads_csr(csr, np.ones(n + 1, bool))
    with pytest.raises(ValueError, match='one entry per read'):
        prep.kept_data_rows(csr, np.ones(n - 1, bool))
    mine, my_ranks = prep.remove_reads_csr(csr, np.ones(n, bool))
    same_columns(mine, csr)
    np.testing.assert_array_equal(my_ranks, np.arange(n))


def test_the_oracle_on_the_compacted_csr_is_the_oracle_on_the_smaller_frame():
    """ties_600 with every third read removed: the CPU oracle gives the same edges (ranks, I, U), degrees and
    components for remove_reads_csr's CSR as for build_csr of the frame without those reads, although the
    compacted CSR keeps the old dense chromosome ids."""
    from oracle import oracle as O
    data, _, kw = host_prepare('ties_600')
    whole = data.csr()
    keep = np.arange(whole.n_reads) % 3 != 1
    mine, _ = prep.remove_reads_csr(whole, keep)
    fresh = build_csr(data.select(prep.kept_data_rows(whole, keep)))
    assert mine.n_chroms >= fresh.n_chroms
    cut = [float(x) for x in kw['jaccard_cutoffs'].split(',')]

    def run(c):
        cnt = np.diff(c.read_off)
        o = O.run_core(O.OracleCSR(c.read_off, c.iv_chrom, c.iv_start, c.iv_end, c.iv_aln, np.repeat(c.read_qlen2, cnt),
                                   np.repeat(c.read_nal, cnt), c.data_pos),
                       kw['overlap'], cut, kw['qlen_diff'], kw['n_alignment_diff'], 10, use_cap=False)
        return (sorted(zip(o['edge_a'].tolist(), o['edge_b'].tolist(), o['edge_I'].tolist(), o['edge_U'].tolist())),
                o['fwd'].tolist(), o['comp'].tolist())
    a, b = run(mine), run(fresh)
    assert len(a[0]) > 100 and a == b
