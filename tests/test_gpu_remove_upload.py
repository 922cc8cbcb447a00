"""prep.remove_reads_csr on the device: a context given fslr_set_reads of the compacted CSR (old dense
chromosome ids, closed-up data positions) against a context given build_csr of the data list without the
removed reads' rows.  Edges (a, b, I, U), forward degrees, labels and the engine are compared exactly; the
search order (ties ranked by data position) shows the compacted data order."""
import numpy as np
import pytest

import match_ref as mr
from fslr_amd import _lib, prep, synth
from fslr_amd.prep import build_csr, fold_overlap_threshold, pass_table

pytestmark = pytest.mark.gpu

PCT, QD, ND = 0.8, 0.04, 0.25
PT = pass_table((1, 1, 0.66, 0.66, 0.66, 0.5))


@pytest.fixture
def ctxs():
    a, b = _lib.Context(0), _lib.Context(0)
    yield a, b
    a.close()
    b.close()


def graph(ctx, csr, engine):
    ctx.load_csr(csr, fold_overlap_threshold(csr.iv_aln, PCT))
    ctx.reserve_edges(max(1 << 16, 12 * csr.n_reads))
    ctx.build_index()
    st = ctx.run_query(1 - QD, 1 - ND, PT, engine=engine)
    a, b, I, U = ctx.edges(st['n_edges'])
    ctx.components()
    return sorted(zip(a.tolist(), b.tolist(), I.tolist(), U.tolist())), ctx.fwd_degree(), ctx.labels(), st['engine']


def compare(ctxs, data, keep, engine):
    whole = data.csr()
    mine, ranks = prep.remove_reads_csr(whole, keep)
    fresh = build_csr(data.select(prep.kept_data_rows(whole, keep)))
    ga, gb = graph(ctxs[0], mine, engine), graph(ctxs[1], fresh, engine)
    assert ga[0] == gb[0] and ga[3] == gb[3]
    np.testing.assert_array_equal(ga[1], gb[1])
    np.testing.assert_array_equal(ga[2], gb[2])
    # the same hits in the same order, each context asked in its own dense chromosome ids
    k = np.unique(np.linspace(0, mine.n_intervals - 1, min(300, mine.n_intervals)).astype(np.int64))
    (oa, ha), (ob, hb) = (c.search(s.iv_chrom[k], s.iv_start[k], s.iv_end[k]) for c, s in zip(ctxs, (mine, fresh)))
    np.testing.assert_array_equal(oa, ob)
    np.testing.assert_array_equal(ha, hb)
    return mine, fresh, ga


@pytest.mark.parametrize('engine', ['walk', 'sweep'])
def test_random_third_removed(ctxs, engine):
    data = synth.generate(300, 8, 3).interval_data()
    keep = np.random.default_rng(1).random(300) >= 0.3
    mine, _, g = compare(ctxs, data, keep, engine)
    assert g[3] == engine and len(g[0]) > 20 and 150 < mine.n_reads < 300


def test_a_middle_chromosome_left_empty(ctxs):
    """Tie runs on three chromosomes; every read on the middle one goes.  The compacted CSR keeps three ids: the
    emptied id answers no hits, the id above it still names its chromosome."""
    rng = np.random.default_rng(8)
    reads = [[(c, int(s) * 10, int(s) * 10 + 100, 100) for s in np.sort(rng.choice(8, int(rng.integers(1, 3))))]
             for c in (1, 2, 3) for _ in range(80)]
    data = mr.resident_data(reads, np.full(240, 1000), np.full(240, 3), shuffle_seed=8)
    whole = data.csr()
    keep = np.ones(whole.n_reads, bool)
    keep[np.repeat(np.arange(whole.n_reads), np.diff(whole.read_off))[whole.iv_chrom == 1]] = False
    keep[::7] = False
    mine, fresh, g = compare(ctxs, data, keep, 'auto')
    assert mine.n_chroms == 3 and fresh.n_chroms == 2 and not (mine.iv_chrom == 1).any() and len(g[0]) > 100
    q = lambda c: ctxs[0].search(np.full(1, c, np.int32), np.zeros(1, np.int32), np.full(1, 10 ** 6, np.int32))[1]
    assert q(1).size == 0 and q(2).size == int((mine.iv_chrom == 2).sum()) > 0
