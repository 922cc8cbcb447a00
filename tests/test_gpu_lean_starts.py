"""The lean index without a start column (index.hip: k_chrom_scatter<false> writes none, k_ranges<false>
takes the starts from the records, k_starts makes the column for the readers that want one).

Sweep windows against np.searchsorted (per 64-position tile, fslr_position_costs), sweep and walk
engines against the C oracle where a window leaves the LDS span of its block, at block, halo and
chromosome boundaries, and every reader of the start column after a lean build, on one context that
is rebuilt and reloaded in between (a validity flag left set would serve the previous column)."""
import dataclasses

import numpy as np
import pytest

import search_ref as sr
from fslr_amd import _lib, synth
from fslr_amd.prep import fold_overlap_threshold, pass_table
from oracle import oracle as O

pytestmark = pytest.mark.gpu

CUTOFFS = (1, 1, 0.66, 0.66, 0.66, 0.5)
QCUT, NCUT = 1 - 0.04, 1 - 0.25
BLOCK, HALO = 1024, 512        # k_ranges: sorted positions per block, forward halo of the lean flavour


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------ inputs and references
@dataclasses.dataclass
class Hand:
    """One interval per read, in start order: CSR index == data position == read rank."""
    chrom: np.ndarray
    start: np.ndarray
    end: np.ndarray
    qlen2: np.ndarray
    nal: np.ndarray
    n_chroms: int

    @property
    def n(self):
        return self.start.size

    @property
    def aln(self):
        return (self.end - self.start).astype(np.int64)

    def oracle(self):
        n = self.n
        return O.OracleCSR(np.arange(n + 1), self.chrom, self.start, self.end, self.aln, self.qlen2, self.nal,
                           np.arange(n))

    def load(self, ctx, overlap=0.8):
        n = self.n
        ctx.set_reads(np.arange(n + 1, dtype=np.int64), self.qlen2.astype(np.int32), self.nal.astype(np.int32),
                      self.chrom.astype(np.int32), self.start.astype(np.int32), self.end.astype(np.int32),
                      fold_overlap_threshold(self.aln, overlap), self.n_chroms, iv_data_pos=np.arange(n))


def hand(chrom, start, end, qlen2=None, nal=None):
    chrom, start, end = (np.asarray(x, np.int64) for x in (chrom, start, end))
    o = np.argsort(start, kind='stable')
    n = start.size
    q = np.full(n, 1000, np.int64) if qlen2 is None else np.asarray(qlen2, np.int64)
    m = np.full(n, 3, np.int64) if nal is None else np.asarray(nal, np.int64)
    return Hand(chrom[o], start[o], end[o], q[o], m[o], int(chrom.max()) + 1)


def expected_tiles(h, overlap=0.8):
    """The sweep windows by np.searchsorted: per sorted position q of chromosome [b, e) the positions
    p in (q, e) with start_p <= end_q - thr_q, summed / their reach maximised per 64-position tile."""
    order = np.argsort(h.chrom, kind='stable')
    c, s, e = h.chrom[order], h.start[order], h.end[order]
    thr = fold_overlap_threshold(h.aln, overlap).astype(np.int64)[order]
    assert (thr >= 1).all()
    win = np.zeros(h.n, np.int64)
    for ch in np.unique(c):
        b, z = np.searchsorted(c, ch, 'left'), np.searchsorted(c, ch, 'right')
        q = np.arange(b, z)
        up = b + np.searchsorted(s[b:z], e[b:z] - thr[b:z], side='right')
        win[b:z] = np.maximum(up - q - 1, 0)
    nt = (h.n + 63) // 64
    pad = nt * 64 - h.n
    tests = np.pad(win, (0, pad)).reshape(nt, 64).sum(1)
    reach = np.pad(np.arange(h.n) + win + 1, (0, pad)).reshape(nt, 64).max(1)
    return win, tests, reach


def edge_table(a, b, I, U):
    t = np.stack([np.asarray(x, np.int64) for x in (a, b, I, U)], 1)
    return t[np.lexsort(t.T[::-1])]


def oracle_edges(o):
    return edge_table(o['edge_a'], o['edge_b'], o['edge_I'], o['edge_U'])


def query(ctx, engine, cutoffs=CUTOFFS):
    st = ctx.run_query(QCUT, NCUT, pass_table(cutoffs), engine=engine)
    assert st['engine'] == engine
    return st


def check_query(ctx, engine, o, cutoffs=CUTOFFS):
    st = query(ctx, engine, cutoffs)
    np.testing.assert_array_equal(edge_table(*ctx.edges(st['n_edges'])), oracle_edges(o))
    np.testing.assert_array_equal(ctx.fwd_degree(), o['fwd'])
    return st


# ------------------------------------------------------------------ 1. a window past the halo
@pytest.fixture(scope='module')
def locus():
    """One chromosome: 700 short intervals, then 2500 long ones on seven starts, then 900 short ones.
    The locus' windows run to its end, up to 2500 positions: from the first block (positions 700 ..
    1023) far past the 1024 + 512 positions its LDS holds.  20 classes of (qlen2, n_alignments), any two
    apart by more than both cuts of the length gate, keep the edge list short."""
    k = np.arange(2500)
    cls = 10 * 2 ** (k % 20 // 2) * np.where(k % 2, 14, 10)                # 100, 140, 200, 280, ...
    start = np.r_[np.arange(700) * 7, np.sort(5000 + k % 7), 8000 + np.arange(900) * 7]
    end = np.r_[np.arange(700) * 7 + 5, np.sort(5000 + k % 7) + 1000 - k % 3, 8000 + np.arange(900) * 7 + 5]
    q = np.r_[np.full(700, 1000), cls, np.full(900, 1000)]
    h = hand(np.zeros(4100, np.int64), start, end, qlen2=q, nal=q)
    return h, O.run_core(h.oracle(), 0.8, (1.0,), 0.04, 0.25, use_cap=False)


def test_window_past_the_halo(ctx, locus):
    h, o = locus
    win, tests, reach = expected_tiles(h)
    assert win[700] == 2499 and 700 + win[700] + 1 > BLOCK + HALO     # leaves block 0's LDS span
    assert (win[BLOCK:2 * BLOCK] > HALO).all()                          # every window of block 1 too
    h.load(ctx)
    ctx.reserve_edges(1 << 20)
    ctx.build_index()
    got_tests, got_reach = ctx.position_costs()
    np.testing.assert_array_equal(got_tests, tests)
    np.testing.assert_array_equal(got_reach, reach)
    st = check_query(ctx, 'sweep', o, (1.0,))
    assert st['n_edges'] > 50_000
    check_query(ctx, 'walk', o, (1.0,))


# ------------------------------------------------------------------ 2. window boundaries
def three_chroms(seed):
    """3000 intervals (not a multiple of 1024) on 3 chromosomes of 1000 / 300 / 1700: the first
    boundary lies inside block 0, the second inside block 0's halo and block 1.  The last 40
    intervals of each chromosome are long, so an unclamped search would run into the next one."""
    rng = np.random.default_rng(seed)
    chrom, start, end = [], [], []
    for c, m in enumerate((1000, 300, 1700)):
        s = np.sort(rng.integers(0, 60_000, m))
        e = s + rng.integers(20, 600, m)
        e[-40:] = s[-40:] + 80_000
        e[::53] += 200_000                      # and a few long ones anywhere: windows of hundreds
        chrom += [c] * m
        start += s.tolist()
        end += e.tolist()
    q = rng.choice([1000, 1010, 2000], 3000)
    return hand(chrom, start, end, qlen2=q)


@pytest.fixture(scope='module')
def bounds():
    h = three_chroms(3)
    return h, O.run_core(h.oracle(), 0.8, CUTOFFS, 0.04, 0.25, use_cap=False)


def test_windows_at_block_and_chromosome_boundaries(ctx, bounds):
    h, o = bounds
    assert h.n == 3000 and h.n % BLOCK
    win, tests, reach = expected_tiles(h)
    assert win[960:1000].max() < 40 and win[:1000].max() > 300          # clamped at the chromosome's end
    assert (np.arange(1000, 1300) + win[1000:1300] + 1).max() == 1300   # reaches the boundary in the halo
    h.load(ctx)
    ctx.reserve_edges(1 << 20)
    ctx.build_index()
    got_tests, got_reach = ctx.position_costs()
    np.testing.assert_array_equal(got_tests, tests)
    np.testing.assert_array_equal(got_reach, reach)
    check_query(ctx, 'sweep', o)
    check_query(ctx, 'walk', o)


def test_fewer_than_64_intervals(ctx):
    rng = np.random.default_rng(9)
    s = np.sort(rng.integers(0, 3000, 41))
    h = hand(rng.integers(0, 2, 41), s, s + rng.integers(100, 2500, 41))
    o = O.run_core(h.oracle(), 0.8, CUTOFFS, 0.04, 0.25, use_cap=False)
    assert o['edge_a'].size > 10
    _, tests, reach = expected_tiles(h)
    h.load(ctx)
    ctx.reserve_edges(1 << 16)
    ctx.build_index()
    got_tests, got_reach = ctx.position_costs()
    np.testing.assert_array_equal(got_tests, tests)
    np.testing.assert_array_equal(got_reach, reach)
    check_query(ctx, 'sweep', o)
    check_query(ctx, 'walk', o)


# ------------------------------------------------------------------ 3. readers of the start column
def oracle_of(csr):
    cnt = np.diff(csr.read_off)
    return O.OracleCSR(csr.read_off, csr.iv_chrom, csr.iv_start, csr.iv_end, csr.iv_aln, np.repeat(csr.read_qlen2, cnt),
                       np.repeat(csr.read_nal, cnt), csr.data_pos)


@pytest.fixture(scope='module')
def pair_of_inputs():
    """Two inputs of about the same size from different seeds, each with its oracle results at overlaps
    0.8 and 0.98."""
    a = synth.generate(3000, 16, 11).interval_data().csr()
    b = synth.generate(3000, 16, 12).interval_data().csr()
    out = []
    for csr in (a, b):
        ref = {ov: O.run_core(oracle_of(csr), ov, CUTOFFS, 0.04, 0.25, use_cap=False) for ov in (0.8, 0.98)}
        assert not np.array_equal(oracle_edges(ref[0.8]), oracle_edges(ref[0.98]))
        out.append((csr, ref))
    assert not np.array_equal(oracle_edges(out[0][1][0.8]), oracle_edges(out[1][1][0.8]))
    return out


def search_case(csr, seed):
    """Queries over the stored intervals and the brute-force hits as CSR indices."""
    rng = np.random.default_rng(seed)
    ni = csr.iv_start.size
    d = {k: np.empty(ni, np.int64) for k in ('chrom', 'start', 'end')}
    d['chrom'][csr.data_pos] = csr.iv_chrom
    d['start'][csr.data_pos] = csr.iv_start
    d['end'][csr.data_pos] = csr.iv_end
    csr_of_data = np.empty(ni, np.int64)
    csr_of_data[csr.data_pos] = np.arange(ni)
    pick = rng.integers(0, ni, 300)
    qc = csr.iv_chrom[pick].astype(np.int64)
    qs = csr.iv_start[pick].astype(np.int64) - rng.integers(0, 3000, 300)
    qe = csr.iv_end[pick].astype(np.int64) + rng.integers(0, 3000, 300)
    qe[::3] = csr.iv_start[pick][::3]                            # qe == a stored start (its ties)
    off, pos = sr.brute_force(d['chrom'], d['start'], d['end'], qc, qs, qe)
    return (qc, qs, qe), off, csr_of_data[pos]


def coverage_case(csr, seed):
    rng = np.random.default_rng(seed)
    c, s, e = csr.iv_chrom.astype(np.int64), csr.iv_start.astype(np.int64), csr.iv_end.astype(np.int64)
    pick = rng.integers(0, s.size, 400)
    qc, qp = c[pick], np.where(rng.random(400) < 0.5, s[pick], e[pick]) + rng.integers(-2, 3, 400)
    qp = np.maximum(qp, 0)
    ks, ke, q = np.sort(c << 32 | s), np.sort(c << 32 | e), qc << 32 | qp
    return (c, s, e), (qc, qp), np.searchsorted(ks, q, side='right') - np.searchsorted(ke, q, side='right')


def reader_walk(ctx, csr, ref):
    check_query(ctx, 'walk', ref[0.8])


def reader_set_thresholds(ctx, csr, ref):
    ctx.set_thresholds(fold_overlap_threshold(csr.iv_aln, 0.98))         # k_swin over the start column
    try:
        check_query(ctx, 'sweep', ref[0.98])
    finally:
        ctx.set_thresholds(fold_overlap_threshold(csr.iv_aln, 0.8))
    check_query(ctx, 'sweep', ref[0.8])


def reader_search(ctx, csr, ref):
    q, off, hits = search_case(csr, 21)
    got_off, got_hits = ctx.search(*q)
    np.testing.assert_array_equal(got_off, off)
    np.testing.assert_array_equal(got_hits, hits)
    assert off[-1] > 1000
    np.testing.assert_array_equal(ctx.search_counts(*q), np.diff(off))


def reader_coverage(ctx, csr, ref):
    rows, q, want = coverage_case(csr, 22)
    ctx.coverage_build(*rows, csr.n_chroms)
    np.testing.assert_array_equal(ctx.coverage_at(*q), want)
    assert want.max() > 1


READERS = [reader_walk, reader_set_thresholds, reader_search, reader_coverage]


@pytest.mark.parametrize('reader', READERS, ids=lambda f: f.__name__[7:])
def test_reader_after_a_lean_build(ctx, pair_of_inputs, reader):
    """Lean build and sweep query, the reader, another lean build, the reader again; then the same on
    the second input (the context's buffers, and a flag left set, would carry over)."""
    for csr, ref in pair_of_inputs:
        ctx.load_csr(csr, fold_overlap_threshold(csr.iv_aln, 0.8))
        ctx.reserve_edges(1 << 20)
        for _ in range(2):
            ctx.build_index()
            check_query(ctx, 'sweep', ref[0.8])
            reader(ctx, csr, ref)
        ctx.build_index()
        reader(ctx, csr, ref)                                            # straight after a build, no query


@pytest.fixture(scope='module')
def capped_pair():
    """600 reads with runs of tied starts (the tie order decides which pairs a capped loop reaches) on
    one locus, then on two loci of 300; the cap of 10 binds on both.  Each with the oracle's reference loop."""
    n = 600
    k = np.arange(n)
    out = []
    for gap in (0, 4000):
        s = np.sort(5000 + k % 7 + (k >= 300) * gap)
        h = hand(np.zeros(n, np.int64), s, s + 1000 - k % 3, qlen2=np.full(n, 100))
        out.append((h, O.run_core(h.oracle(), 0.8, (1.0,), 0.04, 0.25, edge_threshold=10, use_cap=True)))
    assert not np.array_equal(oracle_edges(out[0][1]), oracle_edges(out[1][1]))
    return out


def test_cap_replay_after_a_lean_build(ctx, capped_pair):
    """The cap replay's backward ranges (k_ranges<true>) and its T-interval search read the start column."""
    for h, o in capped_pair:
        h.load(ctx)
        ctx.reserve_edges(h.n * h.n)
        for _ in range(2):
            ctx.build_index()
            query(ctx, 'sweep', (1.0,))
            cap = ctx.apply_edge_cap(10)
            assert cap['applied'] == 1 and cap['capped'] > 0
            ne = ctx.stats()['n_edges']
            np.testing.assert_array_equal(edge_table(*ctx.edges(ne)), oracle_edges(o))
            np.testing.assert_array_equal(ctx.fwd_degree(), o['fwd'])
            assert cap['max_fwd'] == o['stats']['max_fwd']


# ------------------------------------------------------------------ 4. more than 64 chromosomes
def test_more_than_64_chromosomes(ctx):
    """115 chromosome ids: the radix fallback (k_finish writes the start column) on the same context."""
    csr = synth.generate(6000, 16, 37).interval_data().csr()
    ch = csr.iv_chrom.astype(np.int64) * 5 + (csr.iv_start.astype(np.int64) // 1000) % 5
    _, dense = np.unique(ch, return_inverse=True)
    csr = dataclasses.replace(csr, iv_chrom=dense.astype(np.int32), n_chroms=int(dense.max()) + 1)
    assert csr.n_chroms > 64
    o = O.run_core(oracle_of(csr), 0.8, CUTOFFS, 0.04, 0.25, use_cap=False)
    ctx.load_csr(csr, fold_overlap_threshold(csr.iv_aln, 0.8))
    ctx.reserve_edges(1 << 20)
    ctx.build_index()
    check_query(ctx, 'sweep', o)
    check_query(ctx, 'walk', o)
    q, off, hits = search_case(csr, 23)
    got_off, got_hits = ctx.search(*q)
    np.testing.assert_array_equal(got_off, off)
    np.testing.assert_array_equal(got_hits, hits)
