"""Batched pair scoring on the device (fslr_score_pairs / DeviceIntervalIndex.score_pairs): for arbitrary
ordered read pairs, exactly what the reference's pair predicates return (cluster.py:133-183, 216-219),
against its own known answers and the CPU oracle, at the kernel's lane-group widths (16, 32, 64)."""
import ctypes

import numpy as np
import pytest

import fixtures as fx
import search_ref as sr
from fslr_amd import _lib, cluster, synth
from fslr_amd._lib import SCORE_EDGE, SCORE_GATE, SCORE_ZD_GATE, SCORE_ZD_OVERLAP
from fslr_amd.prep import fold_overlap_threshold, pass_table
from oracle import oracle as O

pytestmark = pytest.mark.gpu

CUTOFFS = (1, 1, 0.66, 0.66, 0.66, 0.5)


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def upload(ctx, reads, pct, qlen2=None, nal=None):
    """``reads``: per read a list of (chrom, start, end, aln); thresholds folded for ``pct``.  No index."""
    n = len(reads)
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    flat = np.array([x for r in reads for x in r], np.int64).reshape(-1, 4)
    ctx.set_reads(off, np.full(n, 100, np.int32) if qlen2 is None else qlen2,
                  np.full(n, 3, np.int32) if nal is None else nal, flat[:, 0], flat[:, 1], flat[:, 2],
                  fold_overlap_threshold(flat[:, 3], pct), int(flat[:, 0].max()) + 1)


def oracle_pair(l1, l2, pct):
    """(I, U, zd) of overall_jaccard_similarity by the CPU oracle; a raise is (0, 0, True)."""
    try:
        return (*O.jaccard_lists(l1, l2, pct), False)
    except ZeroDivisionError:
        return 0, 0, True


def oracle_flags(I, U, zd, q1, q2, n1, n2, qd, nd, pt):
    """The flag byte the reference's predicates give the pair."""
    try:
        flags = 0 if O.lengths_differ(q1, q2, n1, n2, qd, nd) else SCORE_GATE
    except ZeroDivisionError:
        flags = SCORE_ZD_GATE
    if zd:
        return flags | SCORE_ZD_OVERLAP
    if flags & SCORE_GATE and I > 0 and pt.reshape(-1, _lib.PASS_STRIDE)[I - 1, U - 1]:
        flags |= SCORE_EDGE
    return flags


# ------------------------------------------------------------------ 1. the reference's Jaccard KATs
def kat_reads():
    kats = fx.kats()['jaccard']
    reads = []
    for t, k in enumerate(kats):
        base = 10_000 + t * 10_000
        for lst in (k['a'], k['b']):
            reads.append([(c, s + base, e + base, a) for c, s, e, a in lst])
    return kats, reads


def test_kat_jaccard(ctx):
    """Every Jaccard KAT as the pair (2t, 2t + 1) and reversed: I == n_i and I / U == j, n_i == 0 included;
    a ZeroDivisionError of the reference is the ZD_OVERLAP flag with I = U = 0."""
    kats, reads = kat_reads()
    assert len(kats) == 3005
    checked = zd_seen = zero_seen = 0
    for pct in sorted({k['pct'] for k in kats}):
        upload(ctx, reads, pct)
        ts = np.array([t for t, k in enumerate(kats) if k['pct'] == pct])
        a, b = np.concatenate([2 * ts, 2 * ts + 1]), np.concatenate([2 * ts + 1, 2 * ts])
        I, U, flags = ctx.score_pairs(a, b, 1.0, 1.0, pass_table([0.0]))
        for m, t in enumerate(ts.tolist()):
            k = kats[t]
            for pos, (l1, l2) in ((m, (k['a'], k['b'])), (m + ts.size, (k['b'], k['a']))):
                wi, wu, zd = oracle_pair(l1, l2, pct)
                got = (int(I[pos]), int(U[pos]), bool(flags[pos] & SCORE_ZD_OVERLAP))
                assert got == (wi, wu, zd), (t, k, pos >= ts.size, got)
                # qlen2 and n_alignments are equal: the gate passes; cutoff 0: an edge iff I > 0
                assert int(flags[pos]) & ~SCORE_ZD_OVERLAP == (SCORE_GATE | (SCORE_EDGE if wi > 0 else 0)), (t, k)
            fi, fu, fz = int(I[m]), int(U[m]), bool(flags[m] & SCORE_ZD_OVERLAP)
            if 'raises' in k:
                assert fz and (fi, fu) == (0, 0), (t, k)
                zd_seen += 1
            elif not fz:                                # (an aln_size == 0 case the walk never reaches included)
                assert fi == k['n_i'] and (fi / fu if fu else 0) == k['j'], (t, k, fi, fu)
                zero_seen += k['n_i'] == 0
            checked += 1
    assert checked == len(kats) and zd_seen >= 1 and zero_seen > 100


# ------------------------------------------------------------------ 2. the gate's KATs
def gate_kats():
    """The lengths KATs the upload accepts (qlen2 >= 0, n_alignments in [0, 2^24)) and the skipped count."""
    kats = fx.kats()['lengths']
    ok = [k for k in kats if min(k['q1'], k['q2'], k['n1'], k['n2']) >= 0 and max(k['n1'], k['n2']) < (1 << 24)
          and max(k['q1'], k['q2']) < (1 << 31)]
    return ok, len(kats) - len(ok)


def test_kat_lengths(ctx):
    kats, skipped = gate_kats()
    assert len(kats) + skipped == 3007 and skipped < 0.01 * 3007
    n = 2 * len(kats)
    q = np.array([v for k in kats for v in (k['q1'], k['q2'])], np.int32)
    nal = np.array([v for k in kats for v in (k['n1'], k['n2'])], np.int32)
    upload(ctx, [[(0, 10 * r, 10 * r + 5, 5)] for r in range(n)], 0.8, q, nal)
    raised = 0
    for qd, nd in sorted({(k['qd'], k['nd']) for k in kats}):
        ts = np.array([t for t, k in enumerate(kats) if (k['qd'], k['nd']) == (qd, nd)])
        _, _, flags = ctx.score_pairs(2 * ts, 2 * ts + 1, 1 - qd, 1 - nd, pass_table(CUTOFFS))
        for t, f in zip(ts.tolist(), flags.tolist()):
            k = kats[t]
            if 'raises' in k:
                assert f & SCORE_ZD_GATE and not f & SCORE_GATE, k
                raised += 1
            else:
                assert not f & SCORE_ZD_GATE and bool(f & SCORE_GATE) == (not k['differ']), k
    assert raised >= 5


# ------------------------------------------------------------------ 3. lane-group boundaries
LENGTHS = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64)


def boundary_reads():
    """One read per length, dense on two chromosomes (a row has several candidate columns); the
    64-interval read holds an aln_size == 0 interval at row / column 57."""
    rng = np.random.default_rng(8)
    reads = []
    for L in LENGTHS:
        s = rng.integers(0, 200, L)
        ln = rng.integers(85, 115, L)
        reads.append([(int(c), int(a), int(a + w), int(w)) for c, a, w in zip(rng.integers(0, 2, L), s, ln)])
    c, s, e, _ = reads[-1][57]
    reads[-1][57] = (c, s, e, 0)
    qlen2 = rng.integers(900, 1100, len(LENGTHS)).astype(np.int32)
    nal = rng.integers(3, 6, len(LENGTHS)).astype(np.int32)
    return reads, qlen2, nal


def boundary_expected(reads, qlen2, nal, a, b, pt):
    out = []
    for x, y in zip(a.tolist(), b.tolist()):
        I, U, zd = oracle_pair(reads[x], reads[y], 0.8)
        out.append((I, U, oracle_flags(I, U, zd, qlen2[x], qlen2[y], nal[x], nal[y], 0.04, 0.25, pt)))
    return out


def test_lane_group_boundaries(ctx):
    reads, qlen2, nal = boundary_reads()
    n = len(reads)
    upload(ctx, reads, 0.8, qlen2, nal)
    order = np.random.default_rng(9).permutation(n * n)
    a, b = (order // n).astype(np.int32), (order % n).astype(np.int32)
    pt = pass_table(CUTOFFS)
    want = boundary_expected(reads, qlen2, nal, a, b, pt)
    I, U, flags = ctx.score_pairs(a, b, 1 - 0.04, 1 - 0.25, pt)
    got = list(zip(I.tolist(), U.tolist(), flags.tolist()))
    for k in range(n * n):
        assert got[k] == want[k], (LENGTHS[a[k]], LENGTHS[b[k]], got[k], want[k])
    assert sum(w[0] >= 8 for w in want) >= 20
    assert any(w[2] & SCORE_ZD_OVERLAP for w in want) and any(w[2] & SCORE_EDGE for w in want)
    # a late aln_size == 0 column that the walk never reaches leaves the values
    assert any(not w[2] & SCORE_ZD_OVERLAP for w, y in zip(want, b.tolist()) if LENGTHS[y] == 64)
    # one pair per call: a pair's result does not depend on its neighbours in the wave
    for k in range(n * n):
        i1, u1, f1 = ctx.score_pairs(a[k:k + 1], b[k:k + 1], 1 - 0.04, 1 - 0.25, pt)
        assert (int(i1[0]), int(u1[0]), int(f1[0])) == got[k], (k, LENGTHS[a[k]], LENGTHS[b[k]])


# ------------------------------------------------------------------ 4. consistency with the query
def consistency_pairs(n, ea, eb, rng, total=200_000):
    """Every edge as (lower, higher), rank neighbours (r, r + d) for d = 1 .. 4 and random a < b."""
    near_a = np.concatenate([np.arange(n - d) for d in range(1, 5)])
    near_b = np.concatenate([np.arange(d, n) for d in range(1, 5)])
    m = max(total - ea.size - near_a.size, 1000)
    ra, rb = rng.integers(0, n, m), rng.integers(0, n, m)
    keep = ra != rb
    ra, rb = np.minimum(ra, rb)[keep], np.maximum(ra, rb)[keep]
    a = np.concatenate([np.minimum(ea, eb), near_a, ra]).astype(np.int32)
    b = np.concatenate([np.maximum(ea, eb), near_b, rb]).astype(np.int32)
    return a, b


def consistency_input():
    """synth reads in clusters of copies (every pair inside one is an edge); every seventh read gets half
    the query length and twice the alignments, so the gate rejects its pairs with the cluster's other
    reads: rank neighbours that share intervals (I > 0) and are no edge."""
    csr = synth.generate(20_000, 16, 31).interval_data().csr()
    odd = np.arange(csr.n_reads) % 7 == 3
    csr.read_qlen2[odd] = np.maximum(csr.read_qlen2[odd] // 2, 1)
    csr.read_nal[odd] = 2 * csr.read_nal[odd] + 1
    return csr


def test_consistent_with_the_query(ctx):
    csr = consistency_input()
    n = csr.n_reads
    pt = pass_table(CUTOFFS)
    ctx.load_csr(csr, fold_overlap_threshold(csr.iv_aln, 0.8))
    ctx.reserve_edges(max(1 << 16, 12 * n))
    ctx.build_index()
    st = ctx.run_query(1 - 0.04, 1 - 0.25, pt, edge_threshold=1 << 30)      # uncapped: no read reaches it
    ctx.components()

    def state():                                    # the edges as they lie in HBM, labels, degrees
        return (*ctx.edges(st['n_edges']), ctx.labels(), ctx.fwd_degree())
    before = state()
    order = np.lexsort((before[1], before[0]))
    ea, eb, eI, eU = (x[order] for x in before[:4])
    assert ea.size >= 1000 and (ea < eb).all()
    a, b = consistency_pairs(n, ea, eb, np.random.default_rng(3))
    assert 150_000 <= a.size <= 250_000
    I, U, flags = ctx.score_pairs(a, b, 1 - 0.04, 1 - 0.25, pt)
    key = a.astype(np.int64) * n + b
    ekey = ea.astype(np.int64) * n + eb
    in_graph = np.isin(key, ekey)
    edge = (flags & SCORE_EDGE) != 0
    np.testing.assert_array_equal(edge, in_graph)
    assert in_graph[:ea.size].all() and int(in_graph.sum()) >= 1000
    np.testing.assert_array_equal(I[:ea.size], eI)
    np.testing.assert_array_equal(U[:ea.size], eU)
    assert int(((I > 0) & ~in_graph).sum()) >= 1000
    assert not (flags & (SCORE_ZD_GATE | SCORE_ZD_OVERLAP)).any()
    after = state()
    for x, y in zip(before, after):
        np.testing.assert_array_equal(x, y)


# ------------------------------------------------------------------ 5. state and errors
def small_index(ctx=None):
    data = synth.generate(2000, 16, 11).interval_data()
    return cluster.build_interval_trees(data, ctx=ctx)


ARGS = (0.8, CUTOFFS, 0.04, 0.25)


def test_empty_batch_and_bad_ranks(ctx):
    idx = small_index(ctx)
    n = idx.csr.n_reads
    r = idx.score_pairs([], [], *ARGS)
    assert len(r) == 0 and r.I.dtype == np.int32 and r.jaccard.dtype == np.float64 and r.to_frame().shape == (0, 6)
    I, U, flags = ctx.score_pairs(np.zeros(0, np.int32), np.zeros(0, np.int32), 0.96, 0.75, pass_table(CUTOFFS))
    assert I.size == U.size == flags.size == 0
    p = ctx._params(0.96, 0.75, pass_table(CUTOFFS), 0)
    vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    for bad, where in ((-1, 'b[2]'), (n, 'a[1]')):
        a, b = np.array([0, 1, 2, 3], np.int32), np.array([1, 2, 3, 4], np.int32)
        (a if where[0] == 'a' else b)[int(where[2])] = bad
        I, U, flags = np.full(4, -7, np.int32), np.full(4, -7, np.int32), np.full(4, 77, np.uint8)
        rc = ctx._L.fslr_score_pairs(ctx._h, ctypes.byref(p), 4, vp(a), vp(b), vp(I), vp(U), vp(flags))
        assert rc == _lib.FSLR_ERR_INVALID
        msg = ctx._L.fslr_last_error(ctx._h).decode()
        assert where in msg and str(bad) in msg
        assert (I == -7).all() and (U == -7).all() and (flags == 77).all()
    with pytest.raises(IndexError):
        idx.score_pairs([0], [n], *ARGS)
    with pytest.raises(KeyError):
        idx.score_pairs(['no such read'], [idx.data.qnames[0]], *ARGS)


def test_no_reads_is_a_state_error():
    c = _lib.Context(0)
    try:
        with pytest.raises(_lib.FslrError, match=f'fslr error {_lib.FSLR_ERR_STATE}.*fslr_set_reads'):
            c.score_pairs([0], [0], 0.96, 0.75, pass_table(CUTOFFS))
    finally:
        c.close()


def test_long_read_index_is_refused():
    rng = np.random.default_rng(44)
    n = 400
    qcode = np.concatenate([np.zeros(70, np.int64), 1 + rng.integers(0, 100, n - 70)])
    start = rng.integers(0, 200, n) * 500
    data = sr.make_data(rng.integers(1, 3, n), start, start + rng.integers(50, 2500, n), qcode=qcode)
    idx = cluster.build_interval_trees(data)
    try:
        assert idx.long is not None
        with pytest.raises(NotImplementedError, match='64'):
            idx.score_pairs([0], [1], *ARGS)
        with pytest.raises(_lib.FslrError, match=f'fslr error {_lib.FSLR_ERR_INVALID}.*64'):
            idx.ctx.score_pairs([0], [1], 0.96, 0.75, pass_table(CUTOFFS))
    finally:
        idx.ctx.close()
    with pytest.raises(NotImplementedError, match='multi-GPU'):
        cluster.MultiGpuIndex(data, 2).score_pairs([0], [1], *ARGS)


def test_scoring_between_search_and_hits(ctx):
    idx = small_index(ctx)
    d = idx.data
    dense = idx._dense_chroms(d.chrom[:200])
    qs, qe = idx._coords(d.start[:200]), idx._coords(d.end[:200])
    want_off, want_hits = ctx.search(dense, qs, qe)
    total = ctx._search(dense, qs, qe, None)
    assert total == want_hits.size > 200
    idx.score_pairs(np.arange(500), np.arange(1, 501), *ARGS)
    hits = np.full(total, -7, np.int32)
    ctx._check(ctx._L.fslr_search_hits(ctx._h, hits.ctypes.data_as(ctypes.c_void_p), total))
    np.testing.assert_array_equal(hits, want_hits)


def test_qnames_and_ranks_agree(ctx):
    idx = small_index(ctx)
    n = idx.csr.n_reads
    rng = np.random.default_rng(12)
    a = np.concatenate([np.arange(n - 1), rng.integers(0, n, 1000)])
    b = np.concatenate([np.arange(1, n), rng.integers(0, n, 1000)])
    names = idx.data.qnames[idx.csr.read_qcode]
    r = idx.score_pairs(a, b, *ARGS)
    q = idx.score_pairs(list(names[a]), list(names[b]), *ARGS)
    for f in ('a', 'b', 'I', 'U', 'flags', 'jaccard', 'gate', 'edge', 'zero_division'):
        np.testing.assert_array_equal(getattr(r, f), getattr(q, f))
    assert r.edge.any() and (r.I[r.edge] > 0).all() and r.gate[r.edge].all() and r.gate.sum() > r.edge.sum()
    np.testing.assert_array_equal(r.jaccard[r.U > 0], (r.I / np.maximum(r.U, 1))[r.U > 0])
    assert (r.U == idx.csr.read_off[a + 1] - idx.csr.read_off[a] + idx.csr.read_off[b + 1] - idx.csr.read_off[b] - r.I).all()
    f = r.to_frame()
    assert list(f.columns) == ['query1', 'query2', 'jaccard_similarity', 'n_i', 'gate', 'edge']
    assert f['query1'].tolist() == list(names[a]) and f['n_i'].tolist() == r.I.tolist()
    # the thresholds follow overlap_cutoff: no overlap reaches 1.5 of an aln_size that spans its interval
    assert (fold_overlap_threshold(idx.csr.iv_aln, 1.5) > idx.csr.iv_end - idx.csr.iv_start).all()
    hi = idx.score_pairs(a, b, 1.5, CUTOFFS, 0.04, 0.25)
    assert (hi.I == 0).all() and not hi.edge.any() and (r.I > 0).any()
    np.testing.assert_array_equal(idx.score_pairs(a, b, *ARGS).I, r.I)


def test_raise_zero_division(ctx):
    data = sr.make_data([1, 1, 2, 2], [100, 110, 5000, 5010], [200, 210, 5100, 5110])
    data.aln_size[3] = 0
    idx = cluster.build_interval_trees(data, ctx=ctx)
    r = idx.score_pairs([0, 2, 3, 0], [1, 3, 2, 3], *ARGS)
    # calculate_overlap raises for the aln_size == 0 interval on its own chromosome only
    assert r.zero_division.tolist() == [False, True, True, False] and r.U.tolist()[3] == 2
    assert r.I.tolist()[:1] == [1] and r.I.tolist()[1:3] == [0, 0] and r.U.tolist()[1:3] == [0, 0]
    assert r.jaccard.tolist()[1:3] == [0.0, 0.0]
    with pytest.raises(ZeroDivisionError, match='pair 1'):
        idx.score_pairs([0, 2, 3], [1, 3, 2], *ARGS, raise_zero_division=True)
