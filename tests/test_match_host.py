"""Matching new reads against the resident index, without a device: the CPU expectation the GPU tests use
(match_ref) agrees with the reference's own loop on a golden fixture, ReadMatches.clusters on hand-made
rows, and the argument checks of the Python layer."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import fixtures as fx
import match_ref as mr
import refharness
import search_ref as sr
from fslr_amd import _lib, bam_header, cluster
from fslr_amd._lib import SCORE_EDGE, SCORE_GATE
from fslr_amd.prep import IntervalData, pass_table
from oracle import oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = 'ties_600'                       # heavy start ties; max_fwd 9, so the golden graph is the uncapped one


def fixture_data():
    kw = fx.cli_options(FIXTURE)
    lens = bam_header.get_chromosome_lengths(fx.input_bam(FIXTURE))
    oc, _ = O.restate_prep(fx.input_bed(FIXTURE), lens, kw['cluster_mask'], kw['filter_false'])
    inv = np.argsort(oc.data_pos)
    read_of = np.repeat(np.arange(oc.n_reads), np.diff(oc.read_off))
    data = IntervalData(chrom=oc.chrom[inv], start=oc.start[inv], end=oc.end[inv], aln_size=oc.aln[inv],
                        qcode=read_of[inv], qnames=np.asarray(oc.qnames, dtype=object), n_alignments=oc.nal[inv],
                        qlen2=oc.qlen2[inv], middle=(oc.start[inv] + oc.end[inv]) // 2,
                        index=np.arange(inv.size, dtype=np.int64))
    return kw, data


def test_reference_agrees_with_the_reference_loop():
    """Every resident read r of the fixture as the query with exclude = r: its candidates come in the
    order the stand-in's search_values gives the loop (cluster.py:197-208), and its EDGE partners of
    rank > r are r's forward edges in the golden (uncapped) graph, with the golden Jaccard."""
    assert fx.meta(FIXTURE)['stage']['max_fwd'] <= 10
    kw, data = fixture_data()
    csr = data.csr()
    n = csr.n_reads
    names = data.qnames[csr.read_qcode]
    dp = np.asarray(csr.data_pos, np.int64)
    reads = [[(int(data.chrom[k]), int(data.start[k]), int(data.end[k]), int(data.aln_size[k]))
              for k in dp[csr.read_off[r]:csr.read_off[r + 1]]] for r in range(n)]
    q = mr.Queries(reads, csr.read_qlen2, csr.read_nal, exclude=np.arange(n))
    # the loop's visiting order by the stand-in: one map per chromosome, filled in `data` order
    trees = {}
    for p, (c, s, e) in enumerate(zip(data.chrom.tolist(), data.start.tolist(), data.end.tolist())):
        trees.setdefault(c, refharness._IntervalMap()).add(s, e, p)
    read_of_pos = np.empty(len(data), np.int64)
    read_of_pos[dp] = np.repeat(np.arange(n), np.diff(csr.read_off))
    cands, _ = mr.candidates(data, csr, q)
    for r in range(n):
        seen, order = set(), []
        for c, s, e, _ in reads[r]:
            for p in trees[c].search_values(s, e):
                o = int(read_of_pos[p])
                if o not in seen:
                    seen.add(o)
                    order.append(o)
        assert cands[r].tolist() == order, r
    cut = [float(x) for x in kw['jaccard_cutoffs'].split(',')]
    off, partner, I, U, flags, counts, best = mr.match_ref(data, csr, q, kw['overlap'], kw['qlen_diff'],
                                                           kw['n_alignment_diff'], pass_table(cut), SCORE_EDGE)
    assert (flags & SCORE_EDGE).all() and (counts[:, 2] == np.diff(off)).all()
    qi = np.repeat(np.arange(n), np.diff(off))
    assert (partner != qi).all()                   # the excluded read never shows up
    fwd = partner > qi
    got = sorted([names[a], names[b], i / u] for a, b, i, u in
                 zip(qi[fwd].tolist(), partner[fwd].tolist(), I[fwd].tolist(), U[fwd].tolist()))
    want = sorted([a, b, j] for a, b, j in fx.stage(FIXTURE)['edges'])
    assert len(want) > 1000 and got == want
    # the backward rows are the same edges seen from the other side
    assert sorted(zip(partner[~fwd].tolist(), qi[~fwd].tolist())) == sorted(zip(qi[fwd].tolist(), partner[fwd].tolist()))
    has = counts[:, 2] > 0
    assert (best[~has] == -1).all() and has.any()
    for r in np.flatnonzero(has)[:50].tolist():
        rows = slice(off[r], off[r + 1])
        j = I[rows] / U[rows]
        assert best[r] == partner[rows][int(np.argmax(j))]     # argmax: the first of equal values


def hand_matches():
    # query 0: edges to 5, 2, 7 (7 gated only), 6; query 1: none; query 2: edges to 9, 9's clustermate 8, 3
    offsets = np.array([0, 4, 4, 7], np.int64)
    partner = np.array([5, 2, 7, 6, 9, 8, 3], np.int32)
    flags = np.array([3, 3, 1, 3, 3, 3, 3], np.uint8)
    I = np.array([2, 1, 1, 2, 3, 3, 1], np.int32)
    U = np.array([2, 3, 4, 2, 3, 4, 1], np.int32)
    counts = np.array([[4, 4, 3], [0, 0, 0], [3, 3, 3]], np.int32)
    return cluster.ReadMatches(offsets, partner, I, U, flags, counts, np.array([5, -1, 9], np.int32),
                               np.asarray(['qa', 'qb', 'qc'], dtype=object),
                               np.asarray([f'r{k}' for k in range(10)], dtype=object))


def test_clusters_on_hand_made_rows():
    m = hand_matches()
    #        rank 0  1  2  3  4  5  6  7  8  9
    labels = [0, 1, 2, 3, 2, 2, 6, 0, 8, 8]
    off, lab, join = m.clusters(np.asarray(labels, np.int32))
    assert off.tolist() == [0, 2, 2, 4]
    assert lab.tolist() == [2, 6, 8, 3]            # first-visit order; 5 and 2 share label 2; 7 is no edge
    assert join.tolist() == [2, -1, 3]
    # the same from a ClusterTable: singletons (cid -1) are components of their own
    cid = np.array([0, -1, 1, -1, 1, 1, -1, 0, 2, 2], np.int32)
    size = np.array([2, 1, 3, 1, 3, 3, 1, 2, 2, 2], np.int32)
    t = cluster.ClusterTable(cid, size, np.array([0, 2, 5, 7], np.int64), np.array([0, 7, 2, 4, 5, 8, 9], np.int32),
                             dict(n_clusters=3, n_nodes=7, max_size=3))
    off2, lab2, join2 = m.clusters(t)
    assert (off2.tolist(), lab2.tolist(), join2.tolist()) == (off.tolist(), lab.tolist(), join.tolist())
    f = m.to_frame()
    assert list(f.columns) == ['query', 'qname', 'jaccard_similarity', 'n_intersections']
    assert f['query'].tolist() == ['qa'] * 4 + ['qc'] * 3 and f['qname'].tolist()[:2] == ['r5', 'r2']
    assert f['jaccard_similarity'].tolist() == [i / u for i, u in zip(m.I.tolist(), m.U.tolist())]
    empty = cluster.ReadMatches(np.zeros(3, np.int64), *(np.zeros(0, np.int32),) * 3, np.zeros(0, np.uint8),
                                np.zeros((2, 3), np.int32), np.full(2, -1, np.int32), ['a', 'b'], m.qnames_by_rank)
    off, lab, join = empty.clusters(np.arange(10))
    assert off.tolist() == [0, 0, 0] and lab.size == 0 and join.tolist() == [-1, -1]
    assert empty.to_frame().shape == (0, 4)


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(['make', '-s', '-C', os.path.join(REPO, 'fslr_amd', 'csrc')], check=True)
    return _lib.load()


def test_match_symbols_reject_a_null_context(lib):
    for name in ('fslr_match_reads', 'fslr_match_rows', 'fslr_match_timings'):
        assert name in _lib.EXPORTED and hasattr(lib, name), name
    total = ctypes.c_int64(-1)
    assert lib.fslr_match_reads(None, None, None, 0, None, None, None, ctypes.byref(total)) == _lib.FSLR_ERR_INVALID
    assert lib.fslr_match_rows(None, None, None, None, None, 0) == _lib.FSLR_ERR_INVALID
    assert lib.fslr_match_timings(None, None) == _lib.FSLR_ERR_INVALID
    assert total.value == -1
    assert _lib.MATCH_SET == 256 and ctypes.sizeof(_lib.MatchQueries) == 16 + 8 * ctypes.sizeof(ctypes.c_void_p)


class _NoDevice:
    """A context that must not be reached: the Python layer refuses the call first."""

    def __getattr__(self, name):
        raise AssertionError(f'the device was asked for {name}')


def test_python_layer_argument_checks():
    data = sr.make_data([5, 2, 9, 2], [10, 20, 30, 40], [15, 25, 35, 45])
    idx = object.__new__(cluster.DeviceIntervalIndex)
    idx.source = idx.data = data
    idx.csr, idx.long, idx.ctx = data.csr(), None, _NoDevice()
    new = sr.make_data([2, 9], [12, 31], [22, 33])
    args = (0.8, [1, 0.5], 0.04, 0.25)
    with pytest.raises(ValueError, match='emit'):
        idx.match_reads(new, *args, emit='some')
    with pytest.raises(ValueError):                                    # min() of an empty cutoff list, cluster.py:188
        idx.match_reads(new, 0.8, [], 0.04, 0.25)
    with pytest.raises(ValueError, match='exclude'):
        idx.match_reads(new, *args, exclude=[0])
    with pytest.raises(IndexError, match='exclude'):
        idx.match_reads(new, *args, exclude=[0, 4])
    with pytest.raises(KeyError):
        idx.match_reads(new, *args, exclude=['q0', 'no such read'])
    long_read = sr.make_data([2] * 65, np.arange(65) * 10, np.arange(65) * 10 + 5, qcode=np.zeros(65, np.int64))
    with pytest.raises(ValueError, match='query read 0 has more than 64'):
        idx.match_reads(long_read, *args)
    idx.long = np.array([70], np.int32)
    with pytest.raises(NotImplementedError, match='64'):
        idx.match_reads(new, *args)
    with pytest.raises(NotImplementedError, match='rank processes'):
        cluster.MultiGpuIndex(data, 2).match_reads(new, *args)
    assert cluster.RowsIndex.match_reads is cluster.DeviceIntervalIndex.match_reads
    for name in ('match_reads', 'match_rows', 'match_timings'):
        assert callable(getattr(_lib.Context, name)), name
    # the binding's own shape checks come before the library is called
    c = object.__new__(_lib.Context)
    with pytest.raises(ValueError, match='read_qlen2'):
        c.match_reads([0, 1], [1, 2], [1], [0], [0], [5], [0], 0.96, 0.75, pass_table([1]))
    with pytest.raises(ValueError, match='one length'):
        c.match_reads([0, 1], [1], [1], [0], [0, 1], [5], [0], 0.96, 0.75, pass_table([1]))
    with pytest.raises(ValueError, match='exclude'):
        c.match_reads([0, 1], [1], [1], [0], [0], [5], [0], 0.96, 0.75, pass_table([1]), exclude=[1, 2])
