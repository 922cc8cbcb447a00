"""Drop-in replacement of ``fslr/cluster.py`` whose hot path runs on MI355X.

Same function names, arguments and return shapes as the reference module
(/root/reference/fslr/cluster.py); the per-pair work of ``query_interval_trees``
and the connected components run in ``libfslr_hip.so`` (HIP, gfx950).  Host
stages are vectorised numpy/pandas with the reference's exact semantics.

Function map (reference file:line → here):
  keep_fillings              cluster.py:14-31    vectorised first/last drop + group span
  rename_chromosomes         cluster.py:34-43    chrN by N, others after (equality-only downstream)
  chrom_to_str               cluster.py:46-49
  calc_coverage              cluster.py:52-67    host drop-in; with device= / ctx=: DeviceCoverage, the sorted
                             (chrom, rstart) and (chrom, rend) keys in HBM (fslr_coverage_build), depths
                             computed for the positions asked for (device_coverage)
  filter_high_coverage       cluster.py:70-77    host drop-in; with device= / ctx=: the depth at every
                             (chrom, middle) in one device call (fslr_coverage_at)
  delete_false               cluster.py:80-86
  mask_sequences2            cluster.py:89-106   vectorised for IntervalData
  prepare_data               cluster.py:109-121  → IntervalData (sequence of IntervalItem)
  build_interval_trees       cluster.py:124-130  → DeviceIntervalIndex (HBM CSR + sorted index);
                             tree[chrom].search_values(start, end) (cluster.py:201) and batches of queries
  get_chromosome_lengths     cluster.py:173-175  own BGZF/BAM header reader (no pysam)
  calculate_overlap          cluster.py:133-136  host drop-in (Python floats)
  overall_jaccard_similarity cluster.py:140-170  host drop-in; batched on the device for arbitrary read
                             pairs: DeviceIntervalIndex.score_pairs (fslr_score_pairs)
  different_lengths_or_alignments cluster.py:178-183  host drop-in; the gate bit of score_pairs
  query_interval_trees       cluster.py:187-227  device pair kernel; returns (match_df, ClusterGraph)
  get_subgraphs              cluster.py:230-234  components ordered by min read rank; with ctx=: the sets from
                             the device member CSR (fslr_cluster_table); cluster_table gives the table itself
  choose_alignment           cluster.py:237-254  vectorised groupby/idxmax; with ctx=: the per-cluster argmax on
                             the device (fslr_choose_representatives)
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np
from ._lazy import pandas as pd

from . import bam_header, ingest, multi
from ._lib import (FSLR_MAX_L, FSLR_THR_ZERO_ALN, SCORE_EDGE, SCORE_GATE, SCORE_ZD_GATE, SCORE_ZD_OVERLAP,
                   Context, FslrError)
from .prep import (CSR, IntervalData, IntervalItem, build_csr, data_order, first_last_masks, fold_overlap_threshold,
                   group_span, has_long_reads, kept_data_rows, mask_keep, pass_table, remove_reads_csr, umax_table)

__all__ = ['IntervalItem', 'keep_fillings', 'rename_chromosomes', 'chrom_to_str', 'calc_coverage',
           'filter_high_coverage', 'delete_false', 'mask_sequences2', 'prepare_data', 'build_interval_trees',
           'get_chromosome_lengths', 'query_interval_trees', 'get_subgraphs', 'choose_alignment',
           'ClusterGraph', 'DeviceIntervalIndex', 'ChromosomeView', 'MultiGpuIndex', 'EdgeCapWarning',
           'calculate_overlap', 'overall_jaccard_similarity', 'different_lengths_or_alignments', 'PairScores',
           'PairMatching',
           'device_coverage', 'DeviceCoverage', 'ClusterTable', 'cluster_table', 'ClusterLoci',
           'ClusterJunctions', 'ClusterPaths', 'ClusterPathSegments', 'ClusterPathContainment',
           'ClusterCollapsedSegments']


class EdgeCapWarning(UserWarning):
    """The reference's result depends on an order this build cannot pin: n_alignments
    that differ between rows of one read (cluster.py:209 reads the row its search
    reaches first)."""


def _default_device() -> int:
    return int(os.environ.get('FSLR_DEVICE', os.environ.get('LOCAL_RANK', '0')))


# ------------------------------------------------------------------ host stages
def keep_fillings(bed_file: pd.DataFrame) -> pd.DataFrame:
    """cluster.py:14-31: drop the first and last row (file order) of every qname; add qlen2."""
    codes, uniq = ingest.factorize_qname(bed_file)
    first, last = first_last_masks(codes)
    keep = ~(first | last)
    out = bed_file[keep]
    kc = codes[keep]
    span = group_span(kc, out['qstart'].to_numpy(), out['qend'].to_numpy(), len(uniq))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        out['qlen2'] = span[kc]
    return out


def _chrom_key(name):
    if isinstance(name, str) and name[:3] == 'chr' and name[3:].isdigit():
        return (0, int(name[3:]))
    return (1, 0)


def rename_chromosomes(bed_file, chromosome_lengths, chromosome_mask):
    """cluster.py:34-43.  chrN → N-order ids, other names after (first-appearance order).

    Only equality of ids is used downstream, so this deterministic numbering is
    interchangeable with the reference's set-iteration order for non-chrN names.
    """
    names = list(pd.unique(bed_file['chrom']))
    order = sorted(range(len(names)), key=lambda i: (_chrom_key(names[i]), i))
    cmap = {names[i]: k + 1 for k, i in enumerate(order)}
    chr_lengths = {cmap.get(k): v for k, v in chromosome_lengths.items()}
    bed_file['chrom'] = bed_file['chrom'].map(cmap)
    mask = [cmap.get(x) if x != 'subtelomere' else x for x in chromosome_mask]
    return bed_file, chr_lengths, mask, cmap


def chrom_to_str(bed_df, chromosome_to_numeric_map):
    """cluster.py:46-49."""
    inv = {v: k for k, v in chromosome_to_numeric_map.items()}
    bed_df['chrom'] = bed_df['chrom'].map(inv)
    return bed_df


def _index_positions(pos, size, what='index'):
    """``pos`` as numpy resolves it as an index into an axis of ``size`` (scalar or per element): values in
    [-size, -1] wrap, anything outside [-size, size) raises IndexError at the first such element."""
    p = np.asarray(pos)
    if p.dtype.kind not in 'iu':
        raise IndexError('arrays used as indices must be of integer (or boolean) type')
    p = p.astype(np.int64)
    size = np.broadcast_to(np.asarray(size, np.int64), p.shape)
    bad = (p < -size) | (p >= size)
    if bad.any():
        k = int(np.argmax(bad))
        raise IndexError(f'{what} {int(p.flat[k])} is out of bounds for axis 0 with size {int(size.flat[k])}')
    return np.where(p < 0, p + size, p)


class _ChromDepth:
    """``cov[chrom]`` of a DeviceCoverage: reads like the reference's float64 array of ``length + 1``
    depths, computed on the device for the positions asked for."""
    dtype = np.dtype(np.float64)

    def __init__(self, cov, dense, size):
        self._cov, self._dense, self._size = cov, dense, size
        self.shape = (size,)

    def __len__(self):
        return self._size

    def _at(self, pos):
        return self._cov._depth_dense(np.full(pos.shape, self._dense, np.int32), pos.astype(np.int32))

    def __getitem__(self, p):
        if isinstance(p, slice):
            return self._at(np.arange(*p.indices(self._size), dtype=np.int64)).astype(np.float64)
        if isinstance(p, (int, np.integer)) and not isinstance(p, (bool, np.bool_)):
            return float(self._at(_index_positions([p], self._size))[0])
        p = np.asarray(p)
        if p.dtype.kind == 'b':
            raise TypeError('DeviceCoverage takes an int, a slice or an integer array')
        if p.size == 0:
            return np.zeros(p.shape, np.float64)
        return self._at(_index_positions(p.ravel(), self._size)).astype(np.float64).reshape(p.shape)


class DeviceCoverage:
    """What calc_coverage returns on the device path: reads like the reference's dict of per-chromosome
    float64 arrays (cluster.py:52-67) but holds only the sorted (chrom, rstart) and (chrom, rend) keys of
    the bed rows in HBM (fslr_coverage_build).  ``chrom in cov``, ``cov.keys()``, ``len(cov[chrom])`` and
    ``cov[chrom][p]`` for an int, a slice or an integer array work; ``depth_at`` is the batched form."""

    def __init__(self, ctx, keys, sizes, owns_ctx):
        self.ctx, self._keys, self._sizes, self._owns_ctx = ctx, list(keys), np.asarray(sizes, np.int64), owns_ctx
        self._ids = {k: i for i, k in enumerate(self._keys)}
        self._gen = ctx.coverage_gen
        self._int_keys = None
        if self._keys and all(isinstance(k, (int, np.integer)) and not isinstance(k, bool) for k in self._keys):
            ks = np.asarray(self._keys, np.int64)
            order = np.argsort(ks, kind='stable')
            self._int_keys = (ks[order], order)

    def close(self):
        """Closes the context when device_coverage made it (a caller's context stays open)."""
        if self._owns_ctx and self.ctx is not None:
            self.ctx.close()
        self.ctx = None

    def __contains__(self, chrom):
        return chrom in self._ids

    def __iter__(self):
        return iter(self._keys)

    def __len__(self):
        return len(self._keys)

    def keys(self):
        return self._ids.keys()

    def __getitem__(self, chrom):
        i = self._ids[chrom]                         # KeyError as the reference's dict lookup raises it
        return _ChromDepth(self, i, int(self._sizes[i]))

    def _depth_dense(self, dense, pos):
        if self.ctx is None:
            raise RuntimeError('this DeviceCoverage is closed')
        if self.ctx.coverage_gen != self._gen:
            raise RuntimeError("the context's coverage was rebuilt since this DeviceCoverage was made")
        return self.ctx.coverage_at(dense, pos)

    def _dense_ids(self, chrom):
        """Dense ids (int64) of chromosome labels, -1 where the coverage has none."""
        q = np.asarray(chrom)
        if self._int_keys is not None and q.dtype.kind in 'iu':
            ks, order = self._int_keys
            at = np.minimum(np.searchsorted(ks, q), ks.size - 1)
            return np.where(ks[at] == q, order[at], -1).astype(np.int64)
        return np.asarray([self._ids.get(v, -1) for v in q.tolist()], np.int64)

    def depth_at(self, chrom, pos):
        """``cov[chrom[k]][pos[k]]`` for every k in one device call, int32.  The errors are those of the
        element-by-element lookups: KeyError for a chromosome without coverage, IndexError for a position
        outside ``[-(length + 1), length]``, whichever the first offending element raises."""
        labels = np.asarray(chrom)
        p = np.asarray(pos)
        if labels.ndim != 1 or labels.shape != p.shape:
            raise ValueError('chrom and pos must be one-dimensional and of one length')
        if p.size and p.dtype.kind not in 'iu':
            raise IndexError('only integers, slices (`:`), ellipsis (`...`), numpy.newaxis (`None`) and integer or '
                             'boolean arrays are valid indices')
        p = p.astype(np.int64)
        dense = self._dense_ids(labels) if labels.size else np.zeros(0, np.int64)
        no_key = dense < 0
        size = self._sizes[np.where(no_key, 0, dense)] if self._sizes.size else np.zeros(p.shape, np.int64)
        bad = no_key | (p < -size) | (p >= size)
        if bad.any():
            k = int(np.argmax(bad))
            if no_key[k]:
                raise KeyError(labels.tolist()[k])
            raise IndexError(f'index {int(p[k])} is out of bounds for axis 0 with size {int(size[k])}')
        return self._depth_dense(dense.astype(np.int32), np.where(p < 0, p + size, p).astype(np.int32))


def device_coverage(bed_file, chromosome_lengths, device=None, ctx=None) -> DeviceCoverage:
    """calc_coverage (cluster.py:52-67) on the device.  The host does what the reference does before its
    arithmetic: rows whose chrom is no key of ``chromosome_lengths`` (or is missing) are dropped, the
    chromosomes that are left get dense ids in the groupby's order, and rstart / rend resolve as indices
    into an array of ``length + 1`` (negative values wrap, anything else outside raises IndexError) before
    anything is uploaded."""
    codes, uniq = pd.factorize(bed_file['chrom'], sort=True)          # groupby('chrom'): sorted keys, NaN dropped
    uniq = np.asarray(uniq, dtype=object).tolist()
    known = np.array([u in chromosome_lengths for u in uniq], dtype=bool)
    dense_of = np.cumsum(known) - 1
    keys = [u for u, k in zip(uniq, known) if k]
    sizes = np.array([int(chromosome_lengths[u]) + 1 for u in keys], np.int64)
    if (sizes < 0).any():
        raise ValueError('negative dimensions are not allowed')
    if (sizes > np.iinfo(np.int32).max).any():
        raise ValueError('the device coverage holds positions below 2**31 - 1')
    keep = codes >= 0
    keep[keep] = known[codes[keep]]
    dense = dense_of[codes[keep]]
    rs, re_ = bed_file['rstart'].to_numpy()[keep], bed_file['rend'].to_numpy()[keep]
    if dense.size and (rs.dtype.kind not in 'iu' or re_.dtype.kind not in 'iu'):
        raise IndexError('arrays used as indices must be of integer (or boolean) type')
    rs, re_ = rs.astype(np.int64), re_.astype(np.int64)
    size = sizes[dense] if dense.size else np.zeros(0, np.int64)
    bad_s, bad_e = (rs < -size) | (rs >= size), (re_ < -size) | (re_ >= size)
    if (bad_s | bad_e).any():
        # np.add.at raises in the reference's order: chromosome after chromosome, rstart before rend
        rows = np.flatnonzero(bad_s | bad_e)
        rows = rows[dense[rows] == dense[rows].min()]
        s_rows = rows[bad_s[rows]]
        value = rs[s_rows[0]] if s_rows.size else re_[rows[0]]
        raise IndexError(f'index {int(value)} is out of bounds for axis 0 with size {int(size[rows[0]])}')
    rs, re_ = np.where(rs < 0, rs + size, rs), np.where(re_ < 0, re_ + size, re_)
    own = ctx is None
    ctx = ctx or Context(_default_device() if device is None else device)
    try:
        ctx.coverage_build(dense, rs, re_, len(keys))
    except BaseException:
        if own:
            ctx.close()
        raise
    return DeviceCoverage(ctx, keys, sizes, own)


def calc_coverage(bed_file, chromosome_lengths, device=None, ctx=None):
    """cluster.py:52-67: per-chromosome +1/-1 coverage at rstart/rend, cumulative.  With ``device`` or
    ``ctx`` given: a DeviceCoverage (nothing of the genome's length is allocated)."""
    if device is not None or ctx is not None:
        return device_coverage(bed_file, chromosome_lengths, device=device, ctx=ctx)
    cov = {}
    for chrom, grp in bed_file.groupby('chrom'):
        if chrom not in chromosome_lengths:
            continue
        c = np.zeros(chromosome_lengths[chrom] + 1)
        np.add.at(c, grp['rstart'].to_numpy(), 1)
        np.add.at(c, grp['rend'].to_numpy(), -1)
        cov[chrom] = np.cumsum(c)
    return cov


def filter_high_coverage(data, bed_file, chromosome_lengths, threshold, device=None, ctx=None):
    """cluster.py:70-77.  (main.py:235 passes a DataFrame here, which fails in the
    reference exactly as it fails here: iterating a DataFrame yields column names.)
    With ``device`` or ``ctx`` given the depth at every ``(chrom, middle)`` comes from one device call."""
    if device is not None or ctx is not None:
        cov = device_coverage(bed_file, chromosome_lengths, device=device, ctx=ctx)
        try:
            if isinstance(data, IntervalData):
                return data.select(cov.depth_at(data.chrom, data.middle) <= threshold)
            data = list(data)
            mids = [aln.middle for aln in data]         # (a DataFrame's column names fail here, as above)
            keep = ~(cov.depth_at(np.asarray([aln.chrom for aln in data]), np.asarray(mids)) > threshold)
            return [aln for aln, k in zip(data, keep.tolist()) if k]
        finally:
            cov.close()
    cov = calc_coverage(bed_file, chromosome_lengths)
    if isinstance(data, IntervalData):
        keep = np.array([cov[c][m] <= threshold for c, m in zip(data.chrom.tolist(), data.middle.tolist())],
                        dtype=bool)
        return data.select(keep)
    return [aln for aln in data if not cov[aln.chrom][aln.middle] > threshold]


def delete_false(bed_file):
    """cluster.py:80-86."""
    return bed_file[~bed_file['qname'].str.contains('False')]


def mask_sequences2(read_alignments, mask, chromosome_lengths, threshold=500_000):
    """cluster.py:89-106 (lines 104-105 can never fire: len==1 and >=4)."""
    if not mask:
        return read_alignments
    if isinstance(read_alignments, IntervalData):
        keep = mask_keep(read_alignments.chrom, read_alignments.start, read_alignments.end, mask,
                         chromosome_lengths, threshold)
        return read_alignments.select(keep)
    long_ = {k: v for k, v in chromosome_lengths.items() if v > 1_000_000}
    out = []
    for a in read_alignments:
        if a.chrom in mask:
            continue
        if 'subtelomere' in mask and a.chrom in long_ and (a.start < threshold or long_[a.chrom] - a.end < threshold):
            continue
        out.append(a)
    return out


def prepare_data(bed_df, cluster_mask, chromosome_lengths, threshold=500_000) -> IntervalData:
    """cluster.py:109-121 → IntervalData in ``sort_values('start')`` order, masked."""
    rs = bed_df['rstart'].to_numpy()
    re_ = bed_df['rend'].to_numpy()
    start = np.minimum(rs, re_)
    end = np.maximum(rs, re_)
    aln = bed_df['aln_size'].to_numpy()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        bed_df['start'] = start
        bed_df['end'] = end
        bed_df['middle'] = aln // 2 + start
    order = data_order(start)
    codes, uniq = ingest.factorize_qname(bed_df)
    chrom = bed_df['chrom'].to_numpy()
    if chrom.dtype.kind not in 'iu':                    # not renamed (rename_chromosomes not called)
        chrom = pd.factorize(bed_df['chrom'], sort=False)[0]
    if cluster_mask:
        # mask_sequences2 (cluster.py:89-106) is a per-interval predicate applied to the sorted list:
        # evaluated before the sort, one gather does both
        keep = mask_keep(np.asarray(chrom, np.int64), np.asarray(start, np.int64), np.asarray(end, np.int64),
                         cluster_mask, chromosome_lengths, threshold)
        order = order[keep[order]]
    cols = ingest.gather_columns([chrom, start, end, aln, codes, bed_df['n_alignments'].to_numpy(),
                                  bed_df['qlen2'].to_numpy(), aln // 2 + start], order)
    c, s, e, a, q, nal, ql2, mid = cols
    ix = bed_df.index.to_numpy()[order]
    return IntervalData(chrom=c, start=s, end=e, aln_size=a, qcode=q, qnames=np.asarray(uniq, dtype=object),
                        n_alignments=nal, qlen2=ql2, middle=mid, index=ix)


def get_chromosome_lengths(bam_path):
    """cluster.py:173-175 (BAM header reference dictionary)."""
    return bam_header.get_chromosome_lengths(bam_path)


# ------------------------------------------------------------------ pair predicates (host drop-ins)
def calculate_overlap(interval1, interval2):
    """cluster.py:133-136: the span the two intervals share (never below 0) as a fraction of each one's
    aln_size; the smaller fraction.  Python floats; an aln_size of 0 raises ZeroDivisionError."""
    shared = max(0, min(interval1.end, interval2.end) - max(interval1.start, interval2.start))
    return min(shared / interval1.aln_size, shared / interval2.aln_size)


def overall_jaccard_similarity(l1, l2, l2_comparisons, percentage, min_threshold):
    """cluster.py:140-170: ``(I / U, I)`` of the first-fit matching of two interval lists.  Rows of ``l1``
    in order; a row takes the first column of ``l2`` not yet taken that lies on its chromosome with
    ``calculate_overlap >= percentage``; U = len(l1) + len(l2) - I.  ``l2_comparisons`` is the caller's
    scratch: its first len(l2) entries are cleared, then set to 1 where a column was taken.  An empty
    list gives ``(0, 0)``.  ``min_threshold`` is accepted and unused (the reference's branch on it,
    :162-163, has no effect)."""
    if not l1 or not l2:
        return 0, 0
    n_cols = len(l2)
    l2_comparisons[:n_cols] = 0
    n_i = 0
    for row in l1:
        for j in range(n_cols):
            if l2_comparisons[j]:
                continue
            col = l2[j]
            if row.chrom == col.chrom and calculate_overlap(row, col) >= percentage:
                l2_comparisons[j] = 1
                n_i += 1
                break
    union = len(l1) + n_cols - n_i
    if union == 0:
        return 0, 0
    return n_i / union, n_i


def different_lengths_or_alignments(itv1, itv2, qlen_diff, diff):
    """cluster.py:178-183: False when the smaller qlen2 is at least ``1 - qlen_diff`` of the larger, or
    (tested second) the smaller n_alignments at least ``1 - diff`` of the larger; True otherwise.
    Python floats; a larger value of 0 raises ZeroDivisionError."""
    if min(itv1.qlen2, itv2.qlen2) / max(itv1.qlen2, itv2.qlen2) >= 1 - qlen_diff:
        return False
    if min(itv1.n_alignments, itv2.n_alignments) / max(itv1.n_alignments, itv2.n_alignments) >= 1 - diff:
        return False
    return True


class PairScores:
    """DeviceIntervalIndex.score_pairs' result, one entry per input pair in input order: ``a``, ``b`` (read
    ranks), ``I``, ``U`` (overall_jaccard_similarity's intersection and union), ``jaccard`` (float64 I / U,
    0.0 where U == 0), ``gate`` (different_lengths_or_alignments is False), ``edge`` (the pair loop would
    add the edge, cluster.py:216-221), ``zero_division`` (the reference raises for this pair: I = U = 0
    where calculate_overlap does) and the raw ``flags`` (fslr_hip.h FSLR_SCORE_*).  ``matching`` is None
    unless the pairs were scored with ``matching=True`` (a PairMatching)."""

    def __init__(self, a, b, I, U, flags, qnames_by_rank, matching=None):
        self.a, self.b, self.I, self.U, self.flags = a, b, I, U, flags
        self.qnames_by_rank = qnames_by_rank
        self.matching = matching
        self.jaccard = np.divide(I, U, out=np.zeros(I.shape, np.float64), where=U != 0)
        self.gate = (flags & SCORE_GATE) != 0
        self.edge = (flags & SCORE_EDGE) != 0
        self.zero_division = (flags & (SCORE_ZD_GATE | SCORE_ZD_OVERLAP)) != 0

    def __len__(self):
        return int(self.I.shape[0])

    def to_frame(self):
        q = self.qnames_by_rank
        n = len(self)
        return pd.DataFrame({'query1': q[self.a] if n else np.zeros(0, object),
                             'query2': q[self.b] if n else np.zeros(0, object),
                             'jaccard_similarity': self.jaccard, 'n_i': self.I, 'gate': self.gate, 'edge': self.edge})


class PairMatching:
    """Which interval of query1's list took which interval of query2's in the first-fit (fslr_pair_matching):
    pair k's rows are ``offsets[k]:offsets[k + 1]`` of ``i`` (index into query1's list, ascending) and ``j``
    (index into query2's list); I[k] rows, none for a pair whose overlap raised ZeroDivisionError."""

    def __init__(self, scores, offsets, i, j, intervals):
        self.offsets, self.i, self.j = offsets, i, j
        self._scores, self._intervals = scores, intervals

    def __len__(self):
        return int(self.i.shape[0])

    def pair_of_row(self) -> np.ndarray:
        """The input pair (its position) of every row."""
        return np.repeat(np.arange(self.offsets.shape[0] - 1, dtype=np.int64), np.diff(self.offsets))

    def to_frame(self):
        """One row per matched interval pair: ``query1``, ``query2``, ``i``, ``j`` and both intervals'
        ``chrom``, ``start``, ``end`` (the chromosome values the index was built with)."""
        s, k = self._scores, self.pair_of_row()
        q = s.qnames_by_rank
        n = len(self)
        chrom, start, end, read_off = self._intervals
        p1 = read_off[s.a[k]] + self.i
        p2 = read_off[s.b[k]] + self.j
        return pd.DataFrame({'query1': q[s.a[k]] if n else np.zeros(0, object),
                             'query2': q[s.b[k]] if n else np.zeros(0, object), 'i': self.i, 'j': self.j,
                             'chrom1': chrom[p1], 'start1': start[p1], 'end1': end[p1],
                             'chrom2': chrom[p2], 'start2': start[p2], 'end2': end[p2]})


class ReadMatches:
    """DeviceIntervalIndex.match_reads' result.  Query read q's rows are ``offsets[q]:offsets[q + 1]`` of
    ``partner`` (resident read ranks), ``I``, ``U`` and ``flags`` (fslr_hip.h FSLR_SCORE_*), in the order the
    reference's loop first meets the partners.  ``counts[q]`` = (candidates, gated, edges) over every candidate
    whatever was emitted; ``best[q]`` = the partner of the edge with the largest I / U (the earlier on ties),
    -1 without an edge.  ``query_names[q]`` names the query reads, ``qnames_by_rank`` the resident ones."""

    def __init__(self, offsets, partner, I, U, flags, counts, best, query_names, qnames_by_rank):
        self.offsets, self.partner, self.I, self.U, self.flags = offsets, partner, I, U, flags
        self.counts, self.best = counts, best
        self.query_names, self.qnames_by_rank = query_names, qnames_by_rank

    def __len__(self):
        return int(self.offsets.shape[0] - 1)

    def query_of_row(self) -> np.ndarray:
        """The query read (its index) of every row."""
        return np.repeat(np.arange(len(self), dtype=np.int64), np.diff(self.offsets))

    def to_frame(self):
        """One row per emitted pair: ``query`` (the new read), ``qname`` (the resident partner),
        ``jaccard_similarity`` (I / U as a Python float would be, 0.0 where U == 0), ``n_intersections``."""
        n = int(self.partner.shape[0])
        j = np.divide(self.I, self.U, out=np.zeros(n, np.float64), where=self.U != 0)
        names = np.asarray(self.query_names, dtype=object)
        return pd.DataFrame({'query': names[self.query_of_row()] if n else np.zeros(0, object),
                             'qname': self.qnames_by_rank[self.partner] if n else np.zeros(0, object),
                             'jaccard_similarity': j, 'n_intersections': self.I})

    def clusters(self, table_or_labels):
        """The resident components each query read's EDGE rows touch: ``(offsets int64[n + 1], labels
        int64[total], join int64[n])``.  ``labels[offsets[q]:offsets[q + 1]]`` are the distinct min-rank
        component labels among q's EDGE partners in first-visit order; ``join[q]`` is the label q would
        join (the smallest), -1 when q has no edge.  ``table_or_labels``: a ClusterTable, a graph with
        ``labels``, or the min-rank label vector itself.  Host numpy, one sort of the edge rows."""
        if isinstance(table_or_labels, ClusterTable):
            t = table_or_labels
            lab_of = np.where(t.cid >= 0, t.roots[np.maximum(t.cid, 0)] if t.n_clusters else 0,
                              np.arange(t.cid.shape[0])).astype(np.int64)
        else:
            lab_of = _labels_of(table_or_labels).astype(np.int64)
        n = len(self)
        rows = np.flatnonzero(self.flags & SCORE_EDGE)
        q = self.query_of_row()[rows]
        lab = lab_of[self.partner[rows]] if rows.size else np.zeros(0, np.int64)
        # the first row of every distinct (query, label): np.unique's first indices, back in row order
        _, first = np.unique(q * np.int64(max(lab_of.shape[0], 1)) + lab, return_index=True)
        first.sort()
        q, lab = q[first], lab[first]
        off = np.zeros(n + 1, np.int64)
        np.cumsum(np.bincount(q, minlength=n), out=off[1:])
        join = np.full(n, -1, np.int64)
        if q.size:
            lo = np.full(n, np.iinfo(np.int64).max)
            np.minimum.at(lo, q, lab)
            join = np.where(off[1:] > off[:-1], lo, -1)
        return off, lab, join


class ClusterLoci:
    """DeviceIntervalIndex.cluster_loci's result (fslr_cluster_loci): per cluster and chromosome the merged
    spans of the cluster's reads' intervals.  Cluster k's rows are ``off[k]:off[k + 1]`` of ``chrom`` (the
    chromosome values the index was built with), ``start``, ``end`` (end-inclusive, the largest end in the
    locus), ``n_intervals`` and ``n_reads`` (distinct reads among them); rows are ordered by (cluster, the
    index's dense chromosome id, start).  ``chrom_id`` keeps the dense ids."""

    def __init__(self, off, chrom, start, end, n_intervals, n_reads, chrom_id):
        self.off, self.chrom, self.start, self.end = off, chrom, start, end
        self.n_intervals, self.n_reads, self.chrom_id = n_intervals, n_reads, chrom_id

    def __len__(self):
        return int(self.start.shape[0])

    def cluster_of_row(self) -> np.ndarray:
        """The dense cluster id of every row."""
        return np.repeat(np.arange(self.off.shape[0] - 1, dtype=np.int64), np.diff(self.off))

    def to_frame(self):
        """One row per locus: ``cluster``, ``chrom``, ``start``, ``end``, ``n_intervals``, ``n_reads``."""
        return pd.DataFrame({'cluster': self.cluster_of_row(), 'chrom': self.chrom, 'start': self.start,
                             'end': self.end, 'n_intervals': self.n_intervals, 'n_reads': self.n_reads})


class ClusterJunctions:
    """DeviceIntervalIndex.cluster_junctions' result (fslr_cluster_junctions): the junctions between locus ends
    that each cluster's reads support.  Cluster k's rows are ``off[k]:off[k + 1]``.  A row joins end ``side_a``
    of locus ``locus_a`` to end ``side_b`` of locus ``locus_b`` (row indices of ``loci``, the ClusterLoci the
    call was made on; side 0 is a locus's left end, 1 its right end), with ``n_obs`` observations from
    ``n_reads`` distinct reads and the smallest and largest breakpoint seen on either side.  Rows are ordered by
    (locus_a * 2 + side_a, locus_b * 2 + side_b)."""

    COLUMNS = ('locus_a', 'side_a', 'locus_b', 'side_b', 'n_obs', 'n_reads', 'bp_a_min', 'bp_a_max', 'bp_b_min',
               'bp_b_max')

    def __init__(self, off, cols, loci):
        self.off, self.loci = off, loci
        for name, col in zip(self.COLUMNS, cols):
            setattr(self, name, col)

    def __len__(self):
        return int(self.locus_a.shape[0])

    def cluster_of_row(self) -> np.ndarray:
        """The dense cluster id of every row."""
        return np.repeat(np.arange(self.off.shape[0] - 1, dtype=np.int64), np.diff(self.off))

    def to_frame(self):
        """One row per junction: ``cluster, chrom_a, side_a, locus_a, bp_a_min, bp_a_max, chrom_b, side_b,
        locus_b, bp_b_min, bp_b_max, n_obs, n_reads`` (the chromosomes are the values the index was built with)."""
        ch = self.loci.chrom
        return pd.DataFrame({'cluster': self.cluster_of_row(),
                             'chrom_a': ch[self.locus_a], 'side_a': self.side_a, 'locus_a': self.locus_a,
                             'bp_a_min': self.bp_a_min, 'bp_a_max': self.bp_a_max,
                             'chrom_b': ch[self.locus_b], 'side_b': self.side_b, 'locus_b': self.locus_b,
                             'bp_b_min': self.bp_b_min, 'bp_b_max': self.bp_b_max,
                             'n_obs': self.n_obs, 'n_reads': self.n_reads})


class ClusterPaths:
    """DeviceIntervalIndex.cluster_paths' result (fslr_cluster_paths): the distinct read structures of each
    cluster.  Cluster k's rows are ``off[k]:off[k + 1]``.  A row is one path, the chain of pieces its reads walk:
    its tokens are ``locus[tok_off[row]:tok_off[row + 1]]`` (row indices of ``loci``, the ClusterLoci the call was
    made on) with ``rev`` beside them (1: the piece runs against the path's direction), ``n_reads`` reads of the
    cluster have it and ``first_read`` is the smallest rank among them.  A path is stored in the smaller of its two
    reading directions; ``flipped[read]`` says that the read walks it backwards, ``path_of_read[read]`` is its
    global row (-1 for a read alone).  Rows ascend lexicographically by ``locus * 2 + rev``, a prefix before its
    extensions.  ``read_names`` are the reads' qnames (or codes) by rank."""

    def __init__(self, off, tok_off, n_reads, first_read, locus, rev, path_of_read, flipped, loci, read_names):
        self.off, self.tok_off, self.n_reads, self.first_read = off, tok_off, n_reads, first_read
        self.locus, self.rev, self.path_of_read, self.flipped = locus, rev, path_of_read, flipped
        self.loci, self.read_names = loci, read_names

    def __len__(self):
        return int(self.n_reads.shape[0])

    def cluster_of_row(self) -> np.ndarray:
        """The dense cluster id of every row."""
        return np.repeat(np.arange(self.off.shape[0] - 1, dtype=np.int64), np.diff(self.off))

    def tokens(self, row):
        """``(locus, rev)`` of one row: its pieces in path order."""
        s = slice(int(self.tok_off[row]), int(self.tok_off[row + 1]))
        return self.locus[s], self.rev[s]

    def _path_in_cluster(self) -> np.ndarray:
        return np.arange(len(self), dtype=np.int64) - np.repeat(self.off[:-1], np.diff(self.off))

    def to_frame(self):
        """One row per path: ``cluster, path`` (0-based within its cluster), ``n_reads, n_loci`` (the pieces),
        ``first_read`` (its qname or code) and ``structure``, ``chrom:start-end:+`` (``-`` for a reversed piece)
        per piece joined by ``,`` (the chromosomes are the values the index was built with)."""
        lo = self.loci
        piece = [f'{c}:{s}-{e}:' for c, s, e in zip(lo.chrom.tolist(), lo.start.tolist(), lo.end.tolist())]
        toks = [piece[k] + '-+'[r == 0] for k, r in zip(self.locus.tolist(), self.rev.tolist())]
        to = self.tok_off.tolist()
        return pd.DataFrame({'cluster': self.cluster_of_row(), 'path': self._path_in_cluster(),
                             'n_reads': self.n_reads, 'n_loci': np.diff(self.tok_off),
                             'first_read': np.asarray(self.read_names)[self.first_read],
                             'structure': np.asarray([','.join(toks[a:b]) for a, b in zip(to[:-1], to[1:])], dtype=object)})

    def read_frame(self):
        """One row per read: ``qname, cluster, path`` (within its cluster; both -1 for a read alone), ``flipped``."""
        row = self.path_of_read.astype(np.int64)
        have = row >= 0
        safe = np.where(have, row, 0)
        if len(self):
            cl = np.where(have, self.cluster_of_row()[safe], -1)
            path = np.where(have, self._path_in_cluster()[safe], -1)
        else:
            cl = path = np.full(row.shape, -1, np.int64)
        return pd.DataFrame({'qname': np.asarray(self.read_names), 'cluster': cl, 'path': path, 'flipped': self.flipped})

    def dominant(self) -> np.ndarray:
        """Per cluster the global row with the most reads, ties to the first row."""
        return np.asarray([a + int(np.argmax(self.n_reads[a:b])) for a, b in zip(self.off[:-1].tolist(), self.off[1:].tolist())],
                          np.int64)


class ClusterPathSegments:
    """DeviceIntervalIndex.cluster_path_segments' result (fslr_cluster_path_segments): per piece of every row of
    ``paths`` (the ClusterPaths it was made on; slot ``tok_off[row] + piece``) the minimum, lower median and
    maximum of the reference start and end of the piece in the reads that walk this path, and per link between a
    piece and the next the same of the query-space gap (next piece's query start minus this piece's query end in
    the read's own order: negative = overlap / microhomology, positive = inserted sequence).  A row's last piece
    holds gap 0, 0, 0; without ``qend`` every gap is 0.  Nine int32 columns of ``n_tokens`` each."""

    NAMES = ('start_min', 'start_med', 'start_max', 'end_min', 'end_med', 'end_max', 'gap_min', 'gap_med', 'gap_max')

    def __init__(self, paths, start_min, start_med, start_max, end_min, end_med, end_max, gap_min, gap_med, gap_max):
        self.paths = paths
        self.start_min, self.start_med, self.start_max = start_min, start_med, start_max
        self.end_min, self.end_med, self.end_max = end_min, end_med, end_max
        self.gap_min, self.gap_med, self.gap_max = gap_min, gap_med, gap_max

    def __len__(self):
        return int(self.start_med.shape[0])

    def columns(self):
        """The nine columns in NAMES' order."""
        return tuple(getattr(self, k) for k in self.NAMES)

    def to_frame(self):
        """One line per piece: ``cluster, path`` (0-based within its cluster), ``piece`` (0-based within its path),
        ``chrom, start, end`` (the medians), ``strand`` ('-' for a reversed piece), ``n_reads`` of the path, then
        ``start_min, start_max, end_min, end_max, gap_min, gap, gap_max`` (gap = the median)."""
        p = self.paths
        n_pieces = np.diff(p.tok_off)
        row = np.repeat(np.arange(len(p), dtype=np.int64), n_pieces)
        piece = np.arange(len(self), dtype=np.int64) - np.repeat(p.tok_off[:-1], n_pieces)
        strand = np.where(p.rev == 0, '+', '-').astype(object)
        return pd.DataFrame({'cluster': p.cluster_of_row()[row], 'path': p._path_in_cluster()[row], 'piece': piece,
                             'chrom': np.asarray(p.loci.chrom)[p.locus], 'start': self.start_med, 'end': self.end_med,
                             'strand': strand, 'n_reads': p.n_reads[row],
                             'start_min': self.start_min, 'start_max': self.start_max,
                             'end_min': self.end_min, 'end_max': self.end_max,
                             'gap_min': self.gap_min, 'gap': self.gap_med, 'gap_max': self.gap_max})

    def structure(self, row) -> str:
        """The path of global row ``row`` as ClusterPaths.to_frame writes it, ``chrom:start-end:+`` per piece joined
        by ``,``, with the consensus (median) coordinates of the piece in place of the locus' span."""
        p = self.paths
        a, b = int(p.tok_off[row]), int(p.tok_off[row + 1])
        ch = np.asarray(p.loci.chrom)[p.locus[a:b]].tolist()
        return ','.join(f'{c}:{s}-{e}:' + '-+'[r == 0] for c, s, e, r in
                        zip(ch, self.start_med[a:b].tolist(), self.end_med[a:b].tolist(), p.rev[a:b].tolist()))


class ClusterPathContainment:
    """DeviceIntervalIndex.cluster_path_containment's result (fslr_cluster_path_containment): which rows of ``paths``
    (the ClusterPaths it was made on) are contiguous sub-chains of a longer row of their cluster, in either reading
    direction, and each row's support with those counted.  The pairs of inner row A are ``coff[A]:coff[A + 1]`` of
    ``outer`` (the containing row), ``offset`` (the smallest offset of A in it), ``rev`` (1: A lies there reverse
    complemented) and ``n_occ`` (its occurrences); pairs ascend by (inner, outer).  Per path row: ``n_inner`` rows
    it contains, ``support`` = its reads plus theirs, ``collapse_to`` = itself when nothing contains it (it is
    maximal), else the maximal row with the largest support among those that contain it (ties to the smaller row),
    ``collapsed_reads`` = the reads of a maximal row and of the rows that collapse to it, 0 for the others."""

    PAIR_NAMES = ('outer', 'offset', 'rev', 'n_occ')
    ROW_NAMES = ('n_inner', 'support', 'collapse_to', 'collapsed_reads')

    def __init__(self, paths, coff, outer, offset, rev, n_occ, n_inner, support, collapse_to, collapsed_reads):
        self.paths, self.coff = paths, coff
        self.outer, self.offset, self.rev, self.n_occ = outer, offset, rev, n_occ
        self.n_inner, self.support, self.collapse_to, self.collapsed_reads = n_inner, support, collapse_to, collapsed_reads

    def __len__(self):
        return int(self.outer.shape[0])

    def inner_of_pair(self) -> np.ndarray:
        """The inner row of every pair."""
        return np.repeat(np.arange(self.coff.shape[0] - 1, dtype=np.int64), np.diff(self.coff))

    def maximal(self) -> np.ndarray:
        """Per path row: nothing contains it."""
        return np.diff(self.coff) == 0

    def to_frame(self):
        """One line per containment pair: ``cluster, inner, outer`` (global path rows), ``offset, rev, n_occ``."""
        inner = self.inner_of_pair()
        cl = self.paths.cluster_of_row()[inner] if len(self) else np.zeros(0, np.int64)
        return pd.DataFrame({'cluster': cl, 'inner': inner, 'outer': self.outer, 'offset': self.offset,
                             'rev': self.rev, 'n_occ': self.n_occ})

    def paths_frame(self):
        """One line per path row: ``cluster, row`` (the global path row), ``n_tokens, n_reads, n_inner, support,
        maximal, collapse_to, collapsed_reads``."""
        p = self.paths
        return pd.DataFrame({'cluster': p.cluster_of_row(), 'row': np.arange(len(p), dtype=np.int64),
                             'n_tokens': np.diff(p.tok_off), 'n_reads': p.n_reads, 'n_inner': self.n_inner,
                             'support': self.support, 'maximal': self.maximal(), 'collapse_to': self.collapse_to,
                             'collapsed_reads': self.collapsed_reads})


class ClusterCollapsedSegments:
    """DeviceIntervalIndex.cluster_collapsed_segments' result (fslr_cluster_collapsed_segments): per piece of every
    MAXIMAL row of ``paths`` (slot ``tok_off[row] + piece``) the minimum, lower median and maximum of the reference
    start and end of the piece over all reads that collapse onto the row (``containment.collapse_to``), and per link
    between a piece and the next the same of the query-space gap.  A truncated read counts at the pieces it covers
    and nowhere else: ``n_cov`` intervals and ``n_link`` read links stand behind a slot.  The slots of rows that are
    not maximal hold 0 in every column; a row's last piece has ``n_link`` 0 and gap 0, 0, 0; without ``qend`` every
    gap is 0 and ``n_link`` is still filled.  Eleven int32 columns of ``n_tokens`` each.  ``paths`` is the
    ClusterPaths and ``containment`` the ClusterPathContainment the call stood on."""

    NAMES = ('n_cov', 'n_link', 'start_min', 'start_med', 'start_max', 'end_min', 'end_med', 'end_max',
             'gap_min', 'gap_med', 'gap_max')
    FRAME_COLUMNS = ('cluster', 'path', 'piece', 'chrom', 'start', 'end', 'strand', 'n_cov', 'start_min', 'start_max',
                     'end_min', 'end_max', 'gap_min', 'gap', 'gap_max', 'n_link', 'collapsed_reads')

    def __init__(self, paths, containment, n_cov, n_link, start_min, start_med, start_max, end_min, end_med, end_max,
                 gap_min, gap_med, gap_max):
        self.paths, self.containment = paths, containment
        self.n_cov, self.n_link = n_cov, n_link
        self.start_min, self.start_med, self.start_max = start_min, start_med, start_max
        self.end_min, self.end_med, self.end_max = end_min, end_med, end_max
        self.gap_min, self.gap_med, self.gap_max = gap_min, gap_med, gap_max

    def __len__(self):
        return int(self.n_cov.shape[0])

    def columns(self):
        """The eleven columns in NAMES' order."""
        return tuple(getattr(self, k) for k in self.NAMES)

    def to_frame(self):
        """One line per piece of every maximal row (FRAME_COLUMNS): ``cluster, path`` (0-based within its cluster),
        ``piece`` (0-based within its path), ``chrom`` (of the piece's loci row), ``start, end`` (the medians),
        ``strand`` ('-' for a reversed piece), ``n_cov``, ``start_min, start_max, end_min, end_max``, ``gap_min, gap,
        gap_max`` (gap = the median), ``n_link`` and ``collapsed_reads`` of the row."""
        p, ct = self.paths, self.containment
        n_pieces = np.diff(p.tok_off)
        row = np.repeat(np.arange(len(p), dtype=np.int64), n_pieces)
        piece = np.arange(len(self), dtype=np.int64) - np.repeat(p.tok_off[:-1], n_pieces)
        keep = np.asarray(ct.collapse_to, np.int64)[row] == row
        row = row[keep]
        strand = np.where(p.rev == 0, '+', '-').astype(object)
        return pd.DataFrame({'cluster': p.cluster_of_row()[row], 'path': p._path_in_cluster()[row], 'piece': piece[keep],
                             'chrom': np.asarray(p.loci.chrom)[p.locus][keep], 'start': self.start_med[keep],
                             'end': self.end_med[keep], 'strand': strand[keep], 'n_cov': self.n_cov[keep],
                             'start_min': self.start_min[keep], 'start_max': self.start_max[keep],
                             'end_min': self.end_min[keep], 'end_max': self.end_max[keep],
                             'gap_min': self.gap_min[keep], 'gap': self.gap_med[keep], 'gap_max': self.gap_max[keep],
                             'n_link': self.n_link[keep],
                             'collapsed_reads': np.asarray(ct.collapsed_reads, np.int64)[row]})


def _rev_bits(strand) -> np.ndarray:
    """uint8 0/1 of a strand column given as booleans, 0/1 or '+' / '-' ('-' and true values are 1)."""
    s = np.asarray(strand)
    if s.dtype.kind in 'USO':
        txt = s.astype(str)
        bad = ~((txt == '+') | (txt == '-'))
        if bad.any():
            raise ValueError(f"strand holds {txt[bad][0]!r}: booleans, 0/1 or '+' / '-' are taken")
        return (txt == '-').astype(np.uint8)
    return (s != 0).astype(np.uint8)


# ------------------------------------------------------------------ device stages
class DeviceIntervalIndex:
    """What build_interval_trees returns: the CSR in HBM plus the sorted interval index."""

    def __init__(self, data, device: int | None = None, ctx: Context | None = None):
        self.source = data                      # what the caller passed (query_interval_trees checks it)
        if not isinstance(data, IntervalData):
            # the reference's own prepare_data output: a list of IntervalItem (cluster.py:116-121)
            data = IntervalData.from_items(data)
        self.data = data
        self.csr = data.csr()
        self.ctx = ctx or Context(_default_device() if device is None else device)
        c = self.csr
        thr0 = np.where(c.iv_aln == 0, FSLR_THR_ZERO_ALN, 0).astype(np.int32)
        # reads of more than FSLR_MAX_L intervals: the library uploads them as FSLR_MAX_L-interval
        # chunks (fslr_set_reads_any); self.long = the real reads' lengths
        self.long = np.diff(np.asarray(c.read_off, np.int64)).astype(np.int32) if has_long_reads(c) else None
        if self.long is not None:
            self.ctx.load_csr_any(c, thr0)
        else:
            self.ctx.load_csr(c, thr0)
        self.ctx.build_index()

    # -- more reads for the resident set (fslr_append_reads) ------------------------
    def append(self, new_data):
        """Add the reads of ``new_data`` (prepare_data's result for the new rows, or the reference's item
        list) to the resident set on the device and rebuild the index.  The resident reads keep their ranks,
        the new ones follow in the order of ``build_csr(new_data)``; the `data` list becomes the stable merge
        of the two start-sorted lists (resident first on equal starts).  Only the new reads' columns go to
        the device; the host mirrors (``data``, ``csr``) are rebuilt by numpy concatenation, O(n + m).
        Afterwards ``self.data`` (also ``self.source``) is the merged IntervalData and ``self.csr`` the
        concatenated CSR with the merged data positions.  A read is a whole list: a qname that is already
        resident raises ValueError.  Chromosome values the index has not seen take the next dense ids in
        ascending value.  A read of more than 64 intervals, on either side, raises NotImplementedError here:
        ``append_any`` takes those."""
        return self._append(new_data, False)

    def append_any(self, new_data):
        """``append`` for reads of any length (fslr_append_reads_any): the index may hold reads
        of more than 64 intervals and ``new_data`` may bring some (up to 4096 intervals each).  On the device
        the resident chunk reads are relocated around the batch; afterwards the index is what
        ``build_interval_trees`` of the union gives, with the resident reads first.  Without a long read on
        either side it is ``append``."""
        return self._append(new_data, True)

    def _append(self, new_data, any_length):
        if self.long is not None and not any_length:
            raise NotImplementedError(f'append does not take an index with reads of more than {FSLR_MAX_L} intervals '
                                      f'(append_any does)')
        if not isinstance(new_data, IntervalData):
            new_data = IntervalData.from_items(new_data)
        old, oc = self.data, self.csr
        if old.chrom.dtype.kind not in 'iu' or new_data.chrom.dtype.kind not in 'iu':
            raise TypeError('append needs numeric chromosome values (rename_chromosomes)')
        if not getattr(oc, 'start_sorted', True):
            raise ValueError('append needs an index built from a start-sorted data list')
        nc = build_csr(new_data)
        if not nc.start_sorted:
            raise ValueError('the new data list is not in start order (prepare_data sorts it)')
        if has_long_reads(nc) and not any_length:
            raise NotImplementedError(f'append does not take a read of more than {FSLR_MAX_L} intervals (append_any does)')
        # a read of more than FSLR_MAX_L intervals on either side: fslr_append_reads_any
        any_length = any_length and (self.long is not None or has_long_reads(nc))
        names = lambda q: q if isinstance(q, np.ndarray) else q[np.arange(len(q))]
        old_names, new_names = names(old.qnames), names(new_data.qnames)
        resident = set(old_names[np.asarray(oc.read_qcode, np.int64)].tolist())
        twice = [q for q in new_names[np.asarray(nc.read_qcode, np.int64)].tolist() if q in resident]
        if twice:
            raise ValueError(f'{twice[0]!r} is already a read of this index (a read is a whole list and is never '
                             f'extended); {len(twice)} such qname(s)')
        # the batch's raw chromosome values -> the resident dense ids, unseen values behind them
        keys, ids, _ = self._chrom_table()
        raw = np.asarray(new_data.chrom, np.int64)[np.asarray(nc.data_pos, np.int64)]
        keys = np.zeros(0, np.int64) if keys is None else keys
        unseen = np.setdiff1d(raw, keys)                                  # sorted, unique
        all_keys = np.concatenate([keys, unseen])
        all_ids = np.concatenate([np.asarray(ids, np.int64) if keys.size else np.zeros(0, np.int64),
                                  oc.n_chroms + np.arange(unseen.size, dtype=np.int64)])
        o = np.argsort(all_keys, kind='stable')
        dense = all_ids[o][np.searchsorted(all_keys[o], raw)].astype(np.int32) if raw.size else np.zeros(0, np.int32)
        n_chroms = int(oc.n_chroms + unseen.size)
        batch = CSR(read_off=nc.read_off, read_qlen2=nc.read_qlen2, read_nal=nc.read_nal, iv_chrom=dense,
                    iv_start=nc.iv_start, iv_end=nc.iv_end, iv_aln=nc.iv_aln, n_chroms=n_chroms,
                    read_qcode=nc.read_qcode, data_pos=nc.data_pos, nal_varies=nc.nal_varies)
        # the host mirrors first (where each element of either list lands in the merged list): should
        # making them fail, the device still holds what self.data and self.csr describe
        a, b = np.asarray(old.start, np.int64), np.asarray(new_data.start, np.int64)
        pos_old = np.arange(a.size, dtype=np.int64) + np.searchsorted(b, a, side='left')
        pos_new = np.arange(b.size, dtype=np.int64) + np.searchsorted(a, b, side='right')

        def merged(x, y):
            x, y = np.asarray(x), np.asarray(y)
            out = np.empty(x.size + y.size, np.result_type(x.dtype, y.dtype))
            out[pos_old], out[pos_new] = x, y
            return out
        cols = {f: merged(getattr(old, f), getattr(new_data, f))
                for f in ('chrom', 'start', 'end', 'aln_size', 'n_alignments', 'qlen2', 'middle', 'index')}
        data = IntervalData(qcode=merged(old.qcode, np.asarray(new_data.qcode, np.int64) + len(old_names)),
                            qnames=np.concatenate([old_names, new_names]), **cols)
        cat = lambda f: np.concatenate([getattr(oc, f), getattr(batch, f)])
        data._csr = CSR(read_off=np.concatenate([oc.read_off, oc.n_intervals + nc.read_off[1:]]).astype(np.int32),
                        read_qlen2=cat('read_qlen2'), read_nal=cat('read_nal'), iv_chrom=cat('iv_chrom'),
                        iv_start=cat('iv_start'), iv_end=cat('iv_end'), iv_aln=cat('iv_aln'), n_chroms=n_chroms,
                        read_qcode=np.concatenate([oc.read_qcode, np.asarray(nc.read_qcode, np.int64) + len(old_names)]),
                        data_pos=np.concatenate([pos_old[np.asarray(oc.data_pos, np.int64)],
                                                 pos_new[np.asarray(nc.data_pos, np.int64)]]),
                        nal_varies=bool(oc.nal_varies or nc.nal_varies), start_sorted=True)
        # the batch goes up folded for the overlap score_pairs / match_reads last installed, if those
        # thresholds are still the device's (they key their skip of set_thresholds on _thr_key); otherwise
        # with placeholders, and the next call folds every threshold as after a fresh upload
        ctx = self.ctx
        key = self.__dict__.get('_thr_key')
        live = key is not None and key[1] == getattr(ctx, 'thr_gen', 0)
        self.__dict__.pop('_thr_key', None)
        thr = fold_overlap_threshold(nc.iv_aln, key[0]) if live else \
            np.where(nc.iv_aln == 0, FSLR_THR_ZERO_ALN, 0).astype(np.int32)
        if any_length:
            ctx.append_csr_any(batch, thr)
        else:
            ctx.append_csr(batch, thr)
        self.source = self.data = data
        self.csr = data._csr
        self.long = np.diff(np.asarray(self.csr.read_off, np.int64)).astype(np.int32) if has_long_reads(self.csr) else None
        self.__dict__.pop('_ctable', None)
        self.__dict__.pop('_rank_of', None)
        if live:
            self._thr_key = (key[0], ctx.thr_gen)
        ctx.build_index()
        return self

    # -- fewer reads in the resident set (fslr_remove_reads) ------------------------
    def remove(self, keep=None, qnames=None):
        """Drop whole reads from the resident set on the device and rebuild the index: ``keep`` is a boolean
        mask over the read ranks (True: the read stays), or ``qnames`` names the reads to drop (an unknown one
        raises ValueError).  The survivors close the gaps in rank, CSR order and `data` list; the dense chromosome
        ids, the qname table and the qname codes stay, so a chromosome may be left without intervals and a
        removed qname may be appended again.  Only the mask goes to the device; the host mirrors are numpy
        selections, O(n).  Afterwards ``self.data`` (also ``self.source``) is the list without the removed
        reads' rows and ``self.csr`` ``prep.remove_reads_csr``'s result.  Returns the old rank -> new rank map
        (int32, -1 for a removed read).  Keeping nothing raises ValueError.  An index with reads of more than 64
        intervals raises NotImplementedError here: ``remove_any`` takes it."""
        return self._remove(keep, qnames, False)

    def remove_any(self, keep=None, qnames=None):
        """``remove`` for an index that may hold reads of more than 64 intervals (fslr_remove_reads_any, DESIGN.md
        §13.7): ``keep`` and the returned map are over the real read ranks, a removed read loses all its chunks,
        and once no long read is left the index is a plain one.  Without a long read it is ``remove``."""
        return self._remove(keep, qnames, True)

    def _remove(self, keep, qnames, any_length):
        if self.long is not None and not any_length:
            raise NotImplementedError(f'remove does not take an index with reads of more than {FSLR_MAX_L} intervals '
                                      f'(remove_any does)')
        if (keep is None) == (qnames is None):
            raise TypeError('remove takes either keep (a mask over the read ranks) or qnames (the reads to drop)')
        oc = self.csr
        if not getattr(oc, 'start_sorted', True):
            raise ValueError('remove needs an index built from a start-sorted data list')
        if qnames is not None:
            try:
                gone = self._ranks(np.asarray(list(qnames), dtype=object))
            except KeyError as e:
                raise ValueError(e.args[0]) from None
            keep = np.ones(oc.n_reads, bool)
            keep[gone] = False
        keep = np.asarray(keep)
        if keep.dtype != bool or keep.shape != (oc.n_reads,):
            raise ValueError(f'keep needs one boolean per read ({oc.n_reads})')
        # the host mirrors first: should making them fail, the device still holds what self.data and
        # self.csr describe
        table = self._chrom_table()                   # the dense ids stay, so the table made for the larger set holds
        csr, _ = remove_reads_csr(oc, keep)
        data = self.data.select(kept_data_rows(oc, keep))
        data._csr = csr
        ctx = self.ctx
        key = self.__dict__.get('_thr_key')
        live = key is not None and key[1] == getattr(ctx, 'thr_gen', 0)
        self.__dict__.pop('_thr_key', None)
        # with a read of more than FSLR_MAX_L intervals resident: fslr_remove_reads_any
        new_rank = ctx.remove_reads_any(keep) if self.long is not None else ctx.remove_reads(keep)
        self.source = self.data = data
        self.csr = csr
        self.long = np.diff(np.asarray(csr.read_off, np.int64)).astype(np.int32) if has_long_reads(csr) else None
        self._ctable = table
        self.__dict__.pop('_rank_of', None)
        if live:                                      # the survivors' thresholds are the ones that were installed
            self._thr_key = (key[0], ctx.thr_gen)
        ctx.build_index()
        return new_rank

    # -- search (cluster.py:201: tree[itv.chrom].search_values(itv.start, itv.end)) ----------------
    # A query (chrom, start, end) hits the stored interval (c, s, e) iff c == chrom, s <= end and
    # e >= start (end-inclusive, superintervals search_values).  Hits are positions in the `data` list
    # the index was built from, in descending position of the order (start ascending, end descending,
    # data position ascending): the search order of the superintervals stand-in
    # (tests/golden/refharness.py), the one the edge cap is replayed in.
    def _chrom_table(self):
        """The caller's chromosome values -> the CSR's dense ids, made once per index: ``(keys, ids,
        table)``, keys a sorted int64 array (or None when the values are not integers)."""
        t = self.__dict__.get('_ctable')
        if t is None:
            csr = self.csr
            dense = np.empty(csr.n_intervals, np.int64)
            dense[np.asarray(csr.data_pos, np.int64)] = csr.iv_chrom       # per data position
            raw = getattr(self.source, 'chrom', None)
            raw = np.asarray([it[0] for it in self.source] if raw is None else raw)
            keys = ids = None
            if raw.dtype.kind in 'iu':
                keys, first = np.unique(raw.astype(np.int64), return_index=True)
                ids = dense[first]
                table = dict(zip(keys.tolist(), ids.tolist()))
            else:
                table = {}
                for v, d in zip(raw.tolist(), dense.tolist()):
                    table.setdefault(v, d)
            t = self._ctable = (keys, ids, table)
        return t

    def _dense_chroms(self, chrom) -> np.ndarray:
        """Dense ids (int32) of the caller's chromosome values; -1 for one the index does not hold."""
        keys, ids, table = self._chrom_table()
        q = np.asarray(chrom)
        if q.ndim != 1:
            raise ValueError('chrom, start and end must be one-dimensional')
        if keys is not None and q.dtype.kind in 'iu':
            if not keys.size:
                return np.full(q.shape, -1, np.int32)
            at = np.minimum(np.searchsorted(keys, q), keys.size - 1)
            return np.where(keys[at] == q, ids[at], -1).astype(np.int32)
        return np.asarray([table.get(v, -1) for v in q.tolist()], np.int32)

    @staticmethod
    def _coords(x) -> np.ndarray:
        # Stored coordinates lie in [0, 2**30): a bound below 0 selects what -1 selects and one above
        # 2**30 what 2**30 selects, so the clip (which makes the int32 cast safe) changes no result.
        return np.clip(np.asarray(x, dtype=np.int64), -1, 1 << 30).astype(np.int32)

    def search_batch(self, chrom, start, end):
        """The hits of a batch of query intervals: ``(offsets int64[nq + 1], data_positions int64[total])``;
        query k's hits are ``data_positions[offsets[k]:offsets[k + 1]]`` in search order.  ``chrom`` holds
        the caller's chromosome values (what ``data.chrom`` holds), coordinates are integers."""
        off, hits = self.ctx.search(self._dense_chroms(chrom), self._coords(start), self._coords(end))
        pos = np.asarray(self.csr.data_pos, np.int64)[hits]
        if not getattr(self.csr, 'start_sorted', True) and pos.size:
            # a list that is not start-sorted is uploaded without its data positions (the (chrom, start)
            # sort path), so the device ranks equal (start, end) by CSR index: put those runs in data order
            s, e = self.csr.iv_start[hits], self.csr.iv_end[hits]
            seg = np.repeat(np.arange(off.size - 1), np.diff(off))
            if ((seg[1:] == seg[:-1]) & (s[1:] == s[:-1]) & (e[1:] == e[:-1])).any():
                pos = pos[np.lexsort((-pos, e, -s.astype(np.int64), seg))]
        return off, pos

    def count_batch(self, chrom, start, end) -> np.ndarray:
        """Hits per query (int64[nq]); no hit list is made."""
        return self.ctx.search_counts(self._dense_chroms(chrom), self._coords(start), self._coords(end))

    # -- pair predicates (cluster.py:209-219) for arbitrary read pairs -----------------------------
    def _ranks(self, query) -> np.ndarray:
        """Read ranks (int32) of integer ranks or of qnames."""
        q = np.asarray(query)
        if q.ndim != 1:
            raise ValueError('query1 and query2 must be one-dimensional')
        if q.size == 0:
            return np.zeros(0, np.int32)
        if q.dtype.kind in 'iu':
            if q.min() < 0 or q.max() >= self.csr.n_reads:
                raise IndexError(f'read rank outside [0, {self.csr.n_reads})')
            return q.astype(np.int32)
        table = self.__dict__.get('_rank_of')
        if table is None:
            names = self.data.qnames[self.csr.read_qcode]
            table = self._rank_of = dict(zip(names.tolist(), range(len(names))))
        try:
            return np.asarray([table[v] for v in q.tolist()], np.int32)
        except KeyError as e:
            raise KeyError(f'{e.args[0]!r} is not a read of this index') from None

    def score_pairs(self, query1, query2, overlap_cutoff, jaccard_threshold, qlen_diff, diff,
                    raise_zero_division=False, matching=False) -> PairScores:
        """What the reference's pair loop computes for the ordered read pairs ``(query1[k], query2[k])``
        (integer read ranks, or qnames), whether or not a query would reach them: list1 = query1's
        intervals, list2 = query2's.  One batched device call (fslr_score_pairs); the query state of the
        index (edges, labels) is left alone.  ZeroDivisionError is flagged per pair
        (``PairScores.zero_division``); ``raise_zero_division`` raises it for the first flagged pair.
        ``matching=True`` also returns which interval took which (fslr_pair_matching) as
        ``PairScores.matching``, a PairMatching."""
        min(jaccard_threshold)                              # cluster.py:188 raises on an empty list
        if self.long is not None:
            raise NotImplementedError(f'score_pairs does not take an index with reads of more than {FSLR_MAX_L} '
                                      f'intervals')
        return self._score_pairs(query1, query2, overlap_cutoff, jaccard_threshold, qlen_diff, diff,
                                 raise_zero_division, False, matching)

    def score_pairs_any(self, query1, query2, overlap_cutoff, jaccard_threshold, qlen_diff, diff,
                        raise_zero_division=False, matching=False) -> PairScores:
        """score_pairs on any index, with or without reads of more than FSLR_MAX_L intervals (up to 4096, the
        index's limit): the ranks are the reads' own, a read's list is its whole list, I and U are unclamped
        and the edge rule beyond the pass table is ``umax_table(jaccard_threshold, longest read)``
        (fslr_score_pairs_any).  On an index without such reads it is score_pairs, byte for byte."""
        if not len(jaccard_threshold):
            raise ValueError('jaccard_threshold is empty (cluster.py:188 takes its min())')
        return self._score_pairs(query1, query2, overlap_cutoff, jaccard_threshold, qlen_diff, diff,
                                 raise_zero_division, True, matching)

    def _score_pairs(self, query1, query2, overlap_cutoff, jaccard_threshold, qlen_diff, diff, raise_zero_division,
                     any_length, matching=False):
        a, b = self._ranks(query1), self._ranks(query2)
        if a.shape != b.shape:
            raise ValueError('query1 and query2 must be of one length')
        ctx = self.ctx
        if isinstance(self, RowsIndex):
            if self.overlap != float(overlap_cutoff):            # folded on the device at the upload
                ctx.fold_thresholds(overlap_cutoff)
                self.overlap = float(overlap_cutoff)
        elif self.__dict__.get('_thr_key') != (float(overlap_cutoff), getattr(ctx, 'thr_gen', 0)):
            ctx.set_thresholds(fold_overlap_threshold(self.csr.iv_aln, overlap_cutoff))
            self._thr_key = (float(overlap_cutoff), ctx.thr_gen)
        rows = None
        if any_length:
            umax = umax_table(jaccard_threshold, int(self.long.max())) if self.long is not None else None
            call = ctx.pair_matching_any if matching else ctx.score_pairs_any
            I, U, flags, *rows = call(a, b, 1 - qlen_diff, 1 - diff, pass_table(jaccard_threshold), umax)
        else:
            call = ctx.pair_matching if matching else ctx.score_pairs
            I, U, flags, *rows = call(a, b, 1 - qlen_diff, 1 - diff, pass_table(jaccard_threshold))
        qn = self.data.qnames[self.csr.read_qcode]
        if raise_zero_division:
            bad = np.flatnonzero(flags & (SCORE_ZD_GATE | SCORE_ZD_OVERLAP))
            if bad.size:
                k = int(bad[0])
                raise ZeroDivisionError(f'division by zero (pair {k}: {qn[a[k]]!r}, {qn[b[k]]!r})')
        scores = PairScores(a, b, I, U, flags, qn)
        if matching:
            # the intervals in CSR order, chromosomes as the caller's values (data positions of the `data` list)
            dp = np.asarray(self.csr.data_pos, np.int64)
            d = self.data
            cols = (np.asarray(d.chrom)[dp], np.asarray(d.start)[dp], np.asarray(d.end)[dp],
                    np.asarray(self.csr.read_off, np.int64))
            scores.matching = PairMatching(scores, *rows, cols)
        return scores

    # -- new reads against the resident index (cluster.py:197-222 with an external list1) -----------
    _EMIT = {'edges': SCORE_EDGE, 'gated': SCORE_GATE, 'all': 0}

    def match_reads(self, reads, overlap_cutoff, jaccard_threshold, qlen_diff, diff, emit='edges',
                    exclude=None) -> ReadMatches:
        """What the reference's pair loop would do for reads that are not in this index: per new read its
        candidate partners in first-visit order and, per partner, score_pairs' I, U and flags for (list1 =
        the new read, list2 = the partner).  The edge cap is not applied.  One device call
        (fslr_match_reads); the query state of the index is left alone.

        ``reads``: an IntervalData or a list of IntervalItem (the new reads' `data` list: reads rank by first
        appearance, a read's intervals keep list order, chromosomes are the values this index was built
        with), or a ``prep.CSR`` whose ``iv_chrom`` already holds this index's dense ids.  ``emit``: the
        rows to return: 'edges', 'gated' (the length gate passed) or 'all' candidates.  ``exclude``: per
        new read a resident rank (or qname) to skip, -1 / None for none."""
        min(jaccard_threshold)                              # cluster.py:188 raises on an empty list
        if emit not in self._EMIT:
            raise ValueError(f"emit must be 'edges', 'gated' or 'all', not {emit!r}")
        if self.long is not None:
            raise NotImplementedError(f'match_reads does not take an index with reads of more than {FSLR_MAX_L} '
                                      f'intervals')
        return self._match_reads(reads, overlap_cutoff, jaccard_threshold, qlen_diff, diff, emit, exclude, False)

    def match_reads_any(self, reads, overlap_cutoff, jaccard_threshold, qlen_diff, diff, emit='edges',
                        exclude=None) -> ReadMatches:
        """match_reads on any index and for new reads of up to 4096 intervals (fslr_match_reads_any): partners
        and ``exclude`` are the reads' own ranks, a long resident read is one candidate however many of its
        intervals are hit, I and U are unclamped, and the edge rule beyond the pass table is
        ``umax_table(jaccard_threshold, longest list)``.  On an index without long reads and for new reads of
        at most FSLR_MAX_L intervals it is match_reads, byte for byte."""
        if not len(jaccard_threshold):
            raise ValueError('jaccard_threshold is empty (cluster.py:188 takes its min())')
        if emit not in self._EMIT:
            raise ValueError(f"emit must be 'edges', 'gated' or 'all', not {emit!r}")
        return self._match_reads(reads, overlap_cutoff, jaccard_threshold, qlen_diff, diff, emit, exclude, True)

    def _match_reads(self, reads, overlap_cutoff, jaccard_threshold, qlen_diff, diff, emit, exclude, any_length):
        if isinstance(reads, CSR):
            qcsr, chrom = reads, np.asarray(reads.iv_chrom, np.int32)
            names = np.arange(qcsr.n_reads)
        else:
            raw = None
            if not isinstance(reads, IntervalData):
                reads = list(reads)
                raw = np.asarray([it[0] for it in reads])
                reads = IntervalData.from_items(reads)
            qcsr = reads.csr()
            raw = np.asarray(reads.chrom) if raw is None else raw
            chrom = self._dense_chroms(raw[np.asarray(qcsr.data_pos, np.int64)]) if len(reads) else \
                np.zeros(0, np.int32)
            names = reads.qnames[qcsr.read_qcode]
        qlen = np.diff(np.asarray(qcsr.read_off, np.int64))
        limit = 4096 if any_length else FSLR_MAX_L
        if qlen.size and qlen.max() > limit:
            r = int(np.argmax(qlen > limit))
            raise ValueError(f'query read {r} has more than {limit} intervals')
        n = qcsr.n_reads
        ex = None
        if exclude is not None:
            e = np.asarray(exclude)
            if e.shape != (n,):
                raise ValueError('exclude must have one entry per query read')
            if e.dtype.kind in 'iu':
                if e.size and (e.min() < -1 or e.max() >= self.csr.n_reads):
                    raise IndexError(f'exclude: a value is neither -1 nor a read rank in [0, {self.csr.n_reads})')
                ex = e.astype(np.int32)
            else:
                ex = np.full(n, -1, np.int32)
                has = np.asarray([v is not None for v in e.tolist()], bool)
                ex[has] = self._ranks(e[has])
        ctx = self.ctx
        if isinstance(self, RowsIndex):
            if self.overlap != float(overlap_cutoff):            # folded on the device at the upload
                ctx.fold_thresholds(overlap_cutoff)
                self.overlap = float(overlap_cutoff)
        elif self.__dict__.get('_thr_key') != (float(overlap_cutoff), getattr(ctx, 'thr_gen', 0)):
            ctx.set_thresholds(fold_overlap_threshold(self.csr.iv_aln, overlap_cutoff))
            self._thr_key = (float(overlap_cutoff), ctx.thr_gen)
        cols = (qcsr.read_off, qcsr.read_qlen2, qcsr.read_nal, chrom, qcsr.iv_start, qcsr.iv_end,
                fold_overlap_threshold(qcsr.iv_aln, overlap_cutoff), 1 - qlen_diff, 1 - diff,
                pass_table(jaccard_threshold), self._EMIT[emit], ex)
        if any_length:
            umax = None
            if self.long is not None or (qlen.size and qlen.max() > FSLR_MAX_L):
                # over the longest list of either side: the table then reaches every U = L1 + L2 - I
                resident = int(self.long.max()) if self.long is not None else \
                    int(np.diff(np.asarray(self.csr.read_off, np.int64)).max(initial=1))
                umax = umax_table(jaccard_threshold, max(resident, int(qlen.max(initial=1))))
            off, counts, best = ctx.match_reads_any(*cols, umax=umax)
            partner, I, U, flags = ctx.match_rows_any()
        else:
            off, counts, best = ctx.match_reads(*cols)
            partner, I, U, flags = ctx.match_rows()
        return ReadMatches(off, partner, I, U, flags, counts, best, names, self.data.qnames[self.csr.read_qcode])

    def cluster_loci(self, G_or_labels=None) -> ClusterLoci:
        """Where each cluster lies: the merged spans of its reads' intervals per chromosome, made on the device
        from the resident index and cluster table (fslr_cluster_loci).  ``G_or_labels`` None uses the context's
        resident table; a graph or a vector of min-rank labels makes the table first (cluster_table) - the way
        in for an index with reads of more than 64 intervals, whose labels live on the host."""
        if G_or_labels is not None:
            cluster_table(G_or_labels, ctx=self.ctx)
        return self._wrap_loci(self.ctx.cluster_loci())

    def _wrap_loci(self, cols) -> ClusterLoci:
        off, dense, start, end, n_intervals, n_reads = cols
        table = self._chrom_table()[2]
        raw = np.asarray(list(table.keys()))
        if dense.size:
            inv = np.empty(max(table.values()) + 1, raw.dtype)
            inv[np.asarray(list(table.values()), np.int64)] = raw
            chrom = inv[dense]
        else:
            chrom = raw[:0]
        return ClusterLoci(off, chrom, start, end, n_intervals, n_reads, dense)

    def _chain_inputs(self, who, qstart, strand, G_or_labels, any_length=False):
        """cluster_junctions' and cluster_paths' arguments: the checked ``qstart`` and ``strand`` in CSR order and
        the loci rows (the table from ``G_or_labels`` first, the rows made when the context holds none)."""
        if self.long is not None and not any_length:
            raise NotImplementedError(f'{who} does not take an index with reads of more than {FSLR_MAX_L} '
                                      f'intervals')
        n = int(self.csr.n_intervals)
        q = np.asarray(qstart)
        if q.shape != (n,):
            raise ValueError(f'qstart holds {q.shape} values, the data list {n} intervals')
        if q.dtype.kind not in 'iu' or (q.size and (q.min() < -(1 << 31) or q.max() >= (1 << 31))):
            raise ValueError('qstart must hold int32 values')
        rev = None
        if strand is not None:
            rev = _rev_bits(strand)
            if rev.shape != (n,):
                raise ValueError(f'strand holds {rev.shape} values, the data list {n} intervals')
        if G_or_labels is not None:
            cluster_table(G_or_labels, ctx=self.ctx)
        pos = np.asarray(self.csr.data_pos, np.int64)
        loci = self._wrap_loci(self.ctx.cluster_loci_rows())
        return q[pos].astype(np.int32), None if rev is None else rev[pos], loci

    def cluster_junctions(self, qstart, strand=None, G_or_labels=None) -> ClusterJunctions:
        """Which pieces each cluster's reads join, and where the breakpoints lie (fslr_cluster_junctions).  A read's
        intervals in query order form a chain of loci; each consecutive pair is one observation of a junction
        between two locus ends, and a cluster's rows group them.  ``qstart`` and ``strand`` are aligned with the
        ``data`` list the index was built from (list order: ``bed.loc[tree.data.index, 'qstart']``); they are
        permuted to the CSR's order through ``csr.data_pos``.  ``strand`` (booleans, 0/1 or '+' / '-'; None: all
        forward) says that an interval runs against the query order.  ``G_or_labels`` makes the cluster table
        first, as for cluster_loci; the loci rows are made when the context holds none.  An index with reads of
        more than 64 intervals raises NotImplementedError.  A RowsIndex supports the call: its data positions
        come down with fslr_get_csr on first use."""
        qkey, rev, loci = self._chain_inputs('cluster_junctions', qstart, strand, G_or_labels)
        off, *cols = self.ctx.cluster_junctions(qkey, rev)
        return ClusterJunctions(off, cols, loci)

    def cluster_junctions_any(self, qstart, strand=None, G_or_labels=None) -> ClusterJunctions:
        """cluster_junctions for an index that may hold reads of more than 64 intervals, up to 4096
        (fslr_cluster_junctions_any): a long read's chain runs over all its intervals.  The arguments and the result
        are cluster_junctions'; ``qstart`` / ``strand`` go through ``csr.data_pos`` to the real CSR's order.  On an
        index with long reads the labels live on the host, so give ``G_or_labels`` (a graph or a label vector over
        the real reads) unless cluster_loci made the table already.  On an index without long reads it returns what
        cluster_junctions returns."""
        qkey, rev, loci = self._chain_inputs('cluster_junctions_any', qstart, strand, G_or_labels, True)
        off, *cols = self.ctx.cluster_junctions_any(qkey, rev)
        return ClusterJunctions(off, cols, loci)

    def cluster_paths_any(self, qstart, strand=None, G_or_labels=None) -> ClusterPaths:
        """cluster_paths for an index that may hold reads of more than 64 intervals, up to 4096
        (fslr_cluster_paths_any); the arguments and the result are cluster_paths', the rules for ``G_or_labels``
        cluster_junctions_any's.  On an index without long reads it returns what cluster_paths returns."""
        qkey, rev, loci = self._chain_inputs('cluster_paths_any', qstart, strand, G_or_labels, True)
        qn = getattr(self.data, 'qnames', None)
        code = np.asarray(self.csr.read_qcode)
        paths = ClusterPaths(*self.ctx.cluster_paths_any(qkey, rev), loci, code if qn is None else np.asarray(qn[code]))
        self._paths_made = (getattr(self.ctx, '_cluster_info', None), qkey, rev, paths)     # (see cluster_paths)
        return paths

    def cluster_paths(self, qstart, strand=None, G_or_labels=None) -> ClusterPaths:
        """The distinct read structures of each cluster and how many reads agree on each (fslr_cluster_paths).  A
        read's intervals in query order are a chain of (locus, strand) tokens; read from the other strand the
        chain is reversed with every strand flipped, and the smaller of the two is the read's path.  A cluster's
        rows are its distinct paths.  The arguments are cluster_junctions': ``qstart`` and ``strand`` aligned with
        the ``data`` list, ``G_or_labels`` makes the cluster table first; an index with reads of more than 64
        intervals raises NotImplementedError."""
        qkey, rev, loci = self._chain_inputs('cluster_paths', qstart, strand, G_or_labels)
        qn = getattr(self.data, 'qnames', None)
        code = np.asarray(self.csr.read_qcode)
        paths = ClusterPaths(*self.ctx.cluster_paths(qkey, rev), loci, code if qn is None else np.asarray(qn[code]))
        # what cluster_path_segments may reuse: the rows, the table they were made on and the columns they were made with
        self._paths_made = (getattr(self.ctx, '_cluster_info', None), qkey, rev, paths)
        return paths

    def cluster_path_segments(self, qstart, qend=None, strand=None, G_or_labels=None) -> ClusterPathSegments:
        """Consensus coordinates and junction gaps per piece of every cluster path (fslr_cluster_path_segments): where
        each piece lies in the reads that walk the path (min, lower median, max of start and end) and, with
        ``qend``, the query-space gap the reads leave between a piece and the next.  ``qstart``, ``qend`` and
        ``strand`` are aligned with the ``data`` list, as for cluster_paths; ``G_or_labels`` makes the cluster table
        first.  The table's loci and paths are made when needed; the path rows this index made with the same
        ``qstart`` and ``strand`` since its last table are reused.  An index with reads of more than 64 intervals
        raises NotImplementedError.  The result holds its ClusterPaths as ``.paths``."""
        if self.long is not None:
            raise NotImplementedError(f'cluster_path_segments does not take an index with reads of more than '
                                      f'{FSLR_MAX_L} intervals')
        return self._path_segments(False, qstart, qend, strand, G_or_labels)

    def cluster_path_segments_any(self, qstart, qend=None, strand=None, G_or_labels=None) -> ClusterPathSegments:
        """cluster_path_segments for an index that may hold reads of more than 64 intervals, up to 4096
        (fslr_cluster_path_segments_any): a long read's pieces and gaps run over all its intervals.  The arguments,
        the reuse of resident path rows and the result are cluster_path_segments'; the loci and the paths are made
        through cluster_loci / cluster_paths_any, the rules for ``G_or_labels`` are cluster_junctions_any's.  On an
        index without long reads it returns what cluster_path_segments returns."""
        return self._path_segments(True, qstart, qend, strand, G_or_labels)

    def _path_segments(self, any_length, qstart, qend, strand, G_or_labels):
        make_paths = self.cluster_paths_any if any_length else self.cluster_paths
        segments = self.ctx.cluster_path_segments_any if any_length else self.ctx.cluster_path_segments
        n = int(self.csr.n_intervals)
        qe = None
        if qend is not None:
            e = np.asarray(qend)
            if e.shape != (n,):
                raise ValueError(f'qend holds {e.shape} values, the data list {n} intervals')
            if e.dtype.kind not in 'iu' or (e.size and (e.min() < -(1 << 31) or e.max() >= (1 << 31))):
                raise ValueError('qend must hold int32 values')
            qe = e[np.asarray(self.csr.data_pos, np.int64)].astype(np.int32)
        made = self._paths_to_reuse(qstart, strand, G_or_labels)
        if made is not None:
            try:
                return ClusterPathSegments(made[3], *segments(made[1], qe))
            except FslrError as err:                     # the rows were dropped since (cluster_loci again): make them
                if 'no cluster paths' not in str(err):
                    raise
        paths = make_paths(qstart, strand, G_or_labels)
        return ClusterPathSegments(paths, *segments(self._paths_made[1], qe))

    def _paths_to_reuse(self, qstart, strand, G_or_labels):
        """What cluster_paths* remembered (table, qkey, rev, ClusterPaths) when a call on the resident path rows may
        reuse it: no new table is asked for, the context's table is still the one the rows were made on, and
        ``qstart`` and ``strand`` are the columns they were made with.  None otherwise."""
        made = self.__dict__.get('_paths_made')
        if G_or_labels is not None or made is None or made[0] is None or \
                made[0] is not getattr(self.ctx, '_cluster_info', None):
            return None
        n = int(self.csr.n_intervals)
        q = np.asarray(qstart)
        rev = None if strand is None else _rev_bits(strand)
        pos = np.asarray(self.csr.data_pos, np.int64)
        if q.shape == (n,) and q.dtype.kind in 'iu' and np.array_equal(q[pos], made[1]) and \
                (rev is None) == (made[2] is None) and (rev is None or (rev.shape == (n,) and np.array_equal(rev[pos], made[2]))):
            return made
        return None

    def cluster_path_containment(self, qstart, strand=None, G_or_labels=None) -> ClusterPathContainment:
        """Which cluster paths are only truncated views of another path, and a full-length path's support once the
        truncated reads are counted (fslr_cluster_path_containment).  ``qstart``, ``strand`` and ``G_or_labels`` are
        cluster_paths_any's; the table's loci and paths are made when needed and the path rows this index made with
        the same ``qstart`` and ``strand`` since its last table are reused (the rule of cluster_path_segments_any).
        The call works on the path rows alone, so an index with reads of more than 64 intervals is taken as any
        other.  The result holds its ClusterPaths as ``.paths``."""
        made = self._paths_to_reuse(qstart, strand, G_or_labels)
        if made is not None:
            try:
                return ClusterPathContainment(made[3], *self.ctx.cluster_path_containment())
            except FslrError as err:                     # the rows were dropped since (cluster_loci again): make them
                if 'no cluster paths' not in str(err):
                    raise
        paths = self.cluster_paths_any(qstart, strand, G_or_labels)
        return ClusterPathContainment(paths, *self.ctx.cluster_path_containment())

    def cluster_collapsed_segments(self, qstart, qend=None, strand=None, G_or_labels=None) -> ClusterCollapsedSegments:
        """Consensus coordinates and junction gaps per piece of every full-length (maximal) cluster path, taken over
        all reads that collapse onto it (fslr_cluster_collapsed_segments): cluster_path_segments' statistics with the
        truncated reads of cluster_path_containment counted at the pieces they cover.  The arguments are
        cluster_path_segments'; the loci, the paths and the containment are made when needed and the path rows this
        index made with the same ``qstart`` and ``strand`` since its last table are reused.  An index with reads of
        more than 64 intervals raises NotImplementedError.  The result holds its ClusterPaths as ``.paths`` and its
        ClusterPathContainment as ``.containment``."""
        if self.long is not None:
            raise NotImplementedError(f'cluster_collapsed_segments does not take an index with reads of more than '
                                      f'{FSLR_MAX_L} intervals (cluster_collapsed_segments_any does)')
        return self._collapsed_segments(False, qstart, qend, strand, G_or_labels)

    def cluster_collapsed_segments_any(self, qstart, qend=None, strand=None, G_or_labels=None) -> ClusterCollapsedSegments:
        """cluster_collapsed_segments for an index that may hold reads of more than 64 intervals, up to 4096
        (fslr_cluster_collapsed_segments_any); the rules for ``G_or_labels`` are cluster_junctions_any's.  On an index
        without long reads it returns what cluster_collapsed_segments returns."""
        return self._collapsed_segments(True, qstart, qend, strand, G_or_labels)

    def _collapsed_segments(self, any_length, qstart, qend, strand, G_or_labels):
        call = self.ctx.cluster_collapsed_segments_any if any_length else self.ctx.cluster_collapsed_segments
        n = int(self.csr.n_intervals)
        qe = None
        if qend is not None:
            e = np.asarray(qend)
            if e.shape != (n,):
                raise ValueError(f'qend holds {e.shape} values, the data list {n} intervals')
            if e.dtype.kind not in 'iu' or (e.size and (e.min() < -(1 << 31) or e.max() >= (1 << 31))):
                raise ValueError('qend must hold int32 values')
            qe = e[np.asarray(self.csr.data_pos, np.int64)].astype(np.int32)
        # through cluster_paths_any (resident rows are reused under _paths_to_reuse) and cluster_path_containment
        ct = self.cluster_path_containment(qstart, strand, G_or_labels)
        return ClusterCollapsedSegments(ct.paths, ct, *call(self._paths_made[1], qe))

    def __getitem__(self, chrom):
        return ChromosomeView(self, chrom)

    def __contains__(self, chrom):
        return chrom in self._chrom_table()[2]

    def keys(self):
        return self._chrom_table()[2].keys()

    def items(self):
        return [(c, ChromosomeView(self, c)) for c in self.keys()]


class ChromosomeView:
    """``tree[chrom]`` of a DeviceIntervalIndex: the reference's per-chromosome IntervalMap as far as
    its pair loop uses it (cluster.py:201).  A chromosome the index does not hold gives an empty view,
    as the reference's defaultdict gives an empty map."""

    def __init__(self, index, chrom):
        self.index, self.chrom = index, chrom

    def search_idxs(self, start, end) -> np.ndarray:
        """Data positions of the hits, in search order."""
        if self.chrom not in self.index:
            return np.zeros(0, np.int64)
        return self.index.search_batch([self.chrom], [start], [end])[1]

    def search_values(self, start, end) -> list:
        """The hit intervals as items of the list the index was built from (IntervalItem)."""
        src = self.index.source
        return [src[p] for p in self.search_idxs(start, end).tolist()]

    def count(self, start, end) -> int:
        if self.chrom not in self.index:
            return 0
        return int(self.index.count_batch([self.chrom], [start], [end])[0])


class RowsCSR:
    """The CSR fslr_set_reads_rows made on the device: the host holds what the CLI reads
    of it (the qname code of each read rank, the counts and flags); the columns are copied off the
    device on first use (fslr_get_csr) and then read as a ``prep.CSR``."""
    start_sorted = True

    def __init__(self, ctx, info):
        self._ctx, self._host = ctx, None
        self._n, self._ni = int(info['n_reads']), int(info['n_intervals'])
        self.n_chroms = int(info['n_chroms'])
        self.nal_varies = bool(info['nal_varies'])
        self.read_qcode = ctx.read_codes()

    n_reads = property(lambda self: self._n)
    n_intervals = property(lambda self: self._ni)

    def host(self) -> CSR:
        if self._host is None:
            d = self._ctx.device_csr(self._ni, self.n_chroms)
            self._host = CSR(read_off=d['read_off'], read_qlen2=d['read_qlen2'], read_nal=d['read_nal'],
                             iv_chrom=d['iv_chrom'], iv_start=d['iv_start'], iv_end=d['iv_end'], iv_aln=d['iv_aln'],
                             n_chroms=self.n_chroms, read_qcode=self.read_qcode, data_pos=d['data_pos'],
                             nal_varies=self.nal_varies, start_sorted=True)
        return self._host

    def __getattr__(self, name):                 # read_off, iv_*, data_pos: the host copy
        if name.startswith('_'):
            raise AttributeError(name)
        return getattr(self.host(), name)


class RowsIndex(DeviceIntervalIndex):
    """build_interval_trees' result for the columnar CLI: the reads set on the device from rows
    (fslr_set_reads_rows, thresholds folded there for ``overlap``) and the index built."""

    def __init__(self, data, csr: RowsCSR, ctx: Context, overlap: float):
        self.source = self.data = data
        self.csr, self.ctx, self.long = csr, ctx, None
        self.overlap = float(overlap)
        ctx.build_index()

    def append(self, new_data):
        raise NotImplementedError('an index made from rows on the device (fslr_set_reads_rows) does not append: '
                                  'fslr_append_reads extends reads set by fslr_set_reads; build the index from '
                                  'prepare_data\'s result to append to it')

    append_any = append

    def remove(self, keep=None, qnames=None):
        raise NotImplementedError('an index made from rows on the device (fslr_set_reads_rows) does not remove: '
                                  'fslr_remove_reads compacts reads set by fslr_set_reads; build the index from '
                                  'prepare_data\'s result to remove reads from it')

    remove_any = remove


class MultiGpuIndex:
    """What build_interval_trees returns for ``n_gpus > 1``: the prepared CSR on the host.  The ranks
    (one process per GPU, fslr_amd.multi) upload it and build their chromosomes' index inside
    query_interval_trees; this process must not have initialised the GPU before then."""

    def __init__(self, data, n_gpus: int, device: int | None = None):
        self.source = data
        if not isinstance(data, IntervalData):
            data = IntervalData.from_items(data)
        self.data = data
        self.csr = data.csr()
        self.n_gpus = int(n_gpus)
        self.first_device = 0 if device is None else int(device)

    def _no_search(self, *args, **kwargs):
        raise NotImplementedError('a multi-GPU index lives in the rank processes and cannot be searched from here; '
                                  'build it with n_gpus=1 to search it')

    search_batch = count_batch = __getitem__ = _no_search

    def score_pairs(self, *args, **kwargs):
        raise NotImplementedError('a multi-GPU index lives in the rank processes and cannot score pairs from here; '
                                  'build it with n_gpus=1 to score pairs')

    score_pairs_any = score_pairs

    def append(self, *args, **kwargs):
        raise NotImplementedError('a multi-GPU index lives in the rank processes and does not append '
                                  '(fslr_append_reads needs the whole index on one context); build it with n_gpus=1')

    def remove(self, *args, **kwargs):
        raise NotImplementedError('a multi-GPU index lives in the rank processes and does not remove '
                                  '(fslr_remove_reads needs the whole index on one context); build it with n_gpus=1')

    append_any, remove_any = append, remove

    def match_reads_any(self, *args, **kwargs):
        return self.match_reads(*args, **kwargs)

    def match_reads(self, *args, **kwargs):
        raise NotImplementedError('a multi-GPU index lives in the rank processes and cannot match reads from here; '
                                  'build it with n_gpus=1 to match reads')

    def cluster_loci(self, *args, **kwargs):
        raise NotImplementedError('a multi-GPU index lives in the rank processes and cannot give cluster loci from '
                                  'here (fslr_cluster_loci needs the whole index on one context); build it with '
                                  'n_gpus=1')

    def cluster_junctions(self, *args, **kwargs):
        raise NotImplementedError('a multi-GPU index lives in the rank processes and cannot give cluster junctions '
                                  'from here (fslr_cluster_junctions needs the whole index on one context); build it '
                                  'with n_gpus=1')

    def cluster_paths(self, *args, **kwargs):
        raise NotImplementedError('a multi-GPU index lives in the rank processes and cannot give cluster paths from '
                                  'here (fslr_cluster_paths needs the whole index on one context); build it with '
                                  'n_gpus=1')

    def cluster_path_segments(self, *args, **kwargs):
        raise NotImplementedError('a multi-GPU index lives in the rank processes and cannot give path segments from '
                                  'here (fslr_cluster_path_segments needs the whole index on one context); build it '
                                  'with n_gpus=1')

    def cluster_path_containment(self, *args, **kwargs):
        raise NotImplementedError('a multi-GPU index lives in the rank processes and cannot give path containment '
                                  'from here (fslr_cluster_path_containment needs the path rows on one context); '
                                  'build it with n_gpus=1')

    def cluster_collapsed_segments(self, *args, **kwargs):
        raise NotImplementedError('a multi-GPU index lives in the rank processes and cannot give collapsed path '
                                  'segments from here (fslr_cluster_collapsed_segments needs the whole index on one '
                                  'context); build it with n_gpus=1')

    def cluster_collapsed_segments_any(self, *args, **kwargs):
        return self.cluster_collapsed_segments(*args, **kwargs)

    def cluster_junctions_any(self, *args, **kwargs):
        return self.cluster_junctions(*args, **kwargs)

    def cluster_paths_any(self, *args, **kwargs):
        return self.cluster_paths(*args, **kwargs)

    def cluster_path_segments_any(self, *args, **kwargs):
        return self.cluster_path_segments(*args, **kwargs)


def _open_context(device: int | None = None) -> Context:
    """A library context on ``device`` (default $FSLR_DEVICE / $LOCAL_RANK / 0)."""
    return Context(_default_device() if device is None else int(device))


def build_interval_trees(data, device: int | None = None, n_gpus: int = 1, ctx: Context | None = None):
    """cluster.py:124-130: upload the prepared intervals and build the (chrom, start) index on the GPU.

    ``data`` is this module's ``prepare_data`` result or the reference's (a list of IntervalItem).
    ``n_gpus > 1``: the chromosome-split multi-GPU query; the upload happens in the
    per-GPU processes that query_interval_trees starts."""
    if int(n_gpus) > 1:
        return MultiGpuIndex(data, n_gpus, device)
    return DeviceIntervalIndex(data, device, ctx=ctx)


class ClusterGraph:
    """Graph of read pairs (the reference's ``nx.Graph``), held as device-computed labels.

    ``labels[r]`` = minimum rank in read r's connected component (ranks are the
    first-appearance order of reads in ``data``).  Nodes are the reads with at
    least one edge, as in ``G.add_edge`` (cluster.py:221).
    """

    def __init__(self, qnames_by_rank, labels, edges_ab, fwd, stats):
        self.qnames_by_rank = qnames_by_rank
        self.labels = labels
        self.edges_ab = edges_ab
        self.fwd = fwd
        self.stats = stats
        n = labels.shape[0]
        sizes = np.bincount(labels, minlength=n) if n else np.zeros(0, np.int64)
        self.comp_size = sizes[labels] if n else np.zeros(0, np.int64)
        self.node_mask = self.comp_size >= 2
        roots = np.flatnonzero((sizes >= 2))          # component roots = min ranks, ascending
        self.roots = roots
        cid = np.full(n, -1, dtype=np.int64)
        if n:
            rid = np.full(n, -1, dtype=np.int64)
            rid[roots] = np.arange(roots.size)
            cid = np.where(self.node_mask, rid[labels], -1)
        self.component_id = cid                        # per rank; -1 = not a node

    def number_of_nodes(self):
        return int(self.node_mask.sum())

    def number_of_edges(self):
        return int(self.edges_ab[0].shape[0])

    @property
    def nodes(self):
        return [self.qnames_by_rank[r] for r in np.flatnonzero(self.node_mask)]

    @property
    def edges(self):
        a, b = self.edges_ab
        return [(self.qnames_by_rank[x], self.qnames_by_rank[y]) for x, y in zip(a.tolist(), b.tolist())]

    def components(self):
        order = np.flatnonzero(self.node_mask)
        cid = self.component_id[order]
        srt = np.argsort(cid, kind='stable')
        out = [set() for _ in range(self.roots.size)]
        for c, r in zip(cid[srt].tolist(), order[srt].tolist()):
            out[c].add(self.qnames_by_rank[r])
        return out

    def to_networkx(self):
        import networkx as nx
        G = nx.Graph()
        G.add_edges_from(self.edges)
        return G


def query_interval_trees(interval_trees, data, overlap_cutoff, jaccard_threshold, edge_threshold, qlen_diff, diff):
    """cluster.py:187-227 on the GPU.

    Returns ``(match_df, G)``.  The pair kernels evaluate every candidate pair
    (E*); when a read has more than ``edge_threshold`` forward partners, the
    reference's per-read cap (cluster.py:223-224) is replayed exactly
    (``fslr_apply_edge_cap``; search order of the superintervals stand-in,
    SURVEY.md §8c).  ``match_df`` rows are the graph's edges as the reference
    records them — (read whose loop formed the edge, partner, I/U as a Python
    float) — sorted by (query1 rank, query2 rank); the reference's row order is
    set order (arbitrary).
    """
    g = query_graph(interval_trees, data, overlap_cutoff, jaccard_threshold, edge_threshold, qlen_diff, diff)
    return _graph_outputs(g.data.qnames[g.csr.read_qcode], g.labels, g.a, g.b, g.I, g.U, g.fwd, g.stats)


class RawGraph:
    """query_graph's result: the graph over read ranks without qname strings (the CLI's columnar
    path maps ranks to qname codes itself).  Edges sorted by (a, b).

    ``a, b, I, U`` and ``fwd`` are arrays, or — from a single-GPU query — ``edges`` / ``fwd`` loaders
    that copy them off the device on first use (the CLI needs only the labels and the edge count)."""

    def __init__(self, data, csr, labels, a=None, b=None, I=None, U=None, fwd=None, st=None, *, edges=None,
                 n_edges=None):
        self.data, self.csr, self.labels, self.stats = data, csr, labels, st
        self._raw = (a, b, I, U) if edges is None else edges
        self._fwd = fwd
        self._sorted = None
        self.n_edges = int(a.shape[0]) if n_edges is None else int(n_edges)

    @property
    def fwd(self):
        if callable(self._fwd):
            self._fwd = self._fwd()
        return self._fwd

    def _edges(self):
        if self._sorted is None:                    # fetched and sorted on first use
            raw = self._raw() if callable(self._raw) else self._raw
            a, b, I, U = raw
            order = np.lexsort((b, a))
            self._sorted = (a[order], b[order], I[order], U[order])
            self._raw = None
        return self._sorted

    a = property(lambda self: self._edges()[0])
    b = property(lambda self: self._edges()[1])
    I = property(lambda self: self._edges()[2])
    U = property(lambda self: self._edges()[3])


def query_graph(interval_trees, data, overlap_cutoff, jaccard_threshold, edge_threshold, qlen_diff, diff):
    """query_interval_trees without the match_df / qname outputs: a RawGraph."""
    min(jaccard_threshold)                              # cluster.py:188 raises on an empty list
    if isinstance(interval_trees, MultiGpuIndex) and (interval_trees.source is data or interval_trees.data is data):
        mg = interval_trees
        thr = fold_overlap_threshold(mg.csr.iv_aln, overlap_cutoff)
        # the sweep split, or for overlap <= 0, an aln_size == 0 interval or reads of more than 64
        # intervals the query-shard split
        return _query_multi_gpu(mg, thr, jaccard_threshold, edge_threshold, qlen_diff, diff)
    if not isinstance(interval_trees, DeviceIntervalIndex) or (interval_trees.source is not data and
                                                               interval_trees.data is not data):
        interval_trees = DeviceIntervalIndex(data)
    idx = interval_trees
    data = idx.data
    csr = idx.csr
    ctx = idx.ctx
    if csr.nal_varies:
        warnings.warn('n_alignments differs between rows of one read; the reference then uses the row its '
                      'search reaches first (order-dependent); the first row in data order is used', EdgeCapWarning)
    if idx.long is not None:
        return _query_long(idx, overlap_cutoff, jaccard_threshold, edge_threshold, qlen_diff, diff)
    if isinstance(idx, RowsIndex):
        if idx.overlap != float(overlap_cutoff):             # folded on the device at the upload
            ctx.fold_thresholds(overlap_cutoff)
            idx.overlap = float(overlap_cutoff)
    else:
        ctx.set_thresholds(fold_overlap_threshold(csr.iv_aln, overlap_cutoff))
    pt = pass_table(jaccard_threshold)
    qcut = 1 - qlen_diff
    ncut = 1 - diff
    ctx.reserve_edges(max(1 << 16, 12 * csr.n_reads))
    st = ctx.run_query(qcut, ncut, pt, int(edge_threshold))
    st['cap'] = ctx.apply_edge_cap(int(edge_threshold))
    st['n_edges'] = ctx.stats()['n_edges']
    st['max_fwd'] = st['cap']['max_fwd']
    ctx.components()
    labels = ctx.labels()
    ne = st['n_edges']
    # the edges and forward degrees stay in HBM until asked for (query_interval_trees does at once;
    # the CLI never does); this context's next query would replace them
    gen = ctx.query_gen = getattr(ctx, 'query_gen', 0) + 1

    def fetch(what):
        if getattr(ctx, 'query_gen', 0) != gen:
            raise RuntimeError('the graph\'s context has run another query since')
        return ctx.edges(ne) if what == 'edges' else ctx.fwd_degree()
    return RawGraph(data, csr, labels, fwd=lambda: fetch('fwd'), st=st, edges=lambda: fetch('edges'), n_edges=ne)


def _graph_outputs(qnames_by_rank, labels, a, b, I, U, fwd, st):
    order = np.lexsort((b, a))
    a, b, I, U = a[order], b[order], I[order], U[order]
    ne = int(a.shape[0])
    match_df = pd.DataFrame({'query1': qnames_by_rank[a] if ne else np.zeros(0, object),
                             'query2': qnames_by_rank[b] if ne else np.zeros(0, object),
                             'jaccard_similarity': I / U if ne else np.zeros(0)})
    return match_df, ClusterGraph(qnames_by_rank, labels, (a, b), fwd, st)


def _query_long(idx, overlap_cutoff, jaccard_threshold, edge_threshold, qlen_diff, diff):
    """query_interval_trees with reads of more than FSLR_MAX_L intervals.

    E*: where the sweep's gates apply (overlap > 0, no aln_size == 0 interval, no long read with qlen2
    or n_alignments 0), the sweep over the virtual CSR writes every match entry; pairs of two short
    reads are decided by its pair stage, pairs with a long read by the first-fit over their whole
    lists (fslr_long_query).  Otherwise every distinct pair goes through the general evaluator
    (fslr_long_pairs).  When a read has more than ``edge_threshold`` forward edges, the reference's
    per-read cap (cluster.py:223-224) is replayed over E* in the real-read space
    (fslr_cap_replay_pairs)."""
    csr, ctx = idx.csr, idx.ctx
    rlen = idx.long
    n = csr.n_reads
    thr = fold_overlap_threshold(csr.iv_aln, overlap_cutoff)           # the real CSR's order
    lg = rlen > FSLR_MAX_L
    fast = (multi.sweep_applies(csr, thr) and not (csr.read_qlen2[lg] == 0).any()
            and not (csr.read_nal[lg] == 0).any())
    ctx.set_thresholds(thr)
    ctx.set_long_cutoffs(umax_table(jaccard_threshold, int(rlen.max())))
    pt = pass_table(jaccard_threshold)
    qcut, ncut = 1 - qlen_diff, 1 - diff
    ctx.reserve_edges(max(1 << 16, 12 * n))
    if fast:
        while True:
            n_long = ctx.long_query(qcut, ncut, pt, int(edge_threshold))
            st = ctx.stats(check=False)
            if st['n_edges'] <= st['edge_capacity']:
                break
            ctx.reserve_edges(int(st['n_edges'] * 1.25) + 4096)
        st = ctx.stats()
        la, lb, lI, lU = ctx.long_edges(n_long)
        a, b, I, U = ctx.edges(st['n_edges'])
        a, b = np.concatenate([a, la]), np.concatenate([b, lb])
        I, U = np.concatenate([I, lI]), np.concatenate([U, lU])
        engine = 'sweep+long'
    else:
        n_long = ctx.long_pairs(qcut, ncut, pt, int(edge_threshold))
        st = ctx.stats()
        a, b, I, U = ctx.long_edges(n_long)
        engine = 'pairs'
    fwd = np.bincount(a, minlength=n).astype(np.int32)
    max_fwd = int(fwd.max()) if n else 0
    if st.get('zd_pairs', 0) and max_fwd <= int(edge_threshold):
        # every loop runs to its end, so each listed pair is visited (cluster.py:178-183, 133-136); with
        # the cap binding the replay decides (fslr_cap_replay_pairs raises where a loop reaches one)
        raise ZeroDivisionError('division by zero')
    cap = {'applied': 0, 'max_fwd': max_fwd}
    if max_fwd > int(edge_threshold):
        # the capped graph: edge k kept when formed in a loop, re-oriented as (former, partner)
        who, fwd, cap = ctx.cap_replay_pairs(int(edge_threshold), a, b, n)
        keep = who != 2
        a, b = np.where(who == 0, a, b)[keep], np.where(who == 0, b, a)[keep]
        I, U = I[keep], U[keep]
        ctx.components()
        labels = ctx.labels()[:n]
    elif fast:
        ctx.components()
        if n_long:
            ctx.union_pairs(la, lb, n_long, on_device=False)
            ctx.finalize_labels()
        labels = ctx.labels()[:n]
    else:
        ctx.components()
        labels = ctx.labels()[:n]
    st = dict(st, engine=engine, n_edges=int(a.shape[0]), max_fwd=max_fwd, long_reads=int(lg.sum()),
              long_pair_edges=int(n_long), cap=cap)
    return RawGraph(idx.data, csr, labels, a, b, I, U, fwd, st)


def _query_multi_gpu(mg, thr, jaccard_threshold, edge_threshold, qlen_diff, diff):
    """query_interval_trees over ``mg.n_gpus`` ranks (fslr_amd.multi): same edges, forward degrees and
    labels as one GPU (union of per-chromosome matchings, label union; the cap replayed on rank 0)."""
    data, csr = mg.data, mg.csr
    if csr.nal_varies:
        warnings.warn('n_alignments differs between rows of one read; the reference then uses the row its '
                      'search reaches first (order-dependent); the first row in data order is used', EdgeCapWarning)
    r = multi.query(csr, thr, 1 - qlen_diff, 1 - diff, pass_table(jaccard_threshold), int(edge_threshold),
                    mg.n_gpus, first_device=mg.first_device, cutoffs=list(jaccard_threshold))
    a, b, I, U = r['edges']
    st = {'engine': r.get('path', 'sweep'), 'n_gpus': mg.n_gpus, 'backend': r['backend'], 'evaluated_pairs': -1,
          'n_edges': int(a.shape[0]), 'max_fwd': r['max_fwd'], 'cap': r['cap'], 'capped': r['capped']}
    return RawGraph(data, csr, np.asarray(r['labels']), a, b, I, U, r['fwd'], st)


class ClusterTable:
    """The cluster table of a label vector (fslr_cluster_table), on the host: ``cid[r]`` the dense id of
    read rank r's component among the components of two or more reads in networkx order (ascending smallest
    rank), -1 for a read alone; ``size[r]`` its component's size; ``roots[k]`` cluster k's smallest rank;
    cluster k's ranks, ascending, are ``members[off[k]:off[k + 1]]``."""

    def __init__(self, cid, size, off, members, info):
        self.cid, self.size, self.off, self.members = cid, size, off, members
        self.n_clusters, self.n_nodes, self.max_size = info['n_clusters'], info['n_nodes'], info['max_size']
        self.roots = members[off[:-1]]

    def __len__(self):
        return int(self.n_clusters)


def _labels_of(G_or_labels):
    return np.asarray(getattr(G_or_labels, 'labels', G_or_labels))


def cluster_table(G_or_labels, ctx=None, device=None) -> ClusterTable:
    """The ClusterTable of a ClusterGraph, a RawGraph or a vector of min-rank labels, made on the device.
    The table stays resident in ``ctx`` (Context.assign_clusters reads it); without ``ctx`` a context on
    ``device`` is opened for the call."""
    labels = _labels_of(G_or_labels)
    own = ctx is None
    ctx = ctx or Context(_default_device() if device is None else device)
    try:
        info = ctx.cluster_table(labels)
        cid, size = ctx.cluster_ids()
        off, members = ctx.cluster_members()
    finally:
        if own:
            ctx.close()
    return ClusterTable(cid, size, off, members, info)


def get_subgraphs(G, ctx=None):
    """cluster.py:230-234: connected components, in the reference's order (by min read rank).  With ``ctx``
    the sets come from the device member CSR (fslr_cluster_table)."""
    if isinstance(G, ClusterGraph):
        if ctx is not None:
            t = cluster_table(G, ctx=ctx)
            names, off = G.qnames_by_rank[t.members].tolist() if t.n_nodes else [], t.off.tolist()
            return [set(names[off[k]:off[k + 1]]) for k in range(t.n_clusters)]
        return G.components()
    import networkx as nx
    return list(nx.connected_components(G))


def choose_alignment(bed_file, ctx=None):
    """cluster.py:237-254: per cluster the read with the highest mean alignment_score (first on ties).
    With ``ctx`` (and a frame _choose_alignment_codes takes) the per-cluster argmax runs on the device."""
    fast = _choose_alignment_codes(bed_file, ctx)
    if fast is not None:
        return fast
    avg = bed_file.groupby('qname')['alignment_score'].mean()
    bed_file['avg_alignment_score'] = bed_file['qname'].map(avg)
    sel = bed_file.groupby('cluster')['avg_alignment_score'].idxmax()
    chosen = bed_file.loc[sel.to_numpy(), 'qname']
    return bed_file[bed_file['qname'].isin(chosen)]


def _choose_alignment_codes(bed_file, ctx=None):
    """choose_alignment from the reader's qname codes (ingest.QnameCodes), for an int64
    alignment_score and numeric cluster ids, or None.

    groupby('qname').mean() of int64 scores: the float64 sum of integers below 2**53 is exact in any
    order (pandas' compensated sum included), divided by the count, so bincount gives the same
    doubles.  groupby('cluster').idxmax() = the first row (in frame order) holding its cluster's
    maximum; scores and clusters are constant per qname, so it is the earliest first row among
    the cluster's qnames with the maximal mean.  With ``ctx`` the means and that argmax come from
    fslr_choose_representatives (the same doubles: one IEEE division per qname)."""
    if not isinstance(bed_file.attrs.get(ingest.ATTR), ingest.QnameCodes) or 'cluster' not in bed_file:
        return None
    score = bed_file['alignment_score'].to_numpy()
    cl = bed_file['cluster'].to_numpy()
    if score.dtype != np.int64 or cl.dtype.kind not in 'iuf' or not len(cl):
        return None
    if np.abs(score).max() >= (1 << 53) // max(1, len(score)):
        return None
    codes, uniq = ingest.factorize_qname(bed_file)
    nq = len(uniq)
    sums = np.bincount(codes, weights=score.astype(np.float64), minlength=nq)
    cnt = np.bincount(codes, minlength=nq)
    avg_q = sums / cnt
    first_row = np.full(nq, -1, dtype=np.int64)
    first_row[codes[::-1]] = np.arange(len(codes) - 1, -1, -1)
    cl_q = cl[first_row]
    if cl.dtype.kind == 'f':
        if np.isnan(cl_q).any() or (cl_q != np.floor(cl_q)).any() or cl_q.min() < 0:
            return None
    if (cl != cl_q[codes]).any():                      # cluster not constant per qname
        return None
    cid = cl_q.astype(np.int64)
    k = int(cid.max()) + 1
    if ctx is not None:
        avg_q, win = ctx.choose_representatives(cid, sums.astype(np.int64), cnt, first_row, k)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        bed_file['avg_alignment_score'] = avg_q[codes]
    if ctx is not None:
        chosen = np.zeros(nq, dtype=bool)
        chosen[win[win >= 0]] = True
        return bed_file[chosen[codes]]
    best = np.full(k, -np.inf)
    np.maximum.at(best, cid, avg_q)
    cand = np.flatnonzero(avg_q == best[cid])
    win_row = np.full(k, len(codes), dtype=np.int64)
    np.minimum.at(win_row, cid[cand], first_row[cand])
    chosen = np.zeros(nq, dtype=bool)
    chosen[codes[win_row[win_row < len(codes)]]] = True
    return bed_file[chosen[codes]]
