#!/usr/bin/env python3
"""Capture the reference's own calc_coverage / filter_high_coverage (cluster.py:52-77) on a tiny input.

    python tests/golden/make_coverage_golden.py

Runs on the CPU where the reference is present (refharness.load()) and writes
``tests/golden/coverage/small.npz``, which holds data only:

* ``bed_chrom / bed_rstart / bed_rend``: about 2,000 rows on chromosomes 1, 2, 5 (lengths 3000, 777,
  1200) and 9 (in the bed, without a length); chromosome 7 has a length and no rows.  Among them rows
  with rstart == rend, rows with rstart > rend (the depth goes negative in between), positions at 0 and
  at the length, and two piles of equal rstart / equal rend.
* ``len_chrom / len_value``: the lengths.  ``cov_<chrom>``: the reference's dense array (its float64
  values are whole numbers; stored as int32).
* ``data_*``: the columns of a ``data`` list of IntervalItem (two negative ``middle`` values wrap);
  ``thresholds`` and ``kept_<k>``: the positions of the items filter_high_coverage kept for each.
* ``wrap_*``: a second small bed with negative rstart / rend inside ``[-(len + 1), -1]`` and its dense
  arrays.
* ``err<k>_*``: inputs on which the reference raises, with the exception's class name in
  ``err<k>_type`` (bed positions out of range; a ``data`` item on a chromosome without coverage or with
  a ``middle`` out of range).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

LENGTHS = {1: 3000, 2: 777, 5: 1200, 7: 500}
THRESHOLDS = (25, 60)
DATA_COLUMNS = ('chrom', 'start', 'end', 'aln_size', 'n_alignments', 'qlen2', 'middle', 'index')


def make_bed(rng):
    chrom, rs, re_ = [], [], []

    def add(c, a, b):
        chrom.append(c), rs.append(a), re_.append(b)
    for c, n in ((1, 900), (2, 450), (5, 500)):
        L = LENGTHS[c]
        a = rng.integers(0, L + 1, n)
        w = rng.integers(1, L // 10, n)
        b = np.minimum(a + w, L)
        rev = rng.random(n) < np.where(a > 0.7 * L, 0.8, 0.1)     # rstart > rend, most rows of the last third
        same = rng.random(n) < 0.04                    # rstart == rend
        for x, y, r, s in zip(a.tolist(), b.tolist(), rev.tolist(), same.tolist()):
            add(c, x, x) if s else add(c, y, x) if r else add(c, x, y)
        add(c, 0, L), add(c, L, 0), add(c, 0, 0), add(c, L, L)
    for k in range(60):                                # piles: one rstart, one rend
        add(1, 1500, 1500 + 10 * k + 1)
        add(5, 100 + 7 * k, 900)
    for x in rng.integers(0, 400, 40).tolist():        # a chromosome without a length
        add(9, x, x + 50)
    order = rng.permutation(len(chrom))
    return tuple(np.asarray(v, np.int64)[order] for v in (chrom, rs, re_))


def make_data(rng, n=600):
    chrom = rng.choice([1, 2, 5], n)
    L = np.array([LENGTHS[c] for c in chrom.tolist()])
    start = (rng.random(n) * (L - 60)).astype(np.int64)
    aln = rng.integers(2, 120, n)
    middle = aln // 2 + start
    middle[:6] = [0, LENGTHS[chrom[1]], 1500, -1, -LENGTHS[chrom[4]] - 1, LENGTHS[chrom[5]] - 1]
    chrom[2] = 1
    order = np.argsort(start, kind='stable')
    cols = dict(chrom=chrom, start=start, end=start + aln, aln_size=aln, n_alignments=rng.integers(3, 9, n),
                qlen2=rng.integers(500, 5000, n), middle=middle, index=np.arange(n))
    return {k: np.asarray(v, np.int64)[order] for k, v in cols.items()}


def items(cluster, cols):
    n = cols['chrom'].size
    return [cluster.IntervalItem(*(int(cols[c][i]) for c in DATA_COLUMNS[:4]), f'q{int(cols["index"][i])}',
                                 *(int(cols[c][i]) for c in DATA_COLUMNS[4:])) for i in range(n)]


def frame(chrom, rs, re_):
    import pandas as pd
    return pd.DataFrame({'chrom': chrom, 'rstart': rs, 'rend': re_})


def error_cases():
    """(bed columns, data chrom, data middle): each makes the reference raise."""
    small = ([1, 1, 2, 2, 5], [10, 200, 5, 300, 40], [90, 100, 70, 777, 41])

    def bed(row, col, value):
        b = [list(v) for v in small]
        b[col][row] = value
        return tuple(b)
    ok = (small, [1], [10])
    return [(bed(2, 1, 778), [2], [5]),                # rstart one past the array's end
            (bed(3, 2, -779), [2], [5]),               # rend one below the wrap range
            (bed(0, 1, 3001), [1], [10]),              # the lower chromosome's rstart raises first
            (ok[0], [7], [10]),                        # a length, no rows
            (ok[0], [9], [10]),                        # no length
            (ok[0], [1, 2, 5], [10, 778, 3]),          # middle one past the array's end
            (ok[0], [1, 2, 7], [10, -779, 3])]         # middle below the wrap range comes before the KeyError


def main():
    import refharness
    cluster, _ = refharness.load()
    rng = np.random.default_rng(20240611)
    out = {}
    chrom, rs, re_ = make_bed(rng)
    out.update(bed_chrom=chrom, bed_rstart=rs, bed_rend=re_, len_chrom=np.array(list(LENGTHS), np.int64),
               len_value=np.array(list(LENGTHS.values()), np.int64))
    cov = cluster.calc_coverage(frame(chrom, rs, re_), LENGTHS)
    assert sorted(cov) == [1, 2, 5]
    for c, v in cov.items():
        assert v.dtype == np.float64 and v.shape == (LENGTHS[c] + 1,) and (v == np.rint(v)).all()
        out[f'cov_{c}'] = v.astype(np.int32)
    assert min(v.min() for v in cov.values()) < -5 and max(v.max() for v in cov.values()) > THRESHOLDS[1]
    cols = make_data(rng)
    out.update({f'data_{k}': v for k, v in cols.items()})
    data = items(cluster, cols)
    out['thresholds'] = np.array(THRESHOLDS, np.int64)
    for k, t in enumerate(THRESHOLDS):
        kept = cluster.filter_high_coverage(data, frame(chrom, rs, re_), LENGTHS, t)
        pos = {id(x): i for i, x in enumerate(data)}
        out[f'kept_{k}'] = np.array([pos[id(x)] for x in kept], np.int64)
        assert 0 < len(kept) < len(data), (t, len(kept))
    wrap = (np.array([2, 2, 2, 5, 5]), np.array([-778, -1, 30, -1201, 7]), np.array([-2, 40, -700, -600, -1]))
    out.update(wrap_chrom=wrap[0], wrap_rstart=wrap[1], wrap_rend=wrap[2])
    for c, v in cluster.calc_coverage(frame(*wrap), LENGTHS).items():
        out[f'wrap_cov_{c}'] = v.astype(np.int32)
    cases = error_cases()
    out['n_err'] = np.array(len(cases))
    for k, (b, dc, dm) in enumerate(cases):
        d = [cluster.IntervalItem(c, 0, 1, 1, 'q', 3, 100, m, i) for i, (c, m) in enumerate(zip(dc, dm))]
        try:
            cluster.filter_high_coverage(d, frame(*b), LENGTHS, 10)
        except (IndexError, KeyError) as e:
            out[f'err{k}_type'] = np.array(type(e).__name__)
        else:
            raise AssertionError(f'error case {k} did not raise')
        out.update({f'err{k}_bed_chrom': np.array(b[0]), f'err{k}_bed_rstart': np.array(b[1]),
                    f'err{k}_bed_rend': np.array(b[2]), f'err{k}_data_chrom': np.array(dc),
                    f'err{k}_data_middle': np.array(dm)})
    path = os.path.join(HERE, 'coverage', 'small.npz')
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes;', len(chrom), 'rows; depth',
          min(int(v.min()) for v in cov.values()), '..', max(int(v.max()) for v in cov.values()),
          '; kept', [int(out[f'kept_{k}'].size) for k in range(len(THRESHOLDS))], 'of', len(data),
          '; errors', [str(out[f'err{k}_type']) for k in range(len(cases))])


if __name__ == '__main__':
    main()
