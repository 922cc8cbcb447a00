#!/usr/bin/env python
"""Time matching new reads against a resident index (not a test): a 1M-read synth resident set (the cfg3
generator) and 100k query reads drawn from the same generator, two ways that give the same rows:

  match      fslr_match_reads + fslr_match_rows (by fslr_match_timings and by wall clock)
  composed   what a caller could do before: fslr_search + fslr_search_hits on every query interval, the
             seen-set on the host, a second upload of the resident reads with the query reads appended,
             fslr_score_pairs

Prints one JSON line.  Warm-up runs come first; the figures are medians over --repeats."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fslr_amd import _lib, synth                                         # noqa: E402
from fslr_amd._lib import SCORE_EDGE                                     # noqa: E402
from fslr_amd.prep import fold_overlap_threshold, pass_table             # noqa: E402

CUTOFFS = (1, 1, 0.66, 0.66, 0.66, 0.5)
PCT, QCUT, NCUT = 0.8, 1 - 0.04, 1 - 0.25


def composed(ctx, ctx2, res, qry, thr_r, thr_q, pt, emit_mask):
    """The path of the parent commit; returns (offsets, partner, I, U, flags, n_hits)."""
    n = res.n_reads
    off, hits = ctx.search(qry.iv_chrom, qry.iv_start, qry.iv_end)
    read_of = np.repeat(np.arange(n, dtype=np.int32), np.diff(res.read_off))
    p = read_of[hits]
    q_of_iv = np.repeat(np.arange(qry.n_reads), np.diff(qry.read_off))
    q_of_hit = np.repeat(q_of_iv, np.diff(off))
    # the seen-set: the first hit of every (query read, partner), in visiting order
    key = q_of_hit.astype(np.int64) * n + p
    _, first = np.unique(key, return_index=True)
    first.sort()
    a, b = q_of_hit[first], p[first]
    ctx2.set_reads(np.concatenate([res.read_off, res.read_off[-1] + qry.read_off[1:]]),
                   np.concatenate([res.read_qlen2, qry.read_qlen2]), np.concatenate([res.read_nal, qry.read_nal]),
                   np.concatenate([res.iv_chrom, qry.iv_chrom]), np.concatenate([res.iv_start, qry.iv_start]),
                   np.concatenate([res.iv_end, qry.iv_end]), np.concatenate([thr_r, thr_q]), res.n_chroms)
    I, U, flags = ctx2.score_pairs(n + a, b, QCUT, NCUT, pt)
    keep = (flags & emit_mask) != 0 if emit_mask else np.ones(flags.size, bool)
    offsets = np.zeros(qry.n_reads + 1, np.int64)
    np.cumsum(np.bincount(a[keep], minlength=qry.n_reads), out=offsets[1:])
    return offsets, b[keep], I[keep], U[keep], flags[keep], int(hits.size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--resident', type=int, default=1_000_000)
    ap.add_argument('--queries', type=int, default=100_000)
    ap.add_argument('--lmax', type=int, default=16)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--emit', choices=('edges', 'gated', 'all'), default='edges')
    args = ap.parse_args()
    emit_mask = {'edges': SCORE_EDGE, 'gated': 1, 'all': 0}[args.emit]
    pt = pass_table(CUTOFFS)
    # one draw of resident + query reads, so the query reads share the resident reads' events; every k-th
    # read rank is taken out as a query read
    data = synth.generate(args.resident + args.queries, args.lmax, 11).interval_data()
    both = data.csr()
    out = np.zeros(both.n_reads, bool)
    out[np.linspace(0, both.n_reads - 1, args.queries).astype(np.int64)] = True
    pos = np.zeros(len(data), bool)
    pos[np.asarray(both.data_pos, np.int64)] = np.repeat(out, np.diff(both.read_off))
    res, qdata = data.select(~pos).csr(), data.select(pos)
    qry = qdata.csr()
    # the query reads' chromosomes as the resident CSR's dense ids (both number the chromosomes present ascending)
    keys = np.unique(np.asarray(data.chrom)[~pos])
    raw = np.asarray(qdata.chrom)[np.asarray(qry.data_pos, np.int64)]
    at = np.minimum(np.searchsorted(keys, raw), keys.size - 1)
    qry.iv_chrom = np.where(keys[at] == raw, at, -1).astype(np.int32)
    thr_r, thr_q = fold_overlap_threshold(res.iv_aln, PCT), fold_overlap_threshold(qry.iv_aln, PCT)
    ctx, ctx2 = _lib.Context(0), _lib.Context(0)
    ctx.set_profiling(2)
    ctx.load_csr(res, thr_r)
    ctx.build_index()
    ctx.sync()

    def match():
        off, counts, best = ctx.match_reads(qry.read_off, qry.read_qlen2, qry.read_nal, qry.iv_chrom, qry.iv_start,
                                            qry.iv_end, thr_q, QCUT, NCUT, pt, emit_mask)
        return (off, *ctx.match_rows(), counts)
    wall_m, wall_c, dev = [], [], []
    for k in range(args.warmup + args.repeats):
        t = time.perf_counter()
        m = match()
        tm = time.perf_counter() - t
        d = ctx.match_timings()
        t = time.perf_counter()
        c = composed(ctx, ctx2, res, qry, thr_r, thr_q, pt, emit_mask)
        tc = time.perf_counter() - t
        if k >= args.warmup:
            wall_m.append(tm), wall_c.append(tc), dev.append(d)
    for x, y in zip(m[:5], c[:5]):
        np.testing.assert_array_equal(x, y)                              # the same rows both ways
    try:
        commit = subprocess.run(['git', 'rev-parse', '--short', 'HEAD'], capture_output=True, text=True,
                                cwd=os.path.dirname(os.path.abspath(__file__))).stdout.strip()
    except OSError:
        commit = ''
    med = statistics.median
    print(json.dumps(dict(resident_reads=res.n_reads, query_reads=qry.n_reads, emit=args.emit, hits=c[5],
                          candidates=int(m[5][:, 0].sum()), rows=int(m[1].size),
                          match_wall_ms=round(1e3 * med(wall_m), 2), composed_wall_ms=round(1e3 * med(wall_c), 2),
                          match_device_ms={k: round(med([d[k] for d in dev]), 3) for k in dev[0]},
                          repeats=args.repeats, warmup=args.warmup, parent_commit=commit)))
    ctx.close()
    ctx2.close()


if __name__ == '__main__':
    main()
