#!/usr/bin/env python
"""Time removing reads from a resident set (not a test): a 1M-read synth resident set (the cfg3 generator) with
m random reads removed, two ways that leave the same context:

  remove   fslr_remove_reads of the keep mask (by fslr_remove_timings and by wall clock)
  fresh    what a caller had to do before: prep.remove_reads_csr on the host, then fslr_set_reads of the
           survivors

Both end before fslr_build_index.  After the timed runs both contexts build the index and query; the edges must
be equal.  Prints one JSON line per m.  Warm-up runs come first; the figures are medians over --repeats.  Before
every timed removal the context is set back to the resident reads with its index built (not timed)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fslr_amd import _lib, synth                                         # noqa: E402
from fslr_amd.prep import fold_overlap_threshold, pass_table, remove_reads_csr   # noqa: E402

CUTOFFS = (1, 1, 0.66, 0.66, 0.66, 0.5)
PCT, QCUT, NCUT = 0.8, 1 - 0.04, 1 - 0.25


def edges_of(ctx, n_reads, pt):
    ctx.reserve_edges(max(1 << 16, 12 * n_reads))
    ctx.build_index()
    st = ctx.run_query(QCUT, NCUT, pt)
    a, b, I, U = ctx.edges(st['n_edges'])
    o = np.lexsort((b, a))
    return a[o], b[o], I[o], U[o]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--resident', type=int, default=1_000_000)
    ap.add_argument('--remove', type=int, nargs='+', default=[10_000, 100_000])
    ap.add_argument('--lmax', type=int, default=16)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=5)
    args = ap.parse_args()
    pt = pass_table(CUTOFFS)
    ctx, ctx2 = _lib.Context(0), _lib.Context(0)
    ctx.set_profiling(2)
    med = statistics.median
    res = synth.generate(args.resident, args.lmax, 11).interval_data().csr()
    thr = fold_overlap_threshold(res.iv_aln, PCT)
    lens = np.diff(np.asarray(res.read_off, np.int64))
    for m in args.remove:
        keep = np.ones(res.n_reads, bool)
        keep[np.random.default_rng(m).choice(res.n_reads, m, replace=False)] = False
        keep_iv = np.repeat(keep, lens)
        wall_r, wall_f, dev = [], [], []
        for k in range(args.warmup + args.repeats):
            ctx.load_csr(res, thr)
            ctx.build_index()
            ctx.sync()
            t = time.perf_counter()
            ctx.remove_reads(keep)
            tr = time.perf_counter() - t
            d = ctx.remove_timings()
            t = time.perf_counter()
            out, _ = remove_reads_csr(res, keep)
            ctx2.load_csr(out, thr[keep_iv])
            tf = time.perf_counter() - t
            if k >= args.warmup:
                wall_r.append(tr), wall_f.append(tf), dev.append(d)
        for x, y in zip(edges_of(ctx, out.n_reads, pt), edges_of(ctx2, out.n_reads, pt)):
            np.testing.assert_array_equal(x, y)                          # the same edges both ways
        n, ni, nk, nik = res.n_reads, res.n_intervals, out.n_reads, out.n_intervals
        # algorithmic bytes.  Maps: every record's line for its tag (16) per interval; keep and
        # length bytes twice, the read's rmeta (16), its maps written (8) per read, its compacted rmeta and
        # length (17) per kept read.  Compaction: record, gate word, chromosome read (28) per interval and
        # written (28) with the new position (4) per kept interval; in CSR order iv, data_pos and newpos[] read
        # (24) per interval, iv and data_pos written (20) per kept interval.
        maps = ni * 16 + n * (4 + 16 + 8) + nk * 17
        compact = ni * (28 + 24) + nik * (28 + 4 + 20)
        maps_ms, compact_ms = med([x['maps'] for x in dev]), med([x['compact'] for x in dev])
        print(json.dumps(dict(resident_reads=n, resident_intervals=ni, removed_reads=m, removed_intervals=ni - nik,
                              remove_wall_ms=round(1e3 * med(wall_r), 2), fresh_wall_ms=round(1e3 * med(wall_f), 2),
                              remove_device_ms={k: round(med([x[k] for x in dev]), 3) for k in dev[0]},
                              h2d_bytes_remove=int(n), h2d_bytes_fresh=int(4 * (3 * nk + 1 + 5 * nik)),
                              maps_algo_bytes=int(maps), maps_gb_per_s=round(maps / maps_ms / 1e6, 1),
                              compact_algo_bytes=int(compact), compact_gb_per_s=round(compact / compact_ms / 1e6, 1),
                              repeats=args.repeats, warmup=args.warmup)), flush=True)
    ctx.close()
    ctx2.close()


if __name__ == '__main__':
    main()
