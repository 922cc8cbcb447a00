#!/usr/bin/env python
"""Time appending reads to a resident set (not a test): a 1M-read synth resident set (the cfg3 generator) and
m reads held out of the same draw, two ways that leave the same context:

  append   fslr_append_reads of the m reads (by fslr_append_timings and by wall clock)
  fresh    what a caller had to do before: concatenate the CSR on the host, merge the data positions, and
           fslr_set_reads of the union

After the timed runs both contexts build the index and query; the edges must be equal.  Prints one JSON line
per m with the held-out reads where the draw put them ('spread': nearly every merge tile mixes both lists),
and one for the largest m with the new reads moved above every resident start ('above': every merge tile but
the last few is a straight copy of resident elements).  Warm-up runs come first; the figures are medians over
--repeats.  Before every timed append the context is set back to the resident reads with its index built
(not timed)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fslr_amd import _lib, synth                                         # noqa: E402
from fslr_amd.prep import CSR, fold_overlap_threshold, pass_table        # noqa: E402

CUTOFFS = (1, 1, 0.66, 0.66, 0.66, 0.5)
PCT, QCUT, NCUT = 0.8, 1 - 0.04, 1 - 0.25


def union_csr(res, new):
    """The host work of the fresh route: the concatenated CSR with the merged data positions."""
    a = np.empty(res.n_intervals, np.int64)
    a[np.asarray(res.data_pos, np.int64)] = res.iv_start
    b = np.empty(new.n_intervals, np.int64)
    b[np.asarray(new.data_pos, np.int64)] = new.iv_start
    pos_res = np.arange(a.size, dtype=np.int64) + np.searchsorted(b, a, side='left')
    pos_new = np.arange(b.size, dtype=np.int64) + np.searchsorted(a, b, side='right')
    cat = lambda f: np.concatenate([getattr(res, f), getattr(new, f)])
    return CSR(read_off=np.concatenate([res.read_off, res.n_intervals + new.read_off[1:]]).astype(np.int32),
               read_qlen2=cat('read_qlen2'), read_nal=cat('read_nal'), iv_chrom=cat('iv_chrom'), iv_start=cat('iv_start'),
               iv_end=cat('iv_end'), iv_aln=cat('iv_aln'), n_chroms=max(res.n_chroms, new.n_chroms),
               read_qcode=cat('read_qcode'),
               data_pos=np.concatenate([pos_res[np.asarray(res.data_pos, np.int64)], pos_new[np.asarray(new.data_pos, np.int64)]]),
               nal_varies=False)


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
    ap.add_argument('--append', type=int, nargs='+', default=[10_000, 100_000])
    ap.add_argument('--lmax', type=int, default=16)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=5)
    args = ap.parse_args()
    pt = pass_table(CUTOFFS)
    ctx, ctx2 = _lib.Context(0), _lib.Context(0)
    ctx.set_profiling(2)
    med = statistics.median
    for m, placement in [(m, 'spread') for m in args.append] + [(max(args.append), 'above')]:
        # one draw of resident + new reads, so the new reads share the resident reads' events; every k-th read
        # rank is held out
        data = synth.generate(args.resident + m, args.lmax, 11).interval_data()
        both = data.csr()
        out = np.zeros(both.n_reads, bool)
        out[np.linspace(0, both.n_reads - 1, m).astype(np.int64)] = True
        pos = np.zeros(len(data), bool)
        pos[np.asarray(both.data_pos, np.int64)] = np.repeat(out, np.diff(both.read_off))
        res, ndata = data.select(~pos).csr(), data.select(pos)
        new = ndata.csr()
        # the new reads' chromosomes as the resident CSR's dense ids (both number the chromosomes present ascending)
        keys = np.unique(np.asarray(data.chrom)[~pos])
        raw = np.asarray(ndata.chrom)[np.asarray(new.data_pos, np.int64)]
        assert np.isin(raw, keys).all()
        new.iv_chrom = np.searchsorted(keys, raw).astype(np.int32)
        new.n_chroms = res.n_chroms
        if placement == 'above':                 # the same reads, moved as one block above every resident start
            shift = 1 << 29
            assert max(int(res.iv_end.max()), int(new.iv_end.max())) < shift
            new.iv_start, new.iv_end = new.iv_start + np.int32(shift), new.iv_end + np.int32(shift)
        thr_r, thr_n = fold_overlap_threshold(res.iv_aln, PCT), fold_overlap_threshold(new.iv_aln, PCT)
        wall_a, wall_f, dev = [], [], []
        for k in range(args.warmup + args.repeats):
            ctx.load_csr(res, thr_r)
            ctx.build_index()
            ctx.sync()
            t = time.perf_counter()
            ctx.append_csr(new, thr_n)
            ta = time.perf_counter() - t
            d = ctx.append_timings()
            t = time.perf_counter()
            u = union_csr(res, new)
            ctx2.load_csr(u, np.concatenate([thr_r, thr_n]))
            tf = time.perf_counter() - t
            if k >= args.warmup:
                wall_a.append(ta), wall_f.append(tf), dev.append(d)
        for x, y in zip(edges_of(ctx, u.n_reads, pt), edges_of(ctx2, u.n_reads, pt)):
            np.testing.assert_array_equal(x, y)                          # the same edges both ways
        ni, mi = res.n_intervals, new.n_intervals
        # the merge phase's algorithmic bytes: every interval's record, gate word and chromosome read and
        # written (28 + 28), its new position written (4) and its data position rewritten through it (12);
        # the batch's CSR rows copied behind the resident ones (32 per interval, 34 per read)
        algo = (ni + mi) * 72 + mi * 32 + new.n_reads * 34
        merge_ms = med([x['merge'] for x in dev])
        print(json.dumps(dict(placement=placement, resident_reads=res.n_reads, resident_intervals=ni, new_reads=new.n_reads, new_intervals=mi,
                              append_wall_ms=round(1e3 * med(wall_a), 2), fresh_wall_ms=round(1e3 * med(wall_f), 2),
                              append_device_ms={k: round(med([x[k] for x in dev]), 3) for k in dev[0]},
                              h2d_bytes_append=int(4 * (3 * new.n_reads + 1 + 5 * mi)),
                              h2d_bytes_fresh=int(4 * (3 * u.n_reads + 1 + 5 * u.n_intervals)),
                              merge_algo_bytes=int(algo), merge_gb_per_s=round(algo / merge_ms / 1e6, 1),
                              repeats=args.repeats, warmup=args.warmup)), flush=True)
    ctx.close()
    ctx2.close()


if __name__ == '__main__':
    main()
