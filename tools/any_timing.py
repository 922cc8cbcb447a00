"""fslr_score_timings / fslr_match_timings of the _any entry points: a short-only batch
through the old call and through _any (the same kernels), and batches of long pairs / long reads.

    python tools/any_timing.py [OUT.jsonl]      # one JSON line per measurement (default: stdout only)

and fslr_append_reads_any / fslr_remove_reads_any on a resident set with long reads, each against
the route a caller had before them (host concatenation or prep.remove_reads_csr of the real CSR, then
fslr_set_reads_any):

    python tools/any_timing.py --resident [OUT.jsonl]    # appends its lines to OUT.jsonl

Workload: synth.generate(1,100,000 reads, 1-16 fillings, seed 11) (the cfg3 generator); every read whose rank is
a multiple of 100 (1 %) is lengthened to 65-300 intervals (default_rng(5); 500-bp steps on its chromosome from its
first start).  The first 1,000,000 reads are resident, the rest held out.  Medians of 5 runs after 2 warm-ups; before
every timed call the context is set back to the resident reads with its index built (not timed).  Both routes end
before fslr_build_index; afterwards both contexts build, query and must give the same edges.
"""
import json
import os
import statistics
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fslr_amd import _lib, synth                                          # noqa: E402
from fslr_amd.prep import fold_overlap_threshold, pass_table, umax_table   # noqa: E402

CUTS = [1, 1, 0.66, 0.66, 0.66, 0.5]
RESIDENT = '--resident' in sys.argv[1:]
_args = [a for a in sys.argv[1:] if a != '--resident']
OUT = open(_args[0], 'a' if RESIDENT else 'w') if _args else None


def emit(**rec):
    line = json.dumps(rec)
    print(line)
    if OUT:
        OUT.write(line + '\n')


def diag(n, shift=0):
    return [(1, 10_000 * k + shift, 10_000 * k + shift + 1000, 1000) for k in range(n)]


def upload_lists(ctx, reads, pct):
    from types import SimpleNamespace
    off = np.zeros(len(reads) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    flat = np.array([x for r in reads for x in r], np.int64).reshape(-1, 4)
    csr = SimpleNamespace(read_off=off, read_qlen2=np.full(len(reads), 1000), read_nal=np.full(len(reads), 4),
                          iv_chrom=flat[:, 0], iv_start=flat[:, 1], iv_end=flat[:, 2], n_chroms=2, start_sorted=False)
    ctx.load_csr_any(csr, fold_overlap_threshold(flat[:, 3], pct))


def main():
    pt = pass_table(CUTS)
    s = synth.generate(20000, 16, 23)
    csr = s.interval_data().csr()
    rng = np.random.default_rng(9)
    n = 1 << 20
    a = rng.integers(0, csr.n_reads, n)
    b = np.clip(a + rng.integers(-4, 5, n), 0, csr.n_reads - 1)
    ctx = _lib.Context(0)
    ctx.set_profiling(1)
    thr = fold_overlap_threshold(csr.iv_aln, 0.8)
    ctx.load_csr(csr, thr)
    ctx.build_index()
    L = np.diff(csr.read_off)
    for rep in range(3):
        ctx.score_pairs(a, b, 0.96, 0.75, pt)
        emit(what='score short', call='fslr_score_pairs', rep=rep, pairs=n, mean_l1_l2=float((L[a] + L[b]).mean()),
             **ctx.score_timings())
        ctx.score_pairs_any(a, b, 0.96, 0.75, pt, None)
        emit(what='score short', call='fslr_score_pairs_any', rep=rep, pairs=n, **ctx.score_timings())
    # matching: every resident read as a query read with itself excluded
    q = (csr.read_off, csr.read_qlen2, csr.read_nal, csr.iv_chrom, csr.iv_start, csr.iv_end, thr, 0.96, 0.75, pt, 2,
         np.arange(csr.n_reads))
    for rep in range(3):
        ctx.match_reads(*q)
        emit(what='match short', call='fslr_match_reads', rep=rep, reads=int(csr.n_reads), **ctx.match_timings())
        ctx.match_reads_any(*q)
        emit(what='match short', call='fslr_match_reads_any', rep=rep, reads=int(csr.n_reads), **ctx.match_timings())
    ctx.close()

    lens = [65, 130, 300, 1000, 4096]
    reads = [diag(Ln, 5 * (t % 2)) for Ln in lens for t in range(2)]
    ctx = _lib.Context(0)
    ctx.set_profiling(1)
    upload_lists(ctx, reads, 0.5)
    ctx.build_index()
    um = umax_table(CUTS, 4096)
    for k, Ln in enumerate(lens):
        m = 4096
        a, b = np.full(m, 2 * k, np.int32), np.full(m, 2 * k + 1, np.int32)
        for rep in range(2):
            I, U, F = ctx.score_pairs_any(a, b, 0.96, 0.75, pt, um)
        t = ctx.score_timings()
        emit(what='score long', call='fslr_score_pairs_any', L=Ln, pairs=m, algorithmic_bytes=m * (16 * 2 * Ln + 40),
             I=int(I[0]), **t)
    # matching: 64 copies of each length's read as query reads against the ten resident reads
    for Ln in lens:
        m = 64
        one = np.array(diag(Ln, 2), np.int64)
        flat = np.tile(one, (m, 1))
        off = np.arange(m + 1, dtype=np.int64) * Ln
        args = (off, np.full(m, 1000), np.full(m, 4), np.ones(m * Ln, np.int32), flat[:, 1], flat[:, 2],
                fold_overlap_threshold(flat[:, 3], 0.5), 0.96, 0.75, pt, 0, None)
        for rep in range(2):
            o, counts, best = ctx.match_reads_any(*args, umax=um)
        emit(what='match long', call='fslr_match_reads_any', L=Ln, reads=m, rows=int(o[-1]),
             candidates=int(counts[:, 0].sum()), **ctx.match_timings())
    ctx.close()


def lengthened(csr, every=100, seed=5):
    """``csr`` with every ``every``-th read's list replaced by 65-300 intervals; data positions by a stable start sort."""
    from fslr_amd.prep import CSR
    rng = np.random.default_rng(seed)
    L = np.diff(np.asarray(csr.read_off, np.int64))
    off = np.asarray(csr.read_off, np.int64)
    newL = L.copy()
    pick = np.arange(0, L.size, every)
    newL[pick] = rng.integers(65, 301, pick.size)
    noff = np.zeros(L.size + 1, np.int64)
    np.cumsum(newL, out=noff[1:])
    r_of = np.repeat(np.arange(L.size), newL)
    j = np.arange(int(noff[-1])) - noff[r_of]
    is_long = np.zeros(L.size, bool)
    is_long[pick] = True
    src = off[r_of] + np.where(is_long[r_of], 0, j)                   # a lengthened read repeats its first interval
    step = np.where(is_long[r_of], 500 * j, 0)
    start = np.asarray(csr.iv_start, np.int64)[src] + step
    end = np.asarray(csr.iv_end, np.int64)[src] + step
    order = np.argsort(start, kind='stable')
    dp = np.empty(order.size, np.int64)
    dp[order] = np.arange(order.size)
    return CSR(read_off=noff.astype(np.int32), read_qlen2=csr.read_qlen2, read_nal=csr.read_nal,
               iv_chrom=np.asarray(csr.iv_chrom)[src], iv_start=start.astype(np.int32), iv_end=end.astype(np.int32),
               iv_aln=np.asarray(csr.iv_aln)[src], n_chroms=csr.n_chroms, read_qcode=csr.read_qcode, data_pos=dp,
               nal_varies=csr.nal_varies)


def concat(res, new):
    """The union's real CSR with the merged data positions (the host concatenation of the old route)."""
    from fslr_amd.prep import CSR

    def starts(c):
        s = np.empty(c.n_intervals, np.int64)
        s[np.asarray(c.data_pos, np.int64)] = c.iv_start
        return s
    a, b = starts(res), starts(new)
    pos_res = np.arange(a.size) + np.searchsorted(b, a, side='left')
    pos_new = np.arange(b.size) + np.searchsorted(a, b, side='right')
    cat = lambda f: np.concatenate([getattr(res, f), getattr(new, f)])
    return CSR(read_off=np.concatenate([res.read_off, res.n_intervals + np.asarray(new.read_off)[1:]]).astype(np.int32),
               read_qlen2=cat('read_qlen2'), read_nal=cat('read_nal'), iv_chrom=cat('iv_chrom'), iv_start=cat('iv_start'),
               iv_end=cat('iv_end'), iv_aln=cat('iv_aln'), n_chroms=res.n_chroms, read_qcode=cat('read_qcode'),
               data_pos=np.concatenate([pos_res[np.asarray(res.data_pos, np.int64)], pos_new[np.asarray(new.data_pos, np.int64)]]),
               nal_varies=False)


def long_edges(ctx, csr):
    from fslr_amd import cluster
    ctx.build_index()
    idx = types.SimpleNamespace(csr=csr, ctx=ctx, long=np.diff(csr.read_off).astype(np.int32), data=None)
    g = cluster._query_long(idx, 0.8, CUTS, 10, 0.04, 0.25)
    return [np.asarray(x) for x in (g.a, g.b, g.I, g.U)]


def resident(n_res=1_000_000, sizes=(10_000, 100_000), warmup=2, repeats=5):
    from fslr_amd.prep import remove_reads_csr
    med = statistics.median
    whole = lengthened(synth.generate(n_res + max(sizes), 16, 11).interval_data().csr())
    ranks = np.arange(whole.n_reads)
    res, _ = remove_reads_csr(whole, ranks < n_res)
    thr_of = lambda c: fold_overlap_threshold(c.iv_aln, 0.8)
    thr_res = thr_of(res)
    Lr = np.diff(res.read_off.astype(np.int64))
    extra = lambda L: int(np.maximum((L + 63) // 64 - 1, 0).sum())
    ca, cb = _lib.Context(0), _lib.Context(0)
    ca.set_profiling(2)
    n, V, ni = res.n_reads, res.n_reads + extra(Lr), res.n_intervals
    for m in sizes:
        bt, _ = remove_reads_csr(whole, (ranks >= n_res) & (ranks < n_res + m))
        thr_bt = thr_of(bt)
        Lb = np.diff(bt.read_off.astype(np.int64))
        e, mi = extra(Lb), bt.n_intervals
        wall, base, dev = [], [], []
        for k in range(warmup + repeats):
            ca.load_csr_any(res, thr_res)
            ca.build_index()
            ca.sync()
            t = time.perf_counter()
            ca.append_csr_any(bt, thr_bt)
            tw = time.perf_counter() - t
            d = ca.append_timings()
            t = time.perf_counter()
            u = concat(res, bt)
            cb.load_csr_any(u, np.concatenate([thr_res, thr_bt]))
            tb = time.perf_counter() - t
            if k >= warmup:
                wall.append(tw), base.append(tb), dev.append(d)
        for x, y in zip(long_edges(ca, u), long_edges(cb, u)):
            np.testing.assert_array_equal(x, y)                      # the same edges both ways
        # the merge phase's algorithmic bytes: merge 60 B, rows 44 B per merged interval; reads 50 B
        # per virtual read, 8 B per real read
        reloc = (ni + mi) * (60 + 44) + (V + m + e) * 50 + (n + m) * 8
        merge_ms = med([x['merge'] for x in dev])
        emit(what='append any', resident_reads=n, resident_virtual_reads=V, resident_intervals=ni, long_resident=int((Lr > 64).sum()),
             batch_reads=m, batch_intervals=mi, long_batch=int((Lb > 64).sum()),
             device_route_wall_ms=round(1e3 * med(wall), 2), fresh_route_wall_ms=round(1e3 * med(base), 2),
             device_ms={k: round(med([x[k] for x in dev]), 3) for k in dev[0]},
             h2d_bytes_device_route=int(4 * (3 * (m + e) + 1 + 5 * mi + 2 * (m + e) + 2 * m)),
             h2d_bytes_fresh_route=int(4 * (3 * (V + m + e) + 1 + 5 * (ni + mi) + 2 * (V + m + e) + 2 * (n + m))),
             relocation_algo_bytes=int(reloc), relocation_gb_per_s=round(reloc / merge_ms / 1e6, 1), repeats=repeats, warmup=warmup)
    for m in sizes:
        keep = np.ones(n, bool)
        keep[np.random.default_rng(m).choice(n, m, replace=False)] = False
        keep_iv = np.repeat(keep, Lr)
        wall, base, dev = [], [], []
        for k in range(warmup + repeats):
            ca.load_csr_any(res, thr_res)
            ca.build_index()
            ca.sync()
            t = time.perf_counter()
            ca.remove_reads_any(keep)
            tw = time.perf_counter() - t
            d = ca.remove_timings()
            t = time.perf_counter()
            left, _ = remove_reads_csr(res, keep)
            cb.load_csr_any(left, thr_res[keep_iv])
            tb = time.perf_counter() - t
            if k >= warmup:
                wall.append(tw), base.append(tb), dev.append(d)
        for x, y in zip(long_edges(ca, left), long_edges(cb, left)):
            np.testing.assert_array_equal(x, y)
        Lk = Lr[keep]
        Vk, nik = left.n_reads + extra(Lk), left.n_intervals
        # the compaction phase (DESIGN.md §3.13 over the virtual reads) plus the maps: 12 B read per old virtual read,
        # 8 B written per kept one, 8 B per kept real read
        compact = ni * (28 + 24) + nik * (28 + 4 + 20) + V * 12 + Vk * 8 + left.n_reads * 8
        compact_ms = med([x['compact'] for x in dev])
        emit(what='remove any', resident_reads=n, resident_virtual_reads=V, resident_intervals=ni, removed_reads=m,
             removed_long=int((Lr[~keep] > 64).sum()), removed_intervals=int(ni - nik),
             device_route_wall_ms=round(1e3 * med(wall), 2), fresh_route_wall_ms=round(1e3 * med(base), 2),
             device_ms={k: round(med([x[k] for x in dev]), 3) for k in dev[0]},
             h2d_bytes_device_route=int(V), h2d_bytes_fresh_route=int(4 * (3 * Vk + 1 + 5 * nik + 2 * Vk + 2 * left.n_reads)),
             compaction_algo_bytes=int(compact), compaction_gb_per_s=round(compact / compact_ms / 1e6, 1),
             repeats=repeats, warmup=warmup)
    ca.close()
    cb.close()


if __name__ == '__main__':
    resident() if RESIDENT else main()
