"""fslr_score_timings / fslr_match_timings of the _any entry points: a short-only batch
through the old call and through _any (the same kernels), and batches of long pairs / long reads.

    python tools/any_timing.py [OUT.jsonl]      # one JSON line per measurement (default: stdout only)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fslr_amd import _lib, synth                                          # noqa: E402
from fslr_amd.prep import fold_overlap_threshold, pass_table, umax_table   # noqa: E402

CUTS = [1, 1, 0.66, 0.66, 0.66, 0.5]
OUT = open(sys.argv[1], 'w') if len(sys.argv) > 1 else None


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


if __name__ == '__main__':
    main()
