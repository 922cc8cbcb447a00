#!/usr/bin/env python3
"""Device time of the batched interval search (fslr_search / fslr_search_hits) per pass.

    python tools/search_timing.py [--out profiles/search/search_timing.jsonl]

Two cases, each in a child process under its own time limit, the second only after the first ended
well: the self-join of cfg2 (synth.generate(100000, 8, 7), every interval as a query) and 1M random
1-kb queries on cfg3's index (synth.generate(1000000, 16, 11)).  Per pass (span, count, scan, fill)
the median and minimum of the library's HIP-event times over --repeats searches after --warmup, hits/s
of count + fill, and the achieved bytes/s against the algorithmic bytes of DESIGN.md §3.7.  The times
are event intervals on the context's stream: they hold the kernels and the gaps between their
launches.  `scan` is the sum of three intervals (the piece scan; the head marks' memset, kernel and
max-scan; the hit scan and the offsets kernel); the host's wait for the piece total and its buffer
growth between the first two lie outside every interval, as do the copies of queries and hits (the
wall time per search is printed beside the passes).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

CASES = {'cfg2_selfjoin': (100_000, 8, 7), 'cfg3_random_1kb': (1_000_000, 16, 11)}


def span_positions(csr, qc, qs, qe):
    """Span lengths of the queries by numpy: [first position whose prefix-max end reaches qs, upper bound
    of qe) inside the chromosome, in (chrom, start) order."""
    out = np.zeros(qc.size, np.int64)
    order = np.lexsort((csr.iv_start, csr.iv_chrom))
    ch, st, en = csr.iv_chrom[order], csr.iv_start[order], csr.iv_end[order]
    for c in np.unique(qc):
        sel = np.flatnonzero(ch == c)
        q = np.flatnonzero(qc == c)
        if not sel.size:
            continue
        hi = np.searchsorted(st[sel], qe[q], side='right')
        lo = np.minimum(np.searchsorted(np.maximum.accumulate(en[sel]), qs[q], side='left'), hi)
        out[q] = hi - lo
    return out


def run_case(name, repeats, warmup):
    from fslr_amd import _lib, synth
    from fslr_amd.prep import fold_overlap_threshold
    reads, lmax, seed = CASES[name]
    csr = synth.generate(reads, lmax, seed).interval_data().csr()
    if name == 'cfg2_selfjoin':
        qc, qs, qe = csr.iv_chrom.copy(), csr.iv_start.copy(), csr.iv_end.copy()
    else:
        rng = np.random.default_rng(1)
        pick = rng.integers(0, csr.n_intervals, 1_000_000)         # loci where the data lie
        qc = csr.iv_chrom[pick]
        qs = (csr.iv_start[pick] + rng.integers(-2000, 2000, pick.size)).astype(np.int32)
        qe = qs + 1000
    ctx = _lib.Context(0, profiling=True)
    ctx.load_csr(csr, fold_overlap_threshold(csr.iv_aln, 0.8))
    ctx.build_index()
    t = {k: [] for k in ('span', 'count', 'scan', 'fill', 'wall')}
    for k in range(warmup + repeats):
        w0 = time.perf_counter()
        off, hits = ctx.search(qc, qs, qe)
        wall = (time.perf_counter() - w0) * 1e3
        if k >= warmup:
            for p, v in ctx.search_timings().items():
                t[p].append(v)
            t['wall'].append(wall)
    ctx.close()
    sp = span_positions(csr, qc, qs, qe)
    nq, nh, npos = int(qc.size), int(hits.size), int(sp.sum())
    med = {k: float(np.median(v)) for k, v in t.items()}
    algo = {'span': 28 * nq, 'count': 8 * npos, 'fill': 16 * npos + 20 * nh}
    res = {'case': name, 'n_intervals': csr.n_intervals, 'n_queries': nq, 'hits': nh, 'span_positions': npos,
           'longest_span': int(sp.max()), 'repeats': repeats, 'warmup': warmup,
           'ms_median': med, 'ms_min': {k: float(np.min(v)) for k, v in t.items()},
           'hits_per_s_count_fill': nh / ((med['count'] + med['fill']) * 1e-3),
           'algo_bytes': algo,
           'achieved_GBps': {k: algo[k] / (med[k] * 1e-3) / 1e9 for k in algo}}
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', choices=list(CASES), default=None, help='(child) run this case in this process')
    ap.add_argument('--repeats', type=int, default=12)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--limit', type=int, default=240, help='seconds per case')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'search', 'search_timing.jsonl'))
    args = ap.parse_args()
    if args.case:
        run_case(args.case, args.repeats, args.warmup)
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    lines = []
    for name in CASES:
        # a fresh child per case under its own limit; a failure ends the run (nothing more on the GPU)
        r = subprocess.run(['timeout', '-k', '10', str(args.limit), sys.executable, os.path.abspath(__file__), '--case',
                            name, '--repeats', str(args.repeats), '--warmup', str(args.warmup)],
                           capture_output=True, text=True)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:
            print(f'{name}: exit status {r.returncode}; stopping', file=sys.stderr)
            return r.returncode
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        lines.append(line)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
