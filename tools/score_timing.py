#!/usr/bin/env python3
"""Device time of the batched pair scoring (fslr_score_pairs) and what its lane-group packing buys.

    python tools/score_timing.py [--out profiles/score/score_timing.jsonl]

On cfg3 (synth.generate(1000000, 16, 11)), after an uncapped query, the batch is that run's edges as
(lower rank, higher rank) plus an equal number of random pairs, shuffled together.  Two lines, made in
one child process under a time limit: the batch as the library scores it (four pairs of short reads
side by side in a wavefront), then the same batch with every pair forced onto a full
64-lane group (FSLR_SCORE_WIDE=1, read by the library per call).  Per line: the pair count, the median
and minimum of the library's HIP-event times (upload, kernel, download) over --repeats calls after
--warmup, pairs/s of the kernel, the algorithmic bytes (32 B of rmeta + 16 B x (L1 + L2) per pair) and
the bandwidth they imply over the kernel time.  The two runs must return the same bytes.

--matching adds a third line: fslr_pair_matching on the same batch (mode 'matching': count, scan and emit
kernels together under 'kernel'), its rows, and its algorithmic bytes: the scoring's, the scan's 12 B per
pair, the emit pass's second read (32 B + 8 B of offsets + 16 B x (L1 + L2) per pair) and 8 B per row out.
Its I, U and flags must equal the scoring's.
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

CFG3 = (1_000_000, 16, 11)
CUTOFFS = (1, 1, 0.66, 0.66, 0.66, 0.5)


def run(repeats, warmup, matching=False):
    from fslr_amd import _lib, synth
    from fslr_amd.prep import fold_overlap_threshold, pass_table
    csr = synth.generate(*CFG3).interval_data().csr()
    n = csr.n_reads
    pt = pass_table(CUTOFFS)
    ctx = _lib.Context(0, profiling=True)
    ctx.load_csr(csr, fold_overlap_threshold(csr.iv_aln, 0.8))
    ctx.reserve_edges(max(1 << 16, 12 * n))
    ctx.build_index()
    st = ctx.run_query(0.96, 0.75, pt, edge_threshold=1 << 30)        # uncapped: no read reaches it
    ea, eb, _, _ = ctx.edges(st['n_edges'])
    rng = np.random.default_rng(1)
    a = np.concatenate([np.minimum(ea, eb), rng.integers(0, n, ea.size)]).astype(np.int32)
    b = np.concatenate([np.maximum(ea, eb), rng.integers(0, n, ea.size)]).astype(np.int32)
    order = rng.permutation(a.size)
    a, b = a[order], b[order]
    lens = np.diff(np.asarray(csr.read_off, np.int64))
    algo = int(32 * a.size + 16 * (lens[a].sum() + lens[b].sum()))
    results = []
    for mode in ('packed', 'wide64'):
        os.environ['FSLR_SCORE_WIDE'] = '1' if mode == 'wide64' else '0'
        t = {k: [] for k in ('upload', 'kernel', 'download', 'wall')}
        for k in range(warmup + repeats):
            w0 = time.perf_counter()
            out = ctx.score_pairs(a, b, 0.96, 0.75, pt)
            wall = (time.perf_counter() - w0) * 1e3
            if k >= warmup:
                for p, v in ctx.score_timings().items():
                    t[p].append(v)
                t['wall'].append(wall)
        results.append(out)
        med = {k: float(np.median(v)) for k, v in t.items()}
        I, U, flags = out
        print(json.dumps({
            'case': 'cfg3_edges_plus_random', 'mode': mode, 'n_reads': n, 'n_intervals': csr.n_intervals,
            'pairs': int(a.size), 'edges_in_batch': int(ea.size), 'edge_bits': int(((flags & 2) != 0).sum()),
            'pairs_with_I': int((I > 0).sum()), 'mean_L1_plus_L2': float((lens[a] + lens[b]).mean()),
            'repeats': repeats, 'warmup': warmup, 'ms_median': med, 'ms_min': {k: float(np.min(v)) for k, v in t.items()},
            'kernel_ms': med['kernel'], 'pairs_per_s': a.size / (med['kernel'] * 1e-3), 'algo_bytes': algo,
            'achieved_GBps': algo / (med['kernel'] * 1e-3) / 1e9}), flush=True)
    if matching:
        os.environ['FSLR_SCORE_WIDE'] = '0'
        t = {k: [] for k in ('upload', 'kernel', 'download', 'wall')}
        for k in range(warmup + repeats):
            w0 = time.perf_counter()
            out = ctx.pair_matching(a, b, 0.96, 0.75, pt)
            wall = (time.perf_counter() - w0) * 1e3
            if k >= warmup:
                for p, v in ctx.pair_matching_timings().items():
                    t[p].append(v)
                t['wall'].append(wall)
        for x, y in zip(out[:3], results[0]):
            assert np.array_equal(x, y), 'the matching call and the scoring call differ'
        rows = int(out[4].size)
        assert rows == int(out[0].sum()) == int(out[3][-1])
        med = {k: float(np.median(v)) for k, v in t.items()}
        algo_m = 2 * algo + (4 + 12 + 8) * int(a.size) + 8 * rows
        print(json.dumps({
            'case': 'cfg3_edges_plus_random', 'mode': 'matching', 'pairs': int(a.size), 'rows': rows,
            'repeats': repeats, 'warmup': warmup, 'ms_median': med, 'ms_min': {k: float(np.min(v)) for k, v in t.items()},
            'kernel_ms': med['kernel'], 'pairs_per_s': a.size / (med['kernel'] * 1e-3), 'algo_bytes': algo_m,
            'score_algo_bytes': algo + 4 * int(a.size), 'achieved_GBps': algo_m / (med['kernel'] * 1e-3) / 1e9}), flush=True)
    ctx.close()
    for x, y in zip(*results):
        assert np.array_equal(x, y), 'the packed and the 64-lane runs differ'
    assert int(((results[0][2] & 2) != 0).sum()) >= ea.size      # every edge of the run carries the edge bit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', action='store_true', help='(child) measure in this process')
    ap.add_argument('--repeats', type=int, default=12)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--matching', action='store_true', help='also time fslr_pair_matching on the same batch')
    ap.add_argument('--limit', type=int, default=420, help='seconds for the run')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'score', 'score_timing.jsonl'))
    args = ap.parse_args()
    if args.child:
        run(args.repeats, args.warmup, args.matching)
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    # a fresh child under its own limit; a failure writes nothing
    r = subprocess.run(['timeout', '-k', '10', str(args.limit), sys.executable, os.path.abspath(__file__), '--child',
                        '--repeats', str(args.repeats), '--warmup', str(args.warmup)] +
                       (['--matching'] if args.matching else []), capture_output=True, text=True)
    sys.stderr.write(r.stderr[-2000:])
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith('{')]
    for ln in lines:
        print(ln, flush=True)
    if r.returncode != 0 or len(lines) != 2 + args.matching:
        print(f'exit status {r.returncode}; nothing written', file=sys.stderr)
        return r.returncode or 1
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
