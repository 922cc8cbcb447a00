#!/usr/bin/env python3
"""Device time of the read-depth stage (fslr_coverage_build / fslr_coverage_at), its two query kernels
side by side, and the host path it stands in for.

    python tools/coverage_timing.py [--out profiles/coverage/coverage_timing.jsonl]

On cfg3 (synth.generate(1000000, 16, 11)): the bed rows are SynthBed.to_dataframe()'s (chromosomes
renamed to numbers, as the pipeline does before the filter), the queries the prepared data's
(chrom, middle).  Lines, made in one child process under a time limit:

* ``build``: median / min / max of the library's HIP-event times (upload with the key packing, the two
  sorts with the tile keys) over --repeats builds after --warmup, rows/s, the algorithmic bytes (12 B per
  row up; 16 B of keys per row read and 16 B written by the sorts) and the bandwidth they imply.
* ``query`` twice: the two-level kernel, then the same batch with FSLR_COV_PLAIN=1 (two full binary
  searches per query; read by the library per call).  Event times (upload + kernel, download), wall
  time, queries/s, probes per query, algorithmic bytes (8 B in, 4 B out, 8 B per probe), implied
  bandwidth.  The two must return the same bytes.  ``ab``: the decision DESIGN.md §3.9 records, the
  two-level kernel stays only if its median is below the plain one's by more than the plain one's own
  spread (max - min of its repeats).
* ``filter``: wall time of cluster.filter_high_coverage(data, bed, lengths, 10000, ctx=ctx) from Python
  (host normalisation, build, one query, select).
* ``host``: the unchanged host filter_high_coverage on the first --host-chroms chromosomes (default: as
  many as half of the free memory holds at 3 dense float64 arrays of 150 Mb in flight), and the device
  path on the same restricted input; their ratio is a description, not a pass mark.
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


def stats(v):
    return {'median': float(np.median(v)), 'min': float(np.min(v)), 'max': float(np.max(v))}


def free_bytes():
    with open('/proc/meminfo') as fh:
        for ln in fh:
            if ln.startswith('MemAvailable:'):
                return int(ln.split()[1]) * 1024
    return 8 << 30


def run(repeats, warmup, host_chroms):
    from fslr_amd import _lib, cluster, synth
    s = synth.generate(*CFG3)
    data = s.interval_data()
    df = s.to_dataframe()[['chrom', 'rstart', 'rend']].copy()
    names = {n: k + 1 for k, n in enumerate(synth.CHROMS)}
    df['chrom'] = df['chrom'].map(names)
    lengths = {names[k]: v for k, v in s.chrom_lengths.items()}
    n_chroms = len(names)
    chrom = (df['chrom'].to_numpy() - 1).astype(np.int32)
    rs, re_ = df['rstart'].to_numpy().astype(np.int32), df['rend'].to_numpy().astype(np.int32)
    qc, qp = (np.asarray(data.chrom) - 1).astype(np.int32), np.asarray(data.middle).astype(np.int32)
    n, nq = int(chrom.size), int(qc.size)
    base = {'case': 'cfg3_bed_rows_at_data_middles', 'n_reads': CFG3[0], 'rows': n, 'queries': nq,
            'repeats': repeats, 'warmup': warmup, 'tile': _lib.COVERAGE_TILE, 'chunk': _lib.COVERAGE_CHUNK}
    ctx = _lib.Context(0, profiling=True)

    t = {k: [] for k in ('build_upload', 'build_sort', 'wall')}
    for k in range(warmup + repeats):
        w0 = time.perf_counter()
        ctx.coverage_build(chrom, rs, re_, n_chroms)
        wall = (time.perf_counter() - w0) * 1e3
        if k >= warmup:
            tm = ctx.coverage_timings()
            t['build_upload'].append(tm['build_upload'])
            t['build_sort'].append(tm['build_sort'])
            t['wall'].append(wall)
    med_sort = float(np.median(t['build_sort']))
    print(json.dumps({**base, 'line': 'build', 'ms': {k: stats(v) for k, v in t.items()},
                      'rows_per_s_sort': n / (med_sort * 1e-3), 'upload_bytes': 12 * n, 'sort_algo_bytes': 32 * n,
                      'upload_GBps': 12 * n / (np.median(t['build_upload']) * 1e-3) / 1e9,
                      'sort_GBps': 32 * n / (med_sort * 1e-3) / 1e9}), flush=True)

    results, kern = {}, {}
    bits = lambda v: int(v).bit_length()
    probes = {'two_level': 2 * (bits(n // _lib.COVERAGE_TILE) + 8), 'plain': 2 * bits(n)}
    for mode in ('two_level', 'plain'):
        os.environ['FSLR_COV_PLAIN'] = '1' if mode == 'plain' else '0'
        t = {k: [] for k in ('query_upload_kernel', 'query_download', 'wall')}
        for k in range(warmup + repeats):
            w0 = time.perf_counter()
            out = ctx.coverage_at(qc, qp)
            wall = (time.perf_counter() - w0) * 1e3
            if k >= warmup:
                tm = ctx.coverage_timings()
                t['query_upload_kernel'].append(tm['query_upload_kernel'])
                t['query_download'].append(tm['query_download'])
                t['wall'].append(wall)
        results[mode], kern[mode] = out, stats(t['query_upload_kernel'])
        algo = nq * (12 + 8 * probes[mode])
        print(json.dumps({**base, 'line': 'query', 'mode': mode, 'ms': {k: stats(v) for k, v in t.items()},
                          'queries_per_s': nq / (kern[mode]['median'] * 1e-3), 'probes_per_query': probes[mode],
                          'algo_bytes': algo, 'implied_GBps': algo / (kern[mode]['median'] * 1e-3) / 1e9,
                          'depth_min': int(out.min()), 'depth_max': int(out.max())}), flush=True)
    os.environ['FSLR_COV_PLAIN'] = '0'
    assert results['two_level'].tobytes() == results['plain'].tobytes(), 'the two kernels differ'
    spread = kern['plain']['max'] - kern['plain']['min']
    gain = kern['plain']['median'] - kern['two_level']['median']
    print(json.dumps({**base, 'line': 'ab', 'plain_median_ms': kern['plain']['median'], 'plain_spread_ms': spread,
                      'two_level_median_ms': kern['two_level']['median'], 'gain_ms': gain,
                      'two_level_stays': bool(gain > spread)}), flush=True)

    t = []
    for k in range(3):
        w0 = time.perf_counter()
        kept = cluster.filter_high_coverage(data, df, lengths, 10_000, ctx=ctx)
        t.append((time.perf_counter() - w0) * 1e3)
    print(json.dumps({**base, 'line': 'filter', 'wall_ms': stats(t), 'kept': len(kept)}), flush=True)

    if host_chroms <= 0:
        host_chroms = int(max(1, min(n_chroms, free_bytes() // 2 // (3 * 8 * (synth.CHROM_LEN + 1)))))
    sub_df = df[df['chrom'] <= host_chroms]
    sub_data = data.select(np.asarray(data.chrom) <= host_chroms)
    sub_len = {k: v for k, v in lengths.items() if k <= host_chroms}
    w0 = time.perf_counter()
    host = cluster.filter_high_coverage(sub_data, sub_df, sub_len, 10_000)
    host_ms = (time.perf_counter() - w0) * 1e3
    w0 = time.perf_counter()
    dev = cluster.filter_high_coverage(sub_data, sub_df, sub_len, 10_000, ctx=ctx)
    dev_ms = (time.perf_counter() - w0) * 1e3
    assert np.array_equal(host.index, dev.index), 'host and device filters differ'
    print(json.dumps({**base, 'line': 'host', 'chromosomes': host_chroms, 'of': n_chroms, 'host_rows': int(len(sub_df)),
                      'host_queries': len(sub_data), 'host_wall_ms': host_ms, 'device_wall_ms': dev_ms,
                      'ratio': host_ms / dev_ms, 'dense_bytes': 8 * sum(v + 1 for v in sub_len.values())}), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', action='store_true', help='(child) measure in this process')
    ap.add_argument('--repeats', type=int, default=12)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--host-chroms', type=int, default=0, help='chromosomes of the host comparison (0: by free memory)')
    ap.add_argument('--limit', type=int, default=540, help='seconds for the run')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'coverage', 'coverage_timing.jsonl'))
    args = ap.parse_args()
    if args.child:
        run(args.repeats, args.warmup, args.host_chroms)
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    # a fresh child under its own limit; a failure writes nothing
    r = subprocess.run(['timeout', '-k', '10', str(args.limit), sys.executable, os.path.abspath(__file__), '--child',
                        '--repeats', str(args.repeats), '--warmup', str(args.warmup), '--host-chroms',
                        str(args.host_chroms)], capture_output=True, text=True)
    sys.stderr.write(r.stderr[-2000:])
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith('{')]
    for ln in lines:
        print(ln, flush=True)
    if r.returncode != 0 or len(lines) != 6:
        print(f'exit status {r.returncode}; nothing written', file=sys.stderr)
        return r.returncode or 1
    with open(args.out, 'a') as fh:
        fh.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
