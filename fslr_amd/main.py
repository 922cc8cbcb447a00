"""``fslr`` command line, clustering entry (``fslr --skip-alignment``).

Mirrors the reference click command (/root/reference/fslr/main.py:19-41): same
options, defaults, messages and output files for the clustering block
(main.py:190-352).  The read-filtering / primer-labelling / bwa+dodi alignment
stages (main.py:76-188) are outside this build: without ``--skip-alignment`` the
command stops with an error instead of running them.

Output assembly (main.py:247-352) is vectorised: cluster ids come straight from
the device union-find labels instead of a DataFrame of Python sets, with the
same values and dtypes the reference writes.
"""
from __future__ import annotations

import os
import sys
import time
import warnings

import click
import numpy as np
from ._lazy import pandas as pd

from . import __version__, cluster, fastcli, ingest

# primer names of the reference's primers.csv (fslr/primers.csv:2-7); main.py:59-67 validates
# --primers against them even under --skip-alignment
PRIMER_NAMES = ('21q1', '17p6', 'XpYpM', '16p1', 'M613', 'M615')
# primer_seq column of the reference's primers.csv: collect_mapping_info's 'missing bread' rows take
# their query span from the primer length (collect_mapping_info.py:130,148)
PRIMER_SEQS = {'21q1': 'CTACCTCTCTCGACACCAAG', '17p6': 'GGCTGAACTATAGCCTCTGC', 'XpYpM': 'AACACACTGGAAAACCTGGT',
               '16p1': 'CTGCCCTAGAAGTGAGAAGTCCA', 'M613': 'GGAGGAAAGCATGTTTCTGAG', 'M615': 'TAGTGGACAAACACGAGAGGC'}


def assign_clusters(bed_file: pd.DataFrame, G: cluster.ClusterGraph, ctx=None):
    """main.py:251-342: add ``cluster`` / ``n_reads`` columns to ``bed_file`` (in place).

    Clustered reads get their component index (components ordered by min read
    rank = networkx order, cluster.py:230-234) and the component size; every
    other qname of ``bed_file`` gets the next ids in first-appearance order with
    n_reads 1.  Both columns are float when any such singleton exists (the
    reference's left merge introduces NaN before fillna), int otherwise.
    With ``ctx`` (a fslr_amd._lib.Context) the table and the numbering are made on the device
    (fslr_cluster_table, fslr_assign_clusters).
    """
    codes, uniq = ingest.factorize_qname(bed_file)
    if ctx is not None:
        if codes.size and (codes < 0).any():
            raise ValueError('missing qname values are not supported')
        nu = len(uniq)
        code_of_rank = pd.Index(uniq, dtype=object).get_indexer(pd.Index(G.qnames_by_rank, dtype=object)).astype(np.int64)
        away = code_of_rank < 0                       # a read of the graph without rows here: a code of its own
        code_of_rank[away] = nu + np.arange(int(away.sum()))
        present = np.zeros(nu + int(away.sum()), np.uint8)
        present[:nu] = 1
        ctx.cluster_table(G.labels)
        cl, nr, k = ctx.assign_clusters(present, code_of_rank)
        dtype = np.float64 if k else np.int64
        bed_file['cluster'] = cl[codes].astype(dtype)
        bed_file['n_reads'] = nr[codes].astype(dtype)
        return bed_file
    rank_names = G.qnames_by_rank
    node = G.node_mask
    cid_by_name = pd.Series(G.component_id[node], index=pd.Index(rank_names[node], dtype=object))
    size_by_name = pd.Series(G.comp_size[node], index=cid_by_name.index)
    u = pd.Index(uniq, dtype=object)
    ucid = cid_by_name.reindex(u).to_numpy()
    usize = size_by_name.reindex(u).to_numpy()
    n_cluster = int(G.roots.size)
    single = np.isnan(ucid.astype(np.float64))
    k = int(single.sum())
    ucid = ucid.astype(np.float64)
    usize = usize.astype(np.float64)
    ucid[single] = np.arange(n_cluster, n_cluster + k, dtype=np.float64)   # uniq is first-appearance order
    usize[single] = 1.0
    if codes.size and (codes < 0).any():
        raise ValueError('missing qname values are not supported')
    if k:
        bed_file['cluster'] = ucid[codes]
        bed_file['n_reads'] = usize[codes]
    else:
        bed_file['cluster'] = ucid[codes].astype(np.int64)
        bed_file['n_reads'] = usize[codes].astype(np.int64)
    return bed_file


@click.command()
@click.option('--name', required=True, help='Sample name')
@click.option('--out', required=True, help='Output folder')
@click.option('--ref', required=True, help='Reference genome')
@click.option('--primers', required=True, help='Comma-separated list of primer names. Make sure these are listed in primers.csv')
@click.option('--basecalled', required=False, help='Folder of basecalled reads in fastq format to analyse')
@click.option('--trim-threshold', required=False, help='Threshold in range 0-1. Fraction of maximum primer alignment score; primer sites with lower scores are labelled False', default=0.4, type=float, show_default=True)
@click.option('--keep-temp', required=False, is_flag=True, flag_value=True, help='Keep temp files')
@click.option('--regions', required=False, type=click.Path(exists=True), help='Target regions in bed form to perform biased mapping')
@click.option('--bias', required=False, default=1.05, show_default=True, type=float, help='Multiply alignment score by bias if alignment falls within target regions')
@click.option('--procs', required=False, default=1, show_default=True, help='Number of processors to use')
@click.option('--reference-mask', required=False, type=click.Path(exists=True), help='A bed file containing target regions for creating a masked reference. Reads are first aligned to the masked reference, prior to using the main reference')
@click.option('--skip-alignment', required=False, is_flag=True, help='Skip alignment step')
@click.option('--skip-clustering', required=False, is_flag=True, help='Skip clustering step')
@click.option('--jaccard-cutoffs', required=False, default='1,1,0.66,0.66,0.66,0.5', show_default=True, help="Comma-separated list of Jaccard similarity thresholds for N-1 intersections e.g. where index=0 corresponds to one the threshold for 1 intersection.")
@click.option('--overlap', required=False, default=0.8, show_default=True, help="A number between 0 and 1. Zero means two reads don't overlap at all, while 1 means the start and end of the reads is identical.")
@click.option('--n-alignment-diff', default=0.25, required=False, show_default=True, help='How much the number of alignments in one cluster can differ. Fraction in the range 0-1.')
@click.option('--qlen-diff', default=0.04, required=False, show_default=True, help="Max difference in query length. Fraction in the range 0-1.")
@click.option('--cluster-mask', default='subtelomere', required=False, show_default=True, help="Comma separated list of chromosome names to be excluded from the clustering. Use 'subtelomere' to exclude alignments within 500kb of telomere end")
@click.option('--filter-high-coverage', required=False, is_flag=True, help='Filter regions with high coverage')
@click.option('--filter-false', required=False, is_flag=True, help='Use reads with both primers labeled')
@click.option('--device', required=False, default=None, type=int, help='HIP device ordinal for the clustering kernels (default: $LOCAL_RANK or 0)')
@click.option('--gpus', required=False, default=1, show_default=True, type=click.IntRange(1, 64),
              help='GPUs for the clustering query: one process per GPU, chromosome-split sweep with RCCL '
                   'exchange (ranks share devices over gloo when fewer are visible)')
@click.option('--cluster-loci', required=False, is_flag=True,
              help='Also write {name}.mappings.cluster_loci.bed: per cluster and chromosome the merged spans of its '
                   "reads' intervals with their interval and read counts (one GPU)")
@click.option('--cluster-junctions', required=False, is_flag=True,
              help='Also write {name}.mappings.cluster_junctions.bed: per cluster the junctions between locus ends '
                   'that its reads support, with their breakpoints and their observation and read counts (one GPU)')
@click.option('--cluster-paths', required=False, is_flag=True,
              help='Also write {name}.mappings.cluster_paths.bed: per cluster its distinct read structures, the chain '
                   'of pieces each read walks, with the reads that agree on each (one GPU)')
@click.option('--cluster-path-segments', required=False, is_flag=True,
              help='Also write {name}.mappings.cluster_path_segments.bed: per piece of every cluster path its consensus '
                   '(median) coordinates with their extrema over the reads that walk the path, and the query-space gap '
                   'to the next piece (negative: overlap, positive: inserted sequence); loads as BED (one GPU; an '
                   'input with reads of more than 64 intervals prints a notice and writes no file: '
                   '--cluster-path-segments-any takes it)')
@click.option('--cluster-path-segments-any', required=False, is_flag=True,
              help='Write {name}.mappings.cluster_path_segments.bed as --cluster-path-segments does, for any input: reads '
                   'of more than 64 intervals (up to 4096) are taken too (fslr_cluster_paths_any / '
                   'fslr_cluster_path_segments_any); without such reads the file is the same, byte for byte (one GPU)')
@click.option('--cluster-path-containment', required=False, is_flag=True,
              help='Also write {name}.mappings.cluster_path_containment.bed: per cluster path the paths it contains as '
                   'truncated views (contiguous sub-chains in either direction), its support with their reads counted, '
                   'the full-length path it collapses to, and the paths that contain it as outer:offset:strand (one '
                   'GPU; any input, reads of more than 64 intervals included)')
@click.option('--cluster-collapsed-segments', required=False, is_flag=True,
              help='Also write {name}.mappings.cluster_collapsed_segments.bed: one BED line per piece of every '
                   'full-length cluster path (one that no other path contains) with its consensus coordinates and '
                   'junction gaps taken over all reads that collapse onto it, the truncated ones counted at the pieces '
                   'they cover (n_cov, n_link) (one GPU; any input, reads of more than 64 intervals included)')
@click.option('--cluster-long-reads', required=False, is_flag=True,
              help='With --cluster-junctions / --cluster-paths: also take inputs that hold reads of more than 64 '
                   'intervals (up to 4096; fslr_cluster_junctions_any / fslr_cluster_paths_any) instead of printing a '
                   'notice and writing no file')
@click.option('--timings', required=False, is_flag=True, help='Print per-stage wall times to stderr')
@click.option('--native-io/--pandas-io', default=True, show_default=True,
              help='Read .mappings.bed and write the outputs with the native threaded reader/writer '
                   '(fslr_ingest.h); inputs it cannot type exactly like pandas fall back to pandas')
@click.version_option(__version__)
def pipeline(**args):
    # the reference ignores all warnings (main.py:13): FutureWarning, and pandas' SettingWithCopyWarning by
    # its message (its class would import pandas, which the columnar path never needs)
    warnings.filterwarnings('ignore', category=FutureWarning)
    warnings.filterwarnings('ignore', message=r'\s*A value is trying to be set on a copy')
    basename = f'{args["out"]}/{args["name"]}'
    print('Basename: ', basename, file=sys.stderr)
    primers = args['primers'].split(',')
    known = set(PRIMER_NAMES)
    for p in primers:
        if p not in known:
            raise ValueError('Input primer name not in primers.csv', p, known)
    if args.get('cluster_loci') and (args.get('gpus') or 1) > 1:
        raise click.UsageError('--cluster-loci needs the whole index on one device: run it with --gpus 1')
    if args.get('cluster_junctions') and (args.get('gpus') or 1) > 1:
        raise click.UsageError('--cluster-junctions needs the whole index on one device: run it with --gpus 1')
    if args.get('cluster_paths') and (args.get('gpus') or 1) > 1:
        raise click.UsageError('--cluster-paths needs the whole index on one device: run it with --gpus 1')
    if args.get('cluster_path_segments') and (args.get('gpus') or 1) > 1:
        raise click.UsageError('--cluster-path-segments needs the whole index on one device: run it with --gpus 1')
    if args.get('cluster_path_segments_any') and (args.get('gpus') or 1) > 1:
        raise click.UsageError('--cluster-path-segments-any needs the whole index on one device: run it with --gpus 1')
    if args.get('cluster_path_containment') and (args.get('gpus') or 1) > 1:
        raise click.UsageError('--cluster-path-containment needs the whole index on one device: run it with --gpus 1')
    if args.get('cluster_collapsed_segments') and (args.get('gpus') or 1) > 1:
        raise click.UsageError('--cluster-collapsed-segments needs the whole index on one device: run it with --gpus 1')
    if not os.path.exists(args['out']):
        os.mkdir(args['out'])
    if not args['skip_alignment']:
        raise click.UsageError('the read filtering / primer labelling / bwa+dodi alignment stages are not part of '
                               'this build; run with --skip-alignment on an existing {name}.mappings.bed')
    if not args['skip_clustering']:
        if not run_clustering(args, basename):
            return                               # main.py:247-249 returns before 'fslr finished'
    print('fslr finished')


def run_clustering(args, basename):
    """main.py:190-352."""
    t = {}
    t0 = time.perf_counter()
    print('Making clusters')
    if (args.get('gpus') or 1) > 1:
        # the other ranks start now: their interpreter, torch import and process-group rendezvous run
        # while this process reads and prepares the input (fslr_amd.multi.RankPool)
        from . import multi
        multi.pool(args['gpus'], first_device=args.get('device') or 0)
    path = f'{basename}.mappings.bed'
    tsv = _open_tsv(path) if args.get('native_io', True) else None
    t['read.open'] = time.perf_counter() - t0
    try:
        if tsv is not None and not args['filter_high_coverage']:
            # the columnar path (fastcli): codes and int columns, no frame of rows; the scan checks
            # that every column round-trips through pandas (verbatim) while parsing the int columns
            try:
                cols = tsv.scan_all(fastcli.INT_COLS, fastcli.STR_COLS)
            except KeyError:
                cols = None
            if cols is not None:
                t['read_csv'] = time.perf_counter() - t0
                try:
                    return fastcli.run(args, basename, tsv, cols[0], cols[1], t)
                except fastcli.Fallback:
                    pass
        if tsv is not None and not tsv.verbatim():
            tsv.close()
            tsv = None
        bed_file = None
        if tsv is not None:
            bed_file = ingest.frame_from(tsv, int_columns=ingest.INT_COLUMNS + ('alignment_score',))
            if bed_file is None:
                tsv.close()
                tsv = None
        if bed_file is None:
            bed_file = pd.read_csv(path, sep='\t')
        t['read_csv'] = time.perf_counter() - t0
        return _cluster_and_write(args, basename, bed_file, tsv, t)
    finally:
        if tsv is not None:
            tsv.close()


def _open_tsv(path):
    """The native reader's TsvFile, or None when it declines the file (pandas reads it)."""
    try:
        tsv = ingest.TsvFile(path)
    except (FileNotFoundError, OSError):
        return None
    if tsv.declined:
        tsv.close()
        return None
    return tsv


def _native_tsv(path):
    """The native reader's TsvFile when every input column would round-trip through pandas unchanged,
    so that writing the input's own row bytes equals ``to_csv`` of the pandas frame (reference
    main.py:349,352); else None (pandas reads the file)."""
    tsv = _open_tsv(path)
    if tsv is not None and not tsv.verbatim():
        tsv.close()
        return None
    return tsv


def _native_open(path):
    """(TsvFile, frame of the columns clustering and the writers read) or (None, None)."""
    tsv = _native_tsv(path)
    if tsv is None:
        return None, None
    bed = ingest.frame_from(tsv, int_columns=ingest.INT_COLUMNS + ('alignment_score',))
    if bed is None:
        tsv.close()
        return None, None
    return tsv, bed


def write_cluster_loci(path, loci, chrom_to_num_map):
    """``loci`` (cluster.ClusterLoci, chromosomes as rename_chromosomes' numbers) as a tab-separated file:
    header ``cluster chrom start end n_intervals n_reads``, chromosome names as in the input, rows in the
    call's order (cluster, chromosome, start)."""
    name_of = {v: k for k, v in chrom_to_num_map.items()}
    cols = [loci.cluster_of_row().tolist(), [name_of[c] for c in loci.chrom.tolist()], loci.start.tolist(),
            loci.end.tolist(), loci.n_intervals.tolist(), loci.n_reads.tolist()]
    with open(path, 'w') as fh:
        fh.write('cluster\tchrom\tstart\tend\tn_intervals\tn_reads\n')
        fh.writelines('\t'.join(map(str, row)) + '\n' for row in zip(*cols))


JUNCTION_COLUMNS = ('cluster', 'chrom_a', 'side_a', 'locus_a', 'bp_a_min', 'bp_a_max', 'chrom_b', 'side_b', 'locus_b',
                    'bp_b_min', 'bp_b_max', 'n_obs', 'n_reads')


def junction_inputs(path, rows, with_qend=False):
    """``(qstart, rev)``, with ``with_qend`` ``(qstart, rev, qend)``, of the .mappings.bed rows ``rows`` (file row
    numbers: ``data.index``) from a narrow read of ``path``.  ``qstart`` is already in the frame of the read's primary alignment, so an interval runs against
    the query order iff its strand differs from the primary row's: rev = (strand == '-') xor (the primary row's
    strand == '-').  The primary row is the read's first row with a non-empty ``seq`` (it may be one of the two
    end rows that clustering drops); a read without one counts as forward."""
    bed = pd.read_csv(path, sep='\t', usecols=['qname', 'qstart', 'strand', 'seq'] + (['qend'] if with_qend else []),
                      dtype={'seq': str, 'strand': str}, na_filter=False)
    codes, uniq = pd.factorize(bed['qname'], sort=False)
    neg = (bed['strand'] == '-').to_numpy()
    prim = np.flatnonzero((bed['seq'] != '').to_numpy())[::-1]        # descending: a read's first row is written last
    prim_neg = np.zeros(len(uniq), bool)
    prim_neg[codes[prim]] = neg[prim]
    rows = np.asarray(rows, np.int64)
    out = (bed['qstart'].to_numpy()[rows], (neg ^ prim_neg[codes])[rows].astype(np.uint8))
    return out + (bed['qend'].to_numpy()[rows],) if with_qend else out


def write_cluster_junctions(path, bed_path, trees, G_or_labels, chrom_to_num_map, long_reads=False):
    """--cluster-junctions: the junctions of ``trees``' clusters (cluster.ClusterJunctions.to_frame) as a
    tab-separated file with JUNCTION_COLUMNS, chromosome names as in the input.  An index with reads of more than
    64 intervals prints a notice and writes nothing, unless ``long_reads`` (--cluster-long-reads) sends the call
    through cluster_junctions_any."""
    if getattr(trees, 'long', None) is not None and not long_reads:
        print('--cluster-junctions: the input holds reads of more than 64 intervals; no junctions file is written.')
        return False
    qstart, rev = junction_inputs(bed_path, trees.data.index)
    call = trees.cluster_junctions_any if long_reads else trees.cluster_junctions
    frame = call(qstart, rev, G_or_labels).to_frame()
    name_of = {v: k for k, v in chrom_to_num_map.items()}
    for col in ('chrom_a', 'chrom_b'):
        frame[col] = [name_of[c] for c in frame[col].tolist()]
    frame[list(JUNCTION_COLUMNS)].to_csv(path, sep='\t', index=False)
    return True


PATH_COLUMNS = ('cluster', 'path', 'n_reads', 'n_loci', 'first_read', 'structure')


def write_cluster_paths(path, bed_path, trees, G_or_labels, chrom_to_num_map, long_reads=False):
    """--cluster-paths: the distinct read structures of ``trees``' clusters (cluster.ClusterPaths.to_frame) as a
    tab-separated file with PATH_COLUMNS, chromosome names as in the input.  An index with reads of more than 64
    intervals prints a notice and writes nothing, unless ``long_reads`` (--cluster-long-reads) sends the call
    through cluster_paths_any."""
    if getattr(trees, 'long', None) is not None and not long_reads:
        print('--cluster-paths: the input holds reads of more than 64 intervals; no paths file is written.')
        return False
    qstart, rev = junction_inputs(bed_path, trees.data.index)
    paths = (trees.cluster_paths_any if long_reads else trees.cluster_paths)(qstart, rev, G_or_labels)
    name_of = {v: k for k, v in chrom_to_num_map.items()}
    paths.loci.chrom = np.asarray([name_of[c] for c in paths.loci.chrom.tolist()], dtype=object)
    paths.to_frame()[list(PATH_COLUMNS)].to_csv(path, sep='\t', index=False)
    return True


SEGMENT_COLUMNS = ('chrom', 'start', 'end', 'cluster', 'path', 'piece', 'strand', 'n_reads', 'start_min', 'start_max',
                   'end_min', 'end_max', 'gap_min', 'gap', 'gap_max')


def write_cluster_path_segments(path, bed_path, trees, G_or_labels, chrom_to_num_map, any_length=False):
    """--cluster-path-segments: one line per piece of every cluster path (cluster.ClusterPathSegments.to_frame) as a
    tab-separated file with SEGMENT_COLUMNS: chrom, median start and median end first, so it loads as BED;
    chromosome names as in the input.  An index with reads of more than 64 intervals prints a notice and writes
    nothing (--cluster-long-reads does not lift this), unless ``any_length`` (--cluster-path-segments-any) sends the
    call through cluster_path_segments_any."""
    if getattr(trees, 'long', None) is not None and not any_length:
        print('--cluster-path-segments: the input holds reads of more than 64 intervals; no path segments file is '
              'written (--cluster-path-segments-any takes such an input).')
        return False
    qstart, rev, qend = junction_inputs(bed_path, trees.data.index, with_qend=True)
    call = trees.cluster_path_segments_any if any_length else trees.cluster_path_segments
    frame = call(qstart, qend, rev, G_or_labels).to_frame()
    name_of = {v: k for k, v in chrom_to_num_map.items()}
    frame['chrom'] = [name_of.get(c, c) for c in frame['chrom'].tolist()]      # (--cluster-paths named its rows' loci)
    frame[list(SEGMENT_COLUMNS)].to_csv(path, sep='\t', index=False)
    return True


CONTAINMENT_COLUMNS = ('cluster', 'row', 'n_tokens', 'n_reads', 'n_inner', 'support', 'maximal', 'collapse_to',
                       'collapsed_reads', 'contained_in')


def write_cluster_path_containment(path, bed_path, trees, G_or_labels):
    """--cluster-path-containment: one line per path row of ``trees``' clusters
    (cluster.ClusterPathContainment.paths_frame) as a tab-separated file with CONTAINMENT_COLUMNS; ``maximal`` is 0 / 1
    and ``contained_in`` lists the rows that contain this one as ``outer:offset:strand`` joined by ``,`` (``-``: it
    lies there reverse complemented; ``.`` for a row nothing contains).  Any input is taken: the call goes through
    cluster_paths_any."""
    qstart, rev = junction_inputs(bed_path, trees.data.index)
    res = trees.cluster_path_containment(qstart, rev, G_or_labels)
    frame = res.paths_frame()
    frame['maximal'] = frame['maximal'].astype(np.int64)
    entry = [f'{o}:{f}:' + '-+'[r == 0] for o, f, r in zip(res.outer.tolist(), res.offset.tolist(), res.rev.tolist())]
    co = res.coff.tolist()
    frame['contained_in'] = np.asarray([','.join(entry[a:b]) or '.' for a, b in zip(co[:-1], co[1:])], dtype=object)
    frame[list(CONTAINMENT_COLUMNS)].to_csv(path, sep='\t', index=False)
    return True


COLLAPSED_COLUMNS = ('chrom', 'start', 'end', 'cluster', 'path', 'piece', 'strand', 'n_cov', 'start_min', 'start_max',
                     'end_min', 'end_max', 'gap_min', 'gap', 'gap_max', 'n_link', 'collapsed_reads')


def write_cluster_collapsed_segments(path, bed_path, trees, G_or_labels, chrom_to_num_map):
    """--cluster-collapsed-segments: one line per piece of every maximal cluster path
    (cluster.ClusterCollapsedSegments.to_frame) as a tab-separated file with COLLAPSED_COLUMNS: chrom, median start and
    median end first, so it loads as BED; chromosome names as in the input.  Any input is taken: the call goes through
    cluster_collapsed_segments_any."""
    qstart, rev, qend = junction_inputs(bed_path, trees.data.index, with_qend=True)
    frame = trees.cluster_collapsed_segments_any(qstart, qend, rev, G_or_labels).to_frame()
    name_of = {v: k for k, v in chrom_to_num_map.items()}
    frame['chrom'] = [name_of.get(c, c) for c in frame['chrom'].tolist()]      # (--cluster-paths named its rows' loci)
    frame[list(COLLAPSED_COLUMNS)].to_csv(path, sep='\t', index=False)
    return True


def _cluster_and_write(args, basename, bed_file, tsv, t):
    chromosome_mask = set()
    if args['cluster_mask']:
        allowed = set(bed_file['chrom'])
        for item in args['cluster_mask'].split(','):
            if item in allowed or item == 'subtelomere':
                chromosome_mask.add(item)
    jaccard_cutoffs = [float(i) for i in args['jaccard_cutoffs'].split(',')]
    overlap = args['overlap']
    edge_threshold = 10
    qlen_diff = args['qlen_diff']
    n_alignments_diff = args['n_alignment_diff']
    chr_lengths = cluster.get_chromosome_lengths(f'{basename}.bwa_dodi.bam')
    bed_file, chr_lengths, chromosome_mask, chrom_to_num_map = cluster.rename_chromosomes(
        bed_file, chr_lengths, chromosome_mask)
    if args['filter_false']:
        bed_file = cluster.delete_false(bed_file)
    t1 = time.perf_counter()
    fillings = cluster.keep_fillings(bed_file)
    if args['filter_high_coverage']:
        fillings = cluster.filter_high_coverage(fillings, bed_file, chr_lengths, threshold=10000)
    data = cluster.prepare_data(fillings, chromosome_mask, chr_lengths, threshold=500_000)
    t['prepare'] = time.perf_counter() - t1
    t1 = time.perf_counter()
    data.csr()                                   # the device layout (host; cached on data)
    t['csr'] = time.perf_counter() - t1
    t2 = time.perf_counter()
    interval_tree = cluster.build_interval_trees(data, device=args.get('device'), n_gpus=args.get('gpus') or 1)
    t['upload'] = time.perf_counter() - t2       # context, CSR H2D, index build
    t2 = time.perf_counter()
    match_data, network = cluster.query_interval_trees(interval_tree, data, overlap, jaccard_cutoffs,
                                                       edge_threshold, qlen_diff, n_alignments_diff)
    t['query'] = time.perf_counter() - t2        # pair engine, cap, components, D2H, match_df
    if network.number_of_edges() == 0:          # main.py:247: #components == #nodes only for an empty graph
        print('No clusters were found.')
        return False
    t3 = time.perf_counter()
    assign_clusters(bed_file, network)
    if tsv is None:                              # the native writer copies the input's own chrom text
        bed_file = cluster.chrom_to_str(bed_file, chrom_to_num_map)
    if tsv is not None:
        added = [c for c in bed_file.columns if c not in set(tsv.columns)]
        tsv.write_rows(f'{basename}.mappings.cluster.bed', bed_file.index.to_numpy(), bed_file[added],
                       ingest.factorize_qname(bed_file))
    else:
        bed_file.to_csv(f'{basename}.mappings.cluster.bed', index=False, sep='\t')
    bed_representative = cluster.choose_alignment(bed_file)
    if tsv is not None:
        added = [c for c in bed_representative.columns if c not in set(tsv.columns)]
        tsv.write_rows(f'{basename}.mappings.representative.bed', bed_representative.index.to_numpy(),
                       bed_representative[added], ingest.factorize_qname(bed_representative))
    else:
        bed_representative.to_csv(f'{basename}.mappings.representative.bed', index=False, sep='\t')
    if args.get('cluster_loci'):
        # the graph's labels go to the device table first (a long-read index holds them on the host only)
        write_cluster_loci(f'{basename}.mappings.cluster_loci.bed', interval_tree.cluster_loci(network),
                           chrom_to_num_map)
    if args.get('cluster_junctions'):
        # the table of --cluster-loci, when it ran, is the graph's: its loci rows are used as they are
        write_cluster_junctions(f'{basename}.mappings.cluster_junctions.bed', f'{basename}.mappings.bed', interval_tree,
                                None if args.get('cluster_loci') else network, chrom_to_num_map,
                                bool(args.get('cluster_long_reads')))
    if args.get('cluster_paths'):
        write_cluster_paths(f'{basename}.mappings.cluster_paths.bed', f'{basename}.mappings.bed', interval_tree,
                            None if args.get('cluster_loci') or args.get('cluster_junctions') else network,
                            chrom_to_num_map, bool(args.get('cluster_long_reads')))
    if args.get('cluster_path_segments'):
        write_cluster_path_segments(f'{basename}.mappings.cluster_path_segments.bed', f'{basename}.mappings.bed',
                                    interval_tree,
                                    None if args.get('cluster_loci') or args.get('cluster_junctions') or
                                    args.get('cluster_paths') else network, chrom_to_num_map)
    if args.get('cluster_path_segments_any'):
        # an earlier flag made the graph's table, unless it only printed its notice about long reads
        chains = (args.get('cluster_junctions') or args.get('cluster_paths')) and \
            (args.get('cluster_long_reads') or getattr(interval_tree, 'long', None) is None)
        write_cluster_path_segments(f'{basename}.mappings.cluster_path_segments.bed', f'{basename}.mappings.bed',
                                    interval_tree, None if args.get('cluster_loci') or chains else network,
                                    chrom_to_num_map, any_length=True)
    if args.get('cluster_path_containment'):
        # the graph's table is made anew: whatever an earlier flag left (or, for long reads, did not make) is replaced
        write_cluster_path_containment(f'{basename}.mappings.cluster_path_containment.bed', f'{basename}.mappings.bed',
                                       interval_tree, network)
    if args.get('cluster_collapsed_segments'):
        # as above: the graph's table is made anew
        write_cluster_collapsed_segments(f'{basename}.mappings.cluster_collapsed_segments.bed', f'{basename}.mappings.bed',
                                         interval_tree, network, chrom_to_num_map)
    t['write'] = time.perf_counter() - t3
    if args.get('timings'):
        st = network.stats
        print('timings_s ' + ' '.join(f'{k}={v:.3f}' for k, v in t.items()) +
              f' evaluated_pairs={st["evaluated_pairs"]} edges={st["n_edges"]} max_fwd={st["max_fwd"]}',
              file=sys.stderr)
    return True


def main():  # console entry
    pipeline()


if __name__ == '__main__':
    main()
