/*
 * fslr_hip.h — C ABI of the MI355X (gfx950) clustering hot path of fslr.
 *
 * The reference (kcleal/fslr, pure Python) has no native FFI for this path; its
 * hot path is the Python driver in fslr/cluster.py calling the third-party
 * native interval index `superintervals`.  Each entry point below replaces one
 * reference interface (file:line into /root/reference/fslr/):
 *
 *   fslr_set_reads        cluster.py:189-191  the per-read interval lists
 *                         (`query_intervals`) handed to the driver, packed CSR
 *   fslr_build_index      cluster.py:124-130  build_interval_trees (per-chrom
 *                         superintervals.IntervalMap add/build)
 *   fslr_query            cluster.py:187-227  query_interval_trees: candidate
 *                         search (:201), seen-set (:205-208),
 *                         different_lengths_or_alignments (:178-183),
 *                         overall_jaccard_similarity (:140-170),
 *                         calculate_overlap (:133-136), cutoff lookup (:218-219)
 *   fslr_query_shard      the same over one multi-GPU shard of the query reads
 *   fslr_components       cluster.py:230-234  get_subgraphs (networkx
 *                         connected_components)
 *   fslr_set_chrom_filter,
 *   fslr_sweep_partition,
 *   fslr_sweep_evaluate   cluster.py:187-227 split over ranks by chromosome (the sweep engine's
 *                         multi-GPU path)
 *   fslr_union_pairs      (multi-GPU merge of per-shard component labels; no
 *                         reference counterpart — the reference is single-process)
 *   fslr_copy_edges_device, fslr_components_from_pairs, fslr_local_forest,
 *   fslr_copy_forest_pairs
 *                         (multi-GPU merge of the ranks' gathered local forests: get_subgraphs,
 *                         cluster.py:230-234, over the union of the ranks' edges)
 *   fslr_copy_edges_iu_device,
 *   fslr_cap_install_edges,
 *   fslr_cap_local,
 *   fslr_cap_copy_local,
 *   fslr_cap_replay      cluster.py:197-224 the edge cap (:223-224) replayed on a rank that holds every
 *                         E* edge but indexes only its chromosomes (multi-GPU)
 *   fslr_cap_install_pairs, fslr_cap_sizes, fslr_cap_dep_local, fslr_cap_shard_plan,
 *   fslr_cap_shard_pack, fslr_cap_replay_shard, fslr_cap_copy_changes,
 *   fslr_cap_apply_changes, fslr_cap_bwd_counts, fslr_cap_restrict, fslr_cap_copy_restricted,
 *   fslr_cap_install_restricted
 *                         cluster.py:197-224 the same loops sharded over the ranks by the components of
 *                         the candidates' hit graph (multi-GPU)
 *   fslr_set_long_reads,
 *   fslr_long_query,
 *   fslr_get_long_edges   cluster.py:140-170 overall_jaccard_similarity for reads of more than
 *                         FSLR_MAX_L intervals (the reference has no limit; its l2_comparisons
 *                         scratch holds 100000 columns, :195)
 *   fslr_search,
 *   fslr_search_hits      cluster.py:201 tree[chrom].search_values(start, end) (superintervals
 *                         IntervalMap), for a batch of arbitrary query intervals
 *   fslr_score_pairs      cluster.py:209-219 the pair predicates of the loop for a batch of arbitrary
 *                         ordered read pairs: different_lengths_or_alignments (:178-183),
 *                         overall_jaccard_similarity (:140-170), calculate_overlap (:133-136) and
 *                         the cutoff lookup (:216-219)
 *   fslr_coverage_build,
 *   fslr_coverage_at      cluster.py:52-77 calc_coverage / filter_high_coverage: the read depth of the
 *                         bed rows at a batch of arbitrary (chrom, position) points, without the
 *                         dense per-chromosome arrays
 *   fslr_cluster_table,
 *   fslr_get_cluster_ids,
 *   fslr_get_cluster_members  cluster.py:230-234 get_subgraphs as a table over read ranks: the components of
 *                         >= 2 reads numbered in networkx order (ascending smallest rank), every read's
 *                         component id and size, and each component's reads
 *   fslr_assign_clusters  main.py:251-342 assign_clusters (the numbering of main.py:334-342) over qname codes
 *   fslr_choose_representatives
 *                         cluster.py:237-254 choose_alignment: per cluster the qname with the highest mean
 *                         alignment_score, the first in frame order on ties (idxmax)
 *   fslr_match_reads,
 *   fslr_match_rows       cluster.py:197-222 the pair loop for query reads that are not in the uploaded set:
 *                         the search (:201), the seen-set (:205-208) and the pair predicates (:209-219)
 *                         against the resident index, without the edge cap (:223-224)
 *   fslr_append_reads     cluster.py:109-121, 189-191 prepare_data's start-sorted `data` list and the per-read
 *                         lists for a set that grows: the lists of the union, made from the resident ones and
 *                         a new batch's (the reference rebuilds both from the whole frame)
 *   fslr_remove_reads     cluster.py:80-86 delete_false followed by :109-121, 189-191 prepare_data for a set that
 *                         shrinks: the lists of the frame without some reads, made from the resident ones
 *
 * Conventions: plain C types, caller-owned host arrays, library-owned device
 * memory behind an opaque context.  Every function returns FSLR_OK (0) or an
 * error code; fslr_last_error() gives the message.  Calls on one context are
 * not re-entrant; different contexts are independent.
 *
 * Semantics the caller folds in on the host (so the device does integer work
 * only, bit-exact to the reference's IEEE-double comparisons):
 *   iv_thr[k]   overlap threshold of interval k for `calculate_overlap >= overlap`
 *               (cluster.py:133-136): with o = max(0, min(e1,e2) - max(s1,s2)),
 *               interval k accepts o iff  thr >= 0 ? o >= thr : o <= ~thr.
 *               FSLR_THR_ZERO_ALN marks aln_size == 0 (the reference raises
 *               ZeroDivisionError when such an interval is compared).
 *   pass_table  [FSLR_MAX_L][2*FSLR_MAX_L] bytes: pass_table[(I-1)*2*FSLR_MAX_L + (U-1)]
 *               = (I/U >= cutoff(I)) evaluated in Python floats (cluster.py:218-219).
 *   qlen_cut, nal_cut = 1 - qlen_diff, 1 - n_alignment_diff (Python floats);
 *               the device evaluates fl(min/max) >= cut in IEEE double, as Python does,
 *               once per query read to get the exact integer range of partner values that
 *               pass (the ratio test is monotone on each side of the read's own value).
 */
#ifndef FSLR_HIP_H
#define FSLR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FSLR_ABI_VERSION 21
#define FSLR_MAX_L 64                /* max intervals per read (bitmask width) */
#define FSLR_MAX_READS (1 << 25)     /* read rank packs into bits 6..30 of the index record */
#define FSLR_THR_ZERO_ALN INT32_MIN

enum {
    FSLR_OK = 0,
    FSLR_ERR_ZERO_DIVISION = 1,   /* the reference would raise ZeroDivisionError */
    FSLR_ERR_INVALID = 2,         /* bad arguments / unsupported input */
    FSLR_ERR_HIP = 3,             /* HIP runtime failure */
    FSLR_ERR_NOMEM = 4,
    FSLR_ERR_STATE = 5            /* call order violated (e.g. query before index) */
};

typedef struct fslr_ctx fslr_ctx;

/* Rank-ordered CSR of the prepared intervals.  Reads are in first-appearance
 * order of the start-sorted `data` list; a read's intervals are in `data` order
 * (cluster.py:189-191).  All coordinates must lie in [0, 2^30). */
typedef struct {
    int64_t n_reads;
    int64_t n_intervals;
    int32_t n_chroms;              /* iv_chrom values lie in [0, n_chroms) */
    const int32_t *read_off;       /* [n_reads+1] */
    const int32_t *read_qlen2;     /* [n_reads]  keep_fillings qlen2 (cluster.py:26-29) */
    const int32_t *read_nal;       /* [n_reads]  n_alignments, in [0, 2^24) */
    const int32_t *iv_chrom;       /* [n_intervals] */
    const int32_t *iv_start;       /* min(rstart, rend)  (cluster.py:111) */
    const int32_t *iv_end;         /* max(rstart, rend)  (cluster.py:112) */
    const int32_t *iv_thr;         /* folded overlap threshold, see above */
    const int32_t *iv_data_pos;    /* optional (NULL): position of each interval in the start-sorted
                                      `data` list (cluster.py:114).  With it the index build is one
                                      stable pass on chromosome instead of a (chrom, start) sort. */
} fslr_reads;

/* fslr_params.flags & 3: the pair engine of fslr_query.  Both compute the same edge set E*,
 * forward degrees and ZeroDivisionError; they differ in what they count (fslr_query_stats).
 *   WALK   one wavefront per query read walks its intervals' hits and dedupes its partners
 *          (the reference's seen-set): counts evaluated_pairs and jaccard_evals.  Any input.
 *   SWEEP  one forward sweep over the sorted index meets every overlapping interval pair once;
 *          match entries are grouped per read and the greedy runs per pair (sweep.hip).  Needs
 *          overlap thresholds >= 1 (overlap > 0) and no aln_size == 0 interval; does not count
 *          evaluated_pairs / jaccard_evals (reported as -1).  It takes no read range: a forced
 *          SWEEP evaluates the pairs of every read, whatever [a_begin, a_end) of fslr_query.
 *   AUTO   SWEEP when the input allows it and the query covers all reads, else WALK. */
#define FSLR_ENGINE_AUTO 0
#define FSLR_ENGINE_WALK 1
#define FSLR_ENGINE_SWEEP 2

typedef struct {
    double qlen_cut;               /* 1 - qlen_diff */
    double nal_cut;                /* 1 - n_alignment_diff */
    const uint8_t *pass_table;     /* host pointer, FSLR_MAX_L * 2*FSLR_MAX_L bytes */
    int32_t edge_threshold;        /* main.py:221 (10); reported against, see max_fwd */
    int32_t flags;                 /* FSLR_ENGINE_* in bits 0..1; other bits reserved, 0 */
} fslr_params;

typedef struct {
    int64_t evaluated_pairs;       /* unique candidate read pairs (the reference's seen-set size) */
    int64_t jaccard_evals;         /* pairs that passed different_lengths_or_alignments */
    int64_t candidates;            /* WALK: interval-level index hits (before pair dedupe); SWEEP: overlapping
                                      interval pairs of two different reads */
    int64_t n_edges;               /* edges of E* (may exceed edge capacity, see fslr_reserve_edges) */
    int32_t max_fwd;               /* max over reads of forward (higher-rank) edges */
    int32_t error;                 /* FSLR_OK or FSLR_ERR_ZERO_DIVISION */
    int32_t err_a, err_b;          /* read ranks of the pair that raised */
    int64_t algo_bytes;            /* sum over evaluated pairs of 16*(L_A+L_B)+32 */
    int64_t overflow_candidates;   /* candidates of reads past the per-wave partner-set limit (witness path) */
    int64_t gather_pairs;          /* pairs evaluated by gathering B's intervals (general thresholds,
                                      aln_size==0 replay, match-list overflow) */
    int64_t match_entries;         /* matching interval pairs recorded in the per-read match lists (SWEEP:
                                      of read pairs that pass different_lengths_or_alignments) */
    int64_t matched_pairs;         /* read pairs with at least one matching interval pair (SWEEP: gate-passing) */
    int64_t deferred;              /* entries on the deferred (gather-evaluated) list */
    int64_t deferred_capacity;     /* its capacity; deferred > capacity ⇒ FSLR_ERR_STATE, reserve + rerun */
    int64_t edge_capacity;         /* edge buffer capacity; n_edges > capacity ⇒ reserve + rerun */
    int64_t walked_records;        /* index records the pair kernels walked (every partner-partition pass) */
    int32_t engine;                /* FSLR_ENGINE_WALK or FSLR_ENGINE_SWEEP: the engine that ran */
    int32_t overflow_flags;        /* 1 deferred list, 2 edge buffer, 4 sweep partner table (rerun with WALK),
                                      8 | 16 sweep entry buffers (rerun) */
    int64_t pair_tests;            /* SWEEP: overlapping interval pairs tested (each pair once) */
    int64_t entry_capacity;        /* SWEEP: match-entry buffer (grown automatically) */
    int64_t zd_pairs;              /* read pairs whose evaluation raises ZeroDivisionError (both qlen2 or both
                                      n_alignments 0 at the length gate, cluster.py:178-183; an aln_size == 0
                                      interval met by first-fit, :133-136).  The reference raises only if a loop
                                      reaches one: always when the edge cap does not bind (max_fwd <=
                                      edge_threshold: fslr_read_stats returns FSLR_ERR_ZERO_DIVISION after
                                      fslr_query), otherwise fslr_apply_edge_cap decides.  After
                                      fslr_sweep_partition / fslr_sweep_evaluate / fslr_long_query /
                                      fslr_long_pairs the caller decides (the binding may be known only over
                                      every rank); overflow_flags 64: the list grew, rerun the query */
} fslr_query_stats;

typedef struct {
    float index_ms;                /* fslr_build_index device time */
    float query_ms;                /* fslr_query: pair kernel device time (events around the launch) */
    float components_ms;           /* union-find device time */
    float total_ms;                /* first to last event of the last fslr_run/individual calls */
    float pair_kernel_ms;          /* the main pair-kernel launch alone (WALK: query_kernel; SWEEP: the count pass) */
    float sweep_count_ms;          /* SWEEP phases of the last query: count pass (+ statistics), */
    float sweep_emit_ms;           /*   emit pass, */
    float sweep_sort_ms;           /*   grouping sort, */
    float sweep_pairs_ms;          /*   per-read pair evaluation */
} fslr_timings;

/* The reference's per-query-read edge cap (cluster.py:223-224), see fslr_apply_edge_cap. */
typedef struct {
    int32_t applied;               /* 1: the cap bound (max forward degree > edge_threshold) and was replayed */
    int32_t max_fwd;               /* max over reads of the edges formed in the read's own loop */
    int64_t candidates;            /* reads whose loop could reach the cap (replayed) */
    int64_t capped;                /* reads whose loop reached it (left hits unvisited) */
    int64_t hits;                  /* index hits of the replayed loops */
    int64_t pairs;                 /* distinct pairs of those hits, evaluated on the device */
    int64_t dropped;               /* E* edges that no loop reached (absent from the reference graph) */
    int64_t backward;              /* edges formed in the higher-rank read's loop */
} fslr_cap_stats;

int  fslr_abi_version(void);
/* first 16 hex digits of the sha256 of the kernel sources the library was built from (the sorted
 * .hip and .hpp files of fslr_amd/csrc, then this header): a binding can refuse a stale build */
const char *fslr_source_hash(void);
const char *fslr_last_error(const fslr_ctx *ctx);

/* device: HIP ordinal; stream: hipStream_t to launch on (NULL = the library creates one). */
int  fslr_ctx_create(int device, void *stream, fslr_ctx **out);
void fslr_ctx_destroy(fslr_ctx *ctx);
int  fslr_set_profiling(fslr_ctx *ctx, int enable);     /* 1: hipEvents per phase + around the pair kernel;
                                                           2: around the pair kernel only (fewer stream
                                                           markers in a timed loop); 0: off */
/* enable (the default) = a sweep query on unchanged input (reads, thresholds, filter, range, cuts) repeats
 * the last synchronous one: it keeps the length-gate ranges and its entry count stays on the device (no
 * mid-query readback).  0 = every query does the full work, as a single query on new input does. */
int  fslr_set_query_reuse(fslr_ctx *ctx, int enable);

/* Copy the CSR (host pointers) into context-owned HBM buffers (H2D). */
int  fslr_set_reads(fslr_ctx *ctx, const fslr_reads *reads);
/* The clustering input from rows (the columnar CLI path).  fslr_rows_upload copies
 * keep_fillings' rows (cluster.py:14-31), file order, as int64 columns (syncs; a caller may run it while
 * it sorts the starts).  fslr_set_reads_rows takes prepare_data's start order of those rows (the
 * argsort of `start`, cluster.py:114) and, optionally, mask_sequences2's keep flag per row
 * (cluster.py:89-106); on the device it forms the `data` list, ranks the reads by first appearance in
 * it and groups each read's intervals in data order (cluster.py:189-191), numbers the chromosomes
 * present densely in ascending order, folds the overlap thresholds for `overlap` (fslr_reads iv_thr)
 * and sets the reads as fslr_set_reads with iv_data_pos would.  A read of more than FSLR_MAX_L
 * intervals sets nothing: FSLR_ERR_INVALID with info->max_len > FSLR_MAX_L (use fslr_set_reads_any).
 * fslr_get_read_codes: the qname code of each read rank.  fslr_get_csr: the CSR the device made (as
 * fslr_reads with its folded thresholds, plus aln_size per interval, the data position of each interval and the chromosome
 * number of each dense id; NULL outputs are skipped).  fslr_fold_thresholds: the thresholds of another
 * overlap, folded on the device (as fslr_set_thresholds). */
typedef struct {
    int64_t n_rows;                /* fillings */
    int64_t n_codes;               /* qcode values lie in [0, n_codes) */
    int64_t n_chrom_ids;           /* chrom values lie in [0, n_chrom_ids) */
    const int64_t *chrom;          /* rename_chromosomes' number (cluster.py:34-43) */
    const int64_t *start, *end;    /* min / max of rstart, rend (cluster.py:111-112) */
    const int64_t *aln;            /* aln_size */
    const int64_t *qcode;          /* the row's qname code */
    const int64_t *nal;            /* n_alignments */
    const int64_t *qlen2;          /* the row's read's keep_fillings qlen2 */
} fslr_rows;
typedef struct {
    int64_t n_reads, n_intervals;
    int32_t n_chroms;              /* chromosomes present (dense ids) */
    int32_t max_len;               /* longest read */
    int32_t nal_varies;            /* n_alignments differs between intervals of a read */
    int32_t general_thresholds;    /* a threshold below 1 (overlap <= 0): the sweep does not apply */
    int32_t any_zero_aln;          /* an aln_size == 0 interval */
    int32_t pad;
} fslr_rows_info;
int  fslr_rows_upload(fslr_ctx *ctx, const fslr_rows *rows);
int  fslr_set_reads_rows(fslr_ctx *ctx, const int64_t *order, const uint8_t *keep, double overlap,
                         fslr_rows_info *info);
int  fslr_get_read_codes(fslr_ctx *ctx, int64_t *codes);
int  fslr_get_csr(fslr_ctx *ctx, int32_t *read_off, int32_t *read_qlen2, int32_t *read_nal, int32_t *iv_chrom,
                  int32_t *iv_start, int32_t *iv_end, int64_t *iv_aln, int32_t *iv_thr, int64_t *data_pos,
                  int64_t *chrom_ids);
int  fslr_fold_thresholds(fslr_ctx *ctx, double overlap);
/* Replace the folded overlap thresholds (iv_thr, CSR order) without re-uploading
 * or re-indexing: the index does not depend on them (calculate_overlap's
 * `percentage`, cluster.py:157, is a query-time parameter). */
int  fslr_set_thresholds(fslr_ctx *ctx, const int32_t *iv_thr);
/* Edge buffer capacity (edges of E*); grows only. */
int  fslr_reserve_edges(fslr_ctx *ctx, int64_t capacity);
/* Deferred-pair list capacity (pairs evaluated by gathering intervals); grows only. */
int  fslr_reserve_deferred(fslr_ctx *ctx, int64_t capacity);

/* Multi-GPU: build the query-side index data (positions, scan ranges) only for the reads of
 * query shard `shard` of `n_shards` (see fslr_query_shard); the walked index stays complete.
 * Takes effect at the next fslr_build_index; fslr_query then needs n_shards == 1. */
int  fslr_set_shard(fslr_ctx *ctx, int32_t shard, int32_t n_shards);
/* cluster.py:124-130 — sort intervals by (chrom, start), prefix-max of end. Async. */
int  fslr_build_index(fslr_ctx *ctx);
/* cluster.py:187-227 — all candidate pairs of query reads with rank in
 * [a_begin, a_end) against every read of higher rank.  Async; stats are read
 * with fslr_read_stats. */
int  fslr_query(fslr_ctx *ctx, const fslr_params *params, int64_t a_begin, int64_t a_end);
/* Multi-GPU query shard: the reads of rank blocks [64 k, 64 k + 64) with k % n_shards == shard
 * (balanced: low ranks have more higher-rank partners).  The shards of 0..n_shards-1 together
 * evaluate exactly the pairs of fslr_query(ctx, params, 0, n_reads).  Async. */
int  fslr_query_shard(fslr_ctx *ctx, const fslr_params *params, int32_t shard, int32_t n_shards);
/* cluster.py:197-224 — the edge cap.  The query computes E* (every candidate pair); when a read
 * has more than edge_threshold forward edges, the reference's graph depends on the order its loops
 * visit pairs.  This replays those loops exactly (search order of the superintervals stand-in the
 * golden fixtures were made with: descending (start, -end, data position)) for the reads that can
 * reach the cap, drops the E* edges no loop reaches, re-orients edges as (read whose loop formed
 * it, partner) and sets forward degrees to the edges formed per loop.  No-op (no sync beyond one
 * counter read) when the cap does not bind.  Needs the last query to be fslr_query over all reads
 * (or fslr_cap_install_edges on an unfiltered index).  The replay runs on the device: loops of
 * different components of the candidates' partner graph are independent.
 * Call between fslr_query and fslr_components.  Syncs; out may be NULL.
 * edge_threshold <= 0 is replayed like any other value: the reference's check `edges >= edge_threshold`
 * (:223) then holds from the start, so every read is a candidate (reads without hits too) and every
 * interval's visit ends at its first new pair that passes the gate with I > 0, edge or not.
 * A second call after a replay, without a new query, leaves the capped graph alone and reports
 * applied = 0 with the capped graph's max_fwd (which post-break walks can leave above the threshold). */
int  fslr_apply_edge_cap(fslr_ctx *ctx, int32_t edge_threshold, fslr_cap_stats *out);
/* The same check without a host round trip, for a repeated query on unchanged input: the device ORs
 * (max forward degree > edge_threshold) | (a listed ZeroDivisionError pair) << 1 into a sticky word (async);
 * fslr_edge_cap_deferred_read syncs, returns the word and clears it.  A nonzero word means a step needed
 * fslr_apply_edge_cap (or raised): its results are to be recomputed synchronously.  FSLR_ERR_STATE on a
 * context that never had reads set (no query can have run). */
int  fslr_edge_cap_deferred(fslr_ctx *ctx, int32_t edge_threshold);
int  fslr_edge_cap_deferred_read(fslr_ctx *ctx, int32_t *flags);
/* cluster.py:230-234 — union-find over the edges: label = min rank in component.  Async.  Every query
 * resets the parents to the identity; a sweep-engine query (fslr_query, fslr_sweep_evaluate) also
 * pre-hooks them as its pair kernel forms the edges, and the next fslr_components / fslr_local_forest
 * then runs only the unions (any call that rewrites the edges or the parents in between — the edge cap,
 * fslr_sort_edges, fslr_reserve_edges, an upload, fslr_union_pairs — makes it start from the identity
 * again).  Labels (fslr_get_labels) are those of the last fslr_components / fslr_local_forest /
 * fslr_components_from_pairs until the next query. */
int  fslr_components(fslr_ctx *ctx);
/* Multi-GPU sweep.  A rank indexes only the chromosomes it owns, sweeps them and
 * routes the match entries to the rank owning each pair's first read, which evaluates the pairs.
 * An interval only meets intervals of its own chromosome (cluster.py:159-160), so the first-fit
 * matching of a pair is the union of its per-chromosome matchings and the split is exact.
 *
 * fslr_set_chrom_filter: owned[n_chroms] != 0 marks the chromosomes the next fslr_build_index
 * indexes (NULL: all).  Needs iv_data_pos and n_chroms <= 64.  The filtered index serves only
 * fslr_sweep_partition (fslr_query refuses it).  Syncs.
 * fslr_sweep_partition: sweep the filtered index (every query read, the pair gates applied) and
 * write its match entries (8 bytes each, layout internal to the library) to the device buffer dst
 * grouped by destination k = (a >> block_shift) % n_dest, a = the pair's first (lower-rank) read:
 * rank blocks dealt round robin, n_dest <= 64; counts[k] = entries for k.  Syncs; FSLR_ERR_STATE if
 * sum(counts) > dst_cap (counts are still filled: grow dst and call again).  Pairs that raise
 * ZeroDivisionError are listed, not raised (fslr_query_stats zd_pairs; fslr_cap_local raises for those
 * the capped loops reach).
 * fslr_sweep_evaluate: evaluate the pairs of the n entries (a device buffer: every rank's segment
 * for this rank, concatenated in any order) into this context's edges and forward degrees.  Every
 * entry of a pair must be present, so each pair's first read belongs to one destination.  Needs only
 * fslr_set_reads.  Async; fslr_read_stats / fslr_components / fslr_get_edges follow as after
 * fslr_query. */
int  fslr_set_chrom_filter(fslr_ctx *ctx, const uint8_t *owned);
/* The position split: a rank sweeps a contiguous range of the (chrom, start)-sorted
 * positions, cut where the pair tests balance, whatever the chromosomes.
 * fslr_position_costs: after fslr_build_index over every chromosome, per tile of 64 sorted positions
 *   its pair tests (the sum of its forward counts) and the end of its forward window (max q + n_fwd(q)
 *   + 1); n_tiles = ceil(n_intervals / 64).  Syncs.
 * fslr_set_position_filter: the next fslr_build_index indexes the sorted positions [lo, end) only and
 *   fslr_sweep_partition sweeps the pairs whose lower position lies in [lo, hi); end must cover the
 *   forward windows of [lo, hi) (fslr_position_costs).  Every pair of overlapping intervals is met by
 *   the rank holding its lower position.  Needs iv_data_pos and <= 64 chromosomes.  Syncs.
 * fslr_position_entries: after fslr_build_index over every chromosome, the match entries of each
 *   tile under the query parameters p (the one-pass sweep over the full index, as fslr_query's):
 *   the per-entry work (partition, exchange, evaluation) is most of a rank's cost where pair tests
 *   rarely match.  Syncs.
 * fslr_use_position_filter: make the last position filter of these reads active again (after
 *   fslr_set_chrom_filter, which the edge cap's sharded replay lists its hits with). */
int  fslr_position_costs(fslr_ctx *ctx, int64_t *tile_tests, int64_t *tile_reach, int64_t n_tiles);
int  fslr_position_entries(fslr_ctx *ctx, const fslr_params *p, int64_t *tile_entries, int64_t n_tiles);
int  fslr_set_position_filter(fslr_ctx *ctx, int64_t lo, int64_t hi, int64_t end);
int  fslr_use_position_filter(fslr_ctx *ctx);
/* Multi-GPU edge cap (cluster.py:197-224).  The replayed loops need every E* edge
 * and every hit of the reads that can reach the cap; a rank's index holds its chromosomes' hits.
 * fslr_copy_edges_iu_device: this context's edges as int32 rows {a, b, I | U << 8, 0} into a device
 *   buffer of n_pad rows, padded with a = -1 (async).  The ranks all-gather them.
 * fslr_cap_install_edges: the n_rows gathered rows (device; a < 0 = padding) become this context's
 *   edge list and forward degrees (as after a full query).  Syncs.
 * fslr_cap_local: the replay's candidates, their intervals (*n_ti, the same on every rank) and the
 *   search-ordered hits of the intervals this rank's index holds (*n_hits).  Syncs.
 * fslr_cap_copy_local: counts[n_ti] (int32, 0 for other ranks' intervals) and hits[n_hits] (the
 *   partner reads, interval after interval) into device buffers (async).  The ranks all-gather both:
 *   counts as world x n_ti, hits padded to `pad` per rank.
 * fslr_cap_replay: replay the loops from the gathered lists and write the capped graph into this
 *   context as fslr_apply_edge_cap does (every rank gets the same graph).  Syncs; out may be NULL. */
int  fslr_copy_edges_iu_device(fslr_ctx *ctx, int32_t *dst, int64_t n_pad);
int  fslr_cap_install_edges(fslr_ctx *ctx, const int32_t *rows, int64_t n_rows);
int  fslr_cap_local(fslr_ctx *ctx, int32_t edge_threshold, int64_t *n_ti, int64_t *n_hits);
int  fslr_cap_copy_local(fslr_ctx *ctx, int32_t *counts, int32_t *hits);
int  fslr_cap_replay(fslr_ctx *ctx, const int32_t *counts, const int32_t *hits, int64_t pad, int32_t world,
                     fslr_cap_stats *out);
/* The multi-GPU edge cap sharded over the ranks (cluster.py:197-224).  Two loops of the
 * replay depend on each other only when an interval of one read hits an interval of the other, so the
 * components of that graph over the candidates T replay independently, each on one rank.
 * fslr_cap_install_pairs: n_rows gathered E* rows as int32 (a, b) pairs (device; a < 0 = padding;
 *   rank w's block is rows [w m, (w + 1) m), m = n_rows / world, in its fslr_copy_edges_device order,
 *   after fslr_sort_edges).  The rows are read in place: keep them unchanged until
 *   fslr_cap_apply_changes.
 *   This context's own edges stay its edge list; fslr_cap_local then computes the closure T over the
 *   gathered rows and lists the hits of T's intervals on this rank's chromosomes (async + syncs).
 * fslr_cap_sizes: |T|, its intervals, the local hits (after fslr_cap_local).
 * fslr_cap_dep_local: out[2 |T|] (device): out[t] = the root (smallest index) of T read t in the forest
 *   of the T-T hits on this rank's chromosomes, out[|T| + t] = its local hit count (async).
 * fslr_cap_shard_plan: gathered = the ranks' out arrays (world x 2 |T|).  Unions the forests, assigns the
 *   components to ranks by cost (hits; largest first onto the least-loaded rank: the same on every
 *   rank) and groups the local lists by destination.  sizes[d] = T-intervals sent to rank d (the same on
 *   every rank), sizes[world + d] = local hits sent to rank d.  Syncs.
 * fslr_cap_shard_pack: counts (sum sizes[0 .. world) int32) and hits (sum sizes[world ..)) for one
 *   all_to_all each, destination-major (async).  The rank receives world x sizes[rank] counts.
 * fslr_cap_replay_shard: replays the loops of this rank's components from the received counts and hits
 *   (source-major) and lists the gathered rows it decides that the lower read's loop does not form:
 *   *n_changes of them; part (may be NULL): its candidates, capped loops, hits and slots.  Syncs.
 * fslr_cap_copy_changes: the changes (int32 row << 2 | who, who 1 = formed in b's loop, 2 = dropped)
 *   padded with -1 to n_pad (device, async).  The ranks all-gather them.
 * fslr_cap_apply_changes: every rank's changes: this context keeps its own capped edges (re-oriented as
 *   (former, partner)) and their formers' counts (fwd), errw max_fwd = the largest edges-per-loop;
 *   the components of the capped graph then come from the ranks' local forests (fslr_local_forest).
 *   Syncs; out: applied, max_fwd, candidates, dropped, backward (capped / hits / pairs: the sum of the
 *   ranks' parts).
 * The restricted gather: only rows whose lower read x has fwd(x) + bwd(x) >= edge_threshold over E* can
 * take part (the closure's join test, cluster.py:210-213 via DESIGN.md §11), about 3% of E* at cfg5.
 * fslr_cap_bwd_counts: this rank's counts of its edges per upper read b into out
 *   (device, n_reads elements of elem_bytes: 1 = uint8 clipped at edge_threshold <= 255, 4 = int32;
 *   async); the caller sums them over the ranks (all_reduce; uint8 needs world x threshold <= 255).
 * fslr_cap_restrict: from the summed counts, this rank's rows of S (its edges whose lower read has
 *   fwd + bwd >= threshold, sorted by lower read: no fslr_sort_edges of the whole list is needed);
 *   *n_rows = their count (syncs).
 * fslr_cap_copy_restricted: those rows as int32 (a, b) pairs padded with -1 to n_pad (device, async).
 * fslr_cap_install_restricted: the ranks' gathered restricted rows, as fslr_cap_install_pairs (the rest
 *   of the sequence is unchanged); fslr_cap_apply_changes then maps this rank's block back onto its
 *   edges and its max_fwd covers S and this rank's reads outside S: the MAX over ranks is the capped
 *   graph's. */
/* The multi-GPU merge by local forests (get_subgraphs, cluster.py:230-234, over the union of the ranks'
 * edges).  fslr_local_forest: union-find over this context's edges; the (read, root) pairs of the
 * reads that are not their own root are kept (the same partition as the edges, in fewer pairs);
 * *n_pairs (may be NULL: no sync) gets their count.  fslr_copy_forest_pairs: those pairs as int32
 * (read, root) into a device buffer of n_pad pairs, padded with -1 (async).  The ranks all-gather
 * them and fslr_components_from_pairs takes the union. */
int  fslr_local_forest(fslr_ctx *ctx, int64_t *n_pairs);
int  fslr_copy_forest_pairs(fslr_ctx *ctx, int32_t *dst, int64_t n_pad);
/* fslr_sort_edges: this context's edge list (with I, U) grouped by a, stably, in place (syncs once for
 * the count).  The sharded cap's ranks sort before the gather, so each read's forward edges are one run of
 * the gathered rows (the closure walks the runs; unsorted blocks still work: their closure runs over
 * every row per round, as for a context's own edge list). */
int  fslr_sort_edges(fslr_ctx *ctx);
int  fslr_cap_install_pairs(fslr_ctx *ctx, const int32_t *pairs, int64_t n_rows, int32_t world, int32_t rank);
int  fslr_cap_sizes(fslr_ctx *ctx, int64_t *n_t, int64_t *n_ti, int64_t *n_hits);
int  fslr_cap_dep_local(fslr_ctx *ctx, int32_t *out);
int  fslr_cap_shard_plan(fslr_ctx *ctx, const int32_t *gathered, int32_t world, int32_t rank, int64_t *sizes);
int  fslr_cap_shard_pack(fslr_ctx *ctx, int32_t *counts, int32_t *hits);
int  fslr_cap_replay_shard(fslr_ctx *ctx, const int32_t *counts, const int32_t *hits, int64_t *n_changes,
                           fslr_cap_stats *part);
int  fslr_cap_copy_changes(fslr_ctx *ctx, int32_t *dst, int64_t n_pad);
int  fslr_cap_apply_changes(fslr_ctx *ctx, const int32_t *changes, int64_t n, fslr_cap_stats *out);
int  fslr_cap_bwd_counts(fslr_ctx *ctx, int32_t edge_threshold, void *out, int32_t elem_bytes);
int  fslr_cap_restrict(fslr_ctx *ctx, const void *bwd, int32_t elem_bytes, int64_t *n_rows);
int  fslr_cap_copy_restricted(fslr_ctx *ctx, int32_t *dst, int64_t n_pad);
int  fslr_cap_install_restricted(fslr_ctx *ctx, const int32_t *pairs, int64_t n_rows, int32_t world, int32_t rank);
int  fslr_sweep_partition(fslr_ctx *ctx, const fslr_params *params, int32_t n_dest, int32_t block_shift,
                          void *dst, int64_t dst_cap, int64_t *counts);
int  fslr_sweep_evaluate(fslr_ctx *ctx, const fslr_params *params, const void *entries, int64_t n);
/* fslr_sweep_partition_repeat: fslr_sweep_partition again on unchanged input (no fslr_set_* since),
 * parameters and split, without the readback: the entries land where the last synchronous call put
 * them (its counts), and a device check flags any difference (fslr_read_stats then returns
 * FSLR_ERR_STATE with overflow_flags & 32: rerun synchronously).  Async.  FSLR_ERR_STATE when the last
 * synchronous call was for another input, parameters or split.  The repeated steps of a benchmark
 * or of a service querying one resident input use it. */
int  fslr_sweep_partition_repeat(fslr_ctx *ctx, const fslr_params *params, int32_t n_dest, int32_t block_shift,
                                 void *dst, int64_t dst_cap);

/* Reads of more than FSLR_MAX_L intervals.  The caller uploads a *virtual* CSR with
 * fslr_set_reads: virtual read v < n_real is real read v (its first <= FSLR_MAX_L intervals), reads
 * v >= n_real are the further <= FSLR_MAX_L-interval chunks of the long reads; vreal[v] = its real
 * read, vbase[v] = the index of its first interval in the real read's list, rlen[r] = the real
 * read's interval count, umax[I-1] = the largest U with I/U >= cutoff(I) (cluster.py:216-219, Python
 * floats), for I = 1 .. n_umax >= max(rlen).  Syncs.
 * fslr_long_query (after fslr_build_index): sweep the virtual index (every match entry), decide the
 * pairs with a long read with the reference's first-fit over their real interval lists (list1 = the
 * lower-rank read) into a list of (a, b, I, U) edges (*n_long_edges), and the pairs of two short
 * reads with the sweep's pair stage into the context's edges and forward degrees (as fslr_query:
 * fslr_read_stats, reserve and rerun on overflow; then fslr_components).  Syncs.
 * fslr_get_long_edges: D2H of the long-pair edges (sync); union them into the labels with
 * fslr_union_pairs + fslr_finalize_labels after fslr_components. */
int  fslr_set_long_reads(fslr_ctx *ctx, int64_t n_real, const int32_t *vreal, const int32_t *vbase,
                         const int32_t *rlen, const int32_t *umax, int32_t n_umax);
/* The same without a caller-made split: fslr_set_reads_any takes the REAL CSR (reads of 1..4096
 * intervals), makes the virtual CSR and maps above and uploads them (as fslr_set_reads when no read
 * exceeds FSLR_MAX_L).  Later fslr_set_thresholds calls take iv_thr in the real CSR's interval order
 * too.  fslr_set_long_cutoffs sets umax (as above) before fslr_long_query / fslr_long_pairs /
 * fslr_cap_replay_pairs.  Replaces the host-side split a binding would otherwise re-implement
 * (reference: overall_jaccard_similarity takes lists of any length, cluster.py:140-170). */
int  fslr_set_reads_any(fslr_ctx *ctx, const fslr_reads *reads);
int  fslr_set_long_cutoffs(fslr_ctx *ctx, const int32_t *umax, int32_t n_umax);
int  fslr_long_query(fslr_ctx *ctx, const fslr_params *params, int64_t *n_long_edges);
int  fslr_get_long_edges(fslr_ctx *ctx, int32_t *a, int32_t *b, int32_t *I, int32_t *U, int64_t capacity);
/* The general pair path (any overlap, aln_size == 0 intervals, qlen2 / n_alignments
 * 0, reads of up to 4096 intervals), replacing cluster.py:197-222 where the sweep's gates do not
 * apply.  fslr_long_pairs (after fslr_set_reads [+ fslr_set_long_reads] and fslr_build_index):
 * every read's search-ordered hits, each distinct pair decided once by the reference's first-fit
 * (list1 = the lower-rank read) into the long-edge list (fslr_get_long_edges, I and U unclamped) and
 * the context's edges and forward degrees (then fslr_components); FSLR_ERR_ZERO_DIVISION when a pair
 * raises.  Syncs.
 * fslr_cap_replay_pairs: the edge cap (cluster.py:223-224) replayed over the given E* — ne pairs of
 * real read ranks a < b, host arrays — in the read space of the last fslr_set_reads (+
 * fslr_set_long_reads).  who[k] = 0 when edge k is formed in a's loop, 1 in b's, 2 when the capped
 * graph drops it; fwd[n_reads] (may be NULL) = edges formed in each read's own loop.  The capped
 * graph also becomes the context's edges (fslr_components).  Syncs; out may be NULL. */
int  fslr_long_pairs(fslr_ctx *ctx, const fslr_params *params, int64_t *n_edges);
/* fslr_long_pairs for the pairs whose lower-rank read lies in query shard `shard` of `n_shards` (read
 * blocks of 64 dealt round robin, as fslr_query_shard): the shards together give fslr_long_pairs'
 * edges, each pair once (the multi-GPU split of the inputs the sweep does not take). */
int  fslr_long_pairs_shard(fslr_ctx *ctx, const fslr_params *params, int32_t shard, int32_t n_shards,
                           int64_t *n_edges);
int  fslr_cap_replay_pairs(fslr_ctx *ctx, int32_t edge_threshold, const int32_t *a, const int32_t *b, int64_t ne,
                           uint8_t *who, int32_t *fwd, fslr_cap_stats *out);

/* build_index + query(all reads) + components, enqueued back to back.  Async. */
int  fslr_run(fslr_ctx *ctx, const fslr_params *params);

int  fslr_sync(fslr_ctx *ctx);
/* syncs; returns stats.error, or FSLR_ERR_STATE when the edge or deferred buffer overflowed
 * (reserve and rerun the query: components and labels of an overflowed query are refused) */
int  fslr_read_stats(fslr_ctx *ctx, fslr_query_stats *out);
int  fslr_get_timings(fslr_ctx *ctx, fslr_timings *out);        /* syncs */
/* Profiling: durations (ms) of the main pair-kernel launch of the last min(n, 256) queries since
 * profiling was enabled, oldest first (hipEvents recorded on the context's stream around that one
 * launch).  Syncs; returns the count or -error. */
int  fslr_get_pair_kernel_times(fslr_ctx *ctx, float *ms, int32_t n);
/* The same for one stage kernel: stage 0 = the main pair kernel (as above), 1 = the sweep engine's
 * pair-stage kernel (the evaluation of the grouped match entries).  Syncs; count or -error. */
int  fslr_get_stage_kernel_times(fslr_ctx *ctx, int32_t stage, float *ms, int32_t n);
/* Raw device counters of the last query (diagnostics; layout is internal, kernels.hpp:
 * Counter).  Copies min(n, 32) words, syncs, returns the count or -error. */
int  fslr_read_counters(fslr_ctx *ctx, uint64_t *out, int n);

/* D2H copies (sync). */
int  fslr_get_labels(fslr_ctx *ctx, int32_t *labels);          /* [n_reads] min-rank root; FSLR_ERR_STATE
                                                                   after an overflowed query */
int  fslr_get_fwd_degree(fslr_ctx *ctx, int32_t *fwd);         /* [n_reads] */
int  fslr_get_edges(fslr_ctx *ctx, int32_t *a, int32_t *b, uint16_t *iu, int64_t capacity);
                                                                /* iu = I | (U << 8); returns count via stats */

/* Batched interval search on the built index: what the reference's pair loop asks per interval,
 * cluster.py:201 `tree[itv.chrom].search_values(itv.start, itv.end)` (superintervals IntervalMap
 * search_values), for n_queries arbitrary intervals at once.
 *   Query (chrom, start, end) hits a stored interval (c, s, e) iff c == chrom, s <= end and
 *   e >= start (end-inclusive; no order of start / end is assumed).  `chrom` is the dense id of the
 *   uploaded CSR; an id outside [0, n_chroms) has no hits.
 *   Order contract: a query's hits come in descending position of the order (start ascending, end
 *   descending, data position ascending), data position = iv_data_pos[k] where the reads came with
 *   it, else the CSR index k.  This is the search order of the superintervals stand-in
 *   (tests/golden/refharness.py), as for fslr_apply_edge_cap; the order of the real superintervals
 *   build may differ between its versions.  The same bytes on every run.
 *   Reads uploaded without iv_data_pos (a list that is not start-sorted) are ranked by CSR index
 *   where (start, end) tie, since the library never saw their data positions: a caller that wants
 *   the list's own order there re-orders those ties itself (fslr_amd.cluster search_batch does).
 * fslr_search counts: offsets (NULL, or [n_queries + 1]) gets the exclusive prefix of the hit counts,
 * *n_hits (may be NULL) their total.  fslr_search_hits then writes the last fslr_search's hits, query
 * after query: indices into the CSR the caller uploaded (fslr_set_reads / fslr_set_reads_any), or
 * into the CSR fslr_get_csr returns (fslr_set_reads_rows).  capacity < total: FSLR_ERR_INVALID, the
 * message carries the count, nothing is written.  n_queries == 0 is valid.  The saved batch belongs
 * to the reads and the index build it was made on: after another fslr_set_reads* or fslr_build_index,
 * fslr_search_hits returns FSLR_ERR_STATE until the next fslr_search.
 * FSLR_ERR_STATE: no index built, a chromosome or position filter active, or n_shards > 1 (a partial
 * index cannot answer).  What the search needs beyond fslr_build_index's work is built on the first
 * search of an index; the query state (edges, labels, degrees, the cap) is left alone.  Sync. */
int  fslr_search(fslr_ctx *ctx, int64_t n_queries, const int32_t *chrom, const int32_t *start, const int32_t *end,
                 int64_t *offsets, int64_t *n_hits);
int  fslr_search_hits(fslr_ctx *ctx, int32_t *hits, int64_t capacity);
/* Profiling (fslr_set_profiling 1): HIP-event times (ms) of the last fslr_search's passes, ms[0..3] =
 * span, count, the scans, fill (0 until fslr_search_hits ran). */
int  fslr_search_timings(fslr_ctx *ctx, float *ms);

/* The pair predicates for a batch of arbitrary ordered read pairs: what the reference's pair loop
 * computes once its search has produced a pair (cluster.py:209-219), whether or not any query would
 * reach that pair.  Pair k = (a[k], b[k]), ranks of the uploaded reads; list1 = read a's intervals,
 * list2 = read b's, both in CSR (data) order; a == b is scored like any other pair.  Per pair, at its
 * input position:
 *   I, U     overall_jaccard_similarity's intersection and union (cluster.py:140-170): first-fit, rows
 *            of list1 ascending, each row takes the lowest unused column of list2 on its chromosome
 *            with calculate_overlap >= overlap; U = L1 + L2 - I.  Computed whether or not the gate
 *            passes.
 *   flags    FSLR_SCORE_GATE        different_lengths_or_alignments is False (cluster.py:178-183)
 *            FSLR_SCORE_EDGE        GATE and I > 0 and pass_table[(I-1)*2*FSLR_MAX_L + (U-1)] (:216-219)
 *            FSLR_SCORE_ZD_GATE     the gate raises ZeroDivisionError (max(qlen2) == 0, or the second
 *                                   ratio is reached with max(n_alignments) == 0); GATE is clear
 *            FSLR_SCORE_ZD_OVERLAP  calculate_overlap raises: first-fit reaches a same-chromosome
 *                                   unused column where either interval has aln_size == 0 before the
 *                                   row's first match.  The reference stops there: I = U = 0, EDGE clear.
 * ZeroDivisionError is only flagged, never returned.  From params the call uses qlen_cut, nal_cut and
 * pass_table (edge_threshold and flags are ignored); the overlap thresholds are the ones currently set
 * (fslr_set_thresholds / fslr_fold_thresholds).  Host pointers; syncs.  n_pairs == 0 is valid.
 * FSLR_ERR_STATE: no reads set.  FSLR_ERR_INVALID: a rank outside [0, n_reads) (the message names the
 * first offending position; nothing is written), or the context holds virtual reads (fslr_set_reads_any
 * with a read of more than FSLR_MAX_L intervals, fslr_set_long_reads): reads of more than FSLR_MAX_L
 * intervals are scored by fslr_score_pairs_any.  Needs only the CSR: works with or without a built index,
 * under a chromosome or position filter and with n_shards > 1.  The query state (edges, labels, degrees,
 * the cap, the ZeroDivisionError list, every error word) and the saved search batch are left alone.
 * Scratch grows on demand, bounded: a large batch is processed in chunks.
 * fslr_score_timings (fslr_set_profiling 1 or 2): HIP-event times (ms) of the last fslr_score_pairs,
 * ms[0..2] = upload, kernel, download, summed over its chunks. */
enum { FSLR_SCORE_GATE = 1, FSLR_SCORE_EDGE = 2, FSLR_SCORE_ZD_GATE = 4, FSLR_SCORE_ZD_OVERLAP = 8 };
int  fslr_score_pairs(fslr_ctx *ctx, const fslr_params *params, int64_t n_pairs, const int32_t *a, const int32_t *b,
                      int32_t *I, int32_t *U, uint8_t *flags);
int  fslr_score_timings(fslr_ctx *ctx, float *ms);

/* Read depth at query points: the reference's calc_coverage (cluster.py:52-67) adds +1 at rstart and -1
 * at rend of every bed row of a chromosome and takes the running sum; filter_high_coverage (:70-77)
 * reads that sum at one position per interval.  For a chromosome c and a position p
 *   cov[c][p] = #{rows of c with rstart <= p} - #{rows of c with rend <= p}
 * so a row counts at its rstart and no longer at its rend, a row with rstart == rend changes nothing and
 * a row with rstart > rend gives -1 in between.  Nothing of the genome's length is allocated.
 * fslr_coverage_build: the n_rows bed rows as (dense chromosome id in [0, n_chroms), rstart, rend), in
 * any order; the library keeps their sorted (chrom, rstart) and (chrom, rend) keys and every
 * FSLR_COVERAGE_TILE-th key of each.  One resident coverage set per context: a build replaces it,
 * fslr_ctx_destroy frees it.  n_rows == 0 is valid (depth 0 everywhere).  Host pointers; syncs.
 * FSLR_ERR_INVALID: a chromosome id outside [0, n_chroms) or a negative position (the message names the
 * first offending row); the resident set is unchanged, as after any other failed build.
 * fslr_coverage_at: depth[k] = cov[chrom[k]][pos[k]] for n_queries queries in any order, each written at
 * its input position; the same bytes on every run.  Positions beyond a chromosome's last row are valid
 * (the library knows no lengths).  n_queries == 0 is valid.  Host pointers; syncs.  FSLR_ERR_STATE: no
 * coverage built.  FSLR_ERR_INVALID: a chromosome id outside the build's [0, n_chroms) or a negative
 * position (the message names the first offending query); nothing is written.  Queries go up in chunks
 * of FSLR_COVERAGE_CHUNK: the scratch does not grow with the batch.
 * Neither call needs fslr_set_reads or a built index, and both work under a chromosome or position
 * filter and with n_shards > 1.  The query state (edges, labels, degrees, the cap, the ZeroDivisionError
 * list, every error word), the saved search batch and the score scratch are left alone.
 * fslr_coverage_timings (fslr_set_profiling 1 or 2): HIP-event times (ms) of the last calls, ms[0..3] =
 * build upload (with the key packing), build sort (both sorts and the tile keys), query upload + kernel,
 * query download, each summed over the call's chunks; 0 for a call that was not profiled. */
#define FSLR_COVERAGE_TILE 256
#define FSLR_COVERAGE_CHUNK (1 << 21)
int  fslr_coverage_build(fslr_ctx *ctx, int64_t n_rows, int32_t n_chroms, const int32_t *chrom, const int32_t *rstart,
                         const int32_t *rend);
int  fslr_coverage_at(fslr_ctx *ctx, int64_t n_queries, const int32_t *chrom, const int32_t *pos, int32_t *depth);
int  fslr_coverage_timings(fslr_ctx *ctx, float *ms);

/* The cluster table: what the reference rebuilds on the host from the connected components
 * (get_subgraphs, cluster.py:230-234; assign_clusters, main.py:251-342; choose_alignment,
 * cluster.py:237-254), from min-rank labels on the device.
 * fslr_cluster_table: labels == NULL takes the context's device labels (the parents after fslr_components,
 *   fslr_components_from_pairs, fslr_local_forest or fslr_finalize_labels; n is ignored): FSLR_ERR_STATE
 *   without reads, after an overflowed query (as fslr_get_labels) or when the labels are not final;
 *   FSLR_ERR_INVALID when the context holds virtual reads (as fslr_score_pairs; pass their labels from the
 *   host).  labels != NULL takes a host vector of n <= 2^30 min-rank labels (the multi-GPU and long-read
 *   paths hold theirs on the host); it needs no reads and no index.  The labels are checked on the device:
 *   labels[r] must lie in [0, r] and labels[labels[r]] == labels[r]; FSLR_ERR_INVALID names the first
 *   offending r and the resident table is unchanged.
 *   The table: size[r] = reads of r's component; cid[r] = the position of its root among the roots with
 *   size >= 2 in ascending root order (networkx's component order), -1 where size == 1; the member CSR
 *   lists each cluster's ranks ascending (its first member is its root).  One resident table per context:
 *   a call replaces it, fslr_ctx_destroy frees it.  n == 0 is valid.  The same bytes on every run.  Syncs;
 *   info may be NULL.  The query state, the saved search batch, the score scratch and the coverage set are
 *   left alone.
 * fslr_get_cluster_ids / fslr_get_cluster_members: D2H of the table (NULL outputs are skipped);
 *   FSLR_ERR_STATE without a table.
 * fslr_assign_clusters (main.py:334-342 in qname-code space): code_of_rank[n] = the qname code of each read
 *   rank (NULL: the identity, n_codes == n), present[n_codes] marks the codes that have rows in the bed
 *   file.  A present code whose rank has cid >= 0 gets that cid and size; every other present code gets
 *   n_clusters + k, k = its index among such codes in ascending code order (first-appearance order), and
 *   size 1; absent codes get -1 / 0.  *n_singletons (may be NULL) = the count of those other codes; the
 *   caller applies the reference's dtype rule (float columns when it is not 0).  FSLR_ERR_STATE without a
 *   table.  FSLR_ERR_INVALID for a code outside [0, n_codes) or a code a lower rank names too: the
 *   message names the first offending rank and nothing is written.  Host pointers; syncs.
 * fslr_choose_representatives (cluster.py:237-254 in code space; independent of the resident table):
 *   codes with cluster < 0 or score_cnt == 0 are skipped, their avg is NaN; for the others avg[c] =
 *   (double)score_sum[c] / (double)score_cnt[c] in IEEE double on the device.  winner_code[k], k < n_out,
 *   = the code with the largest avg in cluster k, ties to the smallest first_row (idxmax: the first row
 *   in frame order), -1 for a cluster without a code.  FSLR_ERR_INVALID for |score_sum| >= 2^53 (the
 *   float64 sum of such scores would not be exact), cluster >= n_out or score_cnt < 0, of any code: the
 *   message names the first offender and nothing is written.  Host pointers; syncs; every array goes up
 *   and down through a bounded pinned chunk.
 * fslr_cluster_timings (fslr_set_profiling 1 or 2): HIP-event times (ms), first to last operation on the
 *   stream, of the last fslr_cluster_table, fslr_assign_clusters and fslr_choose_representatives (ms[0..2];
 *   0 for a call that was not profiled). */
typedef struct {
    int64_t n_clusters;            /* components of >= 2 reads */
    int64_t n_nodes;               /* reads in them (G.number_of_nodes()) */
    int64_t max_size;              /* largest component, 0 if none */
} fslr_cluster_info;
int  fslr_cluster_table(fslr_ctx *ctx, const int32_t *labels, int64_t n, fslr_cluster_info *info);
int  fslr_get_cluster_ids(fslr_ctx *ctx, int32_t *cid, int32_t *size);                  /* [n] each */
int  fslr_get_cluster_members(fslr_ctx *ctx, int64_t *off, int32_t *members);           /* [n_clusters + 1], [n_nodes] */
int  fslr_assign_clusters(fslr_ctx *ctx, int64_t n_codes, const int64_t *code_of_rank, const uint8_t *present,
                          int64_t *cluster, int64_t *n_reads, int64_t *n_singletons);
int  fslr_choose_representatives(fslr_ctx *ctx, int64_t n_codes, const int64_t *cluster, const int64_t *score_sum,
                                 const int64_t *score_cnt, const int64_t *first_row, int64_t n_out, double *avg,
                                 int64_t *winner_code);
int  fslr_cluster_timings(fslr_ctx *ctx, float *ms);

/* Cluster loci: per cluster of the resident table and per chromosome, the merged spans of its reads'
 * intervals (the clustering input, every interval of every member read) and their support.
 *   Within one (cluster, chromosome) group the intervals are walked in ascending start; an interval opens a
 *   new locus iff it is the group's first or its start is greater than the largest end seen so far in the
 *   group (end-inclusive, the index's overlap convention: start == that end merges, start == that end + 1
 *   does not).  A row per locus: chrom (the context's dense id), start (its first interval's), end (the
 *   largest end in it), n_intervals, n_reads (distinct real reads among them).  Rows are ordered by
 *   (cluster, chrom, start); off[n_clusters + 1] gives each cluster's row range.  Reads with cid < 0 give
 *   nothing; no clusters give 0 rows and off == {0}.  The rows depend on the interval sets alone and are the
 *   same bytes on every run.
 *   On a context with virtual reads (reads of more than FSLR_MAX_L intervals) the table must be one of
 *   n_real labels (a host vector); a chunk's intervals count for its real read, once per locus.
 * fslr_cluster_loci: computes the rows and keeps them resident (*n_rows, may be NULL); syncs.
 *   FSLR_ERR_STATE, named in the message: no reads set; no index built (or a partial one: a chromosome or
 *   position filter, n_shards > 1); no cluster table; a table whose n differs from the context's real read
 *   count (a stale table after fslr_append_reads* / fslr_remove_reads*).  A failed call leaves the previous
 *   rows and everything else as they were; a successful call replaces the rows; fslr_cluster_table drops
 *   them; fslr_ctx_destroy frees them.  The query state, the saved search batch, the score scratch and the
 *   coverage set are left alone.  FSLR_LOCI_TILE (256, 512, 1024 or 2048; read per call) sets the scan's
 *   tile for tests.
 * fslr_get_cluster_loci: D2H of the rows (NULL outputs are skipped): off[n_clusters + 1], the others
 *   [n_rows].  FSLR_ERR_STATE without rows, FSLR_ERR_INVALID when capacity < n_rows (nothing is written).
 * fslr_cluster_loci_timings (fslr_set_profiling 1 or 2): HIP-event time (ms[0]), first to last operation
 *   on the stream, of the last fslr_cluster_loci; FSLR_ERR_STATE when it was not profiled. */
int  fslr_cluster_loci(fslr_ctx *ctx, int64_t *n_rows);
int  fslr_get_cluster_loci(fslr_ctx *ctx, int64_t *off, int32_t *chrom, int32_t *start, int32_t *end,
                           int32_t *n_intervals, int32_t *n_reads, int64_t capacity);
int  fslr_cluster_loci_timings(fslr_ctx *ctx, float *ms);

/* Cluster junctions: which locus ends the reads of each cluster join, and where the breakpoints lie.  On top
 * of reads, a whole built index, the resident cluster table and the resident loci rows (fslr_cluster_loci).
 *   Inputs, two caller-owned host arrays in CSR interval order, n_intervals each: iv_qkey, the interval's
 *   position in its read's query order (qstart in practice; any int32, only the order matters), and iv_rev
 *   (may be NULL = all 0), 1 when the interval runs against the query order.
 *   Chain: for every real read r with cid[r] >= 0 and at least two resident intervals, its intervals ordered
 *   by (iv_qkey ascending, CSR position ascending on equal keys); each consecutive pair (x, y) is one
 *   observation.  Only resident intervals count: an interval dropped by the mask before the upload is not in
 *   the chain, its neighbours are consecutive.
 *   Ends: an interval lies in the one locus row of its read's cluster with its chromosome and
 *   start <= iv.start <= end (a global row index of fslr_get_cluster_loci).  The chain leaves x at its right
 *   end (side 1, breakpoint x.end) when rev[x] == 0, else at its left end (side 0, x.start); it enters y at
 *   its left end (side 0, y.start) when rev[y] == 0, else at its right end (side 1, y.end).  An end is
 *   e = locus_row * 2 + side.
 *   Canonical form: the unordered pair, stored as (ea, eb) with ea <= eb, the breakpoints swapped with the
 *   ends; on ea == eb the smaller breakpoint is stored first.  A read and its reverse complement (order
 *   reversed, every rev flipped) give identical observations.
 *   Rows: one per distinct (ea, eb), ordered by (ea, eb), which is cluster order: locus_a, side_a, locus_b,
 *   side_b, n_obs (observations), n_reads (distinct real reads among them), and the extrema of the two
 *   breakpoints.  off[n_clusters + 1] gives each cluster's row range.  No clusters, or no clustered read with
 *   two intervals, give 0 rows and off all zero.  The bytes are the same on every run.
 * fslr_cluster_junctions: computes the rows and keeps them resident (*n_rows, may be NULL); syncs.
 *   FSLR_ERR_STATE, named in the message: no reads set; no index built (or a partial one); no cluster table;
 *   a table whose n differs from the context's real read count (stale after fslr_append_reads* /
 *   fslr_remove_reads*); no resident loci rows of this table (fslr_cluster_loci first).  FSLR_ERR_INVALID:
 *   iv_qkey NULL; n_intervals different from the context's; a context with virtual reads (reads of more than
 *   FSLR_MAX_L intervals are out of scope here); more than 2^30 intervals.  A failed call keeps the previous
 *   rows, a successful one replaces them; whatever drops or replaces the loci rows (fslr_cluster_table, a
 *   successful fslr_cluster_loci) drops them; fslr_ctx_destroy frees them.  The query state, the saved
 *   batches and the loci rows are left alone.
 * fslr_get_cluster_junctions: D2H of the rows (NULL outputs are skipped): off[n_clusters + 1]; locus_a,
 *   locus_b, n_obs, n_reads [n_rows]; sides [n_rows] = side_a | side_b << 1; bp [4 x n_rows] = the columns
 *   a_min, a_max, b_min, b_max one after another.  FSLR_ERR_STATE without rows, FSLR_ERR_INVALID when
 *   capacity < n_rows (nothing is written).
 * fslr_cluster_junctions_timings (fslr_set_profiling 1 or 2): HIP-event time (ms[0]) of the last
 *   fslr_cluster_junctions, from the end of the two columns' upload to the last operation on the stream;
 *   FSLR_ERR_STATE when it was not profiled. */
int  fslr_cluster_junctions(fslr_ctx *ctx, const int32_t *iv_qkey, const uint8_t *iv_rev, int64_t n_intervals, int64_t *n_rows);
int  fslr_get_cluster_junctions(fslr_ctx *ctx, int64_t *off, int32_t *locus_a, int32_t *locus_b, uint8_t *sides /* side_a | side_b << 1 */,
                                int32_t *n_obs, int32_t *n_reads, int32_t *bp /* [4 x n_rows]: a_min, a_max, b_min, b_max */, int64_t capacity);
int  fslr_cluster_junctions_timings(fslr_ctx *ctx, float *ms);

/* Cluster paths: the distinct read structures of each cluster, the ordered chain of (locus, strand) pieces a
 * read walks, and how many reads of the cluster agree on each chain.  Two different chains can share every
 * junction, so the junction rows do not give this.  On top of reads, a whole built index, the resident cluster
 * table and the resident loci rows of that table (fslr_cluster_loci).
 *   Inputs, those of fslr_cluster_junctions: iv_qkey[n_intervals] and iv_rev[n_intervals] (may be NULL = all 0),
 *   caller-owned host arrays in CSR interval order.
 *   Chain: for every real read r with cid[r] >= 0, one-interval reads included, its resident intervals ordered
 *   by (iv_qkey ascending, CSR position ascending on equal keys).
 *   Token: an interval gives t = locus_row * 2 + rev.  locus_row is the global loci row of its read's cluster
 *   that holds it (the rule of the junctions: same chromosome, start <= iv.start <= end), rev its strand bit.
 *   Canonical form: the forward sequence is F = (t_0 .. t_{L-1}); the same molecule read from the other strand
 *   is B = (t_{L-1} ^ 1, .., t_0 ^ 1), the order reversed and every low bit flipped.  The read's path is the
 *   lexicographically smaller of F and B, and flipped[r] = 1 iff B < F strictly: a palindromic chain F == B
 *   (only possible for an even length) has flipped = 0.
 *   Reverse complement: a read and its reverse complement have the same path and opposite flipped, unless the
 *   chain is palindromic.  This holds for a read with distinct query keys; on equal keys the chain order falls
 *   back to the CSR position, which a reverse complement does not reverse.
 *   Rows: one per distinct path, in ascending lexicographic order of the token sequence, a proper prefix before
 *   its extensions.  That is cluster order: the loci rows are cluster-ordered and a path's first token lies in
 *   its cluster's rows.  A row holds n_reads (the reads with this path), first_read (the smallest read rank
 *   among them) and its tokens behind tok_off[n_rows + 1] as locus[n_tokens] and rev[n_tokens].
 *   off[n_clusters + 1] gives each cluster's row range.  Per read: path_of_read[n] is the global row, -1 for a
 *   read that is not clustered, and flipped[n] is 0 where path_of_read is -1.  The n_reads of a cluster's rows
 *   sum to the cluster's size.  No clusters give 0 rows and off all zero.  No hash decides equality and the
 *   bytes are the same on every run.
 * fslr_cluster_paths: computes the rows and keeps them resident (*n_rows, *n_tokens, may be NULL); syncs.
 *   FSLR_ERR_STATE, named in the message: no reads set; no index built (or a partial one); no cluster table;
 *   a table whose n differs from the context's real read count (stale after fslr_append_reads* /
 *   fslr_remove_reads*); no resident loci rows of this table (fslr_cluster_loci first).  FSLR_ERR_INVALID:
 *   iv_qkey NULL; n_intervals different from the context's; a context with virtual reads (reads of more than
 *   FSLR_MAX_L intervals are out of scope here); more than 2^30 intervals.  A failed call keeps the previous
 *   rows, a successful one replaces them; whatever drops or replaces the loci rows (fslr_cluster_table, a
 *   successful fslr_cluster_loci) drops them; fslr_ctx_destroy frees them.  The junction rows, the loci rows,
 *   the query state, the saved batches, the score scratch and the coverage set are left alone, and
 *   fslr_cluster_junctions leaves the path rows alone.  The exact grouping is an LSD radix sort over chain
 *   positions, several tokens per 64-bit key; the environment variable FSLR_PATHS_PACK (1..8, read per call)
 *   caps the tokens per key and changes no result.
 * fslr_get_cluster_paths: D2H of the rows (NULL outputs are skipped): off[n_clusters + 1]; tok_off[n_rows + 1];
 *   n_reads, first_read [n_rows]; locus, rev [n_tokens]; path_of_read, flipped [n reads].  FSLR_ERR_STATE
 *   without rows, FSLR_ERR_INVALID when row_capacity < n_rows or token_capacity < n_tokens (nothing is written).
 * fslr_cluster_paths_timings (fslr_set_profiling 1 or 2): HIP-event time (ms[0]) of the last
 *   fslr_cluster_paths, from the end of the two columns' upload to the last operation on the stream;
 *   FSLR_ERR_STATE when it was not profiled. */
int  fslr_cluster_paths(fslr_ctx *ctx, const int32_t *iv_qkey, const uint8_t *iv_rev, int64_t n_intervals, int64_t *n_rows, int64_t *n_tokens);
int  fslr_get_cluster_paths(fslr_ctx *ctx, int64_t *off, int64_t *tok_off, int32_t *n_reads, int32_t *first_read, int32_t *locus, uint8_t *rev,
                            int32_t *path_of_read, uint8_t *flipped, int64_t row_capacity, int64_t token_capacity);
int  fslr_cluster_paths_timings(fslr_ctx *ctx, float *ms);

/* Cluster junctions and paths for reads of any length: fslr_cluster_junctions / fslr_cluster_paths for a context
 * that holds virtual reads (fslr_set_reads_any, fslr_set_long_reads), as fslr_score_pairs_any stands beside
 * fslr_score_pairs.  The contract is the one above, read for real reads of 1..FSLR_MAX_ANY_L intervals.
 *   Inputs      iv_qkey / iv_rev (may be NULL = all 0) in the REAL CSR's interval order, n_intervals the real
 *               interval count: the order fslr_set_thresholds takes iv_thr in after fslr_set_reads_any (the call
 *               brings them to the virtual order itself; after fslr_set_long_reads, where the caller uploaded the
 *               virtual CSR, the two orders are the same).
 *   Chain       all the intervals of real read r, the chunks behind its first FSLR_MAX_L included, ordered by
 *               (iv_qkey ascending, position in the real list ascending on equal keys).  A chunk is never a read
 *               of its own.
 *   Table       one of n_real labels (the rule of fslr_cluster_loci); cid, path_of_read and flipped are per real
 *               read, n_real of them.
 *   Rows        the resident rows of the plain calls: fslr_get_cluster_junctions, fslr_get_cluster_paths and the
 *               two _timings calls answer for them, whatever drops or frees those rows drops or frees these, a
 *               failed call keeps the previous rows.
 *   Errors      those of the plain calls without the refusal of virtual reads.  FSLR_ERR_INVALID beyond 2^30
 *               intervals (the observations and the clustered tokens are fewer).
 *   On a context without virtual reads each call runs the code of its plain call and leaves the same bytes.
 *   Reads of more than FSLR_MAX_L intervals take one workgroup each (their chain is sorted in LDS); the path
 *   grouping sorts, in the pass of a position group, only the reads long enough to reach it, so its work is the
 *   sum of the reads' group counts.  FSLR_PATHS_PACK keeps its meaning.  One GPU: the whole index on the context. */
int  fslr_cluster_junctions_any(fslr_ctx *ctx, const int32_t *iv_qkey, const uint8_t *iv_rev, int64_t n_intervals, int64_t *n_rows);
int  fslr_cluster_paths_any(fslr_ctx *ctx, const int32_t *iv_qkey, const uint8_t *iv_rev, int64_t n_intervals, int64_t *n_rows, int64_t *n_tokens);

/* Path segments: for every piece (token slot) of every cluster path, where the piece lies in the reads that walk
 * this path (a locus is the merged span of ALL the cluster's reads on that chromosome, not the piece's extent),
 * and for every link between two consecutive pieces the query-space gap the reads leave there.  On top of what
 * fslr_cluster_paths needs plus the resident path rows of the current table.
 *   Inputs: iv_qkey[n_intervals], the column the paths were made with (the query start), and iv_qend[n_intervals]
 *   (the query end; may be NULL: no gaps are computed and the three gap columns are all 0); caller-owned host
 *   arrays in CSR interval order.  The strand column is not needed: flipped is resident.
 *   Chain, as for the paths: a clustered read's resident intervals ordered by (iv_qkey ascending, CSR position
 *   ascending on equal keys).  The interval at chain rank t of a read r of L intervals has canonical position
 *   p = flipped[r] ? L - 1 - t : t and lands in token slot s = tok_off[path_of_read[r]] + p, 0 <= s < n_tokens.
 *   L equals the row's length, so s always lies in the read's own row, whatever column the caller passes: a
 *   different iv_qkey gives this contract's answer for that column's order, never an out-of-range slot.
 *   Per slot, over the k = n_reads[row] intervals that land in it (one per read of the row), six int32 columns:
 *   start_min, start_med, start_max and end_min, end_med, end_max of the intervals' reference start and end.  The
 *   median is the lower median: with the values ascending, element (k - 1) / 2.
 *   Per link: a link joins slots s and s + 1 of one row and is stored at s.  The gap of a read there is iv_qkey
 *   of the later interval in the read's OWN chain order minus iv_qend of the earlier one, computed in 64 bits and
 *   saturated to int32: the same number whichever direction the read walks the path.  Negative: the two pieces
 *   overlap on the query (microhomology); positive: inserted sequence.  Columns gap_min, gap_med, gap_max; the
 *   last slot of every row holds 0, 0, 0.
 *   The bytes are the same on every run.
 * fslr_cluster_path_segments: computes the rows and keeps them resident (*n_tokens, may be NULL); syncs.
 *   FSLR_ERR_STATE, named in the message: those of fslr_cluster_paths (no reads set; no index built, or a partial
 *   one; no cluster table; a table whose n differs from the context's real read count; no loci rows of this
 *   table), and no resident path rows of this table (fslr_cluster_paths first).  FSLR_ERR_INVALID: iv_qkey NULL;
 *   n_intervals different from the context's; a context with virtual reads (reads of more than FSLR_MAX_L
 *   intervals are out of scope here); more than 2^30 intervals.  A failed call keeps the previous segment rows, a
 *   successful one replaces them; whatever drops or replaces the path rows (fslr_cluster_table, a successful
 *   fslr_cluster_loci, a successful fslr_cluster_paths / fslr_cluster_paths_any) drops them; fslr_ctx_destroy
 *   frees them.  The path, junction and loci rows, the query state and everything else are left alone.
 *   The selection runs in three tiers by k: 2..S in a lane group (counting by shuffles), S+1..T sorted in LDS by
 *   one workgroup, above T an exact radix select by one workgroup; k == 1 is written as it is met.  The
 *   environment variables FSLR_SEGS_SMALL (S, 1..64, default 64) and FSLR_SEGS_LDS (T, S..4096, default 4096) are
 *   read per call and change no result.
 * fslr_get_cluster_path_segments: D2H of the rows (NULL outputs are skipped): start, end, gap, each
 *   [3 x n_tokens] = the columns min, med, max one after another.  FSLR_ERR_STATE without rows, FSLR_ERR_INVALID
 *   when token_capacity < n_tokens (nothing is written).
 * fslr_cluster_path_segments_timings (fslr_set_profiling 1 or 2): HIP-event time (ms[0]) of the last
 *   fslr_cluster_path_segments, from the end of the columns' upload to the last operation on the stream;
 *   FSLR_ERR_STATE when it was not profiled. */
int  fslr_cluster_path_segments(fslr_ctx *ctx, const int32_t *iv_qkey, const int32_t *iv_qend, int64_t n_intervals, int64_t *n_tokens);
int  fslr_get_cluster_path_segments(fslr_ctx *ctx, int32_t *start /* [3 x n_tokens]: min, med, max */, int32_t *end, int32_t *gap,
                                    int64_t token_capacity);
int  fslr_cluster_path_segments_timings(fslr_ctx *ctx, float *ms);

/* Path segments for reads of any length: fslr_cluster_path_segments for a context that holds virtual reads
 * (fslr_set_reads_any, fslr_set_long_reads), as fslr_cluster_paths_any stands beside fslr_cluster_paths.  The
 * contract is the one above, read for real reads of 1..FSLR_MAX_ANY_L intervals.
 *   Inputs      iv_qkey / iv_qend (may be NULL: the gap columns are all 0) in the REAL CSR's interval order,
 *               n_intervals the real interval count: the order fslr_cluster_paths_any takes its columns in (the call
 *               brings them to the virtual order itself; after fslr_set_long_reads the two orders are the same).
 *   Chain       all the intervals of real read r, the chunks behind its first FSLR_MAX_L included, ordered by
 *               (iv_qkey ascending, position in the real list ascending on equal keys).  A chunk is never a read
 *               of its own; the link between positions FSLR_MAX_L - 1 and FSLR_MAX_L is a link like any other.
 *   Path rows   the resident ones of the current table, made by fslr_cluster_paths_any; path_of_read and flipped
 *               are per real read.
 *   Rows        the resident rows of the plain call: fslr_get_cluster_path_segments and
 *               fslr_cluster_path_segments_timings answer for them, whatever drops or frees those rows drops or
 *               frees these, a failed call keeps the previous rows.
 *   Errors      those of the plain call without the refusal of virtual reads.  FSLR_ERR_INVALID beyond 2^30
 *               intervals.
 *   On a context without virtual reads the call runs the code of the plain call and leaves the same bytes.
 *   A clustered read of more than FSLR_MAX_L intervals takes one workgroup (its chain is sorted in LDS); the
 *   selection tiers, FSLR_SEGS_SMALL and FSLR_SEGS_LDS keep their meaning: k counts the reads of a row, whatever
 *   their length.  One GPU: the whole index on the context. */
int  fslr_cluster_path_segments_any(fslr_ctx *ctx, const int32_t *iv_qkey, const int32_t *iv_qend, int64_t n_intervals, int64_t *n_tokens);

/* Path containment: which path rows are only truncated views of another row of their cluster, and what a
 * full-length row's support is once the truncated reads are counted.  A read that lost a piece at either end has
 * a path of its own in fslr_cluster_paths; this call finds, per cluster, the rows that are contiguous sub-chains of
 * a longer row, in either reading direction.  On top of the resident path rows of the current table alone
 * (fslr_cluster_paths / fslr_cluster_paths_any): no CSR, no uploaded column, no virtual reads, so one call serves
 * contexts with and without reads of more than FSLR_MAX_L intervals (a path row of up to FSLR_MAX_ANY_L tokens is
 * an ordinary row).
 *   Terms: row A has the tokens A[0..a-1], t = locus * 2 + rev; rc(A)[i] = A[a-1-i] ^ 1; A is palindromic when
 *   rc(A) == A.
 *   Containment: row A is contained in row B iff they lie in the same cluster, a < b, and there is an offset o in
 *   [0, b - a] and a direction d with B[o + i] == A[i] for all i (d = 0) or B[o + i] == rc(A)[i] for all i
 *   (d = 1).  Each such (o, d) is an occurrence.  For a palindromic A only d = 0 is probed, so the occurrences of
 *   a pair always have distinct offsets.  Rows of equal length are never contained in one another (two distinct
 *   canonical rows can be neither equal nor reverse complements) and are not probed.  Tokens of different
 *   clusters never compare equal, because a token names a loci row and the loci rows are per cluster: the
 *   same-cluster condition needs no check of its own.  Containment is transitive.
 *   Containment rows: one per contained pair (A, B), ordered by (A ascending, B ascending), behind
 *   coff[n_rows + 1] (indexed by the inner row A).  Columns: outer (B's global row), offset (the smallest offset
 *   among the pair's occurrences), rev (the direction of the occurrence at that offset), n_occ (the pair's
 *   occurrences).
 *   Per path row: n_inner (how many rows it contains); support (its n_reads plus the n_reads of every row it
 *   contains); collapse_to (the row itself when nothing contains it: it is maximal; otherwise, among the rows
 *   that contain it and are themselves maximal, the one with the largest support, ties to the smallest row:
 *   containment is transitive, so one always exists); collapsed_reads (for a maximal row its n_reads plus the
 *   n_reads of the rows that collapse to it, 0 for the others: the collapsed_reads of a cluster's rows sum to the
 *   cluster's size).  No path rows give empty outputs (coff = {0}).  The bytes are the same on every run.
 * fslr_cluster_path_containment: computes the rows and keeps them resident (*n_pairs, may be NULL); syncs.
 *   FSLR_ERR_STATE, named in the message: no cluster table; no resident path rows of this table
 *   (fslr_cluster_paths first).  FSLR_ERR_INVALID when the occurrences exceed 2^30 (the message names the
 *   count).  A failed call keeps the previous rows, a successful one replaces them; whatever drops or replaces
 *   the path rows (fslr_cluster_table, a successful fslr_cluster_loci, a successful fslr_cluster_paths /
 *   fslr_cluster_paths_any) drops them; fslr_ctx_destroy frees them.  The path, segment, junction and loci rows
 *   and all query state are left alone.  A table that went stale after fslr_append_reads* / fslr_remove_reads*
 *   still describes its path rows: the call reads no read and keeps answering for them.
 *   An inner row of at most 64 tokens is probed by a lane group, a longer one by a workgroup; every candidate
 *   comes from an index of the token occurrences, anchored at the inner row's first token (forward) and at its
 *   last token ^ 1 (reverse).
 * fslr_get_cluster_path_containment: D2H of the rows (NULL outputs are skipped): coff[n_rows + 1]; outer, offset,
 *   rev, n_occ [n_pairs]; n_inner, support, collapse_to, collapsed_reads [n_rows].  FSLR_ERR_STATE without rows,
 *   FSLR_ERR_INVALID when row_capacity < n_rows or pair_capacity < n_pairs (nothing is written).
 * fslr_cluster_path_containment_timings (fslr_set_profiling 1 or 2): HIP-event time (ms[0]) of the last
 *   fslr_cluster_path_containment, from its first operation on the stream to its last; FSLR_ERR_STATE when it
 *   was not profiled. */
int  fslr_cluster_path_containment(fslr_ctx *ctx, int64_t *n_pairs);
int  fslr_get_cluster_path_containment(fslr_ctx *ctx, int64_t *coff, int32_t *outer, int32_t *offset, uint8_t *rev, int32_t *n_occ,
                                       int32_t *n_inner, int64_t *support, int32_t *collapse_to, int64_t *collapsed_reads,
                                       int64_t row_capacity, int64_t pair_capacity);
int  fslr_cluster_path_containment_timings(fslr_ctx *ctx, float *ms);

/* Collapsed path segments: the consensus coordinates of the full-length paths.  fslr_cluster_path_segments takes
 * its order statistics over the reads that walk exactly one path row; fslr_cluster_path_containment says which
 * rows are truncated views of a full-length row (collapse_to).  This call fills, for every MAXIMAL path row
 * (collapse_to[row] == row), each slot with order statistics over ALL reads that collapse onto the row.  A
 * truncated read contributes at the slots it covers and nowhere else, so the number of contributing reads
 * differs from slot to slot and is reported.  On top of the resident path rows of the current table
 * (fslr_cluster_paths / fslr_cluster_paths_any) AND the resident containment rows of those path rows
 * (fslr_cluster_path_containment).
 *   Inputs and chain: those of fslr_cluster_path_segments.  iv_qkey [n_intervals] is the column the paths were
 *   made with; iv_qend [n_intervals] may be NULL: then the three gap columns are 0 and n_link is still filled.
 *   The chain order of a read is (key ascending, CSR position ascending on equal keys).
 *   Where a read lands: read r with row A = path_of_read[r], length a and chain rank t has the canonical position
 *   p = flipped[r] ? a-1-t : t.  Let B = collapse_to[A].  If B == A then q = p.  Otherwise the pair (A, B) is one
 *   of coff[A] .. coff[A + 1] (collapse_to is one of the rows that contain A; the outers ascend there); with its
 *   stored offset o and rev d, q = d ? o + (a-1-p) : o + p.  The interval lands in slot tok_off[B] + q.  The link
 *   between chain ranks t and t+1 is stored at slot tok_off[B] + min(q_t, q_t+1); its gap is that of
 *   fslr_cluster_path_segments: the later piece's key minus the earlier piece's iv_qend in the read's own chain
 *   order, computed in 64 bits and saturated to int32.  Every slot index is checked against the row B, which has
 *   at least a tokens by containment, so a column that is not the paths' own can never leave the row.
 *   Outputs per token slot of all path rows (n_tokens is that of the path rows): n_cov (the intervals that land
 *   in the slot), n_link (the read links stored there), start_min|med|max and end_min|med|max over the n_cov
 *   intervals' reference start and end, gap_min|med|max over the n_link gaps; each triple is [3 x n_tokens] as in
 *   fslr_get_cluster_path_segments.  The median is the lower median: element (k - 1) / 2 of the ascending values.
 *   The slots of rows that are not maximal hold 0 in every column; the last slot of a row has n_link = 0 and gap
 *   0, 0, 0.  The bytes are the same on every run.
 *   Decided: a truncated read's outermost pieces count with the coordinates they have.  The piece where a read
 *   broke off is shorter than the full-length reads' piece there; the median is robust against it, the minimum
 *   and the maximum widen, and n_cov shows how many reads stand behind a figure.
 * fslr_cluster_collapsed_segments: computes the rows and keeps them resident (*n_tokens, may be NULL); syncs.
 *   FSLR_ERR_STATE, named in the message: no resident path rows of this table (fslr_cluster_paths first); no
 *   resident containment rows of those path rows (fslr_cluster_path_containment first); and the state errors of
 *   fslr_cluster_path_segments (no reads, an index that cannot be searched, no table, a stale table, no loci).
 *   FSLR_ERR_INVALID: iv_qkey NULL, n_intervals != the context's, a context with virtual reads (the _any call
 *   takes it), more than 2^30 intervals.  Rows are allocated apart and swapped in at the end: a failed call
 *   keeps the previous rows.  A successful fslr_cluster_path_containment drops them, and so does whatever drops
 *   the containment rows or the path rows; fslr_ctx_destroy frees them.  Nothing else on the context is touched.
 * fslr_cluster_collapsed_segments_any: the same contract for a context with virtual reads (fslr_set_reads_any):
 *   the columns arrive in the real CSR's order, real reads have 1..FSLR_MAX_ANY_L intervals, a chunk is never a
 *   read of its own.  On a context without virtual reads the two calls leave the same bytes.
 * fslr_get_cluster_collapsed_segments: D2H of the rows (NULL outputs are skipped): n_cov, n_link [n_tokens];
 *   start, end, gap [3 x n_tokens].  FSLR_ERR_STATE without rows, FSLR_ERR_INVALID when token_capacity <
 *   n_tokens (nothing is written).
 * fslr_cluster_collapsed_segments_timings (fslr_set_profiling 1 or 2): HIP-event time (ms[0]) of the last
 *   call's device work, the uploads of the two columns excluded; FSLR_ERR_STATE when it was not profiled.
 *   FSLR_SEGS_SMALL and FSLR_SEGS_LDS move the tier seams as they do for fslr_cluster_path_segments; a slot's tier
 *   comes from n_cov. */
int  fslr_cluster_collapsed_segments(fslr_ctx *ctx, const int32_t *iv_qkey, const int32_t *iv_qend, int64_t n_intervals, int64_t *n_tokens);
int  fslr_cluster_collapsed_segments_any(fslr_ctx *ctx, const int32_t *iv_qkey, const int32_t *iv_qend, int64_t n_intervals, int64_t *n_tokens);
int  fslr_get_cluster_collapsed_segments(fslr_ctx *ctx, int32_t *n_cov, int32_t *n_link, int32_t *start, int32_t *end, int32_t *gap, int64_t token_capacity);
int  fslr_cluster_collapsed_segments_timings(fslr_ctx *ctx, float *ms);

/* Match reads that are NOT in the uploaded set against the resident index: for a query read Q, given
 * like a row of fslr_reads (its intervals in the order its loop walks them, dense chromosome ids of the
 * uploaded CSR, folded iv_thr, its qlen2 and n_alignments), what the reference's pair loop
 * (cluster.py:197-222) does with query_key = Q and list1 = Q's intervals.
 *   Candidates  for each interval of Q in order, the hits of fslr_search's contract (its hit rule and
 *               its order) on the built index; the candidates of Q are the distinct resident reads of
 *               those hits in the order the loop first meets them (the seen-set of :205-208, kept per
 *               query read).  exclude[q] (a resident rank, or -1) is skipped entirely, as
 *               `o_data.qname == query_key` (:203) is: it lets a caller ask about a resident read.  A
 *               query read of 0 intervals has no candidates; an interval whose chromosome id lies
 *               outside [0, n_chroms) has no hits.
 *   Per candidate P   flags, I and U are exactly fslr_score_pairs' for the ordered pair (list1 = Q,
 *               list2 = P): the gate from Q's and P's qlen2 and n_alignments, first-fit under Q's and
 *               P's thresholds (the resident ones are those currently set), EDGE from pass_table,
 *               ZD_OVERLAP gives I = U = 0.  ZeroDivisionError is only flagged, never returned.
 *   Rows        (partner rank, I, U, flags) for a candidate iff emit_mask == 0 (every candidate) or
 *               flags & emit_mask != 0, in candidate (first-visit) order per query read.  The first-fit
 *               of a candidate that cannot be emitted is skipped.  The same bytes on every run.
 *   Per query read, whatever emit_mask: counts[3 q ..] = candidates, candidates with GATE, candidates
 *               with EDGE; best[q] = the EDGE candidate with the largest I / U (compared exactly,
 *               I1 U2 against I2 U1; ties to the earlier candidate), -1 without an edge.
 * fslr_match_reads: row_off (NULL, or [n_reads + 1]) gets the exclusive prefix of the row counts,
 * *n_rows (may be NULL) their total; counts and best may be NULL.  fslr_match_rows then writes the last
 * fslr_match_reads' rows, query read after query read.  capacity < n_rows: FSLR_ERR_INVALID, nothing is
 * written.  n_reads == 0 is valid.  The saved batch belongs to the reads and the index build it was made
 * on: after another fslr_set_reads* or fslr_build_index, fslr_match_rows returns FSLR_ERR_STATE until the
 * next fslr_match_reads.
 * FSLR_ERR_STATE where fslr_search gives it: no index built, a chromosome or position filter active, or
 * n_shards > 1.  FSLR_ERR_INVALID: the context holds virtual reads (as fslr_score_pairs), a query read of
 * more than FSLR_MAX_L intervals, read_off not non-decreasing, or an exclude value that is neither -1 nor
 * a resident rank (the message names the first offender; nothing is computed).  From params the call
 * uses qlen_cut, nal_cut and pass_table.  Host pointers; syncs.  The query state (edges, labels, degrees,
 * the cap), the saved search batch, the score scratch, the coverage set and the cluster table are left
 * alone.  The query reads go up in bounded blocks and are evaluated in chunks of a bounded number of
 * hits (at least one read: a read's hits are staged whole): no scratch grows with the batch.
 * FSLR_MATCH_SET: the distinct partners of one query read held in on-chip memory; a read with more is
 * still exact (its later hits are deduplicated against the staged hit list) but slower.
 * Out of scope: the edge cap (:223-224; a matched read's loop is not part of the resident graph's cap
 * replay, so every candidate is evaluated) and matching through the multi-GPU split.  Matched reads join
 * the resident set through fslr_append_reads (below).  Query or resident reads of more than FSLR_MAX_L intervals: fslr_match_reads_any.
 * fslr_match_timings (fslr_set_profiling 1 or 2): HIP-event times (ms) of the last fslr_match_reads,
 * ms[0..3] = upload, search (count + fill), dedupe + score (+ row compaction), download, summed over its
 * blocks and chunks. */
#define FSLR_MATCH_SET 256
typedef struct {
    int64_t n_reads, n_intervals;
    const int32_t *read_off;       /* [n_reads+1] */
    const int32_t *read_qlen2;     /* [n_reads] */
    const int32_t *read_nal;       /* [n_reads] */
    const int32_t *iv_chrom;       /* [n_intervals] dense ids of the uploaded CSR */
    const int32_t *iv_start;
    const int32_t *iv_end;
    const int32_t *iv_thr;         /* folded overlap threshold, as fslr_reads */
    const int32_t *exclude;        /* NULL, or [n_reads]: a resident rank to skip, or -1 */
} fslr_match_queries;
int  fslr_match_reads(fslr_ctx *ctx, const fslr_params *params, const fslr_match_queries *queries, uint32_t emit_mask,
                      int64_t *row_off, int32_t *counts, int32_t *best, int64_t *n_rows);
int  fslr_match_rows(fslr_ctx *ctx, int32_t *partner, int32_t *I, int32_t *U, uint8_t *flags, int64_t capacity);
int  fslr_match_timings(fslr_ctx *ctx, float *ms);

/* Pair scoring and read matching for reads of any length (1..FSLR_MAX_ANY_L intervals, the limit
 * fslr_set_reads_any enforces).  fslr_score_pairs_any, fslr_match_reads_any and
 * fslr_match_rows_any keep the contracts of fslr_score_pairs, fslr_match_reads and fslr_match_rows (the
 * first-fit orientation list1 = a or the query read, the flags, ZD_OVERLAP giving I = U = 0, results at
 * input positions, candidate first-visit order, exclude, emit_mask with its skipped first-fits, counts,
 * best compared exactly with ties to the earlier candidate, the same bytes on every run, the state that is
 * left alone, the bounded scratch, the chunking and FSLR_MATCH_BUDGET, the state errors) with four
 * differences:
 *   Rank space  a, b, exclude and partner are REAL read ranks in [0, n_real): the reads as the caller of
 *               fslr_set_reads_any (or fslr_set_long_reads) numbered them; without virtual reads, every
 *               uploaded read.  A resident read's list is its whole real list.  In matching a hit's
 *               partner is the real read of the chunk it lies in, so the chunks of one long read, hit by
 *               one or several query intervals, are one candidate, standing where its first hit stands;
 *               the seen-set, exclude and FSLR_MATCH_SET count real reads.  A rank >= n_real (a virtual
 *               chunk's rank) is FSLR_ERR_INVALID, named like any other bad rank; nothing is written.
 *   Lengths     both lists may hold 1..FSLR_MAX_ANY_L intervals; a longer query read is FSLR_ERR_INVALID
 *               (the message names it).  I (<= 4096) and U (<= 8191) are returned unclamped.
 *   Cutoff      where I <= FSLR_MAX_L and U <= 2*FSLR_MAX_L, EDGE comes from pass_table as in the old
 *               calls; elsewhere EDGE is GATE and I > 0 and U <= umax[I-1] (umax[i] = the largest passing
 *               U for I = i + 1, i when none passes: the table fslr_set_long_cutoffs takes; make it for
 *               max_i >= the longest list of either side, so that it reaches every U).  umax is a host
 *               pointer, uploaded per call; the table of fslr_set_long_cutoffs is not touched.  It is
 *               required when the context holds virtual reads or (matching) a query read has more than
 *               FSLR_MAX_L intervals: non-NULL with n_umax >= the longest resident real read (I never
 *               exceeds it); otherwise FSLR_ERR_INVALID before anything runs.  When neither holds it may
 *               be NULL and is not looked at.
 *   Tie ranks   (matching) where the reads came without iv_data_pos, a tied hit's data position is its
 *               index in the real CSR, also under virtual reads.
 * On a context without virtual reads and (matching) a batch without a query read of more than FSLR_MAX_L
 * intervals, the _any calls run the very drivers and kernels of the old calls and return the same bytes.
 * The saved batch of fslr_match_reads_any is read by fslr_match_rows_any alone and that of fslr_match_reads
 * by fslr_match_rows alone (FSLR_ERR_STATE otherwise); either call replaces the other's batch.
 * fslr_score_timings and fslr_match_timings report the last call of either kind. */
#define FSLR_MAX_ANY_L 4096          /* max intervals per read of the _any calls and fslr_set_reads_any */
int  fslr_score_pairs_any(fslr_ctx *ctx, const fslr_params *params, const int32_t *umax, int32_t n_umax,
                          int64_t n_pairs, const int32_t *a, const int32_t *b, int32_t *I, int32_t *U, uint8_t *flags);
int  fslr_match_reads_any(fslr_ctx *ctx, const fslr_params *params, const int32_t *umax, int32_t n_umax,
                          const fslr_match_queries *queries, uint32_t emit_mask, int64_t *row_off, int32_t *counts,
                          int32_t *best, int64_t *n_rows);
int  fslr_match_rows_any(fslr_ctx *ctx, int32_t *partner, int32_t *I, int32_t *U, uint8_t *flags, int64_t capacity);

/* The first-fit matching of scored pairs: fslr_score_pairs' batch, and per pair WHICH
 * interval of list1 took which interval of list2 in overall_jaccard_similarity's walk (cluster.py:152-161).
 * a, b, I, U and flags are fslr_score_pairs' (fslr_pair_matching) or fslr_score_pairs_any's
 * (fslr_pair_matching_any: real ranks, lists of 1..FSLR_MAX_ANY_L intervals, umax), byte for byte what those
 * calls return for the same batch.
 *   row_off  [n_pairs + 1] the exclusive scan of I: pair k's rows are row_off[k] .. row_off[k + 1]
 *   row, col [capacity] per row (i, j): interval i of list1 took interval j of list2; i is strictly ascending
 *            within a pair and indexes the whole list1, j the whole list2.  A pair has exactly I[k] rows,
 *            whether or not the gate passes; a pair flagged FSLR_SCORE_ZD_OVERLAP has none.
 *   n_rows   the total row count (row_off[n_pairs])
 * capacity >= the sum of min(L1, L2) over the batch can never be short.  When *n_rows > capacity the call
 * returns FSLR_ERR_INVALID (the message names the count): I, U, flags, row_off and *n_rows are complete, row
 * and col unspecified.  row == col == NULL with capacity == 0 is a count-only call and returns FSLR_OK.
 * Errors are fslr_score_pairs' (fslr_score_pairs_any's): no reads set, a rank out of range named by
 * position with nothing written, virtual reads on the plain call, the umax rules of the _any call.  On a
 * context without virtual reads the _any call runs the plain call's driver and kernels.  The query state,
 * the saved search and match batches, the score scratch and every error word are left alone.  The bytes are
 * the same on every run (no atomic decides a position).  Scratch is bounded: a large batch goes in chunks of
 * pairs (FSLR_SCORE_CHUNK as in fslr_score_pairs) and a chunk's rows are emitted in sub-ranges that fit the
 * row scratch, each landing in row / col at the running offset.  Host pointers; syncs.
 * fslr_pair_matching_timings (fslr_set_profiling 1 or 2): ms[0..2] = upload, kernels (count, scan, emit),
 * download of the last call of either kind, summed over its chunks. */
int  fslr_pair_matching(fslr_ctx *ctx, const fslr_params *params, int64_t n_pairs, const int32_t *a, const int32_t *b,
                        int32_t *I, int32_t *U, uint8_t *flags, int64_t *row_off, int32_t *row, int32_t *col,
                        int64_t capacity, int64_t *n_rows);
int  fslr_pair_matching_any(fslr_ctx *ctx, const fslr_params *params, const int32_t *umax, int32_t n_umax,
                            int64_t n_pairs, const int32_t *a, const int32_t *b, int32_t *I, int32_t *U,
                            uint8_t *flags, int64_t *row_off, int32_t *row, int32_t *col, int64_t capacity,
                            int64_t *n_rows);
int  fslr_pair_matching_timings(fslr_ctx *ctx, float *ms);

/* Append reads to the resident set on the device: what a caller otherwise does by
 * fslr_set_reads of the union.  `reads` describes m new reads with mi intervals exactly as fslr_set_reads
 * takes them: iv_chrom in the resident dense ids, n_chroms >= the resident n_chroms (a larger value adds
 * chromosomes at the end), folded iv_thr, and iv_data_pos REQUIRED: the position of each new interval in the
 * batch's own start-sorted list (a permutation of [0, mi) with non-decreasing starts).
 * After a successful call the context holds n + m reads: the resident reads keep ranks 0 .. n-1 and their CSR
 * rows, new read r has rank n + r and its intervals follow at CSR offset ni + read_off[r].  The `data` list is
 * the stable merge of the two start-sorted lists, the resident element first on equal starts: a resident
 * interval at data position d with start s moves to d + #{new intervals with start < s}, a new interval at
 * its own position e with start t lands at e + #{resident intervals with start <= t}.  Every resident buffer
 * and host-side count then equals, byte for byte, what fslr_set_reads gives for the concatenated CSR with
 * that merged iv_data_pos; the same bytes on every run.  As after fslr_set_reads: no index is built
 * (fslr_build_index next), the saved search, match and score batches, the position plan and the query-reuse
 * state belong to the old reads.  Thresholds are the resident ones currently set plus the batch's.
 * Cost: H2D of the m-sized columns only, no D2H of resident columns and no host pass over resident reads;
 * device buffers that must grow keep their contents.  Syncs.
 * Atomic: the whole batch is validated before any resident buffer is written.  The first failure is reported
 * as fslr_set_reads reports it (FSLR_ERR_INVALID, the same messages; also n + m >= FSLR_MAX_READS, ni + mi >=
 * 2^31 - 1, a NULL iv_data_pos, n_chroms below the resident value) and leaves the context as it was: the same
 * reads, the index still built if it was, the saved batches readable.  m == 0 is valid and changes nothing.
 * Memory is part of that: every buffer that has to grow and the merge output are allocated before anything
 * is freed or written, so FSLR_ERR_NOMEM leaves the context as it was too.  Only a device failure after that
 * point (FSLR_ERR_HIP from a copy or a launch) leaves no reads set.
 * Memory: from the first append on the context keeps a second set of data-order buffers (28 B per interval
 * of capacity, the merge writes into it and the sets swap) and the batch scratch (about 85 B per interval
 * of the largest batch) until fslr_ctx_destroy; growth allocates the new buffers beside the old ones, so
 * its peak is both.
 * FSLR_ERR_STATE, named in the message: no reads set; reads set without iv_data_pos; reads made from rows
 * (fslr_set_reads_rows); virtual reads (fslr_set_reads_any with a long read, fslr_set_long_reads); n_shards >
 * 1; a chromosome or position filter active.  A new read of more than FSLR_MAX_L intervals is
 * FSLR_ERR_INVALID.  Multi-GPU contexts do not append.
 * FSLR_APPEND_TILE: outputs per tile of the merge kernel (a block finds each tile's split by binary search).
 * fslr_append_timings (fslr_set_profiling 1 or 2): HIP-event times (ms) of the last fslr_append_reads,
 * ms[0..3] = upload, validate + pack, merge (row copies, merge, data positions), first to last event. */
#define FSLR_APPEND_TILE 1024
int  fslr_append_reads(fslr_ctx *ctx, const fslr_reads *reads);
int  fslr_append_timings(fslr_ctx *ctx, float *ms);

/* ---- Removing reads from a resident set --------------------------------------------------------------
 * fslr_remove_reads drops whole reads from the resident set on the device, where until now the only route was
 * fslr_set_reads of the survivors.  keep[r] != 0 means resident read r stays; n must equal the resident read
 * count.  new_rank (NULL or int32[n]) receives the old rank -> new rank map, -1 for a removed read.
 * After a successful call the context holds the kept reads with the gaps closed: a survivor's new rank is the
 * number of kept reads of lower rank, its intervals keep their order at CSR offset = the sum of the kept lower
 * reads' lengths, and a kept interval at data position d moves to #{kept elements before d}.  n_chroms and
 * the dense chromosome ids stay (a chromosome may be left without intervals).  Every resident buffer and
 * host-side count then equals, byte for byte, what fslr_set_reads gives for that compacted CSR with the
 * survivors' thresholds as currently set; the same bytes on every run.  The threshold mode and the
 * aln_size == 0 mark are those of the survivors, not carried over: removing the only reads that held a general
 * threshold or an aln_size == 0 interval lets FSLR_ENGINE_AUTO pick the sweep again.  As after fslr_set_reads
 * and fslr_append_reads: no index is built (fslr_build_index next), the saved search, match and score batches,
 * the position plan and the query-reuse state belong to the old reads; the coverage set and the cluster table
 * are left as fslr_append_reads leaves them.
 * Cost: H2D of the n keep bytes; D2H of n_chroms counts, a few status words and, on request, new_rank (and the
 * n read lengths, one byte each, when the context holds an aln_size == 0 interval: the host's marks of those
 * are compacted by them).  No resident column crosses the link and there is no host pass over resident
 * intervals otherwise.  Syncs.
 * Atomic: everything is validated and everything is allocated before any resident buffer is written.
 * FSLR_ERR_INVALID: n differs from the resident count, keep is NULL, nothing would be kept.  FSLR_ERR_STATE,
 * named in the message: no reads set; reads set without iv_data_pos; reads made from rows; virtual reads;
 * n_shards > 1; a chromosome or position filter active.  FSLR_ERR_NOMEM.  All of these leave the context as it
 * was: the same reads, the index still built if it was, the saved batches readable.  Only a device failure
 * after that point (FSLR_ERR_HIP) leaves no reads set.  Keeping every read is valid, changes nothing (no
 * generation moves) and returns the identity map.
 * Memory: the data order is compacted into the second set of data-order buffers fslr_append_reads keeps (28 B
 * per interval of capacity, allocated by whichever call comes first) and the sets swap; the CSR order is
 * compacted into index-build scratch of the same size, which is swapped with the resident buffers (the index
 * is rebuilt anyway); the maps take 10 B per read.  Buffers never shrink.
 * FSLR_REMOVE_TILE: data positions per tile of the data-order compaction.
 * fslr_remove_timings (fslr_set_profiling 1 or 2): HIP-event times (ms) of the last fslr_remove_reads that
 * removed something, ms[0..3] = upload, maps (flags, tile counts, scans, read maps), compaction (data order
 * and CSR order), first to last event. */
#define FSLR_REMOVE_TILE 1024
int  fslr_remove_reads(fslr_ctx *ctx, int64_t n, const uint8_t *keep, int32_t *new_rank);
int  fslr_remove_timings(fslr_ctx *ctx, float *ms);

/* ---- Appending and removing reads of any length -------------------------------------
 * fslr_append_reads_any and fslr_remove_reads_any are fslr_append_reads and fslr_remove_reads for reads of
 * 1..FSLR_MAX_ANY_L intervals and for a context that holds virtual reads made by fslr_set_reads_any.
 *
 * fslr_append_reads_any: `reads` is a REAL CSR (a read's whole list, not chunks) in the resident dense
 * chromosome ids, thresholds folded and in real interval order, iv_data_pos REQUIRED (the batch's own
 * start-sorted order), exactly as fslr_append_reads takes it.  Afterwards the context is the one
 * fslr_set_reads_any of the union leaves (the resident real reads in their rank order, then the batch), byte
 * for byte on every resident buffer fslr_append_reads names and on the virtual-read maps (vreal, vbase, rlen,
 * off2 of the long reads, n_real, the longest read, the host's virtual -> real interval map).  With n resident
 * real reads, V resident virtual reads and m batch reads: resident virtual reads v < n keep their rank, the
 * batch's first chunks take [n, n + m), resident further chunks v >= n become v + m, the batch's further chunks
 * follow; the CSR rows follow the same four groups in that order, and the `data` list is fslr_append_reads'
 * stable merge with the tags in the new numbering.  A context without virtual reads plus a batch without a
 * read of more than FSLR_MAX_L intervals takes fslr_append_reads' path and leaves its bytes; with such a read
 * the context becomes a virtual one.  The long-pair cutoff table is left alone: fslr_set_long_cutoffs must
 * cover the longest read again before the next fslr_long_query / fslr_long_pairs, which otherwise refuse
 * ("umax must cover I up to the longest read"; a context that just became virtual holds the zero placeholder
 * of a fresh upload).
 * Cost: H2D of the batch's columns and maps only; the split into chunks is a host pass over the batch; the
 * relocation of the resident rows, reads and maps runs on the device (never in place: into index-build
 * scratch and freshly allocated maps, swapped in).  The host's per-interval marks and its virtual -> real
 * interval map (4 B + 1 B per interval) are rewritten by one host pass.  The first _any call after an upload
 * reads the real reads' lengths back once (4 B per real read; 1 B on a plain context).
 *
 * fslr_remove_reads_any: keep and new_rank are over the REAL ranks, n must equal the real read count.  A
 * removed read loses all its chunks.  Afterwards the context is fslr_set_reads_any of the surviving real CSR,
 * byte for byte; once no read of more than FSLR_MAX_L intervals survives it is a plain context (the bytes of
 * fslr_set_reads, the threshold mode and the aln_size == 0 mark recomputed as fslr_remove_reads does).  On a
 * context without virtual reads it is fslr_remove_reads.
 *
 * Both: atomic as the short calls are (a refused or out-of-memory call leaves the reads, a built index and the
 * saved batches untouched; nothing resident is written before validation has passed and everything is
 * allocated; a device failure past that point leaves no reads set); the same invalidations; the same
 * FSLR_ERR_STATE list without the virtual-reads line (no reads set, rows-made reads, no iv_data_pos, n_shards
 * > 1, an active filter), plus: virtual reads a caller made with fslr_set_long_reads (their real CSR is not
 * known to the library) are FSLR_ERR_STATE, and a batch read of more than FSLR_MAX_ANY_L intervals is
 * FSLR_ERR_INVALID, named.  fslr_append_timings / fslr_remove_timings report the last call of either kind
 * (the relocation counts into the append's merge phase, the removal's map kernels into its compaction phase). */
int  fslr_append_reads_any(fslr_ctx *ctx, const fslr_reads *reads);
int  fslr_remove_reads_any(fslr_ctx *ctx, int64_t n_real, const uint8_t *keep, int32_t *new_rank);

/* Device-side views for collectives (e.g. RCCL all_gather of labels). */
int  fslr_labels_device_ptr(fslr_ctx *ctx, void **dptr);
/* Copy the [n_reads] labels into a caller-owned device buffer on this device (async, ctx stream). */
int  fslr_copy_labels_device(fslr_ctx *ctx, int32_t *dst);
/* Copy the [n_reads] forward degrees into a caller-owned device buffer (async, ctx stream). */
int  fslr_copy_fwd_device(fslr_ctx *ctx, int32_t *dst);
/* Union (src[k], dst[k]) into the context's forest; pointers are device pointers
 * on this context's device when on_device != 0, else host.  src == NULL means
 * src[k] = k mod n_reads, so W concatenated label vectors merge in one call
 * (FSLR_ERR_INVALID on a context without reads).  There is no padding: every
 * end must lie in [0, n_reads).  Follow with fslr_finalize_labels.  Async. */
int  fslr_union_pairs(fslr_ctx *ctx, const int32_t *src, const int32_t *dst, int64_t n, int on_device);
int  fslr_finalize_labels(fslr_ctx *ctx);
/* Copy this context's edges as int32 (a, b) pairs into a caller-owned device buffer of n_pad pairs,
 * padded with (-1, -1); the edge count is read on the device, so n_pad only has to be at least it
 * (the multi-GPU merge pads every rank to the largest count).  Async, ctx stream. */
int  fslr_copy_edges_device(fslr_ctx *ctx, int32_t *dst, int64_t n_pad);
/* Labels = connected components (min-rank roots) of the n int32 (a, b) device pairs at `pairs`
 * (a pair with a < 0 or b < 0 is padding and is skipped, by the pre-hook and by the union alike; every
 * other end must lie in [0, n_reads)): the union of W ranks' gathered edge lists.  Async. */
int  fslr_components_from_pairs(fslr_ctx *ctx, const int32_t *pairs, int64_t n);

#ifdef __cplusplus
}
#endif
#endif /* FSLR_HIP_H */
