"""ctypes binding of ``libfslr_hip.so`` (C ABI: include/fslr_hip.h).

The HIP library is the only compute path: there is no CPU fallback.  If the
shared object is missing or no HIP device is present, every entry point raises
``HipUnavailable`` — loudly, never silently.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

LIB_PATH = os.environ.get('FSLR_LIB') or os.path.join(os.path.dirname(os.path.abspath(__file__)), 'libfslr_hip.so')

ABI_VERSION = 21         # include/fslr_hip.h FSLR_ABI_VERSION this binding is written against
FSLR_OK, FSLR_ERR_ZERO_DIVISION, FSLR_ERR_INVALID, FSLR_ERR_HIP, FSLR_ERR_NOMEM, FSLR_ERR_STATE = range(6)
FSLR_MAX_L = 64
FSLR_MAX_READS = 1 << 25
FSLR_THR_ZERO_ALN = -(1 << 31)
PASS_STRIDE = 2 * FSLR_MAX_L
# pair engines (fslr_params.flags & 3, include/fslr_hip.h)
ENGINES = {'auto': 0, 'walk': 1, 'sweep': 2}
ENGINE_NAMES = {1: 'walk', 2: 'sweep'}

# every symbol include/fslr_hip.h declares (checked by tests/test_abi.py)
EXPORTED = ['fslr_abi_version', 'fslr_last_error', 'fslr_ctx_create', 'fslr_ctx_destroy', 'fslr_set_profiling',
            'fslr_set_reads', 'fslr_set_thresholds', 'fslr_reserve_edges', 'fslr_reserve_deferred',
            'fslr_set_shard', 'fslr_build_index', 'fslr_query', 'fslr_query_shard',
            'fslr_components', 'fslr_run', 'fslr_sync', 'fslr_read_stats', 'fslr_get_timings', 'fslr_read_counters',
            'fslr_get_labels',
            'fslr_get_fwd_degree', 'fslr_get_edges', 'fslr_labels_device_ptr', 'fslr_copy_labels_device',
            'fslr_copy_fwd_device', 'fslr_union_pairs', 'fslr_finalize_labels', 'fslr_apply_edge_cap',
            'fslr_get_pair_kernel_times', 'fslr_set_chrom_filter', 'fslr_sweep_partition', 'fslr_sweep_evaluate',
            'fslr_sweep_partition_repeat',
            'fslr_copy_edges_device', 'fslr_components_from_pairs', 'fslr_set_long_reads', 'fslr_long_query',
            'fslr_get_long_edges', 'fslr_copy_edges_iu_device', 'fslr_cap_install_edges', 'fslr_cap_local',
            'fslr_cap_copy_local', 'fslr_cap_replay', 'fslr_get_stage_kernel_times', 'fslr_long_pairs',
            'fslr_cap_replay_pairs', 'fslr_source_hash', 'fslr_set_reads_any', 'fslr_set_long_cutoffs',
            'fslr_cap_install_pairs', 'fslr_cap_sizes', 'fslr_cap_dep_local', 'fslr_cap_shard_plan',
            'fslr_cap_shard_pack', 'fslr_cap_replay_shard', 'fslr_cap_copy_changes', 'fslr_cap_apply_changes',
            'fslr_local_forest', 'fslr_copy_forest_pairs', 'fslr_sort_edges', 'fslr_cap_bwd_counts',
            'fslr_cap_restrict', 'fslr_cap_copy_restricted', 'fslr_cap_install_restricted', 'fslr_rows_upload',
            'fslr_set_reads_rows', 'fslr_get_read_codes', 'fslr_get_csr', 'fslr_fold_thresholds',
            'fslr_position_costs', 'fslr_position_entries', 'fslr_set_position_filter', 'fslr_use_position_filter', 'fslr_long_pairs_shard',
            'fslr_edge_cap_deferred', 'fslr_edge_cap_deferred_read', 'fslr_set_query_reuse',
            'fslr_search', 'fslr_search_hits', 'fslr_search_timings', 'fslr_score_pairs', 'fslr_score_timings',
            'fslr_coverage_build', 'fslr_coverage_at', 'fslr_coverage_timings',
            'fslr_cluster_table', 'fslr_get_cluster_ids', 'fslr_get_cluster_members', 'fslr_assign_clusters',
            'fslr_choose_representatives', 'fslr_cluster_timings',
            'fslr_match_reads', 'fslr_match_rows', 'fslr_match_timings', 'fslr_score_pairs_any',
            'fslr_match_reads_any', 'fslr_match_rows_any', 'fslr_append_reads', 'fslr_append_timings',
            'fslr_remove_reads', 'fslr_remove_timings', 'fslr_append_reads_any', 'fslr_remove_reads_any',
            'fslr_pair_matching', 'fslr_pair_matching_any', 'fslr_pair_matching_timings',
            'fslr_cluster_loci', 'fslr_get_cluster_loci', 'fslr_cluster_loci_timings',
            'fslr_cluster_junctions', 'fslr_get_cluster_junctions', 'fslr_cluster_junctions_timings',
            'fslr_cluster_paths', 'fslr_get_cluster_paths', 'fslr_cluster_paths_timings',
            'fslr_cluster_junctions_any', 'fslr_cluster_paths_any',
            'fslr_cluster_path_segments', 'fslr_get_cluster_path_segments', 'fslr_cluster_path_segments_timings',
            'fslr_cluster_path_segments_any',
            'fslr_cluster_path_containment', 'fslr_get_cluster_path_containment', 'fslr_cluster_path_containment_timings',
            'fslr_cluster_collapsed_segments', 'fslr_cluster_collapsed_segments_any',
            'fslr_get_cluster_collapsed_segments', 'fslr_cluster_collapsed_segments_timings']
# fslr_score_pairs' flag bits (include/fslr_hip.h)
SCORE_GATE, SCORE_EDGE, SCORE_ZD_GATE, SCORE_ZD_OVERLAP = 1, 2, 4, 8
# fslr_coverage_*: keys per tile of the sorted arrays, queries per chunk (include/fslr_hip.h)
COVERAGE_TILE = 256
COVERAGE_CHUNK = 1 << 21
# fslr_match_reads: distinct partners of one query read held in on-chip memory (include/fslr_hip.h FSLR_MATCH_SET)
MATCH_SET = 256
# fslr_append_reads: outputs per tile of the merge kernel (include/fslr_hip.h FSLR_APPEND_TILE)
APPEND_TILE = 1024
# fslr_remove_reads: data positions per tile of the data-order compaction (include/fslr_hip.h FSLR_REMOVE_TILE)
REMOVE_TILE = 1024


class HipUnavailable(RuntimeError):
    pass


class FslrError(RuntimeError):
    pass


class Reads(ctypes.Structure):
    _fields_ = [('n_reads', ctypes.c_int64), ('n_intervals', ctypes.c_int64), ('n_chroms', ctypes.c_int32)] + [
        (f, ctypes.c_void_p) for f in ('read_off', 'read_qlen2', 'read_nal', 'iv_chrom', 'iv_start', 'iv_end',
                                       'iv_thr', 'iv_data_pos')]


class Rows(ctypes.Structure):
    _fields_ = [('n_rows', ctypes.c_int64), ('n_codes', ctypes.c_int64), ('n_chrom_ids', ctypes.c_int64)] + [
        (f, ctypes.c_void_p) for f in ('chrom', 'start', 'end', 'aln', 'qcode', 'nal', 'qlen2')]


class RowsInfo(ctypes.Structure):
    _fields_ = [('n_reads', ctypes.c_int64), ('n_intervals', ctypes.c_int64)] + [
        (f, ctypes.c_int32) for f in ('n_chroms', 'max_len', 'nal_varies', 'general_thresholds', 'any_zero_aln',
                                      'pad')]

    def as_dict(self):
        return {f: int(getattr(self, f)) for f, _ in self._fields_ if f != 'pad'}


class MatchQueries(ctypes.Structure):
    _fields_ = [('n_reads', ctypes.c_int64), ('n_intervals', ctypes.c_int64)] + [
        (f, ctypes.c_void_p) for f in ('read_off', 'read_qlen2', 'read_nal', 'iv_chrom', 'iv_start', 'iv_end',
                                       'iv_thr', 'exclude')]


class Params(ctypes.Structure):
    _fields_ = [('qlen_cut', ctypes.c_double), ('nal_cut', ctypes.c_double), ('pass_table', ctypes.c_void_p),
                ('edge_threshold', ctypes.c_int32), ('flags', ctypes.c_int32)]


class QueryStats(ctypes.Structure):
    _fields_ = [('evaluated_pairs', ctypes.c_int64), ('jaccard_evals', ctypes.c_int64),
                ('candidates', ctypes.c_int64), ('n_edges', ctypes.c_int64), ('max_fwd', ctypes.c_int32),
                ('error', ctypes.c_int32), ('err_a', ctypes.c_int32), ('err_b', ctypes.c_int32),
                ('algo_bytes', ctypes.c_int64), ('overflow_candidates', ctypes.c_int64),
                ('gather_pairs', ctypes.c_int64), ('match_entries', ctypes.c_int64),
                ('matched_pairs', ctypes.c_int64), ('deferred', ctypes.c_int64),
                ('deferred_capacity', ctypes.c_int64), ('edge_capacity', ctypes.c_int64),
                ('walked_records', ctypes.c_int64), ('engine', ctypes.c_int32), ('overflow_flags', ctypes.c_int32),
                ('pair_tests', ctypes.c_int64), ('entry_capacity', ctypes.c_int64), ('zd_pairs', ctypes.c_int64)]

    def as_dict(self):
        d = {f: getattr(self, f) for f, _ in self._fields_}
        d['engine'] = ENGINE_NAMES.get(d['engine'], d['engine'])
        return d


class CapStats(ctypes.Structure):
    _fields_ = [('applied', ctypes.c_int32), ('max_fwd', ctypes.c_int32)] + [
        (f, ctypes.c_int64) for f in ('candidates', 'capped', 'hits', 'pairs', 'dropped', 'backward')]

    def as_dict(self):
        return {f: int(getattr(self, f)) for f, _ in self._fields_}


class ClusterInfo(ctypes.Structure):
    _fields_ = [(f, ctypes.c_int64) for f in ('n_clusters', 'n_nodes', 'max_size')]

    def as_dict(self):
        return {f: int(getattr(self, f)) for f, _ in self._fields_}


class Timings(ctypes.Structure):
    _fields_ = [('index_ms', ctypes.c_float), ('query_ms', ctypes.c_float), ('components_ms', ctypes.c_float),
                ('total_ms', ctypes.c_float), ('pair_kernel_ms', ctypes.c_float), ('sweep_count_ms', ctypes.c_float),
                ('sweep_emit_ms', ctypes.c_float), ('sweep_sort_ms', ctypes.c_float), ('sweep_pairs_ms', ctypes.c_float)]

    def as_dict(self):
        return {f: float(getattr(self, f)) for f, _ in self._fields_}


_lib = None


def load(path: str = LIB_PATH):
    """Load the shared library (no device access)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise HipUnavailable(f'{path} is not built: run `python -c "import __graft_entry__ as g; g.build()"` '
                             '(or `make -C fslr_amd/csrc`).  There is no CPU fallback.')
    L = ctypes.CDLL(path)
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    sig = {
        'fslr_abi_version': (ctypes.c_int, []),
        'fslr_last_error': (ctypes.c_char_p, [vp]),
        'fslr_ctx_create': (ctypes.c_int, [ctypes.c_int, vp, ctypes.POINTER(vp)]),
        'fslr_ctx_destroy': (None, [vp]),
        'fslr_set_profiling': (ctypes.c_int, [vp, ctypes.c_int]),
        'fslr_set_query_reuse': (ctypes.c_int, [vp, ctypes.c_int]),
        'fslr_set_reads': (ctypes.c_int, [vp, ctypes.POINTER(Reads)]),
        'fslr_set_thresholds': (ctypes.c_int, [vp, vp]),
        'fslr_reserve_edges': (ctypes.c_int, [vp, i64]),
        'fslr_reserve_deferred': (ctypes.c_int, [vp, i64]),
        'fslr_set_shard': (ctypes.c_int, [vp, i32, i32]),
        'fslr_build_index': (ctypes.c_int, [vp]),
        'fslr_query': (ctypes.c_int, [vp, ctypes.POINTER(Params), i64, i64]),
        'fslr_query_shard': (ctypes.c_int, [vp, ctypes.POINTER(Params), i32, i32]),
        'fslr_components': (ctypes.c_int, [vp]),
        'fslr_run': (ctypes.c_int, [vp, ctypes.POINTER(Params)]),
        'fslr_sync': (ctypes.c_int, [vp]),
        'fslr_read_stats': (ctypes.c_int, [vp, ctypes.POINTER(QueryStats)]),
        'fslr_get_timings': (ctypes.c_int, [vp, ctypes.POINTER(Timings)]),
        'fslr_read_counters': (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]),
        'fslr_get_labels': (ctypes.c_int, [vp, vp]),
        'fslr_get_fwd_degree': (ctypes.c_int, [vp, vp]),
        'fslr_get_edges': (ctypes.c_int, [vp, vp, vp, vp, i64]),
        'fslr_labels_device_ptr': (ctypes.c_int, [vp, ctypes.POINTER(vp)]),
        'fslr_copy_labels_device': (ctypes.c_int, [vp, vp]),
        'fslr_copy_fwd_device': (ctypes.c_int, [vp, vp]),
        'fslr_union_pairs': (ctypes.c_int, [vp, vp, vp, i64, ctypes.c_int]),
        'fslr_finalize_labels': (ctypes.c_int, [vp]),
        'fslr_apply_edge_cap': (ctypes.c_int, [vp, i32, ctypes.POINTER(CapStats)]),
        'fslr_get_pair_kernel_times': (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_float), i32]),
        'fslr_get_stage_kernel_times': (ctypes.c_int, [vp, i32, ctypes.POINTER(ctypes.c_float), i32]),
        'fslr_set_chrom_filter': (ctypes.c_int, [vp, vp]),
        'fslr_sweep_partition': (ctypes.c_int, [vp, ctypes.POINTER(Params), i32, i32, vp, i64,
                                                ctypes.POINTER(ctypes.c_int64)]),
        'fslr_sweep_partition_repeat': (ctypes.c_int, [vp, ctypes.POINTER(Params), i32, i32, vp, i64]),
        'fslr_sweep_evaluate': (ctypes.c_int, [vp, ctypes.POINTER(Params), vp, i64]),
        'fslr_copy_edges_device': (ctypes.c_int, [vp, vp, i64]),
        'fslr_components_from_pairs': (ctypes.c_int, [vp, vp, i64]),
        'fslr_set_long_reads': (ctypes.c_int, [vp, i64, vp, vp, vp, vp, i32]),
        'fslr_set_reads_any': (ctypes.c_int, [vp, ctypes.POINTER(Reads)]),
        'fslr_set_long_cutoffs': (ctypes.c_int, [vp, vp, i32]),
        'fslr_long_query': (ctypes.c_int, [vp, ctypes.POINTER(Params), ctypes.POINTER(ctypes.c_int64)]),
        'fslr_get_long_edges': (ctypes.c_int, [vp, vp, vp, vp, vp, i64]),
        'fslr_long_pairs': (ctypes.c_int, [vp, ctypes.POINTER(Params), ctypes.POINTER(ctypes.c_int64)]),
        'fslr_cap_replay_pairs': (ctypes.c_int, [vp, i32, vp, vp, i64, vp, vp, ctypes.POINTER(CapStats)]),
        'fslr_copy_edges_iu_device': (ctypes.c_int, [vp, vp, i64]),
        'fslr_cap_install_edges': (ctypes.c_int, [vp, vp, i64]),
        'fslr_cap_local': (ctypes.c_int, [vp, i32, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]),
        'fslr_cap_copy_local': (ctypes.c_int, [vp, vp, vp]),
        'fslr_cap_replay': (ctypes.c_int, [vp, vp, vp, i64, i32, ctypes.POINTER(CapStats)]),
        'fslr_cap_install_pairs': (ctypes.c_int, [vp, vp, i64, i32, i32]),
        'fslr_local_forest': (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_int64)]),
        'fslr_sort_edges': (ctypes.c_int, [vp]),
        'fslr_copy_forest_pairs': (ctypes.c_int, [vp, vp, i64]),
        'fslr_cap_sizes': (ctypes.c_int, [vp] + [ctypes.POINTER(ctypes.c_int64)] * 3),
        'fslr_cap_dep_local': (ctypes.c_int, [vp, vp]),
        'fslr_cap_shard_plan': (ctypes.c_int, [vp, vp, i32, i32, vp]),
        'fslr_cap_shard_pack': (ctypes.c_int, [vp, vp, vp]),
        'fslr_cap_replay_shard': (ctypes.c_int, [vp, vp, vp, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(CapStats)]),
        'fslr_cap_copy_changes': (ctypes.c_int, [vp, vp, i64]),
        'fslr_cap_apply_changes': (ctypes.c_int, [vp, vp, i64, ctypes.POINTER(CapStats)]),
        'fslr_cap_bwd_counts': (ctypes.c_int, [vp, i32, vp, i32]),
        'fslr_cap_restrict': (ctypes.c_int, [vp, vp, i32, ctypes.POINTER(ctypes.c_int64)]),
        'fslr_cap_copy_restricted': (ctypes.c_int, [vp, vp, i64]),
        'fslr_cap_install_restricted': (ctypes.c_int, [vp, vp, i64, i32, i32]),
        'fslr_rows_upload': (ctypes.c_int, [vp, ctypes.POINTER(Rows)]),
        'fslr_set_reads_rows': (ctypes.c_int, [vp, vp, vp, ctypes.c_double, ctypes.POINTER(RowsInfo)]),
        'fslr_get_read_codes': (ctypes.c_int, [vp, vp]),
        'fslr_get_csr': (ctypes.c_int, [vp] + [vp] * 10),
        'fslr_fold_thresholds': (ctypes.c_int, [vp, ctypes.c_double]),
        'fslr_position_costs': (ctypes.c_int, [vp, vp, vp, i64]),
        'fslr_position_entries': (ctypes.c_int, [vp, vp, vp, i64]),
        'fslr_set_position_filter': (ctypes.c_int, [vp, i64, i64, i64]),
        'fslr_use_position_filter': (ctypes.c_int, [vp]),
        'fslr_long_pairs_shard': (ctypes.c_int, [vp, ctypes.POINTER(Params), i32, i32, ctypes.POINTER(ctypes.c_int64)]),
        'fslr_edge_cap_deferred': (ctypes.c_int, [vp, i32]),
        'fslr_edge_cap_deferred_read': (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_int32)]),
        'fslr_search': (ctypes.c_int, [vp, i64, vp, vp, vp, vp, ctypes.POINTER(ctypes.c_int64)]),
        'fslr_search_hits': (ctypes.c_int, [vp, vp, i64]),
        'fslr_search_timings': (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_float)]),
        'fslr_score_pairs': (ctypes.c_int, [vp, ctypes.POINTER(Params), i64, vp, vp, vp, vp, vp]),
        'fslr_score_timings': (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_float)]),
        'fslr_score_pairs_any': (ctypes.c_int, [vp, ctypes.POINTER(Params), vp, i32, i64, vp, vp, vp, vp, vp]),
        'fslr_pair_matching': (ctypes.c_int, [vp, ctypes.POINTER(Params), i64, vp, vp, vp, vp, vp, vp, vp, vp, i64,
                                              ctypes.POINTER(ctypes.c_int64)]),
        'fslr_pair_matching_any': (ctypes.c_int, [vp, ctypes.POINTER(Params), vp, i32, i64, vp, vp, vp, vp, vp, vp, vp,
                                                  vp, i64, ctypes.POINTER(ctypes.c_int64)]),
        'fslr_pair_matching_timings': (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_float)]),
        'fslr_match_reads': (ctypes.c_int, [vp, ctypes.POINTER(Params), ctypes.POINTER(MatchQueries), ctypes.c_uint32,
                                            vp, vp, vp, ctypes.POINTER(ctypes.c_int64)]),
        'fslr_match_rows': (ctypes.c_int, [vp, vp, vp, vp, vp, i64]),
        'fslr_match_reads_any': (ctypes.c_int, [vp, ctypes.POINTER(Params), vp, i32, ctypes.POINTER(MatchQueries),
                                                ctypes.c_uint32, vp, vp, vp, ctypes.POINTER(ctypes.c_int64)]),
        'fslr_match_rows_any': (ctypes.c_int, [vp, vp, vp, vp, vp, i64]),
        'fslr_match_timings': (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_float)]),
        'fslr_append_reads': (ctypes.c_int, [vp, ctypes.POINTER(Reads)]),
        'fslr_append_timings': (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_float)]),
        'fslr_remove_reads': (ctypes.c_int, [vp, i64, vp, vp]),
        'fslr_remove_timings': (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_float)]),
        'fslr_append_reads_any': (ctypes.c_int, [vp, ctypes.POINTER(Reads)]),
        'fslr_remove_reads_any': (ctypes.c_int, [vp, i64, vp, vp]),
        'fslr_coverage_build': (ctypes.c_int, [vp, i64, i32, vp, vp, vp]),
        'fslr_coverage_at': (ctypes.c_int, [vp, i64, vp, vp, vp]),
        'fslr_coverage_timings': (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_float)]),
        'fslr_cluster_table': (ctypes.c_int, [vp, vp, i64, ctypes.POINTER(ClusterInfo)]),
        'fslr_get_cluster_ids': (ctypes.c_int, [vp, vp, vp]),
        'fslr_get_cluster_members': (ctypes.c_int, [vp, vp, vp]),
        'fslr_assign_clusters': (ctypes.c_int, [vp, i64, vp, vp, vp, vp, ctypes.POINTER(ctypes.c_int64)]),
        'fslr_choose_representatives': (ctypes.c_int, [vp, i64, vp, vp, vp, vp, i64, vp, vp]),
        'fslr_cluster_timings': (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_float)]),
        'fslr_cluster_loci': (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_int64)]),
        'fslr_get_cluster_loci': (ctypes.c_int, [vp, vp, vp, vp, vp, vp, vp, i64]),
        'fslr_cluster_loci_timings': (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_float)]),
        'fslr_cluster_junctions': (ctypes.c_int, [vp, vp, vp, i64, ctypes.POINTER(ctypes.c_int64)]),
        'fslr_get_cluster_junctions': (ctypes.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, i64]),
        'fslr_cluster_junctions_timings': (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_float)]),
        'fslr_cluster_paths': (ctypes.c_int, [vp, vp, vp, i64, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]),
        'fslr_get_cluster_paths': (ctypes.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i64]),
        'fslr_cluster_paths_timings': (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_float)]),
        'fslr_cluster_junctions_any': (ctypes.c_int, [vp, vp, vp, i64, ctypes.POINTER(ctypes.c_int64)]),
        'fslr_cluster_paths_any': (ctypes.c_int, [vp, vp, vp, i64, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]),
        'fslr_cluster_path_segments': (ctypes.c_int, [vp, vp, vp, i64, ctypes.POINTER(ctypes.c_int64)]),
        'fslr_cluster_path_segments_any': (ctypes.c_int, [vp, vp, vp, i64, ctypes.POINTER(ctypes.c_int64)]),
        'fslr_get_cluster_path_segments': (ctypes.c_int, [vp, vp, vp, vp, i64]),
        'fslr_cluster_path_segments_timings': (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_float)]),
        'fslr_cluster_path_containment': (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_int64)]),
        'fslr_get_cluster_path_containment': (ctypes.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i64]),
        'fslr_cluster_path_containment_timings': (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_float)]),
        'fslr_cluster_collapsed_segments': (ctypes.c_int, [vp, vp, vp, i64, ctypes.POINTER(ctypes.c_int64)]),
        'fslr_cluster_collapsed_segments_any': (ctypes.c_int, [vp, vp, vp, i64, ctypes.POINTER(ctypes.c_int64)]),
        'fslr_get_cluster_collapsed_segments': (ctypes.c_int, [vp, vp, vp, vp, vp, vp, i64]),
        'fslr_cluster_collapsed_segments_timings': (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_float)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    if L.fslr_abi_version() != ABI_VERSION:
        raise HipUnavailable(f'{path} has ABI {L.fslr_abi_version()}, this binding needs {ABI_VERSION}: rebuild it')
    want = source_hash()
    if want is not None and os.environ.get('FSLR_ALLOW_STALE') != '1':
        if not hasattr(L, 'fslr_source_hash'):
            raise HipUnavailable(f'{path} carries no source hash (fslr_source_hash): rebuild it (make -C fslr_amd/csrc), '
                                 f'or set FSLR_ALLOW_STALE=1 to load it anyway')
        L.fslr_source_hash.restype = ctypes.c_char_p
        L.fslr_source_hash.argtypes = []
        got = L.fslr_source_hash().decode()
        if got != want:
            raise HipUnavailable(f'{path} was built from other sources (hash {got}, the sources beside it hash to '
                                 f'{want}): rebuild it (make -C fslr_amd/csrc)')
    _lib = L
    return L


def source_hash():
    """The hash the Makefile embeds (fslr_source_hash): sha256 of the sorted csrc/*.hip and *.hpp, then
    include/fslr_hip.h, first 16 hex digits; None when the sources are not beside the package."""
    import glob
    import hashlib
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, 'csrc')
    hdr = os.path.join(os.path.dirname(here), 'include', 'fslr_hip.h')
    files = sorted(os.path.basename(p) for p in glob.glob(os.path.join(csrc, '*.hip')) + glob.glob(os.path.join(csrc, '*.hpp')))
    if not files or not os.path.exists(hdr):
        return None
    h = hashlib.sha256()
    for f in files:
        with open(os.path.join(csrc, f), 'rb') as fh:
            h.update(fh.read())
    with open(hdr, 'rb') as fh:
        h.update(fh.read())
    return h.hexdigest()[:16]


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(ctypes.c_void_p)


_contexts_created = False


def contexts_created() -> bool:
    """True once this process created a Context (the library's HIP runtime is initialised)."""
    return _contexts_created


class Context:
    """One HIP device context (library-owned HBM buffers + a stream)."""

    def __init__(self, device: int = 0, stream: int | None = None, profiling: bool = False):
        """``stream``: a hipStream_t handle (e.g. ``torch.cuda.Stream().cuda_stream``); None or 0
        (the null stream cannot be shared) = the library creates its own stream."""
        self._L = load()
        h = ctypes.c_void_p()
        rc = self._L.fslr_ctx_create(int(device), ctypes.c_void_p(stream) if stream else None, ctypes.byref(h))
        if rc != FSLR_OK:
            raise HipUnavailable(f'fslr_ctx_create(device={device}) failed (rc={rc}): no usable HIP device')
        self._h = h
        global _contexts_created
        _contexts_created = True
        self.device = device
        self.n_reads = 0
        self.edge_capacity = 0
        self._keep = ()
        if profiling:
            self._check(self._L.fslr_set_profiling(self._h, 1))

    def set_query_reuse(self, enable: bool):
        """False: every query does the full work (length-gate ranges, entry-count readback), as a single
        query on new input does; True (default): a repeat on unchanged input keeps them."""
        self._check(self._L.fslr_set_query_reuse(self._h, 1 if enable else 0))

    def set_profiling(self, level: int):
        """1: per-phase events and the pair-kernel events; 2: the pair-kernel events only; 0: off."""
        self._check(self._L.fslr_set_profiling(self._h, int(level)))

    def close(self):
        if getattr(self, '_h', None):
            self._L.fslr_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc == FSLR_OK:
            return
        msg = (self._L.fslr_last_error(self._h) or b'').decode()
        if rc == FSLR_ERR_ZERO_DIVISION:
            raise ZeroDivisionError('division by zero')
        raise FslrError(f'fslr error {rc}: {msg}')

    # -- data -------------------------------------------------------------------------
    def set_reads(self, read_off, read_qlen2, read_nal, iv_chrom, iv_start, iv_end, iv_thr, n_chroms,
                  iv_data_pos=None):
        arrs = [np.ascontiguousarray(x, dtype=np.int32) for x in
                (read_off, read_qlen2, read_nal, iv_chrom, iv_start, iv_end, iv_thr)]
        dp = None if iv_data_pos is None else np.ascontiguousarray(iv_data_pos, dtype=np.int32)
        r = Reads(len(arrs[1]), len(arrs[3]), int(n_chroms), *(_ptr(a) for a in arrs),
                  _ptr(dp) if dp is not None else None)
        self._check(self._L.fslr_set_reads(self._h, ctypes.byref(r)))
        self._data_order = dp is not None
        if arrs[2].size and (arrs[2].min() < 0 or arrs[2].max() >= (1 << 24)):
            raise ValueError('n_alignments must lie in [0, 2**24) for the device path')
        self.n_reads = len(arrs[1])
        self.n_intervals = len(arrs[3])
        self._read_len = np.diff(arrs[0])                 # remove_reads counts the survivors' intervals with it

    def load_csr_any(self, csr, iv_thr):
        """Upload a CSR whose reads may have more than FSLR_MAX_L intervals (fslr_set_reads_any: the
        library splits them into chunks); thresholds here and in set_thresholds are in
        the CSR's own interval order.  Labels and forward degrees then cover the virtual reads (the
        real reads first)."""
        arrs = [np.ascontiguousarray(x, dtype=np.int32) for x in
                (csr.read_off, csr.read_qlen2, csr.read_nal, csr.iv_chrom, csr.iv_start, csr.iv_end, iv_thr)]
        dp = np.ascontiguousarray(csr.data_pos, dtype=np.int32) if getattr(csr, 'start_sorted', True) else None
        r = Reads(len(arrs[1]), len(arrs[3]), int(csr.n_chroms), *(_ptr(a) for a in arrs),
                  _ptr(dp) if dp is not None else None)
        self._check(self._L.fslr_set_reads_any(self._h, ctypes.byref(r)))
        self._data_order = dp is not None
        L = np.diff(arrs[0].astype(np.int64))
        self.n_reads = int(len(arrs[1]) + np.maximum((L + FSLR_MAX_L - 1) // FSLR_MAX_L - 1, 0).sum())
        self.n_intervals = len(arrs[3])
        self._read_len = L.astype(np.int32)               # the REAL reads' lengths (the _any calls count with them)

    def rows_upload(self, cols, n_codes, n_chrom_ids):
        """fslr_rows_upload: keep_fillings' rows (``cols``: int64 columns chrom, start, end, aln, qcode,
        nal, qlen2 in file order).  Releases the GIL while it copies (a caller sorts beside it)."""
        names = ('chrom', 'start', 'end', 'aln', 'qcode', 'nal', 'qlen2')
        arrs = [np.ascontiguousarray(cols[k], dtype=np.int64) for k in names]
        self._rows_keep = arrs
        r = Rows(int(arrs[0].size), int(n_codes), int(n_chrom_ids), *(_ptr(a) for a in arrs))
        self._check(self._L.fslr_rows_upload(self._h, ctypes.byref(r)))

    def set_reads_rows(self, order, keep, overlap) -> dict:
        """fslr_set_reads_rows: the reads from the uploaded rows, their start order and mask keep flags
        (None: all); thresholds folded for ``overlap``.  Returns the info dict; raises FslrError (with
        ``info``) when the rows do not fit (a read of more than FSLR_MAX_L intervals)."""
        o = np.ascontiguousarray(order, dtype=np.int64)
        k = None if keep is None else np.ascontiguousarray(keep).view(np.uint8)
        info = RowsInfo()
        rc = self._L.fslr_set_reads_rows(self._h, _ptr(o), _ptr(k) if k is not None else None, float(overlap),
                                         ctypes.byref(info))
        self._rows_keep = None
        d = info.as_dict()
        if rc != FSLR_OK:
            try:
                self._check(rc)
            except FslrError as e:
                e.info = d
                raise
        self.n_reads = d['n_reads']
        self.n_intervals = d['n_intervals']
        self._data_order = True
        return d

    def has_data_order(self) -> bool:
        """The reads came with prepare_data's start-sorted data order (the data-order index build, which
        the chromosome filter and the position split need)."""
        return bool(getattr(self, '_data_order', False))

    def read_codes(self) -> np.ndarray:
        out = np.empty(self.n_reads, np.int64)
        self._check(self._L.fslr_get_read_codes(self._h, _ptr(out)))
        return out

    def device_csr(self, n_intervals: int, n_chroms: int):
        """The CSR a fslr_set_reads_rows context holds, as host arrays (fslr_get_csr)."""
        n, ni = self.n_reads, int(n_intervals)
        out = dict(read_off=np.empty(n + 1, np.int32), read_qlen2=np.empty(n, np.int32), read_nal=np.empty(n, np.int32),
                   iv_chrom=np.empty(ni, np.int32), iv_start=np.empty(ni, np.int32), iv_end=np.empty(ni, np.int32),
                   iv_aln=np.empty(ni, np.int64), iv_thr=np.empty(ni, np.int32), data_pos=np.empty(ni, np.int64))
        out['chrom_ids'] = np.empty(max(1, int(n_chroms)), np.int64)
        self._check(self._L.fslr_get_csr(self._h, *(_ptr(out[k]) for k in ('read_off', 'read_qlen2', 'read_nal',
                                                                        'iv_chrom', 'iv_start', 'iv_end', 'iv_aln',
                                                                        'iv_thr', 'data_pos', 'chrom_ids'))))
        return out

    def fold_thresholds(self, overlap):
        self.thr_gen = getattr(self, 'thr_gen', 0) + 1
        self._check(self._L.fslr_fold_thresholds(self._h, float(overlap)))

    def set_long_cutoffs(self, umax):
        u = np.ascontiguousarray(umax, dtype=np.int32)
        self._check(self._L.fslr_set_long_cutoffs(self._h, _ptr(u), int(u.size)))

    def load_csr(self, csr, iv_thr):
        """Upload a ``fslr_amd.prep.CSR`` (with its start-sorted data order) and thresholds."""
        # the data-order index build needs the list in start order (prepare_data's sort); any other
        # order (a caller-built list) takes the full (chrom, start) sort
        self.set_reads(csr.read_off, csr.read_qlen2, csr.read_nal, csr.iv_chrom, csr.iv_start, csr.iv_end, iv_thr,
                       csr.n_chroms, iv_data_pos=csr.data_pos if getattr(csr, 'start_sorted', True) else None)

    def append_reads(self, read_off, read_qlen2, read_nal, iv_chrom, iv_start, iv_end, iv_thr, n_chroms, iv_data_pos):
        """fslr_append_reads: m more reads behind the resident ones (ranks n .., the resident dense chromosome
        ids, ``iv_data_pos`` the batch's own start-sorted order).  A refused batch leaves the context as it
        was; after a successful one build_index again."""
        arrs = [np.ascontiguousarray(x, dtype=np.int32) for x in
                (read_off, read_qlen2, read_nal, iv_chrom, iv_start, iv_end, iv_thr)]
        dp = None if iv_data_pos is None else np.ascontiguousarray(iv_data_pos, dtype=np.int32)
        r = Reads(len(arrs[1]), len(arrs[3]), int(n_chroms), *(_ptr(a) for a in arrs),
                  _ptr(dp) if dp is not None else None)
        rc = self._L.fslr_append_reads(self._h, ctypes.byref(r))
        if rc == FSLR_ERR_HIP:
            # a refused batch (FSLR_ERR_INVALID / FSLR_ERR_STATE) and a failed allocation (FSLR_ERR_NOMEM) leave
            # the context as it was; a device failure may leave no reads set (include/fslr_hip.h)
            self.n_reads = self.n_intervals = 0
        self._check(rc)
        self.n_reads += len(arrs[1])
        self.n_intervals += len(arrs[3])
        self._read_len = np.concatenate([self._read_len, np.diff(arrs[0])])
        if len(arrs[1]):
            self.thr_gen = getattr(self, 'thr_gen', 0) + 1        # the device's threshold column changed

    def append_csr(self, csr, iv_thr):
        """append_reads of a ``fslr_amd.prep.CSR`` whose ``iv_chrom`` holds the resident dense ids."""
        self.append_reads(csr.read_off, csr.read_qlen2, csr.read_nal, csr.iv_chrom, csr.iv_start, csr.iv_end, iv_thr,
                          csr.n_chroms, csr.data_pos)

    def append_reads_any(self, read_off, read_qlen2, read_nal, iv_chrom, iv_start, iv_end, iv_thr, n_chroms, iv_data_pos):
        """fslr_append_reads_any: append_reads for a batch whose reads may have up to FSLR_MAX_ANY_L intervals
        and for a context loaded with load_csr_any.  The batch is a REAL CSR; ``n_reads`` then counts the
        virtual reads as load_csr_any does.  A refused batch leaves the context as it was."""
        arrs = [np.ascontiguousarray(x, dtype=np.int32) for x in
                (read_off, read_qlen2, read_nal, iv_chrom, iv_start, iv_end, iv_thr)]
        dp = None if iv_data_pos is None else np.ascontiguousarray(iv_data_pos, dtype=np.int32)
        r = Reads(len(arrs[1]), len(arrs[3]), int(n_chroms), *(_ptr(a) for a in arrs),
                  _ptr(dp) if dp is not None else None)
        rc = self._L.fslr_append_reads_any(self._h, ctypes.byref(r))
        if rc == FSLR_ERR_HIP:
            self.n_reads = self.n_intervals = 0
        self._check(rc)
        L = np.diff(arrs[0].astype(np.int64))
        self.n_reads += int(len(arrs[1]) + np.maximum((L + FSLR_MAX_L - 1) // FSLR_MAX_L - 1, 0).sum())
        self.n_intervals += len(arrs[3])
        self._read_len = np.concatenate([self._read_len, L.astype(np.int32)])
        if len(arrs[1]):
            self.thr_gen = getattr(self, 'thr_gen', 0) + 1        # the device's threshold column changed

    def append_csr_any(self, csr, iv_thr):
        """append_reads_any of a ``fslr_amd.prep.CSR`` whose ``iv_chrom`` holds the resident dense ids."""
        self.append_reads_any(csr.read_off, csr.read_qlen2, csr.read_nal, csr.iv_chrom, csr.iv_start, csr.iv_end,
                              iv_thr, csr.n_chroms, csr.data_pos)

    def remove_reads_any(self, keep) -> np.ndarray:
        """fslr_remove_reads_any: remove_reads with ``keep`` over the REAL read ranks of a context that may hold
        reads of more than FSLR_MAX_L intervals (a removed read loses all its chunks).  Returns the old real
        rank -> new real rank map (int32, -1 removed)."""
        k = np.ascontiguousarray(np.asarray(keep) != 0, dtype=np.uint8)
        if k.ndim != 1:
            raise ValueError('keep is a vector over the read ranks')
        new_rank = np.empty(k.size, np.int32)
        rc = self._L.fslr_remove_reads_any(self._h, int(k.size), _ptr(k), _ptr(new_rank))
        if rc == FSLR_ERR_HIP:
            self.n_reads = self.n_intervals = 0
        self._check(rc)
        kept = int(np.count_nonzero(k))
        if kept != k.size:
            L = self._read_len[k != 0].astype(np.int64)
            self._read_len = self._read_len[k != 0]
            self.n_reads = int(kept + np.maximum((L + FSLR_MAX_L - 1) // FSLR_MAX_L - 1, 0).sum())
            self.n_intervals = int(L.sum())
            self.thr_gen = getattr(self, 'thr_gen', 0) + 1        # the device's threshold column changed
        return new_rank

    def append_timings(self) -> dict:
        """HIP-event times (ms) of the last append_reads' phases (profiling contexts)."""
        ms = (ctypes.c_float * 4)()
        self._check(self._L.fslr_append_timings(self._h, ms))
        return dict(zip(('upload', 'pack', 'merge', 'total'), (float(x) for x in ms)))

    def remove_reads(self, keep) -> np.ndarray:
        """fslr_remove_reads: drop the reads whose ``keep`` entry (over the ranks) is false; the survivors close
        the gaps in rank, CSR and data order.  Returns the old rank -> new rank map (int32, -1 removed).  A
        refused call leaves the context as it was; after a successful one build_index again."""
        k = np.ascontiguousarray(np.asarray(keep) != 0, dtype=np.uint8)
        if k.ndim != 1:
            raise ValueError('keep is a vector over the read ranks')
        new_rank = np.empty(k.size, np.int32)
        rc = self._L.fslr_remove_reads(self._h, int(k.size), _ptr(k), _ptr(new_rank))
        if rc == FSLR_ERR_HIP:
            # a refused call and a failed allocation leave the context as it was; a device failure may leave no
            # reads set (include/fslr_hip.h)
            self.n_reads = self.n_intervals = 0
        self._check(rc)
        kept = int(np.count_nonzero(k))
        if kept != k.size:
            self._read_len = self._read_len[k != 0]
            self.n_reads = kept
            self.n_intervals = int(self._read_len.sum())
            self.thr_gen = getattr(self, 'thr_gen', 0) + 1        # the device's threshold column changed
        return new_rank

    def remove_timings(self) -> dict:
        """HIP-event times (ms) of the last remove_reads' phases (profiling contexts)."""
        ms = (ctypes.c_float * 4)()
        self._check(self._L.fslr_remove_timings(self._h, ms))
        return dict(zip(('upload', 'maps', 'compact', 'total'), (float(x) for x in ms)))

    def set_thresholds(self, iv_thr):
        t = np.ascontiguousarray(iv_thr, dtype=np.int32)
        self.thr_gen = getattr(self, 'thr_gen', 0) + 1     # a position plan is cut for the old windows
        self._check(self._L.fslr_set_thresholds(self._h, _ptr(t)))

    def reserve_edges(self, cap):
        self._check(self._L.fslr_reserve_edges(self._h, int(cap)))
        self.edge_capacity = max(self.edge_capacity, int(cap))

    # -- compute (async) ------------------------------------------------------------------
    def _params(self, qlen_cut, nal_cut, pass_table, edge_threshold, engine='auto'):
        pt = np.ascontiguousarray(pass_table, dtype=np.uint8)
        assert pt.size == FSLR_MAX_L * PASS_STRIDE
        self._keep = (pt,)
        return Params(float(qlen_cut), float(nal_cut), _ptr(pt), int(edge_threshold), ENGINES[engine])

    def build_index(self):
        self._check(self._L.fslr_build_index(self._h))

    def query(self, qlen_cut, nal_cut, pass_table, edge_threshold=10, a_begin=0, a_end=None, engine='auto'):
        """``engine``: 'auto' (the sweep when the input allows it and the query covers every read),
        'walk' (counts evaluated_pairs / jaccard_evals) or 'sweep' (fslr_hip.h FSLR_ENGINE_*)."""
        p = self._params(qlen_cut, nal_cut, pass_table, edge_threshold, engine)
        a_end = self.n_reads if a_end is None else a_end
        self._check(self._L.fslr_query(self._h, ctypes.byref(p), int(a_begin), int(a_end)))

    def set_shard(self, shard: int, n_shards: int):
        """Build the query-side index data only for shard `shard` of `n_shards` (fslr_set_shard)."""
        self._check(self._L.fslr_set_shard(self._h, int(shard), int(n_shards)))

    def query_shard(self, qlen_cut, nal_cut, pass_table, shard, n_shards, edge_threshold=10):
        """Query shard `shard` of `n_shards` (rank blocks of 64 dealt round robin; fslr_query_shard)."""
        p = self._params(qlen_cut, nal_cut, pass_table, edge_threshold)
        self._check(self._L.fslr_query_shard(self._h, ctypes.byref(p), int(shard), int(n_shards)))

    # -- multi-GPU sweep (fslr_hip.h fslr_set_chrom_filter / fslr_sweep_partition / _evaluate) ----
    def set_chrom_filter(self, owned):
        """Index only the chromosomes with ``owned[c]`` true at the next build_index (None: all)."""
        if owned is None:
            self._check(self._L.fslr_set_chrom_filter(self._h, None))
            return
        o = np.ascontiguousarray(np.asarray(owned, dtype=bool).astype(np.uint8))
        self._check(self._L.fslr_set_chrom_filter(self._h, _ptr(o)))

    def position_costs(self):
        """(pair tests, forward-window end) per 64-position tile of the full index (fslr_position_costs)."""
        nt = (self.n_intervals + 63) // 64
        tests, reach = np.zeros(nt, np.int64), np.zeros(nt, np.int64)
        self._check(self._L.fslr_position_costs(self._h, _ptr(tests), _ptr(reach), nt))
        return tests, reach

    def position_entries(self, qlen_cut, nal_cut, pass_table, edge_threshold=10):
        """Match entries per 64-position tile of the full index under these parameters
        (fslr_position_entries: a counting sweep)."""
        nt = (self.n_intervals + 63) // 64
        ent = np.zeros(nt, np.int64)
        p = self._params(qlen_cut, nal_cut, pass_table, edge_threshold)
        self._check(self._L.fslr_position_entries(self._h, ctypes.byref(p), _ptr(ent), nt))
        return ent

    def set_position_filter(self, lo, hi, end):
        self._check(self._L.fslr_set_position_filter(self._h, int(lo), int(hi), int(end)))

    def use_position_filter(self):
        self._check(self._L.fslr_use_position_filter(self._h))

    def sweep_partition(self, qlen_cut, nal_cut, pass_table, n_dest, block_shift, dst, edge_threshold=10):
        """Sweep the (filtered) index and write the match entries grouped by destination
        (a >> block_shift) % n_dest into ``dst`` (an int64 device tensor on this context's device).
        Returns (ok, counts[n_dest]); ok False means ``dst`` was too small and nothing usable was
        written: grow it to counts.sum() and call again."""
        p = self._params(qlen_cut, nal_cut, pass_table, edge_threshold)
        counts = np.zeros(int(n_dest), np.int64)
        cap = int(dst.numel())
        rc = self._L.fslr_sweep_partition(self._h, ctypes.byref(p), int(n_dest), int(block_shift),
                                          ctypes.c_void_p(dst.data_ptr()) if cap else None, cap,
                                          counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
        if rc == FSLR_ERR_STATE and counts.sum() > cap:
            return False, counts
        self._check(rc)
        return True, counts

    def sweep_partition_repeat(self, qlen_cut, nal_cut, pass_table, n_dest, block_shift, dst, edge_threshold=10):
        """sweep_partition again on unchanged input, parameters and split, without the readback: the
        entries land where the last synchronous call put them (async).  A difference is flagged on
        the device and raised by the next stats() (fslr_sweep_partition_repeat)."""
        p = self._params(qlen_cut, nal_cut, pass_table, edge_threshold)
        self._check(self._L.fslr_sweep_partition_repeat(self._h, ctypes.byref(p), int(n_dest), int(block_shift),
                                                        ctypes.c_void_p(dst.data_ptr()), int(dst.numel())))

    def sweep_evaluate(self, qlen_cut, nal_cut, pass_table, entries, n, edge_threshold=10):
        """Evaluate the pairs of the first ``n`` entries of the int64 device tensor ``entries`` (async)."""
        p = self._params(qlen_cut, nal_cut, pass_table, edge_threshold)
        self._check(self._L.fslr_sweep_evaluate(self._h, ctypes.byref(p),
                                                ctypes.c_void_p(entries.data_ptr()) if n else None, int(n)))

    def labels_into(self, t):
        """Copy the [n_reads] labels into the int32 device tensor ``t`` (async, context stream)."""
        self._check(self._L.fslr_copy_labels_device(self._h, ctypes.c_void_p(t.data_ptr())))

    def edges_into(self, t, n_pad: int):
        """Copy this context's edges as (a, b) int32 pairs into the device tensor ``t`` (at least
        2 * n_pad int32), padded with (-1, -1) to n_pad pairs (async, context stream)."""
        assert t.numel() * t.element_size() >= 8 * n_pad
        self._check(self._L.fslr_copy_edges_device(self._h, ctypes.c_void_p(t.data_ptr()), int(n_pad)))

    def sort_edges(self):
        """This context's edges (with I, U) grouped by lower read, stably, in place."""
        self._check(self._L.fslr_sort_edges(self._h))

    def local_forest(self, count: bool = True):
        """Union-find over this context's edges, keeping the (read, root) pairs of non-root reads; their
        count (one sync) or None (async)."""
        if not count:
            self._check(self._L.fslr_local_forest(self._h, None))
            return None
        k = ctypes.c_int64()
        self._check(self._L.fslr_local_forest(self._h, ctypes.byref(k)))
        return int(k.value)

    def forest_pairs_into(self, t, n_pad: int):
        """The local forest's (read, root) int32 pairs into device tensor ``t`` (int64 view), padded."""
        self._check(self._L.fslr_copy_forest_pairs(self._h, ctypes.c_void_p(t.data_ptr()) if n_pad else None,
                                                   int(n_pad)))

    def components_from_pairs(self, t, n_pairs: int):
        """Labels = components of the n_pairs (a, b) int32 pairs in the device tensor ``t``
        (a < 0 = padding): the union of the ranks' gathered edge lists (async)."""
        self._check(self._L.fslr_components_from_pairs(self._h, ctypes.c_void_p(t.data_ptr()), int(n_pairs)))

    def union_label_vectors(self, t):
        """Union (k mod n_reads, t[k]) for the int32 device tensor ``t`` of W label vectors, then
        finalise the labels (async)."""
        self._check(self._L.fslr_union_pairs(self._h, None, ctypes.c_void_p(t.data_ptr()), int(t.numel()), 1))
        self._check(self._L.fslr_finalize_labels(self._h))

    def apply_edge_cap(self, edge_threshold=10) -> dict:
        """Replay the reference's per-read edge cap (cluster.py:223-224) on the last full query."""
        cs = CapStats()
        self._check(self._L.fslr_apply_edge_cap(self._h, int(edge_threshold), ctypes.byref(cs)))
        return cs.as_dict()

    def edge_cap_deferred(self, edge_threshold=10):
        """The edge-cap check of a repeated query without a host round trip (fslr_edge_cap_deferred)."""
        self._check(self._L.fslr_edge_cap_deferred(self._h, int(edge_threshold)))

    def edge_cap_deferred_read(self) -> int:
        """Sync; the deferred checks' sticky word (1: the cap bound, 2: a ZeroDivisionError pair), cleared."""
        f = ctypes.c_int32()
        self._check(self._L.fslr_edge_cap_deferred_read(self._h, ctypes.byref(f)))
        return int(f.value)

    # -- multi-GPU edge cap (fslr_hip.h fslr_cap_*) ------------------------------------------------
    def edges_iu_into(self, t, n_pad: int):
        """This context's edges as int32 rows {a, b, I | U << 8, 0} into the device tensor ``t`` (at least
        4 * n_pad int32), padded with a = -1 (async)."""
        assert t.numel() * t.element_size() >= 16 * n_pad
        self._check(self._L.fslr_copy_edges_iu_device(self._h, ctypes.c_void_p(t.data_ptr()), int(n_pad)))

    def cap_install_edges(self, t, n_rows: int):
        """The gathered E* rows (device tensor, a < 0 = padding) become this context's edges."""
        self._check(self._L.fslr_cap_install_edges(self._h, ctypes.c_void_p(t.data_ptr()) if n_rows else None,
                                                   int(n_rows)))

    def cap_local(self, edge_threshold=10):
        """Candidates and the search-ordered hits of the candidate intervals this index holds:
        returns (n_ti, n_hits)."""
        nti, nh = ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self._L.fslr_cap_local(self._h, int(edge_threshold), ctypes.byref(nti), ctypes.byref(nh)))
        return int(nti.value), int(nh.value)

    def cap_copy_local(self, counts, hits):
        self._check(self._L.fslr_cap_copy_local(self._h, ctypes.c_void_p(counts.data_ptr()),
                                                ctypes.c_void_p(hits.data_ptr())))

    def cap_replay(self, counts, hits, pad: int, world: int) -> dict:
        cs = CapStats()
        self._check(self._L.fslr_cap_replay(self._h, ctypes.c_void_p(counts.data_ptr()),
                                            ctypes.c_void_p(hits.data_ptr()), int(pad), int(world),
                                            ctypes.byref(cs)))
        return cs.as_dict()

    # -- multi-GPU edge cap sharded by the candidates' hit components (fslr_hip.h) ----------------
    @staticmethod
    def _dp(t, n):
        return ctypes.c_void_p(t.data_ptr()) if n else None

    def cap_install_pairs(self, t, n_rows: int, world: int, rank: int):
        """The gathered E* (a, b) int32 rows (device tensor; a < 0 = padding), rank w's block at w m."""
        self._check(self._L.fslr_cap_install_pairs(self._h, self._dp(t, n_rows), int(n_rows), int(world), int(rank)))

    def cap_bwd_counts(self, edge_threshold: int, t):
        """This rank's edge counts per upper read into device tensor ``t`` (uint8: clipped at the
        threshold, or int32), for the sum over ranks."""
        eb = t.element_size()
        self._check(self._L.fslr_cap_bwd_counts(self._h, int(edge_threshold), ctypes.c_void_p(t.data_ptr()), eb))

    def cap_restrict(self, t) -> int:
        """The rows of S from the summed counts ``t``; their count (one sync)."""
        k = ctypes.c_int64()
        self._check(self._L.fslr_cap_restrict(self._h, ctypes.c_void_p(t.data_ptr()), t.element_size(),
                                              ctypes.byref(k)))
        return int(k.value)

    def cap_copy_restricted(self, t, n_pad: int):
        self._check(self._L.fslr_cap_copy_restricted(self._h, self._dp(t, n_pad), int(n_pad)))

    def cap_install_restricted(self, t, n_rows: int, world: int, rank: int):
        self._check(self._L.fslr_cap_install_restricted(self._h, self._dp(t, n_rows), int(n_rows), int(world),
                                                        int(rank)))

    def cap_sizes(self):
        """(|T|, T-intervals, local hits) after cap_local."""
        v = [ctypes.c_int64() for _ in range(3)]
        self._check(self._L.fslr_cap_sizes(self._h, *[ctypes.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    def cap_dep_local(self, t):
        """t[0 .. 2|T|) (int32 device): local forest roots of T reads, then their local hit counts."""
        self._check(self._L.fslr_cap_dep_local(self._h, ctypes.c_void_p(t.data_ptr())))

    def cap_shard_plan(self, gathered, world: int, rank: int):
        """The components' ranks; returns (T-intervals per destination, local hits per destination)."""
        sizes = np.zeros(2 * world, np.int64)
        self._check(self._L.fslr_cap_shard_plan(self._h, ctypes.c_void_p(gathered.data_ptr()), int(world), int(rank),
                                                _ptr(sizes)))
        return sizes[:world].copy(), sizes[world:].copy()

    def cap_shard_pack(self, counts, hits):
        self._check(self._L.fslr_cap_shard_pack(self._h, ctypes.c_void_p(counts.data_ptr()),
                                                ctypes.c_void_p(hits.data_ptr())))

    def cap_replay_shard(self, counts, hits):
        """Replay this rank's components from the received lists; returns (changes, partial cap stats)."""
        nch = ctypes.c_int64()
        cs = CapStats()
        self._check(self._L.fslr_cap_replay_shard(self._h, ctypes.c_void_p(counts.data_ptr()),
                                                  ctypes.c_void_p(hits.data_ptr()), ctypes.byref(nch), ctypes.byref(cs)))
        return int(nch.value), cs.as_dict()

    def cap_copy_changes(self, t, n_pad: int):
        self._check(self._L.fslr_cap_copy_changes(self._h, self._dp(t, n_pad), int(n_pad)))

    def cap_apply_changes(self, t, n: int) -> dict:
        cs = CapStats()
        self._check(self._L.fslr_cap_apply_changes(self._h, self._dp(t, n), int(n), ctypes.byref(cs)))
        return cs.as_dict()

    def components(self):
        self._check(self._L.fslr_components(self._h))

    def run(self, qlen_cut, nal_cut, pass_table, edge_threshold=10, engine='auto'):
        p = self._params(qlen_cut, nal_cut, pass_table, edge_threshold, engine)
        self._check(self._L.fslr_run(self._h, ctypes.byref(p)))

    def sync(self):
        self._check(self._L.fslr_sync(self._h))

    # -- results ------------------------------------------------------------------------
    def reserve_deferred(self, cap):
        self._check(self._L.fslr_reserve_deferred(self._h, int(cap)))

    def stats(self, check: bool = True) -> dict:
        """Counters of the last query.  With ``check`` a buffer overflow raises FslrError;
        ``run_query`` grows the buffers and reruns instead."""
        s = QueryStats()
        rc = self._L.fslr_read_stats(self._h, ctypes.byref(s))
        if rc == FSLR_ERR_STATE and not check:
            return s.as_dict()
        self._check(rc)
        return s.as_dict()

    def run_query(self, qlen_cut, nal_cut, pass_table, edge_threshold=10, a_begin=0, a_end=None,
                  engine='auto') -> dict:
        """query + stats, growing the edge / deferred buffers and rerunning on overflow (and with the
        walk engine if the sweep's per-read partner table overflowed)."""
        while True:
            self.query(qlen_cut, nal_cut, pass_table, edge_threshold, a_begin, a_end, engine)
            st = self.stats(check=False)
            grow = False
            if st['overflow_flags'] & 4:
                engine = 'walk'
                grow = True
            if st['overflow_flags'] & 24:         # sweep entry buffers (a sync-free repeat query): rerun
                grow = True
            if st['overflow_flags'] & 64:         # the ZeroDivisionError pair list (the cap binds): rerun
                grow = True
            if st['n_edges'] > st['edge_capacity']:
                self.reserve_edges(int(st['n_edges'] * 1.25) + 4096)
                grow = True
            if st['deferred'] > st['deferred_capacity']:
                self.reserve_deferred(int(st['deferred'] * 1.25) + 4096)
                grow = True
            if not grow:
                self.stats()          # raises on a device-side error (ZeroDivisionError)
                return st

    def timings(self) -> dict:
        t = Timings()
        self._check(self._L.fslr_get_timings(self._h, ctypes.byref(t)))
        return t.as_dict()

    def pair_kernel_times(self, n: int = 256) -> np.ndarray:
        """Durations (ms) of the main pair-kernel launch of the last ``n`` queries (profiling contexts)."""
        out = np.zeros(n, np.float32)
        got = self._L.fslr_get_pair_kernel_times(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), n)
        if got < 0:
            self._check(-got)
        return out[:got]

    def stage_kernel_times(self, stage: int, n: int = 256) -> np.ndarray:
        """Durations (ms) of one stage kernel of the last ``n`` queries: 0 the main pair kernel, 1 the sweep
        engine's pair-stage kernel (profiling contexts)."""
        out = np.zeros(n, np.float32)
        got = self._L.fslr_get_stage_kernel_times(self._h, int(stage),
                                                  out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), n)
        if got < 0:
            self._check(-got)
        return out[:got]

    def counters(self, n: int = 80) -> np.ndarray:
        """Raw device counters of the last query (kernels.hpp Counter; diagnostics)."""
        out = np.zeros(n, np.uint64)
        got = self._L.fslr_read_counters(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), n)
        if got < 0:
            self._check(-got)
        return out[:got]

    def labels(self) -> np.ndarray:
        out = np.empty(self.n_reads, np.int32)
        self._check(self._L.fslr_get_labels(self._h, _ptr(out)))
        return out

    def fwd_degree(self) -> np.ndarray:
        out = np.empty(self.n_reads, np.int32)
        self._check(self._L.fslr_get_fwd_degree(self._h, _ptr(out)))
        return out

    def edges(self, n_edges: int):
        a = np.empty(n_edges, np.int32)
        b = np.empty(n_edges, np.int32)
        iu = np.empty(n_edges, np.uint16)
        self._check(self._L.fslr_get_edges(self._h, _ptr(a), _ptr(b), _ptr(iu), int(n_edges)))
        return a, b, (iu & 0xff).astype(np.int32), (iu >> 8).astype(np.int32)

    def labels_device_ptr(self) -> int:
        p = ctypes.c_void_p()
        self._check(self._L.fslr_labels_device_ptr(self._h, ctypes.byref(p)))
        return p.value

    def copy_labels_device(self, dptr: int):
        self._check(self._L.fslr_copy_labels_device(self._h, ctypes.c_void_p(dptr)))

    def copy_fwd_device(self, dptr: int):
        self._check(self._L.fslr_copy_fwd_device(self._h, ctypes.c_void_p(dptr)))

    def union_pairs(self, src, dst, n, on_device: bool):
        """Union (src[k], dst[k]); ``src`` None means src[k] = k mod n_reads.  Pointers are ints when on_device."""
        if on_device:
            self._check(self._L.fslr_union_pairs(self._h, ctypes.c_void_p(src) if src else None,
                                                 ctypes.c_void_p(dst), int(n), 1))
        else:
            s = None if src is None else np.ascontiguousarray(src, np.int32)
            d = np.ascontiguousarray(dst, np.int32)
            self._check(self._L.fslr_union_pairs(self._h, _ptr(s) if s is not None else None, _ptr(d), int(n), 0))

    # -- reads of more than FSLR_MAX_L intervals (fslr_hip.h fslr_set_long_reads / fslr_long_query) --
    def set_long_reads(self, n_real, vreal, vbase, rlen, umax):
        arrs = [np.ascontiguousarray(x, dtype=np.int32) for x in (vreal, vbase, rlen, umax)]
        self._check(self._L.fslr_set_long_reads(self._h, int(n_real), *(_ptr(a) for a in arrs), int(arrs[3].size)))

    def long_query(self, qlen_cut, nal_cut, pass_table, edge_threshold=10) -> int:
        """Sweep the virtual index and decide every pair (fslr_long_query); returns the long-pair edge count."""
        p = self._params(qlen_cut, nal_cut, pass_table, edge_threshold)
        ne = ctypes.c_int64(0)
        self._check(self._L.fslr_long_query(self._h, ctypes.byref(p), ctypes.byref(ne)))
        return int(ne.value)

    def long_pairs(self, qlen_cut, nal_cut, pass_table, edge_threshold=10) -> int:
        """Decide every distinct pair with the general evaluator (fslr_long_pairs); returns the edge count."""
        p = self._params(qlen_cut, nal_cut, pass_table, edge_threshold)
        ne = ctypes.c_int64(0)
        self._check(self._L.fslr_long_pairs(self._h, ctypes.byref(p), ctypes.byref(ne)))
        return int(ne.value)

    def long_pairs_shard(self, qlen_cut, nal_cut, pass_table, shard, n_shards, edge_threshold=10) -> int:
        """fslr_long_pairs for the pairs whose lower read lies in query shard ``shard`` of ``n_shards``."""
        p = self._params(qlen_cut, nal_cut, pass_table, edge_threshold)
        ne = ctypes.c_int64(0)
        self._check(self._L.fslr_long_pairs_shard(self._h, ctypes.byref(p), int(shard), int(n_shards),
                                                  ctypes.byref(ne)))
        return int(ne.value)

    def cap_replay_pairs(self, edge_threshold, a, b, n_reads: int):
        """The edge cap over the E* pairs (a < b): returns (who, fwd, cap stats) — fslr_cap_replay_pairs."""
        a = np.ascontiguousarray(a, np.int32)
        b = np.ascontiguousarray(b, np.int32)
        who = np.empty(a.shape[0], np.uint8)
        fwd = np.empty(int(n_reads), np.int32)
        cs = CapStats()
        self._check(self._L.fslr_cap_replay_pairs(self._h, int(edge_threshold), _ptr(a), _ptr(b), int(a.shape[0]),
                                                  _ptr(who), _ptr(fwd), ctypes.byref(cs)))
        return who, fwd, cs.as_dict()

    def long_edges(self, n_edges: int):
        out = [np.empty(n_edges, np.int32) for _ in range(4)]
        self._check(self._L.fslr_get_long_edges(self._h, *(_ptr(a) for a in out), int(n_edges)))
        return tuple(out)

    def finalize_labels(self):
        self._check(self._L.fslr_finalize_labels(self._h))

    # -- batched interval search (fslr_hip.h fslr_search / fslr_search_hits) -------------------------
    def _search(self, chrom, start, end, offsets):
        q = [np.ascontiguousarray(x, dtype=np.int32) for x in (chrom, start, end)]
        if not (q[0].ndim == 1 and q[0].shape == q[1].shape == q[2].shape):
            raise ValueError('chrom, start and end must be one-dimensional and of one length')
        total = ctypes.c_int64(0)
        self._check(self._L.fslr_search(self._h, int(q[0].size), *(_ptr(a) for a in q),
                                        _ptr(offsets) if offsets is not None else None, ctypes.byref(total)))
        return int(total.value)

    def search(self, chrom, start, end):
        """The stored intervals each query (dense chromosome id, start, end; int32) hits, end-inclusive:
        ``(offsets int64[nq + 1], hits int32[total])``, query k's hits at ``hits[offsets[k]:offsets[k + 1]]``
        as indices into the uploaded CSR, in the search order fslr_hip.h pins (fslr_search)."""
        offsets = np.zeros(np.asarray(chrom).size + 1, np.int64)
        total = self._search(chrom, start, end, offsets)
        hits = np.empty(total, np.int32)
        self._check(self._L.fslr_search_hits(self._h, _ptr(hits), total))
        return offsets, hits

    def search_counts(self, chrom, start, end) -> np.ndarray:
        """Hits per query, int64[nq] (fslr_search alone: no hit list is made)."""
        offsets = np.zeros(np.asarray(chrom).size + 1, np.int64)
        self._search(chrom, start, end, offsets)
        return np.diff(offsets)

    def search_timings(self) -> dict:
        """HIP-event times (ms) of the last search's passes (profiling contexts)."""
        ms = (ctypes.c_float * 4)()
        self._check(self._L.fslr_search_timings(self._h, ms))
        return dict(zip(('span', 'count', 'scan', 'fill'), (float(x) for x in ms)))

    # -- pair scoring (fslr_hip.h fslr_score_pairs) --------------------------------------------------
    def score_pairs(self, a, b, qlen_cut, nal_cut, pass_table):
        """The pair predicates for the ordered read pairs ``(a[k], b[k])`` (ranks of the uploaded reads):
        ``(I int32[n], U int32[n], flags uint8[n])``, flags the SCORE_* bits; the overlap thresholds are the
        ones currently set.  ZeroDivisionError is flagged per pair, not raised."""
        a, b = (np.ascontiguousarray(x, dtype=np.int32) for x in (a, b))
        if not (a.ndim == 1 and a.shape == b.shape):
            raise ValueError('a and b must be one-dimensional and of one length')
        p = self._params(qlen_cut, nal_cut, pass_table, 0)
        I, U, flags = np.zeros(a.size, np.int32), np.zeros(a.size, np.int32), np.zeros(a.size, np.uint8)
        self._check(self._L.fslr_score_pairs(self._h, ctypes.byref(p), int(a.size), _ptr(a), _ptr(b), _ptr(I), _ptr(U),
                                             _ptr(flags)))
        return I, U, flags

    def score_pairs_any(self, a, b, qlen_cut, nal_cut, pass_table, umax=None):
        """score_pairs for reads of any length (fslr_score_pairs_any): ``a`` and ``b`` are real read ranks (the
        reads as load_csr_any numbered them), a read's list is its whole real list, I and U are unclamped.
        ``umax`` (prep.umax_table over the longest read) decides EDGE beyond the pass table; it is required
        when the context holds reads of more than FSLR_MAX_L intervals."""
        a, b = (np.ascontiguousarray(x, dtype=np.int32) for x in (a, b))
        if not (a.ndim == 1 and a.shape == b.shape):
            raise ValueError('a and b must be one-dimensional and of one length')
        um = None
        if umax is not None:
            um = np.ascontiguousarray(umax, dtype=np.int32)
            if um.ndim != 1:
                raise ValueError('umax must be one-dimensional')
        p = self._params(qlen_cut, nal_cut, pass_table, 0)
        I, U, flags = np.zeros(a.size, np.int32), np.zeros(a.size, np.int32), np.zeros(a.size, np.uint8)
        self._check(self._L.fslr_score_pairs_any(self._h, ctypes.byref(p), _ptr(um) if um is not None else None,
                                                 int(um.size) if um is not None else 0, int(a.size), _ptr(a), _ptr(b),
                                                 _ptr(I), _ptr(U), _ptr(flags)))
        return I, U, flags

    def score_timings(self) -> dict:
        """HIP-event times (ms) of the last score_pairs (profiling contexts), summed over its chunks."""
        ms = (ctypes.c_float * 3)()
        self._check(self._L.fslr_score_timings(self._h, ms))
        return dict(zip(('upload', 'kernel', 'download'), (float(x) for x in ms)))

    # -- the matching of scored pairs (fslr_hip.h fslr_pair_matching) ---------------------------------
    def pair_matching(self, a, b, qlen_cut, nal_cut, pass_table):
        """score_pairs and, per pair, which interval of list1 took which interval of list2 in the first-fit
        (fslr_pair_matching): ``(I, U, flags, offsets int64[n + 1], i int32[total], j int32[total])``; pair
        k's rows are ``offsets[k]:offsets[k + 1]``, ``i`` ascending, I[k] of them (none for a pair flagged
        SCORE_ZD_OVERLAP)."""
        return self._pair_matching(False, a, b, qlen_cut, nal_cut, pass_table, None)

    def pair_matching_any(self, a, b, qlen_cut, nal_cut, pass_table, umax=None):
        """pair_matching for reads of any length (fslr_pair_matching_any): real read ranks, whole real
        lists, ``umax`` as score_pairs_any takes it."""
        return self._pair_matching(True, a, b, qlen_cut, nal_cut, pass_table, umax)

    def _pair_matching(self, any_length, a, b, qlen_cut, nal_cut, pass_table, umax):
        a, b = (np.ascontiguousarray(x, dtype=np.int32) for x in (a, b))
        if not (a.ndim == 1 and a.shape == b.shape):
            raise ValueError('a and b must be one-dimensional and of one length')
        um = None
        if umax is not None:
            um = np.ascontiguousarray(umax, dtype=np.int32)
            if um.ndim != 1:
                raise ValueError('umax must be one-dimensional')
        p = self._params(qlen_cut, nal_cut, pass_table, 0)
        n = int(a.size)
        I, U, flags = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint8)
        off = np.zeros(n + 1, np.int64)
        # rows: at most min(L1, L2) per pair, from the host's copy of the reads' lengths.  Where the reads were
        # made on the device (set_reads_rows) there is no such copy: a count-only call sizes the arrays
        L = np.asarray(getattr(self, '_read_len', np.zeros(0)), np.int64)
        # (a copy that is out of date costs a second call, never a wrong answer: a short capacity is retried)
        known = n > 0 and a.min() >= 0 and b.min() >= 0 and max(a.max(), b.max()) < L.size
        cap = int(np.minimum(L[a], L[b]).sum()) if known else 0
        total = ctypes.c_int64(0)
        while True:
            row, col = np.empty(cap, np.int32), np.empty(cap, np.int32)
            tail = (_ptr(a), _ptr(b), _ptr(I), _ptr(U), _ptr(flags), _ptr(off), _ptr(row) if cap else None,
                    _ptr(col) if cap else None, cap, ctypes.byref(total))
            if any_length:
                rc = self._L.fslr_pair_matching_any(self._h, ctypes.byref(p), _ptr(um) if um is not None else None,
                                                    int(um.size) if um is not None else 0, n, *tail)
            else:
                rc = self._L.fslr_pair_matching(self._h, ctypes.byref(p), n, *tail)
            if total.value <= cap:
                break
            cap = int(total.value)
        self._check(rc)
        return I, U, flags, off, row[:total.value], col[:total.value]

    def pair_matching_timings(self) -> dict:
        """HIP-event times (ms) of the last pair_matching (profiling contexts), summed over its chunks."""
        ms = (ctypes.c_float * 3)()
        self._check(self._L.fslr_pair_matching_timings(self._h, ms))
        return dict(zip(('upload', 'kernel', 'download'), (float(x) for x in ms)))

    # -- new reads against the resident index (fslr_hip.h fslr_match_reads / fslr_match_rows) --------
    def match_reads(self, read_off, read_qlen2, read_nal, iv_chrom, iv_start, iv_end, iv_thr, qlen_cut, nal_cut,
                    pass_table, emit_mask=SCORE_EDGE, exclude=None):
        """The pair loop for query reads outside the uploaded set (fslr_match_reads; reads of at most FSLR_MAX_L
        intervals on both sides): see ``_match_reads``.  The rows are fetched with ``match_rows``."""
        return self._match_reads(False, None, read_off, read_qlen2, read_nal, iv_chrom, iv_start, iv_end, iv_thr,
                                 qlen_cut, nal_cut, pass_table, emit_mask, exclude)

    def match_reads_any(self, read_off, read_qlen2, read_nal, iv_chrom, iv_start, iv_end, iv_thr, qlen_cut, nal_cut,
                        pass_table, emit_mask=SCORE_EDGE, exclude=None, umax=None):
        """match_reads for reads of any length (fslr_match_reads_any): query and resident reads of up to 4096
        intervals, ``exclude`` and the partners are real read ranks, I and U are unclamped.  ``umax``
        (prep.umax_table over the longest list) decides EDGE beyond the pass table; it is required when the
        context holds reads of more than FSLR_MAX_L intervals or a query read has more.  The rows are fetched
        with ``match_rows_any``."""
        um = None
        if umax is not None:
            um = np.ascontiguousarray(umax, dtype=np.int32)
            if um.ndim != 1:
                raise ValueError('umax must be one-dimensional')
        return self._match_reads(True, um, read_off, read_qlen2, read_nal, iv_chrom, iv_start, iv_end, iv_thr,
                                 qlen_cut, nal_cut, pass_table, emit_mask, exclude)

    def _match_reads(self, any_length, um, read_off, read_qlen2, read_nal, iv_chrom, iv_start, iv_end, iv_thr,
                     qlen_cut, nal_cut, pass_table, emit_mask, exclude):
        """The pair loop for query reads outside the uploaded set (a CSR like set_reads', dense chromosome
        ids, folded thresholds): ``(offsets int64[n + 1], counts int32[n, 3], best int32[n])``, counts =
        candidates, gated, edges per query read, best = the partner of the largest I / U or -1.  The rows
        (``offsets[-1]`` of them) are fetched with ``match_rows``."""
        off, q2, nal, ch, st, en, th = (np.ascontiguousarray(x, dtype=np.int32) for x in
                                        (read_off, read_qlen2, read_nal, iv_chrom, iv_start, iv_end, iv_thr))
        if off.ndim != 1 or off.size < 1:
            raise ValueError('read_off must be one-dimensional with n_reads + 1 entries')
        n = off.size - 1
        if not (q2.shape == nal.shape == (n,)):
            raise ValueError('read_qlen2 and read_nal must have one entry per query read')
        if not (ch.ndim == 1 and ch.shape == st.shape == en.shape == th.shape):
            raise ValueError('iv_chrom, iv_start, iv_end and iv_thr must be one-dimensional and of one length')
        ex = None
        if exclude is not None:
            ex = np.ascontiguousarray(exclude, dtype=np.int32)
            if ex.shape != (n,):
                raise ValueError('exclude must have one entry per query read')
        q = MatchQueries(n, int(ch.size), *(_ptr(a) for a in (off, q2, nal, ch, st, en, th)),
                         _ptr(ex) if ex is not None else None)
        p = self._params(qlen_cut, nal_cut, pass_table, 0)
        offsets, counts, best = np.zeros(n + 1, np.int64), np.zeros((n, 3), np.int32), np.full(n, -1, np.int32)
        total = ctypes.c_int64(0)
        if any_length:
            self._check(self._L.fslr_match_reads_any(self._h, ctypes.byref(p), _ptr(um) if um is not None else None,
                                                     int(um.size) if um is not None else 0, ctypes.byref(q),
                                                     int(emit_mask), _ptr(offsets), _ptr(counts), _ptr(best),
                                                     ctypes.byref(total)))
        else:
            self._check(self._L.fslr_match_reads(self._h, ctypes.byref(p), ctypes.byref(q), int(emit_mask),
                                                 _ptr(offsets), _ptr(counts), _ptr(best), ctypes.byref(total)))
        self._match_rows = int(total.value)
        return offsets, counts, best

    def match_rows_any(self):
        """The last match_reads_any's rows, as match_rows gives match_reads'."""
        n = getattr(self, '_match_rows', 0)
        partner, I, U = (np.zeros(n, np.int32) for _ in range(3))
        flags = np.zeros(n, np.uint8)
        self._check(self._L.fslr_match_rows_any(self._h, _ptr(partner), _ptr(I), _ptr(U), _ptr(flags), n))
        return partner, I, U, flags

    def match_rows(self):
        """The last match_reads' rows: ``(partner int32, I int32, U int32, flags uint8)``, query read after
        query read in candidate (first-visit) order."""
        n = getattr(self, '_match_rows', 0)
        partner, I, U = (np.zeros(n, np.int32) for _ in range(3))
        flags = np.zeros(n, np.uint8)
        self._check(self._L.fslr_match_rows(self._h, _ptr(partner), _ptr(I), _ptr(U), _ptr(flags), n))
        return partner, I, U, flags

    def match_timings(self) -> dict:
        """HIP-event times (ms) of the last match_reads (profiling contexts), summed over its chunks."""
        ms = (ctypes.c_float * 4)()
        self._check(self._L.fslr_match_timings(self._h, ms))
        return dict(zip(('upload', 'search', 'score', 'download'), (float(x) for x in ms)))

    # -- read depth at query points (fslr_hip.h fslr_coverage_build / fslr_coverage_at) --------------
    def coverage_build(self, chrom, rstart, rend, n_chroms):
        """Make the context's coverage set from the bed rows (dense chromosome id, rstart, rend; int32, any
        order); it replaces the one before.  ``coverage_gen`` counts the builds that succeeded."""
        r = [np.ascontiguousarray(x, dtype=np.int32) for x in (chrom, rstart, rend)]
        if not (r[0].ndim == 1 and r[0].shape == r[1].shape == r[2].shape):
            raise ValueError('chrom, rstart and rend must be one-dimensional and of one length')
        self._check(self._L.fslr_coverage_build(self._h, int(r[0].size), int(n_chroms), *(_ptr(a) for a in r)))
        self.coverage_gen = getattr(self, 'coverage_gen', 0) + 1

    def coverage_at(self, chrom, pos) -> np.ndarray:
        """The depth (int32) at each (dense chromosome id, position) of the batch, in input order:
        rows with rstart <= pos less rows with rend <= pos (cluster.py:52-67)."""
        q = [np.ascontiguousarray(x, dtype=np.int32) for x in (chrom, pos)]
        if not (q[0].ndim == 1 and q[0].shape == q[1].shape):
            raise ValueError('chrom and pos must be one-dimensional and of one length')
        depth = np.zeros(q[0].size, np.int32)
        self._check(self._L.fslr_coverage_at(self._h, int(q[0].size), _ptr(q[0]), _ptr(q[1]), _ptr(depth)))
        return depth

    def coverage_timings(self) -> dict:
        """HIP-event times (ms) of the last coverage_build and coverage_at (profiling contexts), each summed
        over the call's chunks."""
        ms = (ctypes.c_float * 4)()
        self._check(self._L.fslr_coverage_timings(self._h, ms))
        return dict(zip(('build_upload', 'build_sort', 'query_upload_kernel', 'query_download'), (float(x) for x in ms)))

    # -- cluster table and representatives (fslr_hip.h fslr_cluster_table ...) ------------------------
    def cluster_table(self, labels=None) -> dict:
        """Make the context's cluster table from min-rank labels: the device labels of the last components
        call (``labels`` None) or a host vector (int32).  Returns ``{n, n_clusters, n_nodes, max_size}``; the
        table replaces the one before."""
        info = ClusterInfo()
        self._loci_rows = None                   # fslr_cluster_table drops the loci rows
        if labels is None:
            self._check(self._L.fslr_cluster_table(self._h, None, 0, ctypes.byref(info)))
            n = int(self.n_reads)
        else:
            lab = np.ascontiguousarray(labels, dtype=np.int32)
            if lab.ndim != 1:
                raise ValueError('labels must be one-dimensional')
            n = int(lab.size)
            # (a NULL pointer selects the device labels: an empty vector still passes an address)
            self._check(self._L.fslr_cluster_table(self._h, _ptr(lab) if n else _ptr(np.zeros(1, np.int32)), n,
                                                   ctypes.byref(info)))
        self._cluster_info = dict(info.as_dict(), n=n)
        return dict(self._cluster_info)

    def cluster_ids(self):
        """``(cid int32[n], size int32[n])`` of the table: the dense cluster id of each read rank (-1 for a
        read alone) and the size of its component."""
        ci = getattr(self, '_cluster_info', None) or {'n': 0}
        cid, size = np.empty(ci['n'], np.int32), np.empty(ci['n'], np.int32)
        self._check(self._L.fslr_get_cluster_ids(self._h, _ptr(cid), _ptr(size)))
        return cid, size

    def cluster_members(self):
        """``(off int64[n_clusters + 1], members int32[n_nodes])``: cluster k's read ranks, ascending, are
        ``members[off[k]:off[k + 1]]``."""
        ci = getattr(self, '_cluster_info', None) or {'n_clusters': 0, 'n_nodes': 0}
        off, members = np.zeros(ci['n_clusters'] + 1, np.int64), np.empty(ci['n_nodes'], np.int32)
        self._check(self._L.fslr_get_cluster_members(self._h, _ptr(off), _ptr(members)))
        return off, members

    def assign_clusters(self, present, code_of_rank=None):
        """main.py:334-342 over qname codes: ``(cluster int64[n_codes], n_reads int64[n_codes],
        n_singletons)`` for ``present`` (bool per code) and the code of each read rank (None: the
        identity)."""
        pres = np.ascontiguousarray(present, dtype=np.uint8)
        if pres.ndim != 1:
            raise ValueError('present must be one-dimensional')
        cor = None if code_of_rank is None else np.ascontiguousarray(code_of_rank, dtype=np.int64)
        nc = int(pres.size)
        cl, nr = np.empty(nc, np.int64), np.empty(nc, np.int64)
        k = ctypes.c_int64(0)
        self._check(self._L.fslr_assign_clusters(self._h, nc, _ptr(cor) if cor is not None else None, _ptr(pres),
                                                 _ptr(cl), _ptr(nr), ctypes.byref(k)))
        return cl, nr, int(k.value)

    def choose_representatives(self, cluster, score_sum, score_cnt, first_row, n_out):
        """cluster.py:237-254 over qname codes: ``(avg float64[n_codes], winner_code int64[n_out])``."""
        a = [np.ascontiguousarray(x, dtype=np.int64) for x in (cluster, score_sum, score_cnt, first_row)]
        if not (a[0].ndim == 1 and a[0].shape == a[1].shape == a[2].shape == a[3].shape):
            raise ValueError('cluster, score_sum, score_cnt and first_row must be one-dimensional and of one length')
        avg, win = np.empty(a[0].size, np.float64), np.empty(int(n_out), np.int64)
        self._check(self._L.fslr_choose_representatives(self._h, int(a[0].size), *(_ptr(x) for x in a), int(n_out),
                                                        _ptr(avg), _ptr(win)))
        return avg, win

    def cluster_timings(self) -> dict:
        """HIP-event times (ms) of the last cluster_table, assign_clusters and choose_representatives
        (profiling contexts)."""
        ms = (ctypes.c_float * 3)()
        self._check(self._L.fslr_cluster_timings(self._h, ms))
        return dict(zip(('table', 'assign', 'choose'), (float(x) for x in ms)))

    # -- cluster loci (fslr_hip.h fslr_cluster_loci) ---------------------------------------------------
    def cluster_loci(self):
        """The merged spans of each cluster's intervals per chromosome, from the resident index and cluster
        table: ``(off int64[n_clusters + 1], chrom, start, end, n_intervals, n_reads)`` (int32 per row, dense
        chromosome ids), rows ordered by (cluster, chrom, start)."""
        n = ctypes.c_int64(0)
        self._check(self._L.fslr_cluster_loci(self._h, ctypes.byref(n)))
        nr = int(n.value)
        ci = getattr(self, '_cluster_info', None) or {'n_clusters': 0}
        off = np.zeros(ci['n_clusters'] + 1, np.int64)
        cols = [np.empty(nr, np.int32) for _ in range(5)]
        self._check(self._L.fslr_get_cluster_loci(self._h, _ptr(off), *(_ptr(x) for x in cols), nr))
        self._loci_rows = nr
        return (off, *cols)

    def cluster_loci_rows(self):
        """cluster_loci's result without making the rows again when this context made them since its last
        cluster_table (they are copied down as they are); else cluster_loci()."""
        nr = getattr(self, '_loci_rows', None)
        if nr is None:
            return self.cluster_loci()
        ci = getattr(self, '_cluster_info', None) or {'n_clusters': 0}
        off = np.zeros(ci['n_clusters'] + 1, np.int64)
        cols = [np.empty(nr, np.int32) for _ in range(5)]
        self._check(self._L.fslr_get_cluster_loci(self._h, _ptr(off), *(_ptr(x) for x in cols), nr))
        return (off, *cols)

    def cluster_loci_timings(self) -> dict:
        """HIP-event time (ms) of the last cluster_loci (profiling contexts)."""
        ms = (ctypes.c_float * 1)()
        self._check(self._L.fslr_cluster_loci_timings(self._h, ms))
        return {'loci': float(ms[0])}

    # -- cluster junctions (fslr_hip.h fslr_cluster_junctions) ------------------------------------------
    def cluster_junctions(self, qkey, rev=None):
        """The junctions each cluster's reads support, from the resident loci rows (cluster_loci first):
        ``qkey`` (int32) and ``rev`` (uint8 or None = all forward) per CSR interval.  Returns ``(off
        int64[n_clusters + 1], locus_a, side_a, locus_b, side_b, n_obs, n_reads, bp_a_min, bp_a_max, bp_b_min,
        bp_b_max)``: loci as global row indices of cluster_loci (int32), sides uint8 (0 left, 1 right), rows
        ordered by (locus_a * 2 + side_a, locus_b * 2 + side_b)."""
        return self._cluster_junctions('fslr_cluster_junctions', qkey, rev)

    def cluster_junctions_any(self, qkey, rev=None):
        """cluster_junctions for a context that holds reads of more than 64 intervals (fslr_cluster_junctions_any):
        ``qkey`` and ``rev`` per interval of the real CSR, in its order (the order set_thresholds takes); a read's
        chain runs over all its intervals.  On a context without such reads it is cluster_junctions, byte for
        byte."""
        return self._cluster_junctions('fslr_cluster_junctions_any', qkey, rev)

    @staticmethod
    def _chain_columns(qkey, rev):
        """The two columns as the library takes them: int32 keys (values outside int32 are refused, not wrapped)
        and uint8 strand bits of the same shape."""
        q = np.asarray(qkey)
        if q.ndim != 1:
            raise ValueError('qkey must be one-dimensional')
        if q.dtype.kind not in 'iub':
            raise ValueError(f'qkey must hold integers, not {q.dtype}')
        if q.size and (int(q.min()) < -(1 << 31) or int(q.max()) >= (1 << 31)):
            raise ValueError('qkey must hold int32 values')
        q = np.ascontiguousarray(q, dtype=np.int32)
        if rev is not None:
            rev = np.ascontiguousarray(rev, dtype=np.uint8)
            if rev.shape != q.shape:
                raise ValueError('rev must have qkey\'s shape')
        return q, rev

    def _cluster_junctions(self, name, qkey, rev):
        call = getattr(self._L, name)
        if name.endswith('_any'):
            qkey, rev = self._chain_columns(qkey, rev)
        else:
            qkey = np.ascontiguousarray(qkey, dtype=np.int32)
            if qkey.ndim != 1:
                raise ValueError('qkey must be one-dimensional')
            if rev is not None:
                rev = np.ascontiguousarray(rev, dtype=np.uint8)
                if rev.shape != qkey.shape:
                    raise ValueError('rev must have qkey\'s shape')
        n = ctypes.c_int64(0)
        # (an empty array still passes an address: NULL keys are an error of their own)
        self._check(call(self._h, _ptr(qkey) if qkey.size else _ptr(np.zeros(1, np.int32)),
                         None if rev is None else _ptr(rev) if rev.size else _ptr(np.zeros(1, np.uint8)),
                         int(qkey.size), ctypes.byref(n)))
        nr = int(n.value)
        ci = getattr(self, '_cluster_info', None) or {'n_clusters': 0}
        off = np.zeros(ci['n_clusters'] + 1, np.int64)
        la, lb, n_obs, n_reads = (np.empty(nr, np.int32) for _ in range(4))
        sides, bp = np.empty(nr, np.uint8), np.empty((4, nr), np.int32)
        self._check(self._L.fslr_get_cluster_junctions(self._h, _ptr(off), _ptr(la), _ptr(lb), _ptr(sides), _ptr(n_obs),
                                                       _ptr(n_reads), _ptr(bp), nr))
        return (off, la, sides & 1, lb, sides >> 1, n_obs, n_reads, bp[0], bp[1], bp[2], bp[3])

    def cluster_junctions_timings(self) -> dict:
        """HIP-event time (ms) of the last cluster_junctions, uploads excluded (profiling contexts)."""
        ms = (ctypes.c_float * 1)()
        self._check(self._L.fslr_cluster_junctions_timings(self._h, ms))
        return {'junctions': float(ms[0])}

    # -- cluster paths (fslr_hip.h fslr_cluster_paths) --------------------------------------------------
    def cluster_paths(self, qkey, rev=None):
        """The distinct read structures of each cluster, from the resident loci rows (cluster_loci first):
        ``qkey`` (int32) and ``rev`` (uint8 or None = all forward) per CSR interval.  Returns ``(off
        int64[n_clusters + 1], tok_off int64[n_rows + 1], n_reads, first_read, locus, rev, path_of_read,
        flipped)``: a row's tokens are ``locus`` (global row indices of cluster_loci, int32) and ``rev`` (uint8)
        at ``tok_off[row]:tok_off[row + 1]``; ``path_of_read`` (int32, -1 for a read alone) and ``flipped``
        (uint8) are per read; rows ascend lexicographically by their tokens ``locus * 2 + rev``."""
        return self._cluster_paths('fslr_cluster_paths', qkey, rev)

    def cluster_paths_any(self, qkey, rev=None):
        """cluster_paths for a context that holds reads of more than 64 intervals (fslr_cluster_paths_any): ``qkey``
        and ``rev`` per interval of the real CSR, in its order; ``path_of_read`` and ``flipped`` are per real read.
        On a context without such reads it is cluster_paths, byte for byte."""
        return self._cluster_paths('fslr_cluster_paths_any', qkey, rev)

    def _n_real_reads(self) -> int:
        """The reads the per-read outputs of a successful cluster_paths* have: the table's n (the library checked
        it against the context's real read count; ``n_reads`` counts the chunks of long reads too)."""
        ci = getattr(self, '_cluster_info', None)
        return int(ci['n']) if ci else int(self.n_reads)

    def _cluster_paths(self, name, qkey, rev):
        call = getattr(self._L, name)
        if name.endswith('_any'):
            qkey, rev = self._chain_columns(qkey, rev)
        else:
            qkey = np.ascontiguousarray(qkey, dtype=np.int32)
            if qkey.ndim != 1:
                raise ValueError('qkey must be one-dimensional')
            if rev is not None:
                rev = np.ascontiguousarray(rev, dtype=np.uint8)
                if rev.shape != qkey.shape:
                    raise ValueError('rev must have qkey\'s shape')
        nr, nt = ctypes.c_int64(0), ctypes.c_int64(0)
        # (an empty array still passes an address: NULL keys are an error of their own)
        self._check(call(self._h, _ptr(qkey) if qkey.size else _ptr(np.zeros(1, np.int32)),
                         None if rev is None else _ptr(rev) if rev.size else _ptr(np.zeros(1, np.uint8)),
                         int(qkey.size), ctypes.byref(nr), ctypes.byref(nt)))
        nr, nt, n = int(nr.value), int(nt.value), self._n_real_reads()
        self._n_path_rows = nr                     # cluster_path_containment sizes its per-row outputs by it
        ci = getattr(self, '_cluster_info', None) or {'n_clusters': 0}
        off, tok_off = np.zeros(ci['n_clusters'] + 1, np.int64), np.zeros(nr + 1, np.int64)
        n_reads, first_read, locus, path = (np.empty(k, np.int32) for k in (nr, nr, nt, n))
        trev, flipped = np.empty(nt, np.uint8), np.empty(n, np.uint8)
        self._check(self._L.fslr_get_cluster_paths(self._h, _ptr(off), _ptr(tok_off), _ptr(n_reads), _ptr(first_read),
                                                   _ptr(locus), _ptr(trev), _ptr(path), _ptr(flipped), nr, nt))
        return (off, tok_off, n_reads, first_read, locus, trev, path, flipped)

    def cluster_paths_timings(self) -> dict:
        """HIP-event time (ms) of the last cluster_paths, uploads excluded (profiling contexts)."""
        ms = (ctypes.c_float * 1)()
        self._check(self._L.fslr_cluster_paths_timings(self._h, ms))
        return {'paths': float(ms[0])}

    # -- path segments (fslr_hip.h fslr_cluster_path_segments) ------------------------------------------
    def cluster_path_segments(self, qkey, qend=None):
        """Consensus coordinates and junction gaps per slot of the resident path rows (cluster_paths first, with the
        same ``qkey``): ``qkey`` and ``qend`` (int32, or None = no gaps, the gap columns all 0) per CSR interval.
        Returns nine int32 columns of n_tokens each, in the slots' order (``tok_off`` of cluster_paths):
        ``(start_min, start_med, start_max, end_min, end_med, end_max, gap_min, gap_med, gap_max)``; the medians are
        lower medians, a gap is stored at the earlier of the two slots it joins and a row's last slot holds 0."""
        return self._cluster_path_segments('fslr_cluster_path_segments', qkey, qend)

    def cluster_path_segments_any(self, qkey, qend=None):
        """cluster_path_segments for a context that holds reads of more than 64 intervals
        (fslr_cluster_path_segments_any; cluster_paths_any first): ``qkey`` and ``qend`` per interval of the real CSR,
        in its order.  On a context without such reads it is cluster_path_segments, byte for byte."""
        return self._cluster_path_segments('fslr_cluster_path_segments_any', qkey, qend)

    def _cluster_path_segments(self, name, qkey, qend):
        qkey = np.ascontiguousarray(qkey, dtype=np.int32)
        if qkey.ndim != 1:
            raise ValueError('qkey must be one-dimensional')
        if qend is not None:
            qend = np.ascontiguousarray(qend, dtype=np.int32)
            if qend.shape != qkey.shape:
                raise ValueError('qend must have qkey\'s shape')
        nt = ctypes.c_int64(0)
        # (an empty array still passes an address: NULL keys are an error of their own)
        self._check(getattr(self._L, name)(
            self._h, _ptr(qkey) if qkey.size else _ptr(np.zeros(1, np.int32)),
            None if qend is None else _ptr(qend) if qend.size else _ptr(np.zeros(1, np.int32)), int(qkey.size), ctypes.byref(nt)))
        nt = int(nt.value)
        start, end, gap = (np.empty((3, nt), np.int32) for _ in range(3))
        self._check(self._L.fslr_get_cluster_path_segments(self._h, _ptr(start), _ptr(end), _ptr(gap), nt))
        return (start[0], start[1], start[2], end[0], end[1], end[2], gap[0], gap[1], gap[2])

    def cluster_path_segments_timings(self) -> dict:
        """HIP-event time (ms) of the last cluster_path_segments, uploads excluded (profiling contexts)."""
        ms = (ctypes.c_float * 1)()
        self._check(self._L.fslr_cluster_path_segments_timings(self._h, ms))
        return {'segments': float(ms[0])}

    # -- path containment (fslr_hip.h fslr_cluster_path_containment) ------------------------------------
    def cluster_path_containment(self):
        """Which of the resident path rows (cluster_paths / cluster_paths_any first) are contiguous sub-chains of a
        longer row of their cluster, in either reading direction, and each row's support with them counted.
        Nothing is uploaded.  Returns ``(coff int64[n_rows + 1], outer int32, offset int32, rev uint8, n_occ int32,
        n_inner int32, support int64, collapse_to int32, collapsed_reads int64)``: the pairs of inner row A are
        ``coff[A]:coff[A + 1]`` of the four pair columns, the last four columns are per path row."""
        n = ctypes.c_int64(0)
        self._check(self._L.fslr_cluster_path_containment(self._h, ctypes.byref(n)))
        # the per-row outputs are sized by the rows this context's last cluster_paths* made; the library refuses a
        # smaller capacity than its own row count, and a larger one is cut back below
        npairs, n_rows = int(n.value), int(getattr(self, '_n_path_rows', 0))
        coff = np.full(n_rows + 1, -1, np.int64)
        outer, offset, n_occ = (np.empty(npairs, np.int32) for _ in range(3))
        rev = np.empty(npairs, np.uint8)
        n_inner, collapse_to = np.empty(n_rows, np.int32), np.empty(n_rows, np.int32)
        support, collapsed = np.empty(n_rows, np.int64), np.empty(n_rows, np.int64)
        self._check(self._L.fslr_get_cluster_path_containment(
            self._h, _ptr(coff), _ptr(outer), _ptr(offset), _ptr(rev), _ptr(n_occ), _ptr(n_inner), _ptr(support),
            _ptr(collapse_to), _ptr(collapsed), n_rows, npairs))
        have = int((coff >= 0).sum()) - 1                # the library wrote coff[0 .. its rows]: offsets, never negative
        if have != n_rows:                               # (path rows made past this wrapper): keep what was written
            coff, n_inner, support = coff[:have + 1], n_inner[:have], support[:have]
            collapse_to, collapsed = collapse_to[:have], collapsed[:have]
        return (coff, outer, offset, rev, n_occ, n_inner, support, collapse_to, collapsed)

    def cluster_path_containment_timings(self) -> dict:
        """HIP-event time (ms) of the last cluster_path_containment (profiling contexts)."""
        ms = (ctypes.c_float * 1)()
        self._check(self._L.fslr_cluster_path_containment_timings(self._h, ms))
        return {'containment': float(ms[0])}

    # -- collapsed path segments (fslr_hip.h fslr_cluster_collapsed_segments) ---------------------------
    def cluster_collapsed_segments(self, qkey, qend=None):
        """Consensus coordinates and junction gaps per slot of every maximal path row, over all reads that collapse
        onto it (cluster_paths and cluster_path_containment first, the paths made with the same ``qkey``): ``qkey``
        and ``qend`` (int32, or None = no gaps, the gap columns all 0) per CSR interval.  Returns eleven int32
        columns of n_tokens each, in the slots' order (``tok_off`` of cluster_paths): ``(n_cov, n_link, start_min,
        start_med, start_max, end_min, end_med, end_max, gap_min, gap_med, gap_max)``; ``n_cov`` intervals and
        ``n_link`` read links stand behind a slot, the medians are lower medians, and the slots of rows that are not
        maximal hold 0."""
        return self._cluster_collapsed_segments('fslr_cluster_collapsed_segments', qkey, qend)

    def cluster_collapsed_segments_any(self, qkey, qend=None):
        """cluster_collapsed_segments for a context that holds reads of more than 64 intervals
        (fslr_cluster_collapsed_segments_any; cluster_paths_any first): ``qkey`` and ``qend`` per interval of the real
        CSR, in its order.  On a context without such reads it is cluster_collapsed_segments, byte for byte."""
        return self._cluster_collapsed_segments('fslr_cluster_collapsed_segments_any', qkey, qend)

    def _cluster_collapsed_segments(self, name, qkey, qend):
        qkey = np.ascontiguousarray(qkey, dtype=np.int32)
        if qkey.ndim != 1:
            raise ValueError('qkey must be one-dimensional')
        if qend is not None:
            qend = np.ascontiguousarray(qend, dtype=np.int32)
            if qend.shape != qkey.shape:
                raise ValueError('qend must have qkey\'s shape')
        nt = ctypes.c_int64(0)
        # (an empty array still passes an address: NULL keys are an error of their own)
        self._check(getattr(self._L, name)(
            self._h, _ptr(qkey) if qkey.size else _ptr(np.zeros(1, np.int32)),
            None if qend is None else _ptr(qend) if qend.size else _ptr(np.zeros(1, np.int32)), int(qkey.size), ctypes.byref(nt)))
        nt = int(nt.value)
        n_cov, n_link = np.empty(nt, np.int32), np.empty(nt, np.int32)
        start, end, gap = (np.empty((3, nt), np.int32) for _ in range(3))
        self._check(self._L.fslr_get_cluster_collapsed_segments(self._h, _ptr(n_cov), _ptr(n_link), _ptr(start), _ptr(end),
                                                                _ptr(gap), nt))
        return (n_cov, n_link, start[0], start[1], start[2], end[0], end[1], end[2], gap[0], gap[1], gap[2])

    def cluster_collapsed_segments_timings(self) -> dict:
        """HIP-event time (ms) of the last cluster_collapsed_segments, uploads excluded (profiling contexts)."""
        ms = (ctypes.c_float * 1)()
        self._check(self._L.fslr_cluster_collapsed_segments_timings(self._h, ms))
        return {'collapsed': float(ms[0])}
