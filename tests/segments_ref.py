"""The plain statement of the path segments (include/fslr_hip.h fslr_cluster_path_segments), on the host, on top of
tests/paths_ref.py.

A clustered read's chain is its intervals ordered by (query key, CSR position).  The interval at chain rank t of a
read of L intervals has canonical position p = L - 1 - t when the read is flipped, else t, and lands in slot
tok_off[path_of_read[r]] + p.  Per slot, over the intervals that land in it: min, lower median (sorted()[(k - 1) // 2])
and max of the reference starts and of the ends.  Per link between slots s and s + 1 of a row, stored at s: the same of
the reads' gaps there, a gap being the query key of the later interval in the read's own chain order minus the query
end of the earlier one, clamped to int32.  A row's last slot has gap 0, 0, 0; without ``qend`` every gap is 0.
tests/test_segments_ref.py pins it to hand-worked cases.
"""
import numpy as np

import paths_ref

NAMES = ('start_min', 'start_med', 'start_max', 'end_min', 'end_med', 'end_max', 'gap_min', 'gap_med', 'gap_max')
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def three(values):
    v = sorted(values)
    return v[0], v[(len(v) - 1) // 2], v[-1]


def segments(read_off, iv_start, iv_end, paths, qkey, qend=None):
    """The nine int32 columns as a dict (NAMES) for ``paths`` (paths_ref.paths' result, made with ``qkey``)."""
    read_off = np.asarray(read_off, np.int64)
    n_tokens = int(paths['tok_off'][-1])
    starts, ends, gaps = ([[] for _ in range(n_tokens)] for _ in range(3))
    for r in range(read_off.shape[0] - 1):
        row = int(paths['path_of_read'][r])
        if row < 0:
            continue
        ks = sorted(range(int(read_off[r]), int(read_off[r + 1])), key=lambda k: (int(qkey[k]), k))
        L, base = len(ks), int(paths['tok_off'][row])
        assert L == int(paths['tok_off'][row + 1]) - base
        pos = [L - 1 - t if paths['flipped'][r] else t for t in range(L)]
        for t, k in enumerate(ks):
            starts[base + pos[t]].append(int(iv_start[k]))
            ends[base + pos[t]].append(int(iv_end[k]))
            if qend is not None and t + 1 < L:
                gap = int(qkey[ks[t + 1]]) - int(qend[k])
                gaps[base + min(pos[t], pos[t + 1])].append(max(I32_MIN, min(I32_MAX, gap)))
    out = {k: np.zeros(n_tokens, np.int32) for k in NAMES}
    for s in range(n_tokens):
        for name, lists in (('start', starts), ('end', ends), ('gap', gaps)):
            if lists[s]:
                out[name + '_min'][s], out[name + '_med'][s], out[name + '_max'][s] = three(lists[s])
    return out


def segments_of_csr(csr, labels, qkey, qend=None, rev=None):
    """(paths_ref.paths_of_csr's result, segments()) for a prep.CSR and min-rank labels."""
    p = paths_ref.paths_of_csr(csr, labels, qkey, rev)
    return p, segments(csr.read_off, csr.iv_start, csr.iv_end, p, qkey, qend)
