"""The plain statement of the collapsed path segments (include/fslr_hip.h fslr_cluster_collapsed_segments), on the
host, on top of tests/paths_ref.py and tests/containment_ref.py.

A clustered read r of row A = path_of_read[r] with a intervals has the chain of tests/segments_ref.py: its intervals
ordered by (query key, CSR position); the interval at chain rank t has the canonical position p = a - 1 - t when the
read is flipped, else t.  With B = collapse_to[A]: q = p when B == A; otherwise the pair (A, B) of the containment rows
gives its offset o and direction d, and q = o + (a - 1 - p) when d else o + p.  The interval lands in slot
tok_off[B] + q; the link between ranks t and t + 1 at slot tok_off[B] + min(q_t, q_t+1), its gap being the query key of
the later interval in the read's own chain order minus the query end of the earlier one, clamped to int32.  Per slot:
n_cov intervals, n_link links, and min, lower median and max (segments_ref.three) of the starts, the ends and the
gaps.  Without ``qend`` every gap is 0 and n_link is still counted.  tests/test_collapsed_ref.py pins it to hand-worked
cases.
"""
import numpy as np

import segments_ref

NAMES = ('n_cov', 'n_link') + segments_ref.NAMES
I32_MIN, I32_MAX = segments_ref.I32_MIN, segments_ref.I32_MAX


def row_map(cont, A):
    """(B, o, d) of row ``A``: the row it collapses to, and where and in which direction it lies there."""
    B = int(cont['collapse_to'][A])
    if B == A:
        return B, 0, 0
    at = [k for k in range(int(cont['coff'][A]), int(cont['coff'][A + 1])) if int(cont['outer'][k]) == B]
    assert len(at) == 1, 'collapse_to is one of the rows that contain A'
    return B, int(cont['offset'][at[0]]), int(cont['rev'][at[0]])


def collapsed(read_off, iv_start, iv_end, paths, cont, qkey, qend=None):
    """The eleven int32 columns as a dict (NAMES) for ``paths`` (paths_ref.paths' result, made with ``qkey``) and
    ``cont`` (containment_ref.containment's result for them)."""
    read_off = np.asarray(read_off, np.int64)
    tok_off = np.asarray(paths['tok_off'], np.int64)
    n_tokens = int(tok_off[-1])
    starts, ends, gaps = ([[] for _ in range(n_tokens)] for _ in range(3))
    n_link = np.zeros(n_tokens, np.int32)
    for r in range(read_off.shape[0] - 1):
        A = int(paths['path_of_read'][r])
        if A < 0:
            continue
        ks = sorted(range(int(read_off[r]), int(read_off[r + 1])), key=lambda k: (int(qkey[k]), k))
        a = len(ks)
        assert a == int(tok_off[A + 1] - tok_off[A])
        B, o, d = row_map(cont, A)
        pos = [a - 1 - t if paths['flipped'][r] else t for t in range(a)]
        q = [o + (a - 1 - p) if d else o + p for p in pos]
        assert 0 <= min(q) and max(q) < int(tok_off[B + 1] - tok_off[B])
        base = int(tok_off[B])
        for t, k in enumerate(ks):
            starts[base + q[t]].append(int(iv_start[k]))
            ends[base + q[t]].append(int(iv_end[k]))
            if t + 1 < a:
                s = base + min(q[t], q[t + 1])
                n_link[s] += 1
                if qend is not None:
                    gap = int(qkey[ks[t + 1]]) - int(qend[k])
                    gaps[s].append(max(I32_MIN, min(I32_MAX, gap)))
    out = {k: np.zeros(n_tokens, np.int32) for k in NAMES}
    out['n_link'] = n_link
    for s in range(n_tokens):
        out['n_cov'][s] = len(starts[s])
        for name, lists in (('start', starts), ('end', ends), ('gap', gaps)):
            if lists[s]:
                out[name + '_min'][s], out[name + '_med'][s], out[name + '_max'][s] = segments_ref.three(lists[s])
    return out


def collapsed_of_csr(csr, paths, cont, qkey, qend=None):
    """collapsed() for a prep.CSR."""
    return collapsed(csr.read_off, csr.iv_start, csr.iv_end, paths, cont, qkey, qend)
