"""The numpy statement of fslr_append_reads_any / fslr_remove_reads_any: the virtual layout and
the maps after an append and after a removal, from the real reads' lengths alone.

A read of L intervals is L consecutive real intervals; the virtual layout (fslr_set_reads_any) gives every real
read one first chunk of min(L, 64) intervals at virtual rank = its real rank, and its further 64-interval chunks
ranks behind all first chunks, in real-rank then chunk order; the virtual CSR rows follow the virtual ranks.
Everything here is written with plain loops over reads and chunks, on purpose unlike prep.split_long_reads'
sort, which tests/test_append_any_ref.py pins it to."""
import numpy as np

MAX_L = 64


def virtual_layout(lens):
    """(vreal, vbase, vlen, rows, off2) of the real lengths ``lens``: per virtual read its real read, the index
    of its first interval there and its length; rows[k] = the real interval (index into the real CSR) at
    virtual CSR row k; off2[r] = the virtual CSR row of real read r's interval 64 (-1 for a short read)."""
    lens = [int(x) for x in lens]
    real_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    vreal, vbase, vlen = [], [], []
    for r, L in enumerate(lens):
        vreal.append(r), vbase.append(0), vlen.append(min(L, MAX_L))
    for r, L in enumerate(lens):
        for base in range(MAX_L, L, MAX_L):
            vreal.append(r), vbase.append(base), vlen.append(min(L - base, MAX_L))
    rows, off2 = [], np.full(len(lens), -1, np.int64)
    for r, base, n in zip(vreal, vbase, vlen):
        if base == MAX_L:
            off2[r] = len(rows)
        rows.extend(range(int(real_off[r]) + base, int(real_off[r]) + base + n))
    return (np.asarray(vreal, np.int64), np.asarray(vbase, np.int64), np.asarray(vlen, np.int64),
            np.asarray(rows, np.int64), off2)


def shape(res_lens, new_lens):
    """The eight numbers any_idx.hpp's Shape holds."""
    r, b = np.asarray(res_lens, np.int64), np.asarray(new_lens, np.int64)
    extra = lambda L: int(np.maximum((L + MAX_L - 1) // MAX_L - 1, 0).sum())
    return dict(n=int(r.size), V=int(r.size) + extra(r), o1=int(np.minimum(r, MAX_L).sum()), ni=int(r.sum()),
                m=int(b.size), e=extra(b), mi1=int(np.minimum(b, MAX_L).sum()), mi=int(b.sum()))


def append_layout(res_lens, new_lens):
    """The union's virtual layout in terms of the two sides' own layouts: ``rank_src[u]`` / ``row_src[k]`` = the
    resident virtual rank / row (>= 0) or ~(the batch's virtual rank / row) the union's rank u / row k holds;
    ``new_vrank`` / ``new_row`` = where each resident virtual rank / row goes; and the union's vreal, vbase,
    rlen, off2."""
    res_lens, new_lens = [int(x) for x in res_lens], [int(x) for x in new_lens]
    n, ni = len(res_lens), sum(res_lens)
    rv, rb, _, rrows, _ = virtual_layout(res_lens)
    bv, bb, _, brows, _ = virtual_layout(new_lens)
    uv, ub, ulen, urows, uoff2 = virtual_layout(res_lens + new_lens)
    where = {(int(r), int(b)): v for v, (r, b) in enumerate(zip(rv, rb))}
    where.update({(n + int(r), int(b)): ~v for v, (r, b) in enumerate(zip(bv, bb))})
    rank_src = np.asarray([where[(int(r), int(b))] for r, b in zip(uv, ub)], np.int64)
    row_of = {int(x): k for k, x in enumerate(rrows)}
    row_of.update({ni + int(x): ~k for k, x in enumerate(brows)})
    row_src = np.asarray([row_of[int(x)] for x in urows], np.int64)
    new_vrank = np.empty(rv.size, np.int64)
    new_vrank[rank_src[rank_src >= 0]] = np.flatnonzero(rank_src >= 0)
    new_row = np.empty(rrows.size, np.int64)
    new_row[row_src[row_src >= 0]] = np.flatnonzero(row_src >= 0)
    return dict(rank_src=rank_src, row_src=row_src, new_vrank=new_vrank, new_row=new_row, vreal=uv, vbase=ub,
                vlen=ulen, rlen=np.asarray(res_lens + new_lens, np.int64), off2=uoff2, rows=urows)


def remove_layout(res_lens, keep):
    """The survivors' virtual layout: ``new_vrank[v]`` of every old virtual rank (-1 removed), ``new_rank[r]`` of
    every old real rank, ``row_src[k]`` = the old virtual row at the survivors' row k, and their vreal, vbase,
    rlen, off2."""
    res_lens = [int(x) for x in res_lens]
    keep = np.asarray(keep, bool)
    rv, rb, _, rrows, _ = virtual_layout(res_lens)
    kept = [L for L, k in zip(res_lens, keep) if k]
    sv, sb, slen, srows, soff2 = virtual_layout(kept)
    new_rank = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int64)
    where = {(int(new_rank[r]), int(b)): v for v, (r, b) in enumerate(zip(rv, rb)) if keep[r]}
    src_v = np.asarray([where[(int(r), int(b))] for r, b in zip(sv, sb)], np.int64)
    new_vrank = np.full(rv.size, -1, np.int64)
    new_vrank[src_v] = np.arange(sv.size)
    real_off = np.concatenate([[0], np.cumsum(res_lens)]).astype(np.int64)
    kept_off = np.concatenate([[0], np.cumsum(kept)]).astype(np.int64)
    old_real = np.flatnonzero(keep)
    # the old real interval behind each surviving real interval, then the old virtual row that held it
    r_of = np.repeat(np.arange(len(kept)), kept)
    old_iv = real_off[old_real[r_of]] + (np.arange(int(kept_off[-1])) - kept_off[r_of])
    row_of = {int(x): k for k, x in enumerate(rrows)}
    row_src = np.asarray([row_of[int(old_iv[x])] for x in srows], np.int64)
    return dict(new_vrank=new_vrank, new_rank=new_rank, row_src=row_src, vreal=sv, vbase=sb, vlen=slen,
                rlen=np.asarray(kept, np.int64), off2=soff2, rows=srows)
