// idxsearch.hpp — the built index as an interval search reads it (search.hip's batch of queries,
// match.hip's query reads): the span of a query, the hit test, the re-rank of equal starts, the map
// from a stored interval's tag to its ids, and the host side that assembles the view.
//
// A query (c, qs, qe) hits a stored interval (chrom, start, end) iff chrom == c, start <= qe and
// end >= qs.  Its hits lie in a span [lo, hi) of index positions and come in descending position of
// the order (start ascending, end descending, data position ascending); the index itself keeps ties
// of equal (chrom, start) in index order.
#pragma once
#include <string>

#include "ctx.hpp"
#include "fslr_hip.h"
#include "kernels.hpp"

namespace fslr {

constexpr int kTile = 256;             // index.hip: pmax tiles
constexpr int kGroup = 1024;           // index.hip: tiles per scan group

struct IndexView {
  const int2* crange;
  const int* s_start;
  const unsigned long long* endkey;
  // index.hip's tile prefix: pmaxkey = tile maxima [0, nt), local group prefixes [nt, 2 nt), exclusive
  // group prefixes [2 nt, 2 nt + ng)
  const unsigned long long* loc;
  const unsigned long long* group_excl;
  const int4* idx4;
  const int4* rmeta;
  const int* data_pos;                 // null: the data position is the uploaded CSR index
  const int* perm;                     // null, or virtual -> real interval (fslr_set_reads_any)
  // ni: positions of the index, and the bound of an uploaded CSR index too: the two counts differ only
  // under a filter, which search_state refuses
  int nt, ni, n, n_chroms;

  // the inclusive prefix max of (chrom, end) of tile t
  __device__ __forceinline__ unsigned long long incl(int t) const {
    FSLR_BOUND(t, nt);
    const unsigned long long a = group_excl[t / kGroup], b = loc[t];
    return a > b ? a : b;
  }

  // the end at position p reaches qs: with start <= qe (every position of a span), a hit
  __device__ __forceinline__ bool reaches(long long p, int qs) const {
    FSLR_BOUND(p, ni);
    return static_cast<int>(static_cast<unsigned>(endkey[p])) >= qs;
  }

  // [lo, hi) of query (c, qs, qe), qs >= 0: hi = upper bound of qe in the chromosome's starts; lo = the
  // first position of the chromosome whose end reaches qs.  Every hit lies in it; a position of it is a
  // hit iff reaches(p, qs).
  __device__ __forceinline__ int2 span_of(int c, int qs, int qe) const {
    int lo = 0, hi = 0;
    if (c >= 0 && c < n_chroms) {
      const int2 cr = crange[c];
      int a = cr.x, z = cr.y;                      // first position of the chromosome with start > qe
      while (a < z) {
        const int mid = (a + z) >> 1;
        FSLR_BOUND(mid, ni);
        if (s_start[mid] <= qe) a = mid + 1; else z = mid;
      }
      lo = hi = a;
      if (hi > cr.x) {
        // positions before cr.x hold smaller chromosomes, so their keys stay below (c, qs): the first
        // tile from the chromosome's whose inclusive prefix reaches the key holds the first such end
        const unsigned long long key = (static_cast<unsigned long long>(c) << 32) | static_cast<unsigned>(qs);
        int tb = cr.x / kTile, te = (hi - 1) / kTile;
        if (incl(te) >= key) {
          while (tb < te) {
            const int mid = (tb + te) >> 1;
            if (incl(mid) >= key) te = mid; else tb = mid + 1;
          }
          int p = max(tb * kTile, cr.x);
          const int pe = min((tb + 1) * kTile, hi);
          for (; p < pe; ++p)
            if (reaches(p, qs)) break;
          lo = p;
        }
      }
    }
    return make_int2(lo, hi);
  }

  // {the uploaded CSR's index, the data position} of the stored interval with tag read << 6 | j; kPerm = false
  // (match.hip, which refuses virtual reads): perm is null and is not looked at
  template <bool kPerm>
  __device__ __forceinline__ int2 ids(int tag) const {
    FSLR_BOUND(tag >> 6, n);
    const int kv = rmeta[tag >> 6].x + (tag & 63);
    FSLR_BOUND(kv, ni);
    const int k = kPerm && perm ? perm[kv] : kv;
    return make_int2(k, data_pos ? data_pos[kv] : k);
  }

  // the hit at position p of span sp, of start `start`, has an equal-start neighbour in the span
  __device__ __forceinline__ bool tied(int2 sp, int p, int start) const {
    return (p > sp.x && s_start[p - 1] == start) || (p + 1 < sp.y && s_start[p + 1] == start);
  }

  // what a tied hit at position p (record rec, data position me) of span sp adds to its ascending rank
  // among the span's hits in index order
  template <bool kPerm>
  __device__ __forceinline__ int tie_shift(int2 sp, int p, int4 rec, int qs, int me) const {
    // the run of equal start inside the span: the hits of it before p leave the rank, those that
    // precede p in (end descending, data position ascending) enter it
    int rb = p;
    while (rb > sp.x && s_start[rb - 1] == rec.x) --rb;
    int before = 0, first = 0;
    for (int f = rb; f < sp.y; ++f) {
      FSLR_BOUND(f, ni);
      const int4 rf = idx4[f];
      if (rf.x != rec.x) break;
      if (rf.y < qs || f == p) continue;
      before += f < p;
      first += rf.y > rec.y || (rf.y == rec.y && ids<kPerm>(rf.w).y < me);
    }
    return first - before;
  }
};

// the view of c's index (built, ensure_bwd_ranges done); perm: the device copy of lg_perm, or null
inline IndexView index_view(const fslr_ctx* c, const int* perm) {
  const int ni = static_cast<int>(c->ni_idx);
  const int nt = (ni + kTile - 1) / kTile;
  return IndexView{c->crange, c->s_start, c->endkey, c->pmaxkey + nt, c->pmaxkey + 2 * static_cast<size_t>(nt),
                   c->idx4, c->rmeta, c->have_data_pos ? c->data_pos : nullptr, perm,
                   nt, ni, static_cast<int>(c->n), c->n_chroms};
}

// why this context's index cannot answer a search (it is missing or partial), or FSLR_OK
inline int search_state(fslr_ctx* c, const char* who) {
  const std::string f = std::string(who) + ": ";
  if (!c->index_built) return fail(c, FSLR_ERR_STATE, f + "fslr_build_index first");
  if (c->filter_active)
    return fail(c, FSLR_ERR_STATE, f + "a chromosome or position filter is active (the index is partial)");
  if (c->n_shards > 1 || c->built_n_shards > 1)
    return fail(c, FSLR_ERR_STATE, f + "the index was built for one of several shards (it is partial)");
  return FSLR_OK;
}

// blocks of four wavefronts for `waves` wavefronts of work
inline int wave_grid(long long waves) { return grid_for(waves, 4, 256 * 32); }

}  // namespace fslr
