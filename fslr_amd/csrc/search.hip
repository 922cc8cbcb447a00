// search.hip — batched interval search on the built index (replaces the candidate search the
// reference's pair loop makes per interval, cluster.py:201: tree[chrom].search_values(start, end) of
// the superintervals IntervalMap that build_interval_trees makes, cluster.py:124-130).
//
// A query (c, qs, qe) hits a stored interval (chrom, start, end) iff chrom == c, start <= qe and
// end >= qs (end-inclusive; no order of qs / qe assumed).  Its hits come in descending position of
// the order (start ascending, end descending, data position ascending): the stand-in's search order
// (tests/golden/refharness.py), the one the edge-cap replay walks (cap.hip).  Data position =
// iv_data_pos[k] where the reads came with it, else the CSR index k.
//
// Passes (the index parts are those of index.hip; the tile prefix and the (chrom, end) keys come from
// ensure_bwd_ranges on the first search of an index generation, never from fslr_build_index; a query's
// span, the hit test and the re-rank of equal starts are IndexView's, idxsearch.hpp, as match.hip's are):
//   span    one lane per query: hi = upper bound of qe in the chromosome's starts; lo = the first
//           position of the chromosome whose end reaches qs: the first 256-position tile whose
//           prefix max of (chrom, end) reaches (c, qs) (binary search), then the first such end in
//           it.  Every hit lies in [lo, hi); a position of it is a hit iff end >= qs.
//   scan    spans are cut into pieces of 64 positions (exclusive scan of the piece counts), and a
//           max-scan of the pieces' head marks gives every piece its query: one long stored interval
//           drags lo back across many tiles, so the work is split by span position, not by query
//   count   one wavefront per piece: ballot of end >= qs; the piece's hit count
//   scan    exclusive scan of the piece counts (int64): a piece's, and so a query's, output offset
//   fill    one wavefront per piece: a hit's ascending rank is its piece's offset plus its lane rank,
//           and it is written top-down into its query's segment.  The index keeps ties of equal
//           (chrom, start) in index order, so a hit with an equal-start neighbour is re-ranked inside
//           its run on (end descending, data position ascending).  Every output slot is a function of
//           the input alone: no atomics, the same bytes on every run.
// Algorithmic bytes: span 12 B in + 16 B out per query and ~2 log2 probes; count 8 B
// per span position; fill 16 B per span position, 16 B (the read's CSR offset) + 4 B out per hit.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>
#include <string>

#include "ctx.hpp"
#include "fslr_hip.h"
#include "idxsearch.hpp"
#include "kernels.hpp"
#include "wave.hpp"

using namespace fslr;

// the search's buffers (grow only) and the last search's state (what fslr_search_hits fills from)
struct SearchWork {
  int* q3 = nullptr;                 // [3 x q_cap] the queries' chrom, start, end as uploaded
  int2* span = nullptr;              // [q_cap] {lo, hi}
  long long* npc = nullptr;          // [q_cap + 1] pieces per query (0 at nq)
  long long* poff = nullptr;         // [q_cap + 1] their exclusive scan
  long long* off = nullptr;          // [q_cap + 1] hit offsets
  int64_t q_cap = 0;
  int* pqh = nullptr;                // [p_cap] the queries at their head pieces, 0 elsewhere
  int* pq = nullptr;                 // [p_cap] piece -> query (their max-scan)
  long long* pcnt = nullptr;         // [p_cap + 1] hits per piece (0 at np)
  long long* pscan = nullptr;        // [p_cap + 1] their exclusive scan
  int64_t p_cap = 0;
  int* hits = nullptr;               // [h_cap]
  int64_t h_cap = 0;
  void* temp = nullptr;
  size_t temp_bytes = 0;
  int* perm = nullptr;               // fslr_set_reads_any: virtual -> real interval (lg_perm), per reads_gen
  int64_t perm_cap = 0;
  uint64_t perm_gen = 0;
  long long* pin = nullptr;          // [2] pinned: piece total, hit total
  // the last search
  bool valid = false;
  uint64_t reads_gen = 0, index_gen = 0;   // the reads and the index build it was made on
  int64_t nq = 0, np = 0, total = 0;
  // (profiling contexts) 0 span 1 piece scan 7 | the piece total's readback and the host's buffer growth,
  // not timed | 8 head marks + max-scan 2 count 3 hit scan + offsets 4, then 5 fill 6
  hipEvent_t ev[9] = {};
  bool ev_ok = false, ev_rec = false, ev_fill = false;
};

void fslr_search_free(fslr_ctx* c) {
  SearchWork* w = c->srw;
  if (!w) return;
  void* bufs[] = {w->q3, w->span, w->npc, w->poff, w->off, w->pqh, w->pq, w->pcnt, w->pscan, w->hits, w->temp, w->perm};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  if (w->pin) (void)hipHostFree(w->pin);
  if (w->ev_ok)
    for (hipEvent_t e : w->ev) (void)hipEventDestroy(e);
  delete w;
  c->srw = nullptr;
}

namespace {

constexpr int kPiece = 64;             // span positions per piece (one wavefront)

__global__ __launch_bounds__(256) void k_search_span(const int* __restrict__ qc, const int* __restrict__ qs_,
                                                     const int* __restrict__ qe_, long long nq, IndexView ix,
                                                     int2* __restrict__ span, long long* __restrict__ npc) {
  for (long long i = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x; i <= nq;
       i += static_cast<long long>(gridDim.x) * blockDim.x) {
    if (i == nq) {
      npc[nq] = 0;
      break;
    }
    const int2 sp = ix.span_of(qc[i], max(qs_[i], 0), qe_[i]);   // stored ends are >= 0: the same hits
    span[i] = sp;
    npc[i] = (static_cast<long long>(sp.y) - sp.x + kPiece - 1) / kPiece;
  }
}

// piece -> query: the head piece of every query with pieces is marked with the query; a max-scan
// carries the mark over the query's further pieces
__global__ __launch_bounds__(256) void k_search_heads(const long long* __restrict__ poff, long long nq, long long np,
                                                      int* __restrict__ pq) {
  for (long long i = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x; i < nq;
       i += static_cast<long long>(gridDim.x) * blockDim.x) {
    const long long g = poff[i];
    if (poff[i + 1] > g) {
      FSLR_BOUND(g, np);
      pq[g] = static_cast<int>(i);
    }
  }
}

__global__ __launch_bounds__(256) void k_search_count(const int* __restrict__ pq, const long long* __restrict__ poff,
                                                      const int2* __restrict__ span, const int* __restrict__ qs_,
                                                      IndexView ix, long long np, long long nq,
                                                      long long* __restrict__ pcnt) {
  const int lane = threadIdx.x & 63;
  const long long nw = static_cast<long long>(gridDim.x) * (blockDim.x >> 6);
  for (long long g = blockIdx.x * static_cast<long long>(blockDim.x >> 6) + (threadIdx.x >> 6); g <= np; g += nw) {
    if (g == np) {
      if (lane == 0) pcnt[np] = 0;
      break;
    }
    const int i = pq[g];
    FSLR_BOUND(i, nq);
    const int2 sp = span[i];
    const int qs = max(qs_[i], 0);
    const long long p = sp.x + (g - poff[i]) * kPiece + lane;
    const bool hit = p < sp.y && ix.reaches(p, qs);
    const unsigned long long hm = __ballot(hit);
    if (lane == 0) pcnt[g] = __popcll(hm);
  }
}

__global__ __launch_bounds__(256) void k_search_offsets(const long long* __restrict__ poff,
                                                        const long long* __restrict__ pscan, long long nq,
                                                        long long np, long long* __restrict__ off) {
  for (long long i = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x; i <= nq;
       i += static_cast<long long>(gridDim.x) * blockDim.x) {
    FSLR_BOUND(poff[i], np + 1);
    off[i] = pscan[poff[i]];
  }
}

__global__ __launch_bounds__(256) void k_search_fill(const int* __restrict__ pq, const long long* __restrict__ poff,
                                                     const long long* __restrict__ pscan,
                                                     const int2* __restrict__ span, const int* __restrict__ qs_,
                                                     IndexView ix, long long np, long long nq, long long total,
                                                     int* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long long nw = static_cast<long long>(gridDim.x) * (blockDim.x >> 6);
  for (long long g = blockIdx.x * static_cast<long long>(blockDim.x >> 6) + (threadIdx.x >> 6); g < np; g += nw) {
    const int i = pq[g];
    FSLR_BOUND(i, nq);
    const int2 sp = span[i];
    const int qs = max(qs_[i], 0);
    const long long g0 = poff[i], g1 = poff[i + 1];
    const long long p64 = sp.x + (g - g0) * kPiece + lane;
    bool hit = false;
    int4 rec = make_int4(0, 0, 0, 0);
    if (p64 < sp.y) {
      FSLR_BOUND(p64, ix.ni);
      rec = ix.idx4[p64];
      hit = rec.y >= qs;
    }
    const unsigned long long hm = __ballot(hit);
    if (!hit) continue;
    const int p = static_cast<int>(p64);
    const long long base = pscan[g0], cnt = pscan[g1] - base;
    long long r = pscan[g] - base + mbcnt(hm);   // ascending rank among the query's hits, ties in index order
    const int2 me = ix.ids<true>(rec.w);
    if (ix.tied(sp, p, rec.x)) r += ix.tie_shift<true>(sp, p, rec, qs, me.y);
    const long long dst = base + cnt - 1 - r;      // top-down
    FSLR_BOUND(dst, total);
    out[dst] = me.x;
  }
}

int ensure_queries(fslr_ctx* c, SearchWork* w, int64_t nq) {
  if (w->off && nq <= w->q_cap) return FSLR_OK;
  w->q_cap = 0;
  const int64_t cap = std::max<int64_t>(nq + nq / 4, 1024);
  int rc;
  if ((rc = dalloc(c, &w->q3, 3 * cap)) || (rc = dalloc(c, &w->span, cap)) || (rc = dalloc(c, &w->npc, cap + 1)) ||
      (rc = dalloc(c, &w->poff, cap + 1)) || (rc = dalloc(c, &w->off, cap + 1)))
    return rc;
  w->q_cap = cap;
  return FSLR_OK;
}

int ensure_temp(fslr_ctx* c, SearchWork* w, int64_t items) {
  size_t b1 = 0, b2 = 0;
  HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, b1, static_cast<long long*>(nullptr),
                                              static_cast<long long*>(nullptr), items, c->stream));
  HIP_TRY(c, hipcub::DeviceScan::InclusiveScan(nullptr, b2, static_cast<int*>(nullptr), static_cast<int*>(nullptr),
                                               hipcub::Max(), items, c->stream));
  const size_t need = std::max(b1, b2);
  if (need > w->temp_bytes) {
    if (w->temp) (void)hipFree(w->temp);
    w->temp = nullptr;
    w->temp_bytes = 0;
    HIP_TRY(c, hipMalloc(&w->temp, need));
    w->temp_bytes = need;
  }
  return FSLR_OK;
}

int ensure_pieces(fslr_ctx* c, SearchWork* w, int64_t np) {
  if (w->pscan && np <= w->p_cap) return FSLR_OK;
  w->p_cap = 0;                                   // (a failed growth leaves no buffer behind its capacity)
  const int64_t cap = std::max<int64_t>(np + np / 4, 4096);
  int rc;
  if ((rc = dalloc(c, &w->pqh, cap)) || (rc = dalloc(c, &w->pq, cap)) || (rc = dalloc(c, &w->pcnt, cap + 1)) || (rc = dalloc(c, &w->pscan, cap + 1)))
    return rc;
  w->p_cap = cap;
  return FSLR_OK;
}

}  // namespace

extern "C" {

int fslr_search(fslr_ctx* c, int64_t nq, const int32_t* chrom, const int32_t* start, const int32_t* end,
                int64_t* offsets, int64_t* n_hits) {
  if (!c) return FSLR_ERR_INVALID;
  if (nq < 0 || nq >= (int64_t(1) << 31) - 1) return fail(c, FSLR_ERR_INVALID, "fslr_search: query count out of range");
  if (nq && (!chrom || !start || !end)) return fail(c, FSLR_ERR_INVALID, "fslr_search: null query array");
  if (int rc = search_state(c, "fslr_search")) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  if (!c->srw) c->srw = new SearchWork();
  SearchWork* w = c->srw;
  w->valid = false;
  w->ev_rec = w->ev_fill = false;
  hipStream_t st = c->stream;
  const int ni = static_cast<int>(c->ni_idx);
  // no query, no interval or no span position: every count is 0 and nothing more runs on the device
  auto no_hits = [&]() {
    if (offsets) std::fill(offsets, offsets + nq + 1, int64_t(0));
    if (n_hits) *n_hits = 0;
    w->valid = true;
    w->reads_gen = c->reads_gen;
    w->index_gen = c->index_gen;
    w->nq = nq;
    w->np = w->total = 0;
    return FSLR_OK;
  };
  if (nq == 0 || ni == 0) return no_hits();
  // the tile prefix of end and the (chrom, end) keys of a sweep-only index, once per index
  if (int rc = ensure_bwd_ranges(c)) return rc;
  if (int rc = ensure_queries(c, w, nq)) return rc;
  if (int rc = ensure_temp(c, w, nq + 1)) return rc;
  if (!w->pin) HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&w->pin), 2 * sizeof(long long), hipHostMallocDefault));
  if (c->prof_phases && !w->ev_ok) {
    for (hipEvent_t& e : w->ev) HIP_TRY(c, hipEventCreate(&e));
    w->ev_ok = true;
  }
  const bool prof = c->prof_phases && w->ev_ok;
  int *qc = w->q3, *qs = w->q3 + w->q_cap, *qe = w->q3 + 2 * w->q_cap;
  const size_t qb = static_cast<size_t>(nq) * sizeof(int);
  HIP_TRY(c, hipMemcpyAsync(qc, chrom, qb, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(qs, start, qb, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(qe, end, qb, hipMemcpyHostToDevice, st));
  const IndexView ix = index_view(c, nullptr);
  if (prof) HIP_TRY(c, hipEventRecord(w->ev[0], st));
  k_search_span<<<grid_for(nq + 1), 256, 0, st>>>(qc, qs, qe, nq, ix, w->span, w->npc);
  HIP_TRY(c, hipGetLastError());
  if (prof) HIP_TRY(c, hipEventRecord(w->ev[1], st));
  size_t tb = w->temp_bytes;
  HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(w->temp, tb, w->npc, w->poff, nq + 1, st));
  if (prof) HIP_TRY(c, hipEventRecord(w->ev[7], st));
  HIP_TRY(c, hipMemcpyAsync(&w->pin[0], w->poff + nq, sizeof(long long), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  const int64_t np = w->pin[0];
  if (np >= (int64_t(1) << 31) - 1)
    return fail(c, FSLR_ERR_NOMEM, "fslr_search: the batch's spans hold " + std::to_string(np) +
                                       " 64-position pieces (limit 2^31): split the batch");
  if (np == 0) return no_hits();                 // every span is empty (the piece buffers may not exist yet)
  if (int rc = ensure_pieces(c, w, np)) return rc;
  if (int rc = ensure_temp(c, w, np + 1)) return rc;
  if (prof) HIP_TRY(c, hipEventRecord(w->ev[8], st));
  HIP_TRY(c, hipMemsetAsync(w->pqh, 0, static_cast<size_t>(np) * sizeof(int), st));
  k_search_heads<<<grid_for(nq), 256, 0, st>>>(w->poff, nq, np, w->pqh);
  HIP_TRY(c, hipGetLastError());
  tb = w->temp_bytes;
  HIP_TRY(c, hipcub::DeviceScan::InclusiveScan(w->temp, tb, w->pqh, w->pq, hipcub::Max(), np, st));
  if (prof) HIP_TRY(c, hipEventRecord(w->ev[2], st));
  k_search_count<<<wave_grid(np + 1), 256, 0, st>>>(w->pq, w->poff, w->span, qs, ix, np, nq, w->pcnt);
  HIP_TRY(c, hipGetLastError());
  if (prof) HIP_TRY(c, hipEventRecord(w->ev[3], st));
  tb = w->temp_bytes;
  HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(w->temp, tb, w->pcnt, w->pscan, np + 1, st));
  k_search_offsets<<<grid_for(nq + 1), 256, 0, st>>>(w->poff, w->pscan, nq, np, w->off);
  HIP_TRY(c, hipGetLastError());
  if (prof) HIP_TRY(c, hipEventRecord(w->ev[4], st));
  HIP_TRY(c, hipMemcpyAsync(&w->pin[1], w->off + nq, sizeof(long long), hipMemcpyDeviceToHost, st));
  if (offsets)
    HIP_TRY(c, hipMemcpyAsync(offsets, w->off, static_cast<size_t>(nq + 1) * sizeof(long long), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  w->ev_rec = prof;
  w->valid = true;
  w->reads_gen = c->reads_gen;
  w->index_gen = c->index_gen;
  w->nq = nq;
  w->np = np;
  w->total = w->pin[1];
  if (n_hits) *n_hits = w->total;
  return FSLR_OK;
}

int fslr_search_hits(fslr_ctx* c, int32_t* hits, int64_t capacity) {
  if (!c) return FSLR_ERR_INVALID;
  SearchWork* w = c->srw;
  if (!w || !w->valid || w->reads_gen != c->reads_gen || w->index_gen != c->index_gen)
    return fail(c, FSLR_ERR_STATE, "fslr_search_hits: fslr_search first (on these reads and this index build)");
  if (int rc = search_state(c, "fslr_search")) return rc;
  if (capacity < w->total)
    return fail(c, FSLR_ERR_INVALID, "fslr_search_hits: capacity " + std::to_string(capacity) + " < " +
                                         std::to_string(w->total) + " hits");
  if (w->total == 0) return FSLR_OK;
  if (!hits) return fail(c, FSLR_ERR_INVALID, "fslr_search_hits: null array");
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  if (w->total > w->h_cap) {
    const int64_t cap = w->total + w->total / 4;
    if (int rc = dalloc(c, &w->hits, cap)) {
      w->h_cap = 0;
      return rc;
    }
    w->h_cap = cap;
  }
  if (!c->lg_perm.empty() && w->perm_gen != c->reads_gen) {
    const int64_t m = static_cast<int64_t>(c->lg_perm.size());
    if (m > w->perm_cap) {
      if (int rc = dalloc(c, &w->perm, m)) {
        w->perm_cap = 0;
        return rc;
      }
      w->perm_cap = m;
    }
    HIP_TRY(c, hipMemcpyAsync(w->perm, c->lg_perm.data(), m * sizeof(int), hipMemcpyHostToDevice, st));
    w->perm_gen = c->reads_gen;
  }
  const IndexView ix = index_view(c, c->lg_perm.empty() ? nullptr : w->perm);
  const bool prof = w->ev_rec && c->prof_phases;
  if (prof) HIP_TRY(c, hipEventRecord(w->ev[5], st));
  k_search_fill<<<wave_grid(w->np), 256, 0, st>>>(w->pq, w->poff, w->pscan, w->span, w->q3 + w->q_cap, ix, w->np,
                                                  w->nq, w->total, w->hits);
  HIP_TRY(c, hipGetLastError());
  if (prof) HIP_TRY(c, hipEventRecord(w->ev[6], st));
  HIP_TRY(c, hipMemcpyAsync(hits, w->hits, static_cast<size_t>(w->total) * sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  w->ev_fill = prof;
  return FSLR_OK;
}

int fslr_search_timings(fslr_ctx* c, float* ms) {
  if (!c || !ms) return FSLR_ERR_INVALID;
  SearchWork* w = c->srw;
  if (!w || !w->ev_rec) return fail(c, FSLR_ERR_STATE, "fslr_search_timings: no profiled search (fslr_set_profiling 1)");
  // the scans: the piece scan, the head marks and their max-scan, the hit scan and the offsets; the
  // host's wait for the piece total between the first two is outside every interval
  float span = 0, s1 = 0, s2 = 0, count = 0, s3 = 0, fill = 0;
  HIP_TRY(c, hipEventElapsedTime(&span, w->ev[0], w->ev[1]));
  HIP_TRY(c, hipEventElapsedTime(&s1, w->ev[1], w->ev[7]));
  HIP_TRY(c, hipEventElapsedTime(&s2, w->ev[8], w->ev[2]));
  HIP_TRY(c, hipEventElapsedTime(&count, w->ev[2], w->ev[3]));
  HIP_TRY(c, hipEventElapsedTime(&s3, w->ev[3], w->ev[4]));
  if (w->ev_fill) HIP_TRY(c, hipEventElapsedTime(&fill, w->ev[5], w->ev[6]));
  ms[0] = span;
  ms[1] = count;
  ms[2] = s1 + s2 + s3;
  ms[3] = fill;
  return FSLR_OK;
}

}  // extern "C"
