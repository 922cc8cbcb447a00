// segments.hip — path segments: per slot of every cluster path the minimum, lower median and maximum of the
// reference start and end of the intervals that land in it, and per link between two slots the same of the
// query-space gap (fslr_hip.h states the contract; DESIGN.md §3.10.5 the bytes; tests/segments_ref.py the plain
// statement).
//
// The path rows are resident (paths.hip): tok_off, n_reads, path_of_read, flipped.  The caller brings the query
// key and, for the gaps, the query end per CSR interval.  Passes, all on the context's stream:
//   k_seg_keys      key[r] = path_of_read[r] + 1 (0: not clustered), val[r] = r
//   hipcub sort     stable radix SortPairs of (key, read): the reads of a row adjacent, in ascending rank
//   k_seg_rowprep   per row: n_reads and, for a row of k >= 2 reads, len * k (64-bit), one more word of zeros
//   hipcub scans    rfirst = exclusive sum of n_reads, base = exclusive 64-bit sum of len * k (base[n_rows] = V,
//                   the bucket words per stream)
//   k_seg_ord       ord[read] = its place minus the unclustered reads minus rfirst[row]
//   k_seg_emit      one lane per interval, lane groups of 16 / 32 / 64 by read length: the rank in the chain by
//                   shuffles, the next piece's key through LDS by rank; the value of (row, position p, ordinal o)
//                   goes to base[row] + p * k + o of its stream; a row of one read writes min = med = max to
//                   the output; the read of ordinal 0 writes k, the bucket's first word and "last slot" per slot
//   fslr_cluster_path_segments_any on virtual reads: k_chain_long_flag on path_of_read, a hipcub scan and
//                   k_chain_long_compact list the clustered reads of more than FSLR_MAX_L intervals (their count
//                   comes back with the bucket words'), and when there are any
//   k_seg_emit_long one workgroup per such read: chain.hpp's bitonic sort of the chain words in LDS, the thread at
//                   rank t takes its interval from the word's low bits and the next piece's key from word t + 1,
//                   and writes what k_seg_emit's lane writes.  A row's reads share its length, so one of the two
//                   kernels serves a row wholly
//   k_seg_flags     per slot: which tier its k falls in
//   hipcub select   the slots of each tier, ascending (three Flagged selections of a counting iterator)
//   k_seg_small     2 <= k <= S: a lane group of 16 / 32 / 64 per (slot, stream); each lane counts the smaller and
//                   the smaller-or-equal values by shuffles
//   k_seg_lds       S < k <= T: one workgroup per (slot, stream), chain.hpp's bitonic sort in LDS
//   k_seg_select    k > T: one workgroup per (slot, stream), block min / max and an exact radix select, four
//                   rounds of eight bits with integer LDS counters
// No block waits for another.  Every bucket word has one writer; a gap word of the output is zeroed and then
// written at most once; the LDS counters take integer additions whose sum does not depend on the order.  The
// bytes are the same on every run.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>

#include "chain.hpp"
#include "ctx.hpp"
#include "fslr_hip.h"
#include "idxsearch.hpp"
#include "kernels.hpp"
#include "wave.hpp"

using namespace fslr;

// the resident rows, the scratch (grown on demand) and the last call's event time
struct SegmentWork {
  // resident rows
  int* out = nullptr;                // [9 x n_tokens] start min, med, max; end min, med, max; gap min, med, max
  int64_t n_tokens = 0;
  bool have = false;
  // the caller's columns, CSR interval order
  int* qkey = nullptr;               // [icap]
  int* qend = nullptr;               // [icap]
  int64_t icap = 0;
  // per read: sort keys in / out, reads in / out, ord
  unsigned* rbuf = nullptr;          // [5 x rcap]
  int64_t rcap = 0;
  // fslr_cluster_path_segments_any on virtual reads: flag, pos and the list of the clustered reads of more than
  // FSLR_MAX_L intervals
  int* lbuf = nullptr;               // [3 x (lcap + 1)]
  int64_t lcap = 0;
  // per row: n_reads and their scan; len * k and their scan
  int* wbuf = nullptr;               // [2 x (wcap + 1)]
  long long* wbuf64 = nullptr;       // [2 x (wcap + 1)]
  int64_t wcap = 0;
  // per slot: k, the tier lists (3), then the bucket's first word, then last-slot and the tier flags (3)
  int* tbuf = nullptr;               // [4 x tcap]
  long long* tbuf64 = nullptr;       // [tcap]
  unsigned char* tbuf8 = nullptr;    // [4 x tcap]
  int64_t tcap = 0;
  // the buckets: start, end, gap
  int* vbuf = nullptr;               // [3 x vcap]
  int64_t vcap = 0;
  int* cnt = nullptr;                // [4] device: the tier counts
  long long* host = nullptr;         // [4] pinned: the counts read back
  unsigned char* stage = nullptr;    // [kStageBytes] pinned staging of the uploads
  void* temp = nullptr;
  size_t temp_bytes = 0;
  hipEvent_t ev[2] = {};
  bool ev_ok = false, timed = false;
  float ms = 0;
};

namespace {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr int64_t kMaxItems = int64_t(1) << 30;             // hipcub's item count is an int
constexpr size_t kStageBytes = size_t(4) << 20;
constexpr int kSmallMax = 64;                               // a lane group is at most a wavefront
constexpr int kLdsMax = kChainMaxL;                         // chain_sort_lds' words

template <typename T>
void dfree(T*& p) {
  if (p) (void)hipFree(p);
  p = nullptr;
}

}  // namespace

void fslr_segments_drop(fslr_ctx* c) {
  if (c->sgw) c->sgw->have = false;
}

void fslr_segments_free(fslr_ctx* c) {
  SegmentWork* w = c->sgw;
  if (!w) return;
  dfree(w->out), dfree(w->qkey), dfree(w->qend), dfree(w->rbuf), dfree(w->wbuf), dfree(w->wbuf64), dfree(w->tbuf);
  dfree(w->tbuf64), dfree(w->tbuf8), dfree(w->vbuf), dfree(w->cnt), dfree(w->temp), dfree(w->lbuf);
  if (w->host) (void)hipHostFree(w->host);
  if (w->stage) (void)hipHostFree(w->stage);
  if (w->ev_ok)
    for (hipEvent_t e : w->ev) (void)hipEventDestroy(e);
  delete w;
  c->sgw = nullptr;
}

namespace {

// ---- ordinals -----------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_seg_keys(const int* __restrict__ por, long long n, long long n_rows,
                                                     unsigned* __restrict__ key, unsigned* __restrict__ val) {
  for (long long r = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; r < n; r += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(r, n);
    const int row = por[r];
    key[r] = (row >= 0 && row < n_rows) ? static_cast<unsigned>(row) + 1u : 0u;
    val[r] = static_cast<unsigned>(r);
  }
}

__global__ __launch_bounds__(kBlock) void k_seg_rowprep(const int* __restrict__ nreads, const long long* __restrict__ tok_off,
                                                        long long n_rows, int* __restrict__ nr, long long* __restrict__ lk) {
  for (long long l = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; l <= n_rows; l += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(l, n_rows + 1);
    int k = 0;
    long long v = 0;
    if (l < n_rows) {
      k = nreads[l];
      if (k >= 2) v = (tok_off[l + 1] - tok_off[l]) * k;      // a row of one read needs no bucket
    }
    nr[l] = k;                                      // [n_rows] = 0: the scans' last outputs are the totals
    lk[l] = v;
  }
}

__global__ __launch_bounds__(kBlock) void k_seg_ord(const unsigned* __restrict__ key, const unsigned* __restrict__ val,
                                                    const int* __restrict__ rfirst, long long n, long long n_rows,
                                                    int* __restrict__ ord) {
  const long long n_out = n - rfirst[n_rows];       // the reads of key 0 stand in front
  for (long long s = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; s < n; s += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(s, n);
    const unsigned k = key[s];
    if (k == 0u) continue;
    FSLR_BOUND(k - 1u, n_rows);
    FSLR_BOUND(val[s], n);
    ord[val[s]] = static_cast<int>(s - n_out - rfirst[k - 1u]);
  }
}

// ---- emit ---------------------------------------------------------------------------------------
struct EmitArgs {
  RealReads rr;                      // the real lists on a context with virtual reads (n = the real reads)
  const int* longs;                  // [n_long] the reads of k_seg_emit_long
  long long n_long;
  const int4* iv;                    // {chrom, start, end, thr}
  const int *qkey, *qend;            // qend null: no gaps
  const int* por;
  const unsigned char* flipped;
  const int *ord, *nreads;
  const long long *tok_off, *base;
  long long n, ni, n_rows, nt, n_vals, n_quads;
  int *vs, *ve, *vg;                 // [n_vals] the buckets
  int* out;                          // [9 x nt]
  int* slot_k;                       // [nt]
  long long* slot_base;              // [nt]
  unsigned char* slot_last;          // [nt]
};

__device__ __forceinline__ int sat32(long long v) {
  return static_cast<int>(max(static_cast<long long>(INT_MIN), min(static_cast<long long>(INT_MAX), v)));
}

__device__ __forceinline__ int unbias(unsigned u) { return static_cast<int>(u ^ 0x80000000u); }

// a clustered read as the emit kernels see it: len == 0 when it writes nothing
struct EmitRead {
  int len = 0, first = 0, k = 0, o = 0, flip = 0;
  long long t0 = 0, b0 = 0;
};

// read r of `len` intervals (the caller checked it against its kernel's range): its row, ordinal and bucket
__device__ __forceinline__ EmitRead emit_read(const EmitArgs& a, long long r, int first, int len) {
  EmitRead e;
  e.first = first;
  const int row = a.por[r];
  if (row < 0 || row >= a.n_rows) return e;
  e.t0 = a.tok_off[row];
  e.k = a.nreads[row];
  e.o = a.ord[r];
  e.b0 = a.base[row];
  e.flip = a.flipped[r] != 0;
  // a read's row has the read's length and holds its ordinal, so every slot below lies in the row
  if (a.tok_off[row + 1] - e.t0 == len && e.o >= 0 && e.o < e.k) e.len = len;
  return e;
}

// the interval at chain rank `rank` of read e: record rec, and with link (a next piece exists and the caller
// brought the query ends) the gap to that piece
__device__ __forceinline__ void emit_piece(const EmitArgs& a, const EmitRead& e, int rank, const int4& rec, bool link, int gap) {
  const int len = e.len, k = e.k, o = e.o;
  const long long t0 = e.t0, b0 = e.b0;
  const int p = e.flip ? len - 1 - rank : rank;
  const long long s = t0 + p;
  FSLR_BOUND(s, a.nt);
  // the link to the next piece of the read's own chain lies between positions p and p -+ 1: stored at the smaller
  const int pl = e.flip ? len - 2 - rank : rank;
  if (k == 1) {
    a.out[s] = a.out[a.nt + s] = a.out[2 * a.nt + s] = rec.y;
    a.out[3 * a.nt + s] = a.out[4 * a.nt + s] = a.out[5 * a.nt + s] = rec.z;
    if (link) {
      FSLR_BOUND(t0 + pl, a.nt);
      a.out[6 * a.nt + t0 + pl] = a.out[7 * a.nt + t0 + pl] = a.out[8 * a.nt + t0 + pl] = gap;
    }
    a.slot_k[s] = 1;
  } else {
    const long long at = b0 + static_cast<long long>(p) * k + o;
    FSLR_BOUND(at, a.n_vals);
    a.vs[at] = rec.y;
    a.ve[at] = rec.z;
    if (link) {
      FSLR_BOUND(b0 + static_cast<long long>(pl) * k + o, a.n_vals);
      a.vg[b0 + static_cast<long long>(pl) * k + o] = gap;
    }
    if (o == 0) {                                   // one read per row describes its slots
      a.slot_k[s] = k;
      a.slot_base[s] = b0 + static_cast<long long>(p) * k;
      a.slot_last[s] = static_cast<unsigned char>(p == len - 1);
    }
  }
}

// 64 / W reads side by side: read r (valid: it exists) on the W-lane group of this lane, interval j = the lane's
// place in the group.  lds: this wavefront's 64 slots.
template <int W>
__device__ __forceinline__ void emit_group(const EmitArgs& a, long long r, bool valid, int lane, int* lds) {
  const int j = lane & (W - 1), gbase = lane & ~(W - 1);
  EmitRead e;
  if (valid) {
    FSLR_BOUND(r, a.n);
    const int4 rm = a.rr.rmeta[r];
    const int len = a.rr.len(r, rm);
    // len > W: a real read of more than FSLR_MAX_L intervals (k_seg_emit_long's; its first chunk is not a read of
    // its own); otherwise the caller chose W for its reads
    if (len <= W) e = emit_read(a, r, rm.x, len);
  }
  const int len = e.len;
  const bool have = j < len;
  int key = 0, qe = 0;
  int4 rec = make_int4(0, 0, 0, 0);
  if (have) {
    const long long i = static_cast<long long>(e.first) + j;
    FSLR_BOUND(i, a.ni);
    rec = a.iv[i];
    key = a.qkey[i];
    if (a.qend) qe = a.qend[i];
  }
  const int rank = chain_rank(key, len, j, gbase);
  if (have) lds[gbase + rank] = key;                // rank < len <= W: the group's slots
  wave_lds_sync();
  if (have) {
    const bool link = a.qend && rank + 1 < len;
    int gap = 0;
    if (link) gap = sat32(static_cast<long long>(lds[gbase + rank + 1]) - static_cast<long long>(qe));
    emit_piece(a, e, rank, rec, link, gap);
  }
  wave_lds_sync();                                  // the next pass writes the slots again
}

__global__ __launch_bounds__(kBlock) void k_seg_emit(EmitArgs a) {
  __shared__ int s_slot[kWavesPerBlock][kWave];
  const int lane = lane_id(), wv = threadIdx.x / kWave;
  int* lds = s_slot[wv];
  // a wavefront takes four consecutive reads at a time
  for (long long q = blockIdx.x * static_cast<long long>(kWavesPerBlock) + wv; q < a.n_quads;
       q += gridDim.x * static_cast<long long>(kWavesPerBlock)) {
    const long long r0 = q * 4;
    const long long r16 = r0 + (lane >> 4);
    int len = 0;
    if (r16 < a.n) {
      FSLR_BOUND(r16, a.n);
      len = a.rr.len(r16, a.rr.rmeta[r16]);
      if (a.por[r16] < 0 || len > FSLR_MAX_L) len = 0;
    }
    const bool over16 = __ballot(len > 16) != 0ull, over32 = __ballot(len > 32) != 0ull;
    if (__ballot(len > 0) == 0ull) continue;        // wave-uniform: nothing to write
    if (!over16) {
      emit_group<16>(a, r16, r16 < a.n, lane, lds);
    } else if (!over32) {
      for (int p = 0; p < 2; ++p) {
        const long long r = r0 + 2 * p + (lane >> 5);
        emit_group<32>(a, r, r < a.n, lane, lds);
      }
    } else {
      for (int p = 0; p < 4; ++p) emit_group<64>(a, r0 + p, r0 + p < a.n, lane, lds);
    }
  }
}

// One workgroup per clustered read of more than FSLR_MAX_L intervals (a.longs): the chain order by an LDS sort;
// the thread that holds rank t takes its interval's place in the list from the word's low bits and the next
// piece's key from word t + 1, and writes what emit_group's lane writes.  32 KiB of LDS, no atomics.
__global__ __launch_bounds__(kChainBlock) void k_seg_emit_long(EmitArgs a) {
  __shared__ unsigned long long s_w[kChainMaxL];
  for (long long q = blockIdx.x; q < a.n_long; q += gridDim.x) {
    FSLR_BOUND(q, a.n_long);
    const int r = a.longs[q];
    FSLR_BOUND(r, a.n);
    const int4 rm = a.rr.rmeta[r];
    const int rlen = a.rr.len(r, rm), off2 = a.rr.second(r, rlen);
    EmitRead e;
    if (rlen > FSLR_MAX_L && rlen <= kChainMaxL) e = emit_read(a, r, rm.x, rlen);
    const int len = min(e.len, kChainMaxL);         // bounds the LDS indices below
    if (len == 0) continue;                         // block-uniform: no barrier is skipped by a part of the block
    chain_sort_lds(s_w, a.qkey, e.first, off2, len, a.ni);
    for (int t = threadIdx.x; t < len; t += kChainBlock) {
      FSLR_BOUND(t, kChainMaxL);
      const unsigned long long w = s_w[t];
      const int j = static_cast<int>(w & (kChainMaxL - 1));
      FSLR_BOUND(j, len);
      const long long i = list_at(e.first, off2, j);
      FSLR_BOUND(i, a.ni);
      const int4 rec = a.iv[i];
      const bool link = a.qend && t + 1 < len;
      int gap = 0;
      if (link) {
        FSLR_BOUND(t + 1, kChainMaxL);
        gap = sat32(static_cast<long long>(unbias(static_cast<unsigned>(s_w[t + 1] >> 12))) - static_cast<long long>(a.qend[i]));
      }
      emit_piece(a, e, t, rec, link, gap);
    }
    __syncthreads();                                // the next read writes the words again
  }
}

// ---- tiers --------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_seg_flags(const int* __restrict__ slot_k, long long nt, int small, int lds,
                                                      unsigned char* __restrict__ flag) {
  for (long long s = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; s < nt; s += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(s, nt);
    const int k = slot_k[s];
    flag[s] = k >= 2 && k <= small;
    flag[nt + s] = k >= 2 && k > small && k <= lds;
    flag[2 * nt + s] = k >= 2 && k > small && k > lds;
  }
}

struct SelArgs {
  const int* list;                   // [n_list] the tier's slots
  long long n_list, n_items;         // items: stream * n_list + place in the list
  const int* slot_k;
  const long long* slot_base;
  const unsigned char* slot_last;
  const int* vals[3];                // start, end, gap buckets
  long long nt, n_vals;
  int* out;                          // [9 x nt]
};

// the k of an item, 0 for none (past the end, or the gap stream of a row's last slot: its words stay 0)
__device__ __forceinline__ int item_k(const SelArgs& a, long long item, long long* s, int* stream) {
  if (item >= a.n_items) return 0;
  const long long i = item % a.n_list;
  *stream = static_cast<int>(item / a.n_list);
  FSLR_BOUND(i, a.n_list);
  *s = a.list[i];
  FSLR_BOUND(*s, a.nt);
  if (*stream == 2 && a.slot_last[*s]) return 0;
  return a.slot_k[*s];
}

__device__ __forceinline__ void put3(const SelArgs& a, int stream, long long s, int c, int v) {
  FSLR_BOUND(s, a.nt);
  a.out[(3 * stream + c) * a.nt + s] = v;
}

// 64 / W items side by side: lane j of the group holds value j of the item's bucket
template <int W>
__device__ __forceinline__ void small_group(const SelArgs& a, long long item, int lane) {
  const int j = lane & (W - 1), gbase = lane & ~(W - 1);
  long long s = 0;
  int stream = 0;
  int k = item_k(a, item, &s, &stream);
  if (k > W) k = 0;                                 // the caller chose W for its items
  const bool have = j < k;
  int v = 0;
  if (have) {
    const long long at = a.slot_base[s] + j;
    FSLR_BOUND(at, a.n_vals);
    v = a.vals[stream][at];
  }
  int kmax = k;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) kmax = max(kmax, __shfl_xor(kmax, d));
  int lt = 0, le = 0;
  for (int i = 0; i < kmax; ++i) {                  // kmax <= W: gbase + i stays in the group
    const int o = __shfl(v, gbase + i);
    lt += (i < k) && o < v;
    le += (i < k) && o <= v;
  }
  // the sorted places [lt, le) hold v: the lowest lane that covers a place writes it
  const int m = (k - 1) / 2;
  const unsigned long long gmask = W == 64 ? ~0ull : (1ull << (W & 63)) - 1ull;
  const unsigned long long b_min = (__ballot(have && lt == 0) >> gbase) & gmask;
  const unsigned long long b_med = (__ballot(have && lt <= m && m < le) >> gbase) & gmask;
  const unsigned long long b_max = (__ballot(have && le == k) >> gbase) & gmask;
  if (have) {
    if (j == __ffsll(static_cast<long long>(b_min)) - 1) put3(a, stream, s, 0, v);
    if (j == __ffsll(static_cast<long long>(b_med)) - 1) put3(a, stream, s, 1, v);
    if (j == __ffsll(static_cast<long long>(b_max)) - 1) put3(a, stream, s, 2, v);
  }
}

__global__ __launch_bounds__(kBlock) void k_seg_small(SelArgs a) {
  const int lane = lane_id(), wv = threadIdx.x / kWave;
  const long long n_quads = (a.n_items + 3) / 4;
  for (long long q = blockIdx.x * static_cast<long long>(kWavesPerBlock) + wv; q < n_quads;
       q += gridDim.x * static_cast<long long>(kWavesPerBlock)) {
    const long long i0 = q * 4;
    long long s = 0;
    int stream = 0;
    const int k = item_k(a, i0 + (lane >> 4), &s, &stream);
    const bool over16 = __ballot(k > 16) != 0ull, over32 = __ballot(k > 32) != 0ull;
    if (__ballot(k > 0) == 0ull) continue;          // wave-uniform
    if (!over16) {
      small_group<16>(a, i0 + (lane >> 4), lane);
    } else if (!over32) {
      for (int p = 0; p < 2; ++p) small_group<32>(a, i0 + 2 * p + (lane >> 5), lane);
    } else {
      for (int p = 0; p < 4; ++p) small_group<64>(a, i0 + p, lane);
    }
  }
}

// One workgroup per (slot, stream) of k <= kLdsMax values: chain_sort_lds' words are (biased value, place), so the
// sorted words give elements 0, (k - 1) / 2 and k - 1.  32 KiB of LDS.
__global__ __launch_bounds__(kChainBlock) void k_seg_lds(SelArgs a) {
  __shared__ unsigned long long s_w[kChainMaxL];
  for (long long item = blockIdx.x; item < a.n_items; item += gridDim.x) {
    long long s = 0;
    int stream = 0;
    const int k = item_k(a, item, &s, &stream);     // block-uniform
    if (k < 1 || k > kLdsMax) continue;
    const long long b = a.slot_base[s];
    FSLR_BOUND(b + k - 1, a.n_vals);
    // the bucket as a list of k words from its first: interval i of the list is word i (first 0, the rest from 64)
    chain_sort_lds(s_w, a.vals[stream] + b, 0, FSLR_MAX_L, k, k);
    if (threadIdx.x == 0) {
      put3(a, stream, s, 0, unbias(static_cast<unsigned>(s_w[0] >> 12)));
      put3(a, stream, s, 1, unbias(static_cast<unsigned>(s_w[(k - 1) / 2] >> 12)));
      put3(a, stream, s, 2, unbias(static_cast<unsigned>(s_w[k - 1] >> 12)));
    }
    __syncthreads();                                // the next item writes the words again
  }
}

// One workgroup per (slot, stream) of any k: min and max by a block reduction; the lower median by a radix select
// on the biased value, most significant byte first: each round counts, among the values that share the prefix
// found so far, the next byte into 256 LDS counters, and thread 0 walks them to the byte that holds the target
// place.  Four rounds, each one pass over the bucket.
__global__ __launch_bounds__(kBlock) void k_seg_select(SelArgs a) {
  __shared__ int s_hist[256];
  __shared__ int s_red[2 * kWavesPerBlock];
  __shared__ unsigned s_prefix;
  __shared__ int s_target;
  const int lane = lane_id(), wv = threadIdx.x / kWave;
  for (long long item = blockIdx.x; item < a.n_items; item += gridDim.x) {
    long long s = 0;
    int stream = 0;
    const int k = item_k(a, item, &s, &stream);     // block-uniform
    if (k < 1) continue;
    const long long b = a.slot_base[s];
    FSLR_BOUND(b + k - 1, a.n_vals);
    const int* v = a.vals[stream] + b;
    int lo = INT_MAX, hi = INT_MIN;
    for (int i = threadIdx.x; i < k; i += kBlock) {
      lo = min(lo, v[i]);
      hi = max(hi, v[i]);
    }
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
      lo = min(lo, __shfl_xor(lo, d));
      hi = max(hi, __shfl_xor(hi, d));
    }
    if (lane == 0) {
      s_red[wv] = lo;
      s_red[kWavesPerBlock + wv] = hi;
    }
    if (threadIdx.x == 0) {
      s_prefix = 0u;
      s_target = (k - 1) / 2;
    }
    for (int round = 0; round < 4; ++round) {
      const int shift = 24 - 8 * round;
      s_hist[threadIdx.x] = 0;                      // kBlock == 256 counters
      __syncthreads();
      const unsigned prefix = s_prefix;
      for (int i = threadIdx.x; i < k; i += kBlock) {
        const unsigned u = static_cast<unsigned>(v[i]) ^ 0x80000000u;
        // round > 0: shift + 8 <= 24, the bits above this round's byte
        if (round == 0 || (u >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&s_hist[(u >> shift) & 255u], 1);
      }
      __syncthreads();
      if (threadIdx.x == 0) {
        int t = s_target, d = 0;
        while (d < 255 && t >= s_hist[d]) t -= s_hist[d++];      // the counts sum to more than t: d stops in range
        s_target = t;
        s_prefix = prefix | (static_cast<unsigned>(d) << shift);
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      lo = s_red[0], hi = s_red[kWavesPerBlock];
#pragma unroll
      for (int i = 1; i < kWavesPerBlock; ++i) {
        lo = min(lo, s_red[i]);
        hi = max(hi, s_red[kWavesPerBlock + i]);
      }
      put3(a, stream, s, 0, lo);
      put3(a, stream, s, 1, unbias(s_prefix));
      put3(a, stream, s, 2, hi);
    }
    __syncthreads();                                // the next item writes the words again
  }
}

// ---- host side ----------------------------------------------------------------------------------
int bits_for(int64_t n_keys) {                   // bits that hold the keys 0 .. n_keys - 1, at least 1
  int b = 1;
  while ((int64_t(1) << b) < n_keys) ++b;
  return b;
}

// FSLR_SEGS_SMALL (1..64) and FSLR_SEGS_LDS (from it up to 4096), read per call: the largest k of the lane-group
// tier and of the LDS tier; the tests set them to move the seams between the tiers
void tier_caps(int* small, int* lds) {
  *small = kSmallMax;
  *lds = kLdsMax;
  if (const char* e = std::getenv("FSLR_SEGS_SMALL")) {
    const int v = std::atoi(e);
    if (v >= 1 && v <= kSmallMax) *small = v;
  }
  if (const char* e = std::getenv("FSLR_SEGS_LDS")) {
    const int v = std::atoi(e);
    if (v >= *small && v <= kLdsMax) *lds = v;
  }
}

int ensure_temp(fslr_ctx* c, SegmentWork* w, size_t bytes) {
  if (bytes <= w->temp_bytes && w->temp) return FSLR_OK;
  dfree(w->temp);
  w->temp_bytes = 0;
  HIP_TRY(c, hipMalloc(&w->temp, bytes ? bytes : 1));
  w->temp_bytes = bytes ? bytes : 1;
  return FSLR_OK;
}

// host -> device through the pinned chunk; each chunk syncs (the chunk is reused)
int up(fslr_ctx* c, SegmentWork* w, void* dst, const void* src, size_t bytes) {
  for (size_t at = 0; at < bytes; at += kStageBytes) {
    const size_t m = std::min(kStageBytes, bytes - at);
    std::memcpy(w->stage, static_cast<const unsigned char*>(src) + at, m);
    HIP_TRY(c, hipMemcpyAsync(static_cast<unsigned char*>(dst) + at, w->stage, m, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  return FSLR_OK;
}

// the rows of a result (allocated apart from the resident ones: a failure keeps those)
struct NewRows {
  int* out = nullptr;
  ~NewRows() { dfree(out); }
};

// fslr_cluster_path_segments (any = false: a context with virtual reads is refused) and
// fslr_cluster_path_segments_any.  On a context without virtual reads the two run the same code.
int segments_run(fslr_ctx* c, const int32_t* iv_qkey, const int32_t* iv_qend, int64_t n_intervals, int64_t* n_tokens_out,
                 bool any) {
  if (!c) return FSLR_ERR_INVALID;
  if (!c->reads_set || c->n == 0) return fail(c, FSLR_ERR_STATE, "fslr_cluster_path_segments: no reads set");
  if (int rc = search_state(c, any ? "fslr_cluster_path_segments_any" : "fslr_cluster_path_segments")) return rc;
  const int* cid = nullptr;
  int64_t tn = 0, nc = 0;
  if (!fslr_cluster_view(c, &cid, &tn, &nc))
    return fail(c, FSLR_ERR_STATE, "fslr_cluster_path_segments: no cluster table (fslr_cluster_table first)");
  const int64_t n_real = c->lg_set ? c->lg_n_real : c->n;
  if (tn != n_real)
    return fail(c, FSLR_ERR_STATE, "fslr_cluster_path_segments: the cluster table holds " + std::to_string(tn) +
                                       " reads, the context " + std::to_string(n_real) +
                                       " (a table from before fslr_append_reads / fslr_remove_reads, or of other "
                                       "reads: fslr_cluster_table again)");
  const long long* loff = nullptr;
  const int* lrows = nullptr;
  int64_t lcap = 0, n_loci = 0, lnc = 0;
  if (!fslr_loci_view(c, &loff, &lrows, &lcap, &n_loci, &lnc) || lnc != nc)
    return fail(c, FSLR_ERR_STATE, "fslr_cluster_path_segments: no cluster loci of this table (fslr_cluster_loci first)");
  fslr_paths_rows pv;
  if (!fslr_paths_view(c, &pv) || pv.n_clusters != nc || pv.n != n_real)
    return fail(c, FSLR_ERR_STATE, "fslr_cluster_path_segments: no cluster paths of this table (fslr_cluster_paths first)");
  if (c->lg_set && !any)
    return fail(c, FSLR_ERR_INVALID, "fslr_cluster_path_segments: the context holds reads of more than " +
                                         std::to_string(FSLR_MAX_L) + " intervals (out of scope here)");
  if (!iv_qkey) return fail(c, FSLR_ERR_INVALID, "fslr_cluster_path_segments: iv_qkey is NULL");
  if (n_intervals != c->ni)
    return fail(c, FSLR_ERR_INVALID, "fslr_cluster_path_segments: n_intervals " + std::to_string(n_intervals) +
                                         ", the context holds " + std::to_string(c->ni));
  // n: the real reads (on a context with virtual reads the chunks behind them are no reads of their own)
  const bool virt = c->lg_set;
  const int64_t n = n_real, ni = c->ni, n_rows = pv.n_rows, nt = pv.n_tokens;
  const RealReads rr{c->rmeta, virt ? c->lg_rlen : nullptr, virt ? c->lg_off2 : nullptr};
  if (virt && !c->lg_perm.empty() && static_cast<int64_t>(c->lg_perm.size()) != ni)
    return fail(c, FSLR_ERR_STATE, "fslr_cluster_path_segments: the interval permutation does not span the intervals (internal)");
  if (ni > kMaxItems || n >= kMaxItems)
    return fail(c, FSLR_ERR_INVALID, "fslr_cluster_path_segments: " + std::to_string(ni) + " intervals: more than 2^30");
  if (n_rows < 0 || n_rows > n || nt < n_rows || nt > ni)
    return fail(c, FSLR_ERR_STATE, "fslr_cluster_path_segments: inconsistent path rows (internal)");
  HIP_TRY(c, hipSetDevice(c->device));
  if (!c->sgw) c->sgw = new SegmentWork();
  SegmentWork* w = c->sgw;
  int rc;
  hipStream_t st = c->stream;
  if (!w->cnt)
    if ((rc = dalloc(c, &w->cnt, 4))) return rc;
  if (!w->host) HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&w->host), 4 * sizeof(long long), hipHostMallocDefault));
  if (!w->stage) HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&w->stage), kStageBytes, hipHostMallocDefault));
  if (c->profiling && !w->ev_ok) {
    for (hipEvent_t& e : w->ev) HIP_TRY(c, hipEventCreate(&e));
    w->ev_ok = true;
  }
  if (ni > w->icap || !w->qkey) {
    w->icap = 0;
    if ((rc = dalloc(c, &w->qkey, static_cast<size_t>(ni))) || (rc = dalloc(c, &w->qend, static_cast<size_t>(ni)))) return rc;
    w->icap = ni;
  }
  if (n > w->rcap || !w->rbuf) {
    w->rcap = 0;
    if ((rc = dalloc(c, &w->rbuf, static_cast<size_t>(5 * n)))) return rc;
    w->rcap = n;
  }
  int *lflag = nullptr, *lpos = nullptr, *longs = nullptr;
  if (virt) {
    if (n > w->lcap || !w->lbuf) {
      w->lcap = 0;
      if ((rc = dalloc(c, &w->lbuf, static_cast<size_t>(3 * (n + 1))))) return rc;
      w->lcap = n;
    }
    lflag = w->lbuf, lpos = lflag + (w->lcap + 1), longs = lpos + (w->lcap + 1);
  }
  if (n_rows > w->wcap || !w->wbuf) {
    w->wcap = 0;
    if ((rc = dalloc(c, &w->wbuf, static_cast<size_t>(2 * (n_rows + 1)))) || (rc = dalloc(c, &w->wbuf64, static_cast<size_t>(2 * (n_rows + 1)))))
      return rc;
    w->wcap = n_rows;
  }
  if (nt > w->tcap || !w->tbuf) {
    w->tcap = 0;
    if ((rc = dalloc(c, &w->tbuf, static_cast<size_t>(4 * nt))) || (rc = dalloc(c, &w->tbuf64, static_cast<size_t>(nt))) ||
        (rc = dalloc(c, &w->tbuf8, static_cast<size_t>(4 * nt))))
      return rc;
    w->tcap = nt;
  }
  NewRows nr;
  if ((rc = dalloc(c, &nr.out, static_cast<size_t>(9 * nt)))) return rc;
  unsigned *key_in = w->rbuf, *key_out = key_in + w->rcap, *val_in = key_out + w->rcap, *val_out = val_in + w->rcap;
  int* ord = reinterpret_cast<int*>(val_out + w->rcap);
  int *nrin = w->wbuf, *rfirst = nrin + (w->wcap + 1);
  long long *lk = w->wbuf64, *base = lk + (w->wcap + 1);
  int *slot_k = w->tbuf, *lists = slot_k + w->tcap;           // lists: 3 x tcap
  unsigned char *slot_last = w->tbuf8, *flags = slot_last + w->tcap;   // flags: 3 x nt
  const int kbits = bits_for(n_rows + 1), ni_n = static_cast<int>(n), nw = static_cast<int>(n_rows + 1);
  size_t tb_sort = 0, tb_s32 = 0, tb_s64 = 0, tb_sel = 0, tb_long = 0;
  HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(nullptr, tb_sort, key_in, key_out, val_in, val_out, ni_n, 0, kbits, st));
  HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, tb_s32, nrin, rfirst, nw, st));
  HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, tb_s64, lk, base, nw, st));
  hipcub::CountingInputIterator<int> iota(0);
  HIP_TRY(c, hipcub::DeviceSelect::Flagged(nullptr, tb_sel, iota, flags, lists, w->cnt, static_cast<int>(std::max<int64_t>(nt, 1)), st));
  if (virt) HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, tb_long, lflag, lpos, static_cast<int>(n + 1), st));
  if ((rc = ensure_temp(c, w, std::max(std::max(std::max(tb_sort, tb_sel), std::max(tb_s32, tb_s64)), tb_long)))) return rc;
  int small = 0, lds = 0;
  tier_caps(&small, &lds);
  w->timed = false;
  w->ms = 0;
  if (virt && !c->lg_perm.empty()) {                // the caller's order is the real CSR's
    if ((rc = up_perm(c, w->stage, kStageBytes, w->qkey, iv_qkey, c->lg_perm))) return rc;
    if (iv_qend)
      if ((rc = up_perm(c, w->stage, kStageBytes, w->qend, iv_qend, c->lg_perm))) return rc;
  } else {
    if ((rc = up(c, w, w->qkey, iv_qkey, static_cast<size_t>(ni) * sizeof(int)))) return rc;
    if (iv_qend)
      if ((rc = up(c, w, w->qend, iv_qend, static_cast<size_t>(ni) * sizeof(int)))) return rc;
  }
  if (c->profiling) HIP_TRY(c, hipEventRecord(w->ev[0], st));     // the columns are up: the device work from here
  if (nt > 0) {
    size_t tb;
    k_seg_keys<<<grid_for(n), kBlock, 0, st>>>(pv.path_of_read, n, n_rows, key_in, val_in);
    HIP_TRY(c, hipGetLastError());
    tb = w->temp_bytes;
    HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(w->temp, tb, key_in, key_out, val_in, val_out, ni_n, 0, kbits, st));
    k_seg_rowprep<<<grid_for(n_rows + 1), kBlock, 0, st>>>(pv.rows, pv.tok_off, n_rows, nrin, lk);
    HIP_TRY(c, hipGetLastError());
    tb = w->temp_bytes;
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(w->temp, tb, nrin, rfirst, nw, st));
    tb = w->temp_bytes;
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(w->temp, tb, lk, base, nw, st));
    k_seg_ord<<<grid_for(n), kBlock, 0, st>>>(key_out, val_out, rfirst, n, n_rows, ord);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(w->host, base + n_rows, sizeof(long long), hipMemcpyDeviceToHost, st));
    if (virt) {
      // the clustered reads of more than FSLR_MAX_L intervals: flag and scan; their count comes back beside n_vals
      k_chain_long_flag<<<grid_for(n + 1), kChainBlock, 0, st>>>(pv.path_of_read, rr.rlen, n, lflag);
      HIP_TRY(c, hipGetLastError());
      tb = w->temp_bytes;
      HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(w->temp, tb, lflag, lpos, static_cast<int>(n + 1), st));
      HIP_TRY(c, hipMemcpyAsync(w->host + 1, lpos + n, sizeof(int), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(c, hipStreamSynchronize(st));
    const int64_t n_vals = w->host[0];               // the intervals of the rows of two or more reads
    const int64_t n_long = virt ? *reinterpret_cast<const int*>(w->host + 1) : 0;
    if (n_vals < 0 || n_vals > ni || n_long < 0 || n_long > n)
      return fail(c, FSLR_ERR_STATE, "fslr_cluster_path_segments: inconsistent counts (internal)");
    if (n_vals > w->vcap || !w->vbuf) {
      w->vcap = 0;
      if ((rc = dalloc(c, &w->vbuf, static_cast<size_t>(3 * std::max<int64_t>(n_vals, 1))))) return rc;
      w->vcap = std::max<int64_t>(n_vals, 1);
    }
    int *vs = w->vbuf, *ve = vs + w->vcap, *vg = ve + w->vcap;
    // the gap columns: 0 for a row's last slot and without iv_qend, every other word is written once below
    HIP_TRY(c, hipMemsetAsync(nr.out + 6 * nt, 0, static_cast<size_t>(3 * nt) * sizeof(int), st));
    HIP_TRY(c, hipMemsetAsync(slot_k, 0, static_cast<size_t>(nt) * sizeof(int), st));
    const long long n_quads = (n + 3) / 4;
    EmitArgs ea{rr, longs, n_long, c->iv, w->qkey, iv_qend ? w->qend : nullptr, pv.path_of_read, pv.flipped, ord, pv.rows, pv.tok_off, base,
                n, ni, n_rows, nt, n_vals, n_quads, vs, ve, vg, nr.out, slot_k, w->tbuf64, slot_last};
    k_seg_emit<<<grid_for(n_quads, kWavesPerBlock, 256 * 32), kBlock, 0, st>>>(ea);
    HIP_TRY(c, hipGetLastError());
    if (n_long > 0) {                                // only when such reads exist, one workgroup each
      k_chain_long_compact<<<grid_for(n), kChainBlock, 0, st>>>(lflag, lpos, n, n_long, longs);
      HIP_TRY(c, hipGetLastError());
      k_seg_emit_long<<<grid_for(n_long, 1, 256 * 8), kChainBlock, 0, st>>>(ea);
      HIP_TRY(c, hipGetLastError());
    }
    if (n_vals > 0) {
      k_seg_flags<<<grid_for(nt), kBlock, 0, st>>>(slot_k, nt, small, lds, flags);
      HIP_TRY(c, hipGetLastError());
      for (int t = 0; t < 3; ++t) {
        tb = w->temp_bytes;
        HIP_TRY(c, hipcub::DeviceSelect::Flagged(w->temp, tb, iota, flags + t * nt, lists + t * w->tcap, w->cnt + t, static_cast<int>(nt), st));
      }
      HIP_TRY(c, hipMemcpyAsync(w->host, w->cnt, 3 * sizeof(int), hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipStreamSynchronize(st));
      const int* hc = reinterpret_cast<const int*>(w->host);
      const int64_t cnt[3] = {hc[0], hc[1], hc[2]};
      for (int t = 0; t < 3; ++t)
        if (cnt[t] < 0 || cnt[t] > nt) return fail(c, FSLR_ERR_STATE, "fslr_cluster_path_segments: inconsistent counts (internal)");
      const int n_streams = iv_qend ? 3 : 2;
      for (int t = 0; t < 3; ++t) {                   // a tier launches only when it has slots
        if (cnt[t] == 0) continue;
        SelArgs sa{lists + t * w->tcap, cnt[t], cnt[t] * n_streams, slot_k, w->tbuf64, slot_last, {vs, ve, vg}, nt, n_vals, nr.out};
        if (t == 0)
          k_seg_small<<<grid_for((sa.n_items + 3) / 4, kWavesPerBlock, 256 * 32), kBlock, 0, st>>>(sa);
        else if (t == 1)
          k_seg_lds<<<grid_for(sa.n_items, 1, 256 * 8), kChainBlock, 0, st>>>(sa);
        else
          k_seg_select<<<grid_for(sa.n_items, 1, 256 * 8), kBlock, 0, st>>>(sa);
        HIP_TRY(c, hipGetLastError());
      }
    }
  }
  if (c->profiling) HIP_TRY(c, hipEventRecord(w->ev[1], st));
  HIP_TRY(c, hipStreamSynchronize(st));
  if (c->profiling) {
    HIP_TRY(c, hipEventElapsedTime(&w->ms, w->ev[0], w->ev[1]));
    w->timed = true;
  }
  // install
  std::swap(w->out, nr.out);
  w->n_tokens = nt;
  w->have = true;
  if (n_tokens_out) *n_tokens_out = nt;
  return FSLR_OK;
}

}  // namespace

extern "C" {

int fslr_cluster_path_segments(fslr_ctx* c, const int32_t* iv_qkey, const int32_t* iv_qend, int64_t n_intervals,
                               int64_t* n_tokens_out) {
  return segments_run(c, iv_qkey, iv_qend, n_intervals, n_tokens_out, false);
}

int fslr_cluster_path_segments_any(fslr_ctx* c, const int32_t* iv_qkey, const int32_t* iv_qend, int64_t n_intervals,
                                   int64_t* n_tokens_out) {
  return segments_run(c, iv_qkey, iv_qend, n_intervals, n_tokens_out, true);
}

int fslr_get_cluster_path_segments(fslr_ctx* c, int32_t* start, int32_t* end, int32_t* gap, int64_t token_capacity) {
  if (!c) return FSLR_ERR_INVALID;
  SegmentWork* w = c->sgw;
  if (!w || !w->have)
    return fail(c, FSLR_ERR_STATE, "fslr_get_cluster_path_segments: fslr_cluster_path_segments first");
  if (token_capacity < w->n_tokens)
    return fail(c, FSLR_ERR_INVALID, "fslr_get_cluster_path_segments: token capacity " + std::to_string(token_capacity) +
                                         " < " + std::to_string(w->n_tokens) + " tokens");
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t nt = static_cast<size_t>(w->n_tokens);
  int32_t* out[3] = {start, end, gap};
  for (int k = 0; k < 3; ++k)
    if (out[k] && nt)
      HIP_TRY(c, hipMemcpyAsync(out[k], w->out + 3 * k * nt, 3 * nt * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FSLR_OK;
}

int fslr_cluster_path_segments_timings(fslr_ctx* c, float* ms) {
  if (!c || !ms) return FSLR_ERR_INVALID;
  SegmentWork* w = c->sgw;
  if (!w || !w->timed)
    return fail(c, FSLR_ERR_STATE,
                "fslr_cluster_path_segments_timings: no profiled fslr_cluster_path_segments (fslr_set_profiling 1 or 2)");
  ms[0] = w->ms;
  return FSLR_OK;
}

}  // extern "C"
