// segshared.hpp — what segments.hip (path segments) and collapsed.hip (collapsed path segments) share: the walk
// over a clustered read's chain, parameterised by what is written per piece, and the three selection tiers that
// take the minimum, lower median and maximum of a slot's values, with a k per stream.
//
// The chain walk.  A is the kernel's argument struct.  It has the members
//   rr, longs, n_long, iv, qkey, qend, por, n, ni, n_quads            (as segments.hip's EmitArgs documents them)
//   A::Read           default-constructible, with int len (0: the read writes nothing) and int first
//   A::kPrevGap       whether piece() wants the gap of the link that ENDS at its interval as well
//   Read read(r, first, len) const
//   void piece(const Read&, int rank, long long i, const int4& rec, bool link, int gap, int pgap) const
//                     the interval at chain rank `rank`, CSR position i, record rec; link: a next piece exists and
//                     the caller brought the query ends, gap: the gap to it; pgap (kPrevGap, rank > 0, query ends
//                     given): the gap from the piece before, else 0
// The tiers.  SelArgs names, per stream, the k of every slot (kk) and the three buckets; a slot's bucket begins at
// slot_base in each of them and the stream takes its first kk[stream][slot] words.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <cstdlib>

#include "chain.hpp"
#include "fslr_hip.h"
#include "kernels.hpp"
#include "wave.hpp"

namespace fslr {

constexpr int kSegBlock = 256;
constexpr int kSegWaves = kSegBlock / kWave;
constexpr int kSegSmallMax = 64;                            // a lane group is at most a wavefront
constexpr int kSegLdsMax = kChainMaxL;                      // chain_sort_lds' words

__device__ __forceinline__ int sat32(long long v) {
  return static_cast<int>(max(static_cast<long long>(INT_MIN), min(static_cast<long long>(INT_MAX), v)));
}

__device__ __forceinline__ int unbias(unsigned u) { return static_cast<int>(u ^ 0x80000000u); }

// ---- the chain walk -----------------------------------------------------------------------------
// 64 / W reads side by side: read r (valid: it exists) on the W-lane group of this lane, interval j = the lane's
// place in the group.  lds: this wavefront's 64 slots.
template <int W, typename A>
__device__ __forceinline__ void emit_group(const A& a, long long r, bool valid, int lane, int* lds) {
  const int j = lane & (W - 1), gbase = lane & ~(W - 1);
  typename A::Read e;
  if (valid) {
    FSLR_BOUND(r, a.n);
    const int4 rm = a.rr.rmeta[r];
    const int len = a.rr.len(r, rm);
    // len > W: a real read of more than FSLR_MAX_L intervals (the long kernel's; its first chunk is not a read of
    // its own); otherwise the caller chose W for its reads
    if (len <= W) e = a.read(r, rm.x, len);
  }
  const int len = e.len;
  const bool have = j < len;
  int key = 0, qe = 0;
  long long i = 0;
  int4 rec = make_int4(0, 0, 0, 0);
  if (have) {
    i = static_cast<long long>(e.first) + j;
    FSLR_BOUND(i, a.ni);
    rec = a.iv[i];
    key = a.qkey[i];
    if (a.qend) qe = a.qend[i];
  }
  const int rank = chain_rank(key, len, j, gbase);
  if (have) lds[gbase + rank] = key;                // rank < len <= W: the group's slots
  wave_lds_sync();
  const bool link = have && a.qend && rank + 1 < len;
  int gap = 0, pgap = 0;
  if (link) gap = sat32(static_cast<long long>(lds[gbase + rank + 1]) - static_cast<long long>(qe));
  if (A::kPrevGap && a.qend) {                      // wave-uniform: the gaps through the same slots, by rank
    wave_lds_sync();                                // the keys are read
    if (have) lds[gbase + rank] = gap;
    wave_lds_sync();
    if (have && rank > 0) pgap = lds[gbase + rank - 1];
  }
  if (have) a.piece(e, rank, i, rec, link, gap, pgap);
  wave_lds_sync();                                  // the next pass writes the slots again
}

// the body of the lane-group kernel: a wavefront takes four consecutive reads at a time, on 16 lanes each, or two /
// one at a time on 32 / 64 lanes when one of them is longer.  lds: this wavefront's 64 slots.
template <typename A>
__device__ __forceinline__ void emit_waves(const A& a, int* lds) {
  const int lane = lane_id(), wv = threadIdx.x / kWave;
  for (long long q = blockIdx.x * static_cast<long long>(kSegWaves) + wv; q < a.n_quads;
       q += gridDim.x * static_cast<long long>(kSegWaves)) {
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

// the body of the long kernel: one workgroup per clustered read of more than FSLR_MAX_L intervals (a.longs): the
// chain order by an LDS sort; the thread that holds rank t takes its interval's place in the list from the word's
// low bits and the neighbouring pieces' keys from the words beside it, and writes what emit_group's lane writes.
// s_w: kChainMaxL words of LDS (32 KiB), no atomics.
template <typename A>
__device__ __forceinline__ void emit_long_blocks(const A& a, unsigned long long* s_w) {
  for (long long q = blockIdx.x; q < a.n_long; q += gridDim.x) {
    FSLR_BOUND(q, a.n_long);
    const int r = a.longs[q];
    FSLR_BOUND(r, a.n);
    const int4 rm = a.rr.rmeta[r];
    const int rlen = a.rr.len(r, rm), off2 = a.rr.second(r, rlen);
    typename A::Read e;
    if (rlen > FSLR_MAX_L && rlen <= kChainMaxL) e = a.read(r, rm.x, rlen);
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
      int gap = 0, pgap = 0;
      if (link) {
        FSLR_BOUND(t + 1, kChainMaxL);
        gap = sat32(static_cast<long long>(unbias(static_cast<unsigned>(s_w[t + 1] >> 12))) - static_cast<long long>(a.qend[i]));
      }
      if (A::kPrevGap && a.qend && t > 0) {
        const int jp = static_cast<int>(s_w[t - 1] & (kChainMaxL - 1));
        FSLR_BOUND(jp, len);
        const long long ip = list_at(e.first, off2, jp);
        FSLR_BOUND(ip, a.ni);
        pgap = sat32(static_cast<long long>(unbias(static_cast<unsigned>(w >> 12))) - static_cast<long long>(a.qend[ip]));
      }
      a.piece(e, t, i, rec, link, gap, pgap);
    }
    __syncthreads();                                // the next read writes the words again
  }
}

// ---- tiers --------------------------------------------------------------------------------------
// which tier a slot's k falls in: flag [3 x nt]
static __global__ __launch_bounds__(kSegBlock) void k_seg_flags(const int* __restrict__ slot_k, long long nt, int small, int lds,
                                                                unsigned char* __restrict__ flag) {
  for (long long s = blockIdx.x * static_cast<long long>(kSegBlock) + threadIdx.x; s < nt; s += gridDim.x * static_cast<long long>(kSegBlock)) {
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
  const int* kk[3];                  // [nt] per stream: the slot's k (the tier comes from the largest of them)
  const long long* slot_base;
  const unsigned char* slot_last;    // [nt] or null: the gap stream of a marked slot has no values
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
  if (*stream == 2 && a.slot_last && a.slot_last[*s]) return 0;
  return a.kk[*stream][*s];
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

static __global__ __launch_bounds__(kSegBlock) void k_seg_small(SelArgs a) {
  const int lane = lane_id(), wv = threadIdx.x / kWave;
  const long long n_quads = (a.n_items + 3) / 4;
  for (long long q = blockIdx.x * static_cast<long long>(kSegWaves) + wv; q < n_quads;
       q += gridDim.x * static_cast<long long>(kSegWaves)) {
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

// One workgroup per (slot, stream) of k <= kSegLdsMax values: chain_sort_lds' words are (biased value, place), so
// the sorted words give elements 0, (k - 1) / 2 and k - 1.  32 KiB of LDS.
static __global__ __launch_bounds__(kChainBlock) void k_seg_lds(SelArgs a) {
  __shared__ unsigned long long s_w[kChainMaxL];
  for (long long item = blockIdx.x; item < a.n_items; item += gridDim.x) {
    long long s = 0;
    int stream = 0;
    const int k = item_k(a, item, &s, &stream);     // block-uniform
    if (k < 1 || k > kSegLdsMax) continue;
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
static __global__ __launch_bounds__(kSegBlock) void k_seg_select(SelArgs a) {
  __shared__ int s_hist[256];
  __shared__ int s_red[2 * kSegWaves];
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
    for (int i = threadIdx.x; i < k; i += kSegBlock) {
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
      s_red[kSegWaves + wv] = hi;
    }
    if (threadIdx.x == 0) {
      s_prefix = 0u;
      s_target = (k - 1) / 2;
    }
    for (int round = 0; round < 4; ++round) {
      const int shift = 24 - 8 * round;
      s_hist[threadIdx.x] = 0;                      // kSegBlock == 256 counters
      __syncthreads();
      const unsigned prefix = s_prefix;
      for (int i = threadIdx.x; i < k; i += kSegBlock) {
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
      lo = s_red[0], hi = s_red[kSegWaves];
#pragma unroll
      for (int i = 1; i < kSegWaves; ++i) {
        lo = min(lo, s_red[i]);
        hi = max(hi, s_red[kSegWaves + i]);
      }
      put3(a, stream, s, 0, lo);
      put3(a, stream, s, 1, unbias(s_prefix));
      put3(a, stream, s, 2, hi);
    }
    __syncthreads();                                // the next item writes the words again
  }
}

// ---- host side ----------------------------------------------------------------------------------
inline int bits_for(int64_t n_keys) {            // bits that hold the keys 0 .. n_keys - 1, at least 1
  int b = 1;
  while ((int64_t(1) << b) < n_keys) ++b;
  return b;
}

// FSLR_SEGS_SMALL (1..64) and FSLR_SEGS_LDS (from it up to 4096), read per call: the largest k of the lane-group
// tier and of the LDS tier; the tests set them to move the seams between the tiers
inline void tier_caps(int* small, int* lds) {
  *small = kSegSmallMax;
  *lds = kSegLdsMax;
  if (const char* e = std::getenv("FSLR_SEGS_SMALL")) {
    const int v = std::atoi(e);
    if (v >= 1 && v <= kSegSmallMax) *small = v;
  }
  if (const char* e = std::getenv("FSLR_SEGS_LDS")) {
    const int v = std::atoi(e);
    if (v >= *small && v <= kSegLdsMax) *lds = v;
  }
}

// the launches of the tiers that have slots: lists [3 x list_stride], cnt their lengths; sa carries everything but
// list / n_list / n_items
inline hipError_t launch_tiers(SelArgs sa, const int* lists, int64_t list_stride, const int64_t cnt[3], int n_streams,
                               hipStream_t st) {
  for (int t = 0; t < 3; ++t) {                     // a tier launches only when it has slots
    if (cnt[t] == 0) continue;
    sa.list = lists + t * list_stride;
    sa.n_list = cnt[t];
    sa.n_items = cnt[t] * n_streams;
    if (t == 0)
      k_seg_small<<<grid_for((sa.n_items + 3) / 4, kSegWaves, 256 * 32), kSegBlock, 0, st>>>(sa);
    else if (t == 1)
      k_seg_lds<<<grid_for(sa.n_items, 1, 256 * 8), kChainBlock, 0, st>>>(sa);
    else
      k_seg_select<<<grid_for(sa.n_items, 1, 256 * 8), kSegBlock, 0, st>>>(sa);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace fslr
