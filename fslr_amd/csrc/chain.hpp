// chain.hpp — a read as a chain of loci, the per-lane pieces shared by junctions.hip and paths.hip: lane j of a
// lane group holds interval j of its read; its place in the chain is its rank by (query key, CSR position), its
// locus is the row of its read's cluster that holds it.  Below them the pieces for reads of more than FSLR_MAX_L
// intervals (the _any calls): the list's addressing, the LDS sort of one read per workgroup, the list of such reads.
#pragma once
#include <hip/hip_runtime.h>

#include "fslr_hip.h"
#include "kernels.hpp"

namespace fslr {

// the locus row of cluster c that holds (chrom, start): the last of the cluster's rows whose (chrom, start) is
// not above it; the rows are (chrom, start)-ordered and cover every interval of the cluster's reads.
// A: loff [n_clusters + 1], lchrom / lstart [n_loci], n_loci, n_clusters
template <typename A>
__device__ __forceinline__ int locus_of(const A& a, int c, int chrom, int start) {
  FSLR_BOUND(c, a.n_clusters);
  long long lo = a.loff[c], hi = a.loff[c + 1] - 1;
  lo = max(0ll, min(lo, a.n_loci - 1));
  hi = max(lo, min(hi, a.n_loci - 1));
  for (int it = 0; it < 32 && lo < hi; ++it) {      // rows < 2^30: at most 30 halvings
    const long long mid = (lo + hi + 1) >> 1;
    FSLR_BOUND(mid, a.n_loci);
    const int mc = a.lchrom[mid];
    if (mc < chrom || (mc == chrom && a.lstart[mid] <= start))
      lo = mid;
    else
      hi = mid - 1;
  }
  return static_cast<int>(lo);
}

// the rank of lane j's interval in its read's chain: the intervals of the group (lanes gbase .. gbase + len - 1)
// with a smaller (key, j).  Every lane of the wavefront calls it; the wavefront's longest read bounds the loop,
// and the caller's group width holds it, so gbase + i stays inside the group.
__device__ __forceinline__ int chain_rank(int key, int len, int j, int gbase) {
  int lmax = len;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) lmax = max(lmax, __shfl_xor(lmax, d));
  int rank = 0;
  for (int i = 0; i < lmax; ++i) {
    const int ok = __shfl(key, gbase + i);
    rank += (i < len) && (ok < key || (ok == key && i < j));
  }
  return rank;
}

// ---- reads of more than FSLR_MAX_L intervals (the _any calls on a context with virtual reads) ----------------
// A real read's list: rlen[r] intervals, the first FSLR_MAX_L at rmeta[r].x, the rest from off2[r] (long.hip).
// rlen == null: a context without virtual reads, the length is rmeta's.
struct RealReads {
  const int4* rmeta;
  const int* rlen;
  const int* off2;
  __device__ __forceinline__ int len(long long r, const int4& rm) const { return rlen ? rlen[r] : (rm.y & 0xFFFF); }
  __device__ __forceinline__ int second(long long r, int len) const { return (off2 && len > FSLR_MAX_L) ? off2[r] : 0; }
};

// the CSR position of interval i of a list
__device__ __forceinline__ long long list_at(int first, int off2, int i) {
  return i < FSLR_MAX_L ? static_cast<long long>(first) + i : static_cast<long long>(off2) + (i - FSLR_MAX_L);
}

constexpr int kChainMaxL = 4096;                 // FSLR_MAX_ANY_L: a list's index fits the word's low 12 bits
constexpr int kChainBlock = 256;
constexpr unsigned long long kChainPad = ~0ull;  // above every word: the padding sorts to the end

// the sort word of interval j with query key `key`: ascending words = (key ascending, j ascending)
__device__ __forceinline__ unsigned long long chain_word(int key, int j) {
  return (static_cast<unsigned long long>(static_cast<unsigned>(key) ^ 0x80000000u) << 12) | static_cast<unsigned>(j);
}

// the smallest power of two >= len, at most kChainMaxL for len <= kChainMaxL
__device__ __forceinline__ int chain_pow2(int len) {
  int n2 = 2;
  while (n2 < len && n2 < kChainMaxL) n2 <<= 1;
  return n2;
}

// One workgroup loads the words of a list of len <= kChainMaxL intervals into s[0 .. n2) (n2 = chain_pow2(len),
// padded) and sorts them ascending with a bitonic network; every thread of the block calls it, the words are
// sorted and visible to all when it returns.  s: kChainMaxL words of LDS.
__device__ __forceinline__ int chain_sort_lds(unsigned long long* s, const int* __restrict__ qkey, int first, int off2,
                                              int len, long long ni) {
  const int n2 = chain_pow2(len);
  for (int i = threadIdx.x; i < n2; i += blockDim.x) {
    FSLR_BOUND(i, kChainMaxL);
    unsigned long long w = kChainPad;
    if (i < len) {
      const long long k = list_at(first, off2, i);
      FSLR_BOUND(k, ni);
      w = chain_word(qkey[k], i);
    }
    s[i] = w;
  }
  __syncthreads();
  for (int k = 2; k <= n2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < (n2 >> 1); i += blockDim.x) {
        const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;      // hi < n2: i < n2 / 2
        FSLR_BOUND(hi, n2);
        const unsigned long long a = s[lo], b = s[hi];
        if ((a > b) == ((lo & k) == 0)) {
          s[lo] = b;
          s[hi] = a;
        }
      }
      __syncthreads();
    }
  return n2;
}

// the reads the one-workgroup-per-read kernels take: clustered, more than FSLR_MAX_L intervals
static __global__ __launch_bounds__(kChainBlock) void k_chain_long_flag(const int* __restrict__ cid, const int* __restrict__ rlen,
                                                                        long long n, int* __restrict__ flag) {
  for (long long r = blockIdx.x * static_cast<long long>(kChainBlock) + threadIdx.x; r <= n; r += gridDim.x * static_cast<long long>(kChainBlock)) {
    FSLR_BOUND(r, n + 1);
    flag[r] = r < n && cid[r] >= 0 && rlen[r] > FSLR_MAX_L;      // flag[n] = 0: the scan's last output is the total
  }
}

static __global__ __launch_bounds__(kChainBlock) void k_chain_long_compact(const int* __restrict__ flag, const int* __restrict__ pos,
                                                                           long long n, long long n_long, int* __restrict__ out) {
  for (long long r = blockIdx.x * static_cast<long long>(kChainBlock) + threadIdx.x; r < n; r += gridDim.x * static_cast<long long>(kChainBlock)) {
    FSLR_BOUND(r, n);
    if (flag[r]) {
      FSLR_BOUND(pos[r], n_long);
      out[pos[r]] = static_cast<int>(r);
    }
  }
}

}  // namespace fslr
