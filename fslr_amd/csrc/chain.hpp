// chain.hpp — a read as a chain of loci, the per-lane pieces shared by junctions.hip and paths.hip: lane j of a
// lane group holds interval j of its read; its place in the chain is its rank by (query key, CSR position), its
// locus is the row of its read's cluster that holds it.
#pragma once
#include <hip/hip_runtime.h>

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

}  // namespace fslr
