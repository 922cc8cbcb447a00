// firstfit.hpp — the pair predicates of an ordered pair (list1, list2) as score.hip and match.hip
// evaluate them: the length gate's flags, the lane-group first-fit of overall_jaccard_similarity
// (cluster.py:140-170) and the packed result word I | U << 8 | flags << 16.  thr_ok, iv_match_general
// and lengths_pass are those of kernels.hpp.
//
// List2's columns sit on the lanes of a W-lane group (W in {16, 32, 64}; 64 / W pairs side by side in a
// wavefront), list1's rows are stepped uniformly over the group: where a row comes from (a broadcast
// record in score.hip, LDS in match.hip) is the caller's.
#pragma once
#include <cstdint>

#include "fslr_hip.h"
#include "kernels.hpp"

namespace fslr {

constexpr int kPassBytes = FSLR_MAX_L * kPassStride;

// different_lengths_or_alignments as flag bits: FSLR_SCORE_ZD_GATE where it divides by zero, else
// FSLR_SCORE_GATE where the pair passes, else 0
__device__ __forceinline__ int gate_flags(int q1, int q2, int n1, int n2, double qcut, double ncut) {
  bool zd = false;
  const bool pass = lengths_pass(q1, q2, n1, n2, qcut, ncut, &zd);
  return zd ? FSLR_SCORE_ZD_GATE : pass ? FSLR_SCORE_GATE : 0;
}

// the first-fit state of this lane's group: its column is taken, the pair met calculate_overlap's
// ZeroDivisionError, and the matches so far (zd and I are uniform over the group)
struct FirstFit {
  bool used = false, zd = false;
  int I = 0;

  // one row (chrom, start, end, thr) of list1 against the group's columns (col: this lane holds column
  // bj of list2); live: the row exists for this group (the wave may step past a shorter list1)
  template <int W>
  __device__ __forceinline__ void row(int c, int si, int ei, int ti, bool live, int4 bj, bool col, int lane) {
    const int l = lane & (W - 1);
    const int gbase = lane & ~(W - 1);
    // on copies, written back at the end: the step then compiles as it did inside the kernels' loops
    bool u = used, z = zd;
    int n = I;
    const int4 b = bj;
    const bool cand = col && live && !z && !u && b.x == c;
    // FSLR_THR_ZERO_ALN is a sentinel thr_ok would accept: tested before iv_match_general
    const bool zero = cand && (ti == FSLR_THR_ZERO_ALN || b.w == FSLR_THR_ZERO_ALN);
    const bool hit = cand && (zero || iv_match_general(si, ei, ti, b.y, b.z, b.w));
    unsigned long long hm = __ballot(hit), zm = __ballot(zero);
    if constexpr (W < kWave) {
      hm = (hm >> gbase) & ((1ull << W) - 1);
      zm >>= gbase;
    }
    if (hm) {
      const int j = __builtin_ctzll(hm);
      if ((zm >> j) & 1ull) {
        z = true;                      // the row's walk meets the aln_size == 0 column before any match
      } else {
        u |= l == j;
        ++n;
      }
    }
    used = u, zd = z, I = n;
  }
};

// the result word of a pair of LA x LB intervals with I matches: I | U << 8 | flags << 16 (pt: the pass
// table); calculate_overlap's ZeroDivisionError ends the pair with I = U = 0
__device__ __forceinline__ unsigned fit_result(int LA, int LB, int I, bool zd, int gate, const unsigned char* pt) {
  int U = LA + LB - I, flags = gate;
  if (zd) {
    I = U = 0;
    flags |= FSLR_SCORE_ZD_OVERLAP;
  } else if ((flags & FSLR_SCORE_GATE) && I > 0) {
    const int t = (I - 1) * kPassStride + (U - 1);
    FSLR_BOUND(t, kPassBytes);
    if (pt[t]) flags |= FSLR_SCORE_EDGE;
  }
  return static_cast<unsigned>(I) | (static_cast<unsigned>(U) << 8) | (static_cast<unsigned>(flags) << 16);
}

// (host) the result word's fields
inline void fit_unpack(unsigned v, int32_t* I, int32_t* U, uint8_t* flags) {
  *I = static_cast<int32_t>(v & 0xff);
  *U = static_cast<int32_t>((v >> 8) & 0xff);
  *flags = static_cast<uint8_t>(v >> 16);
}

}  // namespace fslr
