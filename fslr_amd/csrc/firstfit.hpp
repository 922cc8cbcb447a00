// firstfit.hpp — the pair predicates of an ordered pair (list1, list2): the length gate's flags, the
// first-fit of overall_jaccard_similarity (cluster.py:140-170) and the packed result word
// I | U << 8 | flags << 16.  thr_ok, iv_match_general and lengths_pass are those of kernels.hpp.  This
// is the one place on the device that states the greedy; its users:
//   score.hip  k_score_pairs<kAny>: FirstFit::row on 16-, 32- and 64-lane groups, long_fit for long pairs
//   match.hip  k_match_score<kAny>: the same, list1's rows read from LDS
//   cap.hip    k_cap_eval: lane_fit for two short reads, long_fit for every other slot
//   query.hip  deferred_kernel: FirstFit::row<64> for a deferred pair
//   matching.hip  k_pair_matching<kAny, kEmit>: score.hip's groups; the emit pass with the recording variant
//              (FirstFitT<true>, long_fit with a recorder), which keeps which row took which column
//
// List2's columns sit on the lanes of a W-lane group (W in {16, 32, 64}; 64 / W pairs side by side in a
// wavefront), list1's rows are stepped uniformly over the group: where a row comes from (a broadcast
// record in score.hip and query.hip, LDS in match.hip) is the caller's.
#pragma once
#include <cstdint>
#include <type_traits>

#include "fslr_hip.h"
#include "kernels.hpp"
#include "wave.hpp"

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
// ZeroDivisionError, and the matches so far (zd and I are uniform over the group).
// kRec (matching.hip): the recording variant.  The lane that wins a row keeps that row's index (ri) and the
// pair's match count at that moment (ord): in registers, no memory is touched.  Where the rows are stepped in
// ascending order over one set of columns (the lane groups), ord is the row's position among the pair's
// matched rows.  FirstFit, the plain state, holds neither (FitNoRec) and compiles as it did before the variant
// existed.
struct FitNoRec {};
struct FitRowRec {
  int ri = -1, ord = 0;
};
template <bool kRec>
struct FirstFitT : std::conditional_t<kRec, FitRowRec, FitNoRec> {
  bool used = false, zd = false;
  int I = 0;

  // one row (chrom, start, end, thr) of list1 against the group's columns (col: this lane holds column
  // bj of list2); live: the row exists for this group (the wave may step past a shorter list1); i (kRec):
  // the row's index in list1
  template <int W>
  __device__ __forceinline__ void row(int c, int si, int ei, int ti, bool live, int4 bj, bool col, int lane,
                                      int i = 0) {
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
        if constexpr (kRec) {
          if (l == j) this->ri = i, this->ord = n;
        }
        ++n;
      }
    }
    used = u, zd = z, I = n;
  }
};
using FirstFit = FirstFitT<false>;

// The scalar statement of the same rule, by one lane, for two reads of few intervals (LB <= 32: one bit of
// `used` per column; cap.hip takes it up to 16): rows ascending, the lowest unused column of the row's
// chromosome that matches or, where either interval has aln_size == 0, raises.  FirstFit::row is this loop
// with the columns on lanes: cand = column unused and same chromosome, zero = the raise, hit = zero or
// match, and the row takes the lowest hit.
__device__ __forceinline__ void lane_fit(const int4* __restrict__ iv, int oa, int ob, int LA, int LB, int* I_out,
                                         bool* zd_out) {
  unsigned used = 0u;
  int I = 0;
  bool zd = false;
  for (int i = 0; i < LA && !zd; ++i) {
    const int4 ai = iv[oa + i];
    for (int j = 0; j < LB; ++j) {
      if ((used >> j) & 1u) continue;
      const int4 bj = iv[ob + j];
      if (bj.x != ai.x) continue;
      if (ai.w == FSLR_THR_ZERO_ALN || bj.w == FSLR_THR_ZERO_ALN) {
        zd = true;
        break;
      }
      if (iv_match_general(ai.y, ai.z, ai.w, bj.y, bj.z, bj.w)) {
        used |= 1u << j;
        ++I;
        break;
      }
    }
  }
  *I_out = I;
  *zd_out = zd;
}

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

// ---- lists of up to FSLR_MAX_ANY_L intervals --------------------------------------------------------

// The first-fit of two lists of 1..FSLR_MAX_ANY_L intervals on one wavefront, chunk-outer: list2 is walked
// 64 columns at a time (column 64 c + l on lane l); per chunk the rows of list1 that no earlier chunk
// matched are stepped in ascending order through FirstFit::row<64>, and a row that finds a free matching
// column there takes the lowest one.  Exact: a row's choice depends on the earlier rows
// alone; an earlier row still unmatched when the chunk starts is stepped before it inside the chunk, and a
// row matched in an earlier chunk never looks at this one.  rows(i) / cols(j): record i of list1 / j of
// list2 (chrom, start, end, thr).  The matched bits: rows [64 s, 64 s + 64) on lane s, two 32-bit words.
//
// rec (matching.hip): what a caller keeps of the matching.  A column is taken at most once, so after a
// chunk every used lane still holds the row that took its column: rec->chunk(used, row, column) runs once
// per chunk, outside the row loops, on every lane; rec->done(lo, hi) hands over the matched bits at the end.
// A row may be matched in a later chunk than a later row was, so the order of the matches is not the order
// of the rows here: the caller ranks the rows from the matched bits.  Without a recorder (NoFitRec, the
// default: rec is not looked at) the function compiles as it did before it took one.
struct NoFitRec {
  static constexpr bool on = false;
  __device__ __forceinline__ void chunk(bool, int, int) {}
  __device__ __forceinline__ void done(unsigned, unsigned) {}
};

template <class Rows, class Cols, class Rec = NoFitRec>
__device__ __forceinline__ void long_fit(int LA, int LB, Rows rows, Cols cols, int lane, int* I_out, bool* zd_out,
                                         Rec* rec = nullptr) {
  unsigned done_lo = 0, done_hi = 0;
  int matched = 0;
  bool zd = false;
  const int nslice = (LA + kWave - 1) / kWave;
  for (int c0 = 0; c0 < LB && matched < LA && !zd; c0 += kWave) {
    const bool col = c0 + lane < LB;
    int4 bj = make_int4(-2, 0, 0, 0);
    if (col) bj = cols(c0 + lane);
    FirstFitT<Rec::on> ff;                         // this chunk's columns: used, and the matches made in it
    for (int s = 0; s < nslice && !ff.zd; ++s) {
      const int nr = min(kWave, LA - s * kWave);
      const unsigned long long live = nr == kWave ? ~0ull : (1ull << nr) - 1;
      const unsigned long long have = static_cast<unsigned>(rdl(static_cast<int>(done_lo), s)) |
                                      (static_cast<unsigned long long>(static_cast<unsigned>(rdl(static_cast<int>(done_hi), s))) << 32);
      unsigned long long pend = ~have & live;
      if (!pend) continue;
      if (__ballot(col && !ff.used) == 0) break;   // every column of the chunk is taken: no row can stop here
      int4 ai = make_int4(-1, 0, 0, 0);
      if (lane < nr) ai = rows(s * kWave + lane);
      unsigned long long got = 0;
      while (pend) {
        const int i = __builtin_ctzll(pend);
        pend &= pend - 1;
        const int before = ff.I;
        ff.template row<kWave>(rdl(ai.x, i), rdl(ai.y, i), rdl(ai.z, i), rdl(ai.w, i), true, bj, col, lane,
                               s * kWave + i);
        if (ff.zd) break;
        if (ff.I != before) got |= 1ull << i;
      }
      if (lane == s) {
        done_lo |= static_cast<unsigned>(got);
        done_hi |= static_cast<unsigned>(got >> 32);
      }
      matched += __popcll(got);
    }
    zd = ff.zd;
    if constexpr (Rec::on) rec->chunk(ff.used, ff.ri, c0 + lane);
  }
  if constexpr (Rec::on) rec->done(done_lo, done_hi);
  *I_out = matched;
  *zd_out = zd;
}

constexpr int kAnyIBits = 13, kAnyUBits = 14;      // I <= 4096, U <= 8191, four flag bits: 31 bits

// the result word of the _any calls: I | U << 13 | flags << 27.  EDGE from the pass table where it reaches
// (I <= FSLR_MAX_L and U <= 2 FSLR_MAX_L), else U <= umax[I - 1] (prep.umax_table; umax may be null where
// no pair can leave the table)
__device__ __forceinline__ unsigned fit_result_any(int LA, int LB, int I, bool zd, int gate, const unsigned char* pt,
                                                   const int* umax, int n_umax) {
  int U = LA + LB - I, flags = gate;
  if (zd) {
    I = U = 0;
    flags |= FSLR_SCORE_ZD_OVERLAP;
  } else if ((flags & FSLR_SCORE_GATE) && I > 0) {
    bool edge;
    if (I <= FSLR_MAX_L && U <= kPassStride) {
      const int t = (I - 1) * kPassStride + (U - 1);
      FSLR_BOUND(t, kPassBytes);
      edge = pt[t] != 0;
    } else {
      edge = umax && I <= n_umax && U <= umax[I - 1];
    }
    if (edge) flags |= FSLR_SCORE_EDGE;
  }
  return static_cast<unsigned>(I) | (static_cast<unsigned>(U) << kAnyIBits) |
         (static_cast<unsigned>(flags) << (kAnyIBits + kAnyUBits));
}

__host__ __device__ inline int any_I(unsigned v) { return static_cast<int>(v & ((1u << kAnyIBits) - 1)); }
__host__ __device__ inline int any_U(unsigned v) { return static_cast<int>((v >> kAnyIBits) & ((1u << kAnyUBits) - 1)); }
__host__ __device__ inline int any_flags(unsigned v) { return static_cast<int>(v >> (kAnyIBits + kAnyUBits)); }

// (host) the wide result word's fields
inline void fit_unpack_any(unsigned v, int32_t* I, int32_t* U, uint8_t* flags) {
  *I = any_I(v);
  *U = any_U(v);
  *flags = static_cast<uint8_t>(any_flags(v));
}

// Record j of a resident real read's list: its first FSLR_MAX_L intervals lie at `off`, the rest are
// consecutive from `off2` (long.hip's lg_off2; unused for a read of at most FSLR_MAX_L intervals)
struct ReadList {
  const int4* iv;
  int off, off2, ni;
  __device__ __forceinline__ int4 operator()(int j) const {
    const int k = j < FSLR_MAX_L ? off + j : off2 + (j - FSLR_MAX_L);
    FSLR_BOUND(k, ni);
    return iv[k];
  }
};

}  // namespace fslr
