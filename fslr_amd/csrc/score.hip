// score.hip — the pair predicates of the reference's pair loop for a batch of arbitrary ordered read
// pairs (cluster.py:197-224 without the search): different_lengths_or_alignments (:178-183),
// overall_jaccard_similarity (:140-170) over calculate_overlap (:133-136) and the cutoff lookup
// (:216-219), each pair's result written at its input position.
//
// Pair k = (a[k], b[k]): list1 = read a's intervals, list2 = read b's, both in CSR (data) order.  Only
// rmeta and iv are read: no index, no query state.
//
// Layout: list2's columns sit on lanes; the row loop over list1 is uniform over the lane group.  Per
// row: ballot of (column unused, same chromosome, overlap reaches both thresholds), find-first-set in
// the group's slice of the ballot, the winner marks itself used.  No LDS, no atomics.
// Lane-group packing: reads of the headline workload hold 1-16 intervals, so a wavefront takes four
// consecutive pairs and gives each a 16-lane group; when one of the four has a list2 of more than 16
// (32) intervals the wave runs its four pairs two (one) at a time on 32 (64) lanes instead.  The
// choice is per wave and a pair never leaves its wave: outputs are not reordered.
// List1 is loaded one record per lane of the group (chunks of the group's width) and broadcast per row.
//
// ZeroDivisionError is flagged, never raised: the gate's (max(qlen2) == 0, or the second ratio reached
// with max(n_alignments) == 0) by lengths_pass; calculate_overlap's when first-fit reaches a
// same-chromosome unused column where either interval has aln_size == 0 (thr == FSLR_THR_ZERO_ALN)
// before the row's first match: such a column counts as a hit, and a first hit that is one ends the
// pair with I = U = 0 (the reference stops there).
// Algorithmic bytes per pair: 8 B of ranks + 32 B of rmeta + 16 B x (L1 + L2) in,
// 4 B out.
//
// fslr_score_pairs_any (reads of up to FSLR_MAX_ANY_L intervals): on a context without
// virtual reads it is the driver and k_score_pairs<false>.  On one with virtual reads k_score_pairs<true> takes
// real ranks: a read's list is its first chunk at rmeta[r].x and the rest from lg_off2[r], lg_rlen[r]
// intervals in all.  A wave whose four pairs are all of two lists <= FSLR_MAX_L keeps the lane groups; a
// wave that meets a longer pair runs its pairs one at a time on 64 lanes, the long ones through long_fit
// (firstfit.hpp: list2 in chunks of 64 columns, one matched bit per row).  The result word is the wide one
// (I | U << 13 | flags << 27) and EDGE beyond the pass table comes from the call's umax.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <string>

#include "ctx.hpp"
#include "firstfit.hpp"
#include "fslr_hip.h"
#include "kernels.hpp"
#include "wave.hpp"

using namespace fslr;

// the scoring scratch (grows only, bounded by the chunk) and the last call's event times
struct ScoreWork {
  int* ab = nullptr;                 // [2 x cap] the chunk's a, b
  unsigned* out = nullptr;           // [cap] I | U << 8 | flags << 16; a virtual context's: I | U << 13 | flags << 27
  int64_t cap = 0;
  unsigned char* pt = nullptr;       // [FSLR_MAX_L x kPassStride] the pass table
  int* umax = nullptr;               // [umax_cap] the _any call's cutoff table
  int umax_cap = 0;
  unsigned* host = nullptr;          // [host_cap] pinned: the chunk's packed results
  int64_t host_cap = 0;
  hipEvent_t ev[4] = {};             // upload | kernel | download boundaries of a chunk
  bool ev_ok = false, timed = false;
  float ms[3] = {0, 0, 0};           // summed over the last call's chunks
};

void fslr_score_free(fslr_ctx* c) {
  ScoreWork* w = c->scw;
  if (!w) return;
  void* bufs[] = {w->ab, w->out, w->pt, w->umax};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  if (w->host) (void)hipHostFree(w->host);
  if (w->ev_ok)
    for (hipEvent_t e : w->ev) (void)hipEventDestroy(e);
  delete w;
  c->scw = nullptr;
}

namespace {

constexpr int64_t kChunk = int64_t(1) << 21;   // pairs per launch: 24 MiB of scratch at most

struct ScoreArgs {
  const int4* rmeta;
  const int4* iv;
  const unsigned char* pt;
  const int* a;
  const int* b;
  unsigned* out;
  int n_pairs, n_reads, ni;          // <true>: n_reads counts the real reads
  double qcut, ncut;
  int wide;                          // (timing tool) every pair on a full 64-lane group
  // <true> kernel only: real ranks on a context with virtual reads
  const int* rlen;                   // [n_real] a real read's interval count
  const int* off2;                   // [n_real] where a long read's intervals beyond FSLR_MAX_L begin
  const int* umax;
  int n_umax;
};

struct PairMeta {
  int offA, LA, offB, LB, gate;      // gate: FSLR_SCORE_GATE or FSLR_SCORE_ZD_GATE or 0
  int offA2, offB2;                  // <true>: offA, offB are the first chunks, LA, LB the real lengths
};

template <bool kAny>
__device__ __forceinline__ PairMeta pair_meta(const ScoreArgs& s, int k, bool valid) {
  PairMeta m{0, 0, 0, 0, 0, 0, 0};
  if (valid) {
    const int ra = s.a[k], rb = s.b[k];
    FSLR_BOUND(ra, s.n_reads);
    FSLR_BOUND(rb, s.n_reads);
    const int4 ma = s.rmeta[ra], mb = s.rmeta[rb];
    m.offA = ma.x;
    m.LA = ma.y & 0xffff;
    m.offB = mb.x;
    m.LB = mb.y & 0xffff;
    m.gate = gate_flags(ma.z, mb.z, ma.w, mb.w, s.qcut, s.ncut);
    if constexpr (kAny) {
      m.LA = s.rlen[ra];
      m.LB = s.rlen[rb];
      if (m.LA > FSLR_MAX_L) m.offA2 = s.off2[ra];
      if (m.LB > FSLR_MAX_L) m.offB2 = s.off2[rb];
    }
  }
  return m;
}

// 64 / W pairs side by side, the pair of meta m on the W-lane group of this lane (valid: it is a pair):
// its first-fit
template <int W>
__device__ __forceinline__ FirstFit group_fit(const ScoreArgs& s, bool valid, const PairMeta& m, int lane) {
  const int l = lane & (W - 1);
  const int gbase = lane & ~(W - 1);
  const bool col = valid && l < m.LB;
  int4 bj = make_int4(-2, 0, 0, 0);
  if (col) {
    FSLR_BOUND(m.offB + l, s.ni);
    bj = s.iv[m.offB + l];
  }
  // the row loop's bound: the longest list1 of the wave's groups (LA is uniform over a group of >= 16 lanes)
  int max_la = valid ? m.LA : 0;
  max_la = max(max_la, __shfl_xor(max_la, 16));
  max_la = max(max_la, __shfl_xor(max_la, 32));
  max_la = rdl(max_la, 0);
  FirstFit ff;
  for (int r0 = 0; r0 < max_la; r0 += W) {
    int4 ai = make_int4(-1, 0, 0, 0);
    if (valid && r0 + l < m.LA) {
      FSLR_BOUND(m.offA + r0 + l, s.ni);
      ai = s.iv[m.offA + r0 + l];
    }
    const int nr = min(W, max_la - r0);
    for (int i = 0; i < nr; ++i) {
      int c, si, ei, ti;
      if constexpr (W == kWave) {
        c = rdl(ai.x, i), si = rdl(ai.y, i), ei = rdl(ai.z, i), ti = rdl(ai.w, i);
      } else {
        const int src = gbase | i;
        c = __shfl(ai.x, src), si = __shfl(ai.y, src), ei = __shfl(ai.z, src), ti = __shfl(ai.w, src);
      }
      ff.row<W>(c, si, ei, ti, r0 + i < m.LA, bj, col, lane);
    }
  }
  return ff;
}

// the pair's result word: the narrow one, or <true> the wide one with EDGE beyond the pass table from umax
template <bool kAny>
__device__ __forceinline__ unsigned pair_result(const ScoreArgs& s, const PairMeta& m, int I, bool zd) {
  if constexpr (kAny)
    return fit_result_any(m.LA, m.LB, I, zd, m.gate, s.pt, s.umax, s.n_umax);
  else
    return fit_result(m.LA, m.LB, I, zd, m.gate, s.pt);
}

template <int W, bool kAny>
__device__ __forceinline__ void score_groups(const ScoreArgs& s, int k, bool valid, const PairMeta& m, int lane) {
  const FirstFit ff = group_fit<W>(s, valid, m, lane);
  if (valid && (lane & (W - 1)) == 0) s.out[k] = pair_result<kAny>(s, m, ff.I, ff.zd);
}

// <false>: ranks of a context without virtual reads.  <true>: real ranks on a context with virtual reads; a
// wave that meets a pair with a list beyond FSLR_MAX_L runs its pairs one at a time, the long ones through
// long_fit
template <bool kAny>
__global__ __launch_bounds__(256) void k_score_pairs(ScoreArgs s) {
  const int lane = threadIdx.x & 63;
  const int nq = (s.n_pairs + 3) >> 2;           // a wave takes pairs [4 q, 4 q + 4)
  const int nw = gridDim.x * (blockDim.x >> 6);
  for (int q = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); q < nq; q += nw) {
    const int k0 = q << 2;
    const int k = k0 + (lane >> 4);
    const bool valid = k < s.n_pairs;
    const PairMeta m = pair_meta<kAny>(s, k, valid);
    if constexpr (kAny) {
      if (__ballot(m.LA > FSLR_MAX_L || m.LB > FSLR_MAX_L) != 0) {
        for (int p = 0; p < 4 && k0 + p < s.n_pairs; ++p) {
          const PairMeta m1 = pair_meta<kAny>(s, k0 + p, true);
          if (m1.LA > FSLR_MAX_L || m1.LB > FSLR_MAX_L) {
            int I = 0;
            bool zd = false;
            long_fit(m1.LA, m1.LB, ReadList{s.iv, m1.offA, m1.offA2, s.ni}, ReadList{s.iv, m1.offB, m1.offB2, s.ni}, lane,
                     &I, &zd);
            if (lane == 0) s.out[k0 + p] = pair_result<kAny>(s, m1, I, zd);
          } else {
            score_groups<64, kAny>(s, k0 + p, true, m1, lane);
          }
        }
        continue;
      }
    }
    const bool w64 = s.wide || __ballot(m.LB > 32) != 0;
    const bool w32 = __ballot(m.LB > 16) != 0;
    if (w64) {
      for (int p = 0; p < 4 && k0 + p < s.n_pairs; ++p)
        score_groups<64, kAny>(s, k0 + p, true, pair_meta<kAny>(s, k0 + p, true), lane);
    } else if (w32) {
      for (int p = 0; p < 4 && k0 + p < s.n_pairs; p += 2) {
        const int k2 = k0 + p + (lane >> 5);
        const bool v2 = k2 < s.n_pairs;
        score_groups<32, kAny>(s, k2, v2, pair_meta<kAny>(s, k2, v2), lane);
      }
    } else {
      score_groups<16, kAny>(s, k, valid, m, lane);
    }
  }
}

int ensure_scratch(fslr_ctx* c, ScoreWork* w, int64_t n) {
  int rc;
  if (!w->pt && (rc = dalloc(c, &w->pt, kPassBytes))) return rc;
  if (n > w->cap) {
    w->cap = 0;                                   // (a failed growth leaves no buffer behind its capacity)
    const int64_t cap = std::min<int64_t>(kChunk, std::max<int64_t>(n + n / 4, 4096));
    if ((rc = dalloc(c, &w->ab, 2 * cap)) || (rc = dalloc(c, &w->out, cap))) return rc;
    w->cap = cap;
  }
  if (n > w->host_cap) {
    if (w->host) (void)hipHostFree(w->host);
    w->host = nullptr;
    w->host_cap = 0;
    HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&w->host), static_cast<size_t>(w->cap) * sizeof(unsigned),
                             hipHostMallocDefault));
    w->host_cap = w->cap;
  }
  return FSLR_OK;
}

// the checked batch of either entry point, chunk after chunk.  virt: the context holds virtual reads and the
// ranks are real ones (k_score_pairs<true>, the wide result word, umax); else k_score_pairs<false>
int score_run(fslr_ctx* c, const fslr_params* p, bool virt, const int32_t* umax, int32_t n_umax, int64_t n_pairs,
              const int32_t* a, const int32_t* b, int32_t* I, int32_t* U, uint8_t* flags) {
  const int64_t n_reads = virt ? c->lg_n_real : c->n;
  if (n_pairs == 0) return FSLR_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  if (!c->scw) c->scw = new ScoreWork();
  ScoreWork* w = c->scw;
  w->timed = false;
  w->ms[0] = w->ms[1] = w->ms[2] = 0;
  if (int rc = ensure_scratch(c, w, std::min(n_pairs, kChunk))) return rc;
  const bool prof = c->profiling;
  if (prof && !w->ev_ok) {
    for (hipEvent_t& e : w->ev) HIP_TRY(c, hipEventCreate(&e));
    w->ev_ok = true;
  }
  hipStream_t st = c->stream;
  const char* wide = std::getenv("FSLR_SCORE_WIDE");       // the timing tool's comparison only
  ScoreArgs s{c->rmeta, c->iv, w->pt, w->ab, w->ab + w->cap, w->out, 0, static_cast<int>(n_reads), static_cast<int>(c->ni),
              p->qlen_cut, p->nal_cut, wide && wide[0] == '1', c->lg_rlen, c->lg_off2, nullptr, 0};
  if (virt && umax) {
    if (n_umax > w->umax_cap) {
      w->umax_cap = 0;
      if (int rc = dalloc(c, &w->umax, n_umax)) return rc;
      w->umax_cap = n_umax;
    }
    HIP_TRY(c, hipMemcpyAsync(w->umax, umax, static_cast<size_t>(n_umax) * sizeof(int), hipMemcpyHostToDevice, st));
    s.umax = w->umax, s.n_umax = n_umax;
  }
  int64_t step = w->cap;
  // FSLR_SCORE_CHUNK (tests): a small launch chunk, so that a small batch spans several; anything but a
  // positive number is refused
  if (const char* e = std::getenv("FSLR_SCORE_CHUNK")) {
    char* end = nullptr;
    const long long v = std::strtoll(e, &end, 10);
    if (end == e || *end != '\0' || v < 1)
      return fail(c, FSLR_ERR_INVALID, std::string("FSLR_SCORE_CHUNK=") + e + " is not a positive pair count");
    step = std::min<int64_t>(step, v);
  }
  for (int64_t k0 = 0; k0 < n_pairs; k0 += step) {
    const int64_t m = std::min<int64_t>(step, n_pairs - k0);
    const size_t mb = static_cast<size_t>(m) * sizeof(int);
    if (prof) HIP_TRY(c, hipEventRecord(w->ev[0], st));
    if (k0 == 0) HIP_TRY(c, hipMemcpyAsync(w->pt, p->pass_table, kPassBytes, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(w->ab, a + k0, mb, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(w->ab + w->cap, b + k0, mb, hipMemcpyHostToDevice, st));
    if (prof) HIP_TRY(c, hipEventRecord(w->ev[1], st));
    s.n_pairs = static_cast<int>(m);
    if (virt)
      k_score_pairs<true><<<grid_for((m + 3) / 4, 4, 256 * 32), 256, 0, st>>>(s);
    else
      k_score_pairs<false><<<grid_for((m + 3) / 4, 4, 256 * 32), 256, 0, st>>>(s);
    HIP_TRY(c, hipGetLastError());
    if (prof) HIP_TRY(c, hipEventRecord(w->ev[2], st));
    HIP_TRY(c, hipMemcpyAsync(w->host, w->out, mb, hipMemcpyDeviceToHost, st));
    if (prof) HIP_TRY(c, hipEventRecord(w->ev[3], st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (virt)
      for (int64_t k = 0; k < m; ++k) fit_unpack_any(w->host[k], &I[k0 + k], &U[k0 + k], &flags[k0 + k]);
    else
      for (int64_t k = 0; k < m; ++k) fit_unpack(w->host[k], &I[k0 + k], &U[k0 + k], &flags[k0 + k]);
    if (prof)
      for (int t = 0; t < 3; ++t) {
        float ms = 0;
        HIP_TRY(c, hipEventElapsedTime(&ms, w->ev[t], w->ev[t + 1]));
        w->ms[t] += ms;
      }
  }
  w->timed = prof;
  return FSLR_OK;
}

}  // namespace

extern "C" {

int fslr_score_pairs(fslr_ctx* c, const fslr_params* p, int64_t n_pairs, const int32_t* a, const int32_t* b,
                     int32_t* I, int32_t* U, uint8_t* flags) {
  if (!c) return FSLR_ERR_INVALID;
  if (!p || !p->pass_table) return fail(c, FSLR_ERR_INVALID, "fslr_score_pairs: null params or pass_table");
  if (n_pairs < 0) return fail(c, FSLR_ERR_INVALID, "fslr_score_pairs: negative pair count");
  if (n_pairs && (!a || !b || !I || !U || !flags)) return fail(c, FSLR_ERR_INVALID, "fslr_score_pairs: null array");
  if (!c->reads_set) return fail(c, FSLR_ERR_STATE, "fslr_score_pairs: fslr_set_reads first");
  if (c->lg_set)
    return fail(c, FSLR_ERR_INVALID, "fslr_score_pairs: the context holds reads of more than " +
                                         std::to_string(FSLR_MAX_L) + " intervals (virtual reads), which it does not score");
  for (int64_t k = 0; k < n_pairs; ++k) {
    const bool bad_a = a[k] < 0 || a[k] >= c->n;
    if (bad_a || b[k] < 0 || b[k] >= c->n)
      return fail(c, FSLR_ERR_INVALID, std::string("fslr_score_pairs: ") + (bad_a ? "a[" : "b[") + std::to_string(k) +
                                           "] = " + std::to_string(bad_a ? a[k] : b[k]) + " is outside [0, " +
                                           std::to_string(c->n) + ")");
  }
  return score_run(c, p, false, nullptr, 0, n_pairs, a, b, I, U, flags);
}

int fslr_score_pairs_any(fslr_ctx* c, const fslr_params* p, const int32_t* umax, int32_t n_umax, int64_t n_pairs,
                         const int32_t* a, const int32_t* b, int32_t* I, int32_t* U, uint8_t* flags) {
  if (!c) return FSLR_ERR_INVALID;
  if (!p || !p->pass_table) return fail(c, FSLR_ERR_INVALID, "fslr_score_pairs_any: null params or pass_table");
  if (n_pairs < 0) return fail(c, FSLR_ERR_INVALID, "fslr_score_pairs_any: negative pair count");
  if (n_pairs && (!a || !b || !I || !U || !flags)) return fail(c, FSLR_ERR_INVALID, "fslr_score_pairs_any: null array");
  if (!c->reads_set) return fail(c, FSLR_ERR_STATE, "fslr_score_pairs_any: fslr_set_reads first");
  const bool virt = c->lg_set;
  if (virt && (!umax || n_umax < c->lg_max_len))
    return fail(c, FSLR_ERR_INVALID, "fslr_score_pairs_any: the context holds reads of more than " +
                                         std::to_string(FSLR_MAX_L) + " intervals: umax must cover I up to the longest read (" +
                                         std::to_string(c->lg_max_len) + ")");
  const int64_t n_real = virt ? c->lg_n_real : c->n;
  for (int64_t k = 0; k < n_pairs; ++k) {
    const bool bad_a = a[k] < 0 || a[k] >= n_real;
    if (bad_a || b[k] < 0 || b[k] >= n_real)
      return fail(c, FSLR_ERR_INVALID, std::string("fslr_score_pairs_any: ") + (bad_a ? "a[" : "b[") + std::to_string(k) +
                                           "] = " + std::to_string(bad_a ? a[k] : b[k]) + " is outside [0, " +
                                           std::to_string(n_real) + ")");
  }
  return score_run(c, p, virt, umax, n_umax, n_pairs, a, b, I, U, flags);
}

int fslr_score_timings(fslr_ctx* c, float* ms) {
  if (!c || !ms) return FSLR_ERR_INVALID;
  ScoreWork* w = c->scw;
  if (!w || !w->timed) return fail(c, FSLR_ERR_STATE, "fslr_score_timings: no profiled fslr_score_pairs (fslr_set_profiling 1)");
  for (int t = 0; t < 3; ++t) ms[t] = w->ms[t];
  return FSLR_OK;
}

}  // extern "C"
