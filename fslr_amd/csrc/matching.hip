// matching.hip — the first-fit matching of scored pairs (fslr_pair_matching): for a batch
// of ordered read pairs, fslr_score_pairs' I, U and flags and, per pair, which interval of list1 took which
// interval of list2 in overall_jaccard_similarity's walk (cluster.py:152-161): I rows (i, j), i ascending.
//
// Two passes over a chunk of pairs, both the greedy of firstfit.hpp on the lane groups of score.hip:
//   count   k_pair_matching<kAny, false>: the result word per pair, as k_score_pairs writes it
//   scan    k_mt_scan<.., false>, k_mt_parts, k_mt_scan<.., true>: the exclusive scan of I, 1024 pairs per
//           block, into 64-bit row offsets (no atomics: a pair's rows have one place)
//   emit    k_pair_matching<kAny, true>: the fit again with the recording FirstFitT<true>; after it every
//           used lane holds (its column j, the row i that took it, that row's ordinal) and stores (i, j) at
//           off[k] + ordinal.  A pair that raised stores nothing.
// Long pairs (a list beyond FSLR_MAX_L, contexts with virtual reads): long_fit keeps the column of every
// matched row in LDS (u16 per row, 8 KiB per wave) and the rows are emitted in ascending order from the
// matched bits: each 64-row slice's popcount on its lane, a wave prefix for the slice's base, the rank
// inside the slice from the bits below the lane's.
// The emit pass runs over sub-ranges of the chunk whose rows fit the row scratch, so the scratch is bounded
// whatever the lists' lengths; each sub-range's rows are copied to the caller's arrays at the running offset.
// Algorithmic bytes per pair: fslr_score_pairs' (8 B ranks + 32 B rmeta + 16 B x (L1 + L2) in, 4 B out),
// 4 B + 8 B for the scan, 32 B + 16 B x (L1 + L2) + 8 B in again for the emit pass, 8 B x I rows out.
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

// the matching's scratch (grows only, bounded by the chunk and the row budget) and the last call's times
struct PairMatchingWork {
  int* ab = nullptr;                 // [2 x cap] the chunk's a, b
  unsigned* out = nullptr;           // [cap] the result words (narrow, or wide on a virtual context)
  long long* off = nullptr;          // [cap + 1] the chunk's row offsets
  long long* part = nullptr;         // [cap / kScanBlock + 1] the scan's block sums
  int64_t cap = 0;
  int* rows = nullptr;               // [2 x row_cap] a sub-range's row, then col
  int64_t row_cap = 0;
  unsigned char* pt = nullptr;       // [FSLR_MAX_L x kPassStride] the pass table
  int* umax = nullptr;               // [umax_cap] the _any call's cutoff table
  int umax_cap = 0;
  unsigned* host = nullptr;          // [host_cap] pinned: the chunk's result words
  int64_t host_cap = 0;
  hipEvent_t ev[7] = {};             // upload | count + scan | download || emit | download
  bool ev_ok = false, timed = false;
  float ms[3] = {0, 0, 0};
};

void fslr_pair_matching_free(fslr_ctx* c) {
  PairMatchingWork* w = c->pmw;
  if (!w) return;
  void* bufs[] = {w->ab, w->out, w->off, w->part, w->rows, w->pt, w->umax};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  if (w->host) (void)hipHostFree(w->host);
  if (w->ev_ok)
    for (hipEvent_t e : w->ev) (void)hipEventDestroy(e);
  delete w;
  c->pmw = nullptr;
}

namespace {

constexpr int64_t kChunk = int64_t(1) << 21;      // pairs per count launch, as fslr_score_pairs
constexpr int64_t kRowBudget = int64_t(1) << 23;  // rows per emit launch: 64 MiB of row scratch at most
constexpr int kScanBlock = 1024;                  // pairs per block of the scan
static_assert(kRowBudget >= FSLR_MAX_ANY_L, "one pair's rows fit the row scratch");

struct MatchingArgs {
  const int4* rmeta;
  const int4* iv;
  const unsigned char* pt;
  const int* a;
  const int* b;
  unsigned* out;                     // count pass: [n_pairs] the result words
  int n_pairs, n_reads, ni;          // <true>: n_reads counts the real reads
  double qcut, ncut;
  // <true> kernel only: real ranks on a context with virtual reads
  const int* rlen;
  const int* off2;
  const int* umax;
  int n_umax;
  // emit pass: pair k's rows go to row / col [off[k] - base, off[k + 1] - base)
  const long long* off;
  long long base, row_cap;
  int* row;
  int* col;
};

struct PairMeta {
  int offA, LA, offB, LB, gate;
  int offA2, offB2;                  // <true>: offA, offB are the first chunks, LA, LB the real lengths
};

template <bool kAny>
__device__ __forceinline__ PairMeta pair_meta(const MatchingArgs& s, int k, bool valid) {
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

// score.hip's group_fit with the state of the pass: list2's columns on the lanes of the W-lane group, list1
// loaded one record per lane in chunks of W rows and stepped in ascending order (so a recorded ordinal is
// the row's position in the output)
template <int W, bool kRec>
__device__ __forceinline__ FirstFitT<kRec> group_fit(const MatchingArgs& s, bool valid, const PairMeta& m, int lane) {
  const int l = lane & (W - 1);
  const int gbase = lane & ~(W - 1);
  const bool col = valid && l < m.LB;
  int4 bj = make_int4(-2, 0, 0, 0);
  if (col) {
    FSLR_BOUND(m.offB + l, s.ni);
    bj = s.iv[m.offB + l];
  }
  int max_la = valid ? m.LA : 0;
  max_la = max(max_la, __shfl_xor(max_la, 16));
  max_la = max(max_la, __shfl_xor(max_la, 32));
  max_la = rdl(max_la, 0);
  FirstFitT<kRec> ff;
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
      ff.template row<W>(c, si, ei, ti, r0 + i < m.LA, bj, col, lane, r0 + i);
    }
  }
  return ff;
}

template <bool kAny>
__device__ __forceinline__ unsigned pair_result(const MatchingArgs& s, const PairMeta& m, int I, bool zd) {
  if constexpr (kAny)
    return fit_result_any(m.LA, m.LB, I, zd, m.gate, s.pt, s.umax, s.n_umax);
  else
    return fit_result(m.LA, m.LB, I, zd, m.gate, s.pt);
}

// where row number `ord` of pair k goes; -1 (nothing is stored) outside the row scratch, which the count
// pass and the host's sub-ranges rule out
__device__ __forceinline__ long long row_slot(const MatchingArgs& s, int k, int ord) {
  const long long pos = s.off[k] - s.base + ord;
  FSLR_BOUND(pos, s.row_cap);
  FSLR_BOUND(pos, s.off[k + 1] - s.base);
  return pos >= 0 && pos < s.row_cap ? pos : -1;
}

// count: the pair's result word.  emit: every used lane stores (the row that took its column, its column)
template <int W, bool kAny, bool kEmit>
__device__ __forceinline__ void fit_groups(const MatchingArgs& s, int k, bool valid, const PairMeta& m, int lane) {
  const FirstFitT<kEmit> ff = group_fit<W, kEmit>(s, valid, m, lane);
  if constexpr (kEmit) {
    if (valid && !ff.zd && ff.used) {
      const long long pos = row_slot(s, k, ff.ord);
      if (pos >= 0) {
        s.row[pos] = ff.ri;
        s.col[pos] = lane & (W - 1);
      }
    }
  } else {
    if (valid && (lane & (W - 1)) == 0) s.out[k] = pair_result<kAny>(s, m, ff.I, ff.zd);
  }
}

// long_fit's recorder: the column of every matched row, u16 in this wave's LDS; the matched bits
struct ColumnRec {
  static constexpr bool on = true;
  unsigned short* colof;             // [FSLR_MAX_ANY_L]
  unsigned lo = 0, hi = 0;
  __device__ __forceinline__ void chunk(bool used, int ri, int j) {
    if (used) {
      FSLR_BOUND(ri, FSLR_MAX_ANY_L);
      colof[ri] = static_cast<unsigned short>(j);
    }
  }
  __device__ __forceinline__ void done(unsigned l, unsigned h) { lo = l, hi = h; }
};

// one long pair on the wave.  count: its result word.  emit: its rows in ascending order of i
template <bool kEmit>
__device__ __forceinline__ void fit_long(const MatchingArgs& s, int k, const PairMeta& m, int lane, unsigned short* colof) {
  const ReadList rows{s.iv, m.offA, m.offA2, s.ni}, cols{s.iv, m.offB, m.offB2, s.ni};
  int I = 0;
  bool zd = false;
  if constexpr (!kEmit) {
    long_fit(m.LA, m.LB, rows, cols, lane, &I, &zd);
    if (lane == 0) s.out[k] = pair_result<true>(s, m, I, zd);
  } else {
    ColumnRec rec{colof};
    long_fit(m.LA, m.LB, rows, cols, lane, &I, &zd, &rec);
    if (zd) return;
    wave_lds_sync();
    const int cnt = __popc(rec.lo) + __popc(rec.hi);         // slice `lane`'s matched rows
    const int before = wave_incl_scan(cnt) - cnt;
    const int nslice = (m.LA + kWave - 1) / kWave;
    for (int sl = 0; sl < nslice; ++sl) {
      const unsigned long long bits = static_cast<unsigned>(rdl(static_cast<int>(rec.lo), sl)) |
                                      (static_cast<unsigned long long>(static_cast<unsigned>(rdl(static_cast<int>(rec.hi), sl))) << 32);
      const int sbase = rdl(before, sl);
      if ((bits >> lane) & 1ull) {
        const int i = sl * kWave + lane;
        const long long pos = row_slot(s, k, sbase + __popcll(bits & ((1ull << lane) - 1)));
        if (pos >= 0) {
          s.row[pos] = i;
          s.col[pos] = colof[i];
        }
      }
    }
    wave_lds_sync();                 // the next long pair of this wave writes the same columns
  }
}

// The wave packing of k_score_pairs: four consecutive pairs per wave on 16-lane groups, two at a time on 32
// lanes or one at a time on 64 where a list2 of the four needs it; <true>: a wave that meets a list beyond
// FSLR_MAX_L runs its four pairs one at a time, the long ones through fit_long
template <bool kAny, bool kEmit>
__global__ __launch_bounds__(256) void k_pair_matching(MatchingArgs s) {
  __shared__ unsigned short colof_s[(kAny && kEmit) ? 4 * FSLR_MAX_ANY_L : 1];
  const int lane = threadIdx.x & 63;
  unsigned short* colof = (kAny && kEmit) ? colof_s + (threadIdx.x >> 6) * FSLR_MAX_ANY_L : colof_s;
  const int nq = (s.n_pairs + 3) >> 2;
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
          if (m1.LA > FSLR_MAX_L || m1.LB > FSLR_MAX_L)
            fit_long<kEmit>(s, k0 + p, m1, lane, colof);
          else
            fit_groups<64, kAny, kEmit>(s, k0 + p, true, m1, lane);
        }
        continue;
      }
    }
    const bool w64 = __ballot(m.LB > 32) != 0;
    const bool w32 = __ballot(m.LB > 16) != 0;
    if (w64) {
      for (int p = 0; p < 4 && k0 + p < s.n_pairs; ++p)
        fit_groups<64, kAny, kEmit>(s, k0 + p, true, pair_meta<kAny>(s, k0 + p, true), lane);
    } else if (w32) {
      for (int p = 0; p < 4 && k0 + p < s.n_pairs; p += 2) {
        const int k2 = k0 + p + (lane >> 5);
        const bool v2 = k2 < s.n_pairs;
        fit_groups<32, kAny, kEmit>(s, k2, v2, pair_meta<kAny>(s, k2, v2), lane);
      }
    } else {
      fit_groups<16, kAny, kEmit>(s, k, valid, m, lane);
    }
  }
}

// ---- the exclusive scan of I over a chunk: block sums, their scan by one wave, then the offsets ----------

// block b takes pairs [1024 b, 1024 b + 1024), four consecutive ones per thread.  <.., false>: part[b] = the
// block's rows.  <.., true>: off[k] = part[b] (by then the rows before the block) + the rows before k in it
template <bool kAny, bool kWrite>
__global__ __launch_bounds__(256) void k_mt_scan(const unsigned* __restrict__ out, int n, long long* __restrict__ part,
                                                 long long* __restrict__ off) {
  __shared__ int wsum[4];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const long long k0 = static_cast<long long>(blockIdx.x) * kScanBlock + t * 4;
  int v[4], sum = 0;
  for (int q = 0; q < 4; ++q) {
    v[q] = 0;
    if (k0 + q < n) v[q] = kAny ? any_I(out[k0 + q]) : static_cast<int>(out[k0 + q] & 0xff);
    sum += v[q];
  }
  const int incl = wave_incl_scan(sum);            // (a block's rows: at most 1024 x 4096)
  if (lane == kWave - 1) wsum[w] = incl;
  __syncthreads();
  int wbase = 0, total = 0;
  for (int x = 0; x < 4; ++x) {
    if (x < w) wbase += wsum[x];
    total += wsum[x];
  }
  if constexpr (!kWrite) {
    if (t == 0) part[blockIdx.x] = total;
  } else {
    long long o = part[blockIdx.x] + wbase + incl - sum;
    for (int q = 0; q < 4; ++q)
      if (k0 + q < n) {
        off[k0 + q] = o;
        o += v[q];
      }
  }
}

// one wave: part[] becomes its exclusive scan, *total the chunk's rows (off[n])
__global__ __launch_bounds__(64) void k_mt_parts(long long* __restrict__ part, int nb, long long* __restrict__ total) {
  const int lane = threadIdx.x;
  long long carry = 0;
  for (int b0 = 0; b0 < nb; b0 += kWave) {
    const long long x = b0 + lane < nb ? part[b0 + lane] : 0;
    long long inc = x;
    for (int d = 1; d < kWave; d <<= 1) {
      const long long y = __shfl_up(inc, d);
      if (lane >= d) inc += y;
    }
    if (b0 + lane < nb) part[b0 + lane] = carry + inc - x;
    carry += __shfl(inc, kWave - 1);
  }
  if (lane == 0) *total = carry;
}

int ensure_scratch(fslr_ctx* c, PairMatchingWork* w, int64_t n) {
  int rc;
  if (!w->pt && (rc = dalloc(c, &w->pt, kPassBytes))) return rc;
  if (n > w->cap) {
    w->cap = 0;                                   // (a failed growth leaves no buffer behind its capacity)
    const int64_t cap = std::min<int64_t>(kChunk, std::max<int64_t>(n + n / 4, 4096));
    if ((rc = dalloc(c, &w->ab, 2 * cap)) || (rc = dalloc(c, &w->out, cap)) || (rc = dalloc(c, &w->off, cap + 1)) ||
        (rc = dalloc(c, &w->part, cap / kScanBlock + 1)))
      return rc;
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

int ensure_rows(fslr_ctx* c, PairMatchingWork* w, int64_t n) {
  if (n <= w->row_cap) return FSLR_OK;
  w->row_cap = 0;
  const int64_t cap = std::min<int64_t>(kRowBudget, std::max<int64_t>(n + n / 4, FSLR_MAX_ANY_L));
  if (int rc = dalloc(c, &w->rows, 2 * cap)) return rc;
  w->row_cap = cap;
  return FSLR_OK;
}

// the checked batch of either entry point, chunk after chunk.  virt: the context holds virtual reads and the
// ranks are real ones (the <true> kernels, the wide result word, umax)
int matching_run(fslr_ctx* c, const char* who, const fslr_params* p, bool virt, const int32_t* umax, int32_t n_umax,
                 int64_t n_pairs, const int32_t* a, const int32_t* b, int32_t* I, int32_t* U, uint8_t* flags,
                 int64_t* row_off, int32_t* row, int32_t* col, int64_t capacity, int64_t* n_rows) {
  const int64_t n_reads = virt ? c->lg_n_real : c->n;
  row_off[0] = 0;
  *n_rows = 0;
  if (n_pairs == 0) return FSLR_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  if (!c->pmw) c->pmw = new PairMatchingWork();
  PairMatchingWork* w = c->pmw;
  w->timed = false;
  w->ms[0] = w->ms[1] = w->ms[2] = 0;
  if (int rc = ensure_scratch(c, w, std::min(n_pairs, kChunk))) return rc;
  const bool prof = c->profiling;
  if (prof && !w->ev_ok) {
    for (hipEvent_t& e : w->ev) HIP_TRY(c, hipEventCreate(&e));
    w->ev_ok = true;
  }
  hipStream_t st = c->stream;
  MatchingArgs s{c->rmeta, c->iv, w->pt, w->ab, w->ab + w->cap, w->out, 0, static_cast<int>(n_reads),
                 static_cast<int>(c->ni), p->qlen_cut, p->nal_cut, c->lg_rlen, c->lg_off2, nullptr, 0,
                 w->off, 0, 0, nullptr, nullptr};
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
  // FSLR_SCORE_CHUNK (tests): a small launch chunk, as fslr_score_pairs honours it
  if (const char* e = std::getenv("FSLR_SCORE_CHUNK")) {
    char* end = nullptr;
    const long long v = std::strtoll(e, &end, 10);
    if (end == e || *end != '\0' || v < 1)
      return fail(c, FSLR_ERR_INVALID, std::string("FSLR_SCORE_CHUNK=") + e + " is not a positive pair count");
    step = std::min<int64_t>(step, v);
  }
  // FSLR_MATCHING_ROWS (tests): a small row budget, so that a small chunk is emitted in several sub-ranges;
  // never below one pair's rows
  int64_t budget = kRowBudget;
  if (const char* e = std::getenv("FSLR_MATCHING_ROWS")) {
    char* end = nullptr;
    const long long v = std::strtoll(e, &end, 10);
    if (end == e || *end != '\0' || v < 1)
      return fail(c, FSLR_ERR_INVALID, std::string("FSLR_MATCHING_ROWS=") + e + " is not a positive row count");
    budget = std::min<int64_t>(budget, std::max<int64_t>(v, virt ? FSLR_MAX_ANY_L : FSLR_MAX_L));
  }
  auto lap = [&](int t, int e0, int e1) -> int {
    float ms = 0;
    HIP_TRY(c, hipEventElapsedTime(&ms, w->ev[e0], w->ev[e1]));
    w->ms[t] += ms;
    return FSLR_OK;
  };
  bool emit = row != nullptr && col != nullptr;    // until the rows no longer fit the caller's arrays
  int64_t total = 0;
  for (int64_t k0 = 0; k0 < n_pairs; k0 += step) {
    const int64_t m = std::min<int64_t>(step, n_pairs - k0);
    const size_t mb = static_cast<size_t>(m) * sizeof(int);
    const int nb = static_cast<int>((m + kScanBlock - 1) / kScanBlock);
    if (prof) HIP_TRY(c, hipEventRecord(w->ev[0], st));
    if (k0 == 0) HIP_TRY(c, hipMemcpyAsync(w->pt, p->pass_table, kPassBytes, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(w->ab, a + k0, mb, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(w->ab + w->cap, b + k0, mb, hipMemcpyHostToDevice, st));
    if (prof) HIP_TRY(c, hipEventRecord(w->ev[1], st));
    s.a = w->ab, s.b = w->ab + w->cap, s.out = w->out;
    s.n_pairs = static_cast<int>(m);
    const int grid = grid_for((m + 3) / 4, 4, 256 * 32);
    if (virt)
      k_pair_matching<true, false><<<grid, 256, 0, st>>>(s);
    else
      k_pair_matching<false, false><<<grid, 256, 0, st>>>(s);
    HIP_TRY(c, hipGetLastError());
    if (emit) {
      if (virt) {
        k_mt_scan<true, false><<<nb, 256, 0, st>>>(w->out, static_cast<int>(m), w->part, w->off);
        k_mt_parts<<<1, kWave, 0, st>>>(w->part, nb, w->off + m);
        k_mt_scan<true, true><<<nb, 256, 0, st>>>(w->out, static_cast<int>(m), w->part, w->off);
      } else {
        k_mt_scan<false, false><<<nb, 256, 0, st>>>(w->out, static_cast<int>(m), w->part, w->off);
        k_mt_parts<<<1, kWave, 0, st>>>(w->part, nb, w->off + m);
        k_mt_scan<false, true><<<nb, 256, 0, st>>>(w->out, static_cast<int>(m), w->part, w->off);
      }
      HIP_TRY(c, hipGetLastError());
    }
    if (prof) HIP_TRY(c, hipEventRecord(w->ev[2], st));
    HIP_TRY(c, hipMemcpyAsync(w->host, w->out, mb, hipMemcpyDeviceToHost, st));
    if (prof) HIP_TRY(c, hipEventRecord(w->ev[3], st));
    HIP_TRY(c, hipStreamSynchronize(st));
    const int64_t chunk_base = total;
    for (int64_t k = 0; k < m; ++k) {
      if (virt)
        fit_unpack_any(w->host[k], &I[k0 + k], &U[k0 + k], &flags[k0 + k]);
      else
        fit_unpack(w->host[k], &I[k0 + k], &U[k0 + k], &flags[k0 + k]);
      total += I[k0 + k];
      row_off[k0 + k + 1] = total;
    }
    if (prof)
      for (int t = 0; t < 3; ++t)
        if (int rc = lap(t, t, t + 1)) return rc;
    if (total > capacity) emit = false;
    if (!emit || total == chunk_base) continue;
    // the emit pass, over sub-ranges [p0, p1) of the chunk whose rows fit the row scratch
    if (int rc = ensure_rows(c, w, std::min<int64_t>(total - chunk_base, budget))) return rc;
    const int64_t lim = std::min<int64_t>(budget, w->row_cap);   // (a budget above the scratch: the chunk fits it)
    for (int64_t p0 = 0; p0 < m;) {
      const int64_t r0 = row_off[k0 + p0];
      int64_t p1 = p0 + 1;
      while (p1 < m && row_off[k0 + p1 + 1] - r0 <= lim) ++p1;
      const int64_t nr = row_off[k0 + p1] - r0;
      if (nr > 0) {
        s.a = w->ab + p0, s.b = w->ab + w->cap + p0, s.out = nullptr;
        s.n_pairs = static_cast<int>(p1 - p0);
        s.off = w->off + p0, s.base = r0 - chunk_base, s.row_cap = w->row_cap;
        s.row = w->rows, s.col = w->rows + w->row_cap;
        const int g = grid_for((p1 - p0 + 3) / 4, 4, 256 * 32);
        if (prof) HIP_TRY(c, hipEventRecord(w->ev[4], st));
        if (virt)
          k_pair_matching<true, true><<<g, 256, 0, st>>>(s);
        else
          k_pair_matching<false, true><<<g, 256, 0, st>>>(s);
        HIP_TRY(c, hipGetLastError());
        if (prof) HIP_TRY(c, hipEventRecord(w->ev[5], st));
        const size_t rb = static_cast<size_t>(nr) * sizeof(int);
        HIP_TRY(c, hipMemcpyAsync(row + r0, s.row, rb, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(col + r0, s.col, rb, hipMemcpyDeviceToHost, st));
        if (prof) HIP_TRY(c, hipEventRecord(w->ev[6], st));
        HIP_TRY(c, hipStreamSynchronize(st));
        if (prof) {
          if (int rc = lap(1, 4, 5)) return rc;
          if (int rc = lap(2, 5, 6)) return rc;
        }
      }
      p0 = p1;
    }
  }
  *n_rows = total;
  w->timed = prof;
  if (total > capacity && (row || col || capacity > 0))
    return fail(c, FSLR_ERR_INVALID, std::string(who) + ": the matching has " + std::to_string(total) +
                                         " rows, capacity is " + std::to_string(capacity));
  return FSLR_OK;
}

// the argument checks of both entry points; n_real: the rank space
int check_args(fslr_ctx* c, const char* who, const fslr_params* p, int64_t n_real, int64_t n_pairs, const int32_t* a,
               const int32_t* b, const int32_t* I, const int32_t* U, const uint8_t* flags, const int64_t* row_off,
               const int32_t* row, const int32_t* col, int64_t capacity, const int64_t* n_rows) {
  const std::string w(who);
  if (!p || !p->pass_table) return fail(c, FSLR_ERR_INVALID, w + ": null params or pass_table");
  if (n_pairs < 0) return fail(c, FSLR_ERR_INVALID, w + ": negative pair count");
  if (!row_off || !n_rows || (n_pairs && (!a || !b || !I || !U || !flags))) return fail(c, FSLR_ERR_INVALID, w + ": null array");
  if (capacity < 0 || (!row != !col) || (capacity > 0 && !row))
    return fail(c, FSLR_ERR_INVALID, w + ": row and col are both arrays of `capacity` rows, or both NULL with capacity 0");
  if (!c->reads_set) return fail(c, FSLR_ERR_STATE, w + ": fslr_set_reads first");
  for (int64_t k = 0; k < n_pairs && n_real >= 0; ++k) {
    const bool bad_a = a[k] < 0 || a[k] >= n_real;
    if (bad_a || b[k] < 0 || b[k] >= n_real)
      return fail(c, FSLR_ERR_INVALID, w + ": " + (bad_a ? "a[" : "b[") + std::to_string(k) + "] = " +
                                           std::to_string(bad_a ? a[k] : b[k]) + " is outside [0, " +
                                           std::to_string(n_real) + ")");
  }
  return FSLR_OK;
}

}  // namespace

extern "C" {

int fslr_pair_matching(fslr_ctx* c, const fslr_params* p, int64_t n_pairs, const int32_t* a, const int32_t* b, int32_t* I,
                       int32_t* U, uint8_t* flags, int64_t* row_off, int32_t* row, int32_t* col, int64_t capacity,
                       int64_t* n_rows) {
  if (!c) return FSLR_ERR_INVALID;
  const char* who = "fslr_pair_matching";
  if (int rc = check_args(c, who, p, -1, n_pairs, a, b, I, U, flags, row_off, row, col, capacity, n_rows)) return rc;
  if (c->lg_set)
    return fail(c, FSLR_ERR_INVALID, "fslr_pair_matching: the context holds reads of more than " +
                                         std::to_string(FSLR_MAX_L) + " intervals (virtual reads): fslr_pair_matching_any takes them");
  if (int rc = check_args(c, who, p, c->n, n_pairs, a, b, I, U, flags, row_off, row, col, capacity, n_rows)) return rc;
  return matching_run(c, who, p, false, nullptr, 0, n_pairs, a, b, I, U, flags, row_off, row, col, capacity, n_rows);
}

int fslr_pair_matching_any(fslr_ctx* c, const fslr_params* p, const int32_t* umax, int32_t n_umax, int64_t n_pairs,
                           const int32_t* a, const int32_t* b, int32_t* I, int32_t* U, uint8_t* flags, int64_t* row_off,
                           int32_t* row, int32_t* col, int64_t capacity, int64_t* n_rows) {
  if (!c) return FSLR_ERR_INVALID;
  const char* who = "fslr_pair_matching_any";
  if (int rc = check_args(c, who, p, -1, n_pairs, a, b, I, U, flags, row_off, row, col, capacity, n_rows)) return rc;
  const bool virt = c->lg_set;
  if (virt && (!umax || n_umax < c->lg_max_len))
    return fail(c, FSLR_ERR_INVALID, "fslr_pair_matching_any: the context holds reads of more than " +
                                         std::to_string(FSLR_MAX_L) + " intervals: umax must cover I up to the longest read (" +
                                         std::to_string(c->lg_max_len) + ")");
  const int64_t n_real = virt ? c->lg_n_real : c->n;
  if (int rc = check_args(c, who, p, n_real, n_pairs, a, b, I, U, flags, row_off, row, col, capacity, n_rows)) return rc;
  // without virtual reads: the plain call's driver and kernels
  return matching_run(c, who, p, virt, umax, n_umax, n_pairs, a, b, I, U, flags, row_off, row, col, capacity, n_rows);
}

int fslr_pair_matching_timings(fslr_ctx* c, float* ms) {
  if (!c || !ms) return FSLR_ERR_INVALID;
  PairMatchingWork* w = c->pmw;
  if (!w || !w->timed)
    return fail(c, FSLR_ERR_STATE, "fslr_pair_matching_timings: no profiled fslr_pair_matching (fslr_set_profiling 1)");
  for (int t = 0; t < 3; ++t) ms[t] = w->ms[t];
  return FSLR_OK;
}

}  // extern "C"
