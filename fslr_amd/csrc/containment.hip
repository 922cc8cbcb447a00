// containment.hip — path containment: which path rows of a cluster are contiguous sub-chains of a longer row, in
// either reading direction, and what a full-length row's support is once the truncated reads are counted
// (fslr_hip.h states the contract; DESIGN.md §3.10.7 the bytes; tests/containment_ref.py the plain statement).
//
// The path rows are resident (paths.hip): tok_off, n_reads, the tokens as locus / rev.  Nothing is uploaded.
// Passes, all on the context's stream:
//   k_ct_tokens     tok[s] = locus[s] * 2 + rev[s]; the sort's (token, slot) pairs
//   hipcub sort     stable radix SortPairs of (token, slot) on the token bits in use: the slots of a token value
//                   adjacent, in ascending slot order, which is ascending (row, position)
//   k_ct_occ        per sorted place: {slot, row, room = the tokens from the slot to its row's end, the row's
//                   length}, one 16-byte record per candidate; the row by a binary search in tok_off
//   k_ct_long_flag  flag[r] = row r has more than 64 tokens; a hipcub scan and k_ct_long_compact list those rows
//   k_ct_small      inner rows of at most 64 tokens, four to a wavefront on 16 lanes each, or two / one at a time
//                   on 32 / 64 lanes: lane j holds A[j] and rc(A)[j]; the range of the anchor token (A[0] forward,
//                   A[a-1] ^ 1 reverse) by two binary searches in the sorted tokens; per candidate with b > a and
//                   room >= a the lanes load B[p + j] and one ballot of "differs", shifted and masked to the group,
//                   decides
//   k_ct_long       inner rows of more than 64 tokens, one workgroup each, only when there are any: A and rc(A) in
//                   LDS, each wave tests positions in strides of 64 and stops at its first differing ballot, the
//                   four waves meet in LDS
//                   both kernels run twice: count (cnt[A]), a hipcub exclusive 64-bit sum, emit (the 64-bit key
//                   inner << rbits | outer and the value offset * 2 + d at base[A] + the occurrence's ordinal)
//   hipcub sort     stable radix SortPairs of the occurrences on the 2 * rbits key bits
//   k_ct_heads      head[i] = the key differs from its predecessor's; a hipcub scan numbers the pairs
//   k_ct_hpos       hpos[pair] = the head's place
//   k_ct_pairs      one thread per pair: outer, n_occ = the head distance, coff[A] for every inner row whose pairs
//                   begin here
//   k_ct_min        one thread per occurrence: atomicMin of offset * 2 + d into its pair's word
//   k_ct_rowinit    support = n_reads, n_inner = 0, collapsed_reads = 0
//   k_ct_support    one thread per pair: offset and rev from the word, n_inner and support of the outer by atomics
//   k_ct_collapse   one thread per row over its coff range: the argmax of (support, -row) over the maximal outers
//   k_ct_collapsed  collapsed_reads by atomics at collapse_to
// No atomic decides where anything lands: the atomics are integer minima and sums, which do not depend on the
// order.  No block waits for another, no floating point.  The bytes are the same on every run.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <string>

#include "ctx.hpp"
#include "fslr_hip.h"
#include "kernels.hpp"
#include "wave.hpp"

using namespace fslr;

// the resident rows, the scratch (grown on demand) and the last call's event time
struct ContainmentWork {
  // resident rows
  long long* coff = nullptr;         // [n_rows + 1]
  int* pairs = nullptr;              // [3 x n_pairs] outer, offset, n_occ
  unsigned char* prev = nullptr;     // [n_pairs] rev
  int* rows32 = nullptr;             // [2 x n_rows] n_inner, collapse_to
  long long* rows64 = nullptr;       // [2 x n_rows] support, collapsed_reads
  int64_t n_rows = 0, n_pairs = 0;
  bool have = false;
  // per token slot: tok, sort keys in / out, slots in / out; the candidate records
  unsigned* tbuf = nullptr;          // [5 x tcap]
  int4* occ = nullptr;               // [tcap]
  int64_t tcap = 0;
  // per row: flag, pos, the list of the rows of more than 64 tokens; the counts and their scan
  int* rbuf = nullptr;               // [3 x (rcap + 1)]
  long long* rbuf64 = nullptr;       // [2 x (rcap + 1)]
  int64_t rcap = 0;
  // per occurrence: keys in / out; values in / out, head, pair id, hpos
  unsigned long long* okey = nullptr;   // [2 x (ocap + 1)]
  int* oval = nullptr;                  // [5 x (ocap + 1)]
  int64_t ocap = 0;
  long long* host = nullptr;         // [2] pinned: the counts read back
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
constexpr int kSmallMax = 64;                               // a lane group is at most a wavefront
constexpr int kLongMax = FSLR_MAX_ANY_L;                    // the LDS words of k_ct_long: a row's tokens
constexpr int kLongBlock = 256;

template <typename T>
void dfree(T*& p) {
  if (p) (void)hipFree(p);
  p = nullptr;
}

}  // namespace

void fslr_containment_drop(fslr_ctx* c) {
  if (c->ctw) c->ctw->have = false;
  fslr_collapsed_drop(c);                   // the collapsed segments stand on these rows
}

bool fslr_containment_view(const fslr_ctx* c, fslr_containment_rows* v) {
  const ContainmentWork* w = c->ctw;
  if (!w || !w->have) return false;
  *v = fslr_containment_rows{w->coff, w->pairs, w->pairs ? w->pairs + w->n_pairs : nullptr, w->prev,
                             w->rows32 ? w->rows32 + w->n_rows : nullptr, w->n_rows, w->n_pairs};
  return true;
}

void fslr_containment_free(fslr_ctx* c) {
  ContainmentWork* w = c->ctw;
  if (!w) return;
  dfree(w->coff), dfree(w->pairs), dfree(w->prev), dfree(w->rows32), dfree(w->rows64), dfree(w->tbuf), dfree(w->occ);
  dfree(w->rbuf), dfree(w->rbuf64), dfree(w->okey), dfree(w->oval), dfree(w->temp);
  if (w->host) (void)hipHostFree(w->host);
  if (w->ev_ok)
    for (hipEvent_t e : w->ev) (void)hipEventDestroy(e);
  delete w;
  c->ctw = nullptr;
}

namespace {

// ---- the occurrence index -----------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_ct_tokens(const int* __restrict__ locus, const unsigned char* __restrict__ rev,
                                                      long long nt, unsigned* __restrict__ tok, unsigned* __restrict__ key,
                                                      unsigned* __restrict__ val) {
  for (long long s = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; s < nt; s += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(s, nt);
    const unsigned t = static_cast<unsigned>(locus[s]) * 2u + (rev[s] != 0);
    tok[s] = t;
    key[s] = t;
    val[s] = static_cast<unsigned>(s);
  }
}

// the candidate at sorted place i: x = its slot, y = its row, z = the tokens from the slot to the row's end,
// w = the row's length
__global__ __launch_bounds__(kBlock) void k_ct_occ(const unsigned* __restrict__ slot, const long long* __restrict__ tok_off,
                                                   long long nt, long long n_rows, int4* __restrict__ occ) {
  for (long long i = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; i < nt; i += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(i, nt);
    const long long s = slot[i];
    FSLR_BOUND(s, nt);
    long long lo = 0, hi = n_rows - 1;              // the last row whose tok_off is not above s
    for (int it = 0; it < 32 && lo < hi; ++it) {    // rows < 2^30: at most 30 halvings
      const long long mid = (lo + hi + 1) >> 1;
      FSLR_BOUND(mid, n_rows);
      if (tok_off[mid] <= s)
        lo = mid;
      else
        hi = mid - 1;
    }
    FSLR_BOUND(lo, n_rows);
    const long long t0 = tok_off[lo], t1 = tok_off[lo + 1];
    occ[i] = make_int4(static_cast<int>(s), static_cast<int>(lo), static_cast<int>(t1 - s), static_cast<int>(t1 - t0));
  }
}

__global__ __launch_bounds__(kBlock) void k_ct_long_flag(const long long* __restrict__ tok_off, long long n_rows,
                                                         int* __restrict__ flag, long long* __restrict__ cnt) {
  for (long long r = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; r <= n_rows; r += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(r, n_rows + 1);
    flag[r] = r < n_rows && tok_off[r + 1] - tok_off[r] > kSmallMax;      // flag[n_rows] = 0: the scan's last output is the total
    cnt[r] = 0;                                     // a row's probe kernel writes its count
  }
}

__global__ __launch_bounds__(kBlock) void k_ct_long_compact(const int* __restrict__ flag, const int* __restrict__ pos,
                                                            long long n_rows, long long n_long, int* __restrict__ out) {
  for (long long r = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; r < n_rows; r += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(r, n_rows);
    if (flag[r]) {
      FSLR_BOUND(pos[r], n_long);
      out[pos[r]] = static_cast<int>(r);
    }
  }
}

// ---- the probes ---------------------------------------------------------------------------------
struct ProbeArgs {
  const unsigned* tok;               // [nt]
  const unsigned* skey;              // [nt] the tokens, ascending
  const int4* occ;                   // [nt] the candidates in that order
  const long long* tok_off;          // [n_rows + 1]
  const int* longs;                  // [n_long] the rows of k_ct_long
  long long nt, n_rows, n_long, n_occ;
  int rbits;
  long long* cnt;                    // [n_rows + 1] count pass: the occurrences of each inner row
  const long long* base;             // [n_rows + 1] emit pass: their exclusive sum
  unsigned long long* okey;          // [n_occ] inner << rbits | outer
  int* oval;                         // [n_occ] offset * 2 + d
};

// the places [lo, hi) of token t in the sorted tokens
__device__ __forceinline__ void token_range(const ProbeArgs& a, unsigned t, long long* lo_out, long long* hi_out) {
  long long lo = 0, hi = a.nt;                      // the first place with a token >= t
  for (int it = 0; it < 32 && lo < hi; ++it) {      // tokens <= 2^30: at most 31 halvings
    const long long mid = (lo + hi) >> 1;
    FSLR_BOUND(mid, a.nt);
    if (a.skey[mid] < t)
      lo = mid + 1;
    else
      hi = mid;
  }
  *lo_out = lo;
  hi = a.nt;                                        // the first place with a token > t
  long long l2 = lo;
  for (int it = 0; it < 32 && l2 < hi; ++it) {
    const long long mid = (l2 + hi) >> 1;
    FSLR_BOUND(mid, a.nt);
    if (a.skey[mid] <= t)
      l2 = mid + 1;
    else
      hi = mid;
  }
  *hi_out = l2;
}

__device__ __forceinline__ void emit_occ(const ProbeArgs& a, long long r, long long ord, const int4& cand, int dir) {
  const long long at = a.base[r] + ord;
  FSLR_BOUND(at, a.n_occ);
  a.okey[at] = (static_cast<unsigned long long>(r) << a.rbits) | static_cast<unsigned>(cand.y);
  a.oval[at] = (cand.w - cand.z) * 2 + dir;         // the offset p = b - room
}

// 64 / W inner rows side by side: row r (valid: it exists) on the W-lane group of this lane, token j = the lane's
// place in the group
template <int W, bool EMIT>
__device__ __forceinline__ void probe_group(const ProbeArgs& a, long long r, bool valid, int lane) {
  const int j = lane & (W - 1), gbase = lane & ~(W - 1);
  const unsigned long long gmask = W == 64 ? ~0ull : (1ull << (W & 63)) - 1ull;
  long long t0 = 0;
  int len = 0;
  if (valid) {
    FSLR_BOUND(r, a.n_rows);
    t0 = a.tok_off[r];
    const long long l = a.tok_off[r + 1] - t0;
    // l > W: a row of k_ct_long, or the caller chose W for its rows
    if (l >= 1 && l <= W) len = static_cast<int>(l);
  }
  const bool have = j < len;
  unsigned fw = 0, bw = 0;
  if (have) {
    FSLR_BOUND(t0 + len - 1, a.nt);
    fw = a.tok[t0 + j];
    bw = a.tok[t0 + len - 1 - j] ^ 1u;
  }
  const bool pal = ((__ballot(have && fw != bw) >> gbase) & gmask) == 0ull;
  // the anchors: lane 0 of the group holds A[0] and rc(A)[0]
  const unsigned af = static_cast<unsigned>(__shfl(static_cast<int>(fw), gbase));
  const unsigned ab = static_cast<unsigned>(__shfl(static_cast<int>(bw), gbase));
  long long flo = 0, fhi = 0, blo = 0, bhi = 0;
  if (len > 0) {
    token_range(a, af, &flo, &fhi);
    if (!pal) token_range(a, ab, &blo, &bhi);       // a palindromic row: d = 0 alone
  }
  const long long nf = fhi - flo, total = nf + (bhi - blo);
  long long tmax = total;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) tmax = max(tmax, __shfl_xor(tmax, d));
  long long found = 0;
  for (long long i = 0; i < tmax; ++i) {            // tmax <= 2 nt, wave-uniform
    const bool act = i < total;
    const int dir = act && i >= nf;
    int4 cand = make_int4(0, 0, 0, 0);
    if (act) {
      const long long at = dir ? blo + (i - nf) : flo + i;
      FSLR_BOUND(at, a.nt);
      cand = a.occ[at];
    }
    const bool ok = act && cand.w > len && cand.z >= len;      // b > a and p + a <= b
    bool differs = false;
    if (ok && have) {
      FSLR_BOUND(static_cast<long long>(cand.x) + j, a.nt);
      differs = a.tok[static_cast<long long>(cand.x) + j] != (dir ? bw : fw);
    }
    const bool hit = ok && ((__ballot(differs) >> gbase) & gmask) == 0ull;
    if (hit) {
      if (EMIT && j == 0) emit_occ(a, r, found, cand, dir);
      ++found;
    }
  }
  if (!EMIT && j == 0 && len > 0) a.cnt[r] = found;
}

template <bool EMIT>
__global__ __launch_bounds__(kBlock) void k_ct_small(ProbeArgs a) {
  const int lane = lane_id(), wv = threadIdx.x / kWave;
  const long long n_quads = (a.n_rows + 3) / 4;
  // a wavefront takes four consecutive rows at a time
  for (long long q = blockIdx.x * static_cast<long long>(kWavesPerBlock) + wv; q < n_quads;
       q += gridDim.x * static_cast<long long>(kWavesPerBlock)) {
    const long long r0 = q * 4;
    const long long r16 = r0 + (lane >> 4);
    long long len = 0;
    if (r16 < a.n_rows) {
      FSLR_BOUND(r16, a.n_rows);
      len = a.tok_off[r16 + 1] - a.tok_off[r16];
      if (len > kSmallMax) len = 0;
    }
    const bool over16 = __ballot(len > 16) != 0ull, over32 = __ballot(len > 32) != 0ull;
    if (__ballot(len > 0) == 0ull) continue;        // wave-uniform: nothing to probe
    if (!over16) {
      probe_group<16, EMIT>(a, r16, r16 < a.n_rows, lane);
    } else if (!over32) {
      for (int p = 0; p < 2; ++p) {
        const long long r = r0 + 2 * p + (lane >> 5);
        probe_group<32, EMIT>(a, r, r < a.n_rows, lane);
      }
    } else {
      for (int p = 0; p < 4; ++p) probe_group<64, EMIT>(a, r0 + p, r0 + p < a.n_rows, lane);
    }
  }
}

// One workgroup per inner row of more than 64 tokens (a.longs): A and rc(A) in LDS, 32 KiB.  Per candidate wave w
// tests positions 64 w + 256 k + lane and stops at its first differing ballot; the waves' verdicts meet in s_diff,
// two sets of words used in turn so that one barrier per candidate is enough.
template <bool EMIT>
__global__ __launch_bounds__(kLongBlock) void k_ct_long(ProbeArgs a) {
  __shared__ unsigned s_fw[kLongMax];
  __shared__ unsigned s_bw[kLongMax];
  __shared__ int s_diff[2][kLongBlock / kWave];
  const int lane = lane_id(), wv = threadIdx.x / kWave;
  for (long long q = blockIdx.x; q < a.n_long; q += gridDim.x) {
    FSLR_BOUND(q, a.n_long);
    const long long r = a.longs[q];
    FSLR_BOUND(r, a.n_rows);
    const long long t0 = a.tok_off[r];
    const int len = static_cast<int>(min(a.tok_off[r + 1] - t0, static_cast<long long>(kLongMax)));   // bounds the LDS indices below
    if (len <= kSmallMax) continue;                 // block-uniform: no barrier is skipped by a part of the block
    FSLR_BOUND(t0 + len - 1, a.nt);
    for (int t = threadIdx.x; t < len; t += kLongBlock) {
      FSLR_BOUND(t, kLongMax);
      s_fw[t] = a.tok[t0 + t];
      s_bw[t] = a.tok[t0 + len - 1 - t] ^ 1u;
    }
    __syncthreads();
    // palindromic: no position where the two sequences differ
    bool differs = false;
    for (int base = wv * kWave; base < len; base += kLongBlock) {
      const int t = base + lane;
      bool d = false;
      if (t < len) {
        FSLR_BOUND(t, kLongMax);
        d = s_fw[t] != s_bw[t];
      }
      if (__ballot(d) != 0ull) {
        differs = true;
        break;
      }
    }
    if (lane == 0) s_diff[0][wv] = differs;
    __syncthreads();
    bool pal = true;
#pragma unroll
    for (int k = 0; k < kLongBlock / kWave; ++k) pal = pal && s_diff[0][k] == 0;
    long long flo = 0, fhi = 0, blo = 0, bhi = 0;
    token_range(a, s_fw[0], &flo, &fhi);
    if (!pal) token_range(a, s_bw[0], &blo, &bhi);
    const long long nf = fhi - flo, total = nf + (bhi - blo);
    long long found = 0;
    int turn = 1;                                   // set 0 was read above: the first candidate writes set 1
    for (long long i = 0; i < total; ++i) {         // total <= 2 nt, block-uniform
      const int dir = i >= nf;
      const long long at = dir ? blo + (i - nf) : flo + i;
      FSLR_BOUND(at, a.nt);
      const int4 cand = a.occ[at];
      if (!(cand.w > len && cand.z >= len)) continue;          // block-uniform
      FSLR_BOUND(static_cast<long long>(cand.x) + len - 1, a.nt);
      const unsigned* mine = dir ? s_bw : s_fw;
      differs = false;
      for (int base = wv * kWave; base < len; base += kLongBlock) {
        const int t = base + lane;
        bool d = false;
        if (t < len) {
          FSLR_BOUND(t, kLongMax);
          d = a.tok[static_cast<long long>(cand.x) + t] != mine[t];
        }
        if (__ballot(d) != 0ull) {                  // the first differing ballot ends the candidate for this wave
          differs = true;
          break;
        }
      }
      if (lane == 0) s_diff[turn][wv] = differs;
      __syncthreads();                              // the set of two candidates ago was read before the last barrier
      bool hit = true;
#pragma unroll
      for (int k = 0; k < kLongBlock / kWave; ++k) hit = hit && s_diff[turn][k] == 0;
      turn ^= 1;
      if (hit) {
        if (EMIT && threadIdx.x == 0) emit_occ(a, r, found, cand, dir);
        ++found;
      }
    }
    if (!EMIT && threadIdx.x == 0) a.cnt[r] = found;
    __syncthreads();                                // the next row writes the words again
  }
}

// ---- pairs --------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_ct_heads(const unsigned long long* __restrict__ key, long long n_occ,
                                                     int* __restrict__ head) {
  for (long long i = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; i <= n_occ; i += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(i, n_occ + 1);
    head[i] = i < n_occ && (i == 0 || key[i] != key[i - 1]);     // head[n_occ] = 0: the scan's last output is the total
  }
}

__global__ __launch_bounds__(kBlock) void k_ct_hpos(const int* __restrict__ head, const int* __restrict__ pid,
                                                    long long n_occ, long long n_pairs, int* __restrict__ hpos) {
  for (long long i = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; i < n_occ; i += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(i, n_occ);
    if (head[i]) {
      FSLR_BOUND(pid[i], n_pairs);
      hpos[pid[i]] = static_cast<int>(i);
    }
  }
}

struct PairArgs {
  const unsigned long long* key;     // [n_occ] sorted
  const int *val, *head, *pid, *hpos;
  const int* nreads;                 // [n_rows] the path rows' n_reads
  long long n_occ, n_pairs, n_rows;
  int rbits;
  long long* coff;                   // [n_rows + 1]
  int *outer, *offset, *nocc;        // [n_pairs]; offset holds offset * 2 + d until k_ct_support
  unsigned char* rev;                // [n_pairs]
  int *n_inner, *collapse_to;        // [n_rows]
  long long *support, *collapsed;    // [n_rows]
};

__global__ __launch_bounds__(kBlock) void k_ct_pairs(PairArgs a) {
  const unsigned long long rmask = (1ull << a.rbits) - 1ull;
  for (long long p = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; p < a.n_pairs; p += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(p, a.n_pairs);
    const long long h0 = a.hpos[p], h1 = p + 1 < a.n_pairs ? a.hpos[p + 1] : a.n_occ;
    FSLR_BOUND(h0, a.n_occ);
    FSLR_BOUND(h1, a.n_occ + 1);
    const unsigned long long k = a.key[h0];
    const long long in = static_cast<long long>(k >> a.rbits);
    FSLR_BOUND(in, a.n_rows);
    a.outer[p] = static_cast<int>(k & rmask);
    a.nocc[p] = static_cast<int>(h1 - h0);
    a.offset[p] = INT_MAX;                          // k_ct_min's word
    // coff[A] = p for every inner row A whose pairs begin at p: the rows after the previous pair's up to this one's
    long long c0 = 0;
    if (p > 0) {
      FSLR_BOUND(a.hpos[p - 1], a.n_occ);
      c0 = static_cast<long long>(a.key[a.hpos[p - 1]] >> a.rbits) + 1;
    }
    for (long long c = c0; c <= in; ++c) {
      FSLR_BOUND(c, a.n_rows + 1);
      a.coff[c] = p;
    }
    if (p == a.n_pairs - 1)
      for (long long c = in + 1; c <= a.n_rows; ++c) {
        FSLR_BOUND(c, a.n_rows + 1);
        a.coff[c] = a.n_pairs;
      }
  }
}

__global__ __launch_bounds__(kBlock) void k_ct_min(PairArgs a) {
  for (long long i = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; i < a.n_occ; i += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(i, a.n_occ);
    const long long p = static_cast<long long>(a.pid[i]) + a.head[i] - 1;       // pid counts the heads before i
    FSLR_BOUND(p, a.n_pairs);
    atomicMin(a.offset + p, a.val[i]);              // an integer minimum: the order does not matter
  }
}

// ---- per-row columns ----------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_ct_rowinit(PairArgs a) {
  for (long long r = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; r < a.n_rows; r += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(r, a.n_rows);
    a.n_inner[r] = 0;
    a.support[r] = a.nreads[r];
    a.collapsed[r] = 0;
  }
}

__global__ __launch_bounds__(kBlock) void k_ct_support(PairArgs a) {
  for (long long p = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; p < a.n_pairs; p += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(p, a.n_pairs);
    const int w = a.offset[p];
    a.offset[p] = w >> 1;
    a.rev[p] = static_cast<unsigned char>(w & 1);
    FSLR_BOUND(a.hpos[p], a.n_occ);
    const long long in = static_cast<long long>(a.key[a.hpos[p]] >> a.rbits);
    const int out = a.outer[p];
    FSLR_BOUND(in, a.n_rows);
    FSLR_BOUND(out, a.n_rows);
    atomicAdd(a.n_inner + out, 1);                  // integer sums: the order does not matter
    atomicAdd(reinterpret_cast<unsigned long long*>(a.support + out), static_cast<unsigned long long>(a.nreads[in]));
  }
}

__global__ __launch_bounds__(kBlock) void k_ct_collapse(PairArgs a) {
  for (long long r = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; r < a.n_rows; r += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(r, a.n_rows);
    const long long p0 = a.coff[r], p1 = a.coff[r + 1];
    long long best = r, bsup = -1;
    for (long long p = max(p0, 0ll); p < min(p1, a.n_pairs); ++p) {
      FSLR_BOUND(p, a.n_pairs);
      const int out = a.outer[p];
      FSLR_BOUND(out, a.n_rows);
      if (a.coff[out + 1] != a.coff[out]) continue;            // contained itself: not maximal
      const long long s = a.support[out];
      if (s > bsup) {                               // the outers ascend: a tie keeps the smaller row
        bsup = s;
        best = out;
      }
    }
    a.collapse_to[r] = static_cast<int>(best);
  }
}

__global__ __launch_bounds__(kBlock) void k_ct_collapsed(PairArgs a) {
  for (long long r = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; r < a.n_rows; r += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(r, a.n_rows);
    const int to = a.collapse_to[r];
    FSLR_BOUND(to, a.n_rows);
    atomicAdd(reinterpret_cast<unsigned long long*>(a.collapsed + to), static_cast<unsigned long long>(a.nreads[r]));
  }
}

// ---- host side ----------------------------------------------------------------------------------
int bits_for(int64_t n_keys) {                   // bits that hold the keys 0 .. n_keys - 1, at least 1
  int b = 1;
  while ((int64_t(1) << b) < n_keys) ++b;
  return b;
}

int ensure_temp(fslr_ctx* c, ContainmentWork* w, size_t bytes) {
  if (bytes <= w->temp_bytes && w->temp) return FSLR_OK;
  dfree(w->temp);
  w->temp_bytes = 0;
  HIP_TRY(c, hipMalloc(&w->temp, bytes ? bytes : 1));
  w->temp_bytes = bytes ? bytes : 1;
  return FSLR_OK;
}

// the rows of a result (allocated apart from the resident ones: a failure keeps those)
struct NewRows {
  long long *coff = nullptr, *rows64 = nullptr;
  int *pairs = nullptr, *rows32 = nullptr;
  unsigned char* prev = nullptr;
  ~NewRows() { dfree(coff), dfree(rows64), dfree(pairs), dfree(rows32), dfree(prev); }
};

int containment_run(fslr_ctx* c, int64_t* n_pairs_out) {
  if (!c) return FSLR_ERR_INVALID;
  const int* cid = nullptr;
  int64_t tn = 0, nc = 0;
  if (!fslr_cluster_view(c, &cid, &tn, &nc))
    return fail(c, FSLR_ERR_STATE, "fslr_cluster_path_containment: no cluster table (fslr_cluster_table first)");
  fslr_paths_rows pv;
  if (!fslr_paths_view(c, &pv) || pv.n_clusters != nc || pv.n != tn)
    return fail(c, FSLR_ERR_STATE, "fslr_cluster_path_containment: no cluster paths of this table (fslr_cluster_paths first)");
  const int64_t n_rows = pv.n_rows, nt = pv.n_tokens;
  if (n_rows < 0 || nt < n_rows || nt > kMaxItems || (n_rows > 0 && (!pv.locus || !pv.rev || !pv.rows)))
    return fail(c, FSLR_ERR_STATE, "fslr_cluster_path_containment: inconsistent path rows (internal)");
  // the sort's token bits: a token is below twice the loci rows; without that count all 32
  int kbits = 32;
  {
    const long long* loff = nullptr;
    const int* lrows = nullptr;
    int64_t lcap = 0, n_loci = 0, lnc = 0;
    if (fslr_loci_view(c, &loff, &lrows, &lcap, &n_loci, &lnc) && lnc == nc && n_loci > 0) kbits = std::min(32, bits_for(2 * n_loci));
  }
  HIP_TRY(c, hipSetDevice(c->device));
  if (!c->ctw) c->ctw = new ContainmentWork();
  ContainmentWork* w = c->ctw;
  int rc;
  hipStream_t st = c->stream;
  if (!w->host) HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&w->host), 2 * sizeof(long long), hipHostMallocDefault));
  if (c->profiling && !w->ev_ok) {
    for (hipEvent_t& e : w->ev) HIP_TRY(c, hipEventCreate(&e));
    w->ev_ok = true;
  }
  NewRows nr;
  if ((rc = dalloc(c, &nr.coff, static_cast<size_t>(n_rows + 1))) || (rc = dalloc(c, &nr.rows32, static_cast<size_t>(2 * n_rows))) ||
      (rc = dalloc(c, &nr.rows64, static_cast<size_t>(2 * n_rows))))
    return rc;
  w->timed = false;
  w->ms = 0;
  if (c->profiling) HIP_TRY(c, hipEventRecord(w->ev[0], st));
  HIP_TRY(c, hipMemsetAsync(nr.coff, 0, static_cast<size_t>(n_rows + 1) * sizeof(long long), st));
  int64_t n_pairs = 0;
  if (n_rows > 0) {
    if (nt > w->tcap || !w->tbuf) {
      w->tcap = 0;
      if ((rc = dalloc(c, &w->tbuf, static_cast<size_t>(5 * nt))) || (rc = dalloc(c, &w->occ, static_cast<size_t>(nt)))) return rc;
      w->tcap = nt;
    }
    if (n_rows > w->rcap || !w->rbuf) {
      w->rcap = 0;
      if ((rc = dalloc(c, &w->rbuf, static_cast<size_t>(3 * (n_rows + 1)))) || (rc = dalloc(c, &w->rbuf64, static_cast<size_t>(2 * (n_rows + 1)))))
        return rc;
      w->rcap = n_rows;
    }
    unsigned *tok = w->tbuf, *key_in = tok + w->tcap, *key_out = key_in + w->tcap, *val_in = key_out + w->tcap, *val_out = val_in + w->tcap;
    int *lflag = w->rbuf, *lpos = lflag + (w->rcap + 1), *longs = lpos + (w->rcap + 1);
    long long *cnt = w->rbuf64, *base = cnt + (w->rcap + 1);
    const int nti = static_cast<int>(nt), nr1 = static_cast<int>(n_rows + 1);
    size_t tb_sort = 0, tb_s32 = 0, tb_s64 = 0;
    HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(nullptr, tb_sort, key_in, key_out, val_in, val_out, nti, 0, kbits, st));
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, tb_s32, lflag, lpos, nr1, st));
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, tb_s64, cnt, base, nr1, st));
    if ((rc = ensure_temp(c, w, std::max(tb_sort, std::max(tb_s32, tb_s64))))) return rc;
    size_t tb;
    // the occurrence index
    k_ct_tokens<<<grid_for(nt), kBlock, 0, st>>>(pv.locus, pv.rev, nt, tok, key_in, val_in);
    HIP_TRY(c, hipGetLastError());
    tb = w->temp_bytes;
    HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(w->temp, tb, key_in, key_out, val_in, val_out, nti, 0, kbits, st));
    k_ct_occ<<<grid_for(nt), kBlock, 0, st>>>(val_out, pv.tok_off, nt, n_rows, w->occ);
    HIP_TRY(c, hipGetLastError());
    // the rows of more than 64 tokens: flag and scan; their count comes back
    k_ct_long_flag<<<grid_for(n_rows + 1), kBlock, 0, st>>>(pv.tok_off, n_rows, lflag, cnt);
    HIP_TRY(c, hipGetLastError());
    tb = w->temp_bytes;
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(w->temp, tb, lflag, lpos, nr1, st));
    HIP_TRY(c, hipMemcpyAsync(w->host, lpos + n_rows, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    const int64_t n_long = *reinterpret_cast<const int*>(w->host);
    if (n_long < 0 || n_long > n_rows) return fail(c, FSLR_ERR_STATE, "fslr_cluster_path_containment: inconsistent counts (internal)");
    const int rbits = bits_for(n_rows);
    ProbeArgs pa{tok, key_out, w->occ, pv.tok_off, longs, nt, n_rows, n_long, 0, rbits, cnt, base, nullptr, nullptr};
    const long long n_quads = (n_rows + 3) / 4;
    // count
    k_ct_small<false><<<grid_for(n_quads, kWavesPerBlock, 256 * 32), kBlock, 0, st>>>(pa);
    HIP_TRY(c, hipGetLastError());
    if (n_long > 0) {                                // only when such rows exist, one workgroup each
      k_ct_long_compact<<<grid_for(n_rows), kBlock, 0, st>>>(lflag, lpos, n_rows, n_long, longs);
      HIP_TRY(c, hipGetLastError());
      k_ct_long<false><<<grid_for(n_long, 1, 256 * 8), kLongBlock, 0, st>>>(pa);
      HIP_TRY(c, hipGetLastError());
    }
    tb = w->temp_bytes;
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(w->temp, tb, cnt, base, nr1, st));
    HIP_TRY(c, hipMemcpyAsync(w->host, base + n_rows, sizeof(long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    const int64_t n_occ = w->host[0];
    if (n_occ < 0) return fail(c, FSLR_ERR_STATE, "fslr_cluster_path_containment: inconsistent counts (internal)");
    if (n_occ > kMaxItems)
      return fail(c, FSLR_ERR_INVALID, "fslr_cluster_path_containment: " + std::to_string(n_occ) + " occurrences: more than 2^30");
    if (n_occ > 0) {
      if (n_occ > w->ocap || !w->okey) {
        w->ocap = 0;
        if ((rc = dalloc(c, &w->okey, static_cast<size_t>(2 * (n_occ + 1)))) || (rc = dalloc(c, &w->oval, static_cast<size_t>(5 * (n_occ + 1)))))
          return rc;
        w->ocap = n_occ;
      }
      const int64_t oc = w->ocap + 1;
      unsigned long long *ok_in = w->okey, *ok_out = ok_in + oc;
      int *ov_in = w->oval, *ov_out = ov_in + oc, *head = ov_out + oc, *pid = head + oc, *hpos = pid + oc;
      const int noi = static_cast<int>(n_occ);
      size_t tb_o = 0, tb_h = 0;
      HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(nullptr, tb_o, ok_in, ok_out, ov_in, ov_out, noi, 0, 2 * rbits, st));
      HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, tb_h, head, pid, noi + 1, st));
      if ((rc = ensure_temp(c, w, std::max(tb_o, tb_h)))) return rc;
      // emit
      pa.n_occ = n_occ, pa.okey = ok_in, pa.oval = ov_in;
      k_ct_small<true><<<grid_for(n_quads, kWavesPerBlock, 256 * 32), kBlock, 0, st>>>(pa);
      HIP_TRY(c, hipGetLastError());
      if (n_long > 0) {
        k_ct_long<true><<<grid_for(n_long, 1, 256 * 8), kLongBlock, 0, st>>>(pa);
        HIP_TRY(c, hipGetLastError());
      }
      // pairs
      tb = w->temp_bytes;
      HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(w->temp, tb, ok_in, ok_out, ov_in, ov_out, noi, 0, 2 * rbits, st));
      k_ct_heads<<<grid_for(n_occ + 1), kBlock, 0, st>>>(ok_out, n_occ, head);
      HIP_TRY(c, hipGetLastError());
      tb = w->temp_bytes;
      HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(w->temp, tb, head, pid, noi + 1, st));
      HIP_TRY(c, hipMemcpyAsync(w->host, pid + n_occ, sizeof(int), hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipStreamSynchronize(st));
      n_pairs = *reinterpret_cast<const int*>(w->host);
      if (n_pairs < 1 || n_pairs > n_occ) return fail(c, FSLR_ERR_STATE, "fslr_cluster_path_containment: inconsistent counts (internal)");
      if ((rc = dalloc(c, &nr.pairs, static_cast<size_t>(3 * n_pairs))) || (rc = dalloc(c, &nr.prev, static_cast<size_t>(n_pairs)))) return rc;
      PairArgs ga{ok_out, ov_out, head, pid, hpos, pv.rows, n_occ, n_pairs, n_rows, rbits, nr.coff,
                  nr.pairs, nr.pairs + n_pairs, nr.pairs + 2 * n_pairs, nr.prev,
                  nr.rows32, nr.rows32 + n_rows, nr.rows64, nr.rows64 + n_rows};
      k_ct_hpos<<<grid_for(n_occ), kBlock, 0, st>>>(head, pid, n_occ, n_pairs, hpos);
      HIP_TRY(c, hipGetLastError());
      k_ct_pairs<<<grid_for(n_pairs), kBlock, 0, st>>>(ga);
      HIP_TRY(c, hipGetLastError());
      k_ct_min<<<grid_for(n_occ), kBlock, 0, st>>>(ga);
      HIP_TRY(c, hipGetLastError());
      k_ct_rowinit<<<grid_for(n_rows), kBlock, 0, st>>>(ga);
      HIP_TRY(c, hipGetLastError());
      k_ct_support<<<grid_for(n_pairs), kBlock, 0, st>>>(ga);
      HIP_TRY(c, hipGetLastError());
      k_ct_collapse<<<grid_for(n_rows), kBlock, 0, st>>>(ga);
      HIP_TRY(c, hipGetLastError());
      k_ct_collapsed<<<grid_for(n_rows), kBlock, 0, st>>>(ga);
      HIP_TRY(c, hipGetLastError());
    } else {
      // no pair: every row is maximal and stands for itself (coff is all zero)
      PairArgs ga{nullptr, nullptr, nullptr, nullptr, nullptr, pv.rows, 0, 0, n_rows, rbits, nr.coff,
                  nullptr, nullptr, nullptr, nullptr, nr.rows32, nr.rows32 + n_rows, nr.rows64, nr.rows64 + n_rows};
      k_ct_rowinit<<<grid_for(n_rows), kBlock, 0, st>>>(ga);
      HIP_TRY(c, hipGetLastError());
      k_ct_collapse<<<grid_for(n_rows), kBlock, 0, st>>>(ga);
      HIP_TRY(c, hipGetLastError());
      k_ct_collapsed<<<grid_for(n_rows), kBlock, 0, st>>>(ga);
      HIP_TRY(c, hipGetLastError());
    }
  }
  if (c->profiling) HIP_TRY(c, hipEventRecord(w->ev[1], st));
  HIP_TRY(c, hipStreamSynchronize(st));
  if (c->profiling) {
    HIP_TRY(c, hipEventElapsedTime(&w->ms, w->ev[0], w->ev[1]));
    w->timed = true;
  }
  // install
  fslr_collapsed_drop(c);                   // collapsed segments of the rows that go
  std::swap(w->coff, nr.coff);
  std::swap(w->pairs, nr.pairs);
  std::swap(w->prev, nr.prev);
  std::swap(w->rows32, nr.rows32);
  std::swap(w->rows64, nr.rows64);
  w->n_rows = n_rows;
  w->n_pairs = n_pairs;
  w->have = true;
  if (n_pairs_out) *n_pairs_out = n_pairs;
  return FSLR_OK;
}

}  // namespace

extern "C" {

int fslr_cluster_path_containment(fslr_ctx* c, int64_t* n_pairs) { return containment_run(c, n_pairs); }

int fslr_get_cluster_path_containment(fslr_ctx* c, int64_t* coff, int32_t* outer, int32_t* offset, uint8_t* rev, int32_t* n_occ,
                                      int32_t* n_inner, int64_t* support, int32_t* collapse_to, int64_t* collapsed_reads,
                                      int64_t row_capacity, int64_t pair_capacity) {
  if (!c) return FSLR_ERR_INVALID;
  ContainmentWork* w = c->ctw;
  if (!w || !w->have)
    return fail(c, FSLR_ERR_STATE, "fslr_get_cluster_path_containment: fslr_cluster_path_containment first");
  if (row_capacity < w->n_rows)
    return fail(c, FSLR_ERR_INVALID, "fslr_get_cluster_path_containment: row capacity " + std::to_string(row_capacity) +
                                         " < " + std::to_string(w->n_rows) + " rows");
  if (pair_capacity < w->n_pairs)
    return fail(c, FSLR_ERR_INVALID, "fslr_get_cluster_path_containment: pair capacity " + std::to_string(pair_capacity) +
                                         " < " + std::to_string(w->n_pairs) + " pairs");
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const size_t nr = static_cast<size_t>(w->n_rows), np = static_cast<size_t>(w->n_pairs);
  if (coff) HIP_TRY(c, hipMemcpyAsync(coff, w->coff, (nr + 1) * sizeof(long long), hipMemcpyDeviceToHost, st));
  if (outer && np) HIP_TRY(c, hipMemcpyAsync(outer, w->pairs, np * sizeof(int), hipMemcpyDeviceToHost, st));
  if (offset && np) HIP_TRY(c, hipMemcpyAsync(offset, w->pairs + np, np * sizeof(int), hipMemcpyDeviceToHost, st));
  if (n_occ && np) HIP_TRY(c, hipMemcpyAsync(n_occ, w->pairs + 2 * np, np * sizeof(int), hipMemcpyDeviceToHost, st));
  if (rev && np) HIP_TRY(c, hipMemcpyAsync(rev, w->prev, np, hipMemcpyDeviceToHost, st));
  if (n_inner && nr) HIP_TRY(c, hipMemcpyAsync(n_inner, w->rows32, nr * sizeof(int), hipMemcpyDeviceToHost, st));
  if (collapse_to && nr) HIP_TRY(c, hipMemcpyAsync(collapse_to, w->rows32 + nr, nr * sizeof(int), hipMemcpyDeviceToHost, st));
  if (support && nr) HIP_TRY(c, hipMemcpyAsync(support, w->rows64, nr * sizeof(long long), hipMemcpyDeviceToHost, st));
  if (collapsed_reads && nr)
    HIP_TRY(c, hipMemcpyAsync(collapsed_reads, w->rows64 + nr, nr * sizeof(long long), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  return FSLR_OK;
}

int fslr_cluster_path_containment_timings(fslr_ctx* c, float* ms) {
  if (!c || !ms) return FSLR_ERR_INVALID;
  ContainmentWork* w = c->ctw;
  if (!w || !w->timed)
    return fail(c, FSLR_ERR_STATE,
                "fslr_cluster_path_containment_timings: no profiled fslr_cluster_path_containment (fslr_set_profiling 1 or 2)");
  ms[0] = w->ms;
  return FSLR_OK;
}

}  // extern "C"
