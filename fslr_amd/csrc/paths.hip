// paths.hip — cluster paths: the distinct read structures of each cluster, the chain of (locus, strand) tokens
// each read walks, and how many reads agree on each (fslr_hip.h states the contract; DESIGN.md §3.10.3 the bytes;
// tests/paths_ref.py the plain statement).
//
// The loci rows are resident (loci.hip), the table gives cid[read], the caller brings the query key and the
// strand bit per CSR interval.  Passes, all on the context's stream:
//   k_path_count    flag[r] = the read is clustered, lens[r] = its intervals (else 0); path_of_read = -1 and
//                   flipped = 0 for the others
//   hipcub          exclusive sum of flag over n + 1 (pos[n] = m, the clustered reads), max of lens (Lmax)
//   k_path_compact  val[pos[r]] = r: the clustered reads in ascending rank
//   k_path_tokens   one lane per interval, lane groups of 16 / 32 / 64 by read length: the rank in the chain by
//                   shuffles, the locus row by a binary search, the tokens into LDS in chain order, the forward
//                   sequence against the backward one from the first lane where they differ (ballot), the
//                   canonical token + 1 to tok[first + j] (0 stands for "past the end"), flipped[r]
//   per position group, last to first: k_path_keys packs p tokens per 64-bit key (earlier position in the more
//                   significant bits, 0 past the read's end), a stable hipcub radix SortPairs of (key, read) on
//                   the p * kbits bits in use: an LSD radix sort over chain positions, so the final order is the
//                   lexicographic one with a prefix before its extensions and equal paths in ascending rank
//   k_path_heads    head[s] = the read at s differs from its predecessor's in length or in a token; hl = the
//                   head's length
//   hipcub scans    rid = exclusive sum of head, tsum = exclusive sum of hl, both over m + 1 (the totals)
//   k_path_hpos     hpos[rid] = s of each head
//   k_path_rows     one thread per row: n_reads = head distance, first_read = the head's read, tok_off, and
//                   off[c] for every cluster whose rows begin here
//   k_path_copy     one thread per row: its tokens as locus / rev
//   k_path_scatter  path_of_read[val[s]] = the row of s
// No block waits for another, every output word has one writer and no atomic is used, so the bytes are the same
// on every run.
#include <hipcub/hipcub.hpp>

#include <algorithm>
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
struct PathWork {
  // resident rows
  long long* off = nullptr;          // [n_clusters + 1]
  long long* tok_off = nullptr;      // [n_rows + 1]
  int* rows = nullptr;               // [2 x n_rows] n_reads, first_read
  int* locus = nullptr;              // [n_tokens]
  unsigned char* rev = nullptr;      // [n_tokens]
  int* path_of_read = nullptr;       // [n]
  unsigned char* flipped = nullptr;  // [n]
  int64_t n_rows = 0, n_tokens = 0, n_clusters = 0, n = 0;
  bool have = false;
  // the caller's columns, CSR interval order, and the canonical tokens + 1 beside them
  int* qkey = nullptr;               // [icap]
  unsigned char* qrev = nullptr;     // [icap]
  unsigned* tok = nullptr;           // [icap]
  int64_t icap = 0;
  // per read: flag, pos, lens; one more word for the longest
  int* rbuf = nullptr;               // [3 x (rcap + 1) + 1]
  int64_t rcap = 0;
  // fslr_cluster_paths_any on virtual reads: flag, pos and the list of the clustered reads of more than FSLR_MAX_L
  // intervals; gstart[g] = the clustered reads of at most g position groups, and its pinned copy
  int* lbuf = nullptr;               // [3 x (lcap + 1)]
  int64_t lcap = 0;
  int* gstart = nullptr;             // [kChainMaxL]
  int* gstart_host = nullptr;        // [kChainMaxL] pinned
  // per clustered read: sort keys in / out, then seven int columns: reads in / out, head, rid, hl, tsum, hpos
  unsigned long long* kbuf = nullptr;   // [2 x (mcap + 1)]
  int* mbuf = nullptr;                  // [7 x (mcap + 1)]
  int64_t mcap = 0;
  int* host = nullptr;               // [2] pinned: the counts read back
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

template <typename T>
void dfree(T*& p) {
  if (p) (void)hipFree(p);
  p = nullptr;
}

}  // namespace

void fslr_paths_drop(fslr_ctx* c) {
  if (c->ptw) c->ptw->have = false;
  fslr_segments_drop(c);                    // the segments fill these rows' slots
  fslr_containment_drop(c);                 // the containment rows name these rows
}

bool fslr_paths_view(const fslr_ctx* c, fslr_paths_rows* v) {
  const PathWork* w = c->ptw;
  if (!w || !w->have) return false;
  *v = fslr_paths_rows{w->tok_off, w->rows, w->path_of_read, w->flipped, w->n_rows, w->n_tokens, w->n_clusters, w->n,
                       w->locus, w->rev};
  return true;
}

void fslr_paths_free(fslr_ctx* c) {
  PathWork* w = c->ptw;
  if (!w) return;
  dfree(w->off), dfree(w->tok_off), dfree(w->rows), dfree(w->locus), dfree(w->rev), dfree(w->path_of_read);
  dfree(w->flipped), dfree(w->qkey), dfree(w->qrev), dfree(w->tok), dfree(w->rbuf), dfree(w->kbuf), dfree(w->mbuf);
  dfree(w->temp), dfree(w->lbuf), dfree(w->gstart);
  if (w->gstart_host) (void)hipHostFree(w->gstart_host);
  if (w->host) (void)hipHostFree(w->host);
  if (w->stage) (void)hipHostFree(w->stage);
  if (w->ev_ok)
    for (hipEvent_t e : w->ev) (void)hipEventDestroy(e);
  delete w;
  c->ptw = nullptr;
}

namespace {

// ---- count and compact --------------------------------------------------------------------------
// rlen: the real lengths on a context with virtual reads (n = the real reads), else null
__global__ __launch_bounds__(kBlock) void k_path_count(const int4* __restrict__ rmeta, const int* __restrict__ rlen,
                                                       const int* __restrict__ cid, long long n, int* __restrict__ flag, int* __restrict__ lens,
                                                       int* __restrict__ path_of_read, unsigned char* __restrict__ flipped) {
  for (long long r = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; r <= n; r += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(r, n + 1);
    int f = 0, l = 0;
    if (r < n) {
      if (cid[r] >= 0) {
        f = 1;
        l = rlen ? rlen[r] : (rmeta[r].y & 0xFFFF);
      } else {
        path_of_read[r] = -1;                       // a clustered read's words are k_path_scatter's and k_path_tokens'
        flipped[r] = 0;
      }
    }
    flag[r] = f;                                    // flag[n] = 0: the scan's last output is the total
    lens[r] = l;
  }
}

__global__ __launch_bounds__(kBlock) void k_path_compact(const int* __restrict__ flag, const int* __restrict__ pos,
                                                         long long n, long long m, int* __restrict__ val) {
  for (long long r = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; r < n; r += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(r, n);
    if (flag[r]) {
      FSLR_BOUND(pos[r], m);
      val[pos[r]] = static_cast<int>(r);
    }
  }
}

// ---- tokens -------------------------------------------------------------------------------------
struct TokenArgs {
  const int4* rmeta;
  const int *rlen, *off2;            // the real lists on a context with virtual reads (n = the real reads), else null
  const int* longs;                  // [n_long] the reads of k_path_tokens_long
  long long n_long;
  const int4* iv;                    // {chrom, start, end, thr}
  const int* cid;
  const int* qkey;
  const unsigned char* rev;          // null: all forward
  const long long* loff;             // the loci: [n_clusters + 1], then the chrom / start columns
  const int *lchrom, *lstart;
  long long n, ni, n_loci, n_clusters, n_quads;
  unsigned* tok;                     // [ni]
  unsigned char* flipped;            // [n]
};

// 64 / W reads side by side: read r (valid: it exists) on the W-lane group of this lane, interval j = the lane's
// place in the group.  lds: this wavefront's 64 slots.
template <int W>
__device__ __forceinline__ void token_group(const TokenArgs& a, long long r, bool valid, int lane, int* lds) {
  const int j = lane & (W - 1), gbase = lane & ~(W - 1);
  int len = 0, first = 0, c = -1;
  if (valid) {
    FSLR_BOUND(r, a.n);
    const int4 rm = a.rmeta[r];
    first = rm.x;
    len = a.rlen ? a.rlen[r] : (rm.y & 0xFFFF);
    c = a.cid[r];
    // len > W: a real read of more than FSLR_MAX_L intervals (k_path_tokens_long's; its first chunk is not a read
    // of its own); otherwise the caller chose W for its reads
    if (c < 0 || len > W) len = 0;
  }
  const bool have = j < len;
  int key = 0, rv = 0;
  int4 rec = make_int4(0, 0, 0, 0);
  if (have) {
    const long long k = static_cast<long long>(first) + j;
    FSLR_BOUND(k, a.ni);
    rec = a.iv[k];
    key = a.qkey[k];
    rv = a.rev ? (a.rev[k] != 0) : 0;
  }
  const int rank = chain_rank(key, len, j, gbase);
  if (have) lds[gbase + rank] = locus_of(a, c, rec.x, rec.y) * 2 + rv;      // rank < len <= W: the group's slots
  wave_lds_sync();
  // lane j: token j of the forward sequence against token j of the backward one
  int f = 0, b = 0;
  if (have) {
    f = lds[gbase + j];
    b = lds[gbase + len - 1 - j] ^ 1;
  }
  const unsigned long long wide = __ballot(have && f != b);
  const unsigned long long mine = (wide >> gbase) & (W == 64 ? ~0ull : (1ull << (W & 63)) - 1ull);
  int flip = 0;
  if (have && mine != 0ull) {                       // no difference: a palindrome, not flipped
    const int j0 = __ffsll(static_cast<long long>(mine)) - 1;      // j0 < len: only lanes with an interval vote
    flip = (lds[gbase + len - 1 - j0] ^ 1) < lds[gbase + j0];
  }
  if (have) {
    const long long k = static_cast<long long>(first) + j;
    FSLR_BOUND(k, a.ni);
    a.tok[k] = static_cast<unsigned>(flip ? b : f) + 1u;
    if (j == 0) a.flipped[r] = static_cast<unsigned char>(flip);
  }
  wave_lds_sync();                                  // the next pass writes the slots again
}

__global__ __launch_bounds__(kBlock) void k_path_tokens(TokenArgs a) {
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
      len = a.rlen ? a.rlen[r16] : (a.rmeta[r16].y & 0xFFFF);
      if (a.cid[r16] < 0 || len > FSLR_MAX_L) len = 0;
    }
    const bool over16 = __ballot(len > 16) != 0ull, over32 = __ballot(len > 32) != 0ull;
    if (__ballot(len > 0) == 0ull) continue;        // wave-uniform: nothing to write
    if (!over16) {
      token_group<16>(a, r16, r16 < a.n, lane, lds);
    } else if (!over32) {
      for (int p = 0; p < 2; ++p) {
        const long long r = r0 + 2 * p + (lane >> 5);
        token_group<32>(a, r, r < a.n, lane, lds);
      }
    } else {
      for (int p = 0; p < 4; ++p) token_group<64>(a, r0 + p, r0 + p < a.n, lane, lds);
    }
  }
}

// One workgroup per clustered read of more than FSLR_MAX_L intervals (a.longs): the chain order by an LDS sort,
// the thread that holds rank t stores its token in s_tok[t]; the first position where the forward and the
// backward sequence differ is the minimum over the waves' first ballots; the tokens there decide flipped, and
// the canonical token + 1 of position t goes to the t-th interval of the list.  48 KiB of LDS.
__global__ __launch_bounds__(kChainBlock) void k_path_tokens_long(TokenArgs a) {
  __shared__ unsigned long long s_w[kChainMaxL];
  __shared__ int s_tok[kChainMaxL];
  __shared__ int s_min[kChainBlock / kWave];
  const int lane = lane_id(), wv = threadIdx.x / kWave;
  for (long long q = blockIdx.x; q < a.n_long; q += gridDim.x) {
    FSLR_BOUND(q, a.n_long);
    const int r = a.longs[q];
    FSLR_BOUND(r, a.n);
    const int first = a.rmeta[r].x, len = min(a.rlen[r], kChainMaxL), off2 = a.off2[r], c = a.cid[r];
    chain_sort_lds(s_w, a.qkey, first, off2, len, a.ni);
    for (int t = threadIdx.x; t < len; t += kChainBlock) {
      FSLR_BOUND(t, kChainMaxL);
      const int j = static_cast<int>(s_w[t] & (kChainMaxL - 1));
      FSLR_BOUND(j, len);
      const long long k = list_at(first, off2, j);
      FSLR_BOUND(k, a.ni);
      const int4 rec = a.iv[k];
      s_tok[t] = locus_of(a, c, rec.x, rec.y) * 2 + (a.rev ? (a.rev[k] != 0) : 0);
    }
    __syncthreads();
    // wave wv sees positions base + 64 wv + lane in ascending base: its first ballot with a vote holds its minimum
    int wmin = kChainMaxL;
    for (int base = 0; base < len; base += kChainBlock) {          // block-uniform trip count
      const int t = base + static_cast<int>(threadIdx.x);
      bool diff = false;
      if (t < len) {
        FSLR_BOUND(len - 1 - t, kChainMaxL);
        diff = s_tok[t] != (s_tok[len - 1 - t] ^ 1);
      }
      const unsigned long long vote = __ballot(diff);
      if (vote != 0ull && wmin == kChainMaxL) wmin = base + wv * kWave + __ffsll(static_cast<long long>(vote)) - 1;
    }
    if (lane == 0) s_min[wv] = wmin;
    __syncthreads();
    int j0 = s_min[0];
#pragma unroll
    for (int k = 1; k < kChainBlock / kWave; ++k) j0 = min(j0, s_min[k]);
    int flip = 0;
    if (j0 < len) flip = (s_tok[len - 1 - j0] ^ 1) < s_tok[j0];   // no difference: a palindrome, not flipped
    for (int t = threadIdx.x; t < len; t += kChainBlock) {
      const long long k = list_at(first, off2, t);
      FSLR_BOUND(k, a.ni);
      a.tok[k] = static_cast<unsigned>(flip ? (s_tok[len - 1 - t] ^ 1) : s_tok[t]) + 1u;
    }
    if (threadIdx.x == 0) a.flipped[r] = static_cast<unsigned char>(flip);
    __syncthreads();                                // the next read writes the arrays again
  }
}

// ---- group --------------------------------------------------------------------------------------
// the position groups of each clustered read, G = ceil(len / p) >= 1: the key of the layout sort
__global__ __launch_bounds__(kBlock) void k_path_gkeys(const int* __restrict__ val, RealReads rr, long long m, long long n,
                                                       int p, int* __restrict__ gk) {
  for (long long s = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; s < m; s += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(s, m);
    const int r = val[s];
    FSLR_BOUND(r, n);
    gk[s] = (rr.len(r, rr.rmeta[r]) + p - 1) / p;
  }
}

// gk ascending: gstart[g] = the first s with gk[s] > g, for g in [0, n_groups)
__global__ __launch_bounds__(kBlock) void k_path_gstart(const int* __restrict__ gk, long long m, int n_groups,
                                                        int* __restrict__ gstart) {
  for (long long s = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; s <= m; s += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(s, m + 1);
    const int g0 = s == 0 ? 0 : gk[s - 1], g1 = s == m ? n_groups : gk[s];
    for (int g = max(g0, 0); g < min(g1, n_groups); ++g) {
      FSLR_BOUND(g, n_groups);
      gstart[g] = static_cast<int>(s);
    }
  }
}

// the sort key of position group [base, base + p): token base in the most significant of the p * kbits bits
__global__ __launch_bounds__(kBlock) void k_path_keys(const int* __restrict__ val, RealReads rr,
                                                      const unsigned* __restrict__ tok, long long m, long long n,
                                                      long long ni, int base, int p, int kbits,
                                                      unsigned long long* __restrict__ key) {
  for (long long s = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; s < m; s += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(s, m);
    const int r = val[s];
    FSLR_BOUND(r, n);
    const int4 rm = rr.rmeta[r];
    const int len = rr.len(r, rm), off2 = rr.second(r, len);
    unsigned long long k = 0;
    for (int i = 0; i < p; ++i) {
      unsigned t = 0;
      if (base + i < len) {
        const long long at = list_at(rm.x, off2, base + i);
        FSLR_BOUND(at, ni);
        t = tok[at];
      }
      k = (k << kbits) | t;                         // p * kbits <= 64 and t < 2^kbits: nothing is lost
    }
    key[s] = k;
  }
}

__global__ __launch_bounds__(kBlock) void k_path_heads(const int* __restrict__ val, RealReads rr,
                                                       const unsigned* __restrict__ tok, long long m, long long n,
                                                       long long ni, int* __restrict__ head, int* __restrict__ hl) {
  for (long long s = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; s <= m; s += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(s, m + 1);
    int h = 0, l = 0;
    if (s < m) {                                    // the scans run over m + 1: their last outputs are the totals
      const int r = val[s];
      FSLR_BOUND(r, n);
      const int4 rm = rr.rmeta[r];
      l = rr.len(r, rm);
      h = 1;
      if (s > 0) {
        const int q = val[s - 1];
        FSLR_BOUND(q, n);
        const int4 qm = rr.rmeta[q];
        if (rr.len(q, qm) == l) {
          const int r2 = rr.second(r, l), q2 = rr.second(q, l);
          FSLR_BOUND(list_at(rm.x, r2, l - 1), ni);
          FSLR_BOUND(list_at(qm.x, q2, l - 1), ni);
          int i = 0;
          while (i < l && tok[list_at(rm.x, r2, i)] == tok[list_at(qm.x, q2, i)]) ++i;
          h = i < l;
        }
      }
    }
    head[s] = h;
    hl[s] = h ? l : 0;
  }
}

__global__ __launch_bounds__(kBlock) void k_path_hpos(const int* __restrict__ head, const int* __restrict__ rid,
                                                      long long m, long long n_rows, int* __restrict__ hpos) {
  for (long long s = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; s < m; s += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(s, m);
    if (head[s]) {
      FSLR_BOUND(rid[s], n_rows);
      hpos[rid[s]] = static_cast<int>(s);
    }
  }
}

struct RowArgs {
  const int *val, *hpos, *tsum, *head, *rid;
  RealReads rr;
  const int* cid;
  const unsigned* tok;
  long long m, n, ni, n_rows, n_tokens, n_clusters;
  int* rows;                         // [2 x n_rows]
  long long *tok_off, *off;
  int* locus;
  unsigned char* rev;
  int* path_of_read;
};

__global__ __launch_bounds__(kBlock) void k_path_rows(RowArgs a) {
  for (long long l = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; l < a.n_rows; l += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(l, a.n_rows);
    const long long p0 = a.hpos[l], p1 = l + 1 < a.n_rows ? a.hpos[l + 1] : a.m;
    FSLR_BOUND(p0, a.m);
    FSLR_BOUND(p1, a.m + 1);
    const int r = a.val[p0];                        // the stable sort keeps equal paths in ascending rank
    FSLR_BOUND(r, a.n);
    a.rows[l] = static_cast<int>(p1 - p0);
    a.rows[a.n_rows + l] = r;
    a.tok_off[l] = a.tsum[p0];
    // off[c] = l for every cluster c whose rows begin at l.  The rows are in cluster order (a path's first token
    // lies in its cluster's loci rows), so the head's cid says which; a cluster always has rows.
    const long long c1 = a.cid[r];
    long long c0 = 0;
    if (l > 0) {
      FSLR_BOUND(a.hpos[l - 1], a.m);
      FSLR_BOUND(a.val[a.hpos[l - 1]], a.n);
      c0 = static_cast<long long>(a.cid[a.val[a.hpos[l - 1]]]) + 1;
    }
    for (long long c = c0; c <= c1; ++c) {
      FSLR_BOUND(c, a.n_clusters + 1);
      a.off[c] = l;
    }
    if (l == a.n_rows - 1) {
      a.tok_off[a.n_rows] = a.n_tokens;
      for (long long c = c1 + 1; c <= a.n_clusters; ++c) {
        FSLR_BOUND(c, a.n_clusters + 1);
        a.off[c] = a.n_rows;
      }
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_path_copy(RowArgs a) {
  for (long long l = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; l < a.n_rows; l += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(l, a.n_rows);
    const long long p0 = a.hpos[l];
    FSLR_BOUND(p0, a.m);
    const int r = a.val[p0];
    FSLR_BOUND(r, a.n);
    const int4 rm = a.rr.rmeta[r];
    const int len = a.rr.len(r, rm), off2 = a.rr.second(r, len);
    const long long o = a.tsum[p0];
    FSLR_BOUND(o + len, a.n_tokens + 1);
    FSLR_BOUND(list_at(rm.x, off2, len - 1), a.ni);
    for (int i = 0; i < len; ++i) {
      const unsigned t = a.tok[list_at(rm.x, off2, i)] - 1u;
      a.locus[o + i] = static_cast<int>(t >> 1);
      a.rev[o + i] = static_cast<unsigned char>(t & 1u);
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_path_scatter(RowArgs a) {
  for (long long s = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; s < a.m; s += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(s, a.m);
    const int r = a.val[s];
    FSLR_BOUND(r, a.n);
    const int row = a.rid[s] + a.head[s] - 1;       // rid counts the heads before s
    FSLR_BOUND(row, a.n_rows);
    a.path_of_read[r] = row;
  }
}

// ---- host side ----------------------------------------------------------------------------------
int bits_for(int64_t n_keys) {                   // bits that hold the keys 0 .. n_keys - 1, at least 1
  int b = 1;
  while ((int64_t(1) << b) < n_keys) ++b;
  return b;
}

// FSLR_PATHS_PACK: at most this many tokens per sort key (1..8), read per call; the tests set it to move the
// seams between the position groups
int pack_cap() {
  if (const char* e = std::getenv("FSLR_PATHS_PACK")) {
    const int v = std::atoi(e);
    if (v >= 1 && v <= 8) return v;
  }
  return 64;
}

int ensure_temp(fslr_ctx* c, PathWork* w, size_t bytes) {
  if (bytes <= w->temp_bytes && w->temp) return FSLR_OK;
  dfree(w->temp);
  w->temp_bytes = 0;
  HIP_TRY(c, hipMalloc(&w->temp, bytes ? bytes : 1));
  w->temp_bytes = bytes ? bytes : 1;
  return FSLR_OK;
}

// host -> device through the pinned chunk; each chunk syncs (the chunk is reused)
int up(fslr_ctx* c, PathWork* w, void* dst, const void* src, size_t bytes) {
  for (size_t at = 0; at < bytes; at += kStageBytes) {
    const size_t m = std::min(kStageBytes, bytes - at);
    std::memcpy(w->stage, static_cast<const unsigned char*>(src) + at, m);
    HIP_TRY(c, hipMemcpyAsync(static_cast<unsigned char*>(dst) + at, w->stage, m, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  return FSLR_OK;
}

// two device words to the host; syncs
int read_two(fslr_ctx* c, PathWork* w, const int* a, const int* b, int64_t* va, int64_t* vb) {
  HIP_TRY(c, hipMemcpyAsync(w->host, a, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(w->host + 1, b, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  *va = w->host[0];
  *vb = w->host[1];
  return FSLR_OK;
}

// the rows of a result (allocated apart from the resident ones: a failure keeps those)
struct NewRows {
  long long *off = nullptr, *tok_off = nullptr;
  int *rows = nullptr, *locus = nullptr, *path_of_read = nullptr;
  unsigned char *rev = nullptr, *flipped = nullptr;
  ~NewRows() {
    dfree(off), dfree(tok_off), dfree(rows), dfree(locus), dfree(path_of_read), dfree(rev), dfree(flipped);
  }
};

// fslr_cluster_paths (any = false: a context with virtual reads is refused) and fslr_cluster_paths_any.  On a
// context without virtual reads the two run the same code.
int paths_run(fslr_ctx* c, const int32_t* iv_qkey, const uint8_t* iv_rev, int64_t n_intervals, int64_t* n_rows_out,
              int64_t* n_tokens_out, bool any) {
  if (!c) return FSLR_ERR_INVALID;
  const char* who = any ? "fslr_cluster_paths_any" : "fslr_cluster_paths";
  if (!c->reads_set || c->n == 0) return fail(c, FSLR_ERR_STATE, "fslr_cluster_paths: no reads set");
  if (int rc = search_state(c, who)) return rc;
  const int* cid = nullptr;
  int64_t tn = 0, nc = 0;
  if (!fslr_cluster_view(c, &cid, &tn, &nc))
    return fail(c, FSLR_ERR_STATE, "fslr_cluster_paths: no cluster table (fslr_cluster_table first)");
  const int64_t n_real = c->lg_set ? c->lg_n_real : c->n;
  if (tn != n_real)
    return fail(c, FSLR_ERR_STATE, "fslr_cluster_paths: the cluster table holds " + std::to_string(tn) +
                                       " reads, the context " + std::to_string(n_real) +
                                       " (a table from before fslr_append_reads / fslr_remove_reads, or of other "
                                       "reads: fslr_cluster_table again)");
  const long long* loff = nullptr;
  const int* lrows = nullptr;
  int64_t lcap = 0, n_loci = 0, lnc = 0;
  if (!fslr_loci_view(c, &loff, &lrows, &lcap, &n_loci, &lnc) || lnc != nc)
    return fail(c, FSLR_ERR_STATE, "fslr_cluster_paths: no cluster loci of this table (fslr_cluster_loci first)");
  if (c->lg_set && !any)
    return fail(c, FSLR_ERR_INVALID, "fslr_cluster_paths: the context holds reads of more than " +
                                         std::to_string(FSLR_MAX_L) + " intervals (fslr_cluster_paths_any takes them)");
  if (!iv_qkey) return fail(c, FSLR_ERR_INVALID, "fslr_cluster_paths: iv_qkey is NULL");
  if (n_intervals != c->ni)
    return fail(c, FSLR_ERR_INVALID, "fslr_cluster_paths: n_intervals " + std::to_string(n_intervals) +
                                         ", the context holds " + std::to_string(c->ni));
  // n: the real reads (on a context with virtual reads the chunks behind them are no reads of their own)
  const bool virt = c->lg_set;
  const int64_t n = n_real, ni = c->ni;
  const RealReads rr{c->rmeta, virt ? c->lg_rlen : nullptr, virt ? c->lg_off2 : nullptr};
  if (virt && !c->lg_perm.empty() && static_cast<int64_t>(c->lg_perm.size()) != ni)
    return fail(c, FSLR_ERR_STATE, "fslr_cluster_paths: the interval permutation does not span the intervals (internal)");
  if (ni > kMaxItems || n >= kMaxItems)
    return fail(c, FSLR_ERR_INVALID, "fslr_cluster_paths: " + std::to_string(ni) + " intervals: more than 2^30");
  HIP_TRY(c, hipSetDevice(c->device));
  if (!c->ptw) c->ptw = new PathWork();
  PathWork* w = c->ptw;
  int rc;
  hipStream_t st = c->stream;
  if (!w->host) HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&w->host), 2 * sizeof(int), hipHostMallocDefault));
  if (!w->stage) HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&w->stage), kStageBytes, hipHostMallocDefault));
  if (c->profiling && !w->ev_ok) {
    for (hipEvent_t& e : w->ev) HIP_TRY(c, hipEventCreate(&e));
    w->ev_ok = true;
  }
  if (ni > w->icap || !w->qkey) {
    w->icap = 0;
    if ((rc = dalloc(c, &w->qkey, static_cast<size_t>(ni))) || (rc = dalloc(c, &w->qrev, static_cast<size_t>(ni))) ||
        (rc = dalloc(c, &w->tok, static_cast<size_t>(ni))))
      return rc;
    w->icap = ni;
  }
  if (n > w->rcap || !w->rbuf) {
    w->rcap = 0;
    if ((rc = dalloc(c, &w->rbuf, static_cast<size_t>(3 * (n + 1) + 1)))) return rc;
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
    if (!w->gstart)
      if ((rc = dalloc(c, &w->gstart, static_cast<size_t>(kChainMaxL)))) return rc;
    if (!w->gstart_host)
      HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&w->gstart_host), kChainMaxL * sizeof(int), hipHostMallocDefault));
  }
  int *flag = w->rbuf, *pos = flag + (w->rcap + 1), *lens = pos + (w->rcap + 1), *dmax = lens + (w->rcap + 1);
  const int n1 = static_cast<int>(n + 1);
  size_t tb_scan = 0, tb_max = 0;
  HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, tb_scan, flag, pos, n1, st));
  HIP_TRY(c, hipcub::DeviceReduce::Max(nullptr, tb_max, lens, dmax, n1, st));
  if ((rc = ensure_temp(c, w, std::max(tb_scan, tb_max)))) return rc;
  NewRows nr;
  if ((rc = dalloc(c, &nr.off, static_cast<size_t>(nc + 1))) || (rc = dalloc(c, &nr.path_of_read, static_cast<size_t>(n))) ||
      (rc = dalloc(c, &nr.flipped, static_cast<size_t>(n))))
    return rc;
  w->timed = false;
  w->ms = 0;
  if (virt && !c->lg_perm.empty()) {                // the caller's order is the real CSR's
    if ((rc = up_perm(c, w->stage, kStageBytes, w->qkey, iv_qkey, c->lg_perm))) return rc;
    if (iv_rev)
      if ((rc = up_perm(c, w->stage, kStageBytes, w->qrev, iv_rev, c->lg_perm))) return rc;
  } else {
    if ((rc = up(c, w, w->qkey, iv_qkey, static_cast<size_t>(ni) * sizeof(int)))) return rc;
    if (iv_rev)
      if ((rc = up(c, w, w->qrev, iv_rev, static_cast<size_t>(ni)))) return rc;
  }
  if (c->profiling) HIP_TRY(c, hipEventRecord(w->ev[0], st));     // the two columns are up: the device work from here
  k_path_count<<<grid_for(n + 1), kBlock, 0, st>>>(c->rmeta, rr.rlen, cid, n, flag, lens, nr.path_of_read, nr.flipped);
  HIP_TRY(c, hipGetLastError());
  size_t tb = w->temp_bytes;
  HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(w->temp, tb, flag, pos, n1, st));
  tb = w->temp_bytes;
  HIP_TRY(c, hipcub::DeviceReduce::Max(w->temp, tb, lens, dmax, n1, st));
  int64_t m = 0, lmax = 0;
  if ((rc = read_two(c, w, pos + n, dmax, &m, &lmax))) return rc;
  if (m < 0 || m > n || lmax < 0 || lmax > (virt ? FSLR_MAX_ANY_L : FSLR_MAX_L) || (m > 0) != (lmax > 0))
    return fail(c, FSLR_ERR_STATE, "fslr_cluster_paths: inconsistent counts (internal)");
  if (m > 0 && n_loci <= 0)
    return fail(c, FSLR_ERR_STATE, "fslr_cluster_paths: clustered reads without loci rows (internal)");

  int64_t n_rows = 0, n_tokens = 0;
  HIP_TRY(c, hipMemsetAsync(nr.off, 0, static_cast<size_t>(nc + 1) * sizeof(long long), st));
  if (m == 0) {
    if ((rc = dalloc(c, &nr.tok_off, 1))) return rc;
    HIP_TRY(c, hipMemsetAsync(nr.tok_off, 0, sizeof(long long), st));
  } else {
    if (m > w->mcap || !w->mbuf) {
      w->mcap = 0;
      if ((rc = dalloc(c, &w->kbuf, static_cast<size_t>(2 * (m + 1)))) || (rc = dalloc(c, &w->mbuf, static_cast<size_t>(7 * (m + 1)))))
        return rc;
      w->mcap = m;
    }
    const int64_t mc = w->mcap + 1;
    unsigned long long *key_in = w->kbuf, *key_out = w->kbuf + mc;
    int *val = w->mbuf, *val_alt = val + mc, *head = val_alt + mc, *rid = head + mc, *hl = rid + mc, *tsum = hl + mc, *hpos = tsum + mc;
    const int kbits = bits_for(2 * n_loci + 1);      // a token + 1 is at most 2 * n_loci <= 2^31
    const int pack = std::max(1, std::min(64 / kbits, pack_cap()));
    const int mi = static_cast<int>(m);
    size_t tb_sort = 0, tb_m = 0;
    HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(nullptr, tb_sort, key_in, key_out, val, val_alt, mi, 0, pack * kbits, st));
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, tb_m, head, rid, mi + 1, st));
    if ((rc = ensure_temp(c, w, std::max(tb_sort, tb_m)))) return rc;
    const int g = grid_for(m + 1);
    k_path_compact<<<grid_for(n), kBlock, 0, st>>>(flag, pos, n, m, val);
    HIP_TRY(c, hipGetLastError());
    const long long n_quads = (n + 3) / 4;
    // the clustered reads of more than FSLR_MAX_L intervals: flag, scan, compact
    int64_t n_long = 0;
    if (virt && lmax > FSLR_MAX_L) {
      int64_t unused = 0;
      k_chain_long_flag<<<grid_for(n + 1), kChainBlock, 0, st>>>(cid, rr.rlen, n, lflag);
      HIP_TRY(c, hipGetLastError());
      tb = w->temp_bytes;
      HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(w->temp, tb, lflag, lpos, n1, st));
      if ((rc = read_two(c, w, lpos + n, lpos + n, &n_long, &unused))) return rc;
      if (n_long < 1 || n_long > m) return fail(c, FSLR_ERR_STATE, "fslr_cluster_paths: inconsistent counts (internal)");
      k_chain_long_compact<<<grid_for(n), kChainBlock, 0, st>>>(lflag, lpos, n, n_long, longs);
      HIP_TRY(c, hipGetLastError());
    }
    TokenArgs ta{c->rmeta, rr.rlen, rr.off2, longs, n_long, c->iv, cid, w->qkey, iv_rev ? w->qrev : nullptr, loff, lrows, lrows + lcap,
                 n, ni, n_loci, nc, n_quads, w->tok, nr.flipped};
    k_path_tokens<<<grid_for(n_quads, kWavesPerBlock, 256 * 32), kBlock, 0, st>>>(ta);
    HIP_TRY(c, hipGetLastError());
    if (n_long > 0) {                                // only when such reads exist, one workgroup each
      k_path_tokens_long<<<grid_for(n_long, 1, 256 * 8), kChainBlock, 0, st>>>(ta);
      HIP_TRY(c, hipGetLastError());
    }
    // the LSD radix over position groups, last to first
    const int n_groups = static_cast<int>((lmax + pack - 1) / pack);
    if (!virt) {
      for (int grp = n_groups - 1; grp >= 0; --grp) {
        k_path_keys<<<g, kBlock, 0, st>>>(val, rr, w->tok, m, n, ni, grp * pack, pack, kbits, key_in);
        HIP_TRY(c, hipGetLastError());
        tb = w->temp_bytes;
        HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(w->temp, tb, key_in, key_out, val, val_alt, mi, 0, pack * kbits, st));
        std::swap(val, val_alt);
      }
    } else {
      // The same order from less work: a read of G = ceil(len / pack) groups has key 0 in every
      // pass grp >= G, so a full pass leaves it in front, in its initial place among such reads.  The reads are
      // laid out by (G, rank) and pass grp sorts only those of G > grp, the suffix from gstart[grp]: the reads of
      // G == grp + 1 stand in rank order right before the suffix the earlier passes sorted, the order a full pass
      // would have met them in.  Both buffers hold the layout, so the part before the suffix is valid in each.
      int *gk_in = reinterpret_cast<int*>(key_in), *gk_out = reinterpret_cast<int*>(key_out);
      size_t tb_g = 0;
      const int gbits = bits_for(static_cast<int64_t>(n_groups) + 1);
      HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(nullptr, tb_g, gk_in, gk_out, val, val_alt, mi, 0, gbits, st));
      if ((rc = ensure_temp(c, w, tb_g))) return rc;
      k_path_gkeys<<<g, kBlock, 0, st>>>(val, rr, m, n, pack, gk_in);
      HIP_TRY(c, hipGetLastError());
      tb = w->temp_bytes;
      HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(w->temp, tb, gk_in, gk_out, val, val_alt, mi, 0, gbits, st));
      HIP_TRY(c, hipMemcpyAsync(val, val_alt, static_cast<size_t>(m) * sizeof(int), hipMemcpyDeviceToDevice, st));
      k_path_gstart<<<g, kBlock, 0, st>>>(gk_out, m, n_groups, w->gstart);
      HIP_TRY(c, hipGetLastError());
      HIP_TRY(c, hipMemcpyAsync(w->gstart_host, w->gstart, static_cast<size_t>(n_groups) * sizeof(int), hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipStreamSynchronize(st));
      if (n_groups > kChainMaxL || w->gstart_host[0] != 0)
        return fail(c, FSLR_ERR_STATE, "fslr_cluster_paths: inconsistent counts (internal)");
      for (int grp = n_groups - 1; grp >= 0; --grp) {
        const int64_t s0 = w->gstart_host[grp];
        if (s0 < 0 || s0 >= m || (grp + 1 < n_groups && s0 > w->gstart_host[grp + 1]))
          return fail(c, FSLR_ERR_STATE, "fslr_cluster_paths: inconsistent counts (internal)");
        const int cnt = static_cast<int>(m - s0);
        size_t need = 0;
        HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(nullptr, need, key_in + s0, key_out + s0, val + s0, val_alt + s0, cnt, 0, pack * kbits, st));
        if (need > w->temp_bytes) {
          HIP_TRY(c, hipStreamSynchronize(st));       // the passes in flight use the buffer that goes
          if ((rc = ensure_temp(c, w, need))) return rc;
        }
        k_path_keys<<<grid_for(cnt), kBlock, 0, st>>>(val + s0, rr, w->tok, cnt, n, ni, grp * pack, pack, kbits, key_in + s0);
        HIP_TRY(c, hipGetLastError());
        tb = w->temp_bytes;
        HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(w->temp, tb, key_in + s0, key_out + s0, val + s0, val_alt + s0, cnt, 0, pack * kbits, st));
        std::swap(val, val_alt);
      }
    }
    k_path_heads<<<g, kBlock, 0, st>>>(val, rr, w->tok, m, n, ni, head, hl);
    HIP_TRY(c, hipGetLastError());
    tb = w->temp_bytes;
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(w->temp, tb, head, rid, mi + 1, st));
    tb = w->temp_bytes;
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(w->temp, tb, hl, tsum, mi + 1, st));
    if ((rc = read_two(c, w, rid + m, tsum + m, &n_rows, &n_tokens))) return rc;
    if (n_rows < 1 || n_rows > m || n_tokens < n_rows || n_tokens > ni)
      return fail(c, FSLR_ERR_STATE, "fslr_cluster_paths: inconsistent counts (internal)");
    if ((rc = dalloc(c, &nr.tok_off, static_cast<size_t>(n_rows + 1))) || (rc = dalloc(c, &nr.rows, static_cast<size_t>(2 * n_rows))) ||
        (rc = dalloc(c, &nr.locus, static_cast<size_t>(n_tokens))) || (rc = dalloc(c, &nr.rev, static_cast<size_t>(n_tokens))))
      return rc;
    k_path_hpos<<<g, kBlock, 0, st>>>(head, rid, m, n_rows, hpos);
    HIP_TRY(c, hipGetLastError());
    RowArgs ra{val, hpos, tsum, head, rid, rr, cid, w->tok, m, n, ni, n_rows, n_tokens, nc,
               nr.rows, nr.tok_off, nr.off, nr.locus, nr.rev, nr.path_of_read};
    k_path_rows<<<grid_for(n_rows), kBlock, 0, st>>>(ra);
    HIP_TRY(c, hipGetLastError());
    k_path_copy<<<grid_for(n_rows), kBlock, 0, st>>>(ra);
    HIP_TRY(c, hipGetLastError());
    k_path_scatter<<<g, kBlock, 0, st>>>(ra);
    HIP_TRY(c, hipGetLastError());
  }
  if (c->profiling) HIP_TRY(c, hipEventRecord(w->ev[1], st));
  HIP_TRY(c, hipStreamSynchronize(st));
  if (c->profiling) {
    HIP_TRY(c, hipEventElapsedTime(&w->ms, w->ev[0], w->ev[1]));
    w->timed = true;
  }
  // install
  fslr_segments_drop(c);                    // segments of the rows that go
  fslr_containment_drop(c);                 // and the containment rows that name them
  std::swap(w->off, nr.off);
  std::swap(w->tok_off, nr.tok_off);
  std::swap(w->rows, nr.rows);
  std::swap(w->locus, nr.locus);
  std::swap(w->rev, nr.rev);
  std::swap(w->path_of_read, nr.path_of_read);
  std::swap(w->flipped, nr.flipped);
  w->n_rows = n_rows;
  w->n_tokens = n_tokens;
  w->n_clusters = nc;
  w->n = n;
  w->have = true;
  if (n_rows_out) *n_rows_out = n_rows;
  if (n_tokens_out) *n_tokens_out = n_tokens;
  return FSLR_OK;
}

}  // namespace

extern "C" {

int fslr_cluster_paths(fslr_ctx* c, const int32_t* iv_qkey, const uint8_t* iv_rev, int64_t n_intervals,
                       int64_t* n_rows_out, int64_t* n_tokens_out) {
  return paths_run(c, iv_qkey, iv_rev, n_intervals, n_rows_out, n_tokens_out, false);
}

int fslr_cluster_paths_any(fslr_ctx* c, const int32_t* iv_qkey, const uint8_t* iv_rev, int64_t n_intervals,
                           int64_t* n_rows_out, int64_t* n_tokens_out) {
  return paths_run(c, iv_qkey, iv_rev, n_intervals, n_rows_out, n_tokens_out, true);
}

int fslr_get_cluster_paths(fslr_ctx* c, int64_t* off, int64_t* tok_off, int32_t* n_reads, int32_t* first_read,
                           int32_t* locus, uint8_t* rev, int32_t* path_of_read, uint8_t* flipped,
                           int64_t row_capacity, int64_t token_capacity) {
  if (!c) return FSLR_ERR_INVALID;
  PathWork* w = c->ptw;
  if (!w || !w->have) return fail(c, FSLR_ERR_STATE, "fslr_get_cluster_paths: fslr_cluster_paths first");
  if (row_capacity < w->n_rows)
    return fail(c, FSLR_ERR_INVALID, "fslr_get_cluster_paths: row capacity " + std::to_string(row_capacity) + " < " +
                                         std::to_string(w->n_rows) + " rows");
  if (token_capacity < w->n_tokens)
    return fail(c, FSLR_ERR_INVALID, "fslr_get_cluster_paths: token capacity " + std::to_string(token_capacity) +
                                         " < " + std::to_string(w->n_tokens) + " tokens");
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const size_t nr = static_cast<size_t>(w->n_rows), nt = static_cast<size_t>(w->n_tokens), n = static_cast<size_t>(w->n);
  if (off) HIP_TRY(c, hipMemcpyAsync(off, w->off, static_cast<size_t>(w->n_clusters + 1) * sizeof(long long), hipMemcpyDeviceToHost, st));
  if (tok_off) HIP_TRY(c, hipMemcpyAsync(tok_off, w->tok_off, (nr + 1) * sizeof(long long), hipMemcpyDeviceToHost, st));
  if (n_reads && nr) HIP_TRY(c, hipMemcpyAsync(n_reads, w->rows, nr * sizeof(int), hipMemcpyDeviceToHost, st));
  if (first_read && nr) HIP_TRY(c, hipMemcpyAsync(first_read, w->rows + nr, nr * sizeof(int), hipMemcpyDeviceToHost, st));
  if (locus && nt) HIP_TRY(c, hipMemcpyAsync(locus, w->locus, nt * sizeof(int), hipMemcpyDeviceToHost, st));
  if (rev && nt) HIP_TRY(c, hipMemcpyAsync(rev, w->rev, nt, hipMemcpyDeviceToHost, st));
  if (path_of_read && n) HIP_TRY(c, hipMemcpyAsync(path_of_read, w->path_of_read, n * sizeof(int), hipMemcpyDeviceToHost, st));
  if (flipped && n) HIP_TRY(c, hipMemcpyAsync(flipped, w->flipped, n, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  return FSLR_OK;
}

int fslr_cluster_paths_timings(fslr_ctx* c, float* ms) {
  if (!c || !ms) return FSLR_ERR_INVALID;
  PathWork* w = c->ptw;
  if (!w || !w->timed)
    return fail(c, FSLR_ERR_STATE, "fslr_cluster_paths_timings: no profiled fslr_cluster_paths (fslr_set_profiling 1 or 2)");
  ms[0] = w->ms;
  return FSLR_OK;
}

}  // extern "C"
