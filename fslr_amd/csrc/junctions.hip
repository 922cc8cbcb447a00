// junctions.hip — cluster junctions: which locus ends each cluster's reads join, and where the breakpoints
// lie (fslr_hip.h states the contract; DESIGN.md §3.10.2 the bytes; tests/junctions_ref.py the plain statement).
//
// A clustered read's intervals in query order are a chain of loci; each consecutive pair is one observation of
// a junction between two locus ends.  The loci rows are resident (loci.hip), the table gives cid[read], the
// caller brings the query key and the strand bit per CSR interval.  Passes, all on the context's stream:
//   k_jn_count      cnt[r] = L - 1 for a clustered read of L >= 2 intervals, else 0
//   hipcub scan     ofs = exclusive sum of cnt over n + 1: ofs[n] = M, the observations
//   k_jn_emit       one lane per interval, lane groups of 16 / 32 / 64 by read length (four short reads share a
//                   wavefront): the rank in the chain by shuffles, the locus row by a binary search in the
//                   cluster's rows, neighbours in the chain meet through LDS; observation ofs[r] + t gets the
//                   key ea << kbits | eb, the two breakpoints and the read
//   hipcub sort     stable radix SortPairs of (key, observation) on the 2 * kbits bits that hold the ends
//   k_jn_heads      head[p] = the key differs from its predecessor's; rflag[p] = head or another read
//   hipcub scans    rid = exclusive sum of head (R = the rows), rsum = exclusive sum of rflag over M + 1
//   k_jn_hpos       hpos[rid] = p of each head
//   k_jn_rows       one thread per row: the ends from the key, n_obs = head distance, n_reads = rsum difference,
//                   the breakpoint extrema seeded with the head's own, and off[c] for every cluster whose rows
//                   begin here
//   k_jn_minmax     every other element: integer atomicMin / atomicMax into its row's four extrema
// No block waits for another.  Every word but the extrema has one writer, the extrema take order-independent
// integer minima and maxima into rows that are already placed, so the bytes are the same on every run.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>
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
struct JunctionWork {
  // resident rows
  long long* off = nullptr;          // [n_clusters + 1]
  int* rows = nullptr;               // [8 x rows_cap] locus_a, locus_b, n_obs, n_reads, bp a_min, a_max, b_min, b_max
  unsigned char* sides = nullptr;    // [rows_cap] side_a | side_b << 1
  int64_t rows_cap = 0, n_rows = 0, n_clusters = 0;
  bool have = false;
  // the caller's columns, CSR interval order
  int* qkey = nullptr;               // [icap]
  unsigned char* rev = nullptr;      // [icap]
  int64_t icap = 0;
  // per read: cnt, ofs
  int* rbuf = nullptr;               // [2 x (rcap + 1)]
  int64_t rcap = 0;
  // fslr_cluster_junctions_any on virtual reads: flag, pos and the list of the clustered reads of more than
  // FSLR_MAX_L intervals
  int* lbuf = nullptr;               // [3 x (lcap + 1)]
  int64_t lcap = 0;
  // per observation: sort keys in / out (8 B each; the read flags and their scan reuse the input keys), then
  // seven int columns: vals in (the head flags after the sort), vals out, bp_a, bp_b, read, rid, hpos
  unsigned long long* kbuf = nullptr;   // [2 x (mcap + 1)]
  int* mbuf = nullptr;                  // [7 x (mcap + 1)]
  int64_t mcap = 0;
  long long* info = nullptr;         // [2] device; pinned copy below
  long long* host = nullptr;         // [2] pinned
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

void fslr_junctions_drop(fslr_ctx* c) {
  if (c->jnw) c->jnw->have = false;
}

void fslr_junctions_free(fslr_ctx* c) {
  JunctionWork* w = c->jnw;
  if (!w) return;
  dfree(w->off), dfree(w->rows), dfree(w->sides), dfree(w->qkey), dfree(w->rev), dfree(w->rbuf), dfree(w->kbuf);
  dfree(w->lbuf);
  dfree(w->mbuf), dfree(w->info), dfree(w->temp);
  if (w->host) (void)hipHostFree(w->host);
  if (w->stage) (void)hipHostFree(w->stage);
  if (w->ev_ok)
    for (hipEvent_t e : w->ev) (void)hipEventDestroy(e);
  delete w;
  c->jnw = nullptr;
}

namespace {

// ---- count --------------------------------------------------------------------------------------
// rlen: the real lengths on a context with virtual reads (n = the real reads), else null
__global__ __launch_bounds__(kBlock) void k_jn_count(const int4* __restrict__ rmeta, const int* __restrict__ rlen,
                                                     const int* __restrict__ cid, long long n, int* __restrict__ cnt) {
  for (long long r = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; r <= n; r += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(r, n + 1);
    int v = 0;
    if (r < n) {
      const int len = rlen ? rlen[r] : (rmeta[r].y & 0xFFFF);
      if (cid[r] >= 0 && len >= 2) v = len - 1;
    }
    cnt[r] = v;                                     // cnt[n] = 0: the scan's last output is the total
  }
}

__global__ void k_jn_last(const int* __restrict__ a, const int* __restrict__ b, long long last,
                          long long* __restrict__ out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *out = static_cast<long long>(a[last]) + (b ? b[last] : 0);
}

// ---- emit ---------------------------------------------------------------------------------------
struct EmitArgs {
  const int4* rmeta;
  const int *rlen, *off2;            // the real lists on a context with virtual reads (n = the real reads), else null
  const int* longs;                  // [n_long] the reads of k_jn_emit_long
  long long n_long;
  const int4* iv;                    // {chrom, start, end, thr}
  const int* cid;
  const int* qkey;
  const unsigned char* rev;          // null: all forward
  const int* ofs;                    // [n + 1] each read's first observation
  const long long* loff;             // the loci: [n_clusters + 1], then the chrom / start / end columns
  const int *lchrom, *lstart, *lend;
  long long n, ni, m, n_loci, n_clusters, n_quads;
  int kbits;
  unsigned long long* key;
  int *val, *bpa, *bpb, *rd;
};

// 64 / W reads side by side: read r (valid: it exists) on the W-lane group of this lane, interval j = the lane's
// place in the group.  lds: this wavefront's 64 slots.
template <int W>
__device__ __forceinline__ void emit_group(const EmitArgs& a, long long r, bool valid, int lane, int4* lds) {
  const int j = lane & (W - 1), gbase = lane & ~(W - 1);
  int len = 0, first = 0, c = -1;
  if (valid) {
    FSLR_BOUND(r, a.n);
    const int4 rm = a.rmeta[r];
    first = rm.x;
    len = a.rlen ? a.rlen[r] : (rm.y & 0xFFFF);
    c = a.cid[r];
    // len > W: a real read of more than FSLR_MAX_L intervals (k_jn_emit_long's; its first chunk is not a read of
    // its own); otherwise the caller chose W for its reads
    if (c < 0 || len < 2 || len > W) len = 0;
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
  if (have) {
    const int row = locus_of(a, c, rec.x, rec.y);
    // leaving this interval: its right end when it runs with the query, else its left end; entering it: the other
    const int e_out = row * 2 + (rv ? 0 : 1), bp_out = rv ? rec.y : rec.z;
    const int e_in = row * 2 + (rv ? 1 : 0), bp_in = rv ? rec.z : rec.y;
    lds[gbase + rank] = make_int4(e_out, bp_out, e_in, bp_in);      // rank < len <= W: inside the group's slots
  }
  wave_lds_sync();
  if (j + 1 < len) {
    const int4 x = lds[gbase + j], y = lds[gbase + j + 1];
    int ea = x.x, ba = x.y, eb = y.z, bb = y.w;
    // the unordered pair: the smaller end first, its breakpoint with it; on equal ends the smaller breakpoint
    if (ea > eb || (ea == eb && ba > bb)) {
      int t = ea; ea = eb; eb = t;
      t = ba; ba = bb; bb = t;
    }
    const long long o = static_cast<long long>(a.ofs[r]) + j;
    FSLR_BOUND(o, a.m);
    a.key[o] = (static_cast<unsigned long long>(static_cast<unsigned>(ea)) << a.kbits) | static_cast<unsigned>(eb);
    a.val[o] = static_cast<int>(o);
    a.bpa[o] = ba;
    a.bpb[o] = bb;
    a.rd[o] = static_cast<int>(r);
  }
  wave_lds_sync();                                  // the next pass writes the slots again
}

__global__ __launch_bounds__(kBlock) void k_jn_emit(EmitArgs a) {
  __shared__ int4 s_slot[kWavesPerBlock][kWave];
  const int lane = lane_id(), wv = threadIdx.x / kWave;
  int4* lds = s_slot[wv];
  // a wavefront takes four consecutive reads at a time
  for (long long q = blockIdx.x * static_cast<long long>(kWavesPerBlock) + wv; q < a.n_quads;
       q += gridDim.x * static_cast<long long>(kWavesPerBlock)) {
    const long long r0 = q * 4;
    const long long r16 = r0 + (lane >> 4);
    int len = 0;
    if (r16 < a.n) {
      FSLR_BOUND(r16, a.n);
      len = a.rlen ? a.rlen[r16] : (a.rmeta[r16].y & 0xFFFF);
      if (a.cid[r16] < 0 || len < 2 || len > FSLR_MAX_L) len = 0;
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

// One workgroup per clustered read of more than FSLR_MAX_L intervals (a.longs): the chain order by an LDS sort,
// thread t holds rank t: its interval's locus row, then what leaves it into s_w[t] and what enters it into
// s_in[t]; after the barrier thread t < L - 1 writes observation ofs[r] + t from s_w[t] and s_in[t + 1], as
// emit_group does.  64 KiB of LDS.
__global__ __launch_bounds__(kChainBlock) void k_jn_emit_long(EmitArgs a) {
  __shared__ unsigned long long s_w[kChainMaxL];
  __shared__ int2 s_in[kChainMaxL];
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
      const int rv = a.rev ? (a.rev[k] != 0) : 0;
      const int row = locus_of(a, c, rec.x, rec.y);
      const unsigned e_out = static_cast<unsigned>(row * 2 + (rv ? 0 : 1)), bp_out = static_cast<unsigned>(rv ? rec.y : rec.z);
      s_in[t] = make_int2(row * 2 + (rv ? 1 : 0), rv ? rec.z : rec.y);
      s_w[t] = (static_cast<unsigned long long>(e_out) << 32) | bp_out;     // rank t's own slot: no one else reads its word
    }
    __syncthreads();
    for (int t = threadIdx.x; t + 1 < len; t += kChainBlock) {
      FSLR_BOUND(t + 1, kChainMaxL);
      const unsigned long long x = s_w[t];
      const int2 y = s_in[t + 1];
      int ea = static_cast<int>(x >> 32), ba = static_cast<int>(static_cast<unsigned>(x)), eb = y.x, bb = y.y;
      if (ea > eb || (ea == eb && ba > bb)) {
        int u = ea; ea = eb; eb = u;
        u = ba; ba = bb; bb = u;
      }
      const long long o = static_cast<long long>(a.ofs[r]) + t;
      FSLR_BOUND(o, a.m);
      a.key[o] = (static_cast<unsigned long long>(static_cast<unsigned>(ea)) << a.kbits) | static_cast<unsigned>(eb);
      a.val[o] = static_cast<int>(o);
      a.bpa[o] = ba;
      a.bpb[o] = bb;
      a.rd[o] = r;
    }
    __syncthreads();                                // the next read writes the arrays again
  }
}

// ---- reduce -------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_jn_heads(const unsigned long long* __restrict__ key, const int* __restrict__ vo,
                                                     const int* __restrict__ rd, long long m, int* __restrict__ head,
                                                     int* __restrict__ rflag) {
  for (long long p = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; p <= m; p += gridDim.x * static_cast<long long>(kBlock)) {
    if (p == m) {                                   // the scan runs over m + 1 so that rsum[m] is the total
      rflag[p] = 0;
      continue;
    }
    FSLR_BOUND(p, m);
    int h = 1, f = 1;
    if (p > 0) {
      h = key[p] != key[p - 1];
      FSLR_BOUND(vo[p], m);
      FSLR_BOUND(vo[p - 1], m);
      f = h || rd[vo[p]] != rd[vo[p - 1]];          // the sort is stable: a read's observations of a key are adjacent
    }
    head[p] = h;
    rflag[p] = f;
  }
}

__global__ __launch_bounds__(kBlock) void k_jn_hpos(const int* __restrict__ head, const int* __restrict__ rid,
                                                    long long m, long long n_rows, int* __restrict__ hpos) {
  for (long long p = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; p < m; p += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(p, m);
    if (head[p]) {
      FSLR_BOUND(rid[p], n_rows);
      hpos[rid[p]] = static_cast<int>(p);
    }
  }
}

struct RowArgs {
  const unsigned long long* key;
  const int *vo, *bpa, *bpb, *hpos, *rsum, *head, *rid;
  const long long* loff;
  long long m, n_rows, n_clusters, n_loci, cap;
  int kbits;
  int* rows;                         // [8 x cap]
  unsigned char* sides;
  long long* off;
};

// the cluster whose loci rows hold row `locus`: the last c with loff[c] <= locus
__device__ __forceinline__ long long cluster_of(const long long* __restrict__ loff, long long n_clusters, long long locus) {
  long long lo = 0, hi = n_clusters - 1;
  for (int it = 0; it < 64 && lo < hi; ++it) {
    const long long mid = (lo + hi + 1) >> 1;
    FSLR_BOUND(mid, n_clusters + 1);
    if (loff[mid] <= locus)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(kBlock) void k_jn_rows(RowArgs a) {
  const unsigned long long mask = (1ull << a.kbits) - 1ull;
  for (long long l = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; l < a.n_rows; l += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(l, a.n_rows);
    const long long p0 = a.hpos[l], p1 = l + 1 < a.n_rows ? a.hpos[l + 1] : a.m;
    FSLR_BOUND(p0, a.m);
    FSLR_BOUND(p1, a.m + 1);
    const unsigned long long k = a.key[p0];
    const int ea = static_cast<int>(k >> a.kbits), eb = static_cast<int>(k & mask);
    const int o = a.vo[p0];
    FSLR_BOUND(o, a.m);
    FSLR_BOUND(7 * a.cap + l, 8 * a.cap);
    a.rows[l] = ea >> 1;
    a.rows[a.cap + l] = eb >> 1;
    a.rows[2 * a.cap + l] = static_cast<int>(p1 - p0);
    a.rows[3 * a.cap + l] = a.rsum[p1] - a.rsum[p0];
    const int ba = a.bpa[o], bb = a.bpb[o];
    a.rows[4 * a.cap + l] = ba;
    a.rows[5 * a.cap + l] = ba;
    a.rows[6 * a.cap + l] = bb;
    a.rows[7 * a.cap + l] = bb;
    a.sides[l] = static_cast<unsigned char>((ea & 1) | ((eb & 1) << 1));
    // off[c] = l for every cluster c whose rows begin at l (a cluster without rows begins where the next does)
    FSLR_BOUND(ea >> 1, a.n_loci);
    const long long c1 = cluster_of(a.loff, a.n_clusters, ea >> 1);
    long long c0 = 0;
    if (l > 0) {
      FSLR_BOUND(a.hpos[l - 1], a.m);
      c0 = cluster_of(a.loff, a.n_clusters, static_cast<long long>(a.key[a.hpos[l - 1]] >> a.kbits) >> 1) + 1;
    }
    for (long long c = c0; c <= c1; ++c) {
      FSLR_BOUND(c, a.n_clusters + 1);
      a.off[c] = l;
    }
    if (l == a.n_rows - 1)
      for (long long c = c1 + 1; c <= a.n_clusters; ++c) {
        FSLR_BOUND(c, a.n_clusters + 1);
        a.off[c] = a.n_rows;
      }
  }
}

// the elements behind a head fold their breakpoints into the row the head placed and seeded
__global__ __launch_bounds__(kBlock) void k_jn_minmax(RowArgs a) {
  for (long long p = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; p < a.m; p += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(p, a.m);
    if (a.head[p]) continue;
    const long long l = static_cast<long long>(a.rid[p]) - 1;      // heads before p, this row's included
    FSLR_BOUND(l, a.n_rows);
    const int o = a.vo[p];
    FSLR_BOUND(o, a.m);
    const int ba = a.bpa[o], bb = a.bpb[o];
    FSLR_BOUND(7 * a.cap + l, 8 * a.cap);
    atomicMin(a.rows + 4 * a.cap + l, ba);
    atomicMax(a.rows + 5 * a.cap + l, ba);
    atomicMin(a.rows + 6 * a.cap + l, bb);
    atomicMax(a.rows + 7 * a.cap + l, bb);
  }
}

// ---- host side ----------------------------------------------------------------------------------
int bits_for(int64_t n_keys) {                   // bits that hold the keys 0 .. n_keys - 1, at least 1
  int b = 1;
  while ((int64_t(1) << b) < n_keys) ++b;
  return b;
}

int ensure_temp(fslr_ctx* c, JunctionWork* w, size_t bytes) {
  if (bytes <= w->temp_bytes && w->temp) return FSLR_OK;
  dfree(w->temp);
  w->temp_bytes = 0;
  HIP_TRY(c, hipMalloc(&w->temp, bytes ? bytes : 1));
  w->temp_bytes = bytes ? bytes : 1;
  return FSLR_OK;
}

// host -> device through the pinned chunk; each chunk syncs (the chunk is reused)
int up(fslr_ctx* c, JunctionWork* w, void* dst, const void* src, size_t bytes) {
  for (size_t at = 0; at < bytes; at += kStageBytes) {
    const size_t m = std::min(kStageBytes, bytes - at);
    std::memcpy(w->stage, static_cast<const unsigned char*>(src) + at, m);
    HIP_TRY(c, hipMemcpyAsync(static_cast<unsigned char*>(dst) + at, w->stage, m, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  return FSLR_OK;
}

int read_last(fslr_ctx* c, JunctionWork* w, const int* a, const int* b, int64_t last, int64_t* out) {
  k_jn_last<<<1, 64, 0, c->stream>>>(a, b, last, w->info);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(w->host, w->info, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  *out = w->host[0];
  return FSLR_OK;
}

// the rows of a result (allocated apart from the resident ones: a failure keeps those)
struct NewRows {
  long long* off = nullptr;
  int* rows = nullptr;
  unsigned char* sides = nullptr;
  ~NewRows() {
    dfree(off);
    dfree(rows);
    dfree(sides);
  }
};

// fslr_cluster_junctions (any = false: a context with virtual reads is refused) and fslr_cluster_junctions_any.
// On a context without virtual reads the two run the same code.
int junctions_run(fslr_ctx* c, const int32_t* iv_qkey, const uint8_t* iv_rev, int64_t n_intervals, int64_t* n_rows_out,
                  bool any) {
  if (!c) return FSLR_ERR_INVALID;
  const char* who = any ? "fslr_cluster_junctions_any" : "fslr_cluster_junctions";
  if (!c->reads_set || c->n == 0) return fail(c, FSLR_ERR_STATE, "fslr_cluster_junctions: no reads set");
  if (int rc = search_state(c, who)) return rc;
  const int* cid = nullptr;
  int64_t tn = 0, nc = 0;
  if (!fslr_cluster_view(c, &cid, &tn, &nc))
    return fail(c, FSLR_ERR_STATE, "fslr_cluster_junctions: no cluster table (fslr_cluster_table first)");
  const int64_t n_real = c->lg_set ? c->lg_n_real : c->n;
  if (tn != n_real)
    return fail(c, FSLR_ERR_STATE, "fslr_cluster_junctions: the cluster table holds " + std::to_string(tn) +
                                       " reads, the context " + std::to_string(n_real) +
                                       " (a table from before fslr_append_reads / fslr_remove_reads, or of other "
                                       "reads: fslr_cluster_table again)");
  const long long* loff = nullptr;
  const int* lrows = nullptr;
  int64_t lcap = 0, n_loci = 0, lnc = 0;
  if (!fslr_loci_view(c, &loff, &lrows, &lcap, &n_loci, &lnc) || lnc != nc)
    return fail(c, FSLR_ERR_STATE, "fslr_cluster_junctions: no cluster loci of this table (fslr_cluster_loci first)");
  if (c->lg_set && !any)
    return fail(c, FSLR_ERR_INVALID, "fslr_cluster_junctions: the context holds reads of more than " +
                                         std::to_string(FSLR_MAX_L) + " intervals (fslr_cluster_junctions_any takes them)");
  if (!iv_qkey) return fail(c, FSLR_ERR_INVALID, "fslr_cluster_junctions: iv_qkey is NULL");
  if (n_intervals != c->ni)
    return fail(c, FSLR_ERR_INVALID, "fslr_cluster_junctions: n_intervals " + std::to_string(n_intervals) +
                                         ", the context holds " + std::to_string(c->ni));
  // n: the real reads (on a context with virtual reads the chunks behind them are no reads of their own)
  const bool virt = c->lg_set;
  const int64_t n = n_real, ni = c->ni;
  const int *rlen = virt ? c->lg_rlen : nullptr, *off2 = virt ? c->lg_off2 : nullptr;
  if (virt && !c->lg_perm.empty() && static_cast<int64_t>(c->lg_perm.size()) != ni)
    return fail(c, FSLR_ERR_STATE, "fslr_cluster_junctions: the interval permutation does not span the intervals (internal)");
  if (ni > kMaxItems || n >= kMaxItems)
    return fail(c, FSLR_ERR_INVALID, "fslr_cluster_junctions: " + std::to_string(ni) +
                                         " intervals: the observations may exceed 2^30");
  HIP_TRY(c, hipSetDevice(c->device));
  if (!c->jnw) c->jnw = new JunctionWork();
  JunctionWork* w = c->jnw;
  int rc;
  hipStream_t st = c->stream;
  if (!w->info)
    if ((rc = dalloc(c, &w->info, 2))) return rc;
  if (!w->host) HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&w->host), 2 * sizeof(long long), hipHostMallocDefault));
  if (!w->stage) HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&w->stage), kStageBytes, hipHostMallocDefault));
  if (c->profiling && !w->ev_ok) {
    for (hipEvent_t& e : w->ev) HIP_TRY(c, hipEventCreate(&e));
    w->ev_ok = true;
  }
  if (ni > w->icap || !w->qkey) {
    w->icap = 0;
    if ((rc = dalloc(c, &w->qkey, static_cast<size_t>(ni))) || (rc = dalloc(c, &w->rev, static_cast<size_t>(ni)))) return rc;
    w->icap = ni;
  }
  if (n > w->rcap || !w->rbuf) {
    w->rcap = 0;
    if ((rc = dalloc(c, &w->rbuf, static_cast<size_t>(2 * (n + 1))))) return rc;
    w->rcap = n;
  }
  if (virt && (n > w->lcap || !w->lbuf)) {
    w->lcap = 0;
    if ((rc = dalloc(c, &w->lbuf, static_cast<size_t>(3 * (n + 1))))) return rc;
    w->lcap = n;
  }
  int *cnt = w->rbuf, *ofs = w->rbuf + (w->rcap + 1);
  int *lflag = nullptr, *lpos = nullptr, *longs = nullptr;
  if (virt) lflag = w->lbuf, lpos = lflag + (w->lcap + 1), longs = lpos + (w->lcap + 1);
  size_t tb = 0;
  HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, tb, cnt, ofs, static_cast<int>(n + 1), st));
  if ((rc = ensure_temp(c, w, tb))) return rc;
  w->timed = false;
  w->ms = 0;
  if (virt && !c->lg_perm.empty()) {                // the caller's order is the real CSR's
    if ((rc = up_perm(c, w->stage, kStageBytes, w->qkey, iv_qkey, c->lg_perm))) return rc;
    if (iv_rev)
      if ((rc = up_perm(c, w->stage, kStageBytes, w->rev, iv_rev, c->lg_perm))) return rc;
  } else {
    if ((rc = up(c, w, w->qkey, iv_qkey, static_cast<size_t>(ni) * sizeof(int)))) return rc;
    if (iv_rev)
      if ((rc = up(c, w, w->rev, iv_rev, static_cast<size_t>(ni)))) return rc;
  }
  if (c->profiling) HIP_TRY(c, hipEventRecord(w->ev[0], st));     // the two columns are up: the device work from here
  k_jn_count<<<grid_for(n + 1), kBlock, 0, st>>>(c->rmeta, rlen, cid, n, cnt);
  HIP_TRY(c, hipGetLastError());
  tb = w->temp_bytes;
  HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(w->temp, tb, cnt, ofs, static_cast<int>(n + 1), st));
  int64_t m = 0;
  if ((rc = read_last(c, w, ofs, nullptr, n, &m))) return rc;
  if (m < 0 || m >= ni) return fail(c, FSLR_ERR_STATE, "fslr_cluster_junctions: inconsistent counts (internal)");
  // the clustered reads of more than FSLR_MAX_L intervals: flag, scan, compact
  int64_t n_long = 0;
  if (virt && m > 0) {
    k_chain_long_flag<<<grid_for(n + 1), kChainBlock, 0, st>>>(cid, rlen, n, lflag);
    HIP_TRY(c, hipGetLastError());
    tb = w->temp_bytes;
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(w->temp, tb, lflag, lpos, static_cast<int>(n + 1), st));
    if ((rc = read_last(c, w, lpos, nullptr, n, &n_long))) return rc;
    if (n_long < 0 || n_long > n) return fail(c, FSLR_ERR_STATE, "fslr_cluster_junctions: inconsistent counts (internal)");
    if (n_long > 0) {
      k_chain_long_compact<<<grid_for(n), kChainBlock, 0, st>>>(lflag, lpos, n, n_long, longs);
      HIP_TRY(c, hipGetLastError());
    }
  }
  if (m > 0 && n_loci <= 0)
    return fail(c, FSLR_ERR_STATE, "fslr_cluster_junctions: clustered reads without loci rows (internal)");

  NewRows nr;
  int64_t n_rows = 0;
  if ((rc = dalloc(c, &nr.off, static_cast<size_t>(nc + 1)))) return rc;
  HIP_TRY(c, hipMemsetAsync(nr.off, 0, static_cast<size_t>(nc + 1) * sizeof(long long), st));
  if (m > 0) {
    if (m > w->mcap || !w->mbuf) {
      w->mcap = 0;
      if ((rc = dalloc(c, &w->kbuf, static_cast<size_t>(2 * (m + 1)))) || (rc = dalloc(c, &w->mbuf, static_cast<size_t>(7 * (m + 1)))))
        return rc;
      w->mcap = m;
    }
    const int64_t mc = w->mcap + 1;
    unsigned long long *key_in = w->kbuf, *key_out = w->kbuf + mc;
    int *val_in = w->mbuf, *vo = val_in + mc, *bpa = vo + mc, *bpb = bpa + mc, *rd = bpb + mc, *rid = rd + mc, *hpos = rid + mc;
    int* head = val_in;                              // once the sort has read them
    int *rflag = reinterpret_cast<int*>(key_in), *rsum = rflag + mc;   // the input keys' 8 B per element, likewise
    const int kbits = bits_for(2 * n_loci);          // an end is locus * 2 + side < 2 * n_loci <= 2^31
    const int mi = static_cast<int>(m);
    size_t tb_sort = 0, tb_scan = 0;
    HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(nullptr, tb_sort, key_in, key_out, val_in, vo, mi, 0, 2 * kbits, st));
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, tb_scan, rflag, rsum, mi + 1, st));
    if ((rc = ensure_temp(c, w, std::max(tb_sort, tb_scan)))) return rc;
    const long long n_quads = (n + 3) / 4;
    EmitArgs ea{c->rmeta, rlen, off2, longs, n_long, c->iv, cid, w->qkey, iv_rev ? w->rev : nullptr, ofs, loff, lrows, lrows + lcap, lrows + 2 * lcap,
                n, ni, m, n_loci, nc, n_quads, kbits, key_in, val_in, bpa, bpb, rd};
    k_jn_emit<<<grid_for(n_quads, kWavesPerBlock, 256 * 32), kBlock, 0, st>>>(ea);
    HIP_TRY(c, hipGetLastError());
    if (n_long > 0) {                                // only when such reads exist, one workgroup each
      k_jn_emit_long<<<grid_for(n_long, 1, 256 * 8), kChainBlock, 0, st>>>(ea);
      HIP_TRY(c, hipGetLastError());
    }
    tb = w->temp_bytes;
    HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(w->temp, tb, key_in, key_out, val_in, vo, mi, 0, 2 * kbits, st));
    const int g = grid_for(m + 1);
    k_jn_heads<<<g, kBlock, 0, st>>>(key_out, vo, rd, m, head, rflag);
    HIP_TRY(c, hipGetLastError());
    tb = w->temp_bytes;
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(w->temp, tb, head, rid, mi, st));
    tb = w->temp_bytes;
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(w->temp, tb, rflag, rsum, mi + 1, st));
    if ((rc = read_last(c, w, rid, head, m - 1, &n_rows))) return rc;
    if (n_rows < 1 || n_rows > m) return fail(c, FSLR_ERR_STATE, "fslr_cluster_junctions: inconsistent counts (internal)");
    if ((rc = dalloc(c, &nr.rows, static_cast<size_t>(8 * n_rows))) || (rc = dalloc(c, &nr.sides, static_cast<size_t>(n_rows))))
      return rc;
    k_jn_hpos<<<g, kBlock, 0, st>>>(head, rid, m, n_rows, hpos);
    HIP_TRY(c, hipGetLastError());
    RowArgs ra{key_out, vo, bpa, bpb, hpos, rsum, head, rid, loff, m, n_rows, nc, n_loci, n_rows, kbits,
               nr.rows, nr.sides, nr.off};
    k_jn_rows<<<grid_for(n_rows), kBlock, 0, st>>>(ra);
    HIP_TRY(c, hipGetLastError());
    if (m > n_rows) {
      k_jn_minmax<<<g, kBlock, 0, st>>>(ra);
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
  std::swap(w->off, nr.off);
  std::swap(w->rows, nr.rows);
  std::swap(w->sides, nr.sides);
  w->rows_cap = n_rows;
  w->n_rows = n_rows;
  w->n_clusters = nc;
  w->have = true;
  if (n_rows_out) *n_rows_out = n_rows;
  return FSLR_OK;
}

}  // namespace

extern "C" {

int fslr_cluster_junctions(fslr_ctx* c, const int32_t* iv_qkey, const uint8_t* iv_rev, int64_t n_intervals,
                           int64_t* n_rows_out) {
  return junctions_run(c, iv_qkey, iv_rev, n_intervals, n_rows_out, false);
}

int fslr_cluster_junctions_any(fslr_ctx* c, const int32_t* iv_qkey, const uint8_t* iv_rev, int64_t n_intervals,
                               int64_t* n_rows_out) {
  return junctions_run(c, iv_qkey, iv_rev, n_intervals, n_rows_out, true);
}

int fslr_get_cluster_junctions(fslr_ctx* c, int64_t* off, int32_t* locus_a, int32_t* locus_b, uint8_t* sides,
                               int32_t* n_obs, int32_t* n_reads, int32_t* bp, int64_t capacity) {
  if (!c) return FSLR_ERR_INVALID;
  JunctionWork* w = c->jnw;
  if (!w || !w->have) return fail(c, FSLR_ERR_STATE, "fslr_get_cluster_junctions: fslr_cluster_junctions first");
  if (capacity < w->n_rows)
    return fail(c, FSLR_ERR_INVALID, "fslr_get_cluster_junctions: capacity " + std::to_string(capacity) + " < " +
                                         std::to_string(w->n_rows) + " rows");
  HIP_TRY(c, hipSetDevice(c->device));
  if (off)
    HIP_TRY(c, hipMemcpyAsync(off, w->off, static_cast<size_t>(w->n_clusters + 1) * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
  const size_t col = static_cast<size_t>(w->n_rows) * sizeof(int);
  int32_t* out[4] = {locus_a, locus_b, n_obs, n_reads};
  for (int k = 0; k < 4; ++k)
    if (out[k] && w->n_rows)
      HIP_TRY(c, hipMemcpyAsync(out[k], w->rows + k * w->rows_cap, col, hipMemcpyDeviceToHost, c->stream));
  if (bp && w->n_rows)                              // rows_cap == n_rows: the four columns are one block
    HIP_TRY(c, hipMemcpyAsync(bp, w->rows + 4 * w->rows_cap, 4 * col, hipMemcpyDeviceToHost, c->stream));
  if (sides && w->n_rows)
    HIP_TRY(c, hipMemcpyAsync(sides, w->sides, static_cast<size_t>(w->n_rows), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FSLR_OK;
}

int fslr_cluster_junctions_timings(fslr_ctx* c, float* ms) {
  if (!c || !ms) return FSLR_ERR_INVALID;
  JunctionWork* w = c->jnw;
  if (!w || !w->timed)
    return fail(c, FSLR_ERR_STATE,
                "fslr_cluster_junctions_timings: no profiled fslr_cluster_junctions (fslr_set_profiling 1 or 2)");
  ms[0] = w->ms;
  return FSLR_OK;
}

}  // extern "C"
