// loci.hip — cluster loci: per cluster of the resident table and per chromosome, the merged spans of its
// reads' intervals, with the intervals and the distinct reads behind each span (fslr_hip.h states the
// contract; DESIGN.md §3.10.1 the bytes).
//
// The index's records idx4[q] = {start, end, thr, read << 6 | j} are (chromosome, start)-sorted and the
// table gives cid[read], so the loci are one stable sort and one segmented scan away.  Passes, all on the
// context's stream:
//   k_lc_flag       flag[q] = the read at sorted position q is in a cluster (through lg_vreal on a context with
//                   virtual reads)
//   hipcub scan     pos = exclusive sum of flag; k_lc_total leaves M = the clustered intervals
//   k_lc_compact    (cid, q) of the flagged positions, ascending q
//   hipcub sort     stable radix SortPairs on the cid's ceil(log2 n_clusters) bits: (cid, chrom, start) order
//   k_lc_gather     per sorted element: start, end and the segment key cid << 32 | chrom (chrom: the position's
//                   range in crange, searched in LDS up to 64 chromosomes, in global memory beyond)
//   k_lc_tile<0>    the segmented inclusive max-scan of `end` over the (cid, chrom) segments, tile aggregates:
//                   each thread scans its consecutive elements, a wave combines (head flag, max) by shuffles,
//                   the block's waves through LDS
//   k_lc_carry      one block walks the tile aggregates in order: the running max that enters each tile
//   k_lc_tile<1>    the same tile scan seeded with its carry; writes rmax[p], and head[p] = p opens a locus
//                   (first of its segment, or start > the running max before it)
//   hipcub scan     lid = exclusive sum of head; k_lc_total leaves R = the rows
//   k_lc_heads      hpos[lid] = p of each head
//   k_lc_first      first[p] = no other interval of p's real read lies earlier in p's locus (the read's whole
//                   list is looked at, so the order of the list does not matter)
//   hipcub scan     fsum = exclusive sum of first over M + 1
//   k_lc_rows       one thread per row: start, end = rmax at the locus's last element, n_intervals = head
//                   distance, n_reads = fsum difference, chrom; and off[c] for every cluster whose rows begin here
// No block waits for another (the carry is a pass of its own), every sum and maximum is an integer one and
// every word has one writer, so the bytes are the same on every run.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <string>

#include "ctx.hpp"
#include "fslr_hip.h"
#include "idxsearch.hpp"
#include "kernels.hpp"
#include "wave.hpp"

using namespace fslr;

// the resident rows, the scratch (grown on demand) and the last call's event time
struct LociWork {
  // resident rows
  long long* off = nullptr;          // [n_clusters + 1]
  int* rows = nullptr;               // [5 x rows_cap] chrom, start, end, n_intervals, n_reads
  int64_t rows_cap = 0, off_cap = 0;
  int64_t n_rows = 0, n_clusters = 0;
  bool have = false;
  // scratch per index position: flag, pos
  int* qbuf = nullptr;               // [2 x qcap]
  int64_t qcap = 0;
  // scratch per clustered interval: keys in / out, vals in / out, start, end, rmax (ints), seg (u64)
  int* mbuf = nullptr;               // [7 x (mcap + 1)]
  unsigned long long* seg = nullptr; // [mcap]
  int64_t mcap = 0;
  int2* agg = nullptr;               // [tcap] tile aggregates {has head, max}
  int* carry = nullptr;              // [tcap] the running max entering each tile
  int64_t tcap = 0;
  long long* info = nullptr;         // [2] device; pinned copy below
  long long* host = nullptr;         // [2] pinned
  void* temp = nullptr;
  size_t temp_bytes = 0;
  hipEvent_t ev[2] = {};
  bool ev_ok = false, timed = false;
  float ms = 0;
};

namespace {

constexpr int kBlock = 256;
constexpr int kNoMax = -1;                                  // below every end (coordinates are >= 0)
constexpr int64_t kMaxItems = int64_t(1) << 30;             // hipcub's item count is an int

template <typename T>
void dfree(T*& p) {
  if (p) (void)hipFree(p);
  p = nullptr;
}

}  // namespace

void fslr_loci_drop(fslr_ctx* c) {
  if (c->lcw) c->lcw->have = false;
  fslr_junctions_drop(c);                   // the junctions name loci rows
  fslr_paths_drop(c);                       // and so do the paths' tokens
}

bool fslr_loci_view(const fslr_ctx* c, const long long** off, const int** rows, int64_t* rows_cap, int64_t* n_rows,
                    int64_t* n_clusters) {
  const LociWork* w = c->lcw;
  if (!w || !w->have) return false;
  *off = w->off;
  *rows = w->rows;
  *rows_cap = w->rows_cap;
  *n_rows = w->n_rows;
  *n_clusters = w->n_clusters;
  return true;
}

void fslr_loci_free(fslr_ctx* c) {
  LociWork* w = c->lcw;
  if (!w) return;
  dfree(w->off), dfree(w->rows), dfree(w->qbuf), dfree(w->mbuf), dfree(w->seg), dfree(w->agg), dfree(w->carry);
  dfree(w->info), dfree(w->temp);
  if (w->host) (void)hipHostFree(w->host);
  if (w->ev_ok)
    for (hipEvent_t e : w->ev) (void)hipEventDestroy(e);
  delete w;
  c->lcw = nullptr;
}

namespace {

// ---- flag, compact ------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_lc_flag(const int4* __restrict__ idx4, const int* __restrict__ vreal,
                                                    const int* __restrict__ cid, long long ni, long long nv,
                                                    long long n, int* __restrict__ flag) {
  for (long long q = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; q < ni; q += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(q, ni);
    int r = static_cast<int>(static_cast<unsigned>(idx4[q].w) >> 6);
    FSLR_BOUND(r, nv);
    if (vreal) r = vreal[r];
    FSLR_BOUND(r, n);
    flag[q] = cid[r] >= 0;
  }
}

// the total of an exclusive scan: pos[last] + flag[last]
__global__ void k_lc_total(const int* __restrict__ flag, const int* __restrict__ pos, long long last,
                           long long* __restrict__ out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *out = static_cast<long long>(pos[last]) + flag[last];
}

__global__ __launch_bounds__(kBlock) void k_lc_compact(const int4* __restrict__ idx4, const int* __restrict__ vreal,
                                                       const int* __restrict__ cid, const int* __restrict__ flag,
                                                       const int* __restrict__ pos, long long ni, long long nv,
                                                       long long n, long long m, int* __restrict__ keys,
                                                       int* __restrict__ vals) {
  for (long long q = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; q < ni; q += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(q, ni);
    if (!flag[q]) continue;
    int r = static_cast<int>(static_cast<unsigned>(idx4[q].w) >> 6);
    FSLR_BOUND(r, nv);
    if (vreal) r = vreal[r];
    FSLR_BOUND(r, n);
    const int p = pos[q];
    FSLR_BOUND(p, m);
    keys[p] = cid[r];
    vals[p] = static_cast<int>(q);
  }
}

// ---- gather -------------------------------------------------------------------------------------
// the chromosome whose range [crange[c].x, crange[c].y) holds sorted position q (empty ranges hold none)
__device__ __forceinline__ int chrom_of(const int* __restrict__ beg, int n_chroms, int q) {
  // the last c with beg[c] <= q; ranges are consecutive, so an empty one shares its begin with the next
  // and the last of equal begins is the one that holds q
  int lo = 0, hi = n_chroms - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (beg[mid] <= q)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(kBlock) void k_lc_gather(const int4* __restrict__ idx4, const int2* __restrict__ crange,
                                                      int n_chroms, const int* __restrict__ keys,
                                                      const int* __restrict__ vq, long long ni, long long m,
                                                      int* __restrict__ st, int* __restrict__ en,
                                                      unsigned long long* __restrict__ seg) {
  __shared__ int c_beg[64];
  const bool lds = n_chroms <= 64;
  if (lds) {
    if (threadIdx.x < 64) c_beg[threadIdx.x] = static_cast<int>(threadIdx.x) < n_chroms ? crange[threadIdx.x].x : 0x7FFFFFFF;
    __syncthreads();
  }
  for (long long p = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; p < m; p += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(p, m);
    const int q = vq[p];
    FSLR_BOUND(q, ni);
    const int4 rec = idx4[q];
    int ch;
    if (lds) {
      ch = chrom_of(c_beg, n_chroms, q);
    } else {
      int lo = 0, hi = n_chroms - 1;
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        FSLR_BOUND(mid, n_chroms);
        if (crange[mid].x <= q)
          lo = mid;
        else
          hi = mid - 1;
      }
      ch = lo;
    }
    st[p] = rec.x;
    en[p] = rec.y;
    seg[p] = (static_cast<unsigned long long>(static_cast<unsigned>(keys[p])) << 32) | static_cast<unsigned>(ch);
  }
}

// ---- the segmented running maximum --------------------------------------------------------------
// (f, v): f = a segment head lies in the span, v = the running max since the span's last head (or over the
// whole span).  combine(a, b), a before b:
struct FV {
  int f, v;
};
__device__ __forceinline__ FV combine(FV a, FV b) { return FV{a.f | b.f, b.f ? b.v : max(a.v, b.v)}; }

__device__ __forceinline__ FV wave_incl_fv(FV x, int lane) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const int of = __shfl_up(x.f, d);
    const int ov = __shfl_up(x.v, d);
    if (lane >= d) x = combine(FV{of, ov}, x);
  }
  return x;
}

// One tile = kBlock x kItems consecutive elements; thread t holds elements [t * kItems, (t + 1) * kItems) of it.
// kApply = false: agg[tile] = the tile's (f, v).  kApply = true: the scan seeded with carry[tile]; rmax and head.
template <int kItems, bool kApply>
__global__ __launch_bounds__(kBlock) void k_lc_tile(const unsigned long long* __restrict__ seg, const int* __restrict__ st,
                                                    const int* __restrict__ en, long long m, long long n_tiles,
                                                    int2* __restrict__ agg, const int* __restrict__ carry,
                                                    int* __restrict__ rmax, int* __restrict__ head) {
  __shared__ FV s_wave[kBlock / kWave];
  const int lane = lane_id(), wv = threadIdx.x / kWave;
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long base = tile * static_cast<long long>(kBlock * kItems) + static_cast<long long>(threadIdx.x) * kItems;
    int hf[kItems], e[kItems];
    unsigned long long prev = 0;
    if (base > 0 && base <= m) {
      FSLR_BOUND(base - 1, m);
      prev = seg[base - 1];
    }
#pragma unroll
    for (int i = 0; i < kItems; ++i) {
      const long long p = base + i;
      hf[i] = 0;
      e[i] = kNoMax;
      if (p < m) {
        FSLR_BOUND(p, m);
        const unsigned long long s = seg[p];
        hf[i] = p == 0 || s != prev;
        e[i] = en[p];
        prev = s;
      }
    }
    // the thread's own span
    FV t{0, kNoMax};
#pragma unroll
    for (int i = 0; i < kItems; ++i) t = combine(t, FV{hf[i], e[i]});
    const FV incl = wave_incl_fv(t, lane);
    if (lane == kWave - 1) s_wave[wv] = incl;
    __syncthreads();
    if (!kApply) {
      if (threadIdx.x == 0) {
        FV a = s_wave[0];
#pragma unroll
        for (int k = 1; k < kBlock / kWave; ++k) a = combine(a, s_wave[k]);
        FSLR_BOUND(tile, n_tiles);
        agg[tile] = make_int2(a.f, a.v);
      }
    } else {
      // what lies before this thread: the carry, the earlier waves, the earlier lanes
      FSLR_BOUND(tile, n_tiles);
      FV x{0, carry[tile]};
      for (int k = 0; k < wv; ++k) x = combine(x, s_wave[k]);
      const int of = __shfl_up(incl.f, 1), ov = __shfl_up(incl.v, 1);
      if (lane > 0) x = combine(x, FV{of, ov});
      int run = x.v;                                   // the running max of the segment before element i
#pragma unroll
      for (int i = 0; i < kItems; ++i) {
        const long long p = base + i;
        if (p < m) {
          const int h = hf[i] || st[p] > run;
          run = hf[i] ? e[i] : max(run, e[i]);
          rmax[p] = run;
          head[p] = h;
        }
      }
    }
    __syncthreads();
  }
}

// one block: carry[t] = the running max entering tile t (kNoMax where the segment before it is closed by
// nothing: a tile's own first element decides that, its head flag resets the max)
__global__ __launch_bounds__(kBlock) void k_lc_carry(const int2* __restrict__ agg, long long n_tiles,
                                                     int* __restrict__ carry) {
  __shared__ FV s_wave[kBlock / kWave];
  __shared__ FV s_run;
  const int lane = lane_id(), wv = threadIdx.x / kWave;
  if (threadIdx.x == 0) s_run = FV{0, kNoMax};
  __syncthreads();
  for (long long b = 0; b < n_tiles; b += kBlock) {
    const long long t = b + threadIdx.x;
    FV x{0, kNoMax};
    if (t < n_tiles) {
      FSLR_BOUND(t, n_tiles);
      const int2 a = agg[t];
      x = FV{a.x, a.y};
    }
    const FV incl = wave_incl_fv(x, lane);
    if (lane == kWave - 1) s_wave[wv] = incl;
    __syncthreads();
    FV pre = s_run;
    for (int k = 0; k < wv; ++k) pre = combine(pre, s_wave[k]);
    const int of = __shfl_up(incl.f, 1), ov = __shfl_up(incl.v, 1);
    if (lane > 0) pre = combine(pre, FV{of, ov});
    if (t < n_tiles) carry[t] = pre.v;
    __syncthreads();
    if (threadIdx.x == kBlock - 1) s_run = combine(pre, x);
    __syncthreads();
  }
}

// ---- rows ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_lc_heads(const int* __restrict__ head, const int* __restrict__ lid,
                                                     long long m, long long n_rows, int* __restrict__ hpos) {
  for (long long p = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; p < m; p += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(p, m);
    if (head[p]) {
      FSLR_BOUND(lid[p], n_rows);
      hpos[lid[p]] = static_cast<int>(p);
    }
  }
}

struct ReadLists {
  const int4* rmeta;
  const int4* iv;
  const int *vreal, *vbase, *rlen, *off2;      // null without virtual reads
  long long nv, n, ni;
};

// first[p] = 1 iff no other interval of p's real read lies in p's locus before it, in (start, list index)
// order.  An interval of the same read on the same chromosome lies in the locus iff its start is in
// [locus start, p's start]: the read's intervals all belong to this cluster, and a (cluster, chromosome)
// group's loci are disjoint and ordered by start.
__global__ __launch_bounds__(kBlock) void k_lc_first(const int4* __restrict__ idx4, const int* __restrict__ vq,
                                                     const unsigned long long* __restrict__ seg,
                                                     const int* __restrict__ st, const int* __restrict__ head,
                                                     const int* __restrict__ lid, const int* __restrict__ hpos,
                                                     ReadLists rl, long long m, long long n_rows,
                                                     int* __restrict__ first) {
  for (long long p = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; p <= m; p += gridDim.x * static_cast<long long>(kBlock)) {
    if (p == m) {                                      // the scan runs over m + 1 so that fsum[m] is the total
      first[p] = 0;
      continue;
    }
    FSLR_BOUND(p, m);
    const long long l = static_cast<long long>(lid[p]) + head[p] - 1;
    FSLR_BOUND(l, n_rows);
    const int hp = hpos[l];
    FSLR_BOUND(hp, m);
    const int ls = st[hp], s = st[p];
    const int ch = static_cast<int>(static_cast<unsigned>(seg[p]));
    const int q = vq[p];
    FSLR_BOUND(q, rl.ni);
    const unsigned w = static_cast<unsigned>(idx4[q].w);
    int r = static_cast<int>(w >> 6), j = static_cast<int>(w & 63u);
    FSLR_BOUND(r, rl.nv);
    if (rl.vreal) {
      j += rl.vbase[r];
      r = rl.vreal[r];
    }
    FSLR_BOUND(r, rl.n);
    const int4 rm = rl.rmeta[r];
    const int len = rl.rlen ? rl.rlen[r] : (rm.y & 0xFFFF);
    const int off = rm.x, off2 = (rl.off2 && len > FSLR_MAX_L) ? rl.off2[r] : 0;
    int f = 1;
    // downwards from j first: where the list is start-ordered the nearest same-chromosome interval decides
    for (int t = 1; t < len && f; ++t) {
      const int k = t <= j ? j - t : t;
      const long long at = k < FSLR_MAX_L ? static_cast<long long>(off) + k : static_cast<long long>(off2) + (k - FSLR_MAX_L);
      FSLR_BOUND(at, rl.ni);
      const int4 o = rl.iv[at];
      if (o.x == ch && o.y >= ls && (o.y < s || (o.y == s && k < j))) f = 0;
    }
    first[p] = f;
  }
}

__global__ __launch_bounds__(kBlock) void k_lc_rows(const unsigned long long* __restrict__ seg, const int* __restrict__ st,
                                                    const int* __restrict__ rmax, const int* __restrict__ hpos,
                                                    const int* __restrict__ fsum, long long m, long long n_rows,
                                                    long long n_clusters, long long cap, int* __restrict__ rows,
                                                    long long* __restrict__ off) {
  for (long long l = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; l < n_rows; l += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(l, n_rows);
    const long long p0 = hpos[l], p1 = l + 1 < n_rows ? hpos[l + 1] : m;
    FSLR_BOUND(p0, m);
    FSLR_BOUND(p1 - 1, m);
    const unsigned long long s = seg[p0];
    FSLR_BOUND(4 * cap + l, 5 * cap);
    rows[l] = static_cast<int>(static_cast<unsigned>(s));
    rows[cap + l] = st[p0];
    rows[2 * cap + l] = rmax[p1 - 1];
    rows[3 * cap + l] = static_cast<int>(p1 - p0);
    rows[4 * cap + l] = fsum[p1] - fsum[p0];
    // off[c] = l for every cluster c whose rows begin at l (a cluster without rows begins where the next does)
    const long long c1 = static_cast<long long>(s >> 32);
    long long c0 = 0;
    if (l > 0) {
      FSLR_BOUND(hpos[l - 1], m);
      c0 = static_cast<long long>(seg[hpos[l - 1]] >> 32) + 1;
    }
    for (long long c = c0; c <= c1; ++c) {
      FSLR_BOUND(c, n_clusters + 1);
      off[c] = l;
    }
    if (l == n_rows - 1)
      for (long long c = c1 + 1; c <= n_clusters; ++c) {
        FSLR_BOUND(c, n_clusters + 1);
        off[c] = n_rows;
      }
  }
}

// ---- host side ----------------------------------------------------------------------------------
int bits_for(int64_t n_keys) {                   // bits that hold the keys 0 .. n_keys - 1, at least 1
  int b = 1;
  while ((int64_t(1) << b) < n_keys) ++b;
  return b;
}

int ensure_temp(fslr_ctx* c, LociWork* w, size_t bytes) {
  if (bytes <= w->temp_bytes && w->temp) return FSLR_OK;
  dfree(w->temp);
  w->temp_bytes = 0;
  HIP_TRY(c, hipMalloc(&w->temp, bytes ? bytes : 1));
  w->temp_bytes = bytes ? bytes : 1;
  return FSLR_OK;
}

int read_total(fslr_ctx* c, LociWork* w, const int* flag, const int* pos, int64_t count, int64_t* out) {
  k_lc_total<<<1, 64, 0, c->stream>>>(flag, pos, count - 1, w->info);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(w->host, w->info, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  *out = w->host[0];
  return FSLR_OK;
}

// FSLR_LOCI_TILE: the scan's tile in elements (256, 512, 1024, 2048), read per call
int tile_items() {
  int tile = 2048;
  if (const char* e = std::getenv("FSLR_LOCI_TILE")) tile = std::atoi(e);
  switch (tile) {
    case 256: return 1;
    case 512: return 2;
    case 1024: return 4;
    default: return 8;
  }
}

template <bool kApply>
void launch_tile(int items, int grid, hipStream_t st, const unsigned long long* seg, const int* s, const int* e,
                 long long m, long long n_tiles, int2* agg, const int* carry, int* rmax, int* head) {
  switch (items) {
    case 1: k_lc_tile<1, kApply><<<grid, kBlock, 0, st>>>(seg, s, e, m, n_tiles, agg, carry, rmax, head); break;
    case 2: k_lc_tile<2, kApply><<<grid, kBlock, 0, st>>>(seg, s, e, m, n_tiles, agg, carry, rmax, head); break;
    case 4: k_lc_tile<4, kApply><<<grid, kBlock, 0, st>>>(seg, s, e, m, n_tiles, agg, carry, rmax, head); break;
    default: k_lc_tile<8, kApply><<<grid, kBlock, 0, st>>>(seg, s, e, m, n_tiles, agg, carry, rmax, head); break;
  }
}

// the rows of a result of n_rows (allocated apart from the resident ones: a failure keeps those)
struct NewRows {
  long long* off = nullptr;
  int* rows = nullptr;
  ~NewRows() {
    dfree(off);
    dfree(rows);
  }
};

}  // namespace

extern "C" {

int fslr_cluster_loci(fslr_ctx* c, int64_t* n_rows_out) {
  if (!c) return FSLR_ERR_INVALID;
  if (!c->reads_set || c->n == 0) return fail(c, FSLR_ERR_STATE, "fslr_cluster_loci: no reads set");
  if (int rc = search_state(c, "fslr_cluster_loci")) return rc;
  const int* cid = nullptr;
  int64_t tn = 0, nc = 0;
  if (!fslr_cluster_view(c, &cid, &tn, &nc))
    return fail(c, FSLR_ERR_STATE, "fslr_cluster_loci: no cluster table (fslr_cluster_table first)");
  const int64_t n_real = c->lg_set ? c->lg_n_real : c->n;
  if (tn != n_real)
    return fail(c, FSLR_ERR_STATE, "fslr_cluster_loci: the cluster table holds " + std::to_string(tn) +
                                       " reads, the context " + std::to_string(n_real) +
                                       " (a table from before fslr_append_reads / fslr_remove_reads, or of other "
                                       "reads: fslr_cluster_table again)");
  const int64_t ni = c->ni_idx;
  if (ni <= 0 || ni > kMaxItems)
    return fail(c, FSLR_ERR_STATE, "fslr_cluster_loci: the index holds " + std::to_string(ni) + " intervals (1 .. 2^30)");
  HIP_TRY(c, hipSetDevice(c->device));
  if (!c->lcw) c->lcw = new LociWork();
  LociWork* w = c->lcw;
  int rc;
  hipStream_t st = c->stream;
  if (!w->info) {
    if ((rc = dalloc(c, &w->info, 2))) return rc;
  }
  if (!w->host) HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&w->host), 2 * sizeof(long long), hipHostMallocDefault));
  if (c->profiling && !w->ev_ok) {
    for (hipEvent_t& e : w->ev) HIP_TRY(c, hipEventCreate(&e));
    w->ev_ok = true;
  }
  if (ni > w->qcap || !w->qbuf) {
    w->qcap = 0;
    if ((rc = dalloc(c, &w->qbuf, static_cast<size_t>(2 * ni)))) return rc;
    w->qcap = ni;
  }
  int *flag = w->qbuf, *pos = w->qbuf + w->qcap;
  size_t tb = 0;
  HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, tb, flag, pos, static_cast<int>(ni), st));
  if ((rc = ensure_temp(c, w, tb))) return rc;
  w->timed = false;
  w->ms = 0;
  if (c->profiling) HIP_TRY(c, hipEventRecord(w->ev[0], st));
  const int* vreal = c->lg_set ? c->lg_vreal : nullptr;
  const long long nv = c->n;
  k_lc_flag<<<grid_for(ni), kBlock, 0, st>>>(c->idx4, vreal, cid, ni, nv, n_real, flag);
  HIP_TRY(c, hipGetLastError());
  tb = w->temp_bytes;
  HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(w->temp, tb, flag, pos, static_cast<int>(ni), st));
  int64_t m = 0;
  if ((rc = read_total(c, w, flag, pos, ni, &m))) return rc;
  if (m < 0 || m > ni) return fail(c, FSLR_ERR_STATE, "fslr_cluster_loci: inconsistent counts (internal)");

  NewRows nr;
  int64_t n_rows = 0;
  if ((rc = dalloc(c, &nr.off, static_cast<size_t>(nc + 1)))) return rc;
  HIP_TRY(c, hipMemsetAsync(nr.off, 0, static_cast<size_t>(nc + 1) * sizeof(long long), st));
  if (m > 0) {
    if (m > w->mcap || !w->mbuf) {
      w->mcap = 0;
      if ((rc = dalloc(c, &w->mbuf, static_cast<size_t>(7 * (m + 1)))) || (rc = dalloc(c, &w->seg, static_cast<size_t>(m))))
        return rc;
      w->mcap = m;
    }
    const int64_t mc = w->mcap + 1;
    int *keys_in = w->mbuf, *vals_in = keys_in + mc, *keys_out = vals_in + mc, *vq = keys_out + mc;
    int *s_st = vq + mc, *s_en = s_st + mc, *rmax = s_en + mc;
    int *head = keys_in, *lid = vals_in;             // once the sort has read them
    int *hpos = keys_out;                            // once the gather has read the sorted keys
    const int items = tile_items();
    const int64_t tile = static_cast<int64_t>(kBlock) * items;
    const int64_t n_tiles = (m + tile - 1) / tile;
    if (n_tiles > w->tcap || !w->agg) {
      w->tcap = 0;
      if ((rc = dalloc(c, &w->agg, static_cast<size_t>(n_tiles))) || (rc = dalloc(c, &w->carry, static_cast<size_t>(n_tiles))))
        return rc;
      w->tcap = n_tiles;
    }
    size_t tb_sort = 0, tb_scan = 0;
    const int mi = static_cast<int>(m);
    HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(nullptr, tb_sort, keys_in, keys_out, vals_in, vq, mi, 0, 32, st));
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, tb_scan, head, lid, mi + 1, st));
    if ((rc = ensure_temp(c, w, std::max(tb_sort, tb_scan)))) return rc;
    const int g = grid_for(m);
    k_lc_compact<<<grid_for(ni), kBlock, 0, st>>>(c->idx4, vreal, cid, flag, pos, ni, nv, n_real, m, keys_in, vals_in);
    HIP_TRY(c, hipGetLastError());
    tb = w->temp_bytes;
    HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(w->temp, tb, keys_in, keys_out, vals_in, vq, mi, 0, bits_for(nc), st));
    k_lc_gather<<<g, kBlock, 0, st>>>(c->idx4, c->crange, c->built_n_chroms, keys_out, vq, ni, m, s_st, s_en, w->seg);
    HIP_TRY(c, hipGetLastError());
    const int gt = grid_for(n_tiles, 1, 256 * 16);
    launch_tile<false>(items, gt, st, w->seg, s_st, s_en, m, n_tiles, w->agg, nullptr, nullptr, nullptr);
    k_lc_carry<<<1, kBlock, 0, st>>>(w->agg, n_tiles, w->carry);
    launch_tile<true>(items, gt, st, w->seg, s_st, s_en, m, n_tiles, nullptr, w->carry, rmax, head);
    HIP_TRY(c, hipGetLastError());
    tb = w->temp_bytes;
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(w->temp, tb, head, lid, mi, st));
    if ((rc = read_total(c, w, head, lid, m, &n_rows))) return rc;
    if (n_rows < 1 || n_rows > m) return fail(c, FSLR_ERR_STATE, "fslr_cluster_loci: inconsistent counts (internal)");
    if ((rc = dalloc(c, &nr.rows, static_cast<size_t>(5 * n_rows)))) return rc;
    k_lc_heads<<<g, kBlock, 0, st>>>(head, lid, m, n_rows, hpos);
    HIP_TRY(c, hipGetLastError());
    int* first = s_en;                               // the ends are folded into rmax
    int* fsum = w->qbuf;                             // [2 x qcap] >= m + 1 ints: flag and pos are done
    ReadLists rl{c->rmeta, c->iv, vreal, c->lg_set ? c->lg_vbase : nullptr, c->lg_set ? c->lg_rlen : nullptr,
                 c->lg_set ? c->lg_off2 : nullptr, nv, n_real, c->ni};
    k_lc_first<<<grid_for(m + 1), kBlock, 0, st>>>(c->idx4, vq, w->seg, s_st, head, lid, hpos, rl, m, n_rows, first);
    HIP_TRY(c, hipGetLastError());
    tb = w->temp_bytes;
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(w->temp, tb, first, fsum, mi + 1, st));
    k_lc_rows<<<grid_for(n_rows), kBlock, 0, st>>>(w->seg, s_st, rmax, hpos, fsum, m, n_rows, nc, n_rows, nr.rows, nr.off);
    HIP_TRY(c, hipGetLastError());
  }
  if (c->profiling) HIP_TRY(c, hipEventRecord(w->ev[1], st));
  HIP_TRY(c, hipStreamSynchronize(st));
  if (c->profiling) {
    HIP_TRY(c, hipEventElapsedTime(&w->ms, w->ev[0], w->ev[1]));
    w->timed = true;
  }
  // install
  fslr_junctions_drop(c);                   // junctions of the rows that go
  fslr_paths_drop(c);                       // and paths
  std::swap(w->off, nr.off);
  std::swap(w->rows, nr.rows);
  w->rows_cap = n_rows;
  w->off_cap = nc + 1;
  w->n_rows = n_rows;
  w->n_clusters = nc;
  w->have = true;
  if (n_rows_out) *n_rows_out = n_rows;
  return FSLR_OK;
}

int fslr_get_cluster_loci(fslr_ctx* c, int64_t* off, int32_t* chrom, int32_t* start, int32_t* end, int32_t* n_intervals,
                          int32_t* n_reads, int64_t capacity) {
  if (!c) return FSLR_ERR_INVALID;
  LociWork* w = c->lcw;
  if (!w || !w->have) return fail(c, FSLR_ERR_STATE, "fslr_get_cluster_loci: fslr_cluster_loci first");
  if (capacity < w->n_rows)
    return fail(c, FSLR_ERR_INVALID, "fslr_get_cluster_loci: capacity " + std::to_string(capacity) + " < " +
                                         std::to_string(w->n_rows) + " rows");
  HIP_TRY(c, hipSetDevice(c->device));
  if (off)
    HIP_TRY(c, hipMemcpyAsync(off, w->off, static_cast<size_t>(w->n_clusters + 1) * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
  int32_t* out[5] = {chrom, start, end, n_intervals, n_reads};
  for (int k = 0; k < 5; ++k)
    if (out[k] && w->n_rows)
      HIP_TRY(c, hipMemcpyAsync(out[k], w->rows + k * w->rows_cap, static_cast<size_t>(w->n_rows) * sizeof(int),
                                hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FSLR_OK;
}

int fslr_cluster_loci_timings(fslr_ctx* c, float* ms) {
  if (!c || !ms) return FSLR_ERR_INVALID;
  LociWork* w = c->lcw;
  if (!w || !w->timed)
    return fail(c, FSLR_ERR_STATE, "fslr_cluster_loci_timings: no profiled fslr_cluster_loci (fslr_set_profiling 1 or 2)");
  ms[0] = w->ms;
  return FSLR_OK;
}

}  // extern "C"
