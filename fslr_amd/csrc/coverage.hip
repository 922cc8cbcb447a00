// coverage.hip — read depth at query points: the reference's calc_coverage / filter_high_coverage
// (cluster.py:52-77) without the dense per-chromosome arrays.
//
// The reference adds +1 at rstart and -1 at rend of every bed row and takes the running sum, so for a
// chromosome c and a position p
//   cov[c][p] = #{rows of c with rstart <= p} - #{rows of c with rend <= p}.
// With keys chrom << 32 | pos over all chromosomes, the rows of lower chromosomes add the same count to
// both terms and cancel: depth = upper_bound(start keys, c << 32 | p) - upper_bound(end keys, same).
//
// Build (fslr_coverage_build): the rows go up in bounded chunks, k_cov_pack makes the two key arrays,
// hipcub sorts each keys-only over 32 + bits(n_chroms) bits, k_cov_pivots keeps the last key of every
// full kCovTile-key tile of each array.  Both sorted arrays and both pivot arrays stay resident.
// Query (fslr_coverage_at, k_cov_at): one query per lane.  Binary lifting over the pivots (the number
// of tiles that lie entirely at or below the query), then binary lifting inside the one tile that is
// left: log2(n / kCovTile) + 8 probes per array.  The two arrays have the same length, so both searches
// run in one loop with a trip count that depends on n alone: two independent loads in flight per step,
// no lane walks a tile or a run of equal keys, and a pile of equal keys costs what any input costs.
// FSLR_COV_PLAIN=1 (the timing tool's comparison, read per call) lifts over the whole arrays instead.
// No LDS, no atomics: every output word is a function of the input alone.
// Algorithmic bytes: build 12 B per row in, 16 B per row of keys written and sorted;
// query 8 B in, 4 B out and 2 x probes x 8 B of keys read per query.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>

#include "ctx.hpp"
#include "fslr_hip.h"
#include "kernels.hpp"

using namespace fslr;

// the resident coverage set, the chunk staging (bounded) and the last calls' event times
struct CoverageWork {
  unsigned long long* ks = nullptr;  // [n] sorted chrom << 32 | rstart
  unsigned long long* ke = nullptr;  // [n] sorted chrom << 32 | rend
  unsigned long long* ps = nullptr;  // [n / kCovTile] ks[t * kCovTile + kCovTile - 1]
  unsigned long long* pe = nullptr;  // the same of ke
  int64_t n = 0;
  int n_chroms = 0;
  bool built = false;
  uint64_t gen = 0;                  // bumped by every build that replaced the set
  int* stage = nullptr;              // [3 x kCovChunk] a chunk's columns (query: chrom, pos, depth)
  int* host = nullptr;               // [3 x kCovChunk] pinned: the same
  hipEvent_t ev[3] = {};
  bool ev_ok = false, timed_build = false, timed_query = false;
  float ms[4] = {0, 0, 0, 0};        // build upload, build sort, query upload + kernel, query download
};

namespace {

constexpr int kCovTile = FSLR_COVERAGE_TILE;
constexpr int64_t kCovChunk = FSLR_COVERAGE_CHUNK;      // rows or queries per launch: 24 MiB of staging
constexpr int64_t kCovMaxRows = (int64_t(1) << 31) - 1;  // hipcub's item count is an int
constexpr int kCovMaxChroms = 1 << 24;

void free_set(unsigned long long* const (&bufs)[4]) {
  for (unsigned long long* b : bufs)
    if (b) (void)hipFree(b);
}

}  // namespace

void fslr_coverage_free(fslr_ctx* c) {
  CoverageWork* w = c->cvw;
  if (!w) return;
  free_set({w->ks, w->ke, w->ps, w->pe});
  if (w->stage) (void)hipFree(w->stage);
  if (w->host) (void)hipHostFree(w->host);
  if (w->ev_ok)
    for (hipEvent_t e : w->ev) (void)hipEventDestroy(e);
  delete w;
  c->cvw = nullptr;
}

namespace {

// a chunk of rows -> their keys at [at, at + m) of the unsorted arrays
__global__ __launch_bounds__(256) void k_cov_pack(const int* __restrict__ chrom, const int* __restrict__ rstart,
                                                  const int* __restrict__ rend, int m, unsigned long long* __restrict__ ks,
                                                  unsigned long long* __restrict__ ke, long long at, long long n) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) {
    FSLR_BOUND(at + i, n);
    const unsigned long long hi = static_cast<unsigned long long>(static_cast<unsigned>(chrom[i])) << 32;
    ks[at + i] = hi | static_cast<unsigned>(rstart[i]);
    ke[at + i] = hi | static_cast<unsigned>(rend[i]);
  }
}

// the last key of every full tile, of both arrays
__global__ __launch_bounds__(256) void k_cov_pivots(const unsigned long long* __restrict__ ks,
                                                    const unsigned long long* __restrict__ ke, unsigned n, unsigned nt,
                                                    unsigned long long* __restrict__ ps, unsigned long long* __restrict__ pe) {
  for (unsigned t = blockIdx.x * blockDim.x + threadIdx.x; t < nt; t += gridDim.x * blockDim.x) {
    const unsigned long long k = static_cast<unsigned long long>(t) * kCovTile + (kCovTile - 1);
    FSLR_BOUND(k, n);
    ps[t] = ks[k];
    pe[t] = ke[k];
  }
}

struct CovArgs {
  const unsigned long long *ks, *ke, *ps, *pe;
  const int* chrom;
  const int* pos;
  int* depth;
  unsigned n, nt;            // keys per array, full tiles
  unsigned top_n, top_t;     // the largest power of two <= n (<= nt), 0 for 0
  int nq;
};

// Binary lifting, both arrays in step: the largest cs (ce) in [0, len_s] ([0, len_e]) whose keys
// a[base_s .. base_s + cs) (b[base_e .. base_e + ce)) are all <= q.  `top` is uniform and at least the
// largest power of two <= max(len_s, len_e); size = the arrays' length (the bounds build's check).
__device__ __forceinline__ void lift2(const unsigned long long* __restrict__ a, const unsigned long long* __restrict__ b,
                                      unsigned base_s, unsigned base_e, unsigned len_s, unsigned len_e, unsigned top,
                                      unsigned size, unsigned long long q, unsigned& cs, unsigned& ce) {
  cs = ce = 0;
  for (unsigned step = top; step; step >>= 1) {
    const unsigned ts = cs + step, te = ce + step;     // (< 2^32: counts and steps stay below 2^31)
    const bool ins = ts <= len_s, ine = te <= len_e;
    unsigned long long vs = ~0ull, ve = ~0ull;
    if (ins) {
      FSLR_BOUND(base_s + ts - 1, size);
      vs = a[base_s + ts - 1];
    }
    if (ine) {
      FSLR_BOUND(base_e + te - 1, size);
      ve = b[base_e + te - 1];
    }
    if (ins && vs <= q) cs = ts;
    if (ine && ve <= q) ce = te;
  }
}

template <bool kPlain>
__global__ __launch_bounds__(256) void k_cov_at(CovArgs s) {
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < s.nq; k += gridDim.x * blockDim.x) {
    FSLR_BOUND(k, s.nq);
    const unsigned long long q =
        static_cast<unsigned long long>(static_cast<unsigned>(s.chrom[k])) << 32 | static_cast<unsigned>(s.pos[k]);
    unsigned us, ue;
    if constexpr (kPlain) {
      lift2(s.ks, s.ke, 0, 0, s.n, s.n, s.top_n, s.n, q, us, ue);
    } else {
      // tiles whose last key is <= q lie entirely at or below the query
      unsigned t_s, t_e;
      lift2(s.ps, s.pe, 0, 0, s.nt, s.nt, s.top_t, s.nt, q, t_s, t_e);
      // the tile left: its last key is above q (kCovTile - 1 candidates), or it is the tail
      const unsigned b_s = t_s * kCovTile, b_e = t_e * kCovTile;
      const unsigned l_s = t_s < s.nt ? kCovTile - 1 : s.n - b_s;
      const unsigned l_e = t_e < s.nt ? kCovTile - 1 : s.n - b_e;
      lift2(s.ks, s.ke, b_s, b_e, l_s, l_e, kCovTile >> 1, s.n, q, us, ue);
      us += b_s;
      ue += b_e;
    }
    s.depth[k] = static_cast<int>(us) - static_cast<int>(ue);
  }
}

unsigned top_pow2(unsigned v) {
  unsigned t = 0;
  for (unsigned b = 1; b && b <= v; b <<= 1) t = b;
  return t;
}

int key_bits(int n_chroms) {
  int b = 1;
  while ((int64_t(1) << b) <= n_chroms) ++b;
  return 32 + b;
}

// the first row (query) the call refuses, -1 for none
int64_t first_bad(int64_t n, int32_t n_chroms, const int32_t* chrom, const int32_t* a, const int32_t* b) {
  for (int64_t k = 0; k < n; ++k)
    if (chrom[k] < 0 || chrom[k] >= n_chroms || a[k] < 0 || (b && b[k] < 0)) return k;
  return -1;
}

int ensure_stage(fslr_ctx* c, CoverageWork* w) {
  if (!w->stage)
    if (int rc = dalloc(c, &w->stage, static_cast<size_t>(3 * kCovChunk))) return rc;
  if (!w->host)
    HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&w->host), static_cast<size_t>(3 * kCovChunk) * sizeof(int),
                             hipHostMallocDefault));
  if (c->profiling && !w->ev_ok) {
    for (hipEvent_t& e : w->ev) HIP_TRY(c, hipEventCreate(&e));
    w->ev_ok = true;
  }
  return FSLR_OK;
}

// uploads, packs, sorts; the new set's buffers are the caller's to install or free
int build_set(fslr_ctx* c, CoverageWork* w, int64_t n, int32_t n_chroms, const int32_t* chrom, const int32_t* rstart,
              const int32_t* rend, unsigned long long* (&set)[4], unsigned long long* (&raw)[2], void** temp) {
  int rc;
  const bool prof = c->profiling;
  hipStream_t st = c->stream;
  const size_t nk = static_cast<size_t>(n);
  const unsigned nt = static_cast<unsigned>(n / kCovTile);
  for (int k = 0; k < 2; ++k)
    if ((rc = dalloc(c, &set[k], nk)) || (rc = dalloc(c, &raw[k], nk)) || (rc = dalloc(c, &set[2 + k], nt))) return rc;
  if (n == 0) return FSLR_OK;
  const int ni = static_cast<int>(n), bits = key_bits(n_chroms);
  size_t tb = 0;
  HIP_TRY(c, hipcub::DeviceRadixSort::SortKeys(nullptr, tb, raw[0], set[0], ni, 0, bits, st));
  HIP_TRY(c, hipMalloc(temp, tb ? tb : 1));
  float up = 0;
  for (int64_t k0 = 0; k0 < n; k0 += kCovChunk) {
    const int64_t m = std::min<int64_t>(kCovChunk, n - k0);
    const size_t mb = static_cast<size_t>(m) * sizeof(int);
    const int32_t* cols[3] = {chrom + k0, rstart + k0, rend + k0};
    for (int j = 0; j < 3; ++j) std::memcpy(w->host + j * kCovChunk, cols[j], mb);
    if (prof) HIP_TRY(c, hipEventRecord(w->ev[0], st));
    for (int j = 0; j < 3; ++j)
      HIP_TRY(c, hipMemcpyAsync(w->stage + j * kCovChunk, w->host + j * kCovChunk, mb, hipMemcpyHostToDevice, st));
    k_cov_pack<<<grid_for(m), 256, 0, st>>>(w->stage, w->stage + kCovChunk, w->stage + 2 * kCovChunk,
                                            static_cast<int>(m), raw[0], raw[1], k0, n);
    HIP_TRY(c, hipGetLastError());
    if (prof) HIP_TRY(c, hipEventRecord(w->ev[1], st));
    HIP_TRY(c, hipStreamSynchronize(st));              // the pinned chunk is free again
    if (prof) {
      float ms = 0;
      HIP_TRY(c, hipEventElapsedTime(&ms, w->ev[0], w->ev[1]));
      up += ms;
    }
  }
  if (prof) HIP_TRY(c, hipEventRecord(w->ev[0], st));
  for (int k = 0; k < 2; ++k) HIP_TRY(c, hipcub::DeviceRadixSort::SortKeys(*temp, tb, raw[k], set[k], ni, 0, bits, st));
  if (nt) {
    k_cov_pivots<<<grid_for(nt), 256, 0, st>>>(set[0], set[1], static_cast<unsigned>(n), nt, set[2], set[3]);
    HIP_TRY(c, hipGetLastError());
  }
  if (prof) HIP_TRY(c, hipEventRecord(w->ev[1], st));
  HIP_TRY(c, hipStreamSynchronize(st));
  if (prof) {
    w->ms[0] = up;
    HIP_TRY(c, hipEventElapsedTime(&w->ms[1], w->ev[0], w->ev[1]));
  }
  return FSLR_OK;
}

}  // namespace

extern "C" {

int fslr_coverage_build(fslr_ctx* c, int64_t n_rows, int32_t n_chroms, const int32_t* chrom, const int32_t* rstart,
                        const int32_t* rend) {
  if (!c) return FSLR_ERR_INVALID;
  if (n_rows < 0 || n_rows > kCovMaxRows)
    return fail(c, FSLR_ERR_INVALID, "fslr_coverage_build: the row count must lie in [0, 2^31)");
  if (n_chroms < 0 || n_chroms > kCovMaxChroms)
    return fail(c, FSLR_ERR_INVALID, "fslr_coverage_build: n_chroms must lie in [0, 2^24]");
  if (n_rows && (!chrom || !rstart || !rend)) return fail(c, FSLR_ERR_INVALID, "fslr_coverage_build: null array");
  const int64_t bad = first_bad(n_rows, n_chroms, chrom, rstart, rend);
  if (bad >= 0)
    return fail(c, FSLR_ERR_INVALID, "fslr_coverage_build: row " + std::to_string(bad) + " (chrom " +
                                         std::to_string(chrom[bad]) + ", rstart " + std::to_string(rstart[bad]) + ", rend " +
                                         std::to_string(rend[bad]) + "): the chromosome id must lie in [0, " +
                                         std::to_string(n_chroms) + ") and the positions at or above 0");
  HIP_TRY(c, hipSetDevice(c->device));
  if (!c->cvw) c->cvw = new CoverageWork();
  CoverageWork* w = c->cvw;
  w->timed_build = false;
  if (int rc = ensure_stage(c, w)) return rc;
  // the new set is made beside the resident one, which answers until the new one is whole
  unsigned long long* set[4] = {nullptr, nullptr, nullptr, nullptr};
  unsigned long long* raw[2] = {nullptr, nullptr};
  void* temp = nullptr;
  const int rc = build_set(c, w, n_rows, n_chroms, chrom, rstart, rend, set, raw, &temp);
  if (rc != FSLR_OK) (void)hipStreamSynchronize(c->stream);
  for (unsigned long long* b : raw)
    if (b) (void)hipFree(b);
  if (temp) (void)hipFree(temp);
  if (rc != FSLR_OK) {
    free_set({set[0], set[1], set[2], set[3]});
    return rc;
  }
  free_set({w->ks, w->ke, w->ps, w->pe});
  w->ks = set[0], w->ke = set[1], w->ps = set[2], w->pe = set[3];
  w->n = n_rows;
  w->n_chroms = n_chroms;
  w->built = true;
  ++w->gen;
  w->timed_build = c->profiling && n_rows > 0;
  if (!w->timed_build) w->ms[0] = w->ms[1] = 0;
  return FSLR_OK;
}

int fslr_coverage_at(fslr_ctx* c, int64_t n_queries, const int32_t* chrom, const int32_t* pos, int32_t* depth) {
  if (!c) return FSLR_ERR_INVALID;
  if (n_queries < 0) return fail(c, FSLR_ERR_INVALID, "fslr_coverage_at: negative query count");
  if (n_queries && (!chrom || !pos || !depth)) return fail(c, FSLR_ERR_INVALID, "fslr_coverage_at: null array");
  CoverageWork* w = c->cvw;
  if (!w || !w->built) return fail(c, FSLR_ERR_STATE, "fslr_coverage_at: fslr_coverage_build first");
  const int64_t bad = first_bad(n_queries, w->n_chroms, chrom, pos, nullptr);
  if (bad >= 0)
    return fail(c, FSLR_ERR_INVALID, "fslr_coverage_at: query " + std::to_string(bad) + " (chrom " +
                                         std::to_string(chrom[bad]) + ", pos " + std::to_string(pos[bad]) +
                                         "): the chromosome id must lie in [0, " + std::to_string(w->n_chroms) +
                                         ") and the position at or above 0");
  w->timed_query = false;
  w->ms[2] = w->ms[3] = 0;
  if (n_queries == 0) return FSLR_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  if (int rc = ensure_stage(c, w)) return rc;
  const bool prof = c->profiling;
  hipStream_t st = c->stream;
  const char* plain = std::getenv("FSLR_COV_PLAIN");         // the timing tool's comparison only
  const bool use_plain = plain && plain[0] == '1';
  const unsigned n = static_cast<unsigned>(w->n), nt = n / kCovTile;
  CovArgs s{w->ks, w->ke, w->ps, w->pe, w->stage, w->stage + kCovChunk, w->stage + 2 * kCovChunk,
            n,     nt,    top_pow2(n), top_pow2(nt), 0};
  for (int64_t k0 = 0; k0 < n_queries; k0 += kCovChunk) {
    const int64_t m = std::min<int64_t>(kCovChunk, n_queries - k0);
    const size_t mb = static_cast<size_t>(m) * sizeof(int);
    std::memcpy(w->host, chrom + k0, mb);
    std::memcpy(w->host + kCovChunk, pos + k0, mb);
    if (prof) HIP_TRY(c, hipEventRecord(w->ev[0], st));
    HIP_TRY(c, hipMemcpyAsync(w->stage, w->host, mb, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(w->stage + kCovChunk, w->host + kCovChunk, mb, hipMemcpyHostToDevice, st));
    s.nq = static_cast<int>(m);
    if (use_plain)
      k_cov_at<true><<<grid_for(m, 256, 256 * 32), 256, 0, st>>>(s);
    else
      k_cov_at<false><<<grid_for(m, 256, 256 * 32), 256, 0, st>>>(s);
    HIP_TRY(c, hipGetLastError());
    if (prof) HIP_TRY(c, hipEventRecord(w->ev[1], st));
    HIP_TRY(c, hipMemcpyAsync(w->host + 2 * kCovChunk, w->stage + 2 * kCovChunk, mb, hipMemcpyDeviceToHost, st));
    if (prof) HIP_TRY(c, hipEventRecord(w->ev[2], st));
    HIP_TRY(c, hipStreamSynchronize(st));
    std::memcpy(depth + k0, w->host + 2 * kCovChunk, mb);
    if (prof)
      for (int t = 0; t < 2; ++t) {
        float ms = 0;
        HIP_TRY(c, hipEventElapsedTime(&ms, w->ev[t], w->ev[t + 1]));
        w->ms[2 + t] += ms;
      }
  }
  w->timed_query = prof;
  return FSLR_OK;
}

int fslr_coverage_timings(fslr_ctx* c, float* ms) {
  if (!c || !ms) return FSLR_ERR_INVALID;
  CoverageWork* w = c->cvw;
  if (!w || !(w->timed_build || w->timed_query))
    return fail(c, FSLR_ERR_STATE, "fslr_coverage_timings: no profiled fslr_coverage_build or fslr_coverage_at "
                                   "(fslr_set_profiling 1 or 2)");
  for (int t = 0; t < 4; ++t) ms[t] = w->ms[t];
  return FSLR_OK;
}

}  // extern "C"
