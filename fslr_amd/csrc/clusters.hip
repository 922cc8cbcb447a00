// clusters.hip — the cluster table and the representatives from min-rank labels: the reference's
// get_subgraphs (cluster.py:230-234), assign_clusters (main.py:251-342) and choose_alignment
// (cluster.py:237-254) without the host's bincount / flatnonzero / maximum.at passes.
//
// fslr_cluster_table: labels[r] = the smallest rank of r's component (the union-find's output, or a host
// vector).  Passes, all on the context's stream:
//   k_ct_validate   labels[r] in [0, r] and labels[labels[r]] == labels[r]; the first offender (atomicMin)
//   k_ct_sizes      cnt[root] = the component's reads other than the root: one vector atomic per distinct
//                   label per wave (ballot of the lanes that share the leader's label); roots add nothing
//   k_ct_rootflag   flag[r] = r is a root with cnt >= 1 (a component of >= 2 reads)
//   hipcub scan     pos = exclusive sum of flag: the dense id of a root = its position among such roots in
//                   ascending rank, the reference's networkx order
//   k_ct_roots      csz[pos[root]] = cnt + 1; n_clusters, n_nodes, max_size (wave-reduced, then one atomic)
//   k_ct_ids        cid[r], size[r] per rank, coalesced; node flag
//   hipcub scan     off = exclusive sum of csz over n_clusters + 1; npos = exclusive sum of the node flags
//   k_ct_compact    (cid, rank) of the nodes, ascending rank
//   hipcub sort     stable radix SortPairs on the cid's ceil(log2 n_clusters) bits: members, cluster after
//                   cluster, each ascending in rank (no atomic cursor: their order would vary by run)
// Every sum is an integer sum and every write has one writer or is an integer atomic whose result does
// not depend on the order, so the bytes are the same on every run.
// fslr_assign_clusters: qname-code space; singleton numbering = flag pass, hipcub scan, write.
// fslr_choose_representatives: the mean as an order-preserving u64 key; atomicMax per cluster, atomicMin
// of first_row among the codes at the maximum, then the code whose first_row won.
// Algorithmic bytes.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>

#include "ctx.hpp"
#include "fslr_hip.h"
#include "kernels.hpp"
#include "wave.hpp"

using namespace fslr;

// the resident table, the scratch of the three calls (grown on demand) and their last event times
struct ClusterWork {
  // resident table
  int* cid = nullptr;               // [n] dense cluster id, -1 for a read alone
  int* size = nullptr;              // [n] reads of the rank's component
  long long* off = nullptr;         // [n / 2 + 2] member CSR offsets (n_clusters + 1 used)
  int* members = nullptr;           // [n] ranks, cluster after cluster (n_nodes used)
  int64_t cap = 0;
  int64_t n = 0, n_clusters = 0, n_nodes = 0, max_size = 0;
  bool built = false;
  // table scratch
  int* ibuf = nullptr;              // [7 x icap] labels, cnt, flag, pos, keys in, vals in, keys out
  long long* csz = nullptr;         // [icap / 2 + 2] cluster sizes in cid order
  int64_t icap = 0;
  unsigned long long* info = nullptr;   // [4] n_clusters, n_nodes, max_size, first offender
  void* temp = nullptr;
  size_t temp_bytes = 0;
  // assign / representatives scratch
  long long* lbuf = nullptr;        // [lcap] int64 words
  int64_t lcap = 0;
  unsigned char* host = nullptr;    // [kStageBytes] pinned staging of the chunked copies
  hipEvent_t ev[2] = {};
  bool ev_ok = false;
  bool timed[3] = {false, false, false};
  float ms[3] = {0, 0, 0};          // table, assign, representatives
};

namespace {

constexpr size_t kStageBytes = size_t(16) << 20;          // bounded staging of every host copy
constexpr int64_t kMaxItems = int64_t(1) << 30;           // hipcub's item count is an int; ranks stay below 0x7F7F7F7F
constexpr long long kScoreLimit = 1LL << 53;

template <typename T>
void dfree(T*& p) {
  if (p) (void)hipFree(p);
  p = nullptr;
}

}  // namespace

void fslr_cluster_free(fslr_ctx* c) {
  ClusterWork* w = c->clw;
  if (!w) return;
  dfree(w->cid), dfree(w->size), dfree(w->off), dfree(w->members);
  dfree(w->ibuf), dfree(w->csz), dfree(w->info), dfree(w->temp), dfree(w->lbuf);
  if (w->host) (void)hipHostFree(w->host);
  if (w->ev_ok)
    for (hipEvent_t e : w->ev) (void)hipEventDestroy(e);
  delete w;
  c->clw = nullptr;
}

bool fslr_cluster_view(const fslr_ctx* c, const int** cid, int64_t* n, int64_t* n_clusters) {
  const ClusterWork* w = c->clw;
  if (!w || !w->built) return false;
  *cid = w->cid;
  *n = w->n;
  *n_clusters = w->n_clusters;
  return true;
}

namespace {

// ---- wave helpers -----------------------------------------------------------------------------
// `pend` lanes hold key `k`: calls f(key, lanes sharing it, this lane is the group's first) once per
// distinct key, every lane of the wave taking part (the loop's trip count is wave-uniform)
template <typename K, typename F>
__device__ __forceinline__ void wave_groups(bool pend, K k, F f) {
  unsigned long long todo = __ballot(pend);
  const int lane = lane_id();
  while (todo) {
    const int src = __builtin_amdgcn_readfirstlane(__ffsll(static_cast<long long>(todo)) - 1);
    const K lead = __shfl(k, src);
    const unsigned long long m = __ballot(pend && k == lead);
    f(lead, m, lane == src);
    todo &= ~m;
  }
}

template <bool kMax>
__device__ __forceinline__ unsigned long long wave_reduce_u64(unsigned long long x) {
  for (int d = 32; d; d >>= 1) {
    const unsigned long long y = __shfl_xor(x, d);
    x = kMax ? (y > x ? y : x) : (y < x ? y : x);
  }
  return x;
}

__device__ __forceinline__ long long wave_sum_ll(long long x) {
  for (int d = 32; d; d >>= 1) x += __shfl_xor(x, d);
  return x;
}

// the wave-uniform end of a grid-stride loop whose every trip runs whole waves
__device__ __forceinline__ long long wave_trips_end(long long n) { return (n + kWave - 1) / kWave * kWave; }

// ---- the table --------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ct_validate(const int* __restrict__ lab, long long n,
                                                     unsigned long long* __restrict__ bad) {
  for (long long r = blockIdx.x * 256LL + threadIdx.x; r < n; r += gridDim.x * 256LL) {
    FSLR_BOUND(r, n);
    const int l = lab[r];
    bool ok = l >= 0 && l <= r;
    if (ok) {
      FSLR_BOUND(l, n);
      ok = lab[l] == l;
    }
    if (!ok) atomicMin(bad, static_cast<unsigned long long>(r));
  }
}

__global__ __launch_bounds__(256) void k_ct_sizes(const int* __restrict__ lab, long long n, int* __restrict__ cnt) {
  const long long end = wave_trips_end(n);
  for (long long r = blockIdx.x * 256LL + threadIdx.x; r < end; r += gridDim.x * 256LL) {
    int l = -1;
    if (r < n) {
      FSLR_BOUND(r, n);
      l = lab[r];
    }
    wave_groups(r < n && l != r, l, [&](int lead, unsigned long long m, bool first) {
      if (first) {
        FSLR_BOUND(lead, n);
        atomicAdd(cnt + lead, __popcll(m));
      }
    });
  }
}

__global__ __launch_bounds__(256) void k_ct_rootflag(const int* __restrict__ lab, const int* __restrict__ cnt,
                                                     long long n, int* __restrict__ flag) {
  for (long long r = blockIdx.x * 256LL + threadIdx.x; r < n; r += gridDim.x * 256LL) {
    FSLR_BOUND(r, n);
    flag[r] = lab[r] == r && cnt[r] >= 1;
  }
}

__global__ __launch_bounds__(256) void k_ct_roots(const int* __restrict__ cnt, const int* __restrict__ flag,
                                                  const int* __restrict__ pos, long long n, long long ncap,
                                                  long long* __restrict__ csz, unsigned long long* __restrict__ info) {
  const long long end = wave_trips_end(n);
  for (long long r = blockIdx.x * 256LL + threadIdx.x; r < end; r += gridDim.x * 256LL) {
    long long s = 0;
    if (r < n) {
      FSLR_BOUND(r, n);
      const int p = pos[r], f = flag[r];
      if (f) {
        s = cnt[r] + 1LL;
        FSLR_BOUND(p, ncap);
        csz[p] = s;
      }
      if (r == n - 1) {                       // the scan's total; the slot behind the last cluster has no writer
        FSLR_BOUND(p + f, ncap);
        csz[p + f] = 0;
        info[0] = static_cast<unsigned long long>(p + f);
      }
    }
    const long long sum = wave_sum_ll(s);
    const unsigned long long mx = wave_reduce_u64<true>(static_cast<unsigned long long>(s));
    if (lane_id() == 0 && sum) {
      atomicAdd(info + 1, static_cast<unsigned long long>(sum));
      atomicMax(info + 2, mx);
    }
  }
}

__global__ __launch_bounds__(256) void k_ct_ids(const int* __restrict__ lab, const int* __restrict__ cnt,
                                                const int* __restrict__ pos, long long n, int* __restrict__ cid,
                                                int* __restrict__ size, int* __restrict__ nflag) {
  for (long long r = blockIdx.x * 256LL + threadIdx.x; r < n; r += gridDim.x * 256LL) {
    FSLR_BOUND(r, n);
    const int l = lab[r];
    FSLR_BOUND(l, n);
    const int s = cnt[l] + 1;
    const bool node = s >= 2;
    size[r] = s;
    cid[r] = node ? pos[l] : -1;
    nflag[r] = node;
  }
}

__global__ __launch_bounds__(256) void k_ct_compact(const int* __restrict__ cid, const int* __restrict__ npos,
                                                    long long n, long long n_nodes, int* __restrict__ keys,
                                                    int* __restrict__ vals) {
  for (long long r = blockIdx.x * 256LL + threadIdx.x; r < n; r += gridDim.x * 256LL) {
    FSLR_BOUND(r, n);
    const int k = cid[r];
    if (k >= 0) {
      const int p = npos[r];
      FSLR_BOUND(p, n_nodes);
      keys[p] = k;
      vals[p] = static_cast<int>(r);
    }
  }
}

// ---- assign -----------------------------------------------------------------------------------
// owner[code] = the smallest rank naming it; a code outside [0, n_codes) is an offender at once
__global__ __launch_bounds__(256) void k_as_owner(const long long* __restrict__ cor, long long n, long long n_codes,
                                                  int* __restrict__ owner, unsigned long long* __restrict__ bad) {
  for (long long r = blockIdx.x * 256LL + threadIdx.x; r < n; r += gridDim.x * 256LL) {
    FSLR_BOUND(r, n);
    const long long code = cor ? cor[r] : r;
    if (code < 0 || code >= n_codes) {
      atomicMin(bad, static_cast<unsigned long long>(r));
    } else {
      FSLR_BOUND(code, n_codes);
      atomicMin(owner + code, static_cast<int>(r));
    }
  }
}

// a rank that is not its code's owner names a code a lower rank named; the clustered ranks' codes get
// their cid and size (written only when the call is valid: the host reads nothing otherwise)
__global__ __launch_bounds__(256) void k_as_scatter(const long long* __restrict__ cor, long long n, long long n_codes,
                                                    const int* __restrict__ owner, const int* __restrict__ cid,
                                                    const int* __restrict__ size, long long* __restrict__ q_cid,
                                                    long long* __restrict__ q_size, unsigned long long* __restrict__ bad) {
  for (long long r = blockIdx.x * 256LL + threadIdx.x; r < n; r += gridDim.x * 256LL) {
    FSLR_BOUND(r, n);
    const long long code = cor ? cor[r] : r;
    if (code < 0 || code >= n_codes) continue;
    FSLR_BOUND(code, n_codes);
    if (owner[code] != r) {
      atomicMin(bad, static_cast<unsigned long long>(r));
    } else if (cid[r] >= 0) {
      q_cid[code] = cid[r];
      q_size[code] = size[r];
    }
  }
}

__global__ __launch_bounds__(256) void k_as_flag(const unsigned char* __restrict__ present,
                                                 const long long* __restrict__ q_cid, long long n_codes,
                                                 int* __restrict__ flag) {
  for (long long k = blockIdx.x * 256LL + threadIdx.x; k < n_codes; k += gridDim.x * 256LL) {
    FSLR_BOUND(k, n_codes);
    flag[k] = present[k] && q_cid[k] < 0;
  }
}

__global__ __launch_bounds__(256) void k_as_write(const unsigned char* __restrict__ present, const int* __restrict__ flag,
                                                  const int* __restrict__ spos, long long n_codes, long long n_clusters,
                                                  long long* __restrict__ q_cid, long long* __restrict__ q_size,
                                                  unsigned long long* __restrict__ total) {
  for (long long k = blockIdx.x * 256LL + threadIdx.x; k < n_codes; k += gridDim.x * 256LL) {
    FSLR_BOUND(k, n_codes);
    if (flag[k]) {
      q_cid[k] = n_clusters + spos[k];
      q_size[k] = 1;
    } else if (!present[k]) {
      q_cid[k] = -1;
      q_size[k] = 0;
    }
    if (k == n_codes - 1) *total = static_cast<unsigned long long>(spos[k] + flag[k]);
  }
}

// ---- representatives --------------------------------------------------------------------------
// doubles (no NaN here) -> u64 in the same order; every key is above 0
__device__ __forceinline__ unsigned long long order_key(double x) {
  const unsigned long long b = static_cast<unsigned long long>(__double_as_longlong(x));
  return (b >> 63) ? ~b : b | (1ull << 63);
}
__device__ __forceinline__ unsigned long long row_key(long long v) {
  return static_cast<unsigned long long>(v) ^ (1ull << 63);
}

__global__ __launch_bounds__(256) void k_rp_check(const long long* __restrict__ cl, const long long* __restrict__ sum,
                                                  const long long* __restrict__ cnt, long long n_codes, long long n_out,
                                                  unsigned long long* __restrict__ bad) {
  for (long long k = blockIdx.x * 256LL + threadIdx.x; k < n_codes; k += gridDim.x * 256LL) {
    FSLR_BOUND(k, n_codes);
    const long long s = sum[k];
    if (s >= kScoreLimit || s <= -kScoreLimit || cl[k] >= n_out || cnt[k] < 0)
      atomicMin(bad, static_cast<unsigned long long>(k));
  }
}

// pass 1: the mean, and the largest key of each cluster (one atomic per distinct cluster per wave)
__global__ __launch_bounds__(256) void k_rp_max(const long long* __restrict__ cl, const long long* __restrict__ sum,
                                                const long long* __restrict__ cnt, long long n_codes, long long n_out,
                                                double* __restrict__ avg, unsigned long long* __restrict__ best) {
  const long long end = wave_trips_end(n_codes);
  for (long long k = blockIdx.x * 256LL + threadIdx.x; k < end; k += gridDim.x * 256LL) {
    long long g = -1;
    unsigned long long key = 0;
    if (k < n_codes) {
      FSLR_BOUND(k, n_codes);
      const long long q = cnt[k];
      g = q == 0 ? -1 : cl[k];
      double a = __longlong_as_double(0x7FF8000000000000LL);
      if (g >= 0) {
        a = static_cast<double>(sum[k]) / static_cast<double>(q);
        key = order_key(a);
      }
      avg[k] = a;
    }
    wave_groups(g >= 0, g, [&](long long lead, unsigned long long m, bool first) {
      unsigned long long v = key;
      if (m & (m - 1)) v = wave_reduce_u64<true>(((m >> lane_id()) & 1) ? key : 0ull);
      if (first) {
        FSLR_BOUND(lead, n_out);
        atomicMax(best + lead, v);
      }
    });
  }
}

// pass 2: among the codes at their cluster's maximum, the smallest first_row
__global__ __launch_bounds__(256) void k_rp_row(const long long* __restrict__ cl, const long long* __restrict__ cnt,
                                                const double* __restrict__ avg, const long long* __restrict__ first_row,
                                                long long n_codes, long long n_out,
                                                const unsigned long long* __restrict__ best,
                                                unsigned long long* __restrict__ win_row) {
  const long long end = wave_trips_end(n_codes);
  for (long long k = blockIdx.x * 256LL + threadIdx.x; k < end; k += gridDim.x * 256LL) {
    long long g = -1;
    unsigned long long key = ~0ull;
    if (k < n_codes) {
      FSLR_BOUND(k, n_codes);
      g = cnt[k] == 0 ? -1 : cl[k];
      if (g >= 0) {
        FSLR_BOUND(g, n_out);
        if (order_key(avg[k]) == best[g])
          key = row_key(first_row[k]);
        else
          g = -1;
      }
    }
    wave_groups(g >= 0, g, [&](long long lead, unsigned long long m, bool first) {
      unsigned long long v = key;
      if (m & (m - 1)) v = wave_reduce_u64<false>(((m >> lane_id()) & 1) ? key : ~0ull);
      if (first) {
        FSLR_BOUND(lead, n_out);
        atomicMin(win_row + lead, v);
      }
    });
  }
}

// pass 3: the code whose first_row won (first_row is distinct per code; were it not, the smallest code)
__global__ __launch_bounds__(256) void k_rp_pick(const long long* __restrict__ cl, const long long* __restrict__ cnt,
                                                 const double* __restrict__ avg, const long long* __restrict__ first_row,
                                                 long long n_codes, long long n_out,
                                                 const unsigned long long* __restrict__ best,
                                                 const unsigned long long* __restrict__ win_row,
                                                 unsigned long long* __restrict__ winner) {
  for (long long k = blockIdx.x * 256LL + threadIdx.x; k < n_codes; k += gridDim.x * 256LL) {
    FSLR_BOUND(k, n_codes);
    const long long g = cnt[k] == 0 ? -1 : cl[k];
    if (g < 0) continue;
    FSLR_BOUND(g, n_out);
    if (order_key(avg[k]) == best[g] && row_key(first_row[k]) == win_row[g])
      atomicMin(winner + g, static_cast<unsigned long long>(k));
  }
}

// a cluster without a code keeps the fill (all ones) = -1 as int64: nothing to do beyond the fill

// ---- host side --------------------------------------------------------------------------------
int ensure_common(fslr_ctx* c, ClusterWork* w) {
  if (!w->host) HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&w->host), kStageBytes, hipHostMallocDefault));
  if (!w->info)
    if (int rc = dalloc(c, &w->info, 4)) return rc;
  if (c->profiling && !w->ev_ok) {
    for (hipEvent_t& e : w->ev) HIP_TRY(c, hipEventCreate(&e));
    w->ev_ok = true;
  }
  return FSLR_OK;
}

int ensure_temp(fslr_ctx* c, ClusterWork* w, size_t bytes) {
  if (bytes <= w->temp_bytes && w->temp) return FSLR_OK;
  dfree(w->temp);
  w->temp_bytes = 0;
  HIP_TRY(c, hipMalloc(&w->temp, bytes ? bytes : 1));
  w->temp_bytes = bytes ? bytes : 1;
  return FSLR_OK;
}

int ensure_lbuf(fslr_ctx* c, ClusterWork* w, int64_t words) {
  if (words <= w->lcap && w->lbuf) return FSLR_OK;
  w->lcap = 0;
  if (int rc = dalloc(c, &w->lbuf, static_cast<size_t>(words))) return rc;
  w->lcap = words;
  return FSLR_OK;
}

// host -> device and back through the pinned chunk; each chunk syncs (the chunk is reused)
int up(fslr_ctx* c, ClusterWork* w, void* dst, const void* src, size_t bytes) {
  for (size_t at = 0; at < bytes; at += kStageBytes) {
    const size_t m = std::min(kStageBytes, bytes - at);
    std::memcpy(w->host, static_cast<const unsigned char*>(src) + at, m);
    HIP_TRY(c, hipMemcpyAsync(static_cast<unsigned char*>(dst) + at, w->host, m, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  return FSLR_OK;
}

int down(fslr_ctx* c, ClusterWork* w, void* dst, const void* src, size_t bytes) {
  for (size_t at = 0; at < bytes; at += kStageBytes) {
    const size_t m = std::min(kStageBytes, bytes - at);
    HIP_TRY(c, hipMemcpyAsync(w->host, static_cast<const unsigned char*>(src) + at, m, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    std::memcpy(static_cast<unsigned char*>(dst) + at, w->host, m);
  }
  return FSLR_OK;
}

int read_info(fslr_ctx* c, ClusterWork* w, unsigned long long out[4]) {
  HIP_TRY(c, hipMemcpyAsync(w->host, w->info, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  std::memcpy(out, w->host, 4 * sizeof(unsigned long long));
  return FSLR_OK;
}

int t_begin(fslr_ctx* c, ClusterWork* w, int which) {
  w->timed[which] = false;
  w->ms[which] = 0;
  if (c->profiling) HIP_TRY(c, hipEventRecord(w->ev[0], c->stream));
  return FSLR_OK;
}

int t_end(fslr_ctx* c, ClusterWork* w, int which) {
  if (c->profiling) HIP_TRY(c, hipEventRecord(w->ev[1], c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (c->profiling) {
    HIP_TRY(c, hipEventElapsedTime(&w->ms[which], w->ev[0], w->ev[1]));
    w->timed[which] = true;
  }
  return FSLR_OK;
}

int bits_for(int64_t n_keys) {                   // bits that hold the keys 0 .. n_keys - 1, at least 1
  int b = 1;
  while ((int64_t(1) << b) < n_keys) ++b;
  return b;
}

int grow_scratch(fslr_ctx* c, ClusterWork* w, int64_t n) {
  if (n > w->icap || !w->ibuf) {
    w->icap = 0;
    int rc;
    if ((rc = dalloc(c, &w->ibuf, static_cast<size_t>(7 * n))) || (rc = dalloc(c, &w->csz, static_cast<size_t>(n / 2 + 2))))
      return rc;
    w->icap = n;
  }
  return FSLR_OK;
}

// the passes after validation; the table is not `built` while they run
int build_table(fslr_ctx* c, ClusterWork* w, const int* lab, int64_t n) {
  int rc;
  hipStream_t st = c->stream;
  if (n > w->cap || !w->cid) {
    w->cap = 0;
    const size_t sn = static_cast<size_t>(n);
    if ((rc = dalloc(c, &w->cid, sn)) || (rc = dalloc(c, &w->size, sn)) || (rc = dalloc(c, &w->members, sn)) ||
        (rc = dalloc(c, &w->off, sn / 2 + 2)))
      return rc;
    w->cap = n;
  }
  w->n = n;
  w->n_clusters = w->n_nodes = w->max_size = 0;
  if (n == 0) {
    HIP_TRY(c, hipMemsetAsync(w->off, 0, sizeof(long long), st));
    return FSLR_OK;
  }
  const int64_t ic = w->icap;
  int *cnt = w->ibuf + ic, *flag = w->ibuf + 2 * ic, *pos = w->ibuf + 3 * ic;
  int *keys_in = w->ibuf + 4 * ic, *vals_in = w->ibuf + 5 * ic, *keys_out = w->ibuf + 6 * ic;
  int *nflag = flag, *npos = cnt;                     // reused once the ids are written
  const int ni = static_cast<int>(n);
  const long long ncap = n / 2 + 2;
  size_t tb_scan = 0, tb_scan2 = 0, tb_sort = 0;
  HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, tb_scan, flag, pos, ni, st));
  HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, tb_scan2, w->csz, w->off, static_cast<int>(ncap), st));
  HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(nullptr, tb_sort, keys_in, keys_out, vals_in, w->members, ni, 0, 32, st));
  if ((rc = ensure_temp(c, w, std::max({tb_scan, tb_scan2, tb_sort})))) return rc;
  size_t tb = w->temp_bytes;
  const int g = grid_for(n);
  HIP_TRY(c, hipMemsetAsync(cnt, 0, static_cast<size_t>(n) * sizeof(int), st));
  HIP_TRY(c, hipMemsetAsync(w->info, 0, 3 * sizeof(unsigned long long), st));
  k_ct_sizes<<<g, 256, 0, st>>>(lab, n, cnt);
  k_ct_rootflag<<<g, 256, 0, st>>>(lab, cnt, n, flag);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(w->temp, tb, flag, pos, ni, st));
  k_ct_roots<<<g, 256, 0, st>>>(cnt, flag, pos, n, ncap, w->csz, w->info);
  k_ct_ids<<<g, 256, 0, st>>>(lab, cnt, pos, n, w->cid, w->size, nflag);
  HIP_TRY(c, hipGetLastError());
  unsigned long long info[4];
  if ((rc = read_info(c, w, info))) return rc;
  const int64_t nc = static_cast<int64_t>(info[0]), nn = static_cast<int64_t>(info[1]);
  if (nc < 0 || nc > n / 2 || nn < 2 * nc || nn > n)
    return fail(c, FSLR_ERR_STATE, "fslr_cluster_table: inconsistent counts (internal)");
  tb = w->temp_bytes;
  HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(w->temp, tb, w->csz, w->off, static_cast<int>(nc + 1), st));
  if (nn) {
    tb = w->temp_bytes;
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(w->temp, tb, nflag, npos, ni, st));
    k_ct_compact<<<g, 256, 0, st>>>(w->cid, npos, n, nn, keys_in, vals_in);
    HIP_TRY(c, hipGetLastError());
    tb = w->temp_bytes;
    HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(w->temp, tb, keys_in, keys_out, vals_in, w->members,
                                                  static_cast<int>(nn), 0, bits_for(nc), st));
  }
  w->n_clusters = nc;
  w->n_nodes = nn;
  w->max_size = static_cast<int64_t>(info[2]);
  return FSLR_OK;
}

}  // namespace

extern "C" {

int fslr_cluster_table(fslr_ctx* c, const int32_t* labels, int64_t n, fslr_cluster_info* out) {
  if (!c) return FSLR_ERR_INVALID;
  HIP_TRY(c, hipSetDevice(c->device));
  const bool dev = labels == nullptr;
  if (dev) {
    if (!c->reads_set || c->n == 0 || !c->parent) return fail(c, FSLR_ERR_STATE, "fslr_cluster_table: no reads set");
    if (c->lg_set)
      return fail(c, FSLR_ERR_INVALID, "fslr_cluster_table: the context holds virtual reads (reads of more than "
                                       "FSLR_MAX_L intervals): pass their labels as a host vector");
    int ovf = 0;
    if (c->errw) HIP_TRY(c, hipMemcpyAsync(&ovf, c->errw + kErrOverflow, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (ovf)
      return fail(c, FSLR_ERR_STATE, "fslr_cluster_table: the query behind the labels overflowed its edge or deferred "
                                     "buffer: reserve and rerun it");
    n = c->n;
  } else if (n < 0 || n > kMaxItems) {
    return fail(c, FSLR_ERR_INVALID, "fslr_cluster_table: n must lie in [0, 2^30]");
  }
  if (!c->clw) c->clw = new ClusterWork();
  ClusterWork* w = c->clw;
  int rc;
  if ((rc = ensure_common(c, w)) || (rc = grow_scratch(c, w, n))) return rc;
  if ((rc = t_begin(c, w, 0))) return rc;
  const int* lab = c->parent;
  if (!dev) {
    if (n && (rc = up(c, w, w->ibuf, labels, static_cast<size_t>(n) * sizeof(int)))) return rc;
    lab = w->ibuf;
  }
  if (n) {
    // validated before anything resident is touched: the passes index by label
    HIP_TRY(c, hipMemsetAsync(w->info + 3, 0xFF, sizeof(unsigned long long), c->stream));
    k_ct_validate<<<grid_for(n), 256, 0, c->stream>>>(lab, n, w->info + 3);
    HIP_TRY(c, hipGetLastError());
    unsigned long long info[4];
    if ((rc = read_info(c, w, info))) return rc;
    if (info[3] != ~0ull) {
      if (dev)
        return fail(c, FSLR_ERR_STATE, "fslr_cluster_table: the context's labels are not final at read " +
                                           std::to_string(info[3]) + " (fslr_components / fslr_finalize_labels first)");
      const int64_t r = static_cast<int64_t>(info[3]);
      return fail(c, FSLR_ERR_INVALID, "fslr_cluster_table: labels[" + std::to_string(r) + "] = " +
                                           std::to_string(labels[r]) + ": a label must lie in [0, its rank] and be "
                                           "its own label (min-rank roots)");
    }
  }
  w->built = false;
  fslr_loci_drop(c);                        // the loci belong to the table they were made from
  rc = build_table(c, w, lab, n);
  if (rc != FSLR_OK) {
    (void)hipStreamSynchronize(c->stream);
    return rc;
  }
  if ((rc = t_end(c, w, 0))) return rc;
  w->built = true;
  if (out) {
    out->n_clusters = w->n_clusters;
    out->n_nodes = w->n_nodes;
    out->max_size = w->max_size;
  }
  return FSLR_OK;
}

int fslr_get_cluster_ids(fslr_ctx* c, int32_t* cid, int32_t* size) {
  if (!c) return FSLR_ERR_INVALID;
  ClusterWork* w = c->clw;
  if (!w || !w->built) return fail(c, FSLR_ERR_STATE, "fslr_get_cluster_ids: fslr_cluster_table first");
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t b = static_cast<size_t>(w->n) * sizeof(int);
  int rc;
  if (cid && b && (rc = down(c, w, cid, w->cid, b))) return rc;
  if (size && b && (rc = down(c, w, size, w->size, b))) return rc;
  return FSLR_OK;
}

int fslr_get_cluster_members(fslr_ctx* c, int64_t* off, int32_t* members) {
  if (!c) return FSLR_ERR_INVALID;
  ClusterWork* w = c->clw;
  if (!w || !w->built) return fail(c, FSLR_ERR_STATE, "fslr_get_cluster_members: fslr_cluster_table first");
  HIP_TRY(c, hipSetDevice(c->device));
  int rc;
  if (off && (rc = down(c, w, off, w->off, static_cast<size_t>(w->n_clusters + 1) * sizeof(long long)))) return rc;
  if (members && w->n_nodes && (rc = down(c, w, members, w->members, static_cast<size_t>(w->n_nodes) * sizeof(int))))
    return rc;
  return FSLR_OK;
}

int fslr_assign_clusters(fslr_ctx* c, int64_t n_codes, const int64_t* code_of_rank, const uint8_t* present,
                         int64_t* cluster, int64_t* n_reads, int64_t* n_singletons) {
  if (!c) return FSLR_ERR_INVALID;
  ClusterWork* w = c->clw;
  if (!w || !w->built) return fail(c, FSLR_ERR_STATE, "fslr_assign_clusters: fslr_cluster_table first");
  if (n_codes < 0 || n_codes > kMaxItems) return fail(c, FSLR_ERR_INVALID, "fslr_assign_clusters: n_codes must lie in [0, 2^30]");
  if (n_codes && (!present || !cluster || !n_reads)) return fail(c, FSLR_ERR_INVALID, "fslr_assign_clusters: null array");
  const int64_t n = w->n;
  if (!code_of_rank && n_codes != n)
    return fail(c, FSLR_ERR_INVALID, "fslr_assign_clusters: without code_of_rank n_codes must be the table's read count");
  HIP_TRY(c, hipSetDevice(c->device));
  int rc;
  if ((rc = ensure_common(c, w))) return rc;
  if (n_singletons) *n_singletons = 0;
  w->timed[1] = false;
  w->ms[1] = 0;
  if (n_codes == 0 && n == 0) return FSLR_OK;
  // int64 words: code_of_rank [n] | q_cid [nc] | q_size [nc] | owner, flag, spos (ints) [3 nc / 2 + 2] | present
  const int64_t nc = n_codes;
  const int64_t words = n + 2 * nc + (3 * nc + 1) / 2 + 1 + (nc + 7) / 8 + 1;
  if ((rc = ensure_lbuf(c, w, words))) return rc;
  long long* cor = w->lbuf;
  long long *q_cid = cor + n, *q_size = q_cid + nc;
  int* owner = reinterpret_cast<int*>(q_size + nc);
  int *flag = owner + nc, *spos = flag + nc;
  unsigned char* pres = reinterpret_cast<unsigned char*>(w->lbuf + n + 2 * nc + (3 * nc + 1) / 2 + 1);
  size_t tb = 0;
  HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, tb, flag, spos, static_cast<int>(std::max<int64_t>(nc, 1)), c->stream));
  if ((rc = ensure_temp(c, w, tb))) return rc;
  tb = w->temp_bytes;
  hipStream_t st = c->stream;
  if ((rc = t_begin(c, w, 1))) return rc;
  if (code_of_rank && n && (rc = up(c, w, cor, code_of_rank, static_cast<size_t>(n) * sizeof(long long)))) return rc;
  if (nc && (rc = up(c, w, pres, present, static_cast<size_t>(nc)))) return rc;
  const long long* dcor = code_of_rank ? cor : nullptr;
  HIP_TRY(c, hipMemsetAsync(w->info + 3, 0xFF, sizeof(unsigned long long), st));
  if (nc) {
    HIP_TRY(c, hipMemsetAsync(q_cid, 0xFF, static_cast<size_t>(nc) * sizeof(long long), st));      // -1
    HIP_TRY(c, hipMemsetAsync(q_size, 0, static_cast<size_t>(nc) * sizeof(long long), st));
    HIP_TRY(c, hipMemsetAsync(owner, 0x7F, static_cast<size_t>(nc) * sizeof(int), st));            // above every rank
  }
  if (n) {
    k_as_owner<<<grid_for(n), 256, 0, st>>>(dcor, n, nc, owner, w->info + 3);
    k_as_scatter<<<grid_for(n), 256, 0, st>>>(dcor, n, nc, owner, w->cid, w->size, q_cid, q_size, w->info + 3);
    HIP_TRY(c, hipGetLastError());
  }
  unsigned long long info[4];
  if ((rc = read_info(c, w, info))) return rc;
  if (info[3] != ~0ull) {
    const int64_t r = static_cast<int64_t>(info[3]);
    const long long code = code_of_rank ? code_of_rank[r] : r;
    return fail(c, FSLR_ERR_INVALID, "fslr_assign_clusters: rank " + std::to_string(r) + " names code " +
                                         std::to_string(code) + ": a code must lie in [0, " + std::to_string(nc) +
                                         ") and belong to one rank");
  }
  if (nc) {
    k_as_flag<<<grid_for(nc), 256, 0, st>>>(pres, q_cid, nc, flag);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(w->temp, tb, flag, spos, static_cast<int>(nc), st));
    k_as_write<<<grid_for(nc), 256, 0, st>>>(pres, flag, spos, nc, w->n_clusters, q_cid, q_size, w->info + 3);
    HIP_TRY(c, hipGetLastError());
    if ((rc = down(c, w, cluster, q_cid, static_cast<size_t>(nc) * sizeof(long long)))) return rc;
    if ((rc = down(c, w, n_reads, q_size, static_cast<size_t>(nc) * sizeof(long long)))) return rc;
    if ((rc = read_info(c, w, info))) return rc;
    if (n_singletons) *n_singletons = static_cast<int64_t>(info[3]);
  }
  return t_end(c, w, 1);
}

int fslr_choose_representatives(fslr_ctx* c, int64_t n_codes, const int64_t* cluster, const int64_t* score_sum,
                                const int64_t* score_cnt, const int64_t* first_row, int64_t n_out, double* avg,
                                int64_t* winner_code) {
  if (!c) return FSLR_ERR_INVALID;
  if (n_codes < 0 || n_codes > kMaxItems || n_out < 0 || n_out > kMaxItems)
    return fail(c, FSLR_ERR_INVALID, "fslr_choose_representatives: n_codes and n_out must lie in [0, 2^30]");
  if (n_codes && (!cluster || !score_sum || !score_cnt || !first_row || !avg))
    return fail(c, FSLR_ERR_INVALID, "fslr_choose_representatives: null array");
  if (n_out && !winner_code) return fail(c, FSLR_ERR_INVALID, "fslr_choose_representatives: null array");
  HIP_TRY(c, hipSetDevice(c->device));
  if (!c->clw) c->clw = new ClusterWork();
  ClusterWork* w = c->clw;
  int rc;
  if ((rc = ensure_common(c, w))) return rc;
  w->timed[2] = false;
  w->ms[2] = 0;
  if (n_codes == 0 && n_out == 0) return FSLR_OK;
  // int64 words: cluster, sum, cnt, first_row, avg [n_codes each] | best, win_row, winner [n_out each]
  const int64_t nc = n_codes;
  if ((rc = ensure_lbuf(c, w, 5 * nc + 3 * n_out + 1))) return rc;
  long long *cl = w->lbuf, *sum = cl + nc, *cnt = sum + nc, *fr = cnt + nc;
  double* davg = reinterpret_cast<double*>(fr + nc);
  unsigned long long* best = reinterpret_cast<unsigned long long*>(fr + 2 * nc);
  unsigned long long *win_row = best + n_out, *winner = win_row + n_out;
  hipStream_t st = c->stream;
  if ((rc = t_begin(c, w, 2))) return rc;
  const size_t cb = static_cast<size_t>(nc) * sizeof(long long);
  if (nc && ((rc = up(c, w, cl, cluster, cb)) || (rc = up(c, w, sum, score_sum, cb)) || (rc = up(c, w, cnt, score_cnt, cb)) ||
             (rc = up(c, w, fr, first_row, cb))))
    return rc;
  HIP_TRY(c, hipMemsetAsync(w->info + 3, 0xFF, sizeof(unsigned long long), st));
  if (nc) {
    k_rp_check<<<grid_for(nc), 256, 0, st>>>(cl, sum, cnt, nc, n_out, w->info + 3);
    HIP_TRY(c, hipGetLastError());
  }
  unsigned long long info[4];
  if ((rc = read_info(c, w, info))) return rc;
  if (info[3] != ~0ull) {
    const int64_t k = static_cast<int64_t>(info[3]);
    return fail(c, FSLR_ERR_INVALID, "fslr_choose_representatives: code " + std::to_string(k) + " (cluster " +
                                         std::to_string(cluster[k]) + ", score_sum " + std::to_string(score_sum[k]) +
                                         ", score_cnt " + std::to_string(score_cnt[k]) + "): |score_sum| must be below "
                                         "2^53, cluster below n_out = " + std::to_string(n_out) +
                                         " and score_cnt at or above 0");
  }
  if (n_out) {
    HIP_TRY(c, hipMemsetAsync(best, 0, static_cast<size_t>(n_out) * sizeof(long long), st));
    HIP_TRY(c, hipMemsetAsync(win_row, 0xFF, 2 * static_cast<size_t>(n_out) * sizeof(long long), st));   // + winner
  }
  if (nc) {
    const int g = grid_for(nc);
    k_rp_max<<<g, 256, 0, st>>>(cl, sum, cnt, nc, n_out, davg, best);
    k_rp_row<<<g, 256, 0, st>>>(cl, cnt, davg, fr, nc, n_out, best, win_row);
    k_rp_pick<<<g, 256, 0, st>>>(cl, cnt, davg, fr, nc, n_out, best, win_row, winner);
    HIP_TRY(c, hipGetLastError());
    if ((rc = down(c, w, avg, davg, cb))) return rc;
  }
  if (n_out && (rc = down(c, w, winner_code, winner, static_cast<size_t>(n_out) * sizeof(long long)))) return rc;
  return t_end(c, w, 2);
}

int fslr_cluster_timings(fslr_ctx* c, float* ms) {
  if (!c || !ms) return FSLR_ERR_INVALID;
  ClusterWork* w = c->clw;
  if (!w || !(w->timed[0] || w->timed[1] || w->timed[2]))
    return fail(c, FSLR_ERR_STATE, "fslr_cluster_timings: no profiled fslr_cluster_table, fslr_assign_clusters or "
                                   "fslr_choose_representatives (fslr_set_profiling 1 or 2)");
  for (int t = 0; t < 3; ++t) ms[t] = w->timed[t] ? w->ms[t] : 0.f;
  return FSLR_OK;
}

}  // extern "C"
