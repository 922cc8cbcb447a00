// segments.hip — path segments: per slot of every cluster path the minimum, lower median and maximum of the
// reference start and end of the intervals that land in it, and per link between two slots the same of the
// query-space gap (fslr_hip.h states the contract; DESIGN.md §3.10.5 the bytes; tests/segments_ref.py the plain
// statement).
//
// The path rows are resident (paths.hip): tok_off, n_reads, path_of_read, flipped.  The caller brings the query
// key and, for the gaps, the query end per CSR interval.  Passes, all on the context's stream:
//   k_seg_keys      key[r] = path_of_read[r] + 1 (0: not clustered), val[r] = r
//   hipcub sort     stable radix SortPairs of (key, read): the reads of a row adjacent, in ascending rank
//   k_seg_rowprep   per row: n_reads and, for a row of k >= 2 reads, len * k (64-bit), one more word of zeros
//   hipcub scans    rfirst = exclusive sum of n_reads, base = exclusive 64-bit sum of len * k (base[n_rows] = V,
//                   the bucket words per stream)
//   k_seg_ord       ord[read] = its place minus the unclustered reads minus rfirst[row]
//   k_seg_emit      one lane per interval, lane groups of 16 / 32 / 64 by read length: the rank in the chain by
//                   shuffles, the next piece's key through LDS by rank; the value of (row, position p, ordinal o)
//                   goes to base[row] + p * k + o of its stream; a row of one read writes min = med = max to
//                   the output; the read of ordinal 0 writes k, the bucket's first word and "last slot" per slot
//   fslr_cluster_path_segments_any on virtual reads: k_chain_long_flag on path_of_read, a hipcub scan and
//                   k_chain_long_compact list the clustered reads of more than FSLR_MAX_L intervals (their count
//                   comes back with the bucket words'), and when there are any
//   k_seg_emit_long one workgroup per such read: chain.hpp's bitonic sort of the chain words in LDS, the thread at
//                   rank t takes its interval from the word's low bits and the next piece's key from word t + 1,
//                   and writes what k_seg_emit's lane writes.  A row's reads share its length, so one of the two
//                   kernels serves a row wholly
//   k_seg_flags     per slot: which tier its k falls in
//   hipcub select   the slots of each tier, ascending (three Flagged selections of a counting iterator)
//   k_seg_small     2 <= k <= S: a lane group of 16 / 32 / 64 per (slot, stream); each lane counts the smaller and
//                   the smaller-or-equal values by shuffles
//   k_seg_lds       S < k <= T: one workgroup per (slot, stream), chain.hpp's bitonic sort in LDS
//   k_seg_select    k > T: one workgroup per (slot, stream), block min / max and an exact radix select, four
//                   rounds of eight bits with integer LDS counters
// The chain walk behind k_seg_emit / k_seg_emit_long and the three tier kernels live in segshared.hpp, shared with
// collapsed.hip; EmitArgs below says what the walk writes per piece here.
// No block waits for another.  Every bucket word has one writer; a gap word of the output is zeroed and then
// written at most once; the LDS counters take integer additions whose sum does not depend on the order.  The
// bytes are the same on every run.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>

#include "chain.hpp"
#include "ctx.hpp"
#include "fslr_hip.h"
#include "idxsearch.hpp"
#include "kernels.hpp"
#include "segshared.hpp"
#include "wave.hpp"

using namespace fslr;

// the resident rows, the scratch (grown on demand) and the last call's event time
struct SegmentWork {
  // resident rows
  int* out = nullptr;                // [9 x n_tokens] start min, med, max; end min, med, max; gap min, med, max
  int64_t n_tokens = 0;
  bool have = false;
  // the caller's columns, CSR interval order
  int* qkey = nullptr;               // [icap]
  int* qend = nullptr;               // [icap]
  int64_t icap = 0;
  // per read: sort keys in / out, reads in / out, ord
  unsigned* rbuf = nullptr;          // [5 x rcap]
  int64_t rcap = 0;
  // fslr_cluster_path_segments_any on virtual reads: flag, pos and the list of the clustered reads of more than
  // FSLR_MAX_L intervals
  int* lbuf = nullptr;               // [3 x (lcap + 1)]
  int64_t lcap = 0;
  // per row: n_reads and their scan; len * k and their scan
  int* wbuf = nullptr;               // [2 x (wcap + 1)]
  long long* wbuf64 = nullptr;       // [2 x (wcap + 1)]
  int64_t wcap = 0;
  // per slot: k, the tier lists (3), then the bucket's first word, then last-slot and the tier flags (3)
  int* tbuf = nullptr;               // [4 x tcap]
  long long* tbuf64 = nullptr;       // [tcap]
  unsigned char* tbuf8 = nullptr;    // [4 x tcap]
  int64_t tcap = 0;
  // the buckets: start, end, gap
  int* vbuf = nullptr;               // [3 x vcap]
  int64_t vcap = 0;
  int* cnt = nullptr;                // [4] device: the tier counts
  long long* host = nullptr;         // [4] pinned: the counts read back
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

void fslr_segments_drop(fslr_ctx* c) {
  if (c->sgw) c->sgw->have = false;
}

void fslr_segments_free(fslr_ctx* c) {
  SegmentWork* w = c->sgw;
  if (!w) return;
  dfree(w->out), dfree(w->qkey), dfree(w->qend), dfree(w->rbuf), dfree(w->wbuf), dfree(w->wbuf64), dfree(w->tbuf);
  dfree(w->tbuf64), dfree(w->tbuf8), dfree(w->vbuf), dfree(w->cnt), dfree(w->temp), dfree(w->lbuf);
  if (w->host) (void)hipHostFree(w->host);
  if (w->stage) (void)hipHostFree(w->stage);
  if (w->ev_ok)
    for (hipEvent_t e : w->ev) (void)hipEventDestroy(e);
  delete w;
  c->sgw = nullptr;
}

namespace {

// ---- ordinals -----------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_seg_keys(const int* __restrict__ por, long long n, long long n_rows,
                                                     unsigned* __restrict__ key, unsigned* __restrict__ val) {
  for (long long r = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; r < n; r += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(r, n);
    const int row = por[r];
    key[r] = (row >= 0 && row < n_rows) ? static_cast<unsigned>(row) + 1u : 0u;
    val[r] = static_cast<unsigned>(r);
  }
}

__global__ __launch_bounds__(kBlock) void k_seg_rowprep(const int* __restrict__ nreads, const long long* __restrict__ tok_off,
                                                        long long n_rows, int* __restrict__ nr, long long* __restrict__ lk) {
  for (long long l = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; l <= n_rows; l += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(l, n_rows + 1);
    int k = 0;
    long long v = 0;
    if (l < n_rows) {
      k = nreads[l];
      if (k >= 2) v = (tok_off[l + 1] - tok_off[l]) * k;      // a row of one read needs no bucket
    }
    nr[l] = k;                                      // [n_rows] = 0: the scans' last outputs are the totals
    lk[l] = v;
  }
}

__global__ __launch_bounds__(kBlock) void k_seg_ord(const unsigned* __restrict__ key, const unsigned* __restrict__ val,
                                                    const int* __restrict__ rfirst, long long n, long long n_rows,
                                                    int* __restrict__ ord) {
  const long long n_out = n - rfirst[n_rows];       // the reads of key 0 stand in front
  for (long long s = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; s < n; s += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(s, n);
    const unsigned k = key[s];
    if (k == 0u) continue;
    FSLR_BOUND(k - 1u, n_rows);
    FSLR_BOUND(val[s], n);
    ord[val[s]] = static_cast<int>(s - n_out - rfirst[k - 1u]);
  }
}

// ---- emit ---------------------------------------------------------------------------------------
// a clustered read as the emit kernels see it: len == 0 when it writes nothing
struct EmitRead {
  int len = 0, first = 0, k = 0, o = 0, flip = 0;
  long long t0 = 0, b0 = 0;
};

// what segshared.hpp's chain walk writes per piece here: the value of (row, position p, ordinal o) into the row's
// buckets, or straight into the output for a row of one read
struct EmitArgs {
  RealReads rr;                      // the real lists on a context with virtual reads (n = the real reads)
  const int* longs;                  // [n_long] the reads of k_seg_emit_long
  long long n_long;
  const int4* iv;                    // {chrom, start, end, thr}
  const int *qkey, *qend;            // qend null: no gaps
  const int* por;
  const unsigned char* flipped;
  const int *ord, *nreads;
  const long long *tok_off, *base;
  long long n, ni, n_rows, nt, n_vals, n_quads;
  int *vs, *ve, *vg;                 // [n_vals] the buckets
  int* out;                          // [9 x nt]
  int* slot_k;                       // [nt]
  long long* slot_base;              // [nt]
  unsigned char* slot_last;          // [nt]

  using Read = EmitRead;
  static constexpr bool kPrevGap = false;

  // read r of `len` intervals (the caller checked it against its kernel's range): its row, ordinal and bucket
  __device__ __forceinline__ EmitRead read(long long r, int first, int len) const {
    EmitRead e;
    e.first = first;
    const int row = por[r];
    if (row < 0 || row >= n_rows) return e;
    e.t0 = tok_off[row];
    e.k = nreads[row];
    e.o = ord[r];
    e.b0 = base[row];
    e.flip = flipped[r] != 0;
    // a read's row has the read's length and holds its ordinal, so every slot below lies in the row
    if (tok_off[row + 1] - e.t0 == len && e.o >= 0 && e.o < e.k) e.len = len;
    return e;
  }

  // the interval at chain rank `rank` of read e: record rec, and with link (a next piece exists and the caller
  // brought the query ends) the gap to that piece
  __device__ __forceinline__ void piece(const EmitRead& e, int rank, long long, const int4& rec, bool link, int gap, int) const {
    const int len = e.len, k = e.k, o = e.o;
    const long long t0 = e.t0, b0 = e.b0;
    const int p = e.flip ? len - 1 - rank : rank;
    const long long s = t0 + p;
    FSLR_BOUND(s, nt);
    // the link to the next piece of the read's own chain lies between positions p and p -+ 1: stored at the smaller
    const int pl = e.flip ? len - 2 - rank : rank;
    if (k == 1) {
      out[s] = out[nt + s] = out[2 * nt + s] = rec.y;
      out[3 * nt + s] = out[4 * nt + s] = out[5 * nt + s] = rec.z;
      if (link) {
        FSLR_BOUND(t0 + pl, nt);
        out[6 * nt + t0 + pl] = out[7 * nt + t0 + pl] = out[8 * nt + t0 + pl] = gap;
      }
      slot_k[s] = 1;
    } else {
      const long long at = b0 + static_cast<long long>(p) * k + o;
      FSLR_BOUND(at, n_vals);
      vs[at] = rec.y;
      ve[at] = rec.z;
      if (link) {
        FSLR_BOUND(b0 + static_cast<long long>(pl) * k + o, n_vals);
        vg[b0 + static_cast<long long>(pl) * k + o] = gap;
      }
      if (o == 0) {                                   // one read per row describes its slots
        slot_k[s] = k;
        slot_base[s] = b0 + static_cast<long long>(p) * k;
        slot_last[s] = static_cast<unsigned char>(p == len - 1);
      }
    }
  }
};

// four reads per wavefront on 16 lanes, or 32 / 64 lanes when one is longer (segshared.hpp emit_waves)
__global__ __launch_bounds__(kBlock) void k_seg_emit(EmitArgs a) {
  __shared__ int s_slot[kWavesPerBlock][kWave];
  emit_waves(a, s_slot[threadIdx.x / kWave]);
}

// one workgroup per clustered read of more than FSLR_MAX_L intervals (segshared.hpp emit_long_blocks); 32 KiB of
// LDS, no atomics
__global__ __launch_bounds__(kChainBlock) void k_seg_emit_long(EmitArgs a) {
  __shared__ unsigned long long s_w[kChainMaxL];
  emit_long_blocks(a, s_w);
}

// ---- host side ----------------------------------------------------------------------------------
int ensure_temp(fslr_ctx* c, SegmentWork* w, size_t bytes) {
  if (bytes <= w->temp_bytes && w->temp) return FSLR_OK;
  dfree(w->temp);
  w->temp_bytes = 0;
  HIP_TRY(c, hipMalloc(&w->temp, bytes ? bytes : 1));
  w->temp_bytes = bytes ? bytes : 1;
  return FSLR_OK;
}

// host -> device through the pinned chunk; each chunk syncs (the chunk is reused)
int up(fslr_ctx* c, SegmentWork* w, void* dst, const void* src, size_t bytes) {
  for (size_t at = 0; at < bytes; at += kStageBytes) {
    const size_t m = std::min(kStageBytes, bytes - at);
    std::memcpy(w->stage, static_cast<const unsigned char*>(src) + at, m);
    HIP_TRY(c, hipMemcpyAsync(static_cast<unsigned char*>(dst) + at, w->stage, m, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  return FSLR_OK;
}

// the rows of a result (allocated apart from the resident ones: a failure keeps those)
struct NewRows {
  int* out = nullptr;
  ~NewRows() { dfree(out); }
};

// fslr_cluster_path_segments (any = false: a context with virtual reads is refused) and
// fslr_cluster_path_segments_any.  On a context without virtual reads the two run the same code.
int segments_run(fslr_ctx* c, const int32_t* iv_qkey, const int32_t* iv_qend, int64_t n_intervals, int64_t* n_tokens_out,
                 bool any) {
  if (!c) return FSLR_ERR_INVALID;
  if (!c->reads_set || c->n == 0) return fail(c, FSLR_ERR_STATE, "fslr_cluster_path_segments: no reads set");
  if (int rc = search_state(c, any ? "fslr_cluster_path_segments_any" : "fslr_cluster_path_segments")) return rc;
  const int* cid = nullptr;
  int64_t tn = 0, nc = 0;
  if (!fslr_cluster_view(c, &cid, &tn, &nc))
    return fail(c, FSLR_ERR_STATE, "fslr_cluster_path_segments: no cluster table (fslr_cluster_table first)");
  const int64_t n_real = c->lg_set ? c->lg_n_real : c->n;
  if (tn != n_real)
    return fail(c, FSLR_ERR_STATE, "fslr_cluster_path_segments: the cluster table holds " + std::to_string(tn) +
                                       " reads, the context " + std::to_string(n_real) +
                                       " (a table from before fslr_append_reads / fslr_remove_reads, or of other "
                                       "reads: fslr_cluster_table again)");
  const long long* loff = nullptr;
  const int* lrows = nullptr;
  int64_t lcap = 0, n_loci = 0, lnc = 0;
  if (!fslr_loci_view(c, &loff, &lrows, &lcap, &n_loci, &lnc) || lnc != nc)
    return fail(c, FSLR_ERR_STATE, "fslr_cluster_path_segments: no cluster loci of this table (fslr_cluster_loci first)");
  fslr_paths_rows pv;
  if (!fslr_paths_view(c, &pv) || pv.n_clusters != nc || pv.n != n_real)
    return fail(c, FSLR_ERR_STATE, "fslr_cluster_path_segments: no cluster paths of this table (fslr_cluster_paths first)");
  if (c->lg_set && !any)
    return fail(c, FSLR_ERR_INVALID, "fslr_cluster_path_segments: the context holds reads of more than " +
                                         std::to_string(FSLR_MAX_L) + " intervals (out of scope here)");
  if (!iv_qkey) return fail(c, FSLR_ERR_INVALID, "fslr_cluster_path_segments: iv_qkey is NULL");
  if (n_intervals != c->ni)
    return fail(c, FSLR_ERR_INVALID, "fslr_cluster_path_segments: n_intervals " + std::to_string(n_intervals) +
                                         ", the context holds " + std::to_string(c->ni));
  // n: the real reads (on a context with virtual reads the chunks behind them are no reads of their own)
  const bool virt = c->lg_set;
  const int64_t n = n_real, ni = c->ni, n_rows = pv.n_rows, nt = pv.n_tokens;
  const RealReads rr{c->rmeta, virt ? c->lg_rlen : nullptr, virt ? c->lg_off2 : nullptr};
  if (virt && !c->lg_perm.empty() && static_cast<int64_t>(c->lg_perm.size()) != ni)
    return fail(c, FSLR_ERR_STATE, "fslr_cluster_path_segments: the interval permutation does not span the intervals (internal)");
  if (ni > kMaxItems || n >= kMaxItems)
    return fail(c, FSLR_ERR_INVALID, "fslr_cluster_path_segments: " + std::to_string(ni) + " intervals: more than 2^30");
  if (n_rows < 0 || n_rows > n || nt < n_rows || nt > ni)
    return fail(c, FSLR_ERR_STATE, "fslr_cluster_path_segments: inconsistent path rows (internal)");
  HIP_TRY(c, hipSetDevice(c->device));
  if (!c->sgw) c->sgw = new SegmentWork();
  SegmentWork* w = c->sgw;
  int rc;
  hipStream_t st = c->stream;
  if (!w->cnt)
    if ((rc = dalloc(c, &w->cnt, 4))) return rc;
  if (!w->host) HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&w->host), 4 * sizeof(long long), hipHostMallocDefault));
  if (!w->stage) HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&w->stage), kStageBytes, hipHostMallocDefault));
  if (c->profiling && !w->ev_ok) {
    for (hipEvent_t& e : w->ev) HIP_TRY(c, hipEventCreate(&e));
    w->ev_ok = true;
  }
  if (ni > w->icap || !w->qkey) {
    w->icap = 0;
    if ((rc = dalloc(c, &w->qkey, static_cast<size_t>(ni))) || (rc = dalloc(c, &w->qend, static_cast<size_t>(ni)))) return rc;
    w->icap = ni;
  }
  if (n > w->rcap || !w->rbuf) {
    w->rcap = 0;
    if ((rc = dalloc(c, &w->rbuf, static_cast<size_t>(5 * n)))) return rc;
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
  }
  if (n_rows > w->wcap || !w->wbuf) {
    w->wcap = 0;
    if ((rc = dalloc(c, &w->wbuf, static_cast<size_t>(2 * (n_rows + 1)))) || (rc = dalloc(c, &w->wbuf64, static_cast<size_t>(2 * (n_rows + 1)))))
      return rc;
    w->wcap = n_rows;
  }
  if (nt > w->tcap || !w->tbuf) {
    w->tcap = 0;
    if ((rc = dalloc(c, &w->tbuf, static_cast<size_t>(4 * nt))) || (rc = dalloc(c, &w->tbuf64, static_cast<size_t>(nt))) ||
        (rc = dalloc(c, &w->tbuf8, static_cast<size_t>(4 * nt))))
      return rc;
    w->tcap = nt;
  }
  NewRows nr;
  if ((rc = dalloc(c, &nr.out, static_cast<size_t>(9 * nt)))) return rc;
  unsigned *key_in = w->rbuf, *key_out = key_in + w->rcap, *val_in = key_out + w->rcap, *val_out = val_in + w->rcap;
  int* ord = reinterpret_cast<int*>(val_out + w->rcap);
  int *nrin = w->wbuf, *rfirst = nrin + (w->wcap + 1);
  long long *lk = w->wbuf64, *base = lk + (w->wcap + 1);
  int *slot_k = w->tbuf, *lists = slot_k + w->tcap;           // lists: 3 x tcap
  unsigned char *slot_last = w->tbuf8, *flags = slot_last + w->tcap;   // flags: 3 x nt
  const int kbits = bits_for(n_rows + 1), ni_n = static_cast<int>(n), nw = static_cast<int>(n_rows + 1);
  size_t tb_sort = 0, tb_s32 = 0, tb_s64 = 0, tb_sel = 0, tb_long = 0;
  HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(nullptr, tb_sort, key_in, key_out, val_in, val_out, ni_n, 0, kbits, st));
  HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, tb_s32, nrin, rfirst, nw, st));
  HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, tb_s64, lk, base, nw, st));
  hipcub::CountingInputIterator<int> iota(0);
  HIP_TRY(c, hipcub::DeviceSelect::Flagged(nullptr, tb_sel, iota, flags, lists, w->cnt, static_cast<int>(std::max<int64_t>(nt, 1)), st));
  if (virt) HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, tb_long, lflag, lpos, static_cast<int>(n + 1), st));
  if ((rc = ensure_temp(c, w, std::max(std::max(std::max(tb_sort, tb_sel), std::max(tb_s32, tb_s64)), tb_long)))) return rc;
  int small = 0, lds = 0;
  tier_caps(&small, &lds);
  w->timed = false;
  w->ms = 0;
  if (virt && !c->lg_perm.empty()) {                // the caller's order is the real CSR's
    if ((rc = up_perm(c, w->stage, kStageBytes, w->qkey, iv_qkey, c->lg_perm))) return rc;
    if (iv_qend)
      if ((rc = up_perm(c, w->stage, kStageBytes, w->qend, iv_qend, c->lg_perm))) return rc;
  } else {
    if ((rc = up(c, w, w->qkey, iv_qkey, static_cast<size_t>(ni) * sizeof(int)))) return rc;
    if (iv_qend)
      if ((rc = up(c, w, w->qend, iv_qend, static_cast<size_t>(ni) * sizeof(int)))) return rc;
  }
  if (c->profiling) HIP_TRY(c, hipEventRecord(w->ev[0], st));     // the columns are up: the device work from here
  if (nt > 0) {
    size_t tb;
    k_seg_keys<<<grid_for(n), kBlock, 0, st>>>(pv.path_of_read, n, n_rows, key_in, val_in);
    HIP_TRY(c, hipGetLastError());
    tb = w->temp_bytes;
    HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(w->temp, tb, key_in, key_out, val_in, val_out, ni_n, 0, kbits, st));
    k_seg_rowprep<<<grid_for(n_rows + 1), kBlock, 0, st>>>(pv.rows, pv.tok_off, n_rows, nrin, lk);
    HIP_TRY(c, hipGetLastError());
    tb = w->temp_bytes;
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(w->temp, tb, nrin, rfirst, nw, st));
    tb = w->temp_bytes;
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(w->temp, tb, lk, base, nw, st));
    k_seg_ord<<<grid_for(n), kBlock, 0, st>>>(key_out, val_out, rfirst, n, n_rows, ord);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(w->host, base + n_rows, sizeof(long long), hipMemcpyDeviceToHost, st));
    if (virt) {
      // the clustered reads of more than FSLR_MAX_L intervals: flag and scan; their count comes back beside n_vals
      k_chain_long_flag<<<grid_for(n + 1), kChainBlock, 0, st>>>(pv.path_of_read, rr.rlen, n, lflag);
      HIP_TRY(c, hipGetLastError());
      tb = w->temp_bytes;
      HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(w->temp, tb, lflag, lpos, static_cast<int>(n + 1), st));
      HIP_TRY(c, hipMemcpyAsync(w->host + 1, lpos + n, sizeof(int), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(c, hipStreamSynchronize(st));
    const int64_t n_vals = w->host[0];               // the intervals of the rows of two or more reads
    const int64_t n_long = virt ? *reinterpret_cast<const int*>(w->host + 1) : 0;
    if (n_vals < 0 || n_vals > ni || n_long < 0 || n_long > n)
      return fail(c, FSLR_ERR_STATE, "fslr_cluster_path_segments: inconsistent counts (internal)");
    if (n_vals > w->vcap || !w->vbuf) {
      w->vcap = 0;
      if ((rc = dalloc(c, &w->vbuf, static_cast<size_t>(3 * std::max<int64_t>(n_vals, 1))))) return rc;
      w->vcap = std::max<int64_t>(n_vals, 1);
    }
    int *vs = w->vbuf, *ve = vs + w->vcap, *vg = ve + w->vcap;
    // the gap columns: 0 for a row's last slot and without iv_qend, every other word is written once below
    HIP_TRY(c, hipMemsetAsync(nr.out + 6 * nt, 0, static_cast<size_t>(3 * nt) * sizeof(int), st));
    HIP_TRY(c, hipMemsetAsync(slot_k, 0, static_cast<size_t>(nt) * sizeof(int), st));
    const long long n_quads = (n + 3) / 4;
    EmitArgs ea{rr, longs, n_long, c->iv, w->qkey, iv_qend ? w->qend : nullptr, pv.path_of_read, pv.flipped, ord, pv.rows, pv.tok_off, base,
                n, ni, n_rows, nt, n_vals, n_quads, vs, ve, vg, nr.out, slot_k, w->tbuf64, slot_last};
    k_seg_emit<<<grid_for(n_quads, kWavesPerBlock, 256 * 32), kBlock, 0, st>>>(ea);
    HIP_TRY(c, hipGetLastError());
    if (n_long > 0) {                                // only when such reads exist, one workgroup each
      k_chain_long_compact<<<grid_for(n), kChainBlock, 0, st>>>(lflag, lpos, n, n_long, longs);
      HIP_TRY(c, hipGetLastError());
      k_seg_emit_long<<<grid_for(n_long, 1, 256 * 8), kChainBlock, 0, st>>>(ea);
      HIP_TRY(c, hipGetLastError());
    }
    if (n_vals > 0) {
      k_seg_flags<<<grid_for(nt), kBlock, 0, st>>>(slot_k, nt, small, lds, flags);
      HIP_TRY(c, hipGetLastError());
      for (int t = 0; t < 3; ++t) {
        tb = w->temp_bytes;
        HIP_TRY(c, hipcub::DeviceSelect::Flagged(w->temp, tb, iota, flags + t * nt, lists + t * w->tcap, w->cnt + t, static_cast<int>(nt), st));
      }
      HIP_TRY(c, hipMemcpyAsync(w->host, w->cnt, 3 * sizeof(int), hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipStreamSynchronize(st));
      const int* hc = reinterpret_cast<const int*>(w->host);
      const int64_t cnt[3] = {hc[0], hc[1], hc[2]};
      for (int t = 0; t < 3; ++t)
        if (cnt[t] < 0 || cnt[t] > nt) return fail(c, FSLR_ERR_STATE, "fslr_cluster_path_segments: inconsistent counts (internal)");
      const int n_streams = iv_qend ? 3 : 2;
      // every stream of a slot holds the row's k values; the gap stream of a row's last slot holds none
      SelArgs sa{nullptr, 0, 0, {slot_k, slot_k, slot_k}, w->tbuf64, slot_last, {vs, ve, vg}, nt, n_vals, nr.out};
      HIP_TRY(c, launch_tiers(sa, lists, w->tcap, cnt, n_streams, st));
    }
  }
  if (c->profiling) HIP_TRY(c, hipEventRecord(w->ev[1], st));
  HIP_TRY(c, hipStreamSynchronize(st));
  if (c->profiling) {
    HIP_TRY(c, hipEventElapsedTime(&w->ms, w->ev[0], w->ev[1]));
    w->timed = true;
  }
  // install
  std::swap(w->out, nr.out);
  w->n_tokens = nt;
  w->have = true;
  if (n_tokens_out) *n_tokens_out = nt;
  return FSLR_OK;
}

}  // namespace

extern "C" {

int fslr_cluster_path_segments(fslr_ctx* c, const int32_t* iv_qkey, const int32_t* iv_qend, int64_t n_intervals,
                               int64_t* n_tokens_out) {
  return segments_run(c, iv_qkey, iv_qend, n_intervals, n_tokens_out, false);
}

int fslr_cluster_path_segments_any(fslr_ctx* c, const int32_t* iv_qkey, const int32_t* iv_qend, int64_t n_intervals,
                                   int64_t* n_tokens_out) {
  return segments_run(c, iv_qkey, iv_qend, n_intervals, n_tokens_out, true);
}

int fslr_get_cluster_path_segments(fslr_ctx* c, int32_t* start, int32_t* end, int32_t* gap, int64_t token_capacity) {
  if (!c) return FSLR_ERR_INVALID;
  SegmentWork* w = c->sgw;
  if (!w || !w->have)
    return fail(c, FSLR_ERR_STATE, "fslr_get_cluster_path_segments: fslr_cluster_path_segments first");
  if (token_capacity < w->n_tokens)
    return fail(c, FSLR_ERR_INVALID, "fslr_get_cluster_path_segments: token capacity " + std::to_string(token_capacity) +
                                         " < " + std::to_string(w->n_tokens) + " tokens");
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t nt = static_cast<size_t>(w->n_tokens);
  int32_t* out[3] = {start, end, gap};
  for (int k = 0; k < 3; ++k)
    if (out[k] && nt)
      HIP_TRY(c, hipMemcpyAsync(out[k], w->out + 3 * k * nt, 3 * nt * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FSLR_OK;
}

int fslr_cluster_path_segments_timings(fslr_ctx* c, float* ms) {
  if (!c || !ms) return FSLR_ERR_INVALID;
  SegmentWork* w = c->sgw;
  if (!w || !w->timed)
    return fail(c, FSLR_ERR_STATE,
                "fslr_cluster_path_segments_timings: no profiled fslr_cluster_path_segments (fslr_set_profiling 1 or 2)");
  ms[0] = w->ms;
  return FSLR_OK;
}

}  // extern "C"
