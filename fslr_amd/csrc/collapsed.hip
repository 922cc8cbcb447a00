// collapsed.hip — collapsed path segments: per slot of every maximal path row the minimum, lower median and maximum
// of the reference start and end of the intervals of ALL reads that collapse onto the row, and per link the same
// of the query-space gap; n_cov and n_link say how many values stand behind a slot (fslr_hip.h states the contract;
// DESIGN.md §3.10.8 the bytes; tests/collapsed_ref.py the plain statement).
//
// The path rows (paths.hip: tok_off, path_of_read, flipped) and the containment rows (containment.hip: coff, outer,
// offset, rev, collapse_to) are resident.  The caller brings the query key and, for the gaps, the query end per
// CSR interval.  Passes, all on the context's stream:
//   k_cl_init       per interval: key = all ones (lands nowhere: sorts behind every slot), item = its CSR position
//   k_cl_rowmap     per path row A, one thread: B = collapse_to[A] and, when B != A, the pair (A, B) by a binary
//                   search in outer[coff[A] .. coff[A + 1]): its offset o and direction d; a row whose pair is
//                   missing or does not fit B is marked and its reads write nothing
//   k_cl_emit       segshared.hpp's lane-group walk (segments.hip's k_seg_emit shares it): the interval at chain
//                   rank t of a read of row A lands in slot tok_off[B] + q; it writes key = slot * 2 + (it holds
//                   no link) and its gap word; a link belongs to the interval of its two that lies at the smaller
//                   slot, so a read that walks B backwards takes the gap from the piece before (one more round
//                   through the wavefront's 64 LDS slots)
//   fslr_cluster_collapsed_segments_any on virtual reads: k_chain_long_flag, a hipcub scan and k_chain_long_compact
//                   list the clustered reads of more than FSLR_MAX_L intervals, and when there are any
//   k_cl_emit_long  segshared.hpp's one-workgroup-per-read walk, chain.hpp's bitonic sort in 32 KiB of LDS
//   hipcub sort     one stable radix SortPairs of (key, item) on the bits of 2 * n_tokens + 1 keys: a slot's bucket
//                   is contiguous, its items with a link first
//   k_cl_gather     the three value streams in sorted order: start and end from the interval records, the gap word
//   k_cl_desc       per slot: base, n_link and n_cov by three binary searches in the sorted keys; a slot of one
//                   interval writes its outputs
//   k_seg_flags, hipcub select, k_seg_small / k_seg_lds / k_seg_select: segshared.hpp's tiers; the tier comes from
//                   n_cov, the gap stream takes the bucket's first n_link words
// No block waits for another and no atomic decides where anything lands (the select tier's integer LDS counters
// are the only atomics); no floating point.  The bytes are the same on every run.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cstdint>
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
struct CollapsedWork {
  // resident rows
  int* out = nullptr;                // [11 x n_tokens] start min, med, max; end ...; gap ...; n_cov; n_link
  int64_t n_tokens = 0;
  bool have = false;
  // the caller's columns, CSR interval order
  int* qkey = nullptr;               // [icap]
  int* qend = nullptr;               // [icap]
  // per interval: sort keys in / out, items in / out, the gap word; the sorted value streams
  unsigned* ibuf = nullptr;          // [5 x icap]
  int* vbuf = nullptr;               // [3 x icap]
  int64_t icap = 0;
  // fslr_cluster_collapsed_segments_any on virtual reads: flag, pos and the list of the clustered long reads
  int* lbuf = nullptr;               // [3 x (lcap + 1)]
  int64_t lcap = 0;
  // per row: {B, o, d, a}
  int4* rowmap = nullptr;            // [wcap]
  int64_t wcap = 0;
  // per slot: the tier lists (3), the bucket's first word, the tier flags (3)
  int* tbuf = nullptr;               // [3 x tcap]
  long long* tbuf64 = nullptr;       // [tcap]
  unsigned char* tbuf8 = nullptr;    // [3 x tcap]
  int64_t tcap = 0;
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
constexpr unsigned kNoSlot = ~0u;                           // the key of an interval that lands nowhere

template <typename T>
void dfree(T*& p) {
  if (p) (void)hipFree(p);
  p = nullptr;
}

}  // namespace

void fslr_collapsed_drop(fslr_ctx* c) {
  if (c->csw) c->csw->have = false;
}

void fslr_collapsed_free(fslr_ctx* c) {
  CollapsedWork* w = c->csw;
  if (!w) return;
  dfree(w->out), dfree(w->qkey), dfree(w->qend), dfree(w->ibuf), dfree(w->vbuf), dfree(w->lbuf), dfree(w->rowmap);
  dfree(w->tbuf), dfree(w->tbuf64), dfree(w->tbuf8), dfree(w->cnt), dfree(w->temp);
  if (w->host) (void)hipHostFree(w->host);
  if (w->stage) (void)hipHostFree(w->stage);
  if (w->ev_ok)
    for (hipEvent_t e : w->ev) (void)hipEventDestroy(e);
  delete w;
  c->csw = nullptr;
}

namespace {

// ---- items and the row map ----------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_cl_init(long long ni, unsigned* __restrict__ key, unsigned* __restrict__ item,
                                                    int* __restrict__ gap) {
  for (long long i = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; i < ni; i += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(i, ni);
    key[i] = kNoSlot;
    item[i] = static_cast<unsigned>(i);
    gap[i] = 0;
  }
}

struct RowMapArgs {
  const long long *coff, *tok_off;
  const int *outer, *offset, *collapse_to;
  const unsigned char* rev;
  long long n_rows, n_pairs, nt;
  int4* map;                         // [n_rows] {B, o, d, a}; B = -1: the row's reads write nothing
};

__global__ __launch_bounds__(kBlock) void k_cl_rowmap(RowMapArgs a) {
  for (long long r = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; r < a.n_rows; r += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(r, a.n_rows);
    const long long B = a.collapse_to[r];
    const long long la = a.tok_off[r + 1] - a.tok_off[r];
    long long o = 0;
    int d = 0;
    bool ok = B >= 0 && B < a.n_rows && la >= 1 && la <= kChainMaxL;
    if (ok && B != r) {
      // the pair (r, B): the outers of r ascend in coff[r] .. coff[r + 1]
      long long lo = max(0ll, min(a.coff[r], a.n_pairs)), hi = max(lo, min(a.coff[r + 1], a.n_pairs));
      const long long end = hi;
      for (int it = 0; it < 32 && lo < hi; ++it) {  // pairs <= 2^30: at most 31 halvings
        const long long mid = (lo + hi) >> 1;
        FSLR_BOUND(mid, a.n_pairs);
        if (a.outer[mid] < B)
          lo = mid + 1;
        else
          hi = mid;
      }
      ok = lo < end;
      if (ok) {
        FSLR_BOUND(lo, a.n_pairs);
        ok = a.outer[lo] == B;
        o = a.offset[lo];
        d = a.rev[lo] != 0;
      }
    }
    if (ok) {
      // every slot o .. o + la - 1 of B must lie in B, and B in the tokens: checked here, once per row
      const long long t0 = a.tok_off[B], lb = a.tok_off[B + 1] - t0;
      ok = o >= 0 && o + la <= lb && t0 >= 0 && t0 + lb <= a.nt;
    }
    a.map[r] = ok ? make_int4(static_cast<int>(B), static_cast<int>(o), d, static_cast<int>(la)) : make_int4(-1, 0, 0, 0);
  }
}

// ---- emit ---------------------------------------------------------------------------------------
// a clustered read as the walk sees it: len == 0 when it writes nothing
struct ColRead {
  int len = 0, first = 0, o = 0, d = 0, flip = 0;
  long long t0 = 0;                  // tok_off of the row it collapses to
};

// what segshared.hpp's chain walk writes per piece here: the item's key and its gap word
struct ColArgs {
  RealReads rr;                      // the real lists on a context with virtual reads (n = the real reads)
  const int* longs;                  // [n_long] the reads of k_cl_emit_long
  long long n_long;
  const int4* iv;                    // {chrom, start, end, thr}
  const int *qkey, *qend;            // qend null: no gaps
  const int* por;
  const unsigned char* flipped;
  const int4* map;                   // [n_rows] k_cl_rowmap's
  const long long* tok_off;
  long long n, ni, n_rows, nt, n_quads;
  unsigned* key;                     // [ni]
  int* gap;                          // [ni]

  using Read = ColRead;
  static constexpr bool kPrevGap = true;

  __device__ __forceinline__ ColRead read(long long r, int first, int len) const {
    ColRead e;
    e.first = first;
    const int row = por[r];
    if (row < 0 || row >= n_rows) return e;
    const int4 m = map[row];
    if (m.x < 0 || m.x >= n_rows || m.w != len) return e;      // the read's row has the read's length
    e.t0 = tok_off[m.x];
    e.o = m.y;
    e.d = m.z;
    e.flip = flipped[r] != 0;
    e.len = len;
    return e;
  }

  // the interval at chain rank `rank`, CSR position i: its slot in the row it collapses to, and whether it holds
  // a link: the one to the next piece when the read walks that row forwards, the one from the piece before when
  // it walks it backwards
  __device__ __forceinline__ void piece(const ColRead& e, int rank, long long i, const int4&, bool, int gap_next, int gap_prev) const {
    const int len = e.len;
    const int p = e.flip ? len - 1 - rank : rank;
    const int q = e.d ? e.o + (len - 1 - p) : e.o + p;
    const long long s = e.t0 + q;
    if (s < 0 || s >= nt) return;                   // k_cl_rowmap checked the row: never taken
    const bool fwd = e.flip == e.d;                 // q ascends with the rank
    const bool holds = fwd ? rank + 1 < len : rank > 0;
    FSLR_BOUND(i, ni);
    key[i] = static_cast<unsigned>(s) * 2u + (holds ? 0u : 1u);
    if (qend) gap[i] = holds ? (fwd ? gap_next : gap_prev) : 0;
  }
};

__global__ __launch_bounds__(kBlock) void k_cl_emit(ColArgs a) {
  __shared__ int s_slot[kWavesPerBlock][kWave];
  emit_waves(a, s_slot[threadIdx.x / kWave]);
}

__global__ __launch_bounds__(kChainBlock) void k_cl_emit_long(ColArgs a) {
  __shared__ unsigned long long s_w[kChainMaxL];
  emit_long_blocks(a, s_w);
}

// ---- placement ----------------------------------------------------------------------------------
struct PlaceArgs {
  const unsigned *skey, *sitem;      // [ni] sorted keys and their items
  const int4* iv;
  const int* gap;                    // [ni] by item; null: no gaps
  long long ni, nt;
  int *vs, *ve, *vg;                 // [ni] the value streams in sorted order
  long long* slot_base;              // [nt]
  int* out;                          // [11 x nt]
};

__global__ __launch_bounds__(kBlock) void k_cl_gather(PlaceArgs a) {
  for (long long p = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; p < a.ni; p += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(p, a.ni);
    if (a.skey[p] >= 2ull * static_cast<unsigned long long>(a.nt)) continue;       // lands nowhere
    const long long i = a.sitem[p];
    FSLR_BOUND(i, a.ni);
    if (i >= a.ni) continue;
    const int4 rec = a.iv[i];
    a.vs[p] = rec.y;
    a.ve[p] = rec.z;
    if (a.gap) a.vg[p] = a.gap[i];
  }
}

// the first place of the sorted keys that holds a key >= t
__device__ __forceinline__ long long key_lower(const PlaceArgs& a, long long lo, unsigned long long t) {
  long long hi = a.ni;
  for (int it = 0; it < 32 && lo < hi; ++it) {      // items <= 2^30: at most 31 halvings
    const long long mid = (lo + hi) >> 1;
    FSLR_BOUND(mid, a.ni);
    if (a.skey[mid] < t)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kBlock) void k_cl_desc(PlaceArgs a) {
  for (long long s = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; s < a.nt; s += gridDim.x * static_cast<long long>(kBlock)) {
    FSLR_BOUND(s, a.nt);
    const unsigned long long k0 = 2ull * static_cast<unsigned long long>(s);
    const long long b0 = key_lower(a, 0, k0), b1 = key_lower(a, b0, k0 + 1ull), b2 = key_lower(a, b1, k0 + 2ull);
    const int n_cov = static_cast<int>(b2 - b0), n_link = static_cast<int>(b1 - b0);
    a.slot_base[s] = b0;
    a.out[9 * a.nt + s] = n_cov;
    a.out[10 * a.nt + s] = n_link;
    if (n_cov == 1) {                               // one interval: no tier takes the slot
      FSLR_BOUND(b0, a.ni);
      a.out[s] = a.out[a.nt + s] = a.out[2 * a.nt + s] = a.vs[b0];
      a.out[3 * a.nt + s] = a.out[4 * a.nt + s] = a.out[5 * a.nt + s] = a.ve[b0];
      if (n_link == 1 && a.gap) a.out[6 * a.nt + s] = a.out[7 * a.nt + s] = a.out[8 * a.nt + s] = a.vg[b0];
    }
  }
}

// ---- host side ----------------------------------------------------------------------------------
int ensure_temp(fslr_ctx* c, CollapsedWork* w, size_t bytes) {
  if (bytes <= w->temp_bytes && w->temp) return FSLR_OK;
  dfree(w->temp);
  w->temp_bytes = 0;
  HIP_TRY(c, hipMalloc(&w->temp, bytes ? bytes : 1));
  w->temp_bytes = bytes ? bytes : 1;
  return FSLR_OK;
}

// host -> device through the pinned chunk; each chunk syncs (the chunk is reused)
int up(fslr_ctx* c, CollapsedWork* w, void* dst, const void* src, size_t bytes) {
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

// fslr_cluster_collapsed_segments (any = false: a context with virtual reads is refused) and
// fslr_cluster_collapsed_segments_any.  On a context without virtual reads the two run the same code.
int collapsed_run(fslr_ctx* c, const int32_t* iv_qkey, const int32_t* iv_qend, int64_t n_intervals, int64_t* n_tokens_out,
                  bool any) {
  if (!c) return FSLR_ERR_INVALID;
  if (!c->reads_set || c->n == 0) return fail(c, FSLR_ERR_STATE, "fslr_cluster_collapsed_segments: no reads set");
  if (int rc = search_state(c, any ? "fslr_cluster_collapsed_segments_any" : "fslr_cluster_collapsed_segments")) return rc;
  const int* cid = nullptr;
  int64_t tn = 0, nc = 0;
  if (!fslr_cluster_view(c, &cid, &tn, &nc))
    return fail(c, FSLR_ERR_STATE, "fslr_cluster_collapsed_segments: no cluster table (fslr_cluster_table first)");
  const int64_t n_real = c->lg_set ? c->lg_n_real : c->n;
  if (tn != n_real)
    return fail(c, FSLR_ERR_STATE, "fslr_cluster_collapsed_segments: the cluster table holds " + std::to_string(tn) +
                                       " reads, the context " + std::to_string(n_real) +
                                       " (a table from before fslr_append_reads / fslr_remove_reads, or of other "
                                       "reads: fslr_cluster_table again)");
  const long long* loff = nullptr;
  const int* lrows = nullptr;
  int64_t lcap = 0, n_loci = 0, lnc = 0;
  if (!fslr_loci_view(c, &loff, &lrows, &lcap, &n_loci, &lnc) || lnc != nc)
    return fail(c, FSLR_ERR_STATE, "fslr_cluster_collapsed_segments: no cluster loci of this table (fslr_cluster_loci first)");
  fslr_paths_rows pv;
  if (!fslr_paths_view(c, &pv) || pv.n_clusters != nc || pv.n != n_real)
    return fail(c, FSLR_ERR_STATE, "fslr_cluster_collapsed_segments: no cluster paths of this table (fslr_cluster_paths first)");
  fslr_containment_rows cv;
  if (!fslr_containment_view(c, &cv) || cv.n_rows != pv.n_rows)
    return fail(c, FSLR_ERR_STATE, "fslr_cluster_collapsed_segments: no path containment of these cluster paths "
                                   "(fslr_cluster_path_containment first)");
  if (c->lg_set && !any)
    return fail(c, FSLR_ERR_INVALID, "fslr_cluster_collapsed_segments: the context holds reads of more than " +
                                         std::to_string(FSLR_MAX_L) + " intervals (fslr_cluster_collapsed_segments_any takes them)");
  if (!iv_qkey) return fail(c, FSLR_ERR_INVALID, "fslr_cluster_collapsed_segments: iv_qkey is NULL");
  if (n_intervals != c->ni)
    return fail(c, FSLR_ERR_INVALID, "fslr_cluster_collapsed_segments: n_intervals " + std::to_string(n_intervals) +
                                         ", the context holds " + std::to_string(c->ni));
  // n: the real reads (on a context with virtual reads the chunks behind them are no reads of their own)
  const bool virt = c->lg_set;
  const int64_t n = n_real, ni = c->ni, n_rows = pv.n_rows, nt = pv.n_tokens, n_pairs = cv.n_pairs;
  const RealReads rr{c->rmeta, virt ? c->lg_rlen : nullptr, virt ? c->lg_off2 : nullptr};
  if (virt && !c->lg_perm.empty() && static_cast<int64_t>(c->lg_perm.size()) != ni)
    return fail(c, FSLR_ERR_STATE, "fslr_cluster_collapsed_segments: the interval permutation does not span the intervals (internal)");
  if (ni > kMaxItems || n >= kMaxItems)
    return fail(c, FSLR_ERR_INVALID, "fslr_cluster_collapsed_segments: " + std::to_string(ni) + " intervals: more than 2^30");
  if (n_rows < 0 || n_rows > n || nt < n_rows || nt > ni || n_pairs < 0 || (n_pairs > 0 && (!cv.outer || !cv.offset || !cv.rev)) ||
      (n_rows > 0 && (!cv.coff || !cv.collapse_to)))
    return fail(c, FSLR_ERR_STATE, "fslr_cluster_collapsed_segments: inconsistent path or containment rows (internal)");
  HIP_TRY(c, hipSetDevice(c->device));
  if (!c->csw) c->csw = new CollapsedWork();
  CollapsedWork* w = c->csw;
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
    if ((rc = dalloc(c, &w->qkey, static_cast<size_t>(ni))) || (rc = dalloc(c, &w->qend, static_cast<size_t>(ni))) ||
        (rc = dalloc(c, &w->ibuf, static_cast<size_t>(5 * ni))) || (rc = dalloc(c, &w->vbuf, static_cast<size_t>(3 * ni))))
      return rc;
    w->icap = ni;
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
  if (n_rows > w->wcap || !w->rowmap) {
    w->wcap = 0;
    if ((rc = dalloc(c, &w->rowmap, static_cast<size_t>(n_rows)))) return rc;
    w->wcap = n_rows;
  }
  if (nt > w->tcap || !w->tbuf) {
    w->tcap = 0;
    if ((rc = dalloc(c, &w->tbuf, static_cast<size_t>(3 * nt))) || (rc = dalloc(c, &w->tbuf64, static_cast<size_t>(nt))) ||
        (rc = dalloc(c, &w->tbuf8, static_cast<size_t>(3 * nt))))
      return rc;
    w->tcap = nt;
  }
  NewRows nr;
  if ((rc = dalloc(c, &nr.out, static_cast<size_t>(11 * nt)))) return rc;
  unsigned *key_in = w->ibuf, *key_out = key_in + w->icap, *val_in = key_out + w->icap, *val_out = val_in + w->icap;
  int* gapw = reinterpret_cast<int*>(val_out + w->icap);
  int *vs = w->vbuf, *ve = vs + w->icap, *vg = ve + w->icap;
  int* lists = w->tbuf;                               // 3 x tcap
  unsigned char* flags = w->tbuf8;                    // 3 x nt
  int *n_cov = nr.out + 9 * nt, *n_link = nr.out + 10 * nt;
  // one key more than the slots' 2 * nt: the intervals that land nowhere sort behind them
  const int kbits = std::min(32, bits_for(2 * nt + 1)), ni_i = static_cast<int>(ni);
  size_t tb_sort = 0, tb_sel = 0, tb_long = 0;
  HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(nullptr, tb_sort, key_in, key_out, val_in, val_out, ni_i, 0, kbits, st));
  hipcub::CountingInputIterator<int> iota(0);
  HIP_TRY(c, hipcub::DeviceSelect::Flagged(nullptr, tb_sel, iota, flags, lists, w->cnt, static_cast<int>(std::max<int64_t>(nt, 1)), st));
  if (virt) HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, tb_long, lflag, lpos, static_cast<int>(n + 1), st));
  if ((rc = ensure_temp(c, w, std::max(std::max(tb_sort, tb_sel), tb_long)))) return rc;
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
    // every column is 0 where nothing lands: the slots of the rows that are not maximal, the gaps of a last slot
    HIP_TRY(c, hipMemsetAsync(nr.out, 0, static_cast<size_t>(11 * nt) * sizeof(int), st));
    k_cl_init<<<grid_for(ni), kBlock, 0, st>>>(ni, key_in, val_in, gapw);
    HIP_TRY(c, hipGetLastError());
    RowMapArgs ra{cv.coff, pv.tok_off, cv.outer, cv.offset, cv.collapse_to, cv.rev, n_rows, n_pairs, nt, w->rowmap};
    k_cl_rowmap<<<grid_for(n_rows), kBlock, 0, st>>>(ra);
    HIP_TRY(c, hipGetLastError());
    int64_t n_long = 0;
    if (virt) {
      // the clustered reads of more than FSLR_MAX_L intervals: flag and scan; their count comes back
      k_chain_long_flag<<<grid_for(n + 1), kChainBlock, 0, st>>>(pv.path_of_read, rr.rlen, n, lflag);
      HIP_TRY(c, hipGetLastError());
      tb = w->temp_bytes;
      HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(w->temp, tb, lflag, lpos, static_cast<int>(n + 1), st));
      HIP_TRY(c, hipMemcpyAsync(w->host, lpos + n, sizeof(int), hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipStreamSynchronize(st));
      n_long = *reinterpret_cast<const int*>(w->host);
      if (n_long < 0 || n_long > n)
        return fail(c, FSLR_ERR_STATE, "fslr_cluster_collapsed_segments: inconsistent counts (internal)");
    }
    const long long n_quads = (n + 3) / 4;
    ColArgs ea{rr, longs, n_long, c->iv, w->qkey, iv_qend ? w->qend : nullptr, pv.path_of_read, pv.flipped, w->rowmap, pv.tok_off,
               n, ni, n_rows, nt, n_quads, key_in, gapw};
    k_cl_emit<<<grid_for(n_quads, kWavesPerBlock, 256 * 32), kBlock, 0, st>>>(ea);
    HIP_TRY(c, hipGetLastError());
    if (n_long > 0) {                                // only when such reads exist, one workgroup each
      k_chain_long_compact<<<grid_for(n), kChainBlock, 0, st>>>(lflag, lpos, n, n_long, longs);
      HIP_TRY(c, hipGetLastError());
      k_cl_emit_long<<<grid_for(n_long, 1, 256 * 8), kChainBlock, 0, st>>>(ea);
      HIP_TRY(c, hipGetLastError());
    }
    tb = w->temp_bytes;
    HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(w->temp, tb, key_in, key_out, val_in, val_out, ni_i, 0, kbits, st));
    PlaceArgs pa{key_out, val_out, c->iv, iv_qend ? gapw : nullptr, ni, nt, vs, ve, vg, w->tbuf64, nr.out};
    k_cl_gather<<<grid_for(ni), kBlock, 0, st>>>(pa);
    HIP_TRY(c, hipGetLastError());
    k_cl_desc<<<grid_for(nt), kBlock, 0, st>>>(pa);
    HIP_TRY(c, hipGetLastError());
    k_seg_flags<<<grid_for(nt), kBlock, 0, st>>>(n_cov, nt, small, lds, flags);
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
      if (cnt[t] < 0 || cnt[t] > nt) return fail(c, FSLR_ERR_STATE, "fslr_cluster_collapsed_segments: inconsistent counts (internal)");
    // the tier comes from n_cov; the gap stream takes the first n_link words of the same bucket (n_link <= n_cov, so
    // it fits the tier; the three kernels take a k of 1 and skip a k of 0)
    SelArgs sa{nullptr, 0, 0, {n_cov, n_cov, n_link}, w->tbuf64, nullptr, {vs, ve, vg}, nt, ni, nr.out};
    HIP_TRY(c, launch_tiers(sa, lists, w->tcap, cnt, iv_qend ? 3 : 2, st));
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

int fslr_cluster_collapsed_segments(fslr_ctx* c, const int32_t* iv_qkey, const int32_t* iv_qend, int64_t n_intervals,
                                    int64_t* n_tokens_out) {
  return collapsed_run(c, iv_qkey, iv_qend, n_intervals, n_tokens_out, false);
}

int fslr_cluster_collapsed_segments_any(fslr_ctx* c, const int32_t* iv_qkey, const int32_t* iv_qend, int64_t n_intervals,
                                        int64_t* n_tokens_out) {
  return collapsed_run(c, iv_qkey, iv_qend, n_intervals, n_tokens_out, true);
}

int fslr_get_cluster_collapsed_segments(fslr_ctx* c, int32_t* n_cov, int32_t* n_link, int32_t* start, int32_t* end, int32_t* gap,
                                        int64_t token_capacity) {
  if (!c) return FSLR_ERR_INVALID;
  CollapsedWork* w = c->csw;
  if (!w || !w->have)
    return fail(c, FSLR_ERR_STATE, "fslr_get_cluster_collapsed_segments: fslr_cluster_collapsed_segments first");
  if (token_capacity < w->n_tokens)
    return fail(c, FSLR_ERR_INVALID, "fslr_get_cluster_collapsed_segments: token capacity " + std::to_string(token_capacity) +
                                         " < " + std::to_string(w->n_tokens) + " tokens");
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t nt = static_cast<size_t>(w->n_tokens);
  int32_t* out[3] = {start, end, gap};
  for (int k = 0; k < 3; ++k)
    if (out[k] && nt)
      HIP_TRY(c, hipMemcpyAsync(out[k], w->out + 3 * k * nt, 3 * nt * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (n_cov && nt) HIP_TRY(c, hipMemcpyAsync(n_cov, w->out + 9 * nt, nt * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (n_link && nt) HIP_TRY(c, hipMemcpyAsync(n_link, w->out + 10 * nt, nt * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FSLR_OK;
}

int fslr_cluster_collapsed_segments_timings(fslr_ctx* c, float* ms) {
  if (!c || !ms) return FSLR_ERR_INVALID;
  CollapsedWork* w = c->csw;
  if (!w || !w->timed)
    return fail(c, FSLR_ERR_STATE,
                "fslr_cluster_collapsed_segments_timings: no profiled fslr_cluster_collapsed_segments (fslr_set_profiling 1 or 2)");
  ms[0] = w->ms;
  return FSLR_OK;
}

}  // extern "C"
