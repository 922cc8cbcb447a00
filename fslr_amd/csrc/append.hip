// append.hip — fslr_append_reads: more reads for a resident set, on the device.
//
// The batch's columns go up as they are (m reads, mi intervals: the only H2D traffic), are validated and
// packed in scratch by upload.hip's kernels with the ranks based at n and the CSR offsets at ni, and nothing
// resident is written until every check has passed.  Then the batch's rows are copied behind the resident
// CSR and the two start-sorted data lists are merged (k_append_merge, a merge-path: the resident element
// first on equal starts) into a second set of data-order buffers, which is swapped in; one gather rewrites
// the data positions.  No global atomic decides where anything lands: the same bytes on every run, and the
// bytes fslr_set_reads gives for the concatenated CSR with the merged iv_data_pos.
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "fslr_hip.h"
#include "append.hpp"
#include "ctx.hpp"
#include "kernels.hpp"

using namespace fslr;

void fslr_append_free(fslr_ctx* c) {
  AppendWork* w = c->apw;
  if (!w) return;
  void* bufs[] = {w->cols, w->rmeta, w->rlen8, w->iv, w->inv, w->dch, w->drc, w->dgt, w->w64, w->alt_ch, w->alt_rec, w->alt_gate, w->maps, w->rl_out};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  if (w->ev_ok)
    for (hipEvent_t& e : w->ev) (void)hipEventDestroy(e);
  delete w;
  c->apw = nullptr;
}

namespace {

constexpr int kTile = FSLR_APPEND_TILE;

// Stable merge of the resident data list R (ni elements) and the batch's N (mi), both sorted by start
// (rec.x), the resident element first on equal starts.  A block takes output tiles of kTile elements: the
// split of each tile end on its diagonal by binary search (the first i with R[i].x > N[d - 1 - i].x), then
//   - a tile of one list alone is a straight copy (with m << n nearly every tile): 16-B records, 8-B gate
//     words and 4-B chromosomes, consecutive lanes on consecutive elements;
//   - a mixed tile stages its keys in LDS, ranks every element against the other list's run there, and
//     writes its outputs in order from the source index each output position recorded.
// newpos[i] (i < ni) = the merged position of resident data position i, newpos[ni + j] that of the batch's j.
// tag_n, tag_m: a resident record's tag `read << 6 | j` with read >= tag_n moves up by tag_m reads
// (fslr_append_reads_any: the resident further chunks behind the batch's first chunks; tag_m 0: today's bytes).
__global__ __launch_bounds__(256) void k_append_merge(const unsigned* __restrict__ rch, const int4* __restrict__ rrec,
                                                      const int2* __restrict__ rgate, int ni,
                                                      const unsigned* __restrict__ nch, const int4* __restrict__ nrec,
                                                      const int2* __restrict__ ngate, int mi,
                                                      unsigned* __restrict__ och, int4* __restrict__ orec,
                                                      int2* __restrict__ ogate, int* __restrict__ newpos,
                                                      int tag_n, int tag_m) {
  __shared__ int split[2];
  __shared__ int key[kTile];
  __shared__ int src[kTile];
  const long long total = static_cast<long long>(ni) + mi;
  const int tid = threadIdx.x;
  for (long long tile = blockIdx.x; tile * kTile < total; tile += gridDim.x) {
    const int d0 = static_cast<int>(tile * kTile);
    const int d1 = static_cast<int>(std::min<long long>(tile * kTile + kTile, total));
    if (tid < 2) {
      const int d = tid ? d1 : d0;
      int lo = std::max(0, d - mi), hi = std::min(d, ni);
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        FSLR_BOUND(mid, ni);
        FSLR_BOUND(d - 1 - mid, mi);
        if (rrec[mid].x <= nrec[d - 1 - mid].x) lo = mid + 1;
        else hi = mid;
      }
      split[tid] = lo;
    }
    __syncthreads();
    const int i0 = split[0], i1 = split[1];
    const int j0 = d0 - i0, j1 = d1 - i1;
    const int na = i1 - i0, nb = j1 - j0, len = d1 - d0;
    if (nb == 0) {
      for (int t = tid; t < len; t += blockDim.x) {
        FSLR_BOUND(i0 + t, ni);
        FSLR_BOUND(d0 + t, total);
        int4 rec = rrec[i0 + t];
        rec.w = anyidx::retag(rec.w, tag_n, tag_m);
        orec[d0 + t] = rec;
        ogate[d0 + t] = rgate[i0 + t];
        och[d0 + t] = rch[i0 + t];
        newpos[i0 + t] = d0 + t;
      }
    } else if (na == 0) {
      for (int t = tid; t < len; t += blockDim.x) {
        FSLR_BOUND(j0 + t, mi);
        FSLR_BOUND(d0 + t, total);
        orec[d0 + t] = nrec[j0 + t];
        ogate[d0 + t] = ngate[j0 + t];
        och[d0 + t] = nch[j0 + t];
        newpos[ni + j0 + t] = d0 + t;
      }
    } else {
      for (int t = tid; t < len; t += blockDim.x) {
        if (t < na) {
          FSLR_BOUND(i0 + t, ni);
          key[t] = rrec[i0 + t].x;
        } else {
          FSLR_BOUND(j0 + t - na, mi);
          key[t] = nrec[j0 + t - na].x;
        }
      }
      __syncthreads();
      for (int t = tid; t < len; t += blockDim.x) {
        const int k = key[t];
        int pos;
        if (t < na) {                      // + the batch's elements of this tile with a start < k
          int lo = na, hi = len;
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (key[mid] < k) lo = mid + 1;
            else hi = mid;
          }
          pos = t + (lo - na);
          newpos[i0 + t] = d0 + pos;
        } else {                           // + the resident elements of this tile with a start <= k
          int lo = 0, hi = na;
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (key[mid] <= k) lo = mid + 1;
            else hi = mid;
          }
          pos = (t - na) + lo;
          FSLR_BOUND(ni + j0 + t - na, total);
          newpos[ni + j0 + t - na] = d0 + pos;
        }
        FSLR_BOUND(pos, len);
        src[pos] = t;
      }
      __syncthreads();
      for (int p = tid; p < len; p += blockDim.x) {
        const int t = src[p];
        FSLR_BOUND(t, len);
        FSLR_BOUND(d0 + p, total);
        if (t < na) {
          FSLR_BOUND(i0 + t, ni);
          int4 rec = rrec[i0 + t];
          rec.w = anyidx::retag(rec.w, tag_n, tag_m);
          orec[d0 + p] = rec;
          ogate[d0 + p] = rgate[i0 + t];
          och[d0 + p] = rch[i0 + t];
        } else {
          FSLR_BOUND(j0 + t - na, mi);
          orec[d0 + p] = nrec[j0 + t - na];
          ogate[d0 + p] = ngate[j0 + t - na];
          och[d0 + p] = nch[j0 + t - na];
        }
      }
    }
    __syncthreads();                       // split, key and src serve the block's next tile
  }
}

// data_pos (CSR order) after the merge: a resident interval follows its old data position, a new one the
// position in its own list
__global__ void k_append_datapos(int* __restrict__ data_pos, int ni, const int* __restrict__ dp_new, int mi,
                                 const int* __restrict__ newpos) {
  const long long total = static_cast<long long>(ni) + mi;
  for (long long k = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x; k < total;
       k += static_cast<long long>(gridDim.x) * blockDim.x) {
    int at;
    if (k < ni) {
      at = data_pos[k];
      FSLR_BOUND(at, ni);
    } else {
      const int e = dp_new[k - ni];
      FSLR_BOUND(e, mi);
      at = ni + e;
    }
    data_pos[k] = newpos[at];
  }
}

int ensure_batch(fslr_ctx* c, AppendWork* w, int64_t m, int64_t mi, int n_chroms) {
  int rc;
  const int64_t cols = 3 * m + 1 + 5 * mi;
  if (cols > w->cols_cap) {
    w->cols_cap = 0;                             // (a failed growth leaves no buffer behind its capacity)
    if ((rc = dalloc(c, &w->cols, static_cast<size_t>(cols + cols / 4)))) return rc;
    w->cols_cap = cols + cols / 4;
  }
  if (m > w->m_cap) {
    w->m_cap = 0;
    if ((rc = dalloc(c, &w->rmeta, static_cast<size_t>(m + m / 4))) || (rc = dalloc(c, &w->rlen8, static_cast<size_t>(m + m / 4))))
      return rc;
    w->m_cap = m + m / 4;
  }
  if (mi > w->mi_cap) {
    w->mi_cap = 0;
    const size_t cap = static_cast<size_t>(mi + mi / 4);
    if ((rc = dalloc(c, &w->iv, cap)) || (rc = dalloc(c, &w->inv, cap)) || (rc = dalloc(c, &w->dch, cap)) ||
        (rc = dalloc(c, &w->drc, cap)) || (rc = dalloc(c, &w->dgt, cap)))
      return rc;
    w->mi_cap = static_cast<int64_t>(cap);
  }
  if (n_chroms + 2 > w->w64_cap) {
    w->w64_cap = 0;
    if ((rc = dalloc(c, &w->w64, static_cast<size_t>(n_chroms + 2)))) return rc;
    w->w64_cap = n_chroms + 2;
  }
  return FSLR_OK;
}

int broken(fslr_ctx* c, int rc) { return reads_broken(c, rc); }

#define APP_TRY(ctx, expr)                                                                                    \
  do {                                                                                                        \
    hipError_t e_ = (expr);                                                                                   \
    if (e_ != hipSuccess)                                                                                     \
      return broken((ctx), fail((ctx), FSLR_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)));     \
  } while (0)

}  // namespace

// once memory is there nothing but the device can fail; what is then half written is not a set of reads
int fslr::reads_broken(fslr_ctx* c, int rc) {
  c->reads_set = false;
  c->index_built = false;
  return rc;
}

// the states neither append takes, each named; virt: virtual reads are fine (fslr_append_reads_any)
int fslr::append_state(fslr_ctx* c, const std::string& who, bool virt) {
  if (!c->reads_set) return fail(c, FSLR_ERR_STATE, who + ": no reads set (fslr_set_reads first)");
  if (c->rows_set)
    return fail(c, FSLR_ERR_STATE, who + ": the reads were made from rows (fslr_set_reads_rows), which it does not extend");
  if (!virt && (c->lg_set || !c->lg_perm.empty()))
    return fail(c, FSLR_ERR_STATE, who + ": the context holds virtual reads (fslr_set_reads_any / fslr_set_long_reads: "
                                   "reads of more than " + std::to_string(FSLR_MAX_L) + " intervals), which it does not extend");
  if (virt && c->lg_set && c->lg_perm.empty())
    return fail(c, FSLR_ERR_STATE, who + ": the virtual reads were made by the caller (fslr_set_long_reads), not by "
                                   "fslr_set_reads_any: their real CSR is not known here");
  if (!c->have_data_pos)
    return fail(c, FSLR_ERR_STATE, who + ": the reads were set without iv_data_pos (no start-sorted data list to merge into)");
  if (c->n_shards > 1) return fail(c, FSLR_ERR_STATE, who + ": n_shards > 1 (fslr_set_shard): multi-GPU contexts do not append");
  if (c->filter_active || c->pf_on)
    return fail(c, FSLR_ERR_STATE, who + ": a chromosome or position filter is active");
  return FSLR_OK;
}

// plan null: fslr_append_reads.  Otherwise r is the batch's virtual CSR (plan->s.m first chunks, then plan->s.e
// further chunks) and the resident set is relocated around it (any.hip).
int fslr::append_core(fslr_ctx* c, const fslr_reads* r, const AnyPlan* plan, const char* who_c) {
  const std::string who(who_c);
  if (!c || !r) return FSLR_ERR_INVALID;
  if (int rc = append_state(c, who, plan != nullptr)) return rc;
  const int64_t n = c->n, ni = c->ni, m = r->n_reads, mi = r->n_intervals;
  if (m < 0 || mi < 0 || n + m >= FSLR_MAX_READS || ni + mi >= (int64_t(1) << 31) - 1)
    return fail(c, FSLR_ERR_INVALID, "read / interval count out of range");
  if (r->n_chroms < 1 || r->n_chroms >= (1 << 24)) return fail(c, FSLR_ERR_INVALID, "n_chroms out of range");
  if (r->n_chroms < c->n_chroms) return fail(c, FSLR_ERR_INVALID, who + ": n_chroms below the resident value");
  if (!r->read_off || !r->read_qlen2 || !r->read_nal || !r->iv_chrom || !r->iv_start || !r->iv_end || !r->iv_thr)
    return fail(c, FSLR_ERR_INVALID, "null array");
  if (!r->iv_data_pos) return fail(c, FSLR_ERR_INVALID, who + ": iv_data_pos is required");
  if (r->read_off[0] != 0 || r->read_off[m] != mi) return fail(c, FSLR_ERR_INVALID, "read_off does not span intervals");
  if (m == 0) return FSLR_OK;                    // nothing to add: no generation moves
  HIP_TRY(c, hipSetDevice(c->device));
  if (!c->apw) c->apw = new AppendWork();
  AppendWork* w = c->apw;
  w->timed = false;
  const bool prof = c->profiling;
  if (prof && !w->ev_ok) {
    for (hipEvent_t& e : w->ev) HIP_TRY(c, hipEventCreate(&e));
    w->ev_ok = true;
  }
  if (int rc = ensure_batch(c, w, m, mi, r->n_chroms)) return rc;
  const int64_t n_real = plan ? plan->s.n : n, m_real = plan ? plan->s.m : m;
  if (plan) {
    const int64_t maps = 2 * m + 2 * m_real;
    if (maps > w->maps_cap) {
      w->maps_cap = 0;
      if (int rc = dalloc(c, &w->maps, static_cast<size_t>(maps + maps / 4))) return rc;
      w->maps_cap = maps + maps / 4;
    }
  }
  hipStream_t st = c->stream;
  // ---- the batch: up as it is, validated and packed in scratch; nothing resident is written ----------
  int* d_off = w->cols;
  int* d_q2 = d_off + m + 1;
  int* d_nal = d_q2 + m;
  int* d_ch = d_nal + m;
  int* d_st = d_ch + mi;
  int* d_en = d_st + mi;
  int* d_th = d_en + mi;
  int* d_dp = d_th + mi;
  unsigned long long* d_cnt = w->w64;
  unsigned long long* d_err = w->w64 + r->n_chroms;
  const size_t mb = static_cast<size_t>(m) * sizeof(int), ib = static_cast<size_t>(mi) * sizeof(int);
  if (prof) HIP_TRY(c, hipEventRecord(w->ev[0], st));
  HIP_TRY(c, hipMemsetAsync(d_cnt, 0, static_cast<size_t>(r->n_chroms) * sizeof(unsigned long long), st));
  HIP_TRY(c, hipMemsetAsync(d_err, 0xff, 2 * sizeof(unsigned long long), st));
  HIP_TRY(c, hipMemcpyAsync(d_off, r->read_off, mb + sizeof(int), hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_q2, r->read_qlen2, mb, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_nal, r->read_nal, mb, hipMemcpyHostToDevice, st));
  if (mi) {
    HIP_TRY(c, hipMemcpyAsync(d_ch, r->iv_chrom, ib, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(d_st, r->iv_start, ib, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(d_en, r->iv_end, ib, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(d_th, r->iv_thr, ib, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(d_dp, r->iv_data_pos, ib, hipMemcpyHostToDevice, st));
  }
  int* d_bvreal = w->maps;                       // (plan) vreal [m] | vbase [m] | rlen [m_real] | off2 [m_real]
  int* d_bvbase = d_bvreal + m;
  int* d_brlen = d_bvbase + m;
  int* d_boff2 = d_brlen + m_real;
  if (plan) {
    HIP_TRY(c, hipMemcpyAsync(d_bvreal, plan->b_vreal, mb, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(d_bvbase, plan->b_vbase, mb, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(d_brlen, plan->b_rlen, static_cast<size_t>(m_real) * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(d_boff2, plan->b_off2, static_cast<size_t>(m_real) * sizeof(int), hipMemcpyHostToDevice, st));
  }
  if (prof) HIP_TRY(c, hipEventRecord(w->ev[1], st));
  // the reads' own checks on the host, in index order (fslr_set_reads' codes: 3 length, 4 n_alignments, 5 qlen2)
  int bad = 0;
  for (int64_t i = 0; i < m && !bad; ++i) {
    const int len = r->read_off[i + 1] - r->read_off[i];
    if (len < 1 || len > FSLR_MAX_L) bad = 3;
    else if (r->read_nal[i] < 0 || r->read_nal[i] >= (1 << 24)) bad = 4;
    else if (r->read_qlen2[i] < 0) bad = 5;
  }
  UploadArgs ua{};
  ua.off = d_off;
  ua.qlen2 = d_q2;
  ua.nal = d_nal;
  ua.chrom = d_ch;
  ua.start = d_st;
  ua.end = d_en;
  ua.thr = d_th;
  ua.dp = d_dp;
  ua.n = static_cast<int>(m);
  ua.ni = static_cast<int>(mi);
  ua.n_chroms = r->n_chroms;
  ua.reads_ok = bad == 0;
  ua.rank_base = static_cast<int>(n);
  ua.off_base = static_cast<int>(ni);
  if (plan) {                                    // first chunks behind the resident ones, further chunks at the end
    ua.rank_base = plan->s.n;
    ua.off_base = plan->s.o1;
    ua.split = plan->s.m;
    ua.rank_base2 = plan->s.V;
    ua.off_base2 = plan->s.ni;
  }
  ua.iv = w->iv;
  ua.rmeta = w->rmeta;
  ua.rlen8 = w->rlen8;
  ua.dch = w->dch;
  ua.drc = w->drc;
  ua.dgt = w->dgt;
  ua.inv = w->inv;
  ua.chrom_cnt = d_cnt;
  ua.err = d_err;
  HIP_TRY(c, launch_upload_pack(ua, st));
  if (prof) HIP_TRY(c, hipEventRecord(w->ev[2], st));
  int tmode = 0, any_zero = 0;
  for (int64_t k = 0; k < mi; ++k) {
    any_zero |= r->iv_thr[k] == FSLR_THR_ZERO_ALN;
    tmode |= r->iv_thr[k] != FSLR_THR_ZERO_ALN && r->iv_thr[k] < 1;
  }
  std::vector<int64_t> batch_counts(static_cast<size_t>(r->n_chroms), 0);
  unsigned long long err[2] = {0, 0};
  HIP_TRY(c, hipMemcpyAsync(batch_counts.data(), d_cnt, batch_counts.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(err, d_err, sizeof(err), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  if (err[0] != ~0ull) {
    if ((err[0] & 7) == kUpErrChrom) return fail(c, FSLR_ERR_INVALID, "chrom id out of range");
    return fail(c, FSLR_ERR_INVALID, "interval coordinates out of [0, 2^30)");
  }
  if (bad == 3) return fail(c, FSLR_ERR_INVALID, "every read needs 1.." + std::to_string(FSLR_MAX_L) + " intervals");
  if (bad == 4) return fail(c, FSLR_ERR_INVALID, "n_alignments outside [0, 2^24)");
  if (bad == 5) return fail(c, FSLR_ERR_INVALID, "qlen2 < 0");
  if (err[1] != ~0ull) return fail(c, FSLR_ERR_INVALID, "iv_data_pos is not a start-sorted permutation");
  // ---- room: the merge output first (a failure here leaves the context as it was) --------------------
  const int64_t need_n = n + m, need_ni = ni + mi;
  const int64_t cap_n = need_n > c->cap_n ? std::max(need_n, c->cap_n + c->cap_n / 2) : c->cap_n;
  const int64_t cap_ni = need_ni > c->cap_ni ? std::max(need_ni, c->cap_ni + c->cap_ni / 2) : c->cap_ni;
  const int64_t old_cap_ni = c->cap_ni;
  if (w->alt_cap < cap_ni) {
    w->alt_cap = 0;
    int rc;
    const size_t cap = static_cast<size_t>(cap_ni);
    if ((rc = dalloc(c, &w->alt_ch, cap)) || (rc = dalloc(c, &w->alt_rec, cap)) || (rc = dalloc(c, &w->alt_gate, cap))) return rc;
    w->alt_cap = cap_ni;
  }
  // ... and every buffer that has to grow, allocated before any is freed (the same holds for a failure here)
  if (int rc = grow_capacity_keep(c, cap_n, cap_ni, r->n_chroms)) return rc;
  // (plan) the relocated read lengths and the new virtual-read maps, beside the old ones until they are written
  struct NewMaps {                               // freed on every way out but the one that installs them
    int* lg[4] = {nullptr, nullptr, nullptr, nullptr};       // vreal, vbase [need_n] | rlen, off2 [n_real + m_real]
    int* umax = nullptr;
    ~NewMaps() {
      for (int* p : lg)
        if (p) (void)hipFree(p);
      if (umax) (void)hipFree(umax);
    }
  } fresh;
  int** lg_new = fresh.lg;
  int*& umax_new = fresh.umax;
  if (plan) {
    if (need_n > w->rl_cap) {
      w->rl_cap = 0;
      if (int rc = dalloc(c, &w->rl_out, static_cast<size_t>(cap_n))) return rc;
      w->rl_cap = cap_n;
    }
    const size_t cnt[4] = {static_cast<size_t>(need_n), static_cast<size_t>(need_n), static_cast<size_t>(n_real + m_real),
                           static_cast<size_t>(n_real + m_real)};
    for (int k = 0; k < 4; ++k)
      if (hipMalloc(reinterpret_cast<void**>(&lg_new[k]), cnt[k] * sizeof(int)) != hipSuccess) {
        lg_new[k] = nullptr;
        return fail(c, FSLR_ERR_NOMEM, who + ": hipMalloc of the virtual-read maps");
      }
    if (!c->lg_set) {                            // a plain context turns virtual: the placeholder cutoffs of a fresh upload
      if (hipMalloc(reinterpret_cast<void**>(&umax_new), static_cast<size_t>(plan->max_len) * sizeof(int)) != hipSuccess) {
        umax_new = nullptr;
        return fail(c, FSLR_ERR_NOMEM, who + ": hipMalloc of the cutoff table");
      }
    }
    if (!c->lg_cnt)
      if (int rc = dalloc(c, &c->lg_cnt, 4)) return rc;
  }
  // from here the index scratch is reused and the resident buffers are written
  c->index_built = false;
  c->hooked = false;
  if (prof) APP_TRY(c, hipEventRecord(w->ev[3], st));
  if (!plan) {
    APP_TRY(c, hipMemcpyAsync(c->rmeta + n, w->rmeta, static_cast<size_t>(m) * sizeof(int4), hipMemcpyDeviceToDevice, st));
    APP_TRY(c, hipMemcpyAsync(c->rlen8 + n, w->rlen8, static_cast<size_t>(m), hipMemcpyDeviceToDevice, st));
    if (mi) APP_TRY(c, hipMemcpyAsync(c->iv + ni, w->iv, static_cast<size_t>(mi) * sizeof(int4), hipMemcpyDeviceToDevice, st));
  }
  int* newpos = c->vals;                         // [ni + mi] index-build scratch (the index is rebuilt anyway)
  const int64_t tiles = (need_ni + kTile - 1) / kTile;
  if (need_ni) {
    k_append_merge<<<static_cast<int>(std::min<int64_t>(tiles, 256 * 16)), 256, 0, st>>>(
        c->dchrom, c->drec, c->dgate, static_cast<int>(ni), w->dch, w->drc, w->dgt, static_cast<int>(mi), w->alt_ch,
        w->alt_rec, w->alt_gate, newpos, plan ? plan->s.n : 0x7fffffff, plan ? plan->s.m : 0);
    if (!plan)
      k_append_datapos<<<grid_for(need_ni), 256, 0, st>>>(c->data_pos, static_cast<int>(ni), d_dp, static_cast<int>(mi), newpos);
    APP_TRY(c, hipGetLastError());
  }
  if (plan) {
    // the rows, the reads and the maps of the four groups (any_idx.hpp) into index-build scratch and the new
    // maps: never in place, a resident chunk row's destination is another's source
    AnyReloc a{};
    a.s = plan->s;
    a.rmeta = c->rmeta, a.rlen8 = c->rlen8, a.iv = c->iv, a.data_pos = c->data_pos;
    if (c->lg_set) a.vreal = c->lg_vreal, a.vbase = c->lg_vbase, a.rlen = c->lg_rlen, a.off2 = c->lg_off2;
    a.b_rmeta = w->rmeta, a.b_rlen8 = w->rlen8, a.b_iv = w->iv, a.b_dp = d_dp;
    a.b_vreal = d_bvreal, a.b_vbase = d_bvbase, a.b_rlen = d_brlen, a.b_off2 = d_boff2;
    a.newpos = newpos;
    a.rmeta_out = c->lbounds, a.rlen8_out = w->rl_out, a.iv_out = c->idx4, a.dp_out = c->vals2;
    a.vreal_out = lg_new[0], a.vbase_out = lg_new[1], a.rlen_out = lg_new[2], a.off2_out = lg_new[3];
    c->lb_gen = -1;                              // the length gate's ranges belonged to the old reads anyway
    hipError_t e = launch_any_relocate(a, st);
    if (e == hipSuccess) e = hipMemcpyAsync(c->rlen8, w->rl_out, static_cast<size_t>(need_n), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess && umax_new) e = hipMemsetAsync(umax_new, 0, static_cast<size_t>(plan->max_len) * sizeof(int), st);
    if (e != hipSuccess) {
      return broken(c, fail(c, FSLR_ERR_HIP, who + ": relocation: " + hipGetErrorString(e)));
    }
  }
  if (prof) APP_TRY(c, hipEventRecord(w->ev[4], st));
  // chromosome ranges of the (chrom, start)-sorted index from the summed counts, as fslr_set_reads makes them
  std::vector<int64_t> counts(c->chrom_counts);
  counts.resize(static_cast<size_t>(r->n_chroms), 0);
  std::vector<int2> cr(counts.size(), make_int2(0, 0));
  int64_t acc = 0;
  for (size_t ch = 0; ch < counts.size(); ++ch) {
    counts[ch] += batch_counts[ch];
    cr[ch] = make_int2(static_cast<int>(acc), static_cast<int>(acc + counts[ch]));
    acc += counts[ch];
  }
  APP_TRY(c, hipMemcpyAsync(c->crange, cr.data(), cr.size() * sizeof(int2), hipMemcpyHostToDevice, st));
  APP_TRY(c, hipStreamSynchronize(st));
  std::swap(c->dchrom, w->alt_ch);
  std::swap(c->drec, w->alt_rec);
  std::swap(c->dgate, w->alt_gate);
  w->alt_cap = old_cap_ni;                       // what the context's buffers were allocated for, at least
  if (!plan) {
    c->aln_zero_host.resize(static_cast<size_t>(need_ni), 0);
    for (int64_t k = 0; k < mi; ++k) c->aln_zero_host[static_cast<size_t>(ni + k)] = r->iv_thr[k] == FSLR_THR_ZERO_ALN;
  } else {
    std::swap(c->rmeta, c->lbounds);
    std::swap(c->iv, c->idx4);
    std::swap(c->data_pos, c->vals2);
    int** slot[4] = {&c->lg_vreal, &c->lg_vbase, &c->lg_rlen, &c->lg_off2};
    for (int k = 0; k < 4; ++k) {
      if (*slot[k]) (void)hipFree(*slot[k]);
      *slot[k] = lg_new[k];
      lg_new[k] = nullptr;
    }
    if (umax_new) {
      if (c->lg_umax) (void)hipFree(c->lg_umax);
      c->lg_umax = umax_new;
      umax_new = nullptr;
      c->lg_n_umax = plan->max_len;
    }
    // the host's marks and the virtual -> real interval map, in the rows' four groups
    const anyidx::Shape& s = plan->s;
    std::vector<unsigned char> zero(static_cast<size_t>(need_ni));
    std::vector<int> perm(static_cast<size_t>(need_ni));
    const bool ident = c->lg_perm.empty();
    for (int64_t k = 0; k < need_ni; ++k) {
      const int src = anyidx::row_source(static_cast<int>(k), s);
      if (src >= 0) {
        zero[static_cast<size_t>(k)] = c->aln_zero_host[static_cast<size_t>(src)];
        perm[static_cast<size_t>(k)] = ident ? src : c->lg_perm[static_cast<size_t>(src)];
      } else {
        zero[static_cast<size_t>(k)] = r->iv_thr[~src] == FSLR_THR_ZERO_ALN;
        perm[static_cast<size_t>(k)] = static_cast<int>(ni) + plan->b_perm[~src];
      }
    }
    c->aln_zero_host.swap(zero);
    c->lg_perm.swap(perm);
    c->lg_n_real = n_real + m_real;
    c->lg_max_len = plan->max_len;
    c->lg_set = true;
    c->lg_n_edges = 0;
  }
  c->n = need_n;
  c->ni = need_ni;
  c->ni_idx = need_ni;
  c->chrom_counts.swap(counts);
  c->n_chroms = r->n_chroms;
  c->thr_mode |= tmode;
  c->any_zero_aln = c->any_zero_aln || any_zero;
  ++c->reads_gen;
  c->pf_set = c->pf_on = false;
  c->edges_global = false;
  c->cap_gmode = false;
  ++c->input_gen;
  if (prof) {
    for (int t = 0; t < 2; ++t) HIP_TRY(c, hipEventElapsedTime(&w->ms[t], w->ev[t], w->ev[t + 1]));
    HIP_TRY(c, hipEventElapsedTime(&w->ms[2], w->ev[3], w->ev[4]));
    HIP_TRY(c, hipEventElapsedTime(&w->ms[3], w->ev[0], w->ev[4]));
    w->timed = true;
  }
  return FSLR_OK;
}

extern "C" {

int fslr_append_reads(fslr_ctx* c, const fslr_reads* r) { return append_core(c, r, nullptr, "fslr_append_reads"); }

int fslr_append_timings(fslr_ctx* c, float* ms) {
  if (!c || !ms) return FSLR_ERR_INVALID;
  AppendWork* w = c->apw;
  if (!w || !w->timed)
    return fail(c, FSLR_ERR_STATE, "fslr_append_timings: no profiled fslr_append_reads / fslr_append_reads_any (fslr_set_profiling 1 or 2)");
  for (int t = 0; t < 4; ++t) ms[t] = w->ms[t];
  return FSLR_OK;
}

}  // extern "C"
