// any.hip — fslr_append_reads_any / fslr_remove_reads_any: the append and the removal of reads of any length on
// a resident set that may hold virtual reads.
//
// A read of more than FSLR_MAX_L intervals lives on the device as FSLR_MAX_L-interval virtual reads (long.hip):
// the real reads' first chunks first, every further chunk behind them, in rank and in CSR rows alike.
//   Append.  The batch is split into virtual reads on the host (O(batch)) and goes through fslr_append_reads'
//            route (append.hip: upload, validate, pack, merge) with two differences: upload.hip numbers the
//            batch's further chunks behind the resident ones, and the merge moves the tags of the resident
//            further chunks up by the batch's read count.  Then the resident set is relocated around the
//            batch here: k_any_reloc_reads (rmeta, rlen8, vreal, vbase, rlen, off2) and k_any_reloc_rows (iv,
//            data_pos), one thread per OUTPUT element, each reading where any_idx.hpp says it comes from.
//   Remove.  A virtual read stays iff its real read does, so the compaction is fslr_remove_reads' over the
//            virtual reads (remove.hip); k_any_rm_maps compacts the maps through its rank map and k_any_off2
//            finds every surviving long read's first further chunk again.
// Every kernel writes buffers none of its inputs live in (index-build scratch and freshly allocated maps, swapped
// in afterwards), waits on no other block, loops over bounds that are arguments, and places nothing by an atomic:
// the same bytes on every run, the bytes fslr_set_reads_any gives for the union / the survivors.
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "fslr_hip.h"
#include "append.hpp"
#include "ctx.hpp"
#include "kernels.hpp"

using namespace fslr;

namespace {

// per new virtual rank u: the packed read, its length and its place in its real read; per new real rank (the
// first n + m of the same index space): its length and where its intervals beyond FSLR_MAX_L begin
__global__ __launch_bounds__(256) void k_any_reloc_reads(const AnyReloc a) {
  const anyidx::Shape s = a.s;
  const long long total = static_cast<long long>(s.V) + s.m + s.e;
  for (long long u = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x; u < total;
       u += static_cast<long long>(gridDim.x) * blockDim.x) {
    const int src = anyidx::rank_source(static_cast<int>(u), s);
    if (src >= 0) {
      FSLR_BOUND(src, s.V);
      int4 m4 = a.rmeta[src];
      FSLR_BOUND(m4.x, s.ni);
      m4.x = anyidx::new_row(m4.x, s.o1, s.mi1);
      a.rmeta_out[u] = m4;
      a.rlen8_out[u] = a.rlen8[src];
      a.vreal_out[u] = a.vreal ? a.vreal[src] : src;
      a.vbase_out[u] = a.vbase ? a.vbase[src] : 0;
    } else {
      const int b = ~src;
      FSLR_BOUND(b, s.m + s.e);
      a.rmeta_out[u] = a.b_rmeta[b];
      a.rlen8_out[u] = a.b_rlen8[b];
      FSLR_BOUND(a.b_vreal[b], s.m);
      a.vreal_out[u] = s.n + a.b_vreal[b];
      a.vbase_out[u] = a.b_vbase[b];
    }
    if (u < s.n) {
      const int L = a.rlen ? a.rlen[u] : a.rlen8[u];
      a.rlen_out[u] = L;
      a.off2_out[u] = (a.off2 && L > FSLR_MAX_L) ? anyidx::off2_resident(a.off2[u], s.mi1) : 0;
    } else if (u < s.n + s.m) {
      a.rlen_out[u] = a.b_rlen[u - s.n];
      a.off2_out[u] = a.b_off2[u - s.n];
    }
  }
}

// per new CSR row k: the interval and its position in the merged data list
__global__ __launch_bounds__(256) void k_any_reloc_rows(const AnyReloc a) {
  const anyidx::Shape s = a.s;
  const long long total = static_cast<long long>(s.ni) + s.mi;
  for (long long k = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x; k < total;
       k += static_cast<long long>(gridDim.x) * blockDim.x) {
    const int src = anyidx::row_source(static_cast<int>(k), s);
    int at;
    if (src >= 0) {
      FSLR_BOUND(src, s.ni);
      a.iv_out[k] = a.iv[src];
      at = a.data_pos[src];
      FSLR_BOUND(at, s.ni);
    } else {
      const int b = ~src;
      FSLR_BOUND(b, s.mi);
      a.iv_out[k] = a.b_iv[b];
      const int e = a.b_dp[b];
      FSLR_BOUND(e, s.mi);
      at = s.ni + e;
    }
    const int p = a.newpos[at];
    FSLR_BOUND(p, total);
    a.dp_out[k] = p;
  }
}

// the maps of the surviving virtual reads at their new ranks.  new_rank is the virtual rank map of the
// compaction; a real read's new rank is its first chunk's (the first chunks precede the others before and after).
__global__ __launch_bounds__(256) void k_any_rm_maps(const int* __restrict__ vreal, const int* __restrict__ vbase,
                                                     const int* __restrict__ rlen, const int* __restrict__ new_rank,
                                                     int V, int n, int V_new, int n_new, int* __restrict__ vreal_out,
                                                     int* __restrict__ vbase_out, int* __restrict__ rlen_out,
                                                     int* __restrict__ off2_out) {
  for (long long v = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x; v < V;
       v += static_cast<long long>(gridDim.x) * blockDim.x) {
    const int nv = new_rank[v];
    if (nv < 0) continue;
    FSLR_BOUND(nv, V_new);
    const int r = vreal[v];
    FSLR_BOUND(r, n);
    const int nr = new_rank[r];
    FSLR_BOUND(nr, n_new);
    vreal_out[nv] = nr;
    vbase_out[nv] = vbase[v];
    if (v < n) {
      rlen_out[nv] = rlen[v];
      off2_out[nv] = 0;
    }
  }
}

// the CSR offset of each long read's first further chunk (what long.hip's k_long_off2 gives a fresh upload)
__global__ __launch_bounds__(256) void k_any_off2(const int4* __restrict__ rmeta, const int* __restrict__ vreal,
                                                  const int* __restrict__ vbase, int n, int V, int* __restrict__ off2) {
  for (long long v = n + blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x; v < V;
       v += static_cast<long long>(gridDim.x) * blockDim.x)
    if (vbase[v] == FSLR_MAX_L) {
      FSLR_BOUND(vreal[v], n);
      off2[vreal[v]] = rmeta[v].x;
    }
}

// the resident real reads' lengths on the host: kept from the last _any call, else read back once (4 B per real
// read of a virtual context, 1 B per read of a plain one)
int host_rlen(fslr_ctx* c, AppendWork* w) {
  if (w->rlen_ok && w->rlen_gen == c->reads_gen) return FSLR_OK;
  w->rlen_ok = false;
  HIP_TRY(c, hipSetDevice(c->device));
  if (c->lg_set) {
    w->rlen_host.resize(static_cast<size_t>(c->lg_n_real));
    if (c->lg_n_real)
      HIP_TRY(c, hipMemcpyAsync(w->rlen_host.data(), c->lg_rlen, w->rlen_host.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  } else {
    std::vector<unsigned char> l8(static_cast<size_t>(c->n));
    if (c->n) HIP_TRY(c, hipMemcpyAsync(l8.data(), c->rlen8, l8.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    w->rlen_host.assign(l8.begin(), l8.end());
  }
  w->rlen_gen = c->reads_gen;
  w->rlen_ok = true;
  return FSLR_OK;
}

}  // namespace

hipError_t fslr::launch_any_relocate(const AnyReloc& a, hipStream_t s) {
  const long long reads = static_cast<long long>(a.s.V) + a.s.m + a.s.e, rows = static_cast<long long>(a.s.ni) + a.s.mi;
  if (reads > 0) k_any_reloc_reads<<<grid_for(reads), 256, 0, s>>>(a);
  if (rows > 0) k_any_reloc_rows<<<grid_for(rows), 256, 0, s>>>(a);
  return hipGetLastError();
}

extern "C" {

int fslr_append_reads_any(fslr_ctx* c, const fslr_reads* r) {
  const std::string who = "fslr_append_reads_any";
  if (!c || !r) return FSLR_ERR_INVALID;
  if (int rc = append_state(c, who, true)) return rc;
  const int64_t m = r->n_reads, mi = r->n_intervals;
  if (m < 0 || mi < 0 || mi >= (int64_t(1) << 31) - 1) return fail(c, FSLR_ERR_INVALID, "read / interval count out of range");
  if (!r->read_off || !r->read_qlen2 || !r->read_nal || !r->iv_chrom || !r->iv_start || !r->iv_end || !r->iv_thr)
    return fail(c, FSLR_ERR_INVALID, "null array");
  if (!r->iv_data_pos) return fail(c, FSLR_ERR_INVALID, who + ": iv_data_pos is required");
  if (r->read_off[0] != 0 || r->read_off[m] != mi) return fail(c, FSLR_ERR_INVALID, "read_off does not span intervals");
  bool any_long = false;
  int64_t e = 0, mi1 = 0;
  int batch_max = 0;
  for (int64_t i = 0; i < m; ++i) {
    const int64_t L = static_cast<int64_t>(r->read_off[i + 1]) - r->read_off[i];
    if (L > FSLR_MAX_ANY_L)
      return fail(c, FSLR_ERR_INVALID, who + ": read " + std::to_string(i) + " of the batch has " + std::to_string(L) +
                                           " intervals, more than FSLR_MAX_ANY_L = " + std::to_string(FSLR_MAX_ANY_L));
    if (L < 1) return fail(c, FSLR_ERR_INVALID, "every read needs 1.." + std::to_string(FSLR_MAX_ANY_L) + " intervals");
    any_long |= L > FSLR_MAX_L;
    e += anyidx::extra_chunks(static_cast<int>(L));
    mi1 += std::min<int64_t>(L, FSLR_MAX_L);
    batch_max = std::max(batch_max, static_cast<int>(L));
  }
  // nothing virtual on either side: fslr_append_reads' own path and bytes
  if (!c->lg_set && !any_long) return append_core(c, r, nullptr, who.c_str());
  if (m == 0) return FSLR_OK;
  if (!c->apw) c->apw = new AppendWork();
  AppendWork* w = c->apw;
  if (int rc = host_rlen(c, w)) return rc;
  AnyPlan plan{};
  anyidx::Shape& s = plan.s;
  const int64_t n_real = c->lg_set ? c->lg_n_real : c->n;
  int64_t o1 = 0;
  int res_max = 0;
  for (int L : w->rlen_host) {
    o1 += std::min(L, FSLR_MAX_L);
    res_max = std::max(res_max, L);
  }
  if (c->n + m + e >= FSLR_MAX_READS) return fail(c, FSLR_ERR_INVALID, "too many reads after the split into chunks");
  if (c->ni + mi >= (int64_t(1) << 31) - 1) return fail(c, FSLR_ERR_INVALID, "read / interval count out of range");
  s.n = static_cast<int>(n_real), s.V = static_cast<int>(c->n), s.o1 = static_cast<int>(o1), s.ni = static_cast<int>(c->ni);
  s.m = static_cast<int>(m), s.e = static_cast<int>(e), s.mi1 = static_cast<int>(mi1), s.mi = static_cast<int>(mi);
  // the batch's virtual CSR, as fslr_set_reads_any lays one out: the m first chunks, then the further chunks
  const int64_t nb = m + e;
  std::vector<int32_t> voff(static_cast<size_t>(nb) + 1), vreal(static_cast<size_t>(nb)), vbase(static_cast<size_t>(nb));
  std::vector<int32_t> vq(static_cast<size_t>(nb)), vn(static_cast<size_t>(nb)), rlen(static_cast<size_t>(m)), off2(static_cast<size_t>(m));
  std::vector<int> perm(static_cast<size_t>(mi));
  int64_t v = m, before = 0;
  for (int64_t i = 0; i < m; ++i) {
    const int L = r->read_off[i + 1] - r->read_off[i];
    rlen[i] = L;
    vreal[i] = static_cast<int32_t>(i);
    vbase[i] = 0;
    voff[i + 1] = std::min(L, FSLR_MAX_L);
    off2[i] = L > FSLR_MAX_L ? anyidx::off2_batch(s.ni, s.mi1, static_cast<int>(before)) : 0;
    for (int k = 1; k <= anyidx::extra_chunks(L); ++k, ++v) {
      vreal[v] = static_cast<int32_t>(i);
      vbase[v] = k * FSLR_MAX_L;
      voff[v + 1] = std::min(L - k * FSLR_MAX_L, FSLR_MAX_L);
    }
    before += std::max(L - FSLR_MAX_L, 0);
  }
  voff[0] = 0;
  for (int64_t u = 0; u < nb; ++u) voff[u + 1] += voff[u];
  for (int64_t u = 0; u < nb; ++u) {
    const int64_t src = static_cast<int64_t>(r->read_off[vreal[u]]) + vbase[u];
    for (int64_t k = voff[u]; k < voff[u + 1]; ++k) perm[k] = static_cast<int>(src + (k - voff[u]));
    vq[u] = r->read_qlen2[vreal[u]];
    vn[u] = r->read_nal[vreal[u]];
  }
  auto take = [&](const int32_t* a) {
    std::vector<int32_t> out(static_cast<size_t>(mi));
    for (int64_t k = 0; k < mi; ++k) out[k] = a[perm[k]];
    return out;
  };
  const std::vector<int32_t> ch = take(r->iv_chrom), st = take(r->iv_start), en = take(r->iv_end), th = take(r->iv_thr),
                             dp = take(r->iv_data_pos);
  fslr_reads vr = *r;
  vr.n_reads = nb;
  vr.read_off = voff.data();
  vr.read_qlen2 = vq.data();
  vr.read_nal = vn.data();
  vr.iv_chrom = ch.data();
  vr.iv_start = st.data();
  vr.iv_end = en.data();
  vr.iv_thr = th.data();
  vr.iv_data_pos = dp.data();
  plan.b_vreal = vreal.data();
  plan.b_vbase = vbase.data();
  plan.b_rlen = rlen.data();
  plan.b_off2 = off2.data();
  plan.b_perm = perm.data();
  plan.max_len = std::max(res_max, batch_max);
  if (int rc = append_core(c, &vr, &plan, who.c_str())) return rc;
  w->rlen_host.insert(w->rlen_host.end(), rlen.begin(), rlen.end());
  w->rlen_gen = c->reads_gen;
  w->rlen_ok = true;
  return FSLR_OK;
}

int fslr_remove_reads_any(fslr_ctx* c, int64_t n_in, const uint8_t* keep, int32_t* new_rank) {
  const std::string who = "fslr_remove_reads_any";
  if (!c) return FSLR_ERR_INVALID;
  // no virtual reads: fslr_remove_reads' own path and bytes
  if (!c->lg_set) return remove_core(c, n_in, keep, new_rank, n_in, who.c_str(), false);
  if (int rc = remove_state(c, who, true)) return rc;
  const int64_t n = c->lg_n_real, V = c->n;
  if (n_in != n)
    return fail(c, FSLR_ERR_INVALID, who + ": n = " + std::to_string(n_in) + " but the context holds " + std::to_string(n) + " reads");
  if (!keep) return fail(c, FSLR_ERR_INVALID, who + ": keep is NULL");
  int64_t n_kept = 0;
  for (int64_t r = 0; r < n; ++r) n_kept += keep[r] != 0;
  if (n_kept == 0) return fail(c, FSLR_ERR_INVALID, who + ": would leave no reads");
  if (n_kept == n) {                             // nothing to remove: no generation moves
    if (new_rank)
      for (int64_t r = 0; r < n; ++r) new_rank[r] = static_cast<int32_t>(r);
    return FSLR_OK;
  }
  if (!c->apw) c->apw = new AppendWork();
  AppendWork* w = c->apw;
  if (int rc = host_rlen(c, w)) return rc;
  // a virtual read stays iff its real read does: the first chunks' flags, then the further chunks' in their order
  std::vector<uint8_t> kv(static_cast<size_t>(V));
  std::vector<int> kept_len;
  kept_len.reserve(static_cast<size_t>(n_kept));
  int64_t u = n, V_new = 0;
  int max_len = 0;
  for (int64_t r = 0; r < n; ++r) {
    const int L = w->rlen_host[static_cast<size_t>(r)], x = anyidx::extra_chunks(L);
    const uint8_t k = keep[r] != 0;
    kv[static_cast<size_t>(r)] = k;
    if (u + x > V) return fail(c, FSLR_ERR_STATE, who + ": the virtual reads do not match the real reads' lengths");
    for (int j = 0; j < x; ++j) kv[static_cast<size_t>(u++)] = k;
    if (k) {
      kept_len.push_back(L);
      V_new += 1 + x;
      max_len = std::max(max_len, L);
    }
  }
  if (u != V) return fail(c, FSLR_ERR_STATE, who + ": the virtual reads do not match the real reads' lengths");
  const bool still_long = V_new > n_kept;
  // room: the new maps, before anything is written
  HIP_TRY(c, hipSetDevice(c->device));
  struct NewMaps {
    int* p[4] = {nullptr, nullptr, nullptr, nullptr};        // vreal, vbase [V_new] | rlen, off2 [n_kept]
    ~NewMaps() {
      for (int* q : p)
        if (q) (void)hipFree(q);
    }
  } fresh;
  if (still_long) {
    const size_t cnt[4] = {static_cast<size_t>(V_new), static_cast<size_t>(V_new), static_cast<size_t>(n_kept), static_cast<size_t>(n_kept)};
    for (int k = 0; k < 4; ++k)
      if (hipMalloc(reinterpret_cast<void**>(&fresh.p[k]), cnt[k] * sizeof(int)) != hipSuccess) {
        fresh.p[k] = nullptr;
        return fail(c, FSLR_ERR_NOMEM, who + ": hipMalloc of the virtual-read maps");
      }
  }
  if (int rc = remove_core(c, V, kv.data(), new_rank, n, who.c_str(), true)) return rc;
  if (still_long) {
    hipStream_t st = c->stream;
    k_any_rm_maps<<<grid_for(V), 256, 0, st>>>(c->lg_vreal, c->lg_vbase, c->lg_rlen, remove_rank_map(c), static_cast<int>(V),
                                              static_cast<int>(n), static_cast<int>(V_new), static_cast<int>(n_kept),
                                              fresh.p[0], fresh.p[1], fresh.p[2], fresh.p[3]);
    k_any_off2<<<grid_for(V_new - n_kept), 256, 0, st>>>(c->rmeta, fresh.p[0], fresh.p[1], static_cast<int>(n_kept),
                                                        static_cast<int>(V_new), fresh.p[3]);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return reads_broken(c, fail(c, FSLR_ERR_HIP, who + ": the maps: " + hipGetErrorString(e)));
    if (int rc = remove_extend_timings(c)) return rc;    // the map kernels count into the compaction phase
    int** slot[4] = {&c->lg_vreal, &c->lg_vbase, &c->lg_rlen, &c->lg_off2};
    for (int k = 0; k < 4; ++k) {
      if (*slot[k]) (void)hipFree(*slot[k]);
      *slot[k] = fresh.p[k];
      fresh.p[k] = nullptr;
    }
    // virtual interval -> real interval of the survivors, as fslr_set_reads_any lays them out
    std::vector<int> perm;
    perm.reserve(static_cast<size_t>(c->ni));
    int64_t off = 0;
    for (int L : kept_len) {
      for (int j = 0; j < std::min(L, FSLR_MAX_L); ++j) perm.push_back(static_cast<int>(off + j));
      off += L;
    }
    off = 0;
    for (int L : kept_len) {
      for (int j = FSLR_MAX_L; j < L; ++j) perm.push_back(static_cast<int>(off + j));
      off += L;
    }
    if (static_cast<int64_t>(perm.size()) != c->ni)
      return reads_broken(c, fail(c, FSLR_ERR_HIP, who + ": the survivors' intervals disagree with their lengths"));
    c->lg_perm.swap(perm);
    c->lg_n_real = n_kept;
    c->lg_max_len = max_len;
    c->lg_n_edges = 0;
  } else {                                       // no long read is left: a plain context, as fslr_set_reads leaves it
    c->lg_set = false;
    c->lg_perm.clear();
    c->lg_n_real = 0;
    c->lg_n_edges = 0;
  }
  w->rlen_host.swap(kept_len);
  w->rlen_gen = c->reads_gen;
  w->rlen_ok = true;
  return FSLR_OK;
}

}  // extern "C"
