// remove.hip — fslr_remove_reads: whole reads dropped from a resident set, on the device.
//
// A stream compaction over the two orders of the same intervals.  The keep bytes go up (the only H2D traffic);
// then, every step a launch of its own on the context's stream:
//   1. k_rm_read_counts / k_rm_data_counts   kept reads and kept intervals per tile of 256 reads, kept
//                                            elements per tile of FSLR_REMOVE_TILE data positions
//   2. k_rm_scan (one block, three times)    the exclusive scans of those tile counts
//   3. k_rm_read_maps                        new_rank and the new CSR offset of every read; rmeta and rlen8
//                                            compacted into scratch
//   4. k_rm_compact_data                     dchrom / drec / dgate compacted into the second set of data-order
//                                            buffers (the append's), newpos[] into the index build's `vals`
//   5. k_rm_compact_csr                      iv and data_pos compacted into index-build scratch; the
//                                            survivors' threshold mode, aln_size == 0 mark and chromosome counts
// and the compacted buffers are swapped in.  No kernel waits on another block: a tile's base comes from a scan
// that ended in an earlier launch.  Every device loop is a grid-stride (or block-stride) loop whose bounds are
// arguments or resident offsets nobody writes meanwhile, or remove_idx.hpp's bounded search.  No global atomic
// decides where anything lands (the only atomics sum the chromosome counts and OR two flags), so the result
// is the same bytes on every run: the bytes fslr_set_reads gives for the compacted CSR.
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "fslr_hip.h"
#include "append.hpp"
#include "ctx.hpp"
#include "kernels.hpp"
#include "remove_idx.hpp"
#include "wave.hpp"

using namespace fslr;

struct RemoveWork {
  unsigned char* keep = nullptr;     // [n] the caller's keep bytes
  int* new_rank = nullptr;           // [n] old rank -> new rank, -1 removed
  int* new_off = nullptr;            // [n] kept intervals of the lower reads: a kept read's new CSR offset
  unsigned char* rlen8 = nullptr;    // [n] the compacted read lengths (copied back on the stream)
  int64_t n_cap = 0;
  int* rt = nullptr;                 // [4 x rt_cap] per read tile: kept reads, kept intervals, their scans
  int64_t rt_cap = 0;
  int* dt = nullptr;                 // [2 x dt_cap] per data tile: kept elements, their scan
  int64_t dt_cap = 0;
  unsigned long long* cnt = nullptr; // [n_chroms] kept intervals per chromosome
  int64_t cnt_cap = 0;
  int* stat = nullptr;               // [4] kept reads, kept intervals (CSR side), kept elements (data side), flags
  hipEvent_t ev[4] = {};             // start | uploaded | maps made | compacted
  bool ev_ok = false, timed = false;
  float ms[4] = {0, 0, 0, 0};        // upload, maps, compaction, total
};

void fslr_remove_free(fslr_ctx* c) {
  RemoveWork* w = c->rmw;
  if (!w) return;
  void* bufs[] = {w->keep, w->new_rank, w->new_off, w->rlen8, w->rt, w->dt, w->cnt, w->stat};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  if (w->ev_ok)
    for (hipEvent_t& e : w->ev) (void)hipEventDestroy(e);
  delete w;
  c->rmw = nullptr;
}

namespace {

constexpr int kFlagGeneral = 1, kFlagZeroAln = 2;   // stat[3]: a kept general threshold, a kept aln_size == 0 interval

// sum of x over the block's 256 threads, in every thread (ws: 4 ints of LDS, free again on return)
__device__ __forceinline__ int block_sum(int x, int* ws) {
  const int inc = wave_incl_scan(x);
  if (lane_id() == kWave - 1) ws[threadIdx.x >> 6] = inc;
  __syncthreads();
  const int total = ws[0] + ws[1] + ws[2] + ws[3];
  __syncthreads();
  return total;
}

// exclusive prefix of x over the block's 256 threads and the block's total (ws as above)
__device__ __forceinline__ int block_excl_scan(int x, int* ws, int* total) {
  const int inc = wave_incl_scan(x);
  const int wave = threadIdx.x >> 6;
  if (lane_id() == kWave - 1) ws[wave] = inc;
  __syncthreads();
  int pre = 0;
  if (wave > 0) pre += ws[0];
  if (wave > 1) pre += ws[1];
  if (wave > 2) pre += ws[2];
  *total = ws[0] + ws[1] + ws[2] + ws[3];
  __syncthreads();
  return pre + inc - x;
}

// per tile of kReadTile reads: kept reads and their intervals
__global__ __launch_bounds__(256) void k_rm_read_counts(const unsigned char* __restrict__ keep,
                                                        const unsigned char* __restrict__ rlen8, int n,
                                                        int* __restrict__ t_reads, int* __restrict__ t_ivs) {
  __shared__ int ws[4];
  for (long long tile = blockIdx.x; tile * rm::kReadTile < n; tile += gridDim.x) {
    const long long r = tile * rm::kReadTile + threadIdx.x;
    const bool k = r < n && keep[r] != 0;
    const int len = k ? rlen8[r] : 0;
    const int reads = block_sum(k ? 1 : 0, ws);
    const int ivs = block_sum(len, ws);
    if (threadIdx.x == 0) {
      t_reads[tile] = reads;
      t_ivs[tile] = ivs;
    }
  }
}

// per tile of rm::kTile data positions: elements whose read stays (the flag is keep[drec[d].w >> 6])
__global__ __launch_bounds__(256) void k_rm_data_counts(const int4* __restrict__ drec,
                                                        const unsigned char* __restrict__ keep, int ni, int n,
                                                        int* __restrict__ t_kept) {
  __shared__ int ws[4];
  for (long long tile = blockIdx.x; tile * rm::kTile < ni; tile += gridDim.x) {
    const long long d0 = tile * rm::kTile;
    const int len = rm::tile_len(ni, tile, rm::kTile);
    int kept = 0;
#pragma unroll
    for (int s = 0; s < rm::kSteps; ++s) {
      const int e = s * 256 + static_cast<int>(threadIdx.x);
      if (e < len) {
        FSLR_BOUND(d0 + e, ni);
        const int r = reinterpret_cast<const int*>(drec + d0 + e)[3] >> 6;
        FSLR_BOUND(r, n);
        kept += keep[r] != 0;
      }
    }
    kept = block_sum(kept, ws);
    if (threadIdx.x == 0) t_kept[tile] = kept;
  }
}

// exclusive scan of m tile counts by ONE block, 256 at a time with a running carry; total[0] = their sum.
// The second level of the two-level scan, in a launch of its own: nothing waits for another block.
__global__ __launch_bounds__(256) void k_rm_scan(const int* __restrict__ in, int* __restrict__ out, int m,
                                                 int* __restrict__ total) {
  __shared__ int ws[4];
  int carry = 0;
  for (int base = 0; base < m; base += 256) {
    const int i = base + static_cast<int>(threadIdx.x);
    const int x = i < m ? in[i] : 0;
    int sum;
    const int pre = block_excl_scan(x, ws, &sum);
    if (i < m) out[i] = carry + pre;
    carry += sum;
  }
  if (threadIdx.x == 0) *total = carry;
}

// per read: new_rank (-1 removed) and the new CSR offset; the kept reads' rmeta (offset rewritten) and rlen8 at
// their new ranks
__global__ __launch_bounds__(256) void k_rm_read_maps(const unsigned char* __restrict__ keep,
                                                      const int4* __restrict__ rmeta,
                                                      const unsigned char* __restrict__ rlen8, int n,
                                                      const int* __restrict__ t_rank, const int* __restrict__ t_off,
                                                      int* __restrict__ new_rank, int* __restrict__ new_off,
                                                      int4* __restrict__ rmeta_out, unsigned char* __restrict__ rlen_out) {
  __shared__ int ws[4];
  for (long long tile = blockIdx.x; tile * rm::kReadTile < n; tile += gridDim.x) {
    const long long r = tile * rm::kReadTile + threadIdx.x;
    const bool k = r < n && keep[r] != 0;
    const int len = k ? rlen8[r] : 0;
    int unused;
    const int rank = t_rank[tile] + block_excl_scan(k ? 1 : 0, ws, &unused);
    const int off = t_off[tile] + block_excl_scan(len, ws, &unused);
    if (r < n) {
      new_rank[r] = k ? rank : -1;
      new_off[r] = off;
    }
    if (k) {
      FSLR_BOUND(rank, n);
      const int4 m = rmeta[r];
      rmeta_out[rank] = make_int4(off, m.y, m.z, m.w);
      rlen_out[rank] = static_cast<unsigned char>(len);
    }
  }
}

// The data order.  A block takes tiles of rm::kTile data positions; a tile's base is the scanned count of the
// lower tiles.  A tile without a survivor writes nothing, a tile without a removed element is a straight copy;
// otherwise wave w walks elements [256 w, 256 w + 256) in four steps of 64, __ballot gives each step's
// survivors, their counts (16 per tile, through LDS) place the steps and mbcnt the lanes.  The records' tags
// take the new ranks.  newpos[d] = the new data position of kept element d (a removed one gets none).
__global__ __launch_bounds__(256) void k_rm_compact_data(const unsigned* __restrict__ dch, const int4* __restrict__ drec,
                                                         const int2* __restrict__ dgate, int ni, int n,
                                                         const unsigned char* __restrict__ keep,
                                                         const int* __restrict__ new_rank,
                                                         const int* __restrict__ t_kept, const int* __restrict__ t_base,
                                                         unsigned* __restrict__ och, int4* __restrict__ orec,
                                                         int2* __restrict__ ogate, int* __restrict__ newpos) {
  __shared__ int scnt[4 * rm::kSteps];
  const int lane = lane_id(), wave = static_cast<int>(threadIdx.x >> 6);
  for (long long tile = blockIdx.x; tile * rm::kTile < ni; tile += gridDim.x) {
    const long long d0 = tile * rm::kTile;
    const int len = rm::tile_len(ni, tile, rm::kTile);
    const int kept = t_kept[tile], base = t_base[tile];          // the same for every thread of the block
    if (kept == 0) continue;
    if (kept == len) {
      for (int t = threadIdx.x; t < len; t += blockDim.x) {
        FSLR_BOUND(d0 + t, ni);
        FSLR_BOUND(base + t, ni);
        int4 rec = drec[d0 + t];
        FSLR_BOUND(rec.w >> 6, n);
        rec.w = rm::retag(rec.w, new_rank[rec.w >> 6]);
        orec[base + t] = rec;
        ogate[base + t] = dgate[d0 + t];
        och[base + t] = dch[d0 + t];
        newpos[d0 + t] = base + t;
      }
      continue;
    }
    int4 rec[rm::kSteps];
    unsigned long long mask[rm::kSteps];
#pragma unroll
    for (int s = 0; s < rm::kSteps; ++s) {
      const int e = rm::tile_element(wave, s, lane);
      bool stays = false;
      rec[s] = make_int4(0, 0, 0, 0);
      if (e < len) {
        FSLR_BOUND(d0 + e, ni);
        rec[s] = drec[d0 + e];
        FSLR_BOUND(rec[s].w >> 6, n);
        stays = keep[rec[s].w >> 6] != 0;
      }
      mask[s] = __ballot(stays);
      if (lane == 0) scnt[wave * rm::kSteps + s] = __popcll(mask[s]);
    }
    __syncthreads();
    int before = 0;
#pragma unroll
    for (int i = 0; i < 4 * rm::kSteps; ++i)
      if (i < wave * rm::kSteps) before += scnt[i];
#pragma unroll
    for (int s = 0; s < rm::kSteps; ++s) {
      if ((mask[s] >> lane) & 1ull) {
        const long long d = d0 + rm::tile_element(wave, s, lane);
        const int p = rm::survivor_pos(base, before, mbcnt(mask[s]));
        FSLR_BOUND(p, ni);
        FSLR_BOUND(p - base, kept);
        int4 r4 = rec[s];
        r4.w = rm::retag(r4.w, new_rank[r4.w >> 6]);
        orec[p] = r4;
        ogate[p] = dgate[d];
        och[p] = dch[d];
        newpos[d] = p;
      }
      before += __popcll(mask[s]);
    }
    __syncthreads();                                             // scnt serves the block's next tile
  }
}

// The CSR order.  A block takes tiles of rm::kReadTile reads: their first offsets and new offsets go to LDS,
// then the block walks the tile's CSR range (at most 256 x FSLR_MAX_L intervals) 256 at a time; each interval
// finds its read among the tile's by a search of at most rm::kOwnerSteps halvings.  Never in place: the
// destination of one block overlaps the source of another, so the output goes to scratch that is swapped in.
// flags: OR of kFlagGeneral / kFlagZeroAln over the kept intervals; cnt: kept intervals per chromosome.
__global__ __launch_bounds__(256) void k_rm_compact_csr(const int4* __restrict__ rmeta, const unsigned char* __restrict__ rlen8,
                                                        const unsigned char* __restrict__ keep,
                                                        const int* __restrict__ new_off, int n,
                                                        const int4* __restrict__ iv, const int* __restrict__ data_pos,
                                                        const int* __restrict__ newpos, int ni, int n_chroms,
                                                        int4* __restrict__ iv_out, int* __restrict__ dp_out,
                                                        unsigned long long* __restrict__ cnt, int* __restrict__ flags) {
  __shared__ int s_off[rm::kReadTile + 1];
  __shared__ int s_new[rm::kReadTile];
  __shared__ unsigned hist[kUpHistLds];
  const bool lds = n_chroms <= kUpHistLds;
  if (lds)
    for (int i = threadIdx.x; i < n_chroms; i += blockDim.x) hist[i] = 0;
  int bits = 0;
  for (long long tile = blockIdx.x; tile * rm::kReadTile < n; tile += gridDim.x) {
    const long long r0 = tile * rm::kReadTile;
    const int reads = rm::tile_len(n, tile, rm::kReadTile);
    const int t = threadIdx.x;
    __syncthreads();                                             // the last tile's walk is over (and hist is zero)
    if (t < reads) {
      const int off = rmeta[r0 + t].x;
      s_off[t] = off;
      s_new[t] = keep[r0 + t] != 0 ? new_off[r0 + t] : -1;
      if (t == reads - 1) s_off[reads] = off + rlen8[r0 + t];
    }
    __syncthreads();
    const int k0 = s_off[0], k1 = s_off[reads];
    for (int k = k0 + t; k < k1; k += blockDim.x) {
      FSLR_BOUND(k, ni);
      const int o = rm::owner_of(s_off, reads, k, rm::kOwnerSteps);
      FSLR_BOUND(o, reads);
      FSLR_BOUND(k - s_off[o], FSLR_MAX_L);
      if (s_new[o] < 0) continue;
      const int dst = rm::new_csr_index(s_new[o], s_off[o], k);
      FSLR_BOUND(dst, ni);
      const int4 v = iv[k];
      const int d = data_pos[k];
      FSLR_BOUND(d, ni);
      const int p = newpos[d];
      FSLR_BOUND(p, ni);
      iv_out[dst] = v;
      dp_out[dst] = p;
      if (v.w == FSLR_THR_ZERO_ALN) bits |= kFlagZeroAln;
      else if (v.w < 1) bits |= kFlagGeneral;
      if (v.x >= 0 && v.x < n_chroms) {
        if (lds) atomicAdd(&hist[v.x], 1u);
        else atomicAdd(cnt + v.x, 1ull);
      }
    }
  }
  const int general = __syncthreads_or(bits & kFlagGeneral), zero_aln = __syncthreads_or(bits & kFlagZeroAln);
  bits = (general ? kFlagGeneral : 0) | (zero_aln ? kFlagZeroAln : 0);     // (the barrier ORs predicates, not bits)
  if (threadIdx.x == 0 && bits) atomicOr(flags, bits);
  if (lds)
    for (int i = threadIdx.x; i < n_chroms; i += blockDim.x)
      if (hist[i]) atomicAdd(cnt + i, static_cast<unsigned long long>(hist[i]));
}

template <typename T>
int ensure(fslr_ctx* c, T** p, int64_t* cap, int64_t need, int64_t mult = 1) {
  if (need <= *cap) return FSLR_OK;
  *cap = 0;                                       // (a failed growth leaves no buffer behind its capacity)
  const int64_t grown = need + need / 4;
  if (int rc = dalloc(c, p, static_cast<size_t>(grown * mult))) return rc;
  *cap = grown;
  return FSLR_OK;
}

int broken(fslr_ctx* c, int rc) { return reads_broken(c, rc); }

#define RM_TRY(ctx, expr)                                                                                     \
  do {                                                                                                        \
    hipError_t e_ = (expr);                                                                                   \
    if (e_ != hipSuccess)                                                                                     \
      return broken((ctx), fail((ctx), FSLR_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)));     \
  } while (0)

}  // namespace

// the states neither removal takes, each named; virt: virtual reads are fine (fslr_remove_reads_any)
int fslr::remove_state(fslr_ctx* c, const std::string& who, bool virt) {
  if (!c->reads_set) return fail(c, FSLR_ERR_STATE, who + ": no reads set (fslr_set_reads first)");
  if (c->rows_set)
    return fail(c, FSLR_ERR_STATE, who + ": the reads were made from rows (fslr_set_reads_rows), which it does not compact");
  if (!virt && (c->lg_set || !c->lg_perm.empty()))
    return fail(c, FSLR_ERR_STATE, who + ": the context holds virtual reads (fslr_set_reads_any / fslr_set_long_reads: "
                                   "reads of more than " + std::to_string(FSLR_MAX_L) + " intervals), which it does not compact");
  if (virt && c->lg_set && c->lg_perm.empty())
    return fail(c, FSLR_ERR_STATE, who + ": the virtual reads were made by the caller (fslr_set_long_reads), not by "
                                   "fslr_set_reads_any: their real CSR is not known here");
  if (!c->have_data_pos)
    return fail(c, FSLR_ERR_STATE, who + ": the reads were set without iv_data_pos (no start-sorted data list to compact)");
  if (c->n_shards > 1) return fail(c, FSLR_ERR_STATE, who + ": n_shards > 1 (fslr_set_shard): multi-GPU contexts do not remove");
  if (c->filter_active || c->pf_on)
    return fail(c, FSLR_ERR_STATE, who + ": a chromosome or position filter is active");
  return FSLR_OK;
}

// virt: fslr_remove_reads_any's compaction of the virtual reads (keep, n_in and the map are over them; the map's
// first n_rank entries, the real reads', go back to the caller)
int fslr::remove_core(fslr_ctx* c, int64_t n_in, const uint8_t* keep, int32_t* new_rank, int64_t n_rank, const char* who_c,
                      bool virt) {
  if (!c) return FSLR_ERR_INVALID;
  const std::string who(who_c);
  if (int rc = remove_state(c, who, virt)) return rc;
  const int64_t n = c->n, ni = c->ni;
  if (n_in != n)
    return fail(c, FSLR_ERR_INVALID, who + ": n = " + std::to_string(n_in) + " but the context holds " +
                                         std::to_string(n) + " reads");
  if (!keep) return fail(c, FSLR_ERR_INVALID, who + ": keep is NULL");
  int64_t n_kept = 0;
  for (int64_t r = 0; r < n; ++r) n_kept += keep[r] != 0;
  if (n_kept == 0) return fail(c, FSLR_ERR_INVALID, who + ": would leave no reads");
  if (n_kept == n) {                             // nothing to remove: no generation moves
    if (new_rank)
      for (int64_t r = 0; r < n_rank; ++r) new_rank[r] = static_cast<int32_t>(r);
    return FSLR_OK;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  // ---- room: everything is allocated before any resident buffer is written ---------------------------
  if (!c->rmw) c->rmw = new RemoveWork();
  RemoveWork* w = c->rmw;
  if (!c->apw) c->apw = new AppendWork();
  AppendWork* aw = c->apw;                       // its second set of data-order buffers takes the compacted list
  w->timed = false;
  const bool prof = c->profiling;
  if (prof && !w->ev_ok) {
    for (hipEvent_t& e : w->ev) HIP_TRY(c, hipEventCreate(&e));
    w->ev_ok = true;
  }
  const int64_t r_tiles = rm::tiles_of(n, rm::kReadTile), d_tiles = rm::tiles_of(ni, rm::kTile);
  int rc;
  if (n > w->n_cap) {
    w->n_cap = 0;
    const size_t cap = static_cast<size_t>(n + n / 4);
    if ((rc = dalloc(c, &w->keep, cap)) || (rc = dalloc(c, &w->new_rank, cap)) || (rc = dalloc(c, &w->new_off, cap)) ||
        (rc = dalloc(c, &w->rlen8, cap)))
      return rc;
    w->n_cap = static_cast<int64_t>(cap);
  }
  if ((rc = ensure(c, &w->rt, &w->rt_cap, r_tiles, 4)) || (rc = ensure(c, &w->dt, &w->dt_cap, d_tiles, 2)) ||
      (rc = ensure(c, &w->cnt, &w->cnt_cap, c->n_chroms)))
    return rc;
  if (!w->stat && (rc = dalloc(c, &w->stat, 4))) return rc;
  if (aw->alt_cap < c->cap_ni) {
    aw->alt_cap = 0;
    const size_t cap = static_cast<size_t>(c->cap_ni);
    if ((rc = dalloc(c, &aw->alt_ch, cap)) || (rc = dalloc(c, &aw->alt_rec, cap)) || (rc = dalloc(c, &aw->alt_gate, cap))) return rc;
    aw->alt_cap = c->cap_ni;
  }
  hipStream_t st = c->stream;
  const int in = static_cast<int>(n), ini = static_cast<int>(ni);
  int* t_reads = w->rt;
  int* t_ivs = t_reads + w->rt_cap;
  int* t_rank = t_ivs + w->rt_cap;
  int* t_off = t_rank + w->rt_cap;
  int* t_kept = w->dt;
  int* t_base = t_kept + w->dt_cap;
  // ---- the maps: nothing resident is written (only this call's own scratch) --------------------------
  if (prof) HIP_TRY(c, hipEventRecord(w->ev[0], st));
  HIP_TRY(c, hipMemcpyAsync(w->keep, keep, static_cast<size_t>(n), hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemsetAsync(w->cnt, 0, static_cast<size_t>(c->n_chroms) * sizeof(unsigned long long), st));
  HIP_TRY(c, hipMemsetAsync(w->stat, 0, 4 * sizeof(int), st));
  if (prof) HIP_TRY(c, hipEventRecord(w->ev[1], st));
  k_rm_read_counts<<<grid_for(r_tiles, 1), 256, 0, st>>>(w->keep, c->rlen8, in, t_reads, t_ivs);
  k_rm_scan<<<1, 256, 0, st>>>(t_reads, t_rank, static_cast<int>(r_tiles), w->stat + 0);
  k_rm_scan<<<1, 256, 0, st>>>(t_ivs, t_off, static_cast<int>(r_tiles), w->stat + 1);
  if (d_tiles) {
    k_rm_data_counts<<<grid_for(d_tiles, 1), 256, 0, st>>>(c->drec, w->keep, ini, in, t_kept);
    k_rm_scan<<<1, 256, 0, st>>>(t_kept, t_base, static_cast<int>(d_tiles), w->stat + 2);
  }
  HIP_TRY(c, hipGetLastError());
  // from here the index scratch is reused and the resident buffers' successors are written
  c->index_built = false;
  c->hooked = false;
  int4* rmeta_out = c->lbounds;                  // [cap_n] int4, as rmeta: swapped in below (the length gate's ranges
  c->lb_gen = -1;                                //   belong to the old reads anyway)
  int4* iv_out = c->idx4;                        // [cap_ni] int4, as iv
  int* dp_out = c->vals2;                        // [cap_ni] int, as data_pos
  int* newpos = c->vals;                         // [ni] index-build scratch, as the append uses it
  k_rm_read_maps<<<grid_for(r_tiles, 1), 256, 0, st>>>(w->keep, c->rmeta, c->rlen8, in, t_rank, t_off, w->new_rank,
                                                       w->new_off, rmeta_out, w->rlen8);
  RM_TRY(c, hipGetLastError());
  if (prof) RM_TRY(c, hipEventRecord(w->ev[2], st));
  if (d_tiles) {
    k_rm_compact_data<<<grid_for(d_tiles, 1), 256, 0, st>>>(c->dchrom, c->drec, c->dgate, ini, in, w->keep, w->new_rank,
                                                            t_kept, t_base, aw->alt_ch, aw->alt_rec, aw->alt_gate, newpos);
    k_rm_compact_csr<<<grid_for(r_tiles, 1), 256, 0, st>>>(c->rmeta, c->rlen8, w->keep, w->new_off, in, c->iv, c->data_pos,
                                                           newpos, ini, c->n_chroms, iv_out, dp_out, w->cnt, w->stat + 3);
    RM_TRY(c, hipGetLastError());
  }
  if (prof) RM_TRY(c, hipEventRecord(w->ev[3], st));
  // the host's aln_size == 0 marks follow the reads; their lengths come back only when there is a mark to move
  std::vector<unsigned char> old_len;
  if (c->any_zero_aln) {
    old_len.resize(static_cast<size_t>(n));
    RM_TRY(c, hipMemcpyAsync(old_len.data(), c->rlen8, static_cast<size_t>(n), hipMemcpyDeviceToHost, st));
  }
  RM_TRY(c, hipMemcpyAsync(c->rlen8, w->rlen8, static_cast<size_t>(n_kept), hipMemcpyDeviceToDevice, st));
  std::vector<int64_t> counts(static_cast<size_t>(c->n_chroms), 0);
  int stat[4] = {0, 0, 0, 0};
  RM_TRY(c, hipMemcpyAsync(counts.data(), w->cnt, counts.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  RM_TRY(c, hipMemcpyAsync(stat, w->stat, sizeof(stat), hipMemcpyDeviceToHost, st));
  if (new_rank) RM_TRY(c, hipMemcpyAsync(new_rank, w->new_rank, static_cast<size_t>(n_rank) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  RM_TRY(c, hipStreamSynchronize(st));
  const int64_t ni_kept = stat[1];
  if (stat[0] != n_kept || (d_tiles && stat[2] != stat[1]) || ni_kept < n_kept || ni_kept > ni)
    return broken(c, fail(c, FSLR_ERR_HIP, who + ": the two orders disagree (" + std::to_string(stat[0]) + " reads, " +
                                               std::to_string(stat[1]) + " / " + std::to_string(stat[2]) + " intervals kept)"));
  // chromosome ranges of the (chrom, start)-sorted index from the kept counts, as fslr_set_reads makes them
  std::vector<int2> cr(counts.size(), make_int2(0, 0));
  int64_t acc = 0;
  for (size_t ch = 0; ch < counts.size(); ++ch) {
    cr[ch] = make_int2(static_cast<int>(acc), static_cast<int>(acc + counts[ch]));
    acc += counts[ch];
  }
  RM_TRY(c, hipMemcpyAsync(c->crange, cr.data(), cr.size() * sizeof(int2), hipMemcpyHostToDevice, st));
  RM_TRY(c, hipStreamSynchronize(st));
  std::swap(c->dchrom, aw->alt_ch);
  std::swap(c->drec, aw->alt_rec);
  std::swap(c->dgate, aw->alt_gate);
  aw->alt_cap = c->cap_ni;                       // what the context's buffers were allocated for, at least
  std::swap(c->rmeta, c->lbounds);
  std::swap(c->iv, c->idx4);
  std::swap(c->data_pos, c->vals2);
  if (c->any_zero_aln) {
    int64_t src = 0, dst = 0;
    for (int64_t r = 0; r < n; ++r) {
      const int len = old_len[static_cast<size_t>(r)];
      if (keep[r])
        for (int j = 0; j < len; ++j) c->aln_zero_host[static_cast<size_t>(dst++)] = c->aln_zero_host[static_cast<size_t>(src + j)];
      src += len;
    }
  }
  c->aln_zero_host.resize(static_cast<size_t>(ni_kept), 0);
  c->n = n_kept;
  c->ni = ni_kept;
  c->ni_idx = ni_kept;
  c->chrom_counts.swap(counts);
  c->thr_mode = (stat[3] & kFlagGeneral) ? 1 : 0;
  c->any_zero_aln = (stat[3] & kFlagZeroAln) != 0;
  ++c->reads_gen;
  c->pf_set = c->pf_on = false;
  c->edges_global = false;
  c->cap_gmode = false;
  ++c->input_gen;
  if (prof) {
    for (int t = 0; t < 3; ++t) HIP_TRY(c, hipEventElapsedTime(&w->ms[t], w->ev[t], w->ev[t + 1]));
    HIP_TRY(c, hipEventElapsedTime(&w->ms[3], w->ev[0], w->ev[3]));
    w->timed = true;
  }
  return FSLR_OK;
}

const int* fslr::remove_rank_map(fslr_ctx* c) { return c->rmw ? c->rmw->new_rank : nullptr; }

int fslr::remove_extend_timings(fslr_ctx* c) {
  RemoveWork* w = c->rmw;
  if (!w || !w->timed) return FSLR_OK;
  HIP_TRY(c, hipEventRecord(w->ev[3], c->stream));
  HIP_TRY(c, hipEventSynchronize(w->ev[3]));
  HIP_TRY(c, hipEventElapsedTime(&w->ms[2], w->ev[2], w->ev[3]));
  HIP_TRY(c, hipEventElapsedTime(&w->ms[3], w->ev[0], w->ev[3]));
  return FSLR_OK;
}

extern "C" {

int fslr_remove_reads(fslr_ctx* c, int64_t n, const uint8_t* keep, int32_t* new_rank) {
  return remove_core(c, n, keep, new_rank, n, "fslr_remove_reads", false);
}

int fslr_remove_timings(fslr_ctx* c, float* ms) {
  if (!c || !ms) return FSLR_ERR_INVALID;
  RemoveWork* w = c->rmw;
  if (!w || !w->timed)
    return fail(c, FSLR_ERR_STATE, "fslr_remove_timings: no profiled fslr_remove_reads / fslr_remove_reads_any (fslr_set_profiling 1 or 2)");
  for (int t = 0; t < 4; ++t) ms[t] = w->ms[t];
  return FSLR_OK;
}

}  // extern "C"
