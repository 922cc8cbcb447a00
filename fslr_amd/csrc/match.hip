// match.hip — the reference's pair loop (cluster.py:197-222) for reads that are NOT in the resident
// set: query_key = a new read Q, list1 = Q's intervals in the given order, the tree = the built index.
// Per interval of Q the hits of search_values (the hit rule and the order of search.hip), the seen-set
// of :205-208 kept per query read, and per distinct partner P the predicates of score.hip for the
// ordered pair (list1 = Q, list2 = P).
//
// Out of scope (the boundaries the next request meets):
//   - the edge cap (:223-224): a matched read's loop is not part of the resident graph's cap replay,
//     so every candidate is evaluated, however many edges the read has formed;
//   - query or resident reads of more than FSLR_MAX_ANY_L intervals (fslr_match_reads keeps refusing more
//     than FSLR_MAX_L; fslr_match_reads_any takes them, below);
//   - matching through the multi-GPU split (a partial index is refused, as fslr_search refuses it);
//   - inserting matched reads into the index.
//
// Passes.  Query reads go up in blocks of at most kBlockReads reads / kBlockIvs intervals; a block is
// cut into chunks of consecutive reads whose hits fit the hit budget (kBudget, or FSLR_MATCH_BUDGET
// read at call time; a read whose hits alone exceed it is a chunk of its own, so the budget is bounded
// below only by the largest single read's hits).  No scratch grows with the batch.
//   count   one wavefront per query read: one lane per interval finds its span [lo, hi) (the upper
//           bound of qe in the chromosome's starts; the first tile whose prefix max of (chrom, end)
//           reaches (c, qs): IndexView::span_of of idxsearch.hpp, search.hip's span pass too), then the
//           wave counts each span's hits 64 positions at a time
//   fill    one wavefront per read of the chunk: a hit's rank in its interval's list is its ascending
//           rank, re-ranked inside a run of equal start on (end descending, data position ascending:
//           IndexView::tie_shift), written top-down: the read's hit list in visiting order, as
//           partner ranks
//   score   one wavefront per read: Q's intervals staged in LDS; the hit list 64 at a time through a
//           per-wave LDS hash set (kMatchSetCap = FSLR_MATCH_SET distinct partners; a slot keeps the
//           smallest hit index that claimed it, so the first visits of a batch come out in lane order).
//           Once the set holds kMatchSetCap partners it is closed, and a later hit whose partner it lacks
//           is a first visit iff no earlier hit of the staged list past the closing point names the same
//           partner (the witness rule, on the list).  The batch's new partners are scored four (two,
//           one) at a time on 16- (32-, 64-)lane groups: the first-fit of firstfit.hpp, score.hip's
//           too, with list1's rows read from LDS.  Emitted rows are staged at the read's hit offset
//           (rows <= hits).
//   compact exclusive scan of the chunk's row counts, rows copied dense, then D2H
// Every output slot is a function of the input alone: no global atomics, the same bytes on every run.
//
// fslr_match_reads_any: the same driver.  Without virtual reads and without a query read
// of more than FSLR_MAX_L intervals it launches the kernels above (<false>) and keeps the old row word.
// Otherwise the <true> instantiations run: count takes a read's intervals 64 at a time; fill writes REAL
// partner ranks (vreal[tag >> 6]) and ranks tied hits by the real CSR index through the lg_perm copy
// (IndexView::ids<true>); score dedupes real ranks, so the chunks of one long read are one candidate at its
// first hit, and a candidate with LA or LB beyond FSLR_MAX_L runs alone on the wave through long_fit
// (firstfit.hpp), list1's rows read from the block's interval columns.  The result word is the wide one.
// Algorithmic bytes: count 8 B per span position; fill 16 B per span position + 4 B per hit; score 4 B
// per hit, 16 B (rmeta) + 16 B x L_P per candidate, 8 B per row (twice: staged, dense).
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "ctx.hpp"
#include "firstfit.hpp"
#include "fslr_hip.h"
#include "idxsearch.hpp"
#include "kernels.hpp"
#include "wave.hpp"

using namespace fslr;

namespace {

constexpr int kMatchSetCap = FSLR_MATCH_SET;   // distinct partners the LDS set takes before it closes
constexpr int kSetSlots = 512;                 // open addressing; at most kMatchSetCap + 63 keys
constexpr int kWavesPerBlock = 4;
constexpr int64_t kBlockReads = int64_t(1) << 16;
constexpr int64_t kBlockIvs = int64_t(1) << 20;
constexpr int64_t kBudget = int64_t(1) << 21;  // hits per chunk: 40 MiB of hit / row scratch
static_assert(kMatchSetCap + kWave <= kSetSlots * 3 / 4, "the set's table must stay sparse");

}  // namespace

struct MatchWork {
  // the block: the query reads as uploaded and what the count pass makes of them
  int* rd = nullptr;                 // [4 x (kBlockReads + 1)] read_off, qlen2, nal, exclude
  int* qcol = nullptr;               // [4 x kBlockIvs] chrom, start, end, thr
  int2* span = nullptr;              // [kBlockIvs]
  int* ivcnt = nullptr;              // [kBlockIvs] hits per interval
  long long* rhits = nullptr;        // [kBlockReads] hits per read
  long long* hoff = nullptr;         // [kBlockReads] the read's hit offset in its chunk
  int* cnt3 = nullptr;               // [3 x kBlockReads] candidates, gated, edges
  int* best = nullptr;               // [kBlockReads]
  long long* nrows = nullptr;        // [kBlockReads + 1] rows per read of the chunk (0 behind the last)
  long long* roff = nullptr;         // [kBlockReads + 1] their exclusive scan
  unsigned char* pt = nullptr;       // the pass table
  void* temp = nullptr;
  size_t temp_bytes = 0;
  long long* pin = nullptr;          // pinned [3 x (kBlockReads + 1)]: rhits | hoff | roff
  bool block_ok = false;
  // the chunk: bounded by the hit budget (or the largest single read)
  int* hits = nullptr;               // [h_cap] partner ranks in visiting order
  unsigned long long* stage = nullptr;   // [h_cap] rows at their read's hit offset
  unsigned long long* dense = nullptr;   // [h_cap] the chunk's rows, dense
  int64_t h_cap = 0;
  // the last batch (fslr_match_rows): partner | I << 32 | U << 40 | flags << 48
  std::vector<unsigned long long> rows;
  bool valid = false;
  bool any = false, wide = false;    // the batch came from fslr_match_reads_any; its rows hold the wide word
  uint64_t reads_gen = 0, index_gen = 0;
  int* umax = nullptr;               // [umax_cap] the _any call's cutoff table
  int umax_cap = 0;
  int* perm = nullptr;               // fslr_set_reads_any: virtual -> real interval (lg_perm), per reads_gen
  int64_t perm_cap = 0;
  uint64_t perm_gen = 0;
  int short_max = 0;                 // the longest resident read of a context without virtual reads, per reads_gen
  uint64_t short_gen = 0;
  hipEvent_t ev[8] = {};
  bool ev_ok = false, timed = false;
  float ms[4] = {0, 0, 0, 0};        // upload, search, dedupe + score, download
};

void fslr_match_free(fslr_ctx* c) {
  MatchWork* w = c->mtw;
  if (!w) return;
  void* bufs[] = {w->rd, w->qcol, w->span, w->ivcnt, w->rhits, w->hoff, w->cnt3, w->best, w->nrows, w->roff,
                  w->pt, w->temp, w->hits, w->stage, w->dense, w->umax, w->perm};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  if (w->pin) (void)hipHostFree(w->pin);
  if (w->ev_ok)
    for (hipEvent_t e : w->ev) (void)hipEventDestroy(e);
  delete w;
  c->mtw = nullptr;
}

namespace {

struct MatchArgs {
  IndexView ix;
  const int* roffq;                      // the block's read_off (as the caller's: absolute), qlen2, nal, exclude
  const int* qlen2;
  const int* nal;
  const int* excl;
  const int *qc, *qs, *qe, *qt;          // the block's interval columns, from interval ivbase of the batch
  int ivbase;
  int nbi;                               // intervals of the block
  int2* span;
  int* ivcnt;
  long long* rhits;
  const long long* hoff;
  int r0, r1;                            // the chunk's reads (block-relative); count: the whole block
  int* hits;
  unsigned long long* stage;
  long long h_cap;
  const int4* iv;                        // the resident intervals
  const unsigned char* pt;
  double qcut, ncut;
  unsigned emit_mask;
  int* cnt3;
  int* best;
  long long* nrows;                      // chunk-relative
  // <true> kernels only
  const int* vreal;                      // null, or virtual -> real read
  const int* rlen;                       // null, or a real read's interval count
  const int* off2;                       // where a long read's intervals beyond FSLR_MAX_L begin
  const int* umax;
  int n_umax;
};

__global__ __launch_bounds__(256) void k_match_count(MatchArgs s) {
  const int lane = threadIdx.x & 63;
  const int nw = gridDim.x * (blockDim.x >> 6);
  for (int r = s.r0 + blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < s.r1; r += nw) {
    const int ob = s.roffq[r] - s.ivbase, Lr = s.roffq[r + 1] - s.roffq[r];
    long long tot = 0;
    for (int b0 = 0; b0 < Lr; b0 += kWave) {       // 64 intervals at a time (one pass up to FSLR_MAX_L)
      const int o0 = ob + b0, L = min(kWave, Lr - b0);
      int2 sp = make_int2(0, 0);
      int qs = 0;
      if (lane < L) {
        FSLR_BOUND(o0 + lane, s.nbi);
        qs = max(s.qs[o0 + lane], 0);              // stored ends are >= 0: the same hits
        sp = s.ix.span_of(s.qc[o0 + lane], qs, s.qe[o0 + lane]);
        s.span[o0 + lane] = sp;
      }
      int mine = 0;
      for (int i = 0; i < L; ++i) {
        const int lo = rdl(sp.x, i), hi = rdl(sp.y, i), q = rdl(qs, i);
        int cnt = 0;
        for (int p0 = lo; p0 < hi; p0 += kWave) {
          const int p = p0 + lane;
          cnt += __popcll(__ballot(p < hi && s.ix.reaches(p, q)));
        }
        if (lane == i) mine = cnt;
        tot += cnt;
      }
      if (lane < L) s.ivcnt[o0 + lane] = mine;
    }
    if (lane == 0) s.rhits[r] = tot;
  }
}

template <bool kAny>
__global__ __launch_bounds__(256) void k_match_fill(MatchArgs s) {
  const int lane = threadIdx.x & 63;
  const int nw = gridDim.x * (blockDim.x >> 6);
  const IndexView& ix = s.ix;
  for (int r = s.r0 + blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < s.r1; r += nw) {
    const int o0 = s.roffq[r] - s.ivbase, L = s.roffq[r + 1] - s.roffq[r];
    long long base = s.hoff[r];
    for (int i = 0; i < L; ++i) {
      FSLR_BOUND(o0 + i, s.nbi);
      const int2 sp = s.span[o0 + i];
      const int qs = max(s.qs[o0 + i], 0);
      const int cnt = s.ivcnt[o0 + i];
      int asc = 0;                                 // hits of the span's earlier pieces
      for (int p0 = sp.x; p0 < sp.y; p0 += kWave) {
        const int p = p0 + lane;
        bool hit = false;
        int4 rec = make_int4(0, 0, 0, 0);
        if (p < sp.y) {
          FSLR_BOUND(p, ix.ni);
          rec = ix.idx4[p];
          hit = rec.y >= qs;
        }
        const unsigned long long hm = __ballot(hit);
        if (hit) {
          int rk = asc + mbcnt(hm);                // ascending rank among the interval's hits, ties in index order
          // (its data position is looked up for a tied hit only)
          if (ix.tied(sp, p, rec.x))
            rk += ix.template tie_shift<kAny>(sp, p, rec, qs, ix.template ids<kAny>(rec.w).y);
          const long long dst = base + cnt - 1 - rk;   // top-down
          FSLR_BOUND(dst, s.h_cap);
          int partner = static_cast<int>(static_cast<unsigned>(rec.w) >> 6);
          if constexpr (kAny)
            if (s.vreal) partner = s.vreal[partner];   // a chunk's hits are its real read's
          s.hits[dst] = partner;
        }
        asc += __popcll(hm);
      }
      base += cnt;
    }
  }
}

// 64 / W candidates side by side, candidate k on the W-lane group of this lane: the first-fit of firstfit.hpp
// with list1 = the query read's LA rows in LDS (uniform over the wave), list2's columns on the group's lanes
template <int W, bool kAny>
__device__ __forceinline__ void match_groups(const MatchArgs& s, const int4* qiv, int LA, int k, bool valid, int offB,
                                             int LB, int gate, int lane, unsigned* res) {
  const int l = lane & (W - 1);
  const bool col = valid && l < LB;
  int4 bj = make_int4(-2, 0, 0, 0);
  if (col) {
    FSLR_BOUND(offB + l, s.ix.ni);
    bj = s.iv[offB + l];
  }
  FirstFit ff;
  for (int i = 0; i < LA; ++i) {
    const int4 a = qiv[i];
    ff.row<W>(a.x, a.y, a.z, a.w, true, bj, col, lane);
  }
  if (valid && l == 0) {
    if constexpr (kAny)
      res[k] = fit_result_any(LA, LB, ff.I, ff.zd, gate, s.pt, s.umax, s.n_umax);
    else
      res[k] = fit_result(LA, LB, ff.I, ff.zd, gate, s.pt);
  }
}

// list1 of a long first-fit: the query read's rows from the block's interval columns
struct QueryRows {
  const int *qc, *qs, *qe, *qt;
  int o0, nbi;
  __device__ __forceinline__ int4 operator()(int i) const {
    FSLR_BOUND(o0 + i, nbi);
    return make_int4(qc[o0 + i], qs[o0 + i], qe[o0 + i], qt[o0 + i]);
  }
};

struct CandMeta {
  int offB, LB, gate;
  int offB2;                           // <true>: where a long partner's intervals beyond FSLR_MAX_L begin
  bool score;                          // false: no candidate here, or one that cannot be emitted
};

// candidate k of the batch (valid: k is one): the partner's CSR row and the length gate against Q
template <bool kAny>
__device__ __forceinline__ CandMeta cand_meta(const MatchArgs& s, const int* cand, int k, bool valid, int q2, int qn,
                                              unsigned* res) {
  CandMeta m{0, 0, 0, 0, false};
  if (valid) {
    const int p = cand[k];
    FSLR_BOUND(p, s.ix.n);
    const int4 mb = s.ix.rmeta[p];
    m.offB = mb.x;
    m.LB = mb.y & 0xffff;
    if constexpr (kAny) {
      if (s.rlen) {
        m.LB = s.rlen[p];
        if (m.LB > FSLR_MAX_L) m.offB2 = s.off2[p];
      }
    }
    m.gate = gate_flags(q2, mb.z, qn, mb.w, s.qcut, s.ncut);
    // a candidate with the gate clear can carry ZD_GATE and ZD_OVERLAP only: where the mask asks for neither
    // that it has nor for ZD_OVERLAP, no row can come of it and its first-fit is skipped
    m.score = (m.gate & FSLR_SCORE_GATE) || s.emit_mask == 0 || (s.emit_mask & FSLR_SCORE_ZD_OVERLAP) ||
              (s.emit_mask & static_cast<unsigned>(m.gate));
  }
  return m;
}

template <bool kAny>
__global__ __launch_bounds__(256) void k_match_score(MatchArgs s) {
  constexpr int kFlagShift = kAny ? kAnyIBits + kAnyUBits : 16;
  __shared__ int4 sh_q[kWavesPerBlock][FSLR_MAX_L];
  __shared__ int sh_key[kWavesPerBlock][kSetSlots];
  __shared__ int sh_seq[kWavesPerBlock][kSetSlots];
  __shared__ int sh_cand[kWavesPerBlock][kWave];
  __shared__ unsigned sh_res[kWavesPerBlock][kWave];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int nw = gridDim.x * kWavesPerBlock;
  int4* qiv = sh_q[wv];
  int* key = sh_key[wv];
  int* seq = sh_seq[wv];
  int* cand = sh_cand[wv];
  unsigned* res = sh_res[wv];
  for (int r = s.r0 + blockIdx.x * kWavesPerBlock + wv; r < s.r1; r += nw) {
    const int o0 = s.roffq[r] - s.ivbase, LA = s.roffq[r + 1] - s.roffq[r];
    const int q2 = s.qlen2[r], qn = s.nal[r], excl = s.excl[r];
    const long long H = s.rhits[r], base = s.hoff[r];
    wave_lds_sync();                               // the previous read's LDS reads are done
    if (lane < LA && lane < FSLR_MAX_L) {          // (a longer read's rows are read from the columns)
      FSLR_BOUND(o0 + lane, s.nbi);
      qiv[lane] = make_int4(s.qc[o0 + lane], s.qs[o0 + lane], s.qe[o0 + lane], s.qt[o0 + lane]);
    }
    for (int t = lane; t < kSetSlots; t += kWave) {
      key[t] = -1;
      seq[t] = 0x7FFFFFFF;
    }
    wave_lds_sync();
    int nset = 0;
    bool closed = false;
    long long t_close = 0;
    int ncand = 0, ngated = 0, nedges = 0, bst = -1, bI = 0, bU = 1;
    long long nrow = 0;
    for (long long t0 = 0; t0 < H; t0 += kWave) {
      const long long t = t0 + lane;
      bool valid = t < H;
      int p = -1;
      if (valid) {
        FSLR_BOUND(base + t, s.h_cap);
        p = s.hits[base + t];
        valid = p != excl;
      }
      // in the set already: a partner of an earlier batch
      int h = static_cast<int>((static_cast<unsigned>(p) * 2654435761u) >> 23);
      bool found = false;
      if (valid) {
        for (;;) {
          const int kk = key[h];
          if (kk == p) { found = true; break; }
          if (kk == -1) break;
          h = (h + 1) & (kSetSlots - 1);
        }
      }
      bool fresh = false;
      if (!closed) {
        wave_lds_sync();                           // every lane has looked before any lane inserts
        int slot = 0;
        if (valid && !found) {
          for (;;) {
            const int old = atomicCAS(&key[h], -1, p);
            if (old == -1 || old == p) break;
            h = (h + 1) & (kSetSlots - 1);
          }
          slot = h;
          atomicMin(&seq[slot], static_cast<int>(t));
        }
        wave_lds_sync();
        fresh = valid && !found && seq[slot] == static_cast<int>(t);
      } else if (valid && !found) {
        // the set is closed: the first visit iff no earlier hit past the closing point names this partner
        fresh = true;
        for (long long u = t_close; u < t; ++u)
          if (s.hits[base + u] == p) { fresh = false; break; }
      }
      const unsigned long long fm = __ballot(fresh);
      const int nn = __popcll(fm);
      if (!closed) {
        nset += nn;
        if (nset >= kMatchSetCap) {
          closed = true;
          t_close = t0 + kWave;
        }
      }
      if (nn == 0) continue;
      if (fresh) cand[mbcnt(fm)] = p;
      wave_lds_sync();
      // the batch's nn new partners, in visiting order: four side by side, or two, or one
      for (int g0 = 0; g0 < nn; g0 += 4) {
        const int k = g0 + (lane >> 4);
        const bool v = k < nn;
        const CandMeta m = cand_meta<kAny>(s, cand, k, v, q2, qn, res);
        if (v && !m.score && (lane & 15) == 0) res[k] = static_cast<unsigned>(m.gate) << kFlagShift;
        if constexpr (kAny) {
          if (LA > FSLR_MAX_L || __ballot(m.score && m.LB > FSLR_MAX_L) != 0) {
            // a list beyond one wavefront of lanes: the group's candidates one at a time
            for (int q = 0; q < 4 && g0 + q < nn; ++q) {
              const CandMeta m1 = cand_meta<kAny>(s, cand, g0 + q, true, q2, qn, res);
              if (!m1.score) continue;
              if (LA > FSLR_MAX_L || m1.LB > FSLR_MAX_L) {
                int I = 0;
                bool zd = false;
                long_fit(LA, m1.LB, QueryRows{s.qc, s.qs, s.qe, s.qt, o0, s.nbi},
                         ReadList{s.iv, m1.offB, m1.offB2, s.ix.ni}, lane, &I, &zd);
                if (lane == 0) res[g0 + q] = fit_result_any(LA, m1.LB, I, zd, m1.gate, s.pt, s.umax, s.n_umax);
              } else {
                match_groups<64, kAny>(s, qiv, LA, g0 + q, true, m1.offB, m1.LB, m1.gate, lane, res);
              }
            }
            continue;
          }
        }
        const bool w64 = __ballot(m.score && m.LB > 32) != 0;
        const bool w32 = __ballot(m.score && m.LB > 16) != 0;
        if (w64) {
          for (int q = 0; q < 4 && g0 + q < nn; ++q) {
            const CandMeta m1 = cand_meta<kAny>(s, cand, g0 + q, true, q2, qn, res);
            if (m1.score) match_groups<64, kAny>(s, qiv, LA, g0 + q, true, m1.offB, m1.LB, m1.gate, lane, res);
          }
        } else if (w32) {
          for (int q = 0; q < 4 && g0 + q < nn; q += 2) {
            const int k2 = g0 + q + (lane >> 5);
            const CandMeta m2 = cand_meta<kAny>(s, cand, k2, k2 < nn, q2, qn, res);
            match_groups<32, kAny>(s, qiv, LA, k2, m2.score, m2.offB, m2.LB, m2.gate, lane, res);
          }
        } else {
          match_groups<16, kAny>(s, qiv, LA, k, m.score, m.offB, m.LB, m.gate, lane, res);
        }
      }
      wave_lds_sync();
      // lane k takes candidate k: the counts, the best edge, the emitted rows in candidate order
      const bool mine = lane < nn;
      const unsigned rv = mine ? res[lane] : 0u;
      const int pk = mine ? cand[lane] : 0;
      const int fl = kAny ? any_flags(rv) : static_cast<int>(rv >> 16);
      const int ci = kAny ? any_I(rv) : static_cast<int>(rv & 0xff);
      const int cu = kAny ? any_U(rv) : static_cast<int>((rv >> 8) & 0xff);
      ncand += nn;
      ngated += __popcll(__ballot(mine && (fl & FSLR_SCORE_GATE)));
      unsigned long long em = __ballot(mine && (fl & FSLR_SCORE_EDGE));
      nedges += __popcll(em);
      while (em) {
        const int j = __builtin_ctzll(em);
        em &= em - 1;
        const int ei = rdl(ci, j), eu = rdl(cu, j);
        if (bst < 0 || ei * bU > bI * eu) {          // I/U compared exactly; a tie keeps the earlier candidate
          bst = rdl(pk, j);
          bI = ei;
          bU = eu;
        }
      }
      const bool emit = mine && (s.emit_mask == 0 || (static_cast<unsigned>(fl) & s.emit_mask) != 0);
      const unsigned long long om = __ballot(emit);
      if (emit) {
        const long long dst = base + nrow + mbcnt(om);
        FSLR_BOUND(dst, s.h_cap);
        s.stage[dst] = static_cast<unsigned long long>(static_cast<unsigned>(pk)) |
                       (static_cast<unsigned long long>(rv) << 32);
      }
      nrow += __popcll(om);
      wave_lds_sync();                             // cand / res are read before the next batch writes them
    }
    if (lane == 0) {
      s.cnt3[3 * r] = ncand;
      s.cnt3[3 * r + 1] = ngated;
      s.cnt3[3 * r + 2] = nedges;
      s.best[r] = bst;
      s.nrows[r - s.r0] = nrow;
    }
  }
}

__global__ __launch_bounds__(256) void k_match_compact(const long long* __restrict__ hoff,
                                                       const long long* __restrict__ roff,
                                                       const unsigned long long* __restrict__ stage,
                                                       unsigned long long* __restrict__ dense, int r0, int r1,
                                                       long long h_cap) {
  const int lane = threadIdx.x & 63;
  const int nw = gridDim.x * (blockDim.x >> 6);
  for (int r = r0 + blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < r1; r += nw) {
    const long long src = hoff[r], dst = roff[r - r0], n = roff[r - r0 + 1] - dst;
    for (long long t = lane; t < n; t += kWave) {
      FSLR_BOUND(src + t, h_cap);
      FSLR_BOUND(dst + t, h_cap);
      dense[dst + t] = stage[src + t];
    }
  }
}

int ensure_block(fslr_ctx* c, MatchWork* w) {
  if (w->block_ok) return FSLR_OK;
  int rc;
  if ((rc = dalloc(c, &w->rd, 4 * (kBlockReads + 1))) || (rc = dalloc(c, &w->qcol, 4 * kBlockIvs)) ||
      (rc = dalloc(c, &w->span, kBlockIvs)) || (rc = dalloc(c, &w->ivcnt, kBlockIvs)) ||
      (rc = dalloc(c, &w->rhits, kBlockReads)) || (rc = dalloc(c, &w->hoff, kBlockReads)) ||
      (rc = dalloc(c, &w->cnt3, 3 * kBlockReads)) || (rc = dalloc(c, &w->best, kBlockReads)) ||
      (rc = dalloc(c, &w->nrows, kBlockReads + 1)) || (rc = dalloc(c, &w->roff, kBlockReads + 1)) ||
      (rc = dalloc(c, &w->pt, kPassBytes)))
    return rc;
  size_t tb = 0;
  HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, tb, static_cast<long long*>(nullptr),
                                              static_cast<long long*>(nullptr), kBlockReads + 1, c->stream));
  HIP_TRY(c, hipMalloc(&w->temp, std::max<size_t>(tb, 16)));
  w->temp_bytes = tb;
  HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&w->pin), 3 * (kBlockReads + 1) * sizeof(long long),
                           hipHostMallocDefault));
  w->block_ok = true;
  return FSLR_OK;
}

int ensure_hits(fslr_ctx* c, MatchWork* w, int64_t need) {
  if (need <= w->h_cap) return FSLR_OK;
  w->h_cap = 0;                                     // (a failed growth leaves no buffer behind its capacity)
  int rc;
  if ((rc = dalloc(c, &w->hits, need)) || (rc = dalloc(c, &w->stage, need)) || (rc = dalloc(c, &w->dense, need)))
    return rc;
  w->h_cap = need;
  return FSLR_OK;
}

// why this context cannot match (where fslr_search and fslr_score_pairs could not answer), or FSLR_OK
int match_state(fslr_ctx* c, const char* who) {
  if (int rc = search_state(c, who)) return rc;
  if (c->lg_set)
    return fail(c, FSLR_ERR_INVALID, std::string(who) + ": the context holds reads of more than " +
                                         std::to_string(FSLR_MAX_L) + " intervals (virtual reads), which it does not match against");
  return FSLR_OK;
}

// either entry point.  any: fslr_match_reads_any (real ranks, reads of up to FSLR_MAX_ANY_L intervals, umax); the
// <true> kernels and the wide row word only where the context holds virtual reads or a query read exceeds
// FSLR_MAX_L intervals
int match_run(fslr_ctx* c, bool any, const fslr_params* p, const int32_t* umax, int32_t n_umax,
              const fslr_match_queries* q, uint32_t emit_mask, int64_t* row_off, int32_t* counts, int32_t* best,
              int64_t* n_rows) {
  if (!c) return FSLR_ERR_INVALID;
  const std::string who = any ? "fslr_match_reads_any" : "fslr_match_reads";
  if (!p || !p->pass_table) return fail(c, FSLR_ERR_INVALID, who + ": null params or pass_table");
  if (!q) return fail(c, FSLR_ERR_INVALID, who + ": null queries");
  const int64_t nr = q->n_reads;
  if (nr < 0 || q->n_intervals < 0 || q->n_intervals >= (int64_t(1) << 31) - 1)
    return fail(c, FSLR_ERR_INVALID, who + ": read or interval count out of range");
  if (nr && (!q->read_off || !q->read_qlen2 || !q->read_nal))
    return fail(c, FSLR_ERR_INVALID, who + ": null read array");
  if (q->n_intervals && (!q->iv_chrom || !q->iv_start || !q->iv_end || !q->iv_thr))
    return fail(c, FSLR_ERR_INVALID, who + ": null interval array");
  if (int rc = any ? search_state(c, who.c_str()) : match_state(c, who.c_str())) return rc;
  if (nr && (q->read_off[0] < 0 || q->read_off[nr] > q->n_intervals))
    return fail(c, FSLR_ERR_INVALID, who + ": read_off does not lie in [0, n_intervals]");
  const int64_t n_res = any && c->lg_set ? c->lg_n_real : c->n;     // the rank space of exclude and partner
  const int64_t max_l = any ? FSLR_MAX_ANY_L : FSLR_MAX_L;
  int64_t longest = 0;
  for (int64_t r = 0; r < nr; ++r) {
    const int64_t L = static_cast<int64_t>(q->read_off[r + 1]) - q->read_off[r];
    if (L < 0)
      return fail(c, FSLR_ERR_INVALID, who + ": read_off decreases at query read " + std::to_string(r));
    if (L > max_l)
      return fail(c, FSLR_ERR_INVALID, who + ": query read " + std::to_string(r) + " has " +
                                           std::to_string(L) + " intervals (limit " + std::to_string(max_l) + ")");
    longest = std::max(longest, L);
    if (q->exclude && (q->exclude[r] < -1 || q->exclude[r] >= n_res))
      return fail(c, FSLR_ERR_INVALID, who + ": exclude[" + std::to_string(r) + "] = " +
                                           std::to_string(q->exclude[r]) + " is neither -1 nor a rank in [0, " +
                                           std::to_string(n_res) + ")");
  }
  const bool wide = any && (c->lg_set || longest > FSLR_MAX_L);
  HIP_TRY(c, hipSetDevice(c->device));
  if (!c->mtw) c->mtw = new MatchWork();
  MatchWork* w = c->mtw;
  if (wide) {
    // umax must cover I up to the longest resident real read (I <= L2); checked before anything runs
    int need = c->lg_max_len;
    if (!c->lg_set) {
      if (w->short_gen != c->reads_gen || !w->short_max) {
        std::vector<unsigned char> l8(static_cast<size_t>(c->n));
        if (c->n) HIP_TRY(c, hipMemcpy(l8.data(), c->rlen8, l8.size(), hipMemcpyDeviceToHost));
        int m = 0;
        for (unsigned char v : l8) m = std::max<int>(m, v);
        w->short_max = m;
        w->short_gen = c->reads_gen;
      }
      need = w->short_max;
    }
    if (!umax || n_umax < need)
      return fail(c, FSLR_ERR_INVALID, who + ": reads of more than " + std::to_string(FSLR_MAX_L) +
                                           " intervals: umax must cover I up to the longest resident read (" +
                                           std::to_string(need) + ")");
  }
  w->valid = w->timed = false;
  w->any = any, w->wide = wide;
  w->rows.clear();
  for (float& m : w->ms) m = 0;
  auto done = [&]() {
    w->valid = true;
    w->reads_gen = c->reads_gen;
    w->index_gen = c->index_gen;
    if (n_rows) *n_rows = static_cast<int64_t>(w->rows.size());
    return FSLR_OK;
  };
  const int ni = static_cast<int>(c->ni_idx);
  if (nr == 0 || ni == 0) {                         // no query read or no stored interval: no candidate anywhere
    if (row_off) std::fill(row_off, row_off + nr + 1, int64_t(0));
    if (counts) std::fill(counts, counts + 3 * nr, 0);
    if (best) std::fill(best, best + nr, -1);
    return done();
  }
  if (int rc = ensure_bwd_ranges(c)) return rc;     // the tile prefix of end and the (chrom, end) keys, once per index
  if (int rc = ensure_block(c, w)) return rc;
  const bool prof = c->profiling;
  if (prof && !w->ev_ok) {
    for (hipEvent_t& e : w->ev) HIP_TRY(c, hipEventCreate(&e));
    w->ev_ok = true;
  }
  int64_t budget = kBudget;
  // FSLR_MATCH_BUDGET (tests): a small hit budget, so that a small batch spans several chunks
  if (const char* e = std::getenv("FSLR_MATCH_BUDGET")) budget = std::max<int64_t>(1, std::atoll(e));
  hipStream_t st = c->stream;
  MatchArgs s{};
  if (wide) {
    if (n_umax > w->umax_cap) {
      w->umax_cap = 0;
      if (int rc = dalloc(c, &w->umax, n_umax)) return rc;
      w->umax_cap = n_umax;
    }
    HIP_TRY(c, hipMemcpyAsync(w->umax, umax, static_cast<size_t>(n_umax) * sizeof(int), hipMemcpyHostToDevice, st));
    if (!c->lg_perm.empty() && w->perm_gen != c->reads_gen) {
      const int64_t m = static_cast<int64_t>(c->lg_perm.size());
      if (m > w->perm_cap) {
        w->perm_cap = 0;
        if (int rc = dalloc(c, &w->perm, m)) return rc;
        w->perm_cap = m;
      }
      HIP_TRY(c, hipMemcpyAsync(w->perm, c->lg_perm.data(), m * sizeof(int), hipMemcpyHostToDevice, st));
      w->perm_gen = c->reads_gen;
    }
    s.umax = w->umax, s.n_umax = n_umax;
    if (c->lg_set) s.vreal = c->lg_vreal, s.rlen = c->lg_rlen, s.off2 = c->lg_off2;
  }
  // (the old kernels refuse virtual reads and look at no perm)
  s.ix = index_view(c, wide && !c->lg_perm.empty() ? w->perm : nullptr);
  int* rd = w->rd;
  s.roffq = rd, s.qlen2 = rd + (kBlockReads + 1), s.nal = rd + 2 * (kBlockReads + 1), s.excl = rd + 3 * (kBlockReads + 1);
  s.qc = w->qcol, s.qs = w->qcol + kBlockIvs, s.qe = w->qcol + 2 * kBlockIvs, s.qt = w->qcol + 3 * kBlockIvs;
  s.span = w->span, s.ivcnt = w->ivcnt, s.rhits = w->rhits, s.hoff = w->hoff;
  s.iv = c->iv, s.pt = w->pt, s.qcut = p->qlen_cut, s.ncut = p->nal_cut, s.emit_mask = emit_mask;
  s.cnt3 = w->cnt3, s.best = w->best, s.nrows = w->nrows;
  long long *pin_hits = w->pin, *pin_hoff = w->pin + (kBlockReads + 1), *pin_roff = w->pin + 2 * (kBlockReads + 1);
  // seg: 0 upload, 1 search, 2 dedupe + score, 3 download; events ev[2 seg], ev[2 seg + 1], read after a sync
  bool rec[4] = {false, false, false, false};
  auto mark = [&](int seg, int end) -> hipError_t {
    if (!prof) return hipSuccess;
    rec[seg] = true;
    return hipEventRecord(w->ev[2 * seg + end], st);
  };
  auto collect = [&]() -> hipError_t {
    for (int seg = 0; seg < 4; ++seg)
      if (rec[seg]) {
        float ms = 0;
        if (hipError_t e = hipEventElapsedTime(&ms, w->ev[2 * seg], w->ev[2 * seg + 1])) return e;
        w->ms[seg] += ms;
        rec[seg] = false;
      }
    return hipSuccess;
  };
  HIP_TRY(c, hipMemcpyAsync(w->pt, p->pass_table, kPassBytes, hipMemcpyHostToDevice, st));
  for (int64_t b0 = 0; b0 < nr;) {
    int64_t b1 = b0;
    while (b1 < nr && b1 - b0 < kBlockReads && q->read_off[b1 + 1] - q->read_off[b0] <= kBlockIvs) ++b1;
    const int m = static_cast<int>(b1 - b0);
    const int iv0 = q->read_off[b0], nbi = q->read_off[b1] - iv0;
    HIP_TRY(c, mark(0, 0));
    HIP_TRY(c, hipMemcpyAsync(rd, q->read_off + b0, (m + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(rd + (kBlockReads + 1), q->read_qlen2 + b0, m * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(rd + 2 * (kBlockReads + 1), q->read_nal + b0, m * sizeof(int), hipMemcpyHostToDevice, st));
    if (q->exclude)
      HIP_TRY(c, hipMemcpyAsync(rd + 3 * (kBlockReads + 1), q->exclude + b0, m * sizeof(int), hipMemcpyHostToDevice, st));
    else
      HIP_TRY(c, hipMemsetAsync(rd + 3 * (kBlockReads + 1), 0xff, m * sizeof(int), st));
    if (nbi) {
      const size_t ib = static_cast<size_t>(nbi) * sizeof(int);
      HIP_TRY(c, hipMemcpyAsync(w->qcol, q->iv_chrom + iv0, ib, hipMemcpyHostToDevice, st));
      HIP_TRY(c, hipMemcpyAsync(w->qcol + kBlockIvs, q->iv_start + iv0, ib, hipMemcpyHostToDevice, st));
      HIP_TRY(c, hipMemcpyAsync(w->qcol + 2 * kBlockIvs, q->iv_end + iv0, ib, hipMemcpyHostToDevice, st));
      HIP_TRY(c, hipMemcpyAsync(w->qcol + 3 * kBlockIvs, q->iv_thr + iv0, ib, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(c, mark(0, 1));
    s.ivbase = iv0, s.nbi = nbi, s.r0 = 0, s.r1 = m;
    HIP_TRY(c, mark(1, 0));
    k_match_count<<<wave_grid(m), 256, 0, st>>>(s);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, mark(1, 1));
    HIP_TRY(c, hipMemcpyAsync(pin_hits, w->rhits, m * sizeof(long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    HIP_TRY(c, collect());
    // the block's chunks: consecutive reads whose hits fit the budget, at least one read each
    std::vector<int> cuts{0};
    int64_t sum = 0, need = 1;
    for (int r = 0; r < m; ++r) {
      if (pin_hits[r] >= (int64_t(1) << 31) - kWave)
        return fail(c, FSLR_ERR_NOMEM, who + ": query read " + std::to_string(b0 + r) + " has " +
                                           std::to_string(pin_hits[r]) + " hits (limit 2^31)");
      if (r > cuts.back() && sum + pin_hits[r] > budget) {
        cuts.push_back(r);
        sum = 0;
      }
      pin_hoff[r] = sum;
      sum += pin_hits[r];
      need = std::max(need, sum);
    }
    cuts.push_back(m);
    if (int rc = ensure_hits(c, w, need)) return rc;
    s.hits = w->hits, s.stage = w->stage, s.h_cap = w->h_cap;
    HIP_TRY(c, hipMemcpyAsync(w->hoff, pin_hoff, m * sizeof(long long), hipMemcpyHostToDevice, st));
    for (size_t k = 0; k + 1 < cuts.size(); ++k) {
      const int r0 = cuts[k], r1 = cuts[k + 1], mc = r1 - r0;
      s.r0 = r0, s.r1 = r1;
      HIP_TRY(c, mark(1, 0));
      if (wide)
        k_match_fill<true><<<wave_grid(mc), 256, 0, st>>>(s);
      else
        k_match_fill<false><<<wave_grid(mc), 256, 0, st>>>(s);
      HIP_TRY(c, hipGetLastError());
      HIP_TRY(c, mark(1, 1));
      HIP_TRY(c, mark(2, 0));
      HIP_TRY(c, hipMemsetAsync(w->nrows + mc, 0, sizeof(long long), st));
      if (wide)
        k_match_score<true><<<wave_grid(mc), 256, 0, st>>>(s);
      else
        k_match_score<false><<<wave_grid(mc), 256, 0, st>>>(s);
      HIP_TRY(c, hipGetLastError());
      size_t tb = w->temp_bytes;
      HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(w->temp, tb, w->nrows, w->roff, mc + 1, st));
      k_match_compact<<<wave_grid(mc), 256, 0, st>>>(w->hoff, w->roff, w->stage, w->dense, r0, r1, w->h_cap);
      HIP_TRY(c, hipGetLastError());
      HIP_TRY(c, mark(2, 1));
      HIP_TRY(c, hipMemcpyAsync(pin_roff, w->roff, (mc + 1) * sizeof(long long), hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipStreamSynchronize(st));
      HIP_TRY(c, collect());
      const size_t have = w->rows.size(), add = static_cast<size_t>(pin_roff[mc]);
      if (row_off)
        for (int r = 0; r < mc; ++r) row_off[b0 + r0 + r] = static_cast<int64_t>(have) + pin_roff[r];
      if (add) {
        w->rows.resize(have + add);
        HIP_TRY(c, mark(3, 0));
        HIP_TRY(c, hipMemcpyAsync(w->rows.data() + have, w->dense, add * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, mark(3, 1));
        HIP_TRY(c, hipStreamSynchronize(st));
        HIP_TRY(c, collect());
      }
    }
    HIP_TRY(c, mark(3, 0));
    if (counts) HIP_TRY(c, hipMemcpyAsync(counts + 3 * b0, w->cnt3, 3 * m * sizeof(int), hipMemcpyDeviceToHost, st));
    if (best) HIP_TRY(c, hipMemcpyAsync(best + b0, w->best, m * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, mark(3, 1));
    HIP_TRY(c, hipStreamSynchronize(st));
    HIP_TRY(c, collect());
    b0 = b1;
  }
  if (row_off) row_off[nr] = static_cast<int64_t>(w->rows.size());
  w->timed = prof;
  return done();
}

// the saved batch of one entry point's kind, unpacked
int rows_out(fslr_ctx* c, bool any, int32_t* partner, int32_t* I, int32_t* U, uint8_t* flags, int64_t capacity) {
  if (!c) return FSLR_ERR_INVALID;
  const std::string who = any ? "fslr_match_rows_any" : "fslr_match_rows";
  const std::string first = any ? "fslr_match_reads_any" : "fslr_match_reads";
  MatchWork* w = c->mtw;
  if (!w || !w->valid || w->any != any || w->reads_gen != c->reads_gen || w->index_gen != c->index_gen)
    return fail(c, FSLR_ERR_STATE, who + ": " + first + " first (on these reads and this index build)");
  if (int rc = any ? search_state(c, who.c_str()) : match_state(c, who.c_str())) return rc;
  const int64_t total = static_cast<int64_t>(w->rows.size());
  if (capacity < total)
    return fail(c, FSLR_ERR_INVALID, who + ": capacity " + std::to_string(capacity) + " < " +
                                         std::to_string(total) + " rows");
  if (total == 0) return FSLR_OK;
  if (!partner || !I || !U || !flags) return fail(c, FSLR_ERR_INVALID, who + ": null array");
  for (int64_t k = 0; k < total; ++k) {
    const unsigned long long v = w->rows[k];
    partner[k] = static_cast<int32_t>(v & 0xffffffffull);
    if (w->wide)
      fit_unpack_any(static_cast<unsigned>(v >> 32), &I[k], &U[k], &flags[k]);
    else
      fit_unpack(static_cast<unsigned>(v >> 32), &I[k], &U[k], &flags[k]);
  }
  return FSLR_OK;
}

}  // namespace

extern "C" {

int fslr_match_reads(fslr_ctx* c, const fslr_params* p, const fslr_match_queries* q, uint32_t emit_mask,
                     int64_t* row_off, int32_t* counts, int32_t* best, int64_t* n_rows) {
  return match_run(c, false, p, nullptr, 0, q, emit_mask, row_off, counts, best, n_rows);
}

int fslr_match_reads_any(fslr_ctx* c, const fslr_params* p, const int32_t* umax, int32_t n_umax,
                         const fslr_match_queries* q, uint32_t emit_mask, int64_t* row_off, int32_t* counts,
                         int32_t* best, int64_t* n_rows) {
  return match_run(c, true, p, umax, n_umax, q, emit_mask, row_off, counts, best, n_rows);
}

int fslr_match_rows(fslr_ctx* c, int32_t* partner, int32_t* I, int32_t* U, uint8_t* flags, int64_t capacity) {
  return rows_out(c, false, partner, I, U, flags, capacity);
}

int fslr_match_rows_any(fslr_ctx* c, int32_t* partner, int32_t* I, int32_t* U, uint8_t* flags, int64_t capacity) {
  return rows_out(c, true, partner, I, U, flags, capacity);
}

int fslr_match_timings(fslr_ctx* c, float* ms) {
  if (!c || !ms) return FSLR_ERR_INVALID;
  MatchWork* w = c->mtw;
  if (!w || !w->timed)
    return fail(c, FSLR_ERR_STATE, "fslr_match_timings: no profiled fslr_match_reads (fslr_set_profiling 1 or 2)");
  for (int t = 0; t < 4; ++t) ms[t] = w->ms[t];
  return FSLR_OK;
}

}  // extern "C"
