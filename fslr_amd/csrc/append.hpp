// append.hpp — fslr_append_reads' work area (append.hip).  fslr_remove_reads (remove.hip) compacts the data order
// into the same second set of data-order buffers and swaps it in the same way: one spare set per context.
// fslr_append_reads_any / fslr_remove_reads_any (any.hip) run the same two calls over virtual reads: what they
// add to them is declared here too.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "any_idx.hpp"
#include "fslr_hip.h"

struct AppendWork {
  int* cols = nullptr;               // the batch's columns as copied: off, qlen2, nal | chrom, start, end, thr, data_pos
  int64_t cols_cap = 0;
  int4* rmeta = nullptr;             // [m] packed reads (ranks n .., offsets ni ..)
  unsigned char* rlen8 = nullptr;
  int64_t m_cap = 0;
  int4* iv = nullptr;                // [mi] packed intervals, the batch's CSR order
  int* inv = nullptr;                // [mi] data position -> CSR index (the permutation check)
  unsigned* dch = nullptr;           // [mi] the batch's own start-sorted data list
  int4* drc = nullptr;
  int2* dgt = nullptr;
  int64_t mi_cap = 0;
  unsigned long long* w64 = nullptr; // [n_chroms + 2] intervals per chromosome, first failures
  int64_t w64_cap = 0;
  unsigned* alt_ch = nullptr;        // the second set of data-order buffers (merge output; swapped with the context's)
  int4* alt_rec = nullptr;
  int2* alt_gate = nullptr;
  int64_t alt_cap = 0;
  hipEvent_t ev[5] = {};             // start | uploaded | packed | merge start | merge end
  bool ev_ok = false, timed = false;
  float ms[4] = {0, 0, 0, 0};        // upload, validate + pack, merge, total
  // fslr_append_reads_any / fslr_remove_reads_any
  int* maps = nullptr;               // the batch's maps as copied: vreal, vbase [m + e] | rlen, off2 [m]
  int64_t maps_cap = 0;
  unsigned char* rl_out = nullptr;   // [virtual reads] the relocated read lengths (copied back on the stream)
  int64_t rl_cap = 0;
  std::vector<int> rlen_host;        // the resident real reads' lengths, valid while rlen_ok and rlen_gen == reads_gen
  uint64_t rlen_gen = 0;
  bool rlen_ok = false;
};

namespace fslr {

// What fslr_append_reads_any adds to an append (any.hip makes it on the host from the batch's real CSR): the
// batch arrives as a virtual CSR of m first chunks followed by e further chunks.
struct AnyPlan {
  anyidx::Shape s;
  const int32_t* b_vreal;            // [m + e] the batch's real read (0 .. m-1) of each of its virtual reads
  const int32_t* b_vbase;            // [m + e] index of its first interval in that read
  const int32_t* b_rlen;             // [m] the batch's real lengths
  const int32_t* b_off2;             // [m] new CSR offset of a long batch read's first further chunk (else 0)
  const int* b_perm;                 // [mi] the batch's virtual interval -> its real interval
  int max_len;                       // the longest real read of the union
};

// The relocation of a virtual resident set around a batch (any.hip): every output goes to a buffer no input
// lives in.  vreal / vbase / rlen / off2 null: the resident reads are plain (virtual read v is real read v).
struct AnyReloc {
  anyidx::Shape s;
  const int4* rmeta;
  const unsigned char* rlen8;
  const int4* iv;
  const int* data_pos;
  const int *vreal, *vbase, *rlen, *off2;
  const int4* b_rmeta;               // the batch as upload.hip packed it (ranks and offsets in the new numbering)
  const unsigned char* b_rlen8;
  const int4* b_iv;
  const int* b_dp;                   // [mi] the batch's own data positions (its virtual CSR order)
  const int *b_vreal, *b_vbase, *b_rlen, *b_off2;
  const int* newpos;                 // k_append_merge's: merged position of resident d, of the batch's ni + e
  int4* rmeta_out;
  unsigned char* rlen8_out;
  int4* iv_out;
  int* dp_out;
  int *vreal_out, *vbase_out, *rlen_out, *off2_out;
};
hipError_t launch_any_relocate(const AnyReloc& a, hipStream_t s);

// fslr_append_reads (plan null, today's bytes) and fslr_append_reads_any's device route (append.hip)
int append_core(fslr_ctx* c, const fslr_reads* r, const AnyPlan* plan, const char* who);
// fslr_remove_reads and, over the virtual reads (virt: keep and n are theirs), fslr_remove_reads_any's compaction
// (remove.hip); new_rank takes the first n_rank entries of the map
int remove_core(fslr_ctx* c, int64_t n, const uint8_t* keep, int32_t* new_rank, int64_t n_rank, const char* who, bool virt);
// the device rank map (old virtual rank -> new, -1 removed) of the last remove_core that removed something
const int* remove_rank_map(fslr_ctx* c);
// a profiled removal's last event again, after kernels launched behind the compaction: their time counts into
// the compaction phase and the total
int remove_extend_timings(fslr_ctx* c);
// the states the appends / the removals refuse (FSLR_ERR_STATE, named); virt: virtual reads made by fslr_set_reads_any pass
int append_state(fslr_ctx* c, const std::string& who, bool virt);
int remove_state(fslr_ctx* c, const std::string& who, bool virt);
// what is half written after a device failure is not a set of reads
int reads_broken(fslr_ctx* c, int rc);

}  // namespace fslr
