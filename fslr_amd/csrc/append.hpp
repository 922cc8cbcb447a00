// append.hpp — fslr_append_reads' work area (append.hip).  fslr_remove_reads (remove.hip) compacts the data order
// into the same second set of data-order buffers and swaps it in the same way: one spare set per context.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

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
};
