// any_idx.hpp — the index arithmetic of fslr_append_reads_any / fslr_remove_reads_any (any.hip)
// as plain functions of their arguments, for the host and the device alike.
//
// The virtual layout (fslr_set_reads_any): with n real reads and V virtual ones, virtual reads [0, n) are the
// real reads' first chunks and [n, V) the further chunks of the long reads; the CSR rows follow the same two
// groups, the first chunks' rows in [0, o1) and the further chunks' in [o1, ni).  Appending m real reads with
// e further chunks, mi1 first-chunk intervals and mi intervals in all gives four groups, in rank and in rows:
//   resident first chunks   ranks [0, n)            rows [0, o1)
//   batch first chunks      ranks [n, n + m)        rows [o1, o1 + mi1)
//   resident further chunks ranks [n + m, V + m)    rows [o1 + mi1, ni + mi1)
//   batch further chunks    ranks [V + m, V + m + e) rows [ni + mi1, ni + mi)
// Nothing here touches memory, and no function loops.
#pragma once
#include <cstdint>

#include "fslr_hip.h"

#if defined(__HIPCC__)
#define FSLR_ANY_HD __host__ __device__
#else
#define FSLR_ANY_HD
#endif

namespace fslr {
namespace anyidx {

// the shape of one append: what is resident (n, V, o1, ni) and what arrives (m, e, mi1, mi)
struct Shape {
  int n, V, o1, ni;
  int m, e, mi1, mi;
};

// the new virtual rank of resident virtual read v
FSLR_ANY_HD inline int new_vrank(int v, int n, int m) { return v < n ? v : v + m; }

// a resident data-order tag `read << 6 | j` in the new numbering
FSLR_ANY_HD inline int retag(int tag, int n, int m) { return (tag >> 6) < n ? tag : tag + (m << 6); }

// the new CSR offset of resident CSR row k
FSLR_ANY_HD inline int new_row(int k, int o1, int mi1) { return k < o1 ? k : k + mi1; }

// off2 (the CSR offset of a long read's first further chunk) of a resident long read after the append ...
FSLR_ANY_HD inline int off2_resident(int off2, int mi1) { return off2 + mi1; }
// ... and of a batch read whose earlier batch reads hold `before` further-chunk intervals
FSLR_ANY_HD inline int off2_batch(int ni, int mi1, int before) { return ni + mi1 + before; }

// Where new virtual rank u comes from: the resident virtual read (>= 0), or ~b for the batch's virtual read b
// (the batch numbers its m first chunks 0 .. m-1 and its further chunks m .. m+e-1).
FSLR_ANY_HD inline int rank_source(int u, const Shape& s) {
  if (u < s.n) return u;
  if (u < s.n + s.m) return ~(u - s.n);
  if (u < s.V + s.m) return u - s.m;
  return ~(u - s.V);
}

// Where new CSR row k comes from: the resident row (>= 0), or ~b for row b of the batch's virtual CSR.
FSLR_ANY_HD inline int row_source(int k, const Shape& s) {
  if (k < s.o1) return k;
  if (k < s.o1 + s.mi1) return ~(k - s.o1);
  if (k < s.ni + s.mi1) return k - s.mi1;
  return ~(k - s.ni);
}

// further chunks of a read of L intervals
FSLR_ANY_HD inline int extra_chunks(int L) { return (L + FSLR_MAX_L - 1) / FSLR_MAX_L - 1; }

}  // namespace anyidx
}  // namespace fslr
