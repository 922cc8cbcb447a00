// any_idx.hpp on the host: prints, for the Shape given as eight arguments (n V o1 ni m e mi1 mi), every value of
// the append's index arithmetic, one table per line; further arguments "r<off2>" / "b<before>" print off2_resident
// / off2_batch.  tests/test_append_any_ref.py compiles this and compares the tables with tests/append_any_ref.py.
#include <cstdio>
#include <cstdlib>

#include "any_idx.hpp"

using namespace fslr::anyidx;

int main(int argc, char** argv) {
  if (argc < 9) return 2;
  Shape s{};
  int* f[8] = {&s.n, &s.V, &s.o1, &s.ni, &s.m, &s.e, &s.mi1, &s.mi};
  for (int k = 0; k < 8; ++k) *f[k] = std::atoi(argv[1 + k]);
  std::printf("new_vrank");
  for (int v = 0; v < s.V; ++v) std::printf(" %d", new_vrank(v, s.n, s.m));
  std::printf("\nretag");
  for (int v = 0; v < s.V; ++v) std::printf(" %d", retag((v << 6) | (v & 63), s.n, s.m));
  std::printf("\nnew_row");
  for (int k = 0; k < s.ni; ++k) std::printf(" %d", new_row(k, s.o1, s.mi1));
  std::printf("\nrank_source");
  for (int u = 0; u < s.V + s.m + s.e; ++u) std::printf(" %d", rank_source(u, s));
  std::printf("\nrow_source");
  for (int k = 0; k < s.ni + s.mi; ++k) std::printf(" %d", row_source(k, s));
  std::printf("\noff2");
  for (int a = 9; a < argc; ++a) {
    const int x = std::atoi(argv[a] + 1);
    std::printf(" %d", argv[a][0] == 'r' ? off2_resident(x, s.mi1) : off2_batch(s.ni, s.mi1, x));
  }
  std::printf("\nextra_chunks");
  for (int L = 1; L <= 4096; ++L) std::printf(" %d", extra_chunks(L));
  std::printf("\n");
  return 0;
}
