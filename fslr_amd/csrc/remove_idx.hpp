// remove_idx.hpp — the index arithmetic of fslr_remove_reads (remove.hip) as plain functions
// of their arguments, for the host and the device alike: where a tile begins, where a survivor lands, what a
// kept read's record becomes.  Nothing here touches memory except owner_of's reads of the array it is given,
// and no loop's trip count depends on anything but an argument.
#pragma once
#include <cstdint>

#include "fslr_hip.h"

#if defined(__HIPCC__)
#define FSLR_HD __host__ __device__
#else
#define FSLR_HD
#endif

namespace fslr {
namespace rm {

constexpr int kTile = FSLR_REMOVE_TILE;   // data positions per tile of the data-order compaction
constexpr int kReadTile = 256;            // reads per tile of the read maps and of the CSR-order compaction
constexpr int kWaveLanes = 64;
constexpr int kSteps = kTile / 256;       // 64-lane steps of one wave over its quarter of a tile
constexpr int kOwnerSteps = 8;            // halvings that take a range of kReadTile reads down to one

FSLR_HD inline long long tiles_of(long long count, int tile) { return (count + tile - 1) / tile; }

// elements of tile `tile` of `count` elements (the last one may be partial; past the end: none)
FSLR_HD inline int tile_len(long long count, long long tile, int size) {
  const long long left = count - tile * size;
  return left <= 0 ? 0 : static_cast<int>(left < size ? left : size);
}

// the element of a data tile that lane `lane` of wave `wave` takes in step `step`: a wave owns 256 consecutive
// elements and walks them 64 at a time, so the survivors' order is (wave, step, lane)
FSLR_HD inline int tile_element(int wave, int step, int lane) { return wave * (kSteps * kWaveLanes) + step * kWaveLanes + lane; }

// survivors of one 64-lane step below `lane` (what mbcnt gives on the device)
FSLR_HD inline int survivors_below(unsigned long long mask, int lane) {
  return __builtin_popcountll(mask & ((1ull << lane) - 1ull));
}

// new data position of a survivor: the tile's base (kept elements of every lower tile), the kept elements of
// the tile's earlier steps, the kept lanes below it in its own step
FSLR_HD inline int survivor_pos(int tile_base, int kept_before_step, int kept_lanes_below) {
  return tile_base + kept_before_step + kept_lanes_below;
}

// a data-order record's tag `read << 6 | j` under the new rank
FSLR_HD inline int retag(int tag, int new_rank) { return (new_rank << 6) | (tag & 63); }

// new CSR index of interval k of a kept read whose intervals began at old_off and now begin at new_off
FSLR_HD inline int new_csr_index(int new_off, int old_off, int k) { return new_off + (k - old_off); }

// the read that owns CSR interval k among `count` reads with ascending first offsets off[0 .. count): the
// largest t with off[t] <= k (the caller guarantees off[0] <= k).  At most `steps` halvings; an empty range
// returns -1 without one.
FSLR_HD inline int owner_of(const int* off, int count, int k, int steps) {
  if (count <= 0) return -1;
  int lo = 0, hi = count;
  for (int s = 0; s < steps && hi - lo > 1; ++s) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= k) lo = mid;
    else hi = mid;
  }
  return lo;
}

}  // namespace rm
}  // namespace fslr
