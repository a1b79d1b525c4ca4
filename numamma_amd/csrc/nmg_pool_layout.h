// nmg_pool_layout.h -- where the route pass's workgroup pools lie in the chunk
// pool (DESIGN.md "The chunk claim").  Plain C++, no HIP: the host engine and
// tests/c/nmg_pool_layout_host.cpp include it.
//
// The chunk pool is a set of equally sized pieces of 2^K chunks, each piece a
// device allocation of its own.  Chunk ids are global: chunk id lives in
// piece id >> K at chunk id & (2^K - 1).  A workgroup stores through one base
// pointer, so its private id range must lie inside one piece.
#pragma once

#include <cstdint>

namespace nmg {

constexpr uint32_t kPieceLog2 = 16;   // chunks per piece, log2: 64 MiB of 1 KiB chunks

// smallest K with cap <= 2^K
inline uint32_t pool_min_log2(uint64_t cap) {
  uint32_t K = 0;
  while (K < 63 && (1ull << K) < cap) K++;
  return K;
}

// c0[0..n]: workgroup w owns the ids [c0[w], c0[w + 1]), at least cap[w] of
// them, all of one piece: a range that would cross a piece boundary starts at
// the boundary instead, and the ids skipped fall to the workgroup before it.
// *pieces = pieces that hold the ids below c0[n].  False, with nothing
// promised of the outputs, when a capacity is larger than a piece or the ids
// reach `limit`.
inline bool pool_layout(const uint64_t* cap, uint32_t n, uint32_t K, uint64_t limit, uint32_t* c0, uint32_t* pieces) {
  if (K > 31 || limit > (1ull << 32)) return false;
  const uint64_t piece = 1ull << K;
  uint64_t tot = 0;
  for (uint32_t w = 0; w < n; w++) {
    if (cap[w] > piece) return false;
    if (cap[w] && (tot >> K) != ((tot + cap[w] - 1) >> K)) tot = ((tot >> K) + 1) << K;
    if (tot + cap[w] >= limit) return false;
    c0[w] = (uint32_t)tot;
    tot += cap[w];
  }
  if (tot >= limit) return false;
  c0[n] = (uint32_t)tot;
  *pieces = (uint32_t)((tot + piece - 1) >> K);
  return true;
}

}  // namespace nmg
