// nmg_placement.hip -- NUMA placement blocks on the device: the fold and block
// kernels, their launchers (nmg_kernels.h) and the C-ABI calls that run them
// (nmg_count_object_blocks, nmg_get_object_blocks, nmg_report_placement).  The
// rule, the file format and the differences from the reference's
// scripts/counters_to_binding.py are in include/numamma_gpu.h; the host
// statement of the same rule and the writer are in nmg_report.cpp.
//
// The kernels read the page histogram (with NMG_PLACE_HUGE the sparse table
// too) and write arrays of their own: the analysis kernels and their launch
// code are not involved.
#include "nmg_engine_impl.h"

#include <rocprim/device/device_radix_sort.hpp>  // (after <cstring>; this translation unit only)
#include <tuple>

namespace nmg {

// ---------------------------------------------------------------------------
// Fold: one lane per group page.  The nodes in ascending order, within a node
// the group's members and that node's threads; only the running sum, the best
// sum and its node live in registers (a gather: no atomics, no [page][node]
// intermediate).  For a fixed (member, thread) the lanes of a wave that share
// the group read consecutive cells.  Every index stays inside the histogram:
// pg < m_np[m], and the host checks m_base[m] + m_np[m] <= hist_cells and
// thr[k] < T.  CELL: u32 folds the page histogram, u64 the page cost cells,
// which lie at the same index.
template <class CELL>
__global__ __launch_bounds__(256) void place_fold_kernel(PlaceParams p, const CELL* cells, uint64_t pages) {
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < pages; i += gridDim.x * 256ull) {
    // the group g with pg_off[g] <= i < pg_off[g + 1] (i < pages = pg_off[G])
    uint32_t g = 0, len = p.G;
    while (len > 1) {
      const uint32_t half = len >> 1;
      if (p.pg_off[g + half] <= i) {
        g += half;
        len -= half;
      } else {
        len = half;
      }
    }
    const uint32_t pg = (uint32_t)(i - p.pg_off[g]);
    const uint32_t m0 = p.m_off[g], m1 = p.m_off[g + 1];
    uint64_t best = 0;
    uint32_t node = 0;
    for (uint32_t n = 0; n < p.N; n++) {
      const uint32_t k0 = p.node_off[n], k1 = p.node_off[n + 1];
      if (k0 == k1) continue;
      uint64_t s = 0;
      for (uint32_t m = m0; m < m1; m++) {
        if (pg >= p.m_np[m]) continue;
        const CELL* cell = cells + p.m_base[m] + pg;
        for (uint32_t k = k0; k < k1; k++) s += cell[uint64_t(p.thr[k]) * p.hist_cells];
      }
      if (s > best) {  // (strict: the lowest node on a tie)
        best = s;
        node = n;
      }
    }
    p.pv_cnt[i] = best;
    p.pv_node[i] = best > p.D ? (uint8_t)node : (uint8_t)kPlaceNoNode;
  }
}

// ---------------------------------------------------------------------------
// Blocks: one wave per group, 64 pages per step.  A ballot gives the
// qualifying lanes; a lane's previous qualifying page is the highest set bit
// below it, whose node a shuffle fetches, or the last qualifying node of the
// steps before (`last`, wave-uniform).  A qualifying lane whose node differs
// starts a block.  EMIT == false counts the starts per group; after their
// scan EMIT == true writes the rows: the start lane writes (group, node,
// start), and end and count are reduced over each block's lanes of the step
// (a segmented scan keyed by the block's index) and added by the segment's
// last lane -- one atomic max and one atomic add per block and step, on rows
// zeroed before the launch.
template <bool EMIT>
__global__ __launch_bounds__(256) void place_blocks_kernel(PlaceParams p) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t nw = gridDim.x * (blockDim.x / 64);
  for (uint32_t g = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64; g < p.G; g += nw) {
    const uint64_t i0 = p.pg_off[g];
    const uint32_t R = (uint32_t)(p.pg_off[g + 1] - i0);
    const uint64_t o = EMIT ? p.boff[g] : 0;
    uint32_t last = kPlaceNoNode, nb = 0;
    for (uint32_t s0 = 0; s0 < R; s0 += 64) {
      const uint32_t pg = s0 + lane;
      const uint32_t node = pg < R ? (uint32_t)p.pv_node[i0 + pg] : kPlaceNoNode;
      const bool q = node != kPlaceNoNode;
      const uint64_t qm = __ballot(q);
      const uint64_t below = qm & ((1ull << lane) - 1);
      const uint32_t pnode = (uint32_t)__shfl((int)node, below ? 63 - __clzll(below) : 0, 64);
      const bool start = q && node != (below ? pnode : last);
      const uint64_t sm = __ballot(start);
      if (EMIT) {
        // the block a lane belongs to: the starts at or below it (of every step so far)
        const uint32_t k = nb + (uint32_t)__popcll(sm & (lane == 63 ? ~0ull : (2ull << lane) - 1));
        uint64_t cnt = q ? p.pv_cnt[i0 + pg] : 0ull;
        uint32_t end = q ? pg : 0u;
        for (int d = 1; d < 64; d <<= 1) {
          const uint64_t c2 = __shfl_up(cnt, d, 64);
          const uint32_t e2 = (uint32_t)__shfl_up((int)end, d, 64), k2 = (uint32_t)__shfl_up((int)k, d, 64);
          if ((int)lane >= d && k2 == k) {
            cnt += c2;
            end = max(end, e2);
          }
        }
        const uint32_t knext = (uint32_t)__shfl_down((int)k, 1, 64);
        if (k) {  // (k == 0: no block yet)
          uint64_t* r = p.rows + (o + k - 1) * 5;
          if (start) {
            r[0] = p.gid[g];
            r[1] = node;
            r[2] = pg;
          }
          // (a qualifying page counts more than D >= 0: cnt == 0 is a segment without one)
          if ((lane == 63 || knext != k) && cnt) {
            atomicMax(reinterpret_cast<unsigned long long*>(r + 3), (unsigned long long)end);
            atomicAdd(reinterpret_cast<unsigned long long*>(r + 4), (unsigned long long)cnt);
          }
        }
      }
      nb += (uint32_t)__popcll(sm);
      if (qm) last = (uint32_t)__shfl((int)node, 63 - __clzll(qm), 64);
    }
    if (!EMIT && lane == 0) p.bcnt[g] = nb;
  }
}

// ---------------------------------------------------------------------------
// NMG_PLACE_HUGE: the groups with a sparse member, from their touched pages
// (PlaceHugeParams, nmg_kernels.h).  No kernel below waits for another lane
// or workgroup, and every loop ends at a count passed at launch.

// Extract: one lane per slot of the sparse table (SPARSE), or per (thread,
// cell) of the huge groups' dense members.  A non-zero cell of a member, on a
// page below the member's limit, is an item; the items of a wave are appended
// with one atomic.  keys == null: the items are only counted.  COST: the
// cells are the page cost cells (NMG_PLACE_PAGE_COST on an engine with
// NMG_COST_SCOPE_ALL) -- a slot's sparse cost cell, a dense member's cost cell
// at the histogram's index -- in instances of their own.
template <bool SPARSE, bool COST>
__global__ __launch_bounds__(256) void place_huge_extract_kernel(PlaceHugeParams p, uint64_t total) {
  const uint32_t lane = threadIdx.x & 63;
  for (uint64_t i0 = blockIdx.x * 256ull + (threadIdx.x & ~63u); i0 < total; i0 += gridDim.x * 256ull) {
    const uint64_t i = i0 + lane;
    bool has = false;
    uint64_t key = 0, val = 0;
    if (i < total) {
      if (SPARSE) {
        const uint64_t k = p.sparse_keys[i];
        const uint32_t sidx = sparse_key_idx(k), th = sparse_key_thread(k), page = sparse_key_page(k);
        if (k != kEmpty64 && sidx < p.nsent && th < p.T) {
          const uint32_t rank = p.s_rank[sidx];
          val = COST ? p.sparse_cost[i] : (uint64_t)p.sparse_vals[i];
          has = rank != kEmpty32 && page < p.s_lim[sidx] && val != 0;
          key = (uint64_t(rank) << kPlaceRankShift) | (uint64_t(page) << kPlaceNodeBits) | p.tnode[th];
        }
      } else {
        const uint32_t th = (uint32_t)(i / p.dcells);  // (< T: total = T * dcells)
        const uint64_t c = i % p.dcells;
        // the member d with dm_off[d] <= c < dm_off[d + 1] (c < dcells = dm_off[DM]; no member is empty)
        uint32_t d = 0, len = p.DM;
        while (len > 1) {
          const uint32_t half = len >> 1;
          if (p.dm_off[d + half] <= c) {
            d += half;
            len -= half;
          } else {
            len = half;
          }
        }
        const uint64_t page = c - p.dm_off[d];
        const uint64_t cell = uint64_t(th) * p.hist_cells + p.dm_base[d] + page;
        val = COST ? p.cost[cell] : (uint64_t)p.hist[cell];
        has = val != 0;
        key = (uint64_t(p.dm_rank[d]) << kPlaceRankShift) | (page << kPlaceNodeBits) | p.tnode[th];
      }
    }
    const uint64_t mask = __ballot(has);
    if (!mask) continue;  // (wave-uniform)
    const int leader = __ffsll((unsigned long long)mask) - 1;
    unsigned long long at = 0;
    if ((int)lane == leader) at = atomicAdd(p.n_items, (unsigned long long)__popcll(mask));
    at = __shfl(at, leader, 64) + (unsigned long long)__popcll(mask & ((1ull << lane) - 1));
    if (has && p.keys && at < p.cap) {
      p.keys[at] = key;
      p.vals[at] = val;
    }
  }
}

// Reduce: the sorted items of one (rank, page) are consecutive, their nodes
// ascending.  The first of them (the head) walks to the end of its page --
// at most n steps -- summing each node's items: the largest sum and, the
// comparison strict, the lowest node that has it.
__global__ __launch_bounds__(256) void place_huge_reduce_kernel(PlaceHugeParams p, uint64_t n) {
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += gridDim.x * 256ull) {
    const uint64_t gp = p.skeys[i] >> kPlaceNodeBits;
    uint32_t q = 0;
    if (i == 0 || (p.skeys[i - 1] >> kPlaceNodeBits) != gp) {
      uint64_t best = 0, sum = 0;
      uint32_t node = 0, cur = (uint32_t)(p.skeys[i] & 63);
      for (uint64_t j = i; j < n; j++) {
        const uint64_t k = p.skeys[j];
        if ((k >> kPlaceNodeBits) != gp) break;
        if ((uint32_t)(k & 63) != cur) {
          if (sum > best) best = sum, node = cur;
          sum = 0;
          cur = (uint32_t)(k & 63);
        }
        sum += p.svals[j];
      }
      if (sum > best) best = sum, node = cur;
      p.pcnt[i] = best;
      p.pnode[i] = node;
      q = best > p.D;
    }
    p.flag[i] = q;
  }
}

// Compact: the qualifying pages in (rank, page) order -- the list.  Its keys
// (rank << 32 | page) and counts take the place of the unsorted items.
__global__ __launch_bounds__(256) void place_huge_compact_kernel(PlaceHugeParams p, uint64_t n) {
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += gridDim.x * 256ull) {
    if (!p.flag[i]) continue;
    const uint64_t o = p.off[i];  // (< off[n] <= n)
    p.keys[o] = p.skeys[i] >> kPlaceNodeBits;
    p.vals[o] = p.pcnt[i];
    p.lnode[o] = p.pnode[i];
  }
}

// Starts: a list item starts a block when its group or its node is not the
// previous item's.
__global__ __launch_bounds__(256) void place_huge_starts_kernel(PlaceHugeParams p, uint64_t m) {
  for (uint64_t j = blockIdx.x * 256ull + threadIdx.x; j < m; j += gridDim.x * 256ull)
    p.flag[j] = j == 0 || (p.keys[j - 1] >> 32) != (p.keys[j] >> 32) || p.lnode[j - 1] != p.lnode[j];
}

// Count: off = the exclusive scan of the starts, so item j lies in block
// off[j + 1] - 1 of all huge groups' blocks.  A group's first item records
// that number; every start adds one to its group's blocks.
__global__ __launch_bounds__(256) void place_huge_count_kernel(PlaceHugeParams p, uint64_t m) {
  for (uint64_t j = blockIdx.x * 256ull + threadIdx.x; j < m; j += gridDim.x * 256ull) {
    if (!p.flag[j]) continue;
    const uint32_t rank = (uint32_t)(p.keys[j] >> 32);  // (< H: extract takes ranks from s_rank / dm_rank)
    if (j == 0 || (uint32_t)(p.keys[j - 1] >> 32) != rank) p.gfirst[rank] = p.off[j];
    atomicAdd(p.bcnt + p.h_group[rank], 1u);
  }
}

// Emit: one wave per 64 list items.  The start writes (group, node, start),
// the block's last item its end; the counts are summed over each block's
// lanes (a segmented scan keyed by the block number, which ascends along the
// list) and added by the segment's last lane -- one atomic per block and
// wave, on rows zeroed before the launch.
__global__ __launch_bounds__(256) void place_huge_emit_kernel(PlaceHugeParams p, uint64_t m) {
  const uint32_t lane = threadIdx.x & 63;
  for (uint64_t j0 = blockIdx.x * 256ull + (threadIdx.x & ~63u); j0 < m; j0 += gridDim.x * 256ull) {
    const uint64_t j = j0 + lane;
    const bool in = j < m;
    const uint64_t b = in ? p.off[j + 1] - 1 : ~0ull;  // (item 0 is a start: off[j + 1] >= 1)
    uint64_t cnt = in ? p.vals[j] : 0ull;
    for (int d = 1; d < 64; d <<= 1) {
      const uint64_t c2 = __shfl_up(cnt, d, 64), b2 = __shfl_up(b, d, 64);
      if ((int)lane >= d && b2 == b) cnt += c2;
    }
    const uint64_t bnext = __shfl_down(b, 1, 64);
    if (!in) continue;
    const uint64_t key = p.keys[j];
    const uint32_t rank = (uint32_t)(key >> 32), g = p.h_group[rank];
    uint64_t* r = p.rows + (p.boff[g] + (b - p.gfirst[rank])) * 5;  // (below boff[g + 1]: count_kernel's bcnt[g])
    if (p.flag[j]) {
      r[0] = p.gid[g];
      r[1] = p.lnode[j];
      r[2] = (uint32_t)key;
    }
    if (j + 1 == m || p.flag[j + 1]) r[3] = (uint32_t)key;
    if (lane == 63 || bnext != b) atomicAdd(reinterpret_cast<unsigned long long*>(r + 4), (unsigned long long)cnt);
  }
}

static uint32_t huge_grid(uint64_t n) { return (uint32_t)std::min<uint64_t>((n + 255) / 256, 1u << 16); }

hipError_t launch_place_huge_extract(hipStream_t s, const PlaceHugeParams& p, bool sparse, bool from_cost) {
  const uint64_t total = sparse ? p.sparse_cap : p.dcells * p.T;
  if (!total) return hipSuccess;
  if (from_cost && !(sparse ? p.sparse_cost != nullptr : p.cost != nullptr)) return hipErrorInvalidValue;
  const dim3 grid(huge_grid(total));
  if (sparse && from_cost) hipLaunchKernelGGL((place_huge_extract_kernel<true, true>), grid, dim3(256), 0, s, p, total);
  else if (sparse) hipLaunchKernelGGL((place_huge_extract_kernel<true, false>), grid, dim3(256), 0, s, p, total);
  else if (from_cost) hipLaunchKernelGGL((place_huge_extract_kernel<false, true>), grid, dim3(256), 0, s, p, total);
  else hipLaunchKernelGGL((place_huge_extract_kernel<false, false>), grid, dim3(256), 0, s, p, total);
  return hipGetLastError();
}
size_t place_huge_sort_bytes(uint64_t n) {
  size_t bytes = 0;
  uint64_t* k = nullptr;
  if (rocprim::radix_sort_pairs(nullptr, bytes, k, k, k, k, (size_t)n, 0, kPlaceRankShift + 22) != hipSuccess) return 0;
  return std::max<size_t>(bytes, 16);
}
hipError_t launch_place_huge_sort(hipStream_t s, const PlaceHugeParams& p, uint64_t n, void* tmp, size_t tmp_bytes) {
  return rocprim::radix_sort_pairs(tmp, tmp_bytes, p.keys, const_cast<uint64_t*>(p.skeys), p.vals,
                                   const_cast<uint64_t*>(p.svals), (size_t)n, 0, kPlaceRankShift + 22, s);
}
hipError_t launch_place_huge_reduce(hipStream_t s, const PlaceHugeParams& p, uint64_t n) {
  if (n) hipLaunchKernelGGL(place_huge_reduce_kernel, dim3(huge_grid(n)), dim3(256), 0, s, p, n);
  return hipGetLastError();
}
hipError_t launch_place_huge_compact(hipStream_t s, const PlaceHugeParams& p, uint64_t n) {
  if (n) hipLaunchKernelGGL(place_huge_compact_kernel, dim3(huge_grid(n)), dim3(256), 0, s, p, n);
  return hipGetLastError();
}
hipError_t launch_place_huge_starts(hipStream_t s, const PlaceHugeParams& p, uint64_t m) {
  if (m) hipLaunchKernelGGL(place_huge_starts_kernel, dim3(huge_grid(m)), dim3(256), 0, s, p, m);
  return hipGetLastError();
}
hipError_t launch_place_huge_count(hipStream_t s, const PlaceHugeParams& p, uint64_t m) {
  if (m) hipLaunchKernelGGL(place_huge_count_kernel, dim3(huge_grid(m)), dim3(256), 0, s, p, m);
  return hipGetLastError();
}
hipError_t launch_place_huge_emit(hipStream_t s, const PlaceHugeParams& p, uint64_t m) {
  if (m) hipLaunchKernelGGL(place_huge_emit_kernel, dim3(huge_grid(m)), dim3(256), 0, s, p, m);
  return hipGetLastError();
}

hipError_t launch_place_fold(hipStream_t s, const PlaceParams& p, uint64_t pages) {
  const uint32_t grid = (uint32_t)std::min<uint64_t>((pages + 255) / 256, 1u << 20);
  if (pages && p.cost) hipLaunchKernelGGL(place_fold_kernel<uint64_t>, dim3(grid), dim3(256), 0, s, p, p.cost, pages);
  else if (pages) hipLaunchKernelGGL(place_fold_kernel<uint32_t>, dim3(grid), dim3(256), 0, s, p, p.hist, pages);
  return hipGetLastError();
}
hipError_t launch_place_count(hipStream_t s, const PlaceParams& p) {
  const uint32_t grid = std::min<uint32_t>((p.G + 3) / 4, 8192);
  if (p.G) hipLaunchKernelGGL(place_blocks_kernel<false>, dim3(grid), dim3(256), 0, s, p);
  return hipGetLastError();
}
hipError_t launch_place_emit(hipStream_t s, const PlaceParams& p) {
  const uint32_t grid = std::min<uint32_t>((p.G + 3) / 4, 8192);
  if (p.G) hipLaunchKernelGGL(place_blocks_kernel<true>, dim3(grid), dim3(256), 0, s, p);
  return hipGetLastError();
}

}  // namespace nmg

// ---------------------------------------------------------------------------
// host side

namespace {

// the table's page cells by entry id, or by report position (h->order, where a
// live online table set one)
void entry_cells(nmg_engine* h, bool walk_order, std::vector<uint64_t>& npages, std::vector<uint8_t>& dense,
                 std::vector<uint64_t>& base, std::vector<uint32_t>& ids) {
  const uint32_t E = h->E;
  npages.resize(E);
  dense.resize(E);
  base.resize(E);
  ids.resize(E);
  for (uint32_t k = 0; k < E; k++) {
    const uint32_t id = walk_order && !h->order.empty() ? h->order[k] : k;
    ids[k] = id;
    npages[k] = h->tab.npages[id];
    base[k] = h->tab.hist_base[id];
    dense[k] = base[k] != kHistSparse;
  }
}

// The groups uploaded; every member's cells checked against the histogram.
// A huge group (NMG_PLACE_HUGE: it has a sparse member) has no page here: the
// fold and block kernels pass over it.  Its rank, its sparse members by
// sparse index (a slot whose entry an online update made dense: none) and
// its dense members go to the huge kernels' arrays.  ids: entry id by
// report position (the members' index).
int upload_groups(nmg_engine* h, PlaceDev& d, const PlaceGroups& g, const std::vector<uint64_t>& base,
                  const std::vector<uint32_t>& ids) {
  const size_t G = g.gid.size(), M = g.m_entry.size();
  std::vector<uint64_t> pg_off(G + 1, 0), m_base(M, 0);
  std::vector<uint32_t> h_group, dm_rank, e_rank, e_lim;
  std::vector<uint64_t> dm_off{0}, dm_base;
  for (size_t i = 0; i < G; i++) {
    pg_off[i + 1] = pg_off[i] + (g.huge[i] ? 0 : g.rows[i]);
    if (g.huge[i] && e_rank.empty()) e_rank.assign(h->E, kEmpty32), e_lim.assign(h->E, 0);
    for (size_t m = g.m_off[i]; m < g.m_off[i + 1]; m++) {
      const uint32_t e = g.m_entry[m];
      if (g.m_dense[m]) {
        if (base[e] + g.m_np[m] > h->tab.cells()) return fail(h, NMG_ERR_STATE, "placement: cells outside the histogram");
        if (!g.huge[i]) {
          m_base[m] = base[e];
        } else {
          dm_rank.push_back((uint32_t)h_group.size());
          dm_base.push_back(base[e]);
          dm_off.push_back(dm_off.back() + g.m_np[m]);
        }
      } else if (ids[e] < h->E) {  // (an entry belongs to one group at most)
        e_rank[ids[e]] = (uint32_t)h_group.size();
        e_lim[ids[e]] = g.m_np[m];
      }
    }
    if (g.huge[i]) h_group.push_back((uint32_t)i);
  }
  if (h_group.size() > kMaxSparse) return fail(h, NMG_ERR_CAPACITY, "placement: too many groups with sparse members");
  d.H = (uint32_t)h_group.size();
  d.DM = (uint32_t)dm_rank.size();
  d.dcells = dm_off.back();
  d.nsent = 0;
  if (d.H) {
    const std::vector<uint32_t>& sent = h->tab.sparse_entries;
    std::vector<uint32_t> s_rank(sent.size(), kEmpty32), s_lim(sent.size(), 0);
    for (size_t sx = 0; sx < sent.size(); sx++) {
      const uint32_t e = sent[sx];
      if (e >= h->E || h->tab.hist_base[e] != kHistSparse) continue;
      s_rank[sx] = e_rank[e];
      s_lim[sx] = e_lim[e];
    }
    d.nsent = (uint32_t)sent.size();
    HIP_TRY(h, alloc_copy(h, d.h_group, h_group));
    HIP_TRY(h, alloc_copy(h, d.s_rank, s_rank));
    HIP_TRY(h, alloc_copy(h, d.s_lim, s_lim));
    HIP_TRY(h, alloc_copy(h, d.dm_rank, dm_rank));
    HIP_TRY(h, alloc_copy(h, d.dm_base, dm_base));
    HIP_TRY(h, alloc_copy(h, d.dm_off, dm_off));
    HIP_TRY(h, hipStreamSynchronize(h->stream));  // (this block's vectors are read until here)
  }
  HIP_TRY(h, alloc_copy(h, d.gid, g.gid));
  HIP_TRY(h, alloc_copy(h, d.pg_off, pg_off));
  HIP_TRY(h, alloc_copy(h, d.m_off, g.m_off));
  HIP_TRY(h, alloc_copy(h, d.m_base, m_base));
  HIP_TRY(h, alloc_copy(h, d.m_np, g.m_np));
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // (the vectors above are read until here)
  d.G = (uint32_t)G;
  d.pages = pg_off[G];
  return NMG_OK;
}

// The huge groups of d up to their block counts, added to p.bcnt (after the
// dense groups' count pass, on the same stream): *m list items left in q's
// arrays for launch_place_huge_emit.
int run_huge(nmg_engine* h, const PlaceDev& d, const PlaceMap& map, const PlaceParams& p, PlaceHugeParams& q,
             uint64_t* m, bool from_cost) {
  *m = 0;
  PlaceState& S = h->place;
  hipStream_t st = h->stream;
  bool sparse = false;  // nothing inserted since the last reset: the table is not read
  int rc = sparse_nonempty(h, &sparse);
  if (rc) return rc;
  sparse = sparse && d.nsent && h->cnt.d_sparse_keys && h->cnt.d_sparse_vals && (!from_cost || h->cost.d_sparse);
  // (from the cost cells: the dense members' exist, or the table has no dense cell and they have none)
  const bool dm = d.DM && (!from_cost || p.cost);
  if (!sparse && !dm) return NMG_OK;
  HIP_TRY(h, alloc_copy(h, S.d_tnode, map.node));
  HIP_TRY(h, S.d_hn.reserve(1));
  HIP_TRY(h, S.d_hgfirst.reserve(d.H));
  q.sparse_keys = h->cnt.d_sparse_keys;
  q.sparse_vals = h->cnt.d_sparse_vals;
  q.sparse_cap = h->sparse_cap;
  q.sparse_cost = from_cost ? h->cost.d_sparse.get() : nullptr;
  q.cost = from_cost ? p.cost : nullptr;
  q.nsent = d.nsent;
  q.s_rank = d.s_rank;
  q.s_lim = d.s_lim;
  q.hist = p.hist;
  q.hist_cells = p.hist_cells;
  q.DM = d.DM;
  q.dcells = d.dcells;
  q.dm_off = d.dm_off;
  q.dm_base = d.dm_base;
  q.dm_rank = d.dm_rank;
  q.tnode = S.d_tnode;
  q.T = h->T;
  q.D = map.D;
  q.H = d.H;
  q.h_group = d.h_group;
  q.gid = p.gid;
  q.n_items = reinterpret_cast<unsigned long long*>(S.d_hn.get());
  q.gfirst = S.d_hgfirst;
  q.bcnt = p.bcnt;
  q.boff = p.boff;
  // the items counted, then appended into arrays of that size
  uint64_t n = 0;
  for (int pass = 0; pass < 2; pass++) {
    HIP_TRY(h, hipMemsetAsync(S.d_hn, 0, 8, st));
    if (sparse) HIP_TRY(h, launch_place_huge_extract(st, q, true, from_cost));
    if (dm) HIP_TRY(h, launch_place_huge_extract(st, q, false, from_cost));
    uint64_t got = 0;
    HIP_TRY(h, hipMemcpyAsync(&got, S.d_hn, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));  // (also: the thread map's vector was read)
    if (pass == 0) {
      n = got;
      if (!n) return NMG_OK;
      if (n >> 32) return fail(h, NMG_ERR_CAPACITY, "placement: too many cells in groups with sparse members");
      HIP_TRY(h, S.d_hkeys.reserve(n));
      HIP_TRY(h, S.d_hvals.reserve(n));
      HIP_TRY(h, S.d_hskeys.reserve(n));
      HIP_TRY(h, S.d_hsvals.reserve(n));
      HIP_TRY(h, S.d_hpcnt.reserve(n));
      HIP_TRY(h, S.d_hpnode.reserve(n));
      HIP_TRY(h, S.d_hlnode.reserve(n));
      HIP_TRY(h, S.d_hflag.reserve(n + 1));
      HIP_TRY(h, S.d_hoff.reserve(n + 1));
      HIP_TRY(h, S.d_hpart.reserve(scan_parts(n) + 1));
      q.cap = n;
      q.keys = S.d_hkeys;
      q.vals = S.d_hvals;
      q.skeys = S.d_hskeys;
      q.svals = S.d_hsvals;
      q.pcnt = S.d_hpcnt;
      q.pnode = S.d_hpnode;
      q.lnode = S.d_hlnode;
      q.flag = S.d_hflag;
      q.off = S.d_hoff;
    } else if (got != n) {
      return fail(h, NMG_ERR_STATE, "placement: the page cells changed during the call");
    }
  }
  const size_t tmp_bytes = place_huge_sort_bytes(n);
  if (!tmp_bytes) return fail(h, NMG_ERR_HIP, "placement: radix sort workspace");
  HIP_TRY(h, S.d_htmp.reserve(tmp_bytes));
  HIP_TRY(h, launch_place_huge_sort(st, q, n, S.d_htmp, tmp_bytes));
  HIP_TRY(h, launch_place_huge_reduce(st, q, n));
  uint64_t nq = 0;
  rc = scan_total(h, S.d_hflag, n, S.d_hoff, S.d_hpart, &nq);
  if (rc) return rc;
  if (!nq) return NMG_OK;
  HIP_TRY(h, launch_place_huge_compact(st, q, n));
  HIP_TRY(h, launch_place_huge_starts(st, q, nq));
  HIP_TRY(h, hipMemsetAsync(S.d_hflag + nq, 0, 4, st));  // (emit reads flag[j + 1] below m only; kept defined)
  HIP_TRY(h, launch_scan_u32(st, S.d_hflag, nq, S.d_hoff, S.d_hpart));
  HIP_TRY(h, launch_place_huge_count(st, q, nq));
  *m = nq;
  return NMG_OK;
}

// fold, count, scan, emit over the groups d: rows.n rows left in rows.d_rows
int run_blocks(nmg_engine* h, const PlaceDev& d, const PlaceMap& map, bool from_cost, RowSet<uint64_t, 5>& rows) {
  rows.n = 0;
  if (!d.G) return NMG_OK;
  PlaceState& S = h->place;
  hipStream_t st = h->stream;
  HIP_TRY(h, alloc_copy(h, S.d_thr, map.thr));
  HIP_TRY(h, alloc_copy(h, S.d_noff, map.node_off));
  HIP_TRY(h, S.d_pvcnt.reserve(d.pages));
  HIP_TRY(h, S.d_pvnode.reserve(d.pages));
  HIP_TRY(h, S.d_bcnt.reserve(d.G));
  HIP_TRY(h, S.d_boff.reserve(d.G + 1));
  HIP_TRY(h, S.d_part.reserve(scan_parts(d.G) + 1));
  PlaceParams p{};
  p.hist = h->cnt.d_hist;
  p.cost = from_cost ? (const uint64_t*)h->cost.d_cells : nullptr;  // (cells exist: the groups have dense members)
  p.hist_cells = h->tab.cells();
  p.thr = S.d_thr;
  p.node_off = S.d_noff;
  p.N = map.N;
  p.D = map.D;
  p.G = d.G;
  p.gid = d.gid;
  p.pg_off = d.pg_off;
  p.m_off = d.m_off;
  p.m_base = d.m_base;
  p.m_np = d.m_np;
  p.pv_cnt = S.d_pvcnt;
  p.pv_node = S.d_pvnode;
  p.bcnt = S.d_bcnt;
  p.boff = S.d_boff;
  HIP_TRY(h, launch_place_fold(st, p, d.pages));
  HIP_TRY(h, launch_place_count(st, p));
  PlaceHugeParams q{};
  uint64_t m = 0;
  if (d.H) {
    const int rc = run_huge(h, d, map, p, q, &m, from_cost);
    if (rc) return rc;
  }
  uint64_t nrows = 0;
  const int rc = scan_total(h, S.d_bcnt, d.G, S.d_boff, S.d_part, &nrows);  // (its wait also: the thread map's vectors were read)
  if (rc) return rc;
  if (nrows) {
    HIP_TRY(h, rows.reserve(nrows));
    HIP_TRY(h, hipMemsetAsync(rows.d_rows, 0, nrows * 40, st));
    p.rows = rows.d_rows;
    HIP_TRY(h, launch_place_emit(st, p));
    q.rows = rows.d_rows;
    HIP_TRY(h, launch_place_huge_emit(st, q, m));
    HIP_TRY(h, hipStreamSynchronize(st));
  }
  rows.n = (int64_t)nrows;
  return NMG_OK;
}

// every member entry contributes, the sparse ones included: NMG_PLACE_HUGE, or
// the cost source on an engine whose cells were set with NMG_COST_SCOPE_ALL
bool place_all_members(const nmg_engine* h, const nmg_placement_options* p) {
  return (p->source & NMG_PLACE_HUGE) != 0 ||
         (p->source == NMG_PLACE_PAGE_COST && h->cost.on && h->cost.scope == NMG_COST_SCOPE_ALL);
}

// what every placement call checks first
int placement_begin(nmg_engine* h, const nmg_placement_options* p, PlaceMap& map) {
  if (p->source == (NMG_PLACE_PAGE_COST | NMG_PLACE_HUGE))
    return fail(h, NMG_ERR_INVALID, "placement: NMG_PLACE_HUGE with NMG_PLACE_PAGE_COST: sparse entries have no cost cells "
                                    "unless the cells were set with them (set the cells with NMG_COST_SCOPE_ALL and use "
                                    "NMG_PLACE_PAGE_COST)");
  if (placement_map(p, h->T, map)) return fail(h, NMG_ERR_INVALID, "placement options out of range");
  if ((h->flags & NMG_F_DEFAULT) != NMG_F_DEFAULT)
    return fail(h, NMG_ERR_INVALID, "placement needs NMG_F_MATCH_SAMPLES | NMG_F_PAGE_HIST");
  if (!h->have_table) return fail(h, NMG_ERR_STATE, "placement before nmg_set_objects");
  if (p->source == NMG_PLACE_PAGE_COST && !h->cost.on)
    return fail(h, NMG_ERR_STATE, "placement from the page cost cells: none set (nmg_set_page_cost)");
  HIP_TRY(h, hipSetDevice(h->device));
  return nmg_synchronize(h);
}

// the object blocks of the current results epoch and of p, left in place.rows
int object_blocks_prepare(nmg_engine* h, const nmg_placement_options* p, const PlaceMap& map) {
  PlaceState& S = h->place;
  const bool huge = place_all_members(h, p);
  if (S.obj_dirty || S.obj_huge != huge) {  // (the table's groups: uploaded once per table and flag)
    std::vector<uint64_t> npages, base;
    std::vector<uint8_t> dense;
    std::vector<uint32_t> ids;
    entry_cells(h, false, npages, dense, base, ids);
    PlaceGroups g;
    placement_object_groups(h->E, npages.data(), dense.data(), g, huge);
    S.obj_dirty = true;
    const int rc = upload_groups(h, S.obj, g, base, ids);
    if (rc) return rc;
    S.obj_dirty = false;
    S.obj_huge = huge;
  }
  return run_blocks(h, S.obj, map, p->source == NMG_PLACE_PAGE_COST, S.rows);
}

// nmg_count_object_blocks (n null) and nmg_get_object_blocks: the options
// checked, the row set made stale if it was prepared for others, then the rows
int64_t object_blocks(nmg_engine* h, const nmg_placement_options* p, uint64_t* rows, const int64_t* n) {
  PlaceMap map;
  const int rc = placement_begin(h, p, map);
  if (rc) return rc;
  PlaceState& S = h->place;
  if (std::tie(S.N, S.D, S.source, S.node) != std::tie(map.N, map.D, p->source, map.node)) {
    S.rows.epoch = 0;
    std::tie(S.N, S.D, S.source, S.node) = std::tie(map.N, map.D, p->source, map.node);
  }
  auto prepare = [&](nmg_engine*) { return object_blocks_prepare(h, p, map); };
  return n ? rows_get(h, S.rows, prepare, rows, *n) : rows_count(h, S.rows, prepare);
}

}  // namespace

extern "C" int64_t nmg_count_object_blocks(nmg_engine* h, const nmg_placement_options* p) {
  if (!h || !p) return NMG_ERR_INVALID;
  Range range("nmg_count_object_blocks");
  return object_blocks(h, p, nullptr, nullptr);
}

extern "C" int nmg_get_object_blocks(nmg_engine* h, const nmg_placement_options* p, uint64_t* rows, int64_t n) {
  if (!h || !p || (n && !rows)) return NMG_ERR_INVALID;
  Range range("nmg_get_object_blocks");
  return (int)object_blocks(h, p, rows, &n);
}

// The call-site registry from the per-entry counters (as nmg_report builds
// it: first-match ordinals and counts, 5 words per entry, are downloaded for
// it), the sites' members uploaded as groups, the kernels, the block rows to
// the shared writer.  The page cells do not cross PCIe.
extern "C" int nmg_report_placement(nmg_engine* h, const nmg_object_meta* meta, const nmg_report_options* opts,
                                    const nmg_placement_options* p) {
  if (!h || !p || (h->E && !meta)) return NMG_ERR_INVALID;
  Range range("nmg_report_placement");
  PlaceMap map;
  int rc = placement_begin(h, p, map);
  if (rc) return rc;
  ReportInput in;  // (live online tables: meta follows the walk order)
  rc = report_begin(h, in);
  if (rc) return rc;
  std::vector<uint64_t> npages, base;
  std::vector<uint8_t> dense;
  std::vector<uint32_t> ids;
  entry_cells(h, true, npages, dense, base, ids);
  // a site's rows are its creating entry's pages as the report has them
  // (buffer_size / 4096 + 1); a member's pages are the cells it has
  PlaceGroups g;
  std::vector<PlaceSite> sites;
  std::string err;
  rc = placement_site_groups(&in.res, meta, opts && opts->online, npages.data(), dense.data(), g, sites, err,
                             place_all_members(h, p));
  std::vector<uint64_t> rows;
  if (!rc) {
    PlaceDev d;
    RowSet<uint64_t, 5> set;  // (this call's own: the sites' blocks are not kept)
    rc = upload_groups(h, d, g, base, ids);
    if (!rc)
      rc = rows_collect(h, set, [&](nmg_engine*) { return run_blocks(h, d, map, p->source == NMG_PLACE_PAGE_COST, set); }, &rows);
    if (rc) return rc;
    rc = write_blocks(sites, rows.data(), set.n, opts, err);
  }
  if (rc && !err.empty()) h->last_error = err;
  return rc;
}
