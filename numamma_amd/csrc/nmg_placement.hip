// nmg_placement.hip -- NUMA placement blocks on the device: the fold and block
// kernels, their launchers (nmg_kernels.h) and the C-ABI calls that run them
// (nmg_count_object_blocks, nmg_get_object_blocks, nmg_report_placement).  The
// rule, the file format and the differences from the reference's
// scripts/counters_to_binding.py are in include/numamma_gpu.h; the host
// statement of the same rule and the writer are in nmg_report.cpp.
//
// The kernels read the page histogram and write arrays of their own: the
// analysis kernels and their launch code are not involved.
#include "nmg_engine_impl.h"

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
                 std::vector<uint64_t>& base) {
  const uint32_t E = h->E;
  npages.resize(E);
  dense.resize(E);
  base.resize(E);
  for (uint32_t k = 0; k < E; k++) {
    const uint32_t id = walk_order && !h->order.empty() ? h->order[k] : k;
    npages[k] = h->tab.npages[id];
    base[k] = h->tab.hist_base[id];
    dense[k] = base[k] != kHistSparse;
  }
}

// the groups uploaded; every member's cells checked against the histogram
int upload_groups(nmg_engine* h, PlaceDev& d, const PlaceGroups& g, const std::vector<uint64_t>& base) {
  const size_t G = g.gid.size(), M = g.m_entry.size();
  std::vector<uint64_t> pg_off(G + 1, 0), m_base(M);
  for (size_t i = 0; i < G; i++) pg_off[i + 1] = pg_off[i] + g.rows[i];
  for (size_t m = 0; m < M; m++) {
    m_base[m] = base[g.m_entry[m]];
    if (m_base[m] + g.m_np[m] > h->tab.cells()) return fail(h, NMG_ERR_STATE, "placement: cells outside the histogram");
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

// fold, count, scan, emit over the groups d: *n rows left in d_rows
int run_blocks(nmg_engine* h, const PlaceDev& d, const PlaceMap& map, bool from_cost, DevBuf<uint64_t>& d_rows,
               int64_t* n) {
  *n = 0;
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
  HIP_TRY(h, launch_scan_u32(st, S.d_bcnt, d.G, S.d_boff, S.d_part));
  uint64_t nrows = 0;
  HIP_TRY(h, hipMemcpyAsync(&nrows, S.d_boff + d.G, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(h, hipStreamSynchronize(st));  // (also: the thread map's vectors were read)
  if (nrows) {
    HIP_TRY(h, d_rows.reserve(nrows * 5));
    HIP_TRY(h, hipMemsetAsync(d_rows, 0, nrows * 40, st));
    p.rows = d_rows;
    HIP_TRY(h, launch_place_emit(st, p));
    HIP_TRY(h, hipStreamSynchronize(st));
  }
  *n = (int64_t)nrows;
  return NMG_OK;
}

// what every placement call checks first
int placement_begin(nmg_engine* h, const nmg_placement_options* p, PlaceMap& map) {
  if (placement_map(p, h->T, map)) return fail(h, NMG_ERR_INVALID, "placement options out of range");
  if ((h->flags & NMG_F_DEFAULT) != NMG_F_DEFAULT)
    return fail(h, NMG_ERR_INVALID, "placement needs NMG_F_MATCH_SAMPLES | NMG_F_PAGE_HIST");
  if (!h->have_table) return fail(h, NMG_ERR_STATE, "placement before nmg_set_objects");
  if (p->source == NMG_PLACE_PAGE_COST && !h->cost.on)
    return fail(h, NMG_ERR_STATE, "placement from the page cost cells: none set (nmg_set_page_cost)");
  HIP_TRY(h, hipSetDevice(h->device));
  return nmg_synchronize(h);
}

// the object blocks of the current results epoch and of p, left in place.d_rows
int object_blocks_prepare(nmg_engine* h, const nmg_placement_options* p) {
  PlaceMap map;
  int rc = placement_begin(h, p, map);
  if (rc) return rc;
  PlaceState& S = h->place;
  if (S.rows_epoch == h->epoch && S.N == map.N && S.D == map.D && S.source == p->source && S.node == map.node)
    return NMG_OK;
  if (S.obj_dirty) {  // (the table's groups: uploaded once per table)
    std::vector<uint64_t> npages, base;
    std::vector<uint8_t> dense;
    entry_cells(h, false, npages, dense, base);
    PlaceGroups g;
    placement_object_groups(h->E, npages.data(), dense.data(), g);
    rc = upload_groups(h, S.obj, g, base);
    if (rc) return rc;
    S.obj_dirty = false;
  }
  S.rows_epoch = 0;
  rc = run_blocks(h, S.obj, map, p->source == NMG_PLACE_PAGE_COST, S.d_rows, &S.n);
  if (rc) return rc;
  S.rows_epoch = h->epoch;
  S.N = map.N;
  S.D = map.D;
  S.source = p->source;
  S.node = map.node;
  return NMG_OK;
}

}  // namespace

extern "C" int64_t nmg_count_object_blocks(nmg_engine* h, const nmg_placement_options* p) {
  if (!h || !p) return NMG_ERR_INVALID;
  Range range("nmg_count_object_blocks");
  const int rc = object_blocks_prepare(h, p);
  return rc ? rc : h->place.n;
}

extern "C" int nmg_get_object_blocks(nmg_engine* h, const nmg_placement_options* p, uint64_t* rows, int64_t n) {
  if (!h || !p || (n && !rows)) return NMG_ERR_INVALID;
  Range range("nmg_get_object_blocks");
  const int rc = object_blocks_prepare(h, p);
  if (rc) return rc;
  if (h->place.n != n) return fail(h, NMG_ERR_INVALID, "row count mismatch");
  if (n) HIP_TRY(h, hipMemcpy(rows, h->place.d_rows, (size_t)n * 40, hipMemcpyDeviceToHost));
  return NMG_OK;
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
  HostResults r;
  rc = engine_download(h, r, true, false);
  if (rc) return rc;
  nmg_host_results res;
  memset(&res, 0, sizeof(res));
  res.nb_threads = h->T;
  res.match_samples = 1;
  WalkCounters w;  // (live online tables: meta follows the walk order)
  rc = walk_counters(h, r, res, w);
  if (rc) return rc;
  std::vector<uint64_t> npages, base;
  std::vector<uint8_t> dense;
  entry_cells(h, true, npages, dense, base);
  // a site's rows are its creating entry's pages as the report has them
  // (buffer_size / 4096 + 1); a member's pages are the cells it has
  PlaceGroups g;
  std::vector<PlaceSite> sites;
  std::string err;
  rc = placement_site_groups(&res, meta, opts && opts->online, npages.data(), dense.data(), g, sites, err);
  std::vector<uint64_t> rows;
  if (!rc) {
    PlaceDev d;
    DevBuf<uint64_t> d_rows;
    int64_t n = 0;
    rc = upload_groups(h, d, g, base);
    if (!rc) rc = run_blocks(h, d, map, p->source == NMG_PLACE_PAGE_COST, d_rows, &n);
    if (rc) return rc;
    rows.resize((size_t)n * 5);
    if (n) HIP_TRY(h, hipMemcpy(rows.data(), d_rows, (size_t)n * 40, hipMemcpyDeviceToHost));
    rc = write_blocks(sites, rows.data(), n, opts, err);
  }
  if (rc && !err.empty()) h->last_error = err;
  return rc;
}
