// nmg_route_host.hip -- host side of the partition-first path (nmg_route.h):
// eligibility, compact-record layout, chunk pools, the route / count / plan /
// scatter / local launches.
#include "nmg_engine_impl.h"

// ---------------------------------------------------------------------------
// partition-first path (nmg_route.h): eligibility, pool sizing, launches

uint32_t bits_for(uint64_t v) {  // smallest b with v < 2^b
  uint32_t b = 0;
  while (b < 64 && (v >> b) != 0) b++;
  return b;
}

// X word layout of the current buffers; false when the weight field would
// be narrower than kMinWeightBits (escapes would be common)
bool route_layout(nmg_engine* h, const std::vector<BufDesc>& descs, XLayout& xl) {
  uint64_t maxlen = 1;
  for (const BufDesc& d : descs) maxlen = std::max<uint64_t>(maxlen, d.len);
  xl.gbits = bits_for(descs.size() - 1);
  xl.obits = bits_for((maxlen - 1) / 8);
  xl.tbits = bits_for(h->T - 1);
  const uint32_t loc = xl.gbits + xl.obits + xl.tbits + 1;  // (+ access bit)
  if (loc > 48 - kMinWeightBits || xl.gbits > 31 || xl.obits > 31 || xl.tbits > 31) return false;
  xl.wbits = std::min<uint32_t>(48 - loc, 16);  // (the decode reads at most 16 bits of weight)
  xl.wesc = (1ull << xl.wbits) - 1;
  xl.tbase = h->rt.tbase;
  return true;
}

// the partition-first path for this buffer set (the submitted buffers, or a
// streamed chunk of them)
bool route_eligible(nmg_engine* h, const std::vector<BufDesc>& descs) {
  constexpr uint32_t kLegacyOnly = kDbgLoadOnly | kDbgNoGlobal | kDbgNoFlush | kDbgNoTables | kDbgTiming |
                                   kDbgTinyLog | kDbgNoPack | kDbgNoDir | kDbgNoRoute | NMG_F_SINGLE_PASS;
  if (!h->rt.ok || (h->flags & kLegacyOnly) || descs.empty()) return false;
  // the first-match ordinal is rebuilt from the buffer index: seq = seq0 + index
  uint64_t bytes = 0;
  for (size_t i = 0; i < descs.size(); i++) {
    if (descs[i].seq != descs[0].seq + i) return false;
    bytes += descs[i].len;
  }
  // chunk ids (route pass LDS: id << 7 | fill) -- an upper bound of the pool,
  // twice over: the ids skipped before a workgroup's range, so that it lies in
  // one piece (pool_layout), are fewer than the range holds
  const uint64_t chunks = (bytes / kRecBytes + descs.size()) / kChunk + (uint64_t)h->num_cus * (2 * h->rt.nparts + 2);
  if (2 * chunks >= (1ull << kChunkIdBits)) return false;
  XLayout xl;
  return route_layout(h, descs, xl);
}
bool route_eligible(nmg_engine* h) { return route_eligible(h, h->descs); }

// per-workgroup private chunk pools for a new schedule: every SAMPLE record
// of at least 40 B fits (a partition's chunks are full but for its open and
// next chunks); shorter records past that are attributed directly
int route_pool(nmg_engine* h, const std::vector<BufDesc>& descs, uint32_t grid, const uint32_t* ranges,
                      std::vector<uint32_t>& c0) {
  const uint32_t P = h->rt.nparts;
  c0.assign(grid + 1, 0);
  std::vector<uint64_t> caps(grid);
  uint64_t maxcap = 1;
  for (uint32_t w = 0; w < grid; w++) {
    uint64_t rec = 0;
    for (uint32_t b = ranges[w]; b < ranges[w + 1]; b++) rec += (descs[b].len + kRecBytes - 1) / kRecBytes;
    // (route2_kernel keeps two chunks open per partition: the open one and
    // the next, opened ahead)
    caps[w] = (h->flags & kDbgTinyPool) ? 2 : (rec + kChunk - 1) / kChunk + 2 * P;
    maxcap = std::max(maxcap, caps[w]);
  }
  // the workgroups' ranges in the pool's pieces (nmg_pool_layout.h): in the
  // pieces the pool has if they serve, else in pieces of 2^kPieceLog2 chunks,
  // larger where the largest range asks for it
  RoutePool& rp = h->rpool;
  const uint64_t limit = 1ull << kChunkIdBits;
  const uint32_t Kmin = pool_min_log2(maxcap);
  uint32_t K = rp.K, npieces = 0;
  const bool fits = !rp.pieces.empty() && K >= Kmin &&
                    pool_layout(caps.data(), grid, K, limit, c0.data(), &npieces) && npieces <= rp.pieces.size();
  if (!fits) {
    K = (h->flags & kDbgTinyPieces) ? Kmin : std::max(Kmin, kPieceLog2);
    if (!pool_layout(caps.data(), grid, K, limit, c0.data(), &npieces))
      return fail(h, NMG_ERR_RANGE, "partition-first chunk pool too large");
  }
  uint64_t tot = c0[grid];
  size_t items = tot / kItemChunks + P + 1;
  // overflow list: records past a full pool (only SAMPLE records shorter than
  // 40 B can get there; kDbgTinyPool sends nearly all of them)
  uint64_t recs = 0;
  for (const BufDesc& d : descs) recs += (d.len + kRecBytes - 1) / kRecBytes;
  // (a quarter of the records, plus up to three times them for batches under 4M records)
  const size_t ovf = (size_t)((h->flags & kDbgTinyPool) ? recs : recs / 4 + std::min<uint64_t>(3 * recs, 4u << 20)) + 65536;
  if (!fits || tot > rp.d_cmeta.cap() || items > rp.d_items.cap() || grid > rp.d_used.cap() || ovf > rp.d_ovfx.cap()) {
    HIP_TRY(h, hipStreamSynchronize(h->stream));  // a launch in flight may still read the old pool
    rp = RoutePool();  // (the whole pool anew, sized together; route_pending is kept)
    // the pieces, each a device allocation of its own.  The local pass finds a
    // chunk by its distance from the lowest piece, a u32 of chunks
    // (ScatterParams::clist .y): should the allocator ever spread the pieces
    // further than that, the pool is one piece.
    std::vector<uint4*> bases;
    for (bool single = false;; single = true) {
      if (single) {
        uint64_t asked = 0;
        for (uint64_t c : caps) asked += c;
        K = pool_min_log2(std::max<uint64_t>(asked, 1));
        if (!pool_layout(caps.data(), grid, K, limit, c0.data(), &npieces))
          return fail(h, NMG_ERR_RANGE, "partition-first chunk pool too large");
        tot = c0[grid];
        items = tot / kItemChunks + P + 1;
      }
      npieces = std::max(npieces, 1u);
      rp.pieces.clear();
      rp.pieces.resize(npieces);
      bases.assign(npieces + 1, nullptr);  // (one more, null: a range that starts where the ids end)
      uintptr_t lo = ~uintptr_t(0), hi = 0, misaligned = 0;
      for (uint32_t i = 0; i < npieces; i++) {
        // (the last piece ends with the ids: d_cmeta.cap() bounds every later layout)
        const size_t nch = i + 1 < npieces ? size_t(1) << K : std::max<size_t>(tot, 1) - (size_t(i) << K);
        HIP_TRY(h, rp.pieces[i].alloc(nch * kChunk));
        bases[i] = rp.pieces[i];
        const uintptr_t b = reinterpret_cast<uintptr_t>(bases[i]);
        lo = std::min(lo, b);
        hi = std::max(hi, b + nch * kChunk * sizeof(uint4));
        misaligned |= b % (kChunk * sizeof(uint4));
      }
      rp.pool0 = reinterpret_cast<uint4*>(lo);
      if (!misaligned && (hi - lo) / (kChunk * sizeof(uint4)) < (1ull << 32)) break;
      if (single) return fail(h, NMG_ERR_HIP, "partition-first chunk pool: unusable device allocation");
    }
    rp.K = K;
    const size_t cap = std::max<size_t>(tot, 1);
    HIP_TRY(h, rp.d_pieces.alloc(npieces + 1));
    HIP_TRY(h, hipMemcpy(rp.d_pieces, bases.data(), (npieces + 1) * sizeof(uint4*), hipMemcpyHostToDevice));
    HIP_TRY(h, rp.d_cmeta.alloc(cap));
    HIP_TRY(h, rp.d_cmatch.alloc(cap));
    HIP_TRY(h, rp.d_clist.alloc(cap));
    HIP_TRY(h, rp.d_items.alloc(items));
    HIP_TRY(h, rp.d_chunk0.alloc(grid + 1));
    HIP_TRY(h, rp.d_used.alloc(grid));
    HIP_TRY(h, rp.d_pcnt.alloc((size_t)grid * (kMaxParts + 1)));
    HIP_TRY(h, rp.d_pbase.alloc(kMaxParts + 1));
    HIP_TRY(h, rp.d_ctl.alloc(4));
    HIP_TRY(h, hipMemset(rp.d_ctl, 0, 4 * 4));
    HIP_TRY(h, rp.d_ovf16.alloc(ovf));
    HIP_TRY(h, rp.d_ovfx.alloc(ovf));
  }
  rp.ids = tot;
  rp.asked = 0;
  for (uint64_t c : caps) rp.asked += c;
  return NMG_OK;
}

int route_prepare(nmg_engine* h, uint32_t grid, const std::vector<uint32_t>& ranges) {
  std::vector<uint32_t> c0;
  const int rc = route_pool(h, h->descs, grid, ranges.data(), c0);
  if (rc) return rc;
  const int rc2 = stage_h2d(h, h->rpool.d_chunk0, c0.data(), (grid + 1) * 4);
  if (rc2) return rc2;
  h->route_sched_key = route_key(h);
  return NMG_OK;
}


// Route -> plan -> scatter -> local over the buffers of the current schedule
// (analysis order), bracketed by the launch-timing events.
int route_analyze(nmg_engine* h, uint32_t nb, uint32_t grid) {
  (void)nb;
  RouteJob job{&h->descs, h->d_data, h->d_sdescs, h->d_ranges, h->rpool.d_chunk0, grid, 0, false};
  return route_analyze_job(h, job);
}

int route_analyze_job(nmg_engine* h, const RouteJob& job) {
  Range range("nmg_route");
  XLayout xl;
  if (!route_layout(h, *job.descs, xl)) return fail(h, NMG_ERR_STATE, "route layout");
  const uint32_t grid = job.grid;
  Params base = base_params(h, job.data, job.sdescs, job.ranges);
  base.bufcnt = h->d_bufcnt + job.index_base;  // (count slots of the set's first buffer)
  const uint64_t seq0 = (*job.descs)[0].seq;
  h->route_launches++;
  h->route_last_xl = xl;
  int slot = 0;
  int rc = launch_events(h, &slot);
  if (rc) return rc;
  HIP_TRY(h, hipEventRecord(h->ring0[slot], h->stream));
  RouteParams rp;
  memset(&rp, 0, sizeof(rp));
  rp.p = base;
  rp.pbounds = h->rt.d_pbounds;
  rp.pdir = h->rt.d_pdir;
  rp.pdead = h->rt.d_pdead;
  for (uint32_t k = 0; k < kRouteSegs; k++) rp.seg[k] = h->rt.rsegs[k];
  rp.nseg = h->rt.nrsegs;
  rp.nparts = h->rt.nparts;
  rp.xl = xl;
  rp.seq0 = seq0;
  rp.pieces = h->rpool.d_pieces;
  rp.pk = h->rpool.K;
  rp.cmeta = h->rpool.d_cmeta;
  rp.chunk0 = job.chunk0;
  rp.used = h->rpool.d_used;
  rp.ovf16 = h->rpool.d_ovf16;
  rp.ovfx = h->rpool.d_ovfx;
  rp.ovf_cnt = h->rpool.d_ctl + 2;
  rp.ovf_cap = (uint32_t)std::min<size_t>(h->rpool.d_ovfx.cap(), 0xffffffffu);
  if (h->flags & kDbgTinyOvf) rp.ovf_cap = std::min<uint32_t>(rp.ovf_cap, 64);  // (tests: the direct attribution past a full list)
  if (h->flags & kDbgRouteTiming) {  // (internal) per-wave phase cycles, read by nmg_debug_timing
    rc = ensure_dbg(h, (size_t)grid * (kWG / 64) * kRouteTimingWords);
    if (rc) return rc;
    rp.p.dbg = reinterpret_cast<unsigned long long*>(h->d_dbg.get());
  }
  HIP_TRY(h, launch_route(grid, h->stream, rp));
  HIP_TRY(h, hipEventRecord(h->ringr[slot], h->stream));
  HIP_TRY(h, launch_overflow(h->stream, rp));
  ScatterParams sc;
  sc.cmeta = h->rpool.d_cmeta;
  sc.chunk0 = job.chunk0;
  sc.used = h->rpool.d_used;
  sc.pcnt = h->rpool.d_pcnt;
  sc.pbase = h->rpool.d_pbase;
  sc.clist = h->rpool.d_clist;
  sc.pieces = h->rpool.d_pieces;
  sc.pool0 = reinterpret_cast<uint64_t>(h->rpool.pool0);
  sc.pk = h->rpool.K;
  sc.nparts = h->rt.nparts;
  CountParams cp;
  memset(&cp, 0, sizeof(cp));
  cp.sc = sc;
  HIP_TRY(h, launch_count(grid, h->stream, cp));
  PlanParams pl;
  pl.pcnt = h->rpool.d_pcnt;
  pl.pbase = h->rpool.d_pbase;
  pl.items = h->rpool.d_items;
  pl.ctl = h->rpool.d_ctl;
  pl.grid = grid;
  pl.nparts = h->rt.nparts;
  HIP_TRY(h, launch_plan(h->stream, pl));
  HIP_TRY(h, launch_scatter(grid, h->stream, sc));
  LocalParams lp;
  memset(&lp, 0, sizeof(lp));
  lp.p = base;
  lp.parts = h->rt.d_parts;
  lp.pe_keys = h->rt.d_pe_keys;
  lp.pe_nodes = h->rt.d_pe_nodes;
  lp.pe_info = h->rt.d_pe_info;
  lp.pe_pnode = h->rt.d_pe_pnode;
  lp.pe_old = h->rt.d_pe_old;
  lp.pe_oinf = h->rt.d_pe_oinf;
  lp.pe_dir = h->rt.d_pe_dir;
  lp.pe_ids = h->rt.d_pe_ids;
  lp.pe_lrel = h->rt.d_pe_lrel;
  lp.pe_cmap = h->rt.d_pe_cmap;
  lp.pool0 = h->rpool.pool0;
  lp.cmeta = h->rpool.d_cmeta;
  lp.clist = h->rpool.d_clist;
  lp.items = h->rpool.d_items;
  lp.ctl = h->rpool.d_ctl;
  lp.cmatch = h->rpool.d_cmatch;
  lp.descs = job.sdescs;
  lp.xl = xl;
  lp.seq0 = seq0;
  lp.fresh = h->counters_fresh ? 1u : 0u;
  h->counters_fresh = false;
  if ((h->flags & kDbgLocalTiming) && !(h->flags & kDbgRouteTiming)) {  // (internal) per-wave phase cycles
    rc = ensure_dbg(h, (size_t)h->num_cus * (kWG / 64) * kRouteTimingWords);
    if (rc) return rc;
    lp.p.dbg = reinterpret_cast<unsigned long long*>(h->d_dbg.get());
  }
  HIP_TRY(h, launch_local((uint32_t)h->num_cus, h->stream, lp));
  HIP_TRY(h, hipEventRecord(h->ringm[slot], h->stream));
  HIP_TRY(h, hipEventRecord(h->ring1[slot], h->stream));
  h->nlaunch++;
  h->launched = true;
  if (job.settle_now) {  // (a streamed chunk: the next one reuses the pool)
    FoundParams f;
    f.ranges = job.ranges;
    f.chunk0 = job.chunk0;
    f.used = h->rpool.d_used;
    f.cmeta = h->rpool.d_cmeta;
    f.cmatch = h->rpool.d_cmatch;
    f.pieces = h->rpool.d_pieces;
  f.pk = h->rpool.K;
    f.bufcnt = h->d_bufcnt + job.index_base;
    f.nb_bufs = (uint32_t)h->bufcnt_stride;
    f.gbits = xl.gbits;
    f.gshift = 16 + xl.wbits + xl.obits;
    HIP_TRY(h, launch_found(grid, h->stream, f));
    return NMG_OK;
  }
  h->route_pending = true;
  h->route_grid = grid;
  h->route_xl = xl;
  return NMG_OK;
}

// Per-buffer matched-sample counts of the last route analysis (found_kernel),
// enqueued before anything reads or replaces them.  A reset drops them
// instead: it zeroes those counts anyway.
int route_settle(nmg_engine* h) {
  if (!h->route_pending) return NMG_OK;
  h->route_pending = false;
  FoundParams f;
  f.ranges = h->d_ranges;
  f.chunk0 = h->rpool.d_chunk0;
  f.used = h->rpool.d_used;
  f.cmeta = h->rpool.d_cmeta;
  f.cmatch = h->rpool.d_cmatch;
  f.pieces = h->rpool.d_pieces;
  f.pk = h->rpool.K;
  f.bufcnt = h->d_bufcnt;
  f.nb_bufs = (uint32_t)h->bufcnt_stride;
  f.gbits = h->route_xl.gbits;
  f.gshift = 16 + h->route_xl.wbits + h->route_xl.obits;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, launch_found(h->route_grid, h->stream, f));
  return NMG_OK;
}
