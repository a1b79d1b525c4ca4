// nmg_table.hip -- object tables on the device: the sorted keys and LIFO
// entries of mem_list (FOREACH_HASH order, src/mem_analyzer.c:1820-1823), the
// lookup structures of lower_key (ht_lower_key, tools/hash.c:63-77), the
// partition-first path's partitions, and online table updates.
#include "nmg_engine_impl.h"

// Lookup structure of a table larger than kLdsNodes keys (see lower_key):
// fence b = keys[b << fence_log2] (<= kMaxFences fences, Eytzinger order),
// and per bucket a directory of 2^dir_log2 equal-width slots over the bucket's
// key span [first key, last key].
struct BigLookup {
  uint32_t nb_fences = 0, fence_log2 = 0, dir_log2 = 0;
  std::vector<uint64_t> efences;  // [kMaxFences + 1]
  std::vector<uint8_t> shift;     // [nb_fences]
  std::vector<uint2> dir;         // [nb_fences << dir_log2]
};

static void build_big_lookup(const uint64_t* keys, uint32_t K, bool no_dir, BigLookup& bl) {
  while (((uint64_t)K + (1u << bl.fence_log2) - 1) >> bl.fence_log2 > kMaxFences) bl.fence_log2++;
  const uint32_t S = 1u << bl.fence_log2;
  bl.nb_fences = (uint32_t)(((uint64_t)K + S - 1) >> bl.fence_log2);
  // Eytzinger order: an in-order walk of the complete 12-level tree hands out
  // the fences in sorted order; the slots after the last fence hold ~0
  bl.efences.assign(kMaxFences + 1, ~0ull);
  {
    uint32_t r = 0, i = 1;
    std::vector<uint32_t> stack;
    while (i <= kMaxFences || !stack.empty()) {
      while (i <= kMaxFences) {
        stack.push_back(i);
        i = 2 * i;
      }
      i = stack.back();
      stack.pop_back();
      if (r < bl.nb_fences) bl.efences[i] = keys[(uint64_t)r << bl.fence_log2];
      r++;
      i = 2 * i + 1;
    }
  }
  bl.shift.assign(bl.nb_fences, kShiftSearch);
  // bucket-relative indices and counts are 16-bit: S <= 2^16 (larger
  // buckets -- more than 4095 << 16 keys -- are binary-searched)
  if (S == 1 || S > (1u << 16) || no_dir) return;
  bl.dir_log2 = bl.fence_log2 + 1;  // two slots per key
  const uint32_t D = 1u << bl.dir_log2;
  bl.dir.assign((size_t)bl.nb_fences << bl.dir_log2, make_uint2(0, 0));
  for (uint32_t b = 0; b < bl.nb_fences; b++) {
    const uint32_t k0 = b * S, k1 = std::min<uint64_t>((uint64_t)k0 + S, K);
    const uint64_t f = keys[k0], span = keys[k1 - 1] - f;
    uint32_t sh = 0;
    while (sh < 64 && (span >> sh) >= D) sh++;
    if (sh > 32) continue;  // slot offsets must fit 32 bits: binary search instead
    bl.shift[b] = (uint8_t)sh;
    uint2* dd = &bl.dir[(size_t)b << bl.dir_log2];
    uint32_t k = k0;  // largest key <= slot start
    for (uint32_t j = 0; j < D; j++) {
      const uint64_t s0 = (uint64_t)j << sh;  // slot [s0, s0 + 2^sh) relative to f; the last slot is open
      while (k + 1 < k1 && keys[k + 1] - f <= s0) k++;
      uint32_t c = 0;
      while (k + 1 + c < k1 && (j == D - 1 || keys[k + 1 + c] - f < s0 + (1ull << sh))) c++;
      dd[j].x = (k - k0) | (std::min<uint32_t>(c, 0xffffu) << 16);
      dd[j].y = c ? (uint32_t)(keys[k + 1] - f - s0) : 0u;
    }
  }
}

// Lookup structures of a flattened table whose entries, in table order, are
// chain[] (ids in DevEntry::id): node records, then the LDS Eytzinger tree
// (<= kLdsNodes keys) or the fences + directory of the large-table path.
// chain_dev: chain already on the device (the by-id array), else uploaded.
int build_lookup(nmg_engine* h, LookupSet& l, const uint64_t* keys, const uint32_t* entry_off, uint32_t nb_keys,
                 const std::vector<DevEntry>& chain, DevEntry* chain_dev) {
  l.K = nb_keys;
  std::vector<DevEntry> nodes(nb_keys);
  for (uint32_t k = 0; k < nb_keys; k++) {
    nodes[k] = chain[entry_off[k]];
    nodes[k].first = entry_off[k];
    nodes[k].count = entry_off[k + 1] - entry_off[k];
  }
  HIP_TRY(h, alloc_copy(h, l.keys, keys, nb_keys));
  HIP_TRY(h, alloc_copy(h, l.nodes, nodes));
  if (!chain_dev) HIP_TRY(h, alloc_copy(h, l.own_chain, chain));
  l.chain = chain_dev ? chain_dev : l.own_chain.get();
  if (nb_keys <= kLdsNodes) {
    // Eytzinger (BFS) order for the LDS search: an in-order walk of the
    // complete tree of 2^L - 1 nodes hands out the keys in sorted order; the
    // slots after the last key are ~0 keys carrying a copy of the last node
    // (reached only for addr == UINT64_MAX, where the last key is the answer)
    l.elevels = 0;
    while (((1u << l.elevels) - 1) < nb_keys) l.elevels++;
    const uint32_t n = 1u << l.elevels;
    std::vector<uint64_t> ef(n, ~0ull);
    std::vector<DevEntry> en(n);
    memset(en.data(), 0, n * sizeof(DevEntry));
    uint32_t r = 0;
    std::vector<uint32_t> stack;
    uint32_t i = 1;
    while (i < n || !stack.empty()) {  // iterative in-order walk
      while (i < n) {
        stack.push_back(i);
        i = 2 * i;
      }
      i = stack.back();
      stack.pop_back();
      if (r < nb_keys) {
        ef[i] = keys[r];
        en[i] = nodes[r];
      } else if (nb_keys) {
        en[i] = nodes[nb_keys - 1];
      }
      r++;
      i = 2 * i + 1;
    }
    HIP_TRY(h, alloc_copy(h, l.efences, ef));
    HIP_TRY(h, alloc_copy(h, l.enodes, en));
  }
  l.nb_fences = l.fence_log2 = l.dir_log2 = 0;
  if (nb_keys > kLdsNodes) {
    BigLookup bl;
    build_big_lookup(keys, nb_keys, (h->flags & kDbgNoDir) != 0, bl);
    l.nb_fences = bl.nb_fences;
    l.fence_log2 = bl.fence_log2;
    l.dir_log2 = bl.dir_log2;
    HIP_TRY(h, alloc_copy(h, l.ffences, bl.efences));
    HIP_TRY(h, alloc_copy(h, l.fshift, bl.shift));
    HIP_TRY(h, alloc_copy(h, l.dir, bl.dir));
  }
  return NMG_OK;
}

// The route pass's partition search (route_partition, nmg_route.hip) over
// the P ascending partition starts b: up to kRouteSegs segments, split at the
// gaps between consecutive starts that dwarf the median gap (address spaces
// are clustered: globals, heap, mmap'd regions, the stack), each with
// directory slots in proportion to its partitions.  Slot j of a segment holds
// the last partition starting at or before the slot start, and how many
// starts lie inside the slot (saturated at kDirCntSat: search to the
// segment's last partition).
void route_segments(const uint64_t* b, uint32_t P, RSeg* seg, uint32_t* nseg, std::vector<uint16_t>& dir) {
  std::vector<uint32_t> cuts{0};  // segment k starts at partition cuts[k]
  if (P > 1) {
    std::vector<uint64_t> gaps(P - 1);
    for (uint32_t q = 0; q + 1 < P; q++) gaps[q] = b[q + 1] - b[q];
    std::vector<uint64_t> med(gaps);
    std::nth_element(med.begin(), med.begin() + med.size() / 2, med.end());
    const uint64_t m = std::max<uint64_t>(med[med.size() / 2], 1);
    std::vector<uint32_t> idx(P - 1);
    for (uint32_t q = 0; q + 1 < P; q++) idx[q] = q;
    std::sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) { return gaps[x] > gaps[y]; });
    for (uint32_t i = 0; i < idx.size() && cuts.size() < kRouteSegs; i++) {
      if (gaps[idx[i]] / 64 <= m) break;
      cuts.push_back(idx[i] + 1);
    }
    std::sort(cuts.begin(), cuts.end());
  }
  const uint32_t S = (uint32_t)cuts.size();
  dir.assign(kRouteDir, 0);
  uint32_t used = 0;
  for (uint32_t k = 0; k < kRouteSegs; k++) {
    if (k >= S) {
      seg[k] = RSeg{~0ull, 0, 1, 0, 0};
      continue;
    }
    const uint32_t qa = cuts[k], qb = k + 1 < S ? cuts[k + 1] : P;
    const uint32_t ns = (uint32_t)((uint64_t)(kRouteDir - S) * (qb - qa) / P) + 1;
    const uint64_t span = b[qb - 1] - b[qa];
    uint32_t sh = 0;
    while (sh < 63 && (span >> sh) >= ns) sh++;
    seg[k] = RSeg{b[qa], used, ns, sh, qb - 1};
    uint32_t q = qa;
    for (uint32_t j = 0; j < ns; j++) {
      // slot [s0, s1) relative to the segment start
      const unsigned __int128 s0 = (unsigned __int128)j << sh, s1 = (unsigned __int128)(j + 1) << sh;
      while (q + 1 < qb && (unsigned __int128)(b[q + 1] - b[qa]) <= s0) q++;
      uint32_t c = 0;
      if (j == ns - 1) c = qb - 1 - q;
      else
        while (q + 1 + c < qb && (unsigned __int128)(b[q + 1 + c] - b[qa]) < s1) c++;
      dir[used + j] = (uint16_t)(q | (std::min(c, kDirCntSat) << 11));
    }
    used += ns;
  }
  *nseg = S;
}

// Partitions of the partition-first path (nmg_route.h): runs of consecutive
// keys, each at most kPartKeys keys and kPartEntries entries, and -- where
// the keys allow it -- at most kPartCells dense page cells over all threads,
// so that a partition's lookup tree, node records, object counters and page
// cells fit one workgroup's LDS.  A key range owns a range of table
// positions; `ids` (an online table, nmg_update_objects) maps a position to
// its entry id (null: the id is the position).  An online table's entries
// have their page cells in id order, scattered over the address order, so
// its partitions are not cut by cells (the cells of a partition whose span is
// too wide for LDS take global atomics).  Only for engines that count per
// object (NMG_F_MATCH_SAMPLES); the dump modes' per-sample output and the
// per-object levels are outputs of the local pass too (local_kernel's extras).
int build_partitions(nmg_engine* h, const uint64_t* keys, const uint32_t* entry_off, uint32_t K,
                            const std::vector<DevEntry>& dev, const uint32_t* ids) {
  h->rt = RouteTable();
  if (K <= kLdsNodes || !(h->flags & NMG_F_MATCH_SAMPLES)) return NMG_OK;
  if (ids) {  // the identity map is the offline case
    uint32_t e = 0;
    while (e < entry_off[K] && ids[e] == e) e++;
    if (e == entry_off[K]) ids = nullptr;
  }
  if (ids && h->tab.cells() >= (1ull << 31)) return NMG_OK;  // (cell indices of an online table: 32-bit)
  const uint64_t T = h->T;
  std::vector<PartInfo> parts;
  // an online table: the partition's dense cells packed in LDS in table
  // order (lrel: an entry's first LDS cell per table position; cmap: the
  // histogram cell of every packed cell, per partition from PartInfo::cmap)
  std::vector<uint32_t> lrel, cmap;
  if (ids) lrel.assign(entry_off[K], kEmpty32);
  uint32_t k = 0;
  while (k < K) {
    PartInfo pi;
    memset(&pi, 0, sizeof(pi));
    pi.k0 = k;
    pi.e0 = entry_off[k];
    pi.cmap = ~0u;
    uint64_t cb = ~0ull, ce = 0, cc = 0;  // dense cells in [cb, ce), cc of them
    while (k < K && k - pi.k0 < kPartKeys) {
      // a partition's keys span less than 2^(kAddrBits - 1) bytes, so that the
      // compact records' address field (relative to the partition's first key)
      // holds every address its objects cover: a run of keys across a wide gap
      // in the address space (the heap, then the stack) starts a new partition
      if (k > pi.k0 && keys[k] - keys[pi.k0] >= (1ull << (kAddrBits - 1))) break;
      const uint32_t ea = entry_off[k], eb = entry_off[k + 1];
      if (eb - pi.e0 > kPartEntries) {
        if (k == pi.k0) return NMG_OK;  // one address reused more than kPartEntries times: keep attribute_kernel
        break;
      }
      uint64_t ncb = cb, nce = ce, ncc = cc;
      for (uint32_t e = ea; e < eb; e++)
        if (dev[e].hist != kHistSparse) {
          const uint64_t np = h->tab.npages[dev[e].id];
          ncb = std::min<uint64_t>(ncb, dev[e].hist);
          nce = std::max<uint64_t>(nce, dev[e].hist + np);
          ncc += np;
        }
      if (k > pi.k0 && ncb != ~0ull && (ids ? ncc : nce - ncb) * T > kPartCells)
        break;  // (one key alone may exceed: global cells)
      cb = ncb;
      ce = nce;
      cc = ncc;
      k++;
    }
    pi.nk = k - pi.k0;
    pi.ne = entry_off[k] - pi.e0;
    pi.cb = cb == ~0ull ? 0 : cb;
    pi.span = cb == ~0ull ? 0 : (uint32_t)(ce - cb);
    pi.pages_lds = pi.span && (uint64_t)pi.span * T <= kPartCells;
    if (ids && cc && cc * T <= kPartCells) {  // online: the cells packed (cmap), always in LDS
      pi.cmap = (uint32_t)cmap.size();
      pi.span = (uint32_t)cc;
      pi.pages_lds = 1;
      uint32_t off = 0;
      for (uint32_t e = pi.e0; e < pi.e0 + pi.ne; e++)
        if (dev[e].hist != kHistSparse) {
          const uint32_t np = (uint32_t)h->tab.npages[dev[e].id];
          lrel[e] = off;
          for (uint32_t g = 0; g < np; g++) cmap.push_back((uint32_t)(dev[e].hist + g));
          off += np;
        }
    }
    const uint64_t kspan = keys[k - 1] - keys[pi.k0];
    while (pi.dshift < 63 && (kspan >> pi.dshift) >= kPartDir) pi.dshift++;
    parts.push_back(pi);
    if (parts.size() > kMaxParts) return NMG_OK;  // too many partitions for the route pass's LDS tree
  }
  const uint32_t P = (uint32_t)parts.size();
  // the compact records' timestamp base: the earliest allocation (a sample
  // before it can only match objects allocated at time 0, and escapes)
  h->route_tbase = ~0ull;
  for (const DevEntry& d : dev)
    if (d.alloc) h->route_tbase = std::min<uint64_t>(h->route_tbase, d.alloc);
  if (h->route_tbase == ~0ull) h->route_tbase = 0;
  // per partition: keys ascending with their newest entry's node record (the
  // exact one, read by the local pass's rare paths), its packed form and
  // info (the common path), and a directory over the key span: slot j starts
  // at first key + (j << dshift) and holds the index of the largest key <=
  // that start, the number of keys inside the slot (the last slot: every key
  // after its start) and the first kDirInline of those keys' offsets from the
  // slot start when they fit 16 bits (PartDir)
  const uint64_t tb = h->route_tbase;
  std::vector<uint64_t> pk((size_t)P * kPartSlots, ~0ull);
  std::vector<uint4> pn((size_t)P * kPartSlots * 2, make_uint4(0, 0, 0, 0));
  std::vector<uint4> ppn((size_t)P * kPartSlots, make_uint4(0, 0, 0, 0));
  std::vector<uint2> pinf((size_t)P * kPartSlots, make_uint2(kEmpty32, 0));
  std::vector<uint4> pdir((size_t)P * kPartDir, make_uint4(0, 0, 0, 0));
  std::vector<uint4> pold((size_t)P * kOldLds, make_uint4(0, 0, 0, 0));
  std::vector<uint32_t> poinf((size_t)P * kOldLds, kEmpty32);
  // an entry's page cell relative to its partition (as pe_info.x)
  auto cell_rel = [&](const PartInfo& pi, uint32_t e) -> uint32_t {
    const DevEntry& d = dev[e];
    return d.hist == kHistSparse ? kEmpty32 : pi.cmap != ~0u ? lrel[e] : (uint32_t)(d.hist - pi.cb);
  };
  // the quantised dates of an entry (never matching: ~0, 0)
  auto qdates = [&](const DevEntry& d, uint64_t tb, uint32_t& aq, uint32_t& fq) {
    if (d.free < tb) {
      aq = 0xffffffffu;
      fq = 0;
    } else {
      aq = (uint32_t)std::min<uint64_t>((d.alloc > tb ? d.alloc - tb : 0) >> kPnQShift, 0xffffffffull);
      fq = (uint32_t)std::min<uint64_t>((d.free - tb) >> kPnQShift, 0xffffffffull);
    }
  };
  for (uint32_t q = 0; q < P; q++) {
    const PartInfo& pi = parts[q];
    const uint64_t f = keys[pi.k0];
    for (uint32_t r = 0; r < pi.nk; r++) {
      const uint32_t kk = pi.k0 + r;
      const DevEntry& d = dev[entry_off[kk]];
      const size_t o = (size_t)q * kPartSlots + r;
      pk[o] = keys[kk];
      pn[2 * o] = make_uint4((uint32_t)d.addr, (uint32_t)(d.addr >> 32), (uint32_t)d.end, (uint32_t)(d.end >> 32));
      pn[2 * o + 1] = make_uint4((uint32_t)d.alloc, (uint32_t)(d.alloc >> 32), (uint32_t)d.free, (uint32_t)(d.free >> 32));
      const uint32_t older = entry_off[kk + 1] - entry_off[kk] > 1 ? 1u : 0u;
      const uint32_t hrel = cell_rel(pi, entry_off[kk]);
      // packed node (PackedNode): exact where the object's start or end
      // offset from the first key needs more than 32 bits -- unless it was
      // freed before the first allocation (the [stack], Q4): no non-escaped
      // sample can match it, whatever its bounds
      const uint64_t erel = d.end - f, brel = d.addr - f;
      const bool never = d.free < tb;
      const bool exact = !never && (d.addr < f || d.end < d.addr || (erel >> 32) != 0 || (brel >> 32) != 0);
      uint32_t aq, fq;
      qdates(d, tb, aq, fq);
      // the key's older entries in the partition's list (kOldLds) when they fit
      const uint32_t nold = entry_off[kk + 1] - entry_off[kk] - 1, lbase = entry_off[kk] - pi.e0 - r;
      bool old_lds = nold > 0 && nold < 2048 && lbase + nold <= kOldLds;
      for (uint32_t i = 1; old_lds && i <= nold; i++) {
        const uint32_t e = entry_off[kk] + i;
        const DevEntry& od = dev[e];
        uint32_t oa, of;
        qdates(od, tb, oa, of);
        uint4 v = make_uint4(0, oa, of, 0);
        if (od.free >= tb) {  // (else: never matches, bounds irrelevant)
          if (od.addr < f || od.end < od.addr || ((od.end - f) >> 32) != 0) {
            old_lds = false;
            break;
          }
          v.x = (uint32_t)(od.end - f);
          v.w = (uint32_t)(od.addr - f);
        }
        pold[(size_t)q * kOldLds + lbase + i - 1] = v;
        poinf[(size_t)q * kOldLds + lbase + i - 1] = cell_rel(pi, e);
      }
      ppn[o] = make_uint4(exact || never ? 0u : (uint32_t)erel, aq, fq,
                          (entry_off[kk] - pi.e0) | (older ? kPnOlder : 0u) | (exact ? kPnExact : 0u) |
                              (old_lds ? kPnOldLds | (nold << kPnOldShift) : 0u));
      pinf[o] = make_uint2(hrel, exact || never ? 0u : (uint32_t)brel);
    }
    uint32_t lo = 0;
    for (uint32_t j = 0; j < kPartDir; j++) {
      const uint64_t s0 = (uint64_t)j << pi.dshift;  // slot start relative to the first key
      while (lo + 1 < pi.nk && keys[pi.k0 + lo + 1] - f <= s0) lo++;
      uint32_t c = 0;
      while (lo + 1 + c < pi.nk &&
             (j == kPartDir - 1 || keys[pi.k0 + lo + 1 + c] - f < s0 + (1ull << pi.dshift)))
        c++;
      uint32_t off[kDirInline];
      bool inl = true;
      for (uint32_t i = 0; i < kDirInline; i++) {
        off[i] = 0xffffu;
        if (i < c) {
          const uint64_t v = keys[pi.k0 + lo + 1 + i] - f - s0;
          if (v >> 16) inl = false;
          else off[i] = (uint32_t)v;
        }
      }
      pdir[(size_t)q * kPartDir + j] =
          make_uint4(lo | (c << 10) | ((inl && c ? 1u : 0u) << 21), off[0] | (off[1] << 16), off[2] | (off[3] << 16),
                     off[4] | (off[5] << 16));
    }
  }
  // the route pass's partition search: the partitions' first keys ascending,
  // and a directory over them (route_segments)
  std::vector<uint64_t> pb(kMaxParts + 1, ~0ull);
  for (uint32_t q = 0; q < P; q++) pb[q] = keys[parts[q].k0];
  std::vector<uint16_t> rdir;
  route_segments(pb.data(), P, h->rsegs, &h->nrsegs, rdir);
  // partitions whose entries all have free_date 0 (RouteParams::pdead): the
  // route pass keeps only their timestamp-0 samples, the others cannot match
  std::vector<uint32_t> dead((kMaxParts + 1) / 32, 0u);
  for (uint32_t q = 0; q < P; q++) {
    bool d = true;
    for (uint32_t e = parts[q].e0; d && e < parts[q].e0 + parts[q].ne; e++) d = dev[e].free == 0;
    if (d) dead[q >> 5] |= 1u << (q & 31);
  }
  RouteTable& rt = h->rt;
  HIP_TRY(h, alloc_copy(h, rt.d_pdead, dead));
  HIP_TRY(h, alloc_copy(h, rt.d_parts, parts));
  HIP_TRY(h, alloc_copy(h, rt.d_pbounds, pb));
  HIP_TRY(h, alloc_copy(h, rt.d_pdir, rdir));
  HIP_TRY(h, alloc_copy(h, rt.d_pe_keys, pk));
  HIP_TRY(h, alloc_copy(h, rt.d_pe_nodes, pn));
  HIP_TRY(h, alloc_copy(h, rt.d_pe_pnode, ppn));
  HIP_TRY(h, alloc_copy(h, rt.d_pe_old, pold));
  HIP_TRY(h, alloc_copy(h, rt.d_pe_oinf, poinf));
  HIP_TRY(h, alloc_copy(h, rt.d_pe_info, pinf));
  HIP_TRY(h, alloc_copy(h, rt.d_pe_dir, pdir));
  if (ids) {
    HIP_TRY(h, alloc_copy(h, rt.d_pe_ids, ids, entry_off[K]));
    HIP_TRY(h, alloc_copy(h, rt.d_pe_lrel, lrel));
    if (!cmap.empty()) HIP_TRY(h, alloc_copy(h, rt.d_pe_cmap, cmap));
  }
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // (pageable sources)
  rt.nparts = P;
  rt.ok = true;
  return NMG_OK;
}

extern "C" int nmg_set_objects(nmg_engine* h, const uint64_t* keys, const uint32_t* entry_off,
                               uint32_t nb_keys, const nmg_object* entries, uint32_t nb_entries) {
  if (h) h->epoch++;
  if (h) h->counters_fresh = false;
  if (h) h->snap.lay.meta_dirty = h->cprep.lay.meta_dirty = h->place.obj_dirty = true;
  Range range("nmg_set_objects");
  if (!h || (nb_keys && (!keys || !entry_off)) || (nb_entries && !entries))
    return NMG_ERR_INVALID;
  int rc = check_table(h, keys, entry_off, nb_keys, nb_entries);
  if (rc) return rc;
  if (nb_entries >= (1u << 31)) return fail(h, NMG_ERR_RANGE, "too many entries");
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  free_table(h);  // (released before the new ones are allocated: no second table's worth of HBM)
  h->cnt = Counters();
  h->tl = Timeline();  // (a timeline is laid out for one table)
  h->cost = PageCost();  // (and so are the page cost cells)
  h->lk.K = nb_keys;
  h->E = nb_entries;

  // page-histogram layout: dense [page][thread] block per entry within the
  // budget, otherwise sparse hashed cells (e.g. the 412 GB [stack] range)
  EntryTable& tab = h->tab;
  tab = EntryTable();
  tab.cur.threads = h->T;
  tab.cur.budget_cells = h->hist_budget / 4;
  tab.resize(nb_entries);
  h->order.clear();
  const bool want_hist = (h->flags & NMG_F_PAGE_HIST) && (h->flags & NMG_F_MATCH_SAMPLES);
  for (uint32_t e = 0; e < nb_entries; e++) {
    const nmg_object& o = entries[e];
    tab.describe(e, o);
    tab.npages[e] = o.buffer_size / kPageSize + 1;
    if (want_hist && tab.place(e, tab.npages[e], false) == kPlaceSparseFull)
      return fail(h, NMG_ERR_CAPACITY, "too many sparse entries");
    tab.dev_entries[e] = tab.dev_entry(e, o);
  }
  tab.cur.cells = tab.cur.padded_cells();
  HIP_TRY(h, alloc_copy(h, h->d_entries, tab.dev_entries));
  rc = build_lookup(h, h->lk, keys, entry_off, nb_keys, tab.dev_entries, h->d_entries);
  if (rc) return rc;
  rc = build_partitions(h, keys, entry_off, nb_keys, tab.dev_entries, nullptr);
  if (rc) return rc;
  h->cnt.set_sizes(nb_entries, h->flags & NMG_F_OBJECT_LEVELS);
  HIP_TRY(h, h->cnt.d_sum64.alloc(h->cnt.n_sum64));
  HIP_TRY(h, h->cnt.d_min64.alloc(h->cnt.n_min64));
  HIP_TRY(h, h->cnt.d_max64.alloc(h->cnt.n_max64));
  HIP_TRY(h, h->d_found.reserve(1));
  if (nb_entries > kObjSlots) {  // hashed object mode (see launch_attribution)
    HIP_TRY(h, h->cnt.d_pk64.alloc((size_t)nb_entries * 2));
    HIP_TRY(h, hipMemset(h->cnt.d_pk64, 0, (size_t)nb_entries * 2 * 8));
  }
  if (h->tab.cells()) HIP_TRY(h, h->cnt.d_hist.alloc(h->tab.cells() * h->T));
  if (!h->tab.sparse_entries.empty()) {
    HIP_TRY(h, h->cnt.d_sparse_keys.alloc(h->sparse_cap));
    HIP_TRY(h, h->cnt.d_sparse_vals.alloc(h->sparse_cap));
    HIP_TRY(h, h->cnt.d_sparse_dirty.alloc(2));
    const uint32_t ones[2] = {1u, 1u};  // the first reset clears the fresh table
    HIP_TRY(h, hipMemcpy(h->cnt.d_sparse_dirty, ones, 8, hipMemcpyHostToDevice));
  }
  h->have_table = true;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  for (nmg_engine* w : h->workers) {  // multi-GPU: the table on every device
    const int rc = nmg_set_objects(w, keys, entry_off, nb_keys, entries, nb_entries);
    if (rc) return fail(h, rc, w->last_error);
  }
  return nmg_reset_counters(h);
}


// The access timeline's cells for the current table: every entry with dense
// page cells (CellCursor::place) and at least min_object_bytes gets
// nb_bins * T * R cells, in id order; its base and R go into pad1 of its
// by-id record (tl_pad; kTlNone for the others), which is what the kernels
// gather.  The table-order copies of an nmg_update_objects table (chain, node
// records) carry pad1 too but nothing reads it there, so a later accepted
// update -- it rebuilds those from the host records -- keeps the bases.
extern "C" int nmg_set_timeline(nmg_engine* h, const nmg_timeline_options* o) {
  if (!h) return NMG_ERR_INVALID;
  h->epoch++;
  if (h->multi || !h->workers.empty()) return fail(h, NMG_ERR_INVALID, "nmg_set_timeline: not on a multi-GPU handle");
  constexpr uint32_t kNeed = NMG_F_MATCH_SAMPLES | NMG_F_PAGE_HIST;
  if ((h->flags & kNeed) != kNeed)
    return fail(h, NMG_ERR_INVALID, "nmg_set_timeline needs an engine created with NMG_F_MATCH_SAMPLES | NMG_F_PAGE_HIST");
  if (o && (o->bin_shift > 63 || o->nb_bins < 1 || o->nb_bins > 4096 || o->row_shift > 20 || o->reserved != 0))
    return fail(h, NMG_ERR_INVALID, "nmg_set_timeline: option out of range (bin_shift <= 63, nb_bins 1..4096, "
                                    "row_shift <= 20, reserved 0)");
  if (!h->have_table) return fail(h, NMG_ERR_STATE, "nmg_set_timeline before nmg_set_objects");
  if (h->streaming) return fail(h, NMG_ERR_STATE, "nmg_set_timeline while a stream is open");
  HIP_TRY(h, hipSetDevice(h->device));
  int rc = route_settle(h);
  if (rc) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // launches in flight read the entries and the cells
  if (!o) {
    h->tl = Timeline();
    return NMG_OK;
  }
  EntryTable& tab = h->tab;
  const uint32_t E = h->E, T = h->T;
  Timeline t;
  t.opt = *o;
  if (const char* r = getenv("NMG_TL_ROUNDS")) t.rounds = (uint32_t)std::min(64, std::max(0, atoi(r)));  // (see kTlRounds)
  const uint64_t budget = o->budget_bytes ? o->budget_bytes : (1ull << 30);
  unsigned __int128 need = 0;
  for (uint32_t e = 0; e < E; e++) {
    if (tab.hist_base[e] == kHistSparse || tab.buffer_size[e] < o->min_object_bytes) continue;
    const uint64_t R = (tab.buffer_size[e] / kPageSize + 1 + (1ull << o->row_shift) - 1) >> o->row_shift;
    if (need <= 0xffffffffull) {  // (past it the layout is refused below: only the size is still summed)
      t.ids.push_back(e);
      t.base.push_back((uint32_t)need);
      t.nrows.push_back((uint32_t)R);  // (dense: R <= pages <= kMaxEntryCells)
    }
    need += (unsigned __int128)R * o->nb_bins * T;
  }
  const unsigned __int128 bytes = need * 4;
  if (need > 0xffffffffull || bytes > budget) {
    char msg[160];
    snprintf(msg, sizeof(msg), "nmg_set_timeline: the cells need %llu bytes (budget %llu, at most 2^32 - 1 cells)",
             bytes > ~0ull ? ~0ull : (unsigned long long)bytes, (unsigned long long)budget);
    return fail(h, NMG_ERR_CAPACITY, msg);
  }
  t.ncells = (uint64_t)need;
  t.base.push_back((uint32_t)t.ncells);
  // the new layout beside the current one; committed once everything is uploaded
  std::vector<DevEntry> dev = tab.dev_entries;
  for (DevEntry& d : dev) d.pad1 = kTlNone;
  for (size_t k = 0; k < t.ids.size(); k++) dev[t.ids[k]].pad1 = tl_pad(t.base[k], t.nrows[k]);
  HIP_TRY(h, t.d_cells.alloc(t.ncells));
  HIP_TRY(h, hipMemsetAsync(t.d_cells, 0, t.ncells * 4, h->stream));
  HIP_TRY(h, alloc_copy(h, t.d_ids, t.ids));
  HIP_TRY(h, alloc_copy(h, t.d_base, t.base));
  HIP_TRY(h, alloc_copy(h, t.d_nrows, t.nrows));
  if (E) HIP_TRY(h, hipMemcpyAsync(h->d_entries, dev.data(), (size_t)E * sizeof(DevEntry), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // (pageable sources)
  tab.dev_entries = std::move(dev);
  t.on = true;
  h->tl = std::move(t);
  return NMG_OK;
}

// The page cost cells for the current table (the rule is in
// include/numamma_gpu.h): one u64 per cell of the page histogram, at its
// index, zeroed.  Nothing in the table changes: the kernels find a cell from
// the entry's histogram base, which they have.
extern "C" int nmg_set_page_cost(nmg_engine* h, const nmg_page_cost_options* o) {
  return nmg_set_page_cost_ex(h, o, NMG_COST_SCOPE_DENSE);
}

// scope NMG_COST_SCOPE_ALL: also one u64 per slot of the sparse page table
// (PageCost::d_sparse), within the same budget, whenever that table exists.
extern "C" int nmg_set_page_cost_ex(nmg_engine* h, const nmg_page_cost_options* o, uint32_t scope) {
  if (!h) return NMG_ERR_INVALID;
  h->epoch++;
  h->place.obj_dirty = true;  // (the object groups' members depend on the scope)
  if (scope > NMG_COST_SCOPE_ALL)
    return fail(h, NMG_ERR_INVALID, "nmg_set_page_cost_ex: scope is NMG_COST_SCOPE_DENSE or NMG_COST_SCOPE_ALL");
  if (h->multi || !h->workers.empty()) return fail(h, NMG_ERR_INVALID, "nmg_set_page_cost: not on a multi-GPU handle");
  constexpr uint32_t kNeed = NMG_F_MATCH_SAMPLES | NMG_F_PAGE_HIST;
  if ((h->flags & kNeed) != kNeed)
    return fail(h, NMG_ERR_INVALID, "nmg_set_page_cost needs an engine created with NMG_F_MATCH_SAMPLES | NMG_F_PAGE_HIST");
  if (o && (o->bucket_mask == 0 || o->bucket_mask >= (1u << 19) || o->access_mask == 0 || o->access_mask > 3 ||
            o->metric > NMG_COST_WEIGHT || o->reserved != 0))
    return fail(h, NMG_ERR_INVALID, "nmg_set_page_cost: option out of range (bucket_mask 1..2^19 - 1, access_mask 1..3, "
                                    "metric 0 or 1, reserved 0)");
  if (!h->have_table) return fail(h, NMG_ERR_STATE, "nmg_set_page_cost before nmg_set_objects");
  if (h->streaming) return fail(h, NMG_ERR_STATE, "nmg_set_page_cost while a stream is open");
  HIP_TRY(h, hipSetDevice(h->device));
  int rc = route_settle(h);
  if (rc) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // launches in flight add to the cells
  if (!o) {
    h->cost = PageCost();
    return NMG_OK;
  }
  PageCost c;
  c.opt = *o;
  c.budget = o->budget_bytes ? o->budget_bytes : (1ull << 30);
  if (const char* r = getenv("NMG_COST_ROUNDS")) c.rounds = (uint32_t)std::min(64, std::max(0, atoi(r)));  // (see kCostRounds)
  c.scope = scope;
  const uint64_t ncells = h->tab.cells() * h->T;  // (within the histogram's budget: no overflow)
  const uint64_t nsparse = scope == NMG_COST_SCOPE_ALL && h->cnt.d_sparse_keys ? h->sparse_cap : 0;  // (<= 2^31)
  if ((ncells + nsparse) * 8 > c.budget) {
    char msg[160];
    snprintf(msg, sizeof(msg), "nmg_set_page_cost: the cells need %llu bytes (budget %llu)",
             (unsigned long long)((ncells + nsparse) * 8), (unsigned long long)c.budget);
    return fail(h, NMG_ERR_CAPACITY, msg);
  }
  if (ncells) {
    HIP_TRY(h, c.d_cells.alloc(ncells));
    HIP_TRY(h, hipMemsetAsync(c.d_cells, 0, ncells * 8, h->stream));
  }
  if (nsparse) {
    HIP_TRY(h, c.d_sparse.alloc(nsparse));
    HIP_TRY(h, hipMemsetAsync(c.d_sparse, 0, nsparse * 8, h->stream));
  }
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  c.on = true;
  h->cost = std::move(c);
  return NMG_OK;
}

// A live --online-analysis table (nmg_update_objects) may hold entries the
// engine has not seen: objects created since the previous alarm (ids E ..
// newE - 1, _init_mem_info's next id, mem_analyzer.c:567-568, with their
// counters from creation, :569-572), and objects whose size at free
// (ma_record_free, :1287) outgrew their page cells.  New entries get page
// cells like nmg_set_objects gives them (dense within the budget, sparse
// otherwise); a dense entry that outgrew its cells moves to a new range with
// its counts.  Every id-indexed counter array is re-laid out on the device
// for the new entry count, counters kept.  (The stream is idle here.)
int grow_entries(nmg_engine* h, uint32_t newE, const uint32_t* ids, const nmg_object* objs, uint32_t n) {
  const uint32_t oldE = h->E;
  const uint64_t T = h->T;
  const bool want_hist = (h->flags & NMG_F_PAGE_HIST) && (h->flags & NMG_F_MATCH_SAMPLES);
  const bool levels = h->flags & NMG_F_OBJECT_LEVELS;
  EntryTable& tab = h->tab;
  const CellCursor cur0 = tab.cur;
  const uint64_t oldCells = cur0.cells;
  // The table is changed in place below, the cells and pages of every old
  // entry that grows journalled first; every error return undoes it (the new
  // entries dropped, the journal put back), so that a failed update keeps the
  // engine as it was.
  struct Old {
    uint32_t id;
    uint64_t hist, np;
  };
  std::vector<Old> changed;
  auto fail_rb = [&](int code, const std::string& msg) {
    for (auto it = changed.rbegin(); it != changed.rend(); ++it) {
      tab.dev_entries[it->id].hist = tab.hist_base[it->id] = it->hist;
      tab.npages[it->id] = it->np;
    }
    tab.truncate(oldE, cur0);
    return fail(h, code, msg);
  };
  tab.resize(newE);
  for (uint32_t j = 0; j < n; j++) {
    const uint32_t id = ids[j];
    const uint64_t np = objs[j].buffer_size / kPageSize + 1;
    if (id >= oldE) {
      tab.npages[id] = np;
      if (want_hist && tab.place(id, np, false) == kPlaceSparseFull)
        return fail_rb(NMG_ERR_CAPACITY, "too many sparse entries");
    } else if (np > tab.npages[id]) {
      changed.push_back({id, tab.hist_base[id], tab.npages[id]});
      if (want_hist && tab.hist_base[id] != kHistSparse && tab.place(id, np, true) != kPlaceDense)
        return fail_rb(NMG_ERR_CAPACITY, "an object outgrew its page cells past the histogram budget");
      tab.npages[id] = np;
    }
  }
  const uint64_t cells = tab.cur.cells = tab.cur.padded_cells();
  // the page cost cells follow the histogram's layout, within their own budget
  const bool with_cost = h->cost.on;
  const bool new_sparse = cur0.nsparse == 0 && tab.cur.nsparse && !h->cnt.d_sparse_keys;
  // (NMG_COST_SCOPE_ALL: plus the sparse table's, the one this update brings included)
  const bool cost_sparse = with_cost && h->cost.scope == NMG_COST_SCOPE_ALL && (h->cnt.d_sparse_keys || new_sparse);
  const uint64_t cost_bytes = (cells * T + (cost_sparse ? h->sparse_cap : 0)) * 8;
  if (with_cost && cost_bytes > h->cost.budget) {
    char msg[160];
    snprintf(msg, sizeof(msg), "nmg_update_objects: the page cost cells need %llu bytes (budget %llu)",
             (unsigned long long)cost_bytes, (unsigned long long)h->cost.budget);
    return fail_rb(NMG_ERR_CAPACITY, msg);
  }
  // id-indexed counters, re-laid out for newE entries
  const uint64_t n_sum = sum64_words(newE, levels), n_min = min64_words(newE);
  DevBuf<uint64_t> sum, mn, skeys, cost, scost;
  DevBuf<uint32_t> hist, svals, sdirty;
  DevBuf<unsigned long long> pk;
  DevBuf<DevEntry> ent;
  // (the new arrays are released on return, after the copies into them have drained)
  auto undo = [&](hipError_t e, const char* what) {
    (void)hipStreamSynchronize(h->stream);
    return fail_rb(NMG_ERR_HIP, std::string("nmg_update_objects: ") + what + ": " + hipGetErrorString(e));
  };
  hipError_t e;
  if ((e = sum.alloc(n_sum)) != hipSuccess) return undo(e, "counters");
  if ((e = mn.alloc(n_min)) != hipSuccess) return undo(e, "ordinals");
  if (cells && cells * T != oldCells * T && (e = hist.alloc(cells * T)) != hipSuccess)
    return undo(e, "page histogram");
  if (hist && with_cost && (e = cost.alloc(cells * T)) != hipSuccess) return undo(e, "page cost cells");
  if (newE > kObjSlots && (e = pk.alloc((size_t)newE * 2)) != hipSuccess) return undo(e, "packed counters");
  if ((e = ent.alloc(newE)) != hipSuccess) return undo(e, "entries");
  hipStream_t st = h->stream;
  if (new_sparse) {  // the first sparse entry: its table
    if ((e = skeys.alloc(h->sparse_cap)) != hipSuccess || (e = svals.alloc(h->sparse_cap)) != hipSuccess ||
        (e = sdirty.alloc(2)) != hipSuccess || (e = hipMemsetAsync(skeys, 0xff, h->sparse_cap * 8, st)) != hipSuccess ||
        (e = hipMemsetAsync(svals, 0, h->sparse_cap * 4, st)) != hipSuccess ||
        (e = hipMemsetAsync(sdirty, 0, 2 * 4, st)) != hipSuccess)
      return undo(e, "sparse page table");
    if (cost_sparse && ((e = scost.alloc(h->sparse_cap)) != hipSuccess ||
                        (e = hipMemsetAsync(scost, 0, h->sparse_cap * 8, st)) != hipSuccess))
      return undo(e, "sparse page cost cells");
  }
  // the global words as they are, the count/weight rows with the new stride,
  // the level rows and ordinals behind them, the error word at its new place
  const uint64_t* osum = h->cnt.d_sum64;
  const uint64_t* omin = h->cnt.d_min64;
  if ((e = hipMemsetAsync(sum, 0, n_sum * 8, st)) != hipSuccess ||
      (e = hipMemcpyAsync(sum, osum, kCwBase * 8, hipMemcpyDeviceToDevice, st)) != hipSuccess ||
      (oldE && (e = hipMemcpy2DAsync(sum + kCwBase, (size_t)newE * 8, osum + kCwBase, (size_t)oldE * 8, (size_t)oldE * 8,
                                     kCwRows, hipMemcpyDeviceToDevice, st)) != hipSuccess) ||
      (levels && oldE &&
       (e = hipMemcpyAsync(sum + levels_base(newE), osum + levels_base(oldE), (size_t)oldE * 2 * kLevelWords * 8,
                           hipMemcpyDeviceToDevice, st)) != hipSuccess) ||
      (e = hipMemsetAsync(mn, 0xff, n_min * 8, st)) != hipSuccess ||
      (e = hipMemcpyAsync(mn, omin, first_index(oldE) * 8, hipMemcpyDeviceToDevice, st)) != hipSuccess ||
      (e = hipMemcpyAsync(mn + error_index(newE), omin + error_index(oldE), 8, hipMemcpyDeviceToDevice, st)) !=
          hipSuccess ||
      (pk && (e = hipMemsetAsync(pk, 0, (size_t)newE * 2 * 8, st)) != hipSuccess) ||
      (e = hipMemcpyAsync(ent, tab.dev_entries.data(), (size_t)newE * sizeof(DevEntry), hipMemcpyHostToDevice, st)) !=
          hipSuccess)
    return undo(e, "re-layout");
  if (hist) {  // [thread][cell] rows with the new stride; moved entries' counts to their new range
    if ((e = hipMemsetAsync(hist, 0, cells * T * 4, st)) != hipSuccess ||
        (oldCells && (e = hipMemcpy2DAsync(hist, cells * 4, h->cnt.d_hist, oldCells * 4, oldCells * 4, T,
                                           hipMemcpyDeviceToDevice, st)) != hipSuccess))
      return undo(e, "page histogram re-layout");
    for (const Old& m : changed)  // (hist_base changed: a dense entry that moved)
      if (m.hist != tab.hist_base[m.id] &&
          ((e = hipMemcpy2DAsync(hist + tab.hist_base[m.id], cells * 4, hist + m.hist, cells * 4, m.np * 4, T,
                                 hipMemcpyDeviceToDevice, st)) != hipSuccess ||
           (e = hipMemset2DAsync(hist + m.hist, cells * 4, 0, m.np * 4, T, st)) != hipSuccess))
        return undo(e, "page cells of a grown object");
  }
  if (cost) {  // the same re-layout with 8-byte cells
    const uint64_t* ocost = h->cost.d_cells;
    if ((e = hipMemsetAsync(cost, 0, cells * T * 8, st)) != hipSuccess ||
        (oldCells && ocost && (e = hipMemcpy2DAsync(cost, cells * 8, ocost, oldCells * 8, oldCells * 8, T,
                                                    hipMemcpyDeviceToDevice, st)) != hipSuccess))
      return undo(e, "page cost re-layout");
    for (const Old& m : changed)
      if (m.hist != tab.hist_base[m.id] &&
          ((e = hipMemcpy2DAsync(cost + tab.hist_base[m.id], cells * 8, cost + m.hist, cells * 8, m.np * 8, T,
                                 hipMemcpyDeviceToDevice, st)) != hipSuccess ||
           (e = hipMemset2DAsync(cost + m.hist, cells * 8, 0, m.np * 8, T, st)) != hipSuccess))
        return undo(e, "page cost cells of a grown object");
  }
  if ((e = hipStreamSynchronize(st)) != hipSuccess) return undo(e, "re-layout");
  // commit: the old arrays are released as the new ones move in
  if (!h->lk.own_chain) h->lk.chain = ent;  // (the table order is still the id order)
  h->cnt.d_sum64 = std::move(sum);
  h->cnt.d_min64 = std::move(mn);
  h->cnt.d_pk64 = std::move(pk);
  h->d_entries = std::move(ent);
  if (hist) h->cnt.d_hist = std::move(hist);
  if (cost) h->cost.d_cells = std::move(cost);
  h->cnt.set_sizes(newE, levels);
  h->E = newE;
  if (new_sparse) {
    h->cnt.d_sparse_keys = std::move(skeys);
    h->cnt.d_sparse_vals = std::move(svals);
    h->cnt.d_sparse_dirty = std::move(sdirty);
    if (scost) h->cost.d_sparse = std::move(scost);
  }
  return NMG_OK;
}

// --online-analysis: the table at an alarm, counters kept (mem_sampling.c:953-954
// against the live mem_list).  Entry ids index the counters: ids of the
// nmg_set_objects table, and (live hosts) ids past it for objects created
// since (grow_entries).  The report describes each entry as the latest table
// lists it, in the order of the latest table that lists every entry.
extern "C" int nmg_update_objects(nmg_engine* h, const uint64_t* keys, const uint32_t* entry_off,
                                  uint32_t nb_keys, const uint32_t* entry_ids, const nmg_object* objects) {
  if (h) h->epoch++;
  if (h) h->counters_fresh = false;  // (grown objects' page cells move)
  if (h) h->snap.lay.meta_dirty = h->cprep.lay.meta_dirty = h->place.obj_dirty = true;
  Range range("nmg_update_objects");
  if (!h || (nb_keys && (!keys || !entry_off || !entry_ids || !objects))) return NMG_ERR_INVALID;
  if (!h->have_table) return fail(h, NMG_ERR_STATE, "nmg_update_objects before nmg_set_objects");
  const uint32_t n = nb_keys ? entry_off[nb_keys] : 0;
  int rc = check_table(h, keys, nb_keys ? entry_off : nullptr, nb_keys, n);
  if (rc) return rc;
  // with a timeline set, its layout stands: no new entry, no size other than the one it was laid out for
  if (h->tl.on)
    for (uint32_t j = 0; j < n; j++)
      if (entry_ids[j] >= h->E || objects[j].buffer_size != h->tab.buffer_size[entry_ids[j]])
        return fail(h, NMG_ERR_STATE, "nmg_update_objects: with a timeline set, a table may only list existing "
                                      "entries with their sizes unchanged (drop it with nmg_set_timeline(h, NULL))");
  // ids: each at most once; new ones (>= E) consecutive from E
  uint32_t newE = h->E;
  for (uint32_t j = 0; j < n; j++) newE = std::max(newE, entry_ids[j] + 1);
  if (entry_ids && n && (uint64_t)newE > (1ull << 31)) return fail(h, NMG_ERR_RANGE, "too many entries");
  uint64_t nb_grown = 0;
  {
    std::vector<uint8_t> seen(newE, 0);
    for (uint32_t j = 0; j < n; j++) {
      const uint32_t id = entry_ids[j];
      if (seen[id]) return fail(h, NMG_ERR_INVALID, "an entry id listed twice in one table");
      seen[id] = 1;
      if (id < h->E && objects[j].buffer_size / kPageSize + 1 > h->tab.npages[id]) nb_grown++;
    }
    for (uint32_t id = h->E; id < newE; id++)
      if (!seen[id]) return fail(h, NMG_ERR_RANGE, "new entry ids must be consecutive from the current entry count");
  }
  HIP_TRY(h, hipSetDevice(h->device));
  if (h->streaming) {  // the open chunk belongs to the previous alarms' table
    rc = stream_flush(h);
    if (rc) return rc;
  }
  rc = route_settle(h);  // (reads the pool only, not the table)
  if (rc) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // launches in flight read the old table and counters
  if (h->multi_pending) {  // merges in flight write the counters being re-laid out
    rc = multi_finish(h);
    if (rc) return rc;
  }
  if (newE > h->E || nb_grown) {
    rc = grow_entries(h, newE, entry_ids, objects, n);
    if (rc) return rc;
  }
  std::vector<DevEntry> chain(n);
  for (uint32_t j = 0; j < n; j++) chain[j] = h->tab.dev_entry(entry_ids[j], objects[j]);
  h->rt = RouteTable();  // (the partitions describe the previous table)
  // build the alarm's lookup beside the current one; keep the current one if that fails
  LookupSet next;
  rc = build_lookup(h, next, keys, entry_off, nb_keys, chain, nullptr);
  if (rc == NMG_OK && hipStreamSynchronize(h->stream) != hipSuccess)
    rc = fail(h, NMG_ERR_HIP, "nmg_update_objects: table upload failed");
  if (rc) {
    (void)hipStreamSynchronize(h->stream);  // (`next` is released on return, after its uploads)
    return rc;
  }
  h->lk = std::move(next);
  // the report's view: every listed entry as this table lists it, and this
  // table's order when it lists every entry (ma_finalize walks the table it
  // has at exit, FOREACH_HASH, mem_analyzer.c:1381-1383)
  for (uint32_t j = 0; j < n; j++) h->tab.describe(entry_ids[j], objects[j]);
  if (n == h->E) {
    bool identity = true;
    for (uint32_t j = 0; j < n && identity; j++) identity = entry_ids[j] == j;
    if (identity) h->order.clear();
    else h->order.assign(entry_ids, entry_ids + n);
  } else if (!h->order.empty()) {
    // a partial table that brought new entries: they follow the known ones,
    // in id order, until a table lists every entry
    for (uint32_t id = (uint32_t)h->order.size(); id < h->E; id++) h->order.push_back(id);
  }
  // the alarm table's partitions.  The new table is committed above, so a
  // failure here is not the update's: the table stays on attribute_kernel
  // (no partitions) and the update goes on to the workers, which must get
  // the same table (a half-applied update would leave them on the old one).
  if (build_partitions(h, keys, entry_off, nb_keys, chain, entry_ids) != NMG_OK) {
    (void)hipGetLastError();
    h->rt = RouteTable();
  }
  for (nmg_engine* w : h->workers) {  // multi-GPU: the table on every device
    rc = nmg_update_objects(w, keys, entry_off, nb_keys, entry_ids, objects);
    if (rc) return fail(h, rc, w->last_error);
  }
  return NMG_OK;
}
