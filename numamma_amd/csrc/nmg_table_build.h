// nmg_table_build.h -- the object table as the kernels read it: the formats
// (constants, records, directory slots) and the builders that turn a sorted
// table into those arrays on the host.  This is the one definition of the
// table formats; the comments beside the constants are their specification.
// Plain C++ (no HIP): the engine (nmg_table.hip) uploads what the builders
// return, tests/c/nmg_table_build_host.cpp checks it on the CPU.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "nmg_internal.h"

namespace nmg {

constexpr uint32_t kLdsNodes = 1023;           // keys held in LDS with their node records (<= 10 levels)
// Larger tables: up to 4095 fences (every S-th key) in a 12-level Eytzinger
// tree in LDS, then one load from a per-fence-bucket directory in global memory
constexpr uint32_t kFenceLevels = 12;
constexpr uint32_t kMaxFences = (1u << kFenceLevels) - 1;
constexpr uint32_t kShiftSearch = 0xff;        // bucket without a directory: binary search of its keys
constexpr uint32_t kEmpty32 = 0xffffffffu;

// One table entry (64 B).  The node array holds, for node k, a copy of its
// newest entry with `first` = its entry id and `count` = the node's number of
// entries, so the common one-entry node costs a single dependent load.
struct DevEntry {
  uint64_t addr;   // buffer_addr
  uint64_t end;    // buffer_addr + buffer_size (mod 2^64, as the reference's void* sum)
  uint64_t alloc;  // alloc_date
  uint64_t free;   // free_date
  uint64_t hist;   // dense histogram base cell, or kHistSparse
  uint32_t sidx;   // sparse index (valid when hist == kHistSparse && sidx != ~0u)
  uint32_t id;     // entry id: the counters' index (node records: of the node's newest entry)
  uint32_t count;  // (node records) entries of the node
  uint32_t first;  // (node records) table position of the newest entry; the older ones follow it
  uint64_t pad1;
};
static_assert(sizeof(DevEntry) == 64, "DevEntry");

// What the device reads as uint2 / uint4 (nmg_table.hip asserts that size and
// field order match)
struct Word8 {
  uint32_t x, y;
};
struct Word16 {
  uint32_t x, y, z, w;
};

constexpr uint32_t kPartLevels = 11;
constexpr uint32_t kMaxParts = (1u << kPartLevels) - 1;
// route pass: a sample's partition from a directory over the partition starts
// (RSeg): its segment by comparisons with the segment starts (kernel
// arguments), its slot's entry (u16: last partition starting at or before the
// slot start | starts inside the slot << 11, 31 = to the segment's end), then
// a binary search over those few starts (sorted, in LDS)
constexpr uint32_t kRouteDir = 4096;
constexpr uint32_t kRouteSegs = 8;
constexpr uint32_t kDirCntSat = 31;
struct RSeg {
  uint64_t start;   // first partition start of the segment (~0: unused)
  uint32_t base;    // first directory slot
  uint32_t nslots;  // slots (>= 1)
  uint32_t shift;   // slot j covers [start + (j << shift), + 2^shift); the last slot: to the next segment
  uint32_t qlast;   // last partition of the segment
};
constexpr uint32_t kPartKeys = 1023;       // local pass: keys per partition in LDS (sorted)
constexpr uint32_t kPartSlots = 1024;      // per-partition table stride
constexpr uint32_t kPartDir = 1024;        // directory slots per partition (radix over its key span)
// PartDir, one directory slot (16 B): x = largest key index <= slot start
// (10 bits) | keys inside the slot (11) << 10 | inline (1) << 21; y, z, w =
// the first kDirInline inner keys' offsets from the slot start (u16 pairs,
// 0xffff past the count), valid when `inline` (every listed offset < 2^16):
// a lookup counts the offsets <= its own and reads keys only past them
constexpr uint32_t kDirInline = 6;
// PackedNode, a key's newest entry for the local pass's common path (16 B):
//   x = end - first key, y = alloc_q, z = free_q, w = table position - e0
//   (11 bits) | kPnOlder | kPnExact | kPnOldLds | older entries << kPnOldShift
// with alloc_q / free_q = (date - tbase) >> kPnQShift, saturated to 32 bits
// (an entry freed before tbase: alloc_q = ~0, free_q = 0, no sample
// matches); pe_info.y = buffer_addr - first key.  A sample whose quantised
// timestamp equals either bound, or a key marked exact (its object's start or
// end offset needs more than 32 bits), is decided on the exact node record.
constexpr uint32_t kPnQShift = 8;
constexpr uint32_t kPnOlder = 1u << 11, kPnExact = 1u << 12;
// The older entries of a partition's reused keys (the LIFO chain past the
// newest, tools/hash.c:108-114), in table order, up to kOldLds per partition:
// x = end - first key, y = alloc_q, z = free_q, w = buffer_addr - first key
// (an entry freed before tbase: all zero but y = ~0), and per entry its page
// cell (pe_oinf, as PartInfo's info.x).  A key has them in the list
// (kPnOldLds) when all fit: the list index of its i-th older entry is its
// table position - e0 - key index + i - 1.  Otherwise, or when a quantised
// date is ambiguous, the lookup walks the chain in global memory.
constexpr uint32_t kOldLds = 512;
constexpr uint32_t kPnOldLds = 1u << 13, kPnOldShift = 16;
constexpr uint32_t kPartEntries = 1536;    // entries per partition (LDS object counters)
constexpr uint32_t kPartCells = 28672;     // u16 page cells per partition: nb_threads x cell span
// the compact records' address field (nmg_route.h), relative to the
// partition's first key: a partition's keys span less than 2^(kAddrBits - 1)
constexpr uint32_t kAddrBits = 40;

// One partition: keys [k0, k0 + nk), entries [e0, e0 + ne) (entry ids of the
// offline table are table positions, so a key range owns an id range), dense
// page cells [cb, cb + span) of every thread.
struct PartInfo {
  uint32_t k0, nk, e0, ne;
  uint64_t cb;
  uint32_t span;
  uint32_t dshift;     // directory slot j covers [first key + (j << dshift), + 2^dshift)
  uint32_t pages_lds;  // nb_threads * span <= kPartCells: page cells in LDS, else global atomics
  uint32_t cmap;       // ~0: cells [cb, cb + span); else (online table) span packed cells, the
                       // histogram cell of packed cell j at pe_cmap[cmap + j]
  uint32_t pad[2];
};
static_assert(sizeof(PartInfo) == 48, "PartInfo");

// The host's entry table: per entry id, the object as the latest table lists
// it and the page cells it counts into.  The arrays are contiguous (the report
// and the uploads read their data()).
struct EntryTable {
  std::vector<uint64_t> hist_base;  // first dense cell, kHistSparse if sparse / none
  std::vector<uint64_t> npages;     // buffer_size / kPageSize + 1 of the cells it has
  std::vector<uint64_t> buffer_size, entry_addr;
  std::vector<nmg_object> objects;    // the report's objects
  std::vector<DevEntry> dev_entries;  // host copy of d_entries (cells and id; nmg_set_objects' table also its objects)
  std::vector<uint32_t> sparse_entries;  // sparse idx -> entry
  CellCursor cur;  // cur.cells: dense cells per thread (padded between calls)

  uint64_t cells() const { return cur.cells; }
  // E entries; new ones are objects not described yet: one page, no cells
  void resize(uint32_t E) {
    const size_t E0 = dev_entries.size();
    hist_base.resize(E, kHistSparse);
    npages.resize(E, 1);
    buffer_size.resize(E, 0);
    entry_addr.resize(E, 0);
    objects.resize(E, nmg_object{0, 0, 0, 0});
    dev_entries.resize(E, DevEntry{0, 0, 0, 0, kHistSparse, ~0u, 0, 0, 0, 0});
    for (size_t e = E0; e < E; e++) dev_entries[e].id = (uint32_t)e;
  }
  // what resize and place added since the table had E entries and cursor c, dropped again
  void truncate(uint32_t E, const CellCursor& c) {
    resize(E);
    sparse_entries.resize(c.nsparse);
    cur = c;
  }
  // entry id as object o describes it (the report's view)
  void describe(uint32_t id, const nmg_object& o) {
    objects[id] = o;
    buffer_size[id] = o.buffer_size;
    entry_addr[id] = o.buffer_addr;
  }
  // the device record of entry id (its cells) as object o describes it
  DevEntry dev_entry(uint32_t id, const nmg_object& o) const {
    DevEntry d = dev_entries[id];
    d.addr = o.buffer_addr;
    d.end = o.buffer_addr + o.buffer_size;
    d.alloc = o.alloc_date;
    d.free = o.free_date;
    return d;
  }
  // page cells for np pages of entry id (CellCursor::place); the entry is unchanged unless placed
  Placement place(uint32_t id, uint64_t np, bool must_be_dense) {
    DevEntry& d = dev_entries[id];
    uint64_t base = kHistSparse;
    const Placement how = cur.place(np, must_be_dense, &base, &d.sidx);
    if (how == kPlaceDense) d.hist = hist_base[id] = base;
    if (how == kPlaceSparse) sparse_entries.push_back(id);
    return how;
  }
};

// ---- builders.  A table is K sorted unique keys, key k's entries at table
// positions [entry_off[k], entry_off[k + 1]), newest first, as chain[].

// The in-order walk of the complete tree of 2^levels - 1 Eytzinger (BFS)
// slots 1 .. 2^levels - 1: the slot of in-order rank r (0-based), so that
// handing sorted values out by rank leaves them in search order.  Rank r is
// the (r + 1)-th node in order; its trailing zeros count the levels below it.
inline uint32_t eytzinger_slot(uint32_t levels, uint32_t r) {
  const uint32_t p = r + 1, below = (uint32_t)__builtin_ctz(p);
  return (1u << (levels - 1 - below)) + (p >> (below + 1));
}

// The slot walk of every directory here: n ascending keys, `nslots` slots of
// width 2^sh from keys[0] on.  emit(j, lo, c) for each slot j in turn: lo =
// the index of the last key at or before the slot start, c = the keys after
// it inside the slot; the last slot is open and takes all the rest.  (128-bit:
// a slot's end may lie past 2^64.)
template <class Emit>
void slot_walk(const uint64_t* keys, uint32_t n, uint32_t nslots, uint32_t sh, Emit&& emit) {
  uint32_t lo = 0;
  for (uint32_t j = 0; j < nslots; j++) {
    const unsigned __int128 s0 = (unsigned __int128)j << sh, s1 = (unsigned __int128)(j + 1) << sh;
    while (lo + 1 < n && (unsigned __int128)(keys[lo + 1] - keys[0]) <= s0) lo++;
    uint32_t c = 0;
    if (j == nslots - 1) c = n - 1 - lo;
    else
      while (lo + 1 + c < n && (unsigned __int128)(keys[lo + 1 + c] - keys[0]) < s1) c++;
    emit(j, lo, c);
  }
}

// Node record of every key: its newest entry, with the node's place in the chain
inline std::vector<DevEntry> node_records(const uint32_t* entry_off, uint32_t K, const std::vector<DevEntry>& chain) {
  std::vector<DevEntry> nodes(K);
  for (uint32_t k = 0; k < K; k++) {
    nodes[k] = chain[entry_off[k]];
    nodes[k].first = entry_off[k];
    nodes[k].count = entry_off[k + 1] - entry_off[k];
  }
  return nodes;
}

// Lookup structure of a table of at most kLdsNodes keys: keys and node records
// in Eytzinger (BFS) order for the LDS search, [0] unused
struct SmallLookup {
  uint32_t elevels = 0;          // 2^elevels - 1 >= K
  std::vector<uint64_t> ekeys;   // [2^elevels], ~0 padding
  std::vector<DevEntry> enodes;  // [2^elevels]
};

inline SmallLookup build_small_lookup(const uint64_t* keys, uint32_t K, const std::vector<DevEntry>& nodes) {
  // Eytzinger (BFS) order for the LDS search: an in-order walk of the
  // complete tree of 2^L - 1 nodes hands out the keys in sorted order; the
  // slots after the last key are ~0 keys carrying a copy of the last node
  // (reached only for addr == UINT64_MAX, where the last key is the answer)
  SmallLookup s;
  while (((1u << s.elevels) - 1) < K) s.elevels++;
  const uint32_t n = 1u << s.elevels;
  s.ekeys.assign(n, ~0ull);
  s.enodes.resize(n);
  memset(s.enodes.data(), 0, n * sizeof(DevEntry));
  for (uint32_t r = 0; r + 1 < n; r++) {
    const uint32_t i = eytzinger_slot(s.elevels, r);
    if (r < K) s.ekeys[i] = keys[r];
    if (K) s.enodes[i] = nodes[std::min(r, K - 1)];
  }
  return s;
}

// Lookup structure of a table larger than kLdsNodes keys (see lower_key):
// fence b = keys[b << fence_log2] (<= kMaxFences fences, Eytzinger order),
// and per bucket a directory of 2^dir_log2 equal-width slots over the bucket's
// key span [first key, last key].
struct BigLookup {
  uint32_t nb_fences = 0, fence_log2 = 0, dir_log2 = 0;
  std::vector<uint64_t> efences;  // [kMaxFences + 1]
  std::vector<uint8_t> shift;     // [nb_fences]
  std::vector<Word8> dir;         // [nb_fences << dir_log2] {lo | cnt << 16, offset of the slot's first key}
};

inline void build_big_lookup(const uint64_t* keys, uint32_t K, bool no_dir, BigLookup& bl) {
  while (((uint64_t)K + (1u << bl.fence_log2) - 1) >> bl.fence_log2 > kMaxFences) bl.fence_log2++;
  const uint32_t S = 1u << bl.fence_log2;
  bl.nb_fences = (uint32_t)(((uint64_t)K + S - 1) >> bl.fence_log2);
  // Eytzinger order: an in-order walk of the complete 12-level tree hands out
  // the fences in sorted order; the slots after the last fence hold ~0
  bl.efences.assign(kMaxFences + 1, ~0ull);
  for (uint32_t r = 0; r < bl.nb_fences; r++) bl.efences[eytzinger_slot(kFenceLevels, r)] = keys[(uint64_t)r << bl.fence_log2];
  bl.shift.assign(bl.nb_fences, kShiftSearch);
  // bucket-relative indices and counts are 16-bit: S <= 2^16 (larger
  // buckets -- more than 4095 << 16 keys -- are binary-searched)
  if (S == 1 || S > (1u << 16) || no_dir) return;
  bl.dir_log2 = bl.fence_log2 + 1;  // two slots per key
  const uint32_t D = 1u << bl.dir_log2;
  bl.dir.assign((size_t)bl.nb_fences << bl.dir_log2, Word8{0, 0});
  for (uint32_t b = 0; b < bl.nb_fences; b++) {
    const uint32_t k0 = b * S, k1 = std::min<uint64_t>((uint64_t)k0 + S, K);
    const uint64_t f = keys[k0], span = keys[k1 - 1] - f;
    uint32_t sh = 0;
    while (sh < 64 && (span >> sh) >= D) sh++;
    if (sh > 32) continue;  // slot offsets must fit 32 bits: binary search instead
    bl.shift[b] = (uint8_t)sh;
    Word8* dd = &bl.dir[(size_t)b << bl.dir_log2];
    slot_walk(keys + k0, k1 - k0, D, sh, [&](uint32_t j, uint32_t lo, uint32_t c) {
      dd[j].x = lo | (std::min<uint32_t>(c, 0xffffu) << 16);
      dd[j].y = c ? (uint32_t)(keys[k0 + lo + 1] - f - ((uint64_t)j << sh)) : 0u;
    });
  }
}

// The route pass's partition search (route_partition, nmg_route.hip) over
// the P ascending partition starts b: up to kRouteSegs segments, split at the
// gaps between consecutive starts that dwarf the median gap (address spaces
// are clustered: globals, heap, mmap'd regions, the stack), each with
// directory slots in proportion to its partitions.  Slot j of a segment holds
// the last partition starting at or before the slot start, and how many
// starts lie inside the slot (saturated at kDirCntSat: search to the
// segment's last partition).
struct RouteDir {
  RSeg seg[kRouteSegs];
  uint32_t nseg = 0;
  std::vector<uint16_t> dir;  // [kRouteDir]
};

// segment k starts at partition cuts[k]
inline std::vector<uint32_t> route_cuts(const uint64_t* b, uint32_t P) {
  std::vector<uint32_t> cuts{0};
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
  return cuts;
}

inline RouteDir route_segments(const uint64_t* b, uint32_t P) {
  RouteDir rd;
  const std::vector<uint32_t> cuts = route_cuts(b, P);
  const uint32_t S = (uint32_t)cuts.size();
  rd.dir.assign(kRouteDir, 0);
  uint32_t used = 0;
  for (uint32_t k = 0; k < kRouteSegs; k++) {
    if (k >= S) {
      rd.seg[k] = RSeg{~0ull, 0, 1, 0, 0};
      continue;
    }
    const uint32_t qa = cuts[k], qb = k + 1 < S ? cuts[k + 1] : P;
    const uint32_t ns = (uint32_t)((uint64_t)(kRouteDir - S) * (qb - qa) / P) + 1;
    const uint64_t span = b[qb - 1] - b[qa];
    uint32_t sh = 0;
    while (sh < 63 && (span >> sh) >= ns) sh++;
    rd.seg[k] = RSeg{b[qa], used, ns, sh, qb - 1};
    slot_walk(b + qa, qb - qa, ns, sh, [&](uint32_t j, uint32_t lo, uint32_t c) {
      rd.dir[used + j] = (uint16_t)((qa + lo) | (std::min(c, kDirCntSat) << 11));
    });
    used += ns;
  }
  rd.nseg = S;
  return rd;
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
// too wide for LDS take global atomics).
struct TableInput {
  const uint64_t* keys;
  const uint32_t* entry_off;
  uint32_t K;
  const DevEntry* chain;   // [entry_off[K]] the entries in table order (ids in DevEntry::id)
  const uint64_t* npages;  // by entry id
  const uint32_t* ids;     // table position -> entry id, or null
  uint64_t T;              // threads
  uint64_t dense_cells;    // the table's dense cells per thread
};

// Everything the partition-first path reads of a table (RouteParams,
// LocalParams).  ok false: the table keeps the single-pass attribute_kernel.
struct PartTables {
  bool ok = false;
  bool online = false;  // ids given and not the identity: pe_lrel / pe_cmap are in use
  uint32_t nparts = 0;
  uint64_t tbase = 0;   // compact records: timestamps relative to this (XLayout)
  RouteDir route;       // the route pass's segments and directory over pbounds
  std::vector<PartInfo> parts;
  std::vector<uint64_t> pbounds;   // [kMaxParts + 1] partition start keys, ascending, ~0 padding
  std::vector<uint32_t> pdead;     // [(kMaxParts + 1) / 32] (RouteParams::pdead)
  std::vector<uint64_t> pe_keys;   // [nparts][kPartSlots] keys, ascending, ~0 padding
  std::vector<Word16> pe_nodes;    // [nparts][kPartSlots][2] (addr, end), (alloc, free) of each key's newest entry
  std::vector<Word16> pe_pnode;    // [nparts][kPartSlots] the same, packed (PackedNode)
  std::vector<Word8> pe_info;      // [nparts][kPartSlots] (cell - cb, or packed cell, or ~0 sparse; buffer_addr - first key)
  std::vector<Word16> pe_old;      // [nparts][kOldLds] older entries, packed (kOldLds)
  std::vector<uint32_t> pe_oinf;   // [nparts][kOldLds] their page cells
  std::vector<Word16> pe_dir;      // [nparts][kPartDir] directory slots (PartDir)
  // an online table: the partition's dense cells packed in LDS in table
  // order (lrel: an entry's first LDS cell per table position; cmap: the
  // histogram cell of every packed cell, per partition from PartInfo::cmap)
  std::vector<uint32_t> pe_lrel, pe_cmap;
};

// the dense cells of a run of entries: in [cb, ce), cc of them
struct CellRun {
  uint64_t cb = ~0ull, ce = 0, cc = 0;
};

// One partition from key k on: keys are taken while the four rules allow.
// False: key k alone has more than kPartEntries entries (one address reused
// that often: keep attribute_kernel).
inline bool cut_one(const TableInput& in, bool online, uint32_t& k, PartInfo& pi, CellRun& run) {
  while (k < in.K && k - pi.k0 < kPartKeys) {
    // a partition's keys span less than 2^(kAddrBits - 1) bytes, so that the
    // compact records' address field (relative to the partition's first key)
    // holds every address its objects cover: a run of keys across a wide gap
    // in the address space (the heap, then the stack) starts a new partition
    if (k > pi.k0 && in.keys[k] - in.keys[pi.k0] >= (1ull << (kAddrBits - 1))) break;
    const uint32_t ea = in.entry_off[k], eb = in.entry_off[k + 1];
    if (eb - pi.e0 > kPartEntries) {
      if (k == pi.k0) return false;
      break;
    }
    CellRun n = run;
    for (uint32_t e = ea; e < eb; e++)
      if (in.chain[e].hist != kHistSparse) {
        const uint64_t np = in.npages[in.chain[e].id];
        n.cb = std::min<uint64_t>(n.cb, in.chain[e].hist);
        n.ce = std::max<uint64_t>(n.ce, in.chain[e].hist + np);
        n.cc += np;
      }
    if (k > pi.k0 && n.cb != ~0ull && (online ? n.cc : n.ce - n.cb) * in.T > kPartCells)
      break;  // (one key alone may exceed: global cells)
    run = n;
    k++;
  }
  return true;
}

// The partitions of a table, in key order, with an online table's packed cell
// maps.  False: no partition-first path (an address reused more than
// kPartEntries times, or more than kMaxParts partitions: too many for the
// route pass's LDS tree).
inline bool cut_partitions(const TableInput& in, bool online, PartTables& out) {
  if (online) out.pe_lrel.assign(in.entry_off[in.K], kEmpty32);
  uint32_t k = 0;
  while (k < in.K) {
    PartInfo pi;
    memset(&pi, 0, sizeof(pi));
    pi.k0 = k;
    pi.e0 = in.entry_off[k];
    pi.cmap = ~0u;
    CellRun run;
    if (!cut_one(in, online, k, pi, run)) return false;
    pi.nk = k - pi.k0;
    pi.ne = in.entry_off[k] - pi.e0;
    pi.cb = run.cb == ~0ull ? 0 : run.cb;
    pi.span = run.cb == ~0ull ? 0 : (uint32_t)(run.ce - run.cb);
    pi.pages_lds = pi.span && (uint64_t)pi.span * in.T <= kPartCells;
    if (online && run.cc && run.cc * in.T <= kPartCells) {  // online: the cells packed (cmap), always in LDS
      pi.cmap = (uint32_t)out.pe_cmap.size();
      pi.span = (uint32_t)run.cc;
      pi.pages_lds = 1;
      uint32_t off = 0;
      for (uint32_t e = pi.e0; e < pi.e0 + pi.ne; e++)
        if (in.chain[e].hist != kHistSparse) {
          const uint32_t np = (uint32_t)in.npages[in.chain[e].id];
          out.pe_lrel[e] = off;
          for (uint32_t g = 0; g < np; g++) out.pe_cmap.push_back((uint32_t)(in.chain[e].hist + g));
          off += np;
        }
    }
    const uint64_t kspan = in.keys[k - 1] - in.keys[pi.k0];
    while (pi.dshift < 63 && (kspan >> pi.dshift) >= kPartDir) pi.dshift++;
    out.parts.push_back(pi);
    if (out.parts.size() > kMaxParts) return false;
  }
  return true;
}

// the compact records' timestamp base: the earliest allocation (a sample
// before it can only match objects allocated at time 0, and escapes)
inline uint64_t table_tbase(const DevEntry* chain, uint32_t n) {
  uint64_t tb = ~0ull;
  for (uint32_t e = 0; e < n; e++)
    if (chain[e].alloc) tb = std::min<uint64_t>(tb, chain[e].alloc);
  return tb == ~0ull ? 0 : tb;
}

// an entry's page cell relative to its partition (as pe_info.x)
inline uint32_t cell_rel(const TableInput& in, const PartTables& out, const PartInfo& pi, uint32_t e) {
  const DevEntry& d = in.chain[e];
  return d.hist == kHistSparse ? kEmpty32 : pi.cmap != ~0u ? out.pe_lrel[e] : (uint32_t)(d.hist - pi.cb);
}

// the quantised dates of an entry (never matching: ~0, 0)
inline void qdates(const DevEntry& d, uint64_t tb, uint32_t& aq, uint32_t& fq) {
  if (d.free < tb) {
    aq = 0xffffffffu;
    fq = 0;
  } else {
    aq = (uint32_t)std::min<uint64_t>((d.alloc > tb ? d.alloc - tb : 0) >> kPnQShift, 0xffffffffull);
    fq = (uint32_t)std::min<uint64_t>((d.free - tb) >> kPnQShift, 0xffffffffull);
  }
}

// Key kk's (the r-th of partition q) older entries into the partition's list
// (kOldLds) when they fit; false: the key's lookups walk the chain instead
inline bool pack_older(const TableInput& in, uint32_t q, uint32_t r, PartTables& out) {
  const PartInfo& pi = out.parts[q];
  const uint32_t kk = pi.k0 + r, e0 = in.entry_off[kk];
  const uint64_t f = in.keys[pi.k0], tb = out.tbase;
  const uint32_t nold = in.entry_off[kk + 1] - e0 - 1, lbase = e0 - pi.e0 - r;
  if (!(nold > 0 && nold < 2048 && lbase + nold <= kOldLds)) return false;
  for (uint32_t i = 1; i <= nold; i++) {
    const DevEntry& od = in.chain[e0 + i];
    uint32_t oa, of;
    qdates(od, tb, oa, of);
    Word16 v{0, oa, of, 0};
    if (od.free >= tb) {  // (else: never matches, bounds irrelevant)
      if (od.addr < f || od.end < od.addr || ((od.end - f) >> 32) != 0) return false;
      v.x = (uint32_t)(od.end - f);
      v.w = (uint32_t)(od.addr - f);
    }
    out.pe_old[(size_t)q * kOldLds + lbase + i - 1] = v;
    out.pe_oinf[(size_t)q * kOldLds + lbase + i - 1] = cell_rel(in, out, pi, e0 + i);
  }
  return true;
}

// Partition q's keys ascending with their newest entry's node record (the
// exact one, read by the local pass's rare paths), its packed form and info
// (the common path), and the older entries' list
inline void pack_partition(const TableInput& in, uint32_t q, PartTables& out) {
  const PartInfo& pi = out.parts[q];
  const uint64_t f = in.keys[pi.k0], tb = out.tbase;
  for (uint32_t r = 0; r < pi.nk; r++) {
    const uint32_t kk = pi.k0 + r, e0 = in.entry_off[kk];
    const DevEntry& d = in.chain[e0];
    const size_t o = (size_t)q * kPartSlots + r;
    out.pe_keys[o] = in.keys[kk];
    out.pe_nodes[2 * o] = Word16{(uint32_t)d.addr, (uint32_t)(d.addr >> 32), (uint32_t)d.end, (uint32_t)(d.end >> 32)};
    out.pe_nodes[2 * o + 1] =
        Word16{(uint32_t)d.alloc, (uint32_t)(d.alloc >> 32), (uint32_t)d.free, (uint32_t)(d.free >> 32)};
    const uint32_t nold = in.entry_off[kk + 1] - e0 - 1;
    // packed node (PackedNode): exact where the object's start or end
    // offset from the first key needs more than 32 bits -- unless it was
    // freed before the first allocation (the [stack], Q4): no non-escaped
    // sample can match it, whatever its bounds
    const uint64_t erel = d.end - f, brel = d.addr - f;
    const bool never = d.free < tb;
    const bool exact = !never && (d.addr < f || d.end < d.addr || (erel >> 32) != 0 || (brel >> 32) != 0);
    uint32_t aq, fq;
    qdates(d, tb, aq, fq);
    const bool old_lds = pack_older(in, q, r, out);
    out.pe_pnode[o] = Word16{exact || never ? 0u : (uint32_t)erel, aq, fq,
                             (e0 - pi.e0) | (nold ? kPnOlder : 0u) | (exact ? kPnExact : 0u) |
                                 (old_lds ? kPnOldLds | (nold << kPnOldShift) : 0u)};
    out.pe_info[o] = Word8{cell_rel(in, out, pi, e0), exact || never ? 0u : (uint32_t)brel};
  }
}

// Partition q's directory over its key span: slot j starts at first key +
// (j << dshift) and holds the index of the largest key <= that start, the
// number of keys inside the slot (the last slot: every key after its start)
// and the first kDirInline of those keys' offsets from the slot start when
// they fit 16 bits (PartDir)
inline void build_part_dir(const uint64_t* keys, const PartInfo& pi, Word16* pdir) {
  const uint64_t f = keys[pi.k0];
  slot_walk(keys + pi.k0, pi.nk, kPartDir, pi.dshift, [&](uint32_t j, uint32_t lo, uint32_t c) {
    const uint64_t s0 = (uint64_t)j << pi.dshift;  // slot start relative to the first key
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
    pdir[j] = Word16{lo | (c << 10) | ((inl && c ? 1u : 0u) << 21), off[0] | (off[1] << 16), off[2] | (off[3] << 16),
                     off[4] | (off[5] << 16)};
  });
}

// partitions whose entries all have free_date 0 (RouteParams::pdead): the
// route pass keeps only their timestamp-0 samples, the others cannot match
inline std::vector<uint32_t> dead_partitions(const DevEntry* chain, const std::vector<PartInfo>& parts) {
  std::vector<uint32_t> dead((kMaxParts + 1) / 32, 0u);
  for (uint32_t q = 0; q < parts.size(); q++) {
    bool d = true;
    for (uint32_t e = parts[q].e0; d && e < parts[q].e0 + parts[q].ne; e++) d = chain[e].free == 0;
    if (d) dead[q >> 5] |= 1u << (q & 31);
  }
  return dead;
}

// The partition-first path's tables of one object table.  Only tables of more
// than kLdsNodes keys take the path; an online table's cell indices are 32-bit.
inline PartTables build_part_tables(const TableInput& in) {
  PartTables out;
  if (in.K <= kLdsNodes) return out;
  const uint32_t n = in.entry_off[in.K];
  if (in.ids) {  // the identity map is the offline case
    uint32_t e = 0;
    while (e < n && in.ids[e] == e) e++;
    out.online = e < n;
  }
  if (out.online && in.dense_cells >= (1ull << 31)) return out;
  if (!cut_partitions(in, out.online, out)) return out;
  const uint32_t P = out.nparts = (uint32_t)out.parts.size();
  out.tbase = table_tbase(in.chain, n);
  out.pe_keys.assign((size_t)P * kPartSlots, ~0ull);
  out.pe_nodes.assign((size_t)P * kPartSlots * 2, Word16{0, 0, 0, 0});
  out.pe_pnode.assign((size_t)P * kPartSlots, Word16{0, 0, 0, 0});
  out.pe_info.assign((size_t)P * kPartSlots, Word8{kEmpty32, 0});
  out.pe_dir.assign((size_t)P * kPartDir, Word16{0, 0, 0, 0});
  out.pe_old.assign((size_t)P * kOldLds, Word16{0, 0, 0, 0});
  out.pe_oinf.assign((size_t)P * kOldLds, kEmpty32);
  for (uint32_t q = 0; q < P; q++) {
    pack_partition(in, q, out);
    build_part_dir(in.keys, out.parts[q], &out.pe_dir[(size_t)q * kPartDir]);
  }
  // the route pass's partition search: the partitions' first keys ascending,
  // and a directory over them (route_segments)
  out.pbounds.assign(kMaxParts + 1, ~0ull);
  for (uint32_t q = 0; q < P; q++) out.pbounds[q] = in.keys[out.parts[q].k0];
  out.route = route_segments(out.pbounds.data(), P);
  out.pdead = dead_partitions(in.chain, out.parts);
  out.ok = true;
  return out;
}

}  // namespace nmg
