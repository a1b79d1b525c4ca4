// The table builders (numamma_amd/csrc/nmg_table_build.h) on the CPU, no HIP
// involved: the small table's Eytzinger tree, the fences and bucket directory
// of a large one, the route pass's segments, and the partition-first path's
// partitions, node records, directories and dead bits.  Every array is checked
// against a direct restatement of the format comments in that header, and
// every built lookup against a host restatement of the device's read sequence
// (lower_key, route_partition_l, the local pass's slot read), which must
// return upper_bound - 1.  Built by tests/test_table_build_host.py with the
// address and undefined-behaviour sanitizers.
//   nmg_table_build_host [--digests] [tables-file]
// --digests: a 64-bit digest of every output vector of every table built here;
// tables-file: tables written by the Python test, whose partitions and PartDir
// slots are printed for it.
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "nmg_table_build.h"

using namespace nmg;
typedef unsigned __int128 u128;

static int g_failed = 0;
static bool g_digests = false;
#define CHECK(cond)                                                                        \
  do {                                                                                     \
    if (!(cond)) {                                                                         \
      if (g_failed < 40) fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      g_failed++;                                                                          \
    }                                                                                      \
  } while (0)

static void fail(const char* what) {
  if (g_failed++ < 40) fprintf(stderr, "%s\n", what);
}

template <class T>
static void digest(const std::string& name, const T* p, size_t n) {
  if (!g_digests) return;
  uint64_t h = 0xcbf29ce484222325ull;  // FNV-1a over the bytes
  const uint8_t* b = reinterpret_cast<const uint8_t*>(p);
  for (size_t i = 0; i < n * sizeof(T); i++) h = (h ^ b[i]) * 0x100000001b3ull;
  printf("digest %-28s %9zu %016" PRIx64 "\n", name.c_str(), n, h);
}
template <class T>
static void digest(const std::string& name, const std::vector<T>& v) {
  digest(name, v.data(), v.size());
}

// ---- what every lookup must return, and where it is probed

// number of keys <= a (the answer is one less; 0: no key)
static uint32_t keys_le(const uint64_t* k, uint32_t n, uint64_t a) { return (uint32_t)(std::upper_bound(k, k + n, a) - k); }

static std::vector<uint64_t> probes(const uint64_t* k, uint32_t n) {
  std::vector<uint64_t> p{0, ~0ull};
  for (uint32_t i = 0; i < n; i++) {
    p.push_back(k[i]);
    if (k[i]) p.push_back(k[i] - 1);
    if (k[i] != ~0ull) p.push_back(k[i] + 1);
    if (i + 1 < n) p.push_back(k[i] + (k[i + 1] - k[i]) / 2);
  }
  return p;
}

// Slot j of `nslots` slots of width 2^sh over the ascending keys k[0..n),
// relative to k[0]: lo = the last key at or before the slot start, c = the
// keys after it inside the slot; the last slot takes all the rest.
static void slot_ref(const uint64_t* k, uint32_t n, uint32_t nslots, uint32_t sh, uint32_t j, uint32_t& lo, uint32_t& c) {
  const u128 s0 = (u128)j << sh, s1 = (u128)(j + 1) << sh;
  const uint32_t le = (uint32_t)(std::partition_point(k, k + n, [&](uint64_t v) { return (u128)(v - k[0]) <= s0; }) - k);
  const uint32_t lt = (uint32_t)(std::partition_point(k, k + n, [&](uint64_t v) { return (u128)(v - k[0]) < s1; }) - k);
  lo = le - 1;  // (k[0] is at or before every slot start)
  c = (j == nslots - 1 ? n : lt) - le;
}

// the complete tree of 2^levels - 1 slots in order (left, node, right)
static void in_order(uint32_t i, uint32_t n, std::vector<uint32_t>& out) {
  if (i >= n) return;
  in_order(2 * i, n, out);
  out.push_back(i);
  in_order(2 * i + 1, n, out);
}

// eytz_descend and the node of the last right turn (0: none)
static uint32_t eytz_node(const std::vector<uint64_t>& F, uint32_t levels, uint64_t addr) {
  uint32_t i = 1;
  for (uint32_t l = 0; l < levels; l++) {
    if (i >= F.size()) {
      fail("descent past the tree");
      return 0;
    }
    i = 2 * i + (F[i] <= addr ? 1u : 0u);
  }
  return i >> (__builtin_ctz(i) + 1);
}

// ---- the small table's tree

static std::vector<uint64_t> spread_keys(uint32_t K, uint64_t base, uint64_t step) {
  std::vector<uint64_t> k(K);
  for (uint32_t i = 0; i < K; i++) k[i] = base + i * step + (i * 2654435761u) % (step / 2);
  return k;
}

static std::vector<DevEntry> plain_nodes(const std::vector<uint64_t>& keys) {
  std::vector<DevEntry> n(keys.size());
  for (uint32_t i = 0; i < n.size(); i++) n[i] = DevEntry{keys[i], keys[i] + 64, 1000 + i, 2000 + i, i, ~0u, i, 1, i, 0};
  return n;
}

static void check_small(uint32_t K) {
  const std::vector<uint64_t> keys = spread_keys(K, 0x10000, 4096);
  const std::vector<DevEntry> nodes = plain_nodes(keys);
  const SmallLookup s = build_small_lookup(keys.data(), K, nodes);
  const std::string name = "small" + std::to_string(K);
  digest(name + ".ekeys", s.ekeys);
  digest(name + ".enodes", s.enodes);
  uint32_t L = 0;
  while ((1u << L) - 1 < K) L++;
  CHECK(s.elevels == L);
  const uint32_t n = 1u << L;
  CHECK(s.ekeys.size() == n && s.enodes.size() == n);
  if (s.ekeys.size() != n || s.enodes.size() != n) return;
  const DevEntry zero{};
  CHECK(s.ekeys[0] == ~0ull && !memcmp(&s.enodes[0], &zero, sizeof(zero)));  // [0] unused
  std::vector<uint32_t> ord;
  in_order(1, n, ord);
  CHECK(ord.size() == n - 1);
  for (uint32_t r = 0; r < ord.size(); r++) {
    const uint32_t i = ord[r];
    if (r < K) CHECK(s.ekeys[i] == keys[r] && !memcmp(&s.enodes[i], &nodes[r], sizeof(DevEntry)));
    else CHECK(s.ekeys[i] == ~0ull && !memcmp(&s.enodes[i], K ? &nodes[K - 1] : &zero, sizeof(DevEntry)));
  }
  for (uint64_t a : probes(keys.data(), K)) {
    const uint32_t idx = eytz_node(s.ekeys, s.elevels, a), want = keys_le(keys.data(), K, a);
    if (!want) CHECK(idx == 0);
    else CHECK(idx != 0 && idx < n && !memcmp(&s.enodes[idx], &nodes[want - 1], sizeof(DevEntry)));
  }
}

// ---- fences and bucket directory

// lower_key (nmg_kernels.hip): the largest key <= addr, K when there is none
static uint32_t lower_key_ref(const BigLookup& bl, const uint64_t* keys, uint32_t K, uint64_t addr) {
  const uint32_t idx = eytz_node(bl.efences, kFenceLevels, addr);
  if (idx == 0) return K;
  const uint32_t d = 31 - __builtin_clz(idx);
  const uint32_t b = (((idx - (1u << d)) * 2 + 1) << (kFenceLevels - 1 - d)) - 1;
  if (b >= bl.nb_fences) return K - 1;
  const uint32_t k0 = b << bl.fence_log2;
  if (bl.fence_log2 == 0) return k0;
  const uint32_t kend = std::min(k0 + (1u << bl.fence_log2), K);
  const uint32_t sh = bl.shift[b];
  uint32_t lo, n;
  if (sh != kShiftSearch) {
    const uint64_t f = bl.efences[idx], rel = addr - f;
    const uint32_t slots = 1u << bl.dir_log2;
    const uint32_t j = (uint32_t)std::min<uint64_t>(rel >> sh, slots - 1);
    const size_t at = ((size_t)b << bl.dir_log2) + j;
    if (at >= bl.dir.size()) {
      fail("directory slot out of range");
      return K;
    }
    const Word8 de = bl.dir[at];
    lo = k0 + (de.x & 0xffffu);
    const uint32_t cnt = de.x >> 16;
    if (cnt == 0 || rel - ((uint64_t)j << sh) < de.y) return lo;
    lo += 1;
    n = cnt;
  } else {
    lo = k0;
    n = kend - k0;
  }
  while (n > 1) {
    const uint32_t half = n >> 1;
    if (lo + half >= K) {
      fail("key search out of range");
      return K;
    }
    const bool le = keys[lo + half] <= addr;
    lo = le ? lo + half : lo;
    n = le ? n - half : half;
  }
  return lo;
}

// wide_bucket: the bucket whose last key lies 2^40 past its first (none: ~0u)
static void check_big(const std::string& name, std::vector<uint64_t> keys, bool no_dir, uint32_t want_fence_log2,
                      uint32_t wide_bucket = ~0u) {
  const uint32_t K = (uint32_t)keys.size();
  BigLookup bl;
  build_big_lookup(keys.data(), K, no_dir, bl);
  digest(name + ".efences", bl.efences);
  digest(name + ".shift", bl.shift);
  digest(name + ".dir", bl.dir);
  // fence b = keys[b << fence_log2], at most kMaxFences of them
  uint32_t f = 0;
  while ((((uint64_t)K + (1u << f) - 1) >> f) > kMaxFences) f++;
  CHECK(f == want_fence_log2);
  const uint32_t S = 1u << f, nb = (K + S - 1) / S;
  CHECK(bl.fence_log2 == f && bl.nb_fences == nb);
  CHECK(bl.efences.size() == kMaxFences + 1 && bl.shift.size() == nb);
  if (bl.efences.size() != kMaxFences + 1 || bl.shift.size() != nb) return;
  std::vector<uint32_t> ord;
  in_order(1, kMaxFences + 1, ord);
  CHECK(bl.efences[0] == ~0ull);
  for (uint32_t r = 0; r < ord.size(); r++) CHECK(bl.efences[ord[r]] == (r < nb ? keys[(size_t)r << f] : ~0ull));
  // the directory: two slots per key, none for one key per fence or no_dir
  const bool dir = S > 1 && !no_dir;
  CHECK(bl.dir_log2 == (dir ? f + 1 : 0u));
  CHECK(bl.dir.size() == (dir ? (size_t)nb << (f + 1) : 0u));
  if (bl.dir.size() != (dir ? (size_t)nb << (f + 1) : 0u)) return;
  for (uint32_t b = 0; b < nb; b++) {
    if (!dir) {
      CHECK(bl.shift[b] == kShiftSearch);
      continue;
    }
    const uint32_t k0 = b * S, n = std::min(S, K - k0), D = 2 * S;
    const uint64_t span = keys[k0 + n - 1] - keys[k0];
    uint32_t sh = 0;
    while (sh < 64 && (span >> sh) >= D) sh++;  // the narrowest slots that cover the span
    if (b == wide_bucket) CHECK(sh > 32);
    if (sh > 32) {  // slot offsets would not fit 32 bits
      CHECK(bl.shift[b] == kShiftSearch);
      continue;
    }
    CHECK(bl.shift[b] == sh);
    for (uint32_t j = 0; j < D; j++) {
      uint32_t lo, c;
      slot_ref(&keys[k0], n, D, sh, j, lo, c);
      const Word8 de = bl.dir[((size_t)b << bl.dir_log2) + j];
      CHECK(de.x == (lo | (std::min(c, 0xffffu) << 16)));
      CHECK(de.y == (c ? (uint32_t)(keys[k0 + lo + 1] - keys[k0] - ((uint64_t)j << sh)) : 0u));
    }
  }
  if (wide_bucket != ~0u) CHECK(bl.shift[wide_bucket] == kShiftSearch && bl.shift[wide_bucket ^ 1] != kShiftSearch);
  for (uint64_t a : probes(keys.data(), K)) {
    const uint32_t want = keys_le(keys.data(), K, a);
    CHECK(lower_key_ref(bl, keys.data(), K, a) == (want ? want - 1 : K));
  }
}

// ---- route segments

// route_partition_l (nmg_route.hip): the last start <= addr, for addr >= the first start
static uint32_t route_ref(const RouteDir& rd, const std::vector<uint64_t>& pb, uint64_t addr) {
  uint32_t k = 0;
  for (uint32_t j = 1; j < kRouteSegs; j++) k += addr >= rd.seg[j].start;
  k = std::min(k, rd.nseg - 1);
  const RSeg& s = rd.seg[k];
  const uint64_t rel = (addr - s.start) >> s.shift;
  const size_t at = s.base + (rel < s.nslots ? (uint32_t)rel : s.nslots - 1);
  if (at >= rd.dir.size()) {
    fail("route slot out of range");
    return ~0u;
  }
  const uint32_t e = rd.dir[at];
  uint32_t q = e & 2047u;
  const uint32_t c = e >> 11;
  uint32_t n = (c == kDirCntSat ? s.qlast - q : c) + 1;
  while (n > 1) {
    const uint32_t half = n >> 1;
    if (q + half >= pb.size()) {
      fail("start search out of range");
      return ~0u;
    }
    if (pb[q + half] <= addr) {
      q += half;
      n -= half;
    } else {
      n = half;
    }
  }
  return q;
}

// segs: the first partition of every expected segment; returns the slots that saturate
static uint32_t check_route(const std::string& name, const RouteDir& rd, std::vector<uint64_t> b, uint32_t P,
                            const std::vector<uint32_t>* segs = nullptr) {
  digest(name + ".rseg", rd.seg, kRouteSegs);
  digest(name + ".rdir", rd.dir);
  CHECK(rd.dir.size() == kRouteDir && rd.nseg >= 1 && rd.nseg <= kRouteSegs && b.size() == kMaxParts + 1);
  if (rd.dir.size() != kRouteDir || !rd.nseg || rd.nseg > kRouteSegs) return 0;
  if (segs) CHECK(rd.nseg == segs->size());
  uint32_t used = 0, sat = 0;
  for (uint32_t k = 0; k < kRouteSegs; k++) {
    const RSeg& s = rd.seg[k];
    if (k >= rd.nseg) {
      CHECK(s.start == ~0ull && s.nslots == 1);
      continue;
    }
    // its partitions [qa, qb): from its start to the next segment's
    const uint32_t qa = (uint32_t)(std::lower_bound(b.begin(), b.begin() + P, s.start) - b.begin());
    const uint32_t qb = k + 1 < rd.nseg ? (uint32_t)(std::lower_bound(b.begin(), b.begin() + P, rd.seg[k + 1].start) - b.begin()) : P;
    CHECK(qa < qb && b[qa] == s.start && (k || qa == 0) && s.qlast == qb - 1);
    if (segs && k < segs->size()) CHECK(qa == (*segs)[k]);
    CHECK(s.base == used && s.nslots >= 1 && used + s.nslots <= kRouteDir);
    if (!(qa < qb) || used + s.nslots > kRouteDir) return sat;
    CHECK(s.nslots == (uint32_t)((uint64_t)(kRouteDir - rd.nseg) * (qb - qa) / P) + 1);  // slots in proportion
    const uint64_t span = b[qb - 1] - b[qa];
    uint32_t sh = 0;
    while (sh < 63 && (span >> sh) >= s.nslots) sh++;
    CHECK(s.shift == sh);
    for (uint32_t j = 0; j < s.nslots; j++) {
      uint32_t lo, c;
      slot_ref(&b[qa], qb - qa, s.nslots, s.shift, j, lo, c);
      CHECK(rd.dir[used + j] == ((qa + lo) | (std::min(c, kDirCntSat) << 11)));
      sat += c >= kDirCntSat;
    }
    used += s.nslots;
  }
  for (uint64_t a : probes(b.data(), P))
    if (a >= b[0]) CHECK(route_ref(rd, b, a) == keys_le(b.data(), P, a) - 1);
  return sat;
}

static uint32_t check_route_starts(const std::string& name, std::vector<uint64_t> b, const std::vector<uint32_t>* segs = nullptr) {
  const uint32_t P = (uint32_t)b.size();
  b.resize(kMaxParts + 1, ~0ull);
  return check_route(name, route_segments(b.data(), P), b, P, segs);
}

static void route_cases() {
  const std::vector<uint32_t> one{0};
  check_route_starts("route.p1", {0x7000}, &one);
  check_route_starts("route.p2", {0x7000, 0x7000 + (1ull << 45)}, &one);  // (the one gap is the median gap: no cut)
  {  // twelve clusters of ten starts, the gaps between them all huge and growing: the largest seven cut
    std::vector<uint64_t> b;
    uint64_t at = 1ull << 30;
    for (uint32_t c = 0; c < 12; c++) {
      for (uint32_t i = 0; i < 10; i++) b.push_back(at + ((uint64_t)i << 20));
      at += (1ull << 40) + ((uint64_t)c << 36);
    }
    const std::vector<uint32_t> segs{0, 50, 60, 70, 80, 90, 100, 110};
    check_route_starts("route.clusters", b, &segs);
  }
  {  // 140 starts 1 MiB apart, then 60 a byte apart: those share a slot, which saturates
    std::vector<uint64_t> b;
    for (uint32_t i = 0; i < 140; i++) b.push_back(0x100000 + ((uint64_t)i << 20));
    for (uint32_t i = 1; i <= 60; i++) b.push_back(b[139] + i);
    CHECK(check_route_starts("route.saturated", b, &one) >= 1);
  }
  check_route_starts("route.top", {1ull << 63, ~0ull - (1ull << 20), ~0ull - 1});
  check_route_starts("route.whole", {0, ~0ull - 1});  // (slot ends past 2^64)
}

// ---- tables, built as nmg_set_objects / nmg_update_objects build them

struct Tab {
  std::vector<uint64_t> keys;
  std::vector<uint32_t> off{0};
  std::vector<nmg_object> objs;  // table order, a key's newest entry first
  void add(uint64_t key, const std::vector<nmg_object>& entries) {
    keys.push_back(key);
    objs.insert(objs.end(), entries.begin(), entries.end());
    off.push_back((uint32_t)objs.size());
  }
  // n entries of `size` bytes at the key, alive in [1000, 2000] (+ their position)
  void plain(uint64_t key, uint32_t n = 1, uint64_t size = 64) {
    std::vector<nmg_object> e;
    for (uint32_t i = 0; i < n; i++) e.push_back(nmg_object{key, size, 1000 + objs.size() + i, 2000 + objs.size() + i});
    add(key, e);
  }
};

struct Built {
  EntryTable tab;
  std::vector<DevEntry> chain;
  TableInput in;
  PartTables pt;
};

// ids: table position -> entry id (null: the position); page cells are handed out in id order
static void build(const Tab& t, const uint32_t* ids, uint64_t T, Built& b, uint64_t dense_cells = ~0ull) {
  const uint32_t E = (uint32_t)t.objs.size();
  b.tab.cur.threads = T;
  b.tab.cur.budget_cells = (4ull << 30) / 4;
  b.tab.resize(E);
  std::vector<uint32_t> pos(E);
  for (uint32_t j = 0; j < E; j++) pos[ids ? ids[j] : j] = j;
  for (uint32_t id = 0; id < E; id++) {
    const nmg_object& o = t.objs[pos[id]];
    b.tab.describe(id, o);
    b.tab.npages[id] = o.buffer_size / kPageSize + 1;
    CHECK(b.tab.place(id, b.tab.npages[id], false) != kPlaceSparseFull);
    b.tab.dev_entries[id] = b.tab.dev_entry(id, o);
  }
  b.tab.cur.cells = b.tab.cur.padded_cells();
  b.chain.resize(E);
  for (uint32_t j = 0; j < E; j++) b.chain[j] = b.tab.dev_entries[ids ? ids[j] : j];
  b.in = TableInput{t.keys.data(), t.off.data(), (uint32_t)t.keys.size(), b.chain.data(), b.tab.npages.data(), ids, T,
                    dense_cells == ~0ull ? b.tab.cells() : dense_cells};
  b.pt = build_part_tables(b.in);
}

static void digest_parts(const std::string& name, const PartTables& pt) {
  if (!g_digests) return;
  printf("digest %-28s ok %d online %d nparts %u tbase %" PRIu64 "\n", name.c_str(), pt.ok, pt.online, pt.nparts, pt.tbase);
  if (!pt.ok) return;
  digest(name + ".parts", pt.parts);
  digest(name + ".pbounds", pt.pbounds);
  digest(name + ".pdead", pt.pdead);
  digest(name + ".pe_keys", pt.pe_keys);
  digest(name + ".pe_nodes", pt.pe_nodes);
  digest(name + ".pe_pnode", pt.pe_pnode);
  digest(name + ".pe_info", pt.pe_info);
  digest(name + ".pe_old", pt.pe_old);
  digest(name + ".pe_oinf", pt.pe_oinf);
  digest(name + ".pe_dir", pt.pe_dir);
  digest(name + ".pe_lrel", pt.pe_lrel);
  digest(name + ".pe_cmap", pt.pe_cmap);
}

// the local pass's slot read (local_kernel, nmg_route.hip): the index in the
// partition of the largest key <= first key + rel
static uint32_t local_ref(const PartTables& pt, uint32_t q, uint64_t rel) {
  const PartInfo& pi = pt.parts[q];
  const uint64_t* keys = &pt.pe_keys[(size_t)q * kPartSlots];
  const uint32_t slot = (uint32_t)std::min<uint64_t>(rel >> pi.dshift, kPartDir - 1);
  const Word16 de = pt.pe_dir[(size_t)q * kPartDir + slot];
  const uint32_t lo = de.x & 1023u, n = (de.x >> 10) & 2047u;
  const bool inl = n && ((de.x >> 21) & 1u);
  const uint64_t rs64 = rel - ((uint64_t)slot << pi.dshift);
  const uint32_t rs = rs64 >> 16 ? 0x10000u : (uint32_t)rs64;
  const uint32_t c = ((de.y & 0xffffu) <= rs) + ((de.y >> 16) <= rs) + ((de.z & 0xffffu) <= rs) + ((de.z >> 16) <= rs) +
                     ((de.w & 0xffffu) <= rs) + ((de.w >> 16) <= rs);
  uint32_t a = inl ? lo + std::min(c, n) : lo;
  uint32_t m = !inl ? n : (c == kDirInline && n > kDirInline) ? n - kDirInline : 0u;
  while (m) {  // the answer in [a, a + m]
    const uint32_t half = (m + 1) >> 1;
    if (a + half >= pi.nk) {
      fail("partition key search out of range");
      return ~0u;
    }
    const bool le = keys[a + half] - keys[0] <= rel;
    a += le ? half : 0u;
    m = le ? m - half : half - 1;
  }
  return a;
}

// PartDir of partition q, slot by slot, and its lookup over the partition's address range
static void check_part_dir(const Built& b, uint32_t q) {
  const PartTables& pt = b.pt;
  const PartInfo& pi = pt.parts[q];
  const uint64_t* keys = b.in.keys + pi.k0;
  const uint64_t span = keys[pi.nk - 1] - keys[0];
  uint32_t sh = 0;
  while (sh < 63 && (span >> sh) >= kPartDir) sh++;
  CHECK(pi.dshift == sh);
  for (uint32_t j = 0; j < kPartDir; j++) {
    uint32_t lo, c;
    slot_ref(keys, pi.nk, kPartDir, pi.dshift, j, lo, c);
    const Word16 de = pt.pe_dir[(size_t)q * kPartDir + j];
    uint32_t off[kDirInline];
    bool inl = c > 0;
    for (uint32_t i = 0; i < kDirInline; i++) {
      const uint64_t v = i < c ? keys[lo + 1 + i] - keys[0] - ((uint64_t)j << pi.dshift) : 0xffffu;
      if (i < c && (v >> 16)) inl = false;
      off[i] = (uint32_t)v;
    }
    CHECK(de.x == (lo | (c << 10) | ((inl ? 1u : 0u) << 21)));
    if (inl)  // (the offsets are valid when `inline`)
      CHECK(de.y == (off[0] | (off[1] << 16)) && de.z == (off[2] | (off[3] << 16)) && de.w == (off[4] | (off[5] << 16)));
  }
  const uint64_t next = q + 1 < pt.nparts ? b.in.keys[pt.parts[q + 1].k0] : ~0ull;
  for (uint64_t a : probes(keys, pi.nk))
    if (a >= keys[0] && (a < next || q + 1 == pt.nparts)) CHECK(local_ref(pt, q, a - keys[0]) == keys_le(keys, pi.nk, a) - 1);
}

static void quantised(const DevEntry& d, uint64_t tb, uint32_t& aq, uint32_t& fq) {
  if (d.free < tb) {  // freed before tbase: no sample matches
    aq = ~0u;
    fq = 0;
    return;
  }
  const uint64_t a = (d.alloc > tb ? d.alloc - tb : 0) >> kPnQShift, f = (d.free - tb) >> kPnQShift;
  aq = a >> 32 ? ~0u : (uint32_t)a;
  fq = f >> 32 ? ~0u : (uint32_t)f;
}

// an entry's page cell as pe_info.x / pe_oinf hold it
static uint32_t cell_ref(const Built& b, const PartInfo& pi, uint32_t e) {
  const DevEntry& d = b.chain[e];
  if (d.hist == kHistSparse) return kEmpty32;
  return pi.cmap != ~0u ? b.pt.pe_lrel[e] : (uint32_t)(d.hist - pi.cb);
}

// an older entry fits the list: its bounds lie at or after the first key and its end offset fits 32 bits
static bool old_fits(const DevEntry& d, uint64_t f, uint64_t tb) {
  return d.free < tb || !(d.addr < f || d.end < d.addr || ((d.end - f) >> 32));
}

// every record of partition q decoded per the format comments against the chain
static void check_part_records(const Built& b, uint32_t q) {
  const PartTables& pt = b.pt;
  const PartInfo& pi = pt.parts[q];
  const uint64_t f = b.in.keys[pi.k0], tb = pt.tbase;
  for (uint32_t r = 0; r < kPartSlots; r++) {
    const size_t o = (size_t)q * kPartSlots + r;
    const Word16 pn = pt.pe_pnode[o], n0 = pt.pe_nodes[2 * o], n1 = pt.pe_nodes[2 * o + 1];
    const Word8 inf = pt.pe_info[o];
    if (r >= pi.nk) {  // padding
      CHECK(pt.pe_keys[o] == ~0ull && !(pn.x | pn.y | pn.z | pn.w) && !(n0.x | n0.y | n0.z | n0.w) && inf.x == kEmpty32 && !inf.y);
      continue;
    }
    const uint32_t kk = pi.k0 + r, e0 = b.in.entry_off[kk], nold = b.in.entry_off[kk + 1] - e0 - 1;
    const DevEntry& d = b.chain[e0];
    CHECK(pt.pe_keys[o] == b.in.keys[kk]);
    CHECK((((uint64_t)n0.y << 32) | n0.x) == d.addr && (((uint64_t)n0.w << 32) | n0.z) == d.end);
    CHECK((((uint64_t)n1.y << 32) | n1.x) == d.alloc && (((uint64_t)n1.w << 32) | n1.z) == d.free);
    uint32_t aq, fq;
    quantised(d, tb, aq, fq);
    CHECK(pn.y == aq && pn.z == fq);
    CHECK((pn.w & 2047u) == e0 - pi.e0 && !!(pn.w & kPnOlder) == (nold > 0));
    CHECK(inf.x == cell_ref(b, pi, e0));
    const bool never = d.free < tb;
    const bool wide = d.addr < f || d.end < d.addr || ((d.end - f) >> 32) || ((d.addr - f) >> 32);
    CHECK(!!(pn.w & kPnExact) == (!never && wide));
    if (never || wide) CHECK(pn.x == 0 && inf.y == 0);
    else CHECK(f + pn.x == d.end && f + inf.y == d.addr);
    // the older entries: in the list when all of them fit it
    const uint32_t lbase = e0 - pi.e0 - r;
    bool fits = nold > 0 && nold < 2048 && lbase + nold <= kOldLds;
    for (uint32_t i = 1; fits && i <= nold; i++) fits = old_fits(b.chain[e0 + i], f, tb);
    CHECK(!!(pn.w & kPnOldLds) == fits);
    CHECK((pn.w >> kPnOldShift) == (fits ? nold : 0u) && !(pn.w & ~(2047u | kPnOlder | kPnExact | kPnOldLds | (0xffffu << kPnOldShift))));
    for (uint32_t i = 1; fits && i <= nold; i++) {
      const DevEntry& od = b.chain[e0 + i];
      const size_t at = (size_t)q * kOldLds + (e0 - pi.e0) - r + i - 1;  // table position - e0 - key index + i - 1
      const Word16 v = pt.pe_old[at];
      quantised(od, tb, aq, fq);
      CHECK(v.y == aq && v.z == fq && pt.pe_oinf[at] == cell_ref(b, pi, e0 + i));
      if (od.free < tb) CHECK(v.x == 0 && v.w == 0);
      else CHECK(f + v.x == od.end && f + v.w == od.addr);
    }
  }
}

// the partitions: consistent with the table, within the four rules, greedy
// (the next key would break one), and everything derived from them
static void check_parts(const std::string& name, const Built& b) {
  const PartTables& pt = b.pt;
  digest_parts(name, pt);
  if (!pt.ok) return;
  const TableInput& in = b.in;
  const uint32_t P = pt.nparts, n = in.entry_off[in.K];
  CHECK(P == pt.parts.size() && P >= 1 && P <= kMaxParts);
  CHECK(pt.pe_keys.size() == (size_t)P * kPartSlots && pt.pe_nodes.size() == (size_t)P * kPartSlots * 2 &&
        pt.pe_pnode.size() == (size_t)P * kPartSlots && pt.pe_info.size() == (size_t)P * kPartSlots &&
        pt.pe_dir.size() == (size_t)P * kPartDir && pt.pe_old.size() == (size_t)P * kOldLds &&
        pt.pe_oinf.size() == (size_t)P * kOldLds && pt.pbounds.size() == kMaxParts + 1 &&
        pt.pdead.size() == (kMaxParts + 1) / 32);
  CHECK(pt.pe_lrel.size() == (pt.online ? n : 0u) && (pt.online || pt.pe_cmap.empty()));
  if (g_failed) return;
  uint64_t tb = ~0ull;  // the smallest non-zero alloc_date, 0 when there is none
  for (uint32_t e = 0; e < n; e++)
    if (b.chain[e].alloc) tb = std::min(tb, b.chain[e].alloc);
  CHECK(pt.tbase == (tb == ~0ull ? 0 : tb));
  uint32_t k = 0, cmap_at = 0;
  for (uint32_t q = 0; q < P; q++) {
    const PartInfo& pi = pt.parts[q];
    CHECK(pi.k0 == k && pi.nk >= 1 && pi.nk <= kPartKeys && pi.e0 == in.entry_off[k] && k + pi.nk <= in.K);
    if (pi.k0 != k || !pi.nk || k + pi.nk > in.K) return;
    k += pi.nk;
    CHECK(pi.ne == in.entry_off[k] - pi.e0 && (pi.ne <= kPartEntries || pi.nk == 1) && pi.pad[0] == 0 && pi.pad[1] == 0);
    CHECK(in.keys[k - 1] - in.keys[pi.k0] < (1ull << (kAddrBits - 1)));
    // its dense cells, and where they are counted
    uint64_t cb = ~0ull, ce = 0, cc = 0;
    bool dead = true;
    for (uint32_t e = pi.e0; e < pi.e0 + pi.ne; e++) {
      dead = dead && b.chain[e].free == 0;
      if (b.chain[e].hist == kHistSparse) continue;
      const uint64_t np = in.npages[b.chain[e].id];
      cb = std::min(cb, b.chain[e].hist), ce = std::max(ce, b.chain[e].hist + np), cc += np;
    }
    const bool packed = pt.online && cc && cc * in.T <= kPartCells;
    CHECK(pi.cb == (cc ? cb : 0));
    if (packed) {  // an online table's cells in table order: lrel the entry's first, cmap each cell's histogram cell
      CHECK(pi.cmap == cmap_at && pi.span == cc && pi.pages_lds == 1);
      uint32_t off = 0;
      for (uint32_t e = pi.e0; e < pi.e0 + pi.ne; e++) {
        if (b.chain[e].hist == kHistSparse) {
          CHECK(pt.pe_lrel[e] == kEmpty32);
          continue;
        }
        CHECK(pt.pe_lrel[e] == off);
        for (uint64_t g = 0; g < in.npages[b.chain[e].id]; g++, off++)
          CHECK(cmap_at + off < pt.pe_cmap.size() && pt.pe_cmap[cmap_at + off] == b.chain[e].hist + g);
      }
      cmap_at += off;
    } else {
      CHECK(pi.cmap == ~0u && pi.span == (cc ? ce - cb : 0) && pi.pages_lds == (cc && (ce - cb) * in.T <= kPartCells));
      if (pt.online)
        for (uint32_t e = pi.e0; e < pi.e0 + pi.ne; e++) CHECK(pt.pe_lrel[e] == kEmpty32);
    }
    if (pi.nk > 1 && cc) CHECK((pt.online ? cc : ce - cb) * in.T <= kPartCells);  // (one key alone may exceed)
    // greedy: the next key would break a rule
    if (k < in.K) {
      uint64_t nb = cb, ne = ce, nc = cc;
      for (uint32_t e = in.entry_off[k]; e < in.entry_off[k + 1]; e++)
        if (b.chain[e].hist != kHistSparse) {
          const uint64_t np = in.npages[b.chain[e].id];
          nb = std::min(nb, b.chain[e].hist), ne = std::max(ne, b.chain[e].hist + np), nc += np;
        }
      CHECK(pi.nk == kPartKeys || in.keys[k] - in.keys[pi.k0] >= (1ull << (kAddrBits - 1)) ||
            in.entry_off[k + 1] - pi.e0 > kPartEntries || (nc && (pt.online ? nc : ne - nb) * in.T > kPartCells));
    }
    CHECK(pt.pbounds[q] == in.keys[pi.k0]);
    CHECK(((pt.pdead[q >> 5] >> (q & 31)) & 1u) == (dead ? 1u : 0u));
    check_part_dir(b, q);
    check_part_records(b, q);
  }
  CHECK(k == in.K && cmap_at == pt.pe_cmap.size());
  for (uint32_t q = P; q <= kMaxParts; q++) CHECK(pt.pbounds[q] == ~0ull && !((pt.pdead[q >> 5] >> (q & 31)) & 1u));
  check_route(name, pt.route, pt.pbounds, P);
}

static void expect_cut(const Built& b, const std::vector<std::pair<uint32_t, uint32_t>>& want) {
  CHECK(b.pt.ok && b.pt.parts.size() == want.size());
  for (uint32_t q = 0; b.pt.ok && q < want.size() && q < b.pt.parts.size(); q++)
    CHECK(b.pt.parts[q].k0 == want[q].first && b.pt.parts[q].nk == want[q].second);
}

static const uint64_t kHeap = 0x7f0000000000ull;

static void cut_cases() {
  {  // 1024 single-entry keys: 1023 + 1 (and 1023 keys: the small table, no path)
    Tab t;
    for (uint32_t i = 0; i < 1024; i++) t.plain(kHeap + i * 4096ull);
    Built b;
    build(t, nullptr, 2, b);
    expect_cut(b, {{0, 1023}, {1023, 1}});
    check_parts("cut.k1024", b);
    Tab s;
    for (uint32_t i = 0; i < 1023; i++) s.plain(kHeap + i * 4096ull);
    Built c;
    build(s, nullptr, 2, c);
    CHECK(!c.pt.ok);
  }
  {  // two entries per key: kPartEntries cuts at 768 keys; the older entries past kOldLds stay out of the list
    Tab t;
    for (uint32_t i = 0; i < 1100; i++) t.plain(kHeap + i * 4096ull, 2);
    Built b;
    build(t, nullptr, 2, b);
    expect_cut(b, {{0, 768}, {768, 332}});
    check_parts("cut.two_per_key", b);
    const uint32_t w511 = b.pt.pe_pnode[511].w, w512 = b.pt.pe_pnode[512].w;
    CHECK((w511 & kPnOldLds) && (w511 & kPnOlder) && !(w512 & kPnOldLds) && (w512 & kPnOlder));
  }
  for (uint32_t reuse : {1536u, 1537u}) {  // one key reused kPartEntries times is a partition; once more: no path
    Tab t;
    for (uint32_t i = 0; i < 1100; i++) t.plain(kHeap + i * 4096ull, i == 5 ? reuse : 1);
    Built b;
    build(t, nullptr, 2, b);
    if (reuse == 1536) expect_cut(b, {{0, 5}, {5, 1}, {6, 1023}, {1029, 71}});
    else CHECK(!b.pt.ok);
    check_parts("cut.reuse" + std::to_string(reuse), b);
  }
  for (uint64_t lift : {(1ull << 39) - 8, 1ull << 39}) {  // a key 2^39 past the partition's first cuts
    Tab t;
    for (uint32_t i = 0; i < 1100; i++) {
      const uint64_t key = i < 500 ? kHeap + i * 4096ull : kHeap + lift + (i - 500) * 4096ull;
      t.add(key, {nmg_object{key, 64, i < 500 ? 1000 + i : 0ull, i < 500 ? 5000ull : 0ull}});  // (the upper keys: free_date 0)
    }
    Built b;
    build(t, nullptr, 2, b);
    if (lift >> 39) {
      expect_cut(b, {{0, 500}, {500, 600}});
      CHECK(b.pt.ok && b.pt.pdead[0] == 2u);  // the second partition is dead
    } else {
      expect_cut(b, {{0, 501}, {501, 599}});  // (key 500 stays; key 501 is 4088 bytes past 2^39)
    }
    check_parts(lift >> 39 ? "cut.gap39" : "cut.gap39less8", b);
  }
  {  // T = 2, 15 pages an entry: 955 keys hold 14325 cells, 956 would cross kPartCells / 2
    Tab t;
    for (uint32_t i = 0; i < 1100; i++) t.plain(kHeap + i * 65536ull, 1, 14 * 4096 + 100);
    Built b;
    build(t, nullptr, 2, b);
    expect_cut(b, {{0, 955}, {955, 145}});
    CHECK(b.pt.ok && b.pt.parts[0].span == 14325 && b.pt.parts[0].pages_lds == 1);
    check_parts("cut.cells", b);
  }
  {  // one key alone past kPartCells: its own partition, cells in global memory
    Tab t;
    for (uint32_t i = 0; i < 1100; i++) t.plain(kHeap + i * (1ull << 27), 1, i == 10 ? 19999 * 4096ull + 1 : 64);
    Built b;
    build(t, nullptr, 2, b);
    expect_cut(b, {{0, 10}, {10, 1}, {11, 1023}, {1034, 66}});
    CHECK(b.pt.ok && b.pt.parts[1].span == 20000 && b.pt.parts[1].pages_lds == 0 && b.pt.parts[0].pages_lds == 1);
    check_parts("cut.lone_cells", b);
  }
  for (uint32_t K : {2047u, 2048u}) {  // keys 2^39 apart: a partition each; kMaxParts of them at most
    Tab t;
    for (uint32_t i = 0; i < K; i++) t.plain(0x1000 + ((uint64_t)i << 39));
    Built b;
    build(t, nullptr, 2, b);
    CHECK(b.pt.ok == (K == 2047) && (!b.pt.ok || b.pt.nparts == 2047));
    check_parts("cut.apart" + std::to_string(K), b);
  }
}

static void online_cases() {
  // 1100 keys, one in eight reused, one entry too large for dense cells; ids as
  // the identity (offline), as a permutation, and with 2^31 dense cells
  Tab t;
  for (uint32_t i = 0; i < 1100; i++) t.plain(kHeap + i * 65536ull, i % 8 == 3 ? 3 : 1, i == 700 ? 1ull << 36 : 4096 * (i % 5) + 8);
  const uint32_t E = (uint32_t)t.objs.size();
  std::vector<uint32_t> ident(E), perm(E);
  for (uint32_t j = 0; j < E; j++) ident[j] = j, perm[j] = (uint32_t)(((uint64_t)j * 7919 + 13) % E);  // (7919 is prime to E)
  {
    std::vector<uint32_t> seen(E, 0);
    for (uint32_t id : perm) seen[id]++;
    CHECK(std::count(seen.begin(), seen.end(), 1u) == (long)E);
  }
  Built off, idn, on, big;
  build(t, nullptr, 2, off);
  build(t, ident.data(), 2, idn);
  build(t, perm.data(), 2, on);
  build(t, perm.data(), 2, big, 1ull << 31);
  check_parts("online.offline", off);
  check_parts("online.identity", idn);
  check_parts("online.permuted", on);
  CHECK(off.pt.ok && !off.pt.online && idn.pt.ok && !idn.pt.online && idn.pt.pe_lrel.empty() && idn.pt.pe_cmap.empty());
  CHECK(idn.pt.pe_pnode.size() == off.pt.pe_pnode.size() &&
        !memcmp(idn.pt.pe_pnode.data(), off.pt.pe_pnode.data(), off.pt.pe_pnode.size() * sizeof(Word16)) &&
        !memcmp(idn.pt.pe_info.data(), off.pt.pe_info.data(), off.pt.pe_info.size() * sizeof(Word8)));
  CHECK(on.pt.ok && on.pt.online && !on.pt.pe_cmap.empty());
  uint32_t sparse = 0;
  for (uint32_t e = 0; on.pt.ok && e < E; e++) sparse += on.chain[e].hist == kHistSparse && on.pt.pe_lrel[e] == kEmpty32;
  CHECK(sparse == 1);  // the 64 GiB entry
  CHECK(!big.pt.ok);   // (an online table's cell indices are 32-bit)
  digest_parts("online.cells2g", big.pt);
}

static void record_cases() {
  // 1100 keys 1 MiB apart; among plain ones: one freed before tbase, saturated dates, a key
  // with three entries, and last an object above 4 GiB (its page cells make it a partition
  // of its own); all alive from 5000 on
  Tab t;
  for (uint32_t i = 0; i < 1100; i++) {
    const uint64_t key = kHeap + ((uint64_t)i << 20);
    if (i == 1099) t.add(key, {nmg_object{key, (4ull << 30) + 5, 5000, 9000}});
    else if (i == 4) t.add(key, {nmg_object{key, 64, 0, 4999}});
    else if (i == 6) t.add(key, {nmg_object{key, 64, 5000 + (1ull << 40), ~0ull}});
    else if (i == 9) t.add(key, {nmg_object{key, 64, 8000, 9000}, nmg_object{key, 128, 7000, 7999}, nmg_object{key, 32, 0, 100}});
    else t.add(key, {nmg_object{key, 64, 5000 + i, 6000 + i}});
  }
  Built b;
  build(t, nullptr, 2, b);
  check_parts("records", b);
  CHECK(b.pt.ok && b.pt.tbase == 5000);
  expect_cut(b, {{0, 1023}, {1023, 76}, {1099, 1}});
  if (!b.pt.ok || b.pt.nparts != 3) return;
  const Word16 big = b.pt.pe_pnode[2 * kPartSlots], never = b.pt.pe_pnode[4], sat = b.pt.pe_pnode[6], three = b.pt.pe_pnode[9];
  CHECK((big.w & kPnExact) && big.x == 0);
  CHECK(never.y == ~0u && never.z == 0 && never.x == 0 && !(never.w & kPnExact));
  CHECK(sat.y == ~0u && sat.z == ~0u);  // (2^40 >> kPnQShift = 2^32: both dates saturate)
  CHECK((three.w & kPnOldLds) && (three.w >> kPnOldShift) == 2 && (three.w & 2047u) == 9);
  // key 9's older entries at list index (table position - e0 - key index + i - 1) = 0 and 1; the second never matches
  const uint64_t f = t.keys[0], k9 = t.keys[9];
  CHECK(f + b.pt.pe_old[0].x == k9 + 128 && f + b.pt.pe_old[0].w == k9 && b.pt.pe_old[0].y == (2000u >> kPnQShift));
  CHECK(b.pt.pe_old[1].x == 0 && b.pt.pe_old[1].y == ~0u && b.pt.pe_old[1].z == 0 && b.pt.pe_old[1].w == 0);
  // a key whose older entries would end past kOldLds: that key only, the ones before it keep the list
  Tab u;
  for (uint32_t i = 0; i < 1100; i++) u.plain(kHeap + ((uint64_t)i << 20), i == 20 ? 511 : i == 30 ? 4 : i == 40 ? 2 : 1);
  Built c;
  build(u, nullptr, 2, c);
  check_parts("records.old_full", c);
  if (c.pt.ok)
    CHECK((c.pt.pe_pnode[20].w & kPnOldLds) && !(c.pt.pe_pnode[30].w & kPnOldLds) && (c.pt.pe_pnode[30].w & kPnOlder) &&
          !(c.pt.pe_pnode[40].w & kPnOldLds));  // key 20's 510 fit; key 30's three would end at 513; key 40's one at 514
  // no allocation date at all: tbase 0, every partition dead
  Tab z;
  for (uint32_t i = 0; i < 1100; i++) {
    const uint64_t key = kHeap + ((uint64_t)i << 20);
    z.add(key, {nmg_object{key, 64, 0, 0}});
  }
  Built d;
  build(z, nullptr, 2, d);
  check_parts("records.no_dates", d);
  CHECK(d.pt.ok && d.pt.tbase == 0 && d.pt.pdead[0] == 3u);
}

// ---- the Python test's tables: u32 count; per table u32 K, u32 E, u64 keys[K],
// u32 entry_off[K + 1], u64 (addr, size, alloc, free)[E]

static bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, n, 1, f) == 1; }

static int file_tables(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) return 1;
  uint32_t nt = 0;
  bool ok = read_exact(f, &nt, 4);
  for (uint32_t ti = 0; ok && ti < nt; ti++) {
    uint32_t K = 0, E = 0;
    ok = read_exact(f, &K, 4) && read_exact(f, &E, 4);
    Tab t;
    t.keys.resize(K);
    t.off.resize((size_t)K + 1);
    t.objs.resize(E);
    ok = ok && read_exact(f, t.keys.data(), (size_t)K * 8) && read_exact(f, t.off.data(), ((size_t)K + 1) * 4) &&
         read_exact(f, t.objs.data(), (size_t)E * sizeof(nmg_object));
    if (!ok) break;
    Built b;
    build(t, nullptr, 2, b);
    check_parts("file" + std::to_string(ti), b);
    CHECK(b.pt.ok);
    for (uint32_t q = 0; q < b.pt.parts.size(); q++) {
      const PartInfo& pi = b.pt.parts[q];
      printf("part %u %u %u %u %u\n", ti, q, pi.k0, pi.nk, pi.dshift);
      for (uint32_t j = 0; j < kPartDir; j++) {
        const uint32_t x = b.pt.pe_dir[(size_t)q * kPartDir + j].x;
        printf("slot %u %u %u %u %u %u\n", ti, q, j, x & 1023u, (x >> 10) & 2047u, (x >> 21) & 1u);
      }
    }
  }
  fclose(f);
  return ok ? 0 : 1;
}

int main(int argc, char** argv) {
  const char* path = nullptr;
  for (int i = 1; i < argc; i++) {
    if (!strcmp(argv[i], "--digests")) g_digests = true;
    else path = argv[i];
  }
  for (uint32_t K : {0u, 1u, 2u, 1022u, 1023u}) check_small(K);
  check_big("big1024", spread_keys(1024, 0x10000, 4096), false, 0);
  check_big("big4095", spread_keys(4095, 0x10000, 4096), false, 0);
  check_big("big4096", spread_keys(4096, 0x10000, 4096), false, 1);
  check_big("big8190", spread_keys(8190, 0x10000, 4096), false, 1);
  check_big("big8191", spread_keys(8191, 0x10000, 4096), false, 2);  // (4096 fences of two keys would be one too many)
  check_big("big20000", spread_keys(20000, 0x10000, 1 << 20), false, 3);
  check_big("big4096.no_dir", spread_keys(4096, 0x10000, 4096), true, 1);
  {  // bucket 100's second key 2^40 past its first: slots of 2^39 bytes, no directory for it
    std::vector<uint64_t> k = spread_keys(4096, 0x10000, 4096);
    for (uint32_t i = 201; i < 4096; i++) k[i] += 1ull << 40;
    check_big("big4096.wide", k, false, 1, 100);
  }
  route_cases();
  cut_cases();
  online_cases();
  record_cases();
  if (path && file_tables(path)) {
    fprintf(stderr, "cannot read %s\n", path);
    return 1;
  }
  if (g_failed) {
    fprintf(stderr, "nmg_table_build_host: %d checks failed\n", g_failed);
    return 1;
  }
  printf("nmg_table_build_host: ok\n");
  return 0;
}
