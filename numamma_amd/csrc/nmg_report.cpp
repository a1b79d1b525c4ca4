// nmg_report.cpp -- host half of the drop-in: the report part of ma_finalize
// (src/mem_analyzer.c:1802-1884) fed by the engine's device results.
//
//  * call-site registry: sites are created in first-match order (the order
//    __match_sample reaches new_call_site, mem_sampling.c:665-669), then every
//    matched object is re-attached with find_call_site in FOREACH_HASH order
//    (update_call_sites, mem_analyzer.c:1380-1436).  find_call_site's linear
//    scan of the LIFO site list is replaced by two hash maps keyed exactly on
//    its match predicate (callstack-keyed sites / caller_rip-keyed sites);
//    "first in the list" == newest == highest id among the candidates.
//  * __sort_sites (mem_analyzer.c:1531-1557) is reproduced exactly, including
//    its int-truncated running minimum (quirk Q9): a plain sort when every
//    key fits an int, otherwise an O(chain log S) segment-tree simulation of
//    the selection passes.
//  * printf formats are byte-identical to __print_counters (:1438-1487),
//    print_call_site_summary (:1597-1640), __plot_counters (:1559-1583) and
//    mem_sampling_statistics (mem_sampling.c:357-361).
#include <sys/stat.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <thread>
#include <chrono>
#include <cstdlib>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <set>
#include <string>
#include <unordered_map>
#include <vector>

#include "nmg_internal.h"

namespace nmg {
namespace {

constexpr uint32_t kMemTypeStack = 2;  // enum mem_type, mem_analyzer.h:58-64

struct Site {
  uint32_t id;
  std::string caller;
  uint64_t caller_rip;
  const uint64_t* callstack;
  int32_t callstack_size;
  uint64_t buffer_size;            // initial_buffer_size of the creating object
  uint32_t mem_type;               // site->mem_info.mem_type
  uint64_t mem_info_buffer_size;   // site->mem_info.buffer_size (:1363)
  uint32_t nb_mallocs = 0;
  uint64_t read_count = 0, read_weight = 0, write_count = 0, write_weight = 0;
  std::vector<uint32_t> objects;   // entries attached at finalize
};

// (the tail points into the caller's callstack pool, alive for the report)
struct CsKey {
  uint64_t size;
  int32_t cs_size;
  uint32_t n;            // tail length
  const uint64_t* tail;  // callstack[3..cs_size)
  uint64_t hash;
  bool operator==(const CsKey& o) const {
    return size == o.size && cs_size == o.cs_size && n == o.n && (n == 0 || !memcmp(tail, o.tail, 8ull * n));
  }
};
struct CsKeyHash {
  size_t operator()(const CsKey& k) const { return (size_t)k.hash; }
};
struct RipKey {
  uint64_t size, rip;
  bool operator==(const RipKey& o) const { return size == o.size && rip == o.rip; }
};
struct RipKeyHash {
  size_t operator()(const RipKey& k) const { return (size_t)(k.size * 0x9E3779B97F4A7C15ull ^ k.rip); }
};

class Registry {
 public:
  explicit Registry(const nmg_object_meta* meta) : meta_(meta) {}
  const nmg_object_meta* meta() const { return meta_; }

  // find_call_site (mem_analyzer.c:1302-1331)
  int64_t find(uint32_t e) const {
    const nmg_object_meta& m = meta_[e];
    int64_t best = -1;
    auto a = by_cs_.find(cs_key_of(m.initial_buffer_size, m.callstack, m.callstack_size));
    if (a != by_cs_.end()) best = a->second;
    auto b = by_rip_.find(RipKey{m.initial_buffer_size, m.caller_rip});
    if (b != by_rip_.end() && b->second > best) best = b->second;
    return best;  // sites are indexed by creation order == id - 1
  }

  // new_call_site (mem_analyzer.c:1333-1378)
  int64_t create(uint32_t e, uint64_t npages) {
    const nmg_object_meta& m = meta_[e];
    Site s;
    s.id = (uint32_t)sites.size() + 1;  // next_call_site_id starts at 1 (:1339-1340)
    s.caller = caller_string(m);
    s.caller_rip = m.caller_rip;
    s.callstack = m.callstack;
    s.callstack_size = m.callstack_size;
    s.buffer_size = m.initial_buffer_size;
    s.mem_type = m.mem_type;
    // site->mem_info.buffer_size (:1363) is only ever used as buffer_size /
    // 4096 + 1 rows (__plot_counters :1565), i.e. the entry's page count
    s.mem_info_buffer_size = (npages - 1) * kPageSize;
    int64_t idx = (int64_t)sites.size();
    if (m.callstack)
      by_cs_[cs_key_of(m.initial_buffer_size, m.callstack, m.callstack_size)] = idx;
    else
      by_rip_[RipKey{m.initial_buffer_size, m.caller_rip}] = idx;
    sites.push_back(std::move(s));
    return idx;
  }

  std::vector<Site> sites;  // creation order

 private:
  static CsKey cs_key_of(uint64_t size, const uint64_t* cs, int32_t cs_size) {
    CsKey k{size, cs_size, 0, nullptr, 0};
    if (cs && cs_size > 3) {
      k.tail = cs + 3;
      k.n = (uint32_t)(cs_size - 3);
    }
    uint64_t h = size * 0x9E3779B97F4A7C15ull ^ (uint64_t)(uint32_t)cs_size;
    for (uint32_t i = 0; i < k.n; i++) h = (h ^ k.tail[i]) * 0x100000001B3ull;
    k.hash = h;
    return k;
  }
 public:
  // get_caller_function_from_rip (src/mem_tools.c:91-131): "???" for a NULL
  // rip; replays carry the symbolised string; strings live in 1024-byte slots.
  static std::string caller_string(const nmg_object_meta& m) {
    char buf[1024];
    if (m.caller)
      snprintf(buf, sizeof(buf), "%s", m.caller);
    else if (!m.caller_rip)
      snprintf(buf, sizeof(buf), "???");
    else
      snprintf(buf, sizeof(buf), "[0x%" PRIx64 "]", m.caller_rip);
    return buf;
  }

 private:
  const nmg_object_meta* meta_;
  std::unordered_map<CsKey, int64_t, CsKeyHash> by_cs_;
  std::unordered_map<RipKey, int64_t, RipKeyHash> by_rip_;
};

// (uint64_t)(int64_t)(int)x: the comparison in __sort_sites promotes the
// int-truncated running minimum back to uint64_t (mem_analyzer.c:1544-1547)
inline uint64_t trunc_key(uint64_t x) { return (uint64_t)(int64_t)(int32_t)(uint32_t)x; }

// the first position >= from of the min tree whose value < m, or -1
int64_t first_below(const std::vector<uint64_t>& tree, int64_t node, int64_t lo, int64_t hi, int64_t from,
                    uint64_t m) {
  if (hi < from || tree[node] >= m) return -1;
  if (lo == hi) return lo;
  const int64_t mid = (lo + hi) / 2;
  const int64_t r = first_below(tree, 2 * node, lo, mid, from, m);
  return r >= 0 ? r : first_below(tree, 2 * node + 1, mid + 1, hi, from, m);
}

// Returns the final list order (indices into sites), head first.
std::vector<int64_t> sort_sites(const std::vector<Site>& sites) {
  const int64_t n = (int64_t)sites.size();
  std::vector<int64_t> out;
  out.reserve(n);
  bool small = true;
  for (const Site& s : sites) small &= s.read_weight < (1ull << 31);
  if (small) {
    // selection of the first minimum in list order (list = id descending),
    // pushed at the head: final = weight descending, ties by id ascending
    for (int64_t i = 0; i < n; i++) out.push_back(i);
    std::stable_sort(out.begin(), out.end(), [&](int64_t a, int64_t b) {
      if (sites[a].read_weight != sites[b].read_weight) return sites[a].read_weight > sites[b].read_weight;
      return a < b;
    });
    return out;
  }
  // general case: simulate the passes.  pos 0 = head of the LIFO list = newest.
  int64_t sz = 1;
  while (sz < n) sz <<= 1;
  const uint64_t kDead = ~0ull;
  std::vector<uint64_t> tree(2 * sz, kDead);
  for (int64_t pos = 0; pos < n; pos++) tree[sz + pos] = sites[n - 1 - pos].read_weight;
  for (int64_t i = sz - 1; i >= 1; i--) tree[i] = std::min(tree[2 * i], tree[2 * i + 1]);
  auto remove = [&](int64_t pos) {
    int64_t i = sz + pos;
    tree[i] = kDead;
    for (i >>= 1; i >= 1; i >>= 1) tree[i] = std::min(tree[2 * i], tree[2 * i + 1]);
  };
  std::vector<int64_t> removal;
  removal.reserve(n);
  std::vector<char> alive(n, 1);
  int64_t head = 0;
  for (int64_t pass = 0; pass < n; pass++) {
    while (!alive[head]) head++;
    int64_t pick = head;
    uint64_t m = trunc_key(sites[n - 1 - head].read_weight);
    int64_t from = head;  // the head is compared against itself too
    for (;;) {
      int64_t q = first_below(tree, 1, 0, sz - 1, from, m);
      if (q < 0) break;
      pick = q;
      m = trunc_key(sites[n - 1 - q].read_weight);
      from = q + 1;
    }
    alive[pick] = 0;
    remove(pick);
    removal.push_back(n - 1 - pick);
  }
  for (int64_t i = n - 1; i >= 0; i--) out.push_back(removal[i]);
  return out;
}

const char* kHitNames[9] = {"L1 Hit",         "L2 Hit",           "L3 Hit",
                            "LFB Hit",        "Local RAM Hit",    "Remote RAM Hit",
                            "Remote cache Hit", "IO memory Hit",  "Uncached memory Hit"};
const char* kMissNames[9] = {nullptr,          nullptr,           nullptr,
                             "LFB Miss",       "Local RAM Miss",  "Remote RAM Miss",
                             "Remote cache Miss", "IO memory Miss", "Uncached memory Miss"};

// __print_counters (mem_analyzer.c:1438-1487)
void print_counters(FILE* f, const nmg_mem_counters* counters) {
  for (int i = 0; i < 2; i++) {
    const nmg_mem_counters& c = counters[i];
    if (i == 0) {
      fprintf(f, "\n");
      fprintf(f, "# --------------------------------------\n");
      fprintf(f, "# Summary of all the read memory access:\n");
    } else {
      fprintf(f, "# --------------------------------------\n");
      fprintf(f, "# Summary of all the write memory access:\n");
    }
    fprintf(f, "# Total count          : \t %" PRIu64 "\n", c.total_count);
    fprintf(f, "# Total weigh          : \t %" PRIu64 "\n", c.total_weight);
    if (c.na_miss_count)
      fprintf(f, "# N/A                  : \t %" PRIu64 " (%f %%)\n", c.na_miss_count,
              100. * c.na_miss_count / c.total_count);
    auto line = [&](int b, const char* name) {
      const nmg_count& k = c.b[b];
      if (!k.count) return;
      double pct = 100. * k.count / c.total_count;
      uint64_t avg = k.count ? k.sum_weight / k.count : 0;
      double wpct = c.total_weight ? 100. * k.sum_weight / c.total_weight : 0;
      fprintf(f,
              "# %s\t: %ld (%f %%) \tmin: %" PRIu64 " cycles\tmax: %" PRIu64 " cycles\t avg: %" PRIu64
              " cycles\ttotal weight: %" PRIu64 " (%f %%)\n",
              name, (long)k.count, pct, k.min_weight, k.max_weight, avg, k.sum_weight, wpct);
    };
    for (int g = 0; g < 9; g++) line(g, kHitNames[g]);
    fprintf(f, "\n");
    for (int g = 3; g < 9; g++) line(9 + g, kMissNames[g]);
  }
}

// A site's page x thread matrix (__plot_counters, mem_analyzer.c:1557-1585):
// site->mem_info.buffer_size / 4096 + 1 rows of next_thread_rank cells, each
// the sum of the site's objects' cells; their pages past its rows, and threads
// that do not exist, are dropped.  A stack site has none, nor has a stack
// entry (_dump_call_site, mem_sampling.c:775-808).
struct SiteShape {
  uint64_t rows = 0;
  uint32_t T = 0;
  SiteShape() {}
  SiteShape(const Site& s, uint32_t t)
      : rows(s.mem_type == kMemTypeStack ? 0 : s.mem_info_buffer_size / kPageSize + 1), T(t) {}
  bool holds(uint64_t page, uint64_t th) const { return page < rows && th < T; }
};

// The matrix of the page counts: dense unless huge.
struct SiteHist : SiteShape {
  bool dense = true;
  std::vector<uint32_t> cells;                    // [page][thread]
  std::unordered_map<uint64_t, uint32_t> sparse;  // page * T + thread
  explicit SiteHist(const SiteShape& shape) : SiteShape(shape), dense(rows * T <= (1ull << 26)) {
    if (dense) cells.assign(rows * T, 0);
  }
  void add(uint64_t page, uint32_t th, uint32_t v) {
    if (!holds(page, th)) return;
    if (dense) cells[page * T + th] += v;
    else sparse[page * T + th] += v;
  }
  uint32_t get(uint64_t page, uint32_t th) const {
    if (dense) return cells[page * T + th];
    auto it = sparse.find(page * T + th);
    return it == sparse.end() ? 0 : it->second;
  }
};

// get_data_src_level() belongs to numap (unpinned HEAD, absent here): only
// "L1_Hit", "L2_Hit" and "L3_Hit" are pinned, by README.md:142-147.  The same
// restatement as the oracle's o_data_src_level: the first level bit present
// names the level, then "_Hit" / "_Miss".
std::string data_src_level(uint64_t data_src) {
  const uint32_t lvl = (uint32_t)(data_src >> 5) & 0x3fff;  // union perf_mem_data_src.mem_lvl
  static const struct {
    uint32_t bit;
    const char* name;
  } names[] = {{0x01, "NA"},
               {0x08, "L1"},
               {0x10, "LFB"},
               {0x20, "L2"},
               {0x40, "L3"},
               {0x80, "Local_RAM"},
               {0x100, "Remote_RAM_1_hop"},
               {0x200, "Remote_RAM_2_hops"},
               {0x400, "Remote_Cache_1_hop"},
               {0x800, "Remote_Cache_2_hops"},
               {0x1000, "IO_Memory"},
               {0x2000, "Uncached_Memory"}};
  const char* n = "Unknown";
  for (const auto& x : names)
    if (lvl & x.bit) {
      n = x.name;
      break;
    }
  return std::string(n) + ((lvl & 0x02) ? "_Hit" : ((lvl & 0x04) ? "_Miss" : ""));
}

template <class T>
T load(const uint8_t* p) {
  T v;
  memcpy(&v, p, sizeof(T));
  return v;
}

// A file closed when its owner goes; stdout, which write_report may be given to
// write to, is flushed instead.
struct FileClose {
  void operator()(FILE* f) const { f == stdout ? fflush(f) : fclose(f); }
};
typedef std::unique_ptr<FILE, FileClose> File;

// settings.output_dir ("." by default), made here as get_log_dir makes it
// (mem_intercept.c:402-409): where every file but write_report's stdout goes.
struct OutDir {
  std::string dir;
  OutDir() {}  // (none yet)
  explicit OutDir(const nmg_report_options* opts) : dir(opts && opts->output_dir ? opts->output_dir : ".") {
    mkdir(dir.c_str(), S_IRWXU);
  }
  File open(const std::string& base, std::string& err) const {
    const std::string path = dir + "/" + base;
    File f(fopen(path.c_str(), "w"));
    if (!f) err = "cannot open " + path;
    return f;
  }
};
std::string site_file(const char* kind, uint32_t id) {
  return std::string("callsite_") + kind + "_" + std::to_string((int)id) + ".dat";
}

// One matrix file: `shape.rows` lines of `shape.T` cells, in that order;
// cell(buf, size, page, thread) formats one and returns its length.
template <class Cell>
void write_matrix(FILE* f, const SiteShape& shape, Cell&& cell) {
  std::string line;
  char buf[32];
  for (uint64_t pg = 0; pg < shape.rows; pg++) {
    line.clear();
    for (uint32_t th = 0; th < shape.T; th++) line.append(buf, cell(buf, sizeof(buf), pg, th));
    line.push_back('\n');
    fwrite(line.data(), 1, line.size(), f);
  }
}

// (key, value) cells in any order -> ascending keys, each once, the values of equal keys summed
typedef std::vector<std::pair<uint64_t, uint64_t>> KeyedCells;
void sum_runs(KeyedCells& l) {
  std::sort(l.begin(), l.end());
  size_t m = 0;
  for (const auto& c : l)
    if (m && l[m - 1].first == c.first) l[m - 1].second += c.second;
    else l[m++] = c;
  l.resize(m);
}

// entry e's rows of the n (entry, thread, page, count) rows sorted by entry: [begin[e], begin[e + 1])
std::vector<int64_t> entry_ranges(const uint32_t* cells, int64_t n, uint32_t E) {
  std::vector<int64_t> begin((size_t)E + 1, 0);
  for (int64_t i = 0; i < n; i++) begin[cells[4 * i] + 1]++;
  for (uint32_t e = 0; e < E; e++) begin[e + 1] += begin[e];
  return begin;
}

// The unmatched-sample log header (mem_sampling.c:608-638): the traced
// process's maps file copied by `while (!feof) { fgets(line, 1024); fprintf }`,
// which repeats the last line when the file ends with a newline.
void write_maps_header(FILE* f, const nmg_report_options* opts) {
  fprintf(f, "# %s content:\n", opts->maps_path ? opts->maps_path : "/proc/self/maps");
  const char* t = opts->maps_text ? opts->maps_text : "";
  const size_t len = strlen(t);
  char line[1024];
  line[0] = 0;
  size_t pos = 0;
  bool eof = len == 0;
  while (!eof) {
    if (pos >= len) {
      eof = true;  // fgets returns NULL; line keeps the last line
    } else {
      size_t n = 0;
      while (pos < len && n < sizeof(line) - 1) {
        line[n++] = t[pos++];
        if (line[n - 1] == '\n') break;
      }
      line[n] = 0;
      if (pos >= len && line[n - 1] != '\n') eof = true;  // EOF met inside the last line
    }
    fprintf(f, "# %s", line);
  }
  fprintf(f, "#\n#\n#\n");
  fprintf(f, "#thread_rank timestamp address mem_level access_weight access_type\n");
}

// dladdr() of a callstack frame, from the traced process's module table
const nmg_module* find_module(const std::vector<const nmg_module*>& mods, uint64_t rip) {
  auto it = std::upper_bound(mods.begin(), mods.end(), rip,
                             [](uint64_t x, const nmg_module* m) { return x < m->lo; });
  if (it == mods.begin()) return nullptr;
  const nmg_module* m = *(it - 1);
  return rip < m->hi ? m : nullptr;
}

// print_object_summary (mem_analyzer.c:1728-1748): one row per object of
// mem_list in FOREACH_HASH order (= the table's entry order).  Under
// USE_HASHTABLE (:23) print_object_summary_from_list ignores its list
// argument, so the second call, meant for past_mem_list, prints mem_list
// again (quirk Q20: every row twice).
int write_object_summary(const OutDir& dir, const nmg_host_results* r, const nmg_object_meta* meta,
                         const nmg_report_options* opts, std::string& err) {
  const File file = dir.open("all_memory_objects.dat", err);
  if (!file) return NMG_ERR_IO;
  FILE* f = file.get();
  std::vector<const nmg_module*> mods;
  for (uint32_t i = 0; opts->modules && i < opts->nb_modules; i++) mods.push_back(&opts->modules[i]);
  std::sort(mods.begin(), mods.end(), [](const nmg_module* a, const nmg_module* b) { return a->lo < b->lo; });
  fprintf(f, "#object_id\taddress\tsize\tallocation_date\tdeallocation_date\tcallstack_rip\tcallstack_offsets"
             "\tcallsite_rip\tcallsite\n");
  // _print_object_summary (:1642-1704)
  std::vector<std::string> rows(r->nb_entries);
  std::string rips, offs;
  char buf[64];
  for (uint32_t e = 0; e < r->nb_entries; e++) {
    const nmg_object& o = r->objects[e];
    const nmg_object_meta& m = meta[e];
    rips.clear();
    offs.clear();
    if (m.callstack) {
      for (int32_t i = 3; i < m.callstack_size; i++) {
        const uint64_t rip = m.callstack[i];
        const char* prefix = i == 3 ? "" : ",";
        const nmg_module* mod = find_module(mods, rip);
        const uint64_t fbase = mod ? mod->fbase : 0;
        snprintf(buf, sizeof(buf), "%s0x%" PRIx64, prefix, rip);
        rips += buf;
        offs += prefix;
        offs += mod && mod->fname ? mod->fname : "(null)";
        snprintf(buf, sizeof(buf), ":%td", (ptrdiff_t)(rip - fbase));
        offs += buf;
      }
    } else {
      rips = "NULL";
      offs = "NULL";
    }
    std::string& row = rows[e];
    snprintf(buf, sizeof(buf), "%d\t0x%" PRIx64 "\t%ld\t", (int)m.id, o.buffer_addr, (long)o.buffer_size);
    row = buf;
    snprintf(buf, sizeof(buf), "%" PRIu64 "\t%" PRIu64 "\t", o.alloc_date, o.free_date);
    row += buf;
    row += rips;
    row += '\t';
    row += offs;
    snprintf(buf, sizeof(buf), "\t0x%" PRIx64 "\t", m.caller_rip);
    row += buf;
    row += Registry::caller_string(m);
    row += '\n';
  }
  for (int pass = 0; pass < 2; pass++)
    for (const std::string& row : rows) fwrite(row.data(), 1, row.size(), f);
  return NMG_OK;
}

// The call sites of the results r (settings.match_samples on), as ma_finalize
// leaves them: created in the analysis order of each object's first matched
// sample, then every object that reaches update_call_sites attached; none with
// match_samples off.  The one registry of every writer and of the placement
// groups: a site's id is the same in all.  phase: write_report's timing marks.
int site_registry(Registry& reg, const nmg_host_results* r, bool online, std::string& err,
                  const std::function<void(const char*)>& phase = [](const char*) {}) {
  if (!r->match_samples) return NMG_OK;
  const nmg_object_meta* meta = reg.meta();
  const uint32_t E = r->nb_entries;
  std::vector<uint32_t> matched;
  for (uint32_t e = 0; e < E; e++)
    if (r->first_ordinal[e] != ~0ull) matched.push_back(e);
  // objects that reach update_call_sites: the matched ones, or every one online
  std::vector<uint32_t> updated;
  if (online)
    for (uint32_t e = 0; e < E; e++) updated.push_back(e);
  else
    updated = matched;
  for (uint32_t e : updated)
    if (meta[e].callstack == nullptr && meta[e].callstack_size > 3) {
      err = "entry with NULL callstack and callstack_size > 3 (the reference dereferences NULL)";
      return NMG_ERR_INVALID;
    }
  // creation: in the analysis order of each object's first matched sample
  std::vector<uint32_t> order(matched);
  std::sort(order.begin(), order.end(),
            [&](uint32_t a, uint32_t b) { return r->first_ordinal[a] < r->first_ordinal[b]; });
  phase("registry: order");
  for (uint32_t e : order)
    if (reg.find(e) < 0) reg.create(e, r->buffer_size[e] / kPageSize + 1);
  phase("registry: create");
  // update_call_sites in FOREACH_HASH order (= flattened order); online, an
  // object never matched finds or creates its site here
  for (uint32_t e : updated) {
    int si = reg.find(e);
    if (si < 0) si = reg.create(e, r->buffer_size[e] / kPageSize + 1);
    Site& site = reg.sites[si];
    site.nb_mallocs++;
    const uint64_t* cw = r->count_weight + (uint64_t)e * 4;
    site.read_count += cw[0];
    site.read_weight += cw[1];
    site.write_count += cw[2];
    site.write_weight += cw[3];
    site.objects.push_back(e);
  }
  return NMG_OK;
}

// the site whose per-site files take entry e's samples and cells, or -1: a
// stack entry has none, nor has an entry without matched samples
int64_t file_site(const Registry& reg, uint32_t e) {
  return reg.meta()[e].mem_type == kMemTypeStack ? -1 : reg.find(e);
}

}  // namespace

// callsite_timeline_<id>.dat per call site with a non-zero cell (the format is
// in include/numamma_gpu.h).  rows: (entry, bin, thread, row, count), any
// order; a site's cell sums its objects' cells, as update_call_sites sums
// their page blocks.
int write_timeline(const nmg_host_results* r, const nmg_object_meta* meta, const nmg_report_options* opts,
                   const nmg_timeline_options* tl, const uint32_t* rows, int64_t n, std::string& err) {
  Registry reg(meta);
  if (const int rc = site_registry(reg, r, opts && opts->online, err)) return rc;
  // per site: (bin, thread, row) key and count of every row of its objects
  std::vector<KeyedCells> per(reg.sites.size());
  for (int64_t i = 0; i < n; i++) {
    const uint32_t* q = rows + 5 * i;
    const int64_t si = q[4] ? file_site(reg, q[0]) : -1;
    if (si >= 0) per[si].push_back({(uint64_t(q[1]) << 42) | (uint64_t(q[2]) << 32) | q[3], q[4]});
  }
  const OutDir dir(opts);
  for (size_t si = 0; si < per.size(); si++) {
    if (per[si].empty()) continue;
    sum_runs(per[si]);
    const File f = dir.open(site_file("timeline", reg.sites[si].id), err);
    if (!f) return NMG_ERR_IO;
    fprintf(f.get(), "#thread_rank timestamp offset count\n");
    for (const auto& c : per[si]) {
      const uint64_t bin = c.first >> 42, th = (c.first >> 32) & 0x3ff, row = c.first & 0xffffffffull;
      fprintf(f.get(), "%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", th, tl->t0 + (bin << tl->bin_shift),
              row << (12 + tl->row_shift), c.second);
    }
  }
  return NMG_OK;
}

// callsite_cost_<id>.dat per call site with a non-zero cell inside its rows
// (the format is in include/numamma_gpu.h): the matrix of
// callsite_counters_<id>.dat with the cost cells in it.  rows: (entry, thread,
// page, value), any order; a site's cell sums its objects' cells (SiteShape).
int write_page_cost(const nmg_host_results* r, const nmg_object_meta* meta, const nmg_report_options* opts,
                    const uint64_t* rows, int64_t n, std::string& err) {
  const uint32_t T = r->nb_threads;
  Registry reg(meta);
  if (const int rc = site_registry(reg, r, opts && opts->online, err)) return rc;
  // per site: (page * T + thread, value) of every row of its objects inside its matrix
  std::vector<KeyedCells> per(reg.sites.size());
  for (int64_t i = 0; i < n; i++) {
    const uint64_t* q = rows + 4 * i;
    const int64_t si = q[3] ? file_site(reg, (uint32_t)q[0]) : -1;
    if (si >= 0 && SiteShape(reg.sites[si], T).holds(q[2], q[1])) per[si].push_back({q[2] * T + q[1], q[3]});
  }
  const OutDir dir(opts);
  for (size_t si = 0; si < per.size(); si++) {
    const KeyedCells& l = per[si];
    if (l.empty()) continue;
    sum_runs(per[si]);
    const File f = dir.open(site_file("cost", reg.sites[si].id), err);
    if (!f) return NMG_ERR_IO;
    size_t i = 0;  // the cells come in the matrix's order
    write_matrix(f.get(), SiteShape(reg.sites[si], T), [&](char* buf, size_t size, uint64_t pg, uint32_t th) {
      const uint64_t v = i < l.size() && l[i].first == pg * T + th ? l[i++].second : 0;
      return snprintf(buf, size, "\t%" PRIu64, v);
    });
  }
  return NMG_OK;
}

// ---- NUMA placement (the rule, the file and their differences from
// scripts/counters_to_binding.py are in include/numamma_gpu.h)

int placement_map(const nmg_placement_options* p, uint32_t T, PlaceMap& out) {
  // (NMG_PLACE_PAGE_COST | NMG_PLACE_HUGE: sparse entries have no cost cells)
  if (!p || p->nb_nodes < 1 || p->nb_nodes > 64 ||
      (p->source != NMG_PLACE_PAGE_COUNTS && p->source != NMG_PLACE_PAGE_COST &&
       p->source != (NMG_PLACE_PAGE_COUNTS | NMG_PLACE_HUGE)))
    return NMG_ERR_INVALID;
  const uint32_t N = p->nb_nodes;
  if (!p->thread_node && T % N) return NMG_ERR_INVALID;
  std::vector<uint32_t>& node = out.node;
  node.assign(T, 0);
  out.node_off.assign(N + 1, 0);
  for (uint32_t t = 0; t < T; t++) {
    node[t] = p->thread_node ? p->thread_node[t] : t / (T / N);
    if (node[t] >= N) return NMG_ERR_INVALID;
    out.node_off[node[t] + 1]++;
  }
  for (uint32_t n = 0; n < N; n++) out.node_off[n + 1] += out.node_off[n];
  std::vector<uint32_t> at(out.node_off.begin(), out.node_off.end() - 1);
  out.thr.resize(T);
  for (uint32_t t = 0; t < T; t++) out.thr[at[node[t]]++] = t;
  out.N = N;
  out.D = p->density_threshold;
  return NMG_OK;
}

void PlaceGroups::add(uint32_t id, uint64_t R, const std::vector<uint32_t>& entries, const uint64_t* npages,
                      const uint8_t* dense, bool all) {
  const size_t m0 = m_entry.size();
  uint32_t longest = 0;
  bool sparse = false;
  for (uint32_t e : entries) {
    if (!dense[e] && !all) continue;
    // (dense: pages * threads <= 2^24; sparse: the key's 32-bit page field)
    const uint32_t np = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(npages[e], R), kPlaceMaxPages);
    if (!np) continue;
    m_entry.push_back(e);
    m_np.push_back(np);
    m_dense.push_back(dense[e] != 0);
    sparse |= !dense[e];
    longest = std::max(longest, np);
  }
  if (m_entry.size() == m0) return;
  gid.push_back(id);
  rows.push_back(longest);
  huge.push_back(sparse);
  m_off.push_back((uint32_t)m_entry.size());
}

void placement_object_groups(uint32_t E, const uint64_t* npages, const uint8_t* dense, PlaceGroups& g, bool all) {
  std::vector<uint32_t> one(1);
  for (uint32_t e = 0; e < E; e++) {
    one[0] = e;
    g.add(e, npages[e], one, npages, dense, all);
  }
}

int placement_site_groups(const nmg_host_results* r, const nmg_object_meta* meta, bool online,
                          const uint64_t* npages, const uint8_t* dense, PlaceGroups& g,
                          std::vector<PlaceSite>& sites, std::string& err, bool all) {
  Registry reg(meta);
  if (const int rc = site_registry(reg, r, online, err)) return rc;
  constexpr uint32_t kGlobalSymbol = 1, kDynamicAllocation = 3;  // enum mem_type, mem_analyzer.h:58-64
  for (const Site& s : reg.sites) {  // (creation order: ascending id)
    std::string ident;
    if (s.mem_type == kDynamicAllocation) {
      ident = "malloc";
    } else if (s.mem_type == kGlobalSymbol) {
      ident = s.caller;
      if (ident.empty() || ident.find_first_of(" \t\n\v\f\r[/") != std::string::npos) continue;
    } else {
      continue;
    }
    const size_t g0 = g.gid.size();
    g.add(s.id, SiteShape(s, 0).rows, s.objects, npages, dense, all);
    if (g.gid.size() != g0) sites.push_back(PlaceSite{s.id, s.caller, ident, s.buffer_size});
  }
  return NMG_OK;
}

void placement_blocks_host(const PlaceGroups& g, const PlaceMap& m, const uint32_t* cells, int64_t nb_cells,
                           uint32_t nb_entries, std::vector<uint64_t>& rows) {
  const uint32_t T = (uint32_t)m.thr.size();
  // the nodes that have a thread, in ascending order (the others count nothing
  // and never win: a page's matrix row holds these only)
  std::vector<uint32_t> used, col(T, 0);
  for (uint32_t n = 0; n < m.N; n++)
    if (m.node_off[n + 1] > m.node_off[n]) {
      for (uint32_t k = m.node_off[n]; k < m.node_off[n + 1]; k++) col[m.thr[k]] = (uint32_t)used.size();
      used.push_back(n);
    }
  const size_t U = used.size();
  const std::vector<int64_t> cell_begin = entry_ranges(cells, nb_cells, nb_entries);
  // A group's pages in ascending order, each with its dominant node and that
  // node's count: a page that qualifies starts a row (gid, node, first, last,
  // count) or extends the last one; one that does not is skipped and closes
  // nothing, so a run goes on across it.
  bool open = false;
  uint32_t open_gid = 0, prev = 0;
  auto append_block = [&](uint32_t gid, uint64_t page, uint32_t node, uint64_t best) {
    if (best <= m.D) return;
    if (open && gid == open_gid && node == prev) {
      rows[rows.size() - 2] = page;
      rows[rows.size() - 1] += best;
    } else {
      const uint64_t row[5] = {gid, node, page, page, best};
      rows.insert(rows.end(), row, row + 5);
      open = true, open_gid = gid, prev = node;
    }
  };
  std::vector<uint64_t> c;
  KeyedCells list;  // a huge group's cells: (page << 6 | node, count)
  for (size_t gi = 0; gi < g.gid.size(); gi++) {
    // a group's cells inside its members' pages: fn(page, thread, count)
    auto for_cells = [&](auto&& fn) {
      for (uint32_t k = g.m_off[gi]; k < g.m_off[gi + 1]; k++) {
        const uint32_t e = g.m_entry[k], np = g.m_np[k];
        for (int64_t i = cell_begin[e]; i < cell_begin[e + 1]; i++) {
          const uint32_t* q = cells + 4 * i;
          if (q[2] < np && q[1] < T) fn(q[2], q[1], q[3]);
        }
      }
    };
    if (g.huge[gi]) {
      // the touched pages only: the members' cells summed by (page, node), then
      // the pages present (nodes ascending; strict: the lowest on a tie)
      list.clear();
      for_cells([&](uint32_t page, uint32_t th, uint32_t n) {
        if (n) list.push_back({(uint64_t(page) << 6) | m.node[th], n});
      });
      sum_runs(list);
      for (size_t i = 0; i < list.size();) {
        const uint64_t page = list[i].first >> 6;
        uint64_t best = 0;
        uint32_t node = 0;
        for (; i < list.size() && list[i].first >> 6 == page; i++)
          if (list[i].second > best) best = list[i].second, node = (uint32_t)(list[i].first & 63);
        append_block(g.gid[gi], page, node, best);
      }
      continue;
    }
    const uint32_t R = g.rows[gi];
    c.assign((size_t)R * U, 0);
    for_cells([&](uint32_t page, uint32_t th, uint32_t n) { c[(size_t)page * U + col[th]] += n; });
    for (uint32_t p = 0; p < R; p++) {
      uint64_t best = 0;
      uint32_t node = 0;
      for (size_t u = 0; u < U; u++)
        if (c[(size_t)p * U + u] > best) best = c[(size_t)p * U + u], node = used[u];  // (strict: the lowest node on a tie)
      append_block(g.gid[gi], p, node, best);
    }
  }
}

int write_blocks(const std::vector<PlaceSite>& sites, const uint64_t* rows, int64_t n,
                 const nmg_report_options* opts, std::string& err) {
  const OutDir dir(opts);
  File file = dir.open("blocks.dat", err);
  if (!file) return NMG_ERR_IO;
  FILE* f = file.get();
  int64_t i = 0;
  for (const PlaceSite& s : sites) {  // (ascending id, as the rows' groups)
    while (i < n && rows[5 * i] < s.id) i++;
    int64_t j = i;
    while (j < n && rows[5 * j] == s.id) j++;
    if (j == i) continue;
    fprintf(f, "#site %u %s\nbegin_block\n%s %" PRIu64 " %" PRId64 "\n", s.id, s.caller.c_str(), s.ident.c_str(),
            s.size, j - i);
    for (; i < j; i++)
      fprintf(f, "%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", rows[5 * i + 1], rows[5 * i + 2],
              rows[5 * i + 3], rows[5 * i + 4]);
    fprintf(f, "end_block\n");
  }
  const bool bad = ferror(f) != 0;
  if (fclose(file.release()) != 0 || bad) {
    err = "cannot write " + dir.dir + "/blocks.dat";
    return NMG_ERR_IO;
  }
  return NMG_OK;
}

// ---- the report: ma_finalize's steps, each a function over what they share
namespace {

// NMG_REPORT_TIMING=1: the time since the last mark, on stderr
struct PhaseClock {
  const bool on = getenv("NMG_REPORT_TIMING") != nullptr;
  std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
  void operator()(const char* name) {
    if (!on) return;
    const auto t = std::chrono::steady_clock::now();
    fprintf(stderr, "nmg_report: %s %.3f s\n", name, std::chrono::duration<double>(t - last).count());
    last = t;
  }
};

// the dump modes' files
struct DumpFiles {
  std::vector<File> site;  // by site index; callsite_dump_<id>.dat, opened at the site's first line
  File all, unmatched;
  bool maps_read = false;  // unmatched has its header
};
struct Report {
  const nmg_host_results* r;
  const nmg_object_meta* meta;
  const nmg_report_options* opts;
  const DumpInput* dump;
  std::string& err;
  FILE* out;  // stdout, or the file in its place
  Registry reg;
  bool online;
  int dflags;
  bool dump_single;
  uint64_t nb_samples = 0, nb_found = 0;  // print_preamble's totals
  OutDir dir;                             // made once the registry stands
  DumpFiles dumps;
};

// mem_sampling_finalize's messages (mem_sampling.c:321-344; none online, :313) and the banner
void print_preamble(Report& c, const uint64_t* found_override) {
  const nmg_host_results* r = c.r;
  const int nbuf = (int)r->nb_buffers;
  if (!c.online) fprintf(c.out, "Analyzing %d sample buffers\n", nbuf);
  size_t total_bytes = 0;
  for (int b = 0; b < nbuf; b++) {
    if (b % 10 == 0 && !c.online)
      fprintf(c.out, "\rAnalyzing sample buffer %d/%d. Total samples so far: %zu", b, nbuf, (size_t)c.nb_samples);
    c.nb_samples += (uint64_t)(int64_t)(int32_t)r->buf_samples[b];  // int nb_samples (:325, :334, :934)
    c.nb_found += (uint64_t)(int64_t)(int32_t)r->buf_found[b];
    total_bytes += r->buf_bytes[b];
  }
  if (found_override) c.nb_found = *found_override;
  if (!c.online) {
    fprintf(c.out, "\n");
    fprintf(c.out, "%zu bytes processed\n", total_bytes);
  }
  fprintf(c.out, "---------------------------------\n");
  fprintf(c.out, "         MEM ANALYZER\n");
  fprintf(c.out, "---------------------------------\n");
}

// f, opened as `base` with its header line when it is not open yet; NULL: c.err
FILE* opened(Report& c, File& f, const std::string& base, const char* header) {
  if (!f && (f = c.dir.open(base, c.err))) fputs(header, f.get());
  return f.get();
}

// One SAMPLE record's lines in the dump files.  false: a file could not be opened.
bool dump_sample(Report& c, const DumpBuffer& b, uint64_t cur) {
  const uint64_t ts = load<uint64_t>(b.data + cur + 8), addr = load<uint64_t>(b.data + cur + 16);
  const uint64_t w = load<uint64_t>(b.data + cur + 24);
  const std::string level = data_src_level(load<uint64_t>(b.data + cur + 32));
  const char acc = b.access == NMG_ACCESS_READ ? 'r' : 'w';
  const uint32_t m = b.match[cur / 8];
  if (!m) {
    if (!c.dumps.maps_read) write_maps_header(c.dumps.unmatched.get(), c.opts);
    c.dumps.maps_read = true;
    fprintf(c.dumps.unmatched.get(), "%u %" PRIu64 " 0x%" PRIxPTR " %s %" PRIu64 " %c\n", b.thread_rank, ts,
            (uintptr_t)addr, level.c_str(), w, acc);
    return true;
  }
  const uint32_t e = m - 1;
  const uint64_t offset = addr - c.dump->entry_addr[e];
  if (c.meta[e].mem_type == kMemTypeStack) return true;
  if (c.dflags & NMG_DUMP_ALL) {  // _dump_mem_info (:740-773)
    FILE* f = opened(c, c.dumps.all, "all_memory_accesses.dat",
                     "#thread_rank timestamp object_id offset mem_level access_weight access_type\n");
    if (!f) return false;
    fprintf(f, "%u %" PRIu64 " %u %" PRIu64 " %s %" PRIu64 " %c\n", b.thread_rank, ts, c.meta[e].id, offset,
            level.c_str(), w, acc);
  }
  const int64_t si = c.dump_single ? c.reg.find(e) : -1;  // _dump_call_site (:775-808)
  if (si < 0) return true;
  FILE* f = opened(c, c.dumps.site[si], site_file("dump", c.reg.sites[si].id),
                   "#thread_rank timestamp offset mem_level access_weight access_type\n");
  if (!f) return false;
  fprintf(f, "%u %" PRIu64 " %" PRIuPTR " %s %" PRIu64 " %c\n", b.thread_rank, ts, (uintptr_t)offset, level.c_str(), w,
          acc);
  return true;
}

// The dump modes (mem_sampling.c:895-914): per SAMPLE record in analysis order
int dump_records(Report& c) {
  if (c.dflags & NMG_DUMP_UNMATCHED)  // opened at init (mem_intercept.c:528-535)
    if (!(c.dumps.unmatched = c.dir.open("unmatched_samples.log", c.err))) return NMG_ERR_IO;
  if (!c.dump || !c.r->match_samples) return NMG_OK;
  c.dumps.site.resize(c.reg.sites.size());
  const bool matched = c.dflags & (NMG_DUMP_CALLSITES | NMG_DUMP_ALL), unmatched = c.dumps.unmatched != nullptr;
  for (const DumpBuffer& b : c.dump->buffers)
    for (uint64_t cur = 0; cur + 8 <= b.len;) {
      const uint32_t type = load<uint32_t>(b.data + cur);
      const uint16_t size = load<uint16_t>(b.data + cur + 6);
      if (size == 0) break;  // (the analysis already reported it)
      if (type == 9 && cur + 40 <= b.len && (b.match[cur / 8] ? matched : unmatched) && !dump_sample(c, b, cur))
        return NMG_ERR_IO;
      cur += size;
    }
  return NMG_OK;
}

// __print_call_site_stats (:1489-1503): the cumulated counters of a site's
// objects, whose min / max stay 0 (memset, and ACC_COUNTER's inverted tests: Q8)
void site_counters(const Report& c, const Site& site, nmg_mem_counters cc[2]) {
  memset(cc, 0, 2 * sizeof(cc[0]));
  for (uint32_t e : site.objects)
    for (uint32_t a = 0; a < 2; a++) {
      const uint64_t* cw = c.r->count_weight + (uint64_t)e * 4 + a * 2;
      const uint64_t* lv = c.dump->levels + ((uint64_t)e * 2 + a) * kLevelWords;
      cc[a].total_count += cw[0];
      cc[a].total_weight += cw[1];
      cc[a].na_miss_count += lv[0];
      for (uint32_t k = 0; k < kBuckets; k++) {
        cc[a].b[k].count += lv[1 + 2 * k];
        cc[a].b[k].sum_weight += lv[2 + 2 * k];
      }
    }
}

// __remove_site during the sort (mem_analyzer.c:1506-1528): the site the walk
// stops at -- the removed one when it heads the list, else its predecessor
// (quirk Q10) -- gets callsite_summary_<id>.dat and its dump file closed, if it
// has one.  The list is id-descending; removals run in the reverse of the
// final order.
int write_summaries(Report& c, const std::vector<int64_t>& order) {
  if (c.dumps.site.empty()) return NMG_OK;  // (no dump file was ever open)
  std::set<int64_t> remaining;
  for (int64_t i = 0; i < (int64_t)c.reg.sites.size(); i++) remaining.insert(i);
  for (auto it = order.rbegin(); it != order.rend(); ++it) {
    auto pos = remaining.find(*it);
    auto nxt = std::next(pos);
    const int64_t cur = nxt == remaining.end() ? *it : *nxt;
    remaining.erase(pos);
    if (!c.dumps.site[cur]) continue;
    nmg_mem_counters cc[2];
    site_counters(c, c.reg.sites[cur], cc);
    const File sf = c.dir.open(site_file("summary", c.reg.sites[cur].id), c.err);
    if (!sf) return NMG_ERR_IO;
    print_counters(sf.get(), cc);
    c.dumps.site[cur].reset();
  }
  return NMG_OK;
}

// __plot_counters (mem_analyzer.c:1557-1585): one callsite_counters_<id>.dat
// per site of `jobs`.  The files are independent: written by a pool of host
// threads (NMG_REPORT_THREADS, default min(16, cores)); the first error stops
// the pool.
int write_site_counters(Report& c, const std::vector<int64_t>& jobs) {
  const nmg_host_results* r = c.r;
  const std::vector<int64_t> cell_begin = entry_ranges(r->cells, r->nb_cells, r->nb_entries);
  unsigned nth = std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
  if (const char* e = getenv("NMG_REPORT_THREADS")) nth = (unsigned)std::max(1, atoi(e));
  nth = (unsigned)std::min<size_t>(nth, jobs.size());
  int rc = NMG_OK;
  std::atomic<size_t> next{0};
  std::mutex mu;
  auto work = [&]() {
    for (size_t j; (j = next.fetch_add(1)) < jobs.size();) {
      const Site& s = c.reg.sites[jobs[j]];
      SiteHist sh(SiteShape(s, r->nb_threads));
      for (uint32_t e : s.objects)
        for (int64_t i = cell_begin[e]; i < cell_begin[e + 1]; i++) {
          const uint32_t* q = r->cells + 4 * i;
          sh.add(q[2], q[1], q[3]);
        }
      std::string why;
      const File df = c.dir.open(site_file("counters", s.id), why);
      if (!df) {
        std::lock_guard<std::mutex> g(mu);
        if (rc == NMG_OK) rc = NMG_ERR_IO, c.err = why;
        next = jobs.size();  // stop the pool
        break;
      }
      write_matrix(df.get(), sh, [&](char* buf, size_t size, uint64_t pg, uint32_t th) {
        return snprintf(buf, size, "\t%d", (int)sh.get(pg, th));
      });
    }
  };
  std::vector<std::thread> pool;
  for (unsigned t = 1; t < nth; t++) pool.emplace_back(work);
  work();
  for (std::thread& t : pool) t.join();
  return rc;
}

// print_call_site_summary (:1597-1640) of the sites with samples, in report
// order, on stdout and in call_sites.log; then their page files
int list_sites(Report& c, FILE* cf, const std::vector<int64_t>& order) {
  std::vector<int64_t> jobs;  // sites whose page file is written (in report order)
  for (int64_t idx : order) {
    const Site& s = c.reg.sites[idx];
    if (!(s.read_count || s.write_count)) continue;
    double avg = 0;
    if (s.read_count) avg = (double)s.read_weight / s.read_count;
    for (int k = 0; k < 2; k++)
      fprintf(k ? c.out : cf,
              "%d\t%s (size=%zu) - %d buffers. %zu read access (total weight: %" PRIu64
              ", avg weight: %f). %" PRIu64 " wr_access\n",
              (int)s.id, s.caller.c_str(), (size_t)s.buffer_size, (int)s.nb_mallocs, (size_t)s.read_count,
              s.read_weight, avg, s.write_count);
    if (c.dump_single && s.mem_type != kMemTypeStack) jobs.push_back(idx);
  }
  return jobs.empty() ? NMG_OK : write_site_counters(c, jobs);
}

}  // namespace

int write_report(const nmg_host_results* r, const nmg_object_meta* meta, const nmg_report_options* opts,
                 const char* stdout_path, std::string& err, const DumpInput* dump, const uint64_t* found_override) {
  PhaseClock phase;
  const File out(stdout_path ? fopen(stdout_path, "w") : stdout);
  if (!out) {
    err = std::string("cannot open ") + stdout_path;
    return NMG_ERR_IO;
  }
  Report c{r, meta, opts, dump, err, out.get(), Registry(meta), opts && opts->online, opts ? opts->dump_flags : 0,
           opts ? opts->dump_single_items != 0 : true};
  if (c.online && c.dflags) {  // the reference's _dump_* read the NULL `samples` list online
    err = "dump modes are not available with online analysis (mem_sampling.c:644, 764, 799)";
    return NMG_ERR_INVALID;
  }
  print_preamble(c, found_override);
  phase("buffers");
  if (const int rc = site_registry(c.reg, r, c.online, err, std::ref(phase))) return rc;
  phase("call-site registry");
  c.dir = OutDir(opts);
  if (const int rc = dump_records(c)) return rc;
  phase("dumps");
  // ma_finalize prints (mem_analyzer.c:1877-1881)
  print_counters(c.out, r->global);
  fprintf(c.out, "Summary of the call sites:\n");
  fprintf(c.out, "--------------------------\n");
  fprintf(c.out, "Sorting call sites\n");
  const std::vector<int64_t> order = sort_sites(c.reg.sites);
  phase("sort");
  if (const int rc = write_summaries(c, order)) return rc;
  c.dumps = DumpFiles();  // (the rest stay open until exit in the reference)
  File cf = c.dir.open("call_sites.log", err);
  if (!cf) return NMG_ERR_IO;
  int rc = list_sites(c, cf.get(), order);
  cf.reset();
  phase("call_sites.log + page files");
  if (!rc && (c.dflags & NMG_DUMP_ALL)) {
    if (r->objects) {
      rc = write_object_summary(c.dir, r, meta, opts, err);
    } else {
      rc = NMG_ERR_INVALID;
      err = "NMG_DUMP_ALL needs nmg_host_results.objects (all_memory_objects.dat)";
    }
  }
  if (rc) return rc;
  // mem_sampling_statistics (mem_sampling.c:357-361): a float percentage
  float percent = 100.0 * (c.nb_samples - c.nb_found) / c.nb_samples;
  fprintf(c.out, "%" PRIu64 " samples (including %" PRIu64 " samples that do not match a known memory buffer / %f%%)\n",
          c.nb_samples, c.nb_samples - c.nb_found, percent);
  return NMG_OK;
}

}  // namespace nmg

// ---- the host entry points: their arguments checked, the writer's text on stderr
namespace {

// res, its thread count, and what the site registry reads per entry
bool registry_args(const nmg_host_results* res, const nmg_object_meta* meta) {
  return res && res->nb_threads <= NMG_MAX_THREADS &&
         (!res->nb_entries || (meta && res->first_ordinal && res->count_weight && res->buffer_size));
}

// res->cells: there, every entry in range, sorted by entry
bool cells_args(const nmg_host_results* res) {
  if (res->nb_cells && !res->cells) return false;
  for (int64_t i = 0; i < res->nb_cells; i++)
    if (res->cells[4 * i] >= res->nb_entries || (i && res->cells[4 * i] < res->cells[4 * i - 4])) return false;
  return true;
}

int said(const char* who, int rc, const std::string& err) {
  if (rc && !err.empty()) fprintf(stderr, "%s: %s\n", who, err.c_str());
  return rc;
}

// the host's view of the page cells: an entry's pages, and whether the engine
// keeps them dense (CellCursor::place's per-entry cap; budgets aside).  With
// NMG_PLACE_HUGE the cap only chooses how a group is walked: every entry of
// res->cells contributes.
bool placement_host_args(const nmg_host_results* res, const nmg_placement_options* p, nmg::PlaceMap& map,
                         std::vector<uint64_t>& npages, std::vector<uint8_t>& dense) {
  if (!res || (res->nb_entries && !res->buffer_size) || res->nb_cells < 0 || res->nb_threads > NMG_MAX_THREADS ||
      nmg::placement_map(p, res->nb_threads, map) ||
      (p->source & ~(uint64_t)NMG_PLACE_HUGE) != NMG_PLACE_PAGE_COUNTS ||  // (nmg_host_results has no cost rows)
      !cells_args(res))
    return false;
  npages.resize(res->nb_entries);
  dense.resize(res->nb_entries);
  for (uint32_t e = 0; e < res->nb_entries; e++) {
    npages[e] = res->buffer_size[e] / nmg::kPageSize + 1;
    dense[e] = npages[e] * std::max(1u, res->nb_threads) <= nmg::kMaxEntryCells;
  }
  return true;
}

}  // namespace

extern "C" int nmg_report_timeline_host(const nmg_host_results* res, const nmg_object_meta* meta,
                                        const nmg_report_options* opts, const nmg_timeline_options* tl,
                                        const uint32_t* rows, int64_t n) {
  if (!registry_args(res, meta) || !tl || n < 0 || (n && !rows) || tl->bin_shift > 63 || tl->nb_bins < 1 ||
      tl->nb_bins > 4096 || tl->row_shift > 20 || tl->reserved != 0)
    return NMG_ERR_INVALID;
  for (int64_t i = 0; i < n; i++)
    if (rows[5 * i] >= res->nb_entries || rows[5 * i + 1] >= tl->nb_bins || rows[5 * i + 2] >= res->nb_threads)
      return NMG_ERR_INVALID;
  std::string err;
  return said("nmg_report_timeline", nmg::write_timeline(res, meta, opts, tl, rows, n, err), err);
}

extern "C" int nmg_report_page_cost_host(const nmg_host_results* res, const nmg_object_meta* meta,
                                         const nmg_report_options* opts, const uint64_t* rows, int64_t n) {
  if (!registry_args(res, meta) || n < 0 || (n && !rows)) return NMG_ERR_INVALID;
  for (int64_t i = 0; i < n; i++)
    if (rows[4 * i] >= res->nb_entries || rows[4 * i + 1] >= res->nb_threads) return NMG_ERR_INVALID;
  std::string err;
  return said("nmg_report_page_cost", nmg::write_page_cost(res, meta, opts, rows, n, err), err);
}

extern "C" int nmg_report_placement_host(const nmg_host_results* res, const nmg_object_meta* meta,
                                         const nmg_report_options* opts, const nmg_placement_options* p) {
  nmg::PlaceMap map;
  std::vector<uint64_t> npages;
  std::vector<uint8_t> dense;
  if (!placement_host_args(res, p, map, npages, dense) || !registry_args(res, meta)) return NMG_ERR_INVALID;
  std::string err;
  nmg::PlaceGroups g;
  std::vector<nmg::PlaceSite> sites;
  std::vector<uint64_t> rows;
  int rc = nmg::placement_site_groups(res, meta, opts && opts->online, npages.data(), dense.data(), g, sites, err,
                                      (p->source & NMG_PLACE_HUGE) != 0);
  if (!rc) {
    nmg::placement_blocks_host(g, map, res->cells, res->nb_cells, res->nb_entries, rows);
    rc = nmg::write_blocks(sites, rows.data(), (int64_t)(rows.size() / 5), opts, err);
  }
  return said("nmg_report_placement", rc, err);
}

// Internal (not in include/numamma_gpu.h; tools/placement_timing.py and the
// tests): nmg_get_object_blocks' rows computed on the host from res->cells,
// what a caller without the device path does after nmg_get_page_cells.
// Returns the number of rows; the first min(n, cap) are written.
extern "C" int64_t nmg_debug_object_blocks_host(const nmg_host_results* res, const nmg_placement_options* p,
                                                uint64_t* rows, int64_t cap) {
  nmg::PlaceMap map;
  std::vector<uint64_t> npages;
  std::vector<uint8_t> dense;
  if (!placement_host_args(res, p, map, npages, dense) || cap < 0 || (cap && !rows)) return NMG_ERR_INVALID;
  nmg::PlaceGroups g;
  nmg::placement_object_groups(res->nb_entries, npages.data(), dense.data(), g, (p->source & NMG_PLACE_HUGE) != 0);
  std::vector<uint64_t> out;
  nmg::placement_blocks_host(g, map, res->cells, res->nb_cells, res->nb_entries, out);
  const int64_t n = (int64_t)(out.size() / 5);
  if (std::min(n, cap)) memcpy(rows, out.data(), (size_t)std::min(n, cap) * 40);
  return n;
}

extern "C" int nmg_report_host(const nmg_host_results* res, const nmg_object_meta* meta,
                               const nmg_report_options* opts, const char* stdout_path) {
  if (!registry_args(res, meta) || (res->nb_buffers && (!res->buf_samples || !res->buf_found || !res->buf_bytes)) ||
      !cells_args(res))
    return NMG_ERR_INVALID;
  std::string err;
  return said("nmg_report", nmg::write_report(res, meta, opts, stdout_path, err), err);
}

