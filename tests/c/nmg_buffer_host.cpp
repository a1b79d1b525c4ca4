// Host test of numamma_amd/csrc/nmg_buffer.h (tests/test_buffer_host.py): the
// four HIP allocation functions are defined here over malloc, counting live
// blocks and able to make the k-th allocation fail, so DevBuf / PinBuf run
// without a GPU, under the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>

#include "nmg_buffer.h"

static std::set<void*> g_live;
static int g_allocs = 0, g_frees = 0;
static int g_fail_in = 0;  // > 0: the g_fail_in-th allocation from now fails
static unsigned g_last_flags = 0;
static size_t g_last_bytes = 0;

static hipError_t stub_alloc(void** p, size_t bytes) {
  if (g_fail_in > 0 && --g_fail_in == 0) {
    *p = nullptr;
    return hipErrorOutOfMemory;
  }
  *p = malloc(bytes ? bytes : 1);
  g_live.insert(*p);
  g_allocs++;
  g_last_bytes = bytes;
  return hipSuccess;
}

static hipError_t stub_free(void* p) {
  if (!p) return hipSuccess;
  if (!g_live.erase(p)) {
    fprintf(stderr, "free of a block that is not live: %p\n", p);
    abort();
  }
  g_frees++;
  free(p);
  return hipSuccess;
}

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) { return stub_alloc(p, bytes); }
hipError_t hipFree(void* p) { return stub_free(p); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int flags) {
  g_last_flags = flags;
  return stub_alloc(p, bytes);
}
hipError_t hipHostFree(void* p) { return stub_free(p); }
}

#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                      \
    }                                                               \
  } while (0)

using nmg::DevBuf;
using nmg::PinBuf;
using nmg::PinMem;

template <class Buf>
static void exercise(Buf made_empty) {
  const int a0 = g_allocs, f0 = g_frees;
  const size_t live0 = g_live.size();
  {
    Buf b = std::move(made_empty);
    CHECK(b.get() == nullptr && b.cap() == 0);
    b.reset();  // (an empty buffer: nothing to free)
    CHECK(g_frees == f0);

    // reserve: one allocation when n > cap, none when n <= cap
    CHECK(b.reserve(100) == hipSuccess);
    CHECK(b.get() != nullptr && b.cap() == 100 && g_allocs == a0 + 1 && g_frees == f0);
    CHECK(g_last_bytes == 100 * sizeof(*b.get()));
    auto* p100 = b.get();
    b[0] = 1;  // (the implicit conversion to T*)
    b[99] = 2;
    CHECK(b.reserve(100) == hipSuccess && b.reserve(7) == hipSuccess && b.reserve(0) == hipSuccess);
    CHECK(b.get() == p100 && b.cap() == 100 && g_allocs == a0 + 1 && g_frees == f0);
    CHECK(b.reserve(101) == hipSuccess);
    CHECK(b.cap() == 101 && g_allocs == a0 + 2 && g_frees == f0 + 1 && !g_live.count(p100));
    CHECK(g_live.size() == live0 + 1);

    // alloc: always anew, exactly n, the old block freed once
    CHECK(b.alloc(5) == hipSuccess);
    CHECK(b.cap() == 5 && g_allocs == a0 + 3 && g_frees == f0 + 2 && g_live.size() == live0 + 1);

    // a failed reserve / alloc: empty, the old block freed once
    g_fail_in = 1;
    CHECK(b.reserve(1000) == hipErrorOutOfMemory);
    CHECK(b.get() == nullptr && b.cap() == 0 && g_frees == f0 + 3 && g_live.size() == live0);
    CHECK(b.reserve(1) == hipSuccess && b.get() != nullptr && b.cap() == 1);  // (the next call grows again)
    g_fail_in = 1;
    CHECK(b.alloc(1) == hipErrorOutOfMemory);
    CHECK(b.get() == nullptr && b.cap() == 0 && g_frees == f0 + 4 && g_live.size() == live0);
    g_fail_in = 1;
    CHECK(b.alloc(3) == hipErrorOutOfMemory);  // (failing while empty: nothing freed)
    CHECK(b.get() == nullptr && b.cap() == 0 && g_frees == f0 + 4);

    // alloc(0): a pointer all the same
    CHECK(b.alloc(0) == hipSuccess);
    CHECK(b.get() != nullptr && b.cap() == 0 && g_last_bytes > 0 && g_live.size() == live0 + 1);
    CHECK(b.reserve(0) == hipSuccess && g_live.size() == live0 + 1);

    // move construction: the source is left empty, nothing allocated or freed
    CHECK(b.alloc(8) == hipSuccess);
    auto* p8 = b.get();
    const int a1 = g_allocs, f1 = g_frees;
    Buf c(std::move(b));
    CHECK(c.get() == p8 && c.cap() == 8 && b.get() == nullptr && b.cap() == 0);
    CHECK(g_allocs == a1 && g_frees == f1);

    // move assignment: the destination's block freed once, the source left empty
    CHECK(b.alloc(4) == hipSuccess);
    auto* p4 = b.get();
    c = std::move(b);
    CHECK(c.get() == p4 && c.cap() == 4 && b.get() == nullptr && b.cap() == 0);
    CHECK(g_frees == f1 + 1 && !g_live.count(p8) && g_live.count(p4));
    Buf& self = c;
    c = std::move(self);  // (self-assignment keeps the block)
    CHECK(c.get() == p4 && g_live.count(p4));
    c = Buf();  // (how the engine releases a group)
    CHECK(c.get() == nullptr && c.cap() == 0 && g_frees == f1 + 2 && g_live.size() == live0);

    // the destructor frees
    CHECK(b.alloc(2) == hipSuccess && c.alloc(2) == hipSuccess);
    CHECK(g_live.size() == live0 + 2);
  }
  CHECK(g_live.size() == live0);
  CHECK(g_allocs - a0 == g_frees - f0);
}

int main() {
  exercise(DevBuf<unsigned>());
  exercise(DevBuf<unsigned long long>());
  exercise(PinBuf<unsigned char>());
  CHECK(g_last_flags == hipHostMallocDefault);
  exercise(PinBuf<unsigned>(PinMem::portable()));
  {  // the flags travel with the block
    PinBuf<unsigned> a(PinMem::portable()), b;
    CHECK(a.alloc(1) == hipSuccess && g_last_flags == hipHostMallocPortable);
    b = std::move(a);
    CHECK(b.reserve(2) == hipSuccess && g_last_flags == hipHostMallocPortable);
  }
  CHECK(g_live.empty());
  CHECK(g_allocs == g_frees);
  printf("nmg_buffer_host: ok (%d blocks)\n", g_allocs);
  return 0;
}
