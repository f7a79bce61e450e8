// The owners of kwok_amd/csrc/devmem.hpp on the CPU, without HIP: counting stand-ins for the HIP
// names the header uses (over malloc / free), then the owners' contract case by case and a seeded
// random sequence of operations against a reference model.  tests/test_devmem.py builds it with
// -fsanitize=address,undefined.
//   devmem_check [operations] [seed]
#include <cassert>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <vector>

// ---- the stand-ins
typedef int hipError_t;
constexpr hipError_t hipSuccess = 0, hipErrorOutOfMemory = 2;
typedef struct FakeEvent* hipEvent_t;
typedef struct FakeStream* hipStream_t;
enum hipMemcpyKind { hipMemcpyHostToDevice, hipMemcpyDeviceToHost };
constexpr unsigned hipHostMallocDefault = 0, hipEventDefault = 0, hipEventDisableTiming = 2;

static std::set<void*> g_dev, g_host, g_events;  // live
static long g_allocs = 0, g_frees = 0, g_bad_frees = 0, g_syncs = 0;
static long g_fail_at = -1;  // the allocation (device or host, counted from 0 at arming) that fails

static bool fail_now() { return g_fail_at >= 0 && g_fail_at-- == 0; }
static void fail_kth(long k) { g_fail_at = k; }

static hipError_t fake_alloc(std::set<void*>& live, void** p, size_t bytes) {
  *p = nullptr;
  if (fail_now()) return hipErrorOutOfMemory;
  if (bytes == 0) return hipSuccess;  // (as hipMalloc: a null pointer)
  *p = malloc(bytes);
  live.insert(*p);
  ++g_allocs;
  return hipSuccess;
}
static hipError_t fake_free(std::set<void*>& live, void* p) {
  if (!p) return hipSuccess;
  if (!live.erase(p)) {  // not live: a double free, or a block of the other kind
    ++g_bad_frees;
    return hipErrorOutOfMemory;
  }
  ++g_frees;
  free(p);
  return hipSuccess;
}
hipError_t hipMalloc(void** p, size_t bytes) { return fake_alloc(g_dev, p, bytes); }
hipError_t hipFree(void* p) { return fake_free(g_dev, p); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { return fake_alloc(g_host, p, bytes); }
hipError_t hipHostFree(void* p) { return fake_free(g_host, p); }
hipError_t hipEventCreateWithFlags(hipEvent_t* ev, unsigned) {
  *ev = static_cast<hipEvent_t>(malloc(1));
  g_events.insert(*ev);
  return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t ev) {
  if (!g_events.erase(ev)) {
    ++g_bad_frees;
    return hipErrorOutOfMemory;
  }
  free(ev);
  return hipSuccess;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind, hipStream_t) {
  memcpy(dst, src, bytes);
  return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) {
  ++g_syncs;
  return hipSuccess;
}

#include "../kwok_amd/csrc/devmem.hpp"

#define CHECK(c)                                                    \
  do {                                                              \
    if (!(c)) {                                                     \
      fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                      \
    }                                                               \
  } while (0)

struct Slot {  // a struct that holds owners, as the engines' ring slots and output sets do
  DevBuf<void> list;
  DevBuf<uint32_t> offsets;
  HostBuf<char> stage;
  Event ev;
  int tag = 0;
};

template <class B>
static void owner_cases(std::set<void*>& live) {
  const size_t base = live.size();
  {
    B b;  // fresh: empty, reset a no-op
    CHECK(!b && b.get() == nullptr && b.size() == 0);
    const long f0 = g_frees;
    b.reset();
    CHECK(g_frees == f0 && live.size() == base);
    // alloc, alloc: the first block freed exactly once
    CHECK(b.alloc(10) == hipSuccess && b.size() == 10 && b.get() && live.size() == base + 1);
    CHECK(b.alloc(20) == hipSuccess && b.size() == 20 && g_frees == f0 + 1 && live.size() == base + 1);
    // a failing alloc: empty, the earlier block freed
    void* second = b.get();
    fail_kth(0);
    CHECK(b.alloc(30) != hipSuccess && !b && b.size() == 0 && live.size() == base && !live.count(second));
    CHECK(b.alloc(8) == hipSuccess);
    // grow at or below the size: nothing allocated, the pointer kept
    void* p = b.get();
    const long a0 = g_allocs;
    CHECK(b.grow(8) == hipSuccess && b.grow(3) == hipSuccess && b.grow(0) == hipSuccess);
    CHECK(b.get() == p && b.size() == 8 && g_allocs == a0);
    // grow above: the block replaced
    const long f2 = g_frees;
    CHECK(b.grow(9) == hipSuccess && b.size() == 9 && g_allocs == a0 + 1 && g_frees == f2 + 1 && live.size() == base + 1);
    fail_kth(0);  // a failing grow leaves it empty too
    CHECK(b.grow(100) != hipSuccess && !b && b.size() == 0 && live.size() == base);
    CHECK(b.alloc(4) == hipSuccess);
    // move construction, move assignment, self-move-assignment, swap
    p = b.get();
    B c(std::move(b));
    CHECK(!b && b.size() == 0 && c.get() == p && c.size() == 4 && live.size() == base + 1);
    B d;
    CHECK(d.alloc(6) == hipSuccess);
    void* dp = d.get();
    d = std::move(c);  // d's block is freed
    CHECK(!c && d.get() == p && d.size() == 4 && !live.count(dp) && live.size() == base + 1);
    B& self = d;
    d = std::move(self);
    CHECK(d.get() == p && d.size() == 4 && live.size() == base + 1);
    B e;
    std::swap(d, e);
    CHECK(!d && d.size() == 0 && e.get() == p && e.size() == 4);
    CHECK(d.alloc(2) == hipSuccess);
    dp = d.get();
    std::swap(d, e);
    CHECK(d.get() == p && d.size() == 4 && e.get() == dp && e.size() == 2 && live.size() == base + 2);
    // release: emptied without freeing
    const long f1 = g_frees;
    auto* raw = d.release();
    CHECK(raw == p && !d && d.size() == 0 && g_frees == f1 && live.count(p));
    CHECK(fake_free(live, raw) == hipSuccess);
    // the conversion: pointer arithmetic and kernel-argument style reads
    auto* q = e.get();
    CHECK(static_cast<decltype(q)>(e) == q && (e ? 1 : 0) == 1);
  }
  CHECK(live.size() == base);  // the destructors freed the rest
}

static void event_cases() {
  {
    Event ev;
    CHECK(!ev.get() && g_events.empty());
    ev.reset();
    CHECK(ev.create(hipEventDisableTiming) == hipSuccess && ev.get() && g_events.size() == 1);
    hipEvent_t h = ev;
    CHECK(ev.create(hipEventDefault) == hipSuccess && ev.get() == h && g_events.size() == 1);  // exists: a no-op
    Event b(std::move(ev));
    CHECK(!ev.get() && b.get() == h);
    Event c;
    CHECK(c.create(hipEventDefault) == hipSuccess && g_events.size() == 2);
    c = std::move(b);
    CHECK(c.get() == h && g_events.size() == 1);
    Event& self = c;
    c = std::move(self);
    CHECK(c.get() == h && g_events.size() == 1);
    std::swap(b, c);
    CHECK(b.get() == h && !c.get());
  }
  CHECK(g_events.empty());
}

static void vector_cases() {
  {
    std::vector<Slot> v(2);
    for (size_t i = 0; i < v.size(); ++i) {
      CHECK(v[i].list.alloc(64) == hipSuccess && v[i].offsets.alloc(4) == hipSuccess && v[i].stage.alloc(16) == hipSuccess &&
            v[i].ev.create(hipEventDefault) == hipSuccess);
      v[i].tag = (int)i;
    }
    void* l1 = v[1].list.get();
    v.resize(40);  // reallocates: the slots move
    CHECK(v[1].list.get() == l1 && v[1].tag == 1 && !v[39].list && g_dev.size() == 4 && g_host.size() == 2 && g_events.size() == 2);
    CHECK(v[39].list.alloc(8) == hipSuccess);
    v.resize(3);  // slot 39 frees its list
    CHECK(g_dev.size() == 4);
    v.erase(v.begin());  // slot 0 goes, the others move down
    CHECK(v.size() == 2 && v[0].list.get() == l1 && v[0].tag == 1 && g_dev.size() == 2 && g_host.size() == 1 && g_events.size() == 1);
    Slot cur = std::move(v[0]);  // the ring rebuild of kwk_fired_keep
    v.clear();
    v.resize(4);
    v[0] = std::move(cur);
    CHECK(v[0].list.get() == l1 && g_dev.size() == 2 && g_events.size() == 1);
  }
  CHECK(g_dev.empty() && g_host.empty() && g_events.empty());
}

static void copy_cases() {
  DevBuf<uint32_t> d;
  CHECK(d.alloc(4) == hipSuccess);
  const uint32_t in[4] = {1, 2, 3, 4};
  uint32_t out[4] = {};
  const long s0 = g_syncs;
  CHECK(copy_in(nullptr, d, in, sizeof in) == hipSuccess && copy_out(nullptr, out, d, sizeof out) == hipSuccess);
  CHECK(memcmp(in, out, sizeof in) == 0 && g_syncs == s0 + 2);
  CHECK(copy_in(nullptr, d, in, 0) == hipSuccess && g_syncs == s0 + 2);  // nothing to copy: nothing enqueued
}

// a seeded random sequence over eight owners, every operation mirrored in a model
static void model_run(long ops, uint64_t seed) {
  struct Held { void* p; size_t n; };
  {
    DevBuf<uint64_t> own[8];
    std::map<int, Held> model;  // owner index -> what it holds (absent: empty)
    std::vector<void*> released;
    std::mt19937_64 rng(seed);
    auto mirror_alloc = [&](int i, size_t n, bool failed) {
      model.erase(i);
      if (!failed && n) model[i] = Held{own[i].get(), n};
      if (!failed && !n) CHECK(!own[i]);
    };
    for (long k = 0; k < ops; ++k) {
      const int i = (int)(rng() % 8), j = (int)(rng() % 8);
      const size_t n = (size_t)(rng() % 40);
      const bool failing = rng() % 16 == 0;
      switch (rng() % 6) {
        case 0: {  // alloc
          if (failing) fail_kth(0);
          const bool failed = own[i].alloc(n) != hipSuccess;
          g_fail_at = -1;
          CHECK(failed == failing);
          mirror_alloc(i, n, failed);
          break;
        }
        case 1: {  // grow
          const bool grows = n > (model.count(i) ? model[i].n : 0);
          if (failing) fail_kth(0);
          const bool failed = own[i].grow(n) != hipSuccess;
          g_fail_at = -1;
          CHECK(failed == (failing && grows));
          if (grows) mirror_alloc(i, n, failed);
          break;
        }
        case 2: {  // move (onto itself: nothing changes)
          own[i] = std::move(own[j]);
          if (i != j) {
            model.erase(i);
            if (model.count(j)) model[i] = model[j];
            model.erase(j);
          }
          break;
        }
        case 3: {  // swap
          std::swap(own[i], own[j]);
          const bool hi = model.count(i), hj = model.count(j);
          const Held a = hi ? model[i] : Held{}, b = hj ? model[j] : Held{};
          model.erase(i);
          model.erase(j);
          if (i == j) { if (hi) model[i] = a; break; }
          if (hj) model[i] = b;
          if (hi) model[j] = a;
          break;
        }
        case 4: {  // release
          void* p = own[i].release();
          CHECK(p == (model.count(i) ? model[i].p : nullptr));
          if (p) released.push_back(p);
          model.erase(i);
          break;
        }
        default:  // reset
          own[i].reset();
          model.erase(i);
      }
      for (int o = 0; o < 8; ++o) {
        const bool held = model.count(o);
        CHECK(own[o].get() == (held ? model[o].p : nullptr) && own[o].size() == (held ? model[o].n : 0));
      }
      CHECK(g_dev.size() == model.size() + released.size());
      CHECK(g_bad_frees == 0);
    }
    for (void* p : released) CHECK(hipFree(p) == hipSuccess);
  }
  CHECK(g_dev.empty());
}

int main(int argc, char** argv) {
  const long ops = argc > 1 ? atol(argv[1]) : 10000;
  const uint64_t seed = argc > 2 ? strtoull(argv[2], nullptr, 10) : 20261;
  owner_cases<DevBuf<uint32_t>>(g_dev);
  owner_cases<DevBuf<void>>(g_dev);
  owner_cases<HostBuf<char>>(g_host);
  CHECK(g_host.empty() && g_dev.empty());
  event_cases();
  vector_cases();
  copy_cases();
  model_run(ops, seed);
  CHECK(g_dev.empty() && g_host.empty() && g_events.empty());
  CHECK(g_bad_frees == 0 && g_allocs == g_frees);
  printf("%ld operations, %ld blocks allocated and freed, 0 live, 0 bad frees\n", ops, g_allocs);
  return 0;
}
