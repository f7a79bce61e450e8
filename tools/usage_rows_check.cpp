// The host bookkeeping of the incremental usage updates (kwok_amd/csrc/usage_rows.hpp) on the CPU,
// for -fsanitize=address,undefined (tests/test_usage_rows.py builds and runs it):
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/usage_rows_check.cpp -o check
//   ./check [batches] [seed]
//
// A seeded sequence of batches over 300 pods (replacements, value edits, uniform <-> mixed,
// container-count changes, appended mixed entries, key sets that cross the 1-byte dictionary's
// 255 keys and come back) goes through Book::apply; the rows it returns run through
// usage_rows::write_row, the body of usage_rows_kernel itself, on host arrays.  After every batch:
//   * the book's columns are the model's, and everything derived from them is what a fresh
//     configure() + set_mixed() of those columns derives;
//   * the device arrays hold the book's keys and bases; live integrator ranges lie inside the
//     buffer and do not overlap; with the 1-byte column every pod's byte names its key;
//   * the integrators are what the model expects: kept where the pod goes on, 0 where it is new.
// Refused calls (a duplicate slot, a slot / id / mixed index out of range) change nothing.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "../kwok_amd/csrc/usage_rows.hpp"

using usage_rows::Book;
using usage_rows::DevRow;
using usage_rows::Effects;

static int g_fail = 0;
#define CHECK(c, ...)                                                         \
  do {                                                                        \
    if (!(c)) {                                                               \
      std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c);                 \
      std::printf(__VA_ARGS__);                                               \
      std::printf("\n");                                                      \
      if (++g_fail > 20) std::exit(1);                                        \
    }                                                                         \
  } while (0)

struct Device {  // the columns usage_rows_kernel writes; the rows run through its own body (usage_rows::write_row)
  std::vector<uint32_t> ukey, mbase;
  std::vector<uint8_t> ukey8;
  bool has8 = false;
  std::vector<double> ccum, unit;  // {cpu, mem} pairs: the second the negative of the first here
  std::vector<int64_t> last, created;
  void run(const std::vector<DevRow>& rows, uint64_t ccum_end) {
    const usage_rows::RowTargets a{ukey.data(), has8 ? ukey8.data() : nullptr, mbase.data(), last.data(), unit.data(), nullptr,
                                   ccum.data(), nullptr, created.data()};
    for (const DevRow& r : rows) {
      CHECK(r.slot < ukey.size(), "row slot %u", r.slot);
      if (r.flags & usage_rows::kDevRange) {
        CHECK((uint64_t)r.mbase + r.range_n <= ccum_end && 2 * ccum_end <= ccum.size(), "range %u + %u", r.mbase, r.range_n);
        CHECK(r.copy_n <= r.range_n && ((r.flags & usage_rows::kDevSeedUnit) || (uint64_t)r.copy_from + r.copy_n <= ccum_end), "copy");
      }
      if (r.slot < ukey.size()) usage_rows::write_row(r, a);
    }
  }
};

// the dictionary's values after the largest container count shrank and a constant was appended:
// podv has fewer rows then, and the entry of the key that went away must not be read through
static void check_kv_after_shrink() {
  auto key = [](uint32_t c, uint32_t m, uint32_t nc) { return c | (m << 14) | (nc << 28); };
  for (uint32_t big : {3u, 15u}) {
    const std::vector<uint32_t> k = {key(0, 0, 1), key(1, 0, big), key(0, 0, 1)};
    Book b;
    std::vector<uint8_t> k8;
    b.configure(k.data(), 3, 2, 0, 1, 0, &k8);
    CHECK(b.key8 && b.max_nc() == big && b.dict.size() == 2, "configured");
    const kwk_usage_row row{1, key(1, 0, 1), 0, 0, 0};
    std::vector<DevRow> out;
    Effects fx;
    CHECK(b.apply(&row, 1, out, fx).empty() && b.max_nc() == 1 && b.dict_live() == 2, "the %u-container key went away", big);
    b.n_cpu = 3;  // kwk_usage_append of one constant: podv is rebuilt for the new width, 2 rows of 4
    std::vector<double> podv(b.podv_entries());
    for (size_t i = 0; i < podv.size(); ++i) podv[i] = 100.0 + (double)i;
    podv.shrink_to_fit();
    CHECK(podv.size() == 8, "podv entries %zu", podv.size());
    std::vector<double> kv(2 * b.dict.size(), -1.0);
    b.fill_kv(podv, kv.data());
    for (size_t d = 0; d < b.dict.size(); ++d) {
      size_t c = 0, m = 0;
      if (b.dict[d]) b.kv_at(b.dict[d], c, m);
      CHECK(kv[2 * d] == (b.dict[d] ? podv.at(c) : 0.0) && kv[2 * d + 1] == (b.dict[d] ? podv.at(m) : 0.0), "kv entry %zu", d);
    }
    size_t live = 0;
    for (uint32_t x : b.dict) live += x != 0;
    CHECK(live == b.dict_live(), "free entries are marked");
  }
}

// configure()'s counting (a short list, then the map past 256 distinct keys) and build_dict()
// against a plain map, around the dictionary's 255 keys
static void check_configure(uint32_t seed) {
  std::mt19937 rng(seed);
  for (uint32_t distinct : {1u, 2u, 85u, 86u, 256u, 257u, 300u, 5000u}) {
    std::vector<uint32_t> k(60000);
    std::map<uint32_t, uint64_t> want;
    for (uint32_t& x : k) {
      x = ((1u + rng() % 3) << 28) | (rng() % distinct);
      ++want[x];
    }
    Book b;
    std::vector<uint8_t> k8c;  // the column out of configure()'s own pass
    b.configure(k.data(), (uint32_t)k.size(), 16384, 0, 1, 0, &k8c);
    CHECK(b.key8 == (want.size() <= usage_rows::kDictMax), "%u values: configure's column for %zu keys", distinct, want.size());
    if (b.key8)
      for (size_t p = 0; p < k.size(); ++p) CHECK(b.dict[k8c[p]] == k[p], "%u values: pod %zu (configure)", distinct, p);
    CHECK(b.keys.size() == want.size(), "%u values: %zu keys, expected %zu", distinct, b.keys.size(), want.size());
    for (const auto& w : want) {
      const auto it = b.keys.find(w.first);
      CHECK(it != b.keys.end() && it->second.count == w.second, "%u values: key %u count", distinct, w.first);
    }
    std::vector<uint8_t> k8;
    const bool fits = b.build_dict(k8);
    CHECK(fits == (want.size() <= usage_rows::kDictMax), "%u values: the 1-byte column for %zu keys", distinct, want.size());
    if (fits)
      for (size_t p = 0; p < k.size(); ++p) CHECK(b.dict[k8[p]] == k[p], "%u values: pod %zu", distinct, p);
  }
}

int main(int argc, char** argv) {
  const int batches = argc > 1 ? std::atoi(argv[1]) : 20;
  const uint32_t seed = argc > 2 ? (uint32_t)std::strtoul(argv[2], nullptr, 10) : 1u;
  check_configure(seed);
  check_kv_after_shrink();
  std::mt19937 rng(seed);
  auto rnd = [&](uint32_t n) { return (uint32_t)(rng() % n); };
  const uint32_t n_pods = 300, n_cpu = 24, n_mem = 24;
  auto ukey_of = [](uint32_t c, uint32_t m, uint32_t nc) { return c | (m << 14) | (nc << 28); };

  // the initial configuration: a handful of keys, a few mixed pods
  std::vector<uint32_t> mixed = {0, 2, 2, 3}, ckeys = {ukey_of(1, 1, 0), ukey_of(2, 0, 0), ukey_of(0, 0, 0), ukey_of(3, 3, 0), ukey_of(1, 2, 0)};
  std::vector<uint32_t> model(n_pods);
  for (uint32_t p = 0; p < n_pods; ++p) model[p] = p % 37 == 5 ? rnd(2) : ukey_of(rnd(3), rnd(2), 1 + rnd(2));
  Book b;
  b.configure(model.data(), n_pods, n_cpu, 0, n_mem, 0);
  CHECK(b.set_mixed(mixed.data(), 2, ckeys.data(), (uint32_t)ckeys.size()).empty(), "set_mixed");
  Device dev;
  dev.ukey = model;
  dev.mbase = b.mbase;
  dev.ukey8.assign(n_pods, 0);
  dev.ccum.assign(2 * b.ccum_end, 0.0);
  dev.unit.assign(2 * (size_t)n_pods, 0.0);
  dev.last.assign(n_pods, 0);
  dev.created.assign(n_pods, 0);
  // expected integrators: per pod, its containers' (mixed) or its unit's (uniform)
  std::vector<std::vector<double>> want(n_pods);
  for (uint32_t p = 0; p < n_pods; ++p) want[p].assign((model[p] >> 28) ? 1 : b.containers(p), 0.0);

  uint64_t n_rows = 0, n_refused = 0, n_dict_rebuilds = 0, n_dict_drops = 0, n_new_ranges = 0, n_reused = 0;
  std::vector<DevRow> out;
  Effects fx;
  for (int t = 0; t < batches; ++t) {
    // grow the mixed tables now and then (entries of 0..6 containers)
    if (t % 3 == 1) {
      std::vector<uint32_t> m, ck;
      for (uint32_t i = 0, n = 1 + rnd(3); i < n; ++i) {
        const uint32_t cnt = rnd(7);
        m.push_back((uint32_t)(b.ckeys.size() + ck.size()));
        m.push_back(cnt);
        for (uint32_t c = 0; c < cnt; ++c) ck.push_back(ukey_of(rnd(n_cpu), rnd(n_mem), 0));
      }
      CHECK(b.mixed_append(m.data(), (uint32_t)m.size() / 2, ck.data(), (uint32_t)ck.size()).empty(), "mixed_append");
      std::vector<uint32_t> far = {(uint32_t)b.ckeys.size(), 1};
      CHECK(!b.mixed_append(far.data(), 1, nullptr, 0).empty(), "an entry beyond ckeys must be refused");
    }
    // phases: few keys / many keys (past the dictionary) / few keys again, mixed pods in some
    const bool many = t % 10 >= 4 && t % 10 <= 6, allow_mixed = t % 5 != 3 && t % 5 != 4;
    const uint32_t n = many || t % 10 == 7 ? 200 + rnd(100) : 1 + rnd(80);
    std::vector<uint32_t> slots(n_pods);
    for (uint32_t p = 0; p < n_pods; ++p) slots[p] = p;
    for (uint32_t i = 0; i < n; ++i) std::swap(slots[i], slots[i + rnd(n_pods - i)]);
    std::vector<kwk_usage_row> rows(n);
    for (uint32_t i = 0; i < n; ++i) {
      kwk_usage_row r{};
      r.slot = slots[i];
      if (allow_mixed && rnd(6) == 0) r.usage_key = rnd(b.n_mixed());
      else if (many) r.usage_key = ukey_of(rnd(n_cpu), rnd(n_mem), 1 + rnd(4));
      else r.usage_key = ukey_of(rnd(3), rnd(2), 1 + rnd(2));
      if (rnd(2)) r.flags |= KWK_USAGE_ROW_RESET;
      if (rnd(3) == 0) r.flags |= KWK_USAGE_ROW_CREATED, r.created_ns = (int64_t)t * 1000 + i;
      rows[i] = r;
    }
    if (!allow_mixed)  // every mixed pod turns uniform: the fast path and the dictionary can come back
      for (uint32_t p = 0; p < n_pods; ++p)
        if (!(b.ukey[p] >> 28)) {
          bool named = false;
          for (const kwk_usage_row& r : rows) named = named || r.slot == p;
          if (!named) rows.push_back(kwk_usage_row{p, ukey_of(1, 1, 1), 0, 0, 0});
        }
    // refusals first: each leaves the book as it is
    {
      const Book before = b;
      std::vector<kwk_usage_row> bad = rows;
      bad.push_back(rows[rnd((uint32_t)rows.size())]);
      CHECK(b.apply(bad.data(), (uint32_t)bad.size(), out, fx).find("named twice") != std::string::npos, "duplicate");
      bad = rows;
      bad[0].slot = n_pods + rnd(3);
      CHECK(b.apply(bad.data(), (uint32_t)bad.size(), out, fx).find("beyond") != std::string::npos, "slot");
      bad = rows;
      bad.back().usage_key = ukey_of(b.n_cpu, 0, 1);
      CHECK(b.apply(bad.data(), (uint32_t)bad.size(), out, fx).find("value id") != std::string::npos, "id");
      bad = rows;
      bad.back().usage_key = b.n_mixed();
      CHECK(b.apply(bad.data(), (uint32_t)bad.size(), out, fx).find("mixed index") != std::string::npos, "mixed index");
      n_refused += 4;
      CHECK(b.ukey == before.ukey && b.mbase == before.mbase && b.mcap == before.mcap && b.ccum_end == before.ccum_end &&
                b.keys.size() == before.keys.size() && b.dict == before.dict && b.key8 == before.key8 &&
                b.n_mixed_pods == before.n_mixed_pods,
            "a refused call changed the book");
    }
    // the model: keys, and what the integrators become
    for (const kwk_usage_row& r : rows) {
      const uint32_t ko = model[r.slot], kn = r.usage_key;
      const bool reset = r.flags & KWK_USAGE_ROW_RESET, was_mixed = !(ko >> 28), is_mixed = !(kn >> 28);
      std::vector<double> w((kn >> 28) ? 1 : b.key_containers(kn), 0.0);
      if (!reset && was_mixed == is_mixed)
        for (size_t j = 0; j < w.size() && j < want[r.slot].size(); ++j) w[j] = want[r.slot][j];
      if (!reset && !was_mixed && is_mixed)  // the containers shared the unit's total
        for (size_t j = 0; j < w.size() && j < (ko >> 28); ++j) w[j] = want[r.slot][0];
      want[r.slot] = w;
      model[r.slot] = kn;
    }
    const uint64_t end0 = b.ccum_end;
    const std::string err = b.apply(rows.data(), (uint32_t)rows.size(), out, fx);
    CHECK(err.empty(), "%s", err.c_str());
    n_rows += rows.size();
    n_new_ranges += b.ccum_end != end0;
    for (const DevRow& r : out) n_reused += (r.flags & usage_rows::kDevMbase) && r.mbase < end0;
    if (fx.key8_dropped) dev.has8 = false, ++n_dict_drops;
    if (dev.ccum.size() < 2 * b.ccum_end) dev.ccum.resize(std::max<size_t>(2 * b.ccum_end, 2 * dev.ccum.size()), -1.0);
    dev.run(out, b.ccum_end);
    if (!b.key8 && !b.has_mixed() && b.keys.size() <= usage_rows::kDictMax) {  // as the engine rebuilds the column
      CHECK(b.build_dict(dev.ukey8), "build_dict");
      dev.has8 = true;
      ++n_dict_rebuilds;
    }
    // against the model and a fresh book of the same columns
    CHECK(b.ukey == model && dev.ukey == model, "keys (batch %d)", t);
    Book f;
    f.configure(model.data(), n_pods, n_cpu, 0, n_mem, 0);
    CHECK(f.set_mixed(b.mixed.data(), b.n_mixed(), b.ckeys.data(), (uint32_t)b.ckeys.size()).empty(), "fresh set_mixed");
    CHECK(f.n_mixed_pods == b.n_mixed_pods && f.max_nc() == b.max_nc() && f.keys.size() == b.keys.size(), "derived counts (batch %d)", t);
    for (int c = 0; c < 16; ++c) CHECK(f.nc_hist[c] == b.nc_hist[c], "containers histogram");
    for (const auto& kr : f.keys) {
      const auto it = b.keys.find(kr.first);
      CHECK(it != b.keys.end() && it->second.count == kr.second.count, "key %u count", kr.first);
    }
    std::vector<uint8_t> k8;
    CHECK(f.build_dict(k8) == b.key8, "the 1-byte column exists where a configuration builds it (batch %d)", t);
    if (b.key8) {
      if (t % 4 == 2) ++b.n_cpu;  // (an appended constant: the table's rows widen)
      std::vector<double> podv(b.podv_entries(), 1.0), kv(2 * b.dict.size());
      podv.shrink_to_fit();
      b.fill_kv(podv, kv.data());
      CHECK(b.dict_live() == b.keys.size(), "dictionary entries in use");
      for (uint32_t p = 0; p < n_pods; ++p)
        CHECK(dev.ukey8[p] < b.dict.size() && b.dict[dev.ukey8[p]] == model[p], "pod %u: byte %u", p, dev.ukey8[p]);
    }
    std::map<uint32_t, uint32_t> ranges;
    for (uint32_t p = 0; p < n_pods; ++p) {
      if (model[p] >> 28) continue;
      const uint32_t c = b.containers(p);
      CHECK(dev.mbase[p] == b.mbase[p] && b.mcap[p] >= c && (uint64_t)b.mbase[p] + c <= b.ccum_end, "pod %u range", p);
      if (c) ranges[b.mbase[p]] = c;
    }
    uint64_t prev_end = 0;
    for (const auto& r : ranges) {
      CHECK(r.first >= prev_end, "ranges overlap at %u", r.first);
      prev_end = (uint64_t)r.first + r.second;
    }
    // integrate once (every live integrator moves by a value of its own), then compare
    for (uint32_t p = 0; p < n_pods; ++p)
      for (size_t j = 0; j < want[p].size(); ++j) {
        const double x = 1.0 + p * 16 + j + t * 0.5;
        want[p][j] += x;
        double* at = (model[p] >> 28) ? &dev.unit.at(2 * (size_t)p) : &dev.ccum.at(2 * (size_t)(dev.mbase[p] + j));
        at[0] += x, at[1] -= x;
      }
    for (uint32_t p = 0; p < n_pods; ++p)
      for (size_t j = 0; j < want[p].size(); ++j) {
        const double* at = (model[p] >> 28) ? &dev.unit.at(2 * (size_t)p) : &dev.ccum.at(2 * (size_t)(dev.mbase[p] + j));
        const double got = at[0];
        CHECK(at[1] == -want[p][j], "pod %u container %zu: memory %g", p, j, at[1]);
        CHECK(got == want[p][j], "pod %u container %zu: %g, expected %g (batch %d)", p, j, got, want[p][j], t);
      }
  }
  std::printf("%d batches, %llu rows, %llu refused calls, %llu dictionary drops, %llu rebuilds, %llu batches with new ranges, "
              "%llu reused ranges, %d failures\n",
              batches, (unsigned long long)n_rows, (unsigned long long)n_refused, (unsigned long long)n_dict_drops,
              (unsigned long long)n_dict_rebuilds, (unsigned long long)n_new_ranges, (unsigned long long)n_reused, g_fail);
  return g_fail ? 1 : 0;
}
