// kwk_relayout's host side on the CPU (kwok_amd/csrc/relayout.hpp, usage_rows.hpp Book::relayout),
// for -fsanitize=address,undefined (tests/test_relayout.py builds and runs it):
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/relayout_check.cpp -o check
//   ./check [rounds] [seed]
//
//   * relayout::gather_chunk, the body of relayout_gather_kernel itself, over host columns of 1, 2,
//     4, 8, 16 and 32-byte elements against a naive per-element loop: fixed run lists (identity
//     runs, a run of one slot, src and dst that differ modulo 4 and modulo 16, a fresh hole between
//     runs, n_active shrinking and growing, an empty list) and seeded random ones, with the whole
//     list and with the slice a workgroup would stage;
//   * Book::relayout against configure() + set_mixed() of the permuted columns: the counts, the
//     containers histogram, the dictionary's live set and every pod's entry, the 1-byte column kept
//     below and dropped at the 256th distinct key, mixed pods moved and dropped;
//   * relayout::check_layout: every refusal names what it refuses, and a refused layout leaves the
//     book as it was.
// The columns are allocated at exactly the bytes the header promises to touch, so a read or a
// write past them is the sanitizer's finding.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "../kwok_amd/csrc/relayout.hpp"
#include "../kwok_amd/csrc/usage_rows.hpp"

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

using Moves = std::vector<kwk_move>;

// a column of n elements, 16-byte aligned and exactly as long as its whole chunks
struct Column {
  unsigned char* p = nullptr;
  size_t bytes = 0;
  Column(uint64_t n, uint32_t eb) : bytes(16 * (size_t)relayout::chunks_of(n, eb)) {
    p = static_cast<unsigned char*>(std::aligned_alloc(16, bytes ? bytes : 16));
    std::memset(p, 0xEE, bytes ? bytes : 16);
  }
  ~Column() { std::free(p); }
  Column(const Column&) = delete;
  Column& operator=(const Column&) = delete;
};

template <uint32_t EB>
static void gather_case(const char* name, const Moves& mv, uint32_t n_old, uint32_t n_new, uint32_t seed) {
  CHECK(relayout::check_moves(mv.data(), (uint32_t)mv.size(), n_old, n_new, "run").empty(), "%s: the case's own runs", name);
  Column src(n_old, EB), dst(n_new, EB);
  std::mt19937 rng(seed);
  for (size_t i = 0; i < (size_t)n_old * EB; ++i) src.p[i] = (unsigned char)rng();
  unsigned char fill_elem[32];
  for (unsigned char& b : fill_elem) b = (unsigned char)(0xA0u + (rng() & 15u));
  const relayout::Fill fill = relayout::fill_of(fill_elem, EB);
  // the naive loop
  std::vector<unsigned char> want(dst.bytes);
  for (size_t i = 0; i < dst.bytes; ++i) want[i] = fill_elem[i % EB];
  for (const kwk_move& m : mv)
    for (uint32_t i = 0; i < m.n; ++i) std::memcpy(&want[(size_t)(m.dst + i) * EB], src.p + (size_t)(m.src + i) * EB, EB);
  const uint64_t chunks = relayout::chunks_of(n_new, EB);
  for (int sliced = 0; sliced < 2; ++sliced) {
    std::memset(dst.p, 0x55, dst.bytes ? dst.bytes : 16);
    const uint64_t span = 24;  // chunks per "workgroup" of the sliced pass
    for (uint64_t c = 0; c < chunks; ++c) {
      const kwk_move* runs = mv.data();
      uint32_t n_runs = (uint32_t)mv.size();
      if (sliced) {  // the slice relayout_gather_kernel stages for the span that holds chunk c
        const uint64_t base = c / span * span, last = std::min(base + span, chunks);
        const uint32_t r0 = relayout::find_run(mv.data(), (uint32_t)mv.size(), (uint32_t)(base * 16 / EB));
        const uint32_t r1 = relayout::first_run_from(mv.data(), (uint32_t)mv.size(), (uint32_t)((last * 16 + EB - 1) / EB));
        runs = mv.data() + r0;
        n_runs = r1 > r0 ? r1 - r0 : 0;
      }
      const relayout::V16 v = relayout::gather_chunk<EB>(src.p, c, runs, n_runs, fill);
      std::memcpy(dst.p + 16 * c, &v, 16);
    }
    const bool same = dst.bytes == 0 || std::memcmp(dst.p, want.data(), dst.bytes) == 0;
    if (!same) {
      size_t at = 0;
      while (dst.p[at] == want[at]) ++at;
      CHECK(same, "%s: %u-byte elements, %s list: byte %zu (slot %zu) is %02x, the naive loop has %02x", name, EB,
            sliced ? "sliced" : "whole", at, at / EB, dst.p[at], want[at]);
    }
  }
}

static void gather_all(const char* name, const Moves& mv, uint32_t n_old, uint32_t n_new, uint32_t seed) {
  gather_case<1>(name, mv, n_old, n_new, seed);
  gather_case<2>(name, mv, n_old, n_new, seed + 1);
  gather_case<4>(name, mv, n_old, n_new, seed + 2);
  gather_case<8>(name, mv, n_old, n_new, seed + 3);
  gather_case<16>(name, mv, n_old, n_new, seed + 4);
  gather_case<32>(name, mv, n_old, n_new, seed + 5);
}

// a random valid run list: pieces of the old slots, some dropped, kept in order or shuffled,
// laid into the new slots with holes; some pieces keep their place
static Moves random_moves(std::mt19937& rng, uint32_t n_old, uint32_t& n_new) {
  std::vector<kwk_move> pieces;
  for (uint32_t s = 0; s < n_old;) {
    const uint32_t len = std::min(n_old - s, 1u + (uint32_t)(rng() % (rng() % 4 ? 9 : 150)));
    if (rng() % 5) pieces.push_back({0, s, len});
    s += len;
  }
  if (rng() % 2) std::shuffle(pieces.begin(), pieces.end(), rng);
  uint32_t d = 0;
  for (kwk_move& m : pieces) {
    if (rng() % 3 == 0) d += rng() % 20;  // a fresh hole
    m.dst = d;
    d += m.n;
  }
  n_new = d + (rng() % 3 ? 0 : rng() % 40);
  return pieces;
}

static void check_gather(uint32_t rounds, uint32_t seed) {
  gather_all("empty list", {}, 100, 77, seed);
  gather_all("empty list, no slots", {}, 5, 0, seed);
  gather_all("identity", {{0, 0, 100}}, 100, 100, seed);
  gather_all("identity runs and growth", {{0, 0, 40}, {40, 40, 60}}, 100, 133, seed);
  gather_all("a run of length 1", {{3, 50, 1}}, 100, 20, seed);
  gather_all("shift by one", {{0, 0, 10}, {11, 10, 190}}, 200, 201, seed);            // src, dst differ by 1 modulo 4 and 16
  gather_all("shift by 4 and by 7", {{4, 0, 50}, {61, 50, 120}}, 200, 190, seed);      // ... by 4, then by 11
  gather_all("a fresh hole between runs", {{0, 0, 33}, {50, 33, 67}}, 100, 117, seed);
  gather_all("shrink", {{0, 10, 30}, {30, 70, 25}}, 100, 55, seed);
  gather_all("grow", {{0, 0, 100}}, 100, 300, seed);
  gather_all("reversed pieces", {{0, 80, 20}, {20, 60, 20}, {40, 40, 20}, {60, 20, 20}, {80, 0, 20}}, 100, 100, seed);
  gather_all("zero-length runs", {{0, 0, 0}, {0, 5, 10}, {10, 0, 0}, {10, 20, 3}}, 30, 16, seed);
  gather_all("the last source chunk", {{1, 83, 17}}, 100, 18, seed);                  // reads up to the old column's end
  std::mt19937 rng(seed);
  for (uint32_t r = 0; r < rounds; ++r) {
    const uint32_t n_old = 1 + rng() % 700;
    uint32_t n_new = 0;
    const Moves mv = random_moves(rng, n_old, n_new);
    gather_all("random", mv, n_old, n_new, (uint32_t)rng());
  }
  // identity_prefix: what stays where it is
  const Moves a = {{0, 0, 10}, {10, 10, 5}, {15, 16, 4}};
  CHECK(relayout::identity_prefix(a.data(), 3, 19) == 15, "prefix of two identity runs");
  const Moves b = {{0, 0, 10}, {11, 11, 5}};
  CHECK(relayout::identity_prefix(b.data(), 2, 16) == 10, "a gap ends the prefix");
  CHECK(relayout::identity_prefix(a.data(), 2, 15) == 15 && relayout::identity_prefix(nullptr, 0, 0) == 0, "all identity");
}

// ---- Book::relayout against a fresh configuration of the permuted columns
using usage_rows::Book;

static uint32_t ukey_of(uint32_t c, uint32_t m, uint32_t nc) { return c | (m << 14) | (nc << 28); }

static std::vector<uint32_t> permuted(const std::vector<uint32_t>& col, const Moves& mv, uint32_t n_new, uint32_t fill) {
  std::vector<uint32_t> out(n_new, fill);
  for (const kwk_move& m : mv)
    for (uint32_t i = 0; i < m.n; ++i) out[m.dst + i] = col[m.src + i];
  return out;
}

struct BookStats { int drops = 0, kept8 = 0, mixed_dropped = 0, mixed_moved = 0; };

static void compare_books(const Book& b, const Book& f, const char* what) {
  CHECK(b.ukey == f.ukey, "%s: keys", what);
  CHECK(b.n_mixed_pods == f.n_mixed_pods, "%s: mixed pods %llu vs %llu", what, (unsigned long long)b.n_mixed_pods,
        (unsigned long long)f.n_mixed_pods);
  for (int c = 0; c < 16; ++c)
    CHECK(b.nc_hist[c] == f.nc_hist[c], "%s: nc_hist[%d] %llu vs %llu", what, c, (unsigned long long)b.nc_hist[c],
          (unsigned long long)f.nc_hist[c]);
  CHECK(b.keys.size() == f.keys.size(), "%s: distinct keys %zu vs %zu", what, b.keys.size(), f.keys.size());
  for (const auto& kr : f.keys) {
    const auto it = b.keys.find(kr.first);
    CHECK(it != b.keys.end() && it->second.count == kr.second.count, "%s: count of key %08x", what, kr.first);
  }
  CHECK(b.max_nc() == f.max_nc(), "%s: max_nc", what);
  if (b.key8) {  // the live set is the fresh dictionary's; every key in use has one entry, free entries hold 0
    std::set<uint32_t> live, fresh(f.dict.begin(), f.dict.end());
    std::set<uint32_t> free_set(b.dict_free.begin(), b.dict_free.end());
    for (size_t d = 0; d < b.dict.size(); ++d) {
      if (free_set.count((uint32_t)d)) { CHECK(b.dict[d] == 0, "%s: free entry %zu holds a key", what, d); continue; }
      CHECK(live.insert(b.dict[d]).second, "%s: key %08x twice in the dictionary", what, b.dict[d]);
      const auto it = b.keys.find(b.dict[d]);
      CHECK(it != b.keys.end() && it->second.idx == (int32_t)d, "%s: entry %zu and its key's idx", what, d);
    }
    CHECK(f.key8 && live == fresh, "%s: dictionary live set (%zu vs %zu)", what, live.size(), fresh.size());
    CHECK(b.dict_live() == live.size() && b.dict.size() <= usage_rows::kDictMax, "%s: dict_live", what);
  } else {
    for (const auto& kr : b.keys) CHECK(kr.second.idx < 0, "%s: an entry without a dictionary", what);
  }
}

static void check_book(uint32_t rounds, uint32_t seed, BookStats& st) {
  std::mt19937 rng(seed ^ 0x9E3779B9u);
  const uint32_t n_cpu = 40, n_mem = 40;
  // (a) seeded layouts over uniform and mixed pods
  for (uint32_t r = 0; r < rounds; ++r) {
    const uint32_t n_old = 1 + rng() % 400;
    const bool with_mixed = rng() % 2;
    const uint32_t n_mixed_tab = 5;
    std::vector<uint32_t> mixed, ckeys;
    for (uint32_t m = 0; m < n_mixed_tab; ++m) {
      mixed.push_back((uint32_t)ckeys.size()), mixed.push_back(1 + m % 3);
      for (uint32_t c = 0; c < 1 + m % 3; ++c) ckeys.push_back((rng() % n_cpu) | ((rng() % n_mem) << 14));
    }
    const uint32_t key_space = 1 + rng() % 12;
    std::vector<uint32_t> k(n_old);
    for (uint32_t& x : k)
      x = (with_mixed && rng() % 6 == 0) ? rng() % n_mixed_tab : ukey_of(rng() % key_space, rng() % 3, 1 + rng() % 3);
    Book b;
    std::vector<uint8_t> k8;
    b.configure(k.data(), n_old, n_cpu, 0, n_mem, 0, &k8);
    if (with_mixed) CHECK(b.set_mixed(mixed.data(), n_mixed_tab, ckeys.data(), (uint32_t)ckeys.size()).empty(), "set_mixed");
    const bool had8 = b.key8;
    uint32_t n_new = 0;
    const Moves mv = random_moves(rng, n_old, n_new);
    const uint32_t fresh = ukey_of(rng() % n_cpu, rng() % n_mem, 1 + rng() % 15);
    const std::vector<uint32_t> want_k = permuted(k, mv, n_new, fresh);
    const std::vector<uint32_t> old_mbase = b.mbase, old_mcap = b.mcap;
    const uint64_t old_end = b.ccum_end;
    usage_rows::Effects fx;
    uint32_t f8 = 0;
    CHECK(b.relayout(mv.data(), (uint32_t)mv.size(), n_new, fresh, fx, &f8).empty(), "relayout");
    Book f;
    f.configure(want_k.data(), n_new, n_cpu, 0, n_mem, 0, nullptr);
    std::vector<uint8_t> f_k8;
    f.build_dict(f_k8);
    if (with_mixed) CHECK(f.set_mixed(mixed.data(), n_mixed_tab, ckeys.data(), (uint32_t)ckeys.size()).empty(), "set_mixed");
    compare_books(b, f, "seeded");
    if (had8 && n_new) {
      CHECK(b.key8 && !fx.key8_dropped, "the 1-byte column survives a layout of at most 255 keys");
      // the device's column moves as it is: an old pod's byte still names its key, a fresh one's is f8
      std::vector<uint32_t> col(k8.begin(), k8.end());
      const std::vector<uint32_t> moved = permuted(col, mv, n_new, f8);
      for (uint32_t p = 0; p < n_new; ++p)
        CHECK(moved[p] < b.dict.size() && b.dict[moved[p]] == b.ukey[p], "pod %u: byte %u names %08x, its key is %08x", p,
              moved[p], moved[p] < b.dict.size() ? b.dict[moved[p]] : 0u, b.ukey[p]);
      ++st.kept8;
    }
    if (with_mixed) {  // ranges travel with their pods, stay inside the buffer, and nobody shares one
      CHECK(b.ccum_end == old_end, "no range is handed out");
      CHECK(b.mbase == permuted(old_mbase, mv, n_new, 0) && b.mcap == permuted(old_mcap, mv, n_new, 0), "ranges follow the pods");
      std::set<uint32_t> bases;
      uint64_t before = 0, after = 0;
      for (uint32_t p = 0; p < n_old; ++p) before += !(k[p] >> 28);
      for (uint32_t p = 0; p < n_new; ++p)
        if (!(b.ukey[p] >> 28)) {
          ++after;
          CHECK(bases.insert(b.mbase[p]).second && (uint64_t)b.mbase[p] + b.mcap[p] <= b.ccum_end && b.mcap[p] == b.containers(p),
                "pod %u: range %u + %u", p, b.mbase[p], b.mcap[p]);
        }
      st.mixed_moved += (int)after, st.mixed_dropped += (int)(before - after);
    }
  }
  // (b) both sides of 255 -> 256 distinct keys
  for (uint32_t distinct : {254u, 255u}) {
    std::vector<uint32_t> k;
    for (uint32_t d = 0; d < distinct; ++d) k.push_back(ukey_of(d % n_cpu, d / n_cpu, 1)), k.push_back(k.back());
    const uint32_t n = (uint32_t)k.size();
    Book b;
    std::vector<uint8_t> k8;
    b.configure(k.data(), n, n_cpu, 0, n_mem, 0, &k8);
    CHECK(b.key8 && b.dict.size() == distinct, "%u keys: a dictionary", distinct);
    const Moves mv = {{0, 0, n}};
    const uint32_t fresh = ukey_of(1, 1, 9);  // a key nobody has
    usage_rows::Effects fx;
    uint32_t f8 = 0;
    CHECK(b.relayout(mv.data(), 1, n + 3, fresh, fx, &f8).empty(), "relayout");
    Book f;
    const std::vector<uint32_t> want = permuted(k, mv, n + 3, fresh);
    f.configure(want.data(), n + 3, n_cpu, 0, n_mem, 0, &k8);
    CHECK(b.key8 == f.key8 && b.key8 == (distinct < 255) && fx.key8_dropped == (distinct == 255),
          "%u + 1 keys: the column is %s here, %s freshly configured", distinct, b.key8 ? "kept" : "dropped", f.key8 ? "kept" : "dropped");
    if (b.key8) CHECK(fx.kv_set.size() == 1 && fx.kv_set[0] == f8 && b.dict[f8] == fresh, "the fresh key's entry");
    else ++st.drops;
    compare_books(b, f, "256th key");
    // ... and a key that falls out of use frees its entry for the fresh one
    Book c;
    c.configure(k.data(), n, n_cpu, 0, n_mem, 0, &k8);
    const Moves drop2 = {{0, 2, n - 2}};  // the first key's two pods go
    CHECK(c.relayout(drop2.data(), 1, n, fresh, fx, &f8).empty() && c.key8 && !fx.key8_dropped && c.dict_live() == distinct,
          "%u keys, one out and one in: the column stays", distinct);
    Book g;
    const std::vector<uint32_t> want2 = permuted(k, drop2, n, fresh);
    g.configure(want2.data(), n, n_cpu, 0, n_mem, 0, &k8);
    compare_books(c, g, "a freed entry");
  }
}

// ---- refusals: each names what it refuses and changes nothing
static void check_refusals() {
  const uint32_t node_ptr_old[] = {0, 4, 8, 12};
  (void)node_ptr_old;
  std::vector<uint32_t> k(12, ukey_of(0, 0, 1));
  Book b;
  b.configure(k.data(), 12, 2, 0, 2, 0, nullptr);
  const Book before = b;
  const uint32_t good_ptr[] = {0, 5, 9, 13};
  const kwk_move good_mv[] = {{0, 0, 4}, {5, 4, 8}};
  const kwk_move good_nodes[] = {{0, 0, 3}};
  auto layout = [&]() {
    kwk_layout L{};
    L.n_active = 13, L.n_moves = 2, L.moves = good_mv, L.n_nodes = 3, L.node_ptr = good_ptr, L.n_node_moves = 1,
    L.node_moves = good_nodes, L.fresh_usage_key = ukey_of(1, 1, 2);
    return L;
  };
  auto expect = [&](const kwk_layout& L, kwk_status status, const char* needle, const char* what) {
    const relayout::Verdict v = relayout::check_layout(L, 12, 16, true, 3, b.n_cpu, b.n_mem);
    CHECK(v.status == status && v.msg.find(needle) != std::string::npos, "%s: status %d, message \"%s\" (wanted \"%s\")", what,
          v.status, v.msg.c_str(), needle);
    CHECK(b.ukey == before.ukey && b.keys.size() == before.keys.size() && b.nc_hist[1] == before.nc_hist[1], "%s: the book", what);
  };
  expect(layout(), KWK_OK, "", "the good layout");
  kwk_layout L = layout();
  const kwk_move src_out[] = {{0, 0, 4}, {5, 5, 8}};
  L.moves = src_out;
  expect(L, KWK_EINVAL, "run 1 {dst 5, src 5, n 8}: source beyond the 12", "a run outside the old slots");
  L = layout();
  const kwk_move dst_out[] = {{0, 0, 4}, {6, 4, 8}};
  L.moves = dst_out;
  expect(L, KWK_EINVAL, "run 1 {dst 6, src 4, n 8}: destination beyond the 13", "a run outside the new slots");
  L = layout();
  const kwk_move unsorted[] = {{5, 4, 8}, {0, 0, 4}};
  L.moves = unsorted;
  expect(L, KWK_EINVAL, "run 1 {dst 0, src 0, n 4}: not sorted by dst", "unsorted runs");
  L = layout();
  const kwk_move dst_overlap[] = {{0, 0, 4}, {3, 4, 8}};
  L.moves = dst_overlap;
  expect(L, KWK_EINVAL, "run 1 {dst 3, src 4, n 8}: overlaps run 0 in dst", "runs overlapping in dst");
  L = layout();
  const kwk_move src_overlap[] = {{0, 0, 4}, {5, 3, 8}};
  L.moves = src_overlap;
  expect(L, KWK_EINVAL, "run 1 {dst 5, src 3, n 8}: overlaps run 0 in src", "runs overlapping in src");
  L = layout();
  const uint32_t decreasing[] = {0, 9, 5, 13};
  L.node_ptr = decreasing;
  expect(L, KWK_EINVAL, "node 1: node_ptr must be non-decreasing", "a decreasing node_ptr");
  L = layout();
  const uint32_t short_ptr[] = {0, 5, 9, 12};
  L.node_ptr = short_ptr;
  expect(L, KWK_EINVAL, "node_ptr[n_nodes] = 12 must equal n_active = 13", "node_ptr that ends elsewhere");
  L = layout();
  const kwk_move node_out[] = {{0, 1, 3}};
  L.node_moves = node_out;
  expect(L, KWK_EINVAL, "node run 0 {dst 0, src 1, n 3}: source beyond the 3", "a node run outside the old nodes");
  L = layout();
  L.fresh_usage_key = ukey_of(2, 0, 1);
  expect(L, KWK_EINVAL, "fresh_usage_key", "a fresh key outside the cpu table");
  L.fresh_usage_key = ukey_of(0, 2, 1);
  expect(L, KWK_EINVAL, "value id outside the tables", "a fresh key outside the memory table");
  L.fresh_usage_key = 3;
  expect(L, KWK_EINVAL, "a mixed key", "a mixed key as the fresh key");
  L = layout();
  L.n_active = 17;
  expect(L, KWK_EINVAL, "n_active 17 exceeds capacity 16", "n_active beyond capacity");
  // the book refuses the same keys itself, unchanged
  usage_rows::Effects fx;
  CHECK(!b.relayout(good_mv, 2, 13, 3, fx, nullptr).empty() && !b.relayout(good_mv, 2, 13, ukey_of(2, 0, 1), fx, nullptr).empty() &&
            b.ukey == before.ukey && b.nc_hist[1] == before.nc_hist[1],
        "Book::relayout refuses a bad fresh key");
  // an engine without a usage configuration takes no node layout
  kwk_layout N{};
  N.n_active = 13, N.n_moves = 2, N.moves = good_mv;
  CHECK(relayout::check_layout(N, 12, 16, false, 0, 0, 0).status == KWK_OK, "slot runs alone");
  N.n_nodes = 3, N.node_ptr = good_ptr;
  CHECK(relayout::check_layout(N, 12, 16, false, 0, 0, 0).status == KWK_EINVAL, "a node layout without kwk_usage_config");
}

int main(int argc, char** argv) {
  const uint32_t rounds = argc > 1 ? (uint32_t)std::atoi(argv[1]) : 40;
  const uint32_t seed = argc > 2 ? (uint32_t)std::atoi(argv[2]) : 1;
  check_gather(rounds, seed);
  BookStats st;
  check_book(rounds, seed, st);
  check_refusals();
  std::printf("%u rounds, %d kept columns, %d dictionary drops, %d mixed moved, %d mixed dropped, %d failures\n", rounds, st.kept8,
              st.drops, st.mixed_moved, st.mixed_dropped, g_fail);
  return g_fail ? 1 : 0;
}
