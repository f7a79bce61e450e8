// Checks the composite id table of the fused 1-byte sweep (kwok_amd/csrc/id8_compose.hpp) against the
// one-step rule applied k times to every id, restated here on its own: an item is on the list at
// step 0; at a step it is on the list its id is looked up (statistics, maybe a fired record) and it
// stays on the list iff the new id has the need bit; once off it is never looked up again.
//
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tools/id8_compose_check.cpp
//   id8_compose_check [tables] [seed] [table.bin ...]    (table.bin: 512 little-endian uint32 entries)
//
// Exit status 0 and "0 bad" on success.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "../kwok_amd/csrc/id8_compose.hpp"

namespace {

struct Rng {  // splitmix64
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  uint32_t below(uint32_t n) { return (uint32_t)(next() % n); }
};

struct Want {
  bool fire[4] = {false, false, false, false};
  uint32_t rec[4] = {0, 0, 0, 0};  // bits 15-11 of the fired entry
  uint32_t last = 0, bytes = 0, matched = 0, live = 0, per_stage[4] = {0, 0, 0, 0};
};

// the trajectory of one item, one step at a time
Want iterate(const uint32_t* t8, uint32_t id, int k) {
  Want w;
  bool on_list = true;
  uint32_t cur = id;
  for (int s = 0; s < k; ++s) {
    if (!on_list) break;
    if (s >= 1 && cur != 0xFF) ++w.live;  // (the inactive lanes' 0xFF is no item)
    const uint32_t e = t8[cur];
    w.bytes += (e >> 24) % 32;
    if (e & 0x40000000u) ++w.matched;
    if (e & 0x80000000u) {
      w.fire[s] = true;
      w.rec[s] = e & 0xF800u;
      ++w.per_stage[(e >> 11) % 4];
    }
    cur = e % 256;
    on_list = (cur & 0x80u) != 0;
  }
  w.last = cur;
  return w;
}

int check_table(const uint32_t* t8, const char* what, long which) {
  int bad = 0;
  for (int k : {2, 4}) {
    // exact-size heap buffer: a write past the 256 rows is a sanitizer report
    std::unique_ptr<uint32_t[]> out(new uint32_t[256 * kId8cRowWords]);
    id8_compose(t8, k, out.get());
    for (uint32_t id = 0; id < 256; ++id) {
      const uint32_t* r = &out[id * kId8cRowWords];
      const Want w = iterate(t8, id, k);
      bool ok = (r[0] & 0xFFu) == w.last && (r[1] & 7u) == w.matched && ((r[1] >> 16) & 0x7Fu) == w.bytes &&
                (r[2] & 3u) == w.live;
      for (int s = 0; s < 4; ++s) {
        const bool fire = s < k && w.fire[s];
        ok = ok && ((r[s] >> 31) != 0) == fire && (r[s] & 0xF800u) == (fire ? w.rec[s] : 0u);
        ok = ok && ((r[3] >> (8 * s)) & 7u) == w.per_stage[s];
      }
      // nothing outside the documented fields
      ok = ok && !(r[0] & ~(0x8000F800u | 0xFFu)) && !(r[1] & ~(0x8000F800u | 0x7F0007u)) &&
           !(r[2] & ~(0x8000F800u | 3u)) && !(r[3] & ~(0x8000F800u | 0x07070707u));
      if (!ok) {
        if (++bad <= 10)
          std::fprintf(stderr, "BAD %s %ld k=%d id=%u row=%08x %08x %08x %08x\n", what, which, k, id, r[0], r[1], r[2], r[3]);
      }
    }
  }
  return bad;
}

uint32_t entry(Rng& g, uint32_t new_id) {
  const uint32_t stage = g.below(4), flags = g.below(8), fire = g.below(2), match = fire | g.below(2);
  return new_id | stage << 11 | flags << 13 | g.below(32) << 16 | flags << 21 | g.below(32) << 24 | match << 30 | fire << 31;
}

// identity at 0xFF and at a random set of unused ids; every other id moves to a used id (never
// 0xFF, which the dictionary never stores) with random need bit, fire bit, stage, flags and bytes
void random_table(Rng& g, std::vector<uint32_t>& t8, uint32_t need_pct) {
  std::vector<uint32_t> used;
  for (uint32_t id = 0; id < 255; ++id)
    if (id == 0 || g.below(4) != 0) used.push_back(id);
  std::vector<uint32_t> quiet, busy;  // used ids without / with the need bit
  for (uint32_t id : used) (id & 0x80u ? busy : quiet).push_back(id);
  for (uint32_t i = 0; i < 512; ++i) t8[i] = i & 0xFFu;
  for (uint32_t half = 0; half < 2; ++half)
    for (uint32_t id : used) {
      const bool to_busy = !busy.empty() && g.below(100) < need_pct;
      const std::vector<uint32_t>& pool = to_busy || quiet.empty() ? busy : quiet;
      t8[half << 8 | id] = entry(g, pool[g.below((uint32_t)pool.size())]);
    }
}

}  // namespace

int main(int argc, char** argv) {
  const long n_tables = argc > 1 ? std::atol(argv[1]) : 3000;
  Rng g{argc > 2 ? std::strtoull(argv[2], nullptr, 0) : 1};
  long bad = 0, tables = 0;
  std::vector<uint32_t> t8(512);
  for (long i = 0; i < n_tables; ++i, ++tables) {
    random_table(g, t8, (uint32_t)(i % 5) * 25u);
    bad += check_table(t8.data(), "random", i);
  }
  // an id that fires the same stage at every step: 0x80 loops on itself
  for (uint32_t i = 0; i < 512; ++i) t8[i] = i & 0xFFu;
  t8[0x80] = 0x80u | 2u << 11 | 5u << 13 | 2u << 16 | 5u << 21 | 31u << 24 | 1u << 30 | 1u << 31;
  bad += check_table(t8.data(), "loop", 0);
  ++tables;
  // ids that leave the list at each possible step: a chain 0x81 -> 0x82 -> 0x83 -> 0x84 -> 0x21,
  // every link firing another stage, entered at each of its ids
  for (uint32_t i = 0; i < 512; ++i) t8[i] = i & 0xFFu;
  for (uint32_t j = 0; j < 4; ++j)
    t8[0x81 + j] = (j == 3 ? 0x21u : 0x82u + j) | j << 11 | j << 13 | j << 16 | j << 21 | (3u + j) << 24 | 1u << 30 | 1u << 31;
  bad += check_table(t8.data(), "chain", 0);
  ++tables;
  // no entry leads to an id with the need bit: everything leaves at step 0
  for (uint32_t half = 0; half < 2; ++half)
    for (uint32_t id = 0; id < 255; ++id) t8[half << 8 | id] = entry(g, g.below(128));
  t8[0xFF] = t8[0x1FF] = 0xFF;
  bad += check_table(t8.data(), "no-need", 0);
  ++tables;
  for (int a = 3; a < argc; ++a) {  // dumped tables
    std::FILE* f = std::fopen(argv[a], "rb");
    if (!f) {
      std::fprintf(stderr, "cannot open %s\n", argv[a]);
      return 2;
    }
    unsigned char raw[2048];
    const size_t got = std::fread(raw, 1, sizeof raw, f);
    std::fclose(f);
    if (got != sizeof raw) {
      std::fprintf(stderr, "%s: want 2048 bytes\n", argv[a]);
      return 2;
    }
    for (uint32_t i = 0; i < 512; ++i)
      t8[i] = (uint32_t)raw[4 * i] | (uint32_t)raw[4 * i + 1] << 8 | (uint32_t)raw[4 * i + 2] << 16 | (uint32_t)raw[4 * i + 3] << 24;
    bad += check_table(t8.data(), argv[a], 0);
    ++tables;
  }
  std::printf("%ld tables, %ld bad\n", tables, bad);
  return bad ? 1 : 0;
}
