// Moving whole runs of slots between positions of a per-slot column (kwk_relayout, kwok_engine.h):
// the checks of a run list, the lookup of the run that covers a destination slot, and the body of
// relayout_gather_kernel — what one lane writes for one 16-byte destination chunk.  The body is
// __host__ __device__ (the usage_rows.hpp / keycmp.hpp pattern), so the engine's kernel and
// tools/relayout_check.cpp, which runs it on host arrays under the sanitizers, share it.
//
// A column holds elements of 1, 2, 4, 8, 16 or 32 bytes, one per slot.  The gather is out of
// place: destination chunk c (bytes [16 c, 16 c + 16) of the new column) is assembled from the
// old column and stored whole.  A destination slot that a run {dst, src, n} covers takes the
// element of slot src + (slot - dst); every other slot — a fresh one, and the padding up to the
// chunk's end past the last slot — takes the column's fill element.
//
// Bounds: the old column must be readable up to the next multiple of 16 bytes past its last
// element (the aligned 16-byte loads of the 1- and 2-byte fast path), the new one writable
// likewise.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/kwok_engine.h"

namespace relayout {

#if defined(__HIPCC__)
#define RELAYOUT_HD __host__ __device__
#else
#define RELAYOUT_HD
#endif

struct alignas(16) V16 { uint32_t w[4]; };
// the fill element of a column (its first EB bytes), repeated to 32 bytes
struct Fill { uint32_t w[8]; };

inline Fill fill_of(const void* elem, uint32_t eb) {
  Fill f;
  unsigned char* p = reinterpret_cast<unsigned char*>(f.w);
  for (uint32_t i = 0; i < 32; ++i) p[i] = static_cast<const unsigned char*>(elem)[i % eb];
  return f;
}

// an aligned load of T: a plain load on the device, memcpy on the host (no aliasing assumptions
// about the caller's arrays)
template <class T>
RELAYOUT_HD inline T ld(const unsigned char* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return *reinterpret_cast<const T*>(p);
#else
  T v;
  memcpy(&v, p, sizeof(T));
  return v;
#endif
}

// the first run whose end lies past `slot` (runs sorted by dst and disjoint, so ends ascend too);
// n_runs when there is none.  The run covers the slot iff its dst <= slot.
RELAYOUT_HD inline uint32_t find_run(const kwk_move* runs, uint32_t n_runs, uint32_t slot) {
  uint32_t lo = 0, hi = n_runs;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if ((uint64_t)runs[mid].dst + runs[mid].n <= slot) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// the first run whose dst is at or past `slot`
RELAYOUT_HD inline uint32_t first_run_from(const kwk_move* runs, uint32_t n_runs, uint32_t slot) {
  uint32_t lo = 0, hi = n_runs;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (runs[mid].dst < slot) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// bytes [sh, sh + 16) of the 32 bytes {a, b}, sh < 16
RELAYOUT_HD inline V16 shift_bytes(const V16& a, const V16& b, uint32_t sh) {
  const uint32_t ws = sh >> 2, bs = (sh & 3u) * 8u;
  V16 out;
#pragma unroll
  for (uint32_t i = 0; i < 4; ++i) {
    uint32_t lo = 0, hi = 0;  // words i + ws and i + ws + 1 of {a, b}, by selects: no indexed registers
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
      const uint32_t x = j < 4 ? a.w[j & 3u] : b.w[j & 3u];
      lo = (j == i + ws) ? x : lo;
      hi = (j == i + ws + 1) ? x : hi;
    }
    out.w[i] = (uint32_t)((((uint64_t)hi << 32) | lo) >> bs);
  }
  return out;
}

// Destination chunk c of a column of EB-byte elements.  `runs` are runs that may cover the chunk's
// slots: the whole list, or any slice of it that holds every run intersecting the chunk.
template <uint32_t EB>
RELAYOUT_HD inline V16 gather_chunk(const unsigned char* src, uint64_t c, const kwk_move* runs, uint32_t n_runs,
                                    const Fill& fill) {
  static_assert(EB == 1 || EB == 2 || EB == 4 || EB == 8 || EB == 16 || EB == 32, "element bytes");
  V16 out;
  if constexpr (EB >= 16) {  // the chunk is (a half of) one element
    const uint32_t slot = (uint32_t)(c * 16u / EB), part = (uint32_t)(c % (EB / 16u));
    const uint32_t r = find_run(runs, n_runs, slot);
    if (r < n_runs && runs[r].dst <= slot) {
      const uint64_t s = (uint64_t)runs[r].src + (slot - runs[r].dst);
      out = ld<V16>(src + s * EB + 16u * part);
    } else {
#pragma unroll
      for (uint32_t i = 0; i < 4; ++i) out.w[i] = fill.w[4u * part + i];
    }
    return out;
  } else {
    constexpr uint32_t kPer = 16u / EB;  // slots per chunk
    const uint32_t slot0 = (uint32_t)(c * kPer);
    uint32_t r = find_run(runs, n_runs, slot0);
    const bool one = r < n_runs && runs[r].dst <= slot0 && (uint64_t)runs[r].dst + runs[r].n >= (uint64_t)slot0 + kPer;
    if (one) {  // the whole chunk out of one run: aligned 16-byte loads
      const uint64_t sb = ((uint64_t)runs[r].src + (slot0 - runs[r].dst)) * EB;
      const uint32_t sh = (uint32_t)(sb & 15u);
      const unsigned char* p = src + (sb - sh);
      if constexpr (EB <= 2) {  // src and dst differ modulo 16 in general: two loads and a byte shift
        const V16 a = ld<V16>(p);
        const V16 b = ld<V16>(p + (sh ? 16u : 0u));  // (sh = 0: the chunk itself again, never one past the column)
        return shift_bytes(a, b, sh);
      } else if (sh == 0) {
        return ld<V16>(p);
      }
    }
    // across run boundaries and fresh slots: element by element, assembled in registers
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) out.w[i] = fill.w[i];
    for (uint32_t k = 0; k < kPer; ++k) {
      const uint32_t slot = slot0 + k;
      while (r < n_runs && (uint64_t)runs[r].dst + runs[r].n <= slot) ++r;
      if (r >= n_runs || runs[r].dst > slot) continue;
      const unsigned char* p = src + ((uint64_t)runs[r].src + (slot - runs[r].dst)) * EB;
      if constexpr (EB == 8) {
        out.w[2 * k] = ld<uint32_t>(p), out.w[2 * k + 1] = ld<uint32_t>(p + 4);
      } else if constexpr (EB == 4) {
        out.w[k] = ld<uint32_t>(p);
      } else {
        const uint32_t v = EB == 2 ? (uint32_t)ld<uint16_t>(p) : (uint32_t)ld<uint8_t>(p);
        const uint32_t bit = (k * EB * 8u) & 31u, mask = (EB == 2 ? 0xFFFFu : 0xFFu) << bit;
        const uint32_t wi = k * EB / 4u;
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) out.w[i] = i == wi ? ((out.w[i] & ~mask) | (v << bit)) : out.w[i];
      }
    }
    return out;
  }
}

// chunks of a column of n slots
inline uint64_t chunks_of(uint64_t n, uint32_t eb) { return (n * eb + 15u) / 16u; }

// ---- host side: the checks of a run list (made before anything changes)
// "" or what is wrong with which run: outside [0, n_old) / [0, n_new), unsorted by dst, overlapping
// in dst or in src.  `what` names the list in the message ("run", "node run").
inline std::string check_moves(const kwk_move* m, uint32_t n_moves, uint32_t n_old, uint32_t n_new, const char* what) {
  const std::string w(what);
  if (n_moves && !m) return w + " list is null";
  for (uint32_t i = 0; i < n_moves; ++i) {
    const std::string at = w + " " + std::to_string(i) + " {dst " + std::to_string(m[i].dst) + ", src " +
                           std::to_string(m[i].src) + ", n " + std::to_string(m[i].n) + "}: ";
    if ((uint64_t)m[i].src + m[i].n > n_old) return at + "source beyond the " + std::to_string(n_old) + " of the old layout";
    if ((uint64_t)m[i].dst + m[i].n > n_new) return at + "destination beyond the " + std::to_string(n_new) + " of the new layout";
    if (i && m[i].dst < m[i - 1].dst) return at + "not sorted by dst (" + w + " " + std::to_string(i - 1) + ")";
    if (i && (uint64_t)m[i - 1].dst + m[i - 1].n > m[i].dst) return at + "overlaps " + w + " " + std::to_string(i - 1) + " in dst";
  }
  std::vector<uint32_t> by_src(n_moves);
  for (uint32_t i = 0; i < n_moves; ++i) by_src[i] = i;
  std::sort(by_src.begin(), by_src.end(), [&](uint32_t a, uint32_t b) { return m[a].src != m[b].src ? m[a].src < m[b].src : a < b; });
  uint32_t prev = 0;
  bool have = false;
  for (uint32_t j = 0; j < n_moves; ++j) {
    const uint32_t i = by_src[j];
    if (m[i].n == 0) continue;
    if (have && (uint64_t)m[prev].src + m[prev].n > m[i].src)
      return w + " " + std::to_string(i) + " {dst " + std::to_string(m[i].dst) + ", src " + std::to_string(m[i].src) + ", n " +
             std::to_string(m[i].n) + "}: overlaps " + w + " " + std::to_string(prev) + " in src";
    prev = i, have = true;
  }
  return "";
}
// slots [0, result) keep their place: a prefix of identity runs without a gap (the gather starts
// past it).  n_new when every slot does, i.e. the list is all identity and covers [0, n_new).
inline uint32_t identity_prefix(const kwk_move* m, uint32_t n_moves, uint32_t n_new) {
  uint32_t p = 0;
  for (uint32_t i = 0; i < n_moves; ++i) {
    if (m[i].n == 0) continue;
    if (m[i].dst != p || m[i].src != m[i].dst) break;
    p += m[i].n;
  }
  return p < n_new ? p : n_new;
}

// Every check of a kwk_layout that needs no device (kwk_relayout makes them before anything
// changes; tools/relayout_check.cpp runs the same function): KWK_OK, or KWK_EINVAL with
// a message naming the offending run or node.  n_old / nodes_old: the engine's slots and nodes
// now; usage: kwk_usage_config was called, with cpu_ids / mem_ids value ids in its tables.
struct Verdict {
  kwk_status status = KWK_OK;
  std::string msg;
};
inline Verdict check_layout(const kwk_layout& to, uint32_t n_old, uint32_t capacity, bool usage, uint32_t nodes_old,
                            uint32_t cpu_ids, uint32_t mem_ids) {
  const uint32_t n_new = to.n_active;
  if (n_new > capacity)
    return {KWK_EINVAL, "n_active " + std::to_string(n_new) + " exceeds capacity " + std::to_string(capacity) +
                          " (capacity does not grow)"};
  std::string bad = check_moves(to.moves, to.n_moves, n_old, n_new, "run");
  if (!bad.empty()) return {KWK_EINVAL, bad};
  if (!usage) {
    if (to.n_nodes || to.n_node_moves)
      return {KWK_EINVAL, "a node layout on an engine without kwk_usage_config (n_nodes and n_node_moves must be 0)"};
    return {};
  }
  if (!to.node_ptr) return {KWK_EINVAL, "node_ptr is null"};
  if (to.node_ptr[0] != 0) return {KWK_EINVAL, "node 0: node_ptr[0] must be 0"};
  for (uint32_t j = 0; j < to.n_nodes; ++j)
    if (to.node_ptr[j + 1] < to.node_ptr[j])
      return {KWK_EINVAL, "node " + std::to_string(j) + ": node_ptr must be non-decreasing (" + std::to_string(to.node_ptr[j]) +
                              " then " + std::to_string(to.node_ptr[j + 1]) + ")"};
  if (to.node_ptr[to.n_nodes] != n_new)
    return {KWK_EINVAL, "node_ptr[n_nodes] = " + std::to_string(to.node_ptr[to.n_nodes]) + " must equal n_active = " +
                            std::to_string(n_new)};
  bad = check_moves(to.node_moves, to.n_node_moves, nodes_old, to.n_nodes, "node run");
  if (!bad.empty()) return {KWK_EINVAL, bad};
  const uint32_t k = to.fresh_usage_key;
  if (!(k >> 28)) return {KWK_EINVAL, "fresh_usage_key " + std::to_string(k) + ": a mixed key (0 containers)"};
  if ((k & 0x3FFFu) >= cpu_ids || ((k >> 14) & 0x3FFFu) >= mem_ids)
    return {KWK_EINVAL, "fresh_usage_key " + std::to_string(k) + ": value id outside the tables"};
  return {};
}

}  // namespace relayout
