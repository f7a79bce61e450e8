// Host bookkeeping of the usage configuration and of its incremental updates (kwk_usage_set_rows,
// kwk_usage_append, kwk_usage_mixed_append): the mirrors of the key column and the mixed tables,
// the per-container integrator ranges of mixed pods, the 1-byte key dictionary and what decides
// the usage kernel (containers per key, mixed pods, distinct keys).  Plain C++ without HIP, so
// tools/usage_rows_check.cpp drives it under the sanitizers; engine.hip turns what apply() returns
// into one staged copy and one usage_rows_kernel launch.
//
// Everything derived here stays what configure() + set_mixed() of the final columns would
// derive, except the integrator ranges (a fresh configuration packs them in slot order; rows
// reuse a slot's range or take one at the end) and the dictionary's order, which no result shows.
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/kwok_engine.h"

namespace usage_rows {

constexpr uint32_t kMixedIndex = 0x0FFFFFFFu;  // kUKeyMixedIndex
constexpr uint32_t kDictMax = 255;             // kUKeyZero: keys the 1-byte column can name

// what usage_rows_kernel does for one row
constexpr uint32_t kDevReset = 1u << 0;     // pod_last = INT64_MIN, unit integrator and unit_val = 0
constexpr uint32_t kDevCreated = 1u << 1;   // pod_created[slot] = created
constexpr uint32_t kDevMbase = 1u << 2;     // mbase[slot] = mbase
constexpr uint32_t kDevKey8 = 1u << 3;      // ukey8[slot] = k8
constexpr uint32_t kDevZeroUnit = 1u << 4;  // unit integrator and unit_val = 0 (a mixed pod turned uniform)
constexpr uint32_t kDevRange = 1u << 5;     // ccum / cval [mbase, mbase + range_n): the first copy_n from copy_from, the rest 0
constexpr uint32_t kDevSeedUnit = 1u << 6;  // kDevRange's first copy_n entries are the slot's unit integrator / unit_val
                                            // (a uniform pod turned mixed: its containers' totals were that one)
struct DevRow {
  uint32_t slot, key, mbase, flags;
  int64_t created;
  uint32_t range_n, copy_from, copy_n, k8;
};
static_assert(sizeof(DevRow) == 40, "DevRow is copied to the device as is");

#if defined(__HIPCC__)
#define USAGE_ROWS_HD __host__ __device__
#else
#define USAGE_ROWS_HD
#endif
// What one row writes: usage_rows_kernel's body, and what tools/usage_rows_check.cpp runs on host
// arrays.  Null: the engine has no such column (no 1-byte keys, no mixed tables, per-pod outputs
// off — then no integrators either —, no usage programs, no inputs).  pod_cum / unit_val / ccum /
// cval hold {cpu, mem} pairs.
struct RowTargets {
  uint32_t* ukey;
  uint8_t* ukey8;
  uint32_t* mbase;
  int64_t* pod_last;
  double* pod_cum;
  double* unit_val;
  double* ccum;
  double* cval;
  int64_t* pod_created;
};
USAGE_ROWS_HD inline void write_row(const DevRow& r, const RowTargets& a) {
  a.ukey[r.slot] = r.key;
  if (a.ukey8 && (r.flags & kDevKey8)) a.ukey8[r.slot] = (uint8_t)r.k8;  // a byte store: rows may share the dword
  if (a.mbase && (r.flags & kDevMbase)) a.mbase[r.slot] = r.mbase;
  if (a.pod_created && (r.flags & kDevCreated)) a.pod_created[r.slot] = r.created;
  if (a.ccum && (r.flags & kDevRange)) {
    const bool seed = (r.flags & kDevSeedUnit) && a.pod_last;
    for (uint32_t j = 0; j < r.range_n; ++j) {
      const bool keep = j < r.copy_n && (seed || !(r.flags & kDevSeedUnit));
      if (keep && !seed && r.copy_from == r.mbase) continue;
      for (uint32_t x = 0; x < 2; ++x) {
        const size_t to = 2 * (size_t)(r.mbase + j) + x, from = 2 * (size_t)(r.copy_from + j) + x, unit = 2 * (size_t)r.slot + x;
        a.ccum[to] = !keep ? 0.0 : seed ? a.pod_cum[unit] : a.ccum[from];
        if (a.cval) a.cval[to] = !keep ? 0.0 : seed ? (a.unit_val ? a.unit_val[unit] : 0.0) : a.cval[from];
      }
    }
  }
  if (a.pod_last) {
    if (r.flags & kDevReset) a.pod_last[r.slot] = INT64_MIN;
    if (r.flags & (kDevReset | kDevZeroUnit)) {
      a.pod_cum[2 * (size_t)r.slot] = a.pod_cum[2 * (size_t)r.slot + 1] = 0.0;
      if (a.unit_val) a.unit_val[2 * (size_t)r.slot] = a.unit_val[2 * (size_t)r.slot + 1] = 0.0;
    }
  }
}

struct Effects {
  bool layout_changed = false;  // some slot's container count changed (cptr)
  bool key8_dropped = false;    // the call ended the 1-byte column (a mixed key or a 256th distinct key)
  std::vector<uint32_t> kv_set;  // dictionary entries that got a key
};

struct Book {
  // the configuration's mirrors
  std::vector<uint32_t> ukey, mbase, mixed, ckeys;
  std::vector<uint32_t> mcap;  // per pod: integrators of the range at mbase (0: none yet)
  uint32_t n_cpu = 0, n_mem = 0, n_cpu_progs = 0, n_mem_progs = 0;
  bool mixed_tables = false;   // set_mixed / mixed_append was called: mixed keys may be used
  uint64_t ccum_end = 0;       // integrators handed out (abandoned ranges included)
  // derived from the keys
  uint64_t nc_hist[16] = {};   // uniform pods per container count
  uint64_t n_mixed_pods = 0;
  struct Ref { uint64_t count = 0; int32_t idx = -1; };
  std::unordered_map<uint32_t, Ref> keys;  // uniform keys in use; idx: the dictionary entry (key8)
  bool key8 = false;                       // the 1-byte column exists
  std::vector<uint32_t> dict, dict_free;   // key per entry; entries no key uses

  uint32_t n_pods() const { return (uint32_t)ukey.size(); }
  uint32_t n_mixed() const { return (uint32_t)(mixed.size() / 2); }
  bool has_mixed() const { return n_mixed_pods != 0; }
  uint32_t max_nc() const {
    uint32_t m = 0;
    for (uint32_t c = 1; c < 16; ++c) if (nc_hist[c]) m = c;
    return m;
  }
  uint32_t key_containers(uint32_t k) const { return (k >> 28) ? (k >> 28) : mixed[2 * (size_t)(k & kMixedIndex) + 1]; }
  uint32_t containers(uint32_t p) const { return key_containers(ukey[p]); }
  uint32_t dict_live() const { return (uint32_t)(dict.size() - dict_free.size()); }

  void drop_dict() {
    key8 = false;
    dict.clear();
    dict_free.clear();
    for (auto& kr : keys) kr.second.idx = -1;
  }

  // a full configuration (kwk_usage_config_dyn): no mixed tables yet.  With k8, the 1-byte column
  // comes out of the same pass where it can exist (build_dict's result: key8 says whether)
  void configure(const uint32_t* k, uint32_t n, uint32_t ncpu, uint32_t ncpu_progs, uint32_t nmem, uint32_t nmem_progs,
                 std::vector<uint8_t>* k8 = nullptr) {
    ukey.assign(k, k + n);
    mbase.clear(), mcap.clear(), mixed.clear(), ckeys.clear(), keys.clear();
    n_cpu = ncpu, n_cpu_progs = ncpu_progs, n_mem = nmem, n_mem_progs = nmem_progs;
    mixed_tables = false;
    ccum_end = 0;
    n_mixed_pods = 0;
    for (uint64_t& h : nc_hist) h = 0;
    drop_dict();
    if (k8) k8->resize(n);
    // few distinct keys as a rule: a short list searched in order (the last hit first), numbered by
    // first occurrence; past its 256 entries the map takes over
    uint32_t dk[kDictMax + 1];
    uint64_t cnt[kDictMax + 1];
    uint32_t nd = 0, hit = 0, hit_key = 0;  // (hit_key: the uniform key of entry `hit`; 0 until there is one)
    uint8_t* const col = k8 ? k8->data() : nullptr;
    uint32_t p = 0;
    for (; p < n; ++p) {
      const uint32_t key = k[p];
      if (key != hit_key || !(key >> 28)) {
        if (!(key >> 28)) { ++n_mixed_pods; continue; }
        for (hit = 0; hit < nd && dk[hit] != key; ++hit) {}
        if (hit == nd) {
          if (nd > kDictMax) break;  // the 257th: the map from here on
          dk[nd] = key, cnt[nd] = 0, ++nd;
        }
        hit_key = key;
      }
      ++cnt[hit];
      if (col) col[p] = (uint8_t)hit;
    }
    const bool over = p < n;
    for (uint32_t d = 0; d < nd; ++d) keys[dk[d]].count = cnt[d];
    Ref* last = nullptr;
    uint32_t last_key = 0;
    for (; p < n; ++p) {
      const uint32_t key = k[p];
      if (!(key >> 28)) { ++n_mixed_pods; continue; }
      if (!last || key != last_key) last = &keys[key], last_key = key;
      ++last->count;
    }
    for (const auto& kr : keys) nc_hist[kr.first >> 28] += kr.second.count;
    if (k8 && !over && !has_mixed() && nd <= kDictMax && n) {
      dict.assign(dk, dk + nd);
      for (size_t d = 0; d < dict.size(); ++d) keys[dict[d]].idx = (int32_t)d;
      key8 = true;
    }
  }

  // whether the 1-byte column can exist; then k8[p] = the dictionary entry of pod p's key, entries
  // numbered by first occurrence (as a configuration always did)
  bool build_dict(std::vector<uint8_t>& k8) {
    drop_dict();
    if (has_mixed() || keys.size() > kDictMax || ukey.empty()) return false;
    k8.resize(ukey.size());
    size_t hit = 0;  // (at most kDictMax entries: searched in order, the last hit first)
    for (size_t p = 0; p < ukey.size(); ++p) {
      const uint32_t key = ukey[p];
      if (hit >= dict.size() || dict[hit] != key) {
        for (hit = 0; hit < dict.size() && dict[hit] != key; ++hit) {}
        if (hit == dict.size()) dict.push_back(key);
      }
      k8[p] = (uint8_t)hit;
    }
    for (size_t d = 0; d < dict.size(); ++d) keys[dict[d]].idx = (int32_t)d;
    key8 = true;
    return true;
  }

  // kwk_usage_mixed: the whole tables; every mixed pod's range packed in slot order
  // ("" or what is wrong; nothing changes then)
  std::string set_mixed(const uint32_t* m, uint32_t n_m, const uint32_t* ck, uint32_t n_ck) {
    uint64_t nint = 0;
    for (uint32_t p = 0; p < n_pods(); ++p)
      if (!(ukey[p] >> 28)) {
        nint += m[2 * (size_t)(ukey[p] & kMixedIndex) + 1];
        if (nint > 0xFFFFFFFFull) return "more than 2^32 containers of mixed pods";
      }
    mixed.assign(m, m + 2 * (size_t)n_m);
    ckeys.assign(ck, ck + n_ck);
    mbase.assign(n_pods(), 0u);
    mcap.assign(n_pods(), 0u);
    nint = 0;
    for (uint32_t p = 0; p < n_pods(); ++p)
      if (!(ukey[p] >> 28)) {
        mbase[p] = (uint32_t)nint;
        mcap[p] = mixed[2 * (size_t)(ukey[p] & kMixedIndex) + 1];
        nint += mcap[p];
      }
    ccum_end = nint;
    mixed_tables = true;
    return "";
  }

  bool key_ids_ok(uint32_t k) const {
    return (k & 0x3FFFu) < n_cpu + n_cpu_progs && ((k >> 14) & 0x3FFFu) < n_mem + n_mem_progs;
  }

  // kwk_usage_mixed_append: entries whose {first, count} index the table of container keys as it
  // is after the append
  std::string mixed_append(const uint32_t* m, uint32_t n_m, const uint32_t* ck, uint32_t n_ck) {
    if ((uint64_t)n_mixed() + n_m > kMixedIndex) return "more than 2^28 - 1 mixed entries";
    const uint64_t total = (uint64_t)ckeys.size() + n_ck;
    if (total > 0xFFFFFFFFull) return "more than 2^32 container keys";
    for (uint32_t i = 0; i < n_m; ++i)
      if ((uint64_t)m[2 * (size_t)i] + m[2 * (size_t)i + 1] > total)
        return "mixed entry " + std::to_string(n_mixed() + i) + " beyond ckeys";
    for (uint32_t c = 0; c < n_ck; ++c)
      if (!key_ids_ok(ck[c])) return "ckeys " + std::to_string(ckeys.size() + c) + ": value id out of range";
    if (!mixed_tables) {
      mbase.assign(n_pods(), 0u);
      mcap.assign(n_pods(), 0u);
      mixed_tables = true;
    }
    mixed.insert(mixed.end(), m, m + 2 * (size_t)n_m);
    ckeys.insert(ckeys.end(), ck, ck + n_ck);
    return "";
  }

  // usage_fast_kernel's table of pod values: rows 0..max_nc of (n_cpu + n_mem) entries; where a
  // uniform key's {cpu, mem} lie in it
  size_t podv_entries() const { return ((size_t)max_nc() + 1) * ((size_t)n_cpu + n_mem); }
  void kv_at(uint32_t k, size_t& c, size_t& m) const {
    const size_t row = (size_t)(k >> 28) * ((size_t)n_cpu + n_mem);
    c = row + (k & 0x3FFFu);
    m = row + n_cpu + ((k >> 14) & 0x3FFFu);
  }
  // the dictionary's {cpu, mem} values out of that table (the same entries the 4-byte-key kernel
  // reads, so sums are bit-identical); entries no key uses hold a stale key no longer: {0, 0}
  void fill_kv(const std::vector<double>& podv, double* kv) const {
    for (size_t d = 0; d < dict.size(); ++d) {
      size_t c = 0, m = 0;
      if (dict[d]) kv_at(dict[d], c, m);
      kv[2 * d] = dict[d] ? podv[c] : 0.0;
      kv[2 * d + 1] = dict[d] ? podv[m] : 0.0;
    }
  }

  void release(uint32_t k) {
    if (!(k >> 28)) { --n_mixed_pods; return; }
    --nc_hist[k >> 28];
    auto it = keys.find(k);
    if (--it->second.count == 0) {
      if (it->second.idx >= 0) dict_free.push_back((uint32_t)it->second.idx), dict[it->second.idx] = 0u;  // (0: free)
      keys.erase(it);
    }
  }
  void acquire(uint32_t k) {
    if (!(k >> 28)) { ++n_mixed_pods; return; }
    ++nc_hist[k >> 28];
    ++keys[k].count;
  }

  // kwk_usage_set_rows: checks every row, then moves the mirrors to the new columns and fills
  // `out` with what the device has to write.  "" or what is wrong with which row; the book is
  // unchanged then.
  std::string apply(const kwk_usage_row* rows, uint32_t n, std::vector<DevRow>& out, Effects& fx) {
    out.clear();
    fx = Effects{};
    std::vector<std::pair<uint32_t, uint32_t>> seen(n);
    uint64_t worst = ccum_end;
    for (uint32_t i = 0; i < n; ++i) {
      const kwk_usage_row& r = rows[i];
      const std::string at = "row " + std::to_string(i) + ": ";
      if (r.slot >= n_pods())
        return at + "slot " + std::to_string(r.slot) + " beyond the " + std::to_string(n_pods()) + " pods of the usage configuration";
      if (r.flags & ~(uint32_t)(KWK_USAGE_ROW_RESET | KWK_USAGE_ROW_CREATED)) return at + "unknown flags";
      if (r.usage_key >> 28) {
        if (!key_ids_ok(r.usage_key)) return at + "usage_key value id out of range (slot " + std::to_string(r.slot) + ")";
      } else {
        if (!mixed_tables || (r.usage_key & kMixedIndex) >= n_mixed())
          return at + "usage_key mixed index out of range (slot " + std::to_string(r.slot) + ")";
        worst += key_containers(r.usage_key);
      }
      seen[i] = {r.slot, i};
    }
    if (worst > 0xFFFFFFFFull) return "more than 2^32 containers of mixed pods";
    std::sort(seen.begin(), seen.end());
    for (uint32_t i = 1; i < n; ++i)
      if (seen[i].first == seen[i - 1].first)
        return "row " + std::to_string(seen[i].second) + ": slot " + std::to_string(seen[i].first) + " named twice (row " +
               std::to_string(seen[i - 1].second) + ")";
    out.reserve(n);
    for (uint32_t i = 0; i < n; ++i) {
      const kwk_usage_row& r = rows[i];
      const uint32_t s = r.slot, ko = ukey[s], kn = r.usage_key;
      const uint32_t nco = containers(s), ncn = key_containers(kn);
      const bool reset = (r.flags & KWK_USAGE_ROW_RESET) != 0, was_mixed = !(ko >> 28);
      DevRow d{};
      d.slot = s;
      d.key = kn;
      if (reset) d.flags |= kDevReset;
      if (r.flags & KWK_USAGE_ROW_CREATED) d.flags |= kDevCreated, d.created = r.created_ns;
      if (nco != ncn) fx.layout_changed = true;
      if (ko != kn) release(ko), acquire(kn), ukey[s] = kn;
      if (!(kn >> 28)) {  // a mixed pod: its containers' integrators
        // RESET: the range starts at 0.  A mixed pod that goes on keeps its first containers' totals;
        // a uniform pod that goes on gives each of its containers the total they shared
        const bool seed = !reset && !was_mixed;
        const uint32_t kept = reset ? 0u : std::min(nco, ncn);
        if (seed) d.flags |= kDevSeedUnit;
        if (mcap[s] >= ncn) {  // the slot's range is large enough
          d.mbase = d.copy_from = mbase[s];
          if (reset || seed || ncn > nco) d.flags |= kDevRange, d.range_n = ncn, d.copy_n = kept;  // further containers start at 0
        } else {               // a new range at the end
          d.copy_from = mbase[s];
          d.copy_n = kept;
          d.mbase = mbase[s] = (uint32_t)ccum_end;
          mcap[s] = ncn;
          ccum_end += ncn;
          d.flags |= kDevRange;
          d.range_n = ncn;
        }
        d.flags |= kDevMbase;
      } else if (was_mixed && !reset) {
        d.flags |= kDevZeroUnit;
      }
      if (key8) {
        if (!(kn >> 28)) {
          drop_dict(), fx.key8_dropped = true;
        } else {
          Ref& ref = keys[kn];
          if (ref.idx < 0) {
            if (!dict_free.empty()) {
              ref.idx = (int32_t)dict_free.back(), dict_free.pop_back();
              dict[ref.idx] = kn;
            } else if (dict.size() < kDictMax) {
              ref.idx = (int32_t)dict.size(), dict.push_back(kn);
            }
            if (ref.idx >= 0) fx.kv_set.push_back((uint32_t)ref.idx);
          }
          if (ref.idx < 0) drop_dict(), fx.key8_dropped = true;  // the 256th distinct key
          else d.flags |= kDevKey8, d.k8 = (uint32_t)ref.idx;
        }
      }
      out.push_back(d);
    }
    if (fx.key8_dropped) fx.kv_set.clear();
    return "";
  }

  // kwk_relayout: the mirrors permuted by the slot runs (checked by relayout::check_moves: sorted
  // by dst, disjoint, inside the old and the new pods), slots no run covers given fresh_key, pods
  // no run names released — a dropped mixed pod's range is abandoned.  What is derived stays what
  // configure() of the final columns derives; the dictionary keeps its entries' numbers (the device's
  // 1-byte column moves as it is), frees those of keys out of use and gives fresh_key one, or ends
  // as in apply() when that is a 256th distinct key.  *fresh_k8: fresh_key's entry while the
  // dictionary lives.  "" or what is wrong with fresh_key; the book is unchanged then.
  std::string relayout(const kwk_move* moves, uint32_t n_moves, uint32_t n_new, uint32_t fresh_key, Effects& fx,
                       uint32_t* fresh_k8) {
    fx = Effects{};
    if (fresh_k8) *fresh_k8 = 0;
    if (!(fresh_key >> 28)) return "fresh_usage_key " + std::to_string(fresh_key) + ": a mixed key (0 containers)";
    if (!key_ids_ok(fresh_key)) return "fresh_usage_key " + std::to_string(fresh_key) + ": value id out of range";
    const uint32_t n_old = n_pods();
    // slots [0, keep) stay where they are (a prefix of identity runs without a gap): only what lies
    // past it is copied and counted, so appending nodes costs the new slots alone.  The sources of
    // the other runs lie past the prefix too (runs are disjoint in src).
    uint32_t keep = 0, first = 0;
    for (; first < n_moves; ++first) {
      const kwk_move& m = moves[first];
      if (m.n && (m.dst != keep || m.src != keep)) break;
      keep += m.n;
    }
    const size_t tail_new = (size_t)n_new - keep, tail_old = (size_t)n_old - keep;
    std::vector<uint32_t> nk(tail_new, fresh_key), nb, nc;
    if (mixed_tables) nb.assign(tail_new, 0u), nc.assign(tail_new, 0u);
    std::vector<uint8_t> named(tail_old, 0);
    uint64_t covered = keep;
    for (uint32_t i = first; i < n_moves; ++i) {
      const kwk_move& m = moves[i];
      if (!m.n) continue;
      std::copy(ukey.begin() + m.src, ukey.begin() + m.src + m.n, nk.begin() + (m.dst - keep));
      if (mixed_tables) {
        std::copy(mbase.begin() + m.src, mbase.begin() + m.src + m.n, nb.begin() + (m.dst - keep));
        std::copy(mcap.begin() + m.src, mcap.begin() + m.src + m.n, nc.begin() + (m.dst - keep));
      }
      std::fill(named.begin() + (m.src - keep), named.begin() + (m.src - keep) + m.n, (uint8_t)1);
      covered += m.n;
    }
    for (size_t q = 0; q < tail_old; ++q)
      if (!named[q]) release(ukey[keep + q]);
    const uint64_t fresh = (uint64_t)n_new - covered;
    if (fresh) {
      nc_hist[fresh_key >> 28] += fresh;
      Ref& ref = keys[fresh_key];
      ref.count += fresh;
      if (key8 && ref.idx < 0) {
        if (!dict_free.empty()) {
          ref.idx = (int32_t)dict_free.back(), dict_free.pop_back();
          dict[ref.idx] = fresh_key;
        } else if (dict.size() < kDictMax) {
          ref.idx = (int32_t)dict.size(), dict.push_back(fresh_key);
        }
        if (ref.idx >= 0) fx.kv_set.push_back((uint32_t)ref.idx);
        else drop_dict(), fx.key8_dropped = true;  // the 256th distinct key
      }
      if (key8 && fresh_k8) *fresh_k8 = (uint32_t)ref.idx;
    }
    auto retail = [&](std::vector<uint32_t>& col, const std::vector<uint32_t>& tail) {
      col.resize(keep);
      col.insert(col.end(), tail.begin(), tail.end());
    };
    retail(ukey, nk);
    if (mixed_tables) retail(mbase, nb), retail(mcap, nc);
    if (key8 && ukey.empty()) drop_dict(), fx.key8_dropped = true;  // (no pods: no column, as configure())
    fx.layout_changed = true;  // cptr follows the slots whatever the counts
    return "";
  }
};

}  // namespace usage_rows
