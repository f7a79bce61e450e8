// Device patch emission (include/kwok_emit.h): the merge-patch bytes of a step's fired objects,
// expanded from per-(class, template) skeletons on the engine's stream.
//
// Reference: playStage renders each fired object's Stage patches (pkg/utils/lifecycle/
// next.go:73-160, pkg/utils/gotpl/renderer.go:59-124) — here the host's one-time skeleton build
// (patch.cpp: kwk_patch_skeleton / kwk_patch_object_values) leaves only Now and the objects' call
// values (funcPodIPWith / funcNodeIPWith, pod_controller.go:563-600) to fill per fire.
//
// Three launches per list, sized by the device-resident record count (no host round trip):
//   emit_size_kernel   per 256-record tile (one per thread): items and bytes (a gather of one 8-byte
//                      word per record)
//   emit_scan_kernel   one workgroup: exclusive bases of the tiles, the totals
//   emit_write_kernel  per tile again: each record's items / offsets, its guard word, then each wave
//                      writes its 64 records' bytes (one contiguous span), 64 lanes over every literal
//                      run and value, through an LDS window that leaves as 16-byte stores
// A 2-byte ring list (kwk_emit_step of a KWK_COMPACT_PACKED16 slot) takes two more, before the size
// kernel: emit_seg_base_kernel (the exclusive prefix of the records per segment) and
// emit_tile_seg_kernel (every tile's first segment), from which the size and write kernels find each
// record's segment, hence its slot.  Emissions rotate through output sets (kwk_emit_reserve_sets), so
// the emissions of a fused group are enqueued back to back; a device flag stops the ones behind an
// emission that exceeded its set.
// With a finalizer program (kwk_emit_finalizers_load) three more per emission write the fired
// objects' finalizer JSON patches into a stream of their own: emit_fin_size_kernel and
// emit_scan_kernel over its tile arrays between the merge patches' scan and writer (an overflow of
// either stream stops both writers), emit_fin_write_kernel last ("finalizer patches" below).
// The skeleton pieces and literal runs are staged in LDS when they fit (12 KiB of literals).
// Roofline: HBM-bound on the patch bytes written (plus 8 bytes read per record and the literal
// runs, L2-resident); the byte copy is 1-byte stores coalesced per wave.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/kwok_emit.h"
#include "../../include/kwok_events.h"
#include "errscope.hpp"
#include "devmem.hpp"
#include "timefmt.hpp"

namespace {

constexpr uint32_t kBlock = 256, kTile = kBlock;  // records per tile: one per thread, 64 per wave
constexpr uint32_t kWaves = kBlock / 64, kWaveRecs = kTile / kWaves;
constexpr uint32_t kMaxStageTpl = 16;  // templates of one stage (an item mask per record)
constexpr uint32_t kScanBlock = 1024;
constexpr uint32_t kNowWords = 10;      // Now() text (< 40 bytes) as dwords in LDS
constexpr uint32_t kLdsPieces = 256;    // skeleton tables staged in LDS when they fit
constexpr uint32_t kLdsLits = 8192;
constexpr uint32_t kLdsSkels = 64;
constexpr uint32_t kRecSk = 4;          // skeletons of a record's emitted items kept in LDS (more: looked up)

struct Prog {
  const uint32_t* stage_tpl_ptr;
  const uint16_t* stage_tpl;
  const uint8_t* stage_delete;
  const int32_t* skel_of;
  const kwk_emit_skel* skels;
  const kwk_emit_piece* pieces;
  const char* lits;
  const uint8_t* fresh;
  uint8_t* const* cols;
  const uint32_t* stride;
  uint32_t n_classes, n_templates, n_stages, n_pieces;
  uint32_t n_lits, n_cols, n_skels;
};

struct EmitArgs {
  Prog p;
  const kwk_fired_rec* recs;  // or
  const uint32_t* packed;
  const uint32_t* count;
  uint64_t* words;
  uint32_t capacity;
  uint32_t max_recs;                 // records the tile arrays cover (capacity rounded up)
  uint32_t* tile_items;              // per tile: items, then (emit_scan_kernel) the exclusive base
  unsigned long long* tile_bytes;    // per tile: bytes, then the base
  unsigned long long* totals;        // [0] items, [1] bytes, [2] the list is longer than max_recs, [3] items emitted
  kwk_emit_item* items;
  uint64_t* offsets;
  char* out;
  unsigned long long cap_items, cap_bytes;
  uint32_t now_len;
  char now[40];
  uint32_t lencache;                 // words' bits 24-31 cache the value lengths (emit_lens_kernel)
  // several emissions in flight (kwk_emit_reserve_sets): nonzero once an emission exceeded its set —
  // every kernel of the later ones then leaves at once (totals[4] = 1); sticky_on: this emission sets it
  uint32_t* sticky;
  uint32_t sticky_on;
  // the 2-byte source (kSrc16: a KWK_COMPACT_PACKED16 ring list): the records, the records per segment,
  // their exclusive prefix seg_base[n_segs + 1] (emit_seg_base_kernel) and each tile's first record's
  // segment tile_seg (emit_tile_seg_kernel)
  const uint16_t* p16;
  const uint32_t* seg_counts;
  uint32_t* seg_base;
  uint32_t* tile_seg;
  uint32_t n_segs, region_slots;
};

constexpr uint32_t kSrc32 = 0, kSrc16 = 1;  // the list's records: kwk_fired_rec / 4-byte packed | 2-byte
// the records of the list the tile arrays cover
template <uint32_t kSrc>
__device__ __forceinline__ uint32_t list_len(const EmitArgs& a) {
  const uint32_t n = min(*a.count, a.max_recs);
  if constexpr (kSrc == kSrc16) return min(n, a.seg_base[a.n_segs]);  // (no record without a segment)
  return n;
}

// per skeleton (LDS, built per block for this call's Now length): x = its fixed bytes (literal runs
// and Now) | value slots << 24 (kSkszPieces: more than 4, count them piece by piece), y = the slots'
// value columns, a byte each
constexpr uint32_t kSkszPieces = 0xFFu;
__device__ __forceinline__ void build_sksz(const EmitArgs& a, const kwk_emit_piece* pieces, uint2* sksz) {
  for (uint32_t k = threadIdx.x; k < a.p.n_skels && k < kLdsSkels; k += blockDim.x) {
    const kwk_emit_skel S = a.p.skels[k];
    uint32_t fixed = 0, nv = 0, cols = 0;
    for (uint32_t q = 0; q < S.n_pieces; ++q) {
      const kwk_emit_piece P = pieces[S.first_piece + q];
      fixed += P.lit_len + (P.slot == 0 ? a.now_len : 0u);
      if (P.slot != 0 && P.slot != KWK_EMIT_NO_SLOT) {
        if (nv < 4u) cols |= (uint32_t)(P.slot - 1u) << (8u * nv);
        ++nv;
      }
    }
    sksz[k] = make_uint2(nv > 4u || fixed >= (1u << 24) ? kSkszPieces << 24 : fixed | nv << 24, cols);
  }
}

// the skeleton pieces and literal runs a kernel reads: LDS copies when the program's fit
struct Tables {
  const kwk_emit_piece* pieces;
  const char* lits;
  const uint2* sksz = nullptr;  // per-skeleton sizes (build_sksz), when staged
};

template <bool kLds, bool kLits = true>
__device__ __forceinline__ Tables stage_tables(const EmitArgs& a, kwk_emit_piece* s_pieces, uint32_t* s_lits,
                                               uint2* s_sksz) {
  if constexpr (kLds) {
    for (uint32_t j = threadIdx.x; j < a.p.n_pieces; j += blockDim.x) s_pieces[j] = a.p.pieces[j];
    build_sksz(a, a.p.pieces, s_sksz);
    if constexpr (!kLits) {  // the literal runs stay in global memory
      __syncthreads();
      return Tables{s_pieces, a.p.lits, s_sksz};
    }
    const uint32_t nw = (a.p.n_lits + 3u) / 4u;
    for (uint32_t j = threadIdx.x; j < nw; j += blockDim.x) {
      uint32_t w = 0;
      for (uint32_t b = 0; b < 4u; ++b)
        if (4u * j + b < a.p.n_lits) w |= (uint32_t)(uint8_t)a.p.lits[4u * j + b] << (8u * b);
      s_lits[j] = w;
    }
    __syncthreads();
    return Tables{s_pieces, reinterpret_cast<const char*>(s_lits), s_sksz};
  } else {
    return Tables{a.p.pieces, a.p.lits, nullptr};
  }
}

struct Rec {
  uint32_t slot, stage;
  bool valid;
};

__device__ __forceinline__ Rec fetch(const EmitArgs& a, uint32_t r) {
  Rec x;
  if (a.packed) {
    const uint32_t v = a.packed[r];
    x.slot = v & 0x7FFFFFFu;
    x.stage = v >> 27;
  } else {
    const kwk_fired_rec f = a.recs[r];
    x.slot = f.slot;
    x.stage = f.stage;
  }
  x.valid = x.slot < a.capacity;
  return x;
}

// ---- the 2-byte source: which segment a dense record belongs to.  A 2-byte record holds the
// offset inside its segment; record r of the dense list belongs to the segment s with
// seg_base[s] <= r < seg_base[s + 1] (the upper bound of r: it steps over empty segments, equal
// neighbours, and runs of them).  A tile is kTile consecutive records, so its records' segments are
// the range from its first record's segment (tile_seg[t], written once per list by
// emit_tile_seg_kernel: no search) to the next tile's first record's (the list's last segment for
// the last tile): seg_base over that range goes to LDS when it is at most kSegWin entries, and each
// record's binary search runs over that copy — over global memory otherwise, in both cases over the
// tile's own range only.
constexpr uint32_t kSegWin = 264;
struct SegWin {
  const uint32_t* base;  // seg_base + s0, or null: the LDS copy
  uint32_t s0, n;        // entries [0, n]: segments s0 .. s0 + n - 1
};
// (LDS of the 2-byte instantiations only: a function's static, allocated where it is called)
__device__ __forceinline__ uint32_t* seg_win_lds() {
  __shared__ uint32_t w[kSegWin];
  return w;
}

// every thread of the block, once per tile (block-uniform control flow; a barrier inside)
__device__ __forceinline__ SegWin tile_segs(const EmitArgs& a, uint32_t t, uint32_t n, uint32_t* s_win) {
  const uint32_t last = a.n_segs - 1u;
  const uint32_t s0 = min(a.tile_seg[t], last);
  const uint32_t s1 = max(s0, (t + 1u) * kTile < n ? min(a.tile_seg[t + 1u], last) : last);
  const uint32_t cnt = s1 - s0 + 1u;
  if (cnt < kSegWin) {
    for (uint32_t j = threadIdx.x; j <= cnt; j += blockDim.x) s_win[j] = a.seg_base[s0 + j];
    __syncthreads();
    return SegWin{nullptr, s0, cnt};
  }
  return SegWin{a.seg_base + s0, s0, cnt};
}

template <typename P>
__device__ __forceinline__ uint32_t seg_search(P base, uint32_t n, uint32_t r) {
  uint32_t lo = 0, hi = n;  // base[lo] <= r < base[hi]
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (base[mid] <= r) lo = mid;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ Rec fetch16(const EmitArgs& a, uint32_t r, const SegWin& w, const uint32_t* s_win) {
  const uint32_t v = a.p16[r];
  const uint32_t s = w.s0 + (w.base ? seg_search(w.base, w.n, r) : seg_search(s_win, w.n, r));
  Rec x;
  x.slot = s * a.region_slots + KWK_FIRED16_SLOT(v);
  x.stage = KWK_FIRED16_STAGE(v);
  x.valid = x.slot < a.capacity;
  return x;
}

// where a record's call values are read: the value columns in global memory, or the rows the
// write kernel staged in LDS for the tile (kLdsCols columns of 16 bytes)
constexpr uint32_t kLdsCols = 2;
struct Vals {
  const uint8_t* lds;  // [kLdsCols][kTile][16] or null
  uint32_t lr;         // the record's index in the tile
  uint32_t lens = 0xFFu;  // the word's cached value lengths (kLenCache): column 0 | column 1 << 4; 0xFF: none
  __device__ __forceinline__ const uint8_t* row(const EmitArgs& a, uint32_t c, uint32_t slot) const {
    if (lds) return lds + ((uint64_t)c * kTile + lr) * 16u;
    return a.p.cols[c] + (uint64_t)slot * a.p.stride[c];
  }
  // a value's length byte (0xFF: unusable), from the cache when the word holds it
  __device__ __forceinline__ uint32_t len(const EmitArgs& a, uint32_t c, uint32_t slot) const {
    if (lens != 0xFFu && c < 2u) return c ? lens >> 4 : lens & 15u;
    return row(a, c, slot)[0];
  }
};

// Cached value lengths: with at most two value columns of 16-byte rows, a slot's word keeps both
// rows' text lengths in bits 24-31 (column 0 | column 1 << 4; 0xFF when either is unusable or both
// are 15, i.e. "read the rows"), refreshed by the host entry points that write words or rows, so
// that the size kernel gathers one word per record instead of the word and two rows
__global__ void emit_lens_kernel(uint64_t* __restrict__ words, uint8_t* const* __restrict__ cols, uint32_t n_cols,
                                 uint32_t first, uint32_t n) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint64_t s = (uint64_t)first + i;
    const uint32_t l0 = n_cols > 0 ? cols[0][s * 16u] : 0u, l1 = n_cols > 1 ? cols[1][s * 16u] : 0u;
    const uint32_t code = (l0 <= 15u && l1 <= 15u) ? (l0 | l1 << 4) : 0xFFu;
    words[s] = (words[s] & ~(0xFFull << 24)) | (uint64_t)code << 24;
  }
}

// bytes of skeleton k for this slot, or -1 when a value is unusable
__device__ __forceinline__ long long skel_bytes(const EmitArgs& a, const Tables& T, uint32_t k, uint32_t slot,
                                                const Vals& V = Vals{nullptr, 0}) {
  if (T.sksz) {
    const uint2 z = T.sksz[k];
    const uint32_t nv = z.x >> 24;
    if (nv != kSkszPieces) {
      long long b = z.x & 0xFFFFFFu;
      for (uint32_t i = 0; i < nv; ++i) {
        const uint32_t len = V.len(a, (z.y >> (8u * i)) & 0xFFu, slot);
        if (len == 0xFFu) return -1;
        b += len;
      }
      return b;
    }
  }
  const kwk_emit_skel S = a.p.skels[k];
  long long b = 0;
  for (uint32_t q = 0; q < S.n_pieces; ++q) {
    const kwk_emit_piece P = T.pieces[S.first_piece + q];
    b += P.lit_len;
    if (P.slot == 0) {
      b += a.now_len;
    } else if (P.slot != KWK_EMIT_NO_SLOT) {
      const uint32_t len = V.len(a, P.slot - 1u, slot);
      if (len == 0xFFu) return -1;
      b += len;
    }
  }
  return b;
}

__device__ __forceinline__ int skel_index(const EmitArgs& a, uint64_t w, uint32_t tid) {
  const uint32_t cls = (uint32_t)(w & 0xFFFFu), g = (uint32_t)(w >> 16) & 0xFFu;
  if (cls >= a.p.n_classes || tid >= 32u || !((w >> (32u + tid)) & 1u)) return -1;
  const int k = a.p.skel_of[cls * a.p.n_templates + tid];
  if (k < 0) return -1;
  const uint32_t need = a.p.skels[k].need;
  return (g & need) == need ? k : -1;
}

struct Size {
  uint32_t items, ok;  // ok: bit j = the stage's j-th template is emitted here
  unsigned long long bytes;
};

__device__ __forceinline__ Size rec_size(const EmitArgs& a, const Tables& T, const Rec& x, uint64_t w,
                                         const Vals& V = Vals{nullptr, 0}) {
  Size s{0u, 0u, 0ull};
  if (x.stage >= a.p.n_stages) return s;
  const uint32_t t0 = a.p.stage_tpl_ptr[x.stage], t1 = a.p.stage_tpl_ptr[x.stage + 1];
  for (uint32_t j = t0; j < t1; ++j) {
    ++s.items;
    const int k = x.valid ? skel_index(a, w, a.p.stage_tpl[j]) : -1;
    if (k < 0) continue;
    const long long b = skel_bytes(a, T, (uint32_t)k, x.slot, V);
    if (b < 0) continue;
    s.ok |= 1u << (j - t0);
    s.bytes += (unsigned long long)b;
  }
  return s;
}

// One lane's output stream (a record written by the thread that sized it), assembled four bytes
// at a time in a 16-byte register window {lo, hi}: every append is one shifted OR at the window's
// byte position (no per-byte work), a full window leaves as one 16-byte store.  The stream starts
// at global byte g0: the window starts with g0 & 15 phantom bytes, so that every store is 16-byte
// aligned; the first window (it shares its 16 bytes with the record before) and the last one (the
// record after) are written with dword and byte stores covering exactly the record's bytes.
struct Acc {
  char* out;
  unsigned long long w0;  // global position of the window's byte 0 (16-byte aligned)
  uint64_t lo, hi;
  uint32_t n;             // bytes in the window (incl. the phantom head)
  uint32_t head;          // phantom bytes of the first window (0 once it has left)
  __device__ __forceinline__ Acc(char* o, unsigned long long g0)
      : out(o), w0(g0 & ~15ull), lo(0), hi(0), n((uint32_t)(g0 & 15u)), head((uint32_t)(g0 & 15u)) {}
  // bytes [b0, b1) of the window at w0, for a window shared with a neighbouring record
  __device__ __forceinline__ void partial(uint32_t b0, uint32_t b1) const {
    for (uint32_t b = b0; b < b1;) {
      const uint64_t v = b < 8u ? lo : hi;
      const uint32_t sh = 8u * (b & 7u);
      if ((b & 3u) == 0u && b + 4u <= b1) {
        *reinterpret_cast<uint32_t*>(out + w0 + b) = (uint32_t)(v >> sh);
        b += 4u;
      } else {
        out[w0 + b] = (char)((v >> sh) & 0xFFu);
        ++b;
      }
    }
  }
  __device__ __forceinline__ void flush_full() {
    if (head) {
      partial(head, 16u);
      head = 0;
    } else {
      *reinterpret_cast<uint4*>(out + w0) = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
    }
  }
  // `cnt` (1..4) bytes, low byte first; w's bytes above cnt are zero
  __device__ __forceinline__ void put(uint32_t w, uint32_t cnt) {
    const uint64_t x = (uint64_t)w;
    const uint32_t sh = 8u * n;  // 0..120
    if (sh < 64u) {
      lo |= x << sh;
      hi |= sh > 32u ? x >> (64u - sh) : 0ull;
    } else {
      hi |= x << (sh - 64u);
    }
    const uint64_t spill = sh > 96u ? x >> (128u - sh) : 0ull;  // bytes past the window
    n += cnt;
    if (n >= 16u) {
      flush_full();
      w0 += 16u;
      lo = spill;
      hi = 0;
      n -= 16u;
    }
  }
  __device__ __forceinline__ void finish() const { partial(head, n); }
};

__device__ __forceinline__ uint32_t low_bytes(uint32_t w, uint32_t cnt) {
  return cnt >= 4u ? w : w & ((1u << (8u * cnt)) - 1u);
}

// `len` bytes starting at byte `off` of a dword array (aligned dword reads, one per step, joined by
// alignbyte): the literal runs (LDS or global, 16 bytes of zero padding after them), Now (LDS) and
// a value row's text (byte 1 on)
__device__ __forceinline__ void put_run(Acc& o, const uint32_t* __restrict__ src, uint32_t off, uint32_t len) {
  if (!len) return;
  uint32_t d = off >> 2;
  const uint32_t sh = off & 3u;
  uint32_t cur = src[d];
  for (uint32_t k = 0; k < len; k += 4u) {
    const uint32_t nxt = src[d + 1u];
    const uint32_t w = sh ? __builtin_amdgcn_alignbyte(nxt, cur, sh) : cur;
    const uint32_t cnt = min(4u, len - k);
    o.put(low_bytes(w, cnt), cnt);
    cur = nxt;
    ++d;
  }
}

// one emitted item by one lane
__device__ __forceinline__ void lane_skel(const EmitArgs& a, const Tables& T, const kwk_emit_skel& S, uint32_t slot,
                                          const uint32_t* s_now, const Vals& V, Acc& o) {
  const uint32_t* L = reinterpret_cast<const uint32_t*>(T.lits);
  for (uint32_t q = 0; q < S.n_pieces; ++q) {
    const kwk_emit_piece P = T.pieces[S.first_piece + q];
    put_run(o, L, P.lit_off, P.lit_len);
    if (P.slot == 0) {
      put_run(o, s_now, 0u, a.now_len);
    } else if (P.slot != KWK_EMIT_NO_SLOT) {
      const uint8_t* v = V.row(a, P.slot - 1u, slot);  // [length][text]: rows 16-byte aligned in LDS, 4 in global
      const uint32_t* v32 = reinterpret_cast<const uint32_t*>(v);
      put_run(o, v32, 1u, (uint32_t)(v32[0] & 0xFFu));
    }
  }
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <typename T>
__device__ __forceinline__ T wave_incl(T v, uint32_t lane) {
  for (int o = 1; o < 64; o <<= 1) {
    const T y = __shfl_up(v, o);
    if (lane >= (uint32_t)o) v += y;
  }
  return v;
}

template <bool kLds, uint32_t kSrc = kSrc32>
__global__ __launch_bounds__(kBlock) void emit_size_kernel(EmitArgs a) {
  __shared__ kwk_emit_piece s_pieces[kLds ? kLdsPieces : 1];
  __shared__ uint32_t s_lits[kLds ? kLdsLits / 4 : 1];
  __shared__ uint2 s_sksz[kLds ? kLdsSkels : 1];
  __shared__ uint32_t s_i[kWaves];
  __shared__ unsigned long long s_b[kWaves];
  if (*a.sticky) return;  // an earlier emission in flight exceeded its set
  const Tables T = stage_tables<kLds>(a, s_pieces, s_lits, s_sksz);
  const uint32_t n = list_len<kSrc>(a), n_tiles = (n + kTile - 1) / kTile;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t* s_win = nullptr;
  if constexpr (kSrc == kSrc16) s_win = seg_win_lds();
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    uint32_t it = 0;
    unsigned long long by = 0;
    const uint32_t r = t * kTile + threadIdx.x;
    SegWin sw{};
    if constexpr (kSrc == kSrc16) sw = tile_segs(a, t, n, s_win);
    if (r < n) {
      Rec x;
      if constexpr (kSrc == kSrc16) x = fetch16(a, r, sw, s_win);
      else x = fetch(a, r);
      const uint64_t w = x.valid ? a.words[x.slot] : 0ull;
      const Size s = rec_size(a, T, x, w, Vals{nullptr, 0u, a.lencache ? (uint32_t)(w >> 24) & 0xFFu : 0xFFu});
      it = s.items;
      by = s.bytes;
    }
    it = wave_sum(it);
    by = wave_sum(by);
    if (lane == 0) {
      s_i[wave] = it;
      s_b[wave] = by;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t ti = 0;
      unsigned long long tb = 0;
      for (uint32_t w = 0; w < kWaves; ++w) {
        ti += s_i[w];
        tb += s_b[w];
      }
      a.tile_items[t] = ti;
      a.tile_bytes[t] = tb;
    }
    __syncthreads();
  }
}

// 8 consecutive tiles per thread: 8192 tiles per pass of the one workgroup
constexpr uint32_t kScanPer = 8;
__global__ __launch_bounds__(kScanBlock) void emit_scan_kernel(EmitArgs a) {
  __shared__ uint32_t s_i[kScanBlock / 64];
  __shared__ unsigned long long s_b[kScanBlock / 64];
  if (*a.sticky) {  // nothing was sized: this emission reads KWK_ECAP too
    if (threadIdx.x < 5u) a.totals[threadIdx.x] = threadIdx.x == 4u ? 1ull : 0ull;
    return;
  }
  const uint32_t n = a.p16 ? list_len<kSrc16>(a) : list_len<kSrc32>(a), n_tiles = (n + kTile - 1) / kTile;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t run_i = 0;
  unsigned long long run_b = 0;
  for (uint32_t base = 0; base < n_tiles; base += kScanBlock * kScanPer) {
    const uint32_t t0 = base + threadIdx.x * kScanPer;
    uint32_t vi[kScanPer];
    unsigned long long vb[kScanPer];
    uint32_t si = 0;
    unsigned long long sb = 0;
#pragma unroll
    for (uint32_t k = 0; k < kScanPer; ++k) {
      vi[k] = t0 + k < n_tiles ? a.tile_items[t0 + k] : 0u;
      vb[k] = t0 + k < n_tiles ? a.tile_bytes[t0 + k] : 0ull;
      si += vi[k];
      sb += vb[k];
    }
    const uint32_t ii = wave_incl(si, lane);
    const unsigned long long ib = wave_incl(sb, lane);
    if (lane == 63) {
      s_i[wave] = ii;
      s_b[wave] = ib;
    }
    __syncthreads();
    uint32_t pi = 0, ti = 0;
    unsigned long long pb = 0, tb = 0;
    for (uint32_t w = 0; w < kScanBlock / 64; ++w) {
      if (w < wave) {
        pi += s_i[w];
        pb += s_b[w];
      }
      ti += s_i[w];
      tb += s_b[w];
    }
    uint32_t ei = run_i + pi + ii - si;
    unsigned long long eb = run_b + pb + ib - sb;
#pragma unroll
    for (uint32_t k = 0; k < kScanPer; ++k) {
      if (t0 + k < n_tiles) {
        a.tile_items[t0 + k] = ei;
        a.tile_bytes[t0 + k] = eb;
      }
      ei += vi[k];
      eb += vb[k];
    }
    run_i += ti;
    run_b += tb;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    a.totals[0] = run_i;
    a.totals[1] = run_b;
    a.totals[2] = *a.count > a.max_recs ? 1ull : 0ull;
    a.totals[3] = 0;
    a.totals[4] = 0;
    if (a.sticky_on && (run_i > a.cap_items || run_b > a.cap_bytes || a.totals[2])) *a.sticky = 1u;
  }
}

// The 2-byte source's segment bases, once per emission before the size kernel: the exclusive prefix
// of the list's records per segment (~49k segments at 100M pods), one workgroup as emit_scan_kernel
__global__ __launch_bounds__(kScanBlock) void emit_seg_base_kernel(EmitArgs a) {
  __shared__ uint32_t s_w[kScanBlock / 64];
  if (*a.sticky) return;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t run = 0;
  for (uint32_t base = 0; base < a.n_segs; base += kScanBlock * kScanPer) {
    const uint32_t t0 = base + threadIdx.x * kScanPer;
    uint32_t v[kScanPer], s = 0;
#pragma unroll
    for (uint32_t k = 0; k < kScanPer; ++k) {
      v[k] = t0 + k < a.n_segs ? a.seg_counts[t0 + k] : 0u;
      s += v[k];
    }
    const uint32_t incl = wave_incl(s, lane);
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    uint32_t p = 0, tot = 0;
    for (uint32_t w = 0; w < kScanBlock / 64; ++w) {
      if (w < wave) p += s_w[w];
      tot += s_w[w];
    }
    uint32_t e = run + p + incl - s;
#pragma unroll
    for (uint32_t k = 0; k < kScanPer; ++k) {
      if (t0 + k < a.n_segs) a.seg_base[t0 + k] = e;
      e += v[k];
    }
    run += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) a.seg_base[a.n_segs] = run;
}

// ... and the segment of every tile's first record: segment s owns the tile starts inside
// [seg_base[s], seg_base[s + 1]) (at most 1 + its records / kTile of them; each tile start once)
__global__ __launch_bounds__(kBlock) void emit_tile_seg_kernel(EmitArgs a) {
  if (*a.sticky) return;
  const uint32_t t_max = a.max_recs / kTile;  // tile_seg holds t_max + 1 entries
  for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < a.n_segs; s += gridDim.x * blockDim.x) {
    const uint32_t b0 = a.seg_base[s], b1 = a.seg_base[s + 1u];
    for (uint32_t t = (b0 + kTile - 1u) / kTile; t <= t_max && t * kTile < b1; ++t) a.tile_seg[t] = s;
  }
}

// ---- the chunk writer (the default when the program's tables fit in LDS) ----
// Per call, every block renders each skeleton once into an LDS template with Now filled in:
// consecutive literal runs and Now slots merge into one template run, so a skeleton is a short
// list of segments (template run | value column c).  A record's bytes are the concatenation of its
// items' segments; the thread that sized the record writes it as aligned 16-byte chunks: each chunk
// gathers the bytes of the segments overlapping it (16 unaligned bytes from LDS: five aligned dword
// reads joined by alignbyte, merged under a byte mask), and leaves as one 16-byte store.  The first
// and the last chunk of a record share their 16 bytes with the neighbouring records: they are
// written at the end with dword / byte stores covering exactly the record's bytes.  Every store
// goes through a buffer resource with the offset out of range where a lane has nothing to store,
// so no store sits under a divergent branch.
constexpr uint32_t kTplBytes = 8192;                     // rendered templates in LDS
constexpr uint32_t kMaxSegs = 2 * kLdsPieces + kLdsSkels;  // segments of every skeleton
constexpr uint32_t kSegValue = 1u << 24;                 // segment kind: value column (y >> 24) - 1
constexpr uint32_t kOOB = 0x80000000u;                   // buffer offset past the resource: no store

typedef __attribute__((address_space(3))) uint32_t lds_u32;
typedef __attribute__((address_space(3))) uint8_t lds_u8;
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
  return (uint32_t)(size_t)(const __attribute__((address_space(3))) uint8_t*)p;
}
__device__ __forceinline__ uint32_t lds_rd(uint32_t a) { return *(const lds_u32*)(size_t)a; }

// the 16 bytes at LDS byte address A (any alignment; bytes outside the arrays are don't-care)
__device__ __forceinline__ void lds_load16(uint32_t A, uint32_t (&y)[4]) {
  const uint32_t d = A & ~3u, sh = A & 3u;
  const uint32_t w0 = lds_rd(d), w1 = lds_rd(d + 4u), w2 = lds_rd(d + 8u), w3 = lds_rd(d + 12u), w4 = lds_rd(d + 16u);
  y[0] = __builtin_amdgcn_alignbyte(w1, w0, sh);
  y[1] = __builtin_amdgcn_alignbyte(w2, w1, sh);
  y[2] = __builtin_amdgcn_alignbyte(w3, w2, sh);
  y[3] = __builtin_amdgcn_alignbyte(w4, w3, sh);
}

// a if bit is 0, b if 1 (bit: 0 or 1)
__device__ __forceinline__ uint32_t blend(uint32_t a, uint32_t b, uint32_t bit) { return a ^ ((a ^ b) & (0u - bit)); }

// byte mask of [lo, hi) (0 <= lo <= hi <= 16) as two 64-bit halves
__device__ __forceinline__ uint64_t ones_bytes(uint32_t n) { return n >= 8u ? ~0ull : (1ull << (8u * n)) - 1ull; }
__device__ __forceinline__ void merge16(uint32_t (&x)[4], const uint32_t (&y)[4], uint32_t lo, uint32_t hi) {
  const uint64_t ml = ones_bytes(min(hi, 8u)) & ~ones_bytes(min(lo, 8u));
  const uint64_t mh = ones_bytes(hi > 8u ? hi - 8u : 0u) & ~ones_bytes(lo > 8u ? lo - 8u : 0u);
  x[0] = (y[0] & (uint32_t)ml) | (x[0] & ~(uint32_t)ml);
  x[1] = (y[1] & (uint32_t)(ml >> 32)) | (x[1] & ~(uint32_t)(ml >> 32));
  x[2] = (y[2] & (uint32_t)mh) | (x[2] & ~(uint32_t)mh);
  x[3] = (y[3] & (uint32_t)(mh >> 32)) | (x[3] & ~(uint32_t)(mh >> 32));
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, (int)bytes, 0x00020000);
}
// bytes [b0, b1) of the chunk x stored at offset `at` of the resource (dword stores where whole
// dwords lie inside, byte stores for the rest; all with out-of-range offsets where not needed)
__device__ __forceinline__ void store_part(const __amdgpu_buffer_rsrc_t r, uint32_t at, const uint32_t (&x)[4], uint32_t b0,
                                           uint32_t b1, bool live) {
#pragma unroll
  for (uint32_t k = 0; k < 4u; ++k) {
    const bool whole = live && 4u * k >= b0 && 4u * k + 4u <= b1;
    __builtin_amdgcn_raw_buffer_store_b32(x[k], r, whole ? at + 4u * k : kOOB, 0, 0);
  }
  // the partial dword at the front (bytes b0 .. its dword's end) and at the back (its dword's start .. b1)
  const uint32_t f0 = b0, f1 = min(b1, (b0 + 3u) & ~3u);
  const uint32_t e0 = max(b0, b1 & ~3u), e1 = b1;
  const uint32_t x0 = x[0], x1 = x[1], x2 = x[2], x3 = x[3];
  auto byte_at = [=](uint32_t b) __attribute__((always_inline)) {  // mask blends, not an indexed register array
    const uint32_t d = blend(blend(x0, x1, (b >> 2) & 1u), blend(x2, x3, (b >> 2) & 1u), (b >> 3) & 1u);
    return (d >> (8u * (b & 3u))) & 0xFFu;
  };
#pragma unroll
  for (uint32_t j = 0; j < 3u; ++j) {
    const uint32_t bf = f0 + j, be = e0 + j;
    const uint32_t vf = byte_at(bf), ve = byte_at(be);
    __builtin_amdgcn_raw_buffer_store_b8((uint8_t)vf, r, live && bf < f1 ? at + bf : kOOB, 0, 0);
    __builtin_amdgcn_raw_buffer_store_b8((uint8_t)ve, r, live && be < e1 && (be & 3u) < (e1 & 3u) ? at + be : kOOB, 0, 0);
  }
}

// chunk idx (0..7, per lane) of a 128-byte line buffer: mask blends (a select of two array elements
// would be folded into an indexed load, and the buffer would leave the registers for scratch)
constexpr uint32_t kLine = 128;            // bytes per burst of the line writer: one L2 line (64-byte bursts
constexpr uint32_t kLineChunks = kLine / 16;  // left the L2 writing half lines back: r5h, 1.35x the bytes)
__device__ __forceinline__ void pick_chunk(const uint32_t (&buf)[kLineChunks][4], uint32_t idx, uint32_t (&x)[4]) {
  static_assert(kLineChunks == 8, "a three-level blend tree");
  const uint32_t b0 = idx & 1u, b1 = (idx >> 1) & 1u, b2 = (idx >> 2) & 1u;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t t0 = blend(buf[0][k], buf[1][k], b0), t1 = blend(buf[2][k], buf[3][k], b0);
    const uint32_t t2 = blend(buf[4][k], buf[5][k], b0), t3 = blend(buf[6][k], buf[7][k], b0);
    x[k] = blend(blend(t0, t1, b1), blend(t2, t3, b1), b2);
  }
}

// bytes [lo, hi) (0 <= lo < hi <= kLine) of a line buffer at resource offset L: whole chunks
// as 16-byte stores, the (at most two) chunks cut by lo / hi with dword and byte stores
__device__ __forceinline__ void store_line_part(const __amdgpu_buffer_rsrc_t r, uint32_t L, const uint32_t (&buf)[kLineChunks][4],
                                                uint32_t lo, uint32_t hi, bool live) {
#pragma unroll
  for (uint32_t i = 0; i < kLineChunks; ++i) {
    const bool whole = live && 16u * i >= lo && 16u * i + 16u <= hi;
    __builtin_amdgcn_raw_buffer_store_b128(u32x4{buf[i][0], buf[i][1], buf[i][2], buf[i][3]}, r, whole ? L + 16u * i : kOOB,
                                           0, 0);
  }
  const uint32_t il = lo >> 4, ih = (hi - 1u) >> 4;
  uint32_t x[4];
  pick_chunk(buf, il, x);
  const bool cut_lo = (lo & 15u) || (il == ih && (hi & 15u));
  store_part(r, L + 16u * il, x, lo - 16u * il, min(hi - 16u * il, 16u), live && cut_lo);
  pick_chunk(buf, ih, x);
  const bool cut_hi = (hi & 15u) && ih != il;
  store_part(r, L + 16u * ih, x, 0u, hi - 16u * ih, live && cut_hi);
}


// the tile's bytes from record `rec` on, segment by segment in output order: each record's items'
// skeleton segment lists (template runs in LDS; value column c of record r at vals0 + (c * kTile +
// r) * 16), records of no bytes skipped
struct SegIter {
  const uint2* skseg;
  const uint2* seg;
  const int16_t* sk;       // per record: its skeleton ids (kRecSk each)
  const uint8_t* nsk;      // per record: its items
  uint32_t vals0;
  uint32_t rec, n_sk, j, q, n, f;
  uint32_t sa, sb;         // the current segment's output range [sa, sb) ...
  uint32_t src;            // ... and the LDS address of its first byte
  __device__ __forceinline__ void next() {  // the next non-empty segment (sa = ~0 past the tile's last)
    uint32_t a0 = sb, b0 = 0xFFFFFFFFu, s0 = src;
    bool found = false;
    while (!found) {
      if (q < n) {
        const uint2 sg = seg[f + q];
        ++q;
        uint32_t so = sg.x, len = sg.y;
        if (sg.y >= kSegValue) {
          const uint32_t row = vals0 + (sg.x * kTile + rec) * 16u;
          so = row + 1u;
          len = lds_rd(row) & 0xFFu;
        }
        if (len) {
          b0 = a0 + len;
          s0 = so;
          found = true;
        }
      } else if (j < n_sk) {
        const uint2 ss = skseg[sk[rec * kRecSk + j]];
        f = ss.x;
        n = ss.y;
        q = 0;
        ++j;
      } else if (rec + 1u < kTile) {  // the next record: its bytes follow these
        ++rec;
        n_sk = nsk[rec];
        j = q = n = 0;
      } else {
        break;
      }
    }
    sa = found ? a0 : 0xFFFFFFFFu;
    sb = b0;
    src = s0;
  }
};

// merge16 with the byte masks from two LDS tables: bytes >= lo (mlo[lo]) and bytes < hi (mhi[hi])
__device__ __forceinline__ void merge16_lut(uint32_t (&x)[4], const uint32_t (&y)[4], uint32_t lo, uint32_t hi,
                                            uint32_t mlo, uint32_t mhi) {
  const u32x4 a = *(const __attribute__((address_space(3))) u32x4*)(size_t)(mlo + 16u * lo);
  const u32x4 b = *(const __attribute__((address_space(3))) u32x4*)(size_t)(mhi + 16u * hi);
  const uint32_t m0 = a.x & b.x, m1 = a.y & b.y, m2 = a.z & b.z, m3 = a.w & b.w;
  x[0] = __builtin_amdgcn_bitop3_b32(y[0], x[0], m0, 0xe4);  // m ? y : x, bit by bit
  x[1] = __builtin_amdgcn_bitop3_b32(y[1], x[1], m1, 0xe4);
  x[2] = __builtin_amdgcn_bitop3_b32(y[2], x[2], m2, 0xe4);
  x[3] = __builtin_amdgcn_bitop3_b32(y[3], x[3], m3, 0xe4);
}

// the 16-byte chunks of the line at L, gathered from the segments overlapping them
__device__ __forceinline__ void produce_line(SegIter& it, uint32_t L, uint32_t (&buf)[kLineChunks][4], uint32_t mlo,
                                             uint32_t mhi) {
#pragma unroll
  for (uint32_t i = 0; i < kLineChunks; ++i) {
    const uint32_t P = L + 16u * i;
    uint32_t x0 = 0u, x1 = 0u, x2 = 0u, x3 = 0u;
    while (it.sa < P + 16u) {
      if (it.sb > P) {
        uint32_t y[4], x[4] = {x0, x1, x2, x3};
        lds_load16(it.src + P - it.sa, y);  // (bytes before the segment are masked out)
        merge16_lut(x, y, it.sa > P ? it.sa - P : 0u, min(it.sb - P, 16u), mlo, mhi);
        x0 = x[0];
        x1 = x[1];
        x2 = x[2];
        x3 = x[3];
      }
      if (it.sb > P + 16u) break;  // the segment continues into the next chunk
      it.next();
    }
    buf[i][0] = x0;
    buf[i][1] = x1;
    buf[i][2] = x2;
    buf[i][3] = x3;
  }
}

// Each thread writes the record it sized.  kChunk (the default when the program's tables fit in
// LDS): the line writer above — the record's bytes gathered 16 at a time from its items' segments
// (the skeletons' rendered templates and its value rows, all in LDS) and stored kLine bytes at a
// time.  (The first version, 16-byte stores as each chunk filled, left the L2 writing half-filled
// lines back and refilling them: r5e, 2x the patch bytes written; a wave writing its records'
// span together, lane L taking chunks L, L + 64, ..., stored whole lines but spent ~4x the VALU
// finding each chunk's record and segment: r5f, 3.1 vs 2.4 ms.)  Records of more than kRecSk items
// and !kChunk: Acc, four bytes per append.  kLds: the skeleton tables and the records' call-value
// rows (at most kLdsCols columns of 16 bytes) staged in LDS
template <bool kLds, bool kChunk, uint32_t kSrc = kSrc32>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(kChunk ? 5 : 1))) void emit_write_kernel(EmitArgs a) {
  static_assert(kLds || !kChunk, "the chunk writer reads its tables from LDS");
  __shared__ __attribute__((aligned(16))) uint32_t s_tpl[kChunk ? kTplBytes / 4 + 8 : 1];
  __shared__ uint2 s_seg[kChunk ? kMaxSegs : 1];
  __shared__ uint2 s_skseg[kChunk ? kLdsSkels : 1];
  __shared__ uint16_t s_pofs[kChunk ? kLdsPieces : 1];
  __shared__ uint2 s_tsz[kChunk ? kLdsSkels : 1];
  __shared__ __attribute__((aligned(16))) uint4 s_vals[kLds ? kLdsCols * kTile : 1];
  __shared__ kwk_emit_skel s_skels[kLds ? kLdsSkels : 1];
  __shared__ int16_t s_sk[kTile * kRecSk];
  __shared__ uint8_t s_nsk[kChunk ? kTile : 1];  // items per record (the line writer's iterator)
  __shared__ uint32_t s_tend;                    // the tile's bytes end (relative to its 16-byte aligned base)
  __shared__ kwk_emit_piece s_pieces[kLds ? kLdsPieces : 1];
  __shared__ uint32_t s_lits[kLds && !kChunk ? kLdsLits / 4 : 1];
  __shared__ uint2 s_sksz[kLds ? kLdsSkels : 1];
  __shared__ uint32_t s_wi[kWaves];
  __shared__ unsigned long long s_wb[kWaves];
  __shared__ uint32_t s_now[kNowWords];
  __shared__ uint4 s_mlo[kChunk ? 17 : 1], s_mhi[kChunk ? 17 : 1];  // merge16_lut's byte masks
  if (*a.sticky) return;  // this emission or an earlier one in flight exceeded its set: nothing is written
  const uint32_t n = list_len<kSrc>(a), n_tiles = (n + kTile - 1) / kTile;
  const unsigned long long tot_i = a.totals[0], tot_b = a.totals[1];
  if (tot_i > a.cap_items || tot_b > a.cap_bytes || a.totals[2]) return;  // KWK_ECAP: nothing is written
  uint32_t* s_win = nullptr;
  if constexpr (kSrc == kSrc16) s_win = seg_win_lds();
  if constexpr (kLds)
    for (uint32_t j = threadIdx.x; j < a.p.n_skels; j += blockDim.x) s_skels[j] = a.p.skels[j];
  if (threadIdx.x < kNowWords) {
    uint32_t w = 0;
    for (uint32_t b = 0; b < 4u; ++b) w |= (uint32_t)(uint8_t)a.now[4u * threadIdx.x + b] << (8u * b);
    s_now[threadIdx.x] = w;
  }
  const Tables T = stage_tables<kLds, !kChunk>(a, s_pieces, s_lits, s_sksz);
  __syncthreads();  // s_skels, s_now
  const kwk_emit_skel* skels = kLds ? s_skels : a.p.skels;
  if constexpr (kChunk) {
    if (threadIdx.x < 34u) {  // mlo[t]: bytes >= t; mhi[t]: bytes < t
      const uint32_t t = threadIdx.x % 17u;
      uint32_t m[4];
      for (uint32_t k = 0; k < 4u; ++k) {
        m[k] = 0;
        for (uint32_t b = 0; b < 4u; ++b) {
          const uint32_t byte = 4u * k + b;
          if (threadIdx.x < 17u ? byte >= t : byte < t) m[k] |= 0xFFu << (8u * b);
        }
      }
      (threadIdx.x < 17u ? s_mlo : s_mhi)[t] = make_uint4(m[0], m[1], m[2], m[3]);
    }
  }
  if constexpr (kChunk) {  // render every skeleton into its template (Now filled in) and its segment list
    const uint32_t ns = a.p.n_skels;
    for (uint32_t q = threadIdx.x; q < a.p.n_pieces; q += kBlock) s_pofs[q] = 0xFFFFu;  // pieces of no skeleton
    if (threadIdx.x < ns) {
      const kwk_emit_skel S = s_skels[threadIdx.x];
      uint32_t sz = 0;
      for (uint32_t q = 0; q < S.n_pieces; ++q) {
        const kwk_emit_piece P = s_pieces[S.first_piece + q];
        sz += P.lit_len + (P.slot == 0 ? a.now_len : 0u);
      }
      s_tsz[threadIdx.x] = make_uint2(sz, 2u * S.n_pieces + 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {  // exclusive bases: template bytes, segment slots
      uint32_t tb = 0, sb = 0;
      for (uint32_t k = 0; k < ns; ++k) {
        const uint2 v = s_tsz[k];
        s_tsz[k] = make_uint2(tb, sb);
        tb += v.x;
        sb += v.y;
      }
    }
    __syncthreads();
    if (threadIdx.x < ns) {
      const kwk_emit_skel S = s_skels[threadIdx.x];
      const uint32_t tpl = lds_addr(s_tpl);
      uint32_t pos = s_tsz[threadIdx.x].x, run = pos, sb = s_tsz[threadIdx.x].y, n = 0;
      for (uint32_t q = 0; q < S.n_pieces; ++q) {
        const kwk_emit_piece P = s_pieces[S.first_piece + q];
        s_pofs[S.first_piece + q] = (uint16_t)pos;
        pos += P.lit_len;
        if (P.slot == 0) {
          pos += a.now_len;
        } else if (P.slot != KWK_EMIT_NO_SLOT) {
          if (pos > run) s_seg[sb + n++] = make_uint2(tpl + run, pos - run);
          s_seg[sb + n++] = make_uint2(P.slot - 1u, (uint32_t)P.slot * kSegValue);
          run = pos;
        }
      }
      if (pos > run) s_seg[sb + n++] = make_uint2(tpl + run, pos - run);
      s_skseg[threadIdx.x] = make_uint2(sb, n);
    }
    __syncthreads();
    for (uint32_t q = threadIdx.x; q < a.p.n_pieces; q += kBlock) {  // the bytes: one piece per thread
      if (s_pofs[q] == 0xFFFFu) continue;
      const kwk_emit_piece P = s_pieces[q];
      lds_u8* d = (lds_u8*)(size_t)(lds_addr(s_tpl) + s_pofs[q]);
      const char* src = T.lits + P.lit_off;
      for (uint32_t k = 0; k < P.lit_len; ++k) d[k] = (uint8_t)src[k];
      if (P.slot == 0)
        for (uint32_t k = 0; k < a.now_len; ++k) d[P.lit_len + k] = (uint8_t)(s_now[k >> 2] >> (8u * (k & 3u)));
    }
    __syncthreads();
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) a.offsets[tot_i] = tot_b;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t n_ok = 0;
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint32_t lr = threadIdx.x, r = t * kTile + lr;
    Rec x{0u, 0xFFFFFFFFu, false};
    uint64_t w = 0;
    Size sz{0u, 0u, 0ull};
    Vals V{nullptr, lr};
    if constexpr (kLds) V.lds = reinterpret_cast<const uint8_t*>(s_vals);
    SegWin sw{};
    if constexpr (kSrc == kSrc16) sw = tile_segs(a, t, n, s_win);
    if (r < n) {
      if constexpr (kSrc == kSrc16) x = fetch16(a, r, sw, s_win);
      else x = fetch(a, r);
      w = x.valid ? a.words[x.slot] : 0ull;
      if constexpr (kLds) {  // the record's value rows, one 16-byte gather per column (stages with patches only)
        const bool any = x.valid && x.stage < a.p.n_stages && a.p.stage_tpl_ptr[x.stage + 1] > a.p.stage_tpl_ptr[x.stage];
        for (uint32_t c = 0; c < kLdsCols; ++c)
          s_vals[c * kTile + lr] = c < a.p.n_cols && any
                                       ? *reinterpret_cast<const uint4*>(a.p.cols[c] + (uint64_t)x.slot * 16u)
                                       : make_uint4(0xFFu, 0u, 0u, 0u);
      }
      sz = rec_size(a, T, x, w, V);
    }
    n_ok += (uint32_t)__popc(sz.ok);
    // block-exclusive prefix of the records' items / bytes, plus the tile's base
    const uint32_t ii = wave_incl(sz.items, lane);
    const unsigned long long ib = wave_incl(sz.bytes, lane);
    if (lane == 63) {
      s_wi[wave] = ii;
      s_wb[wave] = ib;
    }
    __syncthreads();
    uint32_t item = a.tile_items[t] + ii - sz.items;
    unsigned long long pos = a.tile_bytes[t] + ib - sz.bytes;
    for (uint32_t v = 0; v < wave; ++v) {
      item += s_wi[v];
      pos += s_wb[v];
    }
    const unsigned long long rec_base = pos;
    uint32_t n_sk = 0, t0 = 0, t1 = 0;
    if (r < n && x.stage < a.p.n_stages) {
      t0 = a.p.stage_tpl_ptr[x.stage];
      t1 = a.p.stage_tpl_ptr[x.stage + 1];
      uint32_t g = (uint32_t)(w >> 16) & 0xFFu;
      for (uint32_t j = t0; j < t1; ++j, ++item) {
        const uint32_t tid = a.p.stage_tpl[j];
        const bool ok = (sz.ok >> (j - t0)) & 1u;
        a.items[item] = kwk_emit_item{r, (uint16_t)tid, (uint8_t)(ok ? KWK_EMIT_OK : KWK_EMIT_HOST), 0};
        a.offsets[item] = pos;
        if (ok) {
          const int k = skel_index(a, w, tid);
          const kwk_emit_skel& S = skels[k];
          pos += (unsigned long long)skel_bytes(a, T, (uint32_t)k, x.slot, V);
          g = (g & S.keep) | S.set;
          if (n_sk < kRecSk) s_sk[lr * kRecSk + n_sk] = (int16_t)k;
          ++n_sk;
        }
      }
      // the object's guard bits after the patches (all items emitted here; else the host sets them)
      const uint32_t all = t1 - t0 >= 32 ? 0xFFFFFFFFu : (1u << (t1 - t0)) - 1u;
      if (x.valid && sz.ok == all) {
        const uint32_t cls = (uint32_t)(w & 0xFFFFu);
        if (a.p.stage_delete[x.stage] && cls < a.p.n_classes) g = a.p.fresh[cls];
        const uint64_t nw = (w & ~(0xFFull << 16)) | (uint64_t)g << 16;
        if (nw != w) a.words[x.slot] = nw;
      }
    }
    // ---- the bytes
    bool lane_writes = n_sk != 0;  // this lane writes its own record with Acc
    if constexpr (kChunk) {
      const unsigned long long tb = a.tile_bytes[t] & ~15ull;  // the tile's bytes: < 2 GiB past tb
      const uint32_t g0 = (uint32_t)(rec_base - tb), g1 = (uint32_t)(pos - tb);
      s_nsk[lr] = (uint8_t)min(n_sk, kRecSk);
      if (lr == kTile - 1u) s_tend = g1;
      // a record of more than kRecSk items: the whole tile per lane (Acc)
      if (!__syncthreads_or(n_sk > kRecSk)) {
        lane_writes = false;
        // lane r writes the 128-byte lines that start inside its record, their bytes past it
        // from the records after it: every line of the tile leaves whole, once (lane 0 also
        // writes its part of the line the tile shares with the tile before, and the tile's last
        // line is cut at its end)
        const uint32_t tend = s_tend;
        const __amdgpu_buffer_rsrc_t rs = make_rsrc(a.out + tb, 0x7FFFFFFFu);
        const uint32_t L0 = g0 & ~(kLine - 1u), L1 = (g0 + kLine - 1u) & ~(kLine - 1u);
        const bool head = lr == 0 && L0 != g0 && tend > g0;  // the tile's head line
        SegIter it{s_skseg, s_seg, s_sk, s_nsk, lds_addr(s_vals), lr, s_nsk[lr], 0u, 0u, 0u, 0u, g0, g0, 0u};
        if (head || L1 < g1) it.next();  // (a lane with no line to write never walks the records after it)
        uint32_t buf[kLineChunks][4];
        if (head) {
          produce_line(it, L0, buf, lds_addr(s_mlo), lds_addr(s_mhi));
          store_line_part(rs, L0, buf, g0 - L0, min(tend - L0, kLine), true);
        }
        for (uint32_t L = L1; L < g1; L += kLine) {
          produce_line(it, L, buf, lds_addr(s_mlo), lds_addr(s_mhi));
          const bool whole = L + kLine <= tend;
#pragma unroll
          for (uint32_t i = 0; i < kLineChunks; ++i)
            __builtin_amdgcn_raw_buffer_store_b128(u32x4{buf[i][0], buf[i][1], buf[i][2], buf[i][3]}, rs,
                                                   whole ? L + 16u * i : kOOB, 0, 0);
          if (!whole) store_line_part(rs, L, buf, 0u, min(tend - L, kLine), true);  // the tile's last line
        }
      }
    }
    if (lane_writes) {  // per lane, Acc (four bytes per append)
      Acc o(a.out, rec_base);
      if (n_sk <= kRecSk) {
        for (uint32_t j = 0; j < n_sk; ++j) lane_skel(a, T, skels[s_sk[lr * kRecSk + j]], x.slot, s_now, V, o);
      } else {
        for (uint32_t j = t0; j < t1; ++j)
          if ((sz.ok >> (j - t0)) & 1u) lane_skel(a, T, skels[skel_index(a, w, a.p.stage_tpl[j])], x.slot, s_now, V, o);
      }
      o.finish();
    }
    __syncthreads();  // s_wi / s_wb and the tables are rewritten by the next tile
  }
  n_ok = wave_sum(n_ok);
  if (lane == 0 && n_ok) atomicAdd(&a.totals[3], (unsigned long long)n_ok);
}

// ---- finalizer patches (kwok_emit.h "Finalizer patches"; finalizersModify, finalizers.go:83-111) ----
// A record's JSON patch is `[` + ops joined by `,` + `]`, every op one of a fixed set of literals:
// the remove-all op, the remove op of list index 0..6, the add op of dictionary id 0..14 and each
// stage's whole-list add.  Which ops a record has follows from its stage's entry and its slot's
// order word alone (fin_plan), so the passes are the merge patches': emit_fin_size_kernel (per
// tile: items and bytes), emit_scan_kernel over the finalizer tile arrays, emit_fin_write_kernel
// (items, offsets, the new order words, the bytes).  The stage entries and the literal table sit in
// LDS.  The bytes of a tile are contiguous in the output: each thread copies its record's literals
// into an LDS window of the tile's byte range, and the block stores the window as 16-byte chunks,
// consecutive threads consecutive chunks (the two chunks a tile shares with its neighbours: byte
// stores of the tile's own bytes).
constexpr uint32_t kFinLitBytes = 8192;  // the op literals (LDS)
constexpr uint32_t kFinMaxAdd = 16;      // add ids of one stage: 4 bits each in the stage entry
constexpr uint32_t kFinWin = 16384;      // bytes of a tile assembled in LDS per pass
constexpr uint32_t kFinLitRemoveAll = 0, kFinLitRemoveIdx = 1, kFinLitAddId = 8, kFinLitAddList = 23;
constexpr uint32_t kFinLitMax = kFinLitAddList + KWK_MAX_STAGES;
constexpr uint32_t kFinWordHost = 0xF0000000u;

struct FinArgs {
  const uint4* stages;   // per stage: x = remove set | flags << 16 | adds << 24, y / z = the add ids, 4 bits each
  const uint32_t* lit;   // kFinLitMax entries: byte offset | length << 16
  const uint32_t* lits;  // the literals' bytes as dwords
  uint32_t n_stages, n_lit_words;
  uint32_t* words;
  uint32_t* tile_items;
  unsigned long long* tile_bytes;
  unsigned long long* totals;  // the finalizer stream's (EmitArgs::totals' layout)
  kwk_emit_fin_item* items;
  uint64_t* offsets;
  char* out;
  unsigned long long cap_items, cap_bytes;
};

// a record's ops: bits 0-6 the remove op of list index k, 7 the remove-all op, 8 the stage's
// whole-list add, 9 + j the add op of the stage's j-th add id
struct FinPlan {
  uint32_t desc, n_ops;
  uint32_t status;  // 0: no item, 1: an item with bytes, 2: an item for the host
  uint32_t nw;      // the order word afterwards
};

__device__ __forceinline__ FinPlan fin_plan(const uint4 S, uint32_t w, bool valid) {
  const uint32_t flags = (S.x >> 16) & 0xFFu, n_add = S.x >> 24, remove = S.x & 0xFFFFu;
  FinPlan p{0u, 0u, 0u, w};
  if (!(flags & KWK_NEXT_FIN)) {
    if (flags & KWK_NEXT_DELETE) p.nw = 0u;
    return p;
  }
  const uint32_t n = w >> 28;
  if (!valid || n > 7u) {
    p.status = 2u;
    return p;
  }
  uint32_t present = 0, rm = 0;
#pragma unroll
  for (uint32_t k = 0; k < 7u; ++k) {
    const uint32_t id = (w >> (4u * k)) & 15u;
    if (k < n) {
      present |= 1u << id;
      if (id != 15u && ((remove >> id) & 1u)) rm |= 1u << k;
    }
  }
  bool empty = (flags & KWK_NEXT_FIN_EMPTY) != 0;
  if (empty || !(flags & KWK_NEXT_FIN_REMOVE)) {
    rm = 0;
  } else if ((uint32_t)__popc(rm) == n) {  // every entry removed (0 == 0 too): the list goes as a whole
    empty = true;
    rm = 0;
  }
  uint32_t list = 0, m = 0;
  auto push = [&](uint32_t id) __attribute__((always_inline)) {
    if (m < 7u) list |= id << (4u * m);
    ++m;
  };
  uint32_t desc = rm;
  if (!empty) {
#pragma unroll
    for (uint32_t k = 0; k < 7u; ++k)
      if (k < n && !((rm >> k) & 1u)) push((w >> (4u * k)) & 15u);
  } else if (n) {
    desc |= 1u << 7;
  }
  const uint64_t adds = (uint64_t)S.y | (uint64_t)S.z << 32;
  if (n_add) {
    if (empty || n == 0u) {  // finalizersAdd over no list: one add of the whole list
      desc |= 1u << 8;
      for (uint32_t j = 0; j < n_add; ++j) push((uint32_t)(adds >> (4u * j)) & 15u);
    } else {
      for (uint32_t j = 0; j < n_add; ++j) {  // membership in the original list
        const uint32_t id = (uint32_t)(adds >> (4u * j)) & 15u;
        if (!((present >> id) & 1u)) {
          desc |= 1u << (9u + j);
          push(id);
        }
      }
    }
  }
  p.desc = desc;
  p.n_ops = (uint32_t)__popc(desc);
  p.status = p.n_ops ? 1u : 0u;
  p.nw = m > 7u ? kFinWordHost : list | m << 28;
  if (flags & KWK_NEXT_DELETE) p.nw = 0u;
  return p;
}

// the word is gathered only for the stages that read or reset it (most records of a list have neither)
__device__ __forceinline__ bool fin_reads_word(const uint4 S, const Rec& x) {
  return x.valid && ((S.x >> 16) & (KWK_NEXT_FIN | KWK_NEXT_DELETE)) != 0u;
}

// the literal of every op of a plan, in the patch's order: removes from the highest index down
template <typename F>
__device__ __forceinline__ void fin_ops(uint32_t desc, uint32_t stage, const uint4 S, F&& f) {
  for (int k = 6; k >= 0; --k)
    if ((desc >> k) & 1u) f(kFinLitRemoveIdx + (uint32_t)k);
  if (desc & (1u << 7)) f(kFinLitRemoveAll);
  if (desc & (1u << 8)) f(kFinLitAddList + stage);
  const uint64_t adds = (uint64_t)S.y | (uint64_t)S.z << 32;
  for (uint32_t sel = desc >> 9; sel; sel &= sel - 1u) {
    const uint32_t j = (uint32_t)__ffs((int)sel) - 1u;
    f(kFinLitAddId + ((uint32_t)(adds >> (4u * j)) & 15u));
  }
}

__device__ __forceinline__ uint32_t fin_bytes(const FinPlan& p, uint32_t stage, const uint4 S, const uint32_t* s_lit) {
  if (!p.n_ops) return 0u;
  uint32_t b = p.n_ops + 1u;  // [ ] and the commas
  fin_ops(p.desc, stage, S, [&](uint32_t li) { b += s_lit[li] >> 16; });
  return b;
}

__device__ __forceinline__ void fin_stage_tables(const FinArgs& f, uint4* s_stage, uint32_t* s_lit) {
  for (uint32_t j = threadIdx.x; j < KWK_MAX_STAGES; j += blockDim.x)
    s_stage[j] = j < f.n_stages ? f.stages[j] : make_uint4(0u, 0u, 0u, 0u);
  for (uint32_t j = threadIdx.x; j < kFinLitMax; j += blockDim.x) s_lit[j] = f.lit[j];
}

template <uint32_t kSrc>
__global__ __launch_bounds__(kBlock) void emit_fin_size_kernel(EmitArgs a, FinArgs f) {
  __shared__ uint4 s_stage[KWK_MAX_STAGES];
  __shared__ uint32_t s_lit[kFinLitMax];
  __shared__ uint32_t s_i[kWaves];
  __shared__ unsigned long long s_b[kWaves];
  if (*a.sticky) return;  // this emission's merge patches or an earlier emission exceeded a set
  fin_stage_tables(f, s_stage, s_lit);
  __syncthreads();
  const uint32_t n = list_len<kSrc>(a), n_tiles = (n + kTile - 1) / kTile;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t* s_win = nullptr;
  if constexpr (kSrc == kSrc16) s_win = seg_win_lds();
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    uint32_t it = 0;
    unsigned long long by = 0;
    const uint32_t r = t * kTile + threadIdx.x;
    SegWin sw{};
    if constexpr (kSrc == kSrc16) sw = tile_segs(a, t, n, s_win);
    if (r < n) {
      Rec x;
      if constexpr (kSrc == kSrc16) x = fetch16(a, r, sw, s_win);
      else x = fetch(a, r);
      if (x.stage < f.n_stages) {
        const uint4 S = s_stage[x.stage];
        const FinPlan p = fin_plan(S, fin_reads_word(S, x) ? f.words[x.slot] : 0u, x.valid);
        it = p.status ? 1u : 0u;
        by = fin_bytes(p, x.stage, S, s_lit);
      }
    }
    it = wave_sum(it);
    by = wave_sum(by);
    if (lane == 0) {
      s_i[wave] = it;
      s_b[wave] = by;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t ti = 0;
      unsigned long long tb = 0;
      for (uint32_t w = 0; w < kWaves; ++w) {
        ti += s_i[w];
        tb += s_b[w];
      }
      f.tile_items[t] = ti;
      f.tile_bytes[t] = tb;
    }
    __syncthreads();
  }
}

template <uint32_t kSrc>
__global__ __launch_bounds__(kBlock) void emit_fin_write_kernel(EmitArgs a, FinArgs f) {
  __shared__ uint4 s_stage[KWK_MAX_STAGES];
  __shared__ uint32_t s_lit[kFinLitMax];
  __shared__ uint32_t s_lits[kFinLitBytes / 4];
  __shared__ __attribute__((aligned(16))) uint4 s_out[kFinWin / 16];
  __shared__ uint32_t s_wi[kWaves], s_wb[kWaves];
  __shared__ uint32_t s_tend;
  if (*a.sticky) return;  // an emission in flight (this one included) exceeded a set: nothing is written
  if (a.totals[0] > a.cap_items || a.totals[1] > a.cap_bytes || a.totals[2]) return;  // the merge patches did
  const unsigned long long tot_i = f.totals[0], tot_b = f.totals[1];
  if (tot_i > f.cap_items || tot_b > f.cap_bytes) return;
  fin_stage_tables(f, s_stage, s_lit);
  for (uint32_t j = threadIdx.x; j < f.n_lit_words && j < kFinLitBytes / 4; j += blockDim.x) s_lits[j] = f.lits[j];
  __syncthreads();
  const uint32_t n = list_len<kSrc>(a), n_tiles = (n + kTile - 1) / kTile;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t* s_win = nullptr;
  if constexpr (kSrc == kSrc16) s_win = seg_win_lds();
  if (blockIdx.x == 0 && threadIdx.x == 0) f.offsets[tot_i] = tot_b;
  uint8_t* const sb = reinterpret_cast<uint8_t*>(s_out);
  const uint8_t* const lb = reinterpret_cast<const uint8_t*>(s_lits);
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint32_t lr = threadIdx.x, r = t * kTile + lr;
    Rec x{0u, 0xFFFFFFFFu, false};
    FinPlan p{0u, 0u, 0u, 0u};
    uint4 S = make_uint4(0u, 0u, 0u, 0u);
    uint32_t w = 0, by = 0;
    SegWin sw{};
    if constexpr (kSrc == kSrc16) sw = tile_segs(a, t, n, s_win);
    if (r < n) {
      if constexpr (kSrc == kSrc16) x = fetch16(a, r, sw, s_win);
      else x = fetch(a, r);
      if (x.stage < f.n_stages) {
        S = s_stage[x.stage];
        w = fin_reads_word(S, x) ? f.words[x.slot] : 0u;
        p = fin_plan(S, w, x.valid);
        by = fin_bytes(p, x.stage, S, s_lit);
      }
    }
    const uint32_t has = p.status ? 1u : 0u;
    const uint32_t ii = wave_incl(has, lane), ib = wave_incl(by, lane);
    if (lane == 63) {
      s_wi[wave] = ii;
      s_wb[wave] = ib;
    }
    __syncthreads();
    const unsigned long long tb = f.tile_bytes[t];
    const uint32_t head = (uint32_t)(tb & 15ull);  // positions below are relative to the tile's 16-byte aligned base
    uint32_t item = f.tile_items[t] + ii - has, g0 = head + ib - by;
    for (uint32_t v = 0; v < wave; ++v) {
      item += s_wi[v];
      g0 += s_wb[v];
    }
    const uint32_t g1 = g0 + by;
    if (lr == kTile - 1u) s_tend = g1;
    if (has) {
      f.items[item] = kwk_emit_fin_item{r, (uint8_t)(p.status == 2u ? KWK_EMIT_HOST : KWK_EMIT_OK), (uint8_t)p.n_ops, 0};
      f.offsets[item] = (tb & ~15ull) + g0;
    }
    if (x.stage < f.n_stages && fin_reads_word(S, x) && p.status != 2u && p.nw != w) f.words[x.slot] = p.nw;
    __syncthreads();  // s_tend
    const uint32_t tend = s_tend;
    char* const base = f.out + (tb & ~15ull);
    for (uint32_t W = 0; W < tend; W += kFinWin) {  // (block-uniform)
      if (by && g1 > W && g0 < W + kFinWin) {  // this record's bytes inside the window
        uint32_t q = g0 - W;                    // (wraps below the window: such bytes are skipped)
        auto put = [&](uint32_t c) __attribute__((always_inline)) {
          if (q < kFinWin) sb[q] = (uint8_t)c;
          ++q;
        };
        put('[');
        bool first = true;
        fin_ops(p.desc, x.stage, S, [&](uint32_t li) {
          if (!first) put(',');
          first = false;
          const uint32_t e = s_lit[li], off = e & 0xFFFFu, len = e >> 16;
          for (uint32_t b = 0; b < len; ++b) put(lb[off + b]);
        });
        put(']');
      }
      __syncthreads();
      for (uint32_t c = threadIdx.x; c < kFinWin / 16u; c += kBlock) {
        const uint32_t P = W + 16u * c;
        const uint32_t lo = max(P, head), hi = min(P + 16u, tend);
        if (lo >= hi) continue;
        if (hi - lo == 16u) {
          *reinterpret_cast<uint4*>(base + P) = s_out[c];
        } else {  // a chunk shared with the neighbouring tile: this tile's bytes only
          for (uint32_t b = lo; b < hi; ++b) base[b] = (char)sb[b - W];
        }
      }
      __syncthreads();
    }
  }
}

// ---- Events (kwok_events.h; client-go generateEvent / makeEvent, restated in kwok_patch.h) ----
// A record's Event body is fixed text around the object's name (twice), namespace (once or twice)
// and uid: the literals every stage shares (kEvtLit*), `.<hex>","namespace":"` of this emission, and
// the stage's tail — everything after the last inserted value, with the emission's timestamp in
// place twice.  The passes are the other streams': emit_evt_size_kernel (per tile: items and bytes;
// the three row lengths are gathered for event stages only), emit_scan_kernel over the event tile
// arrays, emit_evt_write_kernel.  The writer builds the tails in LDS once per block, lists the
// tile's items in LDS, and gives each item to a group of 16 lanes, which copies its runs and rows
// into the LDS window of the tile's byte range a dword per lane (source and destination are not
// aligned to each other: a funnel shift of two source dwords; the up to three bytes at either end of
// a run are byte stores).  The block stores the window as 16-byte chunks, consecutive threads
// consecutive chunks; the two chunks a tile shares with its neighbours leave as byte stores.
constexpr uint32_t kEvtWin = 16384;        // bytes of a tile assembled in LDS per pass
constexpr uint32_t kEvtTailBytes = 26624;  // the event stages' tails (LDS): KWK_EVT_MAX_TEXT + 32 stages' fixed text
constexpr uint32_t kEvtComWords = 64;      // the shared literals (LDS)
constexpr uint32_t kEvtGroup = 16, kEvtGroups = kBlock / kEvtGroup;
constexpr uint32_t kEvtRowHost = 0xFFu;
// the shared literals: A `{"metadata":{"name":"`, C `","creationTimestamp":null},"involvedObject":{"kind":"<Kind>"`,
// D `,"namespace":"`, E1 `,"name":"`, E2 `","name":"`, F `","uid":"`, `default`
enum : uint32_t { kEvtLitA, kEvtLitC, kEvtLitD, kEvtLitE1, kEvtLitE2, kEvtLitF, kEvtLitDefault, kEvtLits };

struct EvtArgs {
  const uint4* stages;    // per stage: x = byte offset of its tail in `tails` (4-aligned), y = its length (0: no
                          // event), z / w = the offsets of its two timestamps
  const uint32_t* tails;  // the tails' bytes as dwords
  const uint32_t* com;    // the shared literals' bytes as dwords
  uint32_t com_ent[kEvtLits];  // byte offset (4-aligned) | length << 16
  uint32_t n_tail_words, n_com_words, n_stages;
  uint32_t base_bytes;    // A + C + E1 (+ this emission's `.<hex>","namespace":"`): every body has them
  const uint8_t* rows[3];  // name, namespace (null: none), uid
  uint32_t stride[3];
  uint32_t* tile_items;
  unsigned long long* tile_bytes;
  unsigned long long* totals;  // the event stream's (EmitArgs::totals' layout)
  kwk_evt_item* items;
  uint64_t* offsets;
  char* out;
  unsigned long long cap_items, cap_bytes;
  uint32_t b_len;
  char b[36];   // `.<hex>","namespace":"`
  char ts[20];  // 2006-01-02T15:04:05Z
};

struct EvtRec {
  uint32_t has;  // 0: no item, 1: an item with bytes, 2: an item for the host
  uint32_t by, ln, lns, lu;
};

// s_tl: the stages' tail lengths (LDS)
__device__ __forceinline__ EvtRec evt_rec(const EvtArgs& e, const Rec& x, const uint32_t* s_tl) {
  EvtRec v{0u, 0u, 0u, 0u, 0u};
  if (x.stage >= e.n_stages) return v;
  const uint32_t tl = s_tl[x.stage];
  if (!tl) return v;
  v.has = 2u;
  if (!x.valid) return v;
  v.ln = e.rows[0][(size_t)x.slot * e.stride[0]];
  v.lns = e.rows[1] ? e.rows[1][(size_t)x.slot * e.stride[1]] : 0u;
  v.lu = e.rows[2][(size_t)x.slot * e.stride[2]];
  // (an empty name is the host's too: ObjectReference.Name is omitempty, the key goes)
  if (v.ln == kEvtRowHost || v.ln == 0u || v.lns == kEvtRowHost || v.lu == kEvtRowHost) return v;
  v.has = 1u;
  v.by = e.base_bytes + tl + 2u * v.ln + (v.lns ? 2u * v.lns + (e.com_ent[kEvtLitD] >> 16) + 1u : 7u) +
         (v.lu ? (e.com_ent[kEvtLitF] >> 16) + v.lu : 0u);
  return v;
}

template <uint32_t kSrc>
__global__ __launch_bounds__(kBlock) void emit_evt_size_kernel(EmitArgs a, EvtArgs e) {
  __shared__ uint32_t s_tl[KWK_MAX_STAGES];
  __shared__ uint32_t s_i[kWaves];
  __shared__ unsigned long long s_b[kWaves];
  if (*a.sticky) return;  // this emission's other streams or an earlier emission exceeded a set
  if (threadIdx.x < KWK_MAX_STAGES) s_tl[threadIdx.x] = threadIdx.x < e.n_stages ? e.stages[threadIdx.x].y : 0u;
  __syncthreads();
  const uint32_t n = list_len<kSrc>(a), n_tiles = (n + kTile - 1) / kTile;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t* s_win = nullptr;
  if constexpr (kSrc == kSrc16) s_win = seg_win_lds();
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    uint32_t it = 0;
    unsigned long long by = 0;
    const uint32_t r = t * kTile + threadIdx.x;
    SegWin sw{};
    if constexpr (kSrc == kSrc16) sw = tile_segs(a, t, n, s_win);
    if (r < n) {
      Rec x;
      if constexpr (kSrc == kSrc16) x = fetch16(a, r, sw, s_win);
      else x = fetch(a, r);
      const EvtRec v = evt_rec(e, x, s_tl);
      it = v.has ? 1u : 0u;
      by = v.by;
    }
    it = wave_sum(it);
    by = wave_sum(by);
    if (lane == 0) {
      s_i[wave] = it;
      s_b[wave] = by;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t ti = 0;
      unsigned long long tb = 0;
      for (uint32_t w = 0; w < kWaves; ++w) {
        ti += s_i[w];
        tb += s_b[w];
      }
      e.tile_items[t] = ti;
      e.tile_bytes[t] = tb;
    }
    __syncthreads();
  }
}

// `len` bytes from byte `so` of the dword array `src` to window position q (it may start before the
// window or end after it: clipped), by lane gl of a group of kEvtGroup.  Whole destination dwords are
// stored as dwords, the bytes of the run's first and last partial dword as bytes: no byte of
// another run is written.  Reads at most one dword past the run's last (the sources are padded).
template <typename P>
__device__ __forceinline__ void evt_copy(uint8_t* win, int32_t q, P src, uint32_t so, uint32_t len, int32_t gl) {
  const int32_t lo = max(q, 0), hi = min(q + (int32_t)len, (int32_t)kEvtWin);
  if (lo >= hi) return;
  auto byte_at = [&](int32_t b) __attribute__((always_inline)) {
    const uint32_t s = so + (uint32_t)(b - q);
    return (uint8_t)(src[s >> 2] >> (8u * (s & 3u)));
  };
  const int32_t d0 = (lo + 3) >> 2, d1 = hi >> 2;
  if (d0 >= d1) {
    for (int32_t b = lo + gl; b < hi; b += (int32_t)kEvtGroup) win[b] = byte_at(b);
    return;
  }
  const int32_t nh = 4 * d0 - lo, nt = hi - 4 * d1;  // 0..3 each
  if (gl < nh) win[lo + gl] = byte_at(lo + gl);
  else if (gl >= 8 && gl - 8 < nt) win[4 * d1 + gl - 8] = byte_at(4 * d1 + gl - 8);
  uint32_t* const w32 = reinterpret_cast<uint32_t*>(win);
  for (int32_t d = d0 + gl; d < d1; d += (int32_t)kEvtGroup) {
    const uint32_t s = so + (uint32_t)(4 * d - q), sh = 8u * (s & 3u);
    const uint32_t w0 = src[s >> 2];
    w32[d] = sh ? (w0 >> sh) | (src[(s >> 2) + 1u] << (32u - sh)) : w0;
  }
}

template <uint32_t kSrc>
__global__ __launch_bounds__(kBlock) void emit_evt_write_kernel(EmitArgs a, EvtArgs e) {
  __shared__ uint4 s_stage[KWK_MAX_STAGES];
  __shared__ uint32_t s_tl[KWK_MAX_STAGES];
  __shared__ uint32_t s_tails[kEvtTailBytes / 4 + 4];
  __shared__ uint32_t s_com[kEvtComWords + 4];
  __shared__ uint32_t s_b[12];
  __shared__ uint4 s_desc[kTile];  // the tile's items: slot, stage | lengths, start in the tile, bytes
  __shared__ __attribute__((aligned(16))) uint4 s_out[kEvtWin / 16];
  __shared__ uint32_t s_wi[kWaves], s_wb[kWaves];
  __shared__ uint32_t s_tend, s_nit;
  if (*a.sticky) return;  // an emission in flight (this one included) exceeded a set: nothing is written
  if (a.totals[0] > a.cap_items || a.totals[1] > a.cap_bytes || a.totals[2]) return;  // the merge patches did
  const unsigned long long tot_i = e.totals[0], tot_b = e.totals[1];
  if (tot_i > e.cap_items || tot_b > e.cap_bytes) return;
  for (uint32_t j = threadIdx.x; j < KWK_MAX_STAGES; j += blockDim.x) {
    const uint4 S = j < e.n_stages ? e.stages[j] : make_uint4(0u, 0u, 0u, 0u);
    s_stage[j] = S;
    s_tl[j] = S.y;
  }
  for (uint32_t j = threadIdx.x; j < e.n_tail_words && j < kEvtTailBytes / 4; j += blockDim.x) s_tails[j] = e.tails[j];
  for (uint32_t j = threadIdx.x; j < e.n_com_words && j < kEvtComWords; j += blockDim.x) s_com[j] = e.com[j];
  if (threadIdx.x < 9u) {
    uint32_t w = 0;
    for (uint32_t b = 0; b < 4u; ++b) w |= (uint32_t)(uint8_t)e.b[4u * threadIdx.x + b] << (8u * b);
    s_b[threadIdx.x] = w;
  }
  __syncthreads();
  {  // this emission's timestamp into every tail, twice
    uint8_t* const tb8 = reinterpret_cast<uint8_t*>(s_tails);
    for (uint32_t j = threadIdx.x; j < e.n_stages * 40u; j += blockDim.x) {
      const uint4 S = s_stage[j / 40u];
      const uint32_t k = j % 40u;
      if (S.y) tb8[(k < 20u ? S.z : S.w) + k % 20u] = (uint8_t)e.ts[k % 20u];
    }
  }
  __syncthreads();
  const uint32_t n = list_len<kSrc>(a), n_tiles = (n + kTile - 1) / kTile;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t grp = threadIdx.x / kEvtGroup;
  const int32_t gl = (int32_t)(threadIdx.x % kEvtGroup);
  uint32_t* s_win = nullptr;
  if constexpr (kSrc == kSrc16) s_win = seg_win_lds();
  if (blockIdx.x == 0 && threadIdx.x == 0) e.offsets[tot_i] = tot_b;
  uint8_t* const sb = reinterpret_cast<uint8_t*>(s_out);
  const uint32_t lenD = e.com_ent[kEvtLitD] >> 16, lenF = e.com_ent[kEvtLitF] >> 16;
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint32_t lr = threadIdx.x, r = t * kTile + lr;
    Rec x{0u, 0xFFFFFFFFu, false};
    EvtRec v{0u, 0u, 0u, 0u, 0u};
    SegWin sw{};
    if constexpr (kSrc == kSrc16) sw = tile_segs(a, t, n, s_win);
    if (r < n) {
      if constexpr (kSrc == kSrc16) x = fetch16(a, r, sw, s_win);
      else x = fetch(a, r);
      v = evt_rec(e, x, s_tl);
    }
    const uint32_t has = v.has ? 1u : 0u, by = v.by;
    const uint32_t ii = wave_incl(has, lane), ib = wave_incl(by, lane);
    if (lane == 63) {
      s_wi[wave] = ii;
      s_wb[wave] = ib;
    }
    __syncthreads();
    const unsigned long long tb = e.tile_bytes[t];
    const uint32_t head = (uint32_t)(tb & 15ull);  // positions below are relative to the tile's 16-byte aligned base
    uint32_t li = ii - has, g0 = head + ib - by;
    for (uint32_t u = 0; u < wave; ++u) {
      li += s_wi[u];
      g0 += s_wb[u];
    }
    if (lr == kTile - 1u) {
      s_tend = g0 + by;
      s_nit = li + has;
    }
    if (has) {
      const uint32_t item = e.tile_items[t] + li;
      e.items[item] = kwk_evt_item{r, (uint8_t)(v.has == 2u ? KWK_EMIT_HOST : KWK_EMIT_OK), {0, 0, 0}};
      e.offsets[item] = (tb & ~15ull) + g0;
      s_desc[li] = make_uint4(x.slot, x.stage | v.ln << 8 | v.lns << 16 | v.lu << 24, g0, by);
    }
    __syncthreads();  // s_tend, s_nit, s_desc
    const uint32_t tend = s_tend, nit = s_nit;
    char* const base = e.out + (tb & ~15ull);
    for (uint32_t W = 0; W < tend; W += kEvtWin) {  // (block-uniform)
      for (uint32_t k = grp; k < nit; k += kEvtGroups) {
        const uint4 D = s_desc[k];
        if (!D.w || D.z + D.w <= W || D.z >= W + kEvtWin) continue;  // no bytes, or none inside the window
        const uint32_t stage = D.y & 0xFFu, ln = (D.y >> 8) & 0xFFu, lns = (D.y >> 16) & 0xFFu, lu = D.y >> 24;
        int32_t q = (int32_t)D.z - (int32_t)W;
        auto lit = [&](uint32_t id) __attribute__((always_inline)) {
          const uint32_t ent = e.com_ent[id];
          evt_copy(sb, q, (const uint32_t*)s_com, ent & 0xFFFFu, ent >> 16, gl);
          q += (int32_t)(ent >> 16);
        };
        auto row = [&](uint32_t c, uint32_t len) __attribute__((always_inline)) {
          const uint32_t* p = reinterpret_cast<const uint32_t*>(e.rows[c] + (size_t)D.x * e.stride[c]);
          evt_copy(sb, q, p, 1u, len, gl);
          q += (int32_t)len;
        };
        lit(kEvtLitA);
        row(0u, ln);
        evt_copy(sb, q, (const uint32_t*)s_b, 0u, e.b_len, gl);
        q += (int32_t)e.b_len;
        if (lns) row(1u, lns);
        else lit(kEvtLitDefault);
        lit(kEvtLitC);
        if (lns) {
          lit(kEvtLitD);
          row(1u, lns);
          lit(kEvtLitE2);
        } else {
          lit(kEvtLitE1);
        }
        row(0u, ln);
        if (lu) {
          lit(kEvtLitF);
          row(2u, lu);
        }
        const uint4 S = s_stage[stage];
        evt_copy(sb, q, (const uint32_t*)s_tails, S.x, S.y, gl);
      }
      __syncthreads();
      for (uint32_t c = threadIdx.x; c < kEvtWin / 16u; c += kBlock) {
        const uint32_t P = W + 16u * c;
        const uint32_t lo = max(P, head), hi = min(P + 16u, tend);
        if (lo >= hi) continue;
        if (hi - lo == 16u) {
          *reinterpret_cast<uint4*>(base + P) = s_out[c];
        } else {  // a chunk shared with the neighbouring tile: this tile's bytes only
          for (uint32_t b = lo; b < hi; ++b) base[b] = (char)sb[b - W];
        }
      }
      __syncthreads();
    }
  }
}

}  // namespace

struct kwk_emitter {
  std::string err;
  kwk_engine* eng = nullptr;  // must outlive the emitter
  uint64_t layout_epoch = 0;  // the engine's kwk_layout_epoch at create: the slot layout the per-slot words and columns are for
  hipStream_t stream = nullptr;  // the engine's stream as of the current call (kwk_stream at every entry:
                                 // KWK_TUNE_STREAM_PRIORITY re-creates it, so it is never cached across calls)
  int device = 0;
  uint32_t capacity = 0, n_columns = 0, max_tiles = 0, grid = 0, cus = 1;
  int write_occ[6] = {0, 0, 0, 0, 0, 0};  // resident blocks per CU of each write kernel variant (0: not asked yet)
  Prog p{};  // the kernels' view of the program: its pointers alias the tables of `pm`
  struct ProgMem {
    DevBuf<uint32_t> stage_tpl_ptr, stride;
    DevBuf<uint16_t> stage_tpl;
    DevBuf<uint8_t> stage_delete, fresh;
    DevBuf<int32_t> skel_of;
    DevBuf<kwk_emit_skel> skels;
    DevBuf<kwk_emit_piece> pieces;
    DevBuf<char> lits;
    DevBuf<uint8_t*> cols;
  } pm;
  std::vector<uint32_t> stride;
  std::vector<DevBuf<uint8_t>> cols;
  DevBuf<uint64_t> d_words;
  DevBuf<uint32_t> d_tile_items;
  DevBuf<unsigned long long> d_tile_bytes;
  // The output sets (kwk_emit_reserve_sets; one by default): emissions rotate through them, so
  // that the emissions of a fused group are enqueued back to back and all read afterwards
  struct OutSet {
    unsigned long long* d_totals = nullptr;  // 8 words of d_totals_all (an alias, not owned)
    DevBuf<kwk_emit_item> d_items;
    DevBuf<uint64_t> d_offsets;
    DevBuf<char> d_out;
    uint64_t cap_items = 0, cap_bytes = 0;
    Event ev0, ev1;
    bool emitted = false;
    // the finalizer stream (kwk_emit_finalizers_load)
    unsigned long long* d_fin_totals = nullptr;  // 8 words of d_fin_totals_all (an alias, not owned)
    DevBuf<kwk_emit_fin_item> d_fin_items;
    DevBuf<uint64_t> d_fin_offsets;
    DevBuf<char> d_fin_out;
    uint64_t fin_cap_items = 0, fin_cap_bytes = 0;
    // the event stream (kwk_evt_load)
    unsigned long long* d_evt_totals = nullptr;  // 8 words of d_evt_totals_all (an alias, not owned)
    DevBuf<kwk_evt_item> d_evt_items;
    DevBuf<uint64_t> d_evt_offsets;
    DevBuf<char> d_evt_out;
    uint64_t evt_cap_items = 0, evt_cap_bytes = 0;
  };
  std::vector<OutSet> sets;
  uint32_t cur = 0;               // the set of the last emission
  uint32_t n_emitted = 0;         // emissions since the sets were made (kwk_emit_select's range)
  uint32_t sel = 0;               // the readers' emission: `sel` before the last
  DevBuf<unsigned long long> d_totals_all;
  DevBuf<uint32_t> d_sticky;      // device flag: an emission in flight exceeded its set; two words:
  uint32_t* d_zero = nullptr;     // its second, a zero length word (a ring list of no segments is empty; an alias)
  bool sticky_armed = false;      // an emission that may set d_sticky was enqueued since it was cleared
  bool saw_cap = false;           // the host has read KWK_ECAP: the next emission clears d_sticky
  DevBuf<uint32_t> d_seg_base;    // the 2-byte source's segment bases (n_segs + 1) ...
  DevBuf<uint32_t> d_tile_seg;    // ... and every tile's first segment (max_tiles + 1)
  OutSet& selected() { return sets[(cur + (uint32_t)sets.size() - sel) % (uint32_t)sets.size()]; }
  bool chunk_ok = false;          // skeletons own consecutive, disjoint piece ranges (the chunk writer's templates)
  bool lencache = false;          // words' bits 24-31 cache the value lengths (emit_lens_kernel)
  bool fin = false;               // a finalizer program is loaded: every emission also emits its stream
  bool fin_any = false;           // ... and some stage of it has KWK_NEXT_FIN (else its launches are skipped)
  FinArgs f{};                    // the kernels' view of it: its pointers alias `fm`
  struct FinMem {                 // its device tables, order words and tile arrays
    DevBuf<uint4> stages;
    DevBuf<uint32_t> lit, lits, words, tile_items;
    DevBuf<unsigned long long> tile_bytes;
  } fm;
  DevBuf<unsigned long long> d_fin_totals_all;
  uint64_t fin_req_items = 0, fin_req_bytes = 0;  // kwk_emit_reserve_fin's room, given to every set
  bool evt = false;               // an event program is loaded: every emission also emits its stream
  bool evt_any = false;           // ... and some stage of it records an Event (else its launches are skipped)
  EvtArgs e{};                    // the kernels' view of it: its pointers alias `evm`
  struct EvtMem {                 // its device tables, identity columns and tile arrays
    DevBuf<uint4> stages;
    DevBuf<uint32_t> tails, com, tile_items;
    DevBuf<uint8_t> rows[3];
    DevBuf<unsigned long long> tile_bytes;
  } evm;
  uint32_t evt_fixed = 0;         // bytes of the literals every body has, without `.<hex>","namespace":"`
  DevBuf<unsigned long long> d_evt_totals_all;
  uint64_t evt_req_items = 0, evt_req_bytes = 0;  // kwk_evt_reserve's room, given to every set
  uint64_t tpl_lits = 0;          // literal bytes of every skeleton's pieces
  uint32_t tpl_now_slots = 0;     // Now slots of every skeleton's pieces

  // the device is set and the stream idle before the members free themselves
  ~kwk_emitter() {
    hipSetDevice(device);
    void* s = nullptr;
    if (eng && kwk_stream(eng, &s) == KWK_OK && s) hipStreamSynchronize(static_cast<hipStream_t>(s));
  }
};

namespace {

// the engine's current stream and device (every entry point: the stream may have been re-created)
kwk_status bind(kwk_emitter* em) {
  void* s = nullptr;
  if (kwk_stream(em->eng, &s) != KWK_OK || !s)
    return fail(KWK_ESTATE, std::string("kwk_stream: ") + kwk_last_error(em->eng));
  em->stream = static_cast<hipStream_t>(s);
  HIP_TRY(hipSetDevice(em->device));
  return KWK_OK;
}

// host -> device copy ordered on the engine's stream (a pageable hipMemcpy on the null stream can
// return with its DMA in flight, and the engine's non-blocking stream would not wait for it)
kwk_status copy_in(kwk_emitter* em, void* dst, const void* src, size_t bytes) {
  HIP_TRY(copy_in(em->stream, dst, src, bytes));
  return KWK_OK;
}

kwk_status copy_out(kwk_emitter* em, void* dst, const void* src, size_t bytes) {
  HIP_TRY(copy_out(em->stream, dst, src, bytes));
  return KWK_OK;
}

kwk_status fill(kwk_emitter* em, void* dst, int v, size_t bytes) {
  HIP_TRY(hipMemsetAsync(dst, v, bytes, em->stream));
  HIP_TRY(hipStreamSynchronize(em->stream));
  return KWK_OK;
}

// makes `own` a device copy of n items, and *view (a kernel-argument alias) its address
template <typename T, typename V>
kwk_status upload(kwk_emitter* em, DevBuf<T>& own, V* view, const T* src, size_t n) {
  HIP_TRY(own.alloc(std::max<size_t>(1, n)));
  if (kwk_status st = copy_in(em, own, src, n * sizeof(T))) return st;
  *view = own.get();
  return KWK_OK;
}

constexpr uint32_t kMaxSets = 8;

// n fresh output sets (the stream idle): the rotation starts over
kwk_status make_sets(kwk_emitter* em, uint32_t n) {
  em->sets.clear();
  em->sets.resize(n);
  for (uint32_t i = 0; i < n; ++i) {
    em->sets[i].d_totals = em->d_totals_all + 8u * i;
    em->sets[i].d_fin_totals = em->d_fin_totals_all ? em->d_fin_totals_all + 8u * i : nullptr;
    em->sets[i].d_evt_totals = em->d_evt_totals_all ? em->d_evt_totals_all + 8u * i : nullptr;
    HIP_TRY(em->sets[i].ev0.create(hipEventDefault));
    HIP_TRY(em->sets[i].ev1.create(hipEventDefault));
  }
  em->cur = n - 1u;
  em->n_emitted = 0;
  em->sel = 0;
  return KWK_OK;
}

kwk_status check_program(const kwk_emit_program* g) {
  if (!g->stage_tpl_ptr || !g->stage_delete || (g->n_classes && !g->fresh_guards) ||
      (g->n_classes * g->n_templates && !g->skel_of))
    return fail(KWK_EINVAL, "emit program: null array");
  if (g->n_templates > 32) return fail(KWK_EINVAL, "emit program: more than 32 templates");
  if ((uint64_t)g->n_classes * g->n_templates > (1u << 26)) return fail(KWK_EINVAL, "emit program: too many skeletons");
  if (g->stage_tpl_ptr[0] != 0) return fail(KWK_EINVAL, "emit program: stage_tpl_ptr[0] != 0");
  for (uint32_t s = 0; s < g->n_stages; ++s) {
    const uint32_t a = g->stage_tpl_ptr[s], b = g->stage_tpl_ptr[s + 1];
    if (b < a || b - a > kMaxStageTpl) return fail(KWK_EINVAL, "emit program: stage template ranges");
  }
  const uint32_t n_st = g->stage_tpl_ptr[g->n_stages];
  if (n_st && !g->stage_tpl) return fail(KWK_EINVAL, "emit program: null stage_tpl");
  for (uint32_t j = 0; j < n_st; ++j)
    if (g->stage_tpl[j] >= g->n_templates) return fail(KWK_EINVAL, "emit program: template id out of range");
  for (uint64_t i = 0; i < (uint64_t)g->n_classes * g->n_templates; ++i)
    if (g->skel_of[i] < -1 || g->skel_of[i] >= (int64_t)g->n_skels) return fail(KWK_EINVAL, "emit program: skeleton index");
  if ((g->n_skels && !g->skels) || (g->n_pieces && !g->pieces) || (g->n_lit_bytes && !g->lits) ||
      (g->n_columns && !g->column_stride))
    return fail(KWK_EINVAL, "emit program: null array");
  for (uint32_t k = 0; k < g->n_skels; ++k) {
    const kwk_emit_skel& S = g->skels[k];
    if ((uint64_t)S.first_piece + S.n_pieces > g->n_pieces) return fail(KWK_EINVAL, "emit program: piece range");
  }
  for (uint32_t q = 0; q < g->n_pieces; ++q) {
    const kwk_emit_piece& P = g->pieces[q];
    if ((uint64_t)P.lit_off + P.lit_len > g->n_lit_bytes) return fail(KWK_EINVAL, "emit program: literal range");
    if (P.slot != KWK_EMIT_NO_SLOT && P.slot > g->n_columns) return fail(KWK_EINVAL, "emit program: slot out of range");
  }
  for (uint32_t c = 0; c < g->n_columns; ++c)
    if (g->column_stride[c] < 4 || g->column_stride[c] > 256 || (g->column_stride[c] & 3u))
      return fail(KWK_EINVAL, "emit program: column stride 4..256, a multiple of 4");
  return KWK_OK;
}

// the words' cached value lengths for slots [first, first + n) (after any write of words or rows)
kwk_status refresh_lens(kwk_emitter* em, uint32_t first, uint32_t n) {
  if (!em->lencache || !n) return KWK_OK;
  const uint32_t blocks = std::min<uint32_t>((n + 255u) / 256u, em->cus * 16u);
  hipLaunchKernelGGL(emit_lens_kernel, dim3(blocks), dim3(256), 0, em->stream, em->d_words, em->p.cols, em->n_columns,
                     first, n);
  HIP_TRY(hipGetLastError());
  return KWK_OK;
}

kwk_status emitter_init(kwk_emitter* em, const kwk_emit_program* g) {
  em->p.n_classes = g->n_classes;
  em->p.n_templates = g->n_templates;
  em->p.n_stages = g->n_stages;
  em->p.n_pieces = g->n_pieces;
  em->p.n_lits = (uint32_t)std::min<uint64_t>(g->n_lit_bytes, 0xFFFFFFFFu);
  em->p.n_cols = g->n_columns;
  em->p.n_skels = g->n_skels;
  {  // the chunk writer's templates: pieces owned by one skeleton each, in skeleton order
    bool ok = true;
    uint32_t next = 0;
    for (uint32_t k = 0; k < g->n_skels && ok; ++k) {
      const kwk_emit_skel& S = g->skels[k];
      ok = S.first_piece >= next;
      next = S.first_piece + S.n_pieces;
      for (uint32_t q = 0; q < S.n_pieces; ++q) {
        const kwk_emit_piece& P = g->pieces[S.first_piece + q];
        em->tpl_lits += P.lit_len;
        em->tpl_now_slots += P.slot == 0 ? 1u : 0u;
      }
    }
    em->chunk_ok = ok;
  }
  const uint32_t n_st = g->stage_tpl_ptr[g->n_stages];
  if (kwk_status st = upload(em, em->pm.stage_tpl_ptr, &em->p.stage_tpl_ptr, g->stage_tpl_ptr, g->n_stages + 1)) return st;
  if (kwk_status st = upload(em, em->pm.stage_tpl, &em->p.stage_tpl, g->stage_tpl, n_st)) return st;
  if (kwk_status st = upload(em, em->pm.stage_delete, &em->p.stage_delete, g->stage_delete, g->n_stages)) return st;
  if (kwk_status st = upload(em, em->pm.skel_of, &em->p.skel_of, g->skel_of, (size_t)g->n_classes * g->n_templates))
    return st;
  if (kwk_status st = upload(em, em->pm.skels, &em->p.skels, g->skels, g->n_skels)) return st;
  if (kwk_status st = upload(em, em->pm.pieces, &em->p.pieces, g->pieces, g->n_pieces)) return st;
  {  // the literal runs with 16 bytes of zero padding (the writers read aligned dword pairs)
    std::vector<char> lits(g->lits, g->lits + g->n_lit_bytes);
    lits.resize(lits.size() + 16, 0);
    if (kwk_status st = upload(em, em->pm.lits, &em->p.lits, lits.data(), lits.size())) return st;
  }
  if (kwk_status st = upload(em, em->pm.fresh, &em->p.fresh, g->fresh_guards, g->n_classes)) return st;
  em->n_columns = g->n_columns;
  em->stride.assign(g->column_stride, g->column_stride + g->n_columns);
  for (uint32_t c = 0; c < g->n_columns; ++c) {
    DevBuf<uint8_t> d;
    HIP_TRY(d.alloc((size_t)em->capacity * em->stride[c] + 16));  // + the dword a row's last read may touch
    if (kwk_status st = fill(em, d, 0xFF, d.size())) return st;  // unusable until set
    em->cols.push_back(std::move(d));
  }
  const std::vector<uint8_t*> cols(em->cols.begin(), em->cols.end());
  if (kwk_status st = upload(em, em->pm.cols, &em->p.cols, cols.data(), cols.size())) return st;
  if (kwk_status st = upload(em, em->pm.stride, &em->p.stride, em->stride.data(), em->stride.size())) return st;
  HIP_TRY(em->d_words.alloc(std::max(1u, em->capacity)));
  if (kwk_status st = fill(em, em->d_words, 0, em->d_words.size() * 8)) return st;  // class 0, nothing accepted: all to the host
  em->lencache = g->n_columns <= 2;
  for (uint32_t c = 0; c < g->n_columns; ++c) em->lencache = em->lencache && g->column_stride[c] == 16u;
  em->max_tiles = (em->capacity + kTile - 1) / kTile + 1;
  HIP_TRY(em->d_tile_items.alloc(em->max_tiles));
  HIP_TRY(em->d_tile_bytes.alloc(em->max_tiles));
  HIP_TRY(em->d_totals_all.alloc(kMaxSets * 8));
  if (kwk_status st = fill(em, em->d_totals_all, 0, kMaxSets * 8 * 8)) return st;
  HIP_TRY(em->d_sticky.alloc(2));
  em->d_zero = em->d_sticky + 1;
  if (kwk_status st = fill(em, em->d_sticky, 0, 2 * 4)) return st;
  HIP_TRY(em->d_tile_seg.alloc((size_t)em->max_tiles + 1));
  if (kwk_status st = make_sets(em, 1)) return st;
  int cus = 0;
  HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, em->device));
  em->grid = std::max(1u, std::min(em->max_tiles, (uint32_t)std::max(1, cus) * 8u));
  em->cus = (uint32_t)std::max(1, cus);
  if (kwk_status st = refresh_lens(em, 0, em->capacity)) return st;
  return KWK_OK;
}

}  // namespace

extern "C" {

const char* kwk_emit_last_error(const kwk_emitter* em) { return em ? em->err.c_str() : g_err.c_str(); }

kwk_status kwk_emitter_create(kwk_engine* eng, uint32_t capacity, const kwk_emit_program* prog, kwk_emitter** out) {
  ErrScope es_(nullptr);
  if (!eng || !prog || !out) return fail(KWK_EINVAL, "null argument");
  if (capacity > (1u << 27)) return fail(KWK_EINVAL, "capacity above 2^27 slots");
  if (kwk_status st = check_program(prog)) return st;
  void* s = nullptr;
  if (kwk_stream(eng, &s) != KWK_OK) return fail(KWK_EINVAL, std::string("kwk_stream: ") + kwk_last_error(eng));
  auto* em = new kwk_emitter();
  em->eng = eng;
  em->stream = static_cast<hipStream_t>(s);
  em->capacity = capacity;
  em->layout_epoch = kwk_layout_epoch(eng);
  hipError_t e = hipStreamGetDevice(em->stream, &em->device);
  if (e != hipSuccess) {
    delete em;
    return fail(KWK_EHIP, std::string("hipStreamGetDevice: ") + hipGetErrorString(e));
  }
  kwk_status st = bind(em);
  if (!st) st = emitter_init(em, prog);
  if (st) {
    delete em;
    return st;
  }
  *out = em;
  return KWK_OK;
}

kwk_status kwk_emitter_destroy(kwk_emitter* em) {
  delete em;
  return KWK_OK;
}

kwk_status kwk_emit_set_words(kwk_emitter* em, uint32_t first, uint32_t n, const uint64_t* words) {
  ErrScope es_(em ? &em->err : nullptr);
  if (!em || (n && !words)) return fail(KWK_EINVAL, "null argument");
  if ((uint64_t)first + n > em->capacity) return fail(KWK_EINVAL, "rows beyond the capacity");
  if (kwk_status st = bind(em)) return st;
  if (kwk_status st = copy_in(em, em->d_words + first, words, (size_t)n * 8)) return st;
  return refresh_lens(em, first, n);
}

kwk_status kwk_emit_get_words(kwk_emitter* em, uint32_t first, uint32_t n, uint64_t* words) {
  ErrScope es_(em ? &em->err : nullptr);
  if (!em || (n && !words)) return fail(KWK_EINVAL, "null argument");
  if ((uint64_t)first + n > em->capacity) return fail(KWK_EINVAL, "rows beyond the capacity");
  if (kwk_status st = bind(em)) return st;
  if (kwk_status st = copy_out(em, words, em->d_words + first, (size_t)n * 8)) return st;
  for (uint32_t i = 0; i < n; ++i) words[i] &= ~(0xFFull << 24);  // (the device's length cache)
  return KWK_OK;
}

kwk_status kwk_emit_set_column(kwk_emitter* em, uint32_t c, uint32_t first, uint32_t n, const uint8_t* data) {
  ErrScope es_(em ? &em->err : nullptr);
  if (!em || (n && !data)) return fail(KWK_EINVAL, "null argument");
  if (c >= em->n_columns) return fail(KWK_EINVAL, "column out of range");
  if ((uint64_t)first + n > em->capacity) return fail(KWK_EINVAL, "rows beyond the capacity");
  if (kwk_status st = bind(em)) return st;
  if (kwk_status st = copy_in(em, em->cols[c] + (size_t)first * em->stride[c], data, (size_t)n * em->stride[c])) return st;
  return refresh_lens(em, first, n);
}

}  // extern "C"

namespace {

// room of max_items / max_bytes in each of n_sets output sets (the stream idle afterwards); a set
// that grows loses its emission's outputs, another number of sets starts the rotation over
kwk_status reserve_sets(kwk_emitter* em, uint32_t n_sets, uint32_t max_items, uint64_t max_bytes) {
  if (kwk_status st = bind(em)) return st;
  HIP_TRY(hipStreamSynchronize(em->stream));
  if (n_sets != em->sets.size())
    if (kwk_status st = make_sets(em, n_sets)) return st;
  for (kwk_emitter::OutSet& o : em->sets) {
    if (max_items > o.cap_items) {
      o.cap_items = 0;
      HIP_TRY(o.d_items.alloc(max_items));
      HIP_TRY(o.d_offsets.alloc((size_t)max_items + 1));
      o.cap_items = max_items;
    }
    if (max_bytes > o.cap_bytes) {
      o.cap_bytes = 0;
      HIP_TRY(o.d_out.alloc((size_t)max_bytes));
      o.cap_bytes = max_bytes;
    }
  }
  if (em->fin) {  // the finalizer stream's room, in every set
    for (kwk_emitter::OutSet& o : em->sets) {
      if (em->fin_req_items > o.fin_cap_items || !o.d_fin_offsets) {
        o.fin_cap_items = 0;
        const size_t ni = (size_t)std::max<uint64_t>(1, em->fin_req_items);
        HIP_TRY(o.d_fin_items.alloc(ni));
        HIP_TRY(o.d_fin_offsets.alloc(ni + 1));
        o.fin_cap_items = ni;
      }
      if (em->fin_req_bytes > o.fin_cap_bytes || !o.d_fin_out) {
        o.fin_cap_bytes = 0;
        const size_t nb = (size_t)std::max<uint64_t>(1, em->fin_req_bytes);
        HIP_TRY(o.d_fin_out.alloc(nb + 16));
        o.fin_cap_bytes = nb;
      }
    }
  }
  if (em->evt) {  // the event stream's room, in every set
    for (kwk_emitter::OutSet& o : em->sets) {
      if (em->evt_req_items > o.evt_cap_items || !o.d_evt_offsets) {
        o.evt_cap_items = 0;
        const size_t ni = (size_t)std::max<uint64_t>(1, em->evt_req_items);
        HIP_TRY(o.d_evt_items.alloc(ni));
        HIP_TRY(o.d_evt_offsets.alloc(ni + 1));
        o.evt_cap_items = ni;
      }
      if (em->evt_req_bytes > o.evt_cap_bytes || !o.d_evt_out) {
        o.evt_cap_bytes = 0;
        const size_t nb = (size_t)std::max<uint64_t>(1, em->evt_req_bytes);
        HIP_TRY(o.d_evt_out.alloc(nb + 16));
        o.evt_cap_bytes = nb;
      }
    }
  }
  if (em->sticky_armed) {  // the host reserves again: later emissions run
    if (kwk_status st = fill(em, em->d_sticky, 0, 4)) return st;
    em->sticky_armed = false;
  }
  em->saw_cap = false;
  return KWK_OK;
}

// the three launches (five for the 2-byte source) of one emission into the next output set; `a`
// holds the list (recs / packed / p16 ..., count)
kwk_status enqueue_emission(kwk_emitter* em, EmitArgs& a, int64_t now_ns) {
  if (kwk_status st = bind(em)) return st;
  if (!em->sets[0].d_offsets)
    if (kwk_status st = reserve_sets(em, (uint32_t)em->sets.size(), 1, 1)) return st;
  if (em->fin && !em->sets[0].d_fin_offsets)
    if (kwk_status st = reserve_sets(em, (uint32_t)em->sets.size(), 0, 0)) return st;
  if (em->evt && !em->sets[0].d_evt_offsets)
    if (kwk_status st = reserve_sets(em, (uint32_t)em->sets.size(), 0, 0)) return st;
  if (em->evt && now_ns < 0) return fail(KWK_EINVAL, "an event program is loaded: now_ns < 0");
  const bool src16 = a.p16 != nullptr;
  if (src16) HIP_TRY(em->d_seg_base.grow((size_t)a.n_segs + 1u));  // (its free synchronises the device: no kernel still reads it)
  const uint32_t n_sets = (uint32_t)em->sets.size();
  kwk_emitter::OutSet& o = em->sets[(em->cur + 1u) % n_sets];
  a.p = em->p;
  a.words = em->d_words;
  a.capacity = em->capacity;
  a.max_recs = (em->max_tiles - 1) * kTile;
  a.tile_items = em->d_tile_items;
  a.tile_bytes = em->d_tile_bytes;
  a.totals = o.d_totals;
  a.items = o.d_items;
  a.offsets = o.d_offsets;
  a.out = o.d_out;
  a.cap_items = o.cap_items;
  a.cap_bytes = o.cap_bytes;
  a.lencache = em->lencache ? 1u : 0u;
  a.sticky = em->d_sticky;
  a.sticky_on = n_sets > 1u ? 1u : 0u;  // (one set: every emission stands alone, as before the sets)
  a.seg_base = em->d_seg_base;
  a.tile_seg = em->d_tile_seg;
  const std::string now = kwkfmt::rfc3339nano(now_ns);
  if (now.size() >= sizeof a.now) return fail(KWK_EINVAL, "Now() text too long");
  memcpy(a.now, now.data(), now.size());
  a.now_len = (uint32_t)now.size();
  // (one set with a finalizer program: the flag only joins the emission's two streams — a finalizer
  // overflow stops its merge-patch writer — and every emission stands alone, so it starts cleared)
  if ((em->saw_cap || ((em->fin || em->evt) && n_sets == 1u)) && em->sticky_armed) {  // the host has seen the overflow and emits again
    HIP_TRY(hipMemsetAsync(em->d_sticky, 0, 4, em->stream));
    em->sticky_armed = false;
  }
  em->saw_cap = false;
  if (a.sticky_on || em->fin || em->evt) em->sticky_armed = true;
  FinArgs f = em->f;
  EmitArgs fa = a;  // emit_scan_kernel over the finalizer stream's tile arrays and totals
  if (em->fin) {
    f.totals = o.d_fin_totals;
    f.items = o.d_fin_items;
    f.offsets = o.d_fin_offsets;
    f.out = o.d_fin_out;
    f.cap_items = o.fin_cap_items;
    f.cap_bytes = o.fin_cap_bytes;
    fa.tile_items = f.tile_items;
    fa.tile_bytes = f.tile_bytes;
    fa.totals = f.totals;
    fa.cap_items = f.cap_items;
    fa.cap_bytes = f.cap_bytes;
    fa.sticky_on = 1u;
  }
  EvtArgs e = em->e;
  EmitArgs ea = a;  // emit_scan_kernel over the event stream's tile arrays and totals
  if (em->evt) {
    e.totals = o.d_evt_totals;
    e.items = o.d_evt_items;
    e.offsets = o.d_evt_offsets;
    e.out = o.d_evt_out;
    e.cap_items = o.evt_cap_items;
    e.cap_bytes = o.evt_cap_bytes;
    char hex[24];
    const int hn = snprintf(hex, sizeof hex, ".%llx", (unsigned long long)now_ns);
    const std::string b = std::string(hex, (size_t)hn) + "\",\"namespace\":\"";
    memset(e.b, 0, sizeof e.b);
    memcpy(e.b, b.data(), b.size());  // (at most 1 + 16 + 15 bytes)
    e.b_len = (uint32_t)b.size();
    e.base_bytes = em->evt_fixed + e.b_len;
    // metav1.Time: whole seconds (20 bytes for every now_ns >= 0 an int64_t holds: the year is at most 2262)
    const std::string ts = kwkfmt::rfc3339nano(now_ns / 1000000000 * 1000000000);
    memcpy(e.ts, ts.data(), std::min(ts.size(), sizeof e.ts));
    ea.tile_items = e.tile_items;
    ea.tile_bytes = e.tile_bytes;
    ea.totals = e.totals;
    ea.cap_items = e.cap_items;
    ea.cap_bytes = e.cap_bytes;
    ea.sticky_on = 1u;
  }
  // the list's count lives on the device: every tile loop reads it; the grid covers the capacity
  HIP_TRY(hipEventRecord(o.ev0, em->stream));
  bool lds = em->p.n_pieces <= kLdsPieces && em->p.n_lits + 8u <= kLdsLits && em->p.n_skels <= kLdsSkels;
  bool vals16 = em->n_columns <= kLdsCols;
  for (uint32_t c = 0; c < em->n_columns; ++c) vals16 = vals16 && em->stride[c] == 16u;
  if (src16) {
    hipLaunchKernelGGL(emit_seg_base_kernel, dim3(1), dim3(kScanBlock), 0, em->stream, a);
    HIP_TRY(hipGetLastError());
    const uint32_t sgrid = std::max(1u, std::min((a.n_segs + kBlock - 1u) / kBlock, em->cus * 8u));
    hipLaunchKernelGGL(emit_tile_seg_kernel, dim3(sgrid), dim3(kBlock), 0, em->stream, a);
    HIP_TRY(hipGetLastError());
    if (lds)
      hipLaunchKernelGGL((emit_size_kernel<true, kSrc16>), dim3(em->grid), dim3(kBlock), 0, em->stream, a);
    else
      hipLaunchKernelGGL((emit_size_kernel<false, kSrc16>), dim3(em->grid), dim3(kBlock), 0, em->stream, a);
  } else if (lds) {
    hipLaunchKernelGGL(emit_size_kernel<true>, dim3(em->grid), dim3(kBlock), 0, em->stream, a);
  } else {
    hipLaunchKernelGGL(emit_size_kernel<false>, dim3(em->grid), dim3(kBlock), 0, em->stream, a);
  }
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(emit_scan_kernel, dim3(1), dim3(kScanBlock), 0, em->stream, a);
  HIP_TRY(hipGetLastError());
  if (em->fin && !em->fin_any) {  // no stage has a finalizers op: an empty stream, no launch
    HIP_TRY(hipMemsetAsync(f.totals, 0, 5 * 8, em->stream));
  } else if (em->fin) {  // sized and scanned before either writer runs: an overflow of one stream stops both
    if (src16) hipLaunchKernelGGL(emit_fin_size_kernel<kSrc16>, dim3(em->grid), dim3(kBlock), 0, em->stream, a, f);
    else hipLaunchKernelGGL(emit_fin_size_kernel<kSrc32>, dim3(em->grid), dim3(kBlock), 0, em->stream, a, f);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(emit_scan_kernel, dim3(1), dim3(kScanBlock), 0, em->stream, fa);
    HIP_TRY(hipGetLastError());
  }
  if (em->evt && !em->evt_any) {  // no stage records an Event: an empty stream, no launch
    HIP_TRY(hipMemsetAsync(e.totals, 0, 5 * 8, em->stream));
  } else if (em->evt) {  // sized and scanned before any writer runs: an overflow of one stream stops all three
    if (src16) hipLaunchKernelGGL(emit_evt_size_kernel<kSrc16>, dim3(em->grid), dim3(kBlock), 0, em->stream, a, e);
    else hipLaunchKernelGGL(emit_evt_size_kernel<kSrc32>, dim3(em->grid), dim3(kBlock), 0, em->stream, a, e);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(emit_scan_kernel, dim3(1), dim3(kScanBlock), 0, em->stream, ea);
    HIP_TRY(hipGetLastError());
  }
  const bool wl = lds && vals16;  // the write kernel's LDS path also stages the value rows
  // the chunk writer: templates (literals + Now per slot) within kTplBytes, pieces in skeleton order
  const bool chunk = wl && em->chunk_ok && em->tpl_lits + (uint64_t)em->tpl_now_slots * a.now_len + 16u <= kTplBytes;
  const void* wk = src16 ? (chunk ? (const void*)emit_write_kernel<true, true, kSrc16>
                            : wl  ? (const void*)emit_write_kernel<true, false, kSrc16>
                                  : (const void*)emit_write_kernel<false, false, kSrc16>)
                         : (chunk ? (const void*)emit_write_kernel<true, true>
                            : wl  ? (const void*)emit_write_kernel<true, false>
                                  : (const void*)emit_write_kernel<false, false>);
  void* wargs[] = {&a};
  // the write kernel's grid: every block resident at once (one round; its tile loop does the rest)
  const int vi = (chunk ? 0 : wl ? 1 : 2) + (src16 ? 3 : 0);
  if (!em->write_occ[vi]) {
    int occ = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, wk, kBlock, 0));
    em->write_occ[vi] = std::max(1, occ);
  }
  const uint32_t wgrid = std::max(1u, std::min(em->max_tiles, em->cus * (uint32_t)em->write_occ[vi]));
  HIP_TRY(hipLaunchKernel(wk, dim3(wgrid), dim3(kBlock), wargs, 0, em->stream));
  HIP_TRY(hipGetLastError());
  if (em->fin && em->fin_any) {
    if (src16) hipLaunchKernelGGL(emit_fin_write_kernel<kSrc16>, dim3(em->grid), dim3(kBlock), 0, em->stream, a, f);
    else hipLaunchKernelGGL(emit_fin_write_kernel<kSrc32>, dim3(em->grid), dim3(kBlock), 0, em->stream, a, f);
    HIP_TRY(hipGetLastError());
  }
  if (em->evt && em->evt_any) {
    if (src16) hipLaunchKernelGGL(emit_evt_write_kernel<kSrc16>, dim3(em->grid), dim3(kBlock), 0, em->stream, a, e);
    else hipLaunchKernelGGL(emit_evt_write_kernel<kSrc32>, dim3(em->grid), dim3(kBlock), 0, em->stream, a, e);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(o.ev1, em->stream));
  o.emitted = true;
  em->cur = (em->cur + 1u) % n_sets;
  em->n_emitted = std::min(em->n_emitted + 1u, n_sets);
  em->sel = 0;
  return KWK_OK;
}

}  // namespace

extern "C" {

kwk_status kwk_emit_reserve(kwk_emitter* em, uint32_t max_items, uint64_t max_bytes) {
  ErrScope es_(em ? &em->err : nullptr);
  if (!em) return fail(KWK_EINVAL, "null emitter");
  return reserve_sets(em, (uint32_t)em->sets.size(), max_items, max_bytes);
}

kwk_status kwk_emit_reserve_sets(kwk_emitter* em, uint32_t n_sets, uint32_t max_items, uint64_t max_bytes) {
  ErrScope es_(em ? &em->err : nullptr);
  if (!em) return fail(KWK_EINVAL, "null emitter");
  if (n_sets < 1u || n_sets > kMaxSets) return fail(KWK_EINVAL, "kwk_emit_reserve_sets: 1..8 output sets");
  return reserve_sets(em, n_sets, max_items, max_bytes);
}

kwk_status kwk_emit_select(kwk_emitter* em, uint32_t back) {
  ErrScope es_(em ? &em->err : nullptr);
  if (!em) return fail(KWK_EINVAL, "null emitter");
  if (back >= em->sets.size())
    return fail(KWK_EINVAL, "kwk_emit_select: the emitter has " + std::to_string(em->sets.size()) + " output set(s)");
  if (back && back >= em->n_emitted)
    return fail(KWK_ESTATE, "kwk_emit_select: only " + std::to_string(em->n_emitted) + " emission(s) since the sets were made");
  em->sel = back;
  return KWK_OK;
}

// the words, order words, value columns and event rows are per slot: after a kwk_relayout they
// belong to other objects, so nothing is emitted from them (reading them back stays allowed: the
// host permutes them for the new emitter)
static kwk_status same_layout_epoch(const kwk_emitter* em) {
  if (kwk_layout_epoch(em->eng) == em->layout_epoch) return KWK_OK;
  return fail(KWK_ESTATE, "the engine's slot layout changed (kwk_relayout, epoch " + std::to_string(kwk_layout_epoch(em->eng)) +
                              ", emitter created at " + std::to_string(em->layout_epoch) +
                              "): create an emitter for the new layout (kwk_emitter_create) and set its words and columns");
}

kwk_status kwk_emit(kwk_emitter* em, int64_t now_ns, uint32_t source) {
  ErrScope es_(em ? &em->err : nullptr);
  if (!em) return fail(KWK_EINVAL, "null emitter");
  if (kwk_status st = same_layout_epoch(em)) return st;
  EmitArgs a{};
  const uint32_t from = source & 0xFFu;
  if (from != KWK_EMIT_FROM_RECORDS && from != KWK_EMIT_FROM_PACKED)
    return fail(KWK_EINVAL, "source must be KWK_EMIT_FROM_RECORDS or KWK_EMIT_FROM_PACKED");
  const void* list = nullptr;
  if (kwk_fired_device(em->eng, from == KWK_EMIT_FROM_PACKED ? KWK_COMPACT_PACKED : KWK_COMPACT_REC, &list, &a.count) !=
      KWK_OK)
    return fail(KWK_ESTATE, std::string("kwk_fired_device: ") + kwk_last_error(em->eng));
  if (from == KWK_EMIT_FROM_PACKED) a.packed = static_cast<const uint32_t*>(list);
  else a.recs = static_cast<const kwk_fired_rec*>(list);
  if (source & ~0xFFu) return fail(KWK_EINVAL, "unknown source flags");
  return enqueue_emission(em, a, now_ns);
}

kwk_status kwk_emit_step(kwk_emitter* em, uint64_t step, int64_t now_ns) {
  ErrScope es_(em ? &em->err : nullptr);
  if (!em) return fail(KWK_EINVAL, "null emitter");
  if (kwk_status st = same_layout_epoch(em)) return st;
  kwk_fired_view v;
  if (kwk_ring_view(em->eng, step, &v) != KWK_OK)
    return fail(KWK_ESTATE, std::string("kwk_ring_view: ") + kwk_last_error(em->eng));
  EmitArgs a{};
  a.count = v.count;
  switch (v.format) {
    case KWK_COMPACT_REC: a.recs = static_cast<const kwk_fired_rec*>(v.list); break;
    case KWK_COMPACT_PACKED: a.packed = static_cast<const uint32_t*>(v.list); break;
    case KWK_COMPACT_PACKED16:
      if (!v.seg_counts) return fail(KWK_ESTATE, "the 2-byte list of step " + std::to_string(v.step) + " has no segment counts");
      a.p16 = static_cast<const uint16_t*>(v.list);
      a.seg_counts = v.seg_counts;
      a.n_segs = v.n_segs;
      a.region_slots = v.region_slots;
      break;
    case KWK_COMPACT_BITS:
      return fail(KWK_ESTATE, "the list of step " + std::to_string(v.step) +
                                  " is in KWK_COMPACT_BITS: the bitmap format is not emitted (compact it as "
                                  "KWK_COMPACT_PACKED16, _PACKED or _REC)");
    default: return fail(KWK_ESTATE, "the list of step " + std::to_string(v.step) + " is in an unknown format");
  }
  if (v.n_segs == 0) {  // a step that swept nothing: an empty list, whatever its length word holds
    a.recs = nullptr;
    a.packed = nullptr;
    a.p16 = nullptr;
    a.count = em->d_zero;
  }
  return enqueue_emission(em, a, now_ns);
}

kwk_status kwk_emit_result(kwk_emitter* em, uint32_t* n_items, uint64_t* n_bytes) {
  ErrScope es_(em ? &em->err : nullptr);
  if (!em || !n_items || !n_bytes) return fail(KWK_EINVAL, "null argument");
  const kwk_emitter::OutSet& o = em->selected();
  if (!o.emitted) return fail(KWK_ESTATE, "kwk_emit must come first");
  if (kwk_status st = bind(em)) return st;
  unsigned long long t[5];
  if (kwk_status st = copy_out(em, t, o.d_totals, sizeof t)) return st;
  *n_items = (uint32_t)t[0];
  *n_bytes = t[1];
  if (t[4]) {
    em->saw_cap = true;
    return fail(KWK_ECAP, "an earlier emission in flight exceeded its reservation: nothing was written — reserve "
                          "and emit again from the first step that failed");
  }
  if (t[2]) {
    em->saw_cap = true;
    return fail(KWK_ECAP, "the fired list is longer than the emitter's capacity");
  }
  if (t[0] > o.cap_items || t[1] > o.cap_bytes) {
    em->saw_cap = true;
    return fail(KWK_ECAP, "emission exceeds the reservation: kwk_emit_reserve(" + std::to_string(t[0]) + ", " +
                              std::to_string(t[1]) + ") and emit again");
  }
  if (em->fin && o.d_fin_totals) {
    unsigned long long ft[2];
    if (kwk_status st = copy_out(em, ft, o.d_fin_totals, sizeof ft)) return st;
    if (ft[0] > o.fin_cap_items || ft[1] > o.fin_cap_bytes) {
      em->saw_cap = true;
      return fail(KWK_ECAP, "the emission's finalizer patches exceed their reservation: kwk_emit_reserve_fin(" +
                                std::to_string(ft[0]) + ", " + std::to_string(ft[1]) + ") and emit again");
    }
  }
  if (em->evt && o.d_evt_totals) {
    unsigned long long et[2];
    if (kwk_status st = copy_out(em, et, o.d_evt_totals, sizeof et)) return st;
    if (et[0] > o.evt_cap_items || et[1] > o.evt_cap_bytes) {
      em->saw_cap = true;
      return fail(KWK_ECAP, "the emission's events exceed their reservation: kwk_evt_reserve(" + std::to_string(et[0]) +
                                ", " + std::to_string(et[1]) + ") and emit again");
    }
  }
  return KWK_OK;
}

kwk_status kwk_emit_stats(kwk_emitter* em, uint32_t* n_items, uint32_t* n_emitted, uint64_t* n_bytes) {
  ErrScope es_(em ? &em->err : nullptr);
  if (!em || !n_items || !n_emitted || !n_bytes) return fail(KWK_EINVAL, "null argument");
  if (kwk_status st = kwk_emit_result(em, n_items, n_bytes)) return st;
  unsigned long long t = 0;
  if (kwk_status st = copy_out(em, &t, em->selected().d_totals + 3, 8)) return st;
  *n_emitted = (uint32_t)t;
  return KWK_OK;
}

kwk_status kwk_emit_device(kwk_emitter* em, const kwk_emit_item** items, const uint64_t** offsets, const char** bytes) {
  ErrScope es_(em ? &em->err : nullptr);
  if (!em) return fail(KWK_EINVAL, "null emitter");
  const kwk_emitter::OutSet& o = em->selected();
  if (items) *items = o.d_items;
  if (offsets) *offsets = o.d_offsets;
  if (bytes) *bytes = o.d_out;
  return KWK_OK;
}

kwk_status kwk_emit_copy(kwk_emitter* em, kwk_emit_item* items, uint64_t* offsets, char* bytes) {
  ErrScope es_(em ? &em->err : nullptr);
  uint32_t ni = 0;
  uint64_t nb = 0;
  if (kwk_status st = kwk_emit_result(em, &ni, &nb)) return st;
  if ((ni && (!items || !offsets)) || (nb && !bytes) || !offsets) return fail(KWK_EINVAL, "null argument");
  const kwk_emitter::OutSet& o = em->selected();
  if (ni) {
    if (kwk_status st = copy_out(em, items, o.d_items, (size_t)ni * sizeof(kwk_emit_item))) return st;
    if (kwk_status st = copy_out(em, offsets, o.d_offsets, ((size_t)ni + 1) * 8)) return st;
  } else {
    offsets[0] = 0;
  }
  if (kwk_status st = copy_out(em, bytes, o.d_out, (size_t)nb)) return st;
  return KWK_OK;
}

kwk_status kwk_emit_elapsed(kwk_emitter* em, float* ms) {
  ErrScope es_(em ? &em->err : nullptr);
  if (!em || !ms) return fail(KWK_EINVAL, "null argument");
  const kwk_emitter::OutSet& o = em->selected();
  if (!o.emitted) return fail(KWK_ESTATE, "kwk_emit must come first");
  if (kwk_status st = bind(em)) return st;
  HIP_TRY(hipEventSynchronize(o.ev1));
  HIP_TRY(hipEventElapsedTime(ms, o.ev0, o.ev1));
  return KWK_OK;
}


kwk_status kwk_emit_finalizers_load(kwk_emitter* em, const kwk_emit_fin_program* g) {
  ErrScope es_(em ? &em->err : nullptr);
  if (!em || !g) return fail(KWK_EINVAL, "null argument");
  if (em->fin) return fail(KWK_ESTATE, "kwk_emit_finalizers_load: the emitter has a finalizer program");
  if (g->n_values > 15u)
    return fail(KWK_EINVAL, "finalizer program: " + std::to_string(g->n_values) + " dictionary values (more than 15)");
  if (g->n_stages != em->p.n_stages || g->n_stages > KWK_MAX_STAGES)
    return fail(KWK_EINVAL, "finalizer program: " + std::to_string(g->n_stages) + " stages, the emit program has " +
                                std::to_string(em->p.n_stages));
  if ((g->n_values && (!g->value_off || !g->values)) || (g->n_stages && (!g->stage_flags || !g->stage_remove || !g->stage_add_ptr)))
    return fail(KWK_EINVAL, "finalizer program: null array");
  std::vector<std::string> vals;
  for (uint32_t i = 0; i < g->n_values; ++i) {
    if (g->value_off[i + 1] < g->value_off[i]) return fail(KWK_EINVAL, "finalizer program: value offsets");
    vals.emplace_back(g->values + g->value_off[i], g->values + g->value_off[i + 1]);
    for (const char c : vals.back())
      if (!((c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z') || (c >= '0' && c <= '9') || c == '.' || c == '_' || c == '/' ||
            c == '-'))
        return fail(KWK_EINVAL, "finalizer program: value \"" + vals.back() + "\" has a byte outside [A-Za-z0-9._/-]");
  }
  std::vector<std::string> lit(kFinLitMax);
  lit[kFinLitRemoveAll] = "{\"op\":\"remove\",\"path\":\"/metadata/finalizers\"}";
  for (uint32_t k = 0; k < 7u; ++k)
    lit[kFinLitRemoveIdx + k] = "{\"op\":\"remove\",\"path\":\"/metadata/finalizers/" + std::to_string(k) + "\"}";
  for (uint32_t i = 0; i < g->n_values; ++i)
    lit[kFinLitAddId + i] = "{\"op\":\"add\",\"path\":\"/metadata/finalizers/-\",\"value\":\"" + vals[i] + "\"}";
  std::vector<uint4> stages(std::max(1u, g->n_stages), make_uint4(0u, 0u, 0u, 0u));
  if (g->n_stages && g->stage_add_ptr[0] != 0) return fail(KWK_EINVAL, "finalizer program: stage_add_ptr[0] != 0");
  for (uint32_t s = 0; s < g->n_stages; ++s) {
    const uint32_t a0 = g->stage_add_ptr[s], a1 = g->stage_add_ptr[s + 1];
    if (a1 < a0 || a1 - a0 > kFinMaxAdd)
      return fail(KWK_EINVAL, "finalizer program: stage " + std::to_string(s) + " adds more than 16 values");
    if (a1 > a0 && !g->stage_add) return fail(KWK_EINVAL, "finalizer program: null array");
    if (g->stage_remove[s] >> g->n_values) return fail(KWK_EINVAL, "finalizer program: remove id out of range");
    uint64_t adds = 0;
    std::string whole = "{\"op\":\"add\",\"path\":\"/metadata/finalizers\",\"value\":[";
    for (uint32_t j = a0; j < a1; ++j) {
      const uint32_t id = g->stage_add[j];
      if (id >= g->n_values) return fail(KWK_EINVAL, "finalizer program: add id out of range");
      adds |= (uint64_t)id << (4u * (j - a0));
      whole += (j > a0 ? ",\"" : "\"") + vals[id] + "\"";
    }
    if (a1 > a0) lit[kFinLitAddList + s] = whole + "]}";
    const uint32_t keep = KWK_NEXT_DELETE | KWK_NEXT_FIN | KWK_NEXT_FIN_EMPTY | KWK_NEXT_FIN_REMOVE;
    stages[s] = make_uint4((uint32_t)g->stage_remove[s] | (g->stage_flags[s] & keep) << 16 | (a1 - a0) << 24, (uint32_t)adds,
                           (uint32_t)(adds >> 32), 0u);
  }
  std::vector<uint32_t> ent(kFinLitMax, 0u);
  std::string bytes;
  for (uint32_t i = 0; i < kFinLitMax; ++i) {
    if (bytes.size() + lit[i].size() > kFinLitBytes)
      return fail(KWK_EINVAL, "finalizer program: more than " + std::to_string(kFinLitBytes) + " bytes of op literals");
    ent[i] = (uint32_t)bytes.size() | (uint32_t)lit[i].size() << 16;
    bytes += lit[i];
  }
  bytes.resize((bytes.size() + 3u) & ~size_t(3), '\0');
  std::vector<uint32_t> words(std::max<size_t>(1, bytes.size() / 4), 0u);
  memcpy(words.data(), bytes.data(), bytes.size());
  if (kwk_status st = bind(em)) return st;
  HIP_TRY(hipStreamSynchronize(em->stream));
  em->fm = kwk_emitter::FinMem{};  // (what an earlier, failed load left: the stream is idle)
  FinArgs f{};
  if (kwk_status st = upload(em, em->fm.stages, &f.stages, stages.data(), stages.size())) return st;
  if (kwk_status st = upload(em, em->fm.lit, &f.lit, ent.data(), ent.size())) return st;
  if (kwk_status st = upload(em, em->fm.lits, &f.lits, words.data(), words.size())) return st;
  f.n_stages = g->n_stages;
  f.n_lit_words = (uint32_t)(bytes.size() / 4);
  HIP_TRY(em->fm.words.alloc(std::max(1u, em->capacity)));
  if (kwk_status st = fill(em, em->fm.words, 0, em->fm.words.size() * 4)) return st;
  f.words = em->fm.words;
  HIP_TRY(em->fm.tile_items.alloc(em->max_tiles));
  f.tile_items = em->fm.tile_items;
  HIP_TRY(em->fm.tile_bytes.alloc(em->max_tiles));
  f.tile_bytes = em->fm.tile_bytes;
  DevBuf<unsigned long long> totals;  // the emitter's once it is zeroed (make_sets looks at d_fin_totals_all)
  HIP_TRY(totals.alloc(kMaxSets * 8));
  if (kwk_status st = fill(em, totals, 0, kMaxSets * 8 * 8)) return st;
  em->d_fin_totals_all = std::move(totals);
  for (size_t i = 0; i < em->sets.size(); ++i) em->sets[i].d_fin_totals = em->d_fin_totals_all + 8u * i;
  em->f = f;
  em->fin = true;
  for (uint32_t s = 0; s < g->n_stages; ++s) em->fin_any = em->fin_any || (g->stage_flags[s] & KWK_NEXT_FIN);
  return KWK_OK;
}

kwk_status kwk_emit_set_fin_words(kwk_emitter* em, uint32_t first, uint32_t n, const uint32_t* words) {
  ErrScope es_(em ? &em->err : nullptr);
  if (!em || (n && !words)) return fail(KWK_EINVAL, "null argument");
  if (!em->fin) return fail(KWK_ESTATE, "kwk_emit_finalizers_load must come first");
  if ((uint64_t)first + n > em->capacity) return fail(KWK_EINVAL, "rows beyond the capacity");
  if (kwk_status st = bind(em)) return st;
  return copy_in(em, em->f.words + first, words, (size_t)n * 4);
}

kwk_status kwk_emit_get_fin_words(kwk_emitter* em, uint32_t first, uint32_t n, uint32_t* words) {
  ErrScope es_(em ? &em->err : nullptr);
  if (!em || (n && !words)) return fail(KWK_EINVAL, "null argument");
  if (!em->fin) return fail(KWK_ESTATE, "kwk_emit_finalizers_load must come first");
  if ((uint64_t)first + n > em->capacity) return fail(KWK_EINVAL, "rows beyond the capacity");
  if (kwk_status st = bind(em)) return st;
  return copy_out(em, words, em->f.words + first, (size_t)n * 4);
}

kwk_status kwk_emit_reserve_fin(kwk_emitter* em, uint32_t max_items, uint64_t max_bytes) {
  ErrScope es_(em ? &em->err : nullptr);
  if (!em) return fail(KWK_EINVAL, "null emitter");
  if (!em->fin) return fail(KWK_ESTATE, "kwk_emit_finalizers_load must come first");
  em->fin_req_items = max_items;  // (a set keeps the room it has; sets made later get this)
  em->fin_req_bytes = max_bytes;
  return reserve_sets(em, (uint32_t)em->sets.size(), 0, 0);
}

kwk_status kwk_emit_fin_result(kwk_emitter* em, uint32_t* n_items, uint64_t* n_bytes) {
  ErrScope es_(em ? &em->err : nullptr);
  if (!em || !n_items || !n_bytes) return fail(KWK_EINVAL, "null argument");
  if (!em->fin) return fail(KWK_ESTATE, "kwk_emit_finalizers_load must come first");
  uint32_t mi = 0;
  uint64_t mb = 0;
  const kwk_status st = kwk_emit_result(em, &mi, &mb);
  if (st != KWK_OK && st != KWK_ECAP) return st;
  unsigned long long ft[2] = {0, 0};
  const std::string msg = em->err;
  if (em->selected().d_fin_totals)
    if (kwk_status s2 = copy_out(em, ft, em->selected().d_fin_totals, sizeof ft)) return s2;
  *n_items = (uint32_t)ft[0];
  *n_bytes = ft[1];
  return st == KWK_OK ? KWK_OK : fail(st, msg);
}

kwk_status kwk_emit_fin_device(kwk_emitter* em, const kwk_emit_fin_item** items, const uint64_t** offsets,
                               const char** bytes) {
  ErrScope es_(em ? &em->err : nullptr);
  if (!em) return fail(KWK_EINVAL, "null emitter");
  if (!em->fin) return fail(KWK_ESTATE, "kwk_emit_finalizers_load must come first");
  const kwk_emitter::OutSet& o = em->selected();
  if (items) *items = o.d_fin_items;
  if (offsets) *offsets = o.d_fin_offsets;
  if (bytes) *bytes = o.d_fin_out;
  return KWK_OK;
}

kwk_status kwk_emit_fin_copy(kwk_emitter* em, kwk_emit_fin_item* items, uint64_t* offsets, char* bytes) {
  ErrScope es_(em ? &em->err : nullptr);
  uint32_t ni = 0;
  uint64_t nb = 0;
  if (kwk_status st = kwk_emit_fin_result(em, &ni, &nb)) return st;
  if ((ni && !items) || (nb && !bytes) || !offsets) return fail(KWK_EINVAL, "null argument");
  const kwk_emitter::OutSet& o = em->selected();
  if (ni) {
    if (kwk_status st = copy_out(em, items, o.d_fin_items, (size_t)ni * sizeof(kwk_emit_fin_item))) return st;
    if (kwk_status st = copy_out(em, offsets, o.d_fin_offsets, ((size_t)ni + 1) * 8)) return st;
  } else {
    offsets[0] = 0;
  }
  if (kwk_status st = copy_out(em, bytes, o.d_fin_out, (size_t)nb)) return st;
  return KWK_OK;
}

// ---- Events (kwok_events.h)

// a kwk_evt_program checked and turned into the kernels' tables (no emitter, no device)
struct EvtBuilt {
  EvtArgs e{};
  std::vector<uint4> stages;
  std::vector<uint32_t> tw, cw;  // the tails' and the shared literals' bytes as dwords
  std::string tails;
  bool any = false, use_ns = false;
  uint32_t strides[3] = {0, 0, 0};
  uint32_t fixed = 0;
};

static kwk_status evt_build(const kwk_evt_program* g, EvtBuilt& out) {
  if (!g->kind || !g->api_version || !g->component || (g->n_stages && (!g->stage_flags || !g->text_off || !g->text)))
    return fail(KWK_EINVAL, "event program: null pointer");
  if (g->n_stages > KWK_MAX_STAGES)  // (the kernels' per-stage LDS tables hold KWK_MAX_STAGES entries)
    return fail(KWK_EINVAL, "event program: " + std::to_string(g->n_stages) + " stages (more than " +
                                std::to_string(KWK_MAX_STAGES) + ")");
  // only text that json.Marshal writes unchanged: printable ASCII without " \\ < > &
  auto plain = [](const std::string& v, const char* what, std::string& bad) {
    for (const char ch : v) {
      const unsigned char b = (unsigned char)ch;
      if (b < 0x20 || b > 0x7E || b == '"' || b == '\\' || b == '<' || b == '>' || b == '&') {
        char hex[8];
        snprintf(hex, sizeof hex, "0x%02x", b);
        bad = std::string("event program: ") + what + " has byte " + hex + " (outside 0x20..0x7E or one of \" \\ < > &)";
        return false;
      }
    }
    return true;
  };
  std::string bad;
  const std::string kind = g->kind, av = g->api_version, comp = g->component;
  if (!plain(kind, "kind", bad) || !plain(av, "api_version", bad) || !plain(comp, "component", bad)) return fail(KWK_EINVAL, bad);
  if (kind.size() > 63) return fail(KWK_EINVAL, "event program: kind longer than 63 bytes");
  const uint32_t strides[3] = {g->stride_name, g->stride_namespace, g->stride_uid};
  const char* const cols[3] = {"name", "namespace", "uid"};
  for (int c = 0; c < 3; ++c) {
    if (c == 1 && strides[c] == 0) continue;  // a cluster-scoped kind: no column
    if (strides[c] < 4 || strides[c] > 256 || strides[c] % 4)
      return fail(KWK_EINVAL, std::string("event program: the ") + cols[c] + " stride must be a multiple of 4 in 4..256");
  }
  // the typed Node controller passes no namespace (node_controller.go:369): the column is not read
  out.use_ns = strides[1] != 0 && !(av.empty() && kind == "Node");
  // the shared literals, each at a 4-byte aligned offset
  std::string lits[kEvtLits];
  lits[kEvtLitA] = "{\"metadata\":{\"name\":\"";
  lits[kEvtLitC] = "\",\"creationTimestamp\":null},\"involvedObject\":{\"kind\":\"" + kind + "\"";
  lits[kEvtLitD] = ",\"namespace\":\"";
  lits[kEvtLitE1] = ",\"name\":\"";
  lits[kEvtLitE2] = "\",\"name\":\"";
  lits[kEvtLitF] = "\",\"uid\":\"";
  lits[kEvtLitDefault] = "default";
  EvtArgs& e = out.e;
  std::string com;
  for (uint32_t i = 0; i < kEvtLits; ++i) {
    e.com_ent[i] = (uint32_t)com.size() | (uint32_t)lits[i].size() << 16;
    com += lits[i];
    com.resize((com.size() + 3u) & ~size_t(3), '\0');
  }
  if (com.size() > kEvtComWords * 4) return fail(KWK_EINVAL, "event program: the shared literals do not fit");
  // the stages' tails: everything after the last inserted value, the timestamp's 20 bytes left blank twice
  std::vector<uint4>& stages = out.stages;
  stages.assign(std::max(1u, g->n_stages), make_uint4(0u, 0u, 0u, 0u));
  std::string& tails = out.tails;
  uint64_t text = 0;
  bool& any = out.any;
  any = false;
  for (uint32_t s = 0; s < g->n_stages; ++s) {
    if (!(g->stage_flags[s] & KWK_EVT_STAGE_EVENT)) continue;
    std::string f[3];
    static const char* const names[3] = {"type", "reason", "message"};
    for (int k = 0; k < 3; ++k) {
      const uint32_t o0 = g->text_off[3 * s + k], o1 = g->text_off[3 * s + k + 1];
      if (o1 < o0) return fail(KWK_EINVAL, "event program: text offsets");
      f[k].assign(g->text + o0, o1 - o0);
      if (!plain(f[k], names[k], bad)) return fail(KWK_EINVAL, bad + " (stage " + std::to_string(s) + ")");
      text += f[k].size();
    }
    if (f[0] != "Normal" && f[0] != "Warning")
      return fail(KWK_EINVAL, "event program: stage " + std::to_string(s) + " has type \"" + f[0] + "\" (generateEvent sends nothing)");
    std::string t = "\"";
    if (!av.empty()) t += ",\"apiVersion\":\"" + av + "\"";
    t += "},";
    if (!f[1].empty()) t += "\"reason\":\"" + f[1] + "\",";
    if (!f[2].empty()) t += "\"message\":\"" + f[2] + "\",";
    t += "\"source\":{\"component\":\"" + comp + "\"},\"firstTimestamp\":\"";
    const uint32_t off = (uint32_t)tails.size();
    const uint32_t t1 = off + (uint32_t)t.size();
    t += std::string(20, ' ') + "\",\"lastTimestamp\":\"";
    const uint32_t t2 = off + (uint32_t)t.size();
    t += std::string(20, ' ') + "\",\"count\":1,\"type\":\"" + f[0] + "\",\"eventTime\":null,\"reportingComponent\":\"" + comp +
         "\",\"reportingInstance\":\"\"}";
    stages[s] = make_uint4(off, (uint32_t)t.size(), t1, t2);
    tails += t;
    tails.resize((tails.size() + 3u) & ~size_t(3), '\0');
    any = true;
  }
  if (text > KWK_EVT_MAX_TEXT)
    return fail(KWK_EINVAL, "event program: " + std::to_string(text) + " bytes of stage text (more than " +
                                std::to_string(KWK_EVT_MAX_TEXT) + ")");
  if (tails.size() > kEvtTailBytes)
    return fail(KWK_EINVAL, "event program: " + std::to_string(tails.size()) + " bytes of stage tails (more than " +
                                std::to_string(kEvtTailBytes) + ")");
  out.tw.assign(std::max<size_t>(1, tails.size() / 4), 0u);
  out.cw.assign(com.size() / 4, 0u);
  memcpy(out.tw.data(), tails.data(), tails.size());
  memcpy(out.cw.data(), com.data(), com.size());
  for (int c = 0; c < 3; ++c) out.strides[c] = strides[c];
  out.fixed = (uint32_t)(lits[kEvtLitA].size() + lits[kEvtLitC].size() + lits[kEvtLitE1].size());
  return KWK_OK;
}

kwk_status kwk_evt_check(const kwk_evt_program* g) {
  ErrScope es_(nullptr);
  if (!g) return fail(KWK_EINVAL, "null argument");
  EvtBuilt b;
  return evt_build(g, b);
}

kwk_status kwk_evt_load(kwk_emitter* em, const kwk_evt_program* g) {
  ErrScope es_(em ? &em->err : nullptr);
  if (!em || !g) return fail(KWK_EINVAL, "null argument");
  if (em->evt) return fail(KWK_ESTATE, "kwk_evt_load: the emitter has an event program");
  EvtBuilt b;
  if (kwk_status st = evt_build(g, b)) return st;
  if (g->n_stages != em->p.n_stages)
    return fail(KWK_EINVAL, "event program: " + std::to_string(g->n_stages) + " stages, the emit program has " +
                                std::to_string(em->p.n_stages));
  EvtArgs e = b.e;
  const std::vector<uint4>& stages = b.stages;
  const std::vector<uint32_t>&tw = b.tw, &cw = b.cw;
  const std::string& tails = b.tails;
  const uint32_t* strides = b.strides;
  const bool use_ns = b.use_ns, any = b.any;
  if (kwk_status st = bind(em)) return st;
  HIP_TRY(hipStreamSynchronize(em->stream));
  em->evm = kwk_emitter::EvtMem{};  // (what an earlier, failed load left: the stream is idle)
  if (kwk_status st = upload(em, em->evm.stages, &e.stages, stages.data(), stages.size())) return st;
  if (kwk_status st = upload(em, em->evm.tails, &e.tails, tw.data(), tw.size())) return st;
  if (kwk_status st = upload(em, em->evm.com, &e.com, cw.data(), cw.size())) return st;
  e.n_tail_words = (uint32_t)(tails.size() / 4);
  e.n_com_words = (uint32_t)cw.size();
  e.n_stages = g->n_stages;
  for (int c = 0; c < 3; ++c) {
    e.stride[c] = strides[c];
    e.rows[c] = nullptr;
    if (c == 1 && !use_ns) continue;
    // (16 bytes more: the writer's dword reads may run one dword past the last row's text)
    const size_t bytes = (size_t)std::max(1u, em->capacity) * strides[c] + 16;
    HIP_TRY(em->evm.rows[c].alloc(bytes));
    if (kwk_status st = fill(em, em->evm.rows[c], 0xFF, bytes)) return st;  // every row unusable until set
    e.rows[c] = em->evm.rows[c];
  }
  HIP_TRY(em->evm.tile_items.alloc(em->max_tiles));
  e.tile_items = em->evm.tile_items;
  HIP_TRY(em->evm.tile_bytes.alloc(em->max_tiles));
  e.tile_bytes = em->evm.tile_bytes;
  DevBuf<unsigned long long> totals;  // the emitter's once it is zeroed (make_sets looks at d_evt_totals_all)
  HIP_TRY(totals.alloc(kMaxSets * 8));
  if (kwk_status st = fill(em, totals, 0, kMaxSets * 8 * 8)) return st;
  em->d_evt_totals_all = std::move(totals);
  for (size_t i = 0; i < em->sets.size(); ++i) em->sets[i].d_evt_totals = em->d_evt_totals_all + 8u * i;
  em->evt_fixed = b.fixed;
  em->e = e;
  em->evt = true;
  em->evt_any = any;
  return KWK_OK;
}

kwk_status kwk_evt_set_rows(kwk_emitter* em, uint32_t column, uint32_t first, uint32_t n, const uint8_t* data) {
  ErrScope es_(em ? &em->err : nullptr);
  if (!em || (n && !data)) return fail(KWK_EINVAL, "null argument");
  if (!em->evt) return fail(KWK_ESTATE, "kwk_evt_load must come first");
  if (column > KWK_EVT_COL_UID) return fail(KWK_EINVAL, "kwk_evt_set_rows: column must be KWK_EVT_COL_NAME, _NAMESPACE or _UID");
  if ((uint64_t)first + n > em->capacity) return fail(KWK_EINVAL, "rows beyond the capacity");
  if (!em->e.rows[column]) {
    if (column == KWK_EVT_COL_NAMESPACE && em->e.stride[column]) return KWK_OK;  // the typed Node reference has no namespace
    return fail(KWK_EINVAL, "kwk_evt_set_rows: the program has no namespace column (stride 0)");
  }
  const uint32_t stride = em->e.stride[column];
  for (uint32_t i = 0; i < n; ++i) {
    const uint8_t len = data[(size_t)i * stride];
    if (len != KWK_EVT_ROW_UNUSABLE && len > stride - 1u)
      return fail(KWK_EINVAL, "kwk_evt_set_rows: row " + std::to_string(first + i) + " has length " + std::to_string(len) +
                                  ", the stride holds " + std::to_string(stride - 1u));
  }
  if (kwk_status st = bind(em)) return st;
  return copy_in(em, em->evm.rows[column].get() + (size_t)first * stride, data, (size_t)n * stride);
}

kwk_status kwk_evt_reserve(kwk_emitter* em, uint32_t max_items, uint64_t max_bytes) {
  ErrScope es_(em ? &em->err : nullptr);
  if (!em) return fail(KWK_EINVAL, "null emitter");
  if (!em->evt) return fail(KWK_ESTATE, "kwk_evt_load must come first");
  em->evt_req_items = max_items;  // (a set keeps the room it has; sets made later get this)
  em->evt_req_bytes = max_bytes;
  return reserve_sets(em, (uint32_t)em->sets.size(), 0, 0);
}

kwk_status kwk_evt_result(kwk_emitter* em, uint32_t* n_items, uint64_t* n_bytes, uint32_t* launched) {
  ErrScope es_(em ? &em->err : nullptr);
  if (!em || !n_items || !n_bytes) return fail(KWK_EINVAL, "null argument");
  if (!em->evt) return fail(KWK_ESTATE, "kwk_evt_load must come first");
  uint32_t mi = 0;
  uint64_t mb = 0;
  const kwk_status st = kwk_emit_result(em, &mi, &mb);
  if (st != KWK_OK && st != KWK_ECAP) return st;
  unsigned long long et[2] = {0, 0};
  const std::string msg = em->err;
  if (em->selected().d_evt_totals)
    if (kwk_status s2 = copy_out(em, et, em->selected().d_evt_totals, sizeof et)) return s2;
  *n_items = (uint32_t)et[0];
  *n_bytes = et[1];
  if (launched) *launched = em->evt_any ? 1u : 0u;
  return st == KWK_OK ? KWK_OK : fail(st, msg);
}

kwk_status kwk_evt_device(kwk_emitter* em, const kwk_evt_item** items, const uint64_t** offsets, const char** bytes) {
  ErrScope es_(em ? &em->err : nullptr);
  if (!em) return fail(KWK_EINVAL, "null emitter");
  if (!em->evt) return fail(KWK_ESTATE, "kwk_evt_load must come first");
  const kwk_emitter::OutSet& o = em->selected();
  if (items) *items = o.d_evt_items;
  if (offsets) *offsets = o.d_evt_offsets;
  if (bytes) *bytes = o.d_evt_out;
  return KWK_OK;
}

kwk_status kwk_evt_copy(kwk_emitter* em, kwk_evt_item* items, uint64_t* offsets, char* bytes) {
  ErrScope es_(em ? &em->err : nullptr);
  uint32_t ni = 0;
  uint64_t nb = 0;
  if (kwk_status st = kwk_evt_result(em, &ni, &nb, nullptr)) return st;
  if ((ni && !items) || (nb && !bytes) || !offsets) return fail(KWK_EINVAL, "null argument");
  const kwk_emitter::OutSet& o = em->selected();
  if (ni) {
    if (kwk_status st = copy_out(em, items, o.d_evt_items, (size_t)ni * sizeof(kwk_evt_item))) return st;
    if (kwk_status st = copy_out(em, offsets, o.d_evt_offsets, ((size_t)ni + 1) * 8)) return st;
  } else {
    offsets[0] = 0;
  }
  if (kwk_status st = copy_out(em, bytes, o.d_evt_out, (size_t)nb)) return st;
  return KWK_OK;
}

}  // extern "C"
