// Device metric exposition (include/kwok_expo.h): the Prometheus text of a scrape, per node,
// written on the engine's stream from the device-evaluated values.
//
// Reference: UpdateHandler.Update + the promhttp text encoder (pkg/kwok/metrics/metrics.go:
// 480-502,525-573, pkg/kwok/server/metrics.go:129-150; expfmt text_create.go) — here the label
// blocks are rendered once per object on the host (kwk_metric_labels_render), sorted once per node
// (kwk_expo_commit), and only the values change per scrape.
//
// Three launches per scrape (no inter-workgroup waiting, no host round trip); the third template
// parameter is whether the program has histogram families (below):
//   expo_node_kernel<W, false, H> a workgroup of W lanes per node, family-major, series in the committed
//                                 order: line = name + block + ' ' + value + '\n' (dead pod slots: none).
//                                 Formats every live value once (f64fmt.hpp) into a 32-byte stash slot
//                                 (24 bytes + length) and sums the node's bytes with its HELP / TYPE lines
//   expo_scan_kernel              one workgroup: exclusive scan of the node totals into 64-bit offsets,
//                                 the grand total
//   expo_node_kernel<W, true, H>  the same walk; the lanes take a family's lines W at a time and a block scan
//                                 of their lengths gives each its offset in the node.  A wave's 64 lines are
//                                 one contiguous span: each lane assembles its line in LDS (8-byte words,
//                                 read from the sources as aligned 8-byte words), at the span's own
//                                 misalignment, and the wave stores the span as 16-byte vectors (bytes at
//                                 the two ends).  A span longer than the LDS window is written by its
//                                 lanes directly.  The kernel returns at once when the scanned total exceeds
//                                 the reservation, and every store is bounded by the node's scanned range.
// W = 64 (one wave per node) up to kWidePods pods per node, 256 above.
// Both choices were measured against their alternatives — lanes storing their lines directly, and
// formatting the value again in the write pass instead of the stash — at the C4 size (DESIGN.md
// "Device metric exposition", `ab_c4` in profiles/r7/expo_bench.json): this pair is the fastest of
// the four.
//
// Histogram families (kwk_expo_create_hist; kwk_expo_hist_program in kwok_metrics.h): a series is
// n_visible + 3 lines, so a family of a node is count x (n_visible + 3) lines and the lanes walk that
// line index space W at a time: lane L -> series L / lines (its row through the group's permutation),
// line L % lines, whose prefix and tail come from the per-line table and whose value is one word of the
// engine's histogram record (kwk_histograms_eval_device), float64(uint64) for a count, the float64
// bits for the sum.  Each printed word is formatted once, by the lengths pass, into the stash region
// after the scalars'.  The block scan, the LDS staging and the bounded stores are the scalar
// families'.  Only expo_node_kernel<W, ., true> knows any of this: a program without histogram
// families launches <W, ., false>, whose code has no histogram state.
//
// Label rows (the reference keeps its registry current per object, metrics.go:480-502): a group's
// blocks, and the sort keys of a pod or container group, live in an arena with an {offset, length}
// pair per row.  kwk_expo_commit lays every row out packed, sorted on the host; kwk_expo_commit_rows
// brings only the rows set since the last commit up to date, on the stream, without a host
// synchronisation:
//   expo_scatter_kernel  a wave per dirty row: its bytes from the staging copy to its slot (in place
//                        where they fit, else at the arena's tail), its pair
//   expo_sort_kernel     a workgroup per (node, group) that holds a dirty row: the node's slice of
//                        the permutation by a rank sort under the comparator of keycmp.hpp
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/kwok_expo.h"
#include "errscope.hpp"
#include "devmem.hpp"
#include "f64fmt.hpp"
#include "keycmp.hpp"

namespace {

constexpr uint32_t kScanBlock = 1024;
constexpr uint32_t kFmtBlock = 256;
constexpr uint32_t kWidePods = 256;  // pods per node (mean) above which a node gets 256 lanes (64 is faster at 100)

struct DevFamily {
  uint32_t name_off, name_len, header_off, header_len;
  uint32_t dim, group;
  uint32_t before[3];  // gauges / counters of each dimension before this family's in CR order (its value offset);
                       // a histogram family: record words per series of the histograms before its own
  uint32_t hist;       // 0: a gauge / counter; else 1 + its index in ExpoArgs.hist
};

struct DevHist {
  uint32_t nvis, line0;  // n_visible; its n_visible + 3 entries of ExpoArgs.hlines
};

struct DevGroup {
  const uint2* blk_ref;  // per row: {offset, length} of its block in the arena (NULL: no labels; length 0: never set)
  const char* blk;       // the arena (8 readable bytes after every block)
  const uint32_t* perm;  // per node's row range: the rows in key order (NULL: node rows)
};

struct ExpoArgs {
  const DevFamily* fam;
  const DevGroup* grp;
  const char* lits;
  const uint32_t* node_ptr;
  const uint32_t* cptr;
  const uint32_t* pod_of;   // per container: its pod slot
  const uint32_t* alive;    // bit per pod slot of the range
  const double* vals;
  uint32_t n_fam, n0, n_nodes, p0, p1, c0, c1;
  unsigned long long* node_bytes;  // n_nodes
  unsigned long long* offsets;     // n_nodes + 1
  unsigned long long* total;       // [0] the text's size, [1] live series of a labelled group whose row was never set
  char* out;
  unsigned long long cap;
  uint4* stash;  // 32 bytes per value: its formatted bytes and their count (lengths pass -> write pass)
  // histogram families (expo_node_kernel<., ., true> only)
  const DevHist* hist;
  const kwk_expo_hist_line* hlines;
  const unsigned long long* hvals;  // the engine's histogram records
  unsigned long long n_vals;        // the scalars' values: the histogram words' stash slots follow theirs
};

constexpr uint32_t kLdsWave = 12288;  // LDS window of one wave's 64 lines (C4 lines: ~105 bytes)

// a value's formatted bytes (at most 24) in three registers
struct RegSink {
  uint64_t w0 = 0, w1 = 0, w2 = 0;
  uint32_t n = 0;
  __device__ __forceinline__ void put(char c) {
    const uint64_t x = (uint64_t)(uint8_t)c << (8 * (n & 7u));
    if (n < 8) w0 |= x;
    else if (n < 16) w1 |= x;
    else w2 |= x;
    ++n;
  }
};

// bytes of one line, 8 at a time where a whole aligned word is the line's own
template <class C8, class U64>
struct LineSinkT {
  C8* out;
  unsigned long long at;   // address (offset in out) of byte 0 of the current word
  unsigned long long end;  // the node's scanned end: nothing is stored at or beyond it
  uint64_t acc;
  uint32_t n, lo;          // bytes of the word filled so far; the first that is this line's
  __device__ __forceinline__ void open(C8* o, unsigned long long pos, unsigned long long e) {
    out = o;
    end = e;
    lo = (uint32_t)(pos & 7u);
    at = pos - lo;
    n = lo;
    acc = 0;
  }
  __device__ __forceinline__ void flush() {
    if (lo == 0 && n == 8) {
      if (at + 8 <= end) *reinterpret_cast<U64*>(out + at) = acc;
    } else {
      for (uint32_t b = lo; b < n; ++b)
        if (at + b < end) out[at + b] = (char)(acc >> (8 * b));
    }
    at += 8;
    acc = 0;
    n = 0;
    lo = 0;
  }
  __device__ __forceinline__ void put(char c) {
    acc |= (uint64_t)(uint8_t)c << (8 * n);
    if (++n == 8) flush();
  }
  // k <= 8 bytes, the low ones of x
  __device__ __forceinline__ void push(uint64_t x, uint32_t k) {
    if (k < 8) x &= (1ull << (8 * k)) - 1ull;
    const uint32_t nn = n + k;
    acc |= x << (8 * n);
    if (nn >= 8) {
      const uint64_t rest = n ? x >> (8 * (8 - n)) : 0ull;
      n = 8;
      flush();
      acc = rest;
      n = nn - 8;
    } else {
      n = nn;
    }
  }
  // len bytes at src, read as the aligned 8-byte words that hold them (the arrays are padded by 8)
  __device__ __forceinline__ void run(const char* __restrict__ src, uint32_t len) {
    if (!len) return;
    const uint32_t sa = (uint32_t)((size_t)src & 7u);
    const uint64_t* w = reinterpret_cast<const uint64_t*>(src - sa);
    uint64_t cur = *w >> (8 * sa);
    uint32_t avail = 8 - sa;
    for (;;) {
      const uint32_t k = avail < len ? avail : len;
      push(cur, k);
      len -= k;
      if (!len) break;
      cur = *++w;
      avail = 8;
    }
  }
  __device__ __forceinline__ void close() {
    if (n > lo) flush();
  }
};
using LineSink = LineSinkT<char, uint64_t>;
typedef __attribute__((address_space(3))) char lds_c8;
typedef __attribute__((address_space(3))) uint64_t lds_u64;
using LdsSink = LineSinkT<lds_c8, lds_u64>;

__device__ __forceinline__ uint32_t wave_incl(uint32_t v, uint32_t lane) {
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t t = __shfl_up(v, d, 64);
    if (lane >= d) v += t;
  }
  return v;
}

// exclusive offset of this lane's `len` among the workgroup's, and their total (every lane calls)
template <uint32_t W>
__device__ __forceinline__ uint32_t block_excl(uint32_t len, uint32_t* s_wave, uint32_t& total) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t incl = wave_incl(len, lane);
  if (W == 64) {
    total = __shfl(incl, 63, 64);
    return incl - len;
  }
  constexpr uint32_t kWaves = W / 64;
  uint32_t* s = s_wave;  // read before the caller's next barrier: the write loop has two between calls
  if (lane == 63) s[threadIdx.x >> 6] = incl;
  __syncthreads();
  uint32_t base = 0, t = 0;
#pragma unroll
  for (uint32_t w = 0; w < kWaves; ++w) {
    const uint32_t x = s[w];
    if (w < (threadIdx.x >> 6)) base += x;
    t += x;
  }
  total = t;
  return base + incl - len;
}

template <uint32_t W, bool kWrite, bool kHist>
__global__ __launch_bounds__(W) void expo_node_kernel(ExpoArgs a) {
  __shared__ __attribute__((aligned(16))) char s_stage[kWrite ? (W / 64) * kLdsWave : 16];
  __shared__ uint32_t s_wave[W / 64];
  __shared__ unsigned long long s_sum[W / 64];
  const uint32_t j = blockIdx.x, tid = threadIdx.x;
  if (j >= a.n_nodes) return;
  unsigned long long pos = 0, end = 0, sum = 0;
  if (kWrite) {
    // the text does not fit the reservation, or a live series has no labels: nothing is written
    if (a.total[0] > a.cap || a.total[1] != 0) return;
    pos = a.offsets[j];
    end = a.offsets[j + 1];
  }
  const uint32_t node = a.n0 + j;
  const uint32_t pb = a.node_ptr[node], pe = a.node_ptr[node + 1];
  const uint32_t cb = a.cptr[pb], ce = a.cptr[pe];
  for (uint32_t f = 0; f < a.n_fam; ++f) {
    const DevFamily F = a.fam[f];
    const DevGroup G = a.grp[F.group];
    if (kWrite) {
      for (uint32_t i = tid; i < F.header_len; i += W)
        if (pos + i < end) a.out[pos + i] = a.lits[F.header_off + i];
      pos += F.header_len;
    } else if (tid == 0) {
      sum += F.header_len;
    }
    const uint32_t first = F.dim == KWK_METRIC_DIM_NODE ? node : F.dim == KWK_METRIC_DIM_POD ? pb : cb;
    const uint32_t count = F.dim == KWK_METRIC_DIM_NODE ? 1u : F.dim == KWK_METRIC_DIM_POD ? pe - pb : ce - cb;
    const uint32_t base = F.dim == KWK_METRIC_DIM_NODE ? a.n0 : F.dim == KWK_METRIC_DIM_POD ? a.p0 : a.c0;
    const unsigned long long voff = (unsigned long long)F.before[0] * a.n_nodes + (unsigned long long)F.before[1] * (a.p1 - a.p0) +
                                    (unsigned long long)F.before[2] * (a.c1 - a.c0);
    const double* vals = a.vals + voff;
    // a histogram family: `lines` lines per series, the lanes walk count x lines
    const bool hist = kHist && F.hist != 0;
    uint32_t lines = 1, nvis = 0, line0 = 0;
    if (hist) {
      const DevHist H = a.hist[F.hist - 1];
      nvis = H.nvis;
      line0 = H.line0;
      lines = nvis + 3;
    }
    const uint32_t n_lines = count * lines;  // fits: kwk_expo_commit bounds a node's rows
    for (uint32_t s0 = 0; s0 < n_lines; s0 += W) {
      uint32_t s = s0 + tid, k = 0;
      const bool mine = s < n_lines;
      if (hist) {
        const uint32_t q = s / lines;
        k = s - q * lines;
        s = q;
      }
      uint32_t len = 0, row = 0, bo = 0, bl = 0;
      uint32_t po = F.name_off, pl = F.name_len, to = 0, tl = 0;  // the line's prefix and tail in lits
      double v = 0.0;
      RegSink rs;
      if (mine) {
        row = G.perm ? G.perm[first + s] : first + s;
        bool alive = true;
        if (F.dim != KWK_METRIC_DIM_NODE) {
          const uint32_t pod = (F.dim == KWK_METRIC_DIM_POD ? row : a.pod_of[row]) - a.p0;
          alive = (a.alive[pod >> 5] >> (pod & 31u)) & 1u;
        }
        if (alive) {
          if (G.blk_ref) {
            const uint2 ref = G.blk_ref[row];
            bo = ref.x;
            bl = ref.y;
            // a rendered block is never empty ("{..}"); a histogram series counts once, not per line
            if (!kWrite && bl == 0 && k == 0) atomicAdd(&a.total[1], 1ull);
          }
          size_t slot = (size_t)voff + (row - base);
          if (hist) {
            const kwk_expo_hist_line ln = a.hlines[line0 + k];
            po = ln.prefix_off;
            pl = ln.prefix_len;
            to = ln.tail_off;
            tl = ln.tail_len;
            if (bl) --bl;  // the block without its closing brace: the tail closes it
            // text order buckets, +Inf, _sum, _count; record order counts, +Inf, count, sum
            const uint32_t w = k <= nvis ? k : k == nvis + 1 ? nvis + 2 : nvis + 1;
            const size_t rec = (size_t)voff + (size_t)(row - base) * lines;
            slot = (size_t)a.n_vals + rec + k;
            if (!kWrite) {
              const unsigned long long x = a.hvals[rec + w];
              v = w == nvis + 2 ? __longlong_as_double((long long)x) : (double)x;  // float64(uint64): nearest even
            }
          } else {
            v = vals[row - base];
          }
          // the value's text: formatted once, by the lengths pass
          uint4* st = a.stash + 2 * slot;
          if (!kWrite) {
            kwkf64::format(v, rs);
            st[0] = make_uint4((uint32_t)rs.w0, (uint32_t)(rs.w0 >> 32), (uint32_t)rs.w1, (uint32_t)(rs.w1 >> 32));
            st[1] = make_uint4((uint32_t)rs.w2, (uint32_t)(rs.w2 >> 32), rs.n, 0u);
          } else {
            const uint4 x = st[0], y = st[1];
            rs.w0 = x.x | (uint64_t)x.y << 32;
            rs.w1 = x.z | (uint64_t)x.w << 32;
            rs.w2 = y.x | (uint64_t)y.y << 32;
            rs.n = y.z < (uint32_t)kwkf64::kMaxBytes ? y.z : (uint32_t)kwkf64::kMaxBytes;
          }
          len = pl + bl + tl + 2u + rs.n;
        }
      }
      if (!kWrite) {
        sum += len;
      } else {
        uint32_t total;
        const uint32_t at = block_excl<W>(len, s_wave, total);
        // this wave's lines are one contiguous span: staged in LDS at the span's own misalignment and
        // stored as 16-byte vectors (a span beyond the window goes the direct way)
        const uint32_t lane = tid & 63u;
        const uint32_t wfirst = __shfl(at, 0, 64), wtotal = __shfl(at + len, 63, 64) - wfirst;
        const unsigned long long gbase = pos + wfirst;
        const uint32_t mis = (uint32_t)(gbase & 15u);
        const bool staged = mis + wtotal <= kLdsWave;
        char* stage = s_stage + (tid >> 6) * kLdsWave;
        auto line = [&](auto& o) {
          o.run(a.lits + po, pl);
          o.run(G.blk + bo, bl);
          if (kHist) o.run(a.lits + to, tl);
          o.put(' ');
          o.push(rs.w0, rs.n < 8 ? rs.n : 8u);
          if (rs.n > 8) o.push(rs.w1, rs.n < 16 ? rs.n - 8 : 8u);
          if (rs.n > 16) o.push(rs.w2, rs.n - 16);
          o.put('\n');
          o.close();
        };
        if (len) {
          if (staged) {
            LdsSink o;
            o.open((lds_c8*)stage, mis + (at - wfirst), mis + wtotal);
            line(o);
          } else {
            LineSink o;
            o.open(a.out, pos + at, end);
            line(o);
          }
        }
        __syncthreads();
        if (staged) {
          const unsigned long long g0 = gbase - mis;  // 16-byte aligned
          const uint32_t hi = mis + wtotal;
          for (uint32_t q = 16 * lane; q < hi; q += 16 * 64) {
            if (q >= mis && q + 16 <= hi) {
              if (g0 + q + 16 <= end) *reinterpret_cast<uint4*>(a.out + g0 + q) = *reinterpret_cast<const uint4*>(stage + q);
            } else {
              for (uint32_t b = q < mis ? mis : q; b < q + 16 && b < hi; ++b)
                if (g0 + b < end) a.out[g0 + b] = stage[b];
            }
          }
        }
        __syncthreads();
        pos += total;
      }
    }
  }
  if (!kWrite) {
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1) sum += __shfl_down(sum, d, 64);
    if (W == 64) {
      if (tid == 0) a.node_bytes[j] = sum;
    } else {
      if ((tid & 63u) == 0) s_sum[tid >> 6] = sum;
      __syncthreads();
      if (tid == 0) {
        unsigned long long t = 0;
        for (uint32_t w = 0; w < W / 64; ++w) t += s_sum[w];
        a.node_bytes[j] = t;
      }
    }
  }
}

// offsets[j] = sum of node_bytes[0 .. j), offsets[n] = *total = the text's size
__global__ __launch_bounds__(kScanBlock) void expo_scan_kernel(const unsigned long long* __restrict__ node_bytes, uint32_t n,
                                                               unsigned long long* __restrict__ offsets,
                                                               unsigned long long* __restrict__ total) {
  __shared__ unsigned long long s_wave[kScanBlock / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  unsigned long long carry = 0;
  for (uint32_t b = 0; b < n; b += kScanBlock) {
    const uint32_t i = b + tid;
    const unsigned long long v = i < n ? node_bytes[i] : 0ull;
    unsigned long long incl = v;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
      const unsigned long long t = __shfl_up(incl, d, 64);
      if (lane >= d) incl += t;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    unsigned long long base = 0, chunk = 0;
    for (uint32_t w = 0; w < kScanBlock / 64; ++w) {
      const unsigned long long x = s_wave[w];
      if (w < wave) base += x;
      chunk += x;
    }
    if (i < n) offsets[i] = carry + base + incl - v;
    carry += chunk;
    __syncthreads();
  }
  if (tid == 0) {
    offsets[n] = carry;
    *total = carry;
  }
}

__global__ __launch_bounds__(kFmtBlock) void expo_format_kernel(const double* __restrict__ v, uint32_t n, char* __restrict__ out,
                                                                uint8_t* __restrict__ lens) {
  const uint32_t i = blockIdx.x * kFmtBlock + threadIdx.x;
  if (i >= n) return;
  lens[i] = (uint8_t)kwkf64::format_f64(v[i], out + (size_t)i * kwkf64::kMaxBytes);
}

// Incremental commits (kwk_expo_commit_rows).  One staging buffer per call holds, in this order, the
// table of every group's arenas, the scrape's DevGroup table, the scatter rows, the sort segments and
// the bytes; the kernels read the tables from the device copy of the staging itself.
struct ArenaDev {
  char* base;  // a group's block arena, key arena, or its permutation array (as bytes)
  uint2* ref;  // per row {offset, length} (NULL: the permutation)
};
constexpr uint32_t kArenas = 3;  // per group: 0 blocks, 1 keys, 2 permutation

struct ScatterRow {
  unsigned long long dst, src;  // byte offsets in the arena and in the staging
  uint32_t len, row, arena, pad;
};

struct SortSeg {
  uint32_t lo, hi, group, pad;  // rows [lo, hi) of a node
};

constexpr uint32_t kScatterBlock = 256;  // a wave per row
constexpr uint32_t kSortBlock = 256;
constexpr uint32_t kSortMax = KWK_EXPO_SORT_MAX_ROWS;  // a node's rows sorted on the device (their pairs fit LDS)
// row i of the staging -> its arena slot and its {offset, length} pair
__global__ __launch_bounds__(kScatterBlock) void expo_scatter_kernel(const ArenaDev* __restrict__ tab,
                                                                     const ScatterRow* __restrict__ rows, uint32_t n,
                                                                     const char* __restrict__ stage) {
  const uint32_t i = blockIdx.x * (kScatterBlock / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (i >= n) return;
  const ScatterRow R = rows[i];
  const ArenaDev A = tab[R.arena];
  for (uint32_t b = lane; b < R.len; b += 64) A.base[R.dst + b] = stage[R.src + b];
  if (lane == 0 && A.ref) A.ref[R.row] = make_uint2((uint32_t)R.dst, R.len);
}

// One workgroup per (node, group) segment: perm[lo .. hi) = the segment's rows in key order, ties by
// row (std::stable_sort over ascending rows).  A rank sort: row i's place is the count of rows before
// it in that order.  The pairs sit in LDS (every lane reads pair j at once: a broadcast), the keys are
// read from the arena, a few KB per node that stay in the vector L1.
// (Copying the node's keys to LDS first and comparing them there was measured and dropped: 44 KiB of
// LDS per workgroup, and at 10k nodes the kernel took 7.4 ms against 6.2 ms — DESIGN.md "Incremental
// label commits".)
__global__ __launch_bounds__(kSortBlock) void expo_sort_kernel(const ArenaDev* __restrict__ tab,
                                                               const SortSeg* __restrict__ segs) {
  __shared__ uint2 s_ref[kSortMax];
  const SortSeg S = segs[blockIdx.x];
  const uint32_t n = S.hi - S.lo;
  if (S.hi < S.lo || n > kSortMax) return;  // (the host sorts a larger segment itself)
  const ArenaDev K = tab[kArenas * S.group + 1];
  uint32_t* perm = reinterpret_cast<uint32_t*>(tab[kArenas * S.group + 2].base);
  for (uint32_t i = threadIdx.x; i < n; i += kSortBlock) s_ref[i] = K.ref[S.lo + i];
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < n; i += kSortBlock) {
    const uint2 ri = s_ref[i];
    uint32_t rank = 0;
    for (uint32_t j = 0; j < n; ++j) {
      const uint2 rj = s_ref[j];
      const int c = kwkkey::compare(K.base + rj.x, rj.y, K.base + ri.x, ri.y);
      rank += (c < 0 || (c == 0 && j < i)) ? 1u : 0u;
    }
    perm[S.lo + rank] = S.lo + i;
  }
}

// a group's blocks or keys on the device: rows at any offset of one buffer, and what the host knows of it
struct Arena {
  DevBuf<char> d;
  DevBuf<uint2> d_ref;
  uint64_t size = 0, tail = 0;     // bytes allocated; the first free byte (tail + 8 <= size, both multiples of 8)
  std::vector<uint32_t> off, cap;  // per row: its slot
};

struct Group {
  uint32_t dim = 0, n_labels = 0;
  std::vector<std::string> blocks, keys;  // per row
  std::vector<uint32_t> dirty;            // rows set since the last commit of either kind
  std::vector<uint8_t> is_dirty;          // per row
  Arena blk, key;                         // key: groups with a permutation only
  DevBuf<uint32_t> d_perm;
};

struct Pending {  // device buffers replaced by an incremental commit: freed once the stream has passed `ev`
  Event ev;
  std::vector<DevBuf<char>> bufs;
};

constexpr uint64_t kArenaMax = 0xFFFFFFF8ull;  // 32-bit offsets
inline uint64_t up8(uint64_t x) { return (x + 7ull) & ~7ull; }

}  // namespace

struct kwk_expo {
  std::string err;
  kwk_engine* eng = nullptr;  // must outlive the writer
  uint64_t layout_epoch = 0;  // the engine's kwk_layout_epoch at create: the slot and node layout the writer is for
  hipStream_t stream = nullptr;  // the engine's stream as of the current call (it may be re-created)
  int device = 0;
  uint32_t n_nodes = 0, n_pods = 0, n_cont = 0, width = 0;
  DevBuf<uint4> d_stash;
  std::vector<DevFamily> fam;
  std::vector<DevHist> hist;  // of the histogram families' histograms (empty: a scalar-only program)
  uint32_t max_lines = 1;     // most lines of a series
  std::vector<Group> groups;
  std::vector<uint32_t> h_node_ptr, h_cptr;
  DevBuf<DevFamily> d_fam;
  DevBuf<DevHist> d_hist;
  DevBuf<kwk_expo_hist_line> d_hlines;
  DevBuf<DevGroup> d_grp;
  DevBuf<char> d_lits;
  DevBuf<uint32_t> d_pod_of;
  DevBuf<unsigned long long> d_node_bytes;
  DevBuf<unsigned long long> d_offsets;
  DevBuf<unsigned long long> d_total;
  DevBuf<char> d_out;
  uint64_t cap_bytes = 0;
  Event ev[5];
  bool committed = false, scraped = false;
  uint32_t last_nodes = 0;
  // incremental commits
  bool full = false;               // a full commit has laid the arenas out (and no later call left them half written)
  hipStream_t aux = nullptr;       // the layout totals are read here, beside the engine's stream
  HostBuf<uint32_t> h_totals;     // pinned: the device's node_ptr[n_nodes], cptr[n_pods]
  HostBuf<char> h_stage;           // pinned staging and its device copy
  DevBuf<char> d_stage;
  Event ev_stage;                  // the last copy out of h_stage
  bool stage_busy = false;
  Event ev_rows[3];                // around the last commit's scatter and sort kernels
  bool rows_timed = false;
  std::vector<Pending> pending;

  // the device is set and both streams are idle before the members free themselves
  ~kwk_expo() {
    hipSetDevice(device);
    void* s = nullptr;
    if (eng && kwk_stream(eng, &s) == KWK_OK && s) hipStreamSynchronize(static_cast<hipStream_t>(s));
    if (aux) {
      hipStreamSynchronize(aux);
      hipStreamDestroy(aux);
    }
    pending.clear();  // the streams are idle
  }
};

namespace {

kwk_status bind(kwk_expo* ex) {
  void* s = nullptr;
  if (kwk_stream(ex->eng, &s) != KWK_OK || !s) return fail(KWK_ESTATE, std::string("kwk_stream: ") + kwk_last_error(ex->eng));
  ex->stream = static_cast<hipStream_t>(s);
  HIP_TRY(hipSetDevice(ex->device));
  return KWK_OK;
}

// copies ordered on the engine's (non-blocking) stream
kwk_status copy_in(kwk_expo* ex, void* dst, const void* src, size_t bytes) {
  HIP_TRY(copy_in(ex->stream, dst, src, bytes));
  return KWK_OK;
}

kwk_status copy_out(kwk_expo* ex, void* dst, const void* src, size_t bytes) {
  HIP_TRY(copy_out(ex->stream, dst, src, bytes));
  return KWK_OK;
}

// makes dst a device copy of n items (the stream is idle: callers synchronise first)
template <typename T>
kwk_status upload(kwk_expo* ex, DevBuf<T>& dst, const T* src, size_t n) {
  HIP_TRY(dst.alloc(std::max<size_t>(1, n)));
  return copy_in(ex, dst, src, n * sizeof(T));
}

uint32_t group_rows(const kwk_expo* ex, uint32_t dim) {
  return dim == KWK_METRIC_DIM_NODE ? ex->n_nodes : dim == KWK_METRIC_DIM_POD ? ex->n_pods : ex->n_cont;
}

// the engine's node_ptr / cptr as of now (host copies), the row counts of every group
kwk_status refresh_layout(kwk_expo* ex) {
  const uint32_t *np = nullptr, *cp = nullptr, *al = nullptr;
  if (kwk_metrics_series_device(ex->eng, 0, ex->n_nodes, &np, &cp, &al) != KWK_OK)
    return fail(KWK_ESTATE, std::string("kwk_metrics_series_device: ") + kwk_last_error(ex->eng));
  ex->h_node_ptr.resize((size_t)ex->n_nodes + 1);
  if (kwk_status st = copy_out(ex, ex->h_node_ptr.data(), np, 4 * ex->h_node_ptr.size())) return st;
  ex->n_pods = ex->h_node_ptr[ex->n_nodes];
  ex->h_cptr.resize((size_t)ex->n_pods + 1);
  if (kwk_status st = copy_out(ex, ex->h_cptr.data(), cp, 4 * ex->h_cptr.size())) return st;
  ex->n_cont = ex->h_cptr[ex->n_pods];
  for (Group& g : ex->groups) {
    g.blocks.resize(group_rows(ex, g.dim));
    g.keys.resize(group_rows(ex, g.dim));
    g.is_dirty.resize(group_rows(ex, g.dim));
  }
  return KWK_OK;
}

// frees what earlier incremental commits replaced, where the stream has passed their event
// (all = true: the stream is idle)
void drain_pending(kwk_expo* ex, bool all) {
  auto passed = [all](const Pending& p) { return all || hipEventQuery(p.ev) == hipSuccess; };
  ex->pending.erase(std::remove_if(ex->pending.begin(), ex->pending.end(), passed), ex->pending.end());
}

// a full commit's layout of one arena: the set rows packed in row order, slack at the tail
kwk_status pack_arena(kwk_expo* ex, Arena& a, const std::vector<std::string>& items, const char* what) {
  const size_t rows = items.size();
  a.off.assign(rows, 0u);
  a.cap.assign(rows, 0u);
  std::vector<uint2> ref(rows);
  uint64_t total = 0;
  for (size_t r = 0; r < rows; ++r) {
    const uint64_t n = items[r].size();
    if (total + n + 8 > kArenaMax) return fail(KWK_ECAP, std::string("more than 4 GiB of label ") + what + " in a group");
    a.off[r] = (uint32_t)total;
    a.cap[r] = (uint32_t)n;
    ref[r] = make_uint2((uint32_t)total, (uint32_t)n);
    total += n;
  }
  a.tail = up8(total);
  a.size = std::min<uint64_t>(kArenaMax, a.tail + up8(a.tail / 8) + 4096);
  std::string blob;
  blob.reserve(a.tail + 8);
  for (const std::string& b : items) blob += b;
  blob.append(a.tail + 8 - total, '\0');  // read as 8-byte words
  a.d_ref.reset();
  HIP_TRY(a.d.alloc((size_t)a.size));
  if (kwk_status st = copy_in(ex, a.d, blob.data(), blob.size())) return st;
  return upload(ex, a.d_ref, ref.data(), ref.size());
}

}  // namespace

extern "C" {

const char* kwk_expo_last_error(const kwk_expo* ex) { return ex ? ex->err.c_str() : g_err.c_str(); }

uint32_t kwk_expo_format_f64(double v, char out[24]) { return kwkf64::format_f64(v, out); }

}  // extern "C"

namespace {

// kwk_expo_create (hp = NULL: a histogram family is refused) and kwk_expo_create_hist
kwk_status create(kwk_engine* pods, uint32_t n_nodes, const kwk_expo_program* prog, const kwk_expo_hist_program* hp,
                  kwk_expo** out) {
  ErrScope es_(nullptr);
  if (!pods || !prog || !out) return fail(KWK_EINVAL, "null argument");
  if ((prog->n_families && (!prog->families || !prog->lits)) || (prog->n_groups && !prog->groups) ||
      (prog->n_metrics && !prog->metric_dimension))
    return fail(KWK_EINVAL, "exposition program: null array");
  if (hp && ((hp->n_hists && !hp->hists) || (hp->n_lines && !hp->lines)))
    return fail(KWK_EINVAL, "histogram exposition program: null array");
  std::vector<DevFamily> fam;
  std::vector<DevHist> hist;
  uint32_t max_lines = 1;
  for (uint32_t f = 0; f < prog->n_families; ++f) {
    const kwk_expo_family& F = prog->families[f];
    if ((uint64_t)F.name_off + F.name_len > prog->n_lit_bytes || (uint64_t)F.header_off + F.header_len > prog->n_lit_bytes)
      return fail(KWK_EINVAL, "exposition program: family " + std::to_string(f) + " bytes beyond lits");
    const std::string name(prog->lits + F.name_off, F.name_len);
    if (F.reserved > KWK_EXPO_KIND_HISTOGRAM)
      return fail(KWK_EINVAL, "exposition program: family " + std::to_string(f) + " ('" + name + "') has an unknown kind code");
    DevFamily d{};
    d.name_off = F.name_off; d.name_len = F.name_len; d.header_off = F.header_off; d.header_len = F.header_len;
    d.dim = F.dimension; d.group = F.group;
    if (F.reserved == KWK_EXPO_KIND_HISTOGRAM) {
      if (!hp)
        return fail(KWK_EINVAL, "exposition program: family " + std::to_string(f) + " ('" + name + "') is a histogram: "
                                "kwk_expo_create_hist takes its tables (kwk_metric_set_exposition_histograms)");
      if (F.group >= prog->n_groups || F.metric >= hp->n_hists || F.dimension > KWK_METRIC_DIM_CONTAINER ||
          prog->groups[F.group].dimension != F.dimension || hp->hists[F.metric].dimension != F.dimension)
        return fail(KWK_EINVAL, "exposition program: family " + std::to_string(f) + " group / histogram / dimension");
      for (uint32_t h = 0; h <= F.metric; ++h) {
        const kwk_expo_hist& H = hp->hists[h];
        if (H.dimension > KWK_METRIC_DIM_CONTAINER || H.n_visible > 64 ||
            (uint64_t)H.first_line + H.n_visible + 3 > hp->n_lines)
          return fail(KWK_EINVAL, "histogram exposition program: histogram " + std::to_string(h) + " dimension / lines");
        if (h < F.metric) d.before[H.dimension] += H.n_visible + 3;
      }
      const kwk_expo_hist& H = hp->hists[F.metric];
      for (uint32_t k = 0; k < H.n_visible + 3; ++k) {
        const kwk_expo_hist_line& l = hp->lines[H.first_line + k];
        if ((uint64_t)l.prefix_off + l.prefix_len > prog->n_lit_bytes || (uint64_t)l.tail_off + l.tail_len > prog->n_lit_bytes)
          return fail(KWK_EINVAL, "histogram exposition program: family '" + name + "' line " + std::to_string(k) +
                                  " bytes beyond lits");
      }
      hist.push_back(DevHist{H.n_visible, H.first_line});
      d.hist = (uint32_t)hist.size();
      max_lines = std::max(max_lines, H.n_visible + 3);
      fam.push_back(d);
      continue;
    }
    if (F.group >= prog->n_groups || F.metric >= prog->n_metrics || F.dimension > KWK_METRIC_DIM_CONTAINER ||
        prog->groups[F.group].dimension != F.dimension || prog->metric_dimension[F.metric] != F.dimension)
      return fail(KWK_EINVAL, "exposition program: family " + std::to_string(f) + " group / metric / dimension");
    for (uint32_t m = 0; m < F.metric; ++m) {
      if (prog->metric_dimension[m] > KWK_METRIC_DIM_CONTAINER) return fail(KWK_EINVAL, "exposition program: metric dimension");
      ++d.before[prog->metric_dimension[m]];
    }
    fam.push_back(d);
  }
  void* s = nullptr;
  if (kwk_stream(pods, &s) != KWK_OK) return fail(KWK_EINVAL, std::string("kwk_stream: ") + kwk_last_error(pods));
  auto* ex = new kwk_expo();
  ex->eng = pods;
  ex->stream = static_cast<hipStream_t>(s);
  ex->n_nodes = n_nodes;
  ex->layout_epoch = kwk_layout_epoch(pods);
  ex->fam = std::move(fam);
  ex->hist = std::move(hist);
  ex->max_lines = max_lines;
  ex->groups.resize(prog->n_groups);
  for (uint32_t g = 0; g < prog->n_groups; ++g) {
    ex->groups[g].dim = prog->groups[g].dimension;
    ex->groups[g].n_labels = prog->groups[g].n_labels;
  }
  auto init = [&]() -> kwk_status {
    HIP_TRY(hipStreamGetDevice(ex->stream, &ex->device));
    if (kwk_status st = bind(ex)) return st;
    if (kwk_status st = refresh_layout(ex)) return st;
    if (kwk_status st = upload(ex, ex->d_fam, ex->fam.data(), ex->fam.size())) return st;
    const std::string lits = std::string(prog->lits, prog->n_lit_bytes) + std::string(8, '\0');  // read as 8-byte words
    if (kwk_status st = upload(ex, ex->d_lits, lits.data(), lits.size())) return st;
    if (!ex->hist.empty()) {
      if (kwk_status st = upload(ex, ex->d_hist, ex->hist.data(), ex->hist.size())) return st;
      if (kwk_status st = upload(ex, ex->d_hlines, hp->lines, (size_t)hp->n_lines)) return st;
    }
    HIP_TRY(ex->d_total.alloc(2));
    HIP_TRY(hipMemsetAsync(ex->d_total, 0, 16, ex->stream));
    for (Event& e : ex->ev) HIP_TRY(e.create(hipEventDefault));
    for (Event& e : ex->ev_rows) HIP_TRY(e.create(hipEventDefault));
    HIP_TRY(ex->ev_stage.create(hipEventDisableTiming));
    HIP_TRY(hipStreamCreateWithFlags(&ex->aux, hipStreamNonBlocking));
    HIP_TRY(ex->h_totals.alloc(2));
    return KWK_OK;
  };
  if (kwk_status st = init()) {
    delete ex;
    return st;
  }
  *out = ex;
  return KWK_OK;
}

}  // namespace

extern "C" {

kwk_status kwk_expo_create(kwk_engine* pods, uint32_t n_nodes, const kwk_expo_program* prog, kwk_expo** out) {
  return create(pods, n_nodes, prog, nullptr, out);
}

kwk_status kwk_expo_create_hist(kwk_engine* pods, uint32_t n_nodes, const kwk_expo_program* prog,
                                const kwk_expo_hist_program* hist_prog, kwk_expo** out) {
  if (!hist_prog) {
    ErrScope es_(nullptr);
    return fail(KWK_EINVAL, "null argument");
  }
  return create(pods, n_nodes, prog, hist_prog, out);
}

kwk_status kwk_expo_destroy(kwk_expo* ex) {
  delete ex;
  return KWK_OK;
}

// A writer is for one slot layout: its node count is fixed at kwk_expo_create and its rows, arenas,
// permutations and pod_of are placed by that layout's node_ptr.  After a kwk_relayout (nodes added
// or removed, series moved) every call that places or reads rows refuses: a new writer is created
// for the new layout.  No incremental relayout.
static kwk_status same_layout_epoch(const kwk_expo* ex) {
  if (kwk_layout_epoch(ex->eng) == ex->layout_epoch) return KWK_OK;
  return fail(KWK_ESTATE, "the engine's slot layout changed (kwk_relayout, epoch " + std::to_string(kwk_layout_epoch(ex->eng)) +
                              ", writer created at " + std::to_string(ex->layout_epoch) +
                              "): create a writer for the new layout (kwk_expo_create), set the rows of the new layout and kwk_expo_commit");
}

kwk_status kwk_expo_set_labels(kwk_expo* ex, uint32_t group, uint32_t first, uint32_t n, const uint32_t* block_offsets,
                               const char* blocks, const uint32_t* key_offsets, const char* keys) {
  ErrScope es_(ex ? &ex->err : nullptr);
  if (!ex || (n && (!block_offsets || !key_offsets))) return fail(KWK_EINVAL, "null argument");
  if (group >= ex->groups.size()) return fail(KWK_EINVAL, "label group out of range");
  if (kwk_status st = same_layout_epoch(ex)) return st;
  Group& g = ex->groups[group];
  if ((uint64_t)first + n > g.blocks.size()) return fail(KWK_EINVAL, "rows beyond the group's objects");
  for (uint32_t i = 0; i < n; ++i) {
    if (block_offsets[i + 1] < block_offsets[i] || key_offsets[i + 1] < key_offsets[i])
      return fail(KWK_EINVAL, "offsets must be non-decreasing");
    if ((block_offsets[i + 1] > block_offsets[i] && !blocks) || (key_offsets[i + 1] > key_offsets[i] && !keys))
      return fail(KWK_EINVAL, "null argument");
  }
  for (uint32_t i = 0; i < n; ++i) {
    g.blocks[first + i].assign(blocks + block_offsets[i], blocks + block_offsets[i + 1]);
    g.keys[first + i].assign(keys + key_offsets[i], keys + key_offsets[i + 1]);
    if (!g.is_dirty[first + i]) {
      g.is_dirty[first + i] = 1;
      g.dirty.push_back(first + i);
    }
  }
  ex->committed = false;
  return KWK_OK;
}

kwk_status kwk_expo_commit(kwk_expo* ex) {
  ErrScope es_(ex ? &ex->err : nullptr);
  if (!ex) return fail(KWK_EINVAL, "null writer");
  if (kwk_status st = same_layout_epoch(ex)) return st;
  if (kwk_status st = bind(ex)) return st;
  if (kwk_status st = refresh_layout(ex)) return st;
  HIP_TRY(hipStreamSynchronize(ex->stream));
  ex->full = ex->committed = false;  // until every arena is laid out again
  drain_pending(ex, true);
  // a node's family is walked as rows x lines of a series in 32 bits
  for (uint32_t j = 0; j < ex->n_nodes; ++j)
    if ((uint64_t)(ex->h_cptr[ex->h_node_ptr[j + 1]] - ex->h_cptr[ex->h_node_ptr[j]]) * ex->max_lines > 0xFFFFFFFFull ||
        (uint64_t)(ex->h_node_ptr[j + 1] - ex->h_node_ptr[j]) * ex->max_lines > 0xFFFFFFFFull)
      return fail(KWK_ECAP, "node " + std::to_string(j) + ": more than 2^32 lines in a family");
  std::vector<uint32_t> pod_of(ex->n_cont);
  for (uint32_t p = 0; p < ex->n_pods; ++p)
    for (uint32_t c = ex->h_cptr[p]; c < ex->h_cptr[p + 1]; ++c) pod_of[c] = p;
  if (kwk_status st = upload(ex, ex->d_pod_of, pod_of.data(), pod_of.size())) return st;
  std::vector<DevGroup> dg(ex->groups.size());
  for (size_t gi = 0; gi < ex->groups.size(); ++gi) {
    Group& g = ex->groups[gi];
    const size_t rows = g.blocks.size();
    if (g.n_labels)
      if (kwk_status st = pack_arena(ex, g.blk, g.blocks, "blocks")) return st;
    if (g.dim != KWK_METRIC_DIM_NODE) {
      if (kwk_status st = pack_arena(ex, g.key, g.keys, "sort keys")) return st;
      std::vector<uint32_t> perm(rows);
      std::iota(perm.begin(), perm.end(), 0u);
      const std::vector<uint32_t>& first = ex->h_node_ptr;
      for (uint32_t j = 0; j < ex->n_nodes; ++j) {
        const uint32_t lo = g.dim == KWK_METRIC_DIM_POD ? first[j] : ex->h_cptr[first[j]];
        const uint32_t hi = g.dim == KWK_METRIC_DIM_POD ? first[j + 1] : ex->h_cptr[first[j + 1]];
        std::stable_sort(perm.begin() + lo, perm.begin() + hi,
                         [&](uint32_t x, uint32_t y) { return g.keys[x] < g.keys[y]; });  // std::string: unsigned bytes
      }
      if (kwk_status st = upload(ex, g.d_perm, perm.data(), perm.size())) return st;
    }
    dg[gi] = DevGroup{g.blk.d_ref, g.blk.d, g.d_perm};
    g.is_dirty.assign(rows, 0);
    g.dirty.clear();
  }
  if (kwk_status st = upload(ex, ex->d_grp, dg.data(), dg.size())) return st;
  ex->committed = true;
  ex->full = true;
  return KWK_OK;
}

kwk_status kwk_expo_commit_rows(kwk_expo* ex) {
  ErrScope es_(ex ? &ex->err : nullptr);
  if (!ex) return fail(KWK_EINVAL, "null writer");
  if (!ex->full) return fail(KWK_ESTATE, "kwk_expo_commit must come first: kwk_expo_commit_rows updates a full commit's layout");
  if (kwk_status st = same_layout_epoch(ex)) return st;
  if (kwk_status st = bind(ex)) return st;
  // the engine's layout is the one the arenas and permutations were laid out for: its two totals, read on a
  // stream of this writer's own (the engine's stream is not waited for)
  const uint32_t *np = nullptr, *cp = nullptr, *al = nullptr;
  if (kwk_metrics_series_device(ex->eng, ex->n_nodes, 0, &np, &cp, &al) != KWK_OK)
    return fail(KWK_ESTATE, std::string("the engine's layout changed (kwk_metrics_series_device: ") + kwk_last_error(ex->eng) +
                            "): kwk_expo_commit re-reads it");
  HIP_TRY(hipMemcpyAsync(&ex->h_totals[0], np + ex->n_nodes, 4, hipMemcpyDeviceToHost, ex->aux));
  HIP_TRY(hipStreamSynchronize(ex->aux));
  if (ex->h_totals[0] == ex->n_pods) {
    HIP_TRY(hipMemcpyAsync(&ex->h_totals[1], cp + ex->n_pods, 4, hipMemcpyDeviceToHost, ex->aux));
    HIP_TRY(hipStreamSynchronize(ex->aux));
  }
  if (ex->h_totals[0] != ex->n_pods || ex->h_totals[1] != ex->n_cont)
    return fail(KWK_ESTATE, "the engine's pod or container count (" + std::to_string(ex->h_totals[0]) + " pods) is not the last "
                            "full commit's (" + std::to_string(ex->n_pods) + " pods, " + std::to_string(ex->n_cont) +
                            " containers): kwk_expo_commit re-reads the layout");
  drain_pending(ex, false);

  // the plan: what every arena appends, the (node, group) segments to sort, the staging's size
  const size_t n_groups = ex->groups.size();
  struct Grow { Arena* a; uint64_t size; };
  std::vector<Grow> grow;
  std::vector<SortSeg> segs, big;  // sorted by expo_sort_kernel; beyond kSortMax rows, sorted here
  uint64_t n_rows = 0, n_bytes = 0;
  for (size_t gi = 0; gi < n_groups; ++gi) {
    Group& g = ex->groups[gi];
    if (g.dirty.empty()) continue;
    std::sort(g.dirty.begin(), g.dirty.end());
    const bool sorted = g.dim != KWK_METRIC_DIM_NODE;
    uint64_t need_blk = 0, need_key = 0;
    uint32_t node = 0;
    bool have_node = false;
    auto first_row = [&](uint32_t j) { return g.dim == KWK_METRIC_DIM_POD ? ex->h_node_ptr[j] : ex->h_cptr[ex->h_node_ptr[j]]; };
    for (uint32_t r : g.dirty) {
      if (g.n_labels) {
        const uint64_t n = g.blocks[r].size();
        if (n > g.blk.cap[r]) need_blk += up8(n);
        n_bytes += up8(n);
        ++n_rows;
      }
      if (!sorted) continue;
      const uint64_t n = g.keys[r].size();
      if (n > g.key.cap[r]) need_key += up8(n);
      n_bytes += up8(n);
      ++n_rows;
      uint32_t j = have_node ? node : 0;
      while (first_row(j + 1) <= r) ++j;  // the rows ascend, so do their nodes
      if (!have_node || j != node) {
        const SortSeg s{first_row(j), first_row(j + 1), (uint32_t)gi, 0u};
        if (s.hi - s.lo > kSortMax) {
          big.push_back(s);
          n_bytes += up8(4ull * (s.hi - s.lo));
          ++n_rows;
        } else if (s.hi - s.lo > 1) {  // (a segment of one row is its own order)
          segs.push_back(s);
        }
        node = j;
        have_node = true;
      }
    }
    const uint64_t need[2] = {need_blk, need_key};
    Arena* arena[2] = {&g.blk, &g.key};
    for (int k = 0; k < 2; ++k) {
      Arena& a = *arena[k];
      if (!need[k] || a.tail + need[k] + 8 <= a.size) continue;
      if (a.tail + need[k] + 8 > kArenaMax)
        return fail(KWK_ECAP, "group " + std::to_string(gi) + ": its label " + (k ? "sort keys" : "blocks") +
                              " would pass 4 GiB (32-bit offsets): kwk_expo_commit compacts the storage");
      uint64_t size = a.size;
      while (size < a.tail + need[k] + 8) size = std::min<uint64_t>(kArenaMax, 2 * size);
      grow.push_back(Grow{&a, size});
    }
  }
  if (!n_rows) {  // (rows of a node group without labels have nothing on the device)
    for (Group& g : ex->groups) {
      for (uint32_t r : g.dirty) g.is_dirty[r] = 0;
      g.dirty.clear();
    }
    ex->committed = true;
    return KWK_OK;
  }
  if (n_rows > 0xFFFFFFFFull || segs.size() > 0x7FFFFFFFull)
    return fail(KWK_ECAP, "more than 2^32 rows in one incremental commit: kwk_expo_commit");
  const uint64_t tab_at = 0, grp_at = up8(tab_at + sizeof(ArenaDev) * kArenas * n_groups);
  const uint64_t rows_at = up8(grp_at + sizeof(DevGroup) * n_groups), segs_at = rows_at + sizeof(ScatterRow) * n_rows;
  const uint64_t bytes_at = up8(segs_at + sizeof(SortSeg) * segs.size()), stage_bytes = bytes_at + n_bytes;

  Pending pend;  // (a failed call frees it on return, after the stream has been synchronised)
  auto run = [&]() -> kwk_status {
    // the staging buffer is this call's once the last copy out of it is done
    if (ex->stage_busy) HIP_TRY(hipEventSynchronize(ex->ev_stage));
    ex->stage_busy = false;
    if (stage_bytes > ex->h_stage.size()) HIP_TRY(ex->h_stage.alloc((size_t)(stage_bytes + stage_bytes / 2)));
    if (stage_bytes > ex->d_stage.size()) {
      if (ex->d_stage) pend.bufs.push_back(std::move(ex->d_stage));
      HIP_TRY(ex->d_stage.alloc((size_t)(stage_bytes + stage_bytes / 2)));
    }
    // an arena whose tail is full doubles: its rows keep their offsets
    for (const Grow& gr : grow) {
      DevBuf<char> d;
      HIP_TRY(d.alloc((size_t)gr.size));
      HIP_TRY(hipMemcpyAsync(d, gr.a->d, (size_t)gr.a->tail + 8, hipMemcpyDeviceToDevice, ex->stream));
      pend.bufs.push_back(std::move(gr.a->d));
      gr.a->d = std::move(d);
      gr.a->size = gr.size;
    }
    char* h = ex->h_stage;
    ArenaDev* tab = reinterpret_cast<ArenaDev*>(h + tab_at);
    DevGroup* dgrp = reinterpret_cast<DevGroup*>(h + grp_at);
    ScatterRow* rows = reinterpret_cast<ScatterRow*>(h + rows_at);
    uint64_t at = bytes_at, nr = 0;
    for (size_t gi = 0; gi < n_groups; ++gi) {
      Group& g = ex->groups[gi];
      tab[kArenas * gi + 0] = ArenaDev{g.blk.d, g.blk.d_ref};
      tab[kArenas * gi + 1] = ArenaDev{g.key.d, g.key.d_ref};
      tab[kArenas * gi + 2] = ArenaDev{reinterpret_cast<char*>(g.d_perm.get()), nullptr};
      dgrp[gi] = DevGroup{g.blk.d_ref, g.blk.d, g.d_perm};
      for (uint32_t r : g.dirty) {
        for (uint32_t k = 0; k < 2; ++k) {
          if (k == 0 ? g.n_labels == 0 : g.dim == KWK_METRIC_DIM_NODE) continue;
          Arena& a = k ? g.key : g.blk;
          const std::string& s = k ? g.keys[r] : g.blocks[r];
          const uint32_t n = (uint32_t)s.size();
          if (n > a.cap[r]) {  // the slot is too small: a new one at the tail
            a.off[r] = (uint32_t)a.tail;
            a.cap[r] = (uint32_t)up8(n);
            a.tail += up8(n);
          }
          memcpy(h + at, s.data(), n);
          rows[nr++] = ScatterRow{a.off[r], at, n, r, (uint32_t)(kArenas * gi + k), 0u};
          at += up8(n);
        }
        g.is_dirty[r] = 0;
      }
      g.dirty.clear();
    }
    for (const SortSeg& s : big) {
      const Group& g = ex->groups[s.group];
      uint32_t* p = reinterpret_cast<uint32_t*>(h + at);
      std::iota(p, p + (s.hi - s.lo), s.lo);
      std::stable_sort(p, p + (s.hi - s.lo), [&](uint32_t x, uint32_t y) { return g.keys[x] < g.keys[y]; });
      rows[nr++] = ScatterRow{4ull * s.lo, at, 4u * (s.hi - s.lo), 0u, kArenas * s.group + 2, 0u};
      at += up8(4ull * (s.hi - s.lo));
    }
    if (!segs.empty()) memcpy(h + segs_at, segs.data(), sizeof(SortSeg) * segs.size());
    HIP_TRY(hipMemcpyAsync(ex->d_stage, h, (size_t)stage_bytes, hipMemcpyHostToDevice, ex->stream));
    HIP_TRY(hipEventRecord(ex->ev_stage, ex->stream));
    ex->stage_busy = true;
    if (!grow.empty())
      HIP_TRY(hipMemcpyAsync(ex->d_grp, ex->d_stage + grp_at, sizeof(DevGroup) * n_groups, hipMemcpyDeviceToDevice, ex->stream));
    const ArenaDev* d_tab = reinterpret_cast<const ArenaDev*>(ex->d_stage + tab_at);
    HIP_TRY(hipEventRecord(ex->ev_rows[0], ex->stream));
    hipLaunchKernelGGL(expo_scatter_kernel, dim3((uint32_t)((nr + kScatterBlock / 64 - 1) / (kScatterBlock / 64))),
                       dim3(kScatterBlock), 0, ex->stream, d_tab, reinterpret_cast<const ScatterRow*>(ex->d_stage + rows_at),
                       (uint32_t)nr, ex->d_stage);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ex->ev_rows[1], ex->stream));
    if (!segs.empty()) {
      hipLaunchKernelGGL(expo_sort_kernel, dim3((uint32_t)segs.size()), dim3(kSortBlock), 0, ex->stream, d_tab,
                         reinterpret_cast<const SortSeg*>(ex->d_stage + segs_at));
      HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(ex->ev_rows[2], ex->stream));
    ex->rows_timed = true;
    if (!pend.bufs.empty()) {
      HIP_TRY(pend.ev.create(hipEventDisableTiming));
      HIP_TRY(hipEventRecord(pend.ev, ex->stream));
      ex->pending.push_back(std::move(pend));
    }
    return KWK_OK;
  };
  const kwk_status st = run();
  if (st != KWK_OK) {  // the arenas may be half written: only a full commit makes them whole
    ex->full = ex->committed = false;
    hipStreamSynchronize(ex->stream);
    return st;
  }
  ex->committed = true;
  return KWK_OK;
}

kwk_status kwk_expo_commit_rows_elapsed(kwk_expo* ex, float ms[2]) {
  ErrScope es_(ex ? &ex->err : nullptr);
  if (!ex || !ms) return fail(KWK_EINVAL, "null argument");
  if (!ex->rows_timed) return fail(KWK_ESTATE, "a kwk_expo_commit_rows that enqueued work must come first");
  if (kwk_status st = bind(ex)) return st;
  HIP_TRY(hipEventSynchronize(ex->ev_rows[2]));
  for (int i = 0; i < 2; ++i) HIP_TRY(hipEventElapsedTime(&ms[i], ex->ev_rows[i], ex->ev_rows[i + 1]));
  return KWK_OK;
}

kwk_status kwk_expo_read_perm(kwk_expo* ex, uint32_t group, uint32_t* out) {
  ErrScope es_(ex ? &ex->err : nullptr);
  if (!ex) return fail(KWK_EINVAL, "null writer");
  if (group >= ex->groups.size()) return fail(KWK_EINVAL, "label group out of range");
  const Group& g = ex->groups[group];
  if (g.dim == KWK_METRIC_DIM_NODE) return fail(KWK_EINVAL, "a node-dimension group has no permutation");
  if (!ex->full) return fail(KWK_ESTATE, "kwk_expo_commit must come first");
  if (g.blocks.size() && !out) return fail(KWK_EINVAL, "null argument");
  if (kwk_status st = bind(ex)) return st;
  return copy_out(ex, out, g.d_perm, 4 * g.blocks.size());
}

int kwk_expo_key_compare(const char* a, uint32_t na, const char* b, uint32_t nb) { return kwkkey::compare(a, na, b, nb); }

kwk_status kwk_expo_reserve(kwk_expo* ex, uint64_t max_bytes) {
  ErrScope es_(ex ? &ex->err : nullptr);
  if (!ex) return fail(KWK_EINVAL, "null writer");
  if (kwk_status st = bind(ex)) return st;
  HIP_TRY(hipStreamSynchronize(ex->stream));
  ex->cap_bytes = 0;
  HIP_TRY(ex->d_out.alloc(std::max<size_t>(8, (size_t)max_bytes)));
  ex->cap_bytes = max_bytes;
  return KWK_OK;
}

kwk_status kwk_expo_set_width(kwk_expo* ex, uint32_t width) {
  ErrScope es_(ex ? &ex->err : nullptr);
  if (!ex) return fail(KWK_EINVAL, "null writer");
  if (width != 0 && width != 64 && width != 256) return fail(KWK_EINVAL, "width must be 0, 64 or 256");
  ex->width = width;
  return KWK_OK;
}

kwk_status kwk_expo_scrape(kwk_expo* ex, int64_t now_ns, uint32_t node_first, uint32_t n_nodes) {
  ErrScope es_(ex ? &ex->err : nullptr);
  if (!ex) return fail(KWK_EINVAL, "null writer");
  if (!ex->committed) return fail(KWK_ESTATE, "kwk_expo_commit must come first");
  if (kwk_status st = same_layout_epoch(ex)) return st;
  if ((uint64_t)node_first + n_nodes > ex->n_nodes) return fail(KWK_EINVAL, "nodes beyond the writer's");
  if (kwk_status st = bind(ex)) return st;
  if (!ex->d_out)
    if (kwk_status st = kwk_expo_reserve(ex, 0)) return st;
  if ((size_t)n_nodes + 1 > ex->d_offsets.size()) {  // (allocated last of the two)
    HIP_TRY(hipStreamSynchronize(ex->stream));
    HIP_TRY(ex->d_node_bytes.alloc((size_t)n_nodes + 1));
    HIP_TRY(ex->d_offsets.alloc((size_t)n_nodes + 1));
  }
  HIP_TRY(hipEventRecord(ex->ev[0], ex->stream));
  ExpoArgs a{};
  uint64_t n_vals = 0;
  if (kwk_metrics_eval_device(ex->eng, now_ns, node_first, n_nodes, &a.vals, &n_vals) != KWK_OK)
    return fail(KWK_ESTATE, std::string("kwk_metrics_eval_device: ") + kwk_last_error(ex->eng));
  if (kwk_metrics_series_device(ex->eng, node_first, n_nodes, &a.node_ptr, &a.cptr, &a.alive) != KWK_OK)
    return fail(KWK_ESTATE, std::string("kwk_metrics_series_device: ") + kwk_last_error(ex->eng));
  a.fam = ex->d_fam;
  a.grp = ex->d_grp;
  a.lits = ex->d_lits;
  a.pod_of = ex->d_pod_of;
  a.n_fam = (uint32_t)ex->fam.size();
  a.n0 = node_first;
  a.n_nodes = n_nodes;
  a.p0 = ex->h_node_ptr[node_first];
  a.p1 = ex->h_node_ptr[node_first + n_nodes];
  a.c0 = ex->h_cptr[a.p0];
  a.c1 = ex->h_cptr[a.p1];
  a.node_bytes = ex->d_node_bytes;
  a.offsets = ex->d_offsets;
  a.total = ex->d_total;
  a.out = ex->d_out;
  a.cap = ex->cap_bytes;
  // the values this walk reads are the values the engine wrote: the same series count
  const bool has_hist = !ex->hist.empty();
  uint64_t want = 0, want_words = 0, n_words = 0;
  for (const DevFamily& F : ex->fam) {
    const uint64_t series = F.dim == KWK_METRIC_DIM_NODE ? n_nodes : F.dim == KWK_METRIC_DIM_POD ? a.p1 - a.p0 : a.c1 - a.c0;
    if (F.hist) want_words += series * (ex->hist[F.hist - 1].nvis + 3);
    else want += series;
  }
  if (has_hist) {
    const uint64_t* hv = nullptr;
    if (kwk_histograms_eval_device(ex->eng, now_ns, node_first, n_nodes, &hv, &n_words) != KWK_OK)
      return fail(KWK_ESTATE, std::string("kwk_histograms_eval_device: ") + kwk_last_error(ex->eng));
    if (want_words != n_words)
      return fail(KWK_ESTATE, "the engine's loaded histograms (" + std::to_string(n_words) + " record words) are not the "
                              "exposition program's (" + std::to_string(want_words) + "): kwk_histograms_load the same "
                              "Metric CR; commit after kwk_usage_config");
    a.hvals = reinterpret_cast<const unsigned long long*>(hv);
    a.hist = ex->d_hist;
    a.hlines = ex->d_hlines;
    a.n_vals = n_vals;
  }
  if (want != n_vals)
    return fail(KWK_ESTATE, "the engine's loaded metrics (" + std::to_string(n_vals) + " series) are not the exposition "
                            "program's (" + std::to_string(want) + "): kwk_metrics_load the same Metric CR; commit after "
                            "kwk_usage_config");
  const uint32_t width = ex->width ? ex->width : (n_nodes && (a.p1 - a.p0) / n_nodes > kWidePods) ? 256u : 64u;
  const uint64_t n_slots = n_vals + n_words;  // the histogram words' slots after the scalars'
  if (n_slots > ex->d_stash.size() / 2) {  // a slot is two uint4
    HIP_TRY(hipStreamSynchronize(ex->stream));
    HIP_TRY(ex->d_stash.alloc(2 * (size_t)n_slots));
  }
  a.stash = ex->d_stash;
#define KWK_EXPO_LAUNCH_H(WR, H)                                                                                    \
  do {                                                                                                             \
    if (width == 64) hipLaunchKernelGGL((expo_node_kernel<64, WR, H>), dim3(n_nodes), dim3(64), 0, ex->stream, a); \
    else hipLaunchKernelGGL((expo_node_kernel<256, WR, H>), dim3(n_nodes), dim3(256), 0, ex->stream, a);           \
  } while (0)
#define KWK_EXPO_LAUNCH(WR)                 \
  do {                                      \
    if (has_hist) KWK_EXPO_LAUNCH_H(WR, true); \
    else KWK_EXPO_LAUNCH_H(WR, false);      \
  } while (0)
  HIP_TRY(hipMemsetAsync(ex->d_total + 1, 0, 8, ex->stream));
  HIP_TRY(hipEventRecord(ex->ev[1], ex->stream));
  if (n_nodes) {
    KWK_EXPO_LAUNCH(false);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(ex->ev[2], ex->stream));
  hipLaunchKernelGGL(expo_scan_kernel, dim3(1), dim3(kScanBlock), 0, ex->stream, ex->d_node_bytes, n_nodes, ex->d_offsets,
                     ex->d_total);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(ex->ev[3], ex->stream));
  if (n_nodes) {
    KWK_EXPO_LAUNCH(true);
    HIP_TRY(hipGetLastError());
  }
#undef KWK_EXPO_LAUNCH
#undef KWK_EXPO_LAUNCH_H
  HIP_TRY(hipEventRecord(ex->ev[4], ex->stream));
  ex->scraped = true;
  ex->last_nodes = n_nodes;
  return KWK_OK;
}

kwk_status kwk_expo_result(kwk_expo* ex, uint64_t* n_bytes) {
  ErrScope es_(ex ? &ex->err : nullptr);
  if (!ex || !n_bytes) return fail(KWK_EINVAL, "null argument");
  if (!ex->scraped) return fail(KWK_ESTATE, "kwk_expo_scrape must come first");
  if (kwk_status st = bind(ex)) return st;
  unsigned long long t[2] = {0, 0};
  if (kwk_status st = copy_out(ex, t, ex->d_total, sizeof t)) return st;
  *n_bytes = t[0];
  if (t[1])
    return fail(KWK_ESTATE, std::to_string(t[1]) + " live series of a labelled group have no label row: nothing was written; "
                            "kwk_expo_set_labels their rows and kwk_expo_commit");
  if (t[0] > ex->cap_bytes)
    return fail(KWK_ECAP, "the text exceeds the reservation: kwk_expo_reserve(" + std::to_string(t[0]) + ") and scrape again");
  return KWK_OK;
}

kwk_status kwk_expo_device(kwk_expo* ex, const uint64_t** offsets, const char** bytes) {
  ErrScope es_(ex ? &ex->err : nullptr);
  if (!ex) return fail(KWK_EINVAL, "null writer");
  if (offsets) *offsets = reinterpret_cast<const uint64_t*>(ex->d_offsets.get());
  if (bytes) *bytes = ex->d_out;
  return KWK_OK;
}

kwk_status kwk_expo_copy(kwk_expo* ex, uint64_t* offsets, char* bytes) {
  ErrScope es_(ex ? &ex->err : nullptr);
  uint64_t nb = 0;
  if (kwk_status st = kwk_expo_result(ex, &nb)) return st;
  if (!offsets || (nb && !bytes)) return fail(KWK_EINVAL, "null argument");
  if (kwk_status st = copy_out(ex, offsets, ex->d_offsets, 8 * ((size_t)ex->last_nodes + 1))) return st;
  return copy_out(ex, bytes, ex->d_out, (size_t)nb);
}

kwk_status kwk_expo_elapsed(kwk_expo* ex, float ms[4]) {
  ErrScope es_(ex ? &ex->err : nullptr);
  if (!ex || !ms) return fail(KWK_EINVAL, "null argument");
  if (!ex->scraped) return fail(KWK_ESTATE, "kwk_expo_scrape must come first");
  if (kwk_status st = bind(ex)) return st;
  HIP_TRY(hipEventSynchronize(ex->ev[4]));
  HIP_TRY(hipEventElapsedTime(&ms[0], ex->ev[0], ex->ev[4]));
  for (int i = 1; i < 4; ++i) HIP_TRY(hipEventElapsedTime(&ms[i], ex->ev[i], ex->ev[i + 1]));
  return KWK_OK;
}

kwk_status kwk_expo_format_values(kwk_expo* ex, const double* host_values, uint32_t n, char* out, uint8_t* lens) {
  ErrScope es_(ex ? &ex->err : nullptr);
  if (!ex || (n && (!host_values || !out || !lens))) return fail(KWK_EINVAL, "null argument");
  if (!n) return KWK_OK;
  if (kwk_status st = bind(ex)) return st;
  DevBuf<double> d_v;
  DevBuf<char> d_o;
  DevBuf<uint8_t> d_l;
  auto run = [&]() -> kwk_status {
    HIP_TRY(d_v.alloc(n));
    HIP_TRY(d_o.alloc((size_t)kwkf64::kMaxBytes * n));
    HIP_TRY(d_l.alloc(n));
    if (kwk_status st = copy_in(ex, d_v, host_values, 8 * (size_t)n)) return st;
    HIP_TRY(hipMemsetAsync(d_o, 0, (size_t)kwkf64::kMaxBytes * n, ex->stream));
    hipLaunchKernelGGL(expo_format_kernel, dim3((n + kFmtBlock - 1) / kFmtBlock), dim3(kFmtBlock), 0, ex->stream, d_v, n, d_o,
                       d_l);
    HIP_TRY(hipGetLastError());
    if (kwk_status st = copy_out(ex, out, d_o, (size_t)kwkf64::kMaxBytes * n)) return st;
    return copy_out(ex, lens, d_l, n);
  };
  const kwk_status st = run();
  hipStreamSynchronize(ex->stream);  // before the three buffers go
  return st;
}

}  // extern "C"
