// The order of the device exposition's series within a node (kwk_expo_commit / kwk_expo_commit_rows),
// host and device: std::string's operator< over the sort keys kwk_metric_labels_render gives —
// unsigned bytes, a proper prefix first — which is the order of promhttp's sorted label values
// (pkg/kwok/metrics/metrics.go:525-573 gathers, expfmt encodes in that order).
//
// Eight bytes at a time: word k of a key is its bytes [8k, 8k + 8) with zeros past the key's end,
// byte-swapped so that an integer compare is a bytewise one.  Over the words of the shorter key a
// difference decides; equal words leave the lengths to decide (zero padding makes "a" and "a\0"
// equal as words: the shorter is the prefix and sorts first).  Equal keys compare 0: the callers
// break that tie by row index, which is std::stable_sort over ascending rows.
//
// The device build reads a word as the one or two aligned 8-byte words that hold its bytes and
// nothing beyond them, so a key needs no padding of its own, only storage whose size is a multiple
// of 8 (the arenas of expo.hip); the host build copies the bytes.  Everything after the load is the
// same code: kwk_expo_key_compare is the host build (tests/test_expo_key_compare.py).
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KWK_KEY_HD __host__ __device__ __forceinline__
#else
#define KWK_KEY_HD inline
#endif

namespace kwkkey {

// word k of key p[0 .. n) (8 * k < n), big-endian
KWK_KEY_HD uint64_t word(const char* p, uint32_t n, uint32_t k) {
  const uint32_t at = 8u * k;
  const uint32_t have = n - at < 8u ? n - at : 8u;
  uint64_t x = 0;
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t sa = (uint32_t)((size_t)(p + at) & 7u);
  const uint64_t* w = reinterpret_cast<const uint64_t*>(p + at - sa);
  x = w[0] >> (8u * sa);
  if (sa && have > 8u - sa) x |= w[1] << (8u * (8u - sa));
#else
  memcpy(&x, p + at, have);
#endif
  if (have < 8u) x &= (1ull << (8u * have)) - 1ull;
  return __builtin_bswap64(x);
}

// < 0, 0, > 0 as std::string(a, na).compare(std::string(b, nb))
KWK_KEY_HD int compare(const char* a, uint32_t na, const char* b, uint32_t nb) {
  const uint32_t m = na < nb ? na : nb;
  for (uint32_t k = 0; 8u * k < m; ++k) {
    const uint64_t wa = word(a, na, k), wb = word(b, nb, k);
    if (wa != wb) return wa < wb ? -1 : 1;
  }
  return na < nb ? -1 : na > nb ? 1 : 0;
}

}  // namespace kwkkey
