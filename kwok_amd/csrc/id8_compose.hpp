// The 1-byte sweep's id layout and the composite id table of its fused launches (host and device;
// no HIP: tools/id8_compose_check.cpp builds this header alone with g++).
#pragma once
#include <cstdint>

// id: [7] the word needs work whatever its due time, [6] a stage is queued on a managed object,
// [5] alive, [4:0] index within that class
constexpr uint32_t kIdNeed = 0x80u, kIdPend = 0x40u, kIdAlive = 0x20u, kIdIndex = 0x1Fu;
constexpr uint32_t kIdInvalid = 0xFFu;  // not in the dictionary (never stored: the host closes it)
// id transition entry (dict_upload): [7:0] new id, [15:11] the 2-byte fired record's high bits
// (stage 11-12 when the program has <= 4 stages, flags 13-15), [20:16] fired stage, [23:21]
// fired flags, [28:24] algorithmic bytes of the item beyond its 1-byte read, [29] writes due =
// now + fsm_due[entry], [30] matched, [31] fired.  Lookups the sweep never makes (and unused ids,
// kIdInvalid among them) hold the id itself: no change, nothing fires.
constexpr uint32_t kId8Rec16 = 0xF800u, kId8Due = 1u << 29, kId8Match = 1u << 30, kId8Fire = 1u << 31;

// Composite row of an id (16 bytes, one LDS read): what an item that enters a fused launch of k
// steps with this id, on a tile without a queued stage, does over the whole launch.  Such an item
// is looked up at step 0 and then at every step while its new id keeps kIdNeed (an id off the list
// never joins it again: kIdNeed is a function of the id), so its trajectory is a function of the
// first id alone:  e_s = t8[key_s],  key_{s+1} = (e_s & kIdNeed) ? e_s & 0xFF : kIdInvalid.
//   w[s], s < k   [31] fired at step s, [15:11] that record's high bits (0 unless fired)
//   w[0] [7:0]    the id the item ends with
//   w[1] [2:0]    entries with kId8Match, [22:16] their algorithmic bytes summed
//   w[2] [1:0]    steps >= 1 at which the item was still on the list
//   w[3] [2:0], [10:8], [18:16], [26:24]   records fired per stage code (bits 12:11 of the record)
// The statistics fields leave room above them: a lane adds the masked words of up to 16 items.
constexpr uint32_t kId8cFin = 0xFFu;
constexpr uint32_t kId8cMatched = 0x7u, kId8cBytesShift = 16, kId8cBytes = 0x7Fu << kId8cBytesShift;
constexpr uint32_t kId8cStat = kId8cMatched | kId8cBytes;
constexpr uint32_t kId8cLive = 0x3u;
constexpr uint32_t kId8cStages = 0x07070707u;
constexpr uint32_t kId8cRowWords = 4;
constexpr int kId8cMaxSteps = 4;

// out[256 * 4] from the id table t8[512] (the sweep's carried path never takes a ready lookup:
// rows 256-511 are not read) for a launch of k steps, 2 <= k <= 4
inline void id8_compose(const uint32_t* t8, const int k, uint32_t* out) {
  for (uint32_t id = 0; id < 256; ++id) {
    uint32_t w[kId8cRowWords] = {0u, 0u, 0u, 0u};
    uint32_t key = id, fin = kIdInvalid, matched = 0, bytes = 0, live = 0, stages = 0;
    for (int s = 0; s < k && s < kId8cMaxSteps; ++s) {
      if (s > 0 && key != kIdInvalid) ++live;
      const uint32_t e = t8[key];
      bytes += (e >> 24) & 31u;
      matched += (e >> 30) & 1u;
      if (e & kId8Fire) {
        w[s] |= kId8Fire | (e & kId8Rec16);
        stages += 1u << ((e >> 8) & 0x18u);
      }
      const uint32_t nid = e & 0xFFu;
      if (s + 1 < k) {  // (an item that left before: nid = kIdInvalid, which has kIdNeed; fin stays)
        const bool on = (nid & kIdNeed) != 0;
        key = on ? nid : kIdInvalid;
        fin = on ? fin : nid;
      } else {
        fin &= nid;  // still on the list: fin = 0xFF; left before: nid = 0xFF
      }
    }
    w[0] |= fin;
    w[1] |= matched | bytes << kId8cBytesShift;
    w[2] |= live;
    w[3] |= stages;
    for (uint32_t i = 0; i < kId8cRowWords; ++i) out[id * kId8cRowWords + i] = w[i];
  }
}
