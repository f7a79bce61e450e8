// Stand-alone check of kwk_patch_event (include/kwok_patch.h) for a sanitizer build of the host code:
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I include
//       tools/event_check.cpp kwok_amd/csrc/patch.cpp -pthread -o event_check
//   ./event_check cases.txt
//
// cases.txt (written by tests/test_events.py): blocks of
//   spec <event program JSON on one line>
//   case <stage> <namespace hex|-> <name hex|-> <uid hex|-> <apiVersion hex|-> <now_ns> <expected bytes in hex|->
// The event program is wrapped into a patch spec with no templates.  Every output buffer is a heap
// block of exactly the size asked for, so a byte written past it is caught; a too-small buffer must
// give KWK_ECAP and the size, and the call after it must succeed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

#include "kwok_patch.h"

static std::string unhex(const std::string& h) {
  std::string o;
  if (h == "-") return o;
  for (size_t i = 0; i + 1 < h.size(); i += 2) o.push_back((char)strtol(h.substr(i, 2).c_str(), nullptr, 16));
  return o;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s cases.txt\n", argv[0]);
    return 2;
  }
  std::ifstream in(argv[1]);
  if (!in) {
    fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  kwk_patcher* p = nullptr;
  std::string line;
  size_t n_cases = 0, bad = 0;
  while (std::getline(in, line)) {
    if (line.rfind("spec ", 0) == 0) {
      if (p) kwk_patcher_destroy(p);
      p = nullptr;
      const std::string spec = "{\"templates\": [], \"funcs\": [], \"consts\": [], \"events\": " + line.substr(5) + "}";
      if (kwk_patcher_create(spec.c_str(), &p) != KWK_OK) {
        fprintf(stderr, "kwk_patcher_create: %s\n", kwk_patch_last_error(nullptr));
        return 1;
      }
      continue;
    }
    if (line.rfind("case ", 0) != 0 || !p) continue;
    std::istringstream ss(line.substr(5));
    uint32_t stage = 0;
    long long now = 0;
    std::string ns, name, uid, av, hex;
    ss >> stage >> ns >> name >> uid >> av >> now >> hex;
    ns = unhex(ns), name = unhex(name), uid = unhex(uid), av = unhex(av);
    const std::string want = unhex(hex);
    ++n_cases;
    // the size first (no buffer), then a buffer one byte short, then the exact size
    uint64_t len = ~0ull;
    kwk_status st = kwk_patch_event(p, stage, ns.c_str(), name.c_str(), uid.c_str(), av.c_str(), now, nullptr, 0, &len);
    if (len != want.size() || st != (want.empty() ? KWK_OK : KWK_ECAP)) {
      fprintf(stderr, "case %zu: size %llu (status %d), expected %zu\n", n_cases, (unsigned long long)len, st, want.size());
      ++bad;
      continue;
    }
    if (want.empty()) continue;
    char* small = static_cast<char*>(malloc(want.size() - 1));
    len = 0;
    if (kwk_patch_event(p, stage, ns.c_str(), name.c_str(), uid.c_str(), av.c_str(), now, small, want.size() - 1, &len) != KWK_ECAP ||
        len != want.size())
      ++bad;
    free(small);
    char* out = static_cast<char*>(malloc(want.size()));
    st = kwk_patch_event(p, stage, ns.c_str(), name.c_str(), uid.c_str(), av.c_str(), now, out, want.size(), &len);
    if (st != KWK_OK || len != want.size() || memcmp(out, want.data(), want.size()) != 0) {
      fprintf(stderr, "case %zu: bytes differ\n", n_cases);
      ++bad;
    }
    free(out);
  }
  if (p) kwk_patcher_destroy(p);
  printf("%zu cases, %zu bad\n", n_cases, bad);
  return bad || !n_cases ? 1 : 0;
}
