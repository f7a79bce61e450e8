// Stand-alone check of kwk_patch_finalizers / kwk_patch_finalizer_word / _list (include/kwok_patch.h)
// for a sanitizer build of the host code:
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I include
//       tools/fin_patch_check.cpp kwok_amd/csrc/patch.cpp -pthread -o fin_patch_check
//   ./fin_patch_check cases.txt
//
// cases.txt (written by tests/test_patch_finalizers.py): blocks of
//   spec <patch spec JSON on one line>
//   case <stage> <n> <value,value,...|-> <expected bytes in hex|->
// Every output buffer is a heap block of exactly the size asked for, so a byte written past it is
// caught; a too-small buffer must give KWK_ECAP and the size.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

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
      if (kwk_patcher_create(line.c_str() + 5, &p) != KWK_OK) {
        fprintf(stderr, "kwk_patcher_create: %s\n", kwk_patch_last_error(nullptr));
        return 1;
      }
      continue;
    }
    if (line.rfind("case ", 0) != 0 || !p) continue;
    std::istringstream ss(line.substr(5));
    uint32_t stage = 0, n = 0;
    std::string vals, hex;
    ss >> stage >> n >> vals >> hex;
    std::string fins;  // NUL-separated
    if (vals != "-") {
      fins = vals;
      for (char& c : fins)
        if (c == ',') c = '\0';
    }
    const std::string want = unhex(hex);
    ++n_cases;
    // the size first (no buffer), then a buffer one byte short, then the exact size
    uint64_t len = ~0ull;
    kwk_status st = kwk_patch_finalizers(p, stage, n, fins.data(), fins.size(), nullptr, 0, &len);
    if (len != want.size() || st != (want.empty() ? KWK_OK : KWK_ECAP)) {
      fprintf(stderr, "case %zu: size %llu (status %d), expected %zu\n", n_cases, (unsigned long long)len, st, want.size());
      ++bad;
      continue;
    }
    if (!want.empty()) {
      char* small = static_cast<char*>(malloc(want.size() - 1 ? want.size() - 1 : 1));
      if (kwk_patch_finalizers(p, stage, n, fins.data(), fins.size(), small, want.size() - 1, &len) != KWK_ECAP) ++bad;
      free(small);
      char* out = static_cast<char*>(malloc(want.size()));
      st = kwk_patch_finalizers(p, stage, n, fins.data(), fins.size(), out, want.size(), &len);
      if (st != KWK_OK || len != want.size() || memcmp(out, want.data(), want.size()) != 0) {
        fprintf(stderr, "case %zu: bytes differ\n", n_cases);
        ++bad;
      }
      free(out);
    }
    // the order word, and back for lists of known values
    uint32_t word = 0;
    if (kwk_patch_finalizer_word(p, n, fins.data(), fins.size(), &word) != KWK_OK) {
      ++bad;
      continue;
    }
    if ((n > 7) != (word == KWK_FIN_WORD_HOST)) ++bad;
    if (n <= 7) {
      bool known = true;
      for (uint32_t k = 0; k < n; ++k) known = known && ((word >> (4u * k)) & 15u) != KWK_FIN_OTHER;
      uint32_t cnt = 0;
      uint64_t ll = 0;
      char* back = static_cast<char*>(malloc(fins.size() + 1));
      st = kwk_patch_finalizer_list(p, word, &cnt, back, fins.size() + 1, &ll);
      if (known) {
        const std::string full = n ? fins + std::string(1, '\0') : std::string();
        if (st != KWK_OK || cnt != n || ll != full.size() || memcmp(back, full.data(), full.size()) != 0) ++bad;
      } else if (st != KWK_EINVAL) {
        ++bad;
      }
      free(back);
    }
  }
  if (p) kwk_patcher_destroy(p);
  printf("%zu cases, %zu bad\n", n_cases, bad);
  return bad || !n_cases ? 1 : 0;
}
