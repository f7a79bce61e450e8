// Stand-alone walk of the Metric compiler's exposition builder (host only, no GPU), meant for a
// sanitizer build:
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include \
//       tools/expo_program_walk.cpp kwok_amd/csrc/metrics_compiler.cpp -o /tmp/expo_program_walk
//   /tmp/expo_program_walk
//
// Compiles a CR of two scalars and two histograms (a labelled pod histogram with a hidden bucket,
// bounds out of order and a duplicate visible le; a node histogram without labels) with
// KWK_METRICS_EXPO_HISTOGRAMS, reads every byte range of both programs, renders one label row per
// group, and checks the refusals (no flag; a host-evaluated bucket value).  Prints the families and
// exits 0, or says what is wrong and exits 1.
#include <cstdio>
#include <cstring>
#include <string>

#include "kwok_metrics.h"

static const char* kCR = R"JSON({"kind": "Metric", "spec": {"path": "/metrics/nodes/{nodeName}/metrics/hist", "metrics": [
 {"name": "z_counter", "kind": "counter", "dimension": "node", "help": "z", "value": "2.0"},
 {"name": "m_hist", "kind": "histogram", "dimension": "pod", "help": "pod\nhistogram",
  "labels": [{"name": "namespace", "value": "pod.metadata.namespace"}, {"name": "pod", "value": "pod.metadata.name"}],
  "buckets": [{"le": 5, "value": "1.0"}, {"le": 0.5, "value": "pod.Usage(\"memory\") / 1048576.0"},
              {"le": 2.5, "value": "7.0", "hidden": true}, {"le": 1000000, "value": "2.0"},
              {"le": 5, "value": "pod.Usage(\"cpu\")"}]},
 {"name": "n_hist", "kind": "histogram", "dimension": "node", "help": "node histogram",
  "buckets": [{"le": 2, "value": "4.0"}, {"le": 1, "value": "3.0"}]},
 {"name": "a_gauge", "kind": "gauge", "dimension": "pod", "help": "a",
  "labels": [{"name": "namespace", "value": "pod.metadata.namespace"}, {"name": "pod", "value": "pod.metadata.name"}],
  "value": "pod.Usage(\"memory\")"}]}})JSON";

static const char* kHostBucket = R"JSON({"kind": "Metric", "spec": {"path": "/x", "metrics": [
 {"name": "host_hist", "kind": "histogram", "dimension": "node",
  "buckets": [{"le": 1, "value": "node.status.allocatable['cpu']"}]}]}})JSON";

static int bad(const std::string& what) {
  fprintf(stderr, "expo_program_walk: %s (%s)\n", what.c_str(), kwk_metric_set_last_error(nullptr));
  return 1;
}

int main() {
  kwk_metric_set* m = nullptr;
  if (kwk_compile_metrics_flags(kCR, KWK_METRICS_EXPO_HISTOGRAMS, &m) != KWK_OK) return bad("compile with the flag");
  kwk_expo_program p{};
  kwk_expo_hist_program hp{};
  if (kwk_metric_set_exposition(m, &p) != KWK_OK) return bad("kwk_metric_set_exposition");
  if (kwk_metric_set_exposition_histograms(m, &hp) != KWK_OK) return bad("kwk_metric_set_exposition_histograms");
  unsigned long sum = 0;  // every byte is read
  auto text = [&](uint32_t off, uint32_t len) {
    if ((uint64_t)off + len > p.n_lit_bytes) {
      fprintf(stderr, "expo_program_walk: bytes [%u, +%u) beyond lits (%u)\n", off, len, p.n_lit_bytes);
      exit(1);
    }
    std::string s(p.lits + off, len);
    for (char c : s) sum += (unsigned char)c;
    return s;
  };
  uint32_t n_hist_fam = 0;
  for (uint32_t f = 0; f < p.n_families; ++f) {
    const kwk_expo_family& F = p.families[f];
    const std::string name = text(F.name_off, F.name_len);
    text(F.header_off, F.header_len);
    if (F.group >= p.n_groups || p.groups[F.group].dimension != F.dimension) return bad("family group");
    printf("family %u %s kind %u metric %u dimension %u group %u\n", f, name.c_str(), F.reserved, F.metric, F.dimension, F.group);
    if (F.reserved == KWK_EXPO_KIND_SCALAR) {
      if (F.metric >= p.n_metrics || p.metric_dimension[F.metric] != F.dimension) return bad("scalar family metric");
      continue;
    }
    ++n_hist_fam;
    if (F.metric >= hp.n_hists || hp.hists[F.metric].dimension != F.dimension) return bad("histogram family metric");
    const kwk_expo_hist& H = hp.hists[F.metric];
    if ((uint64_t)H.first_line + H.n_visible + 3 > hp.n_lines) return bad("histogram lines");
    for (uint32_t k = 0; k < H.n_visible + 3; ++k) {
      const kwk_expo_hist_line& l = hp.lines[H.first_line + k];
      printf("  line %u: %s + block + %s\n", k, text(l.prefix_off, l.prefix_len).c_str(), text(l.tail_off, l.tail_len).c_str());
    }
  }
  if (p.n_families != 4 || n_hist_fam != 2 || hp.n_hists != 2 || hp.n_lines != 7 + 5) return bad("family / line counts");
  for (uint32_t g = 0; g < p.n_groups; ++g) {
    char block[128], key[128];
    uint32_t bl = 0, kl = 0;
    const char* pod = R"({"metadata": {"namespace": "ns", "name": "p\"1"}, "spec": {"containers": [{"name": "c"}]}})";
    if (kwk_metric_labels_render(m, g, R"({"metadata": {"name": "n"}})", pod, 0, block, sizeof block, &bl, key, sizeof key, &kl) !=
        KWK_OK)
      return bad("kwk_metric_labels_render");
    printf("group %u (dimension %u, %u labels): %.*s\n", g, p.groups[g].dimension, p.groups[g].n_labels, (int)bl, block);
    if ((bl != 0) != (p.groups[g].n_labels != 0)) return bad("label block");
  }
  kwk_metric_set_destroy(m);

  // refusals: without the flag; with it, a host-evaluated bucket value
  if (kwk_compile_metrics(kCR, &m) != KWK_OK) return bad("compile without the flag");
  if (kwk_metric_set_exposition(m, &p) != KWK_ENOLOWER || !strstr(kwk_metric_set_last_error(m), "m_hist"))
    return bad("a histogram CR without the flag must be refused naming m_hist");
  if (kwk_metric_set_exposition_histograms(m, &hp) != KWK_ENOLOWER) return bad("histogram tables without the flag");
  kwk_metric_set_destroy(m);
  if (kwk_compile_metrics_flags(kHostBucket, KWK_METRICS_EXPO_HISTOGRAMS, &m) != KWK_OK) return bad("compile host bucket CR");
  if (kwk_metric_set_exposition(m, &p) != KWK_ENOLOWER || !strstr(kwk_metric_set_last_error(m), "host_hist"))
    return bad("a host-evaluated bucket value must be refused naming host_hist");
  kwk_metric_set_destroy(m);
  printf("ok (byte sum %lu)\n", sum);
  return 0;
}
