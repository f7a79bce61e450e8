/*
 * kwok_metrics.h — native Metric CR compiler (host C++, no GPU): a kwok Metric CR -> the device
 * programs kwk_metrics_load / kwk_histograms_load take (kwok_engine.h).  The drop-in for the
 * reference's per-scrape CEL compilation of Metric values, called from Go through cgo
 * (INTEGRATION.md):
 *
 *   reference (Go)                                              replaced by
 *   ----------------------------------------------------------  -----------------------------------
 *   UpdateHandler.updateGauge / updateCounter / updateHistogram  kwk_compile_metrics once per Metric
 *     -> h.environment.Compile(metricConfig.Value) per metric      CR -> kwk_metric_set_programs /
 *     and bucket  pkg/kwok/metrics/metrics.go:168-462              _histograms -> kwk_metrics_load /
 *   cel.Environment.Compile (cached by source)                     kwk_histograms_load; per scrape
 *     pkg/utils/cel/environment.go:98-114                          kwk_metrics_eval /
 *   the metrics environment (Usage / CumulativeUsage /             kwk_histograms_eval
 *     StartedContainersTotal, node / pod / container variables)
 *     pkg/kwok/metrics/evaluator.go:51-144,201-233
 *
 * A value lowers to a postfix program over doubles when it is double arithmetic over the
 * per-series inputs (KWK_MIN_*) and constants; constant sub-expressions are folded with CEL's
 * semantics (int / uint overflow, Quantity arithmetic incl. the Quantity x double x10 rule).  A
 * metric with any value that has no device form is reported in describe's "host_metrics": the
 * host evaluates it per series (its device program is a placeholder: NaN for a gauge / counter,
 * 0 for every bucket of a histogram), exactly as the Python host's MetricsProgram does
 * (kwok_amd/host/metrics.py, cel.py lower), which is this compiler's CPU cross-check: byte-equal
 * programs on the shipped Metric CR, the histogram CRs and the reference-vector CR
 * (tests/test_metric_compiler.py).
 *
 * Exposition (the Prometheus text of a scrape, written on the device by kwok_expo.h): the set also
 * builds the exposition program — families in name order with their HELP / TYPE bytes and label
 * group — and renders an object's label block natively (kwk_metric_labels_render), for the label
 * expressions that are a string literal or a field selection from node / pod / container.  A CR
 * with any other label or a host-evaluated metric has no exposition program (KWK_ENOLOWER names
 * it): its text stays with the host (kwok_amd/host/metrics.py exposition).  So does a CR with a
 * histogram, unless the set was compiled with KWK_METRICS_EXPO_HISTOGRAMS
 * (kwk_compile_metrics_flags): then the histogram families are part of the program (kind code 1)
 * and kwk_metric_set_exposition_histograms gives their per-line tables.
 *
 * Threading: a metric set is read-only after kwk_compile_metrics; sets are independent.
 */
#ifndef KWOK_METRICS_H
#define KWOK_METRICS_H

#include <stdint.h>

#include "kwok_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KWK_ENOLOWER (-5) /* kwk_cel_lower: a valid expression with no device form (host-evaluated) */

typedef struct kwk_metric_set kwk_metric_set;

/* message of the calling thread's last failing call (m may be NULL: the messages are kept per
 * thread, whichever set the call named) */
const char* kwk_metric_set_last_error(const kwk_metric_set* m);

/* metric_json: one v1alpha1 Metric object (JSON; {"kind": "Metric", "spec": {"path", "metrics":
 * [{name, help, kind: gauge|counter|histogram, dimension: node|pod|container (default node),
 * value, labels: [{name, value}], buckets: [{le, value, hidden}]}]}}).  KWK_EINVAL for a malformed
 * CR, an unknown kind / dimension, a histogram without buckets, or a value that does not compile
 * (CEL syntax, or a constant sub-expression whose evaluation fails: the reference's
 * EvaluateFloat64 would fail at every scrape). */
kwk_status kwk_compile_metrics(const char* metric_json, kwk_metric_set** out);
/* the same with flags (kwk_compile_metrics is flags 0).  KWK_METRICS_EXPO_HISTOGRAMS: histogram
 * families join the exposition program instead of refusing it (below); the device programs,
 * describe and every other accessor are the same with or without it */
#define KWK_METRICS_EXPO_HISTOGRAMS 1u
kwk_status kwk_compile_metrics_flags(const char* metric_json, uint32_t flags, kwk_metric_set** out);
kwk_status kwk_metric_set_destroy(kwk_metric_set* m);

/* gauges and counters, in CR order (arrays owned by the set): for kwk_metrics_load */
kwk_status kwk_metric_set_programs(const kwk_metric_set* m, uint32_t* n_metrics, const kwk_metric_desc** metrics,
                                   uint32_t* n_ops, const kwk_metric_op** ops);
/* histograms, in CR order: for kwk_histograms_load */
kwk_status kwk_metric_set_histograms(const kwk_metric_set* m, uint32_t* n_hist, const kwk_histogram_desc** hists,
                                     uint32_t* n_buckets, const kwk_metric_bucket** buckets, uint32_t* n_ops,
                                     const kwk_metric_op** ops);
/* JSON owned by the set: {"path", "metrics": [{"name", "help", "kind", "dimension", "labels":
 * [{"name", "value"}], "device": bool, "reason": "...", "program": index among the gauges /
 * counters or among the histograms}], "host_metrics": [names]} */
kwk_status kwk_metric_set_describe(const kwk_metric_set* m, const char** json);

/* one value expression -> its device program (dimension KWK_METRIC_DIM_*, or 3 for a dimension
 * the Metric CRD does not define); *n_ops = the program length (also when cap is too small:
 * KWK_ECAP).  KWK_ENOLOWER: no device form; KWK_EINVAL: the expression does not compile. */
kwk_status kwk_cel_lower(const char* expr, uint32_t dimension, kwk_metric_op* out, uint32_t cap, uint32_t* n_ops);

/* ------------------------------------------------------------------ exposition program */
typedef struct {
  uint32_t name_off, name_len;     /* the family's name in lits */
  uint32_t header_off, header_len; /* "# HELP <name> <escaped help>\n# TYPE <name> <kind>\n" in lits */
  uint32_t metric;                 /* index among the gauges / counters: kwk_metrics_eval's order (kind 1:
                                      among the histograms, kwk_histograms_eval's order) */
  uint32_t dimension;              /* KWK_METRIC_DIM_* */
  uint32_t group;                  /* its label group */
  uint32_t reserved;               /* the kind code: KWK_EXPO_KIND_SCALAR (gauge / counter) or _HISTOGRAM */
} kwk_expo_family;
#define KWK_EXPO_KIND_SCALAR 0u
#define KWK_EXPO_KIND_HISTOGRAM 1u /* only in a set compiled with KWK_METRICS_EXPO_HISTOGRAMS */
typedef struct {
  uint32_t dimension;  /* rows are nodes, pod slots or containers (kwk_usage_read_containers order) */
  uint32_t n_labels;   /* 0: the series line has no label block */
} kwk_expo_group;
typedef struct {
  uint32_t n_families, n_groups, n_metrics, n_lit_bytes;
  const kwk_expo_family* families;    /* in name order (client_golang's Gather) */
  const kwk_expo_group* groups;       /* distinct (dimension, ordered labels) */
  const uint32_t* metric_dimension;   /* n_metrics: every gauge / counter of the CR, in CR order */
  const char* lits;
} kwk_expo_program;

/* the set's exposition program (arrays owned by the set).  All or nothing — KWK_ENOLOWER, the
 * message naming the metric (and label), when a family is a histogram (and the set was compiled
 * without KWK_METRICS_EXPO_HISTOGRAMS), is host-evaluated (a histogram: any of its bucket values),
 * or has a label expression outside the supported subset (a string literal, or node / pod /
 * container followed by field selections): a node's text with families missing is not servable.
 * With the flag the histogram families stand in name order among the others, kind code 1, and share
 * label groups with them by the same rule (dimension + ordered labels). */
kwk_status kwk_metric_set_exposition(const kwk_metric_set* m, kwk_expo_program* out);

/* The histogram families' tables (what kwk_expo_program has no room for).  A series of histogram N
 * with label block B = `{a="x"}` is n_visible + 3 lines, in the text's order (expfmt
 * text_create.go over histogram.Write's dto; record word = the word of kwk_histograms_eval's
 * n_visible + 3 word record the line prints):
 *   line k < n_visible   N_bucket{a="x",le="<bound k>"} <count>    word k   (bounds ascending, NaN first)
 *   line n_visible       N_bucket{a="x",le="+Inf"} <count>         word n_visible
 *   line n_visible + 1   N_sum{a="x"} <sum>                        word n_visible + 2 (float64 bits)
 *   line n_visible + 2   N_count{a="x"} <count>                    word n_visible + 1
 * Counts print as float64(uint64) (round to nearest even), every value as strconv 'g', -1, 64.
 * Every line has one shape, so the writer does not branch on the kind of line:
 *   prefix + B without its closing brace + tail + ' ' + value + '\n'
 * prefix = N_bucket / N_sum / N_count; tail = `,le="<bound>"}` for a bucket and `}` for _sum /
 * _count when the family's group has labels, `{le="<bound>"}` and nothing when it has none (B is
 * empty).  <bound> is rendered by the host build of the device formatter. */
typedef struct {
  uint32_t prefix_off, prefix_len; /* in the kwk_expo_program's lits */
  uint32_t tail_off, tail_len;
} kwk_expo_hist_line;
typedef struct {
  uint32_t dimension;  /* KWK_METRIC_DIM_* */
  uint32_t n_visible;  /* visible buckets: a series' record is n_visible + 3 words */
  uint32_t first_line; /* its n_visible + 3 entries of lines */
  uint32_t reserved;
} kwk_expo_hist;
typedef struct {
  uint32_t n_hists, n_lines;
  const kwk_expo_hist* hists;      /* every histogram of the CR, in CR order (kwk_histograms_eval's) */
  const kwk_expo_hist_line* lines;
} kwk_expo_hist_program;
/* arrays owned by the set; n_hists = 0 for a set without the flag or without histograms.
 * KWK_ENOLOWER as kwk_metric_set_exposition. */
kwk_status kwk_metric_set_exposition_histograms(const kwk_metric_set* m, kwk_expo_hist_program* out);

/* One object's labels of `group`: block = `{k="v",k2="v2"}` with the values escaped as the text
 * format does (\\, \n, \") — empty for a group without labels — and key = its sort key: the
 * unescaped values in label order, each ended by a 0 byte (a 0 / 1 byte inside a value is written
 * 1 1 / 1 2), so that bytewise order of keys is the order of the value lists.  node_json /
 * pod_json: the objects the expressions select from (NULL when the group's labels do not read
 * it); container = pod.spec.containers[container_index] for a container group.  *block_len /
 * *key_len are always the sizes needed; KWK_ECAP when a cap is smaller (nothing usable written).
 * KWK_EINVAL, naming the object and label, where the selection fails: a missing object or key, or
 * a leaf that is not a string (the typed zero values CEL would substitute are not guessed). */
kwk_status kwk_metric_labels_render(const kwk_metric_set* m, uint32_t group, const char* node_json, const char* pod_json,
                                    uint32_t container_index, char* block, uint32_t block_cap, uint32_t* block_len,
                                    char* key, uint32_t key_cap, uint32_t* key_len);

#ifdef __cplusplus
}
#endif
#endif /* KWOK_METRICS_H */
