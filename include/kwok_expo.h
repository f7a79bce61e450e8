/* Device metric exposition: the Prometheus text (format 0.0.4) of a scrape written by the GPU —
 * the consumer kwk_metrics_eval_device was left for.
 *
 * Replaces, per node scrape, the reference's registry gather + text encode
 * (pkg/kwok/metrics/metrics.go:480-502,525-573, pkg/kwok/server/metrics.go:129-150:
 * UpdateHandler.Update fills the gauges / counters, promhttp encodes every family sorted by name
 * and every series sorted by label values).  The host builds the exposition program once per
 * Metric CR (kwk_metric_set_exposition, kwok_metrics.h), renders every object's label block once
 * (kwk_metric_labels_render) and uploads blocks and sort keys (kwk_expo_set_labels /
 * kwk_expo_commit).  Each scrape, kwk_expo_scrape evaluates the values on the device
 * (kwk_metrics_eval_device) and writes, for every node of the range, the text
 * MetricsProgram.exposition(MetricsProgram.scrape(..)) gives for that node alone, byte for byte:
 * every family's HELP / TYPE lines (also when the node has no series of it), the series of live
 * pod slots in label order, the values as strconv.AppendFloat(v, 'g', -1, 64).  A histogram family
 * (a set compiled with KWK_METRICS_EXPO_HISTOGRAMS, a writer made by kwk_expo_create_hist) writes
 * what expfmt writes for histogram.Write's dto: per series the _bucket lines of the visible bounds
 * and +Inf, then _sum and _count, from the record kwk_histograms_eval_device leaves on the device
 * (counts as float64(uint64); a dead pod slot, by the alive bits, has no lines).
 *
 * Three launches per scrape on the engine's stream, no host round trip between them:
 *   lengths   a workgroup per node: formats every live value once (32 bytes of device memory per
 *             series of the range, and per record word of a histogram series), the bytes of the
 *             node's text
 *   scan      exclusive scan of the node totals into 64-bit offsets, the grand total
 *   write     a workgroup per node again: every line at its scanned offset
 * Output room is reserved by the caller (kwk_expo_reserve); a scrape whose text does not fit
 * writes nothing and kwk_expo_result returns KWK_ECAP (the write kernel compares the scanned total
 * with the reservation on the device, and every store is bounded by the node's scanned range).
 */
#ifndef KWOK_EXPO_H
#define KWOK_EXPO_H

#include <stdint.h>

#include "kwok_engine.h"
#include "kwok_metrics.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kwk_expo kwk_expo;

const char* kwk_expo_last_error(const kwk_expo* ex);
/* a writer for `pods`' scrapes (after kwk_usage_config / kwk_usage_mixed / kwk_usage_pods and
 * kwk_metrics_load of the same Metric CR) over its n_nodes nodes, on the engine's stream; the
 * program is copied.  Rows of a label group are nodes, pod slots or containers
 * (kwk_usage_read_containers order) by the group's dimension. */
kwk_status kwk_expo_create(kwk_engine* pods, uint32_t n_nodes, const kwk_expo_program* prog, kwk_expo** out);
/* the same for a program with histogram families (kind code 1; also after kwk_histograms_load of
 * the same CR), with their tables (kwk_metric_set_exposition_histograms; copied).  kwk_expo_create
 * given such a program returns KWK_EINVAL naming the family.  Every other call is the same for
 * both; a scrape also runs kwk_histograms_eval_device and returns KWK_ESTATE when the engine's
 * record words are not the program's (every histogram: its series x (n_visible + 3)). */
kwk_status kwk_expo_create_hist(kwk_engine* pods, uint32_t n_nodes, const kwk_expo_program* prog,
                                const kwk_expo_hist_program* hist_prog, kwk_expo** out);
kwk_status kwk_expo_destroy(kwk_expo* ex);
/* rows [first, first + n) of `group`: row i's label block is blocks[block_offsets[i] ..
 * block_offsets[i + 1]) and its sort key keys[key_offsets[i] .. key_offsets[i + 1])
 * (kwk_metric_labels_render's outputs; offsets hold n + 1 entries).  Host-side until
 * kwk_expo_commit or kwk_expo_commit_rows (the rows set since the last commit are remembered as
 * dirty).  After a pod is replaced: set its rows again and kwk_expo_commit_rows.  The row counts are the
 * engine's layout as of kwk_expo_create or the last kwk_expo_commit: after a kwk_usage_config /
 * kwk_usage_mixed that changes the pod or container count, commit once (it re-reads the layout and
 * keeps the rows set so far), then set the new rows and commit again.  Rows of dead slots need not
 * be set; a scrape that meets a live series of a labelled group whose row was never set writes
 * nothing and kwk_expo_result returns KWK_ESTATE with their count (a histogram series counts once,
 * not once per line). */
kwk_status kwk_expo_set_labels(kwk_expo* ex, uint32_t group, uint32_t first, uint32_t n, const uint32_t* block_offsets,
                               const char* blocks, const uint32_t* key_offsets, const char* keys);
/* stable-sorts every node's rows of each group by key (bytewise; ties keep row order: the order of
 * exposition()'s sorted(series, key=label values)) and uploads blocks, keys and permutations, packed
 * (it compacts what kwk_expo_commit_rows appended).  Re-reads the engine's node_ptr / container
 * layout; synchronises the stream; clears the dirty rows.
 * A writer is for one slot layout (the engine's kwk_layout_epoch at kwk_expo_create): its node
 * count is fixed at create and its rows are placed by that layout's node_ptr.  After a kwk_relayout
 * (nodes added or removed, series moved) kwk_expo_set_labels, kwk_expo_commit, kwk_expo_commit_rows
 * and kwk_expo_scrape return KWK_ESTATE ("create a writer for the new layout (kwk_expo_create), set
 * the rows of the new layout and kwk_expo_commit").  There is no incremental relayout: a relayout
 * costs the exposition a new writer, every row set and a full commit. */
kwk_status kwk_expo_commit(kwk_expo* ex);
/* The commit of a live cluster: brings only the rows given to kwk_expo_set_labels since the last
 * commit (of either kind) up to date, at a cost that follows those rows.  After KWK_OK every later
 * scrape writes the text it would write after kwk_expo_commit of the same host state; every row's
 * block and every group's permutation are the ones that call would produce (kwk_expo_read_perm).
 *
 * A group's blocks (and, for pod and container groups, its sort keys) live in a device arena with an
 * {offset, length} pair per row.  kwk_expo_commit lays the rows out packed with slack at the tail; this
 * call overwrites a row in place where the new bytes fit its slot and appends it at the tail where
 * they do not; a full tail doubles the arena (copied on the stream; the old buffer is freed by a later
 * call, after an event).  All dirty blocks and keys go up in one staging copy, a scatter kernel puts
 * them in place, and expo_sort_kernel re-sorts each node that holds a dirty row of a pod or container
 * group — nodes of up to KWK_EXPO_SORT_MAX_ROWS rows of the group on the device; a larger node is
 * sorted on the host (that node only) and its slice of the permutation goes up with the same copy.
 *
 * Everything is enqueued on the engine's stream, before the next scrape.  The call does not wait for
 * that stream: it waits only for its own previous staging copy (an event), and for an 8-byte read of
 * the engine's pod and container totals on a stream of its own.
 *   no dirty rows                      KWK_OK, nothing enqueued
 *   no kwk_expo_commit yet, or an earlier call of this kind failed part-way
 *                                      KWK_ESTATE
 *   the engine's pod or container count is not the last kwk_expo_commit's
 *                                      KWK_ESTATE: kwk_expo_commit (the dirty rows are kept)
 *   a group's blocks or keys would pass 4 GiB (appended slots are not reclaimed)
 *                                      KWK_ECAP: kwk_expo_commit compacts the storage
 * A kwk_usage_config / kwk_usage_mixed that moves pods between nodes or containers between pods but
 * keeps both counts is not seen here: follow every such call with kwk_expo_commit.
 * Measured at 10k nodes / 1M pods (DESIGN.md "Incremental label commits"; every row appended, the
 * dearest case): 0.1 % / 1 % / 10 % of the pods relabelled — the call returns after 0.5 / 3.9 / 32 ms
 * and the stream has finished it after 1.8 / 8.2 / 40 ms, where kwk_expo_commit takes 0.33 s and
 * stalls the stream.  Faster at every fraction measured; by its 0.3-0.4 us per relabelled pod it
 * meets the full commit only near every pod relabelled: prefer kwk_expo_commit then, after a
 * relayout, and when KWK_ECAP asks for compaction. */
kwk_status kwk_expo_commit_rows(kwk_expo* ex);
#define KWK_EXPO_SORT_MAX_ROWS 1024u
/* output room: text bytes one scrape may produce */
kwk_status kwk_expo_reserve(kwk_expo* ex, uint64_t max_bytes);
/* enqueue one scrape of nodes [node_first, node_first + n_nodes) at now_ns, after the caller's
 * kwk_usage(now_ns): kwk_metrics_eval_device, kwk_metrics_series_device (kwk_histograms_eval_device
 * when the program has histogram families), then the three kernels */
kwk_status kwk_expo_scrape(kwk_expo* ex, int64_t now_ns, uint32_t node_first, uint32_t n_nodes);
/* synchronise; the last scrape's text size.  KWK_ECAP when it exceeds the reservation: nothing was
 * written — reserve more and scrape again.  KWK_ESTATE: live series without a label row (above) */
kwk_status kwk_expo_result(kwk_expo* ex, uint64_t* n_bytes);
/* device outputs of the last scrape: n_nodes + 1 byte offsets and the bytes; node j of the range's
 * text is bytes[offsets[j] .. offsets[j + 1]) */
kwk_status kwk_expo_device(kwk_expo* ex, const uint64_t** offsets, const char** bytes);
/* copy them to host memory (n_nodes + 1 offsets; the size from kwk_expo_result) */
kwk_status kwk_expo_copy(kwk_expo* ex, uint64_t* offsets, char* bytes);
/* HIP events around the last scrape's kernels: milliseconds of [0] the whole scrape (value
 * evaluation included), [1] lengths, [2] scan, [3] write */
kwk_status kwk_expo_elapsed(kwk_expo* ex, float ms[4]);
/* Tuning and diagnosis hook, not part of the serving path (tests and tools/expo_bench.py cover both
 * kernels with it; the default's threshold is measured at one shape only and may change): workgroup
 * size per node, 64 (a wave per node), 256, or 0 = the default, chosen from the mean pods per node */
kwk_status kwk_expo_set_width(kwk_expo* ex, uint32_t width);
/* the device formatter over n doubles (tests, diagnosis): out = n x 24 bytes, lens = n lengths */
kwk_status kwk_expo_format_values(kwk_expo* ex, const double* host_values, uint32_t n, char* out, uint8_t* lens);
/* the host build of the same formatter (no GPU): strconv.AppendFloat(v, 'g', -1, 64) -> length */
uint32_t kwk_expo_format_f64(double v, char out[24]);
/* a pod or container group's device permutation copied to the host (synchronises; tests, diagnosis):
 * out = the group's rows; entry i of a node's row range is the row written i-th.  KWK_EINVAL for a
 * node-dimension group (it has none) */
kwk_status kwk_expo_read_perm(kwk_expo* ex, uint32_t group, uint32_t* out);
/* the host build of the device sort's comparator (no GPU): < 0, 0, > 0 as key a sorts before, with or
 * after key b — unsigned bytes, a proper prefix first (std::string's order) */
int kwk_expo_key_compare(const char* a, uint32_t na, const char* b, uint32_t nb);
/* HIP events around the last kwk_expo_commit_rows that enqueued work: milliseconds of [0] the scatter
 * kernel, [1] the sort kernel (synchronises with them) */
kwk_status kwk_expo_commit_rows_elapsed(kwk_expo* ex, float ms[2]);

#ifdef __cplusplus
}
#endif

#endif
