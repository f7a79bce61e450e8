/* The Events of fired Stages as a device stream of the emitter (libkwok_emit.so).
 *
 * playStage sends three things for a fired object, in this order (pod_controller.go:304-352,
 * node_controller.go:369, stage_controller.go:282): the Stage's Event, the finalizer JSON patch,
 * the delete or the merge patches.  kwok_emit.h emits the third and the second; this header adds
 * the first as a third stream of the same output sets.  The entry points live in libkwok_emit.so
 * beside kwok_emit.h's and act on the same kwk_emitter; kwok_emit.h itself does not change.
 *
 * The bytes of an item are the Event body of kwok_patch.h (kwk_patch_event): what recorder.Event
 * hands the broadcaster, restated there from client-go v0.30.2 tools/record/event.go, k8s.io/api
 * core/v1/types.go, apimachinery's ObjectMeta and metav1.Time, and encoding/json.  The sink-side
 * EventCorrelator (dedup into count patches, aggregation, the spam filter) is not applied.
 *
 *   {"metadata":{"name":"<name>.<hex>","namespace":"<ref ns or default>","creationTimestamp":null},
 *    "involvedObject":{"kind":"<Kind>"[,"namespace":"<ns>"][,"name":"<name>"][,"uid":"<uid>"][,"apiVersion":"<av>"]},
 *    ["reason":"<reason>",]["message":"<message>",]"source":{"component":"<component>"},
 *    "firstTimestamp":"<ts>","lastTimestamp":"<ts>","count":1,"type":"<type>","eventTime":null,
 *    "reportingComponent":"<component>","reportingInstance":""}
 *
 * <hex> = now_ns as %x and <ts> = now_ns in whole seconds, UTC, 2006-01-02T15:04:05Z: constants of
 * an emission.  A record's body is its stage's text with the object's name (twice), namespace
 * (once or twice) and uid inserted, read from three identity columns of [length][text] rows.
 *
 * The device writes only text that needs no escaping: the program's strings are bytes 0x20..0x7E
 * without " \ < > & (kwk_program_event_spec(device = 1) refuses others by name) and a row is usable
 * only when its text is bytes 0x21..0x7E without those five; everything else is an item with
 * KWK_EMIT_HOST and no bytes, which the host renders with kwk_patch_event.
 */
#ifndef KWOK_EVENTS_H
#define KWOK_EVENTS_H

#include <stdint.h>

#include "kwok_emit.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KWK_EVT_STAGE_EVENT 1u /* stage_flags: the stage records an Event (type Normal or Warning) */

#define KWK_EVT_COL_NAME 0u
#define KWK_EVT_COL_NAMESPACE 1u
#define KWK_EVT_COL_UID 2u

#define KWK_EVT_ROW_UNUSABLE 0xFFu /* a row's length byte: the host renders this object's Events */
#define KWK_EVT_MAX_TEXT 16384u    /* bytes of type + reason + message over all event stages */

/* The event program (kwk_program_event_spec(device = 1) / KindProgram.event_spec(device=True)).
 * kind, api_version, component: NUL-terminated.  api_version "" is the typed Pod / Node
 * controllers' reference (no apiVersion key; kind Node: no involvedObject.namespace, the column is
 * not read); any other value is written as the reference's apiVersion — the host marks the rows of
 * an object with another apiVersion unusable.
 * Stage s records an Event when stage_flags[s] has KWK_EVT_STAGE_EVENT; its type, reason and message
 * are text[text_off[3s] .. text_off[3s+1]), [3s+1 .. 3s+2), [3s+2 .. 3s+3) (text_off: 3 * n_stages
 * + 1 non-decreasing offsets); an empty reason or message leaves its key out.  The library forms
 * the stage's literal runs from them.
 * stride_*: bytes per row of the identity columns, multiples of 4 in 4..256; stride_namespace 0 is
 * a cluster-scoped kind: no column, every object's namespace is empty. */
typedef struct kwk_evt_program {
  const char* kind;
  const char* api_version;
  const char* component;
  uint32_t n_stages; /* the emit program's */
  const uint8_t* stage_flags;
  const uint32_t* text_off;
  const char* text;
  uint32_t stride_name, stride_namespace, stride_uid;
} kwk_evt_program;

typedef struct kwk_evt_item {
  uint32_t rec;   /* index into the fired list */
  uint8_t status; /* KWK_EMIT_OK: bytes follow; KWK_EMIT_HOST: no bytes, kwk_patch_event renders it */
  uint8_t reserved[3];
} kwk_evt_item;

/* Once per emitter (KWK_ESTATE for a second load).  Afterwards every kwk_emit / kwk_emit_step also
 * emits the list's Events: per record of an event stage one item, in list order — KWK_EMIT_OK and
 * the body when the slot is below the capacity, its three rows are usable and its name is not empty
 * (ObjectReference.Name is omitempty: the key goes, kwk_patch_event writes that), else KWK_EMIT_HOST.
 * The stream reads the rows and writes no per-slot state.  Rows start out unusable.  A program
 * with no event stage launches nothing: its stream is empty.  KWK_EINVAL names a string the device
 * does not carry, more than KWK_EVT_MAX_TEXT bytes of stage text, or a bad stride.
 *
 * Launches per emission: emit_evt_size_kernel (per 256-record tile: items and bytes; the row
 * lengths are gathered only for event stages), emit_scan_kernel over the event tile arrays,
 * emit_evt_write_kernel.  Size and scan run before any writer, with the finalizer stream's: an
 * overflow of the merge-patch, finalizer or event stream raises the flag of the emissions in
 * flight, no writer of that emission or of those behind it writes anything, and every reader
 * returns KWK_ECAP (kwk_emit.h "several emissions in flight"). */
kwk_status kwk_evt_load(kwk_emitter* em, const kwk_evt_program* prog);

/* kwk_evt_load's checks of the program alone — no emitter, no device: the strings, the strides, the
 * text budget and n_stages <= KWK_MAX_STAGES (the kernels' per-stage tables hold that many).  The
 * message is the calling thread's (kwk_emit_last_error(NULL)).  A host calls it where it loads its
 * Stages; kwk_evt_load runs the same checks and also wants n_stages equal to the emit program's. */
kwk_status kwk_evt_check(const kwk_evt_program* prog);

/* rows [first, first + n) of identity column `column` (KWK_EVT_COL_*): n * stride bytes, each row
 * [length][text] with length <= stride - 1, or KWK_EVT_ROW_UNUSABLE.  The host marks a row unusable
 * when its text has a byte outside 0x21..0x7E or one of " \ < > &, does not fit, or belongs to an
 * object whose apiVersion is not the program's. */
kwk_status kwk_evt_set_rows(kwk_emitter* em, uint32_t column, uint32_t first, uint32_t n, const uint8_t* data);

/* room of the event stream in every output set (kwk_emit_reserve_fin's semantics) */
kwk_status kwk_evt_reserve(kwk_emitter* em, uint32_t max_items, uint64_t max_bytes);

/* The selected emission's (kwk_emit_select) event stream: its items and bytes; *launched (may be
 * NULL) = 1 when the program has an event stage, i.e. the emission ran the event kernels, else 0.
 * KWK_ECAP as kwk_emit_result; when the event stream itself was the short one the message names
 * kwk_evt_reserve and the totals. */
kwk_status kwk_evt_result(kwk_emitter* em, uint32_t* n_items, uint64_t* n_bytes, uint32_t* launched);
/* device pointers of the selected emission's stream: items, n_items + 1 offsets, the bytes */
kwk_status kwk_evt_device(kwk_emitter* em, const kwk_evt_item** items, const uint64_t** offsets, const char** bytes);
/* ... and copies of them (kwk_evt_result's counts; offsets always gets offsets[0]) */
kwk_status kwk_evt_copy(kwk_emitter* em, kwk_evt_item* items, uint64_t* offsets, char* bytes);

#ifdef __cplusplus
}
#endif

#endif
