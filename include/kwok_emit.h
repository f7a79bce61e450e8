/* Device patch emission: the merge-patch bytes of fired objects written by the GPU
 * (the device form of kwok_patch.h).
 *
 * Replaces, per fired object, the reference's Next.Patches → computeMergePatch →
 * gotpl.Renderer.ToJSON round trip (pkg/utils/lifecycle/next.go:73-160,
 * pkg/utils/gotpl/renderer.go:59-124) for the templates whose bytes are fixed by the object's
 * class up to Now and the values of the controller's functions: the host builds each
 * (class, template) skeleton once with kwk_patch_skeleton (literal runs + slots), checks every
 * object once with kwk_patch_object_values (its render equals the skeleton; its call values,
 * e.g. funcPodIPWith / funcNodeIPWith of pod_controller.go:563-600, are fixed for the object's
 * life) and uploads per-slot words and value columns.  Each step, kwk_emit expands the engine's
 * fired list into the patches on the device: byte-equal to kwk_patch_render of the same object,
 * or KWK_EMIT_HOST for the items the host renders itself (ineligible template, object not
 * accepted, status guard not met, unusable value).
 *
 * Status guards: the Stages' `index $root.status.<list> $i` inside `range $i := <spec list>`
 * fails the render when the status list is shorter than the spec list.  Guard bit k of a slot's
 * word says the guard holds for the object's current status; the host sets it at ingest, the
 * emitter keeps it through every record it emits (a template's patch leaves it, or sets it to
 * the value its status list gives), an emitted delete resets it to the class's fresh value (the
 * harness re-creates from spec).  A record with an item left to the host keeps its word: the host
 * sets it (kwk_emit_set_words) once it has rendered and applied that object's patches, as it
 * does after any kwk_replace / kwk_upsert.
 *
 * Emission from the hand-back ring (DESIGN.md §5 "Emission from the ring"): kwk_emit reads the
 * engine's last list; kwk_emit_step reads the list of any step the engine's ring still holds
 * (kwk_ring_view), in the format its compaction left — the 2-byte KWK_COMPACT_PACKED16 lists of
 * the fused sweep included — so a host calls kwk_step_n(eng, n, ...) once and kwk_emit_step for
 * step0 .. step0 + n - 1, each into an output set of its own (kwk_emit_reserve_sets), with no
 * synchronisation in between, and reads the n emissions afterwards (kwk_emit_select).  Still
 * refused: KWK_COMPACT_BITS lists, and any host intervention between the steps of a fused group
 * (kwk_emit_set_words / _set_column for host-rendered items belong at group boundaries: the
 * emissions of a group run in step order on the guard bits the earlier ones left).
 */
#ifndef KWOK_EMIT_H
#define KWOK_EMIT_H

#include <stdint.h>

#include "kwok_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kwk_emitter kwk_emitter;

#define KWK_EMIT_NO_SLOT 0xFFFFu
/* a literal run of the skeleton followed by a slot: KWK_EMIT_NO_SLOT, 0 = Now (RFC3339Nano, UTC),
 * 1 + c = value column c */
typedef struct {
  uint32_t lit_off;
  uint16_t lit_len;
  uint16_t slot;
} kwk_emit_piece;

typedef struct {
  uint32_t first_piece, n_pieces;
  uint8_t need;  /* guard bits the template's render requires */
  uint8_t keep;  /* guard bits its patch leaves as they are ... */
  uint8_t set;   /* ... and the values of the others after it */
  uint8_t reserved;
} kwk_emit_skel;

typedef struct {
  uint32_t n_classes, n_templates, n_stages, n_skels, n_pieces, n_columns;
  uint64_t n_lit_bytes;
  const uint32_t* stage_tpl_ptr;  /* n_stages + 1: stage s's templates are stage_tpl[ptr[s] .. ptr[s + 1]) */
  const uint16_t* stage_tpl;      /* template ids (< 32) in patch order */
  const uint8_t* stage_delete;    /* n_stages: the stage deletes the object (KWK_NEXT_DELETE) */
  const int32_t* skel_of;         /* n_classes * n_templates: skeleton index, -1 = the host renders */
  const kwk_emit_skel* skels;
  const kwk_emit_piece* pieces;
  const char* lits;
  const uint8_t* fresh_guards;    /* n_classes: guard bits of an object created from its spec */
  const uint32_t* column_stride;  /* n_columns: bytes per slot, a multiple of 4 in 4..256: [length][text]
                                   (length 0xFF = unusable) */
} kwk_emit_program;

/* per slot: bits 0-15 class, 16-23 guard bits, 32-63 template accepted (bit tid); bits 24-31 are
 * reserved (the device caches the slot's value lengths there: kwk_emit_get_words returns them 0) */
#define KWK_EMIT_WORD(cls, guards, accepted) \
  ((uint64_t)(uint16_t)(cls) | (uint64_t)(uint8_t)(guards) << 16 | (uint64_t)(uint32_t)(accepted) << 32)

#define KWK_EMIT_OK 0
#define KWK_EMIT_HOST 1 /* render this item with kwk_patch_render / the host renderer */
typedef struct {
  uint32_t rec;     /* index in the fired list */
  uint16_t tid;     /* template id */
  uint8_t status;   /* KWK_EMIT_* */
  uint8_t reserved;
} kwk_emit_item;

#define KWK_EMIT_FROM_RECORDS 0u /* kwk_fired_device(KWK_COMPACT_REC)'s list */
#define KWK_EMIT_FROM_PACKED 1u  /* kwk_fired_device(KWK_COMPACT_PACKED)'s list */
/* (round 5: the wave-per-record writers selected by bits 8 / 9 are retired — measured slower than
 * the lane-per-record writer; any other bit of source is KWK_EINVAL) */

const char* kwk_emit_last_error(const kwk_emitter* em);
/* an emitter for `eng`'s fired lists over slots [0, capacity), on the engine's stream.
 * Its words, order words, value columns and event rows are per slot, for the engine's slot layout
 * at create (kwk_layout_epoch): after a kwk_relayout they belong to other objects, so kwk_emit and
 * kwk_emit_step return KWK_ESTATE ("create an emitter for the new layout (kwk_emitter_create) and
 * set its words and columns") instead of emitting from them.  The old emitter's words stay readable
 * (kwk_emit_get_words / _get_fin_words carry the guard bits earlier emissions set): the host
 * permutes them by the relayout's runs for the new emitter.  A device-side move of the columns is
 * not provided. */
kwk_status kwk_emitter_create(kwk_engine* eng, uint32_t capacity, const kwk_emit_program* prog, kwk_emitter** out);
kwk_status kwk_emitter_destroy(kwk_emitter* em);
kwk_status kwk_emit_set_words(kwk_emitter* em, uint32_t first, uint32_t n, const uint64_t* words);
kwk_status kwk_emit_get_words(kwk_emitter* em, uint32_t first, uint32_t n, uint64_t* words);
/* rows [first, first + n) of value column c: n * column_stride[c] bytes */
kwk_status kwk_emit_set_column(kwk_emitter* em, uint32_t c, uint32_t first, uint32_t n, const uint8_t* data);
/* output room: items and patch bytes one kwk_emit may produce (in every output set; their number
 * stays) */
kwk_status kwk_emit_reserve(kwk_emitter* em, uint32_t max_items, uint64_t max_bytes);
/* enqueue the emission of the engine's last compacted fired list (source: KWK_EMIT_FROM_*) */
kwk_status kwk_emit(kwk_emitter* em, int64_t now_ns, uint32_t source);
/* enqueue the emission of the ring list of step `step` (kwk_step's step / kwk_step_n's step0 + k;
 * KWK_STEP_LAST: the engine's list) in whatever format its compaction left: KWK_COMPACT_REC, _PACKED
 * or _PACKED16.  KWK_ESTATE with the engine's message when the ring no longer holds the step
 * (kwk_fired_keep), and for a KWK_COMPACT_BITS list (the message names the format).  A list of no
 * segments (a step that swept nothing) is empty: 0 items, 0 bytes.  Call it while the ring slot is
 * intact (kwk_ring_view's rule: before the engine's next kwk_step_n call, for a call of at most
 * kwk_fired_keep() steps). */
kwk_status kwk_emit_step(kwk_emitter* em, uint64_t step, int64_t now_ns);
/* Several emissions in flight.  An emitter has 1..8 output sets (items, offsets, bytes, totals and
 * the elapsed-time events), one by default; every kwk_emit / kwk_emit_step writes the set after the
 * previous emission's, in turn, so up to n_sets emissions are enqueued back to back and read
 * afterwards.  kwk_emit_reserve_sets synchronises, gives every set room for max_items / max_bytes (a
 * set that has to grow loses its outputs; another number of sets frees them all and starts the turn
 * over).  kwk_emit_select makes kwk_emit_result / _stats / _device / _copy / _elapsed refer to the
 * emission `back` before the last (0 = the last; < n_sets and < the emissions since the sets were
 * made); every new emission selects 0 again.
 *
 * Overflow with emissions in flight (n_sets > 1).  An emission whose totals exceed its set writes
 * nothing and leaves the words unchanged, and raises a flag on the device; every emission enqueued
 * after it, before the host has noticed, finds the flag, writes nothing and leaves the words alone
 * too (its step's emission would read the guard bits the failed one was meant to leave).
 * kwk_emit_result of the failed emission and of each later one returns KWK_ECAP (the later ones'
 * totals read 0), so the words are exactly those after the last emission that completed.  The flag
 * is cleared by kwk_emit_reserve / _reserve_sets, and by the first emission enqueued after a reader
 * has returned KWK_ECAP: the caller reserves more and emits again from the first failed step, and
 * the result is exact.  With one set every emission stands alone, as it always did. */
kwk_status kwk_emit_reserve_sets(kwk_emitter* em, uint32_t n_sets, uint32_t max_items, uint64_t max_bytes);
kwk_status kwk_emit_select(kwk_emitter* em, uint32_t back);
/* synchronise; the (selected) last emission's totals.  KWK_ECAP when they exceed the reservation:
 * nothing was written (words unchanged) — reserve more and emit the same list again */
kwk_status kwk_emit_result(kwk_emitter* em, uint32_t* n_items, uint64_t* n_bytes);
/* kwk_emit_result plus the number of items emitted on the device (status KWK_EMIT_OK) */
kwk_status kwk_emit_stats(kwk_emitter* em, uint32_t* n_items, uint32_t* n_emitted, uint64_t* n_bytes);
/* device outputs of the last emission: items, n_items + 1 byte offsets, the bytes */
kwk_status kwk_emit_device(kwk_emitter* em, const kwk_emit_item** items, const uint64_t** offsets, const char** bytes);
/* copy them to host memory (sizes from kwk_emit_result; offsets holds n_items + 1 entries) */
kwk_status kwk_emit_copy(kwk_emitter* em, kwk_emit_item* items, uint64_t* offsets, char* bytes);
/* HIP events around the last kwk_emit's kernels (bench timing): milliseconds between them */
kwk_status kwk_emit_elapsed(kwk_emitter* em, float* ms);

/* ---- Finalizer patches (DESIGN.md §5 "Finalizer patches"): Next.Finalizers' JSON patch of every
 * fired object (pkg/utils/lifecycle/next.go:43-60, finalizersModify, finalizers.go:83-111), which
 * playStage sends before the object's delete or merge patches — byte-equal to
 * kwk_patch_finalizers (kwok_patch.h) of the same stage and list.
 *
 * State: one order word per slot (kwok_patch.h: bits 4k..4k+3 the dictionary id of list position
 * k < 7, 15 = a value outside the dictionary; bits 28-31 the length 0..7, or 0xF = more than 7
 * entries, not representable), set by the host at ingest and after every kwk_upsert /
 * kwk_replace round trip (kwk_patch_finalizer_word), as it sets the guard words.  A fired record
 * whose stage has KWK_NEXT_FIN and whose ops are not empty gives one item: `[` + the ops joined by
 * `,` + `]`; its word becomes the list after the ops (0xF when that is longer than 7); a fired
 * KWK_NEXT_DELETE stage leaves word 0 after its item (the harness re-creates the object without
 * finalizers).  A word of 0xF (or a slot beyond the capacity) on a KWK_NEXT_FIN stage gives an
 * item with KWK_EMIT_HOST and no bytes, the word kept: the host renders it and sets the word.
 * The word's update does not depend on where the record's merge-patch items were rendered.
 *
 * The finalizer items are a stream of their own beside the merge-patch items of the same output
 * set; the merge-patch outputs are what they are without a finalizer program.  The overflow
 * protocol is the sets': an emission whose finalizer totals exceed kwk_emit_reserve_fin's room
 * writes nothing — neither stream, neither word array — raises the in-flight flag, and every
 * reader of it and of the emissions behind it returns KWK_ECAP; a merge-patch overflow leaves the
 * order words alone in the same way. */
typedef struct {
  uint32_t n_values;              /* dictionary values, <= 15 */
  uint32_t n_stages;              /* the emit program's */
  const uint32_t* value_off;      /* n_values + 1: value i is values[value_off[i] .. value_off[i + 1]) */
  const char* values;             /* bytes of [A-Za-z0-9._/-] */
  const uint8_t* stage_flags;     /* n_stages: KWK_NEXT_DELETE | _FIN | _FIN_EMPTY | _FIN_REMOVE */
  const uint16_t* stage_remove;   /* n_stages: bit id = the stage removes value id */
  const uint32_t* stage_add_ptr;  /* n_stages + 1 */
  const uint8_t* stage_add;       /* ids in the Stage's order, duplicates kept; at most 16 per stage */
} kwk_emit_fin_program;

typedef struct {
  uint32_t rec;      /* index in the fired list */
  uint8_t status;    /* KWK_EMIT_* */
  uint8_t n_ops;
  uint16_t reserved;
} kwk_emit_fin_item;

/* after it, every kwk_emit / kwk_emit_step also emits the finalizer patches of its list (once per
 * emitter; the order words start at 0: no finalizers).  A program none of whose stages has
 * KWK_NEXT_FIN launches nothing: its stream is empty and the words stay as the host set them */
kwk_status kwk_emit_finalizers_load(kwk_emitter* em, const kwk_emit_fin_program* prog);
kwk_status kwk_emit_set_fin_words(kwk_emitter* em, uint32_t first, uint32_t n, const uint32_t* words);
kwk_status kwk_emit_get_fin_words(kwk_emitter* em, uint32_t first, uint32_t n, uint32_t* words);
/* room for the finalizer items and bytes of one emission, in every output set (synchronises; clears
 * the in-flight flag as kwk_emit_reserve does).  A set keeps the room it has: a smaller reservation
 * applies only to the sets made afterwards (kwk_emit_reserve_sets with another number of sets) */
kwk_status kwk_emit_reserve_fin(kwk_emitter* em, uint32_t max_items, uint64_t max_bytes);
/* the selected emission's finalizer stream (kwk_emit_select): totals (KWK_ECAP exactly when
 * kwk_emit_result returns it), device outputs, host copies (offsets: n_items + 1 entries).  With
 * KWK_ECAP the totals are the room to reserve only when the finalizer stream itself was too large
 * (kwk_emit_last_error names kwk_emit_reserve_fin); for an emission whose merge patches overflowed,
 * or that stood down behind an earlier one, they mean nothing (0 where the stream was not sized) */
kwk_status kwk_emit_fin_result(kwk_emitter* em, uint32_t* n_items, uint64_t* n_bytes);
kwk_status kwk_emit_fin_device(kwk_emitter* em, const kwk_emit_fin_item** items, const uint64_t** offsets,
                               const char** bytes);
kwk_status kwk_emit_fin_copy(kwk_emitter* em, kwk_emit_fin_item* items, uint64_t* offsets, char* bytes);

#ifdef __cplusplus
}
#endif

#endif
