/*
 * pimemb_rows.h -- C ABI of the row writer (libpimemb_rows.so), the WRITE half of the storage formats of pimemb.h:
 * fp32 rows in, the table's own bytes out, encoded on the GPU, in place, in stream order with the lookups.
 *
 * A companion library, not part of libpimemb.so: it carries its own gfx950 code object and reaches tables only through the
 * public ABI of pimemb.h (emb_table_info, emb_table_hot_count, emb_device_of, emb_device_alloc, ...).  libpimemb.so's code
 * object -- to whose kernel machine code the committed profiles are tied -- is the same with or without it.  Link with
 * -lpimemb_rows -lpimemb.  All functions are `extern "C"`; plain pointers and sizes only.
 *
 * What an update is.  emb_rows_update(w, table, ids, n, src) is the sequential loop
 *     for p in 0 .. n-1:  if row p is good:  W[ids[p]] = encode(src[p])
 * run on the GPU: where an id occurs more than once its LAST good occurrence wins, and no stored row is ever a mix of two
 * sources.  The table keeps its address and shape, so prepared plans and XCD maps over it stay valid and simply read the new
 * rows when launched behind the update.
 *
 * Encoding (EMB_ROWS_SRC_F32).  The stored bytes are bit for bit what the host encoders of the Python package write
 * (formats.py), special values included:
 *   EMB_F32      the source bits
 *   EMB_F16      IEEE nearest-even, overflow to +-inf, a NaN keeps its sign and the upper ten payload bits (a payload that
 *                lies wholly below them becomes payload 1: a NaN stays a NaN) -- numpy's astype(float16)
 *   EMB_BF16     nearest-even; a NaN keeps sign and upper payload and gets the quiet bit -- formats.to_bf16_bits
 *   EMB_F8_E4M3  nearest-even; whatever rounds beyond 448, infinities included, is NaN (0x7f | sign) -- formats.to_f8_bits
 *   EMB_F8_E5M2  nearest-even; beyond 57344 is +-inf (0x7c | sign), NaN is 0x7f | sign -- formats.to_f8_bits
 *   EMB_MXFP4    per block of 32: scale byte = floor(log2 amax) - 2 + 127 clamped to [0, 254]; elements to nearest, ties to
 *                the even code, saturating at +-6; a block that quantises to all zeros gets scale byte 127 and keeps its
 *                signs; the bytes between the scales and the row stride are written as zeros -- formats.to_mxfp4, over the
 *                whole stride.  A source row holding an inf or a NaN is a BAD row (the format has no encoding for it).
 *   EMB_FIXED32  EMB_ERR_UNSUPPORTED: a fixed-point table takes EMB_ROWS_SRC_TABLE_DTYPE only.
 * Every encoder is integer arithmetic on the fp32 bits (csrc/pimemb_rows_encode.h, compiled for the host too and compared
 * there with formats.py); none relies on a hardware conversion's treatment of NaNs, overflow or denormals.
 *
 * Bad rows.  A row whose id lies outside [0, nr_rows) -- a negative int64 id, an id of 2^32 or more: ids are compared at their
 * full width, never truncated -- or, for an MXFP4 table, whose fp32 source holds a non-finite value, is NOT written and is
 * counted.  The good rows of the call are written all the same.
 *
 * Speed, measured on MI355X (tools/rows_probe.py, profiles/rows/README.md; dim 128, 65 536 random rows per call, fp32 source in
 * HBM): 9 - 12 us per call with EMB_ROWS_UNIQUE_IDS (MXFP4: 15), 34 - 39 us with the duplicate pre-pass (MXFP4: 49), against
 * 3 - 10 us for a device-to-device copy of the bytes stored.  The pre-pass is the larger part of a default call: promise unique
 * ids where you can.  Filling a whole [4 M, 128] table from host fp32 rows takes 0.10 - 0.11 s for every dtype -- 8x - 83x faster
 * than encoding on the host for fp16 ... MXFP4, but 2.8x SLOWER than emb_load_table for an fp32 table, which needs no encoding.
 *
 * Threading.  A writer owns one scratch area: calls on one writer must not overlap -- issue them from one thread and on one
 * stream (or order the streams yourself).  Updates must not run concurrently with table management on the engine
 * (emb_alloc_table / emb_load_* / emb_set_hot_rows).  emb_rows_last_error() is thread-local.
 */
#ifndef PIMEMB_ROWS_H
#define PIMEMB_ROWS_H

#include <stddef.h>
#include <stdint.h>

#include "pimemb.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct emb_rows emb_rows; /* opaque: a writer = device scratch (id hash, counters) + a pinned staging buffer */

/* what `src` holds */
typedef enum emb_rows_src {
    EMB_ROWS_SRC_F32 = 0,        /* float[n_rows][dim], encoded on the GPU into the table's dtype */
    EMB_ROWS_SRC_TABLE_DTYPE = 1 /* n_rows rows of the table's own row stride in bytes (dim * element size; MXFP4:
                                    EMB_MXFP4_ROW_STRIDE(dim)), already encoded: a plain row scatter */
} emb_rows_src;

/* emb_rows_update flags */
#define EMB_ROWS_UNIQUE_IDS 1u /* the caller's promise that no id occurs twice in the call: the duplicate pre-pass is skipped.
                                  With duplicates under this flag the row that ends up stored is one of the sources, whole or
                                  -- the promise being broken -- mixed. */

/* Thread-local text of the last error a function of this header returned on this thread ("" if none).  Errors of the
 * engine's own calls made on the writer's behalf are copied here from emb_last_error(). */
const char *emb_rows_last_error(void);

/* Bytes of DEVICE memory emb_rows_create(e, max_rows_per_call) allocates: the id hash of the duplicate pre-pass -- open
 * addressing, pow2ceil(2 * max_rows_per_call) slots (at least 64) of a 64-bit key and a 32-bit winner position each -- plus
 * 256 bytes of counters.  A pure function, monotone in its argument. */
uint64_t emb_rows_scratch_bytes(uint64_t max_rows_per_call);
/* Bytes of PINNED HOST memory the writer allocates besides, for host-pointer calls: two halves that are filled and consumed
 * in turn; 520 bytes per row of max_rows_per_call, at least 256 KiB, at most 64 MiB.  Pure and monotone as well. */
uint64_t emb_rows_stage_bytes(uint64_t max_rows_per_call);

/* A writer for tables of engine `e`, for calls of up to max_rows_per_call rows (1 .. 2^31 - 1).  All memory a call uses
 * is allocated here, once. */
int emb_rows_create(emb_engine *e, uint64_t max_rows_per_call, emb_rows **out);
/* Waits for the device, then frees the writer.  Destroy writers before emb_destroy of their engine. */
int emb_rows_destroy(emb_rows *w);

/* Write n_rows rows into table `table_id`.
 *   row_ids   uint32[n_rows] or int64[n_rows] (itype), in `space`
 *   src       see emb_rows_src, in the same `space`; 16-byte aligned for rows of 16-byte multiples up to 1 KiB of table bytes
 *             and for every MXFP4 table (any pointer of the host path is fine: rows are staged), 4-byte aligned otherwise
 *   flags     0 or EMB_ROWS_UNIQUE_IDS; unknown bits are EMB_ERR_INVALID
 *   stream    a hipStream_t (NULL = the default stream)
 * EMB_MEM_DEVICE: a pure enqueue on `stream` -- hash clear, duplicate pre-pass, write kernel; no allocation, no copy to or
 *   from the host, no host wait -- so it orders against lookups on that stream like any other launch.  n_rows above the
 *   writer's max_rows_per_call is EMB_ERR_INVALID.  Bad rows are added to the writer's counter (emb_rows_report); n_bad must
 *   be NULL or is set to 0.  Returns EMB_OK when everything was enqueued.
 * EMB_MEM_HOST: synchronous.  ids and rows travel through the writer's pinned buffer in chunks of at most max_rows_per_call
 *   rows, in order, so last-wins holds across chunks as well; n_rows is unlimited.  Returns EMB_ERR_RANGE with *n_bad (may be
 *   NULL) = the number of bad rows if there were any -- after the good rows were written -- else EMB_OK.
 * Kernels: rows of 16-byte multiples up to 1 KiB run the lane-group write kernel (one row per lane group, one 16-byte
 * vector store per lane); MXFP4 rows a lane-group kernel of their own (four lanes per 32-element block, amax by cross-lane
 * shuffles); any other width of the non-MX dtypes an element-wise kernel.
 * EMB_ERR_UNSUPPORTED: the table has a hot set staged (emb_table_hot_count != 0) -- a hot set is a COPY of rows taken when it
 *   was set, lookups would go on serving the old bytes: clear the set (emb_set_hot_rows(e, t, NULL, 0)), update, set it again;
 *   or an fp32 source for an EMB_FIXED32 table. */
int emb_rows_update(emb_rows *w, uint32_t table_id, const void *row_ids, emb_index_type itype, uint64_t n_rows,
                    const void *src, emb_rows_src src_kind, emb_memspace space, uint32_t flags, void *stream,
                    uint64_t *n_bad /* host, may be NULL */);

/* The number of rows skipped (bad) by DEVICE-pointer calls since the last report; resets the count.  Waits for the device
 * first, so the count covers every update enqueued so far. */
int emb_rows_report(emb_rows *w, uint64_t *n_bad);

#ifdef __cplusplus
}
#endif
#endif /* PIMEMB_ROWS_H */
