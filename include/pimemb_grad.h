/*
 * pimemb_grad.h -- C ABI of the backward pass (libpimemb_grad.so): from the gradient of a pooled lookup's output to the
 * sparse gradient of the table, or straight to new table rows by a fused SGD, Adagrad or row-wise Adagrad step -- on the GPU,
 * in stream order with the lookups and the row writer, every sum in a fixed order: results are the same bits on every run.
 *
 * A companion library like libpimemb_rows.so, not part of libpimemb.so: it carries its own gfx950 code object and reaches tables
 * only through the public ABI of pimemb.h (emb_table_info, emb_table_hot_count, emb_device_of, emb_device_alloc, ...), so
 * libpimemb.so's and libpimemb_rows.so's code objects are the same with or without it.  Link with -lpimemb_grad -lpimemb.  All
 * functions are `extern "C"`; plain pointers and sizes only.
 *
 * THE DEFINITION (tests/grad_ref.py restates it as a loop; the kernels are compared with that, bit for bit).
 * One table of nr_rows x dim and a batch as the forward takes it (emb_lookup_desc's conventions): indices[n] (uint32 or int64),
 * offsets[B] (the last bag ends at n; offsets == NULL with fixed_pooling = L means offsets[b] = b * L), the forward's
 * emb_pool_spec, and G, the gradient of the pooled output: fp32 [B, dim] with a row stride of grad_ld >= dim floats (the
 * [B, T*dim] buffer of a strided lookup is read in place: grad = buffer + column, grad_ld = T*dim).
 *   Position to bag.  Position p belongs to bag(p), the LAST b with offsets[b] <= p; positions before offsets[0] belong to no
 *     bag and are skipped.  Offsets are trusted to be the ones the forward accepted (non-decreasing, <= n); whatever they
 *     hold, no access leaves [0, n), [0, B) or the table.
 *   Good positions.  A position is good if it has a bag, its id -- compared at full width, never truncated -- lies in
 *     [0, nr_rows), and (EMB_POOL_PADDING) its id is not padding_idx.  A position that has a bag and an id outside the table
 *     is BAD: skipped and counted (emb_grad_report).  Padding positions are skipped and not counted.
 *   Contribution c_p of a good position, dim fp32 values, every operation rounded on its own, never contracted into an FMA:
 *       sum, no weights          c_p = G[bag(p)]
 *       sum, per_sample_weights  c_p = w[p] * G[bag(p)]                    one fp32 multiply
 *       mean                     c_p = G[bag(p)] / (float)cnt(bag(p))      an IEEE fp32 division; cnt = the number of non-padding
 *                                positions of the bag, good or bad: what the forward divided by.  (A bag with cnt 0 has no good
 *                                position and contributes nothing.)
 *   Row gradient.  For a row r with good positions p1 < p2 < ... < pk:  g[r] = (((+0.0f + c_p1) + c_p2) + ...) + c_pk, fp32
 *     additions IN POSITION ORDER.  That order is the point: float atomics would give sums that depend on scheduling.
 *   Unique list U: the rows with at least one good position, ascending.
 * Two results:
 *   emb_grad_sparse   rows_out[|U|] (int64, ascending), grads_out[|U|, dim] (fp32) and |U| -- what nn.EmbeddingBag(sparse=True)
 *                     leaves in weight.grad after .coalesce().  It depends on the table's SHAPE only: every table dtype but
 *                     EMB_FIXED32 (EMB_ERR_UNSUPPORTED: a fixed-point table is not a floating-point parameter).
 *   emb_grad_sgd      for every r in U:  W[r] = enc(dec(W[r]) - (lr * g[r])), in place; every other row keeps its bytes.  dec is
 *                     the exact widening to fp32, lr * g one fp32 multiply, the subtraction one fp32 subtract, enc the encoder
 *                     of the row writer for the table's dtype (identity, fp16 nearest-even with overflow to inf, bf16
 *                     nearest-even: csrc/pimemb_rows_encode.h; the one-element step is csrc/pimemb_grad_step.h).  g is never
 *                     written to memory.  Tables: EMB_F32, EMB_F16, EMB_BF16.
 * EMB_ERR_UNSUPPORTED for the step, on purpose:
 *   EMB_F8_E4M3 / EMB_F8_E5M2 / EMB_MXFP4   an SGD step in the stored precision mostly rounds away (two or three mantissa bits,
 *                     one for MXFP4), and an MXFP4 block shares one scale: a step on one element would re-quantise its 31
 *                     neighbours.  Keep fp32 master rows, take emb_grad_sparse, and write rows with emb_rows_update -- or
 *                     run all of that as one fused call: emb_grad_master_step (THE MASTER-WEIGHT STEPS, below).
 *   EMB_FIXED32       not a floating-point parameter.
 *   a hot set staged (emb_table_hot_count != 0)   as in the row writer: a hot set is a COPY of rows, lookups would go on serving
 *                     the old bytes: clear the set, step, set it again.
 *   EMB_POOL_MAX      needs the forward's per-element argmax, which no kernel records.
 * Prepared plans stay valid over a stepped table and read the new rows when launched behind the step.
 * emb_grad_step (below) is the same step with an optimizer that keeps state: Adagrad, and row-wise Adagrad.
 * emb_grad_weights (THE GRADIENT OF PER_SAMPLE_WEIGHTS, below) is the other gradient of a weighted sum: one value per position.
 * Out of scope: max mode; optimizers other than SGD, Adagrad and row-wise
 * Adagrad (no momentum, no Adam), weight decay and lr_decay, optimizer state in anything but fp32; row-wise Adagrad off the
 * lane-group shape (the element-wise kernel has no row-wide view of g, and a second reduction is not built for it:
 * EMB_ERR_UNSUPPORTED); a multi-table emb_grad_sparse (it stays single; emb_grad_sgd_multi / emb_grad_step_multi below fuse the
 * steps of several tables); fusing descriptors of different dim, or of the element-wise shape, into one launch (they run on
 * their own, as before); splitting long runs IN THE POSITION ORDER (there a row that occurs thousands of times is one chain walked
 * by one lane group, in the multi-table step as well: a context of EMB_GRAD_ORDER_SEGMENTED, below, sums such a row in parallel, in
 * a second order that is as fixed as this one -- it is opt-in per context and nothing chooses it for the caller); a third level
 * of that order; the ranged / sharded paths; NaN ordering and payloads, as everywhere in this library.
 *
 * How it runs.  A pre-pass gives every position its bag (binary search in offsets), flags it good / bad / padding, counts cnt
 * per bag for mean, and orders the positions by (row id, position): a stable LSD radix sort over the ceil(log2(nr_rows + 1)) id
 * bits, 8 bits a pass (positions that are not good sort behind every row).  The heads of the runs of equal ids are the unique
 * rows; for emb_grad_sparse a scan of the head flags compacts them.  Then ONE LANE GROUP PER UNIQUE ROW walks its run in position order:
 * each lane owns 4 consecutive fp32 elements and loads 16 bytes of G per occurrence, eight occurrences in flight before the
 * first add, the adds in order -- the forward's gather turned round.  emb_grad_sgd ends the same kernel with decode /
 * multiply / subtract / encode and one vector store of the lane's piece of the table row (16 bytes fp32, 8 bytes fp16 / bf16).
 * Lane-group path: dim % 4 == 0, dim <= 512, grad (and grads_out) 16-byte aligned, grad_ld % 4 == 0; anything else runs an
 * element-wise kernel (one thread per element of a unique row).
 * emb_grad_sgd and emb_grad_step run that chain once per descriptor.  emb_grad_sgd_multi and emb_grad_step_multi run it once per
 * GROUP of up to 16 descriptors (the rules are at emb_grad_multi_groups): one classify launch over the concatenated positions
 * of the group, ONE sort over the composite key (descriptor, row) = key_base[k] + id, key_base being the running sum of the
 * group's nr_rows, and one launch of the hot kernel, in which a lane group finds its descriptor from the key of its run.  The
 * sort is stable and the positions are concatenated in descriptor order, so every (descriptor, row) run is in position order
 * and never merges with another table's: a row's sum is the one of the definition, and the tables and states end with the
 * bytes the per-descriptor calls leave.  The descriptor records travel as kernel arguments: no copy, no allocation.
 *
 * Speed, measured on MI355X (tools/grad_probe.py, profiles/grad/README.md; one emb_grad_sgd of 2048 bags x 32 indices, dim 128, 4 M
 * rows, device pointers).  Uniform ids: 72 us per step on fp32 and bf16 tables, against 73 / 106 us for torch's sparse
 * EmbeddingBag backward + SGD step: level, and 1.5x faster.  The Kaggle shape (dim 16, 39 292 one-index bags): 49 against 56 us.
 * Zipf ids, one row occurring 9 035 times: 3.7 ms, 14x SLOWER than torch (260 us) -- that row's sum is one chain of 9 035 ordered
 * additions walked by one lane group, eight loads in flight at a time; splitting it would change the bits.  A step is 12 - 18x
 * the forward lookup of the same batch (3 - 6 us), and with short runs 63 - 87 % of it is the pre-pass: 13 small launches.
 * A context of EMB_GRAD_ORDER_SEGMENTED (below; profiles/grad_segmented/README.md, medians of five alternating rounds) takes that
 * Zipf step in 134 us at S = 64: 28x faster than the position order, 1.9x faster than torch; the 26 Criteo-Kaggle tables (runs of
 * 13 114) by the multi-table step in 0.50 ms against 13.9 ms, 2.2x faster than torch.  Where no run is longer than S it pays for its
 * extra launch: 83 against 72 us on the uniform shape (SLOWER than the position order by 15 %), 52 against 49 us on the Kaggle one.
 *
 * Threading.  A context owns one scratch area: calls on one context must not overlap -- issue them from one thread and on one
 * stream (or order the streams yourself).  Steps must not run concurrently with table management on the engine
 * (emb_alloc_table / emb_load_* / emb_set_hot_rows).  emb_grad_last_error() is thread-local.
 */
#ifndef PIMEMB_GRAD_H
#define PIMEMB_GRAD_H

#include <stddef.h>
#include <stdint.h>

#include "pimemb.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct emb_grad emb_grad; /* opaque: a context = device scratch (sort buffers, bag of every position, counters) */

/* One table's share of a backward call: an emb_lookup_desc without `pooled`, plus the gradient and the forward's pooling. */
typedef struct emb_grad_desc {
    uint32_t table_id;
    uint32_t fixed_pooling; /* offsets == NULL: offsets[b] = b * fixed_pooling (> 0) */
    const void *indices;    /* uint32[n_indices] or int64[n_indices] */
    const void *offsets;    /* uint32[n_bags] or int64[n_bags] (same width as indices), or NULL */
    uint64_t n_indices;
    uint64_t n_bags;
    const float *grad;      /* G: float, row b at grad + b * grad_ld */
    uint64_t grad_ld;       /* >= dim, in floats */
    emb_pool_spec pool;     /* the forward's: mode EMB_POOL_SUM / EMB_POOL_MEAN, per_sample_weights (SUM only) or NULL, flags 0 or
                               EMB_POOL_PADDING with padding_idx in [0, nr_rows); other flag bits are EMB_ERR_INVALID */
} emb_grad_desc;

/* Thread-local text of the last error a function of this header returned on this thread ("" if none). */
const char *emb_grad_last_error(void);

/* Bytes of DEVICE memory emb_grad_create(e, max_indices, max_bags) allocates: per index two (key, position) pairs of the
 * sort, its bag and its unique-row number (24 bytes), the sort's digit counts (256 per 1024 indices) and their partial sums, 4
 * bytes per bag, 256 bytes of counters; every piece rounded up to 256 bytes.  A pure function, monotone in both arguments. */
uint64_t emb_grad_scratch_bytes(uint64_t max_indices, uint64_t max_bags);

/* A context for tables of engine `e`, for calls of up to max_indices indices (1 .. 2^30) and max_bags bags (1 .. 2^31 - 1).  All
 * memory a call uses is allocated here, once.  Its sums follow the position order. */
int emb_grad_create(emb_engine *e, uint64_t max_indices, uint64_t max_bags, emb_grad **out);

/* THE SEGMENTED ORDER: a second, equally fixed order of additions, which long runs can be summed in in parallel.  It is a property
 * of the context, chosen when it is created; the position order stays the default, and a context of one order never gives the
 * other's bits.  tests/grad_seg_ref.py restates it as a loop; the kernels are compared with that, bit for bit.
 *   EMB_GRAD_ORDER_SEGMENTED with segment length S, a power of two, 8 <= S <= 1024.  For a row r with good positions
 *   p1 < p2 < ... < pk and the contributions c_p defined at the top, let m = ceil(k / S):
 *       t_j  = (((+0.0f + c_p[jS+1]) + c_p[jS+2]) + ...) + c_p[min((j+1)S, k)]      j = 0 .. m-1: position order inside a segment
 *       g[r] = ((t_0 + t_1) + t_2) + ... + t_(m-1)                                   segment order, starting FROM t_0
 *   Every addition is rounded on its own; nothing is contracted into an FMA.
 * Segments are counted by a position's ordinal within ITS OWN ROW'S run, never by its place in the sorted batch: g[r] depends on
 * that row's occurrences alone -- not on the rest of the batch, and not on which tables share a group of a multi-table call, whose
 * tables and states therefore still end with the bytes of the per-descriptor calls.
 * For k <= S + 1 the result is bit-identical to the position order: t_0 is the old chain, and a last segment of one element adds
 * that element itself (+0 + c differs from c for c = -0 only, and t_0 + (+0) = t_0 + (-0): a chain that starts from +0 is never
 * -0).  Everything else is unchanged: U, good / bad / padding positions, dec, enc, the SGD, Adagrad and row-wise Adagrad steps, the
 * row-wise pair tree, every refusal, the bad-position count.  Every call on a segmented context follows the order:
 * emb_grad_sparse, emb_grad_sgd, emb_grad_step and the two _multi calls, on the lane-group kernels and on the element-wise one.
 * How it runs.  Behind the sort one more launch, one lane group per sorted place, sums every segment of every run longer than S
 * in position order -- the run walk bounded to S occurrences, live only where a segment starts -- and stores t_j in 16-byte pieces
 * into the context's partial buffer; the hot kernels' segmented twins then read t_0, t_1, ... of such a run, eight independent
 * loads in flight, and add them in segment order.  A run of up to S occurrences is walked as before.  A segment's slot in the
 * buffer follows from its first sorted place alone (csrc/pimemb_grad_segments.h: at most two segments of long runs start in any
 * S-aligned block of places, and then the second is a run head: 2 * ceil(n / S) slots, no scan).  The element-wise kernel folds
 * the segments of a run in one thread, a nested loop: the same bits, no buffer, and no gain in speed.
 * Out of scope: a third level (a row with k occurrences still ends in one chain of ceil(k / S) partials: 2^20 occurrences at S = 64
 * are 16 384 dependent additions); choosing the order or S from the batch. */
typedef enum { EMB_GRAD_ORDER_POSITION = 0, EMB_GRAD_ORDER_SEGMENTED = 1 } emb_grad_order;
typedef struct emb_grad_config {
    uint32_t order;    /* an emb_grad_order */
    uint32_t segment;  /* SEGMENTED: S, a power of two in 8 .. 1024; POSITION: 0 */
    uint32_t max_dim;  /* SEGMENTED: the largest dim of a table a call may name, 1 or more (the engine sets no upper limit on a
                          table's dim, so none is set here); POSITION: 0 */
    uint32_t reserved; /* 0 */
} emb_grad_config;

/* Bytes of DEVICE memory emb_grad_create_ex allocates.  EMB_GRAD_ORDER_POSITION: emb_grad_scratch_bytes(max_indices, max_bags).
 * EMB_GRAD_ORDER_SEGMENTED adds the partial buffer: 2 * ceil(max_indices / S) slots of ceil(min(max_dim, 512) / 4) pieces of 16
 * bytes (512: the widest row of the lane-group kernels; wider tables run element-wise and use no buffer), rounded up to 256 bytes.
 * A pure function, monotone in max_indices, max_bags and max_dim; 0 for a config emb_grad_create_ex refuses. */
uint64_t emb_grad_scratch_bytes_ex(uint64_t max_indices, uint64_t max_bags, const emb_grad_config *cfg);

/* emb_grad_create with the order of additions chosen; with EMB_GRAD_ORDER_POSITION it IS emb_grad_create.  EMB_ERR_INVALID for a
 * NULL config, an unknown order, a segment that is no power of two in 8 .. 1024, max_dim 0, reserved != 0, and segment or max_dim
 * other than 0 with EMB_GRAD_ORDER_POSITION -- checked before the engine is looked at.  On a segmented context a descriptor whose
 * table has dim > max_dim is EMB_ERR_INVALID, found with the other checks, before anything is enqueued. */
int emb_grad_create_ex(emb_engine *e, uint64_t max_indices, uint64_t max_bags, const emb_grad_config *cfg, emb_grad **out);
/* The config the context was created with (emb_grad_create: EMB_GRAD_ORDER_POSITION, zeros). */
int emb_grad_config_of(const emb_grad *g, emb_grad_config *out);
/* Waits for the device, then frees the context.  Destroy contexts before emb_destroy of their engine. */
int emb_grad_destroy(emb_grad *g);

/* The sparse gradient of desc->table_id.  DEVICE pointers only, all of them: indices, offsets, weights, grad, and
 *   rows_out      int64[capacity]
 *   grads_out     float[capacity][dim], no padding between rows
 *   capacity      rows the two hold; less than desc->n_indices is EMB_ERR_INVALID (|U| <= n_indices always fits)
 *   n_unique_dev  a DEVICE uint64_t that receives |U|
 * A pure enqueue on `stream` (a hipStream_t, NULL = the default stream): no allocation, no copy to or from the host, no host
 * wait.  n_indices above the context's max_indices, or n_bags above its max_bags, is EMB_ERR_INVALID; n_indices == 0 is EMB_OK
 * with |U| = 0.  Rows and gradients beyond |U| are left as they were.  Tables of 2^32 - 1 rows or more are EMB_ERR_UNSUPPORTED. */
int emb_grad_sparse(emb_grad *g, const emb_grad_desc *desc, emb_index_type itype, int64_t *rows_out, float *grads_out,
                    uint64_t capacity, uint64_t *n_unique_dev, void *stream);

/* The fused SGD step, descriptor after descriptor (a table named twice is stepped twice, in order).  DEVICE pointers only; a
 * pure enqueue like emb_grad_sparse.  Every descriptor is checked before anything is enqueued: a refused call leaves every
 * table as it was.  That holds for the one refusal that depends on the batch's size too: more than 2^31 - 1 workgroups of the
 * element-wise kernel (n_indices * dim / 256) is EMB_ERR_UNSUPPORTED, found after every descriptor has passed the other checks. */
int emb_grad_sgd(emb_grad *g, const emb_grad_desc *descs, uint32_t n_descs, emb_index_type itype, float lr, void *stream);

/* THE ADAGRAD STEPS (tests/optim_ref.py restates them as loops; the kernels are compared with that, bit for bit).  g[r], U, good /
 * bad / padding positions, dec and enc are the ones defined at the top.  Every fp32 operation below is rounded on its own and
 * never contracted into an FMA; division and square root are the IEEE correctly rounded ones (csrc/pimemb_grad_optim.h: the
 * one-element arithmetic, compiled by the kernels and by a host check alike).  The optimizer state S is fp32 whatever the table's
 * dtype, lives in a buffer of the caller's, and is initialised by the caller (torch's initial_accumulator_value is a fill).
 *
 * EMB_OPT_ADAGRAD: torch.optim.Adagrad on sparse gradients with lr_decay = 0 and weight_decay = 0.  S is float[nr_rows][dim], no
 * padding.  For every r in U and every element d:
 *       q     = g[r][d] * g[r][d]
 *       S'    = S[r][d] + q
 *       den   = sqrt(S') + eps
 *       x     = g[r][d] / den
 *       W'[r][d] = enc(dec(W[r][d]) - (lr * x))          S[r][d] = S'
 *
 * EMB_OPT_ROWWISE_ADAGRAD: the FBGEMM / DLRM "exact row-wise" form, one accumulator per row.  S is float[nr_rows].  For every r in U:
 *       sq[d] = g[r][d] * g[r][d]                         d < dim;  sq[d] = +0 for dim <= d < 4 * pieces
 *       t[c]  = ((sq[4c] + sq[4c+1]) + sq[4c+2]) + sq[4c+3]     c < pieces = dim / 4
 *       v     = t, padded with +0 to L = min(64, pow2ceil(pieces)) entries;
 *               where pieces > 64:  v[l] = t[l] + t[l + 64]  for l + 64 < pieces
 *       while len(v) > 1:  v = [v[0] + v[1], v[2] + v[3], ...]       (adjacent pairs, level by level)
 *       m     = v[0] / (float)dim
 *       S'    = S[r] + m
 *       step  = lr / (sqrt(S') + eps)                     (one division per row)
 *       W'[r][d] = enc(dec(W[r][d]) - (step * g[r][d]))   S[r] = S'
 *   The tree is stated over dim alone.  It is the xor butterfly v[l] += v[l ^ h] for h = 1, 2, 4, ... over the lane group that
 *   already owns the row, in which lane l holds pieces l and l + 64; IEEE addition commutes, so every lane ends with the same bits
 *   and applies `step` to its own pieces.  S[r] is stored by one lane, with a plain vector store.
 * Rows outside U keep their table bytes and their state bytes.  g is never written to memory.  NaN payloads are unspecified.
 * How the row-wise tail runs: the lanes of a group that own no piece (dim 48: 12 pieces in 16 lanes) stay in the kernel, hold +0 and
 * take part in every shuffle; the shuffles come after the run walk, where a group's lanes are together again, with xor distances
 * below the group's size only; beyond dim 256 a lane keeps two accumulators (it walks the run once per piece and holds both sums:
 * the ISA shows no scratch), since the whole row's g is needed before the first table store. */
typedef enum { EMB_OPT_ADAGRAD = 1, EMB_OPT_ROWWISE_ADAGRAD = 2 } emb_opt_kind;
typedef struct emb_opt_spec {
    uint32_t kind;     /* an emb_opt_kind */
    float lr;
    float eps;         /* >= 0 */
    uint32_t reserved; /* 0 */
} emb_opt_spec;

/* Floats of optimizer state a table of nr_rows x dim needs: nr_rows * dim (EMB_OPT_ADAGRAD), nr_rows (EMB_OPT_ROWWISE_ADAGRAD);
 * 0 for an unknown kind.  A pure function. */
uint64_t emb_opt_state_floats(uint32_t kind, uint64_t nr_rows, uint32_t dim);

/* The fused Adagrad / row-wise Adagrad step, descriptor after descriptor, as emb_grad_sgd: DEVICE pointers only, a pure enqueue.
 * states[k] is a caller-owned DEVICE buffer of emb_opt_state_floats(opt->kind, nr_rows, dim) floats for descs[k]'s table, read and
 * written in place.  Every descriptor and every state is checked before anything is enqueued: a refused call leaves every table
 * and every state as it was.  Refused as emb_grad_sgd refuses (fp8 / MXFP4 / fixed-point tables, a hot set staged, EMB_POOL_MAX,
 * the context's limits), and EMB_ERR_INVALID for: a NULL or not 4-byte aligned state where n_indices > 0, an unknown kind,
 * reserved != 0, eps negative or NaN.
 * EMB_OPT_ROWWISE_ADAGRAD needs the lane-group shape -- dim % 4 == 0, dim <= 512, grad 16-byte aligned, grad_ld % 4 == 0 -- and is
 * EMB_ERR_UNSUPPORTED otherwise.  EMB_OPT_ADAGRAD runs on both kernels: the lane-group one where that shape holds and the state
 * is 16-byte aligned as well, the element-wise one otherwise, with the same bits. */
int emb_grad_step(emb_grad *g, const emb_grad_desc *descs, float *const *states, uint32_t n_descs, emb_index_type itype,
                  const emb_opt_spec *opt, void *stream);

/* THE MULTI-TABLE STEPS: emb_grad_sgd / emb_grad_step with one pre-pass and one launch of the hot kernel per GROUP of descriptors
 * instead of per descriptor.  Same arguments, checks, refusals and error texts; every descriptor and every state is checked before
 * anything is enqueued; DEVICE pointers only; a pure enqueue on `stream` (no allocation, no copy to or from the host, no host
 * wait: the records of a group are kernel arguments); the bad-position count is the same.  Every table and every state ends with
 * exactly the bytes emb_grad_sgd / emb_grad_step leave over the same descriptors.
 *
 * Groups.  Descriptors are taken in order; a group is a maximal run of consecutive descriptors -- empty ones (n_indices == 0) are
 * skipped and do not end a run -- for which all of this holds:
 *   1. each has the lane-group shape (dim % 4 == 0, dim <= 512, grad 16-byte aligned, grad_ld % 4 == 0; for EMB_OPT_ADAGRAD the
 *      state 16-byte aligned as well);
 *   2. all have the same dim;
 *   3. no table_id occurs twice (a table named twice is stepped twice, in order: the second naming opens a new group);
 *   4. at most EMB_GRAD_MULTI_MAX descriptors;
 *   5. the sum of n_indices <= the context's max_indices, the sum of n_bags <= its max_bags (the scratch area is the one
 *      emb_grad_scratch_bytes states: a group is laid out in it like one descriptor of that many positions and bags);
 *   6. the sum of nr_rows <= 2^32 - 2: the composite keys and the one key behind them fit in uint32.
 * A group of one descriptor runs the single-table chain of emb_grad_sgd / emb_grad_step, the element-wise kernel included: a call
 * that cannot be fused is exactly that call.  A descriptor that exceeds the context on its own is EMB_ERR_INVALID, as there. */
#define EMB_GRAD_MULTI_MAX 16

typedef struct emb_grad_multi_shape { /* what the grouping looks at: one descriptor and its table */
    uint32_t table_id;
    uint32_t dim;
    uint32_t lane_group; /* 1: rule 1 holds, 0: it does not */
    uint64_t nr_rows;    /* (8-byte aligned: four bytes of padding before it) */
    uint64_t n_indices;
    uint64_t n_bags;
} emb_grad_multi_shape;

/* How a multi-table call over `shapes` would be split in a context of max_indices / max_bags: group_of[k] (n entries, may be NULL)
 * receives the number of descriptor k's group, counted from 0 in order, 0xffffffff for an empty descriptor; returns the number of
 * groups.  A pure host function, no GPU -- and the very function the two calls below split by. */
uint32_t emb_grad_multi_groups(const emb_grad_multi_shape *shapes, uint32_t n, uint64_t max_indices, uint64_t max_bags, uint32_t *group_of);

int emb_grad_sgd_multi(emb_grad *g, const emb_grad_desc *descs, uint32_t n_descs, emb_index_type itype, float lr, void *stream);
int emb_grad_step_multi(emb_grad *g, const emb_grad_desc *descs, float *const *states, uint32_t n_descs, emb_index_type itype,
                        const emb_opt_spec *opt, void *stream);

/* THE GRADIENT OF PER_SAMPLE_WEIGHTS (tests/psw_ref.py restates it as a loop over positions; the kernels are compared with that, bit
 * for bit).  The second gradient of nn.EmbeddingBag(mode="sum", per_sample_weights=w): one fp32 value per position of the batch,
 *       dw[p] = < G[bag(p)] , dec(W[ids[p]]) >
 * Batch, bags, good / bad / padding / no-bag positions, dec, and G with its grad_ld are the ones defined at the top; the table is
 * nr_rows x dim, any dim >= 1.  For a GOOD position p, with b = bag(p), r = ids[p] and pieces = ceil(dim / 4):
 *       prod[d] = G[b][d] * dec(W[r][d])      d < dim: one fp32 multiply;   prod[d] = +0 for dim <= d < 4 * pieces
 *       t[c]    = ((prod[4c] + prod[4c+1]) + prod[4c+2]) + prod[4c+3]                    c < pieces
 *       v       = t, padded with +0 to L = min(64, pow2ceil(pieces)) entries;
 *                 where pieces > 64:  v[l] = ((t[l] + t[l+64]) + t[l+128]) + ...  over all l + 64j < pieces, j ascending
 *       while len(v) > 1:  v = [v[0] + v[1], v[2] + v[3], ...]
 *       dw[p]   = v[0]
 * Every operation is rounded on its own and never contracted into an FMA (csrc/pimemb_grad_dot.h: the one-element arithmetic and the
 * serial form of the tree, compiled by the kernels and by a host check alike).  For dim % 4 == 0, dim <= 512 this is the pair tree
 * of the row-wise Adagrad step above (tests/optim_ref.pair_tree), over products instead of squares.  The +0 padding is part of the
 * definition: absent slots hold +0 and are added -- for G[b] all -0 and W[r] positive, dw[p] is -0 at dim 4 and dim 64 and +0 at
 * dim 48 and dim 3.
 * For a position that is NOT good (padding, no bag, or an id outside the table) dw[p] = +0.0f.  A bad position is counted for
 * emb_grad_report, as in every other call: a backward that runs both this call and a step counts it twice.  Entries of dw at and
 * beyond n_indices are not touched.  dw does not depend on the VALUES of per_sample_weights: pool.per_sample_weights may be NULL or
 * not and is never read.  It does not depend on the context's order of additions either: a segmented context gives the same bits.
 * NaN payloads are unspecified, as everywhere.
 *
 * emb_grad_weights runs descriptor after descriptor; dw_out[k] is a DEVICE float[descs[k].n_indices].  DEVICE pointers only; a pure
 * enqueue on `stream` like the steps -- no allocation, no copy, no host wait: it can be captured in a graph.  ONE launch per
 * non-empty descriptor and no pre-pass; of the context's scratch it uses the bad-position counter alone (the context is there for
 * the device, the limits and the report).  Every descriptor is checked before anything is enqueued: a refused call writes nothing.
 *   EMB_ERR_INVALID      a NULL context, descs or dw_out; a NULL (or not 4-byte aligned) dw_out[k] where n_indices > 0; n_indices or
 *                        n_bags above the context's limits; unknown pool flag bits; a padding_idx outside the table.
 *   EMB_ERR_UNSUPPORTED  a mode other than EMB_POOL_SUM (torch has no weights in mean or max mode either); EMB_F8_* / EMB_MXFP4 /
 *                        EMB_FIXED32 tables (dec knows fp32 / fp16 / bf16); tables of 2^32 - 1 rows or more.
 * A staged hot set does NOT refuse: the call only reads the table's own bytes, which are authoritative.  Issued before a fused
 * step on the same stream it reads the rows the forward read.
 * How it runs.  Lane-group shape (dim % 4 == 0, dim <= 512, grad 16-byte aligned, grad_ld % 4 == 0): one lane group per BAG, the
 * forward's geometry -- bag(p) needs no search; lane l loads its pieces l and l + 64 of G[b] once, walks the bag's positions with the
 * row gathers of eight of them in flight before the first multiply (the positions of a bag are independent here; the ids of the
 * next eight are loaded meanwhile), decodes, multiplies, folds t, and sums over the group with the row-wise step's xor butterfly,
 * the eight positions' butterflies side by side (lanes without a piece hold +0 and take part); one lane stores dw[p].  The group of bag 0 also writes the +0 of the positions before offsets[0].  Any other shape: one
 * lane group per position, its bag by binary search, scalar element loads, the same tree and the same bits.
 * Speed, measured on MI355X (tools/psw_probe.py, profiles/psw/README.md; medians of five alternating rounds, device pointers): dim 128,
 * 2048 bags x 32, 4 M rows: 13.0 us on fp32 and 14.6 us on bf16 tables with uniform ids, 11.4 / 14.0 us with Zipf ids -- 3.3x faster
 * than torch's GPU backward of the weights (42.5 us, host-bound and spread widely; none exists for bfloat16) and 2.2 - 2.6x SLOWER
 * than the forward lookup of the same batch (4.7 - 6.1 us), the floor.  The Kaggle shape (dim 16, 39 292 one-index bags): 5.6 us
 * against torch's 43.2 and the forward's 4.9.  The fallback kernel is not measured.
 * Out of scope: fusing several descriptors into one launch (one launch per table: 26 launches for the Criteo-Kaggle set); fp8 /
 * MXFP4 / fixed-point tables; mean and max mode; the ranged / sharded paths; a second-order gradient. */
int emb_grad_weights(emb_grad *g, const emb_grad_desc *descs, float *const *dw_out, uint32_t n_descs, emb_index_type itype,
                     void *stream);

/* THE MASTER-WEIGHT STEPS: mixed-precision training with fp32 master rows, fused (tests/master_ref.py restates them as a loop; the
 * kernels are compared with that, bit for bit).  This is the recipe above -- fp32 master rows, emb_grad_sparse, two torch ops,
 * emb_rows_update -- in ONE pure enqueue, and the only step that trains EMB_F8_E4M3, EMB_F8_E5M2 and EMB_MXFP4 tables; for EMB_F16 and
 * EMB_BF16 tables it keeps the updates that the in-place step loses below half an ulp of the stored value.
 * g[r], U, good / bad / padding positions, the order of additions (position or segmented, as the context was created) and the
 * bad-position count are the ones defined at the top.  M is float[nr_rows][dim], no padding, caller-owned, in device memory.
 * For every r in U and every element d, every fp32 operation rounded on its own and never contracted into an FMA:
 *   EMB_MASTER_SGD               M'[r][d] = M[r][d] - (lr * g[r][d])        one fp32 multiply, one fp32 subtract: step_f32 of
 *                                csrc/pimemb_grad_step.h on the master element
 *   EMB_MASTER_ADAGRAD           q = g * g;  S' = S[r][d] + q;  den = sqrt(S') + eps;  x = g / den;  M'[r][d] = M[r][d] - (lr * x);
 *                                S[r][d] = S'           (EMB_OPT_ADAGRAD with dec(W[r][d]) replaced by M[r][d])
 *   EMB_MASTER_ROWWISE_ADAGRAD   sq, t, v, m, S' and step as EMB_OPT_ROWWISE_ADAGRAD (the same pair tree over dim);
 *                                M'[r][d] = M[r][d] - (step * g[r][d]);  S[r] = S'
 *   S is fp32 as in emb_grad_step: float[nr_rows][dim], or float[nr_rows] row-wise.  M' -- the value enc would have taken -- is stored to M.
 *   Table row                    W[r] = enc_T(M'[r]), enc_T the row writer's encoder of the table's dtype, bit for bit what formats.py
 *                                writes: enc_f16 / enc_bf16 / enc_e4m3 / enc_e5m2 of csrc/pimemb_rows_encode.h element by element; for
 *                                EMB_MXFP4 per block of 32 mx_scale_of over the block's amax, mx_code_of per element, scale 127 for a block
 *                                that quantises to zeros, the scale bytes and the zero padding where pimemb.h puts them
 *                                (csrc/pimemb_grad_master.h: the one-block arithmetic, compiled by the kernels and by a host check alike).
 * The table row is NOT READ: the master is authoritative.  Keeping W == enc_T(M) outside the steps is the caller's job:
 * emb_rows_update of fp32 rows together with a copy of the same rows into M does it.
 * EMB_MXFP4 rows that cannot be encoded: a row whose M'[r] holds an inf or a NaN anywhere keeps its table bytes, as in the row
 * writer; M'[r] (and S) are stored all the same, and the row is counted in a counter of its own (emb_grad_master_report).  For the
 * other dtypes every value has an encoding and the row is written (an inf is fp16 / e5m2 inf and e4m3 0x7f | sign).
 * Rows outside U keep their table, master and state bytes.  g is never written to memory.
 *
 * emb_grad_master_step runs descriptor after descriptor (a table named twice is stepped twice, in order): DEVICE pointers only;
 * masters[k] is the master of descs[k]'s table, states[k] its state (states may be NULL for EMB_MASTER_SGD); every descriptor, master
 * and state is checked before anything is enqueued -- a refused call leaves everything as it was; no allocation, no copy, no host
 * wait: it can be captured in a graph.  It works on a context of either order.
 *   Tables               EMB_F16, EMB_BF16, EMB_F8_E4M3, EMB_F8_E5M2, EMB_MXFP4.  EMB_F32 is EMB_ERR_UNSUPPORTED: the table is its own
 *                        master, use emb_grad_sgd / emb_grad_step.  EMB_FIXED32, EMB_POOL_MAX, a staged hot set and the context's
 *                        limits refuse as in emb_grad_step.
 *   EMB_ERR_INVALID      a NULL or not 4-byte aligned master where n_indices > 0; a state likewise where the kind needs one; an unknown
 *                        kind; reserved != 0; eps negative or NaN (checked before the context is looked at).
 *   Kernel shape         the lane-group kernel runs where dim % 4 == 0, dim <= 512, grad AND MASTER 16-byte aligned, grad_ld % 4 == 0
 *                        (EMB_MASTER_ADAGRAD: the state too).  Off that shape the 2-byte and 1-byte dtypes run an element-wise kernel
 *                        with EMB_MASTER_SGD and EMB_MASTER_ADAGRAD, the same bits; EMB_MASTER_ROWWISE_ADAGRAD and EMB_MXFP4 are
 *                        EMB_ERR_UNSUPPORTED there (no row-wide and no block-wide view).  EMB_MXFP4 beyond dim 512: EMB_ERR_UNSUPPORTED.
 * How the tail runs.  A lane owns 4 elements per piece: one 16-byte load of M, the step, one 16-byte store of M', one 8-byte (fp16 /
 * bf16) or 4-byte (fp8) store of the encoded piece -- adjacent lanes write adjacent bytes.  MXFP4: eight adjacent lanes hold a block;
 * its amax (integer max of the magnitude bits: order-free) and the zeros rule by an xor butterfly over distances 1, 2 and 4, a lane's
 * four codes packed into 16 bits, the block's 16 bytes and the row's scale piece (dim <= 512: at most 16 scale bytes, exactly one
 * 16-byte tail piece with its padding) assembled with shuffles and stored by one lane per block and by lane 0; the row's inf / NaN flag
 * is reduced over the group before the first table store, so -- as in the row-wise step -- every lane of a run-head group stays
 * through the shuffles, lanes without a piece hold +0, and beyond dim 256 a lane keeps both pieces' sums.
 * The kernels of these steps have a code object of their own, libpimemb_grad_master.so, built from the same source and found next to
 * libpimemb_grad.so, which links against it: libpimemb_grad.so's own code object holds exactly the kernels it held before.
 * The unencodable count lives in the second word of the context's 256-byte counter block: emb_grad_scratch_bytes(_ex) are unchanged.
 * Speed, measured on MI355X (tools/master_probe.py, profiles/master/README.md; SGD, medians of five alternating rounds, device
 * pointers; dim 128, 2048 bags x 32, 4 M rows).  Uniform ids: 75 / 76 / 90 us on bf16 / e4m3 / MXFP4 tables against 177 / 176 / 192 us
 * for the no-wait recipe (fill, emb_grad_sparse, the torch ops, emb_rows_update): 2.1 - 2.4x faster; 1.05x SLOWER than the in-place
 * bf16 emb_grad_sgd (71.5 us) -- the price of the master's extra 8 bytes per element.  Zipf ids, S = 64 context: 137 / 137 / 142 us
 * against 388 / 311 / 398 (2.3 - 2.8x faster; level with the in-place step, 136 us); position-order context: 4.0 ms either way, the
 * hot row's chain (1.04 - 1.06x faster than the recipe, 1.07x SLOWER than in place).  The Kaggle shape (dim 16, 39 292 one-index
 * bags): 50 / 52 us on bf16 / e4m3 against 106 / 107.  The MXFP4 tail is 1.19x the e4m3 step on the uniform shape.
 * Out of scope: a multi-table master step (the group record has no room for the master pointer, and the multi-table kernels keep
 * their text); masters in anything but fp32; the ranged / sharded paths. */
typedef enum { EMB_MASTER_SGD = 0, EMB_MASTER_ADAGRAD = 1, EMB_MASTER_ROWWISE_ADAGRAD = 2 } emb_master_kind;
typedef struct emb_master_spec {
    uint32_t kind;     /* an emb_master_kind */
    float lr;
    float eps;         /* >= 0; not used by EMB_MASTER_SGD */
    uint32_t reserved; /* 0 */
} emb_master_spec;

int emb_grad_master_step(emb_grad *g, const emb_grad_desc *descs, float *const *masters, float *const *states, uint32_t n_descs,
                         emb_index_type itype, const emb_master_spec *spec, void *stream);

/* THE STOCHASTICALLY ROUNDED STEPS: emb_grad_sgd / emb_grad_step on EMB_F16 and EMB_BF16 tables with the LAST rounding alone replaced
 * (tests/sr_ref.py restates them as a loop; the kernels are compared with that, bit for bit).  The in-place step rounds to nearest
 * even and so loses every update below half an ulp of the stored value, every time (a bf16 weight at 1.0 never moves under steps of
 * 2^-12); the master-weight steps keep them at the price of an fp32 master, 4 more bytes per element.  Here the stored table itself is
 * an unbiased accumulator and no master exists.
 * g[r], U, good / bad / padding positions, the order of additions of the context, dec, the fp32 arithmetic of the SGD / Adagrad /
 * row-wise Adagrad steps, the state S (fp32, exact as before) and the bad-position count are unchanged.  Where the in-place step stores
 * enc_T(x), x being the fp32 value dec(W[r][d]) - (...), these steps store enc_sr_T(x, R), R a 32-bit word, T fp16 or bf16.
 *
 * enc_sr_T(x, R) (csrc/pimemb_grad_sr.h: the arithmetic, compiled by the kernels and by a host check alike):
 *   x NaN or +-inf             enc_T(x), the row writer's encoder; R is not used.
 *   fp16 and |x| >= 65536      +-inf, as enc_f16 overflows.
 *   otherwise                  lo = the T value of x's sign nearest to x with |lo| <= |x| (truncation toward zero; -0 stays -0);
 *                              hi = the next T value away from zero: +-inf beyond the largest finite one, which for the fraction
 *                              counts as 2^128 (bf16) or 65536 (fp16);
 *                              f = (|x| - |lo|) / (|hi| - |lo|) in [0, 1);  F = floor(f * 2^32);
 *                              the result is hi if F + R >= 2^32, else lo.
 *   Exactly F of the 2^32 words round away from zero; a representable x (F = 0) is stored as itself for every R.
 *   On the bits, u the fp32 pattern:
 *     bf16                     F = (u & 0xffff) << 16; the result is (u >> 16) + (F + R >= 2^32): the carry runs into the exponent and
 *                              can give inf (0x7f80), never a NaN.
 *     fp16, biased exponent e >= 113    F = (u & 0x1fff) << 19; on carry add 0x2000 to u; clear the low 13 bits: enc_f16 of that is
 *                              exact, or inf.
 *     fp16, below 2^-14        spacing 2^-24: with e' = max(e, 1), m the 24-bit significand (implicit one for e >= 1), s = 126 - e':
 *                              lo = m >> s (0 for s >= 24); F = (m mod 2^s) << (32 - s) for s <= 32, (m mod 2^s) >> (s - 32) beyond
 *                              (0 from s = 56); the result is the fp16 subnormal (or 2^-14) of magnitude lo + carry.
 *                              For s > 32 this TRUNCATES a fraction finer than 2^-32: the one place where P(hi) is not exactly f (it is
 *                              below f by less than 2^-32).
 * The word R: Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC 2011: multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 /
 *   0xBB67AE85, ten rounds) with key (seed_lo, seed_hi) and counter (r, d div 4, t_lo, t_hi) -- r the row, d the element, t the step
 *   number -- and R its output word d mod 4.  A lane that owns 4 consecutive elements runs Philox once per piece; the element-wise
 *   kernel runs it per element and picks its word: the same bits.
 * The step number: descriptor k of a call uses t = spec.step + (step_dev ? *step_dev : 0) + k, mod 2^64; empty descriptors keep their
 *   k.  A table named twice in one call draws different words for its two steps; the caller advances `step` by n_descs per call.
 *   step_dev is NULL or a DEVICE uint64_t the kernels read when they run: a captured graph replays with new words when the caller
 *   advances it on the stream.  R depends on nothing else: not on the batch, the launch geometry, the order of additions, or which
 *   kernel shape ran -- a stochastic step gives the same bits on every run, like every other call here.
 *
 * emb_grad_sgd_sr / emb_grad_step_sr are emb_grad_sgd / emb_grad_step in every other respect: DEVICE pointers only; a pure enqueue (no
 * allocation, no copy, no host wait: capturable); every descriptor and state checked before anything is enqueued; a context of either
 * order; EMB_OPT_ADAGRAD on both kernel shapes, EMB_OPT_ROWWISE_ADAGRAD on the lane-group shape only; the same refusals (fp8 / MXFP4 /
 * fixed-point tables, a hot set staged, EMB_POOL_MAX, the context's limits, eps, an unknown kind).
 *   Tables               EMB_F16 and EMB_BF16.  EMB_F32 is EMB_ERR_UNSUPPORTED: an fp32 step stores its fp32 result, there is nothing to
 *                        round -- use emb_grad_sgd / emb_grad_step.
 *   EMB_ERR_INVALID      a NULL sr, reserved != 0, a step_dev that is not 8-byte aligned (checked before the context is looked at).
 * The kernels (grad_sr_rows_group, grad_sr_rows_elem: three kinds, two orders) have a code object of their own, libpimemb_grad_sr.so,
 * built from the same source and found next to libpimemb_grad.so, which links against it; the other libraries' code objects hold the
 * machine code they held.  The tail is one Philox block -- about sixty integer operations -- per 16 bytes stepped.
 * Bytes moved per stepped element: 2 + 2 in place, 2 + 2 here, 4 + 4 + 2 with a master.
 * Speed, measured on MI355X (tools/sr_probe.py, profiles/sr/README.md; medians of five alternating rounds, device pointers, the in-place
 * step and emb_grad_master_step measured again in the same run; dim 128, 2048 bags x 32, 4 M rows).  Uniform ids, SGD: 72.4 us on bf16
 * and 74.4 us on fp16 tables against 71.3 / 73.4 us in place -- 1.015x SLOWER -- and against 74.1 us for the bf16 master step: 1.02x
 * faster; row-wise Adagrad 77.5 / 80.4 against 76.0 / 78.3 us in place: 1.02 - 1.03x SLOWER.  Zipf ids, S = 64 context: 134.5 / 135.7 us
 * (SGD) against 133.4 / 135.5 in place (1.01x SLOWER on bf16, level on fp16) and 136.3 with a master; position-order context: the hot
 * row's 3.7 - 4.0 ms chain either way (SGD 1.01x faster, row-wise 1.01x SLOWER than in place).  The Kaggle shape (dim 16, 39 292
 * one-index bags): 50.3 / 50.6 us against 49.4 / 50.0 in place (1.01 - 1.02x SLOWER, within the rounds' spread) and 50.2 with a master
 * (level).  No scratch and no spills; the Adagrad kernels take 66 / 71 VGPRs against 63 / 68 and lose one wave per SIMD of eight, the
 * SGD and row-wise kernels keep their occupancy (codeobj.kernel_resources).
 * Out of scope: SR in the _multi steps (the counter above makes a later multi-table form give the same bits), in the master steps and in
 * emb_rows_update; fp8 and MXFP4 in place; optimizer state in anything but fp32; other generators; the ranged / sharded paths. */
typedef struct emb_sr_spec {
    uint64_t seed;
    uint64_t step;            /* t of descriptor 0 */
    const uint64_t *step_dev; /* NULL, or a DEVICE uint64_t added to step when the kernels run */
    uint64_t reserved;        /* 0 */
} emb_sr_spec;

int emb_grad_sgd_sr(emb_grad *g, const emb_grad_desc *descs, uint32_t n_descs, emb_index_type itype, float lr, const emb_sr_spec *sr,
                    void *stream);
int emb_grad_step_sr(emb_grad *g, const emb_grad_desc *descs, float *const *states, uint32_t n_descs, emb_index_type itype,
                     const emb_opt_spec *opt, const emb_sr_spec *sr, void *stream);

/* The number of EMB_MXFP4 rows master steps left unwritten (an inf or a NaN in the new master row) since the last such report;
 * resets the count.  Waits for the device first, like emb_grad_report, whose count of bad positions is a separate one. */
int emb_grad_master_report(emb_grad *g, uint64_t *n_unencodable);

/* The number of BAD positions (an id outside the table) skipped since the last report; resets the count.  Waits for the
 * device first, so the count covers every call enqueued so far. */
int emb_grad_report(emb_grad *g, uint64_t *n_bad);

#ifdef __cplusplus
}
#endif
#endif /* PIMEMB_GRAD_H */
