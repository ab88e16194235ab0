/*
 * dlrm_hip.h — C ABI of the MI355X (gfx950) DLRM embedding + feature-interaction hot path.
 *
 * This is the drop-in boundary for darchr/DLRM.jl.  Every entry point replaces one operator
 * of the reference's hot path (citations are /root/reference paths):
 *
 *   dlrm_maplookup        EmbeddingTables.maplookup(PreallocationStrategy(P), tables, sparse)
 *                         called at src/model/model.jl:161; semantics pinned by
 *                         test/model/embedding_update.jl:23-33, test/model/interact.jl:168-171,
 *                         test/integration.jl:10-11 (the package itself is un-vendored).
 *   dlrm_interact_fwd     (dot::DotInteraction)(x, ys)           src/model/interact.jl:394-411
 *                         = fast_vcat (:271-281) + process_batches (:449-467)
 *                           + process_slice! (:338-362) + triangular_slice_kernel! (:64-75)
 *   dlrm_interact_bwd     dot_back / process_batches_back        src/model/interact.jl:415-489
 *                         (fused unpack :154-173, gemmavx! :318-326, sumavx :329-336)
 *   dlrm_indexer_*        EmbeddingTables.SparseIndexer()        src/train/train.jl:276-281
 *   dlrm_triangular_slice(_back), dlrm_self_batched_mul(_back)
 *                         Implementation 2 of the interaction (dot_interaction, the default of
 *                         dlrm(), model.jl:180): src/model/interact.jl:176-215, :503-551
 *   dlrm_sgd_update       EmbeddingTables.update!(Descent(lr), tables, grads, indexers;
 *                         num_splits, nthreads)                  src/train/train.jl:283-290
 *                         (grads = maplookup pullback = SparseEmbeddingUpdate views of dt,
 *                         test/train/backprop.jl:147-158, src/validation.jl:125-146)
 *
 * Conventions
 *  - All tensors are caller-owned DEVICE memory (from dlrm_malloc, hipMalloc or torch).
 *    Nothing on a launch path allocates or synchronises, so every launching call can be
 *    captured into a hipGraph.
 *  - Layout: a Julia column-major (D, N) matrix is C row-major [N][D].  The lookup output
 *    (P + D*T) x B is C [B][out_ld] with table t at columns out_offset + t*D; the interaction
 *    output (d + F(F-1)/2 + padding) x B is C [B][out_ld].
 *  - Indices are int32 or int64, laid out [T][batch*lookups] with a per-table stride
 *    (sample-major within a table: position p = b*lookups + k, as load_inputs reshapes them,
 *    src/data/criteo.jl:551-557).  index_base is 1 for Julia / DACLoader indices, 0 for
 *    PyTorch / HDF5 indices.
 *  - Errors: every function returns a dlrm_status (0 = OK, negative = error) and no C++
 *    exception crosses the ABI.  dlrm_last_error(ctx) describes the last failure.
 *    Out-of-range indices never fault: kernels skip them and raise a device-side flag that
 *    dlrm_check_bounds() turns into DLRM_E_INDEX (the reference throws BoundsError).
 *  - Threading: one ctx = one device + one stream; calls are asynchronous on that stream;
 *    a ctx must not be used from two host threads at once.
 */
#ifndef DLRM_HIP_H
#define DLRM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DLRM_HIP_ABI_VERSION 3

typedef enum {
    DLRM_OK = 0,
    DLRM_E_ARG = -1,         /* invalid argument (shape, null pointer, dtype)          */
    DLRM_E_HIP = -2,         /* HIP runtime error                                       */
    DLRM_E_INDEX = -3,       /* an index was outside [index_base, index_base + nrows)   */
    DLRM_E_UNSUPPORTED = -4, /* valid request this build does not implement             */
    DLRM_E_NOMEM = -5,       /* device allocation failed                                */
    DLRM_E_STATE = -6        /* object used in the wrong state (e.g. indexer not built) */
} dlrm_status;

typedef enum { DLRM_F32 = 0, DLRM_BF16 = 1 } dlrm_dtype;
typedef enum { DLRM_I32 = 0, DLRM_I64 = 1 } dlrm_itype;

/* dlrm_sgd_update flags */
#define DLRM_UPDATE_ATOMIC 1u   /* float atomics straight into the rows: fastest to launch,
                                   NOT bitwise reproducible (fp32 tables only)            */
#define DLRM_UPDATE_PREBUILT 2u /* the indexer was already built from these indices by
                                   dlrm_indexer_build (e.g. on a side stream during the
                                   forward pass); skip rebuilding it                     */

typedef struct dlrm_ctx dlrm_ctx;         /* device + stream + error word                  */
typedef struct dlrm_tables dlrm_tables;   /* Vector{SimpleEmbedding{Static{D}}} on device  */
typedef struct dlrm_indexer dlrm_indexer; /* Vector{SparseIndexer}: per-table dedupe state */

/* ---- context ---------------------------------------------------------------------- */
int dlrm_abi_version(void);
int dlrm_ctx_create(int device, void* stream /* hipStream_t, NULL = default */, dlrm_ctx** out);
int dlrm_ctx_destroy(dlrm_ctx* ctx);
int dlrm_ctx_set_stream(dlrm_ctx* ctx, void* stream);
const char* dlrm_last_error(const dlrm_ctx* ctx);
/* Diagnostics: on = 1 installs handlers that print a native backtrace to stderr on SIGSEGV, SIGBUS
 * or SIGABRT and then run the previous handler (0 restores them).  Not for production use. */
int dlrm_debug_fatal_trace(int on);
int dlrm_sync(dlrm_ctx* ctx);
/* Synchronises, reads and clears the device out-of-range flag raised by any kernel since
 * the previous call.  DLRM_E_INDEX if it was set. */
int dlrm_check_bounds(dlrm_ctx* ctx);
/* Bounds errors without a per-step synchronisation (the deferred update! of the drop-in chain).
 * The step backward (dlrm_step_bwd / _prepare, backward launch) copies the flag into host memory
 * owned by the ctx as it reads it (one thread's store); for other sequences
 * dlrm_error_snapshot queues a copy of the device flag into host memory owned by the ctx (on the
 * ctx stream; capturable, no synchronisation); dlrm_error_peek reads the last copy that has landed
 * (no GPU call; 0 = no error seen yet).  A kernel that finds the device flag set writes no table
 * row, so the tables keep the state before the failing step until dlrm_check_bounds reports and
 * clears the flag (it also clears the host copy). */
int dlrm_error_snapshot(dlrm_ctx* ctx);
int dlrm_error_peek(const dlrm_ctx* ctx, unsigned* word);

/* ---- device memory (so a host language without ROCm bindings can own buffers) ------- */
int dlrm_malloc(dlrm_ctx* ctx, size_t bytes, void** dptr);
int dlrm_free(dlrm_ctx* ctx, void* dptr);
int dlrm_memcpy_h2d(dlrm_ctx* ctx, void* dst, const void* src, size_t bytes); /* synchronous */
int dlrm_memcpy_d2h(dlrm_ctx* ctx, void* dst, const void* src, size_t bytes); /* synchronous */
/* Page-locks a host range for direct DMA (hipHostRegister) / releases it; dlrm_memcpy_h2d_async
 * queues a copy on the ctx stream and returns (the source must stay unchanged until the stream
 * reaches it; from registered memory the copy is a DMA with no staging). */
int dlrm_host_register(void* ptr, size_t bytes);
int dlrm_host_unregister(void* ptr);
int dlrm_memcpy_h2d_async(dlrm_ctx* ctx, void* dst, const void* src, size_t bytes);

/* ---- embedding tables --------------------------------------------------------------- */
/* Registers T tables of one dtype and feature size `dim` (SimpleEmbedding{Static{dim}}).
 * data[t] points at a device [nrows[t]][dim] row-major table.  The table memory stays
 * caller-owned; dlrm_sgd_update mutates it in place. */
int dlrm_tables_create(dlrm_ctx* ctx, int num_tables, int dim, int dtype,
                       void* const* data, const int64_t* nrows, dlrm_tables** out);
int dlrm_tables_destroy(dlrm_tables* tables);

/* maplookup(PreallocationStrategy(out_offset), tables, sparse):
 *   out[b][out_offset + t*dim + c] = sum_{k<lookups} table_t[idx_t[b*lookups + k] - base][c]
 * Columns [0, out_offset) are not touched (they are reserved for x, interact.jl:264-270).
 * lookups = 1 is the one-hot copy (bit-exact); lookups > 1 sums in k order in fp32. */
int dlrm_maplookup(dlrm_ctx* ctx, const dlrm_tables* tables,
                   const void* indices, int itype, int64_t table_stride, int index_base,
                   int batch, int lookups,
                   void* out, int64_t out_ld, int64_t out_offset);

/* dlrm_maplookup with a general output row map (the table-sharded exchange layout,
 * dlrm.jl_amd/sharded.py: every peer's block written in place, no repack):
 *   row b of table t -> out + (b / block_rows) * block_stride + (b % block_rows) * out_ld
 *                           + out_offset + t * table_stride        (elements)
 * dlrm_maplookup(...) == dlrm_maplookup_blocked(..., table_stride = dim, block_rows = batch,
 * block_stride = 0).  No reference counterpart (DLRM.jl is single-process). */
int dlrm_maplookup_blocked(dlrm_ctx* ctx, const dlrm_tables* tables,
                           const void* indices, int itype, int64_t table_stride, int index_base,
                           int batch, int lookups, void* out, int64_t out_ld, int64_t out_offset,
                           int64_t out_table_stride, int64_t block_rows, int64_t block_stride);

/* Row scatter of the exchange (sharded backward: dt's table columns -> per-owner blocks):
 *   dst + dst_base[t] + b * dst_ld[t]  <-  src + b * src_ld + src_offset + t * dim
 * for b < batch, t < num_tables, dim elements of esize (2 or 4) bytes; dst_base / dst_ld are
 * device arrays of num_tables int64 (elements).  No reference counterpart. */
int dlrm_scatter_rows(dlrm_ctx* ctx, int esize, int num_tables, int batch, int dim,
                      const void* src, int64_t src_ld, int64_t src_offset, void* dst,
                      const int64_t* dst_base, const int64_t* dst_ld);

/* ---- pairwise dot interaction -------------------------------------------------------- */
/* (dot::DotInteraction)(x, ys): copies x[b][0:d] into ys[b][0:d] (fast_vcat), views
 * ys[b][0:F*d] as T_b = [F][d], and writes
 *   out[b] = [ x_b | Z[i][j] for i = 1..F-1, j = 0..i-1 | 0 * padding ],  Z = T_b T_b^T
 * dtype applies to x, ys and out (bf16 in, fp32 accumulate, bf16 out).
 * Padding: the `padding` columns after the pairs are written as zeros (all-zero bits) by every
 * forward (this one, dlrm_lookup_interact_fwd, dlrm_step_fwd), and a row is written in columns
 * [0, d + F(F-1)/2 + padding) only: out_ld may be larger and the rest of the row keeps its bytes.
 * ys is written in columns [0, d) only.  The backwards read dout[b][0 : d + F(F-1)/2] and never its
 * padding columns.  Leading dimensions and base pointers need no alignment (rows that are not 16-B
 * aligned take slower kernels with the same results) except where an entry point says otherwise; a
 * leading dimension smaller than its row, or a negative padding, is DLRM_E_ARG and nothing is
 * launched. */
int dlrm_interact_fwd(dlrm_ctx* ctx, int dtype, int d, int num_features, int batch,
                      const void* x, int64_t x_ld, void* ys, int64_t ys_ld,
                      void* out, int64_t out_ld, int padding);

/* maplookup(PreallocationStrategy(d), tables, sparse) followed by (dot::DotInteraction)(x, ys)
 * as ONE launch (model.jl:161-163 with the bottom MLP already applied): every gathered row is
 * loaded once into MFMA fragments and written to ys from registers, so ys is never re-read.
 * ys and out receive exactly what dlrm_maplookup(out_offset = d) + dlrm_interact_fwd write
 * (bit-identical); shapes without a fused kernel fall back to those two launches.
 * ys may be NULL when the caller will not read the lookup output (a training step whose
 * backward is dlrm_interact_bwd_gather): then only out is written, and shapes without a
 * fused kernel return DLRM_E_UNSUPPORTED.  Requires tables->dim == d; dtype is the tables'. */
int dlrm_lookup_interact_fwd(dlrm_ctx* ctx, const dlrm_tables* tables,
                             const void* indices, int itype, int64_t table_stride, int index_base,
                             int batch, int lookups,
                             const void* x, int64_t x_ld, void* ys, int64_t ys_ld,
                             void* out, int64_t out_ld, int padding);

/* ---- Implementation 2 of the interaction, as separate operators --------------------------
 * dot_interaction (src/model/interact.jl:503-517; the default of dlrm(), model.jl:180) composes
 * fast_vcat + self_batched_mul + triangular_slice; dlrm_interact_fwd / dlrm_interact_bwd are that
 * composition and its pullback in one launch each.  These are the pieces and their rrules, for
 * callers that compose them as the reference does.  Layouts: Z, dZ (sz, sz, B) = [B][sz][sz]
 * (batch stride given, element [b][col][row] = Julia z[row, col, b]); the slice (ncols, B) = [B][ld];
 * T (d, F, B) = [B][F][d] (batch stride t_ld).
 * dlrm_triangular_slice       triangular_slice (:176-191): out[b][col(col-1)/2 + row] = z[b][col][row],
 *                             row < col (triangular_slice_kernel! order, :64-75).  Bit-exact copy.
 * dlrm_triangular_slice_back  its rrule (:193-215): a[b][col][row] = dy[b][col(col-1)/2 + row] for
 *                             row < col, 0 elsewhere (triangular_slice_back_kernel!, :104-120);
 *                             symmetric != 0: also the lower triangle (the fused add-transpose form,
 *                             :150-171).  Bit-exact.
 * dlrm_self_batched_mul       self_batched_mul (:526-537): z[b] = T_b^T T_b (full, F x F), fp32
 *                             accumulation, stored in dtype.  F <= 90.
 * dlrm_self_batched_mul_back  its rrule (:539-551): dt[b] = T_b (dz_b + dz_b^T), fp32 out.  F <= 90. */
int dlrm_triangular_slice(dlrm_ctx* ctx, int dtype, int sz, int batch, const void* z, int64_t z_batch_stride,
                          void* out, int64_t out_ld);
int dlrm_triangular_slice_back(dlrm_ctx* ctx, int dtype, int sz, int batch, const void* dy, int64_t dy_ld, void* a,
                               int64_t a_batch_stride, int symmetric);
int dlrm_self_batched_mul(dlrm_ctx* ctx, int dtype, int d, int num_features, int batch, const void* t, int64_t t_ld,
                          void* z, int64_t z_batch_stride);
int dlrm_self_batched_mul_back(dlrm_ctx* ctx, int dtype, int d, int num_features, int batch, const void* t,
                               int64_t t_ld, const void* dz, int64_t dz_batch_stride, float* dt, int64_t dt_ld);

/* dot_back(dot, dout, t, d, padding): S_b = symmetric zero-diagonal unpack of
 * dout[b][d : d + F(F-1)/2];  dt[b] = S_b T_b  ([F][d], fp32, x-rows included as the
 * reference returns them);  dx[b] = dout[b][0:d] + dt[b][0:d]  (fp32).
 * t is the ys buffer of the forward pass (dtype as dout). */
int dlrm_interact_bwd(dlrm_ctx* ctx, int dtype, int d, int num_features, int batch,
                      const void* dout, int64_t dout_ld, int padding,
                      const void* t, int64_t t_ld,
                      float* dx, int64_t dx_ld, float* dt, int64_t dt_ld);

/* dot_back as dlrm_interact_bwd, with T_b rebuilt from x (row 0) and the tables' rows of the
 * sample's one-hot indices (rows 1..F-1) instead of read from a materialized ys: the same
 * values while the tables are unchanged since the forward (recomputation, not a cache).
 * lookups must be 1; dtype is the tables' (dout and x in it); dx, dt fp32 as above.
 * indexer (may be NULL): also builds it from the same indices, as dlrm_indexer_build would --
 * in the same launch where the shape allows (its workgroups sort while the backward's stream),
 * so the step's dlrm_sgd_update can pass DLRM_UPDATE_PREBUILT.
 * Declared after the indexer type below; see the SparseIndexer section. */

/* ---- sparse indexer + SGD scatter update --------------------------------------------- */
int dlrm_indexer_create(dlrm_ctx* ctx, int num_tables, int64_t max_lookups_per_table,
                        dlrm_indexer** out);
int dlrm_indexer_destroy(dlrm_indexer* indexer);
/* Dedupe: per table, group the lookup positions by row -> one segment per distinct row
 * holding the positions that hit it in ascending order (segment order is unspecified).
 * Asynchronous; device-side counts only.  By batch * lookups positions per table: <= 4096 in LDS
 * (one workgroup per table); <= 8192 in LDS over 4 parts where the indexer was created for 4097..8192
 * positions, else the hash build; <= 32768 (and tables x capacity < 2^31) the bag build (count, place
 * by part, per-part sort: pooled bags, round 6; DLRM_BAG_WAVE=0 selects the hash build instead); up to
 * 2^20 the hash build; above, one workgroup per table sorting in HBM.  Up to 2^20 the build is split
 * (once-hit positions flagged, not listed; the update takes them from the flags).  Out-of-range
 * indices are left out and raise the ctx's bounds flag.  DESIGN.md section 20 has the table. */
int dlrm_indexer_build(dlrm_ctx* ctx, dlrm_indexer* indexer, const dlrm_tables* tables,
                       const void* indices, int itype, int64_t table_stride, int index_base,
                       int batch, int lookups);
/* The split form of the indexer that dlrm_step_bwd consumes (one-hot batches): positions whose
 * row is hit once are flagged (dlrm_step_bwd updates those rows inside the backward), the other
 * rows are listed for the apply.  dlrm_step_fwd builds it inside the forward's launch; building
 * it here instead lets a caller prepare the NEXT batch's indexer ahead of time (it depends only
 * on the indices, e.g. on a side stream during the current step) and run a step as
 * dlrm_lookup_interact_fwd(ys = NULL) + dlrm_step_bwd.  By batch positions per table: <= 4096 in
 * LDS; <= 32768 (and tables x capacity < 2^31) the bag build (DLRM_BAG_SPLIT=0: the forms of
 * dlrm_indexer_build without it, split); up to 2^20 the hash build; above, DLRM_E_UNSUPPORTED and the
 * indexer is left as it was.  Bounds errors go to the ctx's flag. */
int dlrm_indexer_build_split(dlrm_ctx* ctx, dlrm_indexer* indexer, const dlrm_tables* tables,
                             const void* indices, int itype, int64_t table_stride, int index_base,
                             int batch);
/* Inspection (synchronous): unique-row count of one table; if rows != NULL copies up to
 * cap unique rows (0-based, in segment order); if positions != NULL copies up to cap
 * positions (b*lookups + k) grouped by segment and the segment starts (cap+1 entries). */
int dlrm_indexer_read(dlrm_ctx* ctx, const dlrm_indexer* indexer, int table,
                      int64_t* num_unique, int64_t* rows, int64_t* positions,
                      int64_t* seg_start, int64_t cap);

/* The training step's split build of `indices` on the ctx's stream -- a side stream: it depends on
 * the indices only -- so that the dlrm_step_fwd of the same indices only gathers (the build
 * dlrm_step_bwd_prepare runs inside an apply launch, as its own launch).  One-hot, batch <= 32768
 * positions per table (16 table parts per 2048 positions, one wave each; above 2048 positions the
 * scan build: 8 or 16 waves per workgroup scan the table, int32 indices with 16-B aligned tables and
 * batch % 4 == 0, else the build in rounds), any number of tables (tables x capacity < 2^31); the
 * indexer must have been created for >= batch positions.  Replaces the SparseIndexer() build of
 * train.jl:276-281 ahead of the step (also the table-sharded update's build over the global
 * batch).  Out-of-range indices are left out of the build and raise the ctx's bounds flag through
 * the lookup / forward of the same indices, or the apply of this indexer (dlrm_sgd_update PREBUILT,
 * dlrm_step_bwd) -- not from the build itself, which may run beside a step that reads the flag to
 * decide its writes.  DLRM_E_UNSUPPORTED: a shape the wave build does not take (use
 * dlrm_indexer_build). */
int dlrm_indexer_prepare(dlrm_ctx* ctx, dlrm_indexer* indexer, const dlrm_tables* tables,
                         const void* indices, int itype, int64_t table_stride, int index_base, int batch);

/* Device bytes the indexer holds, all allocated by dlrm_indexer_create: the per-part arrays (~92 B
 * per position slot; the wave builds pack a table's parts back to back, so any of them fits cap
 * slots per table -- x 8 for a cap of 4097..8192, the in-LDS parts build's layout), the wave
 * build's flat item lists (<= 256 B per slot) and HBM sort scratch (20 B, cap > 2048), and above
 * 4096 the hash arrays.  Nothing grows on a later build (26 tables x 16384: ~0.2 GB). */
int dlrm_indexer_bytes(const dlrm_indexer* indexer, int64_t* bytes);
/* Kept for callers of round 5's layout, which re-carved the indexer on its first wave build of
 * > 2048 positions: the packed layout needs no re-carving, so this only validates batch. */
int dlrm_indexer_reserve(dlrm_ctx* ctx, dlrm_indexer* indexer, int batch);
/* The wave build's chunk limit for this indexer's later builds (16 or 32, default 32): segments of
 * at most this many positions become chunk items (one lane group each), longer ones hot-slice items
 * (a workgroup each).  16 turns the 17..32-position segments of uniform one-hot batches (the
 * 105-row Kaggle table) into one-round items (DESIGN.md §3 "Round 6").  Deterministic either way; a
 * 17..32-position segment is summed in a different (fixed) order, so its fp32 rounding may differ. */
int dlrm_indexer_set_chunk(dlrm_ctx* ctx, dlrm_indexer* indexer, int max_positions);
/* Parts per table of this indexer's later wave builds of <= 2048 positions per table (the step's
 * in-apply / forward-launch builds, dlrm_indexer_prepare): 16 (the default, 0), 32 or 64; one wave
 * sorts each part.  More parts shorten the build's chain and add workgroups beside the apply: a
 * win where the apply's items are light (rows <= 256 B: D = 16 fp32, Terabyte bf16 rows), a loss
 * at 512-B rows (DESIGN.md §3 "Round 6").  Results are identical for any setting. */
int dlrm_indexer_set_parts(dlrm_ctx* ctx, dlrm_indexer* indexer, int parts);

/* Host-side state of the last build (no GPU call): a mask of DLRM_IX_* bits.  SINGLES_DONE: a
 * split backward (dlrm_step_bwd or dlrm_split_step_bwd) has stepped this build's once-hit rows, so
 * its dt holds only the repeated rows' gradients; SINGLES_SPLIT, set with it: that backward was
 * dlrm_split_step_bwd's (the split rule on split-bf16 tables), so only the split rule's apply may
 * complete it; SINGLES_ADAGRAD / SINGLES_ROWWISE, set with it: that backward was
 * dlrm_adagrad_step_bwd's with an element-wise / a row-wise handle, and only an Adagrad apply with a
 * handle of that kind may complete it; SINGLES_STOCHASTIC, set with it: that backward was
 * dlrm_sr_step_bwd's, and only the stochastic rule's apply with the same dlrm_sr_sgd handle may
 * complete it; SINGLES_SR_ADAGRAD / SINGLES_SR_ROWWISE, set with it: that backward was
 * dlrm_sr_adagrad_step_bwd's with an element-wise / a row-wise dlrm_adagrad_create_sr handle, and
 * only that rule's apply with the same handle may complete it.  (The Julia shim's pullback state,
 * DLRMHip.jl `st.bwd`.) */
enum { DLRM_IX_BUILT = 1, DLRM_IX_SPLIT = 2, DLRM_IX_PREPARED = 4, DLRM_IX_SINGLES_DONE = 8,
       DLRM_IX_SINGLES_SPLIT = 16, DLRM_IX_SINGLES_ADAGRAD = 32, DLRM_IX_SINGLES_ROWWISE = 64,
       DLRM_IX_SINGLES_STOCHASTIC = 128, DLRM_IX_SINGLES_SR_ADAGRAD = 256, DLRM_IX_SINGLES_SR_ROWWISE = 512 };
int dlrm_indexer_state(const dlrm_indexer* indexer, unsigned* state);

/* Backward of a training step without a materialized ys (see above). */
int dlrm_interact_bwd_gather(dlrm_ctx* ctx, const dlrm_tables* tables, dlrm_indexer* indexer,
                             const void* indices, int itype, int64_t table_stride, int index_base,
                             int batch, int lookups, const void* x, int64_t x_ld,
                             const void* dout, int64_t dout_ld, int padding,
                             float* dx, int64_t dx_ld, float* dt, int64_t dt_ld);

/* dlrm_interact_bwd_gather for the table-sharded backward: dx as there, and table t's dt row of
 * sample b written straight to dst + dst_base[t] + b * dst_ld[t] (fp32; dst_base / dst_ld device
 * arrays of num_tables int64 elements, the send layout of dlrm_alltoall_bwd), i.e. the backward
 * and dlrm_scatter_rows in one launch; dt's x rows are not written.  Needs 16-B aligned rows, x,
 * dx and dst (DLRM_E_UNSUPPORTED otherwise).  No reference counterpart. */
int dlrm_interact_bwd_blocked(dlrm_ctx* ctx, const dlrm_tables* tables,
                              const void* indices, int itype, int64_t table_stride, int index_base,
                              int batch, const void* x, int64_t x_ld, const void* dout, int64_t dout_ld,
                              int padding, float* dx, int64_t dx_ld, float* dst,
                              const int64_t* dst_base, const int64_t* dst_ld);

/* update!(Descent(lr), tables, grads, indexers):
 *   table_t[r] -= lr * sum_{(b,k): idx_t[b*lookups+k] - base == r} grad[b][grad_offset + t*dim + :]
 * Default: deterministic (sum in ascending position order per unique row, one
 * read-modify-write per unique row); builds the indexer from `indices` first unless
 * DLRM_UPDATE_PREBUILT.  DLRM_UPDATE_ATOMIC ignores the indexer (may be NULL). */
int dlrm_sgd_update(dlrm_ctx* ctx, dlrm_tables* tables, dlrm_indexer* indexer, unsigned flags,
                    const void* indices, int itype, int64_t table_stride, int index_base,
                    int batch, int lookups,
                    const void* grad, int grad_dtype, int64_t grad_ld, int64_t grad_offset,
                    float lr);

/* ---- sparse Adagrad: update!(ADAGrad(lr, eps), tables, grads, indexers) and its row-wise form.
 * No reference counterpart in DLRM.jl's own training loop (it trains with Descent); the
 * reference's update! is generic over the Flux optimiser (src/model/embedding_update.jl:136).
 *
 * For a table row r touched by the batch, G[c] = sum of grad[b][grad_offset + t*dim + c] over the
 * positions that hit r, summed in fp32 in exactly the order dlrm_sgd_update uses for the same
 * indexer.  Then
 *   element-wise (rowwise = 0; Flux.ADAGrad(lr, eps); dense and sparse agree: an untouched row
 *   has G = 0):
 *       A[r][c] += G[c]^2
 *       w[r][c] -= lr * G[c] / (sqrt(A[r][c]) + eps)
 *     state: fp32 [nrows][dim] per table, caller-owned device memory; Flux initialises it to eps
 *     and so do the Python and Julia wrappers.
 *   row-wise (rowwise = 1):
 *       m[r]    += (1/dim) * sum_c G[c]^2
 *       w[r][c] -= lr * G[c] / (sqrt(m[r]) + eps)
 *     state: fp32 [nrows] per table, initialised to 0.  The sum over c runs in a fixed order per
 *     kernel path (a lane's elements in element order, then an xor butterfly over the lanes that
 *     hold the row, then the waves in wave order), so it is reproducible.
 * All arithmetic is fp32; bf16 tables are read and stored through the same conversions as
 * dlrm_sgd_update's; the state is always fp32.  Each touched row's weights and state are written
 * exactly once, untouched rows keep their bits (weights and state), and the result is bitwise
 * reproducible from run to run.  When the context's bounds flag (or a prepared build's) is set,
 * neither tables nor state are written, as in dlrm_sgd_update.
 *
 * dlrm_adagrad_create uploads the per-table state pointers once (state[t] non-NULL for every
 * table with rows; 16-B aligned pointers let the element-wise rule use the vector kernels).
 * dlrm_adagrad_update: DLRM_UPDATE_PREBUILT is honoured; DLRM_UPDATE_ATOMIC returns
 * DLRM_E_UNSUPPORTED (an atomic add cannot square a sum it never holds).  An indexer in state
 * DLRM_IX_SINGLES_DONE returns DLRM_E_STATE: a split backward has already stepped the once-hit
 * rows with Descent and its dt lacks their rows -- unless DLRM_IX_SINGLES_ADAGRAD or
 * DLRM_IX_SINGLES_ROWWISE says that dlrm_adagrad_step_bwd stepped them with a handle of this
 * handle's kind: then the repeated rows that are left are applied.  A split indexer whose singles are not done is
 * taken whole, once-hit rows included.  Launches neither allocate nor synchronise beyond what
 * dlrm_sgd_update does (partial rows for dim > 256 on first use), so the call is graph-capturable.
 * dlrm_adagrad_destroy of NULL returns 0. */
typedef struct dlrm_adagrad dlrm_adagrad; /* per-table state pointers on the device + kind */
int dlrm_adagrad_create(dlrm_ctx* ctx, const dlrm_tables* tables, int rowwise,
                        float* const* state, dlrm_adagrad** out);
int dlrm_adagrad_destroy(dlrm_adagrad* opt);
int dlrm_adagrad_update(dlrm_ctx* ctx, dlrm_tables* tables, dlrm_adagrad* opt, dlrm_indexer* indexer,
                        unsigned flags, const void* indices, int itype, int64_t table_stride,
                        int index_base, int batch, int lookups,
                        const void* grad, int grad_dtype, int64_t grad_ld, int64_t grad_offset,
                        float lr, float eps);

/* ---- sparse Adagrad with a stochastically rounded store: either rule on DLRM_BF16 tables, the
 * written weight rounded as dlrm_sr_sgd_update rounds it (below).  Round-to-nearest drops a step of
 * lr G / (sqrt(m) + eps) under half a bf16 ulp of the weight every time -- after a few hundred hits
 * of a row, every Adagrad step; the stochastic store keeps it in expectation at no memory beside the
 * rule's fp32 state.  The row-wise kind is the one that fits the largest table sets (bf16 rows plus
 * one fp32 word per row).
 *
 * dlrm_adagrad_create_sr makes a dlrm_adagrad of the stochastic kind (rowwise as in
 * dlrm_adagrad_create, the same state arrays with the same initial values) holding `seed` and one
 * 64-bit device step word, zero at creation.  dlrm_adagrad_update with it: for every touched row,
 * G, the state update and the fp32 result W' of every element are exactly what the plain handle's
 * update computes before its store converts W' (the same expressions, reduction orders and
 * hardware sqrt / rcp), the state is written with the same bits, and the element stored is
 * sr_bf16(W', R) with dlrm_sr_sgd's R, Inf / NaN handling and Philox key / counter unchanged (key =
 * the seed's halves, counter = (row, table << 16 | column >> 2, step lo, step hi), column c takes
 * the low 16 bits of word c & 3).  R depends on (seed, step, table, row, column) alone, not on the
 * indexer's form, chunk limit, parts, launch or lane.  The step word has dlrm_sr_sgd's contract:
 * every launch of a call reads one value and a one-thread launch after the call's last adds one,
 * in stream order (a captured update advances on every replay); it advances when the call returned
 * DLRM_OK and launched, also when a raised bounds flag suppressed the writes, and not on an
 * argument or state error.  dlrm_adagrad_seek / dlrm_adagrad_step set (asynchronous) and read
 * (synchronising) the word; on a handle of dlrm_adagrad_create they return DLRM_E_ARG.
 *
 * Otherwise as dlrm_adagrad_update: touched rows written once, untouched rows keep their bits
 * (weights and state), a set bounds flag leaves both unwritten, DLRM_UPDATE_PREBUILT is honoured,
 * DLRM_UPDATE_ATOMIC returns DLRM_E_UNSUPPORTED, a split indexer whose singles are not done is
 * taken whole.  fp32 tables return DLRM_E_ARG (nothing to round), at create and at update; more
 * than 65536 tables or dim / 4 > 65536 returns DLRM_E_ARG at create (the counter's fields).
 * The fused training step with these rules has entry points of its own, dlrm_sr_adagrad_step_bwd
 * (_prepare) below: dlrm_adagrad_step_bwd(_prepare) with such a handle returns
 * DLRM_E_UNSUPPORTED, and dlrm_adagrad_update(PREBUILT) with one on an indexer in state
 * DLRM_IX_SINGLES_DONE returns DLRM_E_STATE unless dlrm_sr_adagrad_step_bwd marked the build with
 * this very handle (it then applies the repeated rows); the refusals neither launch, write nor
 * move the step word. */
int dlrm_adagrad_create_sr(dlrm_ctx* ctx, const dlrm_tables* tables, int rowwise,
                           float* const* state, int64_t seed, dlrm_adagrad** out);
int dlrm_adagrad_seek(dlrm_ctx* ctx, dlrm_adagrad* opt, int64_t step);
int dlrm_adagrad_step(dlrm_ctx* ctx, dlrm_adagrad* opt, uint64_t* out);

/* ---- split-bf16 tables: update!(Descent(lr), ...) as an exact fp32 step on bf16 rows.
 * The reference names the layout (src/train/train.jl:117, `mantissa_trick`) and never builds it.
 *
 * Layout: every weight has an fp32 master value W.  The bf16 table every other entry point reads
 * (dlrm_maplookup, dlrm_step_fwd, dlrm_interact_bwd_gather, the exchange) holds the HIGH 16 bits of
 * W; a second caller-owned uint16 array per table, lo[t] of shape [nrows][dim], holds the LOW 16
 * bits.  The high half is the truncation of W, not its rounding: the forward sees W moved toward
 * zero by less than one bf16 ulp, and (hi << 16) | lo is W exactly.  A table that was bf16 all
 * along starts with zero low halves.
 *
 * For a table row r touched by the batch, G[c] is dlrm_sgd_update's fp32 gradient sum (same indexer
 * form, same order).  Then
 *     W  = bits((hi[r][c] << 16) | lo[r][c])
 *     W' = fmaf(-lr, G[c], W)
 *     hi[r][c] = bits(W') >> 16,  lo[r][c] = bits(W') & 0xffff
 * so the merged values follow dlrm_sgd_update's trajectory on fp32 tables bit for bit.  When W' is a
 * NaN the high half also gets the quiet bit (0x40), so the bf16 table alone still reads NaN.  Each
 * touched row's two halves are written exactly once, untouched rows keep their bits in both arrays,
 * the result is bitwise reproducible, and a set bounds flag (the context's, or a prepared build's)
 * leaves both arrays unwritten, as in dlrm_sgd_update.  The update moves the bytes per row of an
 * fp32 table's; the two arrays together take 4 bytes per element.
 *
 * Do not mix: dlrm_sgd_update, dlrm_adagrad_update or dlrm_step_bwd on such tables write a ROUNDED
 * bf16 step into the high half and leave the low half as it was, after which the pair no longer
 * holds the master weight.  The fused training step of these tables is dlrm_split_step_bwd (below).
 *
 * dlrm_split_sgd_create uploads the per-table low-half pointers once: tables that are not
 * DLRM_BF16, or a table with rows and lo[t] == NULL, return DLRM_E_ARG.  16-B aligned lo[t] (and
 * dim * 2 % 16 == 0) let the vector kernels run; anything else takes the any-dim kernels with the
 * same results.  dlrm_split_sgd_update: tables that are not DLRM_BF16, or an optimizer created for
 * another table count / dim, return DLRM_E_ARG; DLRM_UPDATE_ATOMIC returns DLRM_E_UNSUPPORTED;
 * DLRM_UPDATE_PREBUILT is honoured; an indexer in state DLRM_IX_SINGLES_DONE without
 * DLRM_IX_SINGLES_SPLIT returns DLRM_E_STATE (dlrm_step_bwd's backward has already written those
 * rows' high halves with a rounded bf16 step), with DLRM_IX_SINGLES_SPLIT (dlrm_split_step_bwd's
 * backward stepped them with this rule) only the repeated rows are applied, from their dt rows; a
 * split indexer whose singles are not done is taken whole, once-hit rows included.  Launches
 * neither allocate nor synchronise beyond what dlrm_sgd_update does, so the call is
 * graph-capturable.  dlrm_split_sgd_destroy of NULL returns 0. */
typedef struct dlrm_split_sgd dlrm_split_sgd; /* per-table low-half pointers on the device */
int dlrm_split_sgd_create(dlrm_ctx* ctx, const dlrm_tables* tables, uint16_t* const* lo,
                          dlrm_split_sgd** out);
int dlrm_split_sgd_destroy(dlrm_split_sgd* opt);
int dlrm_split_sgd_update(dlrm_ctx* ctx, dlrm_tables* tables, dlrm_split_sgd* opt, dlrm_indexer* indexer,
                          unsigned flags, const void* indices, int itype, int64_t table_stride,
                          int index_base, int batch, int lookups,
                          const void* grad, int grad_dtype, int64_t grad_ld, int64_t grad_offset,
                          float lr);

/* ---- stochastic rounding: update!(Descent(lr), ...) on bf16 tables, unbiased, with no memory
 * beside the table.  dlrm_sgd_update on bf16 tables rounds every written element to nearest, so a
 * step below half a bf16 ulp of the weight is dropped every time; the split tables above keep it
 * at 2 more bytes per element.  Here the fp32 result of the step is rounded up or down with
 * probability proportional to its distance to each bf16 neighbour: the stored weight equals the
 * fp32 step in expectation, and small updates accumulate instead of vanishing.
 *
 * For a table row r of table t touched by the batch, G[c] is dlrm_sgd_update's fp32 gradient sum
 * (same indexer form, same order; a once-hit row's is 0.0f + g).  Then
 *     W'      = fmaf(-lr, G[c], bf16_to_f32(w[r][c]))        (dlrm_sgd_update's expression)
 *     w[r][c] = sr_bf16(W', R)
 * sr_bf16(W', R), u = bits(W'): when u's exponent is all ones (Inf, NaN) the round-to-nearest
 * conversion of dlrm_sgd_update (a NaN keeps its quiet bit); otherwise (u + R) >> 16 with R a
 * uniform 16-bit integer.  So the magnitude rounds away from zero with probability
 * (u & 0xffff) / 65536 exactly, a W' that is a bf16 value is kept, and a finite W' above the
 * largest finite bf16 can round to Inf, its upper neighbour.
 *
 * R is a function of (seed, step, t, r, c) and of nothing else -- not of the indexer's form, its
 * chunk limit or parts per table, or of which launch or lane writes the row: Philox4x32-10 with
 * key = (seed low 32 bits, seed high 32 bits) and counter = (r as uint32, (t << 16) | (c >> 2),
 * step low 32 bits, step high 32 bits); column c takes the low 16 bits of output word c & 3.
 * Tables with more than 65536 tables or dim / 4 > 65536 return DLRM_E_ARG at create.
 *
 * The step: the handle owns one 64-bit device word, zero at creation.  Update call number k since
 * creation (or since the last seek) uses step k in every launch of the call; the word then advances
 * by one on the device, in stream order, with no host synchronisation -- so a captured update
 * advances it on every replay.  It advances when the call returned DLRM_OK and launched (also when
 * a raised bounds flag suppressed the writes), not on an argument or state error.
 * dlrm_sr_sgd_seek sets it (asynchronous, on the context's stream); dlrm_sr_sgd_step synchronises
 * the stream and reads it.  seed and step are 64 bits taken as unsigned (passed as int64_t: the
 * bit pattern is what counts).
 *
 * Each touched row is written exactly once, untouched rows keep their bits, the result is bitwise
 * reproducible for a given (seed, step), and a set bounds flag (the context's, or a prepared
 * build's) leaves the tables unwritten.  dlrm_sr_sgd_update: DLRM_UPDATE_PREBUILT is honoured;
 * DLRM_UPDATE_ATOMIC returns DLRM_E_UNSUPPORTED; tables that are not DLRM_BF16 (there is nothing
 * to round), or a handle created for another table count / dim, return DLRM_E_ARG; an indexer in
 * state DLRM_IX_SINGLES_DONE returns DLRM_E_STATE, writes nothing and leaves the step alone (another
 * rule's step backward has already written the once-hit rows rounded to nearest) -- unless
 * DLRM_IX_SINGLES_STOCHASTIC says that dlrm_sr_step_bwd stepped them with this handle, in which case
 * the repeated rows are applied (another handle's: DLRM_E_STATE); a split indexer whose
 * singles are not done is taken whole, once-hit rows included.  The rule keeps no per-row state,
 * so it may be alternated freely with dlrm_sgd_update on the same tables.  Launches neither
 * allocate nor synchronise beyond what dlrm_sgd_update does, so the call is graph-capturable.
 * dlrm_sr_sgd_destroy of NULL returns 0.  The fused training step with this rule is dlrm_sr_step_bwd
 * (below). */
typedef struct dlrm_sr_sgd dlrm_sr_sgd; /* the seed and the device step word */
int dlrm_sr_sgd_create(dlrm_ctx* ctx, const dlrm_tables* tables, int64_t seed, dlrm_sr_sgd** out);
int dlrm_sr_sgd_destroy(dlrm_sr_sgd* opt);
int dlrm_sr_sgd_update(dlrm_ctx* ctx, dlrm_tables* tables, dlrm_sr_sgd* opt, dlrm_indexer* indexer,
                       unsigned flags, const void* indices, int itype, int64_t table_stride,
                       int index_base, int batch, int lookups,
                       const void* grad, int grad_dtype, int64_t grad_ld, int64_t grad_offset,
                       float lr);
int dlrm_sr_sgd_seek(dlrm_ctx* ctx, dlrm_sr_sgd* opt, int64_t step);
int dlrm_sr_sgd_step(dlrm_ctx* ctx, dlrm_sr_sgd* opt, uint64_t* out);

/* ---- training step: fused forms of the four operators --------------------------------
 * One train! iteration of the sparse half of the model (src/train/train.jl:215-227 and
 * custom_update! :283-290) on one-hot lookups, as two launching calls with the tables
 * unchanged between them:
 *
 * dlrm_step_fwd = dlrm_lookup_interact_fwd(ys = NULL) + dlrm_indexer_build, in one launch
 *   where the shape allows (F <= 32, batch <= 2048): the indexer's workgroups sort while the
 *   gather streams.  `out` is bit-identical to dlrm_lookup_interact_fwd's.  The indexer is
 *   built in "split" form: rows hit by exactly one position of the batch are flagged for the
 *   backward instead of listed for the apply.  dlrm_sgd_update(PREBUILT) with such an indexer
 *   updates the flagged rows too -- unless dlrm_step_bwd's backward (DLRM_STEP_BWD_ONLY or flags 0)
 *   already has, in which case it updates only the repeated rows from their dt rows, so every row
 *   is stepped exactly once whichever call follows the backward.
 * dlrm_step_bwd = dlrm_interact_bwd_gather + dlrm_sgd_update(Descent(lr), PREBUILT) with that
 *   indexer.  dx is bit-identical to dlrm_interact_bwd_gather's and the tables end up
 *   bit-identical to dlrm_sgd_update's result: a once-hit row gets w = fmaf(-lr, g, w) inside
 *   the backward (no other sample reads it), so its dt row is never written or read back;
 *   dt holds only the rows the apply launch reads (x rows and rows of repeated table rows).
 *   dx and dt must be 16-B aligned with leading dimensions divisible by 4 (DLRM_E_ARG otherwise,
 *   with no table row, dx or dt written; the indexer stays valid for an aligned call).
 *   flags: 0 runs both launches; DLRM_STEP_BWD_ONLY then DLRM_STEP_APPLY_ONLY run them one at a
 *   time (e.g. the apply on another stream, or timed alone). */
#define DLRM_STEP_BWD_ONLY 1u   /* the backward launch only (dx, dt, once-hit rows)       */
#define DLRM_STEP_APPLY_ONLY 2u /* the apply of repeated rows only (reads dt)             */
int dlrm_step_fwd(dlrm_ctx* ctx, const dlrm_tables* tables, dlrm_indexer* indexer,
                  const void* indices, int itype, int64_t table_stride, int index_base, int batch,
                  const void* x, int64_t x_ld, void* out, int64_t out_ld, int padding);
int dlrm_step_bwd(dlrm_ctx* ctx, dlrm_tables* tables, dlrm_indexer* indexer,
                  const void* indices, int itype, int64_t table_stride, int index_base, int batch,
                  const void* x, int64_t x_ld, const void* dout, int64_t dout_ld, int padding,
                  float* dx, int64_t dx_ld, float* dt, int64_t dt_ld, float lr, unsigned flags);
/* Pipelined step: dlrm_step_bwd (flags 0) whose apply launch also builds the NEXT batch's split
 * indexer into next_indexer (same itype / table_stride / index_base / batch as this batch), as
 * extra workgroups of that launch; the next dlrm_step_fwd with next_indexer and next_indices then
 * only gathers (one launch without the indexer's workgroups).  Tables and results are identical to
 * the unpipelined step.  Shapes whose forward has no in-launch indexer (batch > 2048, F > 32, rows
 * not 16-B aligned) run the plain dlrm_step_bwd and leave next_indexer to the next forward.
 * next_indices must hold the next batch when the apply runs (stream order).  flags as
 * dlrm_step_bwd's (the next build rides on the DLRM_STEP_APPLY_ONLY launch).
 * Whether dlrm_step_fwd only gathers is decided on the host when it is called (the indexer holds
 * these indices, prepared): a hipGraph captured from a pipelined sequence is valid only when it is
 * replayed from the indexer state it was captured in (e.g. re-prime before each replayed run). */
int dlrm_step_bwd_prepare(dlrm_ctx* ctx, dlrm_tables* tables, dlrm_indexer* indexer,
                          const void* indices, int itype, int64_t table_stride, int index_base, int batch,
                          const void* x, int64_t x_ld, const void* dout, int64_t dout_ld, int padding,
                          float* dx, int64_t dx_ld, float* dt, int64_t dt_ld, float lr,
                          dlrm_indexer* next_indexer, const void* next_indices, unsigned flags);

/* ---- the training step on split-bf16 tables (see "split-bf16 tables" above): dlrm_step_bwd and
 * dlrm_step_bwd_prepare with the split rule in place of Descent, after the same forward
 * (dlrm_step_fwd / dlrm_lookup_interact_fwd read the high halves only).
 *   dlrm_split_step_bwd = dlrm_interact_bwd_gather + dlrm_split_sgd_update(opt, PREBUILT): dx is
 *   bit-identical to dlrm_interact_bwd_gather's and both halves of every touched row end up
 *   bit-identical to dlrm_split_sgd_update's.  A once-hit row is stepped inside the backward: its
 *   master weight is the gathered bf16 element (high half) merged with its low half,
 *   W' = fmaf(-lr, 0 + g, W), both halves stored (NaN: the quiet bit, as above); its dt row is
 *   never written.  The apply launch steps the repeated rows from their dt rows with the same rule.
 * Arguments, flags (DLRM_STEP_BWD_ONLY / DLRM_STEP_APPLY_ONLY), alignment rules and fallbacks are
 * dlrm_step_bwd's: a shape without a split backward (F > 32, x or rows not 16-B aligned, low-half
 * pointers not 16-B aligned) runs dlrm_interact_bwd_gather and lets the split apply take the
 * once-hit rows; dlrm_split_step_bwd_prepare on a shape without an in-apply build runs the plain
 * step.  Tables that are not DLRM_BF16, or an optimizer created for another table count / dim,
 * return DLRM_E_ARG.  A set bounds flag leaves both halves of every row unwritten.
 * The indexer remembers the rule that stepped its once-hit rows (DLRM_IX_SINGLES_SPLIT), and only
 * that rule completes the backward: dlrm_step_bwd(APPLY_ONLY), dlrm_sgd_update(PREBUILT) and
 * dlrm_adagrad_update(PREBUILT) after dlrm_split_step_bwd's backward return DLRM_E_STATE, and so
 * does dlrm_split_step_bwd(APPLY_ONLY) after dlrm_step_bwd's; nothing is written.
 * dlrm_split_sgd_update(PREBUILT) after dlrm_split_step_bwd(BWD_ONLY) applies the repeated rows. */
int dlrm_split_step_bwd(dlrm_ctx* ctx, dlrm_tables* tables, dlrm_split_sgd* opt, dlrm_indexer* indexer,
                        const void* indices, int itype, int64_t table_stride, int index_base, int batch,
                        const void* x, int64_t x_ld, const void* dout, int64_t dout_ld, int padding,
                        float* dx, int64_t dx_ld, float* dt, int64_t dt_ld, float lr, unsigned flags);
int dlrm_split_step_bwd_prepare(dlrm_ctx* ctx, dlrm_tables* tables, dlrm_split_sgd* opt,
                                dlrm_indexer* indexer,
                                const void* indices, int itype, int64_t table_stride, int index_base, int batch,
                                const void* x, int64_t x_ld, const void* dout, int64_t dout_ld, int padding,
                                float* dx, int64_t dx_ld, float* dt, int64_t dt_ld, float lr,
                                dlrm_indexer* next_indexer, const void* next_indices, unsigned flags);

/* ---- the training step with sparse Adagrad (see "sparse Adagrad" above): dlrm_step_bwd and
 * dlrm_step_bwd_prepare with the element-wise or the row-wise rule in place of Descent (the kind is
 * the handle's), after the same forward.
 *   dlrm_adagrad_step_bwd = dlrm_interact_bwd_gather + dlrm_adagrad_update(opt, PREBUILT): dx, the
 *   tables and the state end up bit-identical to that pair's.  A once-hit row is stepped inside the
 *   backward from its gathered elements and its state with G = 0 + g (element-wise: A += G^2,
 *   w -= lr G / (sqrt(A) + eps); row-wise: the row's sum of squares in the apply's own order -- a
 *   lane's four columns in column order, then an xor butterfly over the row's lanes --
 *   m += ss / dim, w -= lr G / (sqrt(m) + eps)); its dt row is never written.  The apply launch
 *   steps the repeated rows from their dt rows with the same rule.
 * Arguments, flags, alignment rules and argument errors are dlrm_step_bwd's and
 * dlrm_adagrad_update's.  A shape without a split backward (F > 32, x or rows not 16-B aligned),
 * element-wise state pointers that are not 16-B aligned, and a feature size whose backward has no
 * Adagrad form (dim other than 128 and not <= 64; row-wise: also any dim that is not a power of
 * two >= 8, where the apply itself sums a row's squares in column order) run
 * dlrm_interact_bwd_gather and let the rule's apply take the once-hit rows.  So do the shapes
 * whose backward form would run below dlrm_step_bwd's occupancy and is not built: the row-wise
 * rule with up to 16 features (every dim), and the element-wise rule on DLRM_F32 tables with up to
 * 16 features and dim <= 64.  dlrm_adagrad_step_bwd_prepare on a shape without an in-apply
 * build, every one of these fallback shapes included, runs the plain step (the next dlrm_step_fwd
 * then builds its indexer).  A set
 * bounds flag leaves tables and state unwritten.
 * Only the same rule completes a backward: every other pairing of dlrm_step_bwd,
 * dlrm_split_step_bwd and dlrm_adagrad_step_bwd (element-wise / row-wise handle) with another's
 * (APPLY_ONLY), or with another rule's dlrm_*_update(PREBUILT), returns DLRM_E_STATE and launches
 * nothing.  dlrm_adagrad_update(PREBUILT) with a handle of the same kind after
 * dlrm_adagrad_step_bwd(BWD_ONLY) applies the repeated rows. */
int dlrm_adagrad_step_bwd(dlrm_ctx* ctx, dlrm_tables* tables, dlrm_adagrad* opt, dlrm_indexer* indexer,
                          const void* indices, int itype, int64_t table_stride, int index_base, int batch,
                          const void* x, int64_t x_ld, const void* dout, int64_t dout_ld, int padding,
                          float* dx, int64_t dx_ld, float* dt, int64_t dt_ld, float lr, float eps,
                          unsigned flags);
int dlrm_adagrad_step_bwd_prepare(dlrm_ctx* ctx, dlrm_tables* tables, dlrm_adagrad* opt,
                                  dlrm_indexer* indexer,
                                  const void* indices, int itype, int64_t table_stride, int index_base, int batch,
                                  const void* x, int64_t x_ld, const void* dout, int64_t dout_ld, int padding,
                                  float* dx, int64_t dx_ld, float* dt, int64_t dt_ld, float lr, float eps,
                                  dlrm_indexer* next_indexer, const void* next_indices, unsigned flags);

/* ---- the training step with the stochastic rule (see "stochastically rounded SGD" above):
 * dlrm_step_bwd and dlrm_step_bwd_prepare with that rule in place of Descent on DLRM_BF16 tables,
 * after the same forward.
 *   dlrm_sr_step_bwd = dlrm_interact_bwd_gather + dlrm_sr_sgd_update(opt, PREBUILT): dx is
 *   bit-identical to dlrm_interact_bwd_gather's and every touched row ends up bit-identical to
 *   dlrm_sr_sgd_update's at the same (seed, step).  A once-hit row is stepped inside the backward:
 *   w = sr_bf16(fmaf(-lr, 0 + g, w), R) with the R of (seed, step, t, r, c) defined above, generated
 *   at the write; its dt row is never written.  The apply launch steps the repeated rows from their
 *   dt rows with the same rule.
 * The step: one training step is one value of the handle's word.  The backward launch and the apply
 * launch read the same value; the word advances by one, on the device and in stream order, after
 * the launch that runs the apply -- flags 0, DLRM_STEP_APPLY_ONLY, or dlrm_sr_sgd_update(PREBUILT)
 * completing a DLRM_STEP_BWD_ONLY backward.  DLRM_STEP_BWD_ONLY alone does not advance it.  As for
 * dlrm_sr_sgd_update it advances when the call returned DLRM_OK and launched (also under a raised
 * bounds flag, which leaves every row unwritten), not on an argument or state error; nothing
 * synchronises, and a captured step advances it on every replay.
 * Arguments, flags, alignment rules and fallbacks are dlrm_step_bwd's: a shape without a split
 * backward (F > 32, x or rows not 16-B aligned) and a feature size whose backward has no form with
 * this rule (dim other than 128 and not <= 64) run dlrm_interact_bwd_gather and let the rule's
 * apply take the once-hit rows -- the same bits, since R does not depend on the launch that writes
 * a row; dlrm_sr_step_bwd_prepare on a shape without an in-apply build, these included, runs the
 * plain step.  Tables that are not DLRM_BF16, or a handle created for another table count / dim,
 * return DLRM_E_ARG.
 * The indexer remembers the rule and the handle that stepped its once-hit rows
 * (DLRM_IX_SINGLES_STOCHASTIC), and only that handle completes the backward, through
 * dlrm_sr_step_bwd(APPLY_ONLY) or dlrm_sr_sgd_update(PREBUILT), which then applies the repeated
 * rows.  Every pairing with dlrm_step_bwd, dlrm_split_step_bwd, dlrm_adagrad_step_bwd or their
 * dlrm_*_update(PREBUILT), in either direction, another dlrm_sr_sgd handle, and a second backward
 * on one build return DLRM_E_STATE, launch nothing and leave the step alone. */
int dlrm_sr_step_bwd(dlrm_ctx* ctx, dlrm_tables* tables, dlrm_sr_sgd* opt, dlrm_indexer* indexer,
                     const void* indices, int itype, int64_t table_stride, int index_base, int batch,
                     const void* x, int64_t x_ld, const void* dout, int64_t dout_ld, int padding,
                     float* dx, int64_t dx_ld, float* dt, int64_t dt_ld, float lr, unsigned flags);
int dlrm_sr_step_bwd_prepare(dlrm_ctx* ctx, dlrm_tables* tables, dlrm_sr_sgd* opt,
                             dlrm_indexer* indexer,
                             const void* indices, int itype, int64_t table_stride, int index_base, int batch,
                             const void* x, int64_t x_ld, const void* dout, int64_t dout_ld, int padding,
                             float* dx, int64_t dx_ld, float* dt, int64_t dt_ld, float lr,
                             dlrm_indexer* next_indexer, const void* next_indices, unsigned flags);

/* ---- the training step with a sparse Adagrad rule and the stochastic store (see
 * dlrm_adagrad_create_sr above): dlrm_adagrad_step_bwd and dlrm_adagrad_step_bwd_prepare with a
 * handle of dlrm_adagrad_create_sr on DLRM_BF16 tables, after the same forward.
 *   dlrm_sr_adagrad_step_bwd = dlrm_interact_bwd_gather + dlrm_adagrad_update(opt, PREBUILT) at
 *   the same (seed, step): dx, every element of every table row and every state word or row end up
 *   bit-identical to that pair's.  A once-hit row is stepped inside the backward with
 *   dlrm_adagrad_step_bwd's arithmetic (G = 0 + g, the same reduction orders); its state is
 *   written with the seedless bits and its weights as sr_bf16(W', R), the R of (seed, step, t, r, c)
 *   generated at the write; its dt row is never written.  The apply launch steps the repeated rows
 *   from their dt rows with the same rule.
 * Arguments and flags are dlrm_adagrad_step_bwd's.  opt must come from dlrm_adagrad_create_sr: a
 * handle of dlrm_adagrad_create, tables that are not DLRM_BF16, or a handle created for another
 * table count / dim return DLRM_E_ARG, launch nothing and leave the step word alone.
 * The step word has dlrm_sr_step_bwd's contract: the backward launch and the apply launch read the
 * same value; the word advances by one, in stream order, after the launch that runs the apply --
 * flags 0, DLRM_STEP_APPLY_ONLY, or dlrm_adagrad_update(PREBUILT) completing a DLRM_STEP_BWD_ONLY
 * backward.  DLRM_STEP_BWD_ONLY alone does not advance it.  It advances when the call returned
 * DLRM_OK and launched (also under a raised bounds flag, which leaves tables and state
 * unwritten), not on an argument or state error.
 * Fallbacks are dlrm_adagrad_step_bwd's on bf16 tables: a shape without a split backward, state
 * rows that are not 16-B aligned (element-wise), dim other than 128 and not <= 64, the row-wise
 * rule with up to 16 features or a dim that is not a power of two >= 8 run
 * dlrm_interact_bwd_gather and let the rule's apply take the once-hit rows -- the same bits, since
 * R does not depend on the launch that writes a row.  _prepare on a shape without an in-apply build
 * runs the plain step.
 * The indexer remembers the rule and the handle (DLRM_IX_SINGLES_SR_ADAGRAD /
 * DLRM_IX_SINGLES_SR_ROWWISE), and only that handle completes the backward, through
 * dlrm_sr_adagrad_step_bwd(APPLY_ONLY) or dlrm_adagrad_update(PREBUILT), which then applies the
 * repeated rows.  Every pairing with another rule's step backward or update(PREBUILT), in either
 * direction, another handle of the same kind, and a second backward on one build return
 * DLRM_E_STATE, launch nothing and leave every step word alone. */
int dlrm_sr_adagrad_step_bwd(dlrm_ctx* ctx, dlrm_tables* tables, dlrm_adagrad* opt, dlrm_indexer* indexer,
                             const void* indices, int itype, int64_t table_stride, int index_base, int batch,
                             const void* x, int64_t x_ld, const void* dout, int64_t dout_ld, int padding,
                             float* dx, int64_t dx_ld, float* dt, int64_t dt_ld, float lr, float eps,
                             unsigned flags);
int dlrm_sr_adagrad_step_bwd_prepare(dlrm_ctx* ctx, dlrm_tables* tables, dlrm_adagrad* opt,
                                     dlrm_indexer* indexer,
                                     const void* indices, int itype, int64_t table_stride, int index_base, int batch,
                                     const void* x, int64_t x_ld, const void* dout, int64_t dout_ld, int padding,
                                     float* dx, int64_t dx_ld, float* dt, int64_t dt_ld, float lr, float eps,
                                     dlrm_indexer* next_indexer, const void* next_indices, unsigned flags);

/* ---- table-sharded exchange over RCCL ------------------------------------
 * DLRM.jl is one process: maplookup hands its output straight to the interaction (model.jl:161-163).
 * With the tables sharded by table over the GPUs of a node (one host process per GPU), that hand-off
 * is an all-to-all each way.  table_counts[p] = tables owned by rank p (host array, nranks entries);
 * B = samples per rank; blocks are contiguous and in owner order (exchange layout of
 * dlrm_maplookup_blocked / dlrm_scatter_rows):
 *   dlrm_alltoall_fwd: send [nranks][T_me][B][dim] (dtype) -> recv [src][T_src][B][dim]
 *   dlrm_alltoall_bwd: gsend [owner][B][T_owner][dim] (fp32) -> grecv [src][B][T_me][dim]
 *                      (= the [nranks*B][T_me*dim] gradient of this rank's tables for the global batch)
 * dlrm_comm_unique_id fills DLRM_COMM_ID_BYTES bytes on one rank; the caller hands them to every
 * rank (e.g. Julia's Distributed, MPI or a file), which calls dlrm_comm_init with its rank.  Both
 * exchanges are asynchronous on the ctx stream (RCCL group of one send + one receive per peer). */
#define DLRM_COMM_ID_BYTES 128
typedef struct dlrm_comm dlrm_comm;
int dlrm_comm_unique_id(void* id);
int dlrm_comm_init(dlrm_ctx* ctx, const void* id, int rank, int nranks, dlrm_comm** out);
int dlrm_comm_destroy(dlrm_comm* comm);
/* the rank count RCCL reports for the communicator (ncclCommCount), into *nranks */
int dlrm_comm_count(const dlrm_comm* comm, int* nranks);
int dlrm_alltoall_fwd(dlrm_ctx* ctx, dlrm_comm* comm, int dtype, int dim, int batch_local, const int* table_counts,
                      const void* send, void* recv);
int dlrm_alltoall_bwd(dlrm_ctx* ctx, dlrm_comm* comm, int dim, int batch_local, const int* table_counts,
                      const float* gsend, float* grecv);

/* ---- dense half of the training step (the GEMMs stay on hipBLASLt) --------
 * dlrm_bce_head: one launch for the top MLP's head after its last GEMM, replacing
 *   Flux.sigmoid (model.jl:83-89), bce_loss (train.jl:33-41) and rrule(bce_loss) (train.jl:43-64):
 *   prob[b] = sigmoid(logits[b * logits_ld]); *loss = mean(-y·max(log p, -100) + (y-1)·max(log(1-p), -100));
 *   dlogit[b] = (1/B)·((1-y)/(1-p+eps) - y/(p+eps)) · p(1-p);  *dbias (may be NULL) = Σ_b dlogit[b].
 *   fp32; deterministic (fixed reduction order).  batch >= 1.
 * dlrm_relu_bwd_bias: the Dense(relu) pullback seam (model.jl:72-93): g[b][:] *= (y[b][:] > 0)
 *   in place, dbias[n] = Σ_b g[b][n] (two launches: mask + 16-row column sums, then the column
 *   sums of those in chunk order).  work / counters: caller-owned scratch sized by
 *   dlrm_relu_bwd_bias_workspace (counters zeroed once by the caller; the kernel leaves them 0).
 *   n % 4 == 0, y, g 16-B aligned, leading dimensions % 4 == 0.  Deterministic. */
int dlrm_bce_head(dlrm_ctx* ctx, int batch, const float* logits, int64_t logits_ld, const float* labels,
                  float* prob, float* dlogit, float* loss, float* dbias);
int dlrm_relu_bwd_bias_workspace(int batch, int n, int64_t* work_floats, int64_t* counters);
int dlrm_relu_bwd_bias(dlrm_ctx* ctx, int batch, int n, const float* y, int64_t y_ld, float* g, int64_t g_ld,
                       float* dbias, float* work, unsigned* counters);

/* ---- evaluation (the reference's `test`, src/train/utils.jl:31-46, plus log loss and AUC) ----
 * dlrm_eval_layout: *bins = 130049, *shift = 13, *words = 8 + 2·bins: the size of a state in 8-byte words.
 * dlrm_eval_accumulate: folds one batch of scores and labels into `state`, caller-owned device memory of
 *   `words` words, 8-B aligned.  One launch, no allocation, no synchronisation, hipGraph-capturable.  Reset is
 *   the caller's memset to zero, reading is the caller's copy, and two states merge by integer addition of
 *   words 0-4 and the histogram (loss_sum by a double addition).
 *     word 0 total      1 correct      2 positives (labels == 1.0f)      3 negatives (labels == 0.0f)
 *          4 batches (calls)      5 loss_sum (IEEE double bits)
 *          6 the last call's mean loss (float bits in the low half)      7 zero
 *          8 + c·bins + k   hist[c][k], u64; class c = 0 negatives, 1 positives
 *   Per sample b < batch: p = scores[b·scores_ld] if is_prob, else 1/(1 + exp(-scores[b·scores_ld])) with
 *   dlrm_bce_head's expression (the same bits); prob[b] = p (prob may be NULL).  The sample is correct iff
 *   rintf(p) == labels[b] (round.(predictions) .== labels: ties to even, so p = 0.5 predicts 0; a soft label or
 *   a NaN is never correct).  Its loss term is dlrm_bce_head's, summed over the batch in dlrm_bce_head's order
 *   into a float L: loss_sum += (double)L, word 6 = L·(1.0f/batch).  hist[c][float_bits(min(max(p, 0), 1)) >> shift]
 *   is incremented for a label of exactly 0 or 1 (a NaN p: bin 0): positive float bits order as their values
 *   do, so the histogram ranks the scores truncated to 10 mantissa bits (the AUC's input).
 *   Integer atomics only: every word is reproducible.  Calls on one stream serialise; concurrent calls on one
 *   state from two streams are undefined.  batch >= 1, scores_ld >= 1. */
int dlrm_eval_layout(int* bins, int* shift, int64_t* words);
int dlrm_eval_accumulate(dlrm_ctx* ctx, int64_t* state, int batch, const float* scores, int64_t scores_ld, int is_prob,
                         const float* labels, float* prob);

/* ---- Criteo DAC data path (SURVEY §8 rows f2 + f4; criteo.jl:85-344) ----------------------
 * dlrm_dac_record: DACRecord (criteo.jl:91-95), 160 bytes, the binary file format (mmap-able).
 * dlrm_dac_parse_tsv: parseline over a buffer of TSV lines (criteo.jl:164-176): label Int32,
 *   13 x logtransform(emptyparse(Int32, base 10)) as Float32, 26 x emptyparse(UInt32, base 16).
 *   Blank lines are skipped; *count = records written.  DLRM_E_NOMEM if more than cap lines,
 *   DLRM_E_ARG on a malformed line.  Host only.
 * dlrm_dac_maps_*: categorical_values + reindex/reindex! (criteo.jl:182-262): per feature, ids
 *   1, 2, ... in first-appearance order, accumulated over shards added in order.  Host only.
 * dlrm_dac_reindex: reindex!(data, maps) in place (criteo.jl:251-259); DLRM_E_INDEX for a value
 *   that is not in the maps (the reference's KeyError).
 * dlrm_dac_decode: load! (criteo.jl:284-307) on the device: `batch` contiguous records already in
 *   HBM -> labels [batch] f32, dense [batch][13] f32 (row stride dense_ld), sparse [26][batch]
 *   indices (itype DLRM_I32 / DLRM_I64, table stride table_stride) = DACLoader's
 *   Matrix{UInt32}(B, 26) layout, which is the hot path's [T][B] index layout (index_base 1). */
typedef struct {
    int32_t label;
    float continuous[13];
    uint32_t categorical[26];
} dlrm_dac_record;
typedef struct dlrm_dac_maps dlrm_dac_maps;
int dlrm_dac_parse_tsv(const char* text, int64_t len, dlrm_dac_record* out, int64_t cap, int64_t* count);
int dlrm_dac_maps_create(dlrm_dac_maps** out);
int dlrm_dac_maps_destroy(dlrm_dac_maps* maps);
int dlrm_dac_maps_add(dlrm_dac_maps* maps, const dlrm_dac_record* records, int64_t count);
int dlrm_dac_maps_sizes(const dlrm_dac_maps* maps, int64_t* sizes /* [26] */);
int dlrm_dac_maps_lookup(const dlrm_dac_maps* maps, int feature, uint32_t value, uint32_t* id);
int dlrm_dac_reindex(const dlrm_dac_maps* maps, dlrm_dac_record* records, int64_t count);
int dlrm_dac_decode(dlrm_ctx* ctx, const dlrm_dac_record* records, int batch, float* labels, float* dense,
                    int64_t dense_ld, void* sparse, int itype, int64_t table_stride);
/* Native prefetching DACLoader.  create: `records` (host, count records, kept alive by the
 * caller) and the caller's two output slots (device: labels[k] [batch] f32, dense[k] [batch][13]
 * f32, sparse[k] [26][batch] of itype).  start: one epoch of count/batch whole batches on a
 * native worker thread (pinned staging, upload + dlrm_dac_decode on the loader's own stream).
 * next: blocks until the next batch is decoded, makes consumer_stream wait for it, returns its
 * slot (-1: epoch over).  release: the caller's work on that slot is queued on consumer_stream;
 * the slot may be refilled after it.  stop: ends the epoch early.  start returns DLRM_E_STATE
 * while a slot of the previous epoch is still held (next without release).  The calls for one
 * loader come from one host thread. */
typedef struct dlrm_dac_loader dlrm_dac_loader;
int dlrm_dac_loader_create(int device, const dlrm_dac_record* records, int64_t count, int batch, int itype,
                           float* const* labels, float* const* dense, void* const* sparse, dlrm_dac_loader** out);
int dlrm_dac_loader_start(dlrm_dac_loader* loader, int64_t* nbatches);
int dlrm_dac_loader_next(dlrm_dac_loader* loader, void* consumer_stream, int* slot);
int dlrm_dac_loader_release(dlrm_dac_loader* loader, int slot, void* consumer_stream);
int dlrm_dac_loader_stop(dlrm_dac_loader* loader);
int dlrm_dac_loader_destroy(dlrm_dac_loader* loader);

/* ---- int8 row-quantized tables (inference and evaluation) ------------------------------
 * A quantized table t is two caller-owned device arrays: codes q[nrows[t]][dim] of uint8, row-major,
 * and sb[nrows[t]] of float2 {scale, bias} (passed as float*, 8-B aligned).  They are separate so that
 * rows stay 16-B aligned whenever dim % 16 == 0 (a dim = 128 row is one 128-B line).
 * Quantizing a row w[0..dim) (bf16 elements first converted to fp32), every operation a separately
 * rounded fp32 operation:
 *   lo = min_c w[c]   hi = max_c w[c]   range = hi - lo
 *   scale = range / 255.0f                      inv = range > 0 ? 255.0f / range : 0.0f   (IEEE division)
 *   q[c]  = (uint8) min(255, max(0, rintf((w[c] - lo) * inv)))   (ties to even)      bias = lo
 * Dequantizing is two roundings, never an fma:  v[c] = ((float)q[c] * scale) + bias; a bf16 consumer gets
 * v[c] rounded to nearest even, once.  Every element of a finite row with a finite range satisfies
 *   |v - w| <= (0.5 + 2^-10) * scale + 2^-22 * max(|lo|, |hi|);
 * for any other row nothing faults and what is stored is unspecified.  Min and max are exact in any order,
 * so the quantizer is bitwise reproducible.  No reference counterpart (DLRM.jl trains and scores fp32).
 * create: no device work but the upload of the descriptors; the arrays stay caller-owned.
 * quantize: src is fp32 or bf16; table count, dim and row counts must match (else DLRM_E_ARG); one launch
 *           over every table, 64-bit row offsets.
 * dequantize: writes v (fp32) or bf16(v) into an existing table set of the same shape: the way back.
 * The launching calls allocate nothing and do not synchronise (hipGraph-capturable); an out-of-range
 * index never faults, contributes a zero row and raises the flag dlrm_check_bounds reads. */
typedef struct dlrm_q8_tables dlrm_q8_tables;
int dlrm_q8_tables_create(dlrm_ctx* ctx, int num_tables, int dim, uint8_t* const* q, float* const* sb,
                          const int64_t* nrows, dlrm_q8_tables** out);
int dlrm_q8_tables_destroy(dlrm_q8_tables* q8);
int dlrm_q8_quantize(dlrm_ctx* ctx, const dlrm_tables* src, dlrm_q8_tables* dst);
int dlrm_q8_dequantize(dlrm_ctx* ctx, const dlrm_q8_tables* src, dlrm_tables* dst);

/* dlrm_maplookup reading quantized rows: out (of `dtype`) receives exactly what dlrm_maplookup over the
 * dlrm_q8_dequantize'd set of that dtype writes -- one-hot: v converted to dtype; lookups > 1: the rows as
 * that set holds them (v, or bf16(v)), seeded with the first, added in k order in fp32, converted once.  Any dim >= 1; 16 codes per lane where
 * dim % 16 == 0 and the code rows and the output rows are 16-B aligned, one code per lane otherwise, with
 * the same results. */
int dlrm_q8_maplookup(dlrm_ctx* ctx, const dlrm_q8_tables* q8, const void* indices, int itype,
                      int64_t table_stride, int index_base, int batch, int lookups, int dtype,
                      void* out, int64_t out_ld, int64_t out_offset);

/* The inference forward on quantized rows in ONE launch, no ys: out (of `dtype`, as x) receives exactly
 * what dlrm_q8_maplookup(out_offset = d, into a ys) + dlrm_interact_fwd write.  Requires q8->dim == d.
 * Returns DLRM_E_UNSUPPORTED, with nothing launched, where there is no fused kernel; the caller then
 * takes those two calls.  The fused kernel exists exactly for: lookups == 1; 1 <= num_tables <= 31;
 * d % 4 == 0 (fp32) or d % 8 == 0 (bf16); every q pointer 4-B (fp32) or 8-B (bf16) aligned; x 16-B aligned
 * with x_ld % 4 == 0 (fp32) or x_ld % 8 == 0 (bf16).  out and out_ld need no alignment. */
int dlrm_q8_lookup_interact_fwd(dlrm_ctx* ctx, const dlrm_q8_tables* q8, const void* indices, int itype,
                                int64_t table_stride, int index_base, int batch, int lookups, int dtype,
                                const void* x, int64_t x_ld, void* out, int64_t out_ld, int padding);

#ifdef __cplusplus
}
#endif
#endif /* DLRM_HIP_H */
