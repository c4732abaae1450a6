/*
 * hippomm_hip.h -- C ABI of libhippomm_hip.so, the MI355X (gfx950) implementation of
 * HippoMM's perceptual-encoding + similarity hot path.
 *
 * The reference (linyueqian/HippoMM) is pure Python and has no FFI; its boundary for this
 * path is three Python call sites.  Each entry point below names the reference interface
 * it replaces (file:line relative to the reference repo).  The Python shims that keep the
 * reference signatures live in hippomm_amd/ (vector_ops.py, consolidation.py, encoder.py)
 * and bind these symbols with ctypes; INTEGRATION.md shows the reference-side patch.
 *
 * Conventions
 *   - plain C types only; every pointer named *_dev is a DEVICE pointer owned by the caller
 *     (PyTorch-ROCm allocates).  The library never frees or reallocates caller memory and
 *     never allocates outputs.  Only hmm_encoder_create() allocates (its own packed weights).
 *   - every launch goes to the caller's stream (hipStream_t passed as void*; hmm_encoder_forward also uses streams
 *     owned by the handle, forked from and joined to the caller's stream with events); no call synchronises the
 *     device or allocates, so all calls can be captured into a HIP graph (tests/test_gpu_encoder_batch.py).  A forward
 *     issued under stream capture runs as a single chain whatever hmm_encoder_set_streams says.
 *   - return value: 0 = ok, negative = error (HMM_E_*); hmm_last_error() returns a
 *     thread-local message for the last failing call on this thread.
 *   - single-threaded use per handle, as in the reference (all call sites are on the main
 *     thread of one process).  Never call from a fork()ed child.
 */
#ifndef HIPPOMM_HIP_H
#define HIPPOMM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HMM_OK            0
#define HMM_E_INVALID    -1   /* bad argument (shape, null pointer, unsupported size) */
#define HMM_E_WORKSPACE  -2   /* workspace too small */
#define HMM_E_HIP        -3   /* a HIP runtime call failed */
#define HMM_E_STATE      -4   /* handle not ready (weights missing) */

#define HMM_FEATURE_DIM  1024 /* width of every embedding / store row (reference shape guard:
                                 hippocampal_memory.py:484, :829, :1190, :3135) */

typedef void* hmm_stream_t;   /* hipStream_t */

/* Alignment: stores, queries and workspaces (*_dev) must be 16-byte aligned -- anything hipMalloc or a torch allocation returns is
 * 256-byte aligned; a pointer into the middle of such a buffer must keep the 16 bytes.  Refused with HMM_E_INVALID otherwise.
 * Workspaces: exactly the bytes a *_workspace_bytes query answers suffice (one byte fewer is refused with HMM_E_WORKSPACE before
 * anything is launched or written); their contents need no initialisation; and one workspace may be reused across calls, shapes
 * and entry points on one stream -- no call depends on what an earlier one left there.  No call reads or writes a byte outside
 * the documented extent of its buffers (tests/test_gpu_memory_contract.py).  hmm_encoder_workspace_bytes answers for the
 * handle's current hmm_encoder_set_streams setting: ask again after changing it. */

int         hmm_abi_version(void);
const char* hmm_last_error(void);
/* HMM_OK when the current HIP device is what this library is built for (gfx950 with 256 compute units: the launch
 * geometries and the code objects assume it); HMM_E_STATE with a message otherwise.  The Python package calls it once per
 * device before the first kernel. */
int         hmm_device_supported(void);

/* ------------------------------------------------------------------------------------------
 * feature_search scan.  Replaces top_k_cosine_similarity(a, b, k)
 * (hippomm/utils/vector_ops.py:151-188; callers hippocampal_memory.py:3153, :3304).
 *
 *   sims[i] = dot(store[i], q) / (||store[i]|| * ||q||)      fp32, one pass over the store
 *   result  = the k' = min(k, n_rows) rows with the largest sims, best first.
 *   Order on ties / NaN: UNSPECIFIED in the reference -- it takes argsort(sims)[-k:][::-1] (vector_ops.py:185) and numpy's
 *   default introsort is unstable, so which of several equal (or NaN) similarities survives the cut depends on the input
 *   length and layout.  THIS library's rule is a total order: NaN (zero-norm row or query) ranks above every number; among
 *   equal sims the HIGHER row index comes first; -0.0 == +0.0.  It reproduces what the reference returns on the golden
 *   duplicate-row and zero-row cases (tests/golden/scan_golden.json) but not always: on live case 31 the reference
 *   returns zero-norm row 12 of {12, 55} where this rule returns 55 (tests/test_gpu_live_golden.py checks values and
 *   membership there, not the order inside a tie group).
 *
 *   store_dev  (n_rows, 1024) fp32 row-major, resident in HBM      query_dev (1024) fp32
 *   idx_out_dev int64[k'], sim_out_dev fp32[k'], n_out_dev int32[1] (= k')
 * ---------------------------------------------------------------------------------------- */
size_t hmm_cosine_topk_workspace_bytes(int64_t n_rows, int k);
int    hmm_cosine_topk(const float* store_dev, int64_t n_rows, int dim,
                       const float* query_dev, int k,
                       int64_t* idx_out_dev, float* sim_out_dev, int32_t* n_out_dev,
                       void* workspace_dev, size_t workspace_bytes, hmm_stream_t stream);

/* Sharded scan: same scan, but emits the local top-k as packed 64-bit order keys
 * ((ordered sim bits << 32) | local row) so that ranks can all-gather 8*k bytes and merge with
 * hmm_topk_merge_keys, which adds each shard's row offset and applies the same total order. */
int    hmm_cosine_topk_keys(const float* store_dev, int64_t n_rows, int dim,
                            const float* query_dev, int k, uint64_t* keys_out_dev /* [k], 0-padded */,
                            void* workspace_dev, size_t workspace_bytes, hmm_stream_t stream);
int    hmm_topk_merge_keys(const uint64_t* keys_dev /* [n_shards][k] */, int n_shards, int k,
                           const int64_t* shard_row_offset_dev /* [n_shards] */,
                           int64_t* idx_out_dev, float* sim_out_dev, int32_t* n_out_dev,
                           hmm_stream_t stream);

/* feature_search through a bf16 SHADOW of the store (SURVEY 8d's optional shadow store; reported separately against
 * 2048 B per row).  hmm_shadow_store_build writes shadow row r = bf16(store[r] / ||store[r]||) (2048 B per row, NaN for a
 * zero-norm or non-finite row); hmm_cosine_topk_prefilter streams the shadow for approximate similarities, keeps every row that
 * can be among the k best under a proven error bound (|s~ - s| < 0.004: bf16 has an 8-bit significand), re-scores those rows on
 * the fp32 store with the arithmetic of hmm_cosine_topk and returns the k best: the SAME indices and the SAME fp32 similarities,
 * bit for bit, as hmm_cosine_topk (vector_ops.py:178-186 semantics, same total order).  When the candidate set is not provably
 * complete (a store of thousands of near-ties) the exact scan runs instead, inside the same call, decided on the device.
 * k > 64 or fewer than 16384 rows: the call IS hmm_cosine_topk.  stats_out_dev (may be null) int32[2]: candidates re-scored and
 * saturated block lists of the last call (-1, -1 when the prefilter was not used); a non-zero second entry or more than 1024
 * candidates means the exact scan answered.
 * Precondition of the bit identity: every row's squared norm is finite and non-zero in fp32 (unit-scale embeddings are).  A row
 * whose norm overflows or underflows gets a NaN shadow row, which ranks first here, while hmm_cosine_topk gives it 0 or +-inf.
 * The shadow is a snapshot of the rows it was built from: rebuild it after the rows change. */
size_t hmm_shadow_store_bytes(int64_t n_rows);
int    hmm_shadow_store_build(const float* store_dev, int64_t n_rows, int dim, void* shadow_dev, size_t shadow_bytes,
                              hmm_stream_t stream);
size_t hmm_cosine_topk_prefilter_workspace_bytes(int64_t n_rows, int k);
int    hmm_cosine_topk_prefilter(const float* store_dev, const void* shadow_dev, int64_t n_rows, int dim,
                                 const float* query_dev, int k, int64_t* idx_out_dev, float* sim_out_dev, int32_t* n_out_dev,
                                 int32_t* stats_out_dev, void* workspace_dev, size_t workspace_bytes, hmm_stream_t stream);

/* hmm_cosine_topk_segmented through the shadow: one pass over 2048 B per row for approximate similarities, per event the rows
 * that can be among its k best (same bound) re-scored on the fp32 store.  Same outputs as hmm_cosine_topk_segmented, bit for
 * bit (hippocampal_memory.py:3143-3153 semantics).  k > 64, or events of fewer than 128 rows on average: the call IS
 * hmm_cosine_topk_segmented. */
size_t hmm_cosine_topk_segmented_prefilter_workspace_bytes(int64_t n_rows, int n_segments, int k);
int    hmm_cosine_topk_segmented_prefilter(const float* store_dev, const void* shadow_dev, int64_t n_rows, int dim,
                                           const float* query_dev, const int64_t* seg_offsets_dev, int n_segments, int k,
                                           int64_t* idx_out_dev, float* sim_out_dev, int32_t* n_out_dev,
                                           void* workspace_dev, size_t workspace_bytes, hmm_stream_t stream);

/* A store that grows on the device (EventStore.append_event / remove_events / replace_event): the caller owns a buffer of
 * capacity_rows fp32 rows and, optionally, one of capacity_rows * 2048 bytes for the shadow; these two calls fill them.
 *
 * hmm_store_ingest_rows: src_dtype: 0 = fp32, 1 = fp64.  Writes rows [row_offset, row_offset + n_new) of store_dev and, when
 * shadow_dev is not null, the same rows of the shadow.  Touches no other byte of either buffer.  An fp32 source is copied bit
 * for bit; an fp64 source is narrowed with round-to-nearest-even (ndarray.astype(float32)); the shadow rows have the bits
 * hmm_shadow_store_build gives those rows.  One pass: 4 KB (8 KB) read, 4 KB + 2 KB written per row.
 *
 * hmm_store_gather_segments: out of place.  Destination segment j (rows dst_offsets[j] .. dst_offsets[j+1]) receives source
 * segment src_segment[j] (rows src_offsets[s] .. src_offsets[s+1]), or is left untouched when src_segment[j] == -1 (a hole the
 * caller fills with hmm_store_ingest_rows).  Shadow rows travel with their fp32 rows when both shadow pointers are given; both
 * null is allowed, one null is an error.  Segments of equal length are the caller's precondition; a segment copies
 * min(destination length, source length) rows, reads nothing outside its source segment or beyond src_rows and writes nothing
 * outside its destination segment or at or beyond dst_rows.
 *
 * Both: n_new == 0, n_dst == 0 or dst_rows == 0 return HMM_OK without a launch and without looking at a pointer.  Otherwise
 * HMM_E_INVALID, before anything is launched, for dim != 1024, an unknown src_dtype, a negative count, row_offset + n_new >
 * capacity_rows, dst_rows > dst_capacity_rows, a null pointer, a row pointer that is not 16-byte aligned, or a source byte range
 * that overlaps the bytes to be written.  No workspace; nothing is allocated, copied or synchronised. */
int    hmm_store_ingest_rows(const void* src_dev, int src_dtype, int64_t n_new, int dim,
                             float* store_dev, void* shadow_dev /* nullable */,
                             int64_t capacity_rows, int64_t row_offset, hmm_stream_t stream);
int    hmm_store_gather_segments(const float* src_store_dev, const void* src_shadow_dev, int64_t src_rows,
                                 const int64_t* src_offsets_dev, int n_src_segments,
                                 const int32_t* src_segment_dev /* [n_dst] */, const int64_t* dst_offsets_dev /* [n_dst+1] */,
                                 int n_dst, int dim, float* dst_store_dev, void* dst_shadow_dev, int64_t dst_rows,
                                 int64_t dst_capacity_rows, hmm_stream_t stream);

/* The stack behind consolidate_short_term_memory (hippocampal_memory.py:842: one row per frame out of every segment's own feature
 * block, in time order), built on the device from the blocks where they lie.
 *
 * hmm_rows_gather: src_row_ptrs_dev is a device table of n device addresses; src_row_ptrs_dev[i] is the address of 1024
 * contiguous fp32 values, and row i of out_dev (contiguous (n,1024)) receives them bit for bit.  Unlike
 * hmm_store_gather_segments the sources are independent allocations, addressed row by row: the same source row may be named any
 * number of times and the sources may lie in any order.  Writes exactly n * 4096 bytes of out_dev; reads exactly the named rows
 * and the n table entries.  One wave copies one row with 16-byte loads and stores; a source row that is only 4-byte aligned (a
 * view into a wider matrix at an odd column offset) takes a dword path, chosen per row on its address.  out_dev must be 16-byte
 * aligned, the table 8-byte aligned.
 *
 * The host cannot see the addresses in the table.  THE CALLER GUARANTEES that every one of them is the address of a readable
 * fp32 row of 1024 values on the stream's device, aligned to 4 bytes at least, that stays valid until the launch has run, and
 * that no source row overlaps the n * 4096 bytes of out_dev.  Nothing of this can be checked here; a wrong address is a wild read.
 *
 * n == 0 returns HMM_OK without a launch and without looking at a pointer.  Otherwise HMM_E_INVALID, before anything is launched,
 * for dim != 1024, n < 0, a null table or output, or a misaligned table or output.  No workspace; nothing is allocated, copied
 * or synchronised. */
int    hmm_rows_gather(const uint64_t* src_row_ptrs_dev /* [n] */, int64_t n, int dim, float* out_dev /* (n,1024) */,
                       hmm_stream_t stream);

/* Batched feature_search: the top-k of n_queries queries against the same store in ONE pass over it
 * (16 queries per pass; the Q x rows similarity block runs on the fp32 matrix cores, so a row is still read once from
 * HBM).  The reference calls top_k_cosine_similarity once per question (hippomm/utils/vector_ops.py:151-188 via
 * hippocampal_memory.py:3153, :3304).  queries_dev (n_queries,1024) fp32 row-major.  Outputs are row-major with row
 * stride k: idx_out[q*k ..], sim_out[q*k ..] (the first min(k, n_rows) entries of a row are valid), n_out[q].
 * Same similarity, total order and tie rule as hmm_cosine_topk (results can differ from it only where two similarities
 * agree to fp32 rounding: the dot products are summed in a different order).  k > 64 falls back to one scan per query. */
size_t hmm_cosine_topk_multi_workspace_bytes(int64_t n_rows, int n_queries, int k);
int    hmm_cosine_topk_multi(const float* store_dev, int64_t n_rows, int dim, const float* queries_dev, int n_queries,
                             int k, int64_t* idx_out_dev, float* sim_out_dev, int32_t* n_out_dev,
                             void* workspace_dev, size_t workspace_bytes, hmm_stream_t stream);

/* Per-event feature_search in one pass.  Replaces the Python loop over events that calls
 * top_k_cosine_similarity(query, event.features[...], k=5) once per event
 * (hippomm/core/hippocampal_memory.py:3143-3153, :3294-3304).  store_dev is the concatenation of the
 * events' (n_e,1024) matrices, seg_offsets_dev int64[n_segments+1] their row offsets (non-decreasing,
 * last = n_rows).  Per event e: n_out[e] = min(k, n_e); idx_out[e*k ..] rows WITHIN the event (best first,
 * -1 padded), sim_out[e*k ..] (0 padded).  Same similarity and total order as hmm_cosine_topk. k <= 1024. */
size_t hmm_cosine_topk_segmented_workspace_bytes(int64_t n_rows, int n_segments, int k);
int    hmm_cosine_topk_segmented(const float* store_dev, int64_t n_rows, int dim, const float* query_dev,
                                 const int64_t* seg_offsets_dev, int n_segments, int k,
                                 int64_t* idx_out_dev, float* sim_out_dev, int32_t* n_out_dev,
                                 void* workspace_dev, size_t workspace_bytes, hmm_stream_t stream);

/* The global ranking behind that loop (hippocampal_memory.py:3275-3277: the hits of every event in one list, sorted by similarity
 * descending -- Python's stable sort: equal similarities stay in event order -- and the best ones kept).  Inputs: the three outputs of
 * hmm_cosine_topk_segmented[_prefilter].  Outputs: the best keep' = min(keep, number of hits) hits, best first: event index, row
 * within the event, similarity (-1 / -1 / 0 padded to `keep`), *n_out = keep'.  NaN similarities rank first.  keep <= 64. */
int    hmm_rank_segment_hits(const int64_t* idx_dev, const float* sims_dev, const int32_t* counts_dev, int n_segments, int k,
                             int keep, int64_t* event_out_dev, int64_t* row_out_dev, float* sim_out_dev, int32_t* n_out_dev,
                             hmm_stream_t stream);

/* Per-event feature_search for a BATCH of questions: what n_queries calls of hmm_cosine_topk_segmented return, for one
 * read of the store per 16 questions instead of one per question -- the similarity block of 16 questions x rows runs on the fp32
 * matrix cores exactly as in hmm_cosine_topk_multi, the per-event selection is hmm_cosine_topk_segmented's.  queries_dev
 * (n_queries,1024) fp32 row-major; store_dev / seg_offsets_dev as in hmm_cosine_topk_segmented, n_rows >= 1.  Outputs are
 * query-major: idx_out[(q*n_segments + e)*k ..] rows WITHIN event e (best first, -1 padded), sim_out likewise (0 padded),
 * n_out[q*n_segments + e] = min(k, n_e).  The similarity of (row, query) has the bits hmm_cosine_topk_multi gives it, whatever the
 * row's place in the store and the query's place in the batch: slice (q, e) equals hmm_cosine_topk_multi on event e's rows alone.
 * k > 64: one hmm_cosine_topk_segmented per query inside the call (that function's bits).  k <= 1024.  The workspace does not
 * depend on n_queries or k: it holds the similarities of one pass, 16 x 4 B per row. */
size_t hmm_cosine_topk_segmented_multi_workspace_bytes(int64_t n_rows, int n_segments, int n_queries, int k);
int    hmm_cosine_topk_segmented_multi(const float* store_dev, int64_t n_rows, int dim,
                                       const float* queries_dev, int n_queries,
                                       const int64_t* seg_offsets_dev, int n_segments, int k,
                                       int64_t* idx_out_dev, float* sim_out_dev, int32_t* n_out_dev,
                                       void* workspace_dev, size_t workspace_bytes, hmm_stream_t stream);

/* hmm_cosine_topk_multi through the bf16 shadow (hmm_shadow_store_build; the shadow's format is unchanged): one pass over 2048 B per
 * row per 16 questions on the bf16 matrix cores (each question split into bf16 hi + lo), per question every row that can be among
 * its k best under a proven error bound (|s~ - s| < 0.0042) re-scored on the fp32 store with the arithmetic of hmm_cosine_topk_multi,
 * the k best returned: the SAME indices, similarity bits and counts as hmm_cosine_topk_multi.  When a question's candidate set is
 * not provably complete (thousands of near-ties, a zero or NaN question) the exact pass answers for the 16 questions of that pass,
 * inside the same call, decided on the device.  k > 64, fewer than 16384 rows or n_rows <= k: the call IS hmm_cosine_topk_multi.
 * stats_out_dev (may be null) int32[n_queries][2]: per question, candidates re-scored and saturated workgroup lists (-1, -1 in every
 * slot when the call was the exact function); a non-zero second entry or more than 1024 candidates means the exact pass answered
 * for that question's pass.  Layouts, the precondition on the rows' norms and the snapshot rule are those of hmm_cosine_topk_multi and
 * hmm_cosine_topk_prefilter.  The workspace holds the exact function's and must be 16-byte aligned. */
size_t hmm_cosine_topk_multi_prefilter_workspace_bytes(int64_t n_rows, int n_queries, int k);
int    hmm_cosine_topk_multi_prefilter(const float* store_dev, const void* shadow_dev, int64_t n_rows, int dim,
                                       const float* queries_dev, int n_queries, int k,
                                       int64_t* idx_out_dev, float* sim_out_dev, int32_t* n_out_dev,
                                       int32_t* stats_out_dev /* nullable, int32[n_queries][2] */,
                                       void* workspace_dev, size_t workspace_bytes, hmm_stream_t stream);

/* hmm_cosine_topk_segmented_multi through the shadow: the same pass writes the approximate similarities of 16 questions (64 B per
 * row, the exact function's workspace), then per (event, question) the rows that can be among the event's k best (same bound) are
 * re-scored on the fp32 store -- every row of an event whose candidates do not fit (an event of near-identical rows).  Same
 * outputs as hmm_cosine_topk_segmented_multi, bit for bit.  k > 64, or events of fewer than 128 rows on average: the call IS
 * hmm_cosine_topk_segmented_multi.  stats_out_dev (may be null) int32[2]: (event, question) pairs that re-scored the whole event,
 * and rows re-scored in all (-1, -1 when the call was the exact function); a diagnostic: the second is an int32 sum over all pairs
 * and passes and may wrap on millions of near-identical rows.  Both dispatch limits (here and in hmm_cosine_topk_multi_prefilter)
 * are those of the single-question functions and have not been timed for a batch yet: tools/multi_prefilter_probe.py places them,
 * and until it has run no Python call takes these two routes unless asked to (prefilter=True). */
size_t hmm_cosine_topk_segmented_multi_prefilter_workspace_bytes(int64_t n_rows, int n_segments, int n_queries, int k);
int    hmm_cosine_topk_segmented_multi_prefilter(const float* store_dev, const void* shadow_dev, int64_t n_rows, int dim,
                                                 const float* queries_dev, int n_queries,
                                                 const int64_t* seg_offsets_dev, int n_segments, int k,
                                                 int64_t* idx_out_dev, float* sim_out_dev, int32_t* n_out_dev,
                                                 int32_t* stats_out_dev /* nullable, int32[2] */,
                                                 void* workspace_dev, size_t workspace_bytes, hmm_stream_t stream);

/* hmm_rank_segment_hits for every question of a batch in one launch: inputs are the three outputs of
 * hmm_cosine_topk_segmented_multi, (n_queries, n_segments, k) / (n_queries, n_segments); per question q the best
 * keep' = min(keep, its number of hits) hits at event_out[q*keep ..], row_out[q*keep ..], sim_out[q*keep ..] (-1 / -1 / 0 padded to
 * `keep`), n_out[q] = keep'.  Same key and stable order as hmm_rank_segment_hits.  keep <= 64. */
int    hmm_rank_segment_hits_multi(const int64_t* idx_dev, const float* sims_dev, const int32_t* counts_dev,
                                   int n_queries, int n_segments, int k, int keep,
                                   int64_t* event_out_dev, int64_t* row_out_dev, float* sim_out_dev, int32_t* n_out_dev,
                                   hmm_stream_t stream);

/* hmm_rank_segment_hits with the reference's two per-event rules applied BEFORE the global sort (hippocampal_memory.py:3143-3277,
 * :3294-3381).  Inputs: the three outputs of hmm_cosine_topk_segmented[_prefilter], plus
 *   row_limits_dev  (nullable) int64[n_segments]: a hit of event e counts only when its row idx < row_limits[e] -- the reference's
 *                   `idx < len(event.frame_times)` (:3247, :3262) / `idx < len(event.feature_times['audio_times'])` (:3336, :3370);
 *                   null: no row rule;
 *   defer_dev       (nullable) uint8[n_segments]: event e is DEFERRED iff defer[e] != 0, n_e > 0 and its best similarity (slot 0 of
 *                   the event) < min_similarity, compared as fp32 -- the reference's `max(similarities) < 0.4 and captions` (:3156,
 *                   :3307).  NaN ranks first inside an event, so a NaN makes the comparison false, as np.max(...) < 0.4 and
 *                   max(...) < 0.4 are on an array holding a NaN.  No fp32 value lies strictly between 0.4 and (float)0.4, so
 *                   np.float32(x) < 0.4 decides the same under numpy 1.x (which widens x) and numpy 2 (which narrows 0.4) for every
 *                   fp32 x: pass min_similarity = (float)0.4.  null: nothing is deferred.
 * A deferred event leaves the ranking with all its hits; the hits of the others that pass the row rule are ranked with
 * hmm_rank_segment_hits' key and stable order (NaN first).  keep <= 1024: the best-64 tournament runs in rounds, round r over the
 * keys strictly below the last key of round r - 1; keep <= 64 is one round.
 * Outputs: event_out / row_out / sim_out [keep]: the best keep' = min(keep, candidates) hits, -1 / -1 / 0 padded; *n_out = keep'.
 *   deferred_event_out int32[n_segments]: the deferred events, ascending, -1 padded; *n_deferred_out their number n_d;
 *   deferred_idx_out int64[n_segments*k], deferred_sim_out float[n_segments*k], deferred_count_out int32[n_segments]: for the j-th
 *   deferred event its own (idx, sims, count) slice, copied unchanged, at [j*k ..] / [j].  Entries at and after n_d*k (counts: n_d)
 *   are NOT WRITTEN: they keep whatever the caller left there.
 * One workgroup, no workspace.  The similarities this call ranks are fp32 results.  For a store whose source was float64 the
 * reference computes them in float64, so by DEFAULT a decision within 2e-6 of the threshold, and the order of hits whose cosines
 * differ by less than fp32 accumulation noise, are this library's, not the reference's.  The opt-in float64 route below
 * (hmm_cosine_topk_segmented_f64; exact64=True in Python) removes that for stores whose float64 source held fp32 values: its
 * similarities are within 2^-42 of the exact quotient, and the two rules and the stable sort are then applied to doubles on the
 * host.  What stays this library's own in that mode: the order inside EXACT ties, and, for a query that lives on the device, the
 * last fp32 bit of the query's norm (see there).  The default of every call is unchanged. */
int    hmm_rank_segment_hits_filtered(const int64_t* idx_dev, const float* sims_dev, const int32_t* counts_dev, int n_segments, int k,
                                      int keep, const int64_t* row_limits_dev /* nullable */, const uint8_t* defer_dev /* nullable */,
                                      float min_similarity,
                                      int64_t* event_out_dev, int64_t* row_out_dev, float* sim_out_dev, int32_t* n_out_dev,
                                      int32_t* deferred_event_out_dev, int32_t* n_deferred_out_dev,
                                      int64_t* deferred_idx_out_dev, float* deferred_sim_out_dev, int32_t* deferred_count_out_dev,
                                      hmm_stream_t stream);

/* hmm_rank_segment_hits_filtered for every question of a batch in one launch (one workgroup per question): inputs are the three
 * outputs of hmm_cosine_topk_segmented_multi[_prefilter]; row_limits and defer are shared by all questions.  Every output is
 * query-major: question q's part starts at q*keep (hits), q (counts), q*n_segments (deferred events and counts), q*n_segments*k
 * (deferred slices), and equals what the single call writes for that question, unwritten tails included. */
int    hmm_rank_segment_hits_filtered_multi(const int64_t* idx_dev, const float* sims_dev, const int32_t* counts_dev,
                                            int n_queries, int n_segments, int k, int keep,
                                            const int64_t* row_limits_dev /* nullable */, const uint8_t* defer_dev /* nullable */,
                                            float min_similarity,
                                            int64_t* event_out_dev, int64_t* row_out_dev, float* sim_out_dev, int32_t* n_out_dev,
                                            int32_t* deferred_event_out_dev, int32_t* n_deferred_out_dev,
                                            int64_t* deferred_idx_out_dev, float* deferred_sim_out_dev,
                                            int32_t* deferred_count_out_dev, hmm_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Float64-origin stores: similarities and ranking in float64 (opt-in; no other call changes).
 *
 * load_theta_event hands the reference float64 matrices (hippocampal_memory.py:387-395), so its top_k_cosine_similarity runs
 * np.dot(b, a) / (b_norms * a_norm) in float64 (vector_ops.py:178-186).  A reloaded event holds the repr digits of fp32 tower
 * outputs: every float64 value of such a store is an fp32 value, narrowing it loses nothing, and only the ARITHMETIC differs.
 * These calls keep the resident fp32 rows and do the arithmetic in fp64.
 *
 * Inputs.  store_dev (n_rows, 1024) fp32, each value equal to its float64 source (hmm_rows_f64_are_f32 checks a source).
 *   query_dev 1024 values, fp32 (query_dtype 0) or fp64 (1), widened to double.  16-byte aligned both.
 * Similarity.  sim_r = D_r / (sqrt(S_r) * A), D_r = sum x_ri a_i, S_r = sum x_ri^2, accumulated in fp64 with explicit fma on
 *   exactly widened operands (the product of two fp32-origin doubles is exact in fp64: only the sums round).  Operation order as
 *   in the reference: the norms multiplied first, then one division; sqrt and / correctly rounded (no fast-math).
 * Fixed summation order.  One wave per row.  Lane l (0..63) owns columns 4 (64 j + l) + c, j = 0..3, c = 0..3.  Two chains per
 *   sum, both starting at +0.0: chain 0 takes j = 0 then j = 1, chain 1 takes j = 2 then j = 3, inside a j in the order c = 0, 1,
 *   2, 3.  Lane value = chain 0 + chain 1.  Wave reduction: v += v[lane ^ off] for off = 32, 16, 8, 4, 2, 1.  A row's similarity
 *   bits depend on the row, the query and A alone: not on n_rows, the grid, k, or which of the two entry points computed them.
 * A is the query's norm in the query's own dtype, widened.  query_norm_dev != null: that double is A -- the Python shim passes
 *   np.linalg.norm(a) of a host query, evaluated by numpy itself: the reference's own expression on the same host, hence its
 *   bits.  query_norm_dev == null (a query that lives on the device): the kernel accumulates sum a_i^2 in fp64 in the fixed order
 *   above and takes the square root; for an fp32 query it rounds the root to fp32 and widens it again.  numpy's fp32 dot may differ
 *   from that in the last fp32 bit.  A is a factor common to all rows: it cannot change a ranking, only a threshold decision within
 *   about 6e-8 relative.
 * Error bound (derived, u = 2^-53).  Either sum of 1024 exact products is, in any order, within 1023 u sum|terms| to first order,
 *   and sum|x_i a_i| <= ||x|| ||a||: the dot contributes at most 1.14e-13 relative to ||x|| ||a||; the root of S_r half of that plus
 *   u; the product and the division 3 u.  Total < 1.8e-13 < 2^-42 (2.27e-13), absolute on a cosine (for a device query: relative
 *   to the value computed with the same A).
 * Total order.  NaN first (a zero-norm row gives 0/0, as in the reference, where argsort puts NaN last before the reversal), then
 *   similarity descending, -0.0 == +0.0; exact ties: higher row index first, the library's rule everywhere.  Selection compares
 *   an order-preserving 64-bit transform of the double with the 32-bit position as second word; it is exact, so the flat call's
 *   result does not depend on how many workgroups share its first level.
 *
 * hmm_cosine_topk_f64: idx_out_dev int64[k'], sim_out_dev fp64[k'], k' = min(k, n_rows), best first; n_out_dev (nullable)
 *   int32[1] = k'.  n_rows >= 1; any k >= 1 (k' > 1024 sorts all rows).
 * hmm_cosine_topk_segmented_f64: layout, clamping, padding (-1 / 0) and counts of hmm_cosine_topk_segmented, with sim_out_dev fp64;
 *   every event's slice equals hmm_cosine_topk_f64 on that event's rows, bit for bit.  k <= 1024.  n_rows >= 0.
 * The workspace holds one double per row (plus, for the flat call, the first level's candidates) and needs no initialisation.
 * hmm_rows_f64_are_f32: report_dev int64[2] <- { number of values v of the float64 matrix src_dev (n_rows, 1024) whose bits differ
 *   from (double)(float)v's -- a NaN whose payload narrows exactly passes, a subnormal fp32 value passes --, the lowest flat
 *   offset (row * 1024 + column) of one, or -1 }.  Runs beside hmm_store_ingest_rows, not inside it.  n_rows == 0 writes { 0, -1 }.
 * All: every launch goes on `stream`; nothing is allocated, copied or synchronised; no workgroup waits for another.  HMM_E_INVALID
 *   before anything is launched (no GPU needed) for a null or misaligned pointer, dim != 1024, an unknown query_dtype, k < 1,
 *   n_rows out of range; HMM_E_WORKSPACE for a workspace below the *_workspace_bytes answer.
 * ---------------------------------------------------------------------------------------- */
size_t hmm_cosine_topk_f64_workspace_bytes(int64_t n_rows, int k);
int    hmm_cosine_topk_f64(const float* store_dev, int64_t n_rows, int dim, const void* query_dev, int query_dtype,
                           const double* query_norm_dev /* nullable */, int k,
                           int64_t* idx_out_dev, double* sim_out_dev, int32_t* n_out_dev /* nullable */,
                           void* workspace_dev, size_t workspace_bytes, hmm_stream_t stream);
size_t hmm_cosine_topk_segmented_f64_workspace_bytes(int64_t n_rows, int n_segments, int k);
int    hmm_cosine_topk_segmented_f64(const float* store_dev, int64_t n_rows, int dim, const void* query_dev, int query_dtype,
                                     const double* query_norm_dev /* nullable */, const int64_t* seg_offsets_dev, int n_segments,
                                     int k, int64_t* idx_out_dev, double* sim_out_dev, int32_t* n_out_dev,
                                     void* workspace_dev, size_t workspace_bytes, hmm_stream_t stream);
int    hmm_rows_f64_are_f32(const double* src_dev, int64_t n_rows, int dim, int64_t* report_dev /* [2] */, hmm_stream_t stream);

/* Float64-origin stores, batched: one pass over the store per 16 queries, the same bits.
 *
 * queries_dev (n_queries, 1024), all fp32 (query_dtype 0) or all fp64 (1), 16-byte aligned; query_norms_dev null, or one double per
 *   query, each used as hmm_cosine_topk_f64 uses its query_norm_dev (null: the kernel forms every norm by that call's rule,
 *   (double)(float) for an fp32 query included).  Any n_queries >= 1: served in passes of 16 inside the call.
 * Bit contract.  The fixed summation order above holds per (row, query), unchanged: lane ownership, the two fma chains from +0.0,
 *   lane value = chain 0 + chain 1, the operand pairs of the butterfly 32, 16, 8, 4, 2, 1, sim = D / (sqrt(S) * A).  S does not
 *   depend on the query and is formed once per row.  The pass forms each butterfly sum in the lanes that go on to use it (several
 *   (row, query) values packed per step) instead of in all 64: the same two operands are added, IEEE addition is commutative, and
 *   a sum that is not formed would have been a bitwise copy of one that is.  No matrix cores: fp64 MFMA has its own accumulation
 *   order.  Hence the similarity of row r to query q has the bits that hmm_cosine_topk_f64 computes for query q alone, whatever
 *   the entry point, n_queries, the query's position in the batch, its batch-mates, n_rows or k.
 * Selection.  The single calls' kernels and total order with the query as a second grid dimension: per event one workgroup per
 *   (query, event); flat, two exact levels per query; flat with min(k, n_rows) > 1024, the single call's full sort, query after query.
 * hmm_cosine_topk_multi_f64: idx_out_dev int64 (n_queries, k'), sim_out_dev fp64 (n_queries, k'), k' = min(k, n_rows): row q is what
 *   hmm_cosine_topk_f64 writes for query q, bit for bit; n_out_dev (nullable) int32[n_queries] = k'.  n_rows >= 1.
 * hmm_cosine_topk_segmented_multi_f64: idx_out_dev (n_queries, n_segments, k) int64, -1 padded, sim_out_dev the same shape fp64, 0.0
 *   padded, n_out_dev (n_queries, n_segments) int32: slice q is what hmm_cosine_topk_segmented_f64 writes for query q.  k <= 1024.
 * The workspace holds ONE pass: min(n_queries, 16) planes of n_rows doubles (plane q of a pass at its start + q n_rows doubles),
 *   plus the flat call's candidate pairs; it does not grow with n_queries beyond 16 and needs no initialisation.
 * Every launch goes on `stream`; nothing is allocated, copied or synchronised; no workgroup waits for another.  Before anything is
 *   launched (no GPU needed): HMM_E_INVALID for a null pointer, dim != 1024, an unknown query_dtype, n_queries < 1, k < 1, the
 *   segmented call's k > 1024, a store, query or workspace address that is not 16-byte aligned, a norm or output address that is
 *   not 8-byte aligned; HMM_E_WORKSPACE for a workspace below the *_workspace_bytes answer. */
size_t hmm_cosine_topk_multi_f64_workspace_bytes(int64_t n_rows, int n_queries, int k);
int    hmm_cosine_topk_multi_f64(const float* store_dev, int64_t n_rows, int dim, const void* queries_dev,
                                 int query_dtype /* 0 fp32, 1 fp64: one per call */,
                                 const double* query_norms_dev /* nullable, [n_queries] */, int n_queries, int k,
                                 int64_t* idx_out_dev, double* sim_out_dev, int32_t* n_out_dev /* nullable, [n_queries] */,
                                 void* workspace_dev, size_t workspace_bytes, hmm_stream_t stream);
size_t hmm_cosine_topk_segmented_multi_f64_workspace_bytes(int64_t n_rows, int n_segments, int n_queries, int k);
int    hmm_cosine_topk_segmented_multi_f64(const float* store_dev, int64_t n_rows, int dim, const void* queries_dev, int query_dtype,
                                           const double* query_norms_dev /* nullable, [n_queries] */, int n_queries,
                                           const int64_t* seg_offsets_dev, int n_segments, int k,
                                           int64_t* idx_out_dev, double* sim_out_dev, int32_t* n_out_dev,
                                           void* workspace_dev, size_t workspace_bytes, hmm_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Consolidation similarity.  Replaces HippocampalMemory._select_key_frames(features, times,
 * similarity_threshold=0.9) (hippomm/core/hippocampal_memory.py:944-967; caller :855).
 *
 *   Fn = F / ||F||_rows (fp32), S = Fn Fn^T with every dot accumulated in fp64 (f64 MFMA) and
 *   rounded to fp32 once, keep 0, then keep i iff all S[i, kept] < (float)threshold.
 *   A NaN similarity blocks (as `nan < thr` is False in the reference).  n <= 2 keeps all.
 *
 *   features_dev (n, 1024) fp32 row-major   kept_out_dev int64[n] (first *n_kept valid)
 * ---------------------------------------------------------------------------------------- */
size_t hmm_gram_select_workspace_bytes(int n);
int    hmm_gram_select(const float* features_dev, int n, int dim, float threshold,
                       int64_t* kept_out_dev, int32_t* n_kept_out_dev,
                       void* workspace_dev, size_t workspace_bytes, hmm_stream_t stream);

/* A selection that grows: hmm_keyframe_extend appends m rows (in time order) to a selection whose state lives in caller-owned
 * device memory, and decides each of them on arrival -- the greedy rule is causal.  After any number of calls the state is what
 * hmm_gram_select answers for all rows given so far, bit for bit (the dots run the same f64-MFMA sequence on the same normalised
 * rows), except for the n <= 2 clause: the call keeps the pure greedy state, and "n_seen <= 2 lists all rows" is the caller's
 * read-out rule (row 1 of two identical rows is dropped here, listed by the reference; from the third row on the two agree).
 *
 *   kept_rows_dev (capacity_kept, 1024) fp32: the NORMALISED rows of the kept frames, in kept order
 *   kept_idx_dev  int64[capacity_kept]: their global indices      n_kept_dev: one int64, their number
 *   n_seen_before  the host's exact count of rows given so far; 0 starts a selection: *n_kept_dev and the state buffers need
 *                  no initialisation then, the call treats the count as 0
 *   kept_bound     the host's upper bound on *n_kept_dev (<= n_seen_before): it sizes the new x kept grid, and every kernel clamps
 *                  the device count to it and to capacity_kept -- a stale or wrong count reads or copies less, never elsewhere
 *
 * Writes kept_rows / kept_idx at slots [old n_kept, new n_kept) only and touches no other byte of either; *n_kept_dev becomes the
 * new count.  m == 0 returns HMM_OK without a launch and without looking at a pointer.  HMM_E_INVALID, before anything is launched:
 * dim != 1024, a negative count, kept_bound > n_seen_before, kept_bound + m > capacity_kept, a null pointer, a row pointer or the
 * workspace not 16-byte aligned (kept_idx_dev / n_kept_dev: 8-byte), new rows that overlap the state, an m whose bitmap exceeds LDS (as hmm_gram_select refuses it).
 * HMM_E_WORKSPACE: workspace_bytes below hmm_keyframe_extend_workspace_bytes(m).  The workspace needs no initialisation and may be
 * reused across calls and sizes on one stream.  Launch-only: nothing is allocated, copied to the host or synchronised. */
size_t hmm_keyframe_extend_workspace_bytes(int m);
int    hmm_keyframe_extend(const float* new_rows_dev, int m, int dim, float threshold,
                           float* kept_rows_dev, int64_t* kept_idx_dev, int64_t capacity_kept,
                           int64_t* n_kept_dev,
                           int64_t n_seen_before,   /* host's exact count of rows given so far */
                           int64_t kept_bound,      /* host's upper bound on *n_kept_dev     */
                           void* workspace_dev, size_t workspace_bytes, hmm_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Perceptual encoder.  Replaces ImageBind._load_model / ImageBind.forward
 * (hippomm/models/foundation_models.py:31-35, :116-133), i.e. upstream
 * imagebind_huge's vision and audio towers (un-vendored third-party code; see
 * oracle/imagebind_oracle.py for the restated architecture).
 *
 * One handle per tower.  bf16 MFMA GEMMs with fp32 accumulation, fp32 residual stream,
 * fp32 LayerNorm / softmax statistics.
 * ---------------------------------------------------------------------------------------- */
typedef struct hmm_encoder hmm_encoder;

#define HMM_TOWER_VISION 0   /* (B,3,224,224) fp32 -> (B,1024) unit rows                   */
#define HMM_TOWER_AUDIO  1   /* (B,3,1,128,204) fp32 -> (B,1024) = mean_3clips(20 * unit)  */
#define HMM_TOWER_TEXT   2   /* (B,77) int64 CLIP-BPE token ids -> (B,1024) = exp(log_logit_scale) * unit
                                (the query side of feature_search, hippocampal_memory.py:2173-2176) */

/* depth <= 0 selects the imagebind_huge depth (32 vision / 12 audio); a smaller depth builds
 * the same tower with fewer blocks (used by CI-sized parity fixtures). */
int  hmm_encoder_create(hmm_encoder** out, int tower, int depth);
void hmm_encoder_destroy(hmm_encoder* enc);

/* Upload one parameter by its UPSTREAM state-dict key (e.g.
 * "modality_trunks.vision.blocks.7.attn.in_proj_weight").  data_dev is a DEVICE fp32 tensor
 * with the upstream shape, contiguous; the library packs it (bf16 cast, Conv3d temporal-tap
 * fold, ...) into its own storage on `stream`.  Unknown keys / wrong sizes fail. */
int  hmm_encoder_load_param(hmm_encoder* enc, const char* upstream_key,
                            const float* data_dev, int64_t numel, hmm_stream_t stream);
/* Number of parameters still missing (0 = ready); names via hmm_last_error() when > 0. */
int  hmm_encoder_missing_params(hmm_encoder* enc);

/* Workspace of a forward of `batch` samples.  Non-decreasing in `batch`: a workspace sized for the largest batch a caller will
 * ever pass serves every smaller one (the few-sample forwards keep fp32 split-K slabs that slightly larger batches do not). */
size_t hmm_encoder_workspace_bytes(const hmm_encoder* enc, int batch);
/* input_dev: vision (batch,3,224,224) fp32 | audio (batch,3,1,128,204) fp32 | text (batch,77) int64
 * out_dev:   (batch,1024) fp32
 * The kernels are chosen by the size of the call (the reference calls with one question, one audio segment, the frames of a
 * segment or a 32-frame buffer: hippocampal_memory.py:1180, :1222, :1328, :2173).  A sample's embedding does not depend on the
 * batch it arrives in WITHIN a regime, bit for bit; there are two: few-row forwards (batch x clips x tokens <= 300 rows for the
 * vision tower = one frame, <= 700 for audio / text = one segment, up to nine questions), whose fc2 is a deterministic split-K
 * launch reduced inside the next LayerNorm, and everything larger.  Across the boundary the embeddings agree to 1 - cos ~ 1e-5
 * (stated tolerance 5e-5). */
int  hmm_encoder_forward(hmm_encoder* enc, const void* input_dev, int batch, float* out_dev,
                         void* workspace_dev, size_t workspace_bytes, hmm_stream_t stream);
/* FLOPs (2 x MAC) of one forward of `batch` samples as the REFERENCE computes it (un-folded patch convolution, every
 * block on every token: SURVEY 8d's 334.98 GFLOP per vision frame) -- the figure roofline fractions are quoted on. */
double hmm_encoder_flops(const hmm_encoder* enc, int batch);
/* FLOPs this build actually executes for the same forward: temporal taps of the Conv3d folded into one K-padded matrix,
 * and the last block computed for the selected row only (vision / audio: K,V for every token, the rest for token 0). */
double hmm_encoder_flops_executed(const hmm_encoder* enc, int batch);
/* n_streams = 2 (default): from 13 frames / 4 audio segments (except 5-7, whose fused attention launch is one round of the chip) / 54 questions on, a forward runs as two half-batches, the second on a stream owned
 * by the handle (forked from / joined to the caller's stream with events).  n_streams = 1: one chain on the caller's
 * stream only.  Embeddings are bitwise identical either way (tests/test_gpu_encoder_batch.py). */
int  hmm_encoder_set_streams(hmm_encoder* enc, int n_streams);
/* Vision and audio towers: on (default) = in_proj and the attention core of a block run as ONE kernel per (sample, head)
 * and the packed qkv matrix never goes through HBM; off = a QKV GEMM followed by the attention kernel.  Embeddings are
 * bitwise identical either way.  No effect on the text tower (77 tokens would fill 30 % of the kernel's 256-row tile).
 * Forwards below 48 frames / 9 clips (three segments) use the two-kernel path regardless: the fused kernel is 16 (12) workgroups
 * per sample. */
int  hmm_encoder_set_fused_attention(hmm_encoder* enc, int on);

/* Text tower on PACKED rows: every question at its own length instead of 77 rows (opt-in; hmm_encoder_forward is untouched).
 * The tower is causal and the head reads only the row at the EOS position, so no row behind EOS can change the result; this
 * entry does not compute them.  len[b] = (first index of the largest id of row b) + 1, 1 <= len[b] <= 77: the EOS rule of
 * hmm_encoder_forward.  Sample b owns rows off[b] .. off[b] + len[b] - 1 of one dense [R][1024] residual stream, R = sum len.
 *   ids_dev       (batch,77) int64, as for hmm_encoder_forward; ids behind a row's length are never read; never written
 *   lengths_host  int32[batch] on the HOST: validated here (a length outside 1 .. 77: HMM_E_INVALID) and used for launch sizes,
 *                 the regime and the workspace layout; not read after the call returns
 *   offsets_dev   int32[batch + 1] on the DEVICE: the exclusive prefix sum of lengths_host, the total R behind it.  The library
 *                 derives the same table from lengths_host for its own sizes and never reads offsets_dev on the host (no
 *                 synchronisation); kernels read only offsets_dev.  A device table that differs from that prefix sum breaks a
 *                 precondition: the kernels skip every sample whose entry does not describe 1 .. 77 rows inside [0, R], so no
 *                 byte outside the documented extents is touched, but the embeddings of that call are undefined.
 *   Lengths that do not match the EOS positions of ids_dev are a precondition too, not checked: the embedding is then that
 *   of the row at len[b] - 1.
 *   out_dev       (batch,1024) fp32
 * Workspace: exactly hmm_encoder_text_packed_workspace_bytes(enc, batch, R), a function of (batch, R) alone (0 for a handle
 * that is not a text tower, batch < 1 or R outside batch .. 77 batch); fewer bytes are refused with HMM_E_WORKSPACE before
 * anything is written.  One chain on the caller's stream, no synchronisation, capturable.  Regime and GEMM dispatch follow the
 * rules of hmm_encoder_forward keyed by R (few-row regime: R <= 700); within a regime a question's embedding does not depend on
 * its position in the batch or on its batch-mates, bit for bit.  The last block computes Q, attention, out-proj and the MLP
 * for the EOS rows only.  Bits differ from hmm_encoder_forward's (other row counts, the one-query last block); both meet the
 * stated tolerance against the fp32 oracle. */
size_t hmm_encoder_text_packed_workspace_bytes(const hmm_encoder* enc, int batch, int64_t total_rows);
int  hmm_encoder_forward_text_packed(hmm_encoder* enc, const int64_t* ids_dev, const int32_t* lengths_host,
                                     const int32_t* offsets_dev, int batch, float* out_dev,
                                     void* workspace_dev, size_t workspace_bytes, hmm_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Device-side vision preprocessing.  Replaces, for already decoded frames, the transform chain of
 * imagebind.data.load_and_transform_vision_data (torchvision Resize(224, BICUBIC) -> CenterCrop(224) ->
 * ToTensor -> Normalize(CLIP mean/std) [upstream, recalled]) used at hippomm/models/foundation_models.py:87-90.
 * Bit-identical to Pillow's resize: two passes, 8-bit intermediate, 22-bit fixed-point coefficients computed by
 * the host (hippomm_amd/preprocess.py) for the 224 centre-cropped columns (kh/bh) and rows (kv/bv):
 *   k*_dev int32[224][ksize], b*_dev int32[224][2] = (first tap, tap count); rows [row_first,row_last) of the
 *   input are the ones the vertical taps touch.  frames_dev uint8 (batch,in_h,in_w,3) RGB; out (batch,3,224,224).
 * ---------------------------------------------------------------------------------------- */
size_t hmm_preprocess_vision_workspace_bytes(int batch, int rows_needed);
int    hmm_preprocess_vision_u8(const uint8_t* frames_dev, int batch, int in_h, int in_w,
                                const int32_t* kh_dev, const int32_t* bh_dev, int ksize_h,
                                const int32_t* kv_dev, const int32_t* bv_dev, int ksize_v,
                                int row_first, int row_last, float* out_dev,
                                void* workspace_dev, size_t workspace_bytes, hmm_stream_t stream);

/* Host-side hand-over of one frame decoded by Pillow to the (pinned) upload buffer of hmm_preprocess_vision_u8 -- the step
 * between Image.open(path).convert("RGB") and the transform chain in imagebind.data.load_and_transform_vision_data [upstream,
 * recalled] (hippomm/models/foundation_models.py:87-90).  No GPU call.  Pillow stores RGB as 4 bytes per pixel (R,G,B,pad);
 * src_rgbx: n_pixels * 4 bytes; dst_rgb: n_pixels * 3 bytes, nothing beyond them is written.  The _arrow_ form takes the
 * `struct ArrowArray*` inside the "arrow_array" capsule of Image.__arrow_c_array__() (Arrow C data interface:
 * fixed_size_list<uint8>[4] with width * height entries; HMM_E_INVALID on any other layout) and copies the window
 * [y0, y0 + roi_h) x [x0, x0 + roi_w) as a dense (roi_h, roi_w, 3) block: only the pixels the centre crop's resampling taps
 * touch have to cross PCIe (57 % of a 1280x720 frame).  Called through ctypes these run without the interpreter lock, which
 * is what lets the decode threads of hippomm_amd/preprocess.py scale. */
int hmm_host_rgbx_to_rgb(const uint8_t* src_rgbx, size_t n_pixels, uint8_t* dst_rgb);
int hmm_host_arrow_rgbx_to_rgb(const void* arrow_array, int width, int height, int x0, int y0, int roi_w, int roi_h,
                               uint8_t* dst_rgb);

/* ------------------------------------------------------------------------------------------
 * Device-side audio front end.  Replaces waveform2melspec + Normalize inside
 * imagebind.data.load_and_transform_audio_data [upstream, recalled] as called at
 * hippomm/models/foundation_models.py:106-109: per clip, `waveform -= waveform.mean()`, then
 * torchaudio.compliance.kaldi.fbank(htk_compat=True, sample_frequency=16000, use_energy=False, window_type="hanning",
 * num_mel_bins=128, dither=0.0, frame_length=25, frame_shift=10), transposed to (128, frames), zero-padded / cut to
 * 204 frames, then (x - mean) / std.  clips_dev: n_clips mono fp32 clips at 16 kHz, clip c at clips_dev + c*clip_stride,
 * clip_len samples each (2 s = 32000 in the reference).  out_dev: (n_clips, 128, 204) fp32, i.e. the (B,3,1,128,204)
 * tensor the audio tower takes when n_clips = 3*B.  Clip selection (3 clips spread over the segment) is host logic.
 * window_dev (400 floats: torch.hann_window(400, periodic=False)) and mel_banks_dev (128 x 257 floats: kaldi
 * get_mel_banks(128, 512, 16000, 20, 0) plus one zero column) may be null, in which case the library generates them on
 * the device from the same formulas; pass tables computed on the host to reproduce torchaudio's weights to the bit.
 * ---------------------------------------------------------------------------------------- */
size_t hmm_audio_fbank_workspace_bytes(int n_clips);
int    hmm_audio_fbank(const float* clips_dev, int n_clips, int clip_len, int64_t clip_stride,
                       const float* window_dev, const float* mel_banks_dev,
                       float norm_mean, float norm_std, float* out_dev,
                       void* workspace_dev, size_t workspace_bytes, hmm_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The audio track of a video on the device: all segments of process_sequence in one call.  Replaces, per segment, the slice,
 * `audio_data.mean(axis=1)` (done once on the host for C > 1), `.astype(np.float32)`, the peak normalisation, the temporary wav
 * (hippomm/core/hippocampal_memory.py:1198-1251; :1206, :1212, :1215-1216, :1219) and, inside
 * imagebind.data.load_and_transform_audio_data [upstream, recalled] (hippomm/models/foundation_models.py:106-109), the
 * torchaudio resampling of a file that is not at 16 kHz and the cut into three clips.  The result is the clip batch
 * hmm_audio_fbank takes.
 *
 * track_dev: the mono track, track_len samples, fp32 (track_dtype 0) or fp64 (1: narrowed on the fly with round-to-nearest-even,
 * the bits of astype(float32)); 16-byte aligned.  Every table is given twice: *_host is what the entry point checks before it
 * launches anything (a host pointer, read during the call only), *_dev the same table on the device, which the kernel reads --
 * and clamps to the track, so a device copy that differs reads and writes less, never elsewhere.
 *
 * hmm_audio_span_peaks: spans: n_spans x (start, end) int64, 0 <= start <= end <= track_len.  peaks_out_dev[s] = max |x| over the
 *   narrowed samples of span s, NaN when the span holds a NaN (np.abs(x).max()), 0 for an empty span.
 * hmm_audio_gather_clips: clips: n_clips x (span start, span length, first output sample, span index) int64; peaks_dev[n_spans]
 *   from hmm_audio_span_peaks.  A sample of a span with peak p > 1.0f is x / p (one correctly rounded fp32 division), else x
 *   as it is (p == 1 and a NaN p do not scale).  orig == new (the rate divided by its gcd with 16000, and 16000 divided by it):
 *   clips_out_dev[c][i] = sample first + i of the span, bit-exact; taps_dev may be null.  Otherwise the span is resampled as a
 *   file of its own, torchaudio.functional.resample's polyphase windowed sinc:
 *       out[j] = sum_t taps[j % new][t] * x[(j / new) * orig - width + t],   x = 0 outside [0, span length),
 *   ceil(new * length / orig) output samples, of which clips_out_dev[c][i] is j = first + i.  taps_dev is TAP-MAJOR:
 *   (2 * width + orig, new) floats, taps_dev[t * new + phase].  fp32 fused multiply-adds into four partial sums (t mod 4) added as
 *   (a0 + a1) + (a2 + a3): within (T + 2) 2^-24 sum_t |taps_t x_t| of the exact sum, and the same bits whatever else is in the
 *   batch.  first + clip_len may not exceed the span's output length; the window of one workgroup,
 *   (255 / new + 2) * orig + 2 * width samples, must fit 64 KiB of LDS (HMM_E_INVALID otherwise).  clips_out_dev: (n_clips,
 *   clip_len) fp32, contiguous, not overlapping the track.  Zero n_spans / n_clips / clip_len: HMM_OK, nothing is launched.
 * ---------------------------------------------------------------------------------------- */
int hmm_audio_span_peaks(const void* track_dev, int track_dtype, int64_t track_len, const int64_t* spans_host,
                         const int64_t* spans_dev, int n_spans, float* peaks_out_dev, hmm_stream_t stream);
int hmm_audio_gather_clips(const void* track_dev, int track_dtype, int64_t track_len, const int64_t* clips_host,
                           const int64_t* clips_dev, int n_clips, const float* peaks_dev, int n_spans, int clip_len,
                           int orig, int new_, int width, const float* taps_dev, float* clips_out_dev, hmm_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The audio-level scan of _segment_sequence (hippomm/core/hippocampal_memory.py:993-1000, :1061-1077) on the same track: the sum
 * of squares of every 500 ms window of a walk step in one launch, in numpy's order, so that the host forms the reference's level
 * bit for bit from it: mean = T(sum / n), rms = sqrt(mean), 20 * log10(rms) if rms > 0 else -100.
 *
 * hmm_audio_window_sums: windows: n_windows x (start, length) int64, start >= 0, length >= 0, start + length <= track_len; given
 *   twice like the tables above (the host copy is checked before anything is launched; the kernel reads the device copy and clamps
 *   it to the track).  sums_out_dev[w], in the track's dtype T (fp32 or fp64; aligned to it, not overlapping the track), is
 *   np.sum(np.square(x[start : start + length])) as np.mean evaluates it on a contiguous window: s_i = x_i * x_i rounded to T (a
 *   multiply and a separate add, never fused); consecutive chunks of 8192 squares summed left to right; a chunk of m squares by
 *   pairwise summation -- m < 8 a running sum from 0; m <= 128 eight accumulators r_j over elements 8 i + j combined as
 *   ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the m % 8 tail elements one by one; otherwise split at (m / 2) - (m / 2) % 8 and add
 *   the halves.  0 for an empty window, NaN for one that holds a NaN.  The order depends on the window's length alone: the same
 *   window gives the same bits alone, in any batch and on every run.  No workspace, no synchronisation, no allocation;
 *   n_windows == 0: HMM_OK, nothing is launched.
 * ---------------------------------------------------------------------------------------- */
int hmm_audio_window_sums(const void* track_dev, int track_dtype, int64_t track_len, const int64_t* windows_host,
                          const int64_t* windows_dev, int n_windows, void* sums_out_dev, hmm_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The same track as the 16-bit samples of the extracted WAV (ffmpeg's 16 kHz mono pcm_s16le file, hippomm/core/batch_process.py:280-339):
 * track_dev holds track_len int16 samples, 16-byte aligned, 2 bytes per sample where the fp64 track of np.load(audio.npy) holds 8.
 * The value of sample x is x / 32768 -- what sf.read makes of such a file (libsndfile pcm.c, default normalisation) -- and every
 * output below carries, bit for bit, what the entry point above gives on the fp64 track (double)x / 32768.0 (track_dtype 1):
 *   - x / 32768 is exact in fp64 and has at most 16 significant bits, so narrowing it to fp32 is exact too: (float)x * 2^-15;
 *   - |x / 32768| <= 1 (-32768 gives exactly 1.0 and 1.0f > 1.0f is false): no span is ever scaled, there is no peak pass;
 *   - a square is an integer <= 2^30 times 2^-30, so over a window of at most 2^22 samples every partial sum, in any order, is an
 *     integer <= 2^52 times 2^-30 -- exactly representable: numpy's pairwise sum never rounds, and any order gives its bits.
 * Tables are given twice as above (host copy checked, device copy read by the kernel and clamped to the track).
 *
 * hmm_audio_pcm16_gather_clips: hmm_audio_gather_clips without peaks.  clips: n_clips x (span start, span length, first output
 *   sample, span index) int64 -- the same table; the span index is not looked at.  orig == new: clips_out_dev[c][i] = sample
 *   first + i of the span as (float)x * 2^-15; 16-byte loads of eight samples where the clip's samples fill an aligned group,
 *   element loads before and behind; nothing outside the clip's samples is read.  Otherwise the resampling above on those floats:
 *   the same window, the same order of fused multiply-adds, the same bits.  The same refusals (no track_dtype, no peaks); the
 *   output may not overlap the track's 2 * track_len bytes.
 * hmm_audio_pcm16_window_sums: sums_out_dev[w] fp64 = sum of (x / 32768)^2 over window w, exact (accumulated in integers, scaled by
 *   2^-30 once); 0 for an empty window.  A host window longer than 2^22 samples is HMM_E_INVALID before anything is launched; the
 *   device copy is clamped to that length as well.  Otherwise the refusals of hmm_audio_window_sums.
 * ---------------------------------------------------------------------------------------- */
int hmm_audio_pcm16_gather_clips(const void* track_dev, int64_t track_len, const int64_t* clips_host, const int64_t* clips_dev,
                                 int n_clips, int clip_len, int orig, int new_, int width, const float* taps_dev,
                                 float* clips_out_dev, hmm_stream_t stream);
int hmm_audio_pcm16_window_sums(const void* track_dev, int64_t track_len, const int64_t* windows_host, const int64_t* windows_dev,
                                int n_windows, double* sums_out_dev, hmm_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Frame SSIM (structural similarity) for sequence segmentation and frame differences.  Replaces skimage 0.18.3
 * structural_similarity as hippomm/core/hippocampal_memory.py:980-991 (_compute_frame_similarity, consulted by
 * _segment_sequence :1002-1114) and hippomm/core/batch_process.py:32-69 (compute_frame_difference) call it on gray frames.
 *
 * hmm_gray_u8: frames_dev (n, H, W, 3) u8 interleaved -> gray_out_dev (n, H, W) u8 by OpenCV's 8-bit BGR2GRAY rule,
 *   g = (1868 B + 9617 G + 4899 R + 8192) >> 14, and minmax_out_dev int32[n][2] = (min, max) of each gray frame.
 *   channel_order: HMM_GRAY_FROM_RGB / _BGR give the byte order of the input; HMM_GRAY_FROM_GRAY takes frames_dev as
 *   (n, H, W) gray frames and only writes minmax_out_dev (gray_out_dev may be null).  n <= 65535.
 *
 * hmm_ssim_pairs: scores_out_dev[p] = SSIM(gray[a_p], gray[b_p]) in fp64 for pairs_host[p] = (a_p, b_p), a HOST int32 array
 *   of n_pairs pairs (validated, then passed to the kernels by value: nothing is copied, the call stays capturable).  a plays
 *   skimage's im1.  gray_dev (n_frames, H, W) u8.  data_range >= 0: R = data_range (data_range=1.0 on frames / 255 is R = 255
 *   here); data_range < 0: R = max(a) - min(a) from minmax_dev (hmm_gray_u8's output for the same frames).
 *   Arithmetic: the five 7x7 box sums of the (H-6) x (W-6) window positions inside the image, exact in int32; then in fp64
 *   ux = sum_x / 49 (and likewise uy, uxx, uyy, uxy), v* = 49/48 (u** - u* u*), C1 = (0.01 R)^2, C2 = (0.03 R)^2,
 *   S = ((2 ux uy + C1)(2 vxy + C2)) / ((ux^2 + uy^2 + C1)(vx + vy + C2)), score = fixed-order fp64 sum of S / count.  No
 *   float atomics: a rerun gives the same bits, and a pair's score does not depend on the other pairs of the call.  R = 0 and a
 *   flat frame give NaN, as in skimage.  H < 7 or W < 7 is refused (skimage: "win_size exceeds image extent").
 * ---------------------------------------------------------------------------------------- */
#define HMM_GRAY_FROM_RGB   0
#define HMM_GRAY_FROM_BGR   1
#define HMM_GRAY_FROM_GRAY  2
int    hmm_gray_u8(const uint8_t* frames_dev, int n, int H, int W, int channel_order, uint8_t* gray_out_dev,
                   int32_t* minmax_out_dev, hmm_stream_t stream);
size_t hmm_ssim_pairs_workspace_bytes(int H, int W, int n_pairs);
int    hmm_ssim_pairs(const uint8_t* gray_dev, int n_frames, int H, int W, const int32_t* pairs_host, int n_pairs,
                      double data_range, const int32_t* minmax_dev, double* scores_out_dev,
                      void* workspace_dev, size_t workspace_bytes, hmm_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The decision loop of extract_frames_from_video (hippomm/core/batch_process.py:179-228) with its state on the device: the last
 * saved frame (the anchor), the running cumulative difference and the time of the last save.
 *
 * Slots: gray_slots_dev is (n_slots, H, W) u8, owned by the caller.  Slot 0 holds the anchor carried over from the previous call,
 * slots 1 .. n_slots - 1 this batch's candidates (hmm_gray_u8 fills them in one launch).  hmm_extract_state is the whole state; the
 * caller creates it zeroed (no anchor), may copy it out and back to snapshot and restore it, and never needs to look inside between
 * calls.
 *
 * hmm_extract_walk: for the candidates in slots first_slot .. first_slot + count - 1, in order, with times_host[i], check_host[i] and
 *   deny_host[i] (HOST arrays of count entries, passed to the kernels by value) for the candidate in slot first_slot + i:
 *     compared = has_anchor && check_i && (time_i - last_save_time >= min_gap)
 *     compared:    diff = 1.0 - SSIM(candidate, gray[anchor_slot]) with R = 255, the candidate in skimage's im1 role -- bit for
 *                  bit 1.0 - hmm_ssim_pairs' score of that pair --, cumulative_diff += diff,
 *                  save = diff > max_diff_threshold || cumulative_diff > max_diff_threshold
 *     no anchor:   save = true without a comparison;  otherwise save = false, diff = 0
 *     save && !deny_i:  anchor_slot = the candidate's slot, has_anchor = 1, last_save_time = time_i, cumulative_diff = 0
 *     a denied save leaves the four as they are (the reference when save_frame returns False).
 *   records_out_dev[i] describes candidate i and the state after it; only records_out_dev[0 .. count) is written.  Two launches per
 *   candidate on `stream`, which must execute in order; no host synchronisation, no workgroup waits for another one.  The anchor slot
 *   is the only index read from device memory and is clamped to [0, n_slots) before use.  The inputs are not written.
 *   HMM_E_INVALID before anything is launched (no GPU needed): a null pointer, H or W under 7, n_slots < 2, count < 1,
 *   first_slot < 1 or first_slot + count > n_slots, state / records / workspace not 8-byte aligned, a time that is not finite,
 *   max_diff_threshold or min_gap NaN.  HMM_E_WORKSPACE: workspace_bytes below hmm_extract_walk_workspace_bytes(H, W).
 *
 * hmm_extract_carry: gray[0] = gray[anchor_slot] and anchor_slot = 0, the indirection on the device with the same clamp; nothing
 *   happens without an anchor or with the anchor in slot 0 already.  Afterwards slots 1 .. may be overwritten with the next batch.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int32_t has_anchor;
    int32_t anchor_slot;
    double  cumulative_diff;
    double  last_save_time;
} hmm_extract_state;

typedef struct {
    int32_t compared;               /* 1: the candidate was scored against the anchor */
    int32_t saved;                  /* 1: the candidate became the anchor (save && !deny) */
    int32_t anchor_slot_after;
    int32_t has_anchor_after;
    double  diff;                   /* 0 where nothing was compared */
    double  cumulative_after;
    double  last_save_time_after;
} hmm_extract_record;

size_t hmm_extract_walk_workspace_bytes(int H, int W);
int    hmm_extract_walk(const uint8_t* gray_slots_dev, int n_slots, int H, int W, int first_slot, int count,
                        const double* times_host, const int32_t* check_host, const int32_t* deny_host,
                        double max_diff_threshold, double min_gap, hmm_extract_state* state_dev,
                        hmm_extract_record* records_out_dev, void* workspace_dev, size_t workspace_bytes, hmm_stream_t stream);
int    hmm_extract_carry(uint8_t* gray_slots_dev, int n_slots, int H, int W, hmm_extract_state* state_dev, hmm_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The window walk of _segment_sequence (hippomm/core/hippocampal_memory.py:1002-1114) with its control loop on the device: the
 * adjacent-pair SSIM scores, the frame times and the audio track are resident, the segment list is the only thing read back.
 *
 * hmm_segment_walk: scores_dev fp64 [n_frames - 1], scores_dev[i] = SSIM(frame i + 1, frame i) (hmm_ssim_pairs, the later frame in
 *   skimage's im1 role); flags_dev int32 [n_frames - 1], non-zero where pair i could not be scored (its score is then never read);
 *   times_dev fp64 [n_frames] with the HOST copy times_host, validated finite and non-decreasing.  n_frames == 0: no video (the three
 *   device pointers and times_host may be null; so may scores_dev and flags_dev when n_frames == 1).  track_dev null: no audio; otherwise
 *   the track of hmm_audio_window_sums (track_dtype 0 fp32 / 1 fp64, track_len samples, 16-byte aligned) at the integer sample_rate,
 *   with window = (int64)(0.5 * sample_rate) >= 1.  All arithmetic on times is fp64, operation by operation what the Python floats of
 *   the reference do.  From current_start = 0.0, while current_start < total_duration, one step:
 *     1. current_end = min(current_start + max_segment_duration, total_duration); optimal_end = current_end.
 *     2. the frames with current_start <= t <= current_end are a contiguous index range [first, last].
 *     3. for k = last down to first + 1, pair k - 1: flagged -> the walk stops (status HMM_SEGMENT_WALK_FLAGGED, flagged_pair = k - 1,
 *        no record for this step); scores_dev[k - 1] < frame_similarity_threshold -> optimal_end = t[k], stop reading.  NaN never cuts.
 *     4. S = (int64)(current_start * sample_rate), E = (int64)(current_end * sample_rate); for off = E - S - window, E - S - 2 window,
 *        ... > 0 the window [lo, lo + window), lo = S + off, clipped to the track as a numpy slice would be (n samples, maybe 0):
 *        sum of squares in the track's dtype T by the kernel of hmm_audio_window_sums; mean = T(sum / n) (the division in fp64,
 *        rounded to fp32 for an fp32 track; 0 / 0 = NaN); rms = sqrt(mean) in T, correctly rounded;
 *        silent = rms > 0 ? rms < rms_cut : silent_without_rms.  The first silent window sets optimal_end = lo / sample_rate (it
 *        overrides step 3's) and ends the scan.  rms_cut is the caller's: the least value of T whose level 20 log10(rms) is not
 *        below the silence threshold under the caller's own log10; silent_without_rms is (-100 < threshold).
 *     5. optimal_end - current_start < min_segment_duration -> optimal_end = min(current_start + min_segment_duration, total_duration).
 *     6. records_out_dev[n_segments++] = the step; current_start = optimal_end.
 *   state_out_dev is written by the call (no need to initialise it): status HMM_SEGMENT_WALK_DONE when the loop condition failed,
 *   _FLAGGED as above, _BOUND when max_steps steps did not finish (or a step had more than max_windows windows): the records
 *   written so far are valid and current_start is where the walk stood.  Only records_out_dev[0 .. n_segments) and the state are
 *   written.  Launches, all on `stream`, which must execute in order; no host synchronisation, no workgroup waits for another:
 *   without audio one launch for the whole walk; with audio one planning launch (the window table of step 0, in the workspace), then
 *   per step one launch of the window sums over max_windows table rows and one decide launch that also writes the next step's
 *   table -- all lengths 0 once the walk has ended, so the remaining launches return at once.  2 max_steps + 1 launches.  Every
 *   index formed from device memory (frame indices out of times_dev, n_segments) is clamped to its array before use; the inputs are
 *   not written.
 *   HMM_E_INVALID before anything is launched (no GPU needed): a null pointer; n_frames < 0; times_host not finite or decreasing;
 *   a parameter that is NaN or not finite; min_segment_duration <= 0; max_steps < 1 or max_windows < 0; with audio track_dtype not 0 / 1,
 *   sample_rate < 2, track_len < 0, max_windows < 1, or total_duration * sample_rate at or above 2^52; records / state / workspace /
 *   scores / times not 8-byte aligned, flags not 4-byte aligned, the track not 16-byte aligned.  HMM_E_WORKSPACE: workspace_bytes below
 *   hmm_segment_walk_workspace_bytes(max_windows, max_steps) (0 without audio: max_windows == 0, and workspace_dev may then be null).
 * ---------------------------------------------------------------------------------------- */
#define HMM_SEGMENT_WALK_RUNNING  0            /* never left behind by a call */
#define HMM_SEGMENT_WALK_DONE     1
#define HMM_SEGMENT_WALK_FLAGGED  2
#define HMM_SEGMENT_WALK_BOUND    3

typedef struct {
    double  start_time;
    double  end_time;
    int32_t first_frame;            /* frames first_frame .. last_frame have start_time <= t <= end_time; none: last_frame = first_frame - 1 */
    int32_t last_frame;
    int32_t cut_pair;               /* the pair whose score cut the window in step 3 (even if step 4 or 5 then moved the end), or -1 */
    int32_t cut_window;             /* the window of step 4 that was silent, counted from the end of the step (0: the last), or -1 */
    int32_t pairs_consulted;
    int32_t windows_consulted;
} hmm_segment_record;

typedef struct {
    int32_t n_segments;
    int32_t status;                 /* HMM_SEGMENT_WALK_* */
    int32_t flagged_pair;           /* the pair that stopped the walk (status _FLAGGED), else -1 */
    int32_t steps;                  /* steps taken, the unfinished one of a _FLAGGED walk included */
    double  current_start;
} hmm_segment_walk_state;

size_t hmm_segment_walk_workspace_bytes(int max_windows, int max_steps);
int    hmm_segment_walk(const double* scores_dev, const int32_t* flags_dev, const double* times_dev, const double* times_host,
                        int n_frames, const void* track_dev, int track_dtype, int64_t track_len, int sample_rate,
                        double total_duration, double max_segment_duration, double min_segment_duration,
                        double frame_similarity_threshold, double rms_cut, int silent_without_rms, int max_windows, int max_steps,
                        hmm_segment_record* records_out_dev, hmm_segment_walk_state* state_out_dev, void* workspace_dev,
                        size_t workspace_bytes, hmm_stream_t stream);
/* hmm_segment_walk_pcm16: hmm_segment_walk over the 16-bit track of hmm_audio_pcm16_window_sums (track_dev int16, no track_dtype): the
 *   same walk, one implementation; a window's sum is that entry point's (fp64, exact), mean and rms are formed as for an fp64 track, so
 *   rms_cut is the fp64 one.  The same workspace size, launches and refusals, and two more: window = (int64)(0.5 * sample_rate)
 *   above 2^22, and records, state or workspace overlapping the track's bytes. */
int    hmm_segment_walk_pcm16(const double* scores_dev, const int32_t* flags_dev, const double* times_dev, const double* times_host,
                              int n_frames, const void* track_dev, int64_t track_len, int sample_rate, double total_duration,
                              double max_segment_duration, double min_segment_duration, double frame_similarity_threshold,
                              double rms_cut, int silent_without_rms, int max_windows, int max_steps,
                              hmm_segment_record* records_out_dev, hmm_segment_walk_state* state_out_dev, void* workspace_dev,
                              size_t workspace_bytes, hmm_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * cv2.resize of 8-bit frames to a target no larger than the source, as the reference shrinks every recalled frame
 * (hippomm/core/hippocampal_memory.py:2232, :2795: cv2.resize(frame, (320, 180))).  The arithmetic is OpenCV's 8-bit INTER_LINEAR,
 * restated from its published source (imgproc/src/resize.cpp); a build that routes 8-bit resize through another back end may differ.
 *
 * hmm_resize_linear_u8: src_dev (n, src_h, src_w, channels) u8 dense -> dst_dev (n, dst_h, dst_w, channels) u8 dense; channels 1
 *   or 3; dst_h <= src_h and dst_w <= src_w (an enlargement is HMM_E_INVALID: OpenCV's border rules there are not built).
 *   mode HMM_RESIZE_LINEAR: xofs_dev int32[dst_w] and yofs_dev int32[dst_h] are the first of the two source indices of an output
 *     index, xcoef_dev int16[dst_w][2] and ycoef_dev int16[dst_h][2] its weights on the 2048 scale (for output index d at scale
 *     src / dst in double: f = (float)((d + 0.5) * scale - 0.5), s = floor(f), f -= s in float, weights (short)rint((1.f - f) * 2048)
 *     and (short)rint(f * 2048), half to even; a pair need not sum to 2048).  Per channel, in int32:
 *       h = S[s] * a0 + S[s + 1] * a1 along x (S[s] * 2048 where s + 1 would leave the row), for the rows sy and sy + 1, then
 *       d = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2.
 *     Offsets are clamped to the frame: a wrong table gives wrong pixels, never a read outside src_dev.
 *   mode HMM_RESIZE_AREA2X (src exactly twice dst on both axes, where OpenCV turns INTER_LINEAR into its 2 x 2 area path):
 *     d = (s00 + s01 + s10 + s11 + 2) >> 2; the tables are not read and may be null.
 *   One launch for all n frames (n <= 65535; n == 0: HMM_OK, nothing launched); no workspace, no allocation, no
 *   synchronisation.  Offsets aligned to 4 bytes, coefficients to 2.
 * ---------------------------------------------------------------------------------------- */
#define HMM_RESIZE_LINEAR  0
#define HMM_RESIZE_AREA2X  1
int hmm_resize_linear_u8(const uint8_t* src_dev, int n, int src_h, int src_w, int channels, uint8_t* dst_dev, int dst_h, int dst_w,
                         const int32_t* xofs_dev, const int16_t* xcoef_dev, const int32_t* yofs_dev, const int16_t* ycoef_dev,
                         int mode, hmm_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Baseline JPEG decoding, split between host and GPU.  Replaces the libjpeg decode inside Image.open(path).convert("RGB") of
 * imagebind.data.load_and_transform_vision_data [upstream, recalled] (hippomm/models/foundation_models.py:87-90) and of the
 * frame reads of _segment_sequence (hippomm/core/hippocampal_memory.py:1002-1114), with Pillow's pixels to the bit: libjpeg-turbo's
 * defaults (islow IDCT, fancy upsampling, its fixed-point YCbCr -> RGB).
 *
 * Supported: 8-bit Huffman sequential (SOF0 / SOF1) files with one interleaved scan of one component (grey) or three (YCbCr;
 * not Adobe, not component ids R, G, B) with luma sampling 1x1, 2x1 or 2x2 and chroma 1x1; restart intervals.  Everything else,
 * and every anomaly in the data, is HMM_JPEG_UNSUPPORTED: the caller decodes such a file with Pillow.
 *
 * geometry: int32[HMM_JPEG_GEOMETRY_INTS] = (width, height, components, luma h sampling, luma v sampling, restart interval);
 *   sampling is 1 x 1 for grey.  The first five define the coefficient layout; frames that share them share slots.
 * hmm_jpeg_parse: markers only -> HMM_JPEG_DECODED (geometry filled) or HMM_JPEG_UNSUPPORTED.  Host, no GPU call.
 * hmm_jpeg_slot_bytes: bytes of one coefficient slot for frames of `geometry` cut to the window [x0, x0 + w) x [y0, y0 + h)
 *   (the blocks the window and the upsampling halo touch, plus the quantisation tables; a multiple of 256); 0 for a bad window.
 * hmm_jpeg_decode_coefs: the entropy pass of one file into a host slot -> HMM_JPEG_DECODED; HMM_JPEG_OTHER_GEOMETRY (a supported
 *   file whose first five geometry values differ); HMM_JPEG_UNSUPPORTED; HMM_E_* for bad arguments.  Host, no GPU call, no
 *   interpreter state: safe on any number of threads.
 * hmm_jpeg_reconstruct: n slots at slots_dev + i * slot_stride (device) -> rgb_out_dev (n, h, w, 3) u8, the window of each frame;
 *   grey frames come out with R = G = B.  Two kernels (dequantise + IDCT into u8 planes in the workspace; upsample + colour) on
 *   `stream`; no synchronisation, no allocation.
 * ---------------------------------------------------------------------------------------- */
#define HMM_JPEG_GEOMETRY_INTS   6
#define HMM_JPEG_DECODED         0
#define HMM_JPEG_UNSUPPORTED     1
#define HMM_JPEG_OTHER_GEOMETRY  2
int     hmm_jpeg_parse(const uint8_t* data, size_t n, int32_t* geometry);
int64_t hmm_jpeg_slot_bytes(const int32_t* geometry, int x0, int y0, int w, int h);
int     hmm_jpeg_decode_coefs(const uint8_t* data, size_t n, const int32_t* geometry, int x0, int y0, int w, int h, void* slot,
                              size_t slot_bytes);
size_t  hmm_jpeg_workspace_bytes(const int32_t* geometry, int n, int x0, int y0, int w, int h);
int     hmm_jpeg_reconstruct(const void* slots_dev, int n, size_t slot_stride, const int32_t* geometry, int x0, int y0, int w, int h,
                             uint8_t* rgb_out_dev, void* workspace_dev, size_t workspace_bytes, hmm_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The entropy (Huffman) pass of the same files on the GPU: an opt-in replacement of hmm_jpeg_decode_coefs that fills the same
 * coefficient slots, byte for byte, in device memory.  hmm_jpeg_reconstruct and everything after it are unchanged.
 *
 * hmm_jpeg_entropy_slot_bytes: bytes of a bitstream slot for a file of file_bytes bytes (the file size plus a constant, a
 *   multiple of 256).
 * hmm_jpeg_prepare_entropy: marker parse, then the scan's entropy bytes without FF 00 stuffing, the quantisation tables and up to
 *   four Huffman tables into `slot` (host memory, 16-byte aligned; pinned if it is to be uploaded asynchronously).  Host, no GPU
 *   call, no interpreter state.  -> HMM_JPEG_DECODED (the slot is ready), HMM_JPEG_OTHER_GEOMETRY, or HMM_JPEG_UNSUPPORTED, which
 *   here means "not by this route": everything hmm_jpeg_parse refuses, files with a restart interval, files whose components
 *   select more than four distinct Huffman tables, and scans that do not run up to an EOI marker (FF D9) with no other marker
 *   between.  HMM_E_WORKSPACE when slot_bytes is too small, HMM_E_INVALID for bad arguments.
 * hmm_jpeg_entropy_workspace_bytes: workspace of a call with n frames of `geometry` whose bitstream slots are max_entropy_bytes
 *   apart at the most (pass the bitslot stride); 0 for a bad geometry or n < 1.  Calls with more than 32 frames are run in
 *   chunks of 32 inside the call, so the size stops growing there.
 * hmm_jpeg_decode_coefs_device: n bitstream slots at bitslots_dev + i * bitslot_stride -> coefficient slots at coef_slots_dev +
 *   i * coef_slot_stride for the window, and status_dev[i] = (status, rounds): status HMM_JPEG_DECODED or HMM_JPEG_UNSUPPORTED,
 *   rounds the number of fixed-point rounds the frame took.  For status HMM_JPEG_DECODED the slot holds exactly the
 *   hmm_jpeg_slot_bytes bytes hmm_jpeg_decode_coefs writes for the same file and window (quantisation header, kept blocks) with
 *   zero padding; for any other status its contents are unspecified and must not be used -- decode that file with
 *   hmm_jpeg_decode_coefs, and with Pillow if that refuses too.  Every refusal of the host pass is made here over all blocks:
 *   an invalid code, an index past 63, |v| q > 32767, a DC predictor outside int16, a column of dequantised magnitudes above
 *   5800, a bit taken from past the end of the data, 8 or more unused bits at the end.
 *   The stream is cut into subsequences of 1024 bits that are decoded in parallel from guessed entry states and re-decoded until
 *   every exit state equals the next entry state; the loop is bounded by subsequences + 1 rounds, the proven bound, so no frame
 *   is refused for taking long.  Caller-owned memory, the caller's stream, no synchronisation, no allocation; the workspace
 *   needs no initialisation; all pointers 16-byte aligned (status_dev: 4), both strides multiples of 16; n = 0 is HMM_OK
 *   without a launch; HMM_E_WORKSPACE when workspace_bytes is below hmm_jpeg_entropy_workspace_bytes(geometry, n, bitslot_stride).
 * ---------------------------------------------------------------------------------------- */
int64_t hmm_jpeg_entropy_slot_bytes(size_t file_bytes);
int     hmm_jpeg_prepare_entropy(const uint8_t* data, size_t n, const int32_t* geometry, void* slot, size_t slot_bytes);
size_t  hmm_jpeg_entropy_workspace_bytes(const int32_t* geometry, int n, size_t max_entropy_bytes);
int     hmm_jpeg_decode_coefs_device(const void* bitslots_dev, int n, size_t bitslot_stride, const int32_t* geometry, int x0, int y0,
                                     int w, int h, void* coef_slots_dev, size_t coef_slot_stride, int32_t* status_dev,
                                     void* workspace_dev, size_t workspace_bytes, hmm_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Baseline JPEG encoding on the GPU.  Replaces the libjpeg encode inside cv2.imwrite(frame_path, frame) of save_frame
 * (batch_process.py:202-218), called by extract_frames_from_video (batch_process.py:73-114) for every frame it keeps.  The file
 * is, byte for byte, what Pillow's Image.fromarray(rgb).save(buf, "JPEG", quality=q, subsampling=s) writes ("L" mode for grey):
 * libjpeg's defaults -- the standard tables scaled by jpeg_quality_scaling with force_baseline, the standard Huffman tables, islow
 * forward DCT, one interleaved scan, no restart markers, JFIF 1.01 with density 1 x 1.  Equality with OpenCV's own file is not claimed.
 *
 * geometry: int32[HMM_JPEG_GEOMETRY_INTS] as above = (width, height, components 1 or 3, luma h sampling, luma v sampling, unused):
 *   sides of 1..65535; sampling 1x1 (4:4:4), 2x1 (4:2:2) or 2x2 (4:2:0), ignored for grey; at most 2^32 / 1660 blocks a frame.
 * hmm_jpeg_encode_header: host only, no GPU call.  Writes the bytes FF D8 .. SOS of every file of `geometry` at `quality` (1..100)
 *   into header_out (header_capacity bytes of room; 623 are written for colour, 328 for grey) and the two quantisation tables,
 *   natural order, into qtables_out (uint16[2][64]) -> the number of header bytes, or HMM_E_INVALID.
 * hmm_jpeg_encode_workspace_bytes: workspace of a call with n frames of `geometry`; 0 for a bad geometry or n < 1.
 * hmm_jpeg_encode_bound: an upper bound on the bytes of one file of `geometry`, proven in jpeg_layout.h (kJpegMaxBlockBits): no
 *   block takes more than 22 + 63 * 26 bits, stuffing at most doubles the scan; 0 for a bad geometry.
 * hmm_jpeg_encode: n frames at frames_dev, packed (n, height, width, channels) u8 with channels = components, channel_order
 *   HMM_JPEG_ORDER_RGB or _BGR (ignored for grey) -> the complete file of frame i at out_dev + i * out_stride and status_dev[i] =
 *   (status, bytes): HMM_JPEG_ENCODED and the file's length, or HMM_JPEG_ENCODE_OVERFLOW and the length it would have had when
 *   that exceeds out_stride.  On overflow nothing at or beyond out_dev + (i + 1) * out_stride is touched and the slot's bytes
 *   are unspecified; bytes of a slot beyond the file's length are never written.  qtables_dev (uint16[2][64]) and header_dev
 *   (header_bytes bytes) are hmm_jpeg_encode_header's outputs for the same geometry, in device memory: the caller uploads them
 *   (the library neither copies from host memory nor synchronises).  Five kernels and a memset of the workspace's bitstream part
 *   on `stream`; the workspace needs no initialisation and no call reads what another left there.  After the call its first
 *   n * blocks * 128 bytes hold the quantised blocks (int16[64] in zigzag order, blocks in scan order): the tests read them.
 *   HMM_E_INVALID before any launch for
 *   a null pointer, a bad geometry, channels != components, an unknown channel order, a header_bytes other than the geometry's,
 *   a workspace not 16-byte aligned, a status not 4-byte aligned, out_stride 0; HMM_E_WORKSPACE for a workspace below
 *   hmm_jpeg_encode_workspace_bytes(geometry, n); n = 0 is HMM_OK without a launch.
 * ---------------------------------------------------------------------------------------- */
#define HMM_JPEG_ENCODED          0
#define HMM_JPEG_ENCODE_OVERFLOW  1
#define HMM_JPEG_ORDER_RGB        0
#define HMM_JPEG_ORDER_BGR        1
int     hmm_jpeg_encode_header(const int32_t* geometry, int quality, uint8_t* header_out, size_t header_capacity,
                               uint16_t* qtables_out);
size_t  hmm_jpeg_encode_workspace_bytes(const int32_t* geometry, int n);
size_t  hmm_jpeg_encode_bound(const int32_t* geometry);
int     hmm_jpeg_encode(const uint8_t* frames_dev, int n, const int32_t* geometry, int channels, int channel_order,
                        const uint16_t* qtables_dev, const uint8_t* header_dev, size_t header_bytes, uint8_t* out_dev,
                        size_t out_stride, int32_t* status_dev, void* workspace_dev, size_t workspace_bytes, hmm_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The decoded pixels of frames that were just encoded, without their files: Image.open(file_i).convert("RGB") cut to the window,
 * to the bit, from what hmm_jpeg_encode left on the device.  A decoder recovers from a file the quantised coefficients and the
 * quantisation tables; both are still there (the encoder's workspace and qtables_dev), so no entropy coding is undone and no
 * byte crosses the bus.  The reads of _segment_sequence and of load_and_transform_vision_data that follow save_frame in the
 * formation path need only these pixels.
 *
 * hmm_jpeg_encoded_pixels_workspace_bytes: workspace of a call with n frames of `geometry` cut to the window (the u8 sample planes
 *   of hmm_jpeg_reconstruct); 0 for a geometry hmm_jpeg_encode does not take, a bad window or n < 1.
 * hmm_jpeg_encoded_pixels: encode_workspace_dev is the workspace a finished hmm_jpeg_encode call of the same `geometry` and n left
 *   behind, ordered before this call on `stream`; qtables_dev the tables that call was given.  -> rgb_out_dev (n, h, w, 3) u8, the
 *   window [x0, x0 + w) x [y0, y0 + h) of each frame; grey frames come out with R = G = B.  Two kernels on `stream` (dequantise +
 *   IDCT of the blocks under the window and its upsampling halo, looked up in scan order with the zigzag undone; then the
 *   upsampling and colour kernel of hmm_jpeg_reconstruct); the encoder's workspace and the tables are only read; no
 *   synchronisation, no allocation, no initialisation of the workspace needed.
 *   No frame can be refused, so there is no status: the decoder's refusal (a column of dequantised magnitudes above 5800, beyond
 *   which the first IDCT pass would leave int16) guards against corrupt files, and these blocks come from 8-bit samples -- an
 *   orthonormal block has sum |F| <= sqrt(8) * 1024 < 2897 per column, and dequantising a quantised value adds at most q / 2 per
 *   coefficient, 8 * 255 / 2 = 1020 per column at the most: under 4000 with the forward DCT's own rounding.  The largest column sum over the test table, which holds
 *   the largest AC coefficients 8-bit input can give (`extreme`) and the coarsest tables (quality 1), is 2230
 *   (tests/test_cpu_jpeg_resident.py).
 *   HMM_E_INVALID before any launch for a null pointer, n < 0, a geometry hmm_jpeg_encode does not take, a window outside the
 *   frame, a workspace (either) not 16-byte aligned, an output not 4-byte or tables not 2-byte aligned; HMM_E_WORKSPACE for a
 *   workspace below hmm_jpeg_encoded_pixels_workspace_bytes; n = 0 is HMM_OK without a launch.
 * ---------------------------------------------------------------------------------------- */
size_t  hmm_jpeg_encoded_pixels_workspace_bytes(const int32_t* geometry, int n, int x0, int y0, int w, int h);
int     hmm_jpeg_encoded_pixels(const void* encode_workspace_dev, int n, const int32_t* geometry, const uint16_t* qtables_dev,
                                int x0, int y0, int w, int h, uint8_t* rgb_out_dev, void* workspace_dev, size_t workspace_bytes,
                                hmm_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Building blocks of the encoder, exported so that each kernel is parity-tested on its own
 * against a reference of the same op (GEMM, LayerNorm, attention core: tests/test_gpu_ops.py; every other
 * stage: tests/test_gpu_stage_ops.py) and timed on its own (bench.py roofline).  bf16 tensors are raw uint16 bit patterns in device memory.
 * ---------------------------------------------------------------------------------------- */
#define HMM_EPI_BIAS_BF16        0  /* C_bf16 = A W^T + bias                                  */
#define HMM_EPI_BIAS_GELU_BF16   1  /* C_bf16 = gelu_erf(A W^T + bias)                        */
#define HMM_EPI_BIAS_RESID_F32   2  /* C_f32 += A W^T + bias  (in-place residual)             */
#define HMM_EPI_F32              3  /* C_f32 = A W^T (+ bias if non-null)                     */

/* C[M,N] = A[M,K] (bf16 row-major, lda=K) x W[N,K]^T (bf16 row-major) ; K % 64 == 0, N % 128 == 0.
 * Rows of A beyond M are never read; rows of C beyond M are never written. */
int hmm_op_gemm_bf16(const uint16_t* a_dev, const uint16_t* w_dev, const float* bias_dev,
                     void* c_dev, int M, int N, int K, int epilogue, hmm_stream_t stream);
/* The same product on one named tile geometry (hmm_op_gemm_bf16 picks per shape), so that every kernel the dispatcher
 * can choose is parity-tested on every shape.  Every geometry adds the K products of an output element in the same
 * order, so results are bitwise equal across geometries. */
#define HMM_GEMM_TILE_AUTO       -1  /* by shape; few rows may go to the sliver kernel                              */
#define HMM_GEMM_TILE_AUTO_TILED -2  /* by shape, the sliver kernel never as the whole launch (what a large-batch forward uses); it still takes the
                                        last <= 16 rows that are peeled off a ring launch (HMM_GEMM_PLAN_SLIVER_PEEL) */
#define HMM_GEMM_TILE_128x128     0  /* 4 waves, double-buffered LDS-DMA                                  */
#define HMM_GEMM_TILE_256x128     1
#define HMM_GEMM_TILE_256x256     2  /* 8 waves, same loop                                                */
#define HMM_GEMM_TILE_256x256_PP  3  /* 8 waves, 4-phase ping-pong, counted vmcnt; needs N%256==0, K%128==0 */
#define HMM_GEMM_TILE_PP_PEELED   4  /* what AUTO uses for large shapes: PP on whole rounds + 128x128 tail */
#define HMM_GEMM_TILE_SLIVER      5  /* few rows: one wave per 16..64 x 16 sliver, operands from L2 straight into fragments; epilogues 0..3 */
#define HMM_GEMM_TILE_128x128_RING 6 /* 128x128 tiles behind a 4-deep LDS-DMA ring (counted vmcnt): launches of few tiles, peeled tails */
#define HMM_GEMM_TILE_64x64_RING  7  /* 64x64 tiles, 4 waves, behind the same ring: more workgroups for mid-size M with a long K */
#define HMM_GEMM_TILE_32x32_RING  8  /* 32x32 tiles, one 16x16 block per wave, same ring: a few dozen rows x a long K */
#define HMM_GEMM_TILE_32x32_RING_K2 9   /* 32x32 tiles, deep K: 2 K-tiles per ring stage, 4 stages (64 KiB: two workgroups per CU); K % 128 == 0 */
#define HMM_GEMM_TILE_64x64_RING_K2 11  /* 64x64 tiles, 2 K-tiles per stage, 3 stages (96 KiB, one workgroup per CU): launches of at most 256 such tiles; K % 128 == 0 */
#define HMM_GEMM_TILE_128x64_RING 12  /* 128 rows x 64 columns, 4 waves of 64 x 32, same ring (96 KiB: one workgroup per CU): few-row launches whose 64x64 tiles would exceed the CUs */
#define HMM_GEMM_TILE_64x128_RING 13  /* 64 rows x 128 columns, 4 waves of 32 x 64, same ring */
#define HMM_GEMM_TILE_128x128_RING8 14 /* 128x128 tiles behind the ring with EIGHT waves (64 x 32 each, two per SIMD) */
#define HMM_GEMM_TILE_128x64_RING8  15 /* 128x64 tiles, eight waves of 32 x 32 */
#define HMM_GEMM_TILE_64x128_RING8  16 /* 64x128 tiles, eight waves of 32 x 32 */
#define HMM_GEMM_TILE_32x32_RING_K4 10  /* 32x32 tiles, 4 K-tiles per stage, 4 stages (128 KiB): few rows x a long K (one question's fc2); K % 256 == 0 */
int hmm_op_gemm_bf16_tile(const uint16_t* a_dev, const uint16_t* w_dev, const float* bias_dev,
                          void* c_dev, int M, int N, int K, int epilogue, int tile, hmm_stream_t stream);
/* Deterministic split-K (few-row forwards: one frame, one question, one audio segment; hippocampal_memory.py:1180, :1222,
 * :2173 call the encoder with such batches): part_dev[s][M][N] fp32 = A[:, s K/splits : (s+1) K/splits] W[:, same]^T for
 * s < splits, no bias; K % (64 splits) == 0; tile = one of the *_RING geometries or < 0 for a choice by shape.  An element's
 * bits depend on (K, splits) only -- every geometry walks a split's K range in the same order. */
int hmm_op_gemm_bf16_splitk(const uint16_t* a_dev, const uint16_t* w_dev, float* part_dev, int M, int N, int K,
                            int splits, int tile, hmm_stream_t stream);
/* What hmm_op_gemm_bf16_tile (splits == 0; small_tiles = 128, or 64 as a forward on two chains passes) or
 * hmm_op_gemm_bf16_splitk (splits >= 1; epilogue and small_tiles ignored) would launch for these arguments.  Host only:
 * launches nothing, needs no GPU.  The calls launch from the same plan.  Returns the number of launches -- the first
 * min(that, cap) are written to out, HMM_GEMM_PLAN_FIELDS int32 each, in launch order -- or the status and hmm_last_error text
 * of the real call for the same shape, epilogue and tile.  A record: [0] the geometry that runs, one of the ids 0..16 that
 * name a kernel (never AUTO*, never PP_PEELED); [1] first row; [2] rows; [3] splits (1 unless split-K); [4] 16-row blocks per
 * wave of the sliver kernel (1 / 2 / 4), 0 for every other geometry; [5] HMM_GEMM_PLAN_* flags. */
#define HMM_GEMM_PLAN_FIELDS       6
#define HMM_GEMM_PLAN_PP_TAIL      1  /* the peeled last row tile(s) of a ping-pong launch */
#define HMM_GEMM_PLAN_SLIVER_PEEL  2  /* the last few rows peeled off a ring launch */
int hmm_op_gemm_plan(int M, int N, int K, int epilogue, int tile, int small_tiles, int splits, int32_t* out, int cap);
/* The consumer of those slabs: x_f32[rows, D] = ((part[0] + part[1] + ... + part[splits-1]) + bias) + x (in place, the
 * slabs in split order) and y_bf16 = LayerNorm(x) * gamma + beta -- the residual epilogue of the GEMM and the LayerNorm
 * behind it in one launch.  part_dev [splits][rows][D] fp32; D in {768, 1024, 1280}. */
int hmm_op_layernorm_reduce_bf16(float* x_dev, const float* part_dev, int splits, const float* bias_dev,
                                 const float* gamma_dev, const float* beta_dev, uint16_t* y_dev, int rows, int D,
                                 float eps, hmm_stream_t stream);
/* y_bf16[rows, D] = LayerNorm(x_f32[rows, D]) * gamma + beta ; D in {768, 1024, 1280} */
int hmm_op_layernorm_bf16(const float* x_dev, const float* gamma_dev, const float* beta_dev,
                          uint16_t* y_dev, int rows, int D, float eps, hmm_stream_t stream);
/* Multi-head self-attention core on packed qkv (rows = batch*tokens, 3*D columns ordered
 * [q | k | v], heads contiguous inside each): out[rows, D] bf16.  bias_k/bias_v (D fp32, may be
 * null) append one extra key/value position (nn.MultiheadAttention add_bias_kv). */
int hmm_op_attention_bf16(const uint16_t* qkv_dev, uint16_t* out_dev, int batch, int tokens,
                          int heads, int head_dim, const float* bias_k_dev, const float* bias_v_dev,
                          hmm_stream_t stream);
/* Fused in_proj + attention of the vision tower (D = 1280, 16 heads of 80, 257 tokens per image): a_dev [n_img*257][1280]
 * bf16 (LayerNorm output), w_dev [3840][1280] bf16 + bias_dev [3840] (packed in_proj), qkv_cls_dev [n_img][3840] bf16 =
 * the projection of each image's token 0 (hmm_op_gemm_bf16 on the gathered cls rows), out_dev [n_img*257][1280] bf16.
 * Bitwise equal to hmm_op_gemm_bf16(HMM_EPI_BIAS_BF16) + hmm_op_attention_bf16. */
int hmm_op_qkv_attention_bf16(const uint16_t* a_dev, const uint16_t* w_dev, const float* bias_dev,
                              const uint16_t* qkv_cls_dev, uint16_t* out_dev, int n_img, hmm_stream_t stream);
/* The same fusion for the audio tower (D = 768, 12 heads of 64, 229 tokens per clip, nn.MultiheadAttention add_bias_kv):
 * a_dev [n_clips*229][768] bf16, w_dev [2304][768] bf16 + bias_dev [2304], bias_k_dev / bias_v_dev [768] fp32 (the learned
 * extra key / value position), out_dev [n_clips*229][768] bf16.  All 229 rows of a clip sit inside the kernel's 256-row
 * tile, so there is no separate cls projection.  Bitwise equal to hmm_op_gemm_bf16(HMM_EPI_BIAS_BF16) + hmm_op_attention_bf16
 * with the same bias_k / bias_v. */
int hmm_op_qkv_attention_audio_bf16(const uint16_t* a_dev, const uint16_t* w_dev, const float* bias_dev,
                                    const float* bias_k_dev, const float* bias_v_dev, uint16_t* out_dev, int n_clips,
                                    hmm_stream_t stream);
/* Causal variant (text tower): key j is visible to query i iff j <= i; no bias_kv. */
int hmm_op_attention_causal_bf16(const uint16_t* qkv_dev, uint16_t* out_dev, int batch, int tokens,
                                 int heads, int head_dim, hmm_stream_t stream);
/* Causal attention over packed sequences: sample b owns rows offsets_dev[b] .. offsets_dev[b+1]-1 (int32[batch + 1] on the
 * device, non-decreasing, offsets_dev[batch] = total_rows) of qkv_dev [total_rows][3D] and out_dev [total_rows][D], with as many
 * keys as queries.  head_dim 64 and at most 96 rows per sample; a sample whose table entry is outside 1 .. 96 rows or outside
 * [0, total_rows] is skipped (its output rows keep their bytes).  A sample of T rows gets the bits hmm_op_attention_causal_bf16
 * gives a sample of T tokens. */
int hmm_op_attention_causal_packed_bf16(const uint16_t* qkv_dev, uint16_t* out_dev, const int32_t* offsets_dev, int batch,
                                        int total_rows, int heads, int head_dim, hmm_stream_t stream);

/* ---- the tower stages that are neither a GEMM nor the attention core, each on its own (tests/test_gpu_stage_ops.py) ----
 * Thin entry points over the launchers hmm_encoder_forward uses.  Every one refuses null required pointers and
 * non-positive counts with HMM_E_INVALID before any launch.  All tensors are dense row-major unless a stride is named. */
/* Vision im2col: frames_dev [n_img][3][224][224] fp32 -> out_dev [n_img*256][640] bf16; row = image*256 + py*16 + px (16 x 16
 * patches of 14 x 14), column k = c*196 + dy*14 + dx = pixel (c, py*14 + dy, px*14 + dx); columns 588..639 are 0. */
int hmm_op_im2col_vision_bf16(const float* frames_dev, uint16_t* out_dev, int n_img, hmm_stream_t stream);
/* Audio im2col: mels_dev [n_clip][128][204] fp32 -> out_dev [n_clip*228][256] bf16; row = clip*228 + py*19 + px (py < 12,
 * px < 19, stride 10), column k = dy*16 + dx = mel (py*10 + dy, px*10 + dx).  Mel rows >= 126 and columns >= 196 are not read. */
int hmm_op_im2col_audio_bf16(const float* mels_dev, uint16_t* out_dev, int n_clip, hmm_stream_t stream);
/* Conv3d weight fold: w_dev [D][3][2][14][14] fp32 -> dst_dev [D][640] bf16; column k = c*196 + dy*14 + dx holds
 * bf16(w[d][c][0][dy][dx] + w[d][c][1][dy][dx]) (one fp32 add), columns 588..639 are 0. */
int hmm_op_fold_conv3d_bf16(const float* w_dev, uint16_t* dst_dev, int D, hmm_stream_t stream);
/* Token assembly: x_dev [n_img*T][D] fp32, row b*T + t = pre_ln((t == 0 ? cls : stem_ln(patches[b*(T-1) + t-1])) + pos[t]).
 * patches_dev [n_img*(T-1)][D], cls_dev [D], pos_dev [T][D], the LayerNorm vectors [D], all fp32; D in {768, 1280}.  Either
 * LayerNorm is skipped when its gamma AND beta are null; one of a pair null and the other set is refused. */
int hmm_op_assemble_tokens(const float* patches_dev, const float* cls_dev, const float* pos_dev,
                           const float* stem_gamma_dev, const float* stem_beta_dev, float stem_eps,
                           const float* pre_gamma_dev, const float* pre_beta_dev, float pre_eps,
                           float* x_dev, int n_img, int T, int D, hmm_stream_t stream);
/* hmm_op_layernorm_bf16 on rows that lie in_stride FLOATS apart: y_bf16[r][D] = LayerNorm(x_dev[r*in_stride .. + D)) -- the
 * form the fused path uses for token 0 of every image (in_stride = T*D).  Only the D floats of each row are read.
 * in_stride >= D and a multiple of 4; D in {768, 1024, 1280}. */
int hmm_op_layernorm_strided_bf16(const float* x_dev, size_t in_stride, const float* gamma_dev, const float* beta_dev,
                                  uint16_t* y_dev, int rows, int D, float eps, hmm_stream_t stream);
/* dst_dev[r][0, row_bytes) = src_dev[r*src_row_stride_bytes .. + row_bytes) for r < n_rows, in 16-byte pieces: row_bytes and
 * the stride are multiples of 16, the stride >= row_bytes, both pointers 16-byte aligned.  Nothing past the last byte of the
 * last gathered row is read. */
int hmm_op_gather_rows(const void* src_dev, size_t src_row_stride_bytes, void* dst_dev, int n_rows, int row_bytes,
                       hmm_stream_t stream);
/* One-query attention of the last block: q_cls_dev [batch][D] bf16 (D = heads*head_dim), kv_dev [batch*tokens][2D] bf16 =
 * [k | v], heads contiguous inside each half; out_dev [batch][D] bf16 = softmax(q k^T / sqrt(head_dim)) v per (sample, head).
 * bias_k / bias_v ([D] fp32, rounded to bf16) append one key / value position and come together or not at all; at most 320
 * keys including it; head_dim 64 or 80.  Scores, softmax and P.V are fp32 (P is not rounded); the output is rounded once. */
int hmm_op_attention_cls_bf16(const uint16_t* q_cls_dev, const uint16_t* kv_dev, uint16_t* out_dev, int batch, int tokens,
                              int heads, int head_dim, const float* bias_k_dev, const float* bias_v_dev,
                              hmm_stream_t stream);
/* Text embedding: x_dev [n_rows][1024] fp32, row r = table_dev[clamp(ids_dev[r], 0, vocab-1)] + pos_dev[r % T] (one fp32
 * add); ids_dev [n_rows] int64, table_dev [vocab][1024], pos_dev [T][1024]. */
int hmm_op_embed_tokens(const int64_t* ids_dev, const float* table_dev, const float* pos_dev, float* x_dev, int n_rows,
                        int T, int vocab, hmm_stream_t stream);
/* Text head: y_dev [batch][D] bf16, row b = LayerNorm(x_dev[b*T + e(b)]) with e(b) the FIRST position of the largest id in
 * ids_dev[b][0, T) (int64); x_dev [batch*T][D] fp32.  Same bits as hmm_op_layernorm_bf16 on that row.  D in {768, 1024, 1280}. */
int hmm_op_layernorm_eos_bf16(const float* x_dev, const int64_t* ids_dev, int T, const float* gamma_dev,
                              const float* beta_dev, uint16_t* y_dev, int batch, int D, float eps, hmm_stream_t stream);
/* Post-processing: out_dev [n_out][1024] fp32, row i = mean over s < clips of scale * v[i*clips + s] / max(||v[i*clips + s]||, 1e-12)
 * (each clip normalised first, then the mean); v_dev [n_out*clips][1024] fp32; scale = min(exp(*log_scale_dev), 100), or 1 when
 * log_scale_dev is null. */
int hmm_op_l2norm_rows(const float* v_dev, float* out_dev, int n_out, int clips, const float* log_scale_dev,
                       hmm_stream_t stream);

/* Timing / test hooks of the scan (bench.py roofline, tests): the streaming kernel of hmm_cosine_topk alone --
 * scan_topk_kernel writing its per-block candidate keys (cand_keys_dev: 2048*k uint64) -- and the plain similarity
 * pass (sims_dev: n_rows fp32) that k > 128 uses. */
int hmm_op_scan_topk_only(const float* store_dev, int64_t n_rows, const float* query_dev, int k,
                          uint64_t* cand_keys_dev, hmm_stream_t stream);
int hmm_op_scan_sims(const float* store_dev, int64_t n_rows, const float* query_dev, float* sims_dev,
                     hmm_stream_t stream);

/* ---- memory_store event files: host-side parsing of the feature matrices (no GPU call) ----
 * Replaces, for the 2-D arrays of numbers only, the json.load + np.array(list) of load_theta_event
 * (hippomm/core/hippocampal_memory.py:369-395): hmm_json_find_matrices reports every `[[numbers], ...]` with equally long rows and
 * at least min_values numbers in text[0, len) outside string literals (byte span of the outer brackets + shape; at most `cap`
 * entries written, *n_found counts all); hmm_json_parse_matrix_f32 converts one reported span into rows x cols fp32,
 * out[r][c] = (float)(double)literal with correctly rounded, locale-independent decimal -> double conversion -- the value
 * np.array(json.load(f)[...]).astype(float32) has.  NaN / Infinity / -Infinity (Python's json spelling) are numbers here.  A
 * literal outside the double range fails with HMM_E_INVALID: the caller keeps json.load for that file. */
typedef struct hmm_json_matrix { size_t begin, end, rows, cols; } hmm_json_matrix;
int hmm_json_find_matrices(const char* text, size_t len, size_t min_values, hmm_json_matrix* out, int cap, int* n_found);
int hmm_json_parse_matrix_f32(const char* text, size_t begin, size_t end, size_t rows, size_t cols, float* out_host);
/* The writer's side (save_theta_event, hippocampal_memory.py:331-335: json.dump(event.to_dict(), f, indent=2)): rows x cols host
 * doubles as the text json.dumps(m.tolist(), indent=2) has for that list when its closing bracket sits at close_indent spaces
 * (rows at +2, values at +4) -- float.__repr__ digits and notation, NaN / Infinity / -Infinity as json spells them; byte for byte.
 * out_text needs hmm_json_matrix_text_bound(rows, cols, close_indent) bytes; *written = the length (no terminator). */
size_t hmm_json_matrix_text_bound(size_t rows, size_t cols, int close_indent);
int hmm_json_write_matrix_f64(const double* m_host, size_t rows, size_t cols, int close_indent, char* out_text, size_t cap, size_t* written);

/* ---- the same text, written on the device (csrc/event_json.hip, csrc/event_json_core.h) ----
 * hmm_json_write_matrix_device: a rows x cols row-major matrix ON THE DEVICE, fp32 (dtype HMM_JSON_DTYPE_F32; every value is
 * widened to double first, which is what np.asarray(f32).tolist() hands to json) or fp64 (HMM_JSON_DTYPE_F64) -> exactly the bytes
 * hmm_json_write_matrix_f64 writes for those values at the same close_indent, into out_text_dev[0, *written_dev); *written_dev is a
 * uint64 on the device.  Not one byte of out_text_dev behind *written_dev is written, nor one of the workspace behind
 * hmm_json_write_matrix_device_workspace_bytes(rows, cols); the matrix is only read.  out_text_dev needs no alignment; the
 * workspace and written_dev are 8-byte aligned, the matrix aligned to its element.  Three launches on `stream` (item lengths summed
 * per workgroup of HMM_JSON_VALUES_PER_GROUP values; those sums scanned by one workgroup, HMM_JSON_SCAN_SUMS_PER_ROUND of them per
 * round, i.e. HMM_JSON_VALUES_PER_SCAN_ROUND values; the text formed again, placed in LDS and stored in whole dwords): nothing
 * synchronises or allocates, no workgroup waits for another, the call can be captured into a graph.
 *   HMM_E_INVALID with a message, before any launch and without needing a GPU, for: a null pointer, an unknown dtype, rows or
 *   cols < 1, rows * cols > HMM_JSON_MAX_VALUES, close_indent outside 0 .. HMM_JSON_MAX_INDENT (a workgroup stages its longest
 *   possible round in LDS), cap < hmm_json_matrix_text_bound(rows, cols, close_indent), workspace_bytes below the query's answer
 *   (the query answers 0 for a shape the call refuses), a misaligned matrix, workspace or written_dev.
 * hmm_json_float_repr: HOST only, no GPU call -- the device's float printer run on the host: values[i] -> the characters
 * json.dumps writes for that double (float.__repr__; NaN, Infinity, -Infinity) at out_chars + HMM_JSON_REPR_BYTES * i, their count
 * (at most HMM_JSON_REPR_BYTES, no terminator) in out_lengths[i].  Correct for every double. */
#define HMM_JSON_DTYPE_F32 0
#define HMM_JSON_DTYPE_F64 1
#define HMM_JSON_REPR_BYTES 24
#define HMM_JSON_VALUES_PER_GROUP 1024
#define HMM_JSON_SCAN_SUMS_PER_ROUND 256
#define HMM_JSON_VALUES_PER_SCAN_ROUND (HMM_JSON_VALUES_PER_GROUP * HMM_JSON_SCAN_SUMS_PER_ROUND)
#define HMM_JSON_MAX_VALUES 2147483648ull
#define HMM_JSON_MAX_INDENT 32
size_t hmm_json_write_matrix_device_workspace_bytes(size_t rows, size_t cols);
int hmm_json_write_matrix_device(const void* m_dev, int dtype, size_t rows, size_t cols, int close_indent, char* out_text_dev, size_t cap,
                                 uint64_t* written_dev, void* workspace_dev, size_t workspace_bytes, hmm_stream_t stream);
int hmm_json_float_repr(const double* values, size_t n, char* out_chars, int* out_lengths);

/* ---- and read back on the device (csrc/event_json_parse.hip, csrc/event_json_parse_core.h) ----
 * hmm_json_parse_matrix_device: text_dev[begin, end) ON THE DEVICE is one matrix as hmm_json_find_matrices reported it (its first
 * byte is the outer '['; no string literal inside) -> rows x cols row-major values in out_dev: fp32 (HMM_JSON_DTYPE_F32) with the
 * bits hmm_json_parse_matrix_f32 gives, out = (float)(double)literal, or fp64 (HMM_JSON_DTYPE_F64) with the bits of Python's
 * float(literal), the reference's own in-memory dtype.  NaN is 0x7fc00000 / 0x7ff8000000000000; "-0.0" and "-0e0" keep their sign,
 * "-0" is +0.0 (an int to json.load).  A token is a run of number bytes (digits + - . e E and the letters of NaN and Infinity) behind
 * a separator (space \n \r \t , [ ]); the token with ordinal k is checked against JSON's number grammar (as hmm_json_find_matrices
 * does), converted with integer arithmetic only (Eisel-Lemire on the first 19 significant digits, exact for every such literal) and
 * stored to out[k].  The brackets and commas between the tokens are NOT checked again: the span finder is their authority.
 *   report_dev (32 bytes, 8-byte aligned) is written by every call: n_tokens; n_flagged; first_bad, the lowest byte offset in
 *   text_dev of a wrong byte or token (HMM_JSON_PARSE_NO_OFFSET: none); status, the highest of
 *     HMM_JSON_PARSE_OK;
 *     HMM_JSON_PARSE_COUNT      n_tokens != rows x cols: out[k] is written for k < min(n_tokens, rows x cols) only;
 *     HMM_JSON_PARSE_BAD_BYTE   a byte that is neither a separator nor a number byte;
 *     HMM_JSON_PARSE_BAD_TOKEN  a token that fails the grammar ("1.", ".5", "+1", "01", "nan"); its slot of out holds zero.
 *   FLAGGED values are tokens this call does not convert; their slots of out hold +0.0, so that out is fully defined, and
 *   flagged_dev[0 .. min(n_flagged, flagged_cap)) names them in no particular order: ordinal, byte span [begin, end) in text_dev,
 *   and why -- HMM_JSON_FLAG_UNDECIDED (more than 19 significant digits, counted from the first non-zero digit of the mantissa, and
 *   the first 19 as an integer and that integer plus one round to different doubles), HMM_JSON_FLAG_RANGE (a non-zero literal that
 *   rounds to infinity or to zero, or a decimal exponent above 9999: hmm_json_parse_matrix_f32 declines such a file) or
 *   HMM_JSON_FLAG_TOO_LONG (a token of more than HMM_JSON_TOKEN_MAX bytes).  n_flagged counts all of them; entries behind
 *   flagged_cap are not written, nor is anything of flagged_dev behind min(n_flagged, flagged_cap).  A literal of at most 19
 *   significant digits inside the double range is never flagged.
 * Text of any alignment: it is read as aligned 16-byte words where those lie inside [begin, end) and byte by byte at the two ends;
 * no byte outside the span is read.  out_dev is aligned to its element; report_dev, flagged_dev and the workspace
 * (hmm_json_parse_matrix_device_workspace_bytes(end - begin): one 64-bit count per HMM_JSON_PARSE_GROUP_BYTES bytes of the span; no
 * initialisation) to 8 bytes.  Three launches on `stream` (token starts counted per group; the counts scanned by one workgroup,
 * HMM_JSON_PARSE_SCAN_GROUPS_PER_ROUND per round; the tokens found again and converted): nothing synchronises or allocates, no
 * workgroup waits for another, the call can be captured into a graph.
 *   HMM_E_INVALID with a message, before any launch and without needing a GPU, for: a null pointer (flagged_dev may be null when
 *   flagged_cap is 0), begin >= end, a span above HMM_JSON_PARSE_MAX_SPAN_BYTES, an unknown dtype, rows or cols < 1, rows * cols >
 *   HMM_JSON_MAX_VALUES, flagged_cap < 0, workspace_bytes below the query's answer (0 for a span the call refuses), a misaligned
 *   out_dev, report_dev, flagged_dev or workspace.
 * hmm_json_float_parse: HOST only, no GPU call -- the device's number parser run on the host: token i is text[spans[2 i],
 * spans[2 i + 1]) -> out_f64_bits[i] (Python's float(token)), out_f32_bits[i] ((float)(double)) and out_flags[i]: 0 for a
 * converted token, else one of HMM_JSON_FLAG_* with both values zero (HMM_JSON_FLAG_BAD_TOKEN: not a number by the grammar). */
#define HMM_JSON_TOKEN_MAX 64
#define HMM_JSON_PARSE_GROUP_BYTES 4096
#define HMM_JSON_PARSE_SCAN_GROUPS_PER_ROUND 256
#define HMM_JSON_PARSE_MAX_SPAN_BYTES 1099511627776ull
#define HMM_JSON_PARSE_OK 0
#define HMM_JSON_PARSE_COUNT 1
#define HMM_JSON_PARSE_BAD_BYTE 2
#define HMM_JSON_PARSE_BAD_TOKEN 3
#define HMM_JSON_PARSE_NO_OFFSET 0xFFFFFFFFFFFFFFFFull
#define HMM_JSON_FLAG_UNDECIDED 1
#define HMM_JSON_FLAG_RANGE 2
#define HMM_JSON_FLAG_TOO_LONG 3
#define HMM_JSON_FLAG_BAD_TOKEN 4
typedef struct hmm_json_parse_report { uint64_t n_tokens, n_flagged, first_bad, status; } hmm_json_parse_report;
typedef struct hmm_json_flagged { uint64_t ordinal, begin, end, flag; } hmm_json_flagged;
size_t hmm_json_parse_matrix_device_workspace_bytes(size_t span_bytes);
int hmm_json_parse_matrix_device(const char* text_dev, size_t begin, size_t end, size_t rows, size_t cols, int dtype, void* out_dev,
                                 hmm_json_parse_report* report_dev, hmm_json_flagged* flagged_dev, int64_t flagged_cap,
                                 void* workspace_dev, size_t workspace_bytes, hmm_stream_t stream);
int hmm_json_float_parse(const char* text, const uint64_t* spans, size_t n, uint64_t* out_f64_bits, uint32_t* out_f32_bits, int* out_flags);

/* ---- and found in the text on the device (csrc/event_json_find.hip, csrc/event_json_find_core.h) ----
 * hmm_json_find_matrices_device: hmm_json_find_matrices for a text ON THE DEVICE.  text_dev[0, len) may have any alignment and is
 * only read; no byte outside it is dereferenced.  *report_dev (device, 8-byte aligned) receives
 *   n_found         all matrices, as the host's *n_found; out_dev[0 .. min(n_found, cap)) (device, 8-byte aligned; may be null when
 *                   cap is 0) is the host finder's list, field for field, in document order; nothing behind it is written;
 *   n_candidates    the `[` outside string literals whose next byte that is not whitespace is another `[`;
 *   status          HMM_JSON_FIND_OK: the list equals hmm_json_find_matrices(text, len, min_values, ...) for every byte string --
 *                   malformed JSON, unbalanced quotes and texts that end inside a string included;
 *                   HMM_JSON_FIND_DECLINED: n_found is 0, nothing is listed and the caller runs the host finder.  Two reasons only:
 *                   a candidate that is otherwise a matrix holds a number token of more than HMM_JSON_TOKEN_MAX bytes, or the text
 *                   has more than HMM_JSON_FIND_MAX_CANDIDATES candidates (each takes at most two entries of the workspace's event
 *                   list; the call declines when the list overflows);
 *   first_declined  the text offset of the first candidate that made the call decline (HMM_JSON_PARSE_NO_OFFSET: none).
 * Whitespace runs, backslash runs and nesting of any length and depth and a matrix larger than any group are handled.  The
 * workspace (hmm_json_find_matrices_device_workspace_bytes(len), 8-byte aligned) needs no initialisation and nothing behind the
 * query's answer is written.  Eight launches on `stream` (per group of HMM_JSON_PARSE_GROUP_BYTES bytes: the string-state map and
 * the last non-whitespace byte under each incoming state; one workgroup scans them; the groups count their tokens, rows, illegal
 * bytes and events; one workgroup scans the counts; the groups list candidates and closers; one workgroup pairs them; the groups
 * check every row's place; one workgroup writes the list): nothing synchronises or allocates, no workgroup waits for another, the
 * sequence may be captured into a graph.
 * HMM_E_INVALID before any launch (no GPU needed): a null pointer (out_dev may be null when cap is 0), cap < 0, len of 0 or above
 *   HMM_JSON_PARSE_MAX_SPAN_BYTES, workspace_bytes below the query's answer (0 for a len the call refuses), a misaligned out_dev,
 *   report or workspace.
 * hmm_json_find_matrices_blocks: HOST only, no GPU call -- the same block algorithm (the same per-byte rules, summaries and
 * compositions, the same group size and decline rules) run on host memory; `out` and `report` are host pointers. */
#define HMM_JSON_FIND_OK 0
#define HMM_JSON_FIND_DECLINED 1
#define HMM_JSON_FIND_MAX_CANDIDATES 16384
typedef struct hmm_json_find_report { uint64_t n_found, n_candidates, status, first_declined; } hmm_json_find_report;
size_t hmm_json_find_matrices_device_workspace_bytes(size_t len);
int hmm_json_find_matrices_device(const char* text_dev, size_t len, size_t min_values, hmm_json_matrix* out_dev, int cap,
                                  hmm_json_find_report* report_dev, void* workspace_dev, size_t workspace_bytes, hmm_stream_t stream);
int hmm_json_find_matrices_blocks(const char* text, size_t len, size_t min_values, hmm_json_matrix* out, int cap, hmm_json_find_report* report);

/* ---- base64, for the checkpoint file (csrc/base64.hip, csrc/base64_core.h) ----
 * The reference writes every feature block of a checkpoint as base64(np.array(v.tolist()).tobytes()) (hippocampal_memory.py:308-310,
 * :1506): the block as float64, standard alphabet, '=' padding -- the bytes of Python's base64.b64encode.
 * hmm_base64_encoded_length: 4 * ceil(n_bytes / 3).
 * hmm_base64_encode_device: n_values values at src_dev ON THE DEVICE -> out_dev[0, hmm_base64_encoded_length(bytes)), where bytes is
 *   8 * n_values for HMM_BASE64_DTYPE_F32 (each value widened to double first, as np.array(v.tolist()) does) and for
 *   HMM_BASE64_DTYPE_F64, and n_values for HMM_BASE64_DTYPE_U8 (raw bytes).  One launch on `stream`: a thread encodes
 *   HMM_BASE64_BYTES_PER_THREAD source bytes into 32 characters (two 16-byte stores), a workgroup HMM_BASE64_BYTES_PER_GROUP; the
 *   last, partial unit writes the padding.  Nothing allocates or synchronises, there is no workspace and no count to read back; not a
 *   byte behind the encoded length is written and the source is only read.  n_values == 0 launches nothing.  Quiet NaNs of any
 *   payload pass bit for bit; a SIGNALLING NaN in an fp32 source is outside the contract (widening quiets it, here and in numpy, but
 *   nothing pins the two to the same bits).
 *   Alignment: src_dev to its element (4 / 8 bytes; none for bytes), out_dev to 16 bytes.
 * hmm_base64_decode_device: STRICT.  text_dev[0, n_chars) is accepted only if n_chars is a multiple of 4, every character is of the
 *   alphabet, and padding stands at the very end only ("xxx=" or "xx==") in canonical form (the bits the padding cuts off are zero).
 *   Whitespace and stray characters, which Python's lenient b64decode skips, are refused: the caller then decodes on the host.
 *   report_dev (HMM_BASE64_REPORT_WORDS uint64, 8-byte aligned) is written by every call:
 *     [0] status   HMM_BASE64_OK, or why the text is refused:
 *                  HMM_BASE64_BAD_LENGTH     n_chars % 4 != 0; the offset is where the incomplete quad begins;
 *                  HMM_BASE64_BAD_CHAR       a byte outside the alphabet that is not '=';
 *                  HMM_BASE64_BAD_PADDING    '=' anywhere but in the last two places, or "xx=x";
 *                  HMM_BASE64_NONCANONICAL   the character in front of the padding carries bits the padding cuts off;
 *                  HMM_BASE64_PARTIAL_VALUE  a float dtype_out and the bytes are not whole doubles (offset: the last quad);
 *                  HMM_BASE64_CAPACITY       more values than cap_values (bytes only, see below; offset: the last quad);
 *     [1] offset   the LOWEST offending text offset, with its status in [0]; 0 when the status is OK;
 *     [2] inexact  HMM_BASE64_DTYPE_F32 only: the values v for which (double)(float)v does not have v's 64 bits;
 *     [3] values   the values written (0 on a refusal);
 *     [4] reserved (the call's working word).
 *   On a refusal NOT ONE byte of out_dev is written.  dtype_out: HMM_BASE64_DTYPE_U8, the bytes; HMM_BASE64_DTYPE_F64, the bytes as
 *   they are, which must be whole doubles; HMM_BASE64_DTYPE_F32, each double narrowed (round to nearest even).  Three launches on
 *   `stream` (the report's start values; every quad checked, the lowest offending offset kept by a 64-bit atomic minimum; the
 *   groups decoded unless something was found): nothing allocates or synchronises, no workgroup waits for another.
 *   cap_values: a float dtype_out needs floor(3 (n_chars / 4) / 8), which is the exact count of an accepted text; bytes need
 *   3 (n_chars / 4) - 2, the count under the longest padding, and a text that decodes to more than cap_values is refused on the
 *   device (HMM_BASE64_CAPACITY).  Alignment: text_dev to 16 bytes, out_dev to its element, report_dev to 8.
 * hmm_base64_encode_host / hmm_base64_decode_host: HOST only, no GPU call -- the same core on host memory (no alignment beyond the
 *   element's; `report` as above).
 * HMM_E_INVALID with a message, before any launch and without needing a GPU, for: a null pointer (src / out may be null when
 *   there is nothing to read or write), an unknown dtype, more than HMM_BASE64_MAX_BYTES, a cap below the need, a misaligned
 *   pointer. */
#define HMM_BASE64_DTYPE_F32 0
#define HMM_BASE64_DTYPE_F64 1
#define HMM_BASE64_DTYPE_U8 2
#define HMM_BASE64_BYTES_PER_THREAD 24
#define HMM_BASE64_THREADS_PER_GROUP 256
#define HMM_BASE64_BYTES_PER_GROUP (HMM_BASE64_BYTES_PER_THREAD * HMM_BASE64_THREADS_PER_GROUP)
#define HMM_BASE64_MAX_BYTES 1099511627776ull
#define HMM_BASE64_REPORT_WORDS 5
#define HMM_BASE64_OK 0
#define HMM_BASE64_BAD_LENGTH 1
#define HMM_BASE64_BAD_CHAR 2
#define HMM_BASE64_BAD_PADDING 3
#define HMM_BASE64_NONCANONICAL 4
#define HMM_BASE64_PARTIAL_VALUE 5
#define HMM_BASE64_CAPACITY 6
size_t hmm_base64_encoded_length(size_t n_bytes);
int hmm_base64_encode_device(const void* src_dev, int dtype, size_t n_values, char* out_dev, size_t cap, hmm_stream_t stream);
int hmm_base64_decode_device(const char* text_dev, size_t n_chars, int dtype_out, void* out_dev, size_t cap_values, uint64_t* report_dev,
                             hmm_stream_t stream);
int hmm_base64_encode_host(const void* src, int dtype, size_t n_values, char* out, size_t cap);
int hmm_base64_decode_host(const char* text, size_t n_chars, int dtype_out, void* out, size_t cap_values, uint64_t* report);

#ifdef __cplusplus
}
#endif
#endif /* HIPPOMM_HIP_H */
