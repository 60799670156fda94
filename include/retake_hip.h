/*
 * retake_hip.h — C ABI of libretake_hip.so: the MI355X (gfx950) implementation of ReTaKe's
 * DPSelect + PivotKV hot path.
 *
 * The reference (SCZwangxiao/video-ReTaKe) is pure Python: its "FFI" for this path is the set of
 * torch ATen calls inside two functions.  Each entry point below replaces one group of those call
 * sites; the reference-side binding is a ctypes stub, and the shipped Python
 * package `retake` (video-retake_amd/retake) is that binding behind the reference's own names
 *   retake.visual_compression.memory_bank_compress_keyframe   (visual_compression.py:86-177)
 *   retake.longvideo_cache.PivotKVCache.update                (longvideo_cache.py:217-323)
 *
 * Conventions
 *   - every pointer is a DEVICE pointer on the current HIP device unless marked host;
 *   - the library never allocates or frees device memory: outputs and workspaces are caller-owned;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream) and
 *     re-entrant.  Process-wide state, all of it thread-safe: the thread-local error string; the opt-in
 *     measurement hooks at the end of this header (off by default, mutex-guarded); a memo of which devices
 *     have had the > 64 KiB dynamic-LDS opt-in applied to the score kernels (one atomic bit per device);
 *     a mutex-guarded memo of exhaustive bf16 reciprocal checks keyed by attention_scaling^2.  No results
 *     depend on any of it, and the library reads no environment variables;
 *   - return value 0 = success, negative = rtk_status; no C++ exception crosses the ABI;
 *   - dtype: RTK_F32, RTK_BF16 or RTK_F16 for the frame / q / k / v payloads (the scoring entry points take the
 *     mode-carrying codes as well); scores, distances and RoPE
 *     tables are always fp32; indices are int64 and masks are 1 byte per element (torch.bool layout);
 *   - strides are in ELEMENTS; the innermost (channel / head_dim) axis is always contiguous.
 *
 * Contents (104 entry points; search for the section title).  A binding of the hot path needs §A, §B, §E and the four
 * calls of §G; §D / §F are the stage-by-stage forms the same kernels are also reachable through.
 *   §A  version / errors                rtk_version, rtk_last_error, rtk_arch
 *   §B  "DPSelect"                      rtk_dpselect_dis, rtk_dpselect_select, rtk_gather_frames
 *   §C  "MA-LLM / MA-LLM-hard merges"   rtk_adjacent_cosine, rtk_mallm_argmax, rtk_mallm_merge, rtk_mallm_hard_chain
 *   §D  "RoPE tables"                   rtk_rope_merge, rtk_rope_table, rtk_rope_rotate_rows, rtk_rope_shift(_segments)
 *   §E  "PivotKV" (one unit, by stage)  rtk_pivotkv_score(_stages, _stages_masked, _passes_batched(_q), _partials),
 *                                       rtk_pivotkv_prepare, rtk_pivotkv_select(_batched), *_workspace_bytes
 *   §F  "Chunk-batched cache maintenance"  rtk_pivotkv_append, rtk_pivotkv_evict_batched(_rope), _commit_batched,
 *                                       _place_batched, rtk_pivotkv_compact_batched (+ _compact_sync_ints)
 *   §G  "One-call update and one-call flush"  rtk_pivotkv_update, rtk_pivotkv_flush, rtk_pivotkv_append_rope,
 *                                       rtk_position_shift (+ rtk_pivotkv_shift_ticket_ints): what the shipped
 *                                       package calls per update / per chunk / per decode step
 *   §H  "Direct peer-to-peer all-gather over xGMI"  rtk_p2p_alloc / _free / _export / _open / _close / _push / _wait
 *   §I  "Chunk attention"               rtk_attention_forward (+ rtk_attention_workspace_bytes): the chunk's queries over
 *                                       [compressed prefix | current chunk], opt-in (attention_kernel="hip");
 *                                       rtk_attention_decode (+ _workspace_bytes): the same function for few query
 *                                       rows, GQA-packed, opt-in (decode_attention="packed")
 *   §J  "Measurement support"           rtk_profile_* (off by default)
 *   §K  "FP8 rows of the compressed cache"  rtk_pivotkv_archive_batched, rtk_attention_forward_fp8kv (+ _workspace_bytes_fp8kv),
 *                                       rtk_attention_decode_fp8kv (+ _workspace_bytes_fp8kv), rtk_fp8kv_dequant: opt-in (kv_cache_dtype="fp8_e4m3" with attention_kernel="hip")
 *   §L  "Shared 16-bit rows"            rtk_attention_forward_shared, rtk_attention_decode_shared (+ _workspace_bytes_shared):
 *                                       the keys are [archive | rows of another buffer | own rows] (PivotKVCache.fork);
 *                                       rtk_attention_decode_wide, _wide_fp8kv, _wide_shared (+ their _workspace_bytes):
 *                                       the packed calls for up to 64 packed rows, opt-in (multi_token_attention="packed")
 *   §M  "Group decode"                  rtk_attention_decode_group (+ _workspace_bytes): one token of each of several
 *                                       branches in one launch that reads the shared rows once (retake/branch_group.py)
 *   §N  "Sliding window"                rtk_pivotkv_slide_batched: rows of many buffers moved down in place, one call - the
 *                                       oldest video rows of every layer dropped (opt-in: video_window_rows)
 *   §O  "Video budget"                  rtk_pivotkv_keep_scores_batched, rtk_pivotkv_budget_select_batched,
 *                                       rtk_pivotkv_squeeze_batched: a bounded cache that keeps its best-scored video rows
 *                                       (opt-in: video_budget_rows)
 *   §P  "DPSelect on a stream"          rtk_dpselect_ingest, rtk_dpselect_select_ring: keyframe selection for a video that
 *                                       does not end, in a ring of 2 S frames (retake/dpselect_stream.py)
 *   §Q  "Position re-base"              rtk_pivotkv_rebase_batched: the ids of a bounded video region re-based to follow the
 *                                       pinned rows and its keys re-rotated in place (opt-in: video_position_limit)
 *   §R  "Position renumbering"          rtk_pivotkv_renumber_batched: the id gaps of such a region closed row by row, each
 *                                       key re-rotated by its own row's delta (opt-in: video_position_gap)
 *   §S  "Budget re-scoring"             rtk_pivotkv_rescore_batched (+ _workspace_bytes): the stored scores of a budget's old
 *                                       rows blended with what the newest chunk's last queries see of them (opt-in:
 *                                       video_budget_rescore); rtk_pivotkv_rescore_fp8k_batched: the same over the e4m3
 *                                       key rows of an fp8 archive (opt-in: archive_rescore)
 *   §T  "Question focus"                rtk_pivotkv_focus_gather_batched: the pinned rows, the video rows a question's queries
 *                                       choose and the question's rows of every layer gathered out of place into a small
 *                                       cache of their own (opt-in: PivotKVCache.watch_question / focus)
 *   §U  "Page-sparse decode"            rtk_pivotkv_page_summary_batched, rtk_attention_page_bound, rtk_attention_decode_paged,
 *                                       rtk_attention_decode_sparse (+ their _workspace_bytes): per-page key bounds beside the
 *                                       rows, and a packed decode call that reads, per kv head and token, the pinned rows, the
 *                                       pages with the highest bound and the rows behind the video (opt-in:
 *                                       sparse_decode(cache) of retake/_sparse_decode.py); rtk_pivotkv_page_summary_fp8k_batched,
 *                                       rtk_attention_decode_paged_fp8kv, rtk_attention_decode_sparse_fp8kv: the same with the
 *                                       pages in an fp8 archive (opt-in: sparse_decode(cache, archive=True));
 *                                       rtk_attention_decode_paged_wide, rtk_attention_decode_sparse_wide (+ their
 *                                       _workspace_bytes): the 16-bit calls for up to 64 packed rows, one list per kv head for
 *                                       all their rows (opt-in: sparse_decode(cache, wide=True))
 */
#ifndef RETAKE_HIP_H
#define RETAKE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* rtk_stream_t; /* hipStream_t */

enum rtk_dtype {
    RTK_F32 = 0,
    RTK_BF16 = 1,
    /* Scoring entry points only (rtk_pivotkv_score*, rtk_pivotkv_select_batched): bf16 payloads AND the reference's
     * bf16 rounding chain for the score (longvideo_cache.py:264-270 on a bf16 model rounds the logits, the
     * probabilities, the per-head column sums and both means to bf16).  RTK_BF16 keeps exact bf16 products with fp32
     * accumulation, softmax and sums - more accurate than the reference; this code reproduces the reference's own
     * quantised scores (head_dim 128 only).  Workspace / partial sizes differ: query them with the same code. */
    RTK_BF16_REFROUND = 2,
    /* Scoring entry points and rtk_pivotkv_prepare only: bf16 payloads, scored through the fp16 matrix instruction.  The
     * un-rotated q~ is stored as fp16(q~ * log2(e)/sqrt(D)) - ONE extra rounding, to 11 significant bits - and k~ is
     * re-encoded as fp16 exactly (a second copy inside the score workspace; the bf16 k~ the eviction re-rotates is
     * unchanged), so the accumulators are base-2 logits and both passes spend two instructions per logit instead of
     * three.  Scores move by ~1e-5 relative against RTK_BF16 (far inside the reference's own bf16 rounding of the
     * logits); everything downstream of the score is identical.  Opt in: score_rounding="fast".  head_dim 128 only;
     * |k~| beyond fp16's range (65504) saturates. */
    RTK_BF16_FAST = 3,
    /* fp16 payloads (a float16 model).  Like RTK_BF16, every entry point restates the reference's chain of torch ops
     * with one rounding to the tensor dtype per op; the score uses exact fp16 products with fp32 accumulation.
     * Wherever an argument is called `round_bf16`, 2 selects fp16 tables (1 = bf16, 0 = fp32). */
    RTK_F16 = 4,
    /* Scoring entry points only: fp16 payloads AND the reference's rounding chain on a float16 model - RTK_BF16_REFROUND's
     * chain with every rounding to fp16 instead of bf16 (logits, probabilities, per-head sums, both means); head_dim 128.
     * rtk_pivotkv_prepare takes RTK_F16 for such a batch. */
    RTK_F16_REFROUND = 5
};

/* Flag for the `dtype` argument of the SCORING entry points (rtk_pivotkv_score_workspace_bytes, _score_partials,
 * _score, _score_stages[_masked], _score_passes_batched, rtk_pivotkv_prepare, and score_dtype of rtk_pivotkv_select_batched):
 * the caller batches many (layer, chunk) units per launch, so the key / row splits - which fix the workspace layout, the
 * partial layout AND the reduction order, i.e. the bits of the score - are chosen for the length of a workgroup's stream
 * instead of for the workgroup count of one unit (one key split, about eight row tiles per row split).  Every call that
 * touches the same workspace must carry the same flag. */
#define RTK_SCORE_MANY_UNITS 0x100
/* Flag for the `dtype` argument of rtk_pivotkv_prepare only: the chunk keeps every token (compression_ratio 1, what
 * `dynamic_compression_ratio` gives every prompt within max_input_length, qwen2_vl.py:553-554) and is not scored, so
 * the un-rotated queries are not produced - k~ (for the re-rotation) and the cache tail still are. */
#define RTK_PREPARE_K_ONLY 0x200

enum rtk_status {
    RTK_OK = 0,
    RTK_EINVAL = -1,      /* bad argument (NULL pointer, non-positive size, unsupported dtype) -> ValueError   */
    RTK_EUNSUPPORTED = -2,/* shape outside what the kernels support                      -> NotImplementedError */
    RTK_EWORKSPACE = -3,  /* workspace too small                                          -> ValueError         */
    RTK_EHIP = -4,        /* a HIP runtime call failed (message in rtk_last_error)        -> RuntimeError       */
    RTK_EREFCRASH = -5    /* input on which the reference itself raises (N==1 async)      -> IndexError         */
};

/* ABI version (bumped on any signature change) and the thread-local message of the last failure. */
int rtk_version(void);
const char* rtk_last_error(void);
/* Name of the code-object architecture this library was built for ("gfx950"). */
const char* rtk_arch(void);

/* ---------------------------------------------------------------------------------------------
 * DPSelect  — replaces retake/visual_compression.py:100-175
 * ------------------------------------------------------------------------------------------- */

/* D1-D2  visual_compression.py:100-106  F.cosine_similarity(mb[:, :-1], mb[:, 1:], dim=-1),
 * `1 - sim.float()`, cat(ones).   x [T,N,C] (contiguous) -> dis [T,N] fp32, row 0 = 1.0.
 * RTK_BF16 reproduces the reference's bf16 rounding chain (norm, quotient, product, sum). */
int rtk_dpselect_dis(const void* x, int T, int N, int C, int dtype, float* dis, rtk_stream_t stream);

/* D3-D6  visual_compression.py:108-135 (sync) / :142-169 (async): patch mean, argrelmax peaks
 * (max_pool1d_with_indices window, first index wins), +2 bonus, topk(tgt) + ascending sort.
 *   dis   [T,N] fp32 (not modified)
 *   idx   sync: [tgt] int64;  async: [tgt,N] int64 (column n = patch n)
 *   mask  [tgt,N] bytes (keypatches_mask before .flatten())
 *   keys  workspace AND output: async [N,T] fp32 — the keys after the +2 bonus; sync [2,T]: row 0 the
 *         keys, row 1 the patch-mean distance dis.mean(1)
 * Ties at the k-th boundary are taken lowest index first (torch's order is backend-specific).
 * async with N == 1 returns RTK_EREFCRASH (the reference raises IndexError, :153-156). */
int rtk_dpselect_select(const float* dis, int T, int N, int tgt, int window, int sync,
                        int64_t* idx, uint8_t* mask, float* keys, rtk_stream_t stream);

/* D7  visual_compression.py:138 (sync `mb[:, peaks]`) / :173 (async `mb.gather(1, ...)`).
 * x [T,N,C] -> out [tgt,N,C]; idx as produced by rtk_dpselect_select. */
int rtk_gather_frames(const void* x, int T, int N, int C, int dtype, const int64_t* idx, int tgt, int sync,
                      void* out, rtk_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * MA-LLM / MA-LLM-hard merges — replaces retake/visual_compression.py:5-47 and :50-83 (one merge step;
 * the caller loops until the target frame count is reached, qwen2_vl.py:402-410)
 * ------------------------------------------------------------------------------------------- */

/* :19 / :63  F.cosine_similarity(mb[:, :-1], mb[:, 1:], dim=-1): x [T,N,C] -> cos_out [T-1,N] fp32 holding
 * the value in the INPUT dtype (RTK_BF16: the reference's bf16 rounding chain). */
int rtk_adjacent_cosine(const void* x, int T, int N, int C, int dtype, float* cos_out, rtk_stream_t stream);

/* :20-24 / :64-67  idx[n] = first arg-max over t of cos[t,n]; sync != 0: arg-max of the patch-mean row
 * (rounded to bf16 when round_bf16 != 0), written to every n.  cos [T1,N] fp32, idx [N] int64.
 * The order is torch.max's: NaN (a zero fp16 row: 0 / 0) counts as the maximum, and among equal maxima - several
 * NaNs included - the lowest t wins.  rtk_mallm_hard_chain takes every step by the same rule. */
int rtk_mallm_argmax(const float* cos, int T1, int N, int sync, int round_bf16, int64_t* idx, rtk_stream_t stream);

/* :26-46 / :69-82  the merge: x [T,N,C], sizes [T,N] (dtype of x; soft merge only) -> out [T-1,N,C],
 * sizes_out [T-1,N].  hard == 0: out[t] = (x[d]*s[d]) / s[d] with d = t + (t > idx), and at t = idx the
 * size-weighted mean of frames idx and idx+1, one rounding per torch op; hard != 0: out[t] = x[t + (t >= idx)]
 * (sizes / sizes_out may be NULL). */
int rtk_mallm_merge(const void* x, const void* sizes, const int64_t* idx, int T, int N, int C, int dtype,
                    int hard, void* out, void* sizes_out, rtk_stream_t stream);

/* MA-LLM-hard run to its target length in one call (the reference loops the single step, qwen2_vl.py:406-408: one
 * full pass over the bank per dropped frame).  A hard merge only drops the first frame of the most similar pair, so
 * every other adjacent cosine of the next step is the one already computed: per step ONE new pair is scored (at every
 * patch position when sync) with rtk_adjacent_cosine's arithmetic, bit for bit.  x [T,N,C] -> the surviving frame
 * indices, ascending: async idx [tgt,N] int64 (column n = patch n), sync idx [tgt]; gather the rows with
 * rtk_gather_frames (sync flag alike).  cos_ws: [T-1,N] fp32 scratch.  RTK_EUNSUPPORTED for rows that are not 16-byte
 * vectors or T beyond the LDS-resident frame list (~12 000): loop the single step. */
int rtk_mallm_hard_chain(const void* x, int T, int N, int C, int dtype, int tgt, int sync, float* cos_ws,
                         int64_t* idx_out, rtk_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * RoPE tables — replaces longvideo_cache.py:68-74 (M-RoPE section merge) and, optionally, the
 * rotary_emb_fn(...) calls at :249 and :298 when the rotary module is the standard
 * inv_freq/attention_scaling kind.
 * ------------------------------------------------------------------------------------------- */

/* Merge the [P,L,D] cos and sin returned by rotary_emb_fn (P = 3 for M-RoPE, 1 otherwise; dtype of
 * q) into fp32 [L,D] tables.  sections = mrope_section (host pointer, nsec ints; NULL for P = 1);
 * channel block i of `mrope_section*2` takes row i % 3. */
int rtk_rope_merge(const void* cos_in, const void* sin_in, int P, int L, int D, int dtype,
                   const int* sections_host, int nsec, float* cos_out, float* sin_out, rtk_stream_t stream);

/* Build the merged fp32 [L,D] tables directly from position ids: cos(pos*inv_freq)*scaling.
 * pos [P,L] int64 (row p at pos + p*pos_stride, pos_stride >= L), inv_freq [D/2] fp32.  round_bf16 != 0
 * rounds the table entries to bf16 (what a bf16 model's rotary module returns). */
int rtk_rope_table(const int64_t* pos, int64_t pos_stride, int P, int L, const float* inv_freq, int D,
                   float attention_scaling,
                   const int* sections_host, int nsec, int round_bf16, float* cos_out, float* sin_out,
                   rtk_stream_t stream);

/* Forward rotation in place of UN-rotated key rows at given ids (longvideo_cache.py:297-306 for rows whose re-rotation
 * was deferred, see rtk_pivotkv_batch.defer_rot): k [layers, H, rows, D] (element strides stride_layer, stride_h; rows
 * contiguous), ids of layer l at pos + l*pos_stride_layer, row p of them at + p*pos_stride_p (P = 1 or 3).
 * k' = (k*cos) + (rotate_half(k)*sin), the tables and roundings of rtk_pivotkv_evict_batched_rope, bit for bit. */
int rtk_rope_rotate_rows(void* k, int64_t stride_layer, int64_t stride_h, int layers, int H, int rows, int D, int dtype,
                         const int64_t* pos, int64_t pos_stride_layer, int64_t pos_stride_p, int P, const float* inv_freq,
                         float attention_scaling, const int* sections_host, int nsec, int round_mode, rtk_stream_t stream);

/* In-place k <- R(delta) k on the temporal channels (position row 0; every channel when P = 1) of keys
 * that are already rotated: k [H, n, D] with head stride `stride_h`, delta = one int64 in device
 * memory.  Used by the multi-GPU sharding (retake/sharded.py): ranks compress their chunks at
 * provisional temporal ids; once the global offsets are known, R(p + delta) = R(delta) R(p)
 * (longvideo_cache.py:80-81 composed with the continuity shift of qwen2_vl.py:68-73).
 * rtk_rope_shift and rtk_rope_shift_segments are NOT called by the package any more (finalize keeps the kept keys
 * un-rotated and rotates them once with rtk_rope_rotate_rows); they stay in the ABI and are tested on their own against
 * float64 (tests/test_rope_gpu.py). */
int rtk_rope_shift(void* k, int64_t stride_h, int H, int n, int D, int dtype, const int64_t* delta_dev,
                   const float* inv_freq, int P, const int* sections_host, int nsec, rtk_stream_t stream);

/* The same for a whole assembled cache in one launch: k [layers, H, world * seg, D] (element strides stride_layer,
 * stride_h; rows contiguous), the segment of rank r in layer l rotated by table_dev[r * layers + l] temporal steps
 * (table_dev: device int64 [world, layers], what retake/sharded.exchange_temporal_offsets returns): the arithmetic of
 * layers x world calls of rtk_rope_shift, bit for bit. */
int rtk_rope_shift_segments(void* k, int64_t stride_layer, int64_t stride_h, int layers, int H, int world, int seg, int D,
                            int dtype, const int64_t* table_dev, const float* inv_freq, int P,
                            const int* sections_host, int nsec, rtk_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * PivotKV — replaces retake/longvideo_cache.py:248-318
 * ------------------------------------------------------------------------------------------- */

/* Workspace (bytes) needed by rtk_pivotkv_score for these sizes. */
size_t rtk_pivotkv_score_workspace_bytes(int Hq, int Hkv, int L, int D, int dtype);

/* P2-P5  longvideo_cache.py:248-270.
 *   q [Hq,L,D], k [Hkv,L,D]: element (h,l,d) at h*stride_h + l*stride_l + d  (post-RoPE, as the
 *   attention patch hands them over).
 *   cos/sin: fp32 [L,D] merged tables or NULL.  Non-NULL = pos_embed_reforge: q and k are first
 *   un-rotated, x~ = ((x*cos) - (rotate_half(x)*sin)) / attention_scaling^2   (:76-78, :109-111).
 *   score [L] fp32 = mean_g mean_{h in g} sum_i softmax_j(q~_h,i . k~_g,j / sqrt(D))  — keys are the
 *   current chunk only, no causal mask (:264-270).
 *   k_unrot (optional, may be NULL): receives k~ [Hkv,L,D] contiguous in `dtype` for rtk_pivotkv_evict_batched.
 * The [Hq,L,L] probability tensor is never materialised. */
int rtk_pivotkv_score(const void* q, int64_t q_stride_h, int64_t q_stride_l,
                      const void* k, int64_t k_stride_h, int64_t k_stride_l,
                      int Hq, int Hkv, int L, int D, int dtype,
                      const float* cos, const float* sin, float attention_scaling,
                      float* score, void* k_unrot, void* workspace, size_t workspace_bytes,
                      rtk_stream_t stream);

/* The same computation cut into its three stream-ordered stages, so that a caller can put the two big
 * matrix kernels of consecutive updates back to back on one stream while the small pre / post kernels of the
 * neighbouring updates run on other streams (PivotKVCache pipeline_streams): same arguments, same workspace.
 *   RTK_SCORE_PREPARE   un-rotate + pack q~ (workspace) and k~ (k_unrot or workspace)
 *   RTK_SCORE_PASSES    pass 1, lse combine, pass 2 (reads q~/k~, writes the column partials)
 *   RTK_SCORE_FINALIZE  fixed-order reduction of the partials -> score */
enum rtk_score_stage { RTK_SCORE_PREPARE = 1, RTK_SCORE_PASSES = 2, RTK_SCORE_FINALIZE = 4 };
int rtk_pivotkv_score_stages(const void* q, int64_t q_stride_h, int64_t q_stride_l,
                             const void* k, int64_t k_stride_h, int64_t k_stride_l,
                             int Hq, int Hkv, int L, int D, int dtype,
                             const float* cos, const float* sin, float attention_scaling,
                             float* score, void* k_unrot, void* workspace, size_t workspace_bytes,
                             int stages, float* partial_out /* NULL = inside workspace */, rtk_stream_t stream);

/* The same with the chunk's key-patch mask ([L] bytes, may be NULL) and int32 scratch of L + 1 entries: pass 2 then
 * computes the column partials of the UNMASKED tokens only (the caller's selection overwrites the masked tokens' score
 * with 1.0, longvideo_cache.py:272-274) and the masked entries of partial / score hold no meaning until that override.
 * head_dim 128 kernels; other shapes ignore the mask. */
int rtk_pivotkv_score_stages_masked(const void* q, int64_t q_stride_h, int64_t q_stride_l,
                                    const void* k, int64_t k_stride_h, int64_t k_stride_l,
                                    int Hq, int Hkv, int L, int D, int dtype,
                                    const float* cos, const float* sin, float attention_scaling,
                                    float* score, void* k_unrot, void* workspace, size_t workspace_bytes,
                                    int stages, float* partial_out, const void* key_mask, int32_t* key_index_ws,
                                    rtk_stream_t stream);

/* Fused form of {rtk_rope_table, RTK_SCORE_PREPARE, rtk_pivotkv_append} for the standard inv_freq rotary
 * modules (longvideo_cache.py:238, :248-259): one pass over the chunk's q, k, v that builds each token's
 * cos/sin in registers (same arithmetic and rounding as rtk_rope_table), writes q~ into `workspace` (where
 * rtk_pivotkv_score_stages(RTK_SCORE_PASSES) expects it) and k~ into k_unrot, and appends k and v to the cache
 * tail.  Needs 16-byte aligned pointers / strides; returns RTK_EUNSUPPORTED otherwise (use the three calls). */
int rtk_pivotkv_prepare(const void* q, int64_t q_stride_h, int64_t q_stride_l,
                        const void* k, int64_t k_stride_h, int64_t k_stride_l,
                        const void* v, int64_t v_stride_h, int64_t v_stride_l,
                        int Hq, int Hkv, int L, int D, int dtype,
                        const int64_t* pos, int64_t pos_stride, int P, const float* inv_freq, float attention_scaling,
                        const int* sections_host, int nsec, int round_bf16,
                        void* k_unrot, void* workspace, size_t workspace_bytes,
                        void* k_tail, void* v_tail, int64_t tail_stride_h,
                        int64_t* pos_copy /* optional [P, L]: private copy of the ids for a deferred selection */,
                        rtk_stream_t stream);

/* RTK_SCORE_PASSES for n_units (layer, chunk) units in ONE launch per kernel (blockIdx.y = unit): the units'
 * score workspaces (holding q~ from RTK_SCORE_PREPARE / rtk_pivotkv_prepare), their k~ buffers (k_unrot0 == NULL:
 * inside the workspaces) and their partial outputs lie workspace_stride / k_unrot_stride bytes and
 * partial_stride_floats floats apart.  bf16, head_dim 128 (RTK_EUNSUPPORTED otherwise: run the stage per unit).
 * What PivotKVCache runs from after_forward for all layers of a chunk: 28x larger grids, no per-layer tails.
 * Live keys (optional; both NULL = every column): key_masks_host is a HOST array of n_units device pointers to the units'
 * key-patch masks ([L] bytes, entries may be NULL); key_index_ws is device scratch of n_units * (L + 1) int32.  The
 * reference overwrites the score of every masked token with 1.0 after the scoring (longvideo_cache.py:272-274), so
 * pass 2 - one column mass per key - runs on the unit's unmasked keys only and leaves the masked columns of `partial`
 * UNWRITTEN (the selection's mask override never reads them); every other column gets the bits it always got.  The
 * same mask must be handed to rtk_pivotkv_select_batched. */
int rtk_pivotkv_score_passes_batched(void* workspace0, size_t workspace_stride, void* k_unrot0, size_t k_unrot_stride,
                                     float* partial0, size_t partial_stride_floats, int n_units,
                                     int Hq, int Hkv, int L, int D, int dtype,
                                     const void* const* key_masks_host, int32_t* key_index_ws, rtk_stream_t stream);

/* The same with the units' queries read in place: q_units_host is a HOST array of n_units device pointers to tensors the
 * caller keeps alive until the launches have run, element (h, i, d) of unit u at q_units_host[u] + h*q_stride_h +
 * i*q_stride_l + d (elements; 16-byte aligned rows).  For units whose score operands ARE the caller's tensors - the
 * pre-RoPE projections of the attention prologue - no packed copy of the queries is made at all.  NULL: identical to
 * rtk_pivotkv_score_passes_batched.  16-bit payloads, head_dim 128. */
int rtk_pivotkv_score_passes_batched_q(void* workspace0, size_t workspace_stride, void* k_unrot0, size_t k_unrot_stride,
                                       float* partial0, size_t partial_stride_floats, int n_units,
                                       int Hq, int Hkv, int L, int D, int dtype,
                                       const void* const* key_masks_host, int32_t* key_index_ws,
                                       const void* const* q_units_host, int64_t q_stride_h, int64_t q_stride_l,
                                       rtk_stream_t stream);

/* Prompt-guided scoring (kvcache_compression_kwargs["prompt_guided_scoring"]; NOT in the reference, whose
 * PivotKVCache.before_forward ignores prompt_length): the chunk's L rows are Lv = L - Lp video rows followed by the Lp rows
 * of the appended prompt, and the video keys are scored by the prompt's queries alone -
 *   score[j] = mean_g mean_{h in g} (1/Lp) sum_{i in [Lv,L)} softmax_{j' in [0,Lv)}(q~[h,i] . k~[g,j'] / sqrt(D))[j]
 * for j < Lv: softmax over the video keys only, no causal mask, prompt keys never read; every score is < 1.  Arithmetic of
 * the RTK_F32 / RTK_BF16 / RTK_F16 codes (exact products, fp32 accumulation, softmax and sums; RTK_EUNSUPPORTED for the
 * other codes).  One call serves 1 .. 28 (layer, chunk) units laid out as for rtk_pivotkv_score_passes_batched_q: the units'
 * score workspaces (q~ [Hq, L, D] at offset 0 from RTK_SCORE_PREPARE / rtk_pivotkv_prepare / rtk_pivotkv_update), their k~
 * [Hkv, L, D] (k_unrot0 == NULL: inside the workspaces), optionally the queries read in place through q_units_host +
 * element strides (workspace0 may then be NULL when k_unrot0 is given).  Reads rows [Lv, L) of q~ and rows [0, Lv) of k~;
 * writes the FINAL score[0 .. Lv) of unit u at score0 + u * score_stride_floats (entries >= Lv are not touched).
 * scratch0: rtk_pivotkv_score_prompt_workspace_bytes per unit, units scratch_stride bytes apart, 256-byte aligned (the
 * rows' log-sum-exps between the two launches).  bf16 / fp16 with head_dim 128: MFMA kernels whose row operand packs the
 * G * Lp query rows of a KV group into 32-row blocks (pivotkv_score_prompt.hip); fp32 or any other head_dim: plain FMA,
 * the parity path.  No atomics; every sum runs in an order fixed by the shape, so two runs give the same bits. */
size_t rtk_pivotkv_score_prompt_workspace_bytes(int Hq, int Hkv, int L, int Lp, int D, int dtype);
int rtk_pivotkv_score_prompt_batched(void* workspace0, size_t workspace_stride, void* k_unrot0, size_t k_unrot_stride,
                                     float* score0, size_t score_stride_floats, void* scratch0, size_t scratch_stride,
                                     int n_units, int Hq, int Hkv, int L, int Lp, int D, int dtype,
                                     const void* const* q_units_host, int64_t q_stride_h, int64_t q_stride_l,
                                     rtk_stream_t stream);

/* P6-P7, P9-P10  longvideo_cache.py:272-277, :283-295.
 *   score [L] fp32: entries with mask != 0 are overwritten with 1.0 IN PLACE (masked_fill_, :274);
 *   mask may be NULL.
 *   keep_idx [keep] int64 ascending = topk(keep).sort()  (ties: lowest index first)
 *   rank [L] int32: position of token l in keep_idx, or -1 if evicted (inverse map, for callers that
 *        scan tokens in order); may be NULL when a workspace is given
 *   pos [P,L] int64 (P = 3 M-RoPE rows t,h,w or 1), may be NULL together with pos_out;
 *   pos_out [P,keep] int64 (row p at pos_out + p*pos_out_stride, pos_out_stride >= keep) = gathered ids;
 *       if reforge != 0 row 0 becomes
 *       tmin + (int64)((float)(t - tmin) * (float)(keep / (double)L))        (:293-295)
 *   workspace: rtk_pivotkv_select_workspace_bytes(L) bytes of device scratch.  With it the selection runs
 *       chip-wide (rank-by-counting over ~L/32 workgroups + an ordered emit); without it (NULL) on one
 *       workgroup (radix select).  Same exact result either way. */
size_t rtk_pivotkv_select_workspace_bytes(int L);
int rtk_pivotkv_select(float* score, const uint8_t* mask, int L, int keep,
                       const int64_t* pos, int P, int reforge,
                       int64_t* keep_idx, int32_t* rank, int64_t* pos_out, int64_t pos_out_stride,
                       void* workspace, size_t workspace_bytes, rtk_stream_t stream);

/* The selection of n (layer, chunk) units in the same three launches (finalize of the column partials ->
 * rank -> emit): what PivotKVCache runs from after_forward for all layers of a chunk.  Units share L, keep, P
 * and the partial layout (Hkv, RS, G as reported by rtk_pivotkv_score_partials).  RTK_EUNSUPPORTED for L < 512
 * (call rtk_pivotkv_select per unit).  Fewer than 8 units are ranked chip-wide one after the other; 8 or more
 * (L <= 16384) get one radix-select workgroup each (keys in LDS), all side by side - same result, bit for bit.
 * `units` is a HOST array. */
typedef struct rtk_select_unit {
    const float* partial;   /* column partials [Hkv, RS, L] written by RTK_SCORE_PASSES (partial_out), or NULL: score is final */
    float* score;           /* [L] fp32 (written from the partials, masked entries overwritten with 1.0) */
    const uint8_t* mask;    /* [L] key-patch mask or NULL */
    const int64_t* pos;     /* [P, L] position ids (row stride L) or NULL */
    int64_t* keep_idx;      /* [keep] */
    int32_t* rank;          /* [L] or NULL */
    int64_t* pos_out;       /* rows at pos_out + p*pos_out_stride, or NULL */
    void* workspace;        /* rtk_pivotkv_select_workspace_bytes(L), 256-byte aligned */
} rtk_select_unit;
#define RTK_SELECT_MAX_UNITS 28
int rtk_pivotkv_select_batched(const rtk_select_unit* units, int n_units, int Hkv, int RS, int G, int L,
                               int keep, int P, int reforge, int64_t pos_out_stride,
                               int score_dtype /* RTK_BF16_REFROUND / RTK_F16_REFROUND: partials are per head
                                                  [Hkv*G, RS, L] and the finalize applies the reference's roundings; else 0 */,
                               rtk_stream_t stream);

/* Layout of the column partials rtk_pivotkv_score_stages(RTK_SCORE_PASSES) produces for these sizes: returns the
 * number of floats (Hkv * RS * L) and writes RS (row splits actually used) to *rs_out. */
size_t rtk_pivotkv_score_partials(int Hq, int Hkv, int L, int D, int dtype, int* rs_out);

/* ---------------------------------------------------------------------------------------------
 * Chunk-batched cache maintenance.  The reference rebuilds every layer's cache with two torch.cat per
 * (layer, chunk) (longvideo_cache.py:238, :313-318) and calls cache.after_forward() once per video
 * chunk (qwen2_vl.py:715-716).  Here `update` appends the chunk to the pre-allocated cache tail and
 * records which rows survive; the gather / re-rotation / compaction of every layer of the chunk runs
 * as ONE launch each from after_forward (or from whatever touches the cache first).
 * ------------------------------------------------------------------------------------------- */

/* P1  longvideo_cache.py:238 (DynamicCache.update -> torch.cat): K and V rows of the chunk
 * (element (h,l,d) at h*stride_h + l*stride_l + d) -> k_tail/v_tail (element (h,l,d) at
 * h*tail_stride_h + l*D + d), the uncompressed view the current layer's attention reads. */
int rtk_pivotkv_append(const void* k, int64_t k_stride_h, int64_t k_stride_l,
                       const void* v, int64_t v_stride_h, int64_t v_stride_l,
                       int Hkv, int L, int D, int dtype,
                       void* k_tail, void* v_tail, int64_t tail_stride_h, rtk_stream_t stream);

/* One (layer, chunk) unit of a batched eviction.  Strides in elements. */
typedef struct rtk_evict_unit {
    const void* k_src;        /* K rows of the chunk, element (h,l,d) at h*k_src_stride_h + l*D + d.  With cos_new:
                                 the UN-rotated k~ written by rtk_pivotkv_score; without: the rotated rows */
    int64_t k_src_stride_h;
    const void* v_src;        /* V rows of the chunk, element (h,l,d) at h*v_src_stride_h + l*D + d */
    int64_t v_src_stride_h;
    const int64_t* keep_idx;  /* [keep] ascending, from rtk_pivotkv_select */
    const float* cos_new;     /* fp32 [keep,D] tables of the NEW positions of the kept rows, or NULL (no reforge) */
    const float* sin_new;
    void* k_dst;              /* kept row (h,r) at h*k_dst_stride_h + r*D; must not alias k_src.  NULL: K is left alone */
    int64_t k_dst_stride_h;
    void* v_dst;              /* kept row (h,r) at h*v_dst_stride_h + r*D; must not alias v_src.  NULL: V is left alone
                                 (keep == L: every row already sits where the append put it) */
    int64_t v_dst_stride_h;
    const int64_t* pos_src;   /* optional: ids of the kept rows [P,keep] (row stride pos_src_stride) ... */
    int64_t pos_src_stride;
    int64_t* pos_dst;         /* ... copied to the layer's position cache tail (row stride pos_dst_stride) */
    int64_t pos_dst_stride;
} rtk_evict_unit;
#define RTK_EVICT_MAX_UNITS 28   /* units per launch (the array travels as a kernel argument); more = more launches */

/* P8, P9, P11, P12  longvideo_cache.py:278-288, :297-310 for n_units (layer, chunk) units that share
 * Hkv, D, keep, P and dtype:  K: k' = (k~*cos_new) + (rotate_half(k~)*sin_new) (or a copy), V: copy,
 * position ids: copy.  `units` is a HOST array. */
int rtk_pivotkv_evict_batched(const rtk_evict_unit* units, int n_units, int Hkv, int D, int keep, int P,
                              int dtype, int stage_low_only, rtk_stream_t stream);
/* stage_low_only bit 1 (value 3 together with bit 0): K is copied verbatim from a buffer of its own (k_src is not the
 * tail k_dst lies in - the un-rotated rows of a deferred re-rotation): EVERY kept K row is written to k_dst.
 * stage_low_only != 0 (what PivotKVCache uses, together with rtk_pivotkv_place_batched): rows that are copied verbatim
 * (V; K when there are no tables) are written to k_dst / v_dst ONLY when keep_idx[r] < keep, i.e. when their source
 * lies inside the destination range of the compaction and has to be parked; the other rows are moved in place by
 * rtk_pivotkv_place_batched.  Re-rotated K rows are always written. */

/* The same with the tables of the NEW ids computed in the kernel (reference :297-298: rotary_emb(compressed ids) and
 * the M-RoPE section merge :68-74, i.e. rtk_rope_table's arithmetic: fp32 sincosf(id * inv_freq[d mod D/2]) *
 * attention_scaling, rounded to bf16 when round_bf16): every unit needs pos_src (the kept rows' new ids, [P, keep])
 * and cos_new = sin_new = NULL.  P = 1 (plain RoPE) or 3 (M-RoPE with `sections`).  Saves the table launch and
 * 2 x keep x D x 4 bytes of write + read per unit. */
int rtk_pivotkv_evict_batched_rope(const rtk_evict_unit* units, int n_units, int Hkv, int D, int keep, int P,
                                   int dtype, const float* inv_freq, float attention_scaling,
                                   const int* sections_host, int nsec, int round_bf16, int stage_low_only,
                                   rtk_stream_t stream);

typedef struct rtk_copy_unit {
    const void* src;
    int64_t src_stride_h_bytes;
    void* dst;
    int64_t dst_stride_h_bytes;
} rtk_copy_unit;
#define RTK_COPY_MAX_UNITS 64

/* P13  longvideo_cache.py:313-318 for n_units staged row blocks: dst[h][r][:] = src[h][r][:], r < rows.
 * `units` is a HOST array. */
int rtk_pivotkv_commit_batched(const rtk_copy_unit* units, int n_units, int H, int rows, int D, int dtype,
                               rtk_stream_t stream);

/* P13 without a full staging copy: for every unit, kept row r (r < keep) of the tail block `tail` (element (h, l, d) at
 * h*tail_stride_h_bytes + l*D*es) becomes row r of the same block.  Its source is chunk row keep_idx[r]: read in place
 * when keep_idx[r] >= keep (outside the destination range), from stage[h][r] otherwise (parked there by
 * rtk_pivotkv_evict_batched with stage_low_only).  Only ~ratio of the kept rows take the staging hop.  One unit per
 * tensor (V of a layer; K of a layer when it is not re-rotated).  `units` is a HOST array. */
typedef struct rtk_place_unit {
    const void* stage;             /* [H, keep, D] staged rows (only rows with keep_idx[r] < keep are read) */
    int64_t stage_stride_h_bytes;
    void* tail;                    /* the uncompressed chunk inside the cache: rows [0, L) per head */
    int64_t tail_stride_h_bytes;
    const int64_t* keep_idx;       /* [keep] ascending */
} rtk_place_unit;
#define RTK_PLACE_MAX_UNITS 64
int rtk_pivotkv_place_batched(const rtk_place_unit* units, int n_units, int H, int keep, int D, int dtype,
                              rtk_stream_t stream);

/* P8-P13 in ONE launch, in place (ABI 14): longvideo_cache.py:278-288, :297-310, :313-318 for n_units (layer, chunk)
 * units that share Hkv, D, keep, P and dtype - what rtk_pivotkv_evict_batched[_rope] + rtk_pivotkv_place_batched do in
 * two launches with a staging hop.  Kept row r of a unit's V tail (and K tail, k_mode RTK_COMPACT_K_INPLACE) comes from
 * chunk row keep_idx[r] >= r of the SAME tail: the workgroups of a unit run in ticket order and store a row block only
 * after every lower block has its source rows in registers, so nothing is staged and the kernel moves
 * 4 x keep x Hkv x D x es bytes per unit.  Same arithmetic, same bits as rtk_pivotkv_evict_batched_rope. */
typedef struct rtk_compact_unit {
    const void* k_src;        /* RTK_COMPACT_K_ROTATE / _COPY: K rows of the chunk in a buffer of their own (the un-rotated
                                 k~), element (h,l,d) at h*k_src_stride_h + l*D + d.  _INPLACE: ignored */
    int64_t k_src_stride_h;
    void* k_tail;             /* the chunk inside the layer's cache: chunk row l of head h at h*k_tail_stride_h + l*D;
                                 kept row r is written to row r of the same block */
    int64_t k_tail_stride_h;
    void* v_tail;
    int64_t v_tail_stride_h;
    const int64_t* keep_idx;  /* [keep] ascending, from rtk_pivotkv_select[_batched] */
    const int64_t* pos_src;   /* ids of the kept rows [P, keep] (row stride pos_src_stride): the NEW ids the rotation
                                 uses (RTK_COMPACT_K_ROTATE: required) ... */
    int64_t pos_src_stride;
    int64_t* pos_dst;         /* ... copied to the layer's position cache tail (row stride pos_dst_stride), or NULL */
    int64_t pos_dst_stride;
} rtk_compact_unit;
#define RTK_COMPACT_MAX_UNITS 28   /* units per launch (the array travels as a kernel argument) */
enum rtk_compact_k_mode {
    RTK_COMPACT_K_ROTATE = 0,   /* kept K = k_src row re-rotated at its new ids (pos_embed_reforge, :297-306) */
    RTK_COMPACT_K_COPY = 1,     /* kept K = k_src row verbatim (deferred re-rotation: rtk_pivotkv_batch.defer_rot) */
    RTK_COMPACT_K_INPLACE = 2   /* kept K = row keep_idx[r] of k_tail, compacted in place like V (no reforge, :279) */
};
/* ints of the sync workspace for this geometry: device memory, zero-initialised once by the caller (tickets and flags of
 * the workgroups live in it; every launch that completes leaves it zeroed again, and a call that fails at a launch
 * re-zeroes it on `stream` before returning).  A kernel that aborts on the device (its bounded flag wait traps instead
 * of hanging) leaves the HIP context in error: the workspace - like every other buffer - is then to be re-created. */
size_t rtk_pivotkv_compact_sync_ints(int n_units, int Hkv, int keep, int D, int dtype);
/* `units` is a HOST array.  inv_freq / attention_scaling / sections / round_mode as rtk_pivotkv_evict_batched_rope
 * (RTK_COMPACT_K_ROTATE only).  One launch at a time per workspace: calls that share a workspace must be ordered on
 * ONE stream (PivotKVCache flushes a batch on the caller's current stream only). */
int rtk_pivotkv_compact_batched(const rtk_compact_unit* units, int n_units, int Hkv, int D, int keep, int P, int dtype,
                                int k_mode, const float* inv_freq, float attention_scaling, const int* sections_host,
                                int nsec, int round_mode, int32_t* sync_ws, size_t sync_ws_ints, rtk_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * One-call update and one-call flush (ABI 13).  PivotKVCache.update runs 1,792 times per 2048-frame video and
 * the reference calls cache.after_forward() once per chunk (qwen2_vl.py:715-716): on MI355X the per-call HOST work
 * around the launches decides the real-geometry step, so the argument blocks are bound ONCE per chunk geometry
 * (rtk_pivotkv_batch, HOST memory owned by the caller) and per layer (rtk_layer_state, HOST memory owned by the
 * caller, updated by the library), and each update / flush is ONE call that fills in the launches the
 * entry points above would have been handed one by one.  Nothing new is computed here:
 *   rtk_pivotkv_update  = rtk_pivotkv_prepare (rotated q, k)  or the attention prologue (pre-RoPE q, k; below)
 *   rtk_pivotkv_flush   = rtk_pivotkv_score_passes_batched + rtk_pivotkv_select_batched +
 *                         rtk_pivotkv_compact_batched (or, without batch.compact_sync, rtk_pivotkv_evict_batched[_rope] +
 *                         rtk_pivotkv_place_batched) for the pending layers
 * ------------------------------------------------------------------------------------------- */

/* One layer's pre-allocated cache (longvideo_cache.py: key_cache[l] / value_cache[l] / position_cache[l]).
 * Rewinding (a follow-up question on the same video; PivotKVCache.mark / rewind): the rows below `length` / `pos_len` are
 * never rewritten by later calls - a compressed chunk compacts inside its own tail, rtk_pivotkv_append_rope appends at
 * `length` - so a foreign host goes back to an earlier state by restoring `length` and `pos_len` (with nothing pending)
 * and its own count of archived fp8 rows; no call into the library, no copy. */
typedef struct rtk_layer_state {
    void* k;                 /* [1, Hkv, cap, D] keys   (element (h, r, d) at (h*cap + r)*D + d) */
    void* v;                 /* [1, Hkv, cap, D] values */
    int64_t cap;             /* rows allocated per head */
    int64_t length;          /* committed (compressed) rows                                  - advanced by rtk_pivotkv_flush */
    int64_t pending;         /* uncompressed chunk rows at [length, length + pending)        - set by update, cleared by flush */
    int64_t pending_keep;    /* rows of them that survive                                                                      */
    int64_t* pos;            /* [P, pos_cap] position ids of the cached rows (pos_embed_reforge) or NULL */
    int64_t pos_cap;
    int64_t pos_len;         /*                                                              - advanced by rtk_pivotkv_flush */
    const uint8_t* mask;     /* the pending chunk's key-patch mask [L] or NULL (cache.keypatches_mask_chunk, :272-274) */
} rtk_layer_state;

/* The per-chunk batch: geometry + the slot-strided scratch of all layers (slot = layer index).  Every buffer is
 * caller-allocated device memory; sizes as the per-stage entry points document them. */
typedef struct rtk_pivotkv_batch {
    int32_t Hq, Hkv, L, D, keep, P, slots;
    int32_t dtype;            /* payload: RTK_F32 / RTK_BF16 / RTK_F16 */
    int32_t score_dtype;      /* what the scoring entry points are told (may carry RTK_SCORE_MANY_UNITS) */
    int32_t prep_dtype;       /* what rtk_pivotkv_prepare is told */
    int32_t reforge;          /* pos_embed_reforge */
    int32_t keep_all;         /* keep == L and no scores wanted: selection is the identity, no score passes */
    int32_t round_mode;       /* 0 fp32 / 1 bf16 / 2 fp16 rotary tables */
    int32_t nsec;
    int32_t sections[8];      /* mrope_section (nsec entries; nsec = 0: plain RoPE) */
    int32_t rs_n;             /* row splits of the column partials (rtk_pivotkv_score_partials) */
    int32_t skip_masked;      /* pass 2 on the unmasked keys only */
    float attention_scaling;
    int32_t defer_rot;        /* pos_embed_reforge with the re-rotation of the kept keys deferred: the flush copies the
                                 UN-rotated kept rows into the cache and their ids into the position cache; the owner
                                 rotates them once, at their final ids, with rtk_rope_rotate_rows (chunk-sharded prefill:
                                 a block's temporal offset is known only when the blocks before it are done) */
    const float* inv_freq;    /* [D/2] fp32 */
    void* score_ws;           /* slot s at score_ws + s*score_ws_stride (256-byte aligned): q~, lse, ... */
    uint64_t score_ws_stride, score_ws_bytes;
    void* k_unrot;            /* [slots, Hkv, L, D] un-rotated keys */
    float* partials;          /* [slots, partial_floats] */
    uint64_t partial_floats;
    float* score;             /* [slots, L] */
    int64_t* pos_old;         /* [slots, P, L] ids of the pending chunks (after the continuity shift) */
    int64_t* keep_idx;        /* [slots, keep] */
    int64_t* pos_new;         /* [P, slots, keep] */
    void* sel_ws;             /* slot s at sel_ws + s*sel_ws_stride */
    uint64_t sel_ws_stride;
    int32_t* key_index;       /* [slots, L + 1] */
    void* v_stage;            /* [slots, Hkv, keep, D] */
    void* k_stage;            /* [slots, Hkv, keep, D] (no reforge only, else NULL) */
    int64_t* shift_row;       /* RTK_UPDATE_PRE_ROPE: the caller's temporal-id row; rtk_pivotkv_flush applies the last
                                 pending layer's continuity shift to it in place (qwen2_vl.py:73), then clears this field */
    const void** q_units;     /* HOST array [slots] or NULL.  Non-NULL entries of the pending slots: the unit's queries are
                                 scored where they are (RTK_UPDATE_Q_IN_PLACE; element strides below), all pending units alike */
    int64_t q_stride_h, q_stride_l;
    int32_t pre_rope;         /* the pending units were appended from pre-RoPE projections: 1 k~ == k0 (pre-RoPE operands),
                                 2 k~ = the reference's un-rotation of the rotated row (RTK_UPDATE_ROUNDTRIP); 0 otherwise */
    int32_t batched_passes;   /* 1: the score passes of all pending layers run from rtk_pivotkv_flush, one launch per kernel
                                 (16-bit payloads, head_dim 128); 0: rtk_pivotkv_update runs them per unit */
    int32_t* compact_sync;    /* zero-initialised sync workspace of rtk_pivotkv_compact_batched for (slots, Hkv, keep, D,
                                 dtype), or NULL: the flush then stages through v_stage / k_stage (two launches) */
    uint64_t compact_sync_ints;
} rtk_pivotkv_batch;

/* The tensors of one update call.  Strides in elements; element (h, l, d) at h*stride_h + l*stride_l + d. */
typedef struct rtk_update_io {
    const void* q; int64_t q_stride_h, q_stride_l;   /* [Hq, L, D] */
    const void* k; int64_t k_stride_h, k_stride_l;   /* [Hkv, L, D] */
    const void* v; int64_t v_stride_h, v_stride_l;   /* [Hkv, L, D] */
    const int64_t* pos; int64_t pos_stride;          /* [P, L] ids of the chunk, row p at pos + p*pos_stride */
    void* q_rot; int64_t qr_stride_h, qr_stride_l;   /* RTK_UPDATE_PRE_ROPE: rotated queries out (may alias q) */
    int32_t flags;
    int32_t pad0;
    const int64_t* next_prev;                        /* RTK_UPDATE_SHIFT_NEXT (ABI 16): the NEXT layer's last cached temporal id */
    int32_t* ticket; int64_t ticket_ints;            /*   (device; NULL = -1); rtk_pivotkv_shift_ticket_ints(L, D) device words, */
                                                     /*   zeroed ONCE by the caller: word 0 launch count, word 31 the run-out   */
                                                     /*   LATCH (below), then the arrival counters, a cache line each           */
    int32_t* status;                                 /* (ABI 17) optional HOST-VISIBLE word (pinned host memory the device can   */
} rtk_update_io;                                     /*   write), zeroed by the caller: incremented when a launch's bounded     */
                                                     /*   wait runs out, so the host can see the latch without a device sync    */
size_t rtk_pivotkv_shift_ticket_ints(int L, int D);
enum rtk_update_flags {
    /* q, k are the PRE-RoPE projections (what q_proj / k_proj return).  One launch then does the whole prologue of the
     * attention patch (qwen2_vl.py:55-86, llava_onevision.py:59-141) and of PivotKVCache.update (:238, :248-259):
     *   continuity shift  t' = t + (prev + 1 - t[0]) on the temporal row, prev = the layer's last cached temporal id
     *                     (qwen2_vl.py:68-73; applied to the ids the kernel uses and to pos_old - the caller's tensor is
     *                     shifted in place by rtk_pivotkv_flush, see rtk_pivotkv_batch.shift_row);
     *   rotary tables     cos / sin of the shifted ids (rtk_rope_table's arithmetic, M-RoPE section merge :68-74);
     *   q_rot             = (q*cos) + (rotate_half(q)*sin), one rounding per torch op  -> the layer's attention;
     *   k tail, v tail    rotated k and v appended to the cache (:238);
     *   q~, k~            the un-rotated operands of the score passes are the inputs themselves (un-rotating
     *                     a rotation returns the pre-RoPE value up to rounding), copied to the score workspace / k_unrot.
     * Needs pos_embed_reforge and an inv_freq rotary (batch.inv_freq). */
    RTK_UPDATE_PRE_ROPE = 1,
    /* with RTK_UPDATE_PRE_ROPE and q_rot != q: no copy of the queries is made - the score passes of the flush read
     * io->q itself (the caller keeps it alive and unmodified until rtk_pivotkv_flush has run; the library records the
     * pointer and strides in batch->q_units).  16-bit payloads scored by the batched passes only. */
    RTK_UPDATE_Q_IN_PLACE = 2,
    /* with RTK_UPDATE_PRE_ROPE (ABI 15): q~ / k~ are what the REFERENCE scores and re-rotates - the un-rotation
     * ((x*cos) - (rotate_half(x)*sin)) / a^2 of the rotated rows this launch produced, one rounding of the model dtype
     * per torch op (longvideo_cache.py:76-78, :248-259) - instead of the inputs themselves.  On a bf16 / fp16 model the
     * round trip moves an operand by up to a few ulps, which is what the reference's scores and kept keys carry; with this
     * flag the score operands and the kept keys equal the reference's bit for bit (tables within one fp32 ulp of the rotary
     * module's).  Excludes RTK_UPDATE_Q_IN_PLACE; allows the reference-rounding score modes. */
    RTK_UPDATE_ROUNDTRIP = 4,
    /* without RTK_UPDATE_PRE_ROPE (ABI 16; the reference's protocol: q, k rotated by the caller): the launch that
     * un-rotates and appends the chunk also applies the continuity shift the NEXT layer's attention patch would launch
     * before its RoPE (qwen2_vl.py:68-73):  pos[0, 0:L] += (*next_prev + 1) - pos[0, 0], in place, once every workgroup
     * has read the ids this layer works with (each counts itself in on one of the counters in io->ticket; one extra
     * workgroup watches them, shifts and zeroes them again: nobody else waits).  `pos` is written despite its const.
     * Launches that share the ticket words must be stream ordered.
     * The watcher's wait is bounded by a poll count (~seconds; the workers need microseconds).  If it runs out - the
     * counters were not zero at launch: words shared between streams, or never zeroed - the ids are NOT shifted and the
     * counters NOT zeroed: the launch increments ticket[31] (and *io->status) and returns, and so does the watcher of every
     * later launch on these words (without waiting) until the caller has zeroed ticket and status again.  A caller that
     * skips its own rtk_position_shift on the strength of this flag must check the latch before it trusts the ids
     * (PivotKVCache raises RuntimeError).  Needs the chunk-batched passes or a keep-all batch: otherwise
     * RTK_EUNSUPPORTED is returned BEFORE anything is launched (nothing touched).  With this flag EVERY RTK_EUNSUPPORTED of
     * rtk_pivotkv_update is returned before the launch (alignment, extents, shape): a caller may always fall back.
     * The caller's next rtk_position_shift for that layer is then a no-op and may be skipped - the attention patch of a
     * 28-layer model launches it 27 times per chunk otherwise.  Only with the native prepare kernel (batch.inv_freq). */
    RTK_UPDATE_SHIFT_NEXT = 8
};
/* longvideo_cache.py:217-310 up to the deferred selection, for layer slot `slot`.  Rows go to the layer's tail
 * (ls->k/v + length rows; the caller has made sure length + L <= cap), ls->pending / pending_keep are set. */
int rtk_pivotkv_update(rtk_pivotkv_batch* batch, rtk_layer_state* layer, int slot, const rtk_update_io* io,
                       rtk_stream_t stream);

/* The attention patch's prologue for a segment that is NOT compressed - text prefill, decode (qwen2_vl.py:68-86 with the
 * cache's else-branch, longvideo_cache.py:319-321): continuity shift against the layer's last cached temporal id, rotary
 * tables, RoPE of q (to io->q_rot, which may alias io->q) and of k, the append of the rotated k and of v at the layer's
 * tail, and the shifted ids appended to the layer's position cache - one launch.  shift_ids_in_place (Qwen2-VL's in-place
 * semantics; LLaVA shifts a clone: 0): the caller's ids are shifted too - by the same launch for n == 1 (a decode step),
 * by rtk_position_shift after it otherwise.  io: q [Hq,n,D], k / v [Hkv,n,D],
 * pos [P,n].  The caller has made room (rows and ids); length / pos_len are advanced.  pos_embed_reforge caches only. */
int rtk_pivotkv_append_rope(rtk_layer_state* layer, const rtk_update_io* io, int Hq, int Hkv, int n, int D, int dtype, int P,
                            const float* inv_freq, float attention_scaling, const int* sections_host, int nsec,
                            int round_mode, int shift_ids_in_place, rtk_stream_t stream);

/* longvideo_cache.py:260-318 for the n pending layers slots[0..n) (ascending) of one chunk: score passes (unless
 * keep_all), selection, eviction (re-rotated K straight into the cache, V compacted in place) and the bookkeeping of
 * rtk_layer_state (length, pos_len, pending).  layers[i] is the state of slot slots[i].  Native RoPE (batch.inv_freq)
 * when reforging.  RTK_EUNSUPPORTED when the shape needs the per-stage entry points (L < 512, head_dim != 128 for the
 * batched passes). */
int rtk_pivotkv_flush(rtk_pivotkv_batch* batch, rtk_layer_state* const* layers, const int32_t* slots, int n,
                      rtk_stream_t stream);

/* G1  qwen2_vl.py:68-73 / llava_onevision.py:68-72, without the host round trip of the reference's
 * `if position_ids[0,0,0] != prev + 1`:  t[0:n] += (prev + 1) - t[0]  in place, where t is the temporal
 * row of the chunk's position ids and prev = *prev_dev (device memory: the last temporal id the layer's
 * cache holds) or -1 when prev_dev is NULL. */
int rtk_position_shift(int64_t* temporal_ids, int n, const int64_t* prev_dev, rtk_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Direct peer-to-peer all-gather over xGMI (SURVEY §5 "Distributed backend", §8(b) rtk_allgather_*; used by
 * retake/p2p.py and, opt-in, retake/sharded.py).  xGMI is point to point: a rank that has mapped its peers'
 * receive buffers pushes its block into all of them at once (one hop per link) instead of walking a ring.
 *   - buffers: rtk_p2p_alloc (device memory; uncached != 0 for the flag words, which are polled while
 *     kernels of other ranks write them), exported / opened as hipIpc handles between the processes of a node;
 *   - rtk_p2p_push: nseg segments of seg_bytes from src (+ s * src_stride) to byte dst_offset + s * dst_stride
 *     of EVERY mapped buffer (the own one included), then - from a second launch behind the copy, so that a kernel
 *     boundary orders it after every workgroup of it; system-scope release - the value `epoch` into word `rank` of
 *     every peer's flag array  (ABI 17: the unused `counter` argument of ABI <= 16 is gone);
 *   - rtk_p2p_wait: returns (on the stream) once every sender has published an epoch >= `epoch`; bounded:
 *     after ~timeout_ms the kernel gives up and stores 1 + (first missing sender) into *status (device word,
 *     0 = fine), so that a lost peer is an error, not a hung GPU.
 * Epochs count up from 1; receivers that reuse a landing zone alternate two of them (a sender can be one
 * epoch ahead of a receiver, never two).  What landed in a zone at epoch n is guaranteed intact only for reads
 * the receiver enqueued BEFORE its own push n+1: a peer rewrites the zone at epoch n+2 as soon as its wait n+1
 * has seen that push, and later reads are ordered behind nothing.  All sizes, strides and offsets are multiples
 * of 16 bytes.
 * ------------------------------------------------------------------------------------------- */
#define RTK_IPC_HANDLE_BYTES 64
#define RTK_P2P_MAX_RANKS 16
typedef struct rtk_p2p_peers {
    void* buf[RTK_P2P_MAX_RANKS];        /* rank q's receive buffer as mapped in THIS process (own: the local pointer) */
    uint32_t* flag[RTK_P2P_MAX_RANKS];   /* rank q's flag array [world] */
} rtk_p2p_peers;
int rtk_p2p_alloc(size_t bytes, int uncached, void** ptr);      /* zero-filled */
int rtk_p2p_free(void* ptr);
int rtk_p2p_export(const void* ptr, void* handle_out /* RTK_IPC_HANDLE_BYTES */, size_t* offset_out);
int rtk_p2p_open(const void* handle, void** base_out);          /* ptr in this process = *base_out + offset */
int rtk_p2p_close(void* base);
int rtk_p2p_push(const void* src, size_t seg_bytes, int nseg, size_t src_stride_bytes, const rtk_p2p_peers* peers,
                 int rank, int world, size_t dst_offset_bytes, size_t dst_stride_bytes, uint32_t epoch,
                 rtk_stream_t stream);
int rtk_p2p_wait(const uint32_t* own_flags, int world, uint32_t epoch, int timeout_ms, uint32_t* status,
                 rtk_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Chunk attention: the attention of a chunk's queries over [compressed prefix | current chunk], which the reference's
 * attention patches hand to torch / flash_attn after the cache update (qwen2_vl.py:88-117 eager: repeat_kv, matmul, mask
 * add, fp32 softmax, matmul, transpose + contiguous; :188-219 SDPA: repeat_kv, contiguous, scaled_dot_product_attention
 * with the 4-D mask; :303-358 FlashAttention-2: _flash_attention_forward; llava_onevision.py:118-139).
 *
 *   out[i, h, :] = softmax_j( q[h, i, :] . k[h / (Hq/Hkv), j, :] * scale ) . v[h / (Hq/Hkv), j, :]   over j <= q_offset + i, j < Lk
 *
 * Batch 1, forward only, causal by index, no mask operand, no dropout, no sliding window, no returned weights.
 * q_offset = Lk - Lq is bottom-right causal: the queries are the LAST Lq rows of the Lk keys (what flash-attn computes for
 * an unpadded sequence).  A larger q_offset restates the reference's 4-D additive mask, which HF builds over the
 * UNCOMPRESSED positions [1, 1, Lq, T] and the patches slice to the Lk <= T keys the compressed cache holds
 * (qwen2_vl.py:96-97, :196-198): row i then sees j <= (T - Lq) + i, i.e. q_offset = T - Lq.  Only the mask's width enters.
 * Softmax statistics and accumulation are fp32; out has the tensor dtype.
 *   q    [Hq, Lq, D] by pointer + element strides (q_stride_h, q_stride_l), D contiguous - a transposed view of the
 *        projection's [1, Lq, Hq*D] output or the prologue's packed buffer, read where it is;
 *   k, v [Hkv, Lk, D] with common strides (kv_stride_h, kv_stride_l) - the [:Lk] view of a layer's cache buffer as
 *        PivotKVCache.update returns it (head stride = capacity * D).  Query head h reads kv head h / (Hq/Hkv): no
 *        repeat_kv copy is made or expected;
 *   out  [Lq, Hq, D] contiguous - what o_proj consumes after a reshape.
 * dtype RTK_BF16 / RTK_F16 with D == 128: the flash-style MFMA kernel.  RTK_F32, or any D that is a multiple of 8 up to
 * 256: the general kernel (fp32 FMA; no performance claim).  When there are too few query rows to fill the chip the keys
 * are split over workgroups and the partial (max, sum, acc) triples are folded in split order by a second launch - no
 * atomics; the split is a function of (Hq, Lq, Lk, D, dtype) alone, so results are bit-reproducible.  The partials
 * live in `workspace`: rtk_attention_workspace_bytes() bytes (0 when the shape is not split; 0 as well, with the message
 * set, for arguments rtk_attention_forward would reject), 16-byte aligned.
 * Errors, all before any launch: RTK_EINVAL for NULL pointers, Hq % Hkv != 0, Lk < Lq, q_offset < Lk - Lq, non-positive sizes
 * or scale;
 * RTK_EUNSUPPORTED for another dtype code, a D that is not a multiple of 8 in [8, 256], pointers or strides that are not
 * multiples of 16 bytes, or one head of q / k / v spanning 2 GiB or more; RTK_EWORKSPACE for a short workspace.
 * ------------------------------------------------------------------------------------------- */
size_t rtk_attention_workspace_bytes(int Hq, int Hkv, int Lq, int Lk, int D, int dtype);
int rtk_attention_forward(const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* k, const void* v,
                          int64_t kv_stride_h, int64_t kv_stride_l, void* out, int Hq, int Hkv, int Lq, int Lk, int q_offset,
                          int D, int dtype, float scale, void* workspace, size_t workspace_bytes, rtk_stream_t stream);

/* rtk_attention_forward for FEW query rows (decode steps, short trailing text), GQA-packed: the same function, the same
 * arguments, another kernel.  Envelope: RTK_BF16 / RTK_F16, D == 128 and R = (Hq / Hkv) * Lq <= 16 packed rows - Lq <= 2 at
 * 7 or 8 query heads per kv head, up to Lq 16 at one.  One workgroup serves one kv head and one key range: the R rows
 * (g, i) of the kv head - row i of query head hkv * (Hq / Hkv) + g - are the columns of one MFMA operand, so every K and V
 * byte is fetched once per call, not once per query head.  The range's key tiles of T = 32 keys go to the workgroup's four
 * waves round robin; each wave keeps its own (max, sum, acc), the four are folded in wave order, and the workgroup leaves
 * one un-normalised partial per row, which the second launch of rtk_attention_forward folds in split order.  No atomics.
 * The plan is a function of (Hkv, K) alone, K = Lk keys:
 *     n0     = max(1, min(ceil(512 / Hkv), ceil(K / 128)))
 *     kps    = 128 * ceil(ceil(K / n0) / 128)                      keys per split
 *     nsplit = ceil(K / kps)                                       split s takes keys [s * kps, min(K, (s + 1) * kps))
 * (no split is empty; a split wholly above a row's diagonal leaves that row's partial empty and the fold skips it), so
 * results are bit-reproducible and stream-independent.  They are NOT the bits of rtk_attention_forward: the fp32 sums are
 * grouped differently.  The partials ALWAYS live in `workspace`, laid out [nsplit][Hq][Lq][D] fp32 accumulators followed
 * by [nsplit][Hq][Lq][2] fp32 (max, sum): rtk_attention_decode_workspace_bytes() = nsplit * Hq * Lq * (D + 2) * 4 bytes
 * (0, with the message set, for arguments rtk_attention_decode would reject), 16-byte aligned.
 * Errors, all before any launch: those of rtk_attention_forward, same codes and messages; RTK_EUNSUPPORTED, naming the
 * reason, for RTK_F32, D != 128 and (Hq / Hkv) * Lq > 16 - the caller then makes the rtk_attention_forward call. */
size_t rtk_attention_decode_workspace_bytes(int Hq, int Hkv, int Lq, int Lk, int D, int dtype);
int rtk_attention_decode(const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* k, const void* v,
                         int64_t kv_stride_h, int64_t kv_stride_l, void* out, int Hq, int Hkv, int Lq, int Lk, int q_offset,
                         int D, int dtype, float scale, void* workspace, size_t workspace_bytes, rtk_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Measurement support (bench.py).  When enabled, every kernel launch of this library is bracketed
 * by two hipEvents recorded on the launch stream; rtk_profile_collect() waits for them and folds
 * the elapsed times into per-kernel totals.  Process-wide, off by default.
 * ------------------------------------------------------------------------------------------- */
int rtk_profile_enable(int on);
int rtk_profile_enable_mask(unsigned kernel_id_mask);   /* bit k = time kernel id k only; 0 = off */
int rtk_profile_collect(void);
int rtk_profile_reset(void);
int rtk_profile_num_kernels(void);
const char* rtk_profile_kernel_name(int kernel_id);
int rtk_profile_read(int kernel_id, long long* launches, double* total_ms);
/* Calibration for the HBM rooflines: dst = src over 16-byte vectors with non-temporal loads and stores - the device
 * copy the "achievable" bandwidth beside the nominal 8 TB/s is measured with (bench.py: hbm_achievable). */
int rtk_profile_copy(void* dst, const void* src, size_t bytes, rtk_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * FP8 rows of the compressed cache (opt-in: kv_cache_dtype="fp8_e4m3").  The kept K / V rows of compressed video chunks
 * are stored as D one-byte OCP e4m3fn codes plus ONE power-of-two fp32 scale per (kv head, row): (D + 4) bytes instead of
 * 2 D.  Lossy - the reference has no such option.  RTK_BF16 / RTK_F16 with head_dim 128 only.
 *
 * The rule, for one row of one kv head (D values of the model dtype, taken to fp32).  Supported inputs: finite, and a
 * row's amax either 0 or >= 2^-117, so that its scale is a NORMAL fp32 number (>= 2^-126); below that - bf16 rows of
 * magnitudes no K / V row has - the scale is subnormal, the scaled hardware convert of the dequantisation is not
 * specified to honour it, and rule 5's exactness does not hold; such rows are not tested:
 *   1. amax = max |x_d|;
 *   2. amax == 0: scale = 1;
 *   3. otherwise amax = m 2^E with m in [0.5, 1) (frexp); e = E - 9 if m <= 0.875, else E - 8; scale = 2^e, so that
 *      amax / scale lies in (224, 448];
 *   4. code_d = x_d 2^-e (exact) rounded to nearest even to e4m3fn - nothing saturates;
 *   5. dequantised value = dtype(float(code_d) * scale): exactly representable in bf16 (3 mantissa bits against 7); in
 *      fp16 as well, except that a row with |x| >= 65280 may round up to 65536 = inf.
 * Layout: codes of row (h, r) at h*stride_h + r*D BYTES, scale at h*scale_stride_h + r floats.
 *
 * rtk_pivotkv_archive_batched: the eviction (longvideo_cache.py:278-288, :297-310) of n_units (layer, chunk) units that
 * share Hkv, D, keep, P and dtype into such archives, in one launch per RTK_ARCHIVE_MAX_UNITS units.  Kept row r comes
 * from chunk row keep_idx[r] (keep_idx NULL: row r, a chunk that keeps every token).  k_mode RTK_COMPACT_K_ROTATE: kept
 * K = the k_src row (the un-rotated k~) rotated at its new ids pos_src and rounded to the model dtype - the bits
 * rtk_pivotkv_compact_batched writes - then quantised; RTK_COMPACT_K_COPY: the k_src row verbatim (no reforge: pass the
 * cache tail).  Kept V = the v_src row.  Sources and destinations must not alias; nothing else is synchronised.
 * inv_freq / attention_scaling / sections / round_mode as rtk_pivotkv_compact_batched.
 * Errors, all before any launch: RTK_EINVAL for NULL pointers, bad sizes or modes; RTK_EUNSUPPORTED for another dtype or
 * head_dim and for pointers / strides that are not 16-byte aligned. */
typedef struct rtk_archive_unit {
    const void* k_src;        /* K rows of the chunk, element (h,l,d) at h*k_src_stride_h + l*D + d */
    int64_t k_src_stride_h;
    const void* v_src;        /* V rows of the chunk, same layout */
    int64_t v_src_stride_h;
    const int64_t* keep_idx;  /* [keep] from rtk_pivotkv_select[_batched], or NULL = identity */
    const int64_t* pos_src;   /* ids of the kept rows [P, keep] (row stride pos_src_stride): the NEW ids the rotation uses ... */
    int64_t pos_src_stride;
    int64_t* pos_dst;         /* ... copied to the layer's position cache tail (row stride pos_dst_stride), or NULL */
    int64_t pos_dst_stride;
    void* k8;                 /* codes of kept row r of head h at h*dst_stride_h + r*D bytes: already offset to the first free row */
    void* v8;
    int64_t dst_stride_h;     /* bytes */
    float* k_scale;           /* scale of kept row r of head h at h*scale_stride_h + r */
    float* v_scale;
    int64_t scale_stride_h;   /* floats */
} rtk_archive_unit;
#define RTK_ARCHIVE_MAX_UNITS 28   /* units per launch (the array travels as a kernel argument) */
int rtk_pivotkv_archive_batched(const rtk_archive_unit* units, int n_units, int Hkv, int D, int keep, int P, int dtype,
                                int k_mode, const float* inv_freq, float attention_scaling, const int* sections_host,
                                int nsec, int round_mode, rtk_stream_t stream);

/* Codes + scales -> dense rows of the model dtype (rule 5): out element (h,l,d) at h*out_stride_h + l*D + d (elements).
 * The diagnostic dense view of PivotKVCache and the tests use it; nothing on the hot path does. */
int rtk_fp8kv_dequant(const void* codes, int64_t codes_stride_h, const float* scales, int64_t scale_stride_h, void* out,
                      int64_t out_stride_h, int H, int L, int D, int dtype, rtk_stream_t stream);

/* rtk_attention_forward over keys in two segments: L8 archive rows (k8 / v8 / k_scale / v_scale, head strides
 * stride8_h bytes and scale_stride_h floats) that precede, in sequence order, the Lk rows of the 16-bit segment k / v.
 * Every archive row is visible to every query row; 16-bit row r is visible to query row i iff r <= q_offset + i, so Lk,
 * q_offset (>= Lk - Lq) and Lk >= Lq describe the 16-bit segment alone (the caller passes the offset of the whole
 * sequence minus L8).  The archive tiles are converted to the model dtype on their way into LDS and take the same MFMA /
 * softmax body; archive tiles come first.  The result equals, bit for bit, rtk_attention_forward over
 * [dequantised archive | 16-bit rows] with q_offset + L8 when L8 % 64 == 0 (otherwise the 16-bit rows start a new key
 * tile, i.e. the fp32 sums are grouped differently); L8 == 0 IS rtk_attention_forward (k8 .. v_scale are not read).
 * The key split of few-row shapes covers the concatenation: the workspace is rtk_attention_workspace_bytes_fp8kv().
 * RTK_BF16 / RTK_F16 with D == 128 only (RTK_EUNSUPPORTED otherwise); the other errors as rtk_attention_forward, plus
 * RTK_EINVAL for L8 < 0 or NULL archive pointers with L8 > 0, RTK_EUNSUPPORTED for archive pointers / stride8_h that are
 * not multiples of 16 bytes or an archive head of 2 GiB or more. */
size_t rtk_attention_workspace_bytes_fp8kv(int Hq, int Hkv, int Lq, int Lk, int L8, int D, int dtype);
int rtk_attention_forward_fp8kv(const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* k, const void* v,
                                int64_t kv_stride_h, int64_t kv_stride_l, const void* k8, const void* v8,
                                const float* k_scale, const float* v_scale, int L8, int64_t stride8_h,
                                int64_t scale_stride_h, void* out, int Hq, int Hkv, int Lq, int Lk, int q_offset, int D,
                                int dtype, float scale, void* workspace, size_t workspace_bytes, rtk_stream_t stream);

/* rtk_attention_decode over [archive | 16-bit rows]: the arguments of rtk_attention_forward_fp8kv, the envelope, errors and
 * workspace layout of rtk_attention_decode.  The plan is that of rtk_attention_decode with K = Lk + L8 rounded up to a
 * multiple of the key tile T = 32: the archive comes first, padded to whole tiles, so a tile is of one kind.  Archive rows
 * are dequantised by rule 5 on their way into the operands, and whenever L8 % 32 == 0 the result equals, bit for bit,
 * rtk_attention_decode over [dequantised archive | 16-bit rows] with q_offset + L8.  L8 == 0 IS rtk_attention_decode. */
size_t rtk_attention_decode_workspace_bytes_fp8kv(int Hq, int Hkv, int Lq, int Lk, int L8, int D, int dtype);
int rtk_attention_decode_fp8kv(const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* k, const void* v,
                               int64_t kv_stride_h, int64_t kv_stride_l, const void* k8, const void* v8,
                               const float* k_scale, const float* v_scale, int L8, int64_t stride8_h,
                               int64_t scale_stride_h, void* out, int Hq, int Hkv, int Lq, int Lk, int q_offset, int D,
                               int dtype, float scale, void* workspace, size_t workspace_bytes, rtk_stream_t stream);

/* rtk_attention_forward_fp8kv / rtk_attention_decode_fp8kv with ONE MORE key segment: Ls 16-bit rows ks / vs of the model
 * dtype that live in another buffer (head stride s_stride_h, row stride s_stride_l, elements) and sit between the archive
 * and k / v in sequence order: [archive L8 | shared Ls | own Lk].  A fork of a PivotKVCache reads its parent's rows this
 * way, where they lie.  Every archive row and every shared row is visible to every query row; own row r is visible to
 * query row i iff r <= q_offset + i, so Lk, q_offset (>= Lk - Lq) and Lk >= Lq describe the own rows alone (the caller
 * passes the offset of the whole sequence minus L8 + Ls).  The archive may be empty (L8 == 0: k8 .. v_scale are not read).
 * Key tiles are counted in the padded index space of the _fp8kv calls with one more segment: the archive takes
 * [0, L8p), the shared rows [L8p, L8p + Lsp), own row r sits at L8p + Lsp + r, L8p / Lsp = L8 / Ls rounded up to a whole
 * key tile T (64 in rtk_attention_forward_shared, 32 in rtk_attention_decode_shared).  A tile is of one kind; rows past
 * the end of a segment are zero-filled by the descriptor's bounds and masked; the split plan and the diagonal arithmetic
 * are those of a 16-bit call over the padded total, the workspace layout that of the corresponding existing call.
 * Hence, bit for bit:
 *   Ls == 0              IS the _fp8kv call (ks / vs are not read), and with L8 == 0 as well the plain call;
 *   Ls % T == 0, any L8  equals the _fp8kv call over (archive, [shared | own] concatenated in one buffer) with
 *                        q_offset + Ls - with L8 == 0 the plain call over the concatenation;
 * and the _workspace_bytes_shared functions agree with their counterparts in the same way.  Otherwise the own rows start
 * a new key tile, i.e. the fp32 sums are grouped differently.
 * RTK_BF16 / RTK_F16 with D == 128 only, rtk_attention_decode_shared with (Hq / Hkv) * Lq <= 16 besides
 * (RTK_EUNSUPPORTED otherwise, with the reason in rtk_last_error()).  Errors, all before any launch: those of the _fp8kv
 * call, plus RTK_EINVAL for Ls < 0 or NULL ks / vs with Ls > 0, RTK_EUNSUPPORTED for ks / vs or shared strides that are
 * not multiples of 16 bytes, a shared row stride below D, or a shared head of 2 GiB or more. */
size_t rtk_attention_workspace_bytes_shared(int Hq, int Hkv, int Lq, int Lk, int L8, int Ls, int D, int dtype);
int rtk_attention_forward_shared(const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* k, const void* v,
                                 int64_t kv_stride_h, int64_t kv_stride_l, const void* ks, const void* vs, int Ls,
                                 int64_t s_stride_h, int64_t s_stride_l, const void* k8, const void* v8,
                                 const float* k_scale, const float* v_scale, int L8, int64_t stride8_h,
                                 int64_t scale_stride_h, void* out, int Hq, int Hkv, int Lq, int Lk, int q_offset, int D,
                                 int dtype, float scale, void* workspace, size_t workspace_bytes, rtk_stream_t stream);
size_t rtk_attention_decode_workspace_bytes_shared(int Hq, int Hkv, int Lq, int Lk, int L8, int Ls, int D, int dtype);
int rtk_attention_decode_shared(const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* k, const void* v,
                                int64_t kv_stride_h, int64_t kv_stride_l, const void* ks, const void* vs, int Ls,
                                int64_t s_stride_h, int64_t s_stride_l, const void* k8, const void* v8,
                                const float* k_scale, const float* v_scale, int L8, int64_t stride8_h,
                                int64_t scale_stride_h, void* out, int Hq, int Hkv, int Lq, int Lk, int q_offset, int D,
                                int dtype, float scale, void* workspace, size_t workspace_bytes, rtk_stream_t stream);

/* Wide packed decode: rtk_attention_decode, rtk_attention_decode_fp8kv and rtk_attention_decode_shared for SEVERAL new
 * rows - the verification step of assisted generation (num_assistant_tokens + 1 rows), a few-token continuation: the same
 * functions, the same arguments, the envelope R = (Hq / Hkv) * Lq <= 64 packed rows (Lq <= 9 at 7 query heads per kv
 * head, 8 at 8, 16 at 4, 64 at 1), RTK_BF16 / RTK_F16 with D == 128.  Opt-in (multi_token_attention="packed").
 *   R <= 16 IS the corresponding rtk_attention_decode* call, bit for bit, workspace size included.
 *   16 < R <= 64: one workgroup still serves one kv head and one key range, and a tile's K and V rows, fetched from HBM
 *   once, feed ceil(R / 16) column groups of 16 packed rows, each with its own (max, sum, acc).  Packed row r is position
 *   r / G of query head hkv * G + r % G (G = Hq / Hkv).  Causal by index per packed row: a key row hidden from a query row
 *   contributes nothing to it whatever it holds (V rows above a position's diagonal are zeroed, not only their
 *   probabilities; a tile no row of a column group sees is not read for it).
 * The plan is that of rtk_attention_decode over the same K (Lk, plus L8 and Ls each rounded up to the key tile T = 32), a
 * function of (Hkv, K) alone; the partials have its layout, so the workspace queries return nsplit * Hq * Lq * (D + 2) * 4
 * bytes; the four waves of a workgroup are folded in wave order and the splits in split order: bit-reproducible and
 * stream-independent.  NOT the bits of rtk_attention_forward*, nor (for R > 16) of Lq single-row rtk_attention_decode*
 * calls: the fp32 sums are grouped differently.  With L8 % 32 == 0 and Ls % 32 == 0 the segmented calls equal, bit for bit,
 * rtk_attention_decode_wide over the dequantised, concatenated 16-bit rows with q_offset + L8 + Ls; otherwise the sums
 * are grouped differently.  Ls == 0 IS the _fp8kv call, and L8 == 0 as well the plain one.
 * Errors, all before any launch: those of the narrow calls, same codes and messages; RTK_EUNSUPPORTED, naming the
 * reason, for RTK_F32, D != 128 and (Hq / Hkv) * Lq > 64 - the caller then makes the rtk_attention_forward* call. */
size_t rtk_attention_decode_wide_workspace_bytes(int Hq, int Hkv, int Lq, int Lk, int D, int dtype);
int rtk_attention_decode_wide(const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* k, const void* v,
                              int64_t kv_stride_h, int64_t kv_stride_l, void* out, int Hq, int Hkv, int Lq, int Lk, int q_offset,
                              int D, int dtype, float scale, void* workspace, size_t workspace_bytes, rtk_stream_t stream);
size_t rtk_attention_decode_wide_workspace_bytes_fp8kv(int Hq, int Hkv, int Lq, int Lk, int L8, int D, int dtype);
int rtk_attention_decode_wide_fp8kv(const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* k, const void* v,
                                    int64_t kv_stride_h, int64_t kv_stride_l, const void* k8, const void* v8,
                                    const float* k_scale, const float* v_scale, int L8, int64_t stride8_h,
                                    int64_t scale_stride_h, void* out, int Hq, int Hkv, int Lq, int Lk, int q_offset, int D,
                                    int dtype, float scale, void* workspace, size_t workspace_bytes, rtk_stream_t stream);
size_t rtk_attention_decode_wide_workspace_bytes_shared(int Hq, int Hkv, int Lq, int Lk, int L8, int Ls, int D, int dtype);
int rtk_attention_decode_wide_shared(const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* k, const void* v,
                                     int64_t kv_stride_h, int64_t kv_stride_l, const void* ks, const void* vs, int Ls,
                                     int64_t s_stride_h, int64_t s_stride_l, const void* k8, const void* v8,
                                     const float* k_scale, const float* v_scale, int L8, int64_t stride8_h,
                                     int64_t scale_stride_h, void* out, int Hq, int Hkv, int Lq, int Lk, int q_offset, int D,
                                     int dtype, float scale, void* workspace, size_t workspace_bytes, rtk_stream_t stream);

/* Group decode: ONE new token of each of n_branches sequences that share [archive L8 | shared Ls] and differ in their own
 * rows - the forks of one PivotKVCache, each a token into its answer - in one launch that fetches every archive and
 * shared K / V row from HBM once, whatever n_branches is.  Branch b's one query row per head, q_b [Hq, 1, D], attends to
 * every archive row, every shared row and every one of its own Lk_b rows (the query IS the last own row: no diagonal).
 * ks .. scale_stride_h as rtk_attention_decode_shared; the archive and the shared segment may each be empty.  out is
 * [n_branches, Hq, D], contiguous.
 * The kernel packs row b * G + g (G = Hq / Hkv) of all branches onto the columns of one or two 16x16x32 MFMA operands
 * that read the same K fragments and the same V image, so n_branches * G <= 32.
 * Plan, fixed here.  The shared keys are counted in the padded space of rtk_attention_decode_shared without own rows,
 * Kp = L8p + Lsp (each rounded up to the key tile T = 32), and split by the rule of rtk_attention_decode over Kp keys
 * (ns_sh splits; none when Kp == 0): a function of (Hkv, L8, Ls) alone.  Branch b's own rows are split every
 * RTK_DECODE_GROUP_OWN_KEYS = 512 keys: a function of Lk_b alone.  The launch runs ns_sh shared workgroups and
 * n_own = max_b ceil(Lk_b / 512) own workgroups per branch, per kv head; a branch with no key in an own split leaves an
 * empty partial.  The partials (layout of rtk_attention_decode with (branch, head) as the head index) are folded in the
 * order shared splits, then own splits, empty ones skipped; no atomics.  The workspace is
 *   (ns_sh + n_own) * n_branches * Hq * (D + 2) * sizeof(float) bytes.
 * Hence branch b's output bits depend neither on which other branches are in the group nor on b's position in it.  They
 * are not those of rtk_attention_decode_shared: the fp32 sums are grouped differently.
 * RTK_BF16 / RTK_F16, D == 128, n_branches <= RTK_DECODE_GROUP_MAX and n_branches * G <= 32 only: RTK_EUNSUPPORTED
 * otherwise, with the reason in rtk_last_error().  Errors, all before any launch: RTK_EINVAL for NULL pointers,
 * n_branches < 1, Lk_b < 1, L8 / Ls < 0, NULL ks / vs with Ls > 0 or NULL archive pointers with L8 > 0; RTK_EUNSUPPORTED
 * for pointers or strides that are not multiples of 16 bytes, row strides below D, heads of 2 GiB or more;
 * RTK_EWORKSPACE for a short workspace.  The workspace query returns 0 for what the call would refuse. */
typedef struct rtk_decode_branch {
    const void* q;            /* [Hq, 1, D]: this branch's one query row per head, head stride q_stride_h (elements) */
    int64_t q_stride_h;
    const void* k;            /* its OWN rows [Hkv, Lk, D], the new token's included */
    const void* v;
    int64_t kv_stride_h, kv_stride_l;
    int Lk;                   /* >= 1 */
} rtk_decode_branch;
#define RTK_DECODE_GROUP_MAX 8          /* the array travels as a kernel argument */
#define RTK_DECODE_GROUP_OWN_KEYS 512   /* keys per own split */
size_t rtk_attention_decode_group_workspace_bytes(const int* own_rows, int n_branches, int Hq, int Hkv, int L8, int Ls,
                                                  int D, int dtype);
int rtk_attention_decode_group(const rtk_decode_branch* branches, int n_branches, const void* ks, const void* vs, int Ls,
                               int64_t s_stride_h, int64_t s_stride_l, const void* k8, const void* v8,
                               const float* k_scale, const float* v_scale, int L8, int64_t stride8_h,
                               int64_t scale_stride_h, void* out, int Hq, int Hkv, int D, int dtype, float scale,
                               void* workspace, size_t workspace_bytes, rtk_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Sliding window (opt-in: longvideo_kwargs["video_window_rows"]; NOT in the reference, which processes a finished video).
 * Every attention route reads a layer's rows as buf[:, :, :length], contiguous from the buffer's base, so dropping the OLDEST
 * video rows while the text rows in front of them stay is an in-place move: every later row goes down by `drop` rows - K, V
 * and the position ids of every layer, or the codes, scales and ids of the fp8 archive - in ONE call (one kernel launch per
 * RTK_SLIDE_MAX_UNITS moving units).
 *
 * One unit = `streams` independent byte streams (the kv heads of a K / V / code / scale buffer, the id planes of a position
 * buffer).  Per unit and stream s it is
 *     memmove(base + s*stream_stride + first*row_bytes, base + s*stream_stride + (first + drop)*row_bytes, rows*row_bytes):
 * no byte outside the destination range is written; the rows above it keep their old contents.  Source and destination
 * usually overlap almost entirely (drop ~ one chunk's keep, rows ~ the whole window).  The kernel needs no order between
 * workgroups - no flags, no counters, no cooperative launch: the byte at offset x only ever depends on x + drop_bytes,
 * x + 2 drop_bytes, ..., so a workgroup owns one stream, or one slice of the residues mod drop_bytes of one stream, and walks
 * it from low addresses to high; every byte is read by the workgroup that overwrites it (pivotkv_slide.hip).
 * 16-byte accesses where base, stride, drop and length allow, else 4-byte ones; the result is the same.
 * A unit with drop == 0 or rows == 0 is skipped; n_units == 0 (or nothing but such units) launches nothing.  More than
 * RTK_SLIDE_MAX_UNITS moving units take more launches.  `units` is a HOST array.
 * Errors, all before any launch: RTK_EINVAL for NULL pointers, negative first / drop / rows, streams <= 0, a row_bytes that
 * is not a positive multiple of 4, a base or stream_stride that is not 4-byte aligned.
 * ------------------------------------------------------------------------------------------- */
typedef struct rtk_slide_unit {
    void*   base;           /* first byte of stream 0 */
    int64_t stream_stride;  /* bytes between streams (kv heads, id planes) */
    int32_t streams;        /* Hkv for K / V / codes / scales, P for position ids */
    int32_t row_bytes;      /* D*esize, D (e4m3 codes), 4 (scales), 8 (ids); a multiple of 4 */
    int64_t first;          /* destination row of the first moved row */
    int64_t drop;           /* source row = destination row + drop */
    int64_t rows;           /* rows moved */
} rtk_slide_unit;
#define RTK_SLIDE_MAX_UNITS 96   /* moving units per launch (the array travels as a kernel argument) */
int rtk_pivotkv_slide_batched(const rtk_slide_unit* units, int n_units, rtk_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Video budget (opt-in: longvideo_kwargs["video_budget_rows"]; NOT in the reference, which processes a finished video, and a
 * rule of this project's own: what it does to answer quality has not been evaluated).  The sliding window bounds a layer's
 * video region by AGE; the budget bounds it by the attention score every flush already computes: the region keeps one fp32
 * score per row (the value the selection saw, after the key-patch override to 1.0), and when it holds more than
 * budget + slack rows the newest row and the budget - 1 best-scored others survive, in sequence order, moved down in place.
 * The score is a column sum of row-stochastic softmaxes averaged over heads: it averages 1 over any chunk, whatever its
 * length, so scores of rows from different chunks compare directly.
 *
 * rtk_pivotkv_keep_scores_batched - per flush, one launch: dst[r] = score[keep_idx[r]], r < keep, for every unit (a NULL
 *   keep_idx is the identity).  `score` is the chunk's score row as the selection left it, `dst` the rows of the layer's
 *   score store the flush has just filled.
 * rtk_pivotkv_budget_select_batched - per eviction, one launch, one workgroup per unit: writes the ascending int32 list
 *   idx[keep] of the survivors of score[n]: row n - 1 always, and of rows [0, n - 1) the keep - 1 with the highest score,
 *   ties to the lowest index (the order of a stable descending sort).  Exact: four 8-bit radix passes over the
 *   order-preserving key of the fp32 value and one ordered compaction (select.cuh); the scores are re-read from memory on
 *   every pass, n is not bounded by LDS.  keep == n gives the identity.  RTK_EINVAL unless 1 <= keep <= n.
 * rtk_pivotkv_squeeze_batched - per eviction, the move: one unit = `streams` independent byte streams, as rtk_slide_unit
 *   describes them.  Per stream, row[first + r] = row[first + idx[r]] for r < rows_out, as if read from a snapshot; idx is a
 *   DEVICE array, ascending with idx[r] >= r (rows only move down), and names rows below rows_in.  The kernel clamps idx[r]
 *   into [r, rows_in - 1]: a bad list cannot make it read or write out of bounds, or loop.  No byte outside rows
 *   [first, first + rows_out) of each stream is written.  No flags, no counters, no waiting between workgroups, no scratch:
 *   a workgroup owns a stream, or a 128-byte column slice of every row of a stream, and walks the rows upward R rows a step;
 *   a step's stores land in rows [k R, (k + 1) R) and every later source lies at or above (k + 1) R (pivotkv_budget.hip).
 *   16-byte accesses where base, first, stride and row bytes allow, else 4-byte ones; the result is the same.  A unit with
 *   rows_out == 0 is skipped; more than RTK_SQUEEZE_MAX_UNITS moving units take more launches.
 * `units` are HOST arrays; n_units == 0 launches nothing and returns 0.  Errors, all before any launch: RTK_EINVAL for NULL
 * pointers, negative counts, keep outside [1, n], rows_out > rows_in, rows_in beyond int32, streams <= 0, a row_bytes that is
 * not a positive multiple of 4, a base or stream_stride that is not 4-byte aligned.
 * ------------------------------------------------------------------------------------------- */
typedef struct rtk_keep_scores_unit {
    const float*   score;     /* the chunk's scores [L] */
    const int64_t* keep_idx;  /* kept columns [keep], NULL = 0 .. keep - 1 */
    float*         dst;       /* [keep] */
    int32_t        keep;
} rtk_keep_scores_unit;
#define RTK_KEEP_SCORES_MAX_UNITS 96
int rtk_pivotkv_keep_scores_batched(const rtk_keep_scores_unit* units, int n_units, rtk_stream_t stream);

typedef struct rtk_budget_select_unit {
    const float* score;  /* [n], row n - 1 the newest */
    int32_t*     idx;    /* out: [keep], ascending */
    int32_t      n, keep;
} rtk_budget_select_unit;
#define RTK_BUDGET_SELECT_MAX_UNITS 96
int rtk_pivotkv_budget_select_batched(const rtk_budget_select_unit* units, int n_units, rtk_stream_t stream);

typedef struct rtk_squeeze_unit {
    void*   base;           /* first byte of stream 0 */
    int64_t stream_stride;  /* bytes between streams (kv heads, id planes) */
    int32_t streams;
    int32_t row_bytes;      /* a multiple of 4 */
    int64_t first;          /* row of the region's first row */
    int64_t rows_out;       /* rows written: [first, first + rows_out) */
    int64_t rows_in;        /* rows of the region before the move */
    const int32_t* idx;     /* DEVICE: [rows_out], source row of each destination row, relative to `first` */
} rtk_squeeze_unit;
#define RTK_SQUEEZE_MAX_UNITS 80   /* moving units per launch (the array travels as a kernel argument) */
int rtk_pivotkv_squeeze_batched(const rtk_squeeze_unit* units, int n_units, rtk_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * DPSelect on a stream (retake/dpselect_stream.py; NOT in the reference, which processes a finished video, and a rule of
 * this project's own: what it does to answer quality has not been evaluated).  Frames arrive a few at a time and live in a
 * ring of R = 2 S rows - frames [R,N,C] in the model dtype, dis [R,N] fp32, frame g in row g mod R - until their segment of S
 * frames has been selected and gathered.  The host cuts a push into pieces (contiguous runs of ring rows) at the ring's wrap
 * and behind every frame that completes a segment; nothing is read back and every call is ordered by `stream` alone.
 *
 * rtk_dpselect_ingest - one pass over a piece: frames_out[i] = x[i] and dis_out[i, n] = 1 - cos(x[i-1, n], x[i, n]), i < t,
 *   where x[-1] is `prev` [N,C] - the ring row of the frame before the piece.  prev == NULL: the stream begins with x[0] and
 *   dis_out[0] = 1.0, as at frame 0 of rtk_dpselect_dis.  The arithmetic IS rtk_dpselect_dis's, per dtype, on both of its paths
 *   (16-byte vector rows of at most 16 vectors per lane, else the scalar path; x, prev and frames_out must all be 16-byte
 *   aligned for the vector path): a distance has the bits the whole-video call gives the same pair.  x is read once (plus one
 *   halo row per strip of <= 64 rows).  RTK_EINVAL, before any launch: NULL x / frames_out / dis_out, non-positive sizes, an
 *   unsupported dtype code, frames_out overlapping x, prev inside the rows being written.
 *
 * rtk_dpselect_select_ring - rtk_dpselect_select for one segment: `len` rows from ring row r0 on (rows taken modulo R), with
 *   `left` (0 .. window/2) valid rows in front and `right` (0 .. window - 1 - window/2) behind that only the peak windows look
 *   at; fewer than the window reaches only where the stream began or ended, and the window clips there.  Keeps the top `keep`
 *   keys of the len rows, ties to the lowest index, ascending.
 *     idx   LOCAL to the segment (0 .. len-1): sync [keep] int64, async [keep,N] int64
 *     mask  [keep,N] bytes: whether the kept frame is a peak
 *     keys  workspace AND output: async [N,len] fp32; sync [len] keys followed by the [left+len+right] patch means
 *   left = right = 0 and r0 = 0 is rtk_dpselect_select on the same rows, bit for bit (one device body serves both).
 *   RTK_EINVAL: NULL pointers, r0 outside [0,R), len < 1, left / right out of range, len + left + right > R, keep outside
 *   [1,len]; async with N == 1 returns RTK_EREFCRASH, as rtk_dpselect_select does.
 *
 * The kept frames are gathered with rtk_gather_frames(frames_ring + r0 rows, T = len, idx): a segment never wraps.
 * ------------------------------------------------------------------------------------------- */
int rtk_dpselect_ingest(const void* x, const void* prev, int t, int N, int C, int dtype, void* frames_out,
                        float* dis_out, rtk_stream_t stream);
int rtk_dpselect_select_ring(const float* dis_ring, int R, int N, int r0, int len, int left, int right, int keep,
                             int window, int sync, int64_t* idx, uint8_t* mask, float* keys, rtk_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Position re-base (opt-in: longvideo_kwargs["video_position_limit"]; NOT in the reference, which processes a finished
 * video, and a rule of this project's own: what it does to answer quality has not been evaluated).  A bounded video region
 * drops rows but leaves every surviving id where it was, so the ids of a stream that does not end grow without bound while
 * the rows span a bounded range.  Per unit (a layer), with t = row 0 of its ids and the region's ids t[first, end):
 *     base  = first > 0 ? t[first - 1] + 1 : 0
 *     delta = t[first] - base
 *     if delta > 0 and t[end - 1] >= limit:
 *         t[first, end) -= delta                                   (id rows 1 and 2 are not touched)
 *         K[h, first .. first + rows, temporal pairs] <- R(-delta) K   (every head h < H; V is not an argument)
 *         offsets[slot] += delta
 * The temporal pairs (d, d + D/2) are all D/2 for P == 1 and the pairs whose channels the M-RoPE sections give to id
 * row 0 for P == 3; the other channels keep their bits, and a 16-byte chunk pair without a temporal channel is neither
 * loaded nor stored.  Arithmetic per pair, in fp32: theta = (float)delta * inv_freq[d], (s, c) = correctly rounded
 * sin / cos of theta, o1 = fma(x1, c, x2 * s), o2 = fma(x2, c, -(x1 * s)), one rounding to the storage dtype.  No
 * attention_scaling: a stored key already carries it, and a rotation by R(-delta) leaves it in place.
 *
 * Everything is decided on the device and nothing is read back.  Two launches per RTK_REBASE_MAX_UNITS units and no order
 * between workgroups - no flags, no counters, no waiting: a one-wave-per-unit decision launch writes delta[i] (0: unit i
 * did not trigger) and advances offsets[slot]; the apply launch reads delta[i] alone, so no workgroup reads an id another
 * one rewrites.  A unit with delta 0 costs one load per workgroup.  The grid is sized to the machine, not to the rows.
 *   D, dtype        shared by the units: RTK_BF16 / RTK_F16 with D a multiple of 16, RTK_F32 with D a multiple of 8, D <= 256
 *   inv_freq        DEVICE fp32 [D / 2];  sections_host / nsec: the M-RoPE sections (P == 3)
 *   offsets         DEVICE int64, indexed by unit.slot: the cumulative delta of a layer.  Slots of one call are distinct
 *   delta           DEVICE int64 [n_units] scratch, written for every unit
 * `units` is a HOST array; n_units == 0 launches nothing and returns 0.  Errors, all before any launch: RTK_EINVAL for NULL
 * pointers, negative sizes / strides / slots / limit, a bad dtype, P other than 1 or 3, first > end, a head stride smaller
 * than the rows it is asked to walk, ids_stride < end (P == 3), two units with one slot, bad sections; RTK_EUNSUPPORTED for
 * K pointers or head strides that are not 16-byte aligned, a head_dim outside the envelope, and sections that split a
 * rotation pair between id rows.
 * ------------------------------------------------------------------------------------------- */
typedef struct rtk_rebase_unit {
    void*    k;           /* K buffer of the layer: row r of head h at k + h*k_stride_h + r*D*esize */
    int64_t  k_stride_h;  /* BYTES between kv heads (cap * D * esize) */
    int64_t  first;       /* the region's first row (K and ids alike) */
    int64_t  rows;        /* K rows re-rotated: [first, first + rows) */
    int64_t* ids;         /* id buffer [P, cap], row 0 the temporal ids */
    int64_t  ids_stride;  /* elements between id rows */
    int64_t  end;         /* ids re-based: row 0, [first, end) */
    int32_t  H;           /* kv heads */
    int32_t  slot;        /* the layer's slot in `offsets` */
} rtk_rebase_unit;
#define RTK_REBASE_MAX_UNITS 64   /* units per pair of launches (the array travels as a kernel argument) */
int rtk_pivotkv_rebase_batched(const rtk_rebase_unit* units, int n_units, int D, int dtype, int P, const float* inv_freq,
                               const int* sections_host, int nsec, int64_t limit, int64_t* offsets, int64_t* delta,
                               rtk_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * §R  Position renumbering (opt-in: longvideo_kwargs["video_position_gap"] on top of "video_position_limit"; NOT in the
 * reference, and a rule of this project's own: what it does to answer quality has not been evaluated).  The re-base above
 * subtracts ONE delta per layer, the gap between the pinned rows and the first region row.  Under the budget an old,
 * well-scored survivor keeps t[first] low: that delta stays 0 while evictions open holes everywhere else in the region and
 * the last id grows as if nothing were bounded.  Renumbering closes the holes row by row; it generalises the re-base's
 * rule.  Per unit (a layer), with t = row 0 of its ids, the region's ids t[first, end), the K rows [first, first + rows),
 * rows <= end - first, and prev = t[first - 1] if first > 0, else -1 - all integers, exact:
 *     e[first] = max(0, t[first] - prev - 1)                   the region follows the pinned rows: the re-base's delta
 *     e[i]     = max(0, t[i] - t[i - 1] - gap)  (first < i < end)   inner gaps above `gap` close to `gap`
 *     d[i]     = e[first] + ... + e[i]                         inclusive prefix sum: non-negative, non-decreasing
 *     total    = d[end - 1]
 *     if the region is not empty, t[end - 1] >= limit and total > 0:
 *         t[i] -= d[i]                                             (id rows 1 and 2 are not touched)
 *         K[h, first + r, temporal pairs] <- R(-d[first + r]) K    (r < rows, every head h < H; V is not an argument)
 *         offsets[slot] += total
 * Gaps <= gap stay as they are, 0 (rows of one frame) and negative gaps included: nothing is "repaired".  A row with
 * d = 0 keeps its bits - it is neither loaded, rotated nor re-rounded.  Ids in [first + rows, end) (16-bit rows behind a
 * window's region) take their own d, which is the region's total unless gaps above `gap` lie among them.  The temporal
 * pairs, the other channels and the arithmetic per pair are the re-base's, with d of the row for delta:
 * theta = (float)d * inv_freq[d], correctly rounded sin / cos, one fma chain, one rounding to the storage dtype.
 *
 * With gap at or above every inner gap the call does what rtk_pivotkv_rebase_batched does: ids, K bits and offsets.  For
 * non-decreasing ids the cap composes - min(min(x, gap) + min(y, gap), gap) = min(x + y, gap) - so a row dropped later
 * merges two gaps without changing the result: after a triggered move the stored ids are a closed-form function of the
 * unbounded ids of the surviving rows.  A renumbered region of n rows spans at most 1 + (n - 1) * gap ids behind the
 * pinned rows; `limit` must exceed pinned + (rows a region may hold) * gap, or every move triggers.
 *
 * Everything is decided on the device and nothing is read back.  Two launches per RTK_REBASE_MAX_UNITS units and no order
 * between workgroups - no flags, no counters, no waiting: the scan launch (one workgroup per unit) only reads ids; it walks
 * [first, end) in tiles of RTK_RENUMBER_TILE ids (a wave-level inclusive scan, the waves' sums through LDS, a running int64
 * carry) and writes d into row_delta, delta[i] = total (0: unit i did not trigger) and offsets[slot].  The apply launch
 * returns at once for delta[i] == 0; otherwise it rewrites the ids from row_delta and rotates the keys in the re-base
 * apply's layout, a workgroup over a contiguous block of rows, the cos / sin recomputed only where d changes.
 *   D, dtype, inv_freq, sections_host / nsec, limit, offsets, delta     as for rtk_pivotkv_rebase_batched
 *   gap             >= 1
 *   unit.row_delta  DEVICE int64 scratch of at least end - first entries, 8-byte aligned, the unit's own; written if the
 *                   unit's last id has reached the limit (a unit below it is not scanned), read only if it triggers
 * Errors, all before any launch: those of rtk_pivotkv_rebase_batched, and RTK_EINVAL for gap < 1, rows > end - first and a
 * NULL or misaligned row_delta.
 * ------------------------------------------------------------------------------------------- */
typedef struct rtk_renumber_unit {   /* rtk_rebase_unit's fields, then the scratch */
    void*    k;
    int64_t  k_stride_h;
    int64_t  first;
    int64_t  rows;
    int64_t* ids;
    int64_t  ids_stride;
    int64_t  end;
    int32_t  H;
    int32_t  slot;
    int64_t* row_delta;   /* DEVICE [end - first] scratch: d of every region id */
} rtk_renumber_unit;
#define RTK_RENUMBER_TILE 2048   /* ids the scan kernel's workgroup takes per step (8 per thread) */
int rtk_pivotkv_renumber_batched(const rtk_renumber_unit* units, int n_units, int D, int dtype, int P, const float* inv_freq,
                                 const int* sections_host, int nsec, int64_t limit, int64_t gap, int64_t* offsets,
                                 int64_t* delta, rtk_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * §S  Budget re-scoring (opt-in: longvideo_kwargs["video_budget_rescore"] on top of "video_budget_rows"; NOT in the
 * reference, which processes a finished video, and a rule of this project's own: what it does to answer quality has not
 * been evaluated).  The budget ranks a region row by the one score its own chunk's selection saw for it; this call lets
 * every later chunk look again.  Per unit (a layer), with n old region rows, their stored keys K[g, j] (rotated, as they
 * lie), the last W rotated query rows Q[h, i] of the chunk that has just gone through the layer and G = Hq / Hkv:
 *     p_h[i, .] = softmax over j < n of ( Q[h,i] . K[h / G, j] / sqrt(D) )        no mask; rows >= n are never read
 *     mass[j]   = (1 / Hq) sum_h sum_{i < W} p_h[i, j]                            sum_j mass[j] = W
 *     obs[j]    = mass[j] n / W                                                   averages 1 over the n rows
 *     score[j]  = fmaf(alpha, obs[j], (1 - alpha) * score[j])                     j < n; score[n ..] is not touched
 * in fp32: obs[j] = (sum of the probabilities) * ((float)n / (float)(Hq W)), 1 - alpha rounded once, one product, one fma.
 * Exact products of the operands, fp32 accumulation, softmax and sums; no atomics.  The keys of a unit are split into ranges
 * of RTK_RESCORE_KEYS keys - range kr is keys [kr, kr + 1) * RTK_RESCORE_KEYS, a function of n alone - and every sum runs in
 * an order fixed by (n, W, Hq, Hkv, D, dtype): per range the (max, sum) of every query row, merged in range order; then per
 * key the probabilities of the query rows in row order, the kv groups in order.  The same values give the same bits
 * whatever the strides, the addresses, the unit's place in the call and the number of units.
 *   RTK_BF16 / RTK_F16 with D == 128: the matrix path - the G W query rows of a kv group packed into 32-row blocks
 *   (r = hh W + i), base-2 softmax.  Anything else: plain FMA, dot / sqrt(D), natural exp - the parity path.
 *   q_stride_h / q_stride_l   elements between heads / rows of every unit's queries (>= D)
 *   scratch, scratch_stride   DEVICE, 256-byte aligned; unit i uses [i * scratch_stride, + rtk_pivotkv_rescore_workspace_bytes
 *                             (.., n of the unit, ..)): the rows' log-sum-exps and the ranges' partials
 * `units` is a HOST array; n_units == 0 or nothing but n == 0 units launches nothing and returns 0; more than 32 live units
 * take more launches (three per 32).  rtk_pivotkv_rescore_workspace_bytes returns 0 for a shape the call refuses.
 * Errors, all before any launch: RTK_EINVAL for NULL pointers, n < 0 or beyond 2^24, alpha outside (0, 1], W < 1, Hq % Hkv,
 * query strides below D, k_stride_h < n D, a misaligned score, scratch that is misaligned or shorter than the unit needs
 * and - on the matrix path - q / k pointers or strides that are not 16-byte aligned; RTK_EUNSUPPORTED for another dtype code.
 * ------------------------------------------------------------------------------------------- */
typedef struct rtk_rescore_unit {
    const void* q;          /* [Hq, W, D]: element (h, i, d) at q + h*q_stride_h + i*q_stride_l + d (elements) */
    const void* k;          /* first region key row of kv head 0; row j of head g at k + g*k_stride_h + j*D */
    int64_t     k_stride_h; /* elements between kv heads (cap * D), >= n * D */
    float*      score;      /* [n] in / out */
    int32_t     n;          /* old rows: softmaxed over and blended; 0 = unit skipped */
} rtk_rescore_unit;
#define RTK_RESCORE_KEYS 512   /* keys per range: what one workgroup keeps in registers */
size_t rtk_pivotkv_rescore_workspace_bytes(int Hq, int Hkv, int W, int n_max, int D, int dtype);
int rtk_pivotkv_rescore_batched(const rtk_rescore_unit* units, int n_units, int Hq, int Hkv, int W, int D, int dtype,
                                float alpha, int64_t q_stride_h, int64_t q_stride_l, void* scratch, size_t scratch_stride,
                                rtk_stream_t stream);

/* rtk_pivotkv_rescore_fp8k_batched - the same rule over the e4m3 key rows of an fp8 archive (§K; opt-in:
 * longvideo_kwargs["archive_rescore"] with "kv_cache_dtype"): K[g, j] = dtype(float(code) * scale), rule 5 of §K, where dtype
 * is the queries' - RTK_BF16 or RTK_F16, with D == 128 only (no archive exists for anything else: RTK_EUNSUPPORTED before any
 * launch).  The same three launches, key ranges and order of every sum as the matrix path above; the codes are dequantised
 * where a key fragment is loaded, so the result equals, bit for bit, rtk_pivotkv_rescore_batched over rtk_fp8kv_dequant of
 * the same codes and scales.  Rows at and behind n are not read, neither codes nor scales.  The scratch is that of
 * rtk_pivotkv_rescore_workspace_bytes: it does not depend on the key format.  Scores taken on e4m3 keys are a different
 * rule from scores taken on 16-bit keys; what that does to answer quality has not been evaluated.
 * Errors, all before any launch: those of rtk_pivotkv_rescore_batched that apply, and RTK_EINVAL for a NULL k8 / k_scale of
 * a live unit, k8_stride_h < n D, scale_stride_h < n, a k8 pointer or k8_stride_h that is not 16-byte aligned and a k_scale
 * that is not 4-byte aligned. */
typedef struct rtk_rescore_fp8k_unit {
    const void*  q;              /* as rtk_rescore_unit */
    const void*  k8;             /* codes of the first region row of kv head 0; row j of head g at k8 + g*k8_stride_h + j*D BYTES */
    int64_t      k8_stride_h;    /* bytes between kv heads, >= n*D */
    const float* k_scale;        /* scale of row j of head g at k_scale + g*scale_stride_h + j */
    int64_t      scale_stride_h; /* floats, >= n */
    float*       score;          /* [n] in / out */
    int32_t      n;
} rtk_rescore_fp8k_unit;
int rtk_pivotkv_rescore_fp8k_batched(const rtk_rescore_fp8k_unit* units, int n_units, int Hq, int Hkv, int W, int D,
                                     int dtype, float alpha, int64_t q_stride_h, int64_t q_stride_l, void* scratch,
                                     size_t scratch_stride, rtk_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * §T  Question focus (opt-in: PivotKVCache.watch_question / PivotKVCache.focus; NOT in the reference, and a rule of this
 * project's own: what it does to answer quality has not been evaluated).  Once a question is known, the video rows it reads
 * are chosen by its own queries - rtk_pivotkv_rescore_batched (rtk_pivotkv_rescore_fp8k_batched over the archive of an fp8
 * parent with archive_rescore) with alpha = 1 into a zeroed score row, then
 * rtk_pivotkv_budget_select_batched, both as they are - and moved, with the pinned rows in front of them and the question's
 * rows behind them, into a small cache of their own that the answer is decoded over.  The parent cache is only read.
 *
 * rtk_pivotkv_focus_gather_batched - the move, OUT OF PLACE: one unit = `streams` independent byte streams (the kv heads of a
 * K / V buffer, the id planes of a position buffer) with a source and a destination of their own.  Per stream, destination
 * row r takes
 *     r <  head                : source row r
 *     head <= r < head + keep  : source row first + clamp(idx[r - head], 0, n - 1)
 *     r >= head + keep         : source row tail_src + (r - head - keep),   r < head + keep + tail
 * idx is a DEVICE int32 array, read once per destination row.  The clamp is in the kernel: a bad list can only name a wrong
 * row of the region, never a byte outside source rows [first, first + n).  No byte outside destination rows
 * [0, head + keep + tail) of each stream is written.  Source and destination do not overlap and every destination row has
 * one writer, so nothing orders workgroups: no flags, no counters, no barrier, no LDS, no scratch.  A workgroup owns 64
 * contiguous destination rows of one stream, a wave whole rows, 8 rows in flight per thread; the grid depends on the units
 * alone.  16-byte accesses where both bases, both strides and row_bytes allow, else 4-byte ones; the result is the same.
 * A unit with head + keep + tail == 0 is skipped; more than RTK_FOCUS_MAX_UNITS moving units take more launches.  The
 * destinations of different units must not overlap each other (not checked).
 * `units` is a HOST array; n_units == 0 launches nothing and returns 0.  Errors, all before any launch: RTK_EINVAL for NULL
 * pointers, negative counts or strides, keep > n, row counts beyond int32, streams <= 0, a row_bytes that is not a positive
 * multiple of 4, bases or strides that are not 4-byte aligned, a dst_stride below the rows of a destination stream, and a
 * unit whose source and destination byte spans (first stream's first row to last stream's last row) overlap.
 * ------------------------------------------------------------------------------------------- */
typedef struct rtk_focus_unit {
    const void* src;         /* first byte of source stream 0 (row 0) */
    void*       dst;         /* first byte of destination stream 0 (row 0) */
    int64_t src_stride;      /* bytes between source streams */
    int64_t dst_stride;      /* bytes between destination streams */
    int32_t streams;         /* Hkv for K / V, P for position ids */
    int32_t row_bytes;       /* D*esize, 8 (ids); a multiple of 4 */
    int64_t head;            /* leading rows copied as they lie */
    int64_t first;           /* source row of the region's first row */
    int64_t n;               /* region rows */
    int64_t keep;            /* gathered rows, <= n */
    int64_t tail_src;        /* source row of the first tail row */
    int64_t tail;            /* tail rows */
    const int32_t* idx;      /* DEVICE: [keep], region row of each gathered row */
} rtk_focus_unit;
#define RTK_FOCUS_MAX_UNITS 48   /* moving units per launch (the array travels as a kernel argument) */
int rtk_pivotkv_focus_gather_batched(const rtk_focus_unit* units, int n_units, rtk_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * §U  Page-sparse decode (opt-in: sparse_decode(cache) / dense_decode(cache), retake/_sparse_decode.py; NOT in the reference, and a rule of this
 * project's own: what it does to answer quality has not been evaluated).  The video rows stay where they lie; a small index
 * of per-page key bounds sits beside them, and each decode call picks, per kv head, the pages whose upper bound on the
 * logit is highest (after Quest, Tang et al. 2024) and attends over the pinned rows, those pages and the rows behind the video.
 *
 * Per layer: `first` pinned rows, `ve` rows up to the end of the video, n = ve - first region rows, pages = ceil(n / 32);
 * page p is region rows [32 p, min(32 p + 32, n)) - RTK_PAGE_ROWS = 32 is the packed decode kernel's key tile T.
 *
 * rtk_pivotkv_page_summary_batched - one call for all layers of a device, one streaming launch (per RTK_PAGE_SUMMARY_MAX_UNITS
 *   units) that reads K once: summ[g, p, 0, d] = max, summ[g, p, 1, d] = min over the rows r of page p of k[g, first + r, d],
 *   in the dtype of k, exact (one of the inputs, bit for bit; of -0 and +0 the max is +0, the min -0; inputs are finite).
 *   k is [Hkv, rows, D] with rows D elements apart and heads k_stride_h elements apart; summ is [Hkv, pages, 2, D] with heads
 *   summ_stride_h elements apart.  The partial last page is taken over its existing rows; no row outside [first, first + n)
 *   is read, no byte outside summ's pages * 2 * D elements per head written.  A unit with n == 0 is skipped.  One wave per
 *   (kv head, page), each load instruction four whole 256-byte rows (pivotkv_pages.hip).  RTK_BF16 / RTK_F16 with D == 128
 *   (RTK_EUNSUPPORTED otherwise).  `units` is a HOST array; n_units == 0 launches nothing and returns 0.  RTK_EINVAL, before
 *   any launch, for NULL pointers, negative counts, pointers or strides that are not 16-byte aligned, a head stride below
 *   the rows of a head.
 * rtk_attention_page_bound - ub[g, p] = max over the packed rows r = (hh, i), hh < Hq / Hkv, i < Lq, of
 *       sum_d max(q[g (Hq / Hkv) + hh, i, d] * summ[g, p, 0, d], q[..] * summ[g, p, 1, d])
 *   into ub fp32 [Hkv, pages].  The products are exact in fp32 (both operands are 16-bit); the sum is fp32, a lane adding its
 *   8 channels in order and the 16 lanes of a page folded 1, 2, 4, 8 apart, r in ascending order: a function of the shape
 *   alone, so the bits depend on neither strides nor addresses.  No scale is applied.  Every raw logit of a packed row of the
 *   group against a key of the page is <= ub[g, p], up to the rounding of that sum.  Errors as above.
 * rtk_attention_decode_paged - rtk_attention_decode's arithmetic over the VIRTUAL key space of whole 32-key tiles
 *       [ rows [0, first) of k / v, padded to a multiple of 32 | page list[g][0], list[g][1], .. | rows [ve, Lk) ]
 *   with list a DEVICE int32 array [Hkv, keep_pages] of page numbers.  Rows a padded head tile or the partial last page would
 *   name beyond its segment get logit -inf and contribute nothing, whatever the memory there holds.  Only the tail has a
 *   diagonal (key row j of the tail is visible to query row i when j <= q_offset + i, in physical rows); q_offset >= ve - 1
 *   is required, so that every query row sees the whole region.  The splits are rtk_attention_decode's plan over the virtual
 *   key count K = 32 ceil(first / 32) + 32 keep_pages + Lk - ve; the partials have its layout
 *   (rtk_attention_decode_paged_workspace_bytes = nsplit * Hq * Lq * (D + 2) * 4) and are folded by the same second launch.
 *   Each list entry is read once per tile and clamped into [0, pages - 1] in the kernel: a bad list can only name a wrong
 *   page, never a byte outside rows [first, ve).  With first % 32 == 0 and n % 32 == 0 the result equals, bit for bit,
 *   rtk_attention_decode over the concatenation of those rows (q_offset moved accordingly); with keep_pages == pages and
 *   the identity list as well, over the rows as they lie.  No atomics, no flags, no waiting between workgroups.
 * rtk_attention_decode_sparse - the chain in one call: rtk_attention_page_bound, then
 *   rtk_pivotkv_budget_select_batched as it is with one unit per kv head (score = ub + g * pages, n = pages,
 *   keep = keep_pages: the last page always, of the others the keep_pages - 1 with the highest ub, ties to the lowest
 *   index, ascending), then the paged kernel and the combine.  Its workspace is [ub fp32 [Hkv, pages] | lists int32
 *   [Hkv, keep_pages] | partials], each part starting at a multiple of 16 bytes; ub and the lists of the last call stay
 *   readable there.  The caller chooses keep_pages = min(ceil(keep_rows / 32), pages).
 * Envelope of the two attention calls, as rtk_attention_decode: RTK_BF16 / RTK_F16, D == 128, (Hq / Hkv) * Lq <= 16 -
 * RTK_EUNSUPPORTED otherwise, before any launch.  RTK_EINVAL, before any launch: NULL pointers, non-positive sizes,
 * first < 0, first > ve, ve > Lk, keep_pages outside [1, pages], q_offset < ve - 1 or < Lk - Lq, pointers or strides that
 * are not multiples of 16 bytes, a short or misaligned workspace.  The workspace queries return 0, with the message set,
 * for a shape the call would refuse.
 *
 * Over an fp8 archive (§K; opt-in: sparse_decode(cache, archive=True) on a cache with kv_cache_dtype) the region is the
 * ARCHIVE: n = L8 rows, pages = ceil(L8 / 32), page p is archive rows [32 p, min(32 p + 32, L8)); the 16-bit buffer holds the
 * pinned rows and everything behind the video and follows the archive, as in rtk_attention_decode_fp8kv.
 * rtk_pivotkv_page_summary_fp8k_batched - rtk_pivotkv_page_summary_batched over e4m3 codes and scales: summ[g, p, 0 / 1, d] =
 *   max / min over the existing rows j of page p of K[g, j, d] = dtype(float(code) * scale), rule 5 of §K (exact in the
 *   model dtype), stored as above ([Hkv, pages, 2, D] of `dtype`, the same +-0 convention) - bit for bit
 *   rtk_pivotkv_page_summary_batched over rtk_fp8kv_dequant of the same rows.  Row j of head g: codes at k8 + g * k8_stride_h
 *   + j * D BYTES, scale at k_scale + g * scale_stride_h + j.  One wave per (kv head, page), each load instruction eight
 *   whole 128-byte code rows, a row's scale loaded once per row; rows >= n are not read, neither codes nor scales.
 *   RTK_BF16 / RTK_F16 with D == 128 (RTK_EUNSUPPORTED otherwise).  RTK_EINVAL, before any launch: NULL pointers, a negative
 *   n, k8 / summ / their head strides not 16-byte aligned, k_scale not 4-byte aligned, a head stride below the rows of a
 *   head, n * D at or above 2 GiB (the archive's limit per head).  A unit with n == 0 is skipped; 16 bytes of summaries per
 *   (kv head, row) beside 132 bytes of K codes + scale.
 * rtk_attention_decode_paged_fp8kv - rtk_attention_decode_fp8kv's arithmetic over the VIRTUAL key space of whole 32-key tiles
 *       [ archive page list[g][0], list[g][1], .. list[g][keep_pages - 1] | 16-bit rows [0, Lk) ]
 *   K = 32 keep_pages + Lk virtual keys; the splits are rtk_attention_decode's plan over K, the partials have its layout
 *   (rtk_attention_decode_paged_fp8kv_workspace_bytes = nsplit * Hq * Lq * (D + 2) * 4) and the same second launch folds
 *   them.  Archive rows a partial page names beyond L8 read as zero codes and zero scales (descriptors bounded at exactly
 *   L8 * 128 and L8 * 4 bytes) and get logit -inf.  Only the 16-bit rows have a diagonal: q_offset counts 16-bit rows and
 *   must be >= Lk - Lq; every archive row is visible to every query row.  Each list entry is read once per tile and clamped
 *   into [0, pages - 1].  With the identity list the result equals rtk_attention_decode_fp8kv over the archive as it lies,
 *   bit for bit; with a list that names the partial page last or not at all, that call over the gathered codes and scales.
 * rtk_attention_decode_sparse_fp8kv - the chain in one call, as rtk_attention_decode_sparse: rtk_attention_page_bound on
 *   summ, rtk_pivotkv_budget_select_batched, the fp8 paged kernel, the combine; the workspace is [ub | lists | partials] with
 *   the same layout.  The summaries are 16-bit values of the keys the attention really uses, so the bound holds against the
 *   dequantised keys.
 * Envelope and errors of the two attention calls: those of rtk_attention_decode_fp8kv's shape (RTK_BF16 / RTK_F16, D == 128,
 * (Hq / Hkv) * Lq <= 16 - RTK_EUNSUPPORTED otherwise), and RTK_EINVAL, before any launch, for NULL pointers, non-positive
 * sizes, L8 < 1, keep_pages outside [1, pages], q_offset < Lk - Lq, pointers or strides that are not multiples of 16 bytes
 * (scales: 4), a short or misaligned workspace.  The workspace queries return 0, with the message set, for a shape the call
 * would refuse.  No atomics, no flags, no waiting between workgroups.
 *
 * Several new tokens (opt-in: sparse_decode(cache, wide=True)): the wide family of the two 16-bit attention calls, for the
 * verification call of assisted generation and short turns.
 * rtk_attention_decode_paged_wide - rtk_attention_decode_paged with rtk_attention_decode_wide's arithmetic (§P: packed row
 *   r = i * G + g, two to four column groups, a tile on the diagonal judged per group) for 16 < (Hq / Hkv) * Lq <= 64 packed
 *   rows, over the same virtual key space: ALL Lq rows of the call share the kv head's one list.  Segments, descriptors,
 *   the clamp of a list entry, the diagonal (only the tail has one), q_offset >= ve - 1, the plan over the virtual key
 *   count, the partials and the second launch are those of rtk_attention_decode_paged.  With first % 32 == 0 and
 *   n % 32 == 0 the result equals, bit for bit, rtk_attention_decode_wide over the concatenation of those rows; with the
 *   identity list as well, over the rows as they lie.
 * rtk_attention_decode_sparse_wide - the chain of rtk_attention_decode_sparse around it: rtk_attention_page_bound (its max
 *   runs over the packed rows of EVERY position: a page that any one row needs is ranked by that row),
 *   rtk_pivotkv_budget_select_batched with one unit per kv head, the wide paged kernel, the combine; the workspace is
 *   [ub | lists | partials] with the same layout.  The output is not what Lq one-token sparse calls would give.
 * Envelope: RTK_BF16 / RTK_F16, D == 128, (Hq / Hkv) * Lq <= 64 - RTK_EUNSUPPORTED otherwise, before any launch.  With
 * (Hq / Hkv) * Lq <= 16 the call IS rtk_attention_decode_paged / rtk_attention_decode_sparse (and its workspace query
 * theirs), as rtk_attention_decode_wide is rtk_attention_decode.  Checks, their order and RTK_EINVAL as for the narrow
 * calls.  No atomics, no flags, no waiting between workgroups.  rtk_version() is unchanged: additions only.
 * ------------------------------------------------------------------------------------------- */
#define RTK_PAGE_ROWS 32
typedef struct rtk_page_summary_unit {
    const void* k;            /* row 0 of kv head 0 of the layer's key buffer */
    int64_t k_stride_h;       /* elements between kv heads */
    int64_t first;            /* pinned rows: the region starts here */
    int64_t n;                /* region rows */
    void*   summ;             /* out: [Hkv, ceil(n / 32), 2, D] */
    int64_t summ_stride_h;    /* elements between kv heads */
} rtk_page_summary_unit;
#define RTK_PAGE_SUMMARY_MAX_UNITS 64   /* units per launch (the array travels as a kernel argument) */
int rtk_pivotkv_page_summary_batched(const rtk_page_summary_unit* units, int n_units, int Hkv, int D, int dtype,
                                     rtk_stream_t stream);
int rtk_attention_page_bound(const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* summ, int64_t summ_stride_h,
                             int Hq, int Hkv, int Lq, int pages, int D, int dtype, float* ub, rtk_stream_t stream);
size_t rtk_attention_decode_paged_workspace_bytes(int Hq, int Hkv, int Lq, int Lk, int first, int ve, int keep_pages, int D,
                                                  int dtype);
int rtk_attention_decode_paged(const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* k, const void* v,
                               int64_t kv_stride_h, int64_t kv_stride_l, void* out, int Hq, int Hkv, int Lq, int Lk, int q_offset,
                               int D, int dtype, float scale, int first, int ve, const int32_t* list, int keep_pages,
                               void* workspace, size_t workspace_bytes, rtk_stream_t stream);
size_t rtk_attention_decode_sparse_workspace_bytes(int Hq, int Hkv, int Lq, int Lk, int first, int ve, int keep_pages, int D,
                                                   int dtype);
int rtk_attention_decode_sparse(const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* k, const void* v,
                                int64_t kv_stride_h, int64_t kv_stride_l, void* out, int Hq, int Hkv, int Lq, int Lk, int q_offset,
                                int D, int dtype, float scale, int first, int ve, const void* summ, int64_t summ_stride_h,
                                int keep_pages, void* workspace, size_t workspace_bytes, rtk_stream_t stream);

typedef struct rtk_page_summary_fp8k_unit {
    const void*  k8;             /* codes of archive row 0 of kv head 0 */
    int64_t      k8_stride_h;    /* BYTES between kv heads, >= n*D */
    const float* k_scale;        /* scale of row j of head g at k_scale + g*scale_stride_h + j */
    int64_t      scale_stride_h; /* floats, >= n */
    int64_t      n;              /* archive rows */
    void*        summ;           /* out: [Hkv, ceil(n / 32), 2, D] of `dtype` */
    int64_t      summ_stride_h;  /* elements between kv heads */
} rtk_page_summary_fp8k_unit;
int rtk_pivotkv_page_summary_fp8k_batched(const rtk_page_summary_fp8k_unit* units, int n_units, int Hkv, int D, int dtype,
                                          rtk_stream_t stream);
size_t rtk_attention_decode_paged_fp8kv_workspace_bytes(int Hq, int Hkv, int Lq, int Lk, int L8, int keep_pages, int D, int dtype);
int rtk_attention_decode_paged_fp8kv(const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* k, const void* v,
                                     int64_t kv_stride_h, int64_t kv_stride_l, const void* k8, const void* v8,
                                     const float* k_scale, const float* v_scale, int L8, int64_t stride8_h, int64_t scale_stride_h,
                                     void* out, int Hq, int Hkv, int Lq, int Lk, int q_offset, int D, int dtype, float scale,
                                     const int32_t* list, int keep_pages, void* workspace, size_t workspace_bytes,
                                     rtk_stream_t stream);
size_t rtk_attention_decode_sparse_fp8kv_workspace_bytes(int Hq, int Hkv, int Lq, int Lk, int L8, int keep_pages, int D, int dtype);
int rtk_attention_decode_sparse_fp8kv(const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* k, const void* v,
                                      int64_t kv_stride_h, int64_t kv_stride_l, const void* k8, const void* v8,
                                      const float* k_scale, const float* v_scale, int L8, int64_t stride8_h, int64_t scale_stride_h,
                                      void* out, int Hq, int Hkv, int Lq, int Lk, int q_offset, int D, int dtype, float scale,
                                      const void* summ, int64_t summ_stride_h, int keep_pages, void* workspace,
                                      size_t workspace_bytes, rtk_stream_t stream);
size_t rtk_attention_decode_paged_wide_workspace_bytes(int Hq, int Hkv, int Lq, int Lk, int first, int ve, int keep_pages, int D,
                                                       int dtype);
int rtk_attention_decode_paged_wide(const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* k, const void* v,
                                    int64_t kv_stride_h, int64_t kv_stride_l, void* out, int Hq, int Hkv, int Lq, int Lk,
                                    int q_offset, int D, int dtype, float scale, int first, int ve, const int32_t* list,
                                    int keep_pages, void* workspace, size_t workspace_bytes, rtk_stream_t stream);
size_t rtk_attention_decode_sparse_wide_workspace_bytes(int Hq, int Hkv, int Lq, int Lk, int first, int ve, int keep_pages, int D,
                                                        int dtype);
int rtk_attention_decode_sparse_wide(const void* q, int64_t q_stride_h, int64_t q_stride_l, const void* k, const void* v,
                                     int64_t kv_stride_h, int64_t kv_stride_l, void* out, int Hq, int Hkv, int Lq, int Lk,
                                     int q_offset, int D, int dtype, float scale, int first, int ve, const void* summ,
                                     int64_t summ_stride_h, int keep_pages, void* workspace, size_t workspace_bytes,
                                     rtk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RETAKE_HIP_H */
