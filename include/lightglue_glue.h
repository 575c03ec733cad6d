/*
 * lightglue_glue.h — gfx950 kernels for the LightGlue matcher built around MHAHeadDim64
 * (SURVEY.md section 8(f) ranks 3/4). Not part of the reference plugin's surface: these
 * replace chains of small framework ops around the attention call in
 * lightglue_pytorch_no_plugin/lightglue.py (one launch each instead of 3-8).
 *
 * Layouts are row-major and contiguous. dtype: MHA_HD64_DT_FLOAT (0) or MHA_HD64_DT_HALF (1)
 * for every tensor argument of a call (statistics and softmax math in fp32). All calls are
 * asynchronous on `stream` and return 0 or a nonzero status (message: mha_hd64_last_error()).
 *
 * Image pairs: the row-major side of the split/merge calls holds `pairs` image pairs stacked
 * pair-major — pair p's n0 rows of image 0, then its n1 rows of image 1 — so "[n0+n1, ...]"
 * below reads [pairs*(n0+n1), ...], and each per-image head-major tensor "[heads, ni, 64]" reads
 * [pairs, heads, ni, 64] (the batch dimension of the attention calls). pairs = 1: one pair.
 *
 * ABI version 2 (round 4): `pairs` inserted after n1 in the split / merge / fused-projection calls
 * and `batch` in the dual log-softmax and its workspace query. A host built against an older
 * header links against the same symbol names and would pass shifted arguments: check
 * lg_glue_abi_version() == LG_GLUE_ABI_VERSION once at load.
 * ABI version 3 (round 6): lg_linear_cat_ffn takes the packed weight stream of its one-launch form
 * (w_packed, after b2; lg_ffn_pack). ABI version 4: lg_ffn_pack writes two layouts (the 16-row
 * kernel's after the 32-row kernel's; lg_ffn_packed_bytes doubled). Still version 4 with
 * lg_assign_matches and its workspace query: new symbols change no existing argument list, and a
 * library without them fails the loader's symbol check (reported as stale).
 */
#ifndef LIGHTGLUE_GLUE_H_
#define LIGHTGLUE_GLUE_H_

#include <stddef.h>
#include <stdint.h>

#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LG_GLUE_ABI_VERSION 4
/* The ABI version of the argument lists below that this library implements. */
int32_t lg_glue_abi_version(void);

/* SelfBlock q/k/v (lightglue.py:111-119, rotary :124-134): qkv [n0+n1, heads*64*3] is the Wqkv
 * output with channel (h*64 + d)*3 + j; cos/sin [n0+n1, 64] the positional encoding (pairs
 * repeated, lightglue.py:44-52). Writes q/k (rotated) and v of image i as [heads, ni, 64]. */
int32_t lg_qkv_rotary_split(int32_t dtype, const void* qkv, const void* cos, const void* sin, int32_t heads,
                            int32_t n0, int32_t n1, int32_t pairs, void* q0, void* k0, void* v0, void* q1, void* k1,
                            void* v1, hipStream_t stream);

/* CrossBlock heads (lightglue.py:158-166): a, b [n0+n1, heads*64] -> a0, b0 [heads, n0, 64],
 * a1, b1 [heads, n1, 64]. */
int32_t lg_split_heads2(int32_t dtype, const void* a, const void* b, int32_t heads, int32_t n0, int32_t n1,
                        int32_t pairs, void* a0, void* a1, void* b0, void* b1, hipStream_t stream);

/* The same with row stride `ld` elements for a and b (column views of one wider projection, e.g.
 * the cross block's to_qk | to_v computed as one GEMM: a = qkv, b = qkv + heads*64, ld = 2*heads*64);
 * a and b 16-byte aligned. */
int32_t lg_split_heads2_ld(int32_t dtype, const void* a, const void* b, int32_t ld, int32_t heads, int32_t n0,
                           int32_t n1, int32_t pairs, void* a0, void* a1, void* b0, void* b1, hipStream_t stream);

/* Attention outputs back to rows (lightglue.py:118-120, 163-170): x0 [heads, n0, 64],
 * x1 [heads, n1, 64] -> out [n0+n1, heads*64]. */
int32_t lg_merge_heads(int32_t dtype, const void* x0, const void* x1, int32_t heads, int32_t n0, int32_t n1,
                       int32_t pairs, void* out, hipStream_t stream);

/* The FFN input of both blocks (lightglue.py:104, 181: cat([x, message], -1)) with the message
 * projection folded into the FFN's first weight: out [n0+n1, 2*heads*64] = [x | merge(x0, x1)],
 * x [n0+n1, heads*64]. One pass instead of merge_heads + a concatenation copy. */
int32_t lg_merge_heads_cat(int32_t dtype, const void* x, const void* x0, const void* x1, int32_t heads, int32_t n0,
                           int32_t n1, int32_t pairs, void* out, hipStream_t stream);

/* FFN middle (lightglue.py:101-106): y = GELU(LayerNorm(x) * gamma + beta), exact (erf) GELU,
 * x, y [rows, dim], dim 64, 128, 256, 512 or 1024 (any other: bad parameter); y == x (in place) is
 * allowed: each row is read whole before any of it is written. Mean and variance in fp32, the variance
 * from the squares about the mean (two passes over the row in registers) in every form. */
int32_t lg_layernorm_gelu(int32_t dtype, const void* x, const void* gamma, const void* beta, int32_t rows,
                          int32_t dim, float eps, void* y, hipStream_t stream);

/* ---- projections with their neighbours fused (fp16 only; csrc/lightglue_linear.hip; the FFN entry
 * points lg_linear_cat_ln_gelu: csrc/lightglue_ffn_ln.hip; lg_linear_cat_ffn*, lg_ffn_pack: csrc/lightglue_ffn.hip) ----
 * W [n, k] row-major (nn.Linear layout), bias [n]; k in {256, 512}; n a multiple of 64; rows m
 * any. A/W/x/ctx 16-byte aligned, bias/out/res/cos/sin 8-byte aligned.
 * lg_linear:            out [m, n] = A [m, k] · Wᵀ + bias (+ res [m, n] when res != NULL). */
int32_t lg_linear(const void* a, const void* w, const void* bias, const void* res, int32_t m, int32_t n, int32_t k,
                  void* out, hipStream_t stream);
/* lg_linear_cat:        out [n0+n1, n] = [x | merge_heads(ctx0, ctx1)] · Wᵀ + bias with x [n0+n1, heads*64],
 *                       ctx_i [heads, ni, 64] (k = 2*heads*64; the FFN input of lightglue.py:104/181). */
int32_t lg_linear_cat(const void* x, const void* ctx0, const void* ctx1, int32_t heads, int32_t n0, int32_t n1,
                      int32_t pairs, const void* w, const void* bias, int32_t n, void* out, hipStream_t stream);
/* lg_linear_cat_ln_gelu: the FFN's first half (lightglue.py:101-106) after lg_linear_cat:
 *                       out [n0+n1, 512] = GELU(LayerNorm(fp16([x | merge_heads(ctx0, ctx1)] · Wᵀ + bias)))
 *                       with the LayerNorm's gamma, beta [512] and eps (exact-erf GELU). One launch
 *                       (tiles owning whole rows: 64-row tiles from m >= 16,384, 128-row tiles from
 *                       m >= 32,768; heads * 128 = 512, 16-B aligned bias / gamma / beta / out), else
 *                       lg_linear_cat then lg_layernorm_gelu in place; see lg_linear_set_ln_fused. */
int32_t lg_linear_cat_ln_gelu(const void* x, const void* ctx0, const void* ctx1, int32_t heads, int32_t n0, int32_t n1,
                              int32_t pairs, const void* w, const void* bias, const void* gamma, const void* beta,
                              float eps, void* out, hipStream_t stream);
/* lg_linear_cat_ffn:    the whole FFN with the block's residual (lightglue.py:101-106, 150-151 / 174-175):
 *                       out [n0+n1, d] = x + fp16(W2 · GELU(LayerNorm(W1 · [x | merge_heads(ctx0, ctx1)] + b1)) + b2)
 *                       with d = heads*64 = 256, W1 [2d, 2d], W2 [d, 2d]. With w_packed (W1 and W2 as
 *                       lg_ffn_pack lays them out): ONE launch, whole rows per workgroup (16 rows up to
 *                       4,096 rows, ffn_rows16_kernel; 32 up to 8,192 and 64 beyond, ffn_rows_kernel; each
 *                       wave streams its own weight fragments into registers, the GELU output stays in
 *                       LDS; within 2 fp16 ulps of the two calls).
 *                       With w_packed NULL: lg_linear_cat_ln_gelu into h [m, 2d] then lg_linear(h, W2, b2,
 *                       res = x). h must hold m*2d fp16 either way (unused by the one-launch form); out
 *                       must not alias x (16-B aligned pointers). */
int32_t lg_linear_cat_ffn(const void* x, const void* ctx0, const void* ctx1, int32_t heads, int32_t n0, int32_t n1,
                          int32_t pairs, const void* w1, const void* b1, const void* gamma, const void* beta, float eps,
                          const void* w2, const void* b2, const void* w_packed, void* h, void* out, hipStream_t stream);
/* lg_ffn_pack:          W1 [2d, 2d] and W2 [d, 2d] (nn.Linear layout, fp16, d = heads*64 = 256), and for
 *                       lg_linear_cat_ffn_proj a W3 [n3, d] (n3 = 512 or 768; 0: none), re-laid as the
 *                       one-launch FFN reads them, twice. The 32-row kernel's layout: 8 wave streams of
 *                       (96 + n3/16) KiB, stream w = W1 rows 64w..64w+63 then W2 rows 32w..32w+31 then W3
 *                       rows (n3/8)w.., in 1-KiB pieces i (W1: step j, block b at i = 2j + b; W2: step j at
 *                       i = 64 + j; W3: step j, block b at i = 96 + (n3/256) j + b) whose 16-B lane l holds
 *                       W[row0 + 32b + (l % 32)][16j + 8(l / 32) .. + 8]; then the 16-row kernel's: the same
 *                       rows per stream in 16-row blocks and k32 steps (W1: i = 4j + b, W2: i = 64 + 2j + b,
 *                       W3: i = 96 + (n3/128) j + b), lane l = W[row0 + 16b + (l % 16)][32j + 8(l / 16) .. + 8]
 *                       — every load of either kernel one contiguous KiB. lg_ffn_packed_bytes(heads, n3):
 *                       the size of both (1,572,864 B for n3 = 0; 0 if heads != 4 or n3 is not 0 / 512 /
 *                       768).
 *                       Weights are static: pack once per weight update. lg_linear_cat_ffn takes an n3 = 0 pack. */
size_t lg_ffn_packed_bytes(int32_t heads, int32_t n3);
int32_t lg_ffn_pack(const void* w1, const void* w2, const void* w3, int32_t n3, int32_t heads, void* packed,
                    hipStream_t stream);
/* lg_linear_cat_ffn_proj: lg_linear_cat_ffn's one-launch form, then — in the same launch, on its output
 *                       out = x' still in LDS — the projection the next attention needs (the 32/64-row
 *                       forms bitwise the separate call's outputs; the 16-row form sums each k32 step in
 *                       one MFMA, within 1 fp16 ulp of them; round 6):
 *                         kind LG_PROJ_SPLIT2: W3 = [W_qk; W_v] [512, d], b3 [512] -> a0, a1, b0, b1 as
 *                                              lg_linear_split2 (outs3[0..3]);
 *                         kind LG_PROJ_QKV:    W3 = Wqkv permuted [768, d], b3 [768], cos / sin [m, 64] ->
 *                                              q0, k0, v0, q1, k1, v1 as lg_linear_qkv_rotary (outs3[0..5]);
 *                         kind LG_PROJ_PLAIN:  W3 [512, d] (rows past n_store zero), b3 [512] -> outs3[0]
 *                                              [m, n_store] = x' · W3ᵀ + b3 (n_store <= 512, % 8 == 0).
 *                       w_packed = lg_ffn_pack(W1, W2, W3, 512 or 768); out [m, d] as lg_linear_cat_ffn
 *                       (all pointers 16-B aligned but b3 / cos / sin, 8-B). heads must be 4. */
#define LG_PROJ_SPLIT2 1
#define LG_PROJ_QKV 2
#define LG_PROJ_PLAIN 3
int32_t lg_linear_cat_ffn_proj(const void* x, const void* ctx0, const void* ctx1, int32_t heads, int32_t n0, int32_t n1,
                               int32_t pairs, const void* b1, const void* gamma, const void* beta, float eps, const void* b2,
                               const void* w_packed, int32_t kind, const void* b3, const void* cosv, const void* sinv,
                               int32_t n_store, void* const* outs3, void* out, hipStream_t stream);
/* lg_linear_qkv_rotary: SelfBlock projection (lightglue.py:111-134) with W's rows and the bias in
 *                       [q|k|v][head][dim] order (row j*heads*64 + h*64 + d = Wqkv row (h*64+d)*3 + j):
 *                       rotary (cos/sin [n0+n1, 64]) on q and k in fp16 arithmetic, as the reference's
 *                       fp16 model rounds t * cos + rotate_half(t) * sin (each product and the sum),
 *                       per-image head-major outputs. */
int32_t lg_linear_qkv_rotary(const void* x, const void* w_perm, const void* b_perm, const void* cos, const void* sin,
                             int32_t heads, int32_t n0, int32_t n1, int32_t pairs, int32_t k, void* q0, void* k0,
                             void* v0, void* q1, void* k1, void* v1, hipStream_t stream);
/* lg_linear_split2:     CrossBlock to_qk | to_v as one projection (W = [W_qk; W_v], lightglue.py:158-166):
 *                       per-image head-major a (= qk) and b (= v). */
int32_t lg_linear_split2(const void* x, const void* w, const void* bias, int32_t heads, int32_t n0, int32_t n1,
                         int32_t pairs, int32_t k, void* a0, void* a1, void* b0, void* b1, hipStream_t stream);

/* sigmoid_log_double_softmax (lightglue.py:197-205), fp32: scores[i][j] = 2 sim[i][j]
 * - logsumexp_j' sim[i][j'] - logsumexp_i' sim[i'][j] + logsigmoid(z0[i]) + logsigmoid(z1[j]).
 * sim, scores [batch, m, n]; z0 [batch, m], z1 [batch, n] (batch image pairs, one launch);
 * workspace >= lg_log_double_softmax_workspace(m, n, batch) bytes.
 * Non-finite operands follow IEEE arithmetic on the formula above: a -inf entry of sim adds 0 to its row's and its
 * column's sum and is -inf itself (a row or column of -inf only is outside the contract); a NaN entry makes every
 * score of its row and of its column NaN, and a NaN z its row (column); a finite z of any magnitude gives the
 * log-sigmoid's limit (0 / z) without overflow.
 * (tests/test_gpu_assignment.py holds both this entry point and the fp16 one below to that.) */
size_t lg_log_double_softmax_workspace(int32_t m, int32_t n, int32_t batch);
int32_t lg_log_double_softmax(const float* sim, const float* z0, const float* z1, int32_t m, int32_t n, int32_t batch,
                              float* scores, void* workspace, hipStream_t stream);

/* The same on the fp16 model's outputs (round 5): sim [batch, m, n] fp16 (16-B aligned, n % 8 == 0,
 * n <= 2048) read directly, the matchability logits fp16 and strided — z0 of pair p, row i at
 * z0[p * z_pair_stride + i * z_row_stride], z1 of pair p, column j at z1[p * z_pair_stride + j *
 * z_row_stride] (one channel of the final projection's output) — scores fp32 (16-B aligned). Two
 * launches; workspace >= lg_log_double_softmax_f16_workspace(m, n, batch) bytes. Non-finite operands: as
 * lg_log_double_softmax. */
size_t lg_log_double_softmax_f16_workspace(int32_t m, int32_t n, int32_t batch);
int32_t lg_log_double_softmax_f16(const void* sim, const void* z0, const void* z1, int64_t z_pair_stride,
                                  int64_t z_row_stride, int32_t m, int32_t n, int32_t batch, float* scores,
                                  void* workspace, hipStream_t stream);

/* The fp16 assignment head in two launches (round 6; csrc/lightglue_assign.hip, with the match head
 * below): v [batch][m + n][ld] fp16 is the final
 * projection of both images' rows (image 0's m rows, then image 1's n; pairs pair_stride elements
 * apart), channels 0..255 the scaled descriptors m0 / m1 (final_proj(d) / d^0.25) and channel zc
 * (>= 256) the matchability logit. scores [batch, m, n] fp32 = log_softmax(sim, 2) + log_softmax(sim, 1)
 * + logsig(z0) + logsig(z1)ᵀ with sim = m0 · m1ᵀ rounded to fp16 (lightglue.py:208-233): the similarity
 * by MFMA with each row's and column's (max, sum of exponentials) over shares of the other image (a
 * workgroup owns 32 rows of one image), then the combine, which closes its rows' and columns'
 * logsumexps from those partials.
 * m, n <= 2048, n % 8 == 0, ld % 8 == 0; v, scores, workspace 16-B aligned; workspace >=
 * lg_assign_scores_workspace(m, n, batch) bytes (its first batch * m * n * 2 bytes: sim, fp16).
 * Operands are assumed finite (the file is built without NaN semantics: -fno-honor-nans). What the tests pin beyond
 * that: matchability logits up to +-65504 give the exact log-sigmoid (0 / z); a row of v that is NaN in every
 * channel gives NaN in every score of its row and, where its share of the other image's split holds a finite row as
 * well (always, below 257 rows), of every column; a similarity that overflows fp16 is outside the contract. */
size_t lg_assign_scores_workspace(int32_t m, int32_t n, int32_t batch);
int32_t lg_assign_scores(const void* v, int64_t pair_stride, int32_t ld, int32_t zc, int32_t m, int32_t n, int32_t batch,
                         float* scores, void* workspace, hipStream_t stream);

/* The match head: filter_matches (lightglue.py:235-258, with the dense outputs it keeps commented out)
 * applied to the scores lg_assign_scores would write for the same v, without that tensor: at most
 * three launches (the similarity + logsumexp launch of lg_assign_scores, a "best" pass in the
 * combine's place that keeps each row's and column's (max, index) per block, and one workgroup per
 * pair that closes them and writes the outputs), no atomics, bitwise reproducible.
 *   s[i][j] = (2 sim[i][j] + rterm[i]) + cterm[j]   (each with the bits lg_assign_scores writes)
 *   j*(i) = argmax_j s[i][j], i*(j) = argmax_i s[i][j], ties to the lowest index
 *   mscores0[i] = i*(j*(i)) == i ? expf(s[i][j*(i)]) : 0;  valid0[i] = mscores0[i] > threshold
 *   matches0[i] = valid0[i] ? j*(i) : -1
 *   mutual1[j] = j*(i*(j)) == j;  mscores1[j] = mutual1 ? mscores0[i*(j)] : 0
 *   matches1[j] = mutual1 && valid0[i*(j)] ? i*(j) : -1
 *   matches / mscores: the valid rows (i, j*(i)) / mscores0[i] in ascending i; counts[p] their number
 *   (<= min(m, n)); list rows past it hold -1 / 0.
 * v, pair_stride, ld, zc, m, n, batch as for lg_assign_scores (m, n <= 2048, n % 8 == 0, ld % 8 == 0,
 * 256 <= zc < ld); threshold >= 0; v and workspace 16-B aligned, the outputs 4-B aligned; workspace >=
 * lg_assign_matches_workspace(m, n, batch) bytes (lg_assign_scores' layout, then the per-block bests).
 * batch == 0 is a no-op; m == 0 or n == 0 writes only counts (zeros; it may then be null). Inputs are
 * assumed finite; otherwise values are unspecified but every index written is in range or -1.
 * (Additions leave every earlier argument list as it was, so LG_GLUE_ABI_VERSION stays 4; a library
 * built before them lacks the symbols, which the Python loader reports as a stale library.) */
size_t lg_assign_matches_workspace(int32_t m, int32_t n, int32_t batch);
int32_t lg_assign_matches(const void* v, int64_t pair_stride, int32_t ld, int32_t zc, int32_t m, int32_t n, int32_t batch,
                          float threshold, int32_t* matches0, int32_t* matches1, float* mscores0, float* mscores1,
                          int32_t* matches, float* mscores, int32_t* counts, void* workspace, hipStream_t stream);

/* Both heads on ragged batches: the layout is the padded one (m and n stay the strides and limits:
 * <= 2048, n % 8 == 0), and pair p's leading m_len[p] rows of image 0 and n_len[p] rows of image 1 are
 * real. m_len, n_len: DEVICE int32 [batch], 4-B aligned, clamped into [1, m] / [1, n] by the kernels,
 * multiples of nothing; a null table means every pair has all m (n) rows, and with both null the
 * results equal lg_assign_scores / lg_assign_matches bit for bit. The counts are read when the kernels
 * run (a captured call replays with what the tables hold then).
 * Everything said above for lg_assign_scores / lg_assign_matches holds on the pair's [m_len, n_len]
 * sub-matrix: both logsumexps run over its entries only, and
 *   scores[p][i][j] = -inf exactly for i >= m_len[p] or j >= n_len[p];
 *   matches0 = -1 and mscores0 = 0 on padded rows, matches1 = -1 and mscores1 = 0 on padded columns;
 *   the list keeps min(m, n) rows per pair, counts[p] <= min(m_len[p], n_len[p]).
 * (So filter_matches on the padded scores gives the pair's matches unchanged.) No padded row of v is
 * ever read: it may hold anything, NaN and Inf included. Workspaces: lg_assign_scores_workspace /
 * lg_assign_matches_workspace of (m, n, batch), the same layout. New symbols only:
 * LG_GLUE_ABI_VERSION stays 4. */
int32_t lg_assign_scores_lens(const void* v, int64_t pair_stride, int32_t ld, int32_t zc, int32_t m, int32_t n, int32_t batch,
                              const int32_t* m_len, const int32_t* n_len, float* scores, void* workspace,
                              hipStream_t stream);
int32_t lg_assign_matches_lens(const void* v, int64_t pair_stride, int32_t ld, int32_t zc, int32_t m, int32_t n,
                               int32_t batch, const int32_t* m_len, const int32_t* n_len, float threshold,
                               int32_t* matches0, int32_t* matches1, float* mscores0, float* mscores1, int32_t* matches,
                               float* mscores, int32_t* counts, void* workspace, hipStream_t stream);

/* ---- adaptive depth and width (csrc/lightglue_adaptive.hip; fp16 rows of 256 channels) ----
 * The published LightGlue rules the reference ships the pieces of (TokenConfidence lightglue.py:54-66,
 * MatchAssignment.get_matchability :230-232) and never applies. New symbols only: LG_GLUE_ABI_VERSION
 * stays 4. Rows are pair-major as everywhere ([pairs * (m + n), ...]); m_len / n_len are the lens forms'
 * DEVICE int32 [pairs] tables (null: all m / n rows; clamped into [1, m] / [1, n] by the kernels), and
 * no row past a pair's count is ever read. Every call checks its arguments before any device call.
 *
 * lg_token_scores: for each valid row r of x [pairs * (m + n), 256]
 *   conf = sigmoid(w_tok · x_r + b_tok), mtch = sigmoid(w_match · x_r + b_match)
 * (w_* fp16 [256], 16-B aligned; b_* one fp16 value each, on the device; fp32 accumulation in a fixed
 * order and an fp32 sigmoid), and
 *   keep = 1                                              for an image whose LG_ADAPT_WIDTHi flag is clear,
 *   keep = mtch > t_keep || (LG_ADAPT_DEPTH && conf <= t_conf)   otherwise;
 * a pruned segment (one image of one pair) that kept no row keeps its row of highest mtch, the lowest
 * index on ties. conf, mtch fp32 [pairs, m + n]; keep uint8 [pairs, m + n]; padded rows: 0 in all three.
 * stats int32 [pairs, 4] = (kept rows of image 0, of image 1, valid rows of both images with
 * conf < t_conf, valid rows of both images); the call zeroes it first. One launch, and a second tiny
 * one for the min-one rule when a width flag is set. 0 <= t_conf <= 1. */
#define LG_ADAPT_DEPTH 1
#define LG_ADAPT_WIDTH0 2
#define LG_ADAPT_WIDTH1 4
int32_t lg_token_scores(const void* x, int32_t m, int32_t n, int32_t pairs, const int32_t* m_len, const int32_t* n_len,
                        const void* w_tok, const void* b_tok, const void* w_match, const void* b_match, float t_conf,
                        float t_keep, int32_t flags, float* conf, float* mtch, uint8_t* keep, int32_t* stats,
                        hipStream_t stream);

/* lg_compact_rows: the stable gather of the rows with keep != 0 (keep [pairs, m + n], read below each
 * pair's count only) from the layout (m, n) into the layout (m_out <= m, n_out <= n): x [.., 256], cos and
 * sin [.., 64] (bitwise copies; 16-B aligned, the outputs distinct from the inputs), and the running
 * index maps ind0 [pairs, m] -> ind0_out [pairs, m_out], ind1 [pairs, n] -> ind1_out [pairs, n_out] (a
 * null input map is the identity). m_len_out / n_len_out [pairs]: the kept rows per segment, the next
 * layout's counts (a segment with no kept row gets 0, which every lens form reads as 1: lg_token_scores
 * never leaves one). A kept row whose destination is past m_out / n_out is dropped and the count capped
 * (the caller sizes the layout from lg_token_scores' stats); output rows past the new counts are not
 * written. One launch over 64-row tiles; a tile's first destination is the count of its segment's flags
 * before it. With prune0 [pairs, m_orig] / prune1 [pairs, n_orig] (both or neither): the dropped rows'
 * entries, at their original index, are set to `layers` (the layers they took part in). */
int32_t lg_compact_rows(const void* x, const void* cosv, const void* sinv, const uint8_t* keep, const int32_t* ind0,
                        const int32_t* ind1, int32_t m, int32_t n, int32_t pairs, const int32_t* m_len, const int32_t* n_len,
                        int32_t m_out, int32_t n_out, void* x_out, void* cos_out, void* sin_out, int32_t* ind0_out,
                        int32_t* ind1_out, int32_t* m_len_out, int32_t* n_len_out, int32_t* prune0, int32_t* prune1,
                        int32_t m_orig, int32_t n_orig, int32_t layers, hipStream_t stream);

/* lg_matches_scatter: lg_assign_matches' seven outputs for the surviving rows (layout m_cur x n_cur, the
 * list min(m_cur, n_cur) long; counts m_len / n_len) mapped through ind0 [pairs, m_cur] / ind1 [pairs,
 * n_cur] (null: identity) into the original layout m x n (m_cur <= m, n_cur <= n, m, n <= 2048): indices
 * become original indices, rows and columns that no surviving row maps to hold -1 / 0, the list keeps its
 * order (a stable compaction keeps i ascending) and min(m, n) rows. prune0 [pairs, m] / prune1 [pairs, n]
 * (nullable): the surviving rows' entries are set to `stop`, the others left as lg_compact_rows (or the
 * caller's initial zeros) wrote them. One launch; every output element is written exactly once. */
int32_t lg_matches_scatter(const int32_t* matches0, const int32_t* matches1, const float* mscores0, const float* mscores1,
                           const int32_t* matches, const float* mscores, const int32_t* counts, const int32_t* ind0,
                           const int32_t* ind1, const int32_t* m_len, const int32_t* n_len, int32_t m_cur, int32_t n_cur,
                           int32_t m, int32_t n, int32_t pairs, int32_t stop, int32_t* out_matches0, int32_t* out_matches1,
                           float* out_mscores0, float* out_mscores1, int32_t* out_matches, float* out_mscores,
                           int32_t* out_counts, int32_t* prune0, int32_t* prune1, hipStream_t stream);

/* ---- keypoint front end (csrc/lightglue_frontend.hip) ----
 * SuperPoint's two dense heads (the outputs of convPb and convDb, superpoint.py:157, 172) to the matcher's
 * inputs (kpts, desc, counts) on the device: simple_nms (superpoint.py:52-69), sample_descriptors (:72-87) and
 * SuperPointMonoTRT::PostProcess (demo/superpoint_mono_trt.cpp:153-253) without nonzero's synchronisation.
 * All `batch` images of a call share one size, h = 8 hc, w = 8 wc, and go through every launch together
 * (batch <= 65,535, h * w <= 2^26, batch * h * w <= 2^30). New symbols only: LG_GLUE_ABI_VERSION stays 4.
 * Every call checks its arguments before any device call, runs on `stream`, is a no-op for batch == 0 and
 * clamps every index it forms into range whatever its inputs hold.
 *
 * lg_kp_heatmap: logits [batch, 65, hc, wc] (dtype fp16 or fp32, contiguous) -> scores [batch, h, w] fp32
 * (16-B aligned): the softmax over the 65 channels in fp32 with the maximum subtracted, the dustbin dropped,
 * channel c of cell (i, j) at pixel (8 i + c / 8, 8 j + c % 8) (superpoint.py:160-165). One launch. */
int32_t lg_kp_heatmap(int32_t dtype, const void* logits, int32_t hc, int32_t wc, int32_t batch, float* scores,
                      hipStream_t stream);
/* lg_kp_nms: simple_nms with radius 0..4 on scores [batch, h, w] fp32 (any h, w >= 1) -> out (not in place):
 * the first maximum mask and the two suppression rounds with their == comparisons (every member of a
 * plateau survives) and the pools' -inf padding at the image edge; bitwise the reference's result on finite
 * input. One launch: 32 x 32 tiles with a halo of 5 * radius, the five pools separable in LDS. */
int32_t lg_kp_nms(const float* scores, int32_t h, int32_t w, int32_t batch, int32_t radius, float* out,
                  hipStream_t stream);
/* lg_kp_select: the candidates of nms [batch, h, w] are the pixels at least `border` pixels inside every edge
 * with a value > threshold (threshold >= 0); the k best of each image (1 <= k <= 2048, k % 8 == 0) in
 * descending score, ties by ascending row-major pixel index: count [batch] = min(candidates, k), pix
 * [batch, k] (row-major pixel index; -1 past the count), score [batch, k] (0 past the count). Bitwise
 * reproducible. Two launches (a compaction into per-segment lists, then one workgroup per image: radix select
 * and a bitonic sort), no state kept between calls; workspace (16-B aligned) >= lg_kp_select_workspace(h, w,
 * batch) bytes. */
size_t lg_kp_select_workspace(int32_t h, int32_t w, int32_t batch);
int32_t lg_kp_select(const float* nms, int32_t h, int32_t w, int32_t batch, int32_t border, float threshold, int32_t k,
                     int32_t* count, int32_t* pix, float* score, void* workspace, hipStream_t stream);
/* lg_kp_describe: count / pix as lg_kp_select wrote them (count clamped into [0, k], pix into the image) and
 * the dense descriptors, 256 channels on the hc x wc grid, element (b, c, y, x) at dense[b stride_b + c stride_c
 * + y stride_y + x stride_x] (dense_dtype fp16 or fp32; strides >= 0: NCHW and channels-last without a copy).
 * Per keypoint: grid_sample (bilinear, align_corners, zero padding) at ((x - 3.5) / (8 wc - 4.5)) (wc - 1),
 * likewise y (sample_descriptors / PostProcess:219-232); with dense_normalized == 0 each corner vector is first
 * divided by max(its channel norm, 1e-12) (superpoint.py:173, fused); the result is divided by max(its norm,
 * 1e-12). desc [batch, k, 256] and kpts [batch, k, 2] = (xy - (w / 2, h / 2)) / (max(w, h) / 2) in out_dtype,
 * kpts_px [batch, k, 2] int32 (x, y); rows past the count are zero in all three. One launch, one wave per
 * keypoint. */
int32_t lg_kp_describe(int32_t dense_dtype, const void* dense, int64_t stride_b, int64_t stride_c, int64_t stride_y,
                       int64_t stride_x, int32_t hc, int32_t wc, int32_t batch, int32_t k, const int32_t* count,
                       const int32_t* pix, int32_t dense_normalized, int32_t out_dtype, void* desc, int32_t* kpts_px,
                       void* kpts, hipStream_t stream);

/* ---- SuperPoint encoder (csrc/lightglue_superpoint.hip) ----
 * The SuperPoint forward up to its two dense heads (superpoint.py:143-172) in fp16: activations are NHWC fp16
 * ([batch, h, w, c], 16-B aligned), a layer accumulates in fp32, adds its bias (fp16 values) in fp32, applies
 * ReLU if asked and rounds to fp16 once. Ten launches take images to lg_kp_heatmap's and lg_kp_describe's
 * inputs: lg_sp_conv1, eight lg_sp_conv3x3 (convPa and convDa as one layer of 512 channels) and lg_sp_heads.
 * Limits as the front end's (batch <= 65,535, h * w <= 2^26, batch * h * w <= 2^30). New symbols only:
 * LG_GLUE_ABI_VERSION stays 4. Every call checks its arguments before any device call, runs on `stream`, is
 * a no-op for batch == 0, keeps no state and uses no atomics.
 *
 * Packed weights (fp16, packed once by the host; lightglue_amd.superpoint.pack_conv is the packer): a
 * convolution weight [cout, cin, kh, kw] (cout % 32 == 0, cin % 16 == 0) is stored fragment-major as
 * [cout / 32][kh kw][cin / 16][2][32][8]: element (cb, t, ks, hi, r, j) is weight[32 cb + r][16 ks + 8 hi + j]
 * [t / kw][t % kw], the 16 B lane 32 hi + r feeds v_mfma_f32_32x32x16_f16 as the A operand of tap t, k-step ks.
 * lg_sp_packed_bytes: the size of that stream for a layer the kernels take (taps 9: cin 64 / 128, cout 64 /
 * 128 / 256 / 512; taps 1: the heads' cin 256, cout 352), 0 otherwise. */
#define LG_SP_RELU 1
#define LG_SP_POOL2 2
size_t lg_sp_packed_bytes(int32_t taps, int32_t cin, int32_t cout);
/* lg_sp_conv1: conv1a, 1 -> 64 channels, 3 x 3, pad 1. image [batch, h, w] contiguous (image_dtype fp32 or
 * fp16), weight [64, 1, 3, 3] and bias [64] fp16 (plain, not packed; 16-B aligned) -> out [batch, h, w, 64].
 * flags: LG_SP_RELU. */
int32_t lg_sp_conv1(int32_t image_dtype, const void* image, const void* weight, const void* bias, int32_t h, int32_t w,
                    int32_t batch, int32_t flags, void* out, hipStream_t stream);
/* lg_sp_conv3x3: 3 x 3, pad 1 (zeros outside each image), cin 64 / 128 -> cout 64 / 128 / 256 / 512. in
 * [batch, h, w, cin], w_packed as above (16-B aligned), bias [cout] fp16 (8-B aligned) -> out [batch, h, w,
 * cout], or with LG_SP_POOL2 (h and w even) the 2 x 2 / stride-2 maximum of that, [batch, h / 2, w / 2, cout].
 * flags: LG_SP_RELU | LG_SP_POOL2. Not in place. One launch: 8 x 16 pixel tiles, patch and halo in LDS. */
int32_t lg_sp_conv3x3(const void* in, const void* w_packed, const void* bias, int32_t cin, int32_t cout, int32_t h, int32_t w,
                      int32_t batch, int32_t flags, void* out, hipStream_t stream);
/* lg_sp_heads: the two 1 x 1 heads in one launch. in [batch, hc, wc, 512] = cPa | cDa; w_packed the packing of
 * [convPb's [65, 256] padded with zero rows to 96 ; convDb's [256, 256]] (352 rows) and bias [352] alike (rows
 * 65..95 unused). convPb reads channels 0..255 -> logits [batch, 65, hc, wc] contiguous (lg_kp_heatmap's input),
 * convDb channels 256..511 -> dense [batch, hc, wc, 256] (lg_kp_describe's input through channels-last
 * strides). No ReLU. */
int32_t lg_sp_heads(const void* in, const void* w_packed, const void* bias, int32_t hc, int32_t wc, int32_t batch,
                    void* logits, void* dense, hipStream_t stream);

/* ---- image input (csrc/lightglue_image.hip) ----
 * What the reference does on the host before its network sees a frame (demo/demo_mono.cpp:151-152, 232-233:
 * resize to 640 x 480 with INTER_LINEAR, / 255; lightglue_pytorch_no_plugin/utils.py:30-76: resize, grey) and
 * after it (utils.py:94-97: keypoints back to the source image): uint8 images of any size, channel count and
 * strides -> the encoder's input [batch, ht, wt] (contiguous, grey, in [0, 1], fp16 or fp32) in one launch, and
 * lg_kp_describe's pixel keypoints -> source pixels. New symbols only: LG_GLUE_ABI_VERSION stays 4. Every call
 * checks its arguments before any device call, runs on `stream`, is a no-op for batch == 0, keeps no state,
 * uses no atomics and clamps every index it forms; no workgroup reads what another wrote.
 *
 * A source image: element (y, x, c) is the byte at data + y stride_y + x stride_x + c stride_c (strides in bytes,
 * >= 0: HWC, CHW and cropped views are read in place); h, w in [1, 16384]; channels 1 (grey, used as it is), 3
 * or 4 (the fourth is ignored); bgr != 0: channel 0 is blue. grey = 0.299 R + 0.587 G + 0.114 B (utils.py:72-76).
 *
 * Resampling: out = Wy · grey · Wxᵀ / 255, the rule chosen per axis (shown for x, source w, target wt):
 *   LG_IMG_LINEAR: output column o sits at source position ((2 o + 1) w - wt) / (2 wt) = i + f (i its floor):
 *                  weights 1 - f and f on columns i and i + 1, both clamped into [0, w - 1] (INTER_LINEAR's and
 *                  F.interpolate(bilinear, align_corners=False)'s convention);
 *   LG_IMG_AREA:   where w > wt, output o covers [o w / wt, (o + 1) w / wt) and column i weighs its overlap with
 *                  that interval divided by w / wt (INTER_AREA); on an axis that does not shrink, LG_IMG_LINEAR.
 * Positions and overlaps are exact integer rationals, each weight one fp32 division; sums in fp32, one rounding
 * to the output type. The result is the unrounded float (INTER_LINEAR's fixed-point rounding to uint8 is not
 * reproduced). */
typedef struct lg_img_src {
    const void* data;
    int32_t h, w;
    int32_t channels;
    int32_t bgr;
    int64_t stride_y, stride_x, stride_c;
} lg_img_src;
#define LG_IMG_LINEAR 0
#define LG_IMG_AREA 1
/* sizeof(lg_img_src), for a host that builds the table without this header (48). */
size_t lg_img_src_bytes(void);
/* lg_img_prepare: table: DEVICE array of `batch` descriptors (8-B aligned), read when the kernel runs (a captured
 * call replays on what the table and the images hold then). Its contents are the caller's contract: the kernel
 * clamps h and w into [1, 16384] and takes a channel count other than 3 or 4 as 1, but cannot check a pointer or
 * a stride. ht, wt in [1, 16384] (multiples of nothing); out [batch, ht, wt] of out_dtype (fp16 / fp32).
 * batch <= 65,535. One launch: a lane per output pixel, a wave on 64 adjacent columns of one row. */
int32_t lg_img_prepare(const lg_img_src* table, int32_t batch, int32_t ht, int32_t wt, int32_t interp, int32_t out_dtype,
                       void* out, hipStream_t stream);
/* lg_img_prepare_batch: the same kernel body on `batch` images of one size, image b at data + b stride_b (video
 * frames, one [batch, ...] tensor): no table, every argument checked here (h, w in [1, 16384]; channels 1, 3 or 4;
 * bgr 0 or 1; strides in [0, 2^40]). Bitwise lg_img_prepare's result on the same images. */
int32_t lg_img_prepare_batch(const void* data, int32_t batch, int32_t h, int32_t w, int32_t channels, int32_t bgr,
                             int64_t stride_b, int64_t stride_y, int64_t stride_x, int64_t stride_c, int32_t ht, int32_t wt,
                             int32_t interp, int32_t out_dtype, void* out, hipStream_t stream);
/* lg_kp_to_source: kpts_px [batch, k, 2] int32 (x, y) in the [ht, wt] image (lg_kp_describe's; clamped into it),
 * counts [batch], src_sizes [batch, 2] int32 (h, w of image b's source, clamped into [1, 16384]) -> out
 * [batch, k, 2] fp32 in source pixels: x = (2 px + 1) w / (2 wt) - 1/2, likewise y (utils.py:94-97 with scale =
 * wt / w), the quotient and remainder of ((2 px + 1) w - wt) / (2 wt) exact (w == wt: exactly px). Rows past the
 * count (clamped into [0, k]) are zeros. All pointers 4-B aligned; k >= 1, batch k <= 2^28. One launch. */
int32_t lg_kp_to_source(const int32_t* kpts_px, const int32_t* counts, const int32_t* src_sizes, int32_t ht, int32_t wt,
                        int32_t batch, int32_t k, float* out, hipStream_t stream);

/* ---- geometric verification (csrc/lightglue_geometry.hip) ----
 * What the reference's demo does on the host after PostProcess (demo/demo_mono.cpp:326-366):
 * cv::findFundamentalMat(points0, points1, cv::FM_RANSAC, 3, 0.99, inliers), here per pair of a batch on the
 * device, from the matcher's outputs as they are. New symbols only: LG_GLUE_ABI_VERSION stays 4. Every call
 * checks its arguments before any device call, runs on `stream`, is a no-op for pairs == 0, keeps no state, uses
 * no atomics and allocates nothing; no workgroup reads what another wrote within a launch; every output entry is
 * written on every call. lightglue_amd/geometry_contract.py restates the contract in float64 (ransac_reference).
 *
 * Inputs (shared by the four calls): matches [pairs, kmax, 2] int32 and counts [pairs] int32 (MatchResult's),
 * kpts0 [pairs, k0, 2], kpts1 [pairs, k1, 2] fp32 (x, y) in any pixel frame (lg_kp_to_source's output is the
 * intended one). Correspondence k < counts[p] of pair p is (kpts0[p, matches[p, k, 0]], kpts1[p, matches[p, k, 1]]);
 * counts are clamped into [0, kmax] and indices into range, neither is trusted. 1 <= kmax <= 2048, k0, k1 >= 1,
 * pairs <= 65,535, pairs * kmax, pairs * k0, pairs * k1 <= 2^28; matches, kpts0, kpts1 8-B aligned, every other
 * pointer 4-B.
 *
 * Model: x1ᵀ F x0 = 0 with x = (x, y, 1), F row-major. Error of a correspondence (OpenCV's for FM_RANSAC):
 * l1 = F x0, l0 = Fᵀ x1, d = x1 · l1, err = max(d² / (l1x² + l1y²), d² / (l0x² + l0y²)); an inlier iff
 * err <= threshold² (a non-finite err is none). Per pair, independently:
 *   1. Hartley normalisation per image over all `count` correspondences (centroid to 0, mean distance sqrt 2;
 *      sums in fp64 in a fixed order).
 *   2. Hypothesis h samples 7 distinct indices: draw j = hash32(seed, h, j) % (count - j), moved past the earlier
 *      draws in ascending order (ransac_samples in geometry_contract.py is the definition; the pair is not in the key).
 *   3. The 7-point solve in normalised coordinates, fp64 (an fp32 solve leaves its own sample points up to 0.5 px
 *      off their lines): Gauss-Jordan with row pivoting on the 7 x 9 system (a pivot below 1e-6: no
 *      candidate), the canonical null vectors f1 = (.., 1, 0), f2 = (.., 0, 1), the real roots l of
 *      det(l f1 + (1 - l) f2) = 0 in ascending order, each candidate de-normalised to pixels at unit Frobenius
 *      norm and rounded to fp32 (a non-finite one is dropped): 0 to 3 candidates.
 *   4. Every candidate is scored against all correspondences in pixels, fp32. The winner: the highest inlier
 *      count, then the lowest hypothesis, then the lowest root.
 *   5. `refits` rounds of a normalised 8-point least squares over the current inliers in fp64 (Hartley over the
 *      inliers, the eigenvector of the smallest eigenvalue of the 9 x 9 normal matrix by Jacobi, rank 2 by
 *      F <- F (I - v vᵀ) with v the smallest right-singular direction), then the inliers again. A round with fewer
 *      than 8 inliers, or a refit that is not finite, keeps the previous F and mask.
 * A pair with count < 8, with no candidate or with a winner of fewer than 8 inliers: valid = 0, F = 0, no inlier,
 * best = -1. The number of hypotheses is fixed (no early termination by a confidence): the launches do not
 * depend on the data and a call can be captured. */
/* Bytes of lg_ransac_fundamental's workspace (0 for an empty call). */
size_t lg_ransac_workspace(int32_t pairs, int32_t kmax, int32_t hypotheses);
/* lg_ransac_fundamental: two launches (hypotheses: grid (hypotheses / 64, pairs), four lanes per hypothesis over
 * the pair's correspondences in LDS; then one workgroup per pair: winner, refits, outputs). threshold in (0, 1e6]
 * pixels, 1 <= hypotheses <= 4096, 0 <= refits <= 8, any seed; workspace 16-B aligned, at least
 * lg_ransac_workspace bytes. Outputs: f [pairs, 3, 3] fp32 (unit Frobenius norm, the entry of the largest
 * magnitude positive, the lowest index among equals), inliers [pairs, kmax] uint8 (aligned with the rows of
 * matches, 0 past the count), num_inliers, valid, best [pairs] int32 (best: the winning hypothesis or -1). */
int32_t lg_ransac_fundamental(const int32_t* matches, const int32_t* counts, const float* kpts0, const float* kpts1,
                              int32_t pairs, int32_t kmax, int32_t k0, int32_t k1, float threshold, int32_t hypotheses,
                              int32_t refits, int32_t seed, void* workspace, size_t workspace_bytes, float* f,
                              uint8_t* inliers, int32_t* num_inliers, int32_t* valid, int32_t* best, hipStream_t stream);
/* Stage hooks over the same device code (tests). lg_ransac_samples: step 2 for one count in [7, 2048] ->
 * samples [hypotheses, 7] int32 in draw order. */
int32_t lg_ransac_samples(int32_t count, int32_t hypotheses, int32_t seed, int32_t* samples, hipStream_t stream);
/* lg_ransac_solve7: steps 1 and 3 on given samples [hypotheses, 7] int32 (device; clamped into [0, count), shared
 * by the pairs) -> candidates [pairs, hypotheses, 3, 9] fp32 (those that exist first, the rest zeros) and
 * num_roots [pairs, hypotheses] int32. A pair with count < 8: zeros. */
int32_t lg_ransac_solve7(const int32_t* matches, const int32_t* counts, const float* kpts0, const float* kpts1, int32_t pairs,
                         int32_t kmax, int32_t k0, int32_t k1, const int32_t* samples, int32_t hypotheses, float* candidates,
                         int32_t* num_roots, hipStream_t stream);
/* lg_ransac_score: step 4's count for given candidates [pairs, num_candidates, 9] fp32 (1 <= num_candidates <=
 * 4096) -> inlier_counts [pairs, num_candidates] int32. */
int32_t lg_ransac_score(const int32_t* matches, const int32_t* counts, const float* kpts0, const float* kpts1, int32_t pairs,
                        int32_t kmax, int32_t k0, int32_t k1, const float* candidates, int32_t num_candidates, float threshold,
                        int32_t* inlier_counts, hipStream_t stream);

/* The homography, next to the fundamental matrix: what stitching, planar tracking, registration and the
 * HPatches protocol run on the host as cv::findHomography(pts0, pts1, cv::RANSAC, 3), and the right model where
 * the epipolar constraint is degenerate (a planar scene, a purely rotating camera). The same kernels, templates on
 * the model. Inputs, clamping, limits and alignment are lg_ransac_fundamental's, and so is every general
 * statement above (arguments checked first, a no-op for pairs == 0, no atomics, no allocation, every output
 * entry written). lightglue_amd/geometry_contract.py restates the contract in float64 (homography_reference).
 *
 * Model: x1 ~ H x0 with x = (x, y, 1), H row-major. Error of a correspondence (OpenCV's for findHomography with
 * RANSAC): (X, Y, W) = H x0, err = (x1 - X/W)² + (y1 - Y/W)²; an inlier iff err <= threshold². A non-finite err is
 * none (W = 0, a NaN or Inf coordinate, a zero or NaN H). The kernels test dx² + dy² <= threshold² W² with
 * dx = x1 W - X, dy = y1 W - Y, W² > 0 and the left side finite. Per pair, independently:
 *   1. Hartley normalisation, as step 1 above.
 *   2. Hypothesis h samples 4 distinct indices: the first four draws of step 2 above (for count >= 7 the first
 *      four columns of the 7-sample; defined from count = 4 on; ransac_samples(size=4) in geometry_contract.py).
 *   3. The 4-point solve in normalised coordinates, fp64 (for the reason of the 7-point solve; the fp32 figures
 *      are in profiles/geometry/INDEX.md): the 8 x 9 system of two rows a point,
 *      (-x0, -y0, -1, 0, 0, 0, x1 x0, x1 y0, x1) and (0, 0, 0, -x0, -y0, -1, y1 x0, y1 y0, y1), by Gauss-Jordan with
 *      row pivoting on columns 0..7 in order; the canonical null vector ends in 1 (h8 = 1 in the normalised frame).
 *      A pivot below 1e-6: no candidate (three collinear sample points, a repeated index, a true h8 of 0).
 *      Orientation rule (OpenCV's checkSubset): for the four triples of the sample, the sign of the 2 x 2
 *      orientation determinant in image 0 times that in image 1, in the normalised fp64 coordinates; products
 *      neither all positive nor all negative: no candidate. De-normalised by H = T1⁻¹ Hn T0, scaled to unit
 *      Frobenius norm with the sign rule of f, rounded to fp32 (a non-finite one is dropped): 0 or 1 candidate.
 *   4. The candidate is scored against all correspondences in pixels, fp32. The winner: the highest inlier count,
 *      then the lowest hypothesis.
 *   5. `refits` rounds of a normalised DLT over the current inliers in fp64 (Hartley over the inliers, the same two
 *      rows an inlier, the eigenvector of the smallest eigenvalue of the 9 x 9 normal matrix by the same Jacobi,
 *      no rank step, de-normalised), then the inliers again. A round with fewer than 4 inliers, or a refit that
 *      is not finite, keeps the previous H and mask. OpenCV's final Levenberg-Marquardt polish is not built.
 * A pair with count < 4, with no candidate or with a winner of fewer than 4 inliers: valid = 0, H = 0, no inlier,
 * best = -1. A 4-inlier winner is only its own sample: callers should threshold num_inliers.
 *
 * lg_ransac_homography: lg_ransac_fundamental's arguments with h [pairs, 3, 3] fp32 in place of f; the workspace
 * is lg_ransac_workspace's (the record of a hypothesis is the same). Two launches. */
int32_t lg_ransac_homography(const int32_t* matches, const int32_t* counts, const float* kpts0, const float* kpts1,
                             int32_t pairs, int32_t kmax, int32_t k0, int32_t k1, float threshold, int32_t hypotheses,
                             int32_t refits, int32_t seed, void* workspace, size_t workspace_bytes, float* h,
                             uint8_t* inliers, int32_t* num_inliers, int32_t* valid, int32_t* best, hipStream_t stream);
/* Stage hooks over the same device code (tests). lg_ransac_samples4: step 2 for one count in [4, 2048] ->
 * samples [hypotheses, 4] int32 in draw order. */
int32_t lg_ransac_samples4(int32_t count, int32_t hypotheses, int32_t seed, int32_t* samples, hipStream_t stream);
/* lg_ransac_solve4: steps 1 and 3 on given samples [hypotheses, 4] int32 (device; clamped into [0, count), shared
 * by the pairs) -> candidates [pairs, hypotheses, 9] fp32 (zeros where there is none) and num [pairs, hypotheses]
 * int32, 0 or 1. A pair with count < 4: zeros. */
int32_t lg_ransac_solve4(const int32_t* matches, const int32_t* counts, const float* kpts0, const float* kpts1, int32_t pairs,
                         int32_t kmax, int32_t k0, int32_t k1, const int32_t* samples, int32_t hypotheses, float* candidates,
                         int32_t* num, hipStream_t stream);
/* lg_ransac_score_homography: step 4's count for given candidates [pairs, num_candidates, 9] fp32
 * (1 <= num_candidates <= 4096) -> inlier_counts [pairs, num_candidates] int32. */
int32_t lg_ransac_score_homography(const int32_t* matches, const int32_t* counts, const float* kpts0, const float* kpts1,
                                   int32_t pairs, int32_t kmax, int32_t k0, int32_t k1, const float* candidates,
                                   int32_t num_candidates, float threshold, int32_t* inlier_counts, hipStream_t stream);

/* The calibrated relative pose (csrc/lightglue_essential.hip): an essential matrix per pair by five-point RANSAC
 * and (R, t) from it, for callers who know their cameras (visual odometry, localisation, pose-AUC evaluation).
 * Five points need far fewer hypotheses than seven at the same outlier rate, and the five-point solve is not
 * degenerate on planar scenes, which the 7- and 8-point solves are. Inputs, clamping, limits and alignment are
 * lg_ransac_fundamental's, and so is every general statement above (arguments checked first, a no-op for
 * pairs == 0, counts and indices clamped, no atomics, no allocation, every output entry written).
 * lightglue_amd/geometry_contract.py restates the contract in float64 (essential_reference).
 *
 * Extra input: intrinsics [pairs, 2, 4] fp32, (fx, fy, cx, cy) of image 0 then image 1 in the pixel frame of the
 * keypoints. Model: x1ᵀ E x0 = 0 in camera coordinates q = ((x - cx) / fx, (y - cy) / fy) (fp64), E row-major;
 * X1 = R X0 + t, |t| = 1, det R = +1, E ∝ [t]x R. Canonical: unit Frobenius norm with the sign rule of f. Per pair:
 *   1. Gather as above. Fewer than 5 correspondences, an intrinsic that is not finite or a focal length <= 0:
 *      the pair is invalid, every output zeros and best = -1.
 *   2. Hypothesis h samples 5 distinct indices: the first five draws of step 2 above (ransac_samples5).
 *   3. The five-point solve, fp64: the null space of the 5 x 9 system by Gauss-Jordan with row pivoting on columns
 *      0..4, made orthonormal; E = x X + y Y + z Z + W; the ten cubic constraints det E = 0 and
 *      2 E Eᵀ E - tr(E Eᵀ) E = 0 as a 10 x 20 matrix, eliminated by Gauss-Jordan with row pivoting; the real roots z
 *      of the resulting degree-10 polynomial within its Cauchy bound (brackets from the roots of the successive
 *      derivatives, 36 bisections and 5 bracketed Newton steps each: every loop has a compile-time bound); (x, y)
 *      from the null vector at the root. A pivot of either elimination below 1e-6 or a non-finite value: no
 *      candidate. 0 to 10 candidates.
 *   4. Each candidate is scored in pixels as F = K1⁻ᵀ E K0⁻¹ at unit norm, fp32, with the error and threshold² of
 *      the fundamental matrix. The winner: the highest count, then the lowest hypothesis, then the candidate whose
 *      canonical E has the smallest entry [0, 0].
 *   5. `refits` rounds: with at least 8 inliers, the normalised 8-point least squares of step 5 above on the
 *      Hartley-normalised camera coordinates of the inliers, de-normalised, then the nearest essential matrix
 *      (singular values (1, 1, 0), a one-sided Jacobi SVD). A round whose E counts fewer inliers than the current
 *      one, or is not finite, is dropped and the rounds stop: on a planar scene the 8-point fit is degenerate and
 *      the five-point winner stays.
 *   6. The pose: E = U diag(1, 1, 0) Vᵀ with det U = det V = +1, W the quarter turn about z; of (U W Vᵀ, +u3),
 *      (U W Vᵀ, -u3), (U Wᵀ Vᵀ, +u3), (U Wᵀ Vᵀ, -u3) the one under which the most inliers triangulate (the midpoint
 *      method: the least-squares depths of d0 R a - d1 b = -t for the rays a = (q0, 1), b = (q1, 1)) to a positive
 *      depth in both cameras, the lowest index among equals; num_front is that count.
 *   7. valid = 1 from 5 inliers on. A 5-inlier winner is only its own sample: callers should threshold num_inliers.
 * The non-linear polish of the pose is lg_pose_polish, below. Not built: the choice between the two solutions a
 * plane admits. */
/* Bytes of lg_ransac_essential's workspace (0 for an empty call): a hypothesis' record holds F and E. */
size_t lg_ransac_essential_workspace(int32_t pairs, int32_t kmax, int32_t hypotheses);
/* lg_ransac_essential: two launches, the shapes of lg_ransac_fundamental's (the four lanes of a hypothesis hold five
 * columns of the 10 x 20 matrix each). Parameters as there. Outputs: e, r [pairs, 3, 3], t [pairs, 3] fp32 (e
 * canonical), inliers [pairs, kmax] uint8, num_inliers, num_front, valid, best [pairs] int32. */
int32_t lg_ransac_essential(const int32_t* matches, const int32_t* counts, const float* kpts0, const float* kpts1,
                            const float* intrinsics, int32_t pairs, int32_t kmax, int32_t k0, int32_t k1, float threshold,
                            int32_t hypotheses, int32_t refits, int32_t seed, void* workspace, size_t workspace_bytes, float* e,
                            float* r, float* t, uint8_t* inliers, int32_t* num_inliers, int32_t* num_front, int32_t* valid,
                            int32_t* best, hipStream_t stream);
/* Stage hooks over the same device code (tests). lg_ransac_samples5: step 2 for one count in [5, 2048] ->
 * samples [hypotheses, 5] int32 in draw order. */
int32_t lg_ransac_samples5(int32_t count, int32_t hypotheses, int32_t seed, int32_t* samples, hipStream_t stream);
/* lg_ransac_solve5: step 3 on given samples [hypotheses, 5] int32 (device; clamped into [0, count), shared by the
 * pairs) -> candidates [pairs, hypotheses, 10, 9] fp32, canonical E in camera coordinates (those that exist first,
 * in ascending root, the rest zeros) and num [pairs, hypotheses] int32. An invalid pair: zeros. Step 4 needs no
 * hook: lg_ransac_score takes the F of a candidate. */
int32_t lg_ransac_solve5(const int32_t* matches, const int32_t* counts, const float* kpts0, const float* kpts1,
                         const float* intrinsics, int32_t pairs, int32_t kmax, int32_t k0, int32_t k1, const int32_t* samples,
                         int32_t hypotheses, float* candidates, int32_t* num, hipStream_t stream);
/* lg_pose_from_essential: step 6 for given e [pairs, 3, 3] fp32 (any scale and sign) over the correspondences with
 * inliers [pairs, kmax] uint8 != 0 -> r [pairs, 3, 3], t [pairs, 3] fp32 and num_front [pairs] int32 (zeros where e
 * has no decomposition or an intrinsic is bad). One launch. */
int32_t lg_pose_from_essential(const int32_t* matches, const int32_t* counts, const float* kpts0, const float* kpts1,
                               const float* intrinsics, int32_t pairs, int32_t kmax, int32_t k0, int32_t k1, const float* e,
                               const uint8_t* inliers, float* r, float* t, int32_t* num_front, hipStream_t stream);

/* The pose polish (csrc/lightglue_polish.hip): the (R, t) that lg_ransac_essential returns is the last kept 8-point
 * refit projected to the essential manifold, or the raw five-point winner; neither minimises a geometric error over
 * the inliers. lg_pose_polish does, and lg_triangulate writes the points of the result. New symbols only:
 * LG_GLUE_ABI_VERSION stays 4. The general statements of lg_ransac_fundamental hold (arguments checked before any
 * device call, a no-op for pairs == 0, counts and indices clamped, no atomics, no allocation, no workspace, every output
 * entry written). lightglue_amd/geometry_contract.py restates the contract in float64 by another route (polish_reference:
 * scipy's least squares to convergence in another parameterisation; the converged minimiser is what is compared).
 *
 * Inputs: lg_ransac_essential's pair arguments and intrinsics; r [pairs, 3, 3], t [pairs, 3] fp32; inliers
 * [pairs, kmax] uint8 (non-zero: an inlier) and valid [pairs] int32, as lg_ransac_essential wrote them; threshold;
 * iterations in [1, 16]. The homography has no such call on purpose (its Hartley-normalised DLT refit is at the minimum
 * of the transfer cost to 3e-6 .. 8e-5 relative on the test scenes), and neither has the fundamental matrix
 * (OpenCV polishes neither). Per pair:
 *   1. The fixed set: the rows with inliers != 0 whose residual (step 2) under the entering pose is finite; n_in is the
 *      number of rows with inliers != 0. The pair is passed through (step 5) where valid == 0, an intrinsic is not
 *      finite or a focal length <= 0, the fixed set has fewer than 5 rows, R or t is not finite, or t has zero length.
 *      The entering pose is t at unit length and R one Newton step of the polar iteration nearer the rotations
 *      (R (3 I - Rᵀ R) / 2: a rotation rounded to fp32 is 1e-7 off, the step leaves 1e-14).
 *   2. The residual of a row, fp64, is the signed Sampson distance in pixels: with E = [t]x R, q the camera
 *      coordinates, (a, b, .) = E q0 and (a', b', .) = Eᵀ q1: d = q1ᵀ E q0 and
 *      s = d / sqrt((a / fx1)² + (b / fy1)² + (a' / fx0)² + (b' / fy0)²). The cost is Σ s² over the fixed set, which
 *      does not change during the iterations.
 *   3. `iterations` rounds of Levenberg-Marquardt on the 5 parameters δ = (ω, τ): R <- exp([ω]x) R by the exact
 *      Rodrigues formula, t <- normalise(t + τ1 b1 + τ2 b2) with (b1, b2) an orthonormal basis of t's tangent plane
 *      (b1 = normalise(t x axis), b2 = t x b1, axis the unit axis of t's smallest component in magnitude, the lowest
 *      index among equals). The Jacobian rows are analytic (∂E/∂ω_i = [t]x [e_i]x R, ∂E/∂τ_j = [b_j]x R). A round
 *      solves (JᵀJ + λ diag(JᵀJ)) δ = -Jᵀs by a 5 x 5 Cholesky factorisation in fp64, λ = 1e-3 at first; a pivot that is
 *      not positive or not finite rejects the round. The trial is accepted iff its cost is finite and below the
 *      current cost; then λ <- max(λ / 10, 1e-12), else λ <- min(10 λ, 1e12). Every loop has a compile-time bound but
 *      the rounds', which is the same for every pair; the whole workgroup takes each decision alike, from sums it
 *      reads from one ordered reduction.
 *   4. E <- canonical([t]x R); the mask over all the pair's correspondences as step 4 of the five-point contract
 *      scores (fp32 F = K1⁻ᵀ E K0⁻¹, the fundamental matrix' error, threshold²), n_new its count. If n_new >= n_in:
 *      the polished E, R, t, the new mask, num_inliers = n_new, num_front = the new inliers in front of both cameras
 *      under (R, t) (step 6 there), kept = 1.
 *   5. Else, and for the pairs step 1 names, the pass-through, kept = 0: R and t as given (the same bits), the mask
 *      as given (a non-zero entry written as 1; 0 past the count), E = canonical([t]x R) of the given pose (zeros
 *      where valid == 0 or the pose is not finite), num_inliers = n_in and num_front over the given mask under the
 *      given pose (both zeros where valid == 0; num_front 0 where the intrinsics are bad), both costs equal.
 * Outputs: e, r_out, t_out, inliers_out, num_inliers, num_front as lg_ransac_essential's; cost [pairs, 2] fp32: the
 * entering and the final Σ s² over the fixed set in px² (zeros where the cost was never taken: valid == 0, bad
 * intrinsics, a pose that is not finite); kept [pairs] int32. One launch, one workgroup per pair. The outputs may not
 * alias the inputs. */
int32_t lg_pose_polish(const int32_t* matches, const int32_t* counts, const float* kpts0, const float* kpts1,
                       const float* intrinsics, int32_t pairs, int32_t kmax, int32_t k0, int32_t k1, const float* r, const float* t,
                       const uint8_t* inliers, const int32_t* valid, float threshold, int32_t iterations, float* e_out, float* r_out,
                       float* t_out, uint8_t* inliers_out, int32_t* num_inliers, int32_t* num_front, float* cost, int32_t* kept,
                       hipStream_t stream);
/* lg_triangulate: the 3D point of every inlier under (r, t): points [pairs, kmax, 3] fp32 and ok [pairs, kmax] uint8.
 * For a row below the count with inliers != 0 (and good intrinsics), fp64: the depths (d0, d1) of the midpoint method
 * (step 6 of the five-point contract: the least-squares solution of d0 R a - d1 b = -t for the rays a = (q0, 1),
 * b = (q1, 1)) and X = (d0 a + Rᵀ (d1 b - t)) / 2 in camera 0's frame, at the scale of the given t (|t| = 1 from the
 * calls above). ok = 1 iff both depths are positive and X is finite (in the output's fp32 too); every other entry is
 * zeros. One launch, a flat grid over (rows, pairs). */
int32_t lg_triangulate(const int32_t* matches, const int32_t* counts, const float* kpts0, const float* kpts1,
                       const float* intrinsics, int32_t pairs, int32_t kmax, int32_t k0, int32_t k1, const float* r, const float* t,
                       const uint8_t* inliers, float* points, uint8_t* ok, hipStream_t stream);

/* The absolute pose (csrc/lightglue_absolute.hip): the pose of a camera against 3D points that earlier frames produced,
 * what cv::solvePnPRansac does on the host. lg_ransac_essential gives every pair a frame and a scale (|t| = 1) of its
 * own; localising the next image against the points lg_triangulate wrote gives it a pose in the first pair's frame at
 * the first pair's scale, so a sequence's poses compose (the reference's demo walks a sequence, each frame matched
 * against the previous one: demo/demo_mono.cpp:400-405). New symbols only: LG_GLUE_ABI_VERSION stays 4. The general
 * statements of lg_ransac_fundamental hold for every call below (arguments checked before any device call, a no-op for
 * pairs == 0, counts and indices clamped, never trusted, no allocation, no host synchronisation, every output entry
 * written), with one change to "no atomics": there are no floating-point atomics, and lg_link_landmarks uses an integer
 * atomicMin in LDS, whose result does not depend on the order. lightglue_amd/geometry_contract.py restates the contract
 * in float64 by another route (link_landmarks_reference, absolute_pose_reference).
 *
 * lg_link_landmarks: the 3D points of pair A onto the match rows of pair B, where both pairs share an image. Inputs:
 * matches_a [pairs, kmax_a, 2] and counts_a, points_a [pairs, kmax_a, 3] fp32 and ok_a [pairs, kmax_a] uint8
 * (lg_triangulate's outputs); side_a in {0, 1}: the column of matches_a that indexes the shared image; matches_b
 * [pairs, kmax_b, 2] and counts_b, whose column 0 indexes the shared image and column 1 the new one; kpts_b1
 * [pairs, k_b1, 2] fp32: the new image's keypoints in pixels. 1 <= kmax_a, kmax_b, k_shared <= 2048 (k_shared: the
 * shared image's keypoints), k_b1 >= 1; every pointer but ok_a 4-B aligned. A row r of A below its count with
 * ok_a != 0 owns the shared keypoint matches_a[r, side_a] (clamped into [0, k_shared)); where several rows name one
 * keypoint the lowest row owns it. A row k of B below its count is linked iff its shared keypoint (clamped) has an
 * owner. The linked rows, compacted in ascending k: points [pairs, kmax_b, 3] fp32 (the owner's point, the same bits),
 * image [pairs, kmax_b, 2] fp32 (the new image's keypoint, its index clamped), rows [pairs, kmax_b] int32 (the row of
 * matches_b), n [pairs] int32 (their number); past n points and image are zeros and rows -1. One launch, one workgroup
 * per pair: the owners in LDS, the compaction by a workgroup prefix sum. The outputs may not alias the inputs. */
int32_t lg_link_landmarks(const int32_t* matches_a, const int32_t* counts_a, const float* points_a, const uint8_t* ok_a,
                          int32_t side_a, const int32_t* matches_b, const int32_t* counts_b, const float* kpts_b1, int32_t pairs,
                          int32_t kmax_a, int32_t kmax_b, int32_t k_shared, int32_t k_b1, float* points, float* image,
                          int32_t* rows, int32_t* n, hipStream_t stream);
/* lg_ransac_absolute: the pose from 2D-3D correspondences (a caller with a map of their own needs no
 * lg_link_landmarks). Inputs: points [pairs, kmax, 3] fp32, image [pairs, kmax, 2] fp32 (pixels), counts [pairs] int32
 * (clamped into [0, kmax]), intrinsics [pairs, 4] fp32, (fx, fy, cx, cy) of the one camera. 1 <= kmax <= 2048,
 * pairs <= 65,535, pairs * kmax <= 2^28; every pointer 4-B aligned, the workspace 16-B. Model: X_c = R X + t,
 * det R = +1; t is not normalised: the scale is the map's. The error of a row: with (X_c, Y_c, Z_c) = R X + t,
 * (fx X_c / Z_c + cx - x)² + (fy Y_c / Z_c + cy - y)²; an inlier iff Z_c > 0 and the error <= threshold² (NaN is none).
 * The kernels test dx² + dy² <= threshold² Z_c² with dx = fx X_c + (cx - x) Z_c, dy alike, in fp32. Per pair:
 *   1. Fewer than 4 rows, an intrinsic that is not finite or a focal length <= 0: the pair is invalid, every output
 *      zeros and best = -1.
 *   2. Hypothesis h samples 3 distinct rows: the first three draws of lg_ransac_fundamental's step 2 (ransac_samples3).
 *   3. The P3P solve, fp64 (the route is written out in csrc/lightglue_absolute_math.h). Bearings: the unit vectors
 *      of ((x - cx) / fx, (y - cy) / fy, 1). The quartic in u = s2 / s1 (the ratio of two camera distances; Grunert's),
 *      its real roots in (0, Cauchy bound] by cutting the interval at the real roots of the derivative (a closed-form
 *      cubic), 40 bisections of every piece whose ends differ in sign and 4 bracketed Newton steps; per root the three
 *      camera points and the pose from the two triangles' orthonormal frames. No candidate: anything non-finite, a
 *      sample triangle whose area over its longest side squared is below 1e-6, a distance ratio <= 0, or a candidate
 *      under which one of its own three points has depth <= 0. 0 to 4 candidates, rounded to fp32, in ascending
 *      |R X_s0 + t| (the first sample point's distance from the camera).
 *   4. Each candidate is scored in fp32 over all rows. The winner: the highest count, then the lowest hypothesis, then
 *      the candidates' order.
 *   5. `refits` rounds, each with at least 4 current inliers: Levenberg-Marquardt on the 6 parameters (R <- exp([ω]x) R
 *      by the exact Rodrigues formula, t <- t + δ) over Σ squared reprojection error in px² of the round's fixed set (the
 *      current inliers with a finite residual at a positive depth under the entering pose: the current fp32 pose, R one
 *      Newton step of the polar iteration nearer the rotations; fewer than 3 rows end the rounds), analytic Jacobian,
 *      (JᵀJ + λ diag(JᵀJ)) δ = -Jᵀr by a 6 x 6 Cholesky in fp64, λ and the accept rule lg_pose_polish's, 4 rounds
 *      (kAbsoluteLmRounds), one pass over the rows a round. Then the mask again as in step 4 at the pose rounded to
 *      fp32. A round whose pose counts fewer inliers, or is not finite, is dropped and the rounds stop.
 *   6. valid = 1 from 4 inliers on. A 4-inlier winner is little more than its own sample: threshold num_inliers.
 * Two launches, the shapes of lg_ransac_essential's (the four lanes of a hypothesis take a piece of the quartic's
 * interval each). threshold, hypotheses, refits, seed as there. Outputs: r [pairs, 3, 3], t [pairs, 3] fp32, inliers
 * [pairs, kmax] uint8 (0 past the count), num_inliers, valid, best [pairs] int32. */
size_t lg_ransac_absolute_workspace(int32_t pairs, int32_t kmax, int32_t hypotheses);
int32_t lg_ransac_absolute(const float* points, const float* image, const int32_t* counts, const float* intrinsics,
                           int32_t pairs, int32_t kmax, float threshold, int32_t hypotheses, int32_t refits, int32_t seed,
                           void* workspace, size_t workspace_bytes, float* r, float* t, uint8_t* inliers, int32_t* num_inliers,
                           int32_t* valid, int32_t* best, hipStream_t stream);
/* Stage hooks over the same device code (tests). lg_ransac_samples3: step 2 for one count in [3, 2048] -> samples
 * [hypotheses, 3] int32 in draw order. */
int32_t lg_ransac_samples3(int32_t count, int32_t hypotheses, int32_t seed, int32_t* samples, hipStream_t stream);
/* lg_ransac_solve3: step 3 on given samples [hypotheses, 3] int32 (device; clamped into [0, count), shared by the
 * pairs) -> candidates [pairs, hypotheses, 4, 12] fp32 (R row-major then t; those that exist first, in step 3's order,
 * the rest zeros) and num [pairs, hypotheses] int32. An invalid pair: zeros. */
int32_t lg_ransac_solve3(const float* points, const float* image, const int32_t* counts, const float* intrinsics, int32_t pairs,
                         int32_t kmax, const int32_t* samples, int32_t hypotheses, float* candidates, int32_t* num,
                         hipStream_t stream);
/* lg_ransac_score_absolute: step 4's count for given poses [pairs, num_poses, 12] fp32 (1 <= num_poses <= 4096) ->
 * inlier_counts [pairs, num_poses] int32 (zeros where an intrinsic is bad). */
int32_t lg_ransac_score_absolute(const float* points, const float* image, const int32_t* counts, const float* intrinsics,
                                 int32_t pairs, int32_t kmax, const float* poses, int32_t num_poses, float threshold,
                                 int32_t* inlier_counts, hipStream_t stream);

/* The fp16 forward's inputs (lightglue.py:329-337 and FourierPositionalEncoding :32-52), round 5:
 * x [pairs * (n0 + n1), dim] pair-major from desc0 [pairs, n0, dim] and desc1 [pairs, n1, dim]
 * (dim = 256, 16-B aligned), and the rotary tables cos, sin [pairs * (n0 + n1), 64] from kpts0
 * [pairs, n0, 2], kpts1 [pairs, n1, 2] and Wr [32, 2] (all fp16): proj = Wr · kpt rounded to fp16,
 * cos / sin of it rounded to fp16, each value repeated for the two members of a rotary pair. */
int32_t lg_pair_inputs(const void* desc0, const void* desc1, const void* kpts0, const void* kpts1, const void* wr,
                       int32_t n0, int32_t n1, int32_t pairs, int32_t dim, void* x, void* cosv, void* sinv,
                       hipStream_t stream);

/* Test and benchmark hook: the projections' tile forms for launches of many rows (several image
 * pairs per forward): 0 the 64 x 64 form only; 1 to 5 the 128 x 128 form on 4 waves (two workgroups per
 * CU) where n % 128 == 0, else the 64 x 64 form (the values once named five tile forms; one is left);
 * -1 (the default) chosen by size, the 128 x 128 form from 128 of its tiles and 8,192 rows on. Values
 * outside -1..5 are clamped. The environment variable LG_LINEAR_WIDE sets the initial mode the same
 * way. Both forms give the same bits. Returns the previous mode. */
int32_t lg_linear_set_wide(int32_t mode);

/* Test and benchmark hook for lg_linear_cat_ln_gelu's forms: 1 (the default) one launch from a full
 * round of its tiles on, 0 always two launches, 2 always one launch (A/B). The forms agree within fp16
 * rounding, not in every bit (h rounded once against twice, another summation order). Returns the
 * previous setting. */
int32_t lg_linear_set_ln_fused(int32_t on);
/* Test and benchmark hook for lg_linear_cat_ffn's (and lg_linear_cat_ffn_proj's) forms: 1 (the
 * default) the one-launch form when w_packed is given, its kernel by size (16-row tiles up to 4,096
 * rows, then 32-row up to 8,192, then 64-row); 2 the 32/64-row kernel at every size, 3 the 16-row
 * kernel at every size (A/B); 0 always the two calls (lg_linear_cat_ffn; lg_linear_cat_ffn_proj has
 * only the one-launch form and takes 0 as 1). Values outside 0..3 select 1. Returns the previous
 * setting. */
int32_t lg_linear_set_ffn_fused(int32_t mode);

#ifdef __cplusplus
}
#endif

#endif /* LIGHTGLUE_GLUE_H_ */
