/* pclip.h — C ABI of libpclip.so, the MI355X (gfx950) hot path of Proto-CLIP.
 *
 * The reference (IRVLUTD/Proto-CLIP) is pure Python and has no FFI of its own; each
 * entry point below replaces the eager-PyTorch arithmetic of one reference function, cited as
 * file:line relative to the reference tree.  The host layer (the Python modules under proto-clip_amd/) mirrors the
 * reference's Python signatures and calls these through ctypes (binding shown in INTEGRATION.md).
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller (torch `data_ptr()`); fp16 buffers are
 *    `const void*` (IEEE binary16, row-major, innermost dimension contiguous);
 *  - work is enqueued on the hipStream_t passed as `stream` (void*; NULL = default stream); no entry
 *    point synchronises, allocates or frees; scratch comes from the caller (`ws`, sized by
 *    pclip_workspace_bytes) so every call is hipGraph-capturable and thread-safe per stream;
 *  - return value: 0 = ok, <0 = error (PCLIP_E_*), text via pclip_last_error() (thread-local);
 *  - no torch types, no C++ types, no exceptions cross this boundary.
 */
#ifndef PCLIP_H
#define PCLIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCLIP_ABI_VERSION 1
#define PCLIP_OK 0
#define PCLIP_E_INVALID (-1)   /* bad shape / null pointer / unsupported size */
#define PCLIP_E_LAUNCH (-2)    /* hipLaunch / hipGetLastError failure */
#define PCLIP_E_WORKSPACE (-3) /* workspace too small */

typedef void* pclip_stream_t;

int pclip_abi_version(void);
const char* pclip_last_error(void);
/* number of compute units of the current device (used by host code to size batches) */
int pclip_device_cus(void);
/* Measurement hook of the GEMM kernels (bench.py's roofline): buf = [nslots][2] unsigned 64-bit of device memory, begin words pre-set to ~0 and end words to 0
 * by the caller; every GEMM kernel launch made while the buffer is set takes the next slot and its workgroups fold the device's constant 100 MHz counter
 * (s_memrealtime) into it — slot[0] = first instruction of the launch, slot[1] = its last: the span rocprofv3 reports as the kernel's duration, taken inside the
 * running step without a launch or event between the kernels.  pclip_gemm_timing(NULL, 0) switches it off (the product); pclip_gemm_timing_count() = slots taken. */
int pclip_gemm_timing(void* buf, int nslots);
int pclip_gemm_timing_count(void);
/* cumulative number of GEMM KERNEL launches issued by pclip_gemm_f16 in this process (one call may be split into
 * two launches, see the dispatch in csrc/pclip_encoder.hip); bench.py uses the delta to quote per-launch figures */
long pclip_gemm_kernel_launches(void);

/* ---- memory-bank / prototype reductions -------------------------------------------------- */

/* In-place-capable row L2 normalise: y = r16(x / r16(||x||)).  utils.py:352, main.py:182-185,
 * 408-409.  sq_out (nullable) receives the fp32 squared norm of the *output* row. */
int pclip_l2norm_rows_f16(const void* x, void* y, int R, int D, float* sq_out, pclip_stream_t stream);

/* fp32 squared norms of fp16 rows (the ||.||^2 terms torch.cdist adds, utils.py:230-233). */
int pclip_row_sqnorm_f16(const void* x, int R, int D, float* sq_out, pclip_stream_t stream);

/* Prototype reduction, main.py:399-402 (eval), 260-264 (train), 173-176 (zero-shot init):
 * mem [N*K, D] fp16 (class c owns rows c*K..c*K+K-1) -> proto [N, D].
 *   per_shot_norm=1: zs = r16(m / r16||m||) first (eval/train); 0: skip (zero-shot init).
 *   proto_f16 (nullable): r16(z / r16||z||) with z = r16(mean_K zs)      — eval path
 *   proto_f32 (nullable): fp32 z / ||z||  (no rounding)                     — train path
 *   proto_sq  (nullable): fp32 ||proto_f16||^2 per class. */
int pclip_proto_build_f16(const void* mem, int N, int K, int D, int per_shot_norm, void* proto_f16,
                          float* proto_f32, float* proto_sq, pclip_stream_t stream);

/* Visual-bank reduction, utils.py:318-326: feats [A, R, D] fp16 ->
 * keys[j] = normalise(r16(mean_A feats[:, perm ? perm[j] : j, :])), row-major [R, D] fp16. */
int pclip_bank_reduce_f16(const void* feats, int A, int R, int D, const int32_t* perm, void* keys,
                          pclip_stream_t stream);

/* fp16 matrix transpose x[R,C] -> y[C,R] (bank layout [D, N*K] <-> [N*K, D], utils.py:320). */
int pclip_transpose_f16(const void* x, int R, int C, void* y, pclip_stream_t stream);

/* Multi-GPU shard of the prototype mean: rows of this rank's support slab with
 * NON-DECREASING int32 labels -> fp32 per-class sums of (optionally per-shot normalised) rows and
 * int32 counts.  Classes absent from the slab get zero sums/counts.  Deterministic (no atomics). */
int pclip_partial_sums_f16(const void* mem, const int32_t* labels, int R, int N, int D, int per_shot_norm,
                           float* sums, int32_t* counts, pclip_stream_t stream);

/* Combine W gathered slabs (sums [W,N,D], counts [W,N]) in rank order, then finish as
 * pclip_proto_build_f16 does.  W=1 reproduces the single-GPU result. */
int pclip_proto_finalize(const float* sums, const int32_t* counts, int W, int N, int D, void* proto_f16,
                         float* proto_f32, float* proto_sq, pclip_stream_t stream);

/* ---- classification: utils.py:225-244 `P` ------------------------------------------------ */

/* Squared Euclidean distances against both prototype banks in one pass over the queries:
 * d2x[q, n] = (sqrt(max(||q||^2 + ||z_n||^2 - 2 q.z_n, 0)))^2, fp32, leading dimension ldd >= N.
 * q [Q,D], zi/zt [N,D] fp16; the dot products run on fp16-input / fp32-accumulate MFMA (exact
 * products of the fp16 operands).  q_sq/zi_sq/zt_sq (nullable) are precomputed fp32
 * squared norms; when NULL they are computed into `ws`.  zt may be NULL (single bank). */
int pclip_sqdist_f16(const void* q, const void* zi, const void* zt, int Q, int N, int D,
                     const float* q_sq, const float* zi_sq, const float* zt_sq,
                     float* d2i, float* d2t, int ldd, void* ws, size_t ws_bytes, pclip_stream_t stream);

/* fp32-operand variant for the training path (main.py:262-281: fp32 prototypes and adapted queries): exact
 * fp32 arithmetic on v_mfma_f32_32x32x2_f32; any D; norms computed in the kernel. */
int pclip_sqdist_f32(const float* q, const float* zi, const float* zt, int Q, int N, int D, float* d2i,
                     float* d2t, int ldd, pclip_stream_t stream);

/* p = alpha*softmax(-beta*d2i) + one_minus_alpha*softmax(-beta*d2t) over classes (max-subtracted,
 * fp32).  Outputs (each nullable): p [Q, N] dense; argmax [Q] (lowest index among ties,
 * main.py:190); top-k probabilities/indices [Q, k] sorted descending (toolkit
 * proto_clip_classifier.py:146-147), k <= 16. */
int pclip_fuse_probs(const float* d2i, const float* d2t, int Q, int N, int ldd, float alpha,
                     float one_minus_alpha, float beta, float* p, int32_t* argmax, float* topk_p,
                     int32_t* topk_i, int k, pclip_stream_t stream);

/* Convenience: pclip_sqdist_f16 + pclip_fuse_probs with the distance rows held in `ws` (or one of the one-launch routes, pclip_classify_route).  N <= 4096 on every
 * route (PCLIP_E_INVALID beyond).  Pass ws_bytes = pclip_workspace_bytes(PCLIP_OP_CLASSIFY, Q, N, D) — that size, not a larger buffer's, keeps the route a function of the
 * shape and the flags, the one pclip_classify_route reports (the fused row panels run only if their scratch fits in ws_bytes).  pclip_classify_f16 = flags 0. */
int pclip_classify_f16(const void* q, const void* zi, const void* zt, int Q, int N, int D,
                       const float* q_sq, const float* zi_sq, const float* zt_sq, float alpha,
                       float one_minus_alpha, float beta, float* p, int32_t* argmax, float* topk_p,
                       int32_t* topk_i, int k, void* ws, size_t ws_bytes, pclip_stream_t stream);
int pclip_classify_ex_f16(const void* q, const void* zi, const void* zt, int Q, int N, int D,
                          const float* q_sq, const float* zi_sq, const float* zt_sq, float alpha,
                          float one_minus_alpha, float beta, float* p, int32_t* argmax, float* topk_p,
                          int32_t* topk_i, int k, int flags, void* ws, size_t ws_bytes, pclip_stream_t stream);

/* Routing flags of one classification call (0 = the default routing).  Unknown bits and the contradictory pairs NO_MID | FORCE_MID, NO_PANELS | FORCE_PANELS and
 * PANEL_TWO_PASS | PANEL_FORCE_SECOND are refused (PCLIP_E_INVALID).
 *   NO_SMALL          no one-launch kernel for small class counts
 *   NO_MID            no one-launch kernel for mid-sized class counts; FORCE_MID: it takes every shape it can run (tests), not only 16 < N <= 256 with Q N <= 2e6
 *   NO_PANELS         no fused row panels; FORCE_PANELS: they take every argmax-only shape they can run (tests), not only those with half a 256-query panel per CU
 *   PANEL_TWO_PASS    the row panels walk the class tiles twice always instead of one pass + candidates (pclip_classify_panel_stats)
 *   PANEL_FORCE_SECOND  candidates computed but every panel sent through the second pass (tests)
 *   PANEL_EXACT       the row panels keep torch.cdist's sqrt -> square round trip (bit-identical distances; a third slower)
 * NO_SMALL | NO_MID | NO_PANELS: the two stages, torch.cdist's arithmetic, for every shape. */
#define PCLIP_CLASSIFY_NO_SMALL 0x1
#define PCLIP_CLASSIFY_NO_MID 0x2
#define PCLIP_CLASSIFY_FORCE_MID 0x4
#define PCLIP_CLASSIFY_NO_PANELS 0x8
#define PCLIP_CLASSIFY_FORCE_PANELS 0x10
#define PCLIP_CLASSIFY_PANEL_TWO_PASS 0x20
#define PCLIP_CLASSIFY_PANEL_FORCE_SECOND 0x40
#define PCLIP_CLASSIFY_PANEL_EXACT 0x80

/* The route pclip_classify_ex_f16 takes for a call of this shape and these flags: 0 = two stages (pclip_sqdist_f16 + pclip_fuse_probs), 1 = one launch for
 * small class counts (N <= 16; N <= 32 with top-k), 2 = one launch for 16 < N <= 256, 3 = fused row panels (argmax only, Q N large); PCLIP_E_INVALID for bad flags.
 * The routes agree with the reference's p to 1e-5 and with each other up to fp32 summation order: a query whose top two classes are closer than ~1e-6 in p may get
 * either of them depending on the route, i.e. on the batch it is classified in.  Callers that need one arithmetic for every batch size force the two stages
 * (flags NO_SMALL | NO_MID | NO_PANELS).  ws_bytes: the workspace the call would pass.  pclip_classify_route = flags 0. */
int pclip_classify_route(int Q, int N, int D, float alpha, float one_minus_alpha, float beta, int has_zt, int want_p, int want_argmax, int topk, size_t ws_bytes);
int pclip_classify_route_ex(int Q, int N, int D, float alpha, float one_minus_alpha, float beta, int has_zt, int want_p, int want_argmax, int topk, int flags,
                            size_t ws_bytes);

/* The fused row-panel classification walks the class tiles ONCE where it can prove the result (csrc/pclip_classify_panel.hip: per group of 16 classes the nearest
 * class of each bank is kept as a candidate, everybody else is bounded through the group's second smallest distances; a panel whose rows all satisfy
 * max bound < best candidate is finished from the candidates — the very argmax of the second pass — and only the others walk the tiles again).
 * pclip_classify_panel_stats: out3[0] = panels classified, out3[1] = panels that needed a second pass, out3[2] = class tiles those second passes walked (a second
 * pass covers only the tiles that hold a bound the proof could not beat), since the last reset (host pointer to three ints; synchronises the device). */
int pclip_classify_panel_stats(int* out3, int reset);

/* Test entry of the fused large-N classification (csrc/pclip_classify_panel.hip; pclip_classify_f16 takes that path by itself for N > 32 when only the argmax is
 * asked for): the distances it forms for its first tile — dump [2][256][128] fp32 = d2 of query rows 0..255 x classes 0..127, visual bank then textual bank —
 * with exact != 0 (torch.cdist's sqrt -> square round trip kept, as PCLIP_CLASSIFY_PANEL_EXACT) they must be the bits pclip_sqdist_f16 writes (utils.py:230-233),
 * with exact == 0 (the product's arithmetic: max(v, 0), a third faster) within one fp32 ulp of them.  ws as for pclip_classify_f16. */
int pclip_classify_panel_dump_f16(const void* q, const void* zi, const void* zt, int Q, int N, int D, float* dump, int exact,
                                  void* ws, size_t ws_bytes, pclip_stream_t stream);

/* ---- cosine logits: clip/model.py:356-370 `CLIP.forward`, and the zero-shot line `100. * features @ clip_weights` ---------------- */

/* logits[m, t] = r16( sum_d r16(scale * a'[m, d]) * b'[t, d] ), fp32 accumulation on the matrix pipe (clip/model.py:359-367: both feature matrices
 * normalised, `logit_scale * image_features @ text_features.t()`; main.py's zero-shot baseline on cached features: flags 0, scale 100).
 * a [M, D], b [T, D] fp16 rows lda / ldb >= D halves apart; a' / b' = the rows as given, or L2-normalised with the arithmetic of pclip_l2norm_rows_f16
 * (bit-identical to calling it first) under PCLIP_LOGITS_NORMALIZE_A / _B.  `scale` multiplies in fp32 as passed: the reference casts its 0-dim
 * logit_scale.exp() to fp16 first (its result is r16(r16(s) * x)), so a caller that reproduces it passes the fp16-rounded value.
 * Any M >= 1, T >= 1; D % 64 == 0, D <= 4096; lda, ldb, ldl multiples of 8 halves, 16-byte aligned bases.  Nothing at a column >= D, a row >= M of a or a
 * row >= T of b is read; nothing at a column >= T or a row >= M of logits is written.
 * Outputs, each nullable, at least one: logits [M, ldl >= T] fp16; argmax [M] (lowest index among equal logits); topk_v (fp16) / topk_i [M, k],
 * 1 <= k <= min(16, T), descending, ascending index among equal values (k = 0: both NULL).  argmax / top-k are taken over the ROUNDED fp16 logits — what a
 * reduction of the written matrix gives — and need T <= 4096; with logits == NULL the matrix never reaches memory.
 * A row's logits do not depend on M or the rows that travel with it, a column's not on T (one k order on every route), bit for bit.
 * ws: pclip_workspace_bytes(PCLIP_OP_LOGITS, M, T, D) bytes with PCLIP_LOGITS_NORMALIZE_B (PCLIP_E_WORKSPACE if smaller), unused otherwise.
 * Everything outside this envelope is PCLIP_E_INVALID before any launch. */
int pclip_cosine_logits_f16(const void* a, int lda, int M, const void* b, int ldb, int T, int D, float scale, int flags,
                            void* logits, int ldl, int32_t* argmax, void* topk_v, int32_t* topk_i, int k,
                            void* ws, size_t ws_bytes, pclip_stream_t stream);
#define PCLIP_LOGITS_NORMALIZE_A 0x1
#define PCLIP_LOGITS_NORMALIZE_B 0x2

/* ---- cross-entropy over cosine logits, for training (clip/model.py:356-370 gives the logits; the loss is CLIP's) -------------------- */

/* s[m, t] = scale * cos[m, t], cos = the fp32 matrix-pipe accumulation of a'[m, :] . b'[t, :] (a' / b' as in pclip_cosine_logits_f16 under
 * PCLIP_CE_NORMALIZE_A / _B).  Unlike the inference kernel NOTHING is rounded to fp16 here: neither the scaled operand nor the logit.
 *   labelled (labels [M] int32, or int64 under PCLIP_CE_LABELS_I64):  loss = mean_m ( lse_t s[m, :] - s[m, y_m] )
 *   PCLIP_CE_SYMMETRIC (M == T, labels NULL, targets on the diagonal): loss = 1/2 ( mean_m (lse_t s[m, :] - s[m, m]) + mean_t (lse_m s[:, t] - s[t, t]) )
 * A label is only ever compared with a column index, never used as one: a label outside [0, T) reads nothing; its row's term is lse alone (no target logit)
 * and its gradient the plain softmax.
 * Outputs (fp32, all required but lse_col): lse_row [M], lse_col [T] (symmetric only, NULL otherwise), row_loss [M] (the terms whose mean is the loss; the
 * symmetric one is half the sum of row m's and column m's term), loss [1].  The [M, T] matrix never reaches memory; no floating-point atomics: two calls
 * give the same bits, and in labelled mode a row's lse and loss term do not depend on the rows that travel with it.
 * Any M, T >= 1; D % 64 == 0, D <= 2048; lda, ldb multiples of 8 halves >= D, 16-byte aligned bases; ws: pclip_workspace_bytes(PCLIP_OP_COSINE_CE, M, T, D)
 * (PCLIP_E_WORKSPACE if smaller).  Everything else is PCLIP_E_INVALID before any launch. */
int pclip_cosine_ce_f16(const void* a, int lda, int M, const void* b, int ldb, int T, int D, float scale, int flags, const void* labels,
                        float* lse_row, float* lse_col, float* row_loss, float* loss, void* ws, size_t ws_bytes, pclip_stream_t stream);
/* The gradients of the above (clip/model.py:356-370 has no backward of its own: torch autograd keeps the [M, T] logits and their softmax; this recomputes them
 * tile by tile).  G[m, t] = weight * ( exp(s - lse_row[m]) + [symmetric] exp(s - lse_col[t]) - kappa [t is m's target] ), kappa = 1 labelled, 2 symmetric;
 * weight = 1 / M for the labelled mean, 1 / (2 M) for the symmetric loss (times the upstream gradient, if the caller folds it in).
 *   direction 0: grad [M, D] fp32 (dense) = dL/da = scale G b', chained in fp32 through the normalisation under PCLIP_CE_NORMALIZE_A;
 *   direction 1: grad [T, D] fp32 (dense) = dL/db = scale G^T a', chained under PCLIP_CE_NORMALIZE_B.
 * dscale (nullable, [1] fp32) = sum G o cos, the same value from either direction.  The exp tile is rounded to fp16 (unit 2^-11) for the second matrix
 * product; weight, scale and the target term are applied in fp32.  Deterministic; in labelled mode a row of dL/da does not depend on the other rows of a.
 * Same envelope as the forward; ws: pclip_workspace_bytes(PCLIP_OP_COSINE_CE_BACKWARD, M, T, D). */
int pclip_cosine_ce_backward_f16(const void* a, int lda, int M, const void* b, int ldb, int T, int D, float scale, int flags, const void* labels,
                                 const float* lse_row, const float* lse_col, float weight, int direction, float* grad, float* dscale,
                                 void* ws, size_t ws_bytes, pclip_stream_t stream);
#define PCLIP_CE_NORMALIZE_A 0x1
#define PCLIP_CE_NORMALIZE_B 0x2
#define PCLIP_CE_SYMMETRIC 0x4
#define PCLIP_CE_LABELS_I64 0x8

/* G independent labelled problems of one shape in ONE call (CoCoOp's per-image classifiers, episodes): group g is a_g = a + g * gsa as [M, D] (rows lda
 * apart) against b_g = b + g * gsb as [T, D] (rows ldb apart), fp16, the strides counted in halves; labels [G, M] index the rows of the group's OWN b_g.
 * Outputs (fp32, all required): lse_row [G * M], row_loss [G * M], loss [G] — loss[g] the mean of group g's M terms.
 * A group's numbers are the bits of pclip_cosine_ce_f16 called on that group alone: the group is a grid dimension of the same walk (same tile order, same
 * rounding points), nothing crosses groups, and the number of launches does not depend on G.  No atomics; two calls give the same bits.
 * The envelope of pclip_cosine_ce_f16 per group, and: 1 <= G <= 65535; gsa, gsb multiples of 8 halves (0: the groups share that operand);
 * PCLIP_CE_SYMMETRIC is refused; ws: pclip_cosine_ce_grouped_workspace(0, G, M, T, D) (PCLIP_E_WORKSPACE if smaller).  Everything else is
 * PCLIP_E_INVALID before any launch. */
int pclip_cosine_ce_grouped_f16(const void* a, int lda, size_t gsa, int M, const void* b, int ldb, size_t gsb, int T, int D, int G, float scale, int flags,
                                const void* labels, float* lse_row, float* row_loss, float* loss, void* ws, size_t ws_bytes, pclip_stream_t stream);
/* The gradients of the above, group by group those of pclip_cosine_ce_backward_f16 (labelled) with the one `weight` for every group:
 *   direction 0: grad [G, M, D] fp32 dense = dL_g/da_g;  direction 1: grad [G, T, D] fp32 dense = dL_g/db_g, its walk chunked by the plain call's rule.
 * dscale (nullable, [G] fp32): group g's sum G o cos.  lse_row [G * M] as the forward wrote it.  ws: pclip_cosine_ce_grouped_workspace(1, G, M, T, D). */
int pclip_cosine_ce_grouped_backward_f16(const void* a, int lda, size_t gsa, int M, const void* b, int ldb, size_t gsb, int T, int D, int G, float scale,
                                         int flags, const void* labels, const float* lse_row, float weight, int direction, float* grad, float* dscale,
                                         void* ws, size_t ws_bytes, pclip_stream_t stream);
/* G times pclip_workspace_bytes(PCLIP_OP_COSINE_CE [backward: _BACKWARD], M, T, D): at G = 1 the plain call's size.  0 for G < 1. */
size_t pclip_cosine_ce_grouped_workspace(int backward, int G, int M, int T, int D);

/* ---- distillation: KL from a teacher's cosine logits to the student's (both sets of logits are those of clip/model.py:356-370) -------- */

/* s[m, t] = scale * cos_s[m, t] as in pclip_cosine_ce_f16 on (a [M, D], b [T, D]); z[m, t] = tscale * cos_t[m, t], the same on the teacher's own operands
 * (ta [M, Dt], tb [T, Dt]): its own width Dt, pitches and normalise flags (PCLIP_KD_NORMALIZE_A / _B for a / b, _TA / _TB for ta / tb).  Nothing is rounded
 * to fp16 on the way to s or z.  With p = softmax_t z[m, :] and q = softmax_t s[m, :],
 *   row_loss[m] = sum_t p (z - s) - lse_t z[m, :] + lse_t s[m, :]   ( = KL(p || q) ),   loss = (sum_m row_loss[m]) / M, one fixed-order fp64 sum.
 * No log p is formed: an entry whose p underflows contributes an exact zero.  The value is NOT clamped at zero: a teacher that equals the student gives a
 * row term within a few units of its rounding error of 0, on either side.  A temperature is the caller's: divide both scales by it and multiply the
 * backward's weight by its square.  ta == a (with Dt == D) and tb == b are allowed — the same cached features before two classifiers is the common case.
 * Outputs (fp32, all required): lse_row [M] = lse_t s, tlse_row [M] = lse_t z, row_loss [M], loss [1].  Guarantees:
 *   two calls give the same bits (no floating-point atomics);
 *   a row's lse_row, tlse_row and row_loss depend on that row of a and ta and on b, tb and the scales alone — not on M, the other rows, the panel or the grid;
 *   lse_row has the bits of pclip_cosine_ce_f16's lse_row on (a, b, scale), tlse_row those on (ta, tb, tscale).
 * Any M, T >= 1; D % 64 == 0, D <= 2048, and the same for Dt independently of D; lda, ldb (>= D) and ldta, ldtb (>= Dt) multiples of 8 halves, 16-byte
 * aligned bases; scale and tscale finite; ws: pclip_workspace_bytes(PCLIP_OP_COSINE_KD, M, T, max(D, Dt)) (PCLIP_E_WORKSPACE if smaller).  Everything else
 * is PCLIP_E_INVALID before any launch. */
int pclip_cosine_kd_f16(const void* a, int lda, int M, const void* b, int ldb, int T, int D, float scale, const void* ta, int ldta, const void* tb, int ldtb,
                        int Dt, float tscale, int flags, float* lse_row, float* tlse_row, float* row_loss, float* loss, void* ws, size_t ws_bytes,
                        pclip_stream_t stream);
/* The gradients of the above for the STUDENT (the teacher receives none), recomputed tile by tile from the two lse vectors of the forward:
 *   G[m, t] = weight * ( exp(s - lse_row[m]) - exp(z - tlse_row[m]) ),  weight = 1 / M for the mean (times the upstream gradient and a temperature's square);
 *   direction 0: grad [M, D] fp32 (dense) = dL/da = scale G b', chained in fp32 through the normalisation under PCLIP_KD_NORMALIZE_A;
 *   direction 1: grad [T, D] fp32 (dense) = dL/db = scale G^T a', chained under PCLIP_KD_NORMALIZE_B.
 * dscale (nullable, [1] fp32) = sum G o cos_s, from the unrounded tile.  The signed tile q - p in [-1, 1] enters the second matrix product rounded to fp16
 * as 2^14 (q - p) (unit 2^-11); weight and scale act in fp32.  Deterministic; a row of dL/da depends on that row of a and ta, the class operands, the
 * scales and weight alone.  Same envelope as the forward, direction 0 or 1, grad 16-byte aligned;
 * ws: pclip_workspace_bytes(PCLIP_OP_COSINE_KD_BACKWARD, M, T, max(D, Dt)). */
int pclip_cosine_kd_backward_f16(const void* a, int lda, int M, const void* b, int ldb, int T, int D, float scale, const void* ta, int ldta, const void* tb,
                                 int ldtb, int Dt, float tscale, int flags, const float* lse_row, const float* tlse_row, float weight, int direction,
                                 float* grad, float* dscale, void* ws, size_t ws_bytes, pclip_stream_t stream);
#define PCLIP_KD_NORMALIZE_A 0x1
#define PCLIP_KD_NORMALIZE_B 0x2
#define PCLIP_KD_NORMALIZE_TA 0x4
#define PCLIP_KD_NORMALIZE_TB 0x8

/* ---- feature-level regularisers: a normalised tower output against a constant target ------------------------------------------------- */

/* The distance of n = x / ||x|| (x [M, D] fp16, rows ldx apart, the un-normalised tower output of clip/model.py:338-354; the normalisation is that of
 * clip/model.py:361-362) from a constant t' (t [M, D] fp16, rows ldt apart; t' = t, or t / ||t|| under normalize_t, by the same instruction sequence as n):
 *   PCLIP_FREG_L1:   rows[m] = sum_d |n_md - t'_md|,   loss = sum_m rows[m] / (M D)     torch: F.l1_loss(x / x.norm(dim=-1, keepdim=True), t', reduction="mean")
 *   PCLIP_FREG_COS:  rows[m] = 1 - sum_d n_md t'_md,   loss = sum_m rows[m] / M         torch: 1 - F.cosine_similarity(x, t', dim=-1).mean()
 * n and t' are formed in fp32 from the fp16 rows and NEVER rounded to fp16; every sum has one fixed order (csrc/pclip_feature_reg.hip's header states it and
 * every rounding point).  Outputs, fp32: loss [1], rows [M], inv_norm [M] = 1 / ||x_m||.  No atomics: two calls give the same bits, and a row's term does
 * not depend on M, on the row's position or on the grid.  A row of x with zero norm gives NaN in its own term and in the loss, nowhere else.
 * D % 8 == 0, 8 <= D <= 4096; M >= 0 (M == 0: loss = +0, nothing is launched and rows / inv_norm / x / t are not looked at); ldx, ldt multiples of 8 halves
 * >= D; x and t 16-byte aligned; ws: pclip_feature_reg_workspace(M) bytes, 0 up to PCLIP_FREG_CHUNK rows (PCLIP_E_WORKSPACE if smaller).  Everything else is
 * PCLIP_E_INVALID before any launch. */
int pclip_feature_reg_f16(const void* x, int ldx, const void* t, int ldt, int M, int D, int mode, int normalize_t, float* loss, float* rows, float* inv_norm,
                          void* ws, size_t ws_bytes, pclip_stream_t stream);
/* The gradient of the above with respect to x (t is a constant), what torch's autograd chains through l1_loss / cosine_similarity and the division by the
 * norm: dx [M, D] fp32, dense.  weight = grad / (mean_over D) for L1, grad / mean_over for COS (mean_over = M for the mean above), as
 * pclip_cosine_ce_backward_f16 takes its weight.  dn = weight sgn(n - t') with sgn(0) = 0 (L1), dn = -weight t' (COS); dx = (dn - n (n . dn)) / ||x||, all
 * in fp32.  n and t' are recomputed from x and t by the forward's instruction sequence, so the sign is that of the very difference the forward summed.
 * A row of dx depends on that row of x and t and on weight alone.  Same envelope; dx 16-byte aligned; M == 0 launches nothing. */
int pclip_feature_reg_backward_f16(const void* x, int ldx, const void* t, int ldt, int M, int D, int mode, int normalize_t, float weight, float* dx,
                                   pclip_stream_t stream);
/* Bytes of workspace pclip_feature_reg_f16 needs for M rows: one float per chunk of PCLIP_FREG_CHUNK rows beyond one chunk, else 0. */
size_t pclip_feature_reg_workspace(int M);
#define PCLIP_FREG_L1 0
#define PCLIP_FREG_COS 1
#define PCLIP_FREG_CHUNK 1024

/* ---- the pairwise sigmoid (SigLIP) loss over cosine logits, multi-positive by ids (clip/model.py:356-370 gives the logits) ------------- */

/* x[m, t] = fma(scale, cos[m, t], bias) in fp32, cos = the fp32 matrix-pipe accumulation of a'[m, :] . b'[t, :], one accumulator over k = 0, 32, ... on every
 * route (a' / b' as in pclip_cosine_ce_f16 under PCLIP_SIG_NORMALIZE_A / _B); nothing is rounded to fp16 on the way to x.
 *   loss = 1/M sum_m sum_t softplus(-z[m, t] x[m, t]),  z = +1 on positive pairs, -1 elsewhere.
 * Positives: ids_a [M], ids_b [T], both int32, or both int64 under PCLIP_SIG_IDS_I64 (compared in 64 bits): (m, t) is positive iff ids_a[m] == ids_b[t] and
 * ids_a[m] >= 0.  An id is only ever compared, never used as an index; a negative id matches nothing (rows without a positive, padding).  Both NULL: the
 * diagonal, which needs M == T (the same bits as arange ids on both sides).
 * A term is max(-z x, 0) + log1p(exp(-|x|)) in fp32 (the hardware exp2 / log2 / rcp: the exponential within a relative (|x| + 2) 2^-22, log1p in a compensated
 * form that keeps the term within a relative 2^-20 however small it is); row_loss[m] = sum_t term in fp32:
 * eight waves take every eighth block of 64 columns each, merged in a fixed order — a row's bits depend on that row, b and the ids alone, not on the panel
 * size, the grid or the other rows of a.  loss [1] = (sum_m row_loss[m]) / M, one fixed-order fp64 sum.  Rows >= M and columns >= T contribute exact zeros.
 * Outputs (fp32, both required): row_loss [M], loss [1].  Nothing of size M x T is written; no floating-point atomics: two calls give the same bits.
 * Any M, T >= 1; D % 64 == 0, D <= 2048; lda, ldb multiples of 8 halves >= D, 16-byte aligned bases; scale and bias finite;
 * ws: pclip_workspace_bytes(PCLIP_OP_COSINE_SIGMOID, M, T, D) (PCLIP_E_WORKSPACE if smaller).  Everything else is PCLIP_E_INVALID before any launch. */
int pclip_cosine_sigmoid_f16(const void* a, int lda, int M, const void* b, int ldb, int T, int D, float scale, float bias, int flags,
                             const void* ids_a, const void* ids_b, float* row_loss, float* loss, void* ws, size_t ws_bytes, pclip_stream_t stream);
/* The gradients of the above, recomputed tile by tile (nothing is kept from the forward):  G[m, t] = weight * ( sigma(x[m, t]) - y[m, t] ), y = 1 on positive
 * pairs; weight = 1 / M for the mean (times the upstream gradient, if the caller folds it in), finite.
 *   direction 0: grad [M, D] fp32 (dense) = dL/da = scale G b', chained in fp32 through the normalisation under PCLIP_SIG_NORMALIZE_A;
 *   direction 1: grad [T, D] fp32 (dense) = dL/db = scale G^T a', chained under PCLIP_SIG_NORMALIZE_B.
 * dscale = sum G o cos and dbias = sum G (each nullable, [1] fp32): from the unrounded fp32 sigma, per lane, per-panel partials, one fixed-order fp64 sum; the
 * same value from either direction up to the summation order.  The sigma tile enters the second matrix product rounded to fp16 as 2^14 sigma (relative unit
 * 2^-11 down to sigma = 2^-28, zero below 2^-39); the target tile is exact; weight and scale act in fp32.  Deterministic; a row of dL/da depends on that row,
 * b, the ids and weight alone, not on the other rows of a.
 * Same envelope as the forward, direction 0 or 1, grad 16-byte aligned; ws: pclip_workspace_bytes(PCLIP_OP_COSINE_SIGMOID_BACKWARD, M, T, D). */
int pclip_cosine_sigmoid_backward_f16(const void* a, int lda, int M, const void* b, int ldb, int T, int D, float scale, float bias, int flags,
                                      const void* ids_a, const void* ids_b, float weight, int direction, float* grad, float* dscale, float* dbias,
                                      void* ws, size_t ws_bytes, pclip_stream_t stream);
#define PCLIP_SIG_NORMALIZE_A 0x1
#define PCLIP_SIG_NORMALIZE_B 0x2
#define PCLIP_SIG_IDS_I64 0x8

/* ---- Tip-Adapter's cache logits (Tip-Adapter main.py: run_tip_adapter / search_hp; the baseline the Proto-CLIP tables compare against) ------------- */

/* logit[q, n] = r16( c[q, n] + alpha * S[q, n] ): `100. * features @ clip_weights + alpha * exp(-(beta - beta * features @ cache_keys)) @ cache_values`
 * with the one-hot cache_values given as segments: f [Q, D], keys [NK, D] (rows sorted by class), w [N, D] fp16 rows ldf / ldk / ldw >= D halves apart, all
 * taken as given; seg [N + 1] int32 on the device, class n owns key rows seg[n] .. seg[n + 1] - 1 (ragged, empty classes allowed: S = 0).
 *   aff[q, j] = the fp32 matrix-pipe accumulation of f[q, :] . keys[j, :], one accumulator over k = 0, 32, ... — NOT rounded to fp16;
 *   E[q, j]   = exp(x), x = fma(beta, aff, -beta) in fp32 (the hardware exp2 of x log2 e: relative error within (|x| + 2) 2^-22);
 *   S[q, n]   = ((E[q, seg[n]] + E[q, seg[n] + 1]) + ...) + E[q, seg[n + 1] - 1]: one fp32 accumulator, strictly in ascending j — an association that does not
 *               depend on Q, on the rows that travel with q, on N, on the grid or on any routing choice;
 *   c[q, n]   = what pclip_cosine_logits_f16 (flags 0) accumulates before its final rounding: r16(scale * f) against w, the same k order;
 *   the last step is ONE fma, v = fma(alpha, S, c) rounded to fp32 (the value logits32 receives), and r16(v) is the only fp16 rounding of the result.
 * This is deliberately more exact than the upstream fp16 tensor chain, which rounds the affinity, beta * affinity, the difference, the exp and the class sums
 * (and the product with alpha) to fp16; tests/tip_adapter_ref.py restates that chain as a yardstick (profiles/tip_adapter.txt has both distances to float64).
 * At alpha == 0 the fp16 logits are those of pclip_cosine_logits_f16, bit for bit.
 * Outputs, each nullable, at least one: logits [Q, ldl >= N] fp16; logits32 [Q, N] fp32 (dense), the unrounded fma(alpha, S, c), for the training path;
 * argmax [Q] int32 over the ROUNDED fp16 logits, lowest index among equal logits (the key packing of pclip_cosine_logits_f16).  With only the argmax
 * requested nothing of size Q x N or Q x NK is written.  A row's logits do not depend on Q or on its neighbours, a column's not on N (nor on the key rows
 * of later classes); no floating-point atomics: two calls give the same bits.
 * Envelope: Q >= 1; 1 <= N <= 4096; NK >= 0 (keys may be NULL at NK == 0); D % 64 == 0, D <= 2048; alpha, beta finite and >= 0; ldf, ldk, ldw, ldl multiples
 * of 8 halves, 16-byte aligned bases.  seg must be non-decreasing from 0 to NK: the caller's binding checks that on the host (ops.tip_segments), the kernel
 * does not — whatever seg holds, nothing outside the operands is read or written.  No workspace.  Everything else is PCLIP_E_INVALID before any launch. */
int pclip_tip_logits_f16(const void* f, int ldf, int Q, const void* keys, int ldk, int NK, const int32_t* seg, const void* w, int ldw, int N, int D,
                         float scale, float alpha, float beta, void* logits, int ldl, float* logits32, int32_t* argmax, pclip_stream_t stream);
/* Tip-Adapter's search_hp: correct[ib * na + ia] (int32, beta-major: upstream's loop order) = the number of queries whose fused argmax under
 * (betas[ib], alphas[ia]) equals labels[q] (int32 [Q]; a label outside [0, N) matches nothing) — exactly the counts of nb x na calls of the entry above: the same
 * aff, E, S, c, fma and key arithmetic.  betas [nb], alphas [na] fp32 on the device, 1 <= na <= 32, nb >= 1; their values are the caller's to check (finite, >= 0).
 * The affinity tile is formed once per chunk of 2 betas (measured against 1 and 4: profiles/tip_adapter.txt), not once per pair; nothing of size Q x N or Q x NK is written.  `correct` is cleared and then summed with
 * integer atomics: deterministic.  Same envelope otherwise; no workspace. */
int pclip_tip_grid_f16(const void* f, int ldf, int Q, const void* keys, int ldk, int NK, const int32_t* seg, const void* w, int ldw, int N, int D,
                       float scale, const float* betas, int nb, const float* alphas, int na, const int32_t* labels, int32_t* correct, pclip_stream_t stream);

/* Tip-Adapter-F trains the cache keys only: dkeys[j, :] = alpha beta sum_q dL[q, class(j)] E[q, j] f[q, :]  ([NK, D] fp32, dense) for dL [Q, N] fp32 (dense), the
 * gradient of a loss with respect to the fp32 logits of pclip_tip_logits_f16.  No gradient is produced for f, w, alpha or beta.  E is recomputed tile by tile with
 * the forward's arithmetic (fp32 aff, fma, exp): no [Q, NK] tensor is kept from the forward.  G = dL E is formed in fp32 and enters the second matrix product rounded
 * to fp16 under an exact power-of-two scaling 2^s taken from max |dL| (2^s max |dL| in (2^13, 2^14]: relative unit 2^-11 for |G| >= 2^-27 max |dL|, an absolute
 * 2^-38 max |dL| below; a loss scaled by a power of two moves s with it; E <= 2 is assumed, as normalised features and keys give, so that 2^s G stays inside
 * fp16); the sum over q is fp32 in index order; alpha beta 2^-s multiply in fp32 at the end.
 * Deterministic (no atomics on floating point), and a key row's gradient does not depend on the other key rows or on NK.  Rows of dkeys are written for
 * j < NK only.  Every workgroup walks all Q queries: meant for training batches, not for a 50 000-row split.
 * Envelope of pclip_tip_logits_f16 (Q >= 1, 1 <= N <= 4096, NK >= 0, D % 64 == 0, D <= 2048, alpha, beta finite and >= 0, strides multiples of 8 halves, 16-byte
 * aligned f, keys, dkeys, ws); seg as there (checked by the caller's binding).  ws: pclip_workspace_bytes(PCLIP_OP_TIP_BACKWARD, Q, NK, D) (PCLIP_E_WORKSPACE if
 * smaller).  Everything else is PCLIP_E_INVALID before any launch. */
int pclip_tip_keys_backward_f16(const void* f, int ldf, int Q, const void* keys, int ldk, int NK, const int32_t* seg, int N, int D, float alpha, float beta,
                                const float* dL, float* dkeys, void* ws, size_t ws_bytes, pclip_stream_t stream);

/* (alpha, beta) grid, main.py:142-146, 187-199, 419-430: from the two distance matrices evaluate all
 * na*nb pairs and accumulate correct[ia*nb + ib] += #{q : argmax_n p == labels[q]} (int32, the
 * caller zeroes it; lowest-index tie rule).  Replaces 3*na*nb `P` calls + host syncs. */
int pclip_hp_sweep(const float* d2i, const float* d2t, const int32_t* labels, int Q, int N, int ldd,
                   const float* alphas, const float* one_minus_alphas, int na, const float* betas,
                   int nb, int32_t* correct, pclip_stream_t stream);

/* ---- query adapters: model.py:12-95 ------------------------------------------------------ */

/* Adapter_FC.forward (model.py:81-95): y = r16(r16(ratio*LN_D(W2 LN_{D/r}(W1 x))) + r16((1-ratio)*x)).
 * x [B,D]; w1 [H,D]; g1,b1 [H]; w2 [D,H]; g2,b2 [D]; all fp16.  l2norm_out=1 also applies the
 * following row normalise (main.py:408-409).  y_sq nullable (fp32 ||y||^2).
 * D % 64 == 0, H = D / reduction a multiple of 32 (one k-step of the MFMA, the column count of the GEMM's thinnest tile), both <= 4096. */
int pclip_adapter_fc_f16(const void* x, int B, int D, int H, const void* w1, const void* g1, const void* b1,
                         const void* w2, const void* g2, const void* b2, float ratio, float one_minus_ratio,
                         int l2norm_out, void* y, float* y_sq, void* ws, size_t ws_bytes,
                         pclip_stream_t stream);

/* The last stage of Adapter_FC.forward on its own (model.py:88, 92-95): y = r16(r16(ratio * LN_D(h)) + r16((1-ratio) * x))
 * with fp16 LayerNorm parameters — the training step launches the stages one by one to keep their activations
 * (proto_clip_amd/train.py) and must end with exactly the arithmetic of pclip_adapter_fc_f16.  h, x, y [R, D] fp16. */
int pclip_layernorm_blend_f16(const void* h, const void* gamma, const void* beta, float eps, const void* x, float ratio,
                              float one_minus_ratio, int l2norm_out, void* y, float* y_sq, int R, int D,
                              pclip_stream_t stream);

/* Adapter.forward (model.py:49-78), width 16: pad D -> s*s, conv1 1x1 -> LN[16,s,s] ->
 * (three_x: conv2 3x3 pad 1 -> LN[16,s,s]) -> conv3 1x1 -> LN[1,s,s] -> +identity -> crop.  No ReLU.
 * conv1 [16], ln1w/ln1b [16*s*s], conv2 [16*16*3*3], ln2w/ln2b [16*s*s], conv3 [16], ln3w/ln3b [s*s]. */
int pclip_adapter_conv_f16(const void* x, int B, int D, int three_x, const void* conv1, const void* ln1w,
                           const void* ln1b, const void* conv2, const void* ln2w, const void* ln2b,
                           const void* conv3, const void* ln3w, const void* ln3b, int l2norm_out, void* y,
                           float* y_sq, pclip_stream_t stream);

/* The same at `width` W in {8, 16, 24, 32} (model.py:19 `Adapter(c_in, c_type, width=16)`); any other width is PCLIP_E_INVALID.
 * conv1 [W], ln1w/ln1b [W*s*s], conv2 [W*W*3*3] (layout [co][ci][ky][kx]), ln2w/ln2b [W*s*s], conv3 [W], ln3w/ln3b [s*s], s = ceil(sqrt(D)), D <= 1024.
 * width 16 IS pclip_adapter_conv_f16 (same kernels, same bits); the other widths run conv2 on the matrix pipe with W as a compile-time constant. */
int pclip_adapter_conv_w_f16(const void* x, int B, int D, int three_x, int width, const void* conv1, const void* ln1w,
                             const void* ln1b, const void* conv2, const void* ln2w, const void* ln2b,
                             const void* conv3, const void* ln3w, const void* ln3b, int l2norm_out, void* y,
                             float* y_sq, pclip_stream_t stream);

/* ---- CLIP encoder building blocks: clip/model.py:155-238, 338-354 ------------------------- */

/* C[M,N] = epilogue(A[M,K] . B[N,K]^T): fp16 operands, fp32-accumulate MFMA, fp16 output.
 *   bias (nullable, fp16 [N]) is added before rounding (nn.Linear, clip/model.py:176-178);
 *   act: 0 none, 1 QuickGELU x*sigmoid(1.702x) (clip/model.py:164-166) with per-op fp16 rounding;
 *   residual (nullable, fp16 [M,N], ldc): out = r16(residual + r16(...)) (clip/model.py:188-189).
 * lda/ldb/ldc in elements.  K % 8 == 0 required (K % 64 != 0 runs K-tail instantiations of the same kernels: no element at a column >= K of A or B is read;
 * with N % 8 == 0 they also take N ragged against the tile).  K % 64 == 0 runs the same kernels as before that relaxation.  Calls with no more 128x64 output tiles than the device has CUs (a serving request, the class-token tail) run a latency-oriented kernel with the same arithmetic (bit-identical results). */
int pclip_gemm_f16(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K,
                   const void* bias, int act, const void* residual, pclip_stream_t stream);

/* The same linear on the FOUR-wave 256 x 256 tile with the hand-scheduled (inline-asm) K-loop of csrc/pclip_gemm4w.hip: one wave per
 * SIMD, 128 x 128 accumulators per wave, one barrier per K-tile over a ring of five 32 KB half-tile slots.  Bit-identical to
 * pclip_gemm_f16 (same MFMA, operand roles and k order).  Requires N % 256 == 0, K % 64 == 0, K >= 192, 16-byte aligned rows;
 * a residual needs a bias and act == 0.  PCLIP_E_INVALID otherwise (pclip_gemm_f16 routes its 256 x 256 tiles to it by itself: pclip_gemm4w_config).  Replaces the same call sites as pclip_gemm_f16 (clip/model.py:176-190). */
int pclip_gemm4w_f16(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K,
                     const void* bias, int act, const void* residual, pclip_stream_t stream);
/* ... with the build of the K-loop chosen by the caller: 0 = the product loop, 1 = its RACE-STRESS build (an s_sleep pause of one wave, a different one each
 * time, in front of every counted s_waitcnt and every barrier: a wait that is too weak then reads stale LDS; tests demand bit-identity with variant 0),
 * 6 = ABLATION build that runs the product K-loops and stores NOTHING (timing only: what a fully hidden epilogue would buy), 8 = the product loop in a kernel that
 * keeps time stamps of its tile phases (pclip_gemm4w_stamp_buffer).  6 and 8 exist for epilogues with a bias; without one they run 0.  Any other value is
 * PCLIP_E_INVALID.  Test / tuning entry. */
int pclip_gemm4w_var_f16(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K,
                         const void* bias, int act, const void* residual, int var, pclip_stream_t stream);
/* Test entry: pclip_gemm_f16 / pclip_gemm_bn_f16 / pclip_gemm_bn_res_f16 through the SAME dispatch with everything that routes a call taken from the call instead of
 * the environment, and a report of what ran (tests/test_gpu_gemm_forward.py asserts every route it claims from it).  It launches the product's kernels; no new device code.
 *   act 0 / 1 with bias, residual as pclip_gemm_f16 (scale = shift = NULL); act 2 / 3 = BatchNorm / BatchNorm + ReLU (scale, shift; no bias), act 5 = BatchNorm +
 *     residual + ReLU (the operand checks of the product entries);
 *   cfg (what to run): PCLIP_ROUTE_AUTO = the cost model (and the ring kernel where it applies; no environment switch is read, PCLIP_GEMM_SMALL neither), 0 .. 4 = the persistent kernel on 128 x 128, 256 x 128, 256 x 256, 256 x 64, 256 x 32
 *     tiles (a configuration the shape does not fit falls back to the cost model's, as in the product: read the report), PCLIP_ROUTE_GENERIC, PCLIP_ROUTE_RING
 *     (one workgroup per 128 x 64 tile whatever their number; PCLIP_E_INVALID where the kernel does not apply);
 *   may_split: the row split of a partial last round is allowed (never under a forced cfg);
 *   band / band_n / rev: PCLIP_GEMM_BAND / _BAND_N / _REV of this call (product defaults 0, 0, 2);
 *   use4w: 256 x 256 tiles on 0 the eight-wave kernel, 1 the four-wave kernel, 2 its race-stress build (where pclip_gemm4w_f16 applies);
 *   cus: stands in for the device's CU count in the ring test, the cost model, the row split and the persistent grids (4: a few hundred rows walk several tiles per workgroup);
 *   report (HOST memory, report_len ints): [0] = kernel launches, then PCLIP_ROUTE_FIELDS ints per launch in launch order, as many as fit:
 *     family (what ran: 0 .. 4 persistent cfg, PCLIP_ROUTE_RAN_FOUR_WAVE / _RING / _GENERIC — numbered apart from the cfg values), K-tail / ragged-N instantiation (0 / 1), rows of the
 *     launch, tiles descending (0 / 1), band (column tiles per band, 0 = none). */
#define PCLIP_ROUTE_AUTO (-1)
#define PCLIP_ROUTE_GENERIC 5
#define PCLIP_ROUTE_RING 6
#define PCLIP_ROUTE_FIELDS 5
#define PCLIP_ROUTE_RAN_FOUR_WAVE 10
#define PCLIP_ROUTE_RAN_RING 11
#define PCLIP_ROUTE_RAN_GENERIC 12
int pclip_gemm_route_f16(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K,
                         const void* bias, int act, const void* residual, const float* scale, const float* shift,
                         int cfg, int may_split, int band, int band_n, int rev, int use4w, int cus,
                         int* report, int report_len, pclip_stream_t stream);
/* Diagnostic (loop variant 8 of pclip_gemm4w_var_f16: the product loop in a kernel that keeps time stamps of its tile phases): device buffer of 260 unsigned that the
 * next variant-8 launches fill — stamps [4][64] of (workgroup 0 | gridDim / 2) x (wave 0 | 3), eight s_memrealtime stamps (100 MHz) per tile for the first eight
 * tiles, + one closing stamp per wave at [256 + w].  NULL switches it off.  tools/gemm4w_stamps.py. */
int pclip_gemm4w_stamp_buffer(void* stamps);
/* Routing of pclip_gemm_f16's 256 x 256 tiles: mode 1 = four-wave asm-loop kernel (default; env PCLIP_GEMM_4W), 0 = eight-wave kernel, < 0 = query only.
 * Returns the previous setting (-1 = not decided yet).  Same bits either way. */
int pclip_gemm4w_config(int mode);

/* The same linear for SMALL M (a serving request: M = 197 x batch rows; the class-token tail of the last block: M = batch),
 * where pclip_gemm_f16 has a dozen tiles for 256 CUs and a K-loop of 12 - 48 dependent round trips: the K range is cut into
 * up to 8 slices (a function of K only), one workgroup per (128 x 64 tile, slice) writing an fp32 slab into ws; a second launch
 * adds the slabs in slice order (deterministic) and applies bias / act.  Same arithmetic as pclip_gemm_f16 up to fp32 summation
 * order (no residual operand).
 *   pclip_gemm_splitk_workspace: bytes of `ws` for this shape on the current device, or 0 when the shape gains nothing
 *     (enough tiles, K < 512, N % 64 != 0) — then call pclip_gemm_f16.
 * Replaces the same nn.Linear call sites as pclip_gemm_f16 (clip/model.py:176-190, 236-238) on the serving path
 * (toolkit proto_clip_classifier.py:132-158). */
size_t pclip_gemm_splitk_workspace(int M, int N, int K);
int pclip_gemm_splitk_f16(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K,
                          const void* bias, int act, void* ws, size_t ws_bytes, pclip_stream_t stream);

/* Convolution-as-GEMM with the eval-mode BatchNorm (+ReLU) that follows it in the ModifiedResNet tower (clip/model.py:43-52,
 * 138-142): C = relu?( r16( r16(A B^T) * scale[n] + shift[n] ) ), scale/shift fp32 [N] = the folded running statistics and
 * affine.  Same rounding points as conv (fp16 tensor) followed by pclip_bn_act_f16.  K % 8 == 0 (as pclip_gemm_f16). */
int pclip_gemm_bn_f16(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K,
                      const float* scale, const float* shift, int relu, pclip_stream_t stream);

/* conv3 + bn3 + `out += identity` + ReLU of a bottleneck (clip/model.py:49-52) in one launch:
 * C = relu( r16( r16( r16(A B^T) * scale[n] + shift[n] ) + residual ) ), residual fp16 [M, N] with the row stride ldc of C.
 * Identical to pclip_gemm_f16 followed by pclip_bn_act_f16(residual, relu).  N % 64 == 0, K % 8 == 0, 16-byte aligned operands
 * (PCLIP_E_INVALID otherwise: use the two calls). */
int pclip_gemm_bn_res_f16(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K,
                          const float* scale, const float* shift, const void* residual, pclip_stream_t stream);

/* 3x3 convolution, stride 1, padding 1, on NHWC fp16 activations x [B, H, W, Cin] + eval BatchNorm (+ReLU), as an implicit
 * GEMM: the im2col matrix is never materialised (each K-tile is gathered by buffer LDS-DMA; taps outside the image are out-of-range
 * offsets, i.e. zeros — `zero_line`, >= 128 zero bytes in device memory, is still required non-null for ABI stability but no longer read).  w [Cout, 3, 3, Cin] fp16; y [B*H*W, Cout].
 * Cin % 8 == 0 and Cout % 8 == 0; every row of w is zero-padded to round_up(9 Cin, 64) halves.  Cin outside {8, 16, 32, 64k} or Cout outside
 * {32, 64k} (RN50x4 / RN50x16: 40, 48, 80, 96, 160) run tail instantiations (per-chunk tap gather; columns >= Cout never stored, scale / shift
 * beyond Cout never read).  Identical to pclip_im2col3x3_f16 + pclip_gemm_bn_f16 (clip/model.py:20-22, 45-46) on the 16x16x32 kernels. */
int pclip_conv3x3_bn_f16(const void* x, const void* w, const void* zero_line, int B, int H, int W, int Cin, int Cout,
                         const float* scale, const float* shift, int relu, void* y, pclip_stream_t stream);

/* The narrow layers of the tower (Cin, Cout in {32, 64}; H % 8 == 0, W % 56 == 0: the stem's conv2 / conv3 at 112 x 112, layer1's conv2 at 56 x 56; any batch) are routed by pclip_conv3x3_bn_f16 to a kernel of their own (csrc/pclip_conv_strip.hip: weights in registers, a tile's input block with its halo once
 * in LDS, zero padding by out-of-range buffer loads).  Same rounding points; the fp32 accumulation order differs from the implicit GEMM's ((dx, chunk, dy) instead of
 * (dy, dx, chunk)), so single fp16 results may differ by one ulp.  pclip_conv3x3_strip_applies: would this shape take it (1 / 0); pclip_conv3x3_strip_config: -1 the
 * environment's choice (PCLIP_CONV_STRIP, default on), 0 off, 1 on — returns the previous mode (tests, A/B runs). */
int pclip_conv3x3_strip_applies(int B, int H, int W, int Cin, int Cout);
int pclip_conv3x3_strip_config(int mode);

/* The stem's first convolution (3 -> Cout channels, 3x3, stride 2, pad 1) + eval BatchNorm (+ReLU) straight from the NCHW images `img` [B, 3, R, R] (fp32 if
 * img_is_f32 — rounded to fp16 on the way, as a separate cast would — else fp16) into NHWC fp16 y [B * Ho * Ho, Cout], Ho = (R - 1) / 2 + 1: no im2col matrix, no
 * cast pass (clip/model.py:100-102, 138).  w [Cout][64] fp16: the im2col column order (ky, kx, channel), zero beyond column 27 — the operand pclip_gemm_bn_f16 takes
 * after pclip_im2col3x3_f16, and the same arithmetic.  R even, Ho a multiple of 56, Cout 32 or 64 (pclip_stem_conv_applies; PCLIP_CONV_STEM=0 turns the routing of
 * the python model off); PCLIP_E_INVALID otherwise. */
/* relu(bn(conv3x3(x))) followed by nn.AvgPool2d(2) in one launch (the stem's conv3 / bn3 / relu / avgpool, clip/model.py:104-105, 142-143): y [B * (H / 2) * (W / 2), Cout].
 * The same bits as pclip_conv3x3_bn_f16 + pclip_avgpool_nhwc_f16 without writing and re-reading the unpooled activation.  Cin 32, Cout 64, H % 8 == 0, W % 56 == 0
 * (pclip_conv3x3_pool_applies, which also honours PCLIP_CONV_STRIP / pclip_conv3x3_strip_config); PCLIP_E_INVALID otherwise. */
int pclip_conv3x3_pool_applies(int H, int W, int Cin, int Cout);
int pclip_conv3x3_bn_pool_f16(const void* x, const void* w, int B, int H, int W, int Cin, int Cout, const float* scale, const float* shift, void* y,
                              pclip_stream_t stream);

int pclip_stem_conv_applies(int R, int Cout);
int pclip_stem_conv_bn_f16(const void* img, int img_is_f32, int B, int R, const void* w, int Cout, const float* scale, const float* shift, int relu, void* y,
                           pclip_stream_t stream);

/* LayerNorm over the last dim with fp32 statistics and fp32 affine parameters, fp16 in/out
 * (clip/model.py:155-161).  x rows are ld_x elements apart (lets ln_post read only the CLS rows). */
int pclip_layernorm_f16(const void* x, int ld_x, const float* gamma, const float* beta, float eps, void* y,
                        int R, int D, pclip_stream_t stream);

/* Residual add fused into the following LayerNorm (clip/model.py:188-189 then ln_2 / next ln_1 / ln_post /
 * ln_final): xs = r16(x + delta); x_out (nullable, may alias x; row stride ld) receives xs;
 * y [R, D] = r16(LayerNorm(xs)).  x and delta rows are ld elements apart. */
int pclip_add_layernorm_f16(const void* x, const void* delta, int ld, void* x_out, const float* gamma,
                            const float* beta, float eps, void* y, int R, int D, pclip_stream_t stream);

/* Multi-head self-attention core on a fused QKV buffer (nn.MultiheadAttention inside
 * ResidualAttentionBlock.attention, clip/model.py:183-185): qkv [B, L, 3*H*dh] fp16 (q|k|v blocks,
 * heads contiguous inside each) -> out [B, L, H*dh] fp16 = softmax(q k^T / sqrt(dh) [+causal]) v.
 * dh must be 64; L <= 288 (longer non-causal sequences: pclip_attention_long_q_f16). */
int pclip_attention_f16(const void* qkv, void* out, int B, int L, int H, int dh, int causal,
                        pclip_stream_t stream);

/* The same attention with separate operands: queries = the first Lq tokens of every sequence (q + b*q_batch_stride + row*ldq,
 * head h at column h*64), keys / values in kv [B*L rows, row stride ldkv] at column offsets k_off / v_off; out [B*Lq, H*64].
 * Lq < L serves the last vision block, whose output is only read at the class token (clip/model.py:233); causal needs Lq == L. */
int pclip_attention_q_f16(const void* q, int ldq, long q_batch_stride, const void* kv, int ldkv, int k_off, int v_off, void* out,
                          int B, int L, int Lq, int H, int dh, int causal, pclip_stream_t stream);

/* The same operands and layout as pclip_attention_q_f16 for long NON-causal sequences: 1 <= Lq <= L <= 4096 (ViT-L/14@336px: 577
 * tokens; pclip_attention_q_f16 stops at 288).  K / V are streamed through LDS 128 keys at a time.  For 128 < L <= 288 the result
 * equals pclip_attention_q_f16's bit for bit, and a query row's result does not depend on Lq.  Refuses causal != 0, dh != 64,
 * strides / offsets that are not multiples of 8 halves, and rows that cannot hold H heads at k_off / v_off. */
int pclip_attention_long_q_f16(const void* q, int ldq, long q_batch_stride, const void* kv, int ldkv, int k_off, int v_off, void* out,
                               int B, int L, int Lq, int H, int dh, int causal, pclip_stream_t stream);

/* Kernel choice behind the two attention entry points (same results bit for bit either way): mode -1 / 0 = one workgroup per
 * (image, head) pair (default); 1 = where its shape conditions hold (Lq == L, L <= 256), the persistent kernel that prefetches the
 * next pair's K / V / Q rows by LDS-DMA while the current one is multiplied — built and kept as a measured experiment (faster in
 * isolation, not inside the encoder).  max_grid > 0 caps the persistent grid (test hook: several items per
 * workgroup on small problems).  Process-wide, not thread-safe; PCLIP_ATT_PIPE=0/1 sets the initial mode.  No reference
 * counterpart (nn.MultiheadAttention picks its own kernels, clip/model.py:176-178). */
int pclip_attention_config(int mode, int max_grid);

/* ViT stem (clip/model.py:222-227): patch-conv as an im2col gather of [B,3,R,R] fp16 images into
 * [B*G*G, ld >= 3*P*P] rows, zero beyond 3*P*P (the GEMM against conv1.weight follows), and the token assembly
 * x = [class_emb ; patches] + pos -> fp16 [B, 1+G*G, W]. */
int pclip_im2col_patches_f16(const void* img, int B, int R, int P, void* cols, int ld, pclip_stream_t stream);
/* the same gather from fp32 images, fused with their cast to fp16 (`image.type(self.dtype)`, clip/model.py:339) */
int pclip_im2col_patches_f32(const float* img, int B, int R, int P, void* cols, int ld, pclip_stream_t stream);
int pclip_vit_assemble_tokens_f16(const void* patch_emb, const void* class_emb, const void* pos_emb, int B,
                                  int G2, int W, void* tokens, pclip_stream_t stream);
/* The same assembly fused with ln_pre and the first block's ln_1 (clip/model.py:225-227, 188): x0 = ln_pre(tokens) (the residual
 * stream entering the transformer) and h = ln_1(x0), one pass per token row, bit-identical to the three separate calls.
 * h may be NULL (then gamma_1 / beta_1 are unused): only x0 is produced. */
int pclip_vit_embed_ln_f16(const void* patch_emb, const void* class_emb, const void* pos_emb, int B, int G2, int W,
                           const float* gamma_pre, const float* beta_pre, const float* gamma_1, const float* beta_1, float eps,
                           void* x0, void* h, pclip_stream_t stream);

/* Text stem (clip/model.py:342-344): x = token_embedding[text] + positional_embedding, fp16. */
int pclip_text_embed_f16(const int64_t* tokens, const void* tok_emb, const void* pos_emb, int B, int L, int W,
                         int vocab, void* x, pclip_stream_t stream);
/* Row gather x[b, idx[b], :] (EOT token, clip/model.py:352) ; idx computed by argmax over tokens. */
int pclip_gather_eot_f16(const void* x, const int64_t* tokens, int B, int L, int W, void* out,
                         pclip_stream_t stream);

/* ---- ModifiedResNet tower pieces: clip/model.py:10-152 (activations NHWC fp16) ------------------------ */

/* im2col for a 3x3 / padding 1 / stride 1|2 convolution (clip/model.py:20, 109-113): element (b,y,x,c) of the
 * input sits at x[b*sb + y*sh + x*sw + c*sc] (NHWC activations or the NCHW image);
 * cols[((b*Ho+oy)*Wo+ox)*ld + (ky*3+kx)*C + c], zero outside the image and for columns >= 9*C. */
int pclip_im2col3x3_f16(const void* x, long sb, long sh, long sw, long sc, int B, int H, int W, int C, int stride,
                        void* cols, int ld, pclip_stream_t stream);

/* Eval-mode BatchNorm2d (scale/shift folded from the fp32 statistics) + optional residual add + optional ReLU on
 * [rows, C] fp16: y = relu(r16(r16(x*scale + shift) + residual))  (clip/model.py:43-52). */
int pclip_bn_act_f16(const void* x, const float* scale, const float* shift, const void* residual, int relu, void* y,
                     size_t rows, int C, pclip_stream_t stream);

/* nn.AvgPool2d(k) on NHWC fp16 (clip/model.py:23, 35, 115). */
int pclip_avgpool_nhwc_f16(const void* x, int B, int H, int W, int C, int k, void* y, pclip_stream_t stream);

/* AttentionPool2d token assembly (clip/model.py:68-70): [mean token ; tokens] + positional embedding. */
int pclip_attnpool_tokens_f16(const void* x, const void* pos, int B, int HW, int C, void* tokens, pclip_stream_t stream);

/* fp32 -> fp16 cast (image.type(self.dtype), clip/model.py:339). */
int pclip_cast_f32_f16(const float* x, void* y, size_t n, pclip_stream_t stream);

/* ---- episodic training step (reference main.py:216-310, utils.py:80-109; torch autograd + torch.optim.AdamW there) -------- */

/* fp16 -> fp32 copy (`.float()`, main.py:263, 270, 279). */
int pclip_cast_f16_f32(const void* x, float* y, size_t n, pclip_stream_t stream);

/* C[M,N] (ldc) = alpha * op(A) op(B) + beta * C on v_mfma_f32_32x32x2_f32, element (m,k) of op(A) at A[m*rsa + k*csa], element
 * (k,n) of op(B) at B[k*rsb + n*csb]; a_f16 / b_f16 != 0: that operand is fp16 in memory (exact in fp32).  Serves every
 * matmul autograd issues in the training step: cdist backward (dq = -2 G Z, dz = -2 G^T q), InfoNCE logits and their
 * gradients, Linear weight / input gradients of Adapter_FC. */
int pclip_gemm_f32(const void* A, int a_f16, long rsa, long csa, const void* B, int b_f16, long rsb, long csb, float* C, int ldc,
                   int M, int N, int K, float alpha, float beta, void* ws, size_t ws_bytes, pclip_stream_t stream);
/* ws (nullable): with >= 32 * M * N * 4 bytes, a call with at most 128 output tiles and K >= 1024 is cut into K slices whose
 * partial products are added in slice order (deterministic; differs from the unsplit sum in fp32 order only). */

/* out[c] (+)= scale * sum_r x[r, c]  (fixed summation order; accumulate != 0 adds to out).  ws (nullable, >= 64 * C * 4 bytes):
 * with it, more than 128 rows are summed as up to 64 row blocks in parallel and the block sums added in block order. */
int pclip_colsum_f32(const float* x, int ldx, int R, int C, float scale, float* out, int accumulate, void* ws, size_t ws_bytes,
                     pclip_stream_t stream);

/* C[r, :] += s * rowscale[r] * X[r, :]  (the 2*rowsum(G)*q and 2*colsum(G)*z terms of the cdist backward). */
int pclip_addscaled_rows_f32(float* C, int ldc, const float* X, int ldx, const float* rowscale, float s, int R, int D,
                             pclip_stream_t stream);

/* L = mean_q -log p[q, y_q] with p as in pclip_fuse_probs (utils.py:90-93 `NLLLoss()(torch.log(p), target)`): per-query terms
 * nll[q] = -log p[q,y_q], pmax[q], argmax[q] (utils.py:84-85) and the gradients gi/gt [Q, ldd] of L wrt the two squared-distance
 * rows (columns >= N of gi / gt are left untouched); rowsum[q] = sum_c (gi + gt)[q, c].  q_total >= Q is the number of queries the mean
 * runs over (> Q when the queries of a step are sharded over ranks).  argmax is the LOWEST index among equal maxima.  labels must lie
 * in [0, N): they index the rows and are not checked on the device. */
int pclip_nll_grad(const float* d2i, const float* d2t, const int32_t* labels, int Q, int q_total, int N, int ldd, float alpha,
                   float one_minus_alpha, float beta, float* gi, float* gt, float* rowsum, float* nll, float* pmax,
                   int32_t* argmax, pclip_stream_t stream);

/* Backward of P (utils.py:225-244) for an ARBITRARY upstream gradient dp [Q, N] (leading dimension ldp) — the autograd-
 * transparent `utils.P` the reference's own loop drives (main.py:281-310: NLLLoss(torch.log(p)).backward()): gradients wrt both
 * squared-distance rows (gi, gt [Q, ldd], columns >= N untouched) and rowsum[q] = sum_c (gi + gt)[q, c]. */
int pclip_fuse_probs_backward(const float* d2i, const float* d2t, const float* dp, int ldp, int Q, int N, int ldd, float alpha,
                              float one_minus_alpha, float beta, float* gi, float* gt, float* rowsum, pclip_stream_t stream);

/* Backward of nn.NLLLoss()(torch.log(p), labels) (utils.py:90-93) wrt p: dp[q, c] = -g[0] / (Q p[q, c]) at c == labels[q], else 0;
 * g = upstream gradient of the scalar loss (device pointer). */
int pclip_nll_mean_backward(const float* p, int ldp, const int32_t* labels, int Q, int N, const float* g, float* dp, int lddp,
                            pclip_stream_t stream);

/* The same per-query terms from a materialised p [Q, N] (leading dimension ldp): utils.compute_loss_and_matches as a
 * forward-only drop-in (utils.py:84-93). */
int pclip_nll_rows(const float* p, int ldp, const int32_t* labels, int Q, int N, float* nll, float* pmax, int32_t* argmax,
                   pclip_stream_t stream);

/* Cross entropy of the rows of S [R, C>=R] against the diagonal (InfoNCE of utils.py:72-77 with the info-nce-pytorch
 * defaults): loss[r] = logsumexp(S[r,:]) - S[r,r], dS[r,c] = scale * (softmax(S[r,:])[c] - [c == r]). */
int pclip_softmax_ce_rows(const float* S, int lds, int R, int C, float scale, float* dS, int ldds, float* loss,
                          pclip_stream_t stream);

/* F.normalize(x, dim=-1, eps) on fp32 rows and its backward gx (+)= (gy - y (y.gy)) / max(|x|, eps): InfoNCE normalises
 * both of its arguments (utils.py:72-77). */
int pclip_l2norm_rows_f32(const float* x, float* y, int R, int D, float eps, pclip_stream_t stream);
int pclip_l2norm_rows_backward_f32(const float* x, const float* gy, float* gx, int R, int D, float eps, int accumulate,
                                   pclip_stream_t stream);

/* Backward of the prototype chain (main.py:260-264 image bank; 276-279 text bank with K = 1, final_norm = 0; the query rows
 * `adapter(x).float()` / norm with K = 1, per_shot_norm = 0): g [N, D] fp32 is the gradient wrt the chain's fp32 output, dmem
 * [N*K, D] fp16 the gradient wrt the fp16 rows `mem`; fp16 stages are rounded where autograd materialises fp16 tensors. */
int pclip_proto_backward_f16(const void* mem, const float* g, int N, int K, int D, int per_shot_norm, int final_norm, void* dmem,
                             pclip_stream_t stream);

/* nn.LayerNorm backward on fp16 tensors (model.py:86, 88): dx [R, D]; part [nblk][2][D] fp32 receives the partial
 * (dgamma | dbeta) sums of the rows each of the nblk workgroups visits (reduce with pclip_colsum_f32).  dy_scale: factor applied
 * to dy first, rounded to fp16 (the `ratio * x` of model.py:93-94). */
int pclip_layernorm_backward_f16(const void* x, int ldx, const void* gamma, const void* dy, int lddy, int R, int D, float eps,
                                 float dy_scale, void* dx, int lddx, float* part, int nblk, pclip_stream_t stream);

/* Backward of pclip_adapter_conv_f16 for the training step (reference: autograd through model.py:49-78; the input rows
 * are constants, main.py:266).  x, g [B, D] fp16 (input rows, gradient wrt the adapter output).  Outputs are fp32 PARTIAL sums of the
 * parameter gradients, R rows of them, to be summed over those R rows with pclip_colsum_f32: pw1/pw3 [R,16] (conv1 / conv3),
 * pw2 [R, 16*16*9] (conv2, layout [co][ci][ky][kx]), pg1/pb1, pg2/pb2 [R, 16*s*s], pg3/pb3 [R, s*s] (LayerNorm weight | bias),
 * s = ceil(sqrt(D)).  R = pclip_adapter_conv_backward_partials(B, D, three_x) <= B: conv-3x with D <= 576 runs ONE persistent launch on the
 * matrix pipe whose workgroup w accumulates rows w, w + R, ... (R = min(B, #CU); deterministic: fixed assignment, fixed order); every other
 * case writes one partial per input row (R = B).  conv-2x: conv2 / ln2* / pw2 / pg2 / pb2 are NULL (those parameters receive no gradient). */
int pclip_adapter_conv_backward_partials(int B, int D, int three_x);
int pclip_adapter_conv_backward_f16(const void* x, const void* g, int B, int D, int three_x, const void* conv1, const void* ln1w,
                                    const void* ln1b, const void* conv2, const void* ln2w, const void* ln2b, const void* conv3,
                                    const void* ln3w, float* pw1, float* pw2, float* pw3, float* pg1, float* pb1, float* pg2,
                                    float* pb2, float* pg3, float* pb3, pclip_stream_t stream);

/* The same at `width` W in {8, 16, 24, 32}: pw1/pw3 [R,W], pw2 [R, W*W*9], pg1/pb1, pg2/pb2 [R, W*s*s], pg3/pb3 [R, s*s] with
 * R = pclip_adapter_conv_w_backward_partials(B, D, three_x, width).  Width 16 IS the pair above; every other width writes one partial per
 * input row (R = B) and needs no workspace: the forward is recomputed in LDS at every (W, D <= 1024). */
int pclip_adapter_conv_w_backward_partials(int B, int D, int three_x, int width);
int pclip_adapter_conv_w_backward_f16(const void* x, const void* g, int B, int D, int three_x, int width, const void* conv1,
                                      const void* ln1w, const void* ln1b, const void* conv2, const void* ln2w, const void* ln2b,
                                      const void* conv3, const void* ln3w, float* pw1, float* pw2, float* pw3, float* pg1, float* pb1,
                                      float* pg2, float* pb2, float* pg3, float* pb3, pclip_stream_t stream);

/* ---- backward through the transformer towers (autograd of clip/model.py:171-190; fine-tuning a tail of either tower) ---------- */

/* Gradient of pclip_attention_f16 (nn.MultiheadAttention's core inside ResidualAttentionBlock.attention, clip/model.py:183-185): qkv
 * [B, L, 3*H*64] and dqkv in that layout, dout [B, L, H*64], all fp16.  S and P are recomputed from qkv (the forward saves nothing):
 * dV = P^T dO, dP = dO V^T, dS = P o (dP - rowsum(dO o O)), dQ = dS K / 8, dK = dS^T Q / 8.  Products on MFMA with fp32 accumulation, softmax
 * statistics, dP and the rowsum term in fp32, P and dS rounded to fp16 as they enter their products, every output rounded once (the rounding
 * points are listed in csrc/pclip_attention_bwd.hip).  One workgroup per (sequence, head), no atomics: two calls give the same bits.
 * dh must be 64 and 1 <= L <= 288; dqkv must not alias an input; operands 16-byte aligned. */
int pclip_attention_backward_f16(const void* qkv, const void* dout, void* dqkv, int B, int L, int H, int dh, int causal,
                                 pclip_stream_t stream);

/* QuickGELU backward (clip/model.py:164-166, `x * torch.sigmoid(1.702 * x)`): du = r16(dy * s (1 + t (1 - s))), t = 1.702 u,
 * s = sigmoid(t), in fp32 from the fp16 pre-activation u and the fp16 dy; n elements, 16-byte aligned. */
int pclip_quick_gelu_backward_f16(const void* u, const void* dy, void* du, size_t n, pclip_stream_t stream);

/* Column sums of an fp16 matrix x [R, C] (row stride ldx) in fp32 — the bias gradients of the linears (clip/model.py:176-181: c_fc, c_proj,
 * in_proj, out_proj).  part [nslice][C]: slice i holds the sum of rows [i * ceil(R / nslice), ...) added in row order; reduce with
 * pclip_colsum_f32.  Fixed order: deterministic. */
int pclip_colsum_f16(const void* x, int ldx, int R, int C, float* part, int nslice, pclip_stream_t stream);

/* Backward of CLIP's LayerNorm subclass (clip/model.py:155-161: fp32 computation on fp16 tensors, fp32 weight and bias): x, dy, dx fp16, gamma
 * fp32, statistics fp32.  dx = r16(residual + dLN), `residual` (optional fp16, row stride ldr) being the gradient that reaches x on the residual
 * stream past the LayerNorm (clip/model.py:188-189) — one rounding for the sum.  part [nblk][2][D] fp32: partial (dgamma | dbeta) sums as in
 * pclip_layernorm_backward_f16. */
int pclip_layernorm_backward_g32_f16(const void* x, int ldx, const float* gamma, const void* dy, int lddy, const void* residual, int ldr,
                                     int R, int D, float eps, void* dx, int lddx, float* part, int nblk, pclip_stream_t stream);

/* ---- learned prompt rows (CoOp, VPT, MaPLe): THE SLICE-SUM RULE, stated here once (csrc/pclip_rows.h implements it once) ---------------------------
 * pclip_prompt_ctx_grad_f32, pclip_vpt_grad_f32 and pclip_rows_grad_f32 are one walk: rows off .. off + P - 1 of every sequence of an fp16 stream
 * [B * L, W] (CoOp: off = 1 over the classes; VPT: off = L0 = L - P; MaPLe: any off), summed over the B sequences in fp32 in ONE fixed order —
 * the sequences are cut into slices of 16 consecutive sequences (PCLIP_PROMPT_CTX_SLICE = PCLIP_VPT_SLICE; the last slice may be short); inside a
 * slice, ascending sequence order into one fp32 accumulator per column -> part [nslice][P * W]; then the slices in ascending order into one
 * accumulator -> dctx [P, W]; every sum starts from its first term (no zero is added) and every `+` is one rounded fp32 addition; f32(fp16) is exact
 * and nothing is rounded to fp16.  nslice must be ceil(B / 16); part may be NULL when that is 1 (dctx is then the first stage's output).  No atomics:
 * two calls give the same bits.  clear != 0 (where an entry has it): the same pass writes exact zeros over the rows of g it has read — the lane that
 * loaded a vector stores the zeros over it, after its load; rows outside the window are neither read nor written. */

/* ---- learned prompt context (CoOp: context rows trained through the frozen text tower; csrc/pclip_prompt.hip) ---------------- */

/* The embedded prompts of clip/model.py:342-343 with learned rows in place of the token embeddings at positions 1 .. n_ctx:
 * x [N, L_out, W] fp16, x[n, l] = r16(f32(src) + f32(pos_emb[l])), src = r16(ctx[..][l - 1]) for 1 <= l <= n_ctx and
 * tok_emb[clamp(tokens[n, l], 0, vocab - 1)] elsewhere (pclip_text_embed_f16's clamp; on a context row holding fp16-exact values its bits).
 * ctx fp32: [n_ctx, W] shared by all classes, or with class_specific [N, n_ctx, W].  tokens int64 [N, L_tok], L_out <= L_tok: a truncated
 * assembly reads the full-width token matrix.  pos_emb has at least L_out rows.  W % 8 == 0; operands 16-byte aligned. */
int pclip_prompt_embed_f16(const int64_t* tokens, int L_tok, const void* tok_emb, const void* pos_emb, const float* ctx, int class_specific,
                           int n_ctx, int N, int L_out, int W, int vocab, void* x, pclip_stream_t stream);

/* Gradient of that assembly wrt ctx from dx [N * L_out, W] fp16 (the cast of ctx to fp16 is passed through).  class_specific:
 * dctx [N, n_ctx, W] = f32(dx[n, 1 + j]), exact (the walk with slices of one class); part and nslice are ignored.  Shared: dctx [n_ctx, W] = the
 * sum over the N classes by the slice-sum rule above at off = 1, nslice = ceil(N / PCLIP_PROMPT_CTX_SLICE).  dx is not written.  Context rows at
 * 1 + j >= L_out have no row in dx: they are not read and get a zero gradient. */
#define PCLIP_PROMPT_CTX_SLICE 16
int pclip_prompt_ctx_grad_f32(const void* dx, int N, int L_out, int n_ctx, int W, int class_specific, float* dctx, float* part, int nslice,
                              pclip_stream_t stream);

/* ---- visual prompt tuning (VPT: token rows trained through the frozen vision tower; csrc/pclip_rows.h lists the rounding points) ---------- */

/* A sequence of the vision tower with P learned rows BEHIND its L0 stem rows (class token, patches): L = L0 + P rows, L <= PCLIP_VPT_MAX_L (the
 * attention kernels' resident-K/V envelope).  ctx is fp32 [P, W]; a prompt element enters the fp16 stream rounded once, round to nearest even, with
 * no positional embedding.  All three entries: W % 8 == 0, P >= 1, L0 >= 0, B >= 0 (B == 0 returns PCLIP_OK and touches nothing), B * L * W within
 * an int, operands 16-byte aligned; flat passes of 16-byte vectors, no atomics: two calls give the same bits. */
#define PCLIP_VPT_MAX_L 288
#define PCLIP_VPT_SLICE 16

/* out [B * L, W] fp16 = cat(t.view(B, L0, W), r16(ctx) broadcast over the batch) along the rows of every sequence; t [B * L0, W] fp16 is copied bit
 * for bit (t may be NULL when L0 == 0).  out must not alias t. */
int pclip_vpt_append_f16(const void* t, const float* ctx, int B, int L0, int P, int W, void* out, pclip_stream_t stream);

/* In place on the stream x [B * L, W] fp16: rows L0 .. L - 1 of every sequence become r16(ctx); the other rows are not touched. */
int pclip_vpt_replace_f16(void* x, const float* ctx, int B, int L0, int P, int W, pclip_stream_t stream);

/* dctx [P, W] fp32 = sum over the B sequences of f32(g[b, L0 + j, :]), g [B * L, W] fp16 (L0 == 0: a compact [B * P, W]), by the slice-sum rule
 * above at off = L0, nslice = ceil(B / PCLIP_VPT_SLICE), with its `clear`; rows l < L0 are neither read nor written. */
int pclip_vpt_grad_f32(void* g, int B, int L0, int P, int W, int clear, float* dctx, float* part, int nslice, pclip_stream_t stream);

/* ---- MaPLe: prompt rows at an offset and the text -> vision coupling function (csrc/pclip_small_linear.h and csrc/pclip_maple.hip list the coupling's rounding points and orders) ---- */

/* The two VPT passes above with the P rows at off .. off + P - 1 of sequences of L rows: L, off and P independent, 0 <= off, off + P <= L,
 * L <= PCLIP_VPT_MAX_L, W % 8 == 0, B >= 0, B * L * W within an int, operands 16-byte aligned, no atomics.  At off = L - P they give the bits of
 * pclip_vpt_replace_f16 / pclip_vpt_grad_f32. */

/* In place on the stream x [B * L, W] fp16: rows off .. off + P - 1 of every sequence become r16(ctx), ctx fp32 [P, W]; the other rows are not touched. */
int pclip_rows_replace_f16(void* x, const float* ctx, int B, int L, int off, int P, int W, pclip_stream_t stream);

/* dctx [P, W] fp32 = sum over the B sequences of f32(g[b, off + j, :]) by the slice-sum rule above, nslice = ceil(B / PCLIP_VPT_SLICE), with its
 * `clear`.  Rows outside [off, off + P) are neither read nor written. */
int pclip_rows_grad_f32(void* g, int B, int L, int off, int P, int W, int clear, float* dctx, float* part, int nslice, pclip_stream_t stream);

/* The coupling function, fp32, all depths in one launch: Y[d] = X[d] Wc[d]^T + bc[d], X [depth, P, Wt], Wc [depth, Wv, Wt], bc [depth, Wv],
 * Y [depth, P, Wv].  Envelope: depth >= 1, 1 <= P <= PCLIP_COUPLE_MAX_P, Wt % 64 == 0, Wv % 8 == 0, depth * Wv * Wt within an int, operands 16-byte
 * aligned.  Products and additions are rounded separately (no fused multiply-add) in the one order the source file documents. */
#define PCLIP_COUPLE_MAX_P 16
#define PCLIP_COUPLE_SLICE 32
int pclip_couple_fwd_f32(const float* X, const float* Wc, const float* bc, int depth, int P, int Wt, int Wv, float* Y, pclip_stream_t stream);

/* Gradients of the coupling function from dY [depth, P, Wv]: dWc[d] = dY[d]^T X[d], dbc[d] = sum_p dY[d][p], dX[d] = dY[d] Wc[d]; each output is
 * optional (NULL: not computed; X may be NULL without dWc, Wc without dX).  dX sums the rows of Wc[d] in slices of PCLIP_COUPLE_SLICE rows:
 * nslice = ceil(Wv / PCLIP_COUPLE_SLICE), part [depth][nslice][P * Wt] fp32 (may be NULL when nslice == 1 or dX is NULL).  At most two launches
 * and one merge launch. */
int pclip_couple_bwd_f32(const float* dY, const float* X, const float* Wc, int depth, int P, int Wt, int Wv, float* dWc, float* dbc, float* dX,
                         float* part, int nslice, pclip_stream_t stream);

/* ---- CoCoOp: the image-conditioned context (csrc/pclip_cocoop.hip and csrc/pclip_small_linear.h list every rounding point and summation order) -- */

/* The meta-net, fp32: h[b] = relu(W1 f[b] + b1), pi[b] = W2 h[b] + b2 for f [B, E] fp16 (already normalised; a constant), W1 [Hd, E], b1 [Hd],
 * W2 [Wt, Hd], b2 [Wt]; outputs h [B, Hd] (kept for the backward) and pi [B, Wt], the per-image shift of the context rows.  Envelope:
 * 1 <= B <= PCLIP_COCOOP_MAX_B, E % 64 == 0, Hd % 4 == 0, 4 <= Hd <= 256, Wt % 8 == 0, operands 16-byte aligned.  Products and additions are rounded
 * separately (no fused multiply-add) in the one order the source file documents; the biases are added last.  Two launches. */
#define PCLIP_COCOOP_MAX_B 16
int pclip_metanet_fwd_f32(const void* f, const float* W1, const float* b1, const float* W2, const float* b2, int B, int E, int Hd, int Wt, float* h,
                          float* pi, pclip_stream_t stream);

/* Gradients of the meta-net from dpi [B, Wt]: dW2 = dpi^T h, db2 = sum_b dpi[b], dpre = (dpi W2) masked by h > 0, dW1 = dpre^T f, db1 = sum_b dpre[b];
 * sums over b ascend in one accumulator; f gets no gradient.  Each output is optional (NULL: not computed, nothing launched for it; h may be NULL
 * without dW2 / dW1 / db1, f without dW1, W2 without dW1 / db1).  dpre [B, Hd] fp32 is the workspace dW1 and db1 need (may be NULL without them).
 * The envelope of the forward.  At most three launches. */
int pclip_metanet_bwd_f32(const float* dpi, const void* f, const float* h, const float* W2, int B, int E, int Hd, int Wt, float* dW1, float* db1,
                          float* dW2, float* db2, float* dpre, pclip_stream_t stream);

/* pclip_prompt_embed_f16 with context rows that differ per image and are shared by that image's N classes: x [B * N, L_out, W] fp16,
 * x[b * N + n, l] = r16(f32(src) + f32(pos_emb[l])), src = r16(ctx[l - 1] + pi[b]) for 1 <= l <= n_ctx (one rounded fp32 addition, then the rounding to
 * fp16) and tok_emb[clamp(tokens[n, l], 0, vocab - 1)] elsewhere.  ctx fp32 [n_ctx, W], pi fp32 [B, W], tokens int64 [N, L_tok] shared by the images,
 * L_out <= L_tok.  Envelope: 1 <= B <= PCLIP_COCOOP_MAX_B, N >= 1, n_ctx >= 1, W % 8 == 0, B * N * L_out within an int, operands 16-byte aligned. */
int pclip_prompt_embed_cond_f16(const int64_t* tokens, int L_tok, const void* tok_emb, const void* pos_emb, const float* ctx, const float* pi, int n_ctx,
                                int B, int N, int L_out, int W, int vocab, void* x, pclip_stream_t stream);

/* Gradient of that assembly from dx [B * N * L_out, W] fp16 (read only): dshift [B, n_ctx, W] = the slice-sum rule above at off = 1 applied to the N
 * prompts of every image (nslice = ceil(N / PCLIP_PROMPT_CTX_SLICE); part [B][nslice][n_ctx * W] fp32, may be NULL when nslice == 1), dctx [n_ctx, W] =
 * the sum of dshift over b ascending from b = 0, dpi [B, W] = the sum of dshift over j ascending over the rows that exist (1 + j < L_out; the others
 * are not read and their dshift is +0).  The envelope of the assembly.  Two launches: the grouped partials and one finishing pass. */
int pclip_prompt_cond_grad_f32(const void* dx, int B, int N, int L_out, int n_ctx, int W, float* dshift, float* dctx, float* dpi, float* part, int nslice,
                               pclip_stream_t stream);

/* ---- backward of the embedding stages in front of block 0 (whole-tower fine-tuning; csrc/pclip_embed_bwd.hip lists every rounding) ---------- */

/* Envelope of both entry points: B >= 1, 1 <= L <= 4096, W % 64 == 0, W <= 2048 (and V >= 1); operands 16-byte aligned.  fp32 accumulation, no atomics:
 * two calls give the same bits. */
#define PCLIP_EMBED_BWD_CHUNK 128

/* Backward of the text embedding x = token_embedding(text) + positional_embedding (clip/model.py:342-344) from dx [B * L, W] fp16:
 * dE [V, W] fp32, dense (rows whose id does not occur are exactly zero), and dpos [L, W] fp32 = sum over b, ascending, of dx[b, l].  The caller sorts
 * the B * L flat ids (clamped to [0, V - 1], as pclip_text_embed_f16 clamps them) STABLY: sorted_ids ascending, order[r] = the row of dx at sorted
 * position r.  dE is a segmented reduction over chunks of PCLIP_EMBED_BWD_CHUNK consecutive sorted positions: rows added in ascending sorted position into
 * one fp32 accumulator per column; a run of equal ids inside one chunk is written directly, a run that crosses chunk boundaries leaves one partial per
 * chunk in part [ceil(B * L / CHUNK)][2][W] fp32, and a second pass adds those partials in ascending chunk order.  dE or dpos may be NULL (that
 * gradient is not wanted); sorted_ids, order and part are read only for dE. */
int pclip_text_embed_backward(const void* dx, const int64_t* sorted_ids, const int64_t* order, int B, int L, int W, int V, float* dE, float* dpos,
                              float* part, pclip_stream_t stream);

/* Backward of the vision stem's token assembly x = [class_embedding ; patches] + positional_embedding (clip/model.py:222-227; dt [B, L, W] fp16 is the
 * gradient of the assembled tokens, i.e. what ln_pre's backward returns), one pass over dt: dpos [L, W] fp32 = sum over b, ascending, of dt[b, l] (row 0
 * is also the gradient of class_embedding) and dpatch [B * (L - 1), W] fp16 = the rows dt[b, 1:], contiguous, bit-exact copies (the gradient of the
 * patch convolution's output).  dpos or dpatch may be NULL. */
int pclip_vit_embed_backward_f16(const void* dt, int B, int L, int W, float* dpos, void* dpatch, pclip_stream_t stream);

/* One torch.optim.AdamW step (main.py:134-135: eps 1e-4, weight_decay 0.05) on fp16 parameters with fp16 moments, every
 * intermediate rounded to fp16 where the single-tensor implementation materialises an fp16 tensor; step counts from 1. */
int pclip_adamw_f16(void* p, const void* g, void* m, void* v, size_t n, double lr, double beta1, double beta2, double eps,
                    double weight_decay, int step, pclip_stream_t stream);

/* ---- mixed-precision AdamW for the tower parameters (proto_clip_amd/optim.py: TowerAdamW; csrc/pclip_tower_optim.hip lists every rounding) ---- */
/* fp32 master weights and moments, gradient unscaling with overflow detection, clipping by the global norm and a GradScaler-style dynamic loss
 * scale in three launches for any number of tensors: no host synchronisation, no atomics (deterministic), capturable in a hipGraph.
 *
 * table: ntensors rows of PCLIP_TOWER_ROW_BYTES, eight 64-bit words each:
 *   0 parameter pointer (fp16 or fp32)      1 gradient pointer (fp16 or fp32; NULL = a zero gradient)
 *   2 master weights (fp32; an fp32 parameter is its own master: word 2 == word 0)      3 m (fp32)      4 v (fp32)
 *   5 element count (>= 1)                  6 index of the tensor's first chunk (prefix sum of ceil(n / PCLIP_TOWER_CHUNK), row 0: 0)
 *   7 PCLIP_TOWER_* flags
 * nchunks: the chunks of all tensors.  PCLIP_TOWER_ALIGNED promises that words 0 .. 4 are all 16-byte aligned (16-byte loads and stores);
 * without it every access is a single element.  Both give the same bits.
 * state: PCLIP_TOWER_STATE_BYTES, 8-byte aligned:
 *   +0 double b1^t   +8 double b2^t   (running products, 1.0 before the first step, one multiplication per taken step)
 *   +16 double total (sum of squares of the scaled gradients, this step)
 *   +24 float loss scale   +28 int growth tracker   +32 int steps taken   +36 int found_inf (this step)
 *   +40 float grad_norm (unscaled)   +44 float clip_coef   +48 float inv_scale_used   +52 float bc1   +56 float sqrt(bc2)
 *   +60 float clip_coef * inv_scale_used */
#define PCLIP_TOWER_CHUNK 4096
#define PCLIP_TOWER_ROW_BYTES 64
#define PCLIP_TOWER_STATE_BYTES 64
#define PCLIP_TOWER_PARAM_F16 0x1 /* parameter is fp16 (else fp32) */
#define PCLIP_TOWER_GRAD_F16 0x2  /* gradient is fp16 (else fp32) */
#define PCLIP_TOWER_ALIGNED 0x4
#define PCLIP_TOWER_DECAY 0x8     /* weight decay applies */

/* Launch 1: partials [nchunks] = fp32 sum of squares of each chunk's raw (scaled) gradients in a fixed order; an Inf / NaN gradient makes its
 * partial non-finite. */
int pclip_tower_grad_sumsq(const void* table, int ntensors, int nchunks, float* partials, pclip_stream_t stream);

/* Launch 2 (one workgroup): adds the partials in chunk order in double; writes found_inf, grad_norm = sqrt(total) / scale, clip_coef =
 * min(1, max_norm / (grad_norm + 1e-6)) (1 when max_norm <= 0), inv_scale_used, bc1, sqrt(bc2); advances the step count and b^t on a clean step only;
 * with `dynamic` applies torch.amp.GradScaler's rule (overflow: scale *= backoff, tracker = 0; else tracker += 1 and at growth_interval
 * scale *= growth, tracker = 0). */
int pclip_tower_optim_finish(const float* partials, int nchunks, void* state, float max_norm, double beta1, double beta2, float growth,
                             float backoff, int growth_interval, int dynamic, pclip_stream_t stream);

/* Launch 3: the AdamW update in fp32 from the state block's outputs (nothing when found_inf); hyper [ntensors][2] = {lr, weight_decay} per
 * tensor.  Stores master, m, v and the parameter (half(master) for an fp16 parameter). */
int pclip_tower_adamw(const void* table, const float* hyper, int ntensors, int nchunks, const void* state, double beta1, double beta2,
                      double eps, pclip_stream_t stream);

/* ---- image pre-processing (clip/clip.py:77-84 `_transform`; datasets/imagenet.py:8-23 `get_random_train_tfm`) ------------- */

/* A batch of decoded RGB images (uint8, HWC, device memory; srcs = device array of B pointers) -> normalised CHW tensors
 * out [B, 3, n_px, n_px] (fp32, or fp16 when out_f16: the cast encode_image applies first, clip/model.py:339).  Per image a
 * 16-int32 descriptor (device array desc [B][16]):
 *   0 h, 1 w                  source size
 *   2 box_top, 3 box_left, 4 box_h, 5 box_w   region that is resized (whole image for Resize; the RandomResizedCrop box)
 *   6 rs_h, 7 rs_w            size the box is resized to (PIL bicubic with antialiasing, bit-identical to Image.resize)
 *   8 win_top, 9 win_left     n_px x n_px window of the resized box that is kept (CenterCrop offsets; 0, 0 for the train tfm)
 *   10 flip                   horizontal flip of the window (RandomHorizontalFlip)
 *   11 coef_off               offset (int32 units) of this image's coefficient tables in ws: n_px*(2+ks_h) + n_px*(2+ks_v) ints
 *   12 tmp_off                offset (bytes) of its box_h x n_px x 3 uint8 scratch image in ws
 *   13 ks_h, 14 ks_v          taps per output: ceil(2 * max(box / rs, 1)) * 2 + 1 per axis (1 when box == rs)
 * max_box_h = max over the batch of box_h.  mean / std: Normalize constants. */
int pclip_preprocess_u8(const void* const* srcs, const int32_t* desc, int B, int n_px, int max_box_h, float mean0, float mean1,
                        float mean2, float std0, float std1, float std2, void* out, int out_f16, void* ws, pclip_stream_t stream);

/* ---- workspace sizing -------------------------------------------------------------------- */
/* PCLIP_OP_CLASSIFY: the two-stage distance rows (the least pclip_classify_f16 accepts), or the fused row panels' scratch where that is larger and
 * PCLIP_CLASSIFY_FORCE_PANELS could send the shape there (small Q) — a function of the shape alone. */
#define PCLIP_OP_SQDIST 1
#define PCLIP_OP_CLASSIFY 2
#define PCLIP_OP_ADAPTER_FC 3
#define PCLIP_OP_LOGITS 4 /* Q = M, N = T */
#define PCLIP_OP_COSINE_CE 5          /* Q = M, N = T: normalised rows of b, per-panel column partials, target logits: O(T D + panels T + M) */
#define PCLIP_OP_COSINE_CE_BACKWARD 6 /* Q = M, N = T: the walked operand normalised and transposed, for either direction: O(max(M, T) D) */
#define PCLIP_OP_TIP_BACKWARD 7       /* N = NK, the key rows: the queries transposed, a class per key row, the largest |dL|: O(Q D + NK) */
#define PCLIP_OP_COSINE_SIGMOID 8          /* Q = M, N = T: the normalised rows of b: O(T D) */
#define PCLIP_OP_COSINE_SIGMOID_BACKWARD 9 /* Q = M, N = T: the walked operand normalised and transposed, partial panels of a shared walk, per-panel scalars: O(max(M, T) D + panels) */
#define PCLIP_OP_COSINE_KD 10          /* Q = M, N = T, D = max(D, Dt): both class operands normalised, the cross-entropy forward's own workspace, M labels: O(T D + M) */
#define PCLIP_OP_COSINE_KD_BACKWARD 11 /* Q = M, N = T, D = max(D, Dt): both walked operands normalised, the student's transposed, partial panels of a shared walk: O(max(M, T) D) */
size_t pclip_workspace_bytes(int op, int Q, int N, int D);

#ifdef __cplusplus
}
#endif
#endif /* PCLIP_H */
