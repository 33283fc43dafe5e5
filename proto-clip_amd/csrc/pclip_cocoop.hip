// CoCoOp (conditional context optimisation): the meta-net that maps an image feature to a shift of the context rows, the prompt assembly whose context
// rows differ per image but are shared by that image's N classes, and the gradient of that assembly.  No atomics, no hand-over between workgroups: every
// sum has one fixed order and two calls give the same bits.
//
// ---- the meta-net, fp32 -------------------------------------------------------------------------------------------------------------------------------------
// h[b] = relu(W1 f[b] + b1), pi[b] = W2 h[b] + b2:  f [B, E] fp16 (already normalised; a constant), W1 [Hd, E], b1 [Hd], W2 [Wt, Hd], b2 [Wt], h [B, Hd],
// pi [B, Wt].  Envelope: 1 <= B <= PCLIP_COCOOP_MAX_B = 16, E % 64 == 0, Hd % 4 == 0, 4 <= Hd <= 256, Wt % 8 == 0.  W1 and W2 are read once by the forward.
//
// Rounding points / summation order.  f32(fp16) is exact; everything after it is fp32.  A product is rounded on its own (one fp32 multiplication) and then
// added (one rounded fp32 addition): this file is compiled without floating-point contraction, there is no fused multiply-add in it.  Every accumulator
// starts at +0.
//   layer 1 (h), dW2 with db2 and dW1 with db1: the small linear layer of pclip_small_linear.h at depth 1 with the B images as its rows — the forward with
//     X = f (fp16), K = E, R = Hd and the ReLU;  dW2, db2 from dY = dpi, X = h (K = Hd, R = Wt);  dW1, db1 from dY = dpre, X = f (K = E, R = Hd).  The walks
//     are stated there.
//   layer 2, pi[b][t] = (..((0 + h[b][0] W2[t][0]) + h[b][1] W2[t][1]) + ..) + b2[t]      ascending u, one accumulator, the bias added LAST
//     (1 product + Hd additions + 1 bias addition).
//   dh[b][u]  = (..((0 + dpi[b][0] W2[0][u]) + dpi[b][1] W2[1][u]) + ..)                  ascending t, one accumulator  (1 product + Wt additions)
//   dpre[b][u] = dh[b][u] where h[b][u] > 0, else +0  (a hidden unit that is exactly 0 passes no gradient); f is a constant and gets no gradient.
// Launches: forward 2 (layer 1; layer 2); backward at most 3 (dW2 with db2; dpre; dW1 with db1) — nothing is launched for what is not asked for.
//
// ---- the conditional assembly -----------------------------------------------------------------------------------------------------------------------------------
// x [(b N + n), l, :] = r16(f32(src) + f32(pos[l])) for l < L_out, tokens [N, L_tok] shared by the B images, with
//   src = r16(ctx[l - 1][:] + pi[b][:])             for 1 <= l <= n_ctx   (ONE rounded fp32 addition, then the one rounding to fp16 that prompt_embed_kernel
//                                                                          applies to a context row)
//   src = emb[clamp(tokens[n, l], 0, vocab - 1)]    elsewhere             (prompt_embed_kernel's clamp and its one rounding)
// With pi = +0 the bits are pclip_prompt_embed_f16's of the shared context, repeated B times (c + 0 = c in fp32 for every c but -0).
//
// ---- the conditional context gradient ----------------------------------------------------------------------------------------------------------------------------
// From dx [B N L_out, W] fp16; f32(fp16) is exact, every `+` is one rounded fp32 addition, the roundings of the context to fp16 are passed straight through.
//   dshift[b][j][d]: THE SLICE-SUM RULE of pclip_rows.h (SLICE = PCLIP_PROMPT_CTX_SLICE = 16, off = 1, avail = min(n_ctx, L_out - 1)) applied to the N
//     prompts of image b, its first stage launched with one group per image:
//                          part[b][s][j][d] = (..(f32(dx[b N + 16 s, 1 + j, d]) + f32(dx[b N + 16 s + 1, 1 + j, d])) + ..)   ascending class order
//                          dshift[b][j][d]  = (..(part[b][0][j][d] + part[b][1][j][d]) + ..)                                  ascending slice order
//     each sum starts from its first term; one slice (N <= 16): part is dshift itself.  A row j >= avail has no row in dx: it is not read, its dshift is +0.
//   dctx[j][d] = (..(dshift[0][j][d] + dshift[1][j][d]) + ..)        ascending b, starting from b = 0
//   dpi[b][d]  = (..(dshift[b][0][d] + dshift[b][1][d]) + ..)        ascending j over the rows j < avail, starting from j = 0  (+0 when avail == 0)
// Launches: 2 — the grouped partials, and one finishing pass in which the thread of (b, 4 columns) merges that image's slices (dshift, dpi) and the thread of
// (j, 4 columns) merges them again in the same order for every image and adds the images (dctx): no value passes from one thread to another.
#include "pclip_rows.h"

#pragma clang fp contract(off)

#include "pclip_small_linear.h"

namespace {
constexpr int MAXB = PCLIP_COCOOP_MAX_B;

// ---- meta-net ------------------------------------------------------------------------------------------------------------------------------------------------

// layer 2: one thread per row t of W2 walks its Hd columns in ascending order for every image; grid ceil(Wt / 64)
__global__ __launch_bounds__(64) void metanet_l2_kernel(const float* __restrict__ h, const float* __restrict__ W2, const float* __restrict__ b2, int B, int Hd,
                                                        int Wt, float* __restrict__ pi) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= Wt) return;
    const float* w = W2 + (size_t)t * Hd;
    float acc[MAXB];
#pragma unroll
    for (int b = 0; b < MAXB; ++b) acc[b] = 0.f;
    for (int u = 0; u < Hd; u += 4) {
        const float4_t w4 = *reinterpret_cast<const float4_t*>(w + u);
#pragma unroll
        for (int b = 0; b < MAXB; ++b) {
            if (b < B) {
                const float4_t h4 = *reinterpret_cast<const float4_t*>(h + (size_t)b * Hd + u);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float prod = h4[j] * w4[j];
                    acc[b] = acc[b] + prod;
                }
            }
        }
    }
    const float bias = b2[t];
#pragma unroll
    for (int b = 0; b < MAXB; ++b)
        if (b < B) pi[(size_t)b * Wt + t] = acc[b] + bias;
}

// dpre [B, Hd]: one thread per (b, 4 hidden units) walks the Wt rows of W2 in ascending order, then masks by h > 0; flat over B * Hd / 4
__global__ __launch_bounds__(64) void metanet_dpre_kernel(const float* __restrict__ dpi, const float* __restrict__ W2, const float* __restrict__ h, int B, int Hd,
                                                          int Wt, float* __restrict__ dpre) {
    const int H4 = Hd / 4;
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= B * H4) return;
    const int b = i / H4, c = i % H4;
    const float* g = dpi + (size_t)b * Wt;
    const float* w = W2 + 4 * c;
    float4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int t = 0; t < Wt; ++t) {
        const float gt = g[t];
        const float4_t w4 = *reinterpret_cast<const float4_t*>(w + (size_t)t * Hd);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float prod = gt * w4[j];
            acc[j] = acc[j] + prod;
        }
    }
    const float4_t h4 = *reinterpret_cast<const float4_t*>(h + (size_t)b * Hd + 4 * c);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = h4[j] > 0.f ? acc[j] : 0.f;
    *reinterpret_cast<float4_t*>(dpre + (size_t)b * Hd + 4 * c) = acc;
}

int metanet_envelope(const char* who, int B, int E, int Hd, int Wt) {
    PCLIP_REQUIRE(B >= 1 && B <= PCLIP_COCOOP_MAX_B, "%s: B=%d images outside 1 .. %d", who, B, PCLIP_COCOOP_MAX_B);
    PCLIP_REQUIRE(E > 0 && E % 64 == 0, "%s: E=%d must be a positive multiple of 64 (a quarter wave reads 64 columns per step)", who, E);
    PCLIP_REQUIRE(Hd >= 4 && Hd <= 256 && Hd % 4 == 0, "%s: Hd=%d must be a multiple of 4 in 4 .. 256", who, Hd);
    PCLIP_REQUIRE(Wt > 0 && Wt % 8 == 0, "%s: Wt=%d must be a positive multiple of 8", who, Wt);
    PCLIP_REQUIRE((unsigned long long)Hd * (unsigned long long)E <= 2147483647ull && (unsigned long long)Wt * (unsigned long long)Hd <= 2147483647ull,
                  "%s: Hd * E = %d * %d or Wt * Hd = %d * %d does not fit an int", who, Hd, E, Wt, Hd);
    return PCLIP_OK;
}

// ---- conditional assembly ----------------------------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void prompt_embed_cond_kernel(const int64_t* __restrict__ tokens, int L_tok, const half_t* __restrict__ emb,
                                                                const half_t* __restrict__ pos, const float* __restrict__ ctx, const float* __restrict__ pi,
                                                                int n_ctx, int B, int N, int L_out, int W, int vocab, half_t* __restrict__ x) {
    const int WV = W / 8;
    const size_t nvec = (size_t)B * N * L_out * WV;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (size_t)gridDim.x * 256) {
        const int d = (int)(i % WV) * 8;
        const size_t row = i / WV;
        const int l = (int)(row % L_out);
        const size_t bn = row / L_out;
        const int n = (int)(bn % N);
        const size_t b = bn / N;
        half8_t a;
        if (l >= 1 && l <= n_ctx) {
            const float* c = ctx + (size_t)(l - 1) * W + d;
            const float* s = pi + b * W + d;
            const float4_t c0 = reinterpret_cast<const float4_t*>(c)[0], c1 = reinterpret_cast<const float4_t*>(c)[1];
            const float4_t s0 = reinterpret_cast<const float4_t*>(s)[0], s1 = reinterpret_cast<const float4_t*>(s)[1];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float t0 = c0[j] + s0[j], t1 = c1[j] + s1[j];
                a[j] = (half_t)t0;
                a[4 + j] = (half_t)t1;
            }
        } else {
            int64_t tk = tokens[(size_t)n * L_tok + l];
            tk = tk < 0 ? 0 : (tk >= vocab ? vocab - 1 : tk);
            a = ld_half8(emb + (size_t)tk * W + d);
        }
        const half8_t p = ld_half8(pos + (size_t)l * W + d);
        half8_t o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (half_t)((float)a[j] + (float)p[j]);
        st_half8(x + row * W + d, o);
    }
}

// ---- conditional context gradient --------------------------------------------------------------------------------------------------------------------------------

// the merge of one (b, j, 4 columns): (..(part[b][0][j] + part[b][1][j]) + ..), starting from slice 0
__device__ __forceinline__ float4_t cond_merge(const float* __restrict__ part, size_t b, int j, int c, int P, int W, int nslice) {
    const float* src = part + ((b * nslice) * P + j) * W + 4 * c;
    float4_t acc = *reinterpret_cast<const float4_t*>(src);
    for (int s = 1; s < nslice; ++s) {
        src += (size_t)P * W;
        const float4_t v = *reinterpret_cast<const float4_t*>(src);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] += v[k];
    }
    return acc;
}

// the finishing pass, flat over B * W / 4 + P * W / 4 threads: thread (b, c) of the first group writes dshift[b][:][4c ..] (more than one slice) and
// dpi[b][4c ..]; thread (j, c) of the second group writes dctx[j][4c ..].  part is dshift itself when nslice == 1.
__global__ __launch_bounds__(256) void cond_grad_finish_kernel(const float* __restrict__ part, int B, int P, int avail, int W, int nslice,
                                                               float* __restrict__ dshift, float* __restrict__ dctx, float* __restrict__ dpi) {
    const int W4 = W / 4;
    const size_t n_img = (size_t)B * W4, nvec = n_img + (size_t)P * W4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (size_t)gridDim.x * 256) {
        if (i < n_img) {
            const int c = (int)(i % W4);
            const size_t b = i / W4;
            float4_t sum = {0.f, 0.f, 0.f, 0.f};
            for (int j = 0; j < P; ++j) {
                const float4_t v = cond_merge(part, b, j, c, P, W, nslice);
                if (nslice > 1) *reinterpret_cast<float4_t*>(dshift + (b * P + j) * W + 4 * c) = v;
                if (j == 0) {
                    if (avail > 0) sum = v;
                } else if (j < avail) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) sum[k] += v[k];
                }
            }
            *reinterpret_cast<float4_t*>(dpi + b * W + 4 * c) = sum;
        } else {
            const size_t r = i - n_img;
            const int c = (int)(r % W4);
            const int j = (int)(r / W4);
            float4_t sum = cond_merge(part, 0, j, c, P, W, nslice);
            for (int b = 1; b < B; ++b) {
                const float4_t v = cond_merge(part, (size_t)b, j, c, P, W, nslice);
#pragma unroll
                for (int k = 0; k < 4; ++k) sum[k] += v[k];
            }
            *reinterpret_cast<float4_t*>(dctx + (size_t)j * W + 4 * c) = sum;
        }
    }
}

int cond_envelope(const char* who, int B, int N, int L_out, int n_ctx, int W) {
    PCLIP_REQUIRE(B >= 1 && B <= PCLIP_COCOOP_MAX_B, "%s: B=%d images outside 1 .. %d", who, B, PCLIP_COCOOP_MAX_B);
    PCLIP_REQUIRE(N >= 1 && L_out >= 1 && n_ctx >= 1 && W > 0 && W % 8 == 0, "%s: bad shape N=%d L_out=%d n_ctx=%d W=%d", who, N, L_out, n_ctx, W);
    PCLIP_REQUIRE((unsigned long long)B * (unsigned long long)N * (unsigned long long)L_out <= 2147483647ull, "%s: B * N * L_out = %d * %d * %d does not fit an int",
                  who, B, N, L_out);
    return PCLIP_OK;
}
}  // namespace

extern "C" int pclip_metanet_fwd_f32(const void* f, const float* W1, const float* b1, const float* W2, const float* b2, int B, int E, int Hd, int Wt, float* h,
                                     float* pi, pclip_stream_t stream) {
    PCLIP_REQUIRE(f && W1 && b1 && W2 && b2 && h && pi, "pclip_metanet_fwd_f32: null pointer");
    if (int rc = metanet_envelope("pclip_metanet_fwd_f32", B, E, Hd, Wt)) return rc;
    PCLIP_REQUIRE((((uintptr_t)f | (uintptr_t)W1 | (uintptr_t)b1 | (uintptr_t)W2 | (uintptr_t)b2 | (uintptr_t)h | (uintptr_t)pi) & 15) == 0,
                  "pclip_metanet_fwd_f32: operands must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    rowdot16_kernel<half_t, true, false><<<(Hd + 15) / 16, 256, 0, s>>>((const half_t*)f, W1, b1, B, E, Hd, h);
    metanet_l2_kernel<<<(Wt + 63) / 64, 64, 0, s>>>(h, W2, b2, B, Hd, Wt, pi);
    return pclip_check_launch("metanet_fwd");
}

extern "C" int pclip_metanet_bwd_f32(const float* dpi, const void* f, const float* h, const float* W2, int B, int E, int Hd, int Wt, float* dW1, float* db1,
                                     float* dW2, float* db2, float* dpre, pclip_stream_t stream) {
    PCLIP_REQUIRE(dpi, "pclip_metanet_bwd_f32: null pointer (dpi)");
    PCLIP_REQUIRE(!dW2 || h, "pclip_metanet_bwd_f32: dW2 needs h");
    PCLIP_REQUIRE(!(dW1 || db1) || (h && W2 && dpre), "pclip_metanet_bwd_f32: dW1 and db1 need h, W2 and the dpre buffer");
    PCLIP_REQUIRE(!dW1 || f, "pclip_metanet_bwd_f32: dW1 needs f");
    if (int rc = metanet_envelope("pclip_metanet_bwd_f32", B, E, Hd, Wt)) return rc;
    PCLIP_REQUIRE((((uintptr_t)dpi | (uintptr_t)f | (uintptr_t)h | (uintptr_t)W2 | (uintptr_t)dW1 | (uintptr_t)db1 | (uintptr_t)dW2 | (uintptr_t)db2 |
                    (uintptr_t)dpre) & 15) == 0, "pclip_metanet_bwd_f32: operands must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (dW2)
        small_linear_dw_kernel<float><<<flat_grid((size_t)Wt * (Hd / 4)), 256, 0, s>>>(dpi, h, B, Wt, Hd, dW2, db2);
    else if (db2)
        small_linear_db_kernel<><<<flat_grid((size_t)Wt), 256, 0, s>>>(dpi, B, Wt, db2);
    if (dW1 || db1) {
        metanet_dpre_kernel<<<(B * (Hd / 4) + 63) / 64, 64, 0, s>>>(dpi, W2, h, B, Hd, Wt, dpre);
        if (dW1)
            small_linear_dw_kernel<half_t><<<flat_grid((size_t)Hd * (E / 4)), 256, 0, s>>>(dpre, (const half_t*)f, B, Hd, E, dW1, db1);
        else
            small_linear_db_kernel<><<<flat_grid((size_t)Hd), 256, 0, s>>>(dpre, B, Hd, db1);
    }
    return pclip_check_launch("metanet_bwd");
}

extern "C" int pclip_prompt_embed_cond_f16(const int64_t* tokens, int L_tok, const void* tok_emb, const void* pos_emb, const float* ctx, const float* pi,
                                           int n_ctx, int B, int N, int L_out, int W, int vocab, void* x, pclip_stream_t stream) {
    PCLIP_REQUIRE(tokens && tok_emb && pos_emb && ctx && pi && x, "pclip_prompt_embed_cond_f16: null pointer");
    if (int rc = cond_envelope("pclip_prompt_embed_cond_f16", B, N, L_out, n_ctx, W)) return rc;
    PCLIP_REQUIRE(L_tok >= L_out && vocab > 0, "pclip_prompt_embed_cond_f16: bad shape L_out=%d L_tok=%d vocab=%d", L_out, L_tok, vocab);
    PCLIP_REQUIRE((((uintptr_t)ctx | (uintptr_t)pi | (uintptr_t)tok_emb | (uintptr_t)pos_emb | (uintptr_t)x) & 15) == 0,
                  "pclip_prompt_embed_cond_f16: operands must be 16-byte aligned");
    prompt_embed_cond_kernel<<<flat_grid((size_t)B * N * L_out * (W / 8)), 256, 0, (hipStream_t)stream>>>(
        tokens, L_tok, (const half_t*)tok_emb, (const half_t*)pos_emb, ctx, pi, n_ctx, B, N, L_out, W, vocab, (half_t*)x);
    return pclip_check_launch("prompt_embed_cond");
}

extern "C" int pclip_prompt_cond_grad_f32(const void* dx, int B, int N, int L_out, int n_ctx, int W, float* dshift, float* dctx, float* dpi, float* part,
                                          int nslice, pclip_stream_t stream) {
    PCLIP_REQUIRE(dx && dshift && dctx && dpi, "pclip_prompt_cond_grad_f32: null pointer");
    if (int rc = cond_envelope("pclip_prompt_cond_grad_f32", B, N, L_out, n_ctx, W)) return rc;
    PCLIP_REQUIRE((((uintptr_t)dx | (uintptr_t)dshift | (uintptr_t)dctx | (uintptr_t)dpi | (uintptr_t)part) & 15) == 0,
                  "pclip_prompt_cond_grad_f32: operands must be 16-byte aligned");
    const int want = (N + PCLIP_PROMPT_CTX_SLICE - 1) / PCLIP_PROMPT_CTX_SLICE;
    PCLIP_REQUIRE(nslice == want, "pclip_prompt_cond_grad_f32: nslice=%d, expected ceil(N / %d) = %d", nslice, PCLIP_PROMPT_CTX_SLICE, want);
    PCLIP_REQUIRE(nslice == 1 || part, "pclip_prompt_cond_grad_f32: %d class slices need the part buffer", nslice);
    const int avail = n_ctx < L_out - 1 ? n_ctx : L_out - 1;
    float* first = nslice == 1 ? dshift : part;
    hipStream_t s = (hipStream_t)stream;
    // one group per image; clear = 0: dx is only read
    rows_grad_part_kernel<PCLIP_PROMPT_CTX_SLICE, true><<<dim3(flat_grid((size_t)nslice * n_ctx * (W / 8)), B), 256, 0, s>>>(
        (half_t*)const_cast<void*>(dx), N, L_out, 1, n_ctx, avail, W, 0, nslice, first, (size_t)N * L_out * W, (size_t)nslice * n_ctx * W);
    cond_grad_finish_kernel<<<flat_grid((size_t)(B + n_ctx) * (W / 4)), 256, 0, s>>>(first, B, n_ctx, avail, W, nslice, dshift, dctx, dpi);
    return pclip_check_launch("prompt_cond_grad");
}
