// Learned prompt context (CoOp): assembling the embedded prompts [SOT ; ctx ; class name ; EOT ; padding] + positional embedding, and the
// gradient of that assembly with respect to the fp32 context rows.  Two memory-bound passes, no atomics: every sum has one fixed order.
#include "pclip_common.h"

namespace {
inline int flat_grid(size_t n) { size_t g = (n + 255) / 256; return (int)(g < 1 ? 1 : (g > 16384 ? 16384 : g)); }

// ---- assembly ---------------------------------------------------------------------------------------------------------------------------
// x[n, l, :] = r16(f32(src) + f32(pos[l])) for l < L_out, with
//   src = r16(ctx[n * cstride + (l - 1) * W + :])   for 1 <= l <= n_ctx   (the fp32 parameter rounded once, as an fp16 CoOp concatenates fp16 ctx)
//   src = emb[clamp(tokens[n, l], 0, vocab - 1)]    elsewhere             (text_embed_kernel's clamp and its one rounding)
// cstride = 0: one shared context [n_ctx, W]; cstride = n_ctx * W: a context per class [N, n_ctx, W].  tokens has row stride L_tok >= L_out, so a
// truncated assembly reads the 77-wide token matrix in place.  Context rows at l >= L_out do not exist in the output.
__global__ __launch_bounds__(256) void prompt_embed_kernel(const int64_t* __restrict__ tokens, int L_tok, const half_t* __restrict__ emb,
                                                           const half_t* __restrict__ pos, const float* __restrict__ ctx, size_t cstride,
                                                           int n_ctx, int N, int L_out, int W, int vocab, half_t* __restrict__ x) {
    const int WV = W / 8;
    const size_t nvec = (size_t)N * L_out * WV;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (size_t)gridDim.x * 256) {
        const int d = (int)(i % WV) * 8;
        const size_t row = i / WV;
        const int l = (int)(row % L_out);
        const size_t n = row / L_out;
        half8_t a;
        if (l >= 1 && l <= n_ctx) {
            const float4_t* c = reinterpret_cast<const float4_t*>(ctx + n * cstride + (size_t)(l - 1) * W + d);
            const float4_t c0 = c[0], c1 = c[1];
#pragma unroll
            for (int j = 0; j < 4; ++j) { a[j] = (half_t)c0[j]; a[4 + j] = (half_t)c1[j]; }
        } else {
            int64_t tk = tokens[n * L_tok + l];
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

// ---- gradient of the context rows -------------------------------------------------------------------------------------------------------
// The rounding of ctx to fp16 is passed straight through (as autograd passes a cast), so dctx gathers rows 1 .. n_ctx of dx [N, L_out, W].
//
// Class-specific: dctx[n, j, d] = f32(dx[n, 1 + j, d]), exact.
// Shared: the classes are cut into slices of PCLIP_PROMPT_CTX_SLICE consecutive classes (the last one may be short), and
//   part[s][j][d] = (..((f32(dx[n0, 1 + j, d]) + f32(dx[n0 + 1, 1 + j, d])) + f32(dx[n0 + 2, 1 + j, d])) + ..)       n0 = s * SLICE, classes in order
//   dctx[j][d]    = (..((part[0][j][d] + part[1][j][d]) + part[2][j][d]) + ..)                                        slices in order
// in fp32, every `+` one rounded fp32 addition, each sum starting from its first term (no zero is added).  One slice: part is dctx itself.
// The class-specific form is the same first stage with slices of one class.  A context row at 1 + j >= L_out has no row in dx: its gradient is 0.
__global__ __launch_bounds__(256) void prompt_ctx_grad_part_kernel(const half_t* __restrict__ dx, int N, int L_out, int n_ctx, int W, int slice,
                                                                   int nslice, float* __restrict__ part) {
    const int WV = W / 8;
    const size_t nvec = (size_t)nslice * n_ctx * WV;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (size_t)gridDim.x * 256) {
        const int d = (int)(i % WV) * 8;
        const int j = (int)((i / WV) % n_ctx);
        const int s = (int)(i / ((size_t)WV * n_ctx));
        const int n0 = s * slice, n1 = n0 + slice < N ? n0 + slice : N;
        float acc[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] = 0.f;
        if (1 + j < L_out) {
            const half_t* src = dx + ((size_t)n0 * L_out + 1 + j) * W + d;
            half8_t v = ld_half8(src);
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[k] = (float)v[k];
            for (int n = n0 + 1; n < n1; ++n) {
                src += (size_t)L_out * W;
                v = ld_half8(src);
#pragma unroll
                for (int k = 0; k < 8; ++k) acc[k] += (float)v[k];
            }
        }
        float4_t* dst = reinterpret_cast<float4_t*>(part + ((size_t)s * n_ctx + j) * W + d);
        float4_t o0, o1;
#pragma unroll
        for (int k = 0; k < 4; ++k) { o0[k] = acc[k]; o1[k] = acc[4 + k]; }
        dst[0] = o0;
        dst[1] = o1;
    }
}

// out[i] = (..(part[0][i] + part[1][i]) + ..) + part[nslice - 1][i], four elements per thread (M % 4 == 0)
__global__ __launch_bounds__(256) void prompt_ctx_grad_sum_kernel(const float* __restrict__ part, int nslice, size_t M, float* __restrict__ out) {
    const size_t nvec = M / 4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (size_t)gridDim.x * 256) {
        float4_t acc = reinterpret_cast<const float4_t*>(part)[i];
        for (int s = 1; s < nslice; ++s) {
            const float4_t v = reinterpret_cast<const float4_t*>(part + (size_t)s * M)[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] += v[k];
        }
        reinterpret_cast<float4_t*>(out)[i] = acc;
    }
}
}  // namespace

extern "C" int pclip_prompt_embed_f16(const int64_t* tokens, int L_tok, const void* tok_emb, const void* pos_emb, const float* ctx,
                                      int class_specific, int n_ctx, int N, int L_out, int W, int vocab, void* x, pclip_stream_t stream) {
    PCLIP_REQUIRE(tokens && tok_emb && pos_emb && x && (ctx || n_ctx == 0), "pclip_prompt_embed_f16: null pointer");
    PCLIP_REQUIRE(N >= 0 && L_out > 0 && L_tok >= L_out && W > 0 && W % 8 == 0 && vocab > 0 && n_ctx >= 0,
                  "pclip_prompt_embed_f16: bad shape N=%d L_out=%d L_tok=%d W=%d vocab=%d n_ctx=%d", N, L_out, L_tok, W, vocab, n_ctx);
    PCLIP_REQUIRE((((uintptr_t)ctx | (uintptr_t)tok_emb | (uintptr_t)pos_emb | (uintptr_t)x) & 15) == 0, "pclip_prompt_embed_f16: operands must be 16-byte aligned");
    if (N == 0) return PCLIP_OK;
    prompt_embed_kernel<<<flat_grid((size_t)N * L_out * (W / 8)), 256, 0, (hipStream_t)stream>>>(
        tokens, L_tok, (const half_t*)tok_emb, (const half_t*)pos_emb, ctx, class_specific ? (size_t)n_ctx * W : 0, n_ctx, N, L_out, W, vocab, (half_t*)x);
    return pclip_check_launch("prompt_embed");
}

extern "C" int pclip_prompt_ctx_grad_f32(const void* dx, int N, int L_out, int n_ctx, int W, int class_specific, float* dctx, float* part,
                                         int nslice, pclip_stream_t stream) {
    PCLIP_REQUIRE(dx && dctx, "pclip_prompt_ctx_grad_f32: null pointer");
    PCLIP_REQUIRE(N > 0 && L_out > 0 && n_ctx > 0 && W > 0 && W % 8 == 0, "pclip_prompt_ctx_grad_f32: bad shape N=%d L_out=%d n_ctx=%d W=%d", N, L_out,
                  n_ctx, W);
    PCLIP_REQUIRE((((uintptr_t)dx | (uintptr_t)dctx | (uintptr_t)part) & 15) == 0, "pclip_prompt_ctx_grad_f32: operands must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (class_specific) {                                              // slices of one class: dctx [N][n_ctx][W] is the first stage's output
        prompt_ctx_grad_part_kernel<<<flat_grid((size_t)N * n_ctx * (W / 8)), 256, 0, s>>>((const half_t*)dx, N, L_out, n_ctx, W, 1, N, dctx);
        return pclip_check_launch("prompt_ctx_grad (class-specific)");
    }
    const int want = (N + PCLIP_PROMPT_CTX_SLICE - 1) / PCLIP_PROMPT_CTX_SLICE;
    PCLIP_REQUIRE(nslice == want, "pclip_prompt_ctx_grad_f32: nslice=%d, expected ceil(N / %d) = %d", nslice, PCLIP_PROMPT_CTX_SLICE, want);
    PCLIP_REQUIRE(nslice == 1 || part, "pclip_prompt_ctx_grad_f32: %d class slices need the part buffer", nslice);
    float* first = nslice == 1 ? dctx : part;
    prompt_ctx_grad_part_kernel<<<flat_grid((size_t)nslice * n_ctx * (W / 8)), 256, 0, s>>>((const half_t*)dx, N, L_out, n_ctx, W, PCLIP_PROMPT_CTX_SLICE,
                                                                                          nslice, first);
    if (nslice > 1) prompt_ctx_grad_sum_kernel<<<flat_grid((size_t)n_ctx * W / 4), 256, 0, s>>>(part, nslice, (size_t)n_ctx * W, dctx);
    return pclip_check_launch("prompt_ctx_grad");
}
