// Learned prompt context (CoOp): assembling the embedded prompts [SOT ; ctx ; class name ; EOT ; padding] + positional embedding, and the
// gradient of that assembly with respect to the fp32 context rows (the slice-sum walk of pclip_rows.h).  Memory-bound passes, no atomics: every sum has
// one fixed order.
#include "pclip_rows.h"

namespace {
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
            a = r16_row8(ctx + n * cstride + (size_t)(l - 1) * W + d);
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

// The rounding of ctx to fp16 is passed straight through (as autograd passes a cast), so dctx gathers rows 1 .. n_ctx of dx [N, L_out, W]: the slice-sum
// walk of pclip_rows.h at off = 1 over the classes, with slices of one class for a class-specific context.  A context row at 1 + j >= L_out has no row in
// dx: it is not read and its gradient is +0 (the walk's `avail`).
extern "C" int pclip_prompt_ctx_grad_f32(const void* dx, int N, int L_out, int n_ctx, int W, int class_specific, float* dctx, float* part,
                                         int nslice, pclip_stream_t stream) {
    PCLIP_REQUIRE(dx && dctx, "pclip_prompt_ctx_grad_f32: null pointer");
    PCLIP_REQUIRE(N > 0 && L_out > 0 && n_ctx > 0 && W > 0 && W % 8 == 0, "pclip_prompt_ctx_grad_f32: bad shape N=%d L_out=%d n_ctx=%d W=%d", N, L_out,
                  n_ctx, W);
    PCLIP_REQUIRE((((uintptr_t)dx | (uintptr_t)dctx | (uintptr_t)part) & 15) == 0, "pclip_prompt_ctx_grad_f32: operands must be 16-byte aligned");
    const int avail = n_ctx < L_out - 1 ? n_ctx : L_out - 1;
    void* g = const_cast<void*>(dx);                                   // clear = 0: read only
    if (class_specific)                                                // slices of one class: dctx [N][n_ctx][W] is the first stage's output
        return rows_grad<1>("prompt_ctx_grad (class-specific)", g, N, L_out, 1, n_ctx, avail, W, 0, dctx, N, nullptr, stream);
    const int want = (N + PCLIP_PROMPT_CTX_SLICE - 1) / PCLIP_PROMPT_CTX_SLICE;
    PCLIP_REQUIRE(nslice == want, "pclip_prompt_ctx_grad_f32: nslice=%d, expected ceil(N / %d) = %d", nslice, PCLIP_PROMPT_CTX_SLICE, want);
    PCLIP_REQUIRE(nslice == 1 || part, "pclip_prompt_ctx_grad_f32: %d class slices need the part buffer", nslice);
    return rows_grad<PCLIP_PROMPT_CTX_SLICE>("prompt_ctx_grad", g, N, L_out, 1, n_ctx, avail, W, 0, nslice == 1 ? dctx : part, nslice, dctx, stream);
}
