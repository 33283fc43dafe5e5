// Visual prompt tuning (VPT): learned fp32 token rows spliced into the vision tower's sequence BEHIND the patch rows (the class token stays row 0, the
// patch rows stay where the stem writes them), and the gradient of those rows summed over the batch.  Three flat memory-bound passes of 16-byte
// (8-half) vectors, W % 8 == 0; no atomics, no hand-over between workgroups: every sum has one fixed order and two calls give the same bits.
//
// Shapes: a sequence has L = L0 + P rows, L0 stem rows (class + patches) followed by P prompt rows; B sequences; the stream is [B * L, W] fp16.
//
// Rounding points, the summation order of the gradient and `clear`: pclip_rows.h, whose replace and slice-sum walk these entries are at off = L0,
// L = L0 + P.  append: a prompt element is rounded once (r16), nothing is added to it (no positional embedding on a prompt row); stem rows are copied bit
// for bit.
#include "pclip_rows.h"

namespace {
// out[b, l, :] = t[b, l, :] for l < L0, r16(ctx[l - L0, :]) for L0 <= l < L0 + P
__global__ __launch_bounds__(256) void vpt_append_kernel(const half_t* __restrict__ t, const float* __restrict__ ctx, int B, int L0, int P, int W,
                                                         half_t* __restrict__ out) {
    const int WV = W / 8, L = L0 + P;
    const size_t nvec = (size_t)B * L * WV;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (size_t)gridDim.x * 256) {
        const int d = (int)(i % WV) * 8;
        const size_t row = i / WV;
        const int l = (int)(row % L);
        const size_t b = row / L;
        const half8_t v = l < L0 ? ld_half8(t + (b * L0 + l) * W + d) : r16_row8(ctx + (size_t)(l - L0) * W + d);
        st_half8(out + row * W + d, v);
    }
}

// the envelope all three entries share; 0 = fine
int vpt_envelope(const char* who, int B, int L0, int P, int W) {
    PCLIP_REQUIRE(W > 0 && W % 8 == 0, "%s: W=%d must be a positive multiple of 8 (16-byte vectors)", who, W);
    PCLIP_REQUIRE(P >= 1 && L0 >= 0 && B >= 0, "%s: bad shape B=%d L0=%d P=%d (B >= 0, L0 >= 0, P >= 1)", who, B, L0, P);
    PCLIP_REQUIRE((long long)L0 + P <= PCLIP_VPT_MAX_L, "%s: L0 + P = %d + %d = %lld tokens exceed the attention envelope of %d", who, L0, P,
                  (long long)L0 + P, PCLIP_VPT_MAX_L);
    PCLIP_REQUIRE((unsigned long long)B * (unsigned long long)(L0 + P) * (unsigned long long)W <= 2147483647ull,
                  "%s: B * (L0 + P) * W = %d * %d * %d does not fit an int", who, B, L0 + P, W);
    return PCLIP_OK;
}
}  // namespace

extern "C" int pclip_vpt_append_f16(const void* t, const float* ctx, int B, int L0, int P, int W, void* out, pclip_stream_t stream) {
    PCLIP_REQUIRE(ctx && out && (t || L0 == 0), "pclip_vpt_append_f16: null pointer");
    if (int rc = vpt_envelope("pclip_vpt_append_f16", B, L0, P, W)) return rc;
    PCLIP_REQUIRE((((uintptr_t)t | (uintptr_t)ctx | (uintptr_t)out) & 15) == 0, "pclip_vpt_append_f16: operands must be 16-byte aligned");
    if (B == 0) return PCLIP_OK;
    vpt_append_kernel<<<flat_grid((size_t)B * (L0 + P) * (W / 8)), 256, 0, (hipStream_t)stream>>>((const half_t*)t, ctx, B, L0, P, W, (half_t*)out);
    return pclip_check_launch("vpt_append");
}

extern "C" int pclip_vpt_replace_f16(void* x, const float* ctx, int B, int L0, int P, int W, pclip_stream_t stream) {
    PCLIP_REQUIRE(x && ctx, "pclip_vpt_replace_f16: null pointer");
    if (int rc = vpt_envelope("pclip_vpt_replace_f16", B, L0, P, W)) return rc;
    PCLIP_REQUIRE((((uintptr_t)x | (uintptr_t)ctx) & 15) == 0, "pclip_vpt_replace_f16: operands must be 16-byte aligned");
    if (B == 0) return PCLIP_OK;
    return rows_replace("vpt_replace", x, ctx, B, L0 + P, L0, P, W, stream);
}

extern "C" int pclip_vpt_grad_f32(void* g, int B, int L0, int P, int W, int clear, float* dctx, float* part, int nslice, pclip_stream_t stream) {
    PCLIP_REQUIRE(g && dctx, "pclip_vpt_grad_f32: null pointer");
    if (int rc = vpt_envelope("pclip_vpt_grad_f32", B, L0, P, W)) return rc;
    PCLIP_REQUIRE((((uintptr_t)g | (uintptr_t)dctx | (uintptr_t)part) & 15) == 0, "pclip_vpt_grad_f32: operands must be 16-byte aligned");
    if (B == 0) return PCLIP_OK;
    const int want = (B + PCLIP_VPT_SLICE - 1) / PCLIP_VPT_SLICE;
    PCLIP_REQUIRE(nslice == want, "pclip_vpt_grad_f32: nslice=%d, expected ceil(B / %d) = %d", nslice, PCLIP_VPT_SLICE, want);
    PCLIP_REQUIRE(nslice == 1 || part, "pclip_vpt_grad_f32: %d image slices need the part buffer", nslice);
    return rows_grad<PCLIP_VPT_SLICE>("vpt_grad", g, B, L0 + P, L0, P, P, W, clear, nslice == 1 ? dctx : part, nslice, dctx, stream);
}
