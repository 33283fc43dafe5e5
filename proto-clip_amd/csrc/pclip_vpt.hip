// Visual prompt tuning (VPT): learned fp32 token rows spliced into the vision tower's sequence BEHIND the patch rows (the class token stays row 0, the
// patch rows stay where the stem writes them), and the gradient of those rows summed over the batch.  Three flat memory-bound passes of 16-byte
// (8-half) vectors, W % 8 == 0; no atomics, no hand-over between workgroups: every sum has one fixed order and two calls give the same bits.
//
// Shapes: a sequence has L = L0 + P rows, L0 stem rows (class + patches) followed by P prompt rows; B sequences; the stream is [B * L, W] fp16.
//
// Rounding points
//   append / replace: a prompt element is rounded ONCE, fp32 -> fp16, round to nearest even (r16); nothing is added to it (no positional embedding on a
//                     prompt row).  Stem rows are copied bit for bit (append) or not touched (replace).
//   gradient:         f32(fp16) is exact; every `+` below is one rounded fp32 addition; nothing is rounded to fp16.  The rounding of the prompt to fp16
//                     is passed straight through (as autograd passes a cast).
//
// Summation order of the gradient, dctx[j][d] over the B sequences (`images`):
//   the images are cut into slices of PCLIP_VPT_SLICE = 16 consecutive images (the last one may be short); n0 = 16 s;
//   part[s][j][d] = (..((f32(g[n0, L0 + j, d]) + f32(g[n0 + 1, L0 + j, d])) + f32(g[n0 + 2, L0 + j, d])) + ..)     ascending image order, one accumulator
//   dctx[j][d]    = (..((part[0][j][d] + part[1][j][d]) + part[2][j][d]) + ..)                                      ascending slice order, one accumulator
//   each sum starts from its first term (no zero is added).  One slice: part is dctx itself.
// This is the rule pclip_prompt_ctx_grad_f32 (pclip_prompt.hip) uses for classes.
// clear = 1: the same pass stores exact zeros (+0) over the prompt rows of g it has read — the lane that loaded a vector stores the zeros over it, after
// its load, so no element is cleared before it is read.  Rows l < L0 are neither read nor written.
#include "pclip_common.h"

namespace {
inline int flat_grid(size_t n) { size_t g = (n + 255) / 256; return (int)(g < 1 ? 1 : (g > 16384 ? 16384 : g)); }

__device__ __forceinline__ half8_t r16_row8(const float* __restrict__ c) {
    const float4_t c0 = reinterpret_cast<const float4_t*>(c)[0], c1 = reinterpret_cast<const float4_t*>(c)[1];
    half8_t a;
#pragma unroll
    for (int j = 0; j < 4; ++j) { a[j] = (half_t)c0[j]; a[4 + j] = (half_t)c1[j]; }
    return a;
}

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

// x[b, L0 + j, :] = r16(ctx[j, :]); the other rows are not touched
__global__ __launch_bounds__(256) void vpt_replace_kernel(half_t* __restrict__ x, const float* __restrict__ ctx, int B, int L0, int P, int W) {
    const int WV = W / 8, L = L0 + P;
    const size_t nvec = (size_t)B * P * WV;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (size_t)gridDim.x * 256) {
        const int d = (int)(i % WV) * 8;
        const int j = (int)((i / WV) % P);
        const size_t b = i / ((size_t)WV * P);
        st_half8(x + (b * L + L0 + j) * W + d, r16_row8(ctx + (size_t)j * W + d));
    }
}

// first stage: one thread per (slice, prompt row, 8 columns) walks its slice's images in ascending order
__global__ __launch_bounds__(256) void vpt_grad_part_kernel(half_t* __restrict__ g, int B, int L0, int P, int W, int clear, int nslice,
                                                            float* __restrict__ part) {
    const int WV = W / 8, L = L0 + P;
    const size_t nvec = (size_t)nslice * P * WV;
    half8_t zero;
#pragma unroll
    for (int k = 0; k < 8; ++k) zero[k] = (half_t)0.f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (size_t)gridDim.x * 256) {
        const int d = (int)(i % WV) * 8;
        const int j = (int)((i / WV) % P);
        const int s = (int)(i / ((size_t)WV * P));
        const int n0 = s * PCLIP_VPT_SLICE, n1 = n0 + PCLIP_VPT_SLICE < B ? n0 + PCLIP_VPT_SLICE : B;
        half_t* src = g + ((size_t)n0 * L + L0 + j) * W + d;
        half8_t v = ld_half8(src);
        if (clear) st_half8(src, zero);
        float acc[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] = (float)v[k];
        for (int n = n0 + 1; n < n1; ++n) {
            src += (size_t)L * W;
            v = ld_half8(src);
            if (clear) st_half8(src, zero);
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[k] += (float)v[k];
        }
        float4_t* dst = reinterpret_cast<float4_t*>(part + ((size_t)s * P + j) * W + d);
        float4_t o0, o1;
#pragma unroll
        for (int k = 0; k < 4; ++k) { o0[k] = acc[k]; o1[k] = acc[4 + k]; }
        dst[0] = o0;
        dst[1] = o1;
    }
}

// out[i] = (..(part[0][i] + part[1][i]) + ..) + part[nslice - 1][i], four elements per thread (M % 4 == 0)
__global__ __launch_bounds__(256) void vpt_grad_sum_kernel(const float* __restrict__ part, int nslice, size_t M, float* __restrict__ out) {
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
    vpt_replace_kernel<<<flat_grid((size_t)B * P * (W / 8)), 256, 0, (hipStream_t)stream>>>((half_t*)x, ctx, B, L0, P, W);
    return pclip_check_launch("vpt_replace");
}

extern "C" int pclip_vpt_grad_f32(void* g, int B, int L0, int P, int W, int clear, float* dctx, float* part, int nslice, pclip_stream_t stream) {
    PCLIP_REQUIRE(g && dctx, "pclip_vpt_grad_f32: null pointer");
    if (int rc = vpt_envelope("pclip_vpt_grad_f32", B, L0, P, W)) return rc;
    PCLIP_REQUIRE((((uintptr_t)g | (uintptr_t)dctx | (uintptr_t)part) & 15) == 0, "pclip_vpt_grad_f32: operands must be 16-byte aligned");
    if (B == 0) return PCLIP_OK;
    const int want = (B + PCLIP_VPT_SLICE - 1) / PCLIP_VPT_SLICE;
    PCLIP_REQUIRE(nslice == want, "pclip_vpt_grad_f32: nslice=%d, expected ceil(B / %d) = %d", nslice, PCLIP_VPT_SLICE, want);
    PCLIP_REQUIRE(nslice == 1 || part, "pclip_vpt_grad_f32: %d image slices need the part buffer", nslice);
    hipStream_t s = (hipStream_t)stream;
    vpt_grad_part_kernel<<<flat_grid((size_t)nslice * P * (W / 8)), 256, 0, s>>>((half_t*)g, B, L0, P, W, clear ? 1 : 0, nslice, nslice == 1 ? dctx : part);
    if (nslice > 1) vpt_grad_sum_kernel<<<flat_grid((size_t)P * W / 4), 256, 0, s>>>(part, nslice, (size_t)P * W, dctx);
    return pclip_check_launch("vpt_grad");
}
