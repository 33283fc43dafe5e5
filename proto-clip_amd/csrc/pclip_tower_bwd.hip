// Small kernels of the transformer towers' backward (one ResidualAttentionBlock, clip/model.py:171-190): QuickGELU backward, column sums of an fp16
// matrix (bias gradients) and the backward of CLIP's fp32 LayerNorm subclass.  The linears' gradients run on pclip_gemm_f16, the attention's on
// pclip_attention_backward_f16.  No atomics anywhere: every sum has one fixed order.
#include "pclip_common.h"

namespace {
typedef _Float16 half2v_t __attribute__((ext_vector_type(2)));

// ---- QuickGELU backward (clip/model.py:164-166: x * sigmoid(1.702 x)) -------------------------------------------------------------
// du = r16(dy * g(u)),  g(u) = s (1 + t (1 - s)),  t = 1.702 u,  s = 1 / (1 + exp(-t)), everything between the fp16 operands and the one fp16
// rounding of the result in fp32.
__global__ __launch_bounds__(256) void quick_gelu_backward_kernel(const half_t* __restrict__ u, const half_t* __restrict__ dy,
                                                                  half_t* __restrict__ du, size_t n) {
    for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 8; i < n; i += (size_t)gridDim.x * 256 * 8) {
        if (i + 8 <= n) {
            const half8_t uv = ld_half8(u + i), gv = ld_half8(dy + i);
            half8_t o;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float t = 1.702f * (float)uv[j];
                const float s = 1.f / (1.f + __expf(-t));
                o[j] = (half_t)((float)gv[j] * (s * (1.f + t * (1.f - s))));
            }
            st_half8(du + i, o);
        } else {
            for (size_t k = i; k < n; ++k) {
                const float t = 1.702f * (float)u[k];
                const float s = 1.f / (1.f + __expf(-t));
                du[k] = (half_t)((float)dy[k] * (s * (1.f + t * (1.f - s))));
            }
        }
    }
}

// ---- column sums of an fp16 matrix, fp32 ---------------------------------------------------------------------------------------------
// part[i][c] = sum of x[r][c] over the rows r of slice i (rows [i * rps, (i + 1) * rps)), added one after the other in row order; the caller
// finishes with pclip_colsum_f32 over the nslice rows of `part` (the partial-sum scheme of the LayerNorm backward).
__global__ __launch_bounds__(256) void colsum_f16_kernel(const half_t* __restrict__ x, int ldx, int R, int C, int rps, float* __restrict__ part) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const int r0 = blockIdx.y * rps, r1 = r0 + rps < R ? r0 + rps : R;
    float s = 0.f;
    for (int r = r0; r < r1; ++r) s += (float)x[(size_t)r * ldx + c];
    part[(size_t)blockIdx.y * C + c] = s;
}

// ---- LayerNorm backward, fp32 gamma and fp32 statistics (clip/model.py:155-161: the subclass computes in fp32 and casts back) -------------
// y = r16(xh * gamma + beta), xh = (x - mu) * rstd with x fp16 and everything else fp32.
//   gy = dy * gamma      dx = r16(residual + rstd * (gy - mean(gy) - xh * mean(gy * xh)))
// `residual` (optional, fp16): the gradient that reaches x past the LayerNorm on the residual stream — added in fp32 before the ONE rounding of dx.
// Partial parameter gradients of the rows a workgroup visits go to part[blockIdx.x][0 | 1][D] (dgamma | dbeta), summed by pclip_colsum_f32.
template <int NI>
__global__ __launch_bounds__(256) void layernorm_backward_g32_kernel(const half_t* __restrict__ x, int ldx, const float* __restrict__ gamma,
                                                                     const half_t* __restrict__ dy, int lddy, const half_t* __restrict__ res,
                                                                     int ldr, int R, int D, float eps, half_t* __restrict__ dx, int lddx,
                                                                     float* __restrict__ part) {
    __shared__ float red[4][NI * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float dg[NI], db[NI], gm[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        dg[i] = db[i] = 0.f;
        const int d = i * 64 + lane;
        gm[i] = d < D ? gamma[d] : 0.f;
    }
    for (int row = blockIdx.x * 4 + wave; row < R; row += gridDim.x * 4) {
        const half_t* xr = x + (size_t)row * ldx;
        const half_t* gr = dy + (size_t)row * lddy;
        float xv[NI], gv[NI];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int d = i * 64 + lane;
            xv[i] = d < D ? (float)xr[d] : 0.f;
            gv[i] = d < D ? (float)gr[d] : 0.f;
            s += xv[i];
        }
        const float mu = wave_sum(s) / (float)D;
        float ss = 0.f;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int d = i * 64 + lane;
            const float c = d < D ? xv[i] - mu : 0.f;
            ss = __builtin_fmaf(c, c, ss);
        }
        const float rstd = 1.f / sqrtf(wave_sum(ss) / (float)D + eps);
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int d = i * 64 + lane;
            if (d < D) {
                const float xh = (xv[i] - mu) * rstd, gy = gv[i] * gm[i];
                a += gy;
                b = __builtin_fmaf(gy, xh, b);
                dg[i] = __builtin_fmaf(gv[i], xh, dg[i]);
                db[i] += gv[i];
            }
        }
        a = wave_sum(a) / (float)D;
        b = wave_sum(b) / (float)D;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int d = i * 64 + lane;
            if (d < D) {
                const float xh = (xv[i] - mu) * rstd, gy = gv[i] * gm[i];
                float v = rstd * (gy - a - xh * b);
                if (res) v += (float)res[(size_t)row * ldr + d];
                dx[(size_t)row * lddx + d] = (half_t)v;
            }
        }
    }
    for (int pass = 0; pass < 2; ++pass) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NI; ++i) red[wave][i * 64 + lane] = pass ? db[i] : dg[i];
        __syncthreads();
        for (int d = threadIdx.x; d < D; d += 256)
            part[((size_t)blockIdx.x * 2 + pass) * D + d] = ((red[0][d] + red[1][d]) + red[2][d]) + red[3][d];
    }
}
}  // namespace

extern "C" int pclip_quick_gelu_backward_f16(const void* u, const void* dy, void* du, size_t n, pclip_stream_t stream) {
    PCLIP_REQUIRE((u && dy && du) || n == 0, "pclip_quick_gelu_backward_f16: null pointer");
    PCLIP_REQUIRE(!(((uintptr_t)u | (uintptr_t)dy | (uintptr_t)du) & 15), "pclip_quick_gelu_backward_f16: operands must be 16-byte aligned");
    if (n == 0) return PCLIP_OK;
    size_t g = (n + 2047) / 2048;
    if (g > 16384) g = 16384;
    quick_gelu_backward_kernel<<<(int)g, 256, 0, (hipStream_t)stream>>>((const half_t*)u, (const half_t*)dy, (half_t*)du, n);
    return pclip_check_launch("quick_gelu_backward");
}

extern "C" int pclip_colsum_f16(const void* x, int ldx, int R, int C, float* part, int nslice, pclip_stream_t stream) {
    PCLIP_REQUIRE(x && part, "pclip_colsum_f16: null pointer");
    PCLIP_REQUIRE(R >= 1 && C >= 1 && ldx >= C && nslice >= 1 && nslice <= 65535, "pclip_colsum_f16: bad R=%d C=%d ldx=%d nslice=%d", R, C, ldx, nslice);
    const int rps = ceil_div(R, nslice);                            // slices beyond the last row write zeros
    colsum_f16_kernel<<<dim3(ceil_div(C, 256), nslice), 256, 0, (hipStream_t)stream>>>((const half_t*)x, ldx, R, C, rps, part);
    return pclip_check_launch("colsum_f16");
}

extern "C" int pclip_layernorm_backward_g32_f16(const void* x, int ldx, const float* gamma, const void* dy, int lddy, const void* residual,
                                                int ldr, int R, int D, float eps, void* dx, int lddx, float* part, int nblk,
                                                pclip_stream_t stream) {
    PCLIP_REQUIRE(x && gamma && dy && dx && part, "pclip_layernorm_backward_g32_f16: null pointer");
    PCLIP_REQUIRE(R >= 0 && D > 0 && D <= 2048 && ldx >= D && lddy >= D && lddx >= D && (!residual || ldr >= D) && nblk > 0,
                  "pclip_layernorm_backward_g32_f16: bad R=%d D=%d (<=2048) nblk=%d", R, D, nblk);
    hipStream_t s = (hipStream_t)stream;
#define LNB(NI) layernorm_backward_g32_kernel<NI><<<nblk, 256, 0, s>>>((const half_t*)x, ldx, gamma, (const half_t*)dy, lddy, (const half_t*)residual, ldr, R, D, eps, (half_t*)dx, lddx, part)
    if (D <= 256) LNB(4);
    else if (D <= 512) LNB(8);
    else if (D <= 1024) LNB(16);
    else LNB(32);
#undef LNB
    return pclip_check_launch("layernorm_backward_g32");
}
