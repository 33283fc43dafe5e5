// Learned prompt rows inside an fp16 stream, defined once for CoOp (pclip_prompt.hip), VPT (pclip_vpt.hip), MaPLe (pclip_maple.hip) and CoCoOp
// (pclip_cocoop.hip): writing the rows (replace) and the gradient of the rows summed over the sequences (the slice-sum walk).  Flat memory-bound passes of
// 16-byte (8-half) vectors, W % 8 == 0; no atomics, no hand-over between workgroups: every sum has one fixed order and two calls give the same bits.
//
// Shapes: B sequences of L rows, the stream is [B * L, W] fp16; the P prompt rows are rows off .. off + P - 1 of every sequence.
//   CoOp   off = 1 (the context directly behind SOT), B = the classes
//   VPT    off = L0 = L - P (behind the stem rows); the compact call of the embedding's backward is L = P, off = 0
//   MaPLe  any off with off + P <= L
//   CoCoOp off = 1, B = the classes of ONE image; the images are groups (below)
//
// Rounding points
//   replace:  a prompt element is rounded ONCE, fp32 -> fp16, round to nearest even (r16); nothing is added to it.  Every other row is not touched.
//   gradient: f32(fp16) is exact; every `+` below is one rounded fp32 addition; nothing is rounded to fp16.  The rounding of the prompt to fp16 is
//             passed straight through (as autograd passes a cast).
//
// Summation order of the gradient (THE SLICE-SUM RULE), dctx[j][d] over the B sequences:
//   the sequences are cut into slices of SLICE consecutive sequences (the last one may be short); n0 = SLICE s;
//   part[s][j][d] = (..((f32(g[n0, off + j, d]) + f32(g[n0 + 1, off + j, d])) + f32(g[n0 + 2, off + j, d])) + ..)     ascending sequence order, one accumulator
//   dctx[j][d]    = (..((part[0][j][d] + part[1][j][d]) + part[2][j][d]) + ..)                                        ascending slice order, one accumulator
//   each sum starts from its first term (no zero is added).  One slice: part is dctx itself and there is no merge launch.
//   SLICE is PCLIP_VPT_SLICE = PCLIP_PROMPT_CTX_SLICE = 16 everywhere but for CoOp's class-specific context, which is the first stage alone with slices of
//   ONE class: dctx[n][j][d] = f32(g[n, 1 + j, d]), exact.
//   avail <= P: only the rows j < avail exist in the stream (CoOp's truncated assembly: a context row at 1 + j >= L has no row); the others are not read
//   and their gradient is +0.
//   clear = 1: the same pass stores exact zeros (+0) over the rows of g it has read — the lane that loaded a vector stores the zeros over it, after its
//   load, so no element is cleared before it is read.  Rows outside [off, off + avail) are neither read nor written.
//
// Groups: the GROUPED instantiation of either gradient kernel, launched with gridDim.y = G, runs G independent walks of the same shape, one per
// blockIdx.y; group q reads and writes at its own base, the pointers advanced by q times a per-group stride (elements) the caller passes.  Nothing is
// added across groups and no index is divided by G.  The first stage's groups are CoCoOp's images (stream stride N * L * W, part stride nslice * P * W);
// the merge's groups are the depths of MaPLe's coupling gradient dX (part stride nslice * M, out stride M).  Every other caller takes the ungrouped
// instantiation, which does not read the strides (gridDim.y == 1): the twenty scalar instructions of the two 64-bit base offsets are measurable in passes
// whose time is their launch.
#pragma once
#include "pclip_common.h"

namespace {
inline int flat_grid(size_t n) { size_t g = (n + 255) / 256; return (int)(g < 1 ? 1 : (g > 16384 ? 16384 : g)); }

// r16 of 8 consecutive fp32 elements
__device__ __forceinline__ half8_t r16_row8(const float* __restrict__ c) {
    const float4_t c0 = reinterpret_cast<const float4_t*>(c)[0], c1 = reinterpret_cast<const float4_t*>(c)[1];
    half8_t a;
#pragma unroll
    for (int j = 0; j < 4; ++j) { a[j] = (half_t)c0[j]; a[4 + j] = (half_t)c1[j]; }
    return a;
}

// x[b, off + j, :] = r16(ctx[j, :]); the other rows are not touched
__global__ __launch_bounds__(256) void rows_replace_kernel(half_t* __restrict__ x, const float* __restrict__ ctx, int B, int L, int off, int P, int W) {
    const int WV = W / 8;
    const size_t nvec = (size_t)B * P * WV;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (size_t)gridDim.x * 256) {
        const int d = (int)(i % WV) * 8;
        const int j = (int)((i / WV) % P);
        const size_t b = i / ((size_t)WV * P);
        st_half8(x + (b * L + off + j) * W + d, r16_row8(ctx + (size_t)j * W + d));
    }
}

// first stage: one thread per (slice, prompt row, 8 columns) walks its slice's sequences in ascending order; part [nslice][P][W]; grid (flat, groups)
template <int SLICE, bool GROUPED = false>
__global__ __launch_bounds__(256) void rows_grad_part_kernel(half_t* __restrict__ g, int B, int L, int off, int P, int avail, int W, int clear, int nslice,
                                                             float* __restrict__ part, size_t g_stride, size_t part_stride) {
    if (GROUPED) {
        g += blockIdx.y * g_stride;
        part += blockIdx.y * part_stride;
    }
    const int WV = W / 8;
    const size_t nvec = (size_t)nslice * P * WV;
    half8_t zero;
#pragma unroll
    for (int k = 0; k < 8; ++k) zero[k] = (half_t)0.f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (size_t)gridDim.x * 256) {
        const int d = (int)(i % WV) * 8;
        const int j = (int)((i / WV) % P);
        const int s = (int)(i / ((size_t)WV * P));
        const int n0 = s * SLICE, n1 = n0 + SLICE < B ? n0 + SLICE : B;
        float acc[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] = 0.f;
        if (j < avail) {
            half_t* src = g + ((size_t)n0 * L + off + j) * W + d;
            half8_t v = ld_half8(src);
            if (clear) st_half8(src, zero);
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[k] = (float)v[k];
            for (int n = n0 + 1; n < n1; ++n) {
                src += (size_t)L * W;
                v = ld_half8(src);
                if (clear) st_half8(src, zero);
#pragma unroll
                for (int k = 0; k < 8; ++k) acc[k] += (float)v[k];
            }
        }
        float4_t* dst = reinterpret_cast<float4_t*>(part + ((size_t)s * P + j) * W + d);
        float4_t o0, o1;
#pragma unroll
        for (int k = 0; k < 4; ++k) { o0[k] = acc[k]; o1[k] = acc[4 + k]; }
        dst[0] = o0;
        dst[1] = o1;
    }
}

// the merge: out[i] = (..(part[0][i] + part[1][i]) + ..) + part[nslice - 1][i], four elements per thread (M % 4 == 0); grid (flat, groups)
template <bool GROUPED = false>
__global__ __launch_bounds__(256) void rows_grad_sum_kernel(const float* __restrict__ part, int nslice, size_t M, float* __restrict__ out, size_t part_stride,
                                                            size_t out_stride) {
    if (GROUPED) {
        part += blockIdx.y * part_stride;
        out += blockIdx.y * out_stride;
    }
    const size_t nvec = M / 4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (size_t)gridDim.x * 256) {
        float4_t acc = reinterpret_cast<const float4_t*>(part)[i];
#pragma unroll 8
        for (int s = 1; s < nslice; ++s) {
            const float4_t v = reinterpret_cast<const float4_t*>(part + (size_t)s * M)[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] += v[k];
        }
        reinterpret_cast<float4_t*>(out)[i] = acc;
    }
}

// ---- host: the launches behind the C entries; `name` is the entry's name in a launch error.  The entries check their own envelopes. -----------------------

inline int rows_replace(const char* name, void* x, const float* ctx, int B, int L, int off, int P, int W, pclip_stream_t stream) {
    rows_replace_kernel<<<flat_grid((size_t)B * P * (W / 8)), 256, 0, (hipStream_t)stream>>>((half_t*)x, ctx, B, L, off, P, W);
    return pclip_check_launch(name);
}

// The gradient of rows off .. off + P - 1 in nslice = ceil(B / SLICE) slices: the first stage into `first` [nslice][P][W], then — merged != nullptr and more
// than one slice — the merge of `first` into merged [P][W].  One slice: the caller passes the result itself as `first`.
template <int SLICE>
inline int rows_grad(const char* name, void* g, int B, int L, int off, int P, int avail, int W, int clear, float* first, int nslice, float* merged,
                     pclip_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    rows_grad_part_kernel<SLICE><<<flat_grid((size_t)nslice * P * (W / 8)), 256, 0, s>>>((half_t*)g, B, L, off, P, avail, W, clear ? 1 : 0, nslice, first, 0, 0);
    if (merged && nslice > 1) rows_grad_sum_kernel<><<<flat_grid((size_t)P * W / 4), 256, 0, s>>>(first, nslice, (size_t)P * W, merged, 0, 0);
    return pclip_check_launch(name);
}
}  // namespace
