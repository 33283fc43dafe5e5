// Conv adapter (model.py:12-78) at the widths the width-16 kernels of pclip_adapter.hip do not cover: `Adapter(c_in, c_type, width=W)`, W in {8, 24, 32}.
// Width 16 is forwarded to the existing entry points and runs exactly the kernels it ran before.
//
// One workgroup works on one feature row at a time; the [W, s, s] activation stacks live in LDS as in the width-16 kernels.  What is different:
//  * conv2 (3x3, W -> W) is an implicit GEMM on v_mfma_f32_16x16x32_f16 at every width.  The operand image is pixel-major, [halo pixel][W channels] fp16 with a
//    zero halo, and the reduction index runs over 8-channel chunks: chunk c8 = tap * (W / 8) + ci / 8, four chunks per k-step, so a lane's B fragment is ONE
//    16-byte LDS read of pixel (y + dy, x + dx).  K = 9 W: 72 -> 3 k-steps (W = 8, three chunks of zero weights), 216 -> 7 (W = 24, one zero chunk), 288 -> 9 (W = 32,
//    no padding).  Output channels are ceil(W / 16) M-tiles; rows >= W carry zero weights and are never stored, so the LayerNorm statistics count W s^2 elements.
//  * the forward is persistent over rows (weights fragments and the halo are set up once per workgroup); LayerNorm parameters are re-read per row (L2).
//  * the backward keeps TWO halo images, A and T, and walks  a1 -> A, t2 -> T, dt2 -> A, a1 (recomputed from the row and LN1's two scalars) -> T, da1 -> T:
//    2 * 2 W (s+2)^2 + 8.7 KB = 157 KB at W = 32, D = 1024, inside the 160 KiB a workgroup can have, at every (W, D) of the envelope.  The transposed
//    convolution is the same implicit GEMM with conv2 transposed and its taps mirrored; conv2's weight gradient is plain fp32 chains over the pixels.
// Rounding points are the width-16 kernels' (SURVEY Appendix A): r16 after each convolution's fp32 accumulation, fp32 LayerNorm statistics over the fp16
// tensor, r16 after the affine; gradient tensors are rounded to fp16 where autograd materialises one.
#include "pclip_common.h"

extern "C" int pclip_adapter_conv_f16(const void* x, int B, int D, int three_x, const void* conv1, const void* ln1w, const void* ln1b, const void* conv2,
                                      const void* ln2w, const void* ln2b, const void* conv3, const void* ln3w, const void* ln3b, int l2norm_out, void* y,
                                      float* y_sq, pclip_stream_t stream);
extern "C" int pclip_adapter_conv_backward_partials(int B, int D, int three_x);
extern "C" int pclip_adapter_conv_backward_f16(const void* x, const void* g, int B, int D, int three_x, const void* conv1, const void* ln1w, const void* ln1b,
                                               const void* conv2, const void* ln2w, const void* ln2b, const void* conv3, const void* ln3w, float* pw1,
                                               float* pw2, float* pw3, float* pg1, float* pb1, float* pg2, float* pb2, float* pg3, float* pb3,
                                               pclip_stream_t stream);

namespace {

typedef float float4v_t __attribute__((ext_vector_type(4)));

template <int W>
struct ConvW {
    static_assert(W % 8 == 0 && W <= 32, "conv adapter width");
    static constexpr int MT = (W + 15) / 16;      // 16-row M-tiles of output channels
    static constexpr int C8 = W / 8;              // 8-channel chunks per tap
    static constexpr int NCH = 9 * C8;            // chunks of the reduction
    static constexpr int KS = (NCH + 3) / 4;      // k-steps of 32
};

__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();                       // protect red[] from the previous use
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

template <int W>
__device__ __forceinline__ void block_sum_w(float (&v)[W], float* red /* [4][W] */) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int c = 0; c < W; ++c) v[c] = wave_sum(v[c]);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < W; ++c) red[wave * W + c] = v[c];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < W; ++c) v[c] = red[c] + red[W + c] + red[2 * W + c] + red[3 * W + c];
}

// conv2 as the MFMA A operand: lane holds row (lane & 15) of M-tile m, reduction chunk 4 ks + (lane >> 4).  TRANSPOSED: rows are INPUT channels, the
// reduction runs over output channels and the tap is mirrored (the transposed convolution reads dt2 at (y + 2 - dy, x + 2 - dx) of the halo image).
template <int W, bool TRANSPOSED>
__device__ __forceinline__ void load_conv2_frags(const half_t* __restrict__ conv2, half8_t (&wf)[ConvW<W>::MT][ConvW<W>::KS]) {
    using C = ConvW<W>;
    const int lane = threadIdx.x & 63, q = lane >> 4;
#pragma unroll
    for (int m = 0; m < C::MT; ++m)
#pragma unroll
        for (int ks = 0; ks < C::KS; ++ks) {
            const int row = 16 * m + (lane & 15), c8 = 4 * ks + q, tap = c8 / C::C8, k0 = 8 * (c8 % C::C8);
            const bool ok = row < W && c8 < C::NCH;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int idx = !ok ? 0 : TRANSPOSED ? ((k0 + j) * W + row) * 9 + (8 - tap) : (row * W + k0 + j) * 9 + tap;      // < 9 W W
                wf[m][ks][j] = ok ? conv2[idx] : (half_t)0.f;
            }
        }
}
// offset (in halves) of this lane's chunk inside the halo image, relative to tap (0, 0) of the pixel; chunks >= NCH have zero weights and re-read the last one
template <int W>
__device__ __forceinline__ void conv2_chunk_offsets(int sp, int (&toff)[ConvW<W>::KS]) {
    using C = ConvW<W>;
    const int q = (threadIdx.x & 63) >> 4;
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks) {
        const int c8 = 4 * ks + q < C::NCH ? 4 * ks + q : C::NCH - 1, tap = c8 / C::C8, k0 = 8 * (c8 % C::C8);
        toff[ks] = ((tap / 3) * sp + tap % 3) * W + k0;
    }
}
// out(c, p, v): fp32 accumulation of channel c at pixel p, every (c < W, p < s2) exactly once; wave w owns the 16-pixel tiles w, w + 4, ...
template <int W, class Out>
__device__ __forceinline__ void conv2_mfma(const half_t* src, const half8_t (&wf)[ConvW<W>::MT][ConvW<W>::KS], const int (&toff)[ConvW<W>::KS], int s, int s2,
                                           Out&& out) {
    using C = ConvW<W>;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, sp = s + 2;
    for (int t = wave; 16 * t < s2; t += 4) {
        const int p = 16 * t + (lane & 15), pc = p < s2 ? p : 0, py = pc / s, px = pc - py * s;      // a tile's spare lanes recompute pixel 0 and store nothing
        const half_t* base = src + (py * sp + px) * W;
        float4v_t acc[C::MT];
#pragma unroll
        for (int m = 0; m < C::MT; ++m) acc[m] = float4v_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < C::KS; ++ks) {
            const half8_t bfrag = *reinterpret_cast<const half8_t*>(base + toff[ks]);
#pragma unroll
            for (int m = 0; m < C::MT; ++m) acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[m][ks], bfrag, acc[m], 0, 0, 0);
        }
#pragma unroll
        for (int m = 0; m < C::MT; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = 16 * m + 4 * q + r;
                if (c < W && p < s2) out(c, p, acc[m][r]);
            }
    }
}

// a1 = r16(LN1(r16(w1[c] x))) of every pixel into the interior of a pixel-major halo image
template <int W>
__device__ __forceinline__ void write_a1(half_t* img, const float* xs, const float (&w1)[W], float mean1, float rstd1, const half_t* __restrict__ ln1w,
                                         const half_t* __restrict__ ln1b, int s, int s2) {
    const int sp = s + 2;
    for (int p = threadIdx.x; p < s2; p += 256) {
        const float xv = xs[p];
        const int py = p / s, px = p - py * s;
        half_t* dst = img + ((py + 1) * sp + px + 1) * W;
#pragma unroll
        for (int c8 = 0; c8 < W / 8; ++c8) {
            half8_t o;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int c = 8 * c8 + j;
                o[j] = (half_t)((r16(w1[c] * xv) - mean1) * rstd1 * (float)ln1w[c * s2 + p] + (float)ln1b[c * s2 + p]);
            }
            *reinterpret_cast<half8_t*>(dst + 8 * c8) = o;
        }
    }
}

// LDS (bytes), s2 = s * s, hp = (s + 2)^2:  xs float[1024] | u float[1024] | red float[4] | a1h half[hp][W] | t2 half[W][s2]   (the last two: conv-3x only)
template <int W, bool THREE_X>
__global__ __launch_bounds__(256, 2) void adapter_conv_w_kernel(const half_t* __restrict__ x, int B, int D, int s, const half_t* __restrict__ conv1,
                                                                const half_t* __restrict__ ln1w, const half_t* __restrict__ ln1b,
                                                                const half_t* __restrict__ conv2, const half_t* __restrict__ ln2w,
                                                                const half_t* __restrict__ ln2b, const half_t* __restrict__ conv3,
                                                                const half_t* __restrict__ ln3w, const half_t* __restrict__ ln3b, int l2norm,
                                                                half_t* __restrict__ y, float* __restrict__ y_sq) {
    using C = ConvW<W>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int s2 = s * s, sp = s + 2, hp = sp * sp, n1 = W * s2;
    float* xs = reinterpret_cast<float*>(smem);
    float* u = xs + 1024;
    float* red = u + 1024;
    half_t* a1h = reinterpret_cast<half_t*>(red + 4);
    half_t* t2 = a1h + hp * W;
    const int tid = threadIdx.x;
    const float eps = 1e-5f;

    float w1[W], w3[W];
#pragma unroll
    for (int c = 0; c < W; ++c) { w1[c] = (float)conv1[c]; w3[c] = (float)conv3[c]; }
    half8_t wf[C::MT][C::KS];
    int toff[C::KS];
    if (THREE_X) {
        for (int i = tid; i < hp * W / 2; i += 256) reinterpret_cast<unsigned*>(a1h)[i] = 0u;      // the halo stays zero: rows only rewrite the interior
        load_conv2_frags<W, false>(conv2, wf);
        conv2_chunk_offsets<W>(sp, toff);
    }

    for (int row = blockIdx.x; row < B; row += gridDim.x) {
        __syncthreads();                                                                           // the previous row's readers of xs / u / a1h / t2 are done
        for (int p = tid; p < s2; p += 256) xs[p] = p < D ? (float)x[(size_t)row * D + p] : 0.f;
        __syncthreads();
        // conv1 (1x1, 1 -> W, model.py:63) + LN1 over [W, s, s] (model.py:64): t = r16(w1[c] * x[p])
        float sm = 0.f;
        for (int p = tid; p < s2; p += 256) {
            const float xv = xs[p];
#pragma unroll
            for (int c = 0; c < W; ++c) sm += r16(w1[c] * xv);
        }
        const float mean1 = block_sum(sm, red) / (float)n1;
        float sq = 0.f;
        for (int p = tid; p < s2; p += 256) {
            const float xv = xs[p];
#pragma unroll
            for (int c = 0; c < W; ++c) { const float t = r16(w1[c] * xv) - mean1; sq += t * t; }
        }
        const float rstd1 = 1.f / sqrtf(block_sum(sq, red) / (float)n1 + eps);

        if (THREE_X) {
            write_a1<W>(a1h, xs, w1, mean1, rstd1, ln1w, ln1b, s, s2);
            __syncthreads();
            // conv2 3x3 pad 1, W -> W (model.py:67) on the matrix pipe; t2 = r16(acc), channel-major
            float sm2 = 0.f;
            conv2_mfma<W>(a1h, wf, toff, s, s2, [&](int c, int p, float v) {
                const half_t h = (half_t)v;
                t2[c * s2 + p] = h;
                sm2 += (float)h;
            });
            const float mean2 = block_sum(sm2, red) / (float)n1;   // block_sum's barriers also publish t2
            float sq2 = 0.f;
            for (int i = tid; i < n1; i += 256) { const float t = (float)t2[i] - mean2; sq2 += t * t; }
            const float rstd2 = 1.f / sqrtf(block_sum(sq2, red) / (float)n1 + eps);
            // conv3 (1x1, W -> 1, model.py:70) on a2 = r16(LN2(t2))
            for (int p = tid; p < s2; p += 256) {
                float acc = 0.f;
#pragma unroll
                for (int c = 0; c < W; ++c) {
                    const float a2 = r16(((float)t2[c * s2 + p] - mean2) * rstd2 * (float)ln2w[c * s2 + p] + (float)ln2b[c * s2 + p]);
                    acc = fmaf(w3[c], a2, acc);
                }
                u[p] = r16(acc);
            }
        } else {
            // conv-2x: conv3 directly on a1 = r16(LN1)
            for (int p = tid; p < s2; p += 256) {
                const float xv = xs[p];
                float acc = 0.f;
#pragma unroll
                for (int c = 0; c < W; ++c) {
                    const float a1 = r16((r16(w1[c] * xv) - mean1) * rstd1 * (float)ln1w[c * s2 + p] + (float)ln1b[c * s2 + p]);
                    acc = fmaf(w3[c], a1, acc);
                }
                u[p] = r16(acc);
            }
        }
        // LN3 over [1, s, s] (model.py:71), + identity (model.py:73), crop to D (model.py:75-76)
        float s3 = 0.f;
        for (int p = tid; p < s2; p += 256) s3 += u[p];       // own writes only: no barrier needed yet
        const float mean3 = block_sum(s3, red) / (float)s2;
        float q3 = 0.f;
        for (int p = tid; p < s2; p += 256) { const float t = u[p] - mean3; q3 += t * t; }
        const float rstd3 = 1.f / sqrtf(block_sum(q3, red) / (float)s2 + eps);
        float ss = 0.f;
        for (int p = tid; p < D; p += 256) {
            const float o = r16((u[p] - mean3) * rstd3 * (float)ln3w[p] + (float)ln3b[p]);
            const float v = r16(o + xs[p]);
            u[p] = v;
            ss += v * v;
        }
        if (l2norm) {
            const float n = r16(sqrtf(block_sum(ss, red)));
            ss = 0.f;
            for (int p = tid; p < D; p += 256) {
                const half_t h = (half_t)(u[p] / n);
                y[(size_t)row * D + p] = h;
                ss += (float)h * (float)h;
            }
        } else {
            for (int p = tid; p < D; p += 256) y[(size_t)row * D + p] = (half_t)u[p];
        }
        if (y_sq) {
            const float t = block_sum(ss, red);
            if (tid == 0) y_sq[row] = t;
        }
    }
}

// Backward, one workgroup per row, per-row fp32 contributions as adapter_conv_backward_kernel (pclip_adapter.hip):
//   pw1/pw3 [B,W], pw2 [B,9 W W], pg1/pb1/pg2/pb2 [B,W s2], pg3/pb3 [B,s2]
// LDS: xs float[1024] | u float[1024] | red float[4] | redw float[4][W] | A half[hp][W] | T half[hp][W]   (A, T: conv-3x only, pixel-major halo images)
template <int W, bool THREE_X>
__global__ __launch_bounds__(256) void adapter_conv_w_backward_kernel(
    const half_t* __restrict__ x, const half_t* __restrict__ g, int D, int s, const half_t* __restrict__ conv1, const half_t* __restrict__ ln1w,
    const half_t* __restrict__ ln1b, const half_t* __restrict__ conv2, const half_t* __restrict__ ln2w, const half_t* __restrict__ ln2b,
    const half_t* __restrict__ conv3, const half_t* __restrict__ ln3w, float* __restrict__ pw1, float* __restrict__ pw2, float* __restrict__ pw3,
    float* __restrict__ pg1, float* __restrict__ pb1, float* __restrict__ pg2, float* __restrict__ pb2, float* __restrict__ pg3, float* __restrict__ pb3) {
    using C = ConvW<W>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int s2 = s * s, sp = s + 2, hp = sp * sp, n1 = W * s2;
    float* xs = reinterpret_cast<float*>(smem);
    float* u = xs + 1024;
    float* red = u + 1024;
    float* redw = red + 4;
    half_t* A = reinterpret_cast<half_t*>(redw + 4 * W);
    half_t* T = A + hp * W;
    const int tid = threadIdx.x;
    const size_t row = blockIdx.x;
    const float eps = 1e-5f;
    auto interior = [&](int p) { const int py = p / s, px = p - py * s; return ((py + 1) * sp + px + 1) * W; };

    for (int p = tid; p < s2; p += 256) xs[p] = p < D ? (float)x[row * D + p] : 0.f;
    float w1[W], w3[W];
#pragma unroll
    for (int c = 0; c < W; ++c) { w1[c] = (float)conv1[c]; w3[c] = (float)conv3[c]; }
    half8_t wf[C::MT][C::KS];
    int toff[C::KS];
    if (THREE_X) {
        for (int i = tid; i < hp * W; i += 256) reinterpret_cast<unsigned*>(A)[i] = 0u;           // A and T are adjacent: 2 hp W halves = hp W words
        conv2_chunk_offsets<W>(sp, toff);
    }
    __syncthreads();

    // ---------------- forward recomputation (the arithmetic of adapter_conv_w_kernel) ----------------
    float sm = 0.f;
    for (int p = tid; p < s2; p += 256) {
        const float xv = xs[p];
#pragma unroll
        for (int c = 0; c < W; ++c) sm += r16(w1[c] * xv);
    }
    const float mean1 = block_sum(sm, red) / (float)n1;
    float sq = 0.f;
    for (int p = tid; p < s2; p += 256) {
        const float xv = xs[p];
#pragma unroll
        for (int c = 0; c < W; ++c) { const float t = r16(w1[c] * xv) - mean1; sq += t * t; }
    }
    const float rstd1 = 1.f / sqrtf(block_sum(sq, red) / (float)n1 + eps);
    float mean2 = 0.f, rstd2 = 0.f;
    if (THREE_X) {
        write_a1<W>(A, xs, w1, mean1, rstd1, ln1w, ln1b, s, s2);
        load_conv2_frags<W, false>(conv2, wf);
        __syncthreads();
        float sm2 = 0.f;
        conv2_mfma<W>(A, wf, toff, s, s2, [&](int c, int p, float v) {
            const half_t h = (half_t)v;
            T[interior(p) + c] = h;                                                              // t2, pixel-major
            sm2 += (float)h;
        });
        mean2 = block_sum(sm2, red) / (float)n1;                                                 // block_sum's barriers also publish t2
        float sq2 = 0.f;
        for (int p = tid; p < s2; p += 256) {
            const half_t* tp = T + interior(p);
#pragma unroll
            for (int c = 0; c < W; ++c) { const float t = (float)tp[c] - mean2; sq2 += t * t; }
        }
        rstd2 = 1.f / sqrtf(block_sum(sq2, red) / (float)n1 + eps);
        for (int p = tid; p < s2; p += 256) {
            const half_t* tp = T + interior(p);
            float acc = 0.f;
#pragma unroll
            for (int c = 0; c < W; ++c) {
                const float a2 = r16(((float)tp[c] - mean2) * rstd2 * (float)ln2w[c * s2 + p] + (float)ln2b[c * s2 + p]);
                acc = fmaf(w3[c], a2, acc);
            }
            u[p] = r16(acc);
        }
    } else {
        for (int p = tid; p < s2; p += 256) {
            const float xv = xs[p];
            float acc = 0.f;
#pragma unroll
            for (int c = 0; c < W; ++c) {
                const float a1 = r16((r16(w1[c] * xv) - mean1) * rstd1 * (float)ln1w[c * s2 + p] + (float)ln1b[c * s2 + p]);
                acc = fmaf(w3[c], a1, acc);
            }
            u[p] = r16(acc);
        }
    }
    float s3 = 0.f;
    for (int p = tid; p < s2; p += 256) s3 += u[p];
    const float mean3 = block_sum(s3, red) / (float)s2;
    float q3 = 0.f;
    for (int p = tid; p < s2; p += 256) { const float t = u[p] - mean3; q3 += t * t; }
    const float rstd3 = 1.f / sqrtf(block_sum(q3, red) / (float)s2 + eps);

    // ---------------- LN3 backward: upstream = g on the first D positions (crop + identity add pass it through) ----------
    float sa = 0.f, sb = 0.f;
    for (int p = tid; p < s2; p += 256) {
        const float go = p < D ? (float)g[row * D + p] : 0.f;
        const float xh = (u[p] - mean3) * rstd3, gy = go * (float)ln3w[p];
        sa += gy;
        sb += gy * xh;
        pg3[row * s2 + p] = go * xh;
        pb3[row * s2 + p] = go;
    }
    const float A3 = block_sum(sa, red) / (float)s2, B3 = block_sum(sb, red) / (float)s2;
    for (int p = tid; p < s2; p += 256) {
        const float go = p < D ? (float)g[row * D + p] : 0.f;
        const float xh = (u[p] - mean3) * rstd3, gy = go * (float)ln3w[p];
        u[p] = r16(rstd3 * (gy - A3 - xh * B3));                    // du, fp16 like autograd's grad of conv3's output
    }
    // ---------------- conv3 backward: dW3[c] = sum_p du[p] * a_last[c,p];  da_last = r16(w3[c] * du[p]) ----------------
    float accw[W];
#pragma unroll
    for (int c = 0; c < W; ++c) accw[c] = 0.f;
    for (int p = tid; p < s2; p += 256) {
        const float du = u[p], xv = xs[p];
        const half_t* tp = T + (THREE_X ? interior(p) : 0);
#pragma unroll
        for (int c = 0; c < W; ++c) {
            const float al = THREE_X ? r16(((float)tp[c] - mean2) * rstd2 * (float)ln2w[c * s2 + p] + (float)ln2b[c * s2 + p])
                                     : r16((r16(w1[c] * xv) - mean1) * rstd1 * (float)ln1w[c * s2 + p] + (float)ln1b[c * s2 + p]);
            accw[c] = fmaf(du, al, accw[c]);
        }
    }
    block_sum_w<W>(accw, redw);
    if (tid < W) pw3[row * W + tid] = redw[tid] + redw[W + tid] + redw[2 * W + tid] + redw[3 * W + tid];

    if (THREE_X) {
        // ------------ LN2 backward: da2 = r16(w3[c] du[p]); dt2 = rstd2 (gy - mean gy - xh mean(gy xh)) ------------
        sa = sb = 0.f;
        for (int p = tid; p < s2; p += 256) {
            const float du = u[p];
            const half_t* tp = T + interior(p);
#pragma unroll
            for (int c = 0; c < W; ++c) {
                const float da = r16(w3[c] * du);
                const float xh = ((float)tp[c] - mean2) * rstd2, gy = da * (float)ln2w[c * s2 + p];
                sa += gy;
                sb += gy * xh;
                pg2[row * n1 + c * s2 + p] = da * xh;
                pb2[row * n1 + c * s2 + p] = da;
            }
        }
        const float A2 = block_sum(sa, red) / (float)n1, B2 = block_sum(sb, red) / (float)n1;
        // dt2 replaces a1 in A (conv2's reads of a1 ended before the first block_sum after it); each thread reads t2 of its own pixels only
        for (int p = tid; p < s2; p += 256) {
            const float du = u[p];
            const int ip = interior(p);
#pragma unroll
            for (int c = 0; c < W; ++c) {
                const float da = r16(w3[c] * du);
                const float xh = ((float)T[ip + c] - mean2) * rstd2, gy = da * (float)ln2w[c * s2 + p];
                A[ip + c] = (half_t)(rstd2 * (gy - A2 - xh * B2));
            }
        }
        // a1 again, from the row and LN1's two scalars, over t2 (dead now; a thread overwrites only the pixels whose t2 it alone read above)
        write_a1<W>(T, xs, w1, mean1, rstd1, ln1w, ln1b, s, s2);
        __syncthreads();
        // ------------ conv2 weight gradient: dW2[co,ci,tap] = sum_p dt2[co,p] * a1[ci, p + tap] ------------
        // A work item is (co pair, ci pair, tap): per pixel one 4-byte read of each operand feeds four fmaf chains, every output a (py, px)-ordered fp32 chain.
        for (int it = tid; it < (W / 2) * (W / 2) * 9; it += 256) {
            const int tap = it % 9, cip = (it / 9) % (W / 2), cop = it / (9 * (W / 2));
            const int dy = tap / 3, dx = tap - dy * 3;
            float a00 = 0.f, a01 = 0.f, a10 = 0.f, a11 = 0.f;       // [co parity][ci parity]
            for (int py = 0; py < s; ++py)
                for (int px = 0; px < s; ++px) {
                    const half2_t dv = *reinterpret_cast<const half2_t*>(A + ((py + 1) * sp + px + 1) * W + 2 * cop);
                    const half2_t av = *reinterpret_cast<const half2_t*>(T + ((py + dy) * sp + px + dx) * W + 2 * cip);
                    a00 = fmaf((float)dv[0], (float)av[0], a00);
                    a01 = fmaf((float)dv[0], (float)av[1], a01);
                    a10 = fmaf((float)dv[1], (float)av[0], a10);
                    a11 = fmaf((float)dv[1], (float)av[1], a11);
                }
            float* dst = pw2 + row * (W * W * 9);
            dst[((2 * cop) * W + 2 * cip) * 9 + tap] = a00;
            dst[((2 * cop) * W + 2 * cip + 1) * 9 + tap] = a01;
            dst[((2 * cop + 1) * W + 2 * cip) * 9 + tap] = a10;
            dst[((2 * cop + 1) * W + 2 * cip + 1) * 9 + tap] = a11;
        }
        // ------------ conv2 input gradient (transposed conv): da1[ci,p] = r16(sum_co,tap dt2[co, p - tap + 1] w2[co,ci,tap]) ----
        load_conv2_frags<W, true>(conv2, wf);
        __syncthreads();                                            // T is overwritten with da1 below: all readers of a1 are done
        conv2_mfma<W>(A, wf, toff, s, s2, [&](int c, int p, float v) { T[interior(p) + c] = (half_t)v; });
        __syncthreads();
    }
    // ---------------- LN1 backward + conv1 weight gradient ----------------
    sa = sb = 0.f;
    for (int p = tid; p < s2; p += 256) {
        const float du = u[p], xv = xs[p];
        const half_t* tp = T + (THREE_X ? interior(p) : 0);
#pragma unroll
        for (int c = 0; c < W; ++c) {
            const float da = THREE_X ? (float)tp[c] : r16(w3[c] * du);
            const float xh = (r16(w1[c] * xv) - mean1) * rstd1, gy = da * (float)ln1w[c * s2 + p];
            sa += gy;
            sb += gy * xh;
            pg1[row * n1 + c * s2 + p] = da * xh;
            pb1[row * n1 + c * s2 + p] = da;
        }
    }
    const float A1 = block_sum(sa, red) / (float)n1, B1 = block_sum(sb, red) / (float)n1;
#pragma unroll
    for (int c = 0; c < W; ++c) accw[c] = 0.f;
    for (int p = tid; p < s2; p += 256) {
        const float du = u[p], xv = xs[p];
        const half_t* tp = T + (THREE_X ? interior(p) : 0);
#pragma unroll
        for (int c = 0; c < W; ++c) {
            const float da = THREE_X ? (float)tp[c] : r16(w3[c] * du);
            const float xh = (r16(w1[c] * xv) - mean1) * rstd1, gy = da * (float)ln1w[c * s2 + p];
            const float dt1 = r16(rstd1 * (gy - A1 - xh * B1));
            accw[c] = fmaf(dt1, xv, accw[c]);
        }
    }
    block_sum_w<W>(accw, redw);
    if (tid < W) pw1[row * W + tid] = redw[tid] + redw[W + tid] + redw[2 * W + tid] + redw[3 * W + tid];
}

constexpr size_t kLdsMax = 160 * 1024;

bool width_ok(int width) { return width == 8 || width == 16 || width == 24 || width == 32; }
int side_of(int D) {
    int s = 1;
    while (s * s < D) ++s;          // ceil(sqrt(D)), model.py:30
    return s;
}

template <int W, bool THREE_X>
int launch_forward(const void* x, int B, int D, const void* conv1, const void* ln1w, const void* ln1b, const void* conv2, const void* ln2w, const void* ln2b,
                   const void* conv3, const void* ln3w, const void* ln3b, int l2norm_out, void* y, float* y_sq, hipStream_t st) {
    const int s = side_of(D), s2 = s * s, hp = (s + 2) * (s + 2);
    const size_t lds = (size_t)(1024 + 1024 + 4) * 4 + (THREE_X ? (size_t)2 * W * hp + (size_t)2 * W * s2 : 0);
    if (lds > kLdsMax) { pclip_set_error("pclip_adapter_conv_w_f16: %zu bytes of LDS at width %d, D=%d", lds, W, D); return PCLIP_E_INVALID; }
    static DevOnce once;
    if (int e = pclip_raise_lds(once, {(const void*)adapter_conv_w_kernel<W, THREE_X>}, (int)kLdsMax, "pclip_adapter_conv_w_f16")) return e;
    const int cus = pclip_cus();
    const int grid = B < 2 * cus ? B : 2 * cus;                   // persistent over rows; two workgroups share a CU where their LDS allows it
    adapter_conv_w_kernel<W, THREE_X><<<grid, 256, lds, st>>>((const half_t*)x, B, D, s, (const half_t*)conv1, (const half_t*)ln1w, (const half_t*)ln1b,
        (const half_t*)conv2, (const half_t*)ln2w, (const half_t*)ln2b, (const half_t*)conv3, (const half_t*)ln3w, (const half_t*)ln3b, l2norm_out, (half_t*)y, y_sq);
    return pclip_check_launch("adapter_conv_w");
}

template <int W, bool THREE_X>
int launch_backward(const void* x, const void* g, int B, int D, const void* conv1, const void* ln1w, const void* ln1b, const void* conv2, const void* ln2w,
                    const void* ln2b, const void* conv3, const void* ln3w, float* pw1, float* pw2, float* pw3, float* pg1, float* pb1, float* pg2, float* pb2,
                    float* pg3, float* pb3, hipStream_t st) {
    const int s = side_of(D), hp = (s + 2) * (s + 2);
    const size_t lds = (size_t)(1024 + 1024 + 4 + 4 * W) * 4 + (THREE_X ? (size_t)2 * 2 * W * hp : 0);
    if (lds > kLdsMax) { pclip_set_error("pclip_adapter_conv_w_backward_f16: %zu bytes of LDS at width %d, D=%d", lds, W, D); return PCLIP_E_INVALID; }
    static DevOnce once;
    if (int e = pclip_raise_lds(once, {(const void*)adapter_conv_w_backward_kernel<W, THREE_X>}, (int)kLdsMax, "pclip_adapter_conv_w_backward_f16")) return e;
    adapter_conv_w_backward_kernel<W, THREE_X><<<B, 256, lds, st>>>((const half_t*)x, (const half_t*)g, D, s, (const half_t*)conv1, (const half_t*)ln1w,
        (const half_t*)ln1b, (const half_t*)conv2, (const half_t*)ln2w, (const half_t*)ln2b, (const half_t*)conv3, (const half_t*)ln3w, pw1, pw2, pw3, pg1, pb1,
        pg2, pb2, pg3, pb3);
    return pclip_check_launch("adapter_conv_w_backward");
}

}  // namespace

extern "C" int pclip_adapter_conv_w_f16(const void* x, int B, int D, int three_x, int width, const void* conv1, const void* ln1w, const void* ln1b,
                                        const void* conv2, const void* ln2w, const void* ln2b, const void* conv3, const void* ln3w, const void* ln3b,
                                        int l2norm_out, void* y, float* y_sq, pclip_stream_t stream) {
    PCLIP_REQUIRE(width_ok(width), "pclip_adapter_conv_w_f16: width=%d is not one of 8, 16, 24, 32", width);
    if (width == 16) return pclip_adapter_conv_f16(x, B, D, three_x, conv1, ln1w, ln1b, conv2, ln2w, ln2b, conv3, ln3w, ln3b, l2norm_out, y, y_sq, stream);
    PCLIP_REQUIRE(x && conv1 && ln1w && ln1b && conv3 && ln3w && ln3b && y, "pclip_adapter_conv_w_f16: null pointer");
    PCLIP_REQUIRE(!three_x || (conv2 && ln2w && ln2b), "pclip_adapter_conv_w_f16: conv-3x needs conv2/bn2 parameters");
    PCLIP_REQUIRE(B >= 0 && D > 0 && D <= 1024, "pclip_adapter_conv_w_f16: D=%d must be in (0, 1024]", D);
    if (B == 0) return PCLIP_OK;
    hipStream_t st = (hipStream_t)stream;
#define PCLIP_ADAPTER_W(WIDTH)                                                                                                                             \
    case WIDTH:                                                                                                                                             \
        return three_x ? launch_forward<WIDTH, true>(x, B, D, conv1, ln1w, ln1b, conv2, ln2w, ln2b, conv3, ln3w, ln3b, l2norm_out, y, y_sq, st)             \
                       : launch_forward<WIDTH, false>(x, B, D, conv1, ln1w, ln1b, nullptr, nullptr, nullptr, conv3, ln3w, ln3b, l2norm_out, y, y_sq, st);
    switch (width) { PCLIP_ADAPTER_W(8) PCLIP_ADAPTER_W(24) PCLIP_ADAPTER_W(32) }
#undef PCLIP_ADAPTER_W
    return PCLIP_E_INVALID;
}

extern "C" int pclip_adapter_conv_w_backward_partials(int B, int D, int three_x, int width) {
    return width == 16 ? pclip_adapter_conv_backward_partials(B, D, three_x) : B;
}

extern "C" int pclip_adapter_conv_w_backward_f16(const void* x, const void* g, int B, int D, int three_x, int width, const void* conv1, const void* ln1w,
                                                 const void* ln1b, const void* conv2, const void* ln2w, const void* ln2b, const void* conv3,
                                                 const void* ln3w, float* pw1, float* pw2, float* pw3, float* pg1, float* pb1, float* pg2, float* pb2,
                                                 float* pg3, float* pb3, pclip_stream_t stream) {
    PCLIP_REQUIRE(width_ok(width), "pclip_adapter_conv_w_backward_f16: width=%d is not one of 8, 16, 24, 32", width);
    if (width == 16)
        return pclip_adapter_conv_backward_f16(x, g, B, D, three_x, conv1, ln1w, ln1b, conv2, ln2w, ln2b, conv3, ln3w, pw1, pw2, pw3, pg1, pb1, pg2, pb2, pg3, pb3, stream);
    PCLIP_REQUIRE(x && g && conv1 && ln1w && ln1b && conv3 && ln3w && pw1 && pw3 && pg1 && pb1 && pg3 && pb3, "pclip_adapter_conv_w_backward_f16: null pointer");
    PCLIP_REQUIRE(!three_x || (conv2 && ln2w && ln2b && pw2 && pg2 && pb2), "pclip_adapter_conv_w_backward_f16: conv-3x needs conv2 / bn2 and their outputs");
    PCLIP_REQUIRE(B >= 0 && D > 0 && D <= 1024, "pclip_adapter_conv_w_backward_f16: D=%d must be in [1, 1024]", D);
    if (B == 0) return PCLIP_OK;
    hipStream_t st = (hipStream_t)stream;
#define PCLIP_ADAPTER_W(WIDTH)                                                                                                                             \
    case WIDTH:                                                                                                                                             \
        return three_x ? launch_backward<WIDTH, true>(x, g, B, D, conv1, ln1w, ln1b, conv2, ln2w, ln2b, conv3, ln3w, pw1, pw2, pw3, pg1, pb1, pg2, pb2, pg3, pb3, st) \
                       : launch_backward<WIDTH, false>(x, g, B, D, conv1, ln1w, ln1b, nullptr, nullptr, nullptr, conv3, ln3w, pw1, nullptr, pw3, pg1, pb1, nullptr, nullptr, pg3, pb3, st);
    switch (width) { PCLIP_ADAPTER_W(8) PCLIP_ADAPTER_W(24) PCLIP_ADAPTER_W(32) }
#undef PCLIP_ADAPTER_W
    return PCLIP_E_INVALID;
}
