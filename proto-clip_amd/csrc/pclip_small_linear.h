// A small fp32 linear layer over at most 16 input rows, defined once for MaPLe's coupling function (pclip_maple.hip: all depths in one launch) and for
// CoCoOp's meta-net (pclip_cocoop.hip: layer 1, and the weight / bias gradients of both layers): Y[d] = X[d] W[d]^T + b[d], optionally through a ReLU,
// with dW and db.  Weight-streaming kernels: W is read once, in 16-byte vectors that a wave reads as whole 256-byte row segments.  No atomics, no hand-over
// between workgroups: every sum has one fixed order and two calls give the same bits.
//
// Shapes: X [depth, P, K] fp32 or fp16 (f32(fp16) is exact), W [depth, R, K], b [depth, R], Y and dY [depth, P, R], dW [depth, R, K], db [depth, R];
// 1 <= P <= 16, K % 64 == 0 for the forward, K % 4 == 0 for dW.  The depth is blockIdx.y; the meta-net is depth 1.
//   MaPLe   P = the prompt rows, K = Wt, R = Wv
//   CoCoOp  P = the images B; layer 1: K = E, R = Hd, X = f (fp16), ReLU;  dW2, db2: dY = dpi, X = h, K = Hd, R = Wt;  dW1, db1: dY = dpre, X = f, K = E, R = Hd
//
// Rounding points / summation order.  Everything after f32(fp16) is fp32.  A product is rounded on its own (one fp32 multiplication) and then added (one
// rounded fp32 addition): include this header AFTER `#pragma clang fp contract(off)`, there is no fused multiply-add in these walks.  Every accumulator
// starts at +0.
//   forward, Y[d][p][r]: 16 lanes share the row W[d][r][:]; lane l (0 .. 15) owns columns c = 64 k + 4 l + j, j = 0 .. 3, k = 0 .. K / 64 - 1, and walks
//     them in ascending k, then ascending j, into one accumulator:
//       a_l = (..(((0 + X[p][4l] W[r][4l]) + X[p][4l + 1] W[r][4l + 1]) + .. + X[p][4l + 3] W[r][4l + 3]) + X[p][64 + 4l] W[r][64 + 4l]) + ..)
//     the 16 lane sums are combined by a butterfly at distances 8, 4, 2, 1:  a_l <- a_l + a_(l xor 8);  a_l <- a_l + a_(l xor 4);  a_l <- a_l + a_(l xor 2);
//     a_l <- a_l + a_(l xor 1)   (fp32 addition commutes, so all 16 lanes hold the same bits);  pre = a + b[d][r], the bias added LAST;
//     Y = pre, or with the ReLU +0 where pre <= 0, else pre (a NaN stays a NaN).
//     Rounded operations on the path of one term: 1 product, at most K / 16 chain additions, 4 butterfly additions, 1 bias addition.
//   dW[d][r][c] = (..((0 + dY[d][0][r] X[d][0][c]) + dY[d][1][r] X[d][1][c]) + ..)        ascending p, one accumulator  (1 product + P additions)
//   db[d][r]    = (..((0 + dY[d][0][r]) + dY[d][1][r]) + ..)                              ascending p, one accumulator  (P additions)
#pragma once
#include "pclip_rows.h"

namespace {
// the forward's store `if (l == p)` hands row p's sum to lane p of the quarter wave: the capacity IS the 16 lanes
constexpr int SMALL_LINEAR_MAX_P = 16;
static_assert(PCLIP_COUPLE_MAX_P == 16 && PCLIP_COCOOP_MAX_B == 16, "rowdot16_kernel holds one row of X per lane of a quarter wave");

__device__ __forceinline__ float4_t ld_f32x4(const float* p) { return *reinterpret_cast<const float4_t*>(p); }
__device__ __forceinline__ float4_t ld_f32x4(const half_t* p) {
    const half4_t v = *reinterpret_cast<const half4_t*>(p);
    return float4_t{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}

// forward: a quarter wave (16 lanes) per row r of W[d]: four rows per wave, 16 rows per 256-thread block; grid (ceil(R / 16), depth).  DEEP = false is
// depth 1 known at compile time: the depth's base offset on each of the 16 row pointers is 32 scalar instructions per step of 64 columns otherwise
template <typename XT, bool RELU, bool DEEP>
__global__ __launch_bounds__(256) void rowdot16_kernel(const XT* __restrict__ X, const float* __restrict__ W, const float* __restrict__ b, int P, int K, int R,
                                                       float* __restrict__ Y) {
    const int d = DEEP ? blockIdx.y : 0, l = threadIdx.x & 15;
    const int r = blockIdx.x * 16 + (threadIdx.x >> 4);
    const int rr = r < R ? r : R - 1;                                        // a row past the end reads the last row and stores nothing
    const float* w = W + ((size_t)d * R + rr) * K + 4 * l;
    const XT* x = X + (size_t)d * P * K + 4 * l;
    float acc[SMALL_LINEAR_MAX_P];
#pragma unroll
    for (int p = 0; p < SMALL_LINEAR_MAX_P; ++p) acc[p] = 0.f;
    for (int k = 0; k < K; k += 64) {
        const float4_t w4 = ld_f32x4(w + k);
#pragma unroll
        for (int p = 0; p < SMALL_LINEAR_MAX_P; ++p) {
            if (p < P) {
                const float4_t x4 = ld_f32x4(x + (size_t)p * K + k);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float prod = x4[j] * w4[j];
                    acc[p] = acc[p] + prod;
                }
            }
        }
    }
    float mine = 0.f;
#pragma unroll
    for (int p = 0; p < SMALL_LINEAR_MAX_P; ++p) {
        if (p < P) {
            float s = acc[p];
            s = s + __shfl_xor(s, 8, 16);
            s = s + __shfl_xor(s, 4, 16);
            s = s + __shfl_xor(s, 2, 16);
            s = s + __shfl_xor(s, 1, 16);
            if (l == p) mine = s;
        }
    }
    if (l < P && r < R) {
        const float pre = mine + b[(size_t)d * R + r];
        Y[((size_t)d * P + l) * R + r] = RELU && pre <= 0.f ? 0.f : pre;
    }
}

// dW and db: one thread per (r, 4 columns), flat over R * K / 4, the depth in blockIdx.y; the thread of a row's first vector also sums the row's bias
// gradient (db may be null)
template <typename XT>
__global__ __launch_bounds__(256) void small_linear_dw_kernel(const float* __restrict__ dY, const XT* __restrict__ X, int P, int R, int K,
                                                              float* __restrict__ dW, float* __restrict__ db) {
    const size_t d = blockIdx.y;
    dY += d * P * R;
    X += d * P * K;
    const int K4 = K / 4;
    const size_t nvec = (size_t)R * K4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % K4);
        const int r = (int)(i / K4);
        float4_t acc = {0.f, 0.f, 0.f, 0.f};
        float s = 0.f;
        for (int p = 0; p < P; ++p) {
            const float g = dY[(size_t)p * R + r];
            const float4_t x4 = ld_f32x4(X + (size_t)p * K + 4 * c);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float prod = g * x4[j];
                acc[j] = acc[j] + prod;
            }
            s = s + g;
        }
        reinterpret_cast<float4_t*>(dW + d * R * K)[i] = acc;
        if (db && c == 0) db[d * R + r] = s;
    }
}

// db alone (dW not asked for): one thread per r, the depth in blockIdx.y.  (A template only so that a unit which never launches it does not emit it.)
template <int = 0>
__global__ __launch_bounds__(256) void small_linear_db_kernel(const float* __restrict__ dY, int P, int R, float* __restrict__ db) {
    const size_t d = blockIdx.y;
    dY += d * P * R;
    for (size_t r = (size_t)blockIdx.x * 256 + threadIdx.x; r < (size_t)R; r += (size_t)gridDim.x * 256) {
        float s = 0.f;
        for (int p = 0; p < P; ++p) s = s + dY[(size_t)p * R + r];
        db[d * R + r] = s;
    }
}
}  // namespace
