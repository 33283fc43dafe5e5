// Feature-consistency regularisers: the distance of L2-normalised tower outputs from a constant target, forward and backward in one row pass each.
//   PCLIP_FREG_L1   PromptSRC's  F.l1_loss(x / x.norm(dim=-1, keepdim=True), t', reduction="mean")
//   PCLIP_FREG_COS  KgCoOp's     1 - mean(cosine_similarity(x, t'))
// x [M, D] fp16 (rows ldx apart) is un-normalised; t [M, D] fp16 (rows ldt apart) is a constant, taken as it is or, under normalize_t, normalised as x is.
// Bandwidth-trivial: at the sizes of a prompt-learning step (4 .. 1000 rows of 512) the time is the launches — two forward (rows, then the loss), one backward.
//
// One wave per row, four rows per workgroup; lane l owns the 16-byte vectors v = l, l + 64, l + 128, .. (v < D / 8) of its row, held in registers between the
// norm and the terms, so x and t are read once per call.  No atomics, no hand-over between workgroups; a row's numbers depend on that row of x and t, the
// mode, the flag and (backward) `weight` alone: not on M, the row's index, the grid, or how many vectors a lane is compiled to hold.
//
// Every operation below is ONE correctly rounded fp32 operation (the file is compiled with -ffp-contract=off: no multiply is fused into an addition; sqrtf and
// the division are hipcc's correctly rounded ones); f32(fp16) is exact.  Nothing is rounded to fp16 anywhere.
//
// LANE SUM of a quantity q_d over a row: each lane adds its own columns in ascending order into one accumulator that starts at +0,
//     p_l = (..((0 + q_{8 l}) + q_{8 l + 1}) + .. + q_{8 l + 7}) + q_{8 (l + 64)}) + ..      (a lane without a vector keeps +0)
// then the WAVE BUTTERFLY  p_l <- p_l + p_{l ^ 32};  then ^ 16, ^ 8, ^ 4, ^ 2, ^ 1  — every lane ends with the same bits.  Written S_d q_d below.
//
// The row's operands (the same instruction sequence in the forward and in the backward, and for t under normalize_t as for x):
//     ss   = S_d (f32(x_d) * f32(x_d))           (each square is exact in fp32)
//     inv  = 1 / sqrt(ss)                         inv_norm[m]; a zero row: ss = 0, inv = +inf, n = 0 * inf = NaN in every column
//     n_d  = f32(x_d) * inv
//     t'_d = f32(t_d)            or, normalize_t:  f32(t_d) * (1 / sqrt(S_d f32(t_d)^2))
// Forward:
//     L1:   rows[m] = S_d |n_d - t'_d|
//     COS:  rows[m] = 1 - S_d (n_d * t'_d)
//     loss  = r32( f64(R) / denom ),  denom = M D (L1) or M (COS), the division in double;  R = the BLOCK SUM of rows[0 .. M):
//     BLOCK SUM of a[0 .. n): thread i of 256 adds a[i], a[i + 256], .. in ascending order into one accumulator that starts at +0; the wave butterfly in each
//     of the four waves; then ((w0 + w1) + w2) + w3.  M <= PCLIP_FREG_CHUNK = 1024 rows: R is the block sum of rows.  Beyond: part[c] = the block sum of
//     rows[1024 c .. min(M, 1024 (c + 1))) for every chunk c (one workgroup per chunk, into the workspace), and R = the block sum of part[0 .. ceil(M / 1024)).
// Backward (dx [M, D] fp32, dense), weight = grad / (mean_over D) for L1, grad / mean_over for COS, rounded once to fp32 by the caller:
//     L1:   dn_d = +weight where n_d - t'_d > 0, -weight where < 0, +0 where it is 0 (or NaN)      — the sign of the very difference the forward summed
//     COS:  dn_d = (-weight) * t'_d
//     dot  = S_d (n_d * dn_d)
//     dx_d = (dn_d - n_d * dot) * inv
// A NaN (a zero row) stays in that row's term, that row of dx, and the loss.
#include "pclip_common.h"

#include <math.h>

namespace {
constexpr int ROWS_PER_WG = 4;

// the vectors a lane owns, loaded once: NV = the most a lane holds (D <= 512 NV)
template <int NV>
__device__ __forceinline__ void load_row(const half_t* __restrict__ p, int nvec, int lane, half8_t (&v)[NV]) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        if (c < nvec) v[i] = ld_half8(p + (size_t)c * 8);
    }
}

template <int NV>
__device__ __forceinline__ float inv_norm_of(const half8_t (&v)[NV], int nvec, int lane) {
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if (lane + 64 * i < nvec) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float f = (float)v[i][k];
                acc = acc + f * f;
            }
        }
    }
    return 1.0f / sqrtf(wave_sum(acc));
}

// n_d and t'_d of column k of the lane's vector i
#define FREG_ND(i, k) ((float)xv[i][k] * inv)
#define FREG_TD(i, k) (NORM_T ? (float)tv[i][k] * tinv : (float)tv[i][k])

template <int NV, int MODE, bool NORM_T>
__global__ __launch_bounds__(64 * ROWS_PER_WG) void freg_fwd_kernel(const half_t* __restrict__ x, int ldx, const half_t* __restrict__ t, int ldt, int M, int D,
                                                                    float* __restrict__ rows, float* __restrict__ inv_norm) {
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * ROWS_PER_WG + (threadIdx.x >> 6);
    if (m >= M) return;                                                  // (wave-uniform)
    const int nvec = D / 8;
    half8_t xv[NV], tv[NV];
    load_row<NV>(x + (size_t)m * ldx, nvec, lane, xv);
    load_row<NV>(t + (size_t)m * ldt, nvec, lane, tv);
    const float inv = inv_norm_of<NV>(xv, nvec, lane);
    const float tinv = NORM_T ? inv_norm_of<NV>(tv, nvec, lane) : 1.f;
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if (lane + 64 * i < nvec) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float n = FREG_ND(i, k), tt = FREG_TD(i, k);
                if (MODE == PCLIP_FREG_L1) acc = acc + fabsf(n - tt);
                else acc = acc + n * tt;
            }
        }
    }
    acc = wave_sum(acc);
    if (lane == 0) {
        rows[m] = MODE == PCLIP_FREG_L1 ? acc : 1.f - acc;
        inv_norm[m] = inv;
    }
}

template <int NV, int MODE, bool NORM_T>
__global__ __launch_bounds__(64 * ROWS_PER_WG) void freg_bwd_kernel(const half_t* __restrict__ x, int ldx, const half_t* __restrict__ t, int ldt, int M, int D,
                                                                    float weight, float* __restrict__ dx) {
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * ROWS_PER_WG + (threadIdx.x >> 6);
    if (m >= M) return;
    const int nvec = D / 8;
    half8_t xv[NV], tv[NV];
    load_row<NV>(x + (size_t)m * ldx, nvec, lane, xv);
    load_row<NV>(t + (size_t)m * ldt, nvec, lane, tv);
    const float inv = inv_norm_of<NV>(xv, nvec, lane);
    const float tinv = NORM_T ? inv_norm_of<NV>(tv, nvec, lane) : 1.f;
    const float nweight = -weight;
    auto dn_of = [&](float n, float tt) -> float {
        if (MODE == PCLIP_FREG_L1) {
            const float d = n - tt;
            return d > 0.f ? weight : (d < 0.f ? nweight : 0.f);
        }
        return nweight * tt;
    };
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if (lane + 64 * i < nvec) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float n = FREG_ND(i, k);
                acc = acc + n * dn_of(n, FREG_TD(i, k));
            }
        }
    }
    const float dot = wave_sum(acc);
    float* out = dx + (size_t)m * D;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        if (c < nvec) {
            float4_t o[2];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float n = FREG_ND(i, k);
                o[k >> 2][k & 3] = (dn_of(n, FREG_TD(i, k)) - n * dot) * inv;
            }
            reinterpret_cast<float4_t*>(out + (size_t)c * 8)[0] = o[0];
            reinterpret_cast<float4_t*>(out + (size_t)c * 8)[1] = o[1];
        }
    }
}
#undef FREG_ND
#undef FREG_TD

// the BLOCK SUM of a[0 .. n) by one workgroup of 256 threads; the result in every thread of wave 0
__device__ __forceinline__ float block_sum(const float* __restrict__ a, long n, float* lds4) {
    float acc = 0.f;
    for (long i = threadIdx.x; i < n; i += 256) acc = acc + a[i];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = acc;
    __syncthreads();
    return ((lds4[0] + lds4[1]) + lds4[2]) + lds4[3];
}

// grid = chunks: part[c] = block sum of rows[CHUNK c ..)
__global__ __launch_bounds__(256) void freg_chunk_kernel(const float* __restrict__ rows, int M, float* __restrict__ part) {
    __shared__ float lds4[4];
    const long r0 = (long)blockIdx.x * PCLIP_FREG_CHUNK;
    const long n = M - r0 < PCLIP_FREG_CHUNK ? M - r0 : PCLIP_FREG_CHUNK;
    const float s = block_sum(rows + r0, n, lds4);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// one workgroup: loss = r32(f64(block sum of a[0 .. n)) / denom)
__global__ __launch_bounds__(256) void freg_loss_kernel(const float* __restrict__ a, int n, double denom, float* __restrict__ loss) {
    __shared__ float lds4[4];
    const float s = block_sum(a, n, lds4);
    if (threadIdx.x == 0) loss[0] = (float)((double)s / denom);
}

int chunks_of(int M) { return (int)(((long)M + PCLIP_FREG_CHUNK - 1) / PCLIP_FREG_CHUNK); }
int grid_of(int M) { return (int)(((long)M + ROWS_PER_WG - 1) / ROWS_PER_WG); }

int nv_of(int D) {
    const int per_lane = (D / 8 + 63) / 64;
    return per_lane <= 1 ? 1 : (per_lane <= 2 ? 2 : (per_lane <= 4 ? 4 : 8));
}

int check_operands(const char* who, const void* x, int ldx, const void* t, int ldt, int M, int D, int mode, int normalize_t) {
    PCLIP_REQUIRE(D >= 8 && D <= 4096 && D % 8 == 0, "%s: D=%d must be a multiple of 8 in 8..4096", who, D);
    PCLIP_REQUIRE(M >= 0, "%s: M=%d must not be negative", who, M);
    PCLIP_REQUIRE(mode == PCLIP_FREG_L1 || mode == PCLIP_FREG_COS, "%s: mode=%d is neither PCLIP_FREG_L1 (0) nor PCLIP_FREG_COS (1)", who, mode);
    PCLIP_REQUIRE(normalize_t == 0 || normalize_t == 1, "%s: normalize_t=%d must be 0 or 1", who, normalize_t);
    PCLIP_REQUIRE(ldx % 8 == 0 && ldx >= D, "%s: ldx=%d must be a multiple of 8 halves and at least D=%d", who, ldx, D);
    PCLIP_REQUIRE(ldt % 8 == 0 && ldt >= D, "%s: ldt=%d must be a multiple of 8 halves and at least D=%d", who, ldt, D);
    if (M == 0) return PCLIP_OK;
    PCLIP_REQUIRE(x && t, "%s: null operand", who);
    PCLIP_REQUIRE(((uintptr_t)x | (uintptr_t)t) % 16 == 0, "%s: x and t must be 16-byte aligned", who);
    return PCLIP_OK;
}

#define FREG_LAUNCH(KERNEL, ...)                                                                                             \
    do {                                                                                                                     \
        const int key = nv * 4 + mode * 2 + normalize_t;                                                                     \
        switch (key) {                                                                                                       \
            FREG_CASE(KERNEL, 1, __VA_ARGS__) FREG_CASE(KERNEL, 2, __VA_ARGS__) FREG_CASE(KERNEL, 4, __VA_ARGS__) FREG_CASE(KERNEL, 8, __VA_ARGS__) \
        }                                                                                                                    \
    } while (0)
#define FREG_CASE(KERNEL, NV, ...)                                                                                           \
    case NV * 4 + 0: KERNEL<NV, PCLIP_FREG_L1, false><<<grid, 64 * ROWS_PER_WG, 0, s>>>(__VA_ARGS__); break;                  \
    case NV * 4 + 1: KERNEL<NV, PCLIP_FREG_L1, true><<<grid, 64 * ROWS_PER_WG, 0, s>>>(__VA_ARGS__); break;                   \
    case NV * 4 + 2: KERNEL<NV, PCLIP_FREG_COS, false><<<grid, 64 * ROWS_PER_WG, 0, s>>>(__VA_ARGS__); break;                 \
    case NV * 4 + 3: KERNEL<NV, PCLIP_FREG_COS, true><<<grid, 64 * ROWS_PER_WG, 0, s>>>(__VA_ARGS__); break;
}  // namespace

extern "C" size_t pclip_feature_reg_workspace(int M) {
    return M > PCLIP_FREG_CHUNK ? align_up((size_t)chunks_of(M) * sizeof(float), 256) : 0;
}

extern "C" int pclip_feature_reg_f16(const void* x, int ldx, const void* t, int ldt, int M, int D, int mode, int normalize_t, float* loss, float* rows,
                                     float* inv_norm, void* ws, size_t ws_bytes, pclip_stream_t stream) {
    const char* who = "pclip_feature_reg_f16";
    if (int rc = check_operands(who, x, ldx, t, ldt, M, D, mode, normalize_t)) return rc;
    PCLIP_REQUIRE(loss, "%s: loss is required", who);
    hipStream_t s = (hipStream_t)stream;
    if (M == 0) {                                                        // an empty batch: +0, no launch
        if (hipMemsetAsync(loss, 0, sizeof(float), s) != hipSuccess) {
            pclip_set_error("%s: cannot clear the loss", who);
            return PCLIP_E_LAUNCH;
        }
        return PCLIP_OK;
    }
    PCLIP_REQUIRE(rows && inv_norm, "%s: rows and inv_norm are required", who);
    const size_t need = pclip_feature_reg_workspace(M);
    if (need) {
        PCLIP_REQUIRE(ws, "%s: M=%d rows need a workspace of %zu bytes (pclip_feature_reg_workspace)", who, M, need);
        if (ws_bytes < need) {
            pclip_set_error("%s: workspace of %zu bytes, %zu needed", who, ws_bytes, need);
            return PCLIP_E_WORKSPACE;
        }
    }
    const int nv = nv_of(D), grid = grid_of(M);
    FREG_LAUNCH(freg_fwd_kernel, (const half_t*)x, ldx, (const half_t*)t, ldt, M, D, rows, inv_norm);
    const double denom = mode == PCLIP_FREG_L1 ? (double)M * (double)D : (double)M;
    if (need) {
        const int chunks = chunks_of(M);
        freg_chunk_kernel<<<chunks, 256, 0, s>>>(rows, M, (float*)ws);
        freg_loss_kernel<<<1, 256, 0, s>>>((const float*)ws, chunks, denom, loss);
    } else {
        freg_loss_kernel<<<1, 256, 0, s>>>(rows, M, denom, loss);
    }
    return pclip_check_launch(who);
}

extern "C" int pclip_feature_reg_backward_f16(const void* x, int ldx, const void* t, int ldt, int M, int D, int mode, int normalize_t, float weight, float* dx,
                                              pclip_stream_t stream) {
    const char* who = "pclip_feature_reg_backward_f16";
    if (int rc = check_operands(who, x, ldx, t, ldt, M, D, mode, normalize_t)) return rc;
    if (M == 0) return PCLIP_OK;
    PCLIP_REQUIRE(dx, "%s: dx is required", who);
    PCLIP_REQUIRE((uintptr_t)dx % 16 == 0, "%s: dx must be 16-byte aligned", who);
    hipStream_t s = (hipStream_t)stream;
    const int nv = nv_of(D), grid = grid_of(M);
    FREG_LAUNCH(freg_bwd_kernel, (const half_t*)x, ldx, (const half_t*)t, ldt, M, D, weight, dx);
    return pclip_check_launch(who);
}
