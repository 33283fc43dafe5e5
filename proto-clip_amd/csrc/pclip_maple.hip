// MaPLe (multi-modal prompt learning): learned fp32 rows at an OFFSET inside a sequence (the text tower's context rows sit at positions 1 .. n_ctx of a
// causal sequence, not behind it), and the per-depth linear coupling function that maps each layer's text rows to that layer's visual prompt rows, with
// its gradients.  No atomics, no hand-over between workgroups: every sum has one fixed order and two calls give the same bits.
//
// ---- prompt rows at an offset ------------------------------------------------------------------------------------------------------------------------
// pclip_rows_replace_f16 / pclip_rows_grad_f32: the replace and the slice-sum walk of pclip_rows.h with L, off and P independent
// (0 <= off, off + P <= L <= PCLIP_VPT_MAX_L); rounding points, summation order and `clear` are stated there.  The row kernels hold no multiplication,
// so they are indifferent to this file's contraction setting.
//
// ---- the coupling function, fp32, all depths in one launch -----------------------------------------------------------------------------------------------
// Y[d] = X[d] Wc[d]^T + bc[d]:  X [depth, P, Wt] (text rows), Wc [depth, Wv, Wt], bc [depth, Wv], Y [depth, P, Wv] (visual rows).
// Envelope: depth >= 1, 1 <= P <= PCLIP_COUPLE_MAX_P = 16, Wt % 64 == 0, Wv % 8 == 0.  Weight-streaming kernels: Wc is read once by the forward and once
// by the backward (by the dX pass; dWc is written once), in 16-byte vectors that a wave reads as whole 256-byte row segments.
//
// Rounding points / summation order.  Everything is fp32.  A product is rounded on its own (one fp32 multiplication) and then added (one rounded fp32
// addition): this file is compiled without floating-point contraction, there is no fused multiply-add in it.  Every accumulator starts at +0.
//   forward, Y[d][p][v]: 16 lanes share the row Wc[d][v][:]; lane l (0 .. 15) owns columns t = 64 k + 4 l + j, j = 0 .. 3, k = 0 .. Wt / 64 - 1, and walks
//     them in ascending k, then ascending j, into one accumulator:
//       a_l = (..(((0 + X[p][4l] W[v][4l]) + X[p][4l + 1] W[v][4l + 1]) + .. + X[p][4l + 3] W[v][4l + 3]) + X[p][64 + 4l] W[v][64 + 4l]) + ..)
//     the 16 lane sums are combined by a butterfly at distances 8, 4, 2, 1:  a_l <- a_l + a_(l xor 8);  a_l <- a_l + a_(l xor 4);  a_l <- a_l + a_(l xor 2);
//     a_l <- a_l + a_(l xor 1)   (fp32 addition commutes, so all 16 lanes hold the same bits);  Y = a + bc[d][v], the bias added LAST.
//     Rounded operations on the path of one term: 1 product, at most Wt / 16 chain additions, 4 butterfly additions, 1 bias addition.
//   dWc[d][v][t] = (..((0 + dY[d][0][v] X[d][0][t]) + dY[d][1][v] X[d][1][t]) + ..)       ascending p, one accumulator  (1 product + P additions)
//   dbc[d][v]    = (..((0 + dY[d][0][v]) + dY[d][1][v]) + ..)                             ascending p, one accumulator  (P additions)
//   dX[d][p][t]: the Wv rows of Wc[d] are cut into slices of PCLIP_COUPLE_SLICE = 32 consecutive rows (the last one may be short); v0 = 32 s;
//     part[d][s][p][t] = (..((0 + dY[d][p][v0] Wc[d][v0][t]) + dY[d][p][v0 + 1] Wc[d][v0 + 1][t]) + ..)    ascending v inside the slice, one accumulator
//     dX[d][p][t]      = (..((part[d][0][p][t] + part[d][1][p][t]) + part[d][2][p][t]) + ..)                ascending slice order, starting from slice 0
//     One slice (Wv <= 32): part is dX itself and there is no merge launch.  (1 product + at most 32 additions + nslice - 1 merges)
// Launches: forward 1; backward at most 2 (dWc with dbc; dX partials) + 1 merge, for any depth.
#include "pclip_rows.h"

#pragma clang fp contract(off)

namespace {
// the envelope both row entries share; 0 = fine
int rows_envelope(const char* who, int B, int L, int off, int P, int W) {
    PCLIP_REQUIRE(W > 0 && W % 8 == 0, "%s: W=%d must be a positive multiple of 8 (16-byte vectors)", who, W);
    PCLIP_REQUIRE(P >= 1 && off >= 0 && B >= 0 && L >= 1, "%s: bad shape B=%d L=%d off=%d P=%d (B >= 0, L >= 1, off >= 0, P >= 1)", who, B, L, off, P);
    PCLIP_REQUIRE((long long)off + P <= L, "%s: rows off .. off + P - 1 = %d .. %lld do not lie inside a sequence of L=%d rows", who, off,
                  (long long)off + P - 1, L);
    PCLIP_REQUIRE(L <= PCLIP_VPT_MAX_L, "%s: L = %d tokens exceed the attention envelope of %d", who, L, PCLIP_VPT_MAX_L);
    PCLIP_REQUIRE((unsigned long long)B * (unsigned long long)L * (unsigned long long)W <= 2147483647ull, "%s: B * L * W = %d * %d * %d does not fit an int",
                  who, B, L, W);
    return PCLIP_OK;
}

// ---- coupling ----------------------------------------------------------------------------------------------------------------------------------------

constexpr int MAXP = PCLIP_COUPLE_MAX_P;

// a quarter wave (16 lanes) per row v of Wc[d]: four rows per wave, 16 rows per 256-thread block; grid (ceil(Wv / 16), depth)
__global__ __launch_bounds__(256) void couple_fwd_kernel(const float* __restrict__ X, const float* __restrict__ Wc, const float* __restrict__ bc, int P,
                                                         int Wt, int Wv, float* __restrict__ Y) {
    const int d = blockIdx.y, l = threadIdx.x & 15;
    const int v = blockIdx.x * 16 + (threadIdx.x >> 4);
    const int vr = v < Wv ? v : Wv - 1;                                      // a row past the end reads the last row and stores nothing
    const float* w = Wc + ((size_t)d * Wv + vr) * Wt + 4 * l;
    const float* x = X + (size_t)d * P * Wt + 4 * l;
    float acc[MAXP];
#pragma unroll
    for (int p = 0; p < MAXP; ++p) acc[p] = 0.f;
    for (int k = 0; k < Wt; k += 64) {
        const float4_t w4 = *reinterpret_cast<const float4_t*>(w + k);
#pragma unroll
        for (int p = 0; p < MAXP; ++p) {
            if (p < P) {
                const float4_t x4 = *reinterpret_cast<const float4_t*>(x + (size_t)p * Wt + k);
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
    for (int p = 0; p < MAXP; ++p) {
        if (p < P) {
            float s = acc[p];
            s = s + __shfl_xor(s, 8, 16);
            s = s + __shfl_xor(s, 4, 16);
            s = s + __shfl_xor(s, 2, 16);
            s = s + __shfl_xor(s, 1, 16);
            if (l == p) mine = s;
        }
    }
    if (l < P && v < Wv) Y[((size_t)d * P + l) * Wv + v] = mine + bc[(size_t)d * Wv + v];
}

// dWc and dbc: one thread per (d, v, 4 columns), flat over depth * Wv * Wt / 4; the thread of a row's first vector also sums the row's bias gradient
__global__ __launch_bounds__(256) void couple_dw_kernel(const float* __restrict__ dY, const float* __restrict__ X, int depth, int P, int Wt, int Wv,
                                                        float* __restrict__ dWc, float* __restrict__ dbc) {
    const int WT4 = Wt / 4;
    const size_t nvec = (size_t)depth * Wv * WT4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % WT4);
        const int v = (int)((i / WT4) % Wv);
        const size_t d = i / ((size_t)WT4 * Wv);
        const float* gy = dY + d * P * Wv + v;
        const float* x = X + d * P * Wt + 4 * c;
        float4_t acc = {0.f, 0.f, 0.f, 0.f};
        float b = 0.f;
        for (int p = 0; p < P; ++p) {
            const float g = gy[(size_t)p * Wv];
            const float4_t x4 = *reinterpret_cast<const float4_t*>(x + (size_t)p * Wt);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float prod = g * x4[j];
                acc[j] = acc[j] + prod;
            }
            b = b + g;
        }
        reinterpret_cast<float4_t*>(dWc)[i] = acc;
        if (dbc && c == 0) dbc[d * Wv + v] = b;
    }
}

// dbc alone (dWc not asked for): one thread per (d, v)
__global__ __launch_bounds__(256) void couple_db_kernel(const float* __restrict__ dY, int depth, int P, int Wv, float* __restrict__ dbc) {
    const size_t n = (size_t)depth * Wv;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const size_t d = i / Wv;
        const int v = (int)(i % Wv);
        const float* gy = dY + d * P * Wv + v;
        float b = 0.f;
        for (int p = 0; p < P; ++p) b = b + gy[(size_t)p * Wv];
        dbc[i] = b;
    }
}

// dX, first stage: one wave per (256-column panel, slice of 32 rows of Wc[d], d); a lane owns 4 columns and walks the slice's rows in ascending order;
// grid (ceil(Wt / 256), nslice, depth).  out: part [depth][nslice][P][Wt], or dX itself when nslice == 1
__global__ __launch_bounds__(64) void couple_dx_part_kernel(const float* __restrict__ dY, const float* __restrict__ Wc, int P, int Wt, int Wv, int nslice,
                                                            float* __restrict__ out) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (4 * c >= Wt) return;
    const int s = blockIdx.y, d = blockIdx.z;
    const int v0 = s * PCLIP_COUPLE_SLICE, v1 = v0 + PCLIP_COUPLE_SLICE < Wv ? v0 + PCLIP_COUPLE_SLICE : Wv;
    const float* w = Wc + ((size_t)d * Wv + v0) * Wt + 4 * c;
    const float* gy = dY + (size_t)d * P * Wv;
    float4_t acc[MAXP];
#pragma unroll
    for (int p = 0; p < MAXP; ++p) acc[p] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int v = v0; v < v1; ++v) {
        const float4_t w4 = *reinterpret_cast<const float4_t*>(w);
        w += Wt;
#pragma unroll
        for (int p = 0; p < MAXP; ++p) {
            if (p < P) {
                const float g = gy[(size_t)p * Wv + v];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float prod = g * w4[j];
                    acc[p][j] = acc[p][j] + prod;
                }
            }
        }
    }
    float* dst = out + (((size_t)d * nslice + s) * P) * Wt + 4 * c;
#pragma unroll
    for (int p = 0; p < MAXP; ++p)
        if (p < P) *reinterpret_cast<float4_t*>(dst + (size_t)p * Wt) = acc[p];
}

// dX[d][r] = (..(part[d][0][r] + part[d][1][r]) + ..), r over the P * Wt elements of a depth, four per thread
__global__ __launch_bounds__(256) void couple_dx_sum_kernel(const float* __restrict__ part, int depth, int nslice, size_t M, float* __restrict__ dX) {
    const size_t m4 = M / 4, nvec = (size_t)depth * m4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (size_t)gridDim.x * 256) {
        const size_t d = i / m4, r = i % m4;
        const float* src = part + d * nslice * M + 4 * r;
        float4_t acc = *reinterpret_cast<const float4_t*>(src);
#pragma unroll 8
        for (int s = 1; s < nslice; ++s) {
            const float4_t v = *reinterpret_cast<const float4_t*>(src + (size_t)s * M);
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] += v[k];
        }
        reinterpret_cast<float4_t*>(dX)[i] = acc;
    }
}

int couple_envelope(const char* who, int depth, int P, int Wt, int Wv) {
    PCLIP_REQUIRE(depth >= 1 && depth <= 65535, "%s: depth=%d outside 1 .. 65535", who, depth);
    PCLIP_REQUIRE(P >= 1 && P <= PCLIP_COUPLE_MAX_P, "%s: P=%d rows outside 1 .. %d", who, P, PCLIP_COUPLE_MAX_P);
    PCLIP_REQUIRE(Wt > 0 && Wt % 64 == 0, "%s: Wt=%d must be a positive multiple of 64 (a quarter wave reads 64 columns per step)", who, Wt);
    PCLIP_REQUIRE(Wv > 0 && Wv % 8 == 0, "%s: Wv=%d must be a positive multiple of 8", who, Wv);
    PCLIP_REQUIRE((unsigned long long)depth * (unsigned long long)Wv * (unsigned long long)Wt <= 2147483647ull,
                  "%s: depth * Wv * Wt = %d * %d * %d does not fit an int", who, depth, Wv, Wt);
    PCLIP_REQUIRE((Wv + PCLIP_COUPLE_SLICE - 1) / PCLIP_COUPLE_SLICE <= 65535, "%s: Wv=%d gives more than 65535 row slices", who, Wv);
    return PCLIP_OK;
}
}  // namespace

extern "C" int pclip_rows_replace_f16(void* x, const float* ctx, int B, int L, int off, int P, int W, pclip_stream_t stream) {
    PCLIP_REQUIRE(x && ctx, "pclip_rows_replace_f16: null pointer");
    if (int rc = rows_envelope("pclip_rows_replace_f16", B, L, off, P, W)) return rc;
    PCLIP_REQUIRE((((uintptr_t)x | (uintptr_t)ctx) & 15) == 0, "pclip_rows_replace_f16: operands must be 16-byte aligned");
    if (B == 0) return PCLIP_OK;
    return rows_replace("rows_replace", x, ctx, B, L, off, P, W, stream);
}

extern "C" int pclip_rows_grad_f32(void* g, int B, int L, int off, int P, int W, int clear, float* dctx, float* part, int nslice, pclip_stream_t stream) {
    PCLIP_REQUIRE(g && dctx, "pclip_rows_grad_f32: null pointer");
    if (int rc = rows_envelope("pclip_rows_grad_f32", B, L, off, P, W)) return rc;
    PCLIP_REQUIRE((((uintptr_t)g | (uintptr_t)dctx | (uintptr_t)part) & 15) == 0, "pclip_rows_grad_f32: operands must be 16-byte aligned");
    if (B == 0) return PCLIP_OK;
    const int want = (B + PCLIP_VPT_SLICE - 1) / PCLIP_VPT_SLICE;
    PCLIP_REQUIRE(nslice == want, "pclip_rows_grad_f32: nslice=%d, expected ceil(B / %d) = %d", nslice, PCLIP_VPT_SLICE, want);
    PCLIP_REQUIRE(nslice == 1 || part, "pclip_rows_grad_f32: %d sequence slices need the part buffer", nslice);
    return rows_grad<PCLIP_VPT_SLICE>("rows_grad", g, B, L, off, P, P, W, clear, nslice == 1 ? dctx : part, nslice, dctx, stream);
}

extern "C" int pclip_couple_fwd_f32(const float* X, const float* Wc, const float* bc, int depth, int P, int Wt, int Wv, float* Y, pclip_stream_t stream) {
    PCLIP_REQUIRE(X && Wc && bc && Y, "pclip_couple_fwd_f32: null pointer");
    if (int rc = couple_envelope("pclip_couple_fwd_f32", depth, P, Wt, Wv)) return rc;
    PCLIP_REQUIRE((((uintptr_t)X | (uintptr_t)Wc | (uintptr_t)bc | (uintptr_t)Y) & 15) == 0, "pclip_couple_fwd_f32: operands must be 16-byte aligned");
    couple_fwd_kernel<<<dim3((Wv + 15) / 16, depth), 256, 0, (hipStream_t)stream>>>(X, Wc, bc, P, Wt, Wv, Y);
    return pclip_check_launch("couple_fwd");
}

extern "C" int pclip_couple_bwd_f32(const float* dY, const float* X, const float* Wc, int depth, int P, int Wt, int Wv, float* dWc, float* dbc, float* dX,
                                    float* part, int nslice, pclip_stream_t stream) {
    PCLIP_REQUIRE(dY, "pclip_couple_bwd_f32: null pointer (dY)");
    PCLIP_REQUIRE(!dWc || X, "pclip_couple_bwd_f32: dWc needs X");
    PCLIP_REQUIRE(!dX || Wc, "pclip_couple_bwd_f32: dX needs Wc");
    if (int rc = couple_envelope("pclip_couple_bwd_f32", depth, P, Wt, Wv)) return rc;
    PCLIP_REQUIRE((((uintptr_t)dY | (uintptr_t)X | (uintptr_t)Wc | (uintptr_t)dWc | (uintptr_t)dbc | (uintptr_t)dX | (uintptr_t)part) & 15) == 0,
                  "pclip_couple_bwd_f32: operands must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (dWc)
        couple_dw_kernel<<<flat_grid((size_t)depth * Wv * (Wt / 4)), 256, 0, s>>>(dY, X, depth, P, Wt, Wv, dWc, dbc);
    else if (dbc)
        couple_db_kernel<<<flat_grid((size_t)depth * Wv), 256, 0, s>>>(dY, depth, P, Wv, dbc);
    if (dX) {
        const int want = (Wv + PCLIP_COUPLE_SLICE - 1) / PCLIP_COUPLE_SLICE;
        PCLIP_REQUIRE(nslice == want, "pclip_couple_bwd_f32: nslice=%d, expected ceil(Wv / %d) = %d", nslice, PCLIP_COUPLE_SLICE, want);
        PCLIP_REQUIRE(nslice == 1 || part, "pclip_couple_bwd_f32: %d row slices need the part buffer", nslice);
        couple_dx_part_kernel<<<dim3((Wt + 255) / 256, nslice, depth), 64, 0, s>>>(dY, Wc, P, Wt, Wv, nslice, nslice == 1 ? dX : part);
        if (nslice > 1) couple_dx_sum_kernel<<<flat_grid((size_t)depth * P * Wt / 4), 256, 0, s>>>(part, depth, nslice, (size_t)P * Wt, dX);
    }
    return pclip_check_launch("couple_bwd");
}
