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
//   forward Y, dWc and dbc: the small linear layer of pclip_small_linear.h (X fp32, no ReLU, K = Wt, R = Wv); the walks are stated there.
//   dX[d][p][t]: the Wv rows of Wc[d] are cut into slices of PCLIP_COUPLE_SLICE = 32 consecutive rows (the last one may be short); v0 = 32 s;
//     part[d][s][p][t] = (..((0 + dY[d][p][v0] Wc[d][v0][t]) + dY[d][p][v0 + 1] Wc[d][v0 + 1][t]) + ..)    ascending v inside the slice, one accumulator
//     dX[d][p][t]      = (..((part[d][0][p][t] + part[d][1][p][t]) + part[d][2][p][t]) + ..)                ascending slice order, starting from slice 0
//     (the merge of pclip_rows.h, one group per depth).  One slice (Wv <= 32): part is dX itself and there is no merge launch.
//     (1 product + at most 32 additions + nslice - 1 merges)
// Launches: forward 1; backward at most 2 (dWc with dbc; dX partials) + 1 merge, for any depth.
#include "pclip_rows.h"

#pragma clang fp contract(off)

#include "pclip_small_linear.h"

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
    rowdot16_kernel<float, false, true><<<dim3((Wv + 15) / 16, depth), 256, 0, (hipStream_t)stream>>>(X, Wc, bc, P, Wt, Wv, Y);
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
        small_linear_dw_kernel<float><<<dim3(flat_grid((size_t)Wv * (Wt / 4)), depth), 256, 0, s>>>(dY, X, P, Wv, Wt, dWc, dbc);
    else if (dbc)
        small_linear_db_kernel<><<<dim3(flat_grid((size_t)Wv), depth), 256, 0, s>>>(dY, P, Wv, dbc);
    if (dX) {
        const int want = (Wv + PCLIP_COUPLE_SLICE - 1) / PCLIP_COUPLE_SLICE;
        PCLIP_REQUIRE(nslice == want, "pclip_couple_bwd_f32: nslice=%d, expected ceil(Wv / %d) = %d", nslice, PCLIP_COUPLE_SLICE, want);
        PCLIP_REQUIRE(nslice == 1 || part, "pclip_couple_bwd_f32: %d row slices need the part buffer", nslice);
        couple_dx_part_kernel<<<dim3((Wt + 255) / 256, nslice, depth), 64, 0, s>>>(dY, Wc, P, Wt, Wv, nslice, nslice == 1 ? dX : part);
        const size_t M = (size_t)P * Wt;
        if (nslice > 1) rows_grad_sum_kernel<true><<<dim3(flat_grid(M / 4), depth), 256, 0, s>>>(part, nslice, M, dX, nslice * M, M);
    }
    return pclip_check_launch("couple_bwd");
}
