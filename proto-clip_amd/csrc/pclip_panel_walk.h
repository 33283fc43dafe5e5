// The panel walk: the scheme of the cosine-logit family (pclip_logits.hip, pclip_cosine_ce.hip, pclip_tip.hip), defined once.
//   * A workgroup stages a PANEL of 16 RF rows of one operand in LDS, rows D + PW_PAD halves apart, one wave per row, zeros past the last row (stage_panel).
//   * Its waves then WALK the rows of the other operand straight from memory in the MFMA operand layout: lane l holds row lr = l & 15, k-chunk lq = l >> 4 of a
//     16-row fragment — one 16-byte load per lane per k-step of 32 — as the FIRST operand of v_mfma_f32_16x16x32_f16 against the panel's fragments, so a lane ends
//     with 4 consecutive walked rows (4 lq .. 4 lq + 3) of ONE panel row (lr) per fragment.  Rows past the end are clamped reads whose results the caller drops
//     (walked_row).  One accumulator per element over k = 0, 32, ... D - 32 in that order, whatever the panel, the fragment count or the grid.
//     The forms differ in how far the walked operand is fetched ahead and in what their last step fetches; each states its tail rule.  Forms of different
//     prefetch depth are different schedules and stay apart.  The ONE-STEP-AHEAD form (next k-step's fragments in flight, the last step re-reads its own) is
//     written out in cosine_logits_kernel (four fragments) and twice in tip_kernel (one fragment; the class product scales the panel fragment on the way): as
//     a function it changed those kernels' registers or their measured time (profiles/panel_walk_refactor.txt), so a change to it is still made three times.
//   * The two recomputing backward kernels (ce_bwd_kernel, tip_bwd_kernel) follow the walk with a SECOND product: what they made of the first (an fp16 tile in LDS,
//     [panel row][walked row], rows PW_PLD halves apart) against the walked operand's transpose (transpose_kernel: [D][walked rounded up to 64]) into an fp32
//     gradient panel acc2[RF][NDF], wave w owning columns w D / 4 .. (w + 1) D / 4 - 1 of it.  What lies between the two products is each kernel's own.
// The host side holds what the launches share: the (NCH, RF, NDF) ladder over D, the RF rule, the row-norm and transpose launches, the operand checks.
#pragma once
#include <type_traits>
#include "pclip_proto_dev.h"

namespace {

constexpr int PW_PAD = 8;                      // halves between the LDS rows of the panel beyond D: ds_read_b128 in the operand layout spreads over the banks
constexpr int PW_PLD = 72;                     // halves per LDS row of the backward kernels' fp16 tiles (64 walked rows + 8: 16-byte reads spread over the banks)

// ---- fp16 logits: the operand scaling and the argmax / top-k keys (pclip_logits.hip, pclip_tip.hip) ----------------------------------------------
// the rounded fp16 logit and its column as one 32-bit key (order-preserving value bits | 0xFFFF - column: greater = larger value, then lower column; -0 counts as +0)
__device__ __forceinline__ unsigned logit_key(half_t v, int t) {
    unsigned b = __builtin_bit_cast(unsigned short, v);
    if (b == 0x8000u) b = 0;                                                    // -0 == +0: the lower column wins
    const unsigned o = (b & 0x8000u) ? (~b & 0xFFFFu) : (b | 0x8000u);
    return (o << 16) | (0xFFFFu - (unsigned)t);
}
__device__ __forceinline__ half_t key_value(unsigned key) {
    const unsigned o = key >> 16;
    const unsigned b = (o & 0x8000u) ? (o & 0x7FFFu) : (~o & 0xFFFFu);
    return __builtin_bit_cast(half_t, (unsigned short)b);
}

// r16(s * v): the fp32 product rounded to fp32, then to fp16 (torch's fp16 tensor times a scalar) — not one fused rounding
__device__ __forceinline__ half_t scale_r16(float s, half_t v) {
#pragma clang fp contract(off)
    const float p = s * (float)v;
    return (half_t)p;
}

// ---- the panel ---------------------------------------------------------------------------------------------------------------------------------------
// rows r0 .. r0 + rows - 1 of x into panel rows 0 .. rows - 1, one of the workgroup's NW waves per row: normalised when `norm`, then (SCALED) r16(scale * .);
// rows >= R are zeros and never read from memory
template <int NCH, int NW, bool SCALED = false>
__device__ __forceinline__ void stage_panel(half_t* panel, int LDP, const half_t* __restrict__ x, int ldx, int R, int D, int r0, int rows, int lane, int wave,
                                            int norm, float scale = 1.f) {
    for (int r = wave; r < rows; r += NW) {
        const int m = r0 + r;
        RowRegs<NCH> rr;
        if (m < R) {                                                                         // (wave-uniform)
            load_row<NCH>(x + (size_t)m * ldx, D, lane, rr);
            if (norm) normalise_row<NCH>(rr);
            if constexpr (SCALED) {
#pragma unroll
                for (int c = 0; c < NCH; ++c)
#pragma unroll
                    for (int j = 0; j < 8; ++j) rr.v[c][j] = scale_r16(scale, rr.v[c][j]);
            }
        } else {
#pragma unroll
            for (int c = 0; c < NCH; ++c)
#pragma unroll
                for (int j = 0; j < 8; ++j) rr.v[c][j] = (half_t)0.f;
        }
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int d = c * 512 + lane * 8;
            if (d < D) st_half8(panel + (size_t)r * LDP + d, rr.v[c]);
        }
    }
}

// rows normalised into a workspace (dense [R, D]): the walked operand under a normalise flag
// GROUPED, launched with gridDim.y = G: G operands of R rows each in one launch, group blockIdx.y reading at x + blockIdx.y gsx and writing its dense
// [R, D] block of y [G R, D].  The ungrouped instantiation does not read gsx (the habit of pclip_rows.h).
template <int NCH, bool GROUPED = false>
__global__ __launch_bounds__(256) void norm_rows_kernel(const half_t* __restrict__ x, int ldx, half_t* __restrict__ y, int R, int D, size_t gsx) {
    if (GROUPED) {
        x += blockIdx.y * gsx;
        y += blockIdx.y * ((size_t)R * D);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int row = blockIdx.x * 4 + wave; row < R; row += gridDim.x * 4) {
        RowRegs<NCH> r;
        load_row<NCH>(x + (size_t)row * ldx, D, lane, r);
        normalise_row<NCH>(r);
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int d = c * 512 + lane * 8;
            if (d < D) st_half8(y + (size_t)row * D + d, r.v[c]);
        }
    }
}

// ---- the walk ----------------------------------------------------------------------------------------------------------------------------------------
// this lane's piece of walked row `row` at k = 0; rows >= R read row R - 1
__device__ __forceinline__ const half_t* walked_row(const half_t* x, int ldx, int row, int R, int lq) {
    row = row < R ? row : R - 1;
    return x + (size_t)row * ldx + lq * 8;
}

// k-steps in PAIRS (KS is even), the pair after the one in the MFMAs in flight.  Tail: the last pair re-reads itself — no read past column D.
template <int RF, int NF>
__device__ __forceinline__ void walk_pairs(const half_t* const (&bp)[NF], const half_t* ap, int LDP, int KS, float4_t (&acc)[RF][NF]) {
#pragma unroll
    for (int f = 0; f < RF; ++f)
#pragma unroll
        for (int c = 0; c < NF; ++c) acc[f][c] = float4_t{0.f, 0.f, 0.f, 0.f};
    half8_t b0[NF], b1[NF];
#pragma unroll
    for (int c = 0; c < NF; ++c) b0[c] = ld_half8(bp[c]), b1[c] = ld_half8(bp[c] + 32);
    for (int ks = 0; ks < KS; ks += 2) {
        half8_t n0[NF], n1[NF];
        const int kn = ks + 2 < KS ? ks + 2 : ks;
#pragma unroll
        for (int c = 0; c < NF; ++c) n0[c] = ld_half8(bp[c] + kn * 32), n1[c] = ld_half8(bp[c] + kn * 32 + 32);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            half8_t af[RF];
#pragma unroll
            for (int f = 0; f < RF; ++f) af[f] = ld_half8(ap + (size_t)f * 16 * LDP + (ks + u) * 32);
#pragma unroll
            for (int f = 0; f < RF; ++f)
#pragma unroll
                for (int c = 0; c < NF; ++c) acc[f][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(u ? b1[c] : b0[c], af[f], acc[f][c], 0, 0, 0);
        }
#pragma unroll
        for (int c = 0; c < NF; ++c) b0[c] = n0[c], b1[c] = n1[c];
    }
}

// ---- the recomputing backward: first product, transposed-operand prefetch, second product, gradient store ----------------------------------------------
// (tip_bwd_kernel calls all four; ce_bwd_kernel calls the second product and the store and keeps the text of the first two: the note there)
// One walked fragment per wave, k-steps in pairs (KS is even) with the next pair in flight; c0 / c1 arrive holding the first pair of row wp (the caller loads them
// before its first tile).  Tail: under the last pair the prefetch ROLLS INTO THE NEXT TILE — the first pair of wpn, the wave's (clamped) row of that tile: c0 / c1
// leave as that tile's, and the caller goes on with wp = wpn.  acc[f][r] = x[panel row 16 f + lr] . walked row (4 lq + r of the wave's 16).
template <int RF>
__device__ __forceinline__ void bwd_first_product(const half_t* wp, const half_t* wpn, half8_t& c0, half8_t& c1, const half_t* ap, int LDP, int KS, float4_t (&acc)[RF]) {
#pragma unroll
    for (int f = 0; f < RF; ++f) acc[f] = float4_t{0.f, 0.f, 0.f, 0.f};
    for (int ks = 0; ks < KS; ks += 2) {
        const half_t* np = ks + 2 < KS ? wp + (ks + 2) * 32 : wpn;
        const half8_t n0 = ld_half8(np), n1 = ld_half8(np + 32);
#pragma unroll
        for (int f = 0; f < RF; ++f) acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(c0, ld_half8(ap + (size_t)f * 16 * LDP + ks * 32), acc[f], 0, 0, 0);
#pragma unroll
        for (int f = 0; f < RF; ++f) acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(c1, ld_half8(ap + (size_t)f * 16 * LDP + ks * 32 + 32), acc[f], 0, 0, 0);
        c0 = n0, c1 = n1;
    }
}

// the first eight column fragments of the second product's transposed operand (walked rows j0 .. j0 + 31): issued by the caller before its own work on the first
// product, so that they are in flight under it and the barrier
__device__ __forceinline__ void bwd_prefetch_t(half8_t (&wt0)[8], const half_t* __restrict__ xT, int ldt, int dbase, int ndf, int j0, int lr, int lq) {
#pragma unroll
    for (int u = 0; u < 8; ++u) wt0[u] = u < ndf ? ld_half8(xT + (size_t)(dbase + 16 * u + lr) * ldt + j0 + 8 * lq) : half8_t{};
}

// this wave's quarter of D: acc2 += walked^T tile, the walked index along k.  NDF: the 16-column fragments of a quarter the kernel is compiled for, ndf = D / 64
// <= NDF of them live.  tile / ytile: [2][16 RF][PW_PLD], buffer `buf`; WITH_Y: ytile is a second tile that goes through the same MFMA into the same accumulator
// when `targets` (CE's exact target term).
template <int RF, int NDF, bool WITH_Y>
__device__ __forceinline__ void bwd_second_product(const half_t* __restrict__ xT, int ldt, int dbase, int ndf, int j0, const half8_t (&wt0)[8], const half_t* tile,
                                                   const half_t* ytile, bool targets, int buf, int lr, int lq, float4_t (&acc2)[RF][NDF]) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        half8_t pf[RF], yf[RF];
#pragma unroll
        for (int f = 0; f < RF; ++f) {
            const size_t at = ((size_t)buf * 16 * RF + 16 * f + lr) * PW_PLD + 32 * p + 8 * lq;
            pf[f] = ld_half8(tile + at);
            if constexpr (WITH_Y) yf[f] = ld_half8(ytile + at);
        }
#pragma unroll
        for (int g = 0; g < NDF / 8; ++g) {
            half8_t wt[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (p == 0 && g == 0) wt[u] = wt0[u];
                else wt[u] = 8 * g + u >= ndf ? half8_t{} : ld_half8(xT + (size_t)(dbase + 16 * (8 * g + u) + lr) * ldt + j0 + 32 * p + 8 * lq);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int df = 8 * g + u;
                if (df < ndf) {                                                              // (uniform)
#pragma unroll
                    for (int f = 0; f < RF; ++f) acc2[f][df] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wt[u], pf[f], acc2[f][df], 0, 0, 0);
                    if (WITH_Y && targets) {
#pragma unroll
                        for (int f = 0; f < RF; ++f) acc2[f][df] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wt[u], yf[f], acc2[f][df], 0, 0, 0);
                    }
                }
            }
        }
    }
}

// gout[i0 + 16 f + lr, dbase + 16 df + 4 lq + r] = mul * acc2[f][df][r] for the panel's rows < R
template <int RF, int NDF>
__device__ __forceinline__ void store_grad_panel(float* __restrict__ gout, int i0, int R, int D, int dbase, int ndf, float mul, int lr, int lq,
                                                 const float4_t (&acc2)[RF][NDF]) {
#pragma unroll
    for (int f = 0; f < RF; ++f) {
        const int i = i0 + 16 * f + lr;
        if (i >= R) continue;
#pragma unroll
        for (int df = 0; df < NDF; ++df) {
            if (df < ndf) {
                float4_t o = acc2[f][df];
#pragma unroll
                for (int r = 0; r < 4; ++r) o[r] *= mul;
                *reinterpret_cast<float4_t*>(gout + (size_t)i * D + dbase + 16 * df + 4 * lq) = o;
            }
        }
    }
}

// y [D][ldt] = x^T, 64 x 64 tiles through LDS; rows R .. ldt - 1 of x read as zeros (ldt = R rounded up to 64: every column of y is written)
// (a template, TS = 64 the one tile size: only the files that launch it instantiate it)
// GROUPED, launched with gridDim.z = G: G transposes of one shape, group blockIdx.z from x + blockIdx.z gsx into its dense [D][ldt] block of y.
template <int TS, bool GROUPED = false>
__global__ __launch_bounds__(256) void transpose_kernel(const half_t* __restrict__ x, int ldx, int R, half_t* __restrict__ y, int ldt, size_t gsx) {
    static_assert(TS == 64, "transpose_kernel: 64 x 64 tiles");
    if (GROUPED) {
        x += blockIdx.z * gsx;
        y += blockIdx.z * ((size_t)gridDim.y * 64 * ldt);
    }
    __shared__ half_t tile[64][66];
    const int r0 = blockIdx.x * 64, d0 = blockIdx.y * 64;
    for (int i = threadIdx.x; i < 64 * 64; i += 256) {
        const int r = i >> 6, c = i & 63;
        tile[r][c] = r0 + r < R ? x[(size_t)(r0 + r) * ldx + d0 + c] : (half_t)0.f;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * 64; i += 256) {
        const int c = i >> 6, r = i & 63;
        y[(size_t)(d0 + c) * ldt + r0 + r] = tile[r][c];
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------------------
// row fragments per panel: what the row count asks for, capped by the backward's accumulator panel (RF D / 16 registers per lane <= 128)
inline int rf_for(int rows, int D) {
    const int rfmax = D <= 512 ? 4 : (D <= 1024 ? 2 : 1);
    const int rf = rows <= 16 ? 1 : (rows <= 32 ? 2 : 4);
    return rf > rfmax ? rfmax : rf;
}
inline int round64(int r) { return (r + 63) / 64 * 64; }

// call(NCH, RF, NDF) — three std::integral_constant, usable as template arguments — for the one form of D <= 2048 and RF (<= rf_for's cap, and <= RFMAX where a
// kernel compiles fewer panels) that the kernels are compiled for.  `call` raises its kernel's LDS limit (a static DevOnce per form) and launches; its status returns.
template <int RFMAX = 4, class Call>
int panel_dispatch(int D, int RF, Call&& call) {
    using std::integral_constant;
    if (D <= 512) {
        if constexpr (RFMAX >= 4)
            if (RF == 4) return call(integral_constant<int, 1>{}, integral_constant<int, 4>{}, integral_constant<int, 8>{});
        if (RF == 2) return call(integral_constant<int, 1>{}, integral_constant<int, 2>{}, integral_constant<int, 8>{});
        return call(integral_constant<int, 1>{}, integral_constant<int, 1>{}, integral_constant<int, 8>{});
    }
    if (D <= 1024) {
        if (RF == 2) return call(integral_constant<int, 2>{}, integral_constant<int, 2>{}, integral_constant<int, 16>{});
        return call(integral_constant<int, 2>{}, integral_constant<int, 1>{}, integral_constant<int, 16>{});
    }
    return call(integral_constant<int, 4>{}, integral_constant<int, 1>{}, integral_constant<int, 32>{});
}

// y = the rows of x normalised, dense [R, D].  DMAX: the caller's cap on D — NCH = 8 is compiled only where D can pass 2048
template <int DMAX>
int launch_norm_rows(const half_t* x, int ldx, half_t* y, int R, int D, hipStream_t s, const char* what) {
    int g = ceil_div(R, 4);
    g = g > 8192 ? 8192 : g;
    if (D <= 512) norm_rows_kernel<1><<<g, 256, 0, s>>>(x, ldx, y, R, D, 0);
    else if (D <= 1024) norm_rows_kernel<2><<<g, 256, 0, s>>>(x, ldx, y, R, D, 0);
    else if (DMAX <= 2048 || D <= 2048) norm_rows_kernel<4><<<g, 256, 0, s>>>(x, ldx, y, R, D, 0);
    else if constexpr (DMAX > 2048) norm_rows_kernel<8><<<g, 256, 0, s>>>(x, ldx, y, R, D, 0);
    return pclip_check_launch(what);
}
// the rows of G operands of R rows each (group g at x + g gsx, G <= 65535) normalised in ONE launch: y dense [G R, D]
template <int DMAX>
int launch_norm_rows_grouped(const half_t* x, int ldx, size_t gsx, half_t* y, int R, int D, int G, hipStream_t s, const char* what) {
    static_assert(DMAX <= 2048, "launch_norm_rows_grouped: NCH <= 4");
    int g = ceil_div(R, 4);
    g = g > 8192 ? 8192 : g;
    if (D <= 512) norm_rows_kernel<1, true><<<dim3(g, G), 256, 0, s>>>(x, ldx, y, R, D, gsx);
    else if (D <= 1024) norm_rows_kernel<2, true><<<dim3(g, G), 256, 0, s>>>(x, ldx, y, R, D, gsx);
    else norm_rows_kernel<4, true><<<dim3(g, G), 256, 0, s>>>(x, ldx, y, R, D, gsx);
    return pclip_check_launch(what);
}

// xT [D][ldt] = x^T, zero-filled past row R; ldt = round64(R), the pitch the backward kernel is given too
// (a template only so that, like transpose_kernel, it is instantiated in the files that call it and pclip_logits.hip carries no transpose kernel)
template <int TS = 64>
int launch_transpose(const half_t* x, int ldx, int R, int D, half_t* xT, int ldt, hipStream_t s, const char* what) {
    transpose_kernel<TS><<<dim3(ldt / 64, D / 64), 256, 0, s>>>(x, ldx, R, xT, ldt, 0);
    return pclip_check_launch(what);
}
// G of them in one launch (G <= 65535): x_g = x + g gsx, the xT_g [D][ldt] dense one behind the other
template <int TS = 64>
int launch_transpose_grouped(const half_t* x, int ldx, size_t gsx, int R, int D, int G, half_t* xT, int ldt, hipStream_t s, const char* what) {
    transpose_kernel<TS, true><<<dim3(ldt / 64, D / 64, G), 256, 0, s>>>(x, ldx, R, xT, ldt, gsx);
    return pclip_check_launch(what);
}

// a row operand's pitch `ld` (the message names the variable), and the operands' alignment: `p16` the pointers that need 16 bytes, ORed, `p4` those that need 4
#define PCLIP_REQUIRE_PITCH(fn, ld, D) PCLIP_REQUIRE((ld) >= (D) && (ld) % 8 == 0, "%s: " #ld "=%d must be >= D=%d and a multiple of 8 halves", fn, ld, D)
#define PCLIP_REQUIRE_ALIGNED(fn, p16, p4) PCLIP_REQUIRE((p16) % 16 == 0 && (p4) % 4 == 0, "%s: operands must be 16-byte aligned", fn)

}  // namespace
