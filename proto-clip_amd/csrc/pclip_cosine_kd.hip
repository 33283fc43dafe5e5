// Distillation (soft-target) loss over cosine logits and its gradients: KL from a frozen teacher's prediction to the student's, both of them logits of
// clip/model.py:356-370 (ProGrad's zero-shot classifier against the learned prompts, a logit-consistency term, a teacher of another feature width).
//   s[m, t] = scale  * cos_s[m, t],  cos_s = fp32 MFMA accumulation of a'[m, :]  . b'[t, :]   (one accumulator over k = 0, 32, ... D - 32)
//   z[m, t] = tscale * cos_t[m, t],  cos_t = fp32 MFMA accumulation of ta'[m, :] . tb'[t, :]  (the teacher's own operands, width Dt and normalise flags)
//   p = softmax_t z,  q = softmax_t s,  row_loss[m] = sum_t p (z - s) - lse_t z + lse_t s  ( = KL(p || q) ),  loss = mean_m row_loss.
// NOTHING is rounded to fp16 on the way to s or z; no log p is formed (p = exp(z - tlse) times a finite difference: an entry whose p underflows adds an exact
// zero); the value is not clamped at zero.  Ragged in M and T; nothing of size M T reaches memory, forward or backward.
// Forward, two passes:
//   1. lse_row and tlse_row are written by pclip_cosine_ce_f16 itself, on (a, b, scale) and on (ta, tb, tscale), with labels of -1 (a label outside [0, T)
//      matches nothing: the forward then yields the lse alone).  They are its bits because they are its launches.
//   2. kd_fwd_kernel: the walk of ce_fwd_kernel by eight waves (64-column blocks dealt to the KD_FW waves, k ascending) with TWO panels in LDS, 16 RF rows of a'
//      and the same rows of ta', and two first products per column block.  A lane sums p (z - s) over its columns in block order; a row's four lane groups,
//      then its eight waves are added in a fixed order.  The mean is one fixed-order fp64 sum.
// Backward (kd_bwd_kernel), "own" = the side whose gradient is produced, "walked" = the other (direction 0: own a / ta, walked b / tb; direction 1 exchanged):
//   the walk of ce_bwd_kernel with the shared skeleton of pclip_panel_walk.h (bwd_first_product twice, bwd_prefetch_t, bwd_second_product, store_grad_panel):
//   per 64 walked rows wave w recomputes its 16 RF x 16 fragment of cos_s and of cos_t, forms the SIGNED tile
//       E = exp(s - lse_row[m]) - exp(z - tlse_row[m])          (q - p, in [-1, 1]; m the a-side index of the element)
//   in registers, rounds 2^14 E to fp16 (unit 2^-11: the one rounding the gradient tolerance of tests/cosine_kd_ref.py is built on) into LDS [own][walked],
//   and after one barrier every wave accumulates E . walked'^T (the STUDENT's walked operand: the teacher receives no gradient) into its quarter of D.
//   weight and scale act in fp32 at the store.  dscale = sum G o cos_s from the unrounded E: per-lane fp32, per-panel partials, one fixed-order fp64 sum.
//   Under NORMALIZE_A / _B the panel gradient is chained through x / ||x|| in fp32 (the fp16 rounding of x' taken as the identity).
// Every workgroup walks ALL walked rows in index order and an element has one accumulator: a row's loss term and its row of dL/da depend on that row and the
// class operands alone, not on M, the panel size or the grid.  dL/db over few classes shares its walked tiles between workgroups in fixed chunks (kd_chunks),
// summed in chunk order.  No floating-point atomics.
// The kernels are compiled per (chunks of 512 in the WIDER of D and Dt, RF, column fragments of D): the narrower operand is staged by the wider one's row
// loader (its missing chunks are zeros that are never stored) and walked with its own k-step count at run time.
// Only __syncthreads barriers and compiler-counted waits: nothing here for the race-stress build.
#include <cmath>
#include "pclip_panel_walk.h"

namespace {

constexpr int KD_LDS_MAX = 152 * 1024;           // dynamic LDS asked for (two 16-row panels of 2048 + 8 halves are 132 KB; the most used is 137 KB)
constexpr int KD_DMAX = 2048;
constexpr int KD_FW = 8;                        // waves of a forward workgroup, as CE_FW: each walks every eighth block of 64 columns
constexpr int KD_RFMAX = 2;                     // row fragments per panel: two panels share the LDS one has in the cross-entropy kernels
constexpr float KD_ESCALE = 16384.f;            // E in [-1, 1] enters the fp16 tile as 2^14 E (exact scaling, undone in fp32 with the weight): pclip_cosine_ce.hip, CE_ESCALE

// loss[m] = sum_t p (z - s) - tlse + lse for the panel's rows
template <int NCH, int RF>
__global__ __launch_bounds__(64 * KD_FW) void kd_fwd_kernel(const half_t* __restrict__ a, int lda, int M, const half_t* __restrict__ b, int ldb, int T, int D, float scale,
                                                     int norm_a, const half_t* __restrict__ ta, int ldta, const half_t* __restrict__ tb, int ldtb, int Dt,
                                                     float tscale, int norm_ta, const float* __restrict__ lse_row, const float* __restrict__ tlse_row,
                                                     float* __restrict__ row_loss) {
    extern __shared__ __attribute__((aligned(16))) char kd_smem[];
    __shared__ float red[KD_FW][RF][16];
    const int LDP = D + PW_PAD, LDT = Dt + PW_PAD;
    half_t* panel = reinterpret_cast<half_t*>(kd_smem);                                      // [16 RF][D + 8]
    half_t* tpanel = panel + (size_t)16 * RF * LDP;                                          // [16 RF][Dt + 8]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m0 = blockIdx.x * 16 * RF;
    stage_panel<NCH, KD_FW>(panel, LDP, a, lda, M, D, m0, 16 * RF, lane, wave, norm_a);
    stage_panel<NCH, KD_FW>(tpanel, LDT, ta, ldta, M, Dt, m0, 16 * RF, lane, wave, norm_ta);

    const int lr = lane & 15, lq = lane >> 4;
    float lt[RF], sum[RF];
#pragma unroll
    for (int f = 0; f < RF; ++f) {
        const int m = m0 + 16 * f + lr;
        lt[f] = m < M ? tlse_row[m] : 0.f;
        sum[f] = 0.f;
    }
    __syncthreads();

    const int KS = D >> 5, KST = Dt >> 5, ncb = (T + 63) >> 6;
    for (int cb = wave; cb < ncb; cb += KD_FW) {
        const int t0 = cb * 64;
        const half_t *bp[4], *tp[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            bp[c] = walked_row(b, ldb, t0 + 16 * c + lr, T, lq);
            tp[c] = walked_row(tb, ldtb, t0 + 16 * c + lr, T, lq);
        }
        float4_t acc[RF][4], tacc[RF][4];
        walk_pairs<RF, 4>(bp, panel + (size_t)lr * LDP + lq * 8, LDP, KS, acc);
        walk_pairs<RF, 4>(tp, tpanel + (size_t)lr * LDT + lq * 8, LDT, KST, tacc);
        // acc[f][c][r] = cos_s(m0 + 16 f + lr, t0 + 16 c + 4 lq + r), tacc the teacher's
#pragma unroll
        for (int f = 0; f < RF; ++f)
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int t = t0 + 16 * c + 4 * lq + r;
                    const float s = scale * acc[f][c][r], z = tscale * tacc[f][c][r];
                    const float p = __expf(z - lt[f]);
                    sum[f] += t < T ? p * (z - s) : 0.f;
                }
    }
    // ---- a row's 4 lane groups, then its KD_FW waves, in a fixed order ----------------------------------------------------------------------
#pragma unroll
    for (int f = 0; f < RF; ++f) {
        sum[f] += lane_xor<16>(sum[f]);
        sum[f] += lane_xor<32>(sum[f]);
        if (lq == 0) red[wave][f][lr] = sum[f];
    }
    __syncthreads();
    if (threadIdx.x < 16 * RF) {
        const int f = threadIdx.x >> 4, row = threadIdx.x & 15, m = m0 + threadIdx.x;
        if (m < M) {
            float tot = red[0][f][row];
            for (int w = 1; w < KD_FW; ++w) tot += red[w][f][row];
            row_loss[m] = (tot - tlse_row[m]) + lse_row[m];
        }
    }
}

// out[0] = mul * sum x[0 .. n), one workgroup, fp64, a fixed order (the text of ce_sum_kernel)
__global__ __launch_bounds__(256) void kd_sum_kernel(const float* __restrict__ x, int n, double mul, float* __restrict__ out) {
    __shared__ double part[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += (double)x[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)(mul * part[0]);
}

// out = sum over the chunks of part [nchunks][n], in chunk order (n % 4 == 0)
__global__ __launch_bounds__(256) void kd_sum_chunks_kernel(const float* __restrict__ part, int nchunks, size_t n, float* __restrict__ out) {
    for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += (size_t)gridDim.x * 256 * 4) {
        float4_t s = *reinterpret_cast<const float4_t*>(part + i);
        for (int c = 1; c < nchunks; ++c) s += *reinterpret_cast<const float4_t*>(part + (size_t)c * n + i);
        *reinterpret_cast<float4_t*>(out + i) = s;
    }
}

// a_side_own: the lse vectors (both on the a side) index the own rows (direction 0) or the walked rows (direction 1)
template <int NCH, int RF, int NDF>
__global__ __launch_bounds__(256) void kd_bwd_kernel(const half_t* __restrict__ own, int ldo, int Ro, const half_t* __restrict__ walk, int ldw, int Rw,
                                                     const half_t* __restrict__ walkT, int ldt, int D, float scale, const half_t* __restrict__ town, int ldto,
                                                     const half_t* __restrict__ twalk, int ldtw, int Dt, float tscale, float weight, int norm_own, int norm_town,
                                                     int a_side_own, const float* __restrict__ lse_s, const float* __restrict__ lse_t, float* __restrict__ gout,
                                                     float* __restrict__ dsc_part) {
    extern __shared__ __attribute__((aligned(16))) char kd_smem[];
    const int LDP = D + PW_PAD, LDT = Dt + PW_PAD;
    half_t* panel = reinterpret_cast<half_t*>(kd_smem);                                      // [16 RF][D + 8]
    half_t* tpanel = panel + (size_t)16 * RF * LDP;                                          // [16 RF][Dt + 8]
    half_t* etile = tpanel + (size_t)16 * RF * LDT;                                          // [2][16 RF][PW_PLD]: r16(2^14 E), own row x walked row
    float* dsc_red = reinterpret_cast<float*>(etile + (size_t)2 * 16 * RF * PW_PLD);         // [4]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i0 = blockIdx.x * 16 * RF;
    stage_panel<NCH, 4>(panel, LDP, own, ldo, Ro, D, i0, 16 * RF, lane, wave, norm_own);
    stage_panel<NCH, 4>(tpanel, LDT, town, ldto, Ro, Dt, i0, 16 * RF, lane, wave, norm_town);

    const int lr = lane & 15, lq = lane >> 4;
    const int ndf = D >> 6, dbase = wave * (D >> 2);
    float los[RF], lot[RF];
#pragma unroll
    for (int f = 0; f < RF; ++f) {
        const int i = i0 + 16 * f + lr;
        const bool ok = a_side_own && i < Ro;
        los[f] = ok ? lse_s[i] : 0.f;
        lot[f] = ok ? lse_t[i] : 0.f;
    }
    float4_t acc2[RF][NDF];
#pragma unroll
    for (int f = 0; f < RF; ++f)
#pragma unroll
        for (int df = 0; df < NDF; ++df) acc2[f][df] = float4_t{0.f, 0.f, 0.f, 0.f};
    float dsc = 0.f;
    __syncthreads();

    // blockIdx.y: this workgroup's chunk of the walked tiles (gridDim.y > 1: gout is that chunk's partial panel, summed in chunk order by kd_sum_chunks_kernel)
    const int KS = D >> 5, KST = Dt >> 5, ntiles = (Rw + 63) >> 6, tpc = (ntiles + gridDim.y - 1) / gridDim.y;
    const int tile_end = (int)(blockIdx.y + 1) * tpc < ntiles ? (int)(blockIdx.y + 1) * tpc : ntiles;
    gout += (size_t)blockIdx.y * Ro * D;
    const half_t *wp, *twp;                                                                  // this wave's walked row of the tile at hand (clamped), student's and teacher's
    {
        int jr = (int)blockIdx.y * tpc * 64 + 16 * wave + lr;
        jr = jr < Rw ? jr : Rw - 1;
        wp = walk + (size_t)jr * ldw + lq * 8;
        twp = twalk + (size_t)jr * ldtw + lq * 8;
    }
    half8_t c0 = ld_half8(wp), c1 = ld_half8(wp + 32), d0 = ld_half8(twp), d1 = ld_half8(twp + 32);
    const half_t* ap = panel + (size_t)lr * LDP + lq * 8;
    const half_t* tap = tpanel + (size_t)lr * LDT + lq * 8;
    for (int tile = blockIdx.y * tpc; tile < tile_end; ++tile) {
        const int j0 = tile * 64, buf = tile & 1;
        int jn = j0 + 64 + 16 * wave + lr;
        jn = jn < Rw ? jn : Rw - 1;
        const half_t* wpn = walk + (size_t)jn * ldw + lq * 8;
        const half_t* twpn = twalk + (size_t)jn * ldtw + lq * 8;
        float4_t acc[RF], tacc[RF];
        bwd_first_product<RF>(wp, wpn, c0, c1, ap, LDP, KS, acc);
        bwd_first_product<RF>(twp, twpn, d0, d1, tap, LDT, KST, tacc);
        wp = wpn, twp = twpn;
        half8_t wt0[8];
        bwd_prefetch_t(wt0, walkT, ldt, dbase, ndf, j0, lr, lq);
        // acc[f][r] = cos_s(own i0 + 16 f + lr, walked j0 + 16 wave + 4 lq + r), tacc the teacher's
        const int jb = j0 + 16 * wave + 4 * lq;
        float lws[4], lwt[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool ok = !a_side_own && jb + r < Rw;
            lws[r] = ok ? lse_s[jb + r] : 0.f;
            lwt[r] = ok ? lse_t[jb + r] : 0.f;
        }
#pragma unroll
        for (int f = 0; f < RF; ++f) {
            const int i = i0 + 16 * f + lr;
            half4_t e16;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float cosv = acc[f][r], s = scale * cosv, z = tscale * tacc[f][r];
                const bool ok = i < Ro && jb + r < Rw;
                const float ls = a_side_own ? los[f] : lws[r], lt = a_side_own ? lot[f] : lwt[r];
                const float e = ok ? __expf(s - ls) - __expf(z - lt) : 0.f;
                dsc += e * cosv;
                e16[r] = (half_t)(e * KD_ESCALE);
            }
            const size_t at = ((size_t)buf * 16 * RF + 16 * f + lr) * PW_PLD + 16 * wave + 4 * lq;
            *reinterpret_cast<half4_t*>(etile + at) = e16;
        }
        __syncthreads();                                                                     // the tile is whole; the other buffer is free once every wave is here
        // ---- this wave's quarter of D: acc2 += walked'^T E, the walked index along k -----------------------------------------------------
        bwd_second_product<RF, NDF, false>(walkT, ldt, dbase, ndf, j0, wt0, etile, nullptr, false, buf, lr, lq, acc2);
    }
    // acc2[f][df][r] = 2^14 sum_j E[i0 + 16 f + lr, j] walked'[j, dbase + 16 df + 4 lq + r]
    store_grad_panel<RF, NDF>(gout, i0, Ro, D, dbase, ndf, weight * scale * (1.f / KD_ESCALE), lr, lq, acc2);
    if (dsc_part) {
        dsc = wave_sum(dsc);
        if (lane == 0) dsc_red[wave] = dsc;
        __syncthreads();
        if (threadIdx.x == 0) dsc_part[blockIdx.y * gridDim.x + blockIdx.x] = weight * (((dsc_red[0] + dsc_red[1]) + dsc_red[2]) + dsc_red[3]);
    }
}

// g <- (g - y (y . g)) / ||x||, y = x / ||x|| in fp32: the gradient of x -> x / ||x|| applied to a row of dL/dx' in place (the text of ce_norm_backward_kernel)
template <int NCH>
__global__ __launch_bounds__(256) void kd_norm_backward_kernel(const half_t* __restrict__ x, int ldx, float* __restrict__ g, int R, int D) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int row = blockIdx.x * 4 + wave; row < R; row += gridDim.x * 4) {
        RowRegs<NCH> rr;
        load_row<NCH>(x + (size_t)row * ldx, D, lane, rr);
        float gv[NCH][8];
        float ss = 0.f, dot = 0.f;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int d = c * 512 + lane * 8;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                gv[c][j] = d < D ? g[(size_t)row * D + d + j] : 0.f;
                const float xv = (float)rr.v[c][j];
                ss += xv * xv;
                dot += xv * gv[c][j];
            }
        }
        ss = wave_sum(ss);
        dot = wave_sum(dot);
        const float inv = 1.f / sqrtf(ss), k = dot / ss;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int d = c * 512 + lane * 8;
            if (d < D) {
#pragma unroll
                for (int j = 0; j < 8; ++j) g[(size_t)row * D + d + j] = (gv[c][j] - k * (float)rr.v[c][j]) * inv;
            }
        }
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------------------
// row fragments per panel: rf_for's rule on the wider operand, capped at KD_RFMAX (a row's bits do not depend on RF)
inline int kd_rf(int rows, int Dx) {
    const int rf = rf_for(rows, Dx);
    return rf > KD_RFMAX ? KD_RFMAX : rf;
}
inline int kd_rf_fwd(int M, int Dx) {                 // as ce_rf_fwd: the forward's only workgroups are its panels
    int rf = kd_rf(M, Dx);
    while (rf > 1 && ceil_div(M, 16 * rf) < 256) rf >>= 1;
    return rf;
}

// call(NCH, RF, NDF): NCH the 512-chunks of Dx = max(D, Dt), NDF the column fragments of a quarter of D, RF <= KD_RFMAX (1 past Dx = 1024)
template <class Call>
int kd_dispatch(int D, int Dx, int RF, Call&& call) {
    using std::integral_constant;
#define KD_FORM(nch, rf, ndf) call(integral_constant<int, nch>{}, integral_constant<int, rf>{}, integral_constant<int, ndf>{})
    if (Dx <= 512) return RF == 2 ? KD_FORM(1, 2, 8) : KD_FORM(1, 1, 8);
    if (Dx <= 1024) {
        if (D <= 512) return RF == 2 ? KD_FORM(2, 2, 8) : KD_FORM(2, 1, 8);
        return RF == 2 ? KD_FORM(2, 2, 16) : KD_FORM(2, 1, 16);
    }
    if (D <= 512) return KD_FORM(4, 1, 8);
    if (D <= 1024) return KD_FORM(4, 1, 16);
    return KD_FORM(4, 1, 32);
#undef KD_FORM
}

// the workspaces are laid out for Dx = max(D, Dt) on both sides: pclip_workspace_bytes has one width to ask with
struct KdFwdWs {
    size_t bn, tbn, ce, labels, rows, loss, bytes;
};
inline KdFwdWs kd_fwd_ws(int M, int T, int Dx) {
    KdFwdWs w;
    size_t off = 0;
    w.bn = off, off += align_up((size_t)T * Dx * 2, 256);
    w.tbn = off, off += align_up((size_t)T * Dx * 2, 256);
    w.ce = off, off += align_up(pclip_cosine_ce_workspace(0, M, T, Dx), 256);               // (no smaller for a narrower operand: each of its regions grows with D)
    w.labels = off, off += align_up((size_t)M * 4, 256);
    w.rows = off, off += align_up((size_t)M * 4, 256);
    w.loss = off, off += 256;
    w.bytes = off;
    return w;
}
// dL/db over few classes is few panels: the walked tiles are shared between workgroups, each with a partial fp32 panel in ws (ce_chunks' rule).  Never for
// dL/da: its rows keep their bits whatever the batch.
constexpr int KD_WG_TARGET = 512;
inline int kd_chunks(int Ro, int Rw, int Dx, bool split_allowed) {
    if (!split_allowed) return 1;
    const int npanels = ceil_div(Ro, 16 * kd_rf(Ro, Dx)), ntiles = ceil_div(Rw, 64);
    int n = ceil_div(KD_WG_TARGET, npanels);
    const int cap = (int)(4 * ((size_t)Ro + Rw) / Ro);
    n = n > cap ? cap : n;
    n = n > ntiles ? ntiles : n;
    n = n > 65535 ? 65535 : n;
    return n < 1 ? 1 : n;
}
struct KdBwdWs {
    size_t wn, twn, wt, dsc, part, bytes;
};
inline KdBwdWs kd_bwd_ws(int M, int T, int Dx) {       // either direction fits: sized by the larger side
    const int R = M > T ? M : T;
    const int cb = kd_chunks(T, M, Dx, true);
    const size_t pb = cb > 1 ? (size_t)cb * T : 0;
    const size_t da = (size_t)ceil_div(M, 16), db = (size_t)cb * ceil_div(T, 16);
    KdBwdWs w;
    size_t off = 0;
    w.wn = off, off += align_up((size_t)R * Dx * 2, 256);
    w.twn = off, off += align_up((size_t)R * Dx * 2, 256);
    w.wt = off, off += align_up((size_t)Dx * round64(R) * 2, 256);
    w.dsc = off, off += align_up((da > db ? da : db) * 4, 256);
    w.part = off, off += align_up(pb * Dx * 4, 256);
    w.bytes = off;
    return w;
}

constexpr int KD_FLAGS = PCLIP_KD_NORMALIZE_A | PCLIP_KD_NORMALIZE_B | PCLIP_KD_NORMALIZE_TA | PCLIP_KD_NORMALIZE_TB;

int kd_validate(const char* fn, const void* a, int lda, int M, const void* b, int ldb, int T, int D, float scale, const void* ta, int ldta, const void* tb,
                int ldtb, int Dt, float tscale, int flags, const void* ws, size_t ws_bytes, size_t need) {
    PCLIP_REQUIRE(a && b && ta && tb, "%s: null operand", fn);
    PCLIP_REQUIRE(M >= 1 && T >= 1, "%s: M=%d and T=%d must be positive", fn, M, T);
    PCLIP_REQUIRE(D > 0 && D % 64 == 0, "%s: D=%d must be a multiple of 64", fn, D);
    PCLIP_REQUIRE(D <= KD_DMAX, "%s: D=%d is past the envelope (D <= %d)", fn, D, KD_DMAX);
    PCLIP_REQUIRE(Dt > 0 && Dt % 64 == 0, "%s: Dt=%d must be a multiple of 64", fn, Dt);
    PCLIP_REQUIRE(Dt <= KD_DMAX, "%s: Dt=%d is past the envelope (Dt <= %d)", fn, Dt, KD_DMAX);
    PCLIP_REQUIRE((flags & ~KD_FLAGS) == 0, "%s: unknown flag bits 0x%x", fn, flags);
    PCLIP_REQUIRE(std::isfinite(scale) && std::isfinite(tscale), "%s: scale=%g and tscale=%g must be finite", fn, (double)scale, (double)tscale);
    PCLIP_REQUIRE_PITCH(fn, lda, D);
    PCLIP_REQUIRE_PITCH(fn, ldb, D);
    PCLIP_REQUIRE((ldta) >= (Dt) && (ldta) % 8 == 0, "%s: ldta=%d must be >= Dt=%d and a multiple of 8 halves", fn, ldta, Dt);
    PCLIP_REQUIRE((ldtb) >= (Dt) && (ldtb) % 8 == 0, "%s: ldtb=%d must be >= Dt=%d and a multiple of 8 halves", fn, ldtb, Dt);
    PCLIP_REQUIRE_ALIGNED(fn, (uintptr_t)a | (uintptr_t)b | (uintptr_t)ta | (uintptr_t)tb, 0);
    PCLIP_REQUIRE(ws != nullptr && (uintptr_t)ws % 16 == 0, "%s: needs a 16-byte aligned workspace", fn);
    if (ws_bytes < need) {
        pclip_set_error("%s: workspace %zu < %zu", fn, ws_bytes, need);
        return PCLIP_E_WORKSPACE;
    }
    return PCLIP_OK;
}

}  // namespace

size_t pclip_cosine_kd_workspace(int backward, int M, int T, int Dx) {
    if (M < 1 || T < 1 || Dx < 1) return 0;
    return backward ? kd_bwd_ws(M, T, Dx).bytes : kd_fwd_ws(M, T, Dx).bytes;
}

extern "C" int pclip_cosine_kd_f16(const void* a, int lda, int M, const void* b, int ldb, int T, int D, float scale, const void* ta, int ldta, const void* tb,
                                   int ldtb, int Dt, float tscale, int flags, float* lse_row, float* tlse_row, float* row_loss, float* loss, void* ws,
                                   size_t ws_bytes, pclip_stream_t stream) {
    const char* fn = "pclip_cosine_kd_f16";
    const int Dx = D > Dt ? D : Dt;
    if (int e = kd_validate(fn, a, lda, M, b, ldb, T, D, scale, ta, ldta, tb, ldtb, Dt, tscale, flags, ws, ws_bytes, pclip_cosine_kd_workspace(0, M, T, Dx))) return e;
    PCLIP_REQUIRE(lse_row && tlse_row && row_loss && loss, "%s: lse_row, tlse_row, row_loss and loss are required", fn);
    hipStream_t s = (hipStream_t)stream;
    const KdFwdWs w = kd_fwd_ws(M, T, Dx);
    char* wsb = (char*)ws;
    // ---- pass 1: the two lse vectors by the cross-entropy forward itself (labels of -1: the lse alone) -----------------------------------------
    int32_t* none = (int32_t*)(wsb + w.labels);
    if (hipMemsetAsync(none, 0xFF, (size_t)M * 4, s) != hipSuccess) {
        pclip_set_error("%s: cannot fill the label vector", fn);
        return PCLIP_E_LAUNCH;
    }
    float* rows_scratch = (float*)(wsb + w.rows);
    float* loss_scratch = (float*)(wsb + w.loss);
    const size_t ce_bytes = pclip_cosine_ce_workspace(0, M, T, Dx);
    const int fs = ((flags & PCLIP_KD_NORMALIZE_A) ? PCLIP_CE_NORMALIZE_A : 0) | ((flags & PCLIP_KD_NORMALIZE_B) ? PCLIP_CE_NORMALIZE_B : 0);
    const int ft = ((flags & PCLIP_KD_NORMALIZE_TA) ? PCLIP_CE_NORMALIZE_A : 0) | ((flags & PCLIP_KD_NORMALIZE_TB) ? PCLIP_CE_NORMALIZE_B : 0);
    if (int e = pclip_cosine_ce_f16(a, lda, M, b, ldb, T, D, scale, fs, none, lse_row, nullptr, rows_scratch, loss_scratch, wsb + w.ce, ce_bytes, stream)) return e;
    if (int e = pclip_cosine_ce_f16(ta, ldta, M, tb, ldtb, T, Dt, tscale, ft, none, tlse_row, nullptr, rows_scratch, loss_scratch, wsb + w.ce, ce_bytes, stream)) return e;
    // ---- pass 2: the walk with both lse known ----------------------------------------------------------------------------------------------------
    const half_t *bw = (const half_t*)b, *tbw = (const half_t*)tb;
    int ldbw = ldb, ldtbw = ldtb;
    if (flags & PCLIP_KD_NORMALIZE_B) {
        if (int e = launch_norm_rows<KD_DMAX>((const half_t*)b, ldb, (half_t*)(wsb + w.bn), T, D, s, "cosine_kd (row norms)")) return e;
        bw = (const half_t*)(wsb + w.bn), ldbw = D;
    }
    if (flags & PCLIP_KD_NORMALIZE_TB) {
        if (int e = launch_norm_rows<KD_DMAX>((const half_t*)tb, ldtb, (half_t*)(wsb + w.tbn), T, Dt, s, "cosine_kd (teacher row norms)")) return e;
        tbw = (const half_t*)(wsb + w.tbn), ldtbw = Dt;
    }
    const int RF = kd_rf_fwd(M, Dx), npanels = ceil_div(M, 16 * RF);
    const size_t lds = (size_t)16 * RF * ((D + PW_PAD) + (Dt + PW_PAD)) * 2;
    if (int e = kd_dispatch(D, Dx, RF, [&](auto nch, auto rf, auto) -> int {
            static DevOnce attr;
            if (int e = pclip_raise_lds(attr, {(const void*)kd_fwd_kernel<nch, rf>}, KD_LDS_MAX, fn)) return e;
            kd_fwd_kernel<nch, rf><<<npanels, 64 * KD_FW, lds, s>>>((const half_t*)a, lda, M, bw, ldbw, T, D, scale, (flags & PCLIP_KD_NORMALIZE_A) ? 1 : 0,
                                                                   (const half_t*)ta, ldta, tbw, ldtbw, Dt, tscale, (flags & PCLIP_KD_NORMALIZE_TA) ? 1 : 0, lse_row,
                                                                   tlse_row, row_loss);
            return pclip_check_launch("cosine_kd");
        }))
        return e;
    kd_sum_kernel<<<1, 256, 0, s>>>(row_loss, M, 1.0 / M, loss);
    return pclip_check_launch("cosine_kd (mean)");
}

extern "C" int pclip_cosine_kd_backward_f16(const void* a, int lda, int M, const void* b, int ldb, int T, int D, float scale, const void* ta, int ldta,
                                            const void* tb, int ldtb, int Dt, float tscale, int flags, const float* lse_row, const float* tlse_row, float weight,
                                            int direction, float* grad, float* dscale, void* ws, size_t ws_bytes, pclip_stream_t stream) {
    const char* fn = "pclip_cosine_kd_backward_f16";
    const int Dx = D > Dt ? D : Dt;
    if (int e = kd_validate(fn, a, lda, M, b, ldb, T, D, scale, ta, ldta, tb, ldtb, Dt, tscale, flags, ws, ws_bytes, pclip_cosine_kd_workspace(1, M, T, Dx))) return e;
    PCLIP_REQUIRE(direction == 0 || direction == 1, "%s: direction=%d must be 0 (dL/da) or 1 (dL/db)", fn, direction);
    PCLIP_REQUIRE(lse_row && tlse_row && grad, "%s: lse_row, tlse_row and grad are required", fn);
    PCLIP_REQUIRE((uintptr_t)grad % 16 == 0, "%s: grad must be 16-byte aligned", fn);
    hipStream_t s = (hipStream_t)stream;
    const KdBwdWs w = kd_bwd_ws(M, T, Dx);
    char* wsb = (char*)ws;
    // own = the side whose gradient this call produces, walked = the other; the teacher's operands go with the student's
    const half_t* own = (const half_t*)(direction ? b : a);
    const half_t* walk = (const half_t*)(direction ? a : b);
    const half_t* town = (const half_t*)(direction ? tb : ta);
    const half_t* twalk = (const half_t*)(direction ? ta : tb);
    const int ldo = direction ? ldb : lda, ldto = direction ? ldtb : ldta, Ro = direction ? T : M, Rw = direction ? M : T;
    int ldw = direction ? lda : ldb, ldtw = direction ? ldta : ldtb;
    const int norm_own = (flags & (direction ? PCLIP_KD_NORMALIZE_B : PCLIP_KD_NORMALIZE_A)) ? 1 : 0;
    const int norm_walk = (flags & (direction ? PCLIP_KD_NORMALIZE_A : PCLIP_KD_NORMALIZE_B)) ? 1 : 0;
    const int norm_town = (flags & (direction ? PCLIP_KD_NORMALIZE_TB : PCLIP_KD_NORMALIZE_TA)) ? 1 : 0;
    const int norm_twalk = (flags & (direction ? PCLIP_KD_NORMALIZE_TA : PCLIP_KD_NORMALIZE_TB)) ? 1 : 0;
    if (norm_walk) {
        if (int e = launch_norm_rows<KD_DMAX>(walk, ldw, (half_t*)(wsb + w.wn), Rw, D, s, "cosine_kd_backward (row norms)")) return e;
        walk = (const half_t*)(wsb + w.wn), ldw = D;
    }
    if (norm_twalk) {
        if (int e = launch_norm_rows<KD_DMAX>(twalk, ldtw, (half_t*)(wsb + w.twn), Rw, Dt, s, "cosine_kd_backward (teacher row norms)")) return e;
        twalk = (const half_t*)(wsb + w.twn), ldtw = Dt;
    }
    half_t* walkT = (half_t*)(wsb + w.wt);
    const int ldt = round64(Rw);
    if (int e = launch_transpose(walk, ldw, Rw, D, walkT, ldt, s, "cosine_kd_backward (transpose)")) return e;

    const int RF = kd_rf(Ro, Dx), npanels = ceil_div(Ro, 16 * RF);
    const int nchunks = kd_chunks(Ro, Rw, Dx, direction == 1);
    float* gpanel = nchunks > 1 ? (float*)(wsb + w.part) : grad;
    const dim3 grid(npanels, nchunks);
    const size_t lds = (size_t)16 * RF * ((D + PW_PAD) + (Dt + PW_PAD)) * 2 + (size_t)2 * 16 * RF * PW_PLD * 2 + 4 * sizeof(float);
    float* dsc_part = dscale ? (float*)(wsb + w.dsc) : nullptr;
    if (int e = kd_dispatch(D, Dx, RF, [&](auto nch, auto rf, auto ndf) -> int {
            static DevOnce attr;
            if (int e = pclip_raise_lds(attr, {(const void*)kd_bwd_kernel<nch, rf, ndf>}, KD_LDS_MAX, fn)) return e;
            kd_bwd_kernel<nch, rf, ndf><<<grid, 256, lds, s>>>(own, ldo, Ro, walk, ldw, Rw, walkT, ldt, D, scale, town, ldto, twalk, ldtw, Dt, tscale, weight, norm_own,
                                                              norm_town, direction == 0 ? 1 : 0, lse_row, tlse_row, gpanel, dsc_part);
            return pclip_check_launch("cosine_kd_backward");
        }))
        return e;
    if (nchunks > 1) {
        const size_t n = (size_t)Ro * D;
        size_t g = (n / 4 + 255) / 256;
        g = g > 4096 ? 4096 : g;
        kd_sum_chunks_kernel<<<(int)g, 256, 0, s>>>(gpanel, nchunks, n, grad);
        if (int e = pclip_check_launch("cosine_kd_backward (chunks)")) return e;
    }
    if (norm_own) {
        int g = ceil_div(Ro, 4);
        g = g > 8192 ? 8192 : g;
        if (D <= 512) kd_norm_backward_kernel<1><<<g, 256, 0, s>>>(own, ldo, grad, Ro, D);
        else if (D <= 1024) kd_norm_backward_kernel<2><<<g, 256, 0, s>>>(own, ldo, grad, Ro, D);
        else kd_norm_backward_kernel<4><<<g, 256, 0, s>>>(own, ldo, grad, Ro, D);
        if (int e = pclip_check_launch("cosine_kd_backward (row norms)")) return e;
    }
    if (dscale) {
        kd_sum_kernel<<<1, 256, 0, s>>>(dsc_part, npanels * nchunks, 1.0, dscale);
        if (int e = pclip_check_launch("cosine_kd_backward (dscale)")) return e;
    }
    return PCLIP_OK;
}
