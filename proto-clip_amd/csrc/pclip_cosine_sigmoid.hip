// The pairwise sigmoid (SigLIP) loss over cosine logits and its gradients, multi-positive by ids: L = 1/M sum_m sum_t softplus(-z[m, t] x[m, t]), z = +1 on positive
// pairs and -1 elsewhere, x = scale cos + bias on the logits of clip/model.py:356-370.  Ragged in M and T; the [M, T] matrix never reaches memory, forward or backward.
// A pair's term depends on that pair alone: no log-sum-exp, no column statistics, one forward pass; any block of a larger batch can be computed on its own.
// Built on the panel walk of pclip_panel_walk.h as pclip_cosine_ce.hip is: the forward from stage_panel and walk_pairs, the backward from stage_panel,
// bwd_first_product, bwd_prefetch_t, bwd_second_product and store_grad_panel; what lies between the two products is this file's own.
// ROUNDING POINTS
//   cos[m, t] = the fp32 MFMA accumulation of a'[m, :] . b'[t, :], ONE accumulator over k = 0, 32, ... D - 32 in that order on every route (forward, either backward
//               direction, any RF, any chunking); a' / b' the fp16 rows as given, or the rows pclip_l2norm_rows_f16 gives (the panel side normalised while it is
//               staged, the walked side normalised into the workspace first, as the cross-entropy does).
//   x         = fma(scale, cos, bias), one fp32 rounding.  Nothing is rounded to fp16 on the way to x.
//   y[m, t]   = 1 iff ids_a[m] == ids_b[t] and ids_a[m] >= 0 (ids widened to 64 bits and compared there; NULL ids: the row / column index): an id is compared,
//               never used as an index.
//   forward   : e = exp(-|x|) (v_exp_f32 of -|x| log2 e: relative error within (|x| + 2) 2^-22), u = 1 + e, log1p(e) = log(u) e / (u - 1) (e itself where u == 1):
//               the quotient undoes the rounding of 1 + e, so that the term keeps a RELATIVE error within 2^-20 (v_log_f32 and v_rcp_f32 at 1 ulp, three
//               multiplications, one addition) where a plain log(1 + e) has an absolute 2^-24 — most terms of a SigLIP row are ~ e^-10.
//               term = max(-z x, 0) + log1p(e);  row_loss[m] = sum_t term in fp32: a lane adds its 16 columns of every eighth block of 64 in ascending order, then
//               the 4 lane groups of a row (xor 16, xor 32), then the 8 waves in wave order — T / 32 + 10 additions deep, the same for any RF, grid or batch.
//               loss = (sum_m row_loss[m]) / M: one workgroup, fp64, a fixed order.
//   backward  : E = sigma(x) = 1 / (1 + e) for x >= 0, e / (1 + e) below (fp32, v_rcp_f32) — the unrounded E gives dscale = sum G o cos and dbias = sum G, G = w (E - y):
//               per lane in fp32 over the tiles in order, the wave, the 4 waves, times weight: one partial per workgroup, then one fixed-order fp64 sum;
//               E enters the second product as r16(2^14 E) (<= 16384, exact scaling, undone in fp32 with weight and scale): relative unit 2^-11 down to E = 2^-28,
//               zero below 2^-39; the target term is a second, EXACT tile (-2^14 at the positives) through the same MFMA into the same accumulator, issued only for
//               tiles in which some wave saw a positive; the sum over the walked index is the fp32 MFMA accumulation in index order; grad = (weight scale 2^-14) acc.
//               Under a normalise flag on the own side the panel gradient is chained through x / ||x|| in fp32 (sig_norm_backward_kernel: ce_norm_backward_kernel's
//               map, restated — that one lives in its unit's unnamed namespace).
// Every workgroup walks its walked rows in index order and an element has one accumulator: a row's loss term and its row of dL/da do not depend on RF, the grid or
// the other rows of a.  The walked tiles are shared between workgroups in fixed chunks, each with a partial fp32 panel summed in chunk order: for dL/db, where the own
// rows are few panels (a 1000-class one-vs-rest probe over 50 000 samples: 16), by sig_chunks, the rule of ce_chunks; for dL/da by sig_chunks_a, a function of T
// ALONE (1 below 2048 walked rows, 4 from 4096), so that a row's bits still depend on b and never on M — its panels shrink (RF changes no bit) until the
// workgroups are enough.  No floating-point atomics.  Only __syncthreads barriers and compiler-counted waits: nothing here for the race-stress build.
#include <cmath>
#include "pclip_panel_walk.h"

namespace {

constexpr int SIG_LDS_MAX = 152 * 1024;          // dynamic LDS asked for: the forward kernel keeps 2 KB of static LDS next to it (the most used is 104 KB)
constexpr int SIG_DMAX = 2048;
constexpr int SIG_FW = 8;                        // waves of a forward workgroup: each walks every eighth block of 64 columns (a constant: a row's merge order never changes)
constexpr float SIG_ESCALE = 16384.f;            // E in [0, 1] enters the fp16 tile as 2^14 E

// an id widened to 64 bits; NULL ids: the index itself (the diagonal)
__device__ __forceinline__ long long load_id(const void* ids, int i64, int i) {
    if (!ids) return (long long)i;
    return i64 ? (long long)reinterpret_cast<const int64_t*>(ids)[i] : (long long)reinterpret_cast<const int32_t*>(ids)[i];
}

// exp(-|x|) and log1p of it (see ROUNDING POINTS)
__device__ __forceinline__ float softplus_neg_abs(float x) {
    const float e = __expf(-fabsf(x));
    const float u = 1.f + e, d = u - 1.f;
    return d > 0.f ? __logf(u) * __fdividef(e, d) : e;
}
__device__ __forceinline__ float sigmoid_f32(float x) {
    const float e = __expf(-fabsf(x));
    const float r = __fdividef(1.f, 1.f + e);
    return x >= 0.f ? r : e * r;
}

template <int NCH, int RF>
__global__ __launch_bounds__(64 * SIG_FW) void sig_fwd_kernel(const half_t* __restrict__ a, int lda, int M, const half_t* __restrict__ b, int ldb, int T, int D, float scale,
                                                      float bias, int norm_a, const void* __restrict__ ids_a, const void* __restrict__ ids_b, int id64,
                                                      float* __restrict__ row_loss) {
    extern __shared__ __attribute__((aligned(16))) char sig_smem[];
    __shared__ float red[SIG_FW][RF][16];
    half_t* panel = reinterpret_cast<half_t*>(sig_smem);                                     // [16 RF][D + 8]
    const int LDP = D + PW_PAD;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m0 = blockIdx.x * 16 * RF;
    stage_panel<NCH, SIG_FW>(panel, LDP, a, lda, M, D, m0, 16 * RF, lane, wave, norm_a);

    const int lr = lane & 15, lq = lane >> 4;
    float rl[RF];
    long long ida[RF];                                                                       // the id of this lane's row per fragment (-1 past the last row: matches nothing)
#pragma unroll
    for (int f = 0; f < RF; ++f) {
        const int m = m0 + 16 * f + lr;
        rl[f] = 0.f;
        ida[f] = m < M ? load_id(ids_a, id64, m) : -1;
    }
    __syncthreads();

    const int KS = D >> 5, ncb = (T + 63) >> 6;
    for (int cb = wave; cb < ncb; cb += SIG_FW) {
        const int t0 = cb * 64;
        const half_t* bp[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) bp[c] = walked_row(b, ldb, t0 + 16 * c + lr, T, lq);
        long long idb[4][4];                                                                 // in flight under the walk
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int t = t0 + 16 * c + 4 * lq + r;
                idb[c][r] = t < T ? load_id(ids_b, id64, t) : -1;
            }
        float4_t acc[RF][4];
        walk_pairs<RF, 4>(bp, panel + (size_t)lr * LDP + lq * 8, LDP, KS, acc);
        // acc[f][c][r] = cos(m0 + 16 f + lr, t0 + 16 c + 4 lq + r)
#pragma unroll
        for (int f = 0; f < RF; ++f)
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int t = t0 + 16 * c + 4 * lq + r;
                    const float x = fmaf(scale, acc[f][c][r], bias);
                    const bool hit = ida[f] >= 0 && ida[f] == idb[c][r];
                    const float term = fmaxf(hit ? -x : x, 0.f) + softplus_neg_abs(x);
                    rl[f] += t < T ? term : 0.f;
                }
    }
    // ---- a row's 4 lane groups, then its SIG_FW waves, in a fixed order ---------------------------------------------------------------------
#pragma unroll
    for (int f = 0; f < RF; ++f) {
        rl[f] += lane_xor<16>(rl[f]);
        rl[f] += lane_xor<32>(rl[f]);
        if (lq == 0) red[wave][f][lr] = rl[f];
    }
    __syncthreads();
    if (threadIdx.x < 16 * RF) {
        const int f = threadIdx.x >> 4, row = threadIdx.x & 15, m = m0 + threadIdx.x;
        if (m < M) {
            float s = red[0][f][row];
            for (int w = 1; w < SIG_FW; ++w) s += red[w][f][row];
            row_loss[m] = s;
        }
    }
}

// out[0] = mul * sum x[0 .. n), one workgroup, fp64, a fixed order
__global__ __launch_bounds__(256) void sig_sum_kernel(const float* __restrict__ x, int n, double mul, float* __restrict__ out) {
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
__global__ __launch_bounds__(256) void sig_sum_chunks_kernel(const float* __restrict__ part, int nchunks, size_t n, float* __restrict__ out) {
    for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += (size_t)gridDim.x * 256 * 4) {
        float4_t s = *reinterpret_cast<const float4_t*>(part + i);
        for (int c = 1; c < nchunks; ++c) s += *reinterpret_cast<const float4_t*>(part + (size_t)c * n + i);
        *reinterpret_cast<float4_t*>(out + i) = s;
    }
}

// "own" = the side whose gradient is produced, "walked" = the other (direction 0: own a, walked b; direction 1 exchanged, i.e. G^T).  Per 64 walked rows, wave w
// recomputes the 16 RF x 16 fragment of cos for walked rows 16 w .. 16 w + 15, forms E = sigma(x) in registers, puts r16(2^14 E) and the target tile in LDS
// [own][walked]; after one barrier every wave accumulates (E + Y) . walked'^T into its quarter of the D columns.  The tiles are double-buffered: one barrier per tile.
// sc_part [2][gridDim.y gridDim.x]: this workgroup's weight sum G o cos, then its weight sum G (either half nullable).
template <int NCH, int RF, int NDF>
__global__ __launch_bounds__(256) void sig_bwd_kernel(const half_t* __restrict__ own, int ldo, int Ro, const half_t* __restrict__ walk, int ldw, int Rw,
                                                      const half_t* __restrict__ walkT, int ldt, int D, float scale, float bias, float weight, int norm_own,
                                                      const void* __restrict__ ids_own, const void* __restrict__ ids_walk, int id64, float* __restrict__ gout,
                                                      float* __restrict__ dsc_part, float* __restrict__ dbs_part) {
    extern __shared__ __attribute__((aligned(16))) char sig_smem[];
    const int LDP = D + PW_PAD;
    half_t* panel = reinterpret_cast<half_t*>(sig_smem);                                     // [16 RF][D + 8]
    half_t* etile = panel + (size_t)16 * RF * LDP;                                           // [2][16 RF][PW_PLD]: r16(2^14 E), own row x walked row
    half_t* ytile = etile + (size_t)2 * 16 * RF * PW_PLD;                                    // [2][16 RF][PW_PLD]: -2^14 at the positives
    int* hitflag = reinterpret_cast<int*>(ytile + (size_t)2 * 16 * RF * PW_PLD);             // [2][4]: wave w saw a positive in its fragment of the tile
    float* sc_red = reinterpret_cast<float*>(hitflag + 8);                                   // [2][4]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i0 = blockIdx.x * 16 * RF;
    stage_panel<NCH, 4>(panel, LDP, own, ldo, Ro, D, i0, 16 * RF, lane, wave, norm_own);

    const int lr = lane & 15, lq = lane >> 4;
    const int ndf = D >> 6, dbase = wave * (D >> 2);
    long long ido[RF];                                                                       // the id of this lane's own row per fragment (-1 past the last row)
#pragma unroll
    for (int f = 0; f < RF; ++f) {
        const int i = i0 + 16 * f + lr;
        ido[f] = i < Ro ? load_id(ids_own, id64, i) : -1;
    }
    float4_t acc2[RF][NDF];
#pragma unroll
    for (int f = 0; f < RF; ++f)
#pragma unroll
        for (int df = 0; df < NDF; ++df) acc2[f][df] = float4_t{0.f, 0.f, 0.f, 0.f};
    float dsc = 0.f, dbs = 0.f;
    __syncthreads();

    // blockIdx.y: this workgroup's chunk of the walked tiles (gridDim.y > 1: gout is that chunk's partial panel, summed in chunk order by sig_sum_chunks_kernel)
    const int KS = D >> 5, ntiles = (Rw + 63) >> 6, tpc = (ntiles + gridDim.y - 1) / gridDim.y;
    const int tile_end = (int)(blockIdx.y + 1) * tpc < ntiles ? (int)(blockIdx.y + 1) * tpc : ntiles;
    gout += (size_t)blockIdx.y * Ro * D;
    const half_t* wp = walked_row(walk, ldw, (int)blockIdx.y * tpc * 64 + 16 * wave + lr, Rw, lq);   // this wave's walked row of the tile at hand (clamped)
    half8_t c0 = ld_half8(wp), c1 = ld_half8(wp + 32);
    const half_t* ap = panel + (size_t)lr * LDP + lq * 8;
    for (int tile = blockIdx.y * tpc; tile < tile_end; ++tile) {
        const int j0 = tile * 64, buf = tile & 1;
        const half_t* wpn = walked_row(walk, ldw, j0 + 64 + 16 * wave + lr, Rw, lq);
        float4_t acc[RF];
        bwd_first_product<RF>(wp, wpn, c0, c1, ap, LDP, KS, acc);
        wp = wpn;
        half8_t wt0[8];
        bwd_prefetch_t(wt0, walkT, ldt, dbase, ndf, j0, lr, lq);
        // acc[f][r] = cos(own i0 + 16 f + lr, walked j0 + 16 wave + 4 lq + r)
        const int jb = j0 + 16 * wave + 4 * lq;
        long long idw[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) idw[r] = jb + r < Rw ? load_id(ids_walk, id64, jb + r) : -1;
        bool anyhit = false;
#pragma unroll
        for (int f = 0; f < RF; ++f) {
            const int i = i0 + 16 * f + lr;
            half4_t e16, y16;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float cosv = acc[f][r];
                const bool ok = i < Ro && jb + r < Rw;
                const float e = ok ? sigmoid_f32(fmaf(scale, cosv, bias)) : 0.f;
                const bool hit = ok && ido[f] >= 0 && ido[f] == idw[r];
                anyhit = anyhit || hit;
                const float g = e - (hit ? 1.f : 0.f);
                dsc += g * cosv;
                dbs += g;
                e16[r] = (half_t)(e * SIG_ESCALE);
                y16[r] = hit ? (half_t)(-SIG_ESCALE) : (half_t)0.f;
            }
            const size_t at = ((size_t)buf * 16 * RF + 16 * f + lr) * PW_PLD + 16 * wave + 4 * lq;
            *reinterpret_cast<half4_t*>(etile + at) = e16;
            *reinterpret_cast<half4_t*>(ytile + at) = y16;
        }
        const int wavehit = __any(anyhit) ? 1 : 0;
        if (lane == 0) hitflag[buf * 4 + wave] = wavehit;
        __syncthreads();                                                                     // the tile is whole; the other buffer is free once every wave is here
        const bool targets = (hitflag[buf * 4] | hitflag[buf * 4 + 1] | hitflag[buf * 4 + 2] | hitflag[buf * 4 + 3]) != 0;
        // ---- this wave's quarter of D: acc2 += walked'^T (E + Y), the walked index along k ------------------------------------------------
        bwd_second_product<RF, NDF, true>(walkT, ldt, dbase, ndf, j0, wt0, etile, ytile, targets, buf, lr, lq, acc2);
    }
    // acc2[f][df][r] = 2^14 sum_j (E - y)[i0 + 16 f + lr, j] walked'[j, dbase + 16 df + 4 lq + r]
    store_grad_panel<RF, NDF>(gout, i0, Ro, D, dbase, ndf, weight * scale * (1.f / SIG_ESCALE), lr, lq, acc2);
    if (dsc_part || dbs_part) {
        dsc = wave_sum(dsc);
        dbs = wave_sum(dbs);
        if (lane == 0) sc_red[wave] = dsc, sc_red[4 + wave] = dbs;
        __syncthreads();
        if (threadIdx.x == 0) {
            const size_t at = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
            if (dsc_part) dsc_part[at] = weight * (((sc_red[0] + sc_red[1]) + sc_red[2]) + sc_red[3]);
            if (dbs_part) dbs_part[at] = weight * (((sc_red[4] + sc_red[5]) + sc_red[6]) + sc_red[7]);
        }
    }
}

// g <- (g - y (y . g)) / ||x||, y = x / ||x|| in fp32: the gradient of x -> x / ||x|| applied to a row of dL/dx' in place (one wave per row)
template <int NCH>
__global__ __launch_bounds__(256) void sig_norm_backward_kernel(const half_t* __restrict__ x, int ldx, float* __restrict__ g, int R, int D) {
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

// Smaller panels until there are `target` workgroups (`chunks` of them per panel): a row's bits do not depend on RF
inline int sig_rf_spread(int R, int D, int chunks, int target) {
    int rf = rf_for(R, D);
    while (rf > 1 && ceil_div(R, 16 * rf) * chunks < target) rf >>= 1;
    return rf;
}
constexpr int SIG_WG_TARGET = 512;
// dL/da: a row's bits may depend on b but not on M, so the walk is shared in a number of chunks that T ALONE decides: one per 16 tiles (1024 walked rows), 4 at
// the most (T >= 4096) — the partial panels are 4 M D floats at the most.  Each workgroup's walk is a chain of dependent fetches per tile: a quarter of the chain.
inline int sig_chunks_a(int T) {
    const int n = ceil_div(T, 64) / 16;
    return n < 1 ? 1 : (n > 4 ? 4 : n);
}
// dL/db over few own panels: the walked tiles shared between up to SIG_WG_TARGET / panels workgroups, each with a partial fp32 panel in ws, summed in chunk
// order.  A function of the shape alone, never of the device; the partials stay within 4 (M + T) D floats.
inline int sig_chunks(int Ro, int Rw, int D) {
    const int npanels = ceil_div(Ro, 16 * rf_for(Ro, D)), ntiles = ceil_div(Rw, 64);
    int n = ceil_div(SIG_WG_TARGET, npanels);
    const int cap = (int)(4 * ((size_t)Ro + Rw) / Ro);
    n = n > cap ? cap : n;
    n = n > ntiles ? ntiles : n;
    n = n > 65535 ? 65535 : n;
    return n < 1 ? 1 : n;
}
struct SigBwdWs {
    size_t wn, wt, red, part, bytes;
};
inline SigBwdWs sig_bwd_ws(int M, int T, int D) {      // either direction fits: sized by the larger side
    const int R = M > T ? M : T;
    const int ca = sig_chunks_a(T), cb = sig_chunks(T, M, D);
    const size_t pa = ca > 1 ? (size_t)ca * M : 0, pb = cb > 1 ? (size_t)cb * T : 0;
    const size_t ra = (size_t)ca * ceil_div(M, 16), rb = (size_t)cb * ceil_div(T, 16);
    SigBwdWs w;
    size_t off = 0;
    w.wn = off, off += align_up((size_t)R * D * 2, 256);
    w.wt = off, off += align_up((size_t)D * round64(R) * 2, 256);
    w.red = off, off += 2 * align_up((ra > rb ? ra : rb) * 4, 256);
    w.part = off, off += align_up((pa > pb ? pa : pb) * D * 4, 256);
    w.bytes = off;
    return w;
}

int sig_validate(const char* fn, const void* a, int lda, int M, const void* b, int ldb, int T, int D, float scale, float bias, int flags, const void* ids_a,
                 const void* ids_b, const void* ws, size_t ws_bytes, size_t need) {
    PCLIP_REQUIRE(a && b, "%s: null operand", fn);
    PCLIP_REQUIRE(M >= 1 && T >= 1, "%s: M=%d and T=%d must be positive", fn, M, T);
    PCLIP_REQUIRE(D > 0 && D % 64 == 0, "%s: D=%d must be a multiple of 64", fn, D);
    PCLIP_REQUIRE(D <= SIG_DMAX, "%s: D=%d is past the envelope (D <= %d)", fn, D, SIG_DMAX);
    PCLIP_REQUIRE((flags & ~(PCLIP_SIG_NORMALIZE_A | PCLIP_SIG_NORMALIZE_B | PCLIP_SIG_IDS_I64)) == 0, "%s: unknown flag bits 0x%x", fn, flags);
    PCLIP_REQUIRE(std::isfinite(scale), "%s: scale must be finite", fn);
    PCLIP_REQUIRE(std::isfinite(bias), "%s: bias must be finite", fn);
    PCLIP_REQUIRE((ids_a == nullptr) == (ids_b == nullptr), "%s: ids_a and ids_b go together (both NULL: the diagonal)", fn);
    if (!ids_a) {
        PCLIP_REQUIRE(M == T, "%s: NULL ids are the diagonal and need M == T (M=%d, T=%d)", fn, M, T);
    } else {
        const uintptr_t al = (flags & PCLIP_SIG_IDS_I64) ? 8 : 4;
        PCLIP_REQUIRE((uintptr_t)ids_a % al == 0 && (uintptr_t)ids_b % al == 0, "%s: misaligned ids_a / ids_b", fn);
    }
    PCLIP_REQUIRE_PITCH(fn, lda, D);
    PCLIP_REQUIRE_PITCH(fn, ldb, D);
    PCLIP_REQUIRE_ALIGNED(fn, (uintptr_t)a | (uintptr_t)b, 0);
    PCLIP_REQUIRE(ws != nullptr && (uintptr_t)ws % 16 == 0, "%s: needs a 16-byte aligned workspace", fn);
    if (ws_bytes < need) {
        pclip_set_error("%s: workspace %zu < %zu", fn, ws_bytes, need);
        return PCLIP_E_WORKSPACE;
    }
    return PCLIP_OK;
}

}  // namespace

size_t pclip_cosine_sigmoid_workspace(int backward, int M, int T, int D) {
    if (M < 1 || T < 1 || D < 1) return 0;
    return backward ? sig_bwd_ws(M, T, D).bytes : align_up((size_t)T * D * 2, 256);
}

extern "C" int pclip_cosine_sigmoid_f16(const void* a, int lda, int M, const void* b, int ldb, int T, int D, float scale, float bias, int flags, const void* ids_a,
                                        const void* ids_b, float* row_loss, float* loss, void* ws, size_t ws_bytes, pclip_stream_t stream) {
    const char* fn = "pclip_cosine_sigmoid_f16";
    if (int e = sig_validate(fn, a, lda, M, b, ldb, T, D, scale, bias, flags, ids_a, ids_b, ws, ws_bytes, pclip_cosine_sigmoid_workspace(0, M, T, D))) return e;
    PCLIP_REQUIRE(row_loss && loss, "%s: row_loss and loss are required", fn);
    hipStream_t s = (hipStream_t)stream;
    const half_t* bw = (const half_t*)b;
    int ldbw = ldb;
    if (flags & PCLIP_SIG_NORMALIZE_B) {
        if (int e = launch_norm_rows<SIG_DMAX>((const half_t*)b, ldb, (half_t*)ws, T, D, s, "cosine_sigmoid (row norms)")) return e;
        bw = (const half_t*)ws;
        ldbw = D;
    }
    const int RF = sig_rf_spread(M, D, 1, 256), npanels = ceil_div(M, 16 * RF);                    // (the forward has no other source of workgroups than its panels)
    const size_t lds = (size_t)16 * RF * (D + PW_PAD) * 2;
    if (int e = panel_dispatch(D, RF, [&](auto nch, auto rf, auto) -> int {
            static DevOnce attr;
            if (int e = pclip_raise_lds(attr, {(const void*)sig_fwd_kernel<nch, rf>}, SIG_LDS_MAX, fn)) return e;
            sig_fwd_kernel<nch, rf><<<npanels, 64 * SIG_FW, lds, s>>>((const half_t*)a, lda, M, bw, ldbw, T, D, scale, bias, (flags & PCLIP_SIG_NORMALIZE_A) ? 1 : 0, ids_a,
                                                                    ids_b, (flags & PCLIP_SIG_IDS_I64) ? 1 : 0, row_loss);
            return pclip_check_launch("cosine_sigmoid");
        }))
        return e;
    sig_sum_kernel<<<1, 256, 0, s>>>(row_loss, M, 1.0 / M, loss);
    return pclip_check_launch("cosine_sigmoid (mean)");
}

extern "C" int pclip_cosine_sigmoid_backward_f16(const void* a, int lda, int M, const void* b, int ldb, int T, int D, float scale, float bias, int flags,
                                                 const void* ids_a, const void* ids_b, float weight, int direction, float* grad, float* dscale, float* dbias,
                                                 void* ws, size_t ws_bytes, pclip_stream_t stream) {
    const char* fn = "pclip_cosine_sigmoid_backward_f16";
    if (int e = sig_validate(fn, a, lda, M, b, ldb, T, D, scale, bias, flags, ids_a, ids_b, ws, ws_bytes, pclip_cosine_sigmoid_workspace(1, M, T, D))) return e;
    PCLIP_REQUIRE(direction == 0 || direction == 1, "%s: direction=%d must be 0 (dL/da) or 1 (dL/db)", fn, direction);
    PCLIP_REQUIRE(std::isfinite(weight), "%s: weight must be finite", fn);
    PCLIP_REQUIRE(grad && (uintptr_t)grad % 16 == 0, "%s: grad is required and must be 16-byte aligned", fn);
    hipStream_t s = (hipStream_t)stream;
    const SigBwdWs w = sig_bwd_ws(M, T, D);
    char* wsb = (char*)ws;
    // own = the side whose gradient this call produces, walked = the other
    const half_t* own = (const half_t*)(direction ? b : a);
    const half_t* walk = (const half_t*)(direction ? a : b);
    const int ldo = direction ? ldb : lda, Ro = direction ? T : M, Rw = direction ? M : T;
    int ldw = direction ? lda : ldb;
    const int norm_own = (flags & (direction ? PCLIP_SIG_NORMALIZE_B : PCLIP_SIG_NORMALIZE_A)) ? 1 : 0;
    const int norm_walk = (flags & (direction ? PCLIP_SIG_NORMALIZE_A : PCLIP_SIG_NORMALIZE_B)) ? 1 : 0;
    const void* ids_own = direction ? ids_b : ids_a;
    const void* ids_walk = direction ? ids_a : ids_b;
    if (norm_walk) {
        if (int e = launch_norm_rows<SIG_DMAX>(walk, ldw, (half_t*)(wsb + w.wn), Rw, D, s, "cosine_sigmoid_backward (row norms)")) return e;
        walk = (const half_t*)(wsb + w.wn);
        ldw = D;
    }
    half_t* walkT = (half_t*)(wsb + w.wt);
    const int ldt = round64(Rw);
    if (int e = launch_transpose(walk, ldw, Rw, D, walkT, ldt, s, "cosine_sigmoid_backward (transpose)")) return e;

    // dL/da: chunks by T alone, over panels that shrink until there are enough workgroups; dL/db: rf_for's panels, the chunks by the shape
    const int nchunks = direction ? sig_chunks(Ro, Rw, D) : sig_chunks_a(Rw);
    const int RF = direction ? rf_for(Ro, D) : sig_rf_spread(Ro, D, nchunks, SIG_WG_TARGET), npanels = ceil_div(Ro, 16 * RF);
    float* gpanel = nchunks > 1 ? (float*)(wsb + w.part) : grad;
    const dim3 grid(npanels, nchunks);
    const size_t lds = (size_t)16 * RF * (D + PW_PAD) * 2 + (size_t)4 * 16 * RF * PW_PLD * 2 + 8 * sizeof(int) + 8 * sizeof(float);
    const size_t nparts = (size_t)npanels * nchunks;
    float* dsc_part = dscale ? (float*)(wsb + w.red) : nullptr;
    float* dbs_part = dbias ? (float*)(wsb + w.red) + nparts : nullptr;
    if (int e = panel_dispatch(D, RF, [&](auto nch, auto rf, auto ndf) -> int {
            static DevOnce attr;
            if (int e = pclip_raise_lds(attr, {(const void*)sig_bwd_kernel<nch, rf, ndf>}, SIG_LDS_MAX, fn)) return e;
            sig_bwd_kernel<nch, rf, ndf><<<grid, 256, lds, s>>>(own, ldo, Ro, walk, ldw, Rw, walkT, ldt, D, scale, bias, weight, norm_own, ids_own, ids_walk,
                                                               (flags & PCLIP_SIG_IDS_I64) ? 1 : 0, gpanel, dsc_part, dbs_part);
            return pclip_check_launch("cosine_sigmoid_backward");
        }))
        return e;
    if (nchunks > 1) {
        const size_t n = (size_t)Ro * D;
        size_t g = (n / 4 + 255) / 256;
        g = g > 4096 ? 4096 : g;
        sig_sum_chunks_kernel<<<(int)g, 256, 0, s>>>(gpanel, nchunks, n, grad);
        if (int e = pclip_check_launch("cosine_sigmoid_backward (chunks)")) return e;
    }
    if (norm_own) {
        int g = ceil_div(Ro, 4);
        g = g > 8192 ? 8192 : g;
        if (D <= 512) sig_norm_backward_kernel<1><<<g, 256, 0, s>>>(own, ldo, grad, Ro, D);
        else if (D <= 1024) sig_norm_backward_kernel<2><<<g, 256, 0, s>>>(own, ldo, grad, Ro, D);
        else sig_norm_backward_kernel<4><<<g, 256, 0, s>>>(own, ldo, grad, Ro, D);
        if (int e = pclip_check_launch("cosine_sigmoid_backward (row norms)")) return e;
    }
    if (dscale) {
        sig_sum_kernel<<<1, 256, 0, s>>>(dsc_part, (int)nparts, 1.0, dscale);
        if (int e = pclip_check_launch("cosine_sigmoid_backward (dscale)")) return e;
    }
    if (dbias) {
        sig_sum_kernel<<<1, 256, 0, s>>>(dbs_part, (int)nparts, 1.0, dbias);
        if (int e = pclip_check_launch("cosine_sigmoid_backward (dbias)")) return e;
    }
    return PCLIP_OK;
}
