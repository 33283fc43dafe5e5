// Tip-Adapter's cache logits (Tip-Adapter's main.py: `affinity = features @ cache_keys`, `cache_logits = ((-1) * (beta - beta * affinity)).exp() @ cache_values`,
// `tip_logits = 100. * features @ clip_weights + cache_logits * alpha`) with the one-hot `cache_values` taken as what it is: class n owns the contiguous
// key rows seg[n] .. seg[n + 1] - 1.  Neither the [Q, NK] affinities nor (with the argmax alone, or on the grid) the [Q, N] logits reach memory.
//   aff[q, j]  = fp32 MFMA accumulation of f[q, :] . keys[j, :], one accumulator over k = 0, 32, ... D - 32            (never rounded to fp16)
//   E[q, j]    = __expf(fmaf(beta, aff, -beta))                                                                          (fp32)
//   S[q, n]    = (((0 + E[q, seg[n]]) + E[q, seg[n] + 1]) + ...) + E[q, seg[n + 1] - 1]: ONE fp32 accumulator per (q, n), strictly in ascending j
//   c[q, n]    = the accumulator of cosine_logits_kernel before its rounding: r16(scale * f) against w, the class rows as the first MFMA operand, same k order
//   logit[q,n] = r16(fmaf(alpha, S, c))                                                                                  (one fma, one fp16 rounding)
// The panel walk of pclip_panel_walk.h.  The key gradient is built from its staging and its recomputing-backward skeleton; tip_kernel keeps its staging and its two
// one-step-ahead walks written out (its schedule at the ImageNet split moved by 2 % with either of them behind a function: profiles/panel_walk_refactor.txt).
// A workgroup (four waves) owns a panel of 16 RF query rows, in LDS once and unscaled (the zero-shot product scales its fragments on the way to the MFMA), and
// walks the classes in blocks of 64:
//   * zero-shot tile: wave w forms c for classes n0 + 16 w .. + 15 against the whole panel -> LDS [query][class];
//   * the key rows of the block, seg[n0] .. seg[n0 + 64] - 1, in tiles of 64 from seg[n0] on: wave w forms aff for rows jt + 16 w .. + 15, takes the exponentials
//     in registers (NB of them on the grid: one affinity tile serves a whole beta chunk) and puts E in LDS [query][row]; after a barrier thread (query, part)
//     adds the rows of the classes c % P == part that the tile holds onto S[query][c] in LDS, row by row: a class that crosses a tile boundary goes on from
//     the value the previous tile left, so the association above holds whatever the tiles, the panel or the grid are.  Rows past the block or past NK are
//     clamped reads whose E nobody adds;
//   * the block's logits from S and c: written (fp16 and / or fp32) with a thread per class, so stores are contiguous, and folded into the per-query best key
//     (logit_key of pclip_panel_walk.h: value, then lower column) that lives in registers across the blocks.
// Grid kernel: blockIdx.y is a chunk of TP_NBG betas; every (beta, alpha) pair of the chunk keeps its best key per query in registers, the keys are merged
// across a query's threads with integer LDS maxima, compared with the label and counted; the counts are integer sums (LDS, then one global integer atomic per pair and
// workgroup), so they carry no order.  No floating-point atomics anywhere.
// Key gradient (tip_bwd_kernel; the model is direction 1 of ce_bwd_kernel in pclip_cosine_ce.hip): dkeys[j, :] = alpha beta sum_q dL[q, class(j)] E[q, j] f[q, :].
//   A workgroup owns a panel of 16 RF key rows in LDS and walks ALL queries in tiles of 64, in index order: wave w recomputes aff and E for queries q0 + 16 w .. + 15
//   against the panel, forms G = dL[q, class(j)] E in fp32, rounds 2^s G to fp16 (s from max |dL|, found by a first launch: 2^s max |dL| in (2^13, 2^14], so the
//   relative unit 2^-11 holds down to |G| = 2^-27 max |dL| and a loss scaled by a power of two moves s with it) into LDS [key][query]; after one barrier (the tile is
//   double-buffered) every wave accumulates G f over the tile into ITS quarter of the D columns of the fp32 panel, the queries transposed in ws so that the operand
//   is one 16-byte load per lane.  alpha beta 2^-s acts in fp32 at the end.  One accumulator per element over the queries in order, whatever RF or NK: a key row's
//   gradient does not depend on the other key rows, and two calls give the same bits.  The walk is not shared between workgroups: a training batch is a few tiles.
// Only __syncthreads barriers and compiler-counted waits: nothing here for the race-stress build.
// What bounds it: the segment sums are one thread per (query, class) — with fewer than 64 / P classes in a tile (more than ~16 shots per class) threads idle there;
// and the grid's argmax is Q N nb na fma + round + key + max on the VALU, which no tiling removes.  profiles/tip_adapter.txt.
#include "pclip_panel_walk.h"

namespace {

constexpr int TP_CB = 64;                      // classes per block = key rows per tile
constexpr int TP_TLD = 65;                     // floats per LDS row of the c / S / E tiles (64 + 1: a column is read by consecutive queries conflict-free)
constexpr int TP_LDS_MAX = 160 * 1024;
#ifndef PCLIP_TIP_NBG
#define PCLIP_TIP_NBG 2                        // (tools/tip_adapter_bench.py --lib times a library built with another value)
#endif
constexpr int TP_NBG = PCLIP_TIP_NBG;          // betas per chunk of the grid kernel: 2, measured against 1 and 4 (profiles/tip_adapter.txt)
constexpr int TP_NA = 32;                      // alphas of the grid kernel: its best keys are TP_NBG x TP_NA registers

__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
#define PCLIP_STEP(OFF) do { const unsigned o = (unsigned)lane_xor_i<OFF>((int)v); v = o > v ? o : v; } while (0)
    PCLIP_BUTTERFLY(PCLIP_STEP);
#undef PCLIP_STEP
    return v;
}

// v = fma(alpha, S, c) rounded to fp32, THEN to fp16: two roundings, so that the fp16 logit is the rounding of the fp32 logit the taped path gets (left to itself the
// compiler makes the pair one v_fma_mixlo_f16, whose fp16 result is not always the rounding of the fp32 one)
__device__ __forceinline__ half_t tip_logit(float alpha, float s, float c, float& v) {
    v = __builtin_fmaf(alpha, s, c);
    asm volatile("" : "+v"(v));                                                              // (the conversion sees a register, not the fma)
    return (half_t)v;
}

template <int NCH, int RF, int NB, bool GRID>
__global__ __launch_bounds__(256) void tip_kernel(const half_t* __restrict__ f, int ldf, int Q, const half_t* __restrict__ keys, int ldk, int NK,
                                                  const int32_t* __restrict__ seg, const half_t* __restrict__ w, int ldw, int N, int D, float scale, float alpha,
                                                  float beta, const float* __restrict__ betas, int nb, const float* __restrict__ alphas, int na,
                                                  const int32_t* __restrict__ labels, half_t* __restrict__ logits, int ldl, float* __restrict__ logits32,
                                                  int32_t* __restrict__ argmax, int32_t* __restrict__ correct) {
    constexpr int R = 16 * RF, P = 256 / R, TILE = R * TP_TLD;
    extern __shared__ __attribute__((aligned(16))) char tp_smem[];
    const int LDP = D + PW_PAD;
    half_t* panel = reinterpret_cast<half_t*>(tp_smem);                                      // [R][D + 8]
    float* ctile = reinterpret_cast<float*>(panel + (size_t)R * LDP);                        // [R][65]: c of the class block
    float* stile = ctile + TILE;                                                             // [NB][R][65]: S of the class block
    float* etile = stile + NB * TILE;                                                        // [NB][R][65]: E of the key tile; at the end of the grid kernel the merged keys
    int* segl = reinterpret_cast<int*>(etile + NB * TILE);                                   // [65]: seg[n0 .. n0 + 64], clamped to seg[N]
    int* cnt = segl + TP_CB + 1;                                                             // [NB * 32]: this workgroup's correct counts
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, tid = threadIdx.x;
    const int m0 = blockIdx.x * R;
    const int lr = lane & 15, lq = lane >> 4;
    const int KS = D >> 5;

    // ---- the panel: the query rows as given; rows >= Q are zeros and never read from memory ----------------------------------------------
    for (int r = wave; r < R; r += 4) {
        RowRegs<NCH> rr;
        if (m0 + r < Q) {                                                                    // (wave-uniform)
            load_row<NCH>(f + (size_t)(m0 + r) * ldf, D, lane, rr);
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
    float bet[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        if constexpr (GRID) {
            const int ib = blockIdx.y * NB + b;
            bet[b] = betas[ib < nb ? ib : nb - 1];                                           // (a chunk past nb repeats the last beta; its counts are dropped)
        } else {
            bet[b] = beta;
        }
    }
    float al[GRID ? TP_NA : 1];                                                              // the grid's alphas, read once (uniform: scalar registers)
    if constexpr (GRID) {
#pragma unroll
        for (int ia = 0; ia < TP_NA; ++ia) al[ia] = alphas[ia < na ? ia : na - 1];
    }
    // best keys: forward — query wave + 4 i, this lane's class of every block; grid — this thread's query, its classes c % P == part, per (beta, alpha)
    unsigned best[GRID ? NB * TP_NA : 4 * RF];
#pragma unroll
    for (int i = 0; i < (GRID ? NB * TP_NA : 4 * RF); ++i) best[i] = 0;
    const int sq = tid % R, sp = tid / R;                                                    // segment sums (and the grid's logits): query, part
    const half_t* ap = panel + (size_t)lr * LDP + lq * 8;
    __syncthreads();                                                                         // the panel is whole

    const int nstep = GRID ? TP_CB : (int)gridDim.y * TP_CB;                                 // (forward without argmax: the class blocks are shared between gridDim.y workgroups)
    for (int n0 = GRID ? 0 : (int)blockIdx.y * TP_CB; n0 < N; n0 += nstep) {
        const int nc = N - n0 < TP_CB ? N - n0 : TP_CB;
        if (tid <= TP_CB) segl[tid] = seg[n0 + tid < N ? n0 + tid : N];
        for (int i = tid; i < NB * TILE; i += 256) stile[i] = 0.f;
        // ---- zero-shot tile: classes n0 + 16 wave .. + 15 (clamped to N - 1, dropped later) against r16(scale * panel) ---------------------
        {
            int n = n0 + 16 * wave + lr;
            n = n < N ? n : N - 1;
            const half_t* bp = w + (size_t)n * ldw + lq * 8;
            float4_t acc[RF];
#pragma unroll
            for (int fr = 0; fr < RF; ++fr) acc[fr] = float4_t{0.f, 0.f, 0.f, 0.f};
            half8_t bf = ld_half8(bp);
            for (int ks = 0; ks < KS; ++ks) {
                const int kn = ks + 1 < KS ? ks + 1 : ks;                                    // (the last step re-reads its own fragment: no read past column D)
                const half8_t bn = ld_half8(bp + kn * 32);
#pragma unroll
                for (int fr = 0; fr < RF; ++fr) {
                    half8_t af = ld_half8(ap + (size_t)fr * 16 * LDP + ks * 32);
#pragma unroll
                    for (int j = 0; j < 8; ++j) af[j] = scale_r16(scale, af[j]);
                    acc[fr] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bf, af, acc[fr], 0, 0, 0);
                }
                bf = bn;
            }
            // acc[fr][r] = c(m0 + 16 fr + lr, n0 + 16 wave + 4 lq + r)
#pragma unroll
            for (int fr = 0; fr < RF; ++fr)
#pragma unroll
                for (int r = 0; r < 4; ++r) ctile[(16 * fr + lr) * TP_TLD + 16 * wave + 4 * lq + r] = acc[fr][r];
        }
        __syncthreads();                                                                     // segl, the zeroed S and c are whole
        const int jb = segl[0], je = segl[nc] < NK ? segl[nc] : NK;                         // (never past the key rows, whatever seg holds)
        for (int jt = jb; jt < je; jt += TP_CB) {
            // ---- affinities of key rows jt + 16 wave .. + 15 (clamped into [0, NK)) against the panel ---------------------------------------
            {
                int j = jt + 16 * wave + lr;
                j = j < NK ? j : NK - 1;
                j = j < 0 ? 0 : j;
                const half_t* kp = keys + (size_t)j * ldk + lq * 8;
                float4_t acc[RF];
#pragma unroll
                for (int fr = 0; fr < RF; ++fr) acc[fr] = float4_t{0.f, 0.f, 0.f, 0.f};
                half8_t kf = ld_half8(kp);
                for (int ks = 0; ks < KS; ++ks) {
                    const int kn = ks + 1 < KS ? ks + 1 : ks;
                    const half8_t kn8 = ld_half8(kp + kn * 32);
#pragma unroll
                    for (int fr = 0; fr < RF; ++fr)
                        acc[fr] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, ld_half8(ap + (size_t)fr * 16 * LDP + ks * 32), acc[fr], 0, 0, 0);
                    kf = kn8;
                }
                // acc[fr][r] = aff(m0 + 16 fr + lr, jt + 16 wave + 4 lq + r)
#pragma unroll
                for (int b = 0; b < NB; ++b)
#pragma unroll
                    for (int fr = 0; fr < RF; ++fr)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            etile[b * TILE + (16 * fr + lr) * TP_TLD + 16 * wave + 4 * lq + r] = __expf(__builtin_fmaf(bet[b], acc[fr][r], -bet[b]));
            }
            // the classes of the block that own row jt and the tile's last row: the c with segl[c] <= j < segl[c + 1] (uniform; LDS broadcasts)
            const int jl = (jt + TP_CB < je ? jt + TP_CB : je) - 1;
            int cfirst = 0, clast = 0;
            {
                int lo = 0, hi = nc - 1;
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (segl[mid + 1] <= jt) lo = mid + 1; else hi = mid; }
                cfirst = lo;
                hi = nc - 1;
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (segl[mid + 1] <= jl) lo = mid + 1; else hi = mid; }
                clast = lo;
            }
            __syncthreads();                                                                 // the E tile is whole
            // ---- segment sums: thread (query sq, part sp) takes the classes c % P == sp, each in ascending row order onto its one accumulator ---
            for (int c = cfirst + ((sp - cfirst) & (P - 1)); c <= clast; c += P) {
                int lo = segl[c], hi = segl[c + 1];
                lo = lo > jt ? lo : jt;
                hi = hi < jt + TP_CB ? hi : jt + TP_CB;
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    float s = stile[b * TILE + sq * TP_TLD + c];
                    const float* e = etile + b * TILE + sq * TP_TLD;
                    for (int j = lo - jt; j < hi - jt; ++j) s += e[j];
                    stile[b * TILE + sq * TP_TLD + c] = s;
                }
            }
            __syncthreads();                                                                 // the E tile is free, S is whole
        }
        // ---- the block's logits ------------------------------------------------------------------------------------------------------------
        if constexpr (!GRID) {
            const int cl = lane, n = n0 + cl;                                                // a thread per class: contiguous stores
#pragma unroll
            for (int i = 0; i < 4 * RF; ++i) {
                const int q = wave + 4 * i, m = m0 + q;
                if (cl < nc && m < Q) {
                    float v;
                    const half_t h = tip_logit(alpha, stile[q * TP_TLD + cl], ctile[q * TP_TLD + cl], v);
                    if (logits) logits[(size_t)m * ldl + n] = h;
                    if (logits32) logits32[(size_t)m * N + n] = v;
                    const unsigned key = logit_key(h, n);
                    best[i] = key > best[i] ? key : best[i];
                }
            }
        } else {
            for (int c = sp; c < nc; c += P) {
                const float cv = ctile[sq * TP_TLD + c];
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    const float s = stile[b * TILE + sq * TP_TLD + c];
#pragma unroll
                    for (int ia = 0; ia < TP_NA; ++ia) {
                        if (ia < na) {                                                       // (uniform)
                            float v;
                            const unsigned key = logit_key(tip_logit(al[ia], s, cv, v), n0 + c);
                            best[b * TP_NA + ia] = key > best[b * TP_NA + ia] ? key : best[b * TP_NA + ia];
                        }
                    }
                }
            }
        }
        __syncthreads();                                                                     // c, S and segl are free for the next block
    }

    if constexpr (!GRID) {
        if (argmax) {
#pragma unroll
            for (int i = 0; i < 4 * RF; ++i) {
                const unsigned k = wave_max_u32(best[i]);
                const int m = m0 + wave + 4 * i;
                if (lane == 0 && m < Q) argmax[m] = (int)(0xFFFFu - (k & 0xFFFFu));
            }
        }
    } else {
        // ---- merge a query's P threads (integer maxima in LDS), compare with the label, count ---------------------------------------------------
        unsigned* bestl = reinterpret_cast<unsigned*>(etile);                                // [R][NB * 32]
        for (int i = tid; i < R * NB * TP_NA; i += 256) bestl[i] = 0;
        if (tid < NB * TP_NA) cnt[tid] = 0;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NB * TP_NA; ++i)
            if ((i & (TP_NA - 1)) < na) atomicMax(&bestl[sq * NB * TP_NA + i], best[i]);
        __syncthreads();
        for (int i = tid; i < R * NB * TP_NA; i += 256) {
            const int q = i / (NB * TP_NA), pair = i % (NB * TP_NA), m = m0 + q;
            if (m < Q && (pair & (TP_NA - 1)) < na) {
                const int idx = (int)(0xFFFFu - (bestl[i] & 0xFFFFu));
                if (idx == labels[m]) atomicAdd(&cnt[pair], 1);
            }
        }
        __syncthreads();
        if (tid < NB * TP_NA) {
            const int b = tid / TP_NA, ia = tid % TP_NA, ib = blockIdx.y * NB + b;
            if (ib < nb && ia < na && cnt[tid]) atomicAdd(&correct[(size_t)ib * na + ia], cnt[tid]);
        }
    }
}

// ---- the key gradient ---------------------------------------------------------------------------------------------------------------------------
// cls[j] = the class that owns key row j (the c with seg[c] <= j < seg[c + 1]; N - 1 where seg says none), and gmax = the bits of max |dL| (integer maximum)
__global__ __launch_bounds__(256) void tip_bwd_prep_kernel(const int32_t* __restrict__ seg, int N, int NK, int32_t* __restrict__ cls, const float* __restrict__ dL,
                                                           size_t ndl, unsigned* __restrict__ gmax) {
    const size_t t0 = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    for (size_t j = t0; j < (size_t)NK; j += stride) {
        int lo = 0, hi = N - 1;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (seg[mid + 1] <= (int)j) lo = mid + 1; else hi = mid; }
        cls[j] = lo;
    }
    unsigned m = 0;
    for (size_t i = t0; i < ndl; i += stride) {
        const unsigned b = __builtin_bit_cast(unsigned, dL[i]) & 0x7FFFFFFFu;
        m = b > m ? b : m;
    }
    m = wave_max_u32(m);
    if ((threadIdx.x & 63) == 0 && m) atomicMax(gmax, m);
}

// NDF: the 16-column fragments of one wave's quarter of D the kernel is compiled for (D / 64 <= NDF of them are live)
template <int NCH, int RF, int NDF>
__global__ __launch_bounds__(256) void tip_bwd_kernel(const half_t* __restrict__ keys, int ldk, int NK, const half_t* __restrict__ f, int ldf, int Q,
                                                      const half_t* __restrict__ fT, int ldt, int D, float alpha, float beta, const int32_t* __restrict__ cls,
                                                      const float* __restrict__ dL, int N, const unsigned* __restrict__ gmax, float* __restrict__ gout) {
    extern __shared__ __attribute__((aligned(16))) char tp_smem[];
    const int LDP = D + PW_PAD;
    half_t* panel = reinterpret_cast<half_t*>(tp_smem);                                      // [16 RF][D + 8]: this workgroup's key rows
    half_t* gtile = panel + (size_t)16 * RF * LDP;                                           // [2][16 RF][PW_PLD]: r16(2^s G), key row x query
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i0 = blockIdx.x * 16 * RF;
    stage_panel<NCH, 4>(panel, LDP, keys, ldk, NK, D, i0, 16 * RF, lane, wave, 0);
    // 2^s: max |dL| = m 2^e with m in [0.5, 1), s = 14 - e (capped: a gradient of denormals keeps a finite scale)
    float gs = 1.f, ginv = 1.f;
    {
        const float gm = __builtin_bit_cast(float, gmax[0]);
        if (gm > 0.f && gm <= 3.0e38f) {
            int e;
            (void)frexpf(gm, &e);
            int sh = 14 - e;
            sh = sh > 100 ? 100 : (sh < -100 ? -100 : sh);
            gs = ldexpf(1.f, sh);
            ginv = ldexpf(1.f, -sh);
        }
    }
    const int lr = lane & 15, lq = lane >> 4;
    const int ndf = D >> 6, dbase = wave * (D >> 2);
    int cj[RF];                                                                              // the class of this lane's key row per fragment
#pragma unroll
    for (int fr = 0; fr < RF; ++fr) {
        const int j = i0 + 16 * fr + lr;
        cj[fr] = j < NK ? cls[j] : 0;
    }
    float4_t acc2[RF][NDF];
#pragma unroll
    for (int fr = 0; fr < RF; ++fr)
#pragma unroll
        for (int df = 0; df < NDF; ++df) acc2[fr][df] = float4_t{0.f, 0.f, 0.f, 0.f};
    __syncthreads();

    const int KS = D >> 5, ntiles = (Q + 63) >> 6;
    // this wave's query row of the tile at hand, and its first two k-steps
    const half_t* wp = walked_row(f, ldf, 16 * wave + lr, Q, lq);
    half8_t c0 = ld_half8(wp), c1 = ld_half8(wp + 32);
    for (int tile = 0; tile < ntiles; ++tile) {
        const int q0 = tile * 64, buf = tile & 1;
        // ---- aff of queries q0 + 16 wave .. + 15 against the panel ----------------------------------------------------------------------------
        float4_t acc[RF];
        const half_t* wpn = walked_row(f, ldf, q0 + 64 + 16 * wave + lr, Q, lq);
        bwd_first_product<RF>(wp, wpn, c0, c1, panel + (size_t)lr * LDP + lq * 8, LDP, KS, acc);
        wp = wpn;
        half8_t wt0[8];
        bwd_prefetch_t(wt0, fT, ldt, dbase, ndf, q0, lr, lq);                                // in flight under the exponentials and the barrier
        // acc[fr][r] = aff(key i0 + 16 fr + lr, query q0 + 16 wave + 4 lq + r)
        const int qb = q0 + 16 * wave + 4 * lq;
#pragma unroll
        for (int fr = 0; fr < RF; ++fr) {
            const int j = i0 + 16 * fr + lr;
            half4_t g16;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool ok = j < NK && qb + r < Q;
                const float up = ok ? dL[(size_t)(qb + r) * N + cj[fr]] : 0.f;
                const float e = __expf(__builtin_fmaf(beta, acc[fr][r], -beta));
                g16[r] = ok ? (half_t)((up * e) * gs) : (half_t)0.f;
            }
            *reinterpret_cast<half4_t*>(gtile + ((size_t)buf * 16 * RF + 16 * fr + lr) * PW_PLD + 16 * wave + 4 * lq) = g16;
        }
        __syncthreads();                                                                     // the tile is whole; the other buffer is free once every wave is here
        // ---- this wave's quarter of D: acc2 += f^T G, the query index along k ----------------------------------------------------------------
        bwd_second_product<RF, NDF, false>(fT, ldt, dbase, ndf, q0, wt0, gtile, nullptr, false, buf, lr, lq, acc2);
    }
    // acc2[fr][df][r] = 2^s sum_q G[i0 + 16 fr + lr, q] f[q, dbase + 16 df + 4 lq + r]
    store_grad_panel<RF, NDF>(gout, i0, NK, D, dbase, ndf, (alpha * beta) * ginv, lr, lq, acc2);
}

struct TipBwdWs {
    size_t ft, cls, gmax, bytes;
};
inline TipBwdWs tip_bwd_ws(int Q, int NK, int D) {
    TipBwdWs w;
    size_t off = 0;
    w.ft = off, off += align_up((size_t)D * round64(Q) * 2, 256);
    w.cls = off, off += align_up((size_t)NK * 4, 256);
    w.gmax = off, off += 256;
    w.bytes = off;
    return w;
}

inline size_t tip_lds(int D, int RF, int NB) {
    return (size_t)16 * RF * (D + PW_PAD) * 2 + (size_t)(1 + 2 * NB) * 16 * RF * TP_TLD * 4 + (TP_CB + 1 + TP_NBG * TP_NA) * 4;
}

int tip_validate(const char* fn, const void* f, int ldf, int Q, const void* keys, int ldk, int NK, const int32_t* seg, const void* w, int ldw, int N, int D) {
    PCLIP_REQUIRE(f && w && seg, "%s: null operand", fn);
    PCLIP_REQUIRE(Q >= 1, "%s: Q=%d must be positive", fn, Q);
    PCLIP_REQUIRE(N >= 1 && N <= 4096, "%s: N=%d must be in [1, 4096] (the fused argmax's cap)", fn, N);
    PCLIP_REQUIRE(NK >= 0 && (NK == 0 || keys), "%s: NK=%d key rows need a key pointer", fn, NK);
    PCLIP_REQUIRE(D > 0 && D % 64 == 0 && D <= 2048, "%s: D=%d must be a multiple of 64, <= 2048", fn, D);
    PCLIP_REQUIRE_PITCH(fn, ldf, D);
    PCLIP_REQUIRE_PITCH(fn, ldk, D);
    PCLIP_REQUIRE_PITCH(fn, ldw, D);
    PCLIP_REQUIRE_ALIGNED(fn, (uintptr_t)f | (uintptr_t)keys | (uintptr_t)w, (uintptr_t)seg);
    return PCLIP_OK;
}
inline bool tip_coef_ok(float v) { return v >= 0.f && v <= 3.0e38f; }                       // (false for NaN and inf)

}  // namespace

size_t pclip_tip_workspace(int Q, int NK, int D) {
    if (Q < 1 || NK < 0 || D < 1) return 0;
    return tip_bwd_ws(Q, NK, D).bytes;
}

extern "C" int pclip_tip_keys_backward_f16(const void* f, int ldf, int Q, const void* keys, int ldk, int NK, const int32_t* seg, int N, int D, float alpha, float beta,
                                           const float* dL, float* dkeys, void* ws, size_t ws_bytes, pclip_stream_t stream) {
    const char* fn = "pclip_tip_keys_backward_f16";
    PCLIP_REQUIRE(f && seg && dL, "%s: null operand", fn);
    PCLIP_REQUIRE(Q >= 1, "%s: Q=%d must be positive", fn, Q);
    PCLIP_REQUIRE(N >= 1 && N <= 4096, "%s: N=%d must be in [1, 4096]", fn, N);
    PCLIP_REQUIRE(NK >= 0 && (NK == 0 || (keys && dkeys)), "%s: NK=%d key rows need the keys and their gradient", fn, NK);
    PCLIP_REQUIRE(D > 0 && D % 64 == 0 && D <= 2048, "%s: D=%d must be a multiple of 64, <= 2048", fn, D);
    PCLIP_REQUIRE_PITCH(fn, ldf, D);
    PCLIP_REQUIRE_PITCH(fn, ldk, D);
    PCLIP_REQUIRE_ALIGNED(fn, (uintptr_t)f | (uintptr_t)keys | (uintptr_t)dkeys, (uintptr_t)seg | (uintptr_t)dL);
    PCLIP_REQUIRE(tip_coef_ok(alpha) && tip_coef_ok(beta), "%s: alpha=%g and beta=%g must be finite and >= 0", fn, (double)alpha, (double)beta);
    const TipBwdWs w = tip_bwd_ws(Q, NK, D);
    PCLIP_REQUIRE(ws != nullptr && (uintptr_t)ws % 16 == 0, "%s: needs a 16-byte aligned workspace", fn);
    if (ws_bytes < w.bytes) { pclip_set_error("%s: workspace %zu < %zu", fn, ws_bytes, w.bytes); return PCLIP_E_WORKSPACE; }
    if (NK == 0) return PCLIP_OK;
    hipStream_t s = (hipStream_t)stream;
    char* wsb = (char*)ws;
    half_t* fT = (half_t*)(wsb + w.ft);
    int32_t* cls = (int32_t*)(wsb + w.cls);
    unsigned* gmax = (unsigned*)(wsb + w.gmax);
    const int ldt = round64(Q);
    if (hipMemsetAsync(gmax, 0, 4, s) != hipSuccess) { pclip_set_error("%s: cannot clear the workspace", fn); return PCLIP_E_LAUNCH; }
    const size_t ndl = (size_t)Q * N;
    size_t g = ((ndl > (size_t)NK ? ndl : (size_t)NK) + 255) / 256;
    g = g > 2048 ? 2048 : g;
    tip_bwd_prep_kernel<<<(int)g, 256, 0, s>>>(seg, N, NK, cls, dL, ndl, gmax);
    if (int e = pclip_check_launch("tip_keys_backward (classes, max)")) return e;
    if (int e = launch_transpose((const half_t*)f, ldf, Q, D, fT, ldt, s, "tip_keys_backward (transpose)")) return e;
    const int RF = rf_for(NK, D);
    const size_t lds = (size_t)16 * RF * (D + PW_PAD) * 2 + (size_t)2 * 16 * RF * PW_PLD * 2;
    const int npanels = ceil_div(NK, 16 * RF);
    return panel_dispatch(D, RF, [&](auto nch, auto rf, auto ndf) -> int {
        static DevOnce attr;
        if (int e = pclip_raise_lds(attr, {(const void*)tip_bwd_kernel<nch, rf, ndf>}, TP_LDS_MAX, fn)) return e;
        tip_bwd_kernel<nch, rf, ndf><<<npanels, 256, lds, s>>>((const half_t*)keys, ldk, NK, (const half_t*)f, ldf, Q, fT, ldt, D, alpha, beta, cls, dL, N, gmax, dkeys);
        return pclip_check_launch("tip_keys_backward");
    });
}

extern "C" int pclip_tip_logits_f16(const void* f, int ldf, int Q, const void* keys, int ldk, int NK, const int32_t* seg, const void* w, int ldw, int N, int D,
                                    float scale, float alpha, float beta, void* logits, int ldl, float* logits32, int32_t* argmax, pclip_stream_t stream) {
    const char* fn = "pclip_tip_logits_f16";
    if (int e = tip_validate(fn, f, ldf, Q, keys, ldk, NK, seg, w, ldw, N, D)) return e;
    PCLIP_REQUIRE(tip_coef_ok(alpha) && tip_coef_ok(beta), "%s: alpha=%g and beta=%g must be finite and >= 0", fn, (double)alpha, (double)beta);
    PCLIP_REQUIRE(logits || logits32 || argmax, "%s: no output requested", fn);
    PCLIP_REQUIRE(!logits || (ldl >= N && ldl % 8 == 0), "%s: ldl=%d must be >= N=%d and a multiple of 8 halves", fn, ldl, N);
    PCLIP_REQUIRE((uintptr_t)logits % 16 == 0 && (uintptr_t)logits32 % 4 == 0 && (uintptr_t)argmax % 4 == 0, "%s: misaligned output", fn);
    hipStream_t s = (hipStream_t)stream;
    // rows per panel: as large as D allows, smaller where that leaves the device short of workgroups (a row's bits do not depend on it)
    int RF = D <= 512 ? 4 : (D <= 1024 ? 2 : 1);
    while (RF > 1 && ceil_div(Q, 16 * RF) < 512) RF >>= 1;
    const size_t lds = tip_lds(D, RF, 1);
    const int npanels = ceil_div(Q, 16 * RF), nblocks = ceil_div(N, TP_CB);
    int ysplit = 1;                                       // without the argmax few panels share the class blocks between workgroups
    if (!argmax) {
        ysplit = ceil_div(512, npanels);
        ysplit = ysplit > nblocks ? nblocks : ysplit;
    }
    const dim3 grid(npanels, ysplit);
    return panel_dispatch(D, RF, [&](auto nch, auto rf, auto) -> int {
        static DevOnce attr;
        if (int e = pclip_raise_lds(attr, {(const void*)tip_kernel<nch, rf, 1, false>}, TP_LDS_MAX, fn)) return e;
        tip_kernel<nch, rf, 1, false><<<grid, 256, lds, s>>>((const half_t*)f, ldf, Q, (const half_t*)keys, ldk, NK, seg, (const half_t*)w, ldw, N, D, scale, alpha, beta,
                                                            nullptr, 0, nullptr, 0, nullptr, (half_t*)logits, ldl, logits32, argmax, nullptr);
        return pclip_check_launch("tip_logits");
    });
}

extern "C" int pclip_tip_grid_f16(const void* f, int ldf, int Q, const void* keys, int ldk, int NK, const int32_t* seg, const void* w, int ldw, int N, int D,
                                  float scale, const float* betas, int nb, const float* alphas, int na, const int32_t* labels, int32_t* correct,
                                  pclip_stream_t stream) {
    const char* fn = "pclip_tip_grid_f16";
    if (int e = tip_validate(fn, f, ldf, Q, keys, ldk, NK, seg, w, ldw, N, D)) return e;
    PCLIP_REQUIRE(betas && alphas && labels && correct, "%s: null operand", fn);
    PCLIP_REQUIRE(nb >= 1 && nb <= 65535 * TP_NBG, "%s: nb=%d must be in [1, %d]", fn, nb, 65535 * TP_NBG);
    PCLIP_REQUIRE(na >= 1 && na <= TP_NA, "%s: na=%d must be in [1, %d]", fn, na, TP_NA);
    PCLIP_REQUIRE(((uintptr_t)betas | (uintptr_t)alphas | (uintptr_t)labels | (uintptr_t)correct) % 4 == 0, "%s: misaligned operand", fn);
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(correct, 0, (size_t)nb * na * sizeof(int32_t), s) != hipSuccess) {
        pclip_set_error("%s: cannot clear the counts", fn);
        return PCLIP_E_LAUNCH;
    }
    int RF = D <= 1024 ? 2 : 1;
    while (RF > 1 && ceil_div(Q, 16 * RF) * ceil_div(nb, TP_NBG) < 512) RF >>= 1;
    const size_t lds = tip_lds(D, RF, TP_NBG);
    const dim3 grid(ceil_div(Q, 16 * RF), ceil_div(nb, TP_NBG));
    return panel_dispatch<2>(D, RF, [&](auto nch, auto rf, auto) -> int {            // (RF <= 2 above: the grid kernel is compiled for no wider panel)
        static DevOnce attr;
        if (int e = pclip_raise_lds(attr, {(const void*)tip_kernel<nch, rf, TP_NBG, true>}, TP_LDS_MAX, fn)) return e;
        tip_kernel<nch, rf, TP_NBG, true><<<grid, 256, lds, s>>>((const half_t*)f, ldf, Q, (const half_t*)keys, ldk, NK, seg, (const half_t*)w, ldw, N, D, scale, 0.f, 0.f,
                                                                betas, nb, alphas, na, labels, nullptr, 0, nullptr, nullptr, correct);
        return pclip_check_launch("tip_grid");
    });
}
