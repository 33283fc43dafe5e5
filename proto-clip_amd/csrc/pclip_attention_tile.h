// Per-query-tile attention arithmetic shared by the resident-K/V kernels (pclip_attention.hip) and the streamed-K/V kernel of long
// sequences (pclip_attention_long.hip): one instruction sequence per pair of key tiles, hence the same bits from every kernel that walks
// the same key tiles in the same order.  Everything lives in an anonymous namespace: each translation unit gets its own copy.
#pragma once
#include "pclip_encoder_common.h"
#include <type_traits>

namespace {
// ---- attention: 32-query tiles against 32-key tiles, online softmax in registers ----------------------------------------------
// The CLIP sequences (50 .. 257 tokens) fit one workgroup with K / V resident in LDS (pclip_attention.hip); longer ones stream K / V
// through LDS 128 keys at a time (pclip_attention_long.hip).  Both contractions are computed TRANSPOSED so
// that a lane owns ONE query row throughout:
//   S^T = K Q^T      (A = K rows from LDS, B = Q rows in registers)  -> lane (q = lane&31) holds 16 keys
//   O^T = V^T P^T    (A = V^T rows from LDS, B = P^T = the S^T registers, already in B-operand order)
// so the softmax max / sum / rescale are in-lane scalars (one cross-half shuffle), no LDS round trip for P,
// and the k-order of the second contraction is whatever the first one produced (a contraction does not
// care, as long as A and B agree).  Keys are walked in 32-wide tiles with an online softmax, which keeps
// the register footprint at ~100 VGPRs (2 workgroups per CU) for any L <= 288.
constexpr int ATT_DH = 64;
// Softmax variants of attn_query_tile (bit mask VAR; same-process A/B of the seven combinations, tools/ab_multi.py attn,
// profiles/r03_ab_attention_var.txt — ViT-B/16, B = 1024: 336 us -> 306 us with all four, each contributing):
//   1  deferred maximum: a row's running maximum only moves when the row outgrew it by more than 2^kAttDefer; in between the
//      probabilities are taken against the OLD maximum (they reach 2^kAttDefer instead of 1: exact in fp32, and the fp16 rounding of
//      P is relative) and the rescale of the 32 output accumulators (+ its v_exp) is skipped.  On N(0,1) data the maximum of a later
//      key tile practically never exceeds the first tiles' by a factor 4, so the rescale runs once per query tile instead of 4 times.
//   2  the row sum as two interleaved partial sums (v_pk_add_f32: 16 instead of 32 dependent adds per pair of key tiles)
//   4  scale-and-shift of two scores per instruction (v_pk_fma_f32)
//   8  s_setprio(1) around the MFMA clusters (four waves per SIMD at different phases: the guide's T5 regime)
// The eight-wave kernel (long sequences: ViT-B/16, ViT-L/14) takes all four; the four-wave kernel (ViT-B/32, the text tower) only the
// deferred maximum — the packed forms and the priority flips cost the causal L = 77 kernel 4 %.  Not bit-identical to round 2's
// kernel: outputs differ by one fp16 ulp on ~1e-4 of the elements, error against fp32 attention unchanged (tests/test_gpu_encoder.py).
constexpr float kAttDefer = 2.f;
#ifndef PCLIP_ATT_VAR_LONG
#define PCLIP_ATT_VAR_LONG 15
#endif
#ifndef PCLIP_ATT_VAR_SHORT
#define PCLIP_ATT_VAR_SHORT 1
#endif

// ds_read_b64_tr_b16: 64 bits per lane, 16-bit elements transposed inside each 16-lane group (see attention_kernel)
typedef __fp16 fp16x4_t __attribute__((__vector_size__(4 * sizeof(__fp16))));
__device__ __forceinline__ half4_t tr_read4(const char* lds_addr) {
    const fp16x4_t v = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16x4_t*)(lds_addr));
    return __builtin_bit_cast(half4_t, v);
}

// Transpose-read addressing (probed on gfx950, tools/probe/tr_probe.hip): inside a 16-lane group, lane i supplies the address
// of 4 consecutive halfs and lane l receives element (l & 3) of the words addressed by lanes 4*jj + ((l & 15) >> 2), jj = 0..3.
// With lane i pointing at V[key0 + (i >> 2)][d0 + 4*(i & 3) ..], lane l therefore receives V[key0 + jj][d0 + (l & 15)]: four
// consecutive keys of ITS output dimension — the A-operand fragment of O^T = V^T P^T, without a transposed copy of V.
// voff[j]: byte offset of this lane's word for the output halves j = 0, 1.
__device__ __forceinline__ void attn_voff(int lane, int (&voff)[2]) {
    const int hi = lane >> 5;
    const int i16 = lane & 15, vrow = hi * 4 + (i16 >> 2), vd = ((lane >> 4) & 1) * 16 + 4 * (i16 & 3), vswz = ((vrow >> 1) & 1) << 2;
#pragma unroll
    for (int j = 0; j < 2; ++j) voff[j] = vrow * (ATT_DH * 2) + ((((j * 4 + (vd >> 3)) ^ vswz)) << 4) + (vd & 7) * 2;
}

// One 32-query tile (query row q = qb*32 + (lane & 31), fragments qf) against every key tile of the sequence resident in LDS:
// Ks [>= L rows][64] with the 16-byte chunks XOR-swizzled by swz_key(row) — rows >= L may hold ANYTHING, their scores are
// overwritten by the mask; Vs [NT*32 rows][64] with chunk ^ 4*((row >> 1) & 1) — rows >= L must be finite (their probabilities
// are exact zeros).  Returns O^T (unnormalised) and the row sum.  Shared by attention_kernel, attention_pipe_kernel and (through
// attn_key_tiles) attention_long_kernel: one instruction order, bit-identical results.
// max / sum of a value with its partner lane (lane ^ 32) through v_permlane32_swap (a VALU instruction) instead of the LDS round
// trip of a ds_bpermute: swap(v, v) leaves {own, partner} in the lower half-wave and {partner, own} in the upper one, and both
// operations are commutative, so every lane gets exactly the value of `x op shfl_xor(x, 32)`.
// (The two results are copied into scalars before the bit casts: __builtin_bit_cast(float, r[1]) applied to the builtin's result
// directly reads element 0 under this hipcc — the max / add of the pair silently became max(r0, r0).)
__device__ __forceinline__ void half_wave_pair(float v, float& r0, float& r1) {
#if defined(__HIP_DEVICE_COMPILE__)
    const unsigned a = __builtin_bit_cast(unsigned, v);
    const auto r = __builtin_amdgcn_permlane32_swap(a, a, false, false);
    const unsigned x = r[0], y = r[1];
    r0 = __builtin_bit_cast(float, x);
    r1 = __builtin_bit_cast(float, y);
#else
    r0 = r1 = v;
#endif
}
__device__ __forceinline__ float half_wave_max(float v) { float a, b; half_wave_pair(v, a, b); return fmaxf(a, b); }
__device__ __forceinline__ float half_wave_sum(float v) { float a, b; half_wave_pair(v, a, b); return a + b; }

// DEEP (the persistent kernel: two waves per SIMD, registers to spare): the K fragments of the NEXT pair of key tiles and the
// V^T fragments of THIS pair are requested right after the pair's score MFMAs, so their LDS latency passes under the softmax
// arithmetic instead of in front of every MFMA (+64 VGPRs).  Same operations in the same order per accumulator: same bits.
// VBAR: the caller has only made K visible so far (V is still landing); the first pair of key tiles waits for V — own pieces, then a workgroup barrier —
// between its softmax and its second contraction, so V's arrival passes under the first scores.  Every wave of the workgroup must pass that barrier once.
#ifndef PCLIP_ATT_QF4
#define PCLIP_ATT_QF4 1           // query-first form of the four-wave kernel for short non-causal sequences (0: A/B)
#endif
#ifndef PCLIP_ATT_EDGE
#define PCLIP_ATT_EDGE 1          // a lone last key tile with at most 24 valid keys skips its fully masked groups (tile_edge below; 0: A/B)
#endif
// The key tiles 0 .. NT-1 of Ks / Vs for one query tile, continuing the online-softmax state (o, mrun, lrun; attn_query_tile starts it
// at 0, -inf, 0).  Key tiles are taken in pairs, a lone tile only at the end.  A non-causal walk over a WINDOW of the sequence — Ks / Vs
// pointing at key row k0 (a multiple of 64), L and NT counted from k0 — runs, tile for tile, the instructions the whole walk runs on
// those keys (the masks only compare against L - 32 t): the streamed kernel (pclip_attention_long.hip) walks one LDS stage at a time
// and gets the bits of the resident kernels.
//
// ROUNDING POINTS (tests/attention_fwd_ref.py derives the per-element tolerance of the forward attention from exactly these; u11 = 2^-11 an fp16
// rounding, u24 = 2^-24 an fp32 rounding, 2^-25 the absolute error of an fp16 rounding in the subnormal range; S = q k^T / 8, P = softmax(S)):
//   1. S^T = K Q^T: fp16 operands, 64 exact products accumulated in fp32 by four MFMAs                       64 u24 |q| |k|^T / 8
//   2. kScale = log2(e) / 8 is a rounded fp32 constant; s kScale - mnew is ONE fma (VAR & 4: v_pk_fma_f32)      2 u24 |S|, and u24 of the result
//   3. p = v_exp_f32(.) against the RUNNING maximum mnew, which under VAR & 1 is up to kAttDefer stale: p reaches 2^kAttDefer, exact in fp32
//   4. the row sum: a lane's 16 / 32 probabilities of the pair one after the other (VAR & 2: two interleaved chains), the half-waves added, lrun += psum;
//      with 5. and 7. inside (L + 16) u24 relative
//   5. a rescale: alpha = v_exp_f32(mrun - mnew) — the exponents are fp32 differences that telescope over a row (the maximum only rises) — times lrun
//      and times every o: the SAME alpha on both sides of the final quotient
//   6. p -> fp16 as the B operand of O^T = V^T P^T: relative u11, absolute 2^-25 in the subnormal range — at the unnormalised scale, where it stays:
//      the pair that last set the maximum added exp2(0) = 1 to lrun and every later alpha is <= 1, so lrun >= 1 at the end.  Masked keys: exp2(-inf) = 0.
//      O^T accumulates in fp32 over the L keys                                                                  L u24 P |V|
//   7. attn_store_tile: inv = 1.f / lrun, o * inv in fp32, then the ONE fp16 rounding of the output             u11 |O| + 2^-25
// Which maximum a probability was taken against and when the state was rescaled is exact algebra on the softmax: it adds no term.
template <bool DEEP = false, int VAR = 0, bool VBAR = false>
__device__ __forceinline__ void attn_key_tiles(const half_t* Ks, const half_t* Vs, const half8_t (&qf)[4], int q, int qb, int L, int causal,
                                               int NT, int hi, int ql, const int (&voff)[2], float16_t (&o)[2],
                                               float& mrun_io, float& lrun_io) {
    // scores are kept in the log2 domain: s2 = (q.k) * (1/sqrt(64)) * log2(e), p = exp2(s2 - max2) — one
    // v_exp_f32 per probability; masks are applied only on the tiles that need them (last key tile, causal
    // diagonal); the running output is rescaled only when some row's maximum actually moved.
    constexpr float kScale = 0.125f * 1.4426950408889634f;
    float mrun = mrun_io, lrun = lrun_io;
    const int tend = causal ? (qb + 1 < NT ? qb + 1 : NT) : NT;      // causal: keys beyond the block's last query are all masked
    // Key tiles are taken two at a time: the two score accumulators are independent MFMA chains (a single
    // 32x32x16 chain is issue-limited by its own accumulator dependency), and one max / rescale serves 64 keys.
    auto k_frag = [&](int t, int sidx) {
        const int kr = t * 32 + ql;                                // key row this lane feeds as the A operand
        return *reinterpret_cast<const half8_t*>(Ks + kr * ATT_DH + (((sidx * 2 + hi) ^ pgemm::swz_key(kr)) << 3));
    };
    auto v_frag = [&](int t, int sidx, int j) {
        // V^T fragment: row d = j*32 + ql, keys t*32 + 16s + 4hi + {0..3} and the same + 8: two transpose-reads
        const char* vb = reinterpret_cast<const char*>(Vs) + (t * 32 + sidx * 16) * (ATT_DH * 2) + voff[j];
        const half4_t v0 = tr_read4(vb);
        const half4_t v1 = tr_read4(vb + 8 * (ATT_DH * 2));
        return half8_t{v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
    };
    half8_t kpre[2][4];                                            // DEEP: K fragments of the pair about to be multiplied
    auto k_prefetch = [&](int t0) {                                // always two tiles (the second clamped: one shape of code, no select between register sets)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int tt = t0 + u < NT ? t0 + u : NT - 1;
#pragma unroll
            for (int sidx = 0; sidx < 4; ++sidx) kpre[u][sidx] = k_frag(tt, sidx);
        }
    };
    auto tiles = [&](auto NTILE_C, int t0) {
        constexpr int NTILE = decltype(NTILE_C)::value;
        float16_t st[NTILE];
#pragma unroll
        for (int u = 0; u < NTILE; ++u)
#pragma unroll
            for (int e = 0; e < 16; ++e) st[u][e] = 0.f;
#if defined(__HIP_DEVICE_COMPILE__)
        if (VAR & 8) __builtin_amdgcn_s_setprio(1);
#endif
#pragma unroll
        for (int sidx = 0; sidx < 4; ++sidx)
#pragma unroll
            for (int u = 0; u < NTILE; ++u) {
                const half8_t kf = DEEP ? kpre[u][sidx] : k_frag(t0 + u, sidx);
                st[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[sidx], st[u], 0, 0, 0);
            }
#if defined(__HIP_DEVICE_COMPILE__)
        if (VAR & 8) __builtin_amdgcn_s_setprio(0);
#endif
        half8_t vpre[NTILE][2][2];
        if (DEEP) {
#pragma unroll
            for (int u = 0; u < NTILE; ++u)
#pragma unroll
                for (int sidx = 0; sidx < 2; ++sidx)
#pragma unroll
                    for (int j = 0; j < 2; ++j) vpre[u][sidx][j] = v_frag(t0 + u, sidx, j);
            const int tn = t0 + NTILE;
            if (tn < tend) k_prefetch(tn);
#if defined(__HIP_DEVICE_COMPILE__)
            __builtin_amdgcn_sched_barrier(0);                     // keep the requests ahead of the softmax arithmetic
#endif
        }
        float tmax = -__builtin_inff();
#pragma unroll
        for (int u = 0; u < NTILE; ++u) {
            const int t = t0 + u;
            if ((t * 32 + 32 > L) || (causal && t == qb)) {        // wave-uniform: only edge tiles pay for the mask
                // key k = t*32 + c_e + 4*hi is valid iff k < L and (causal) k <= q, i.e. k < min(L, q + 1): ONE per-lane limit
                // against the compile-time c_e — a compare + select per element (the two-condition form was 12 instructions each)
                const int kend = causal ? (q + 1 < L ? q + 1 : L) : L;
                const int lim = kend - t * 32 - 4 * hi;
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    if (!((e & 3) + 8 * (e >> 2) < lim)) st[u][e] = -__builtin_inff();
            }
        }
        {   // four independent maximum chains instead of one 32-deep dependent one (max is exact: same value)
            float m4[4] = {tmax, tmax, tmax, tmax};
#pragma unroll
            for (int u = 0; u < NTILE; ++u)
#pragma unroll
                for (int e = 0; e < 16; ++e) m4[e & 3] = fmaxf(m4[e & 3], st[u][e]);
            tmax = fmaxf(fmaxf(m4[0], m4[1]), fmaxf(m4[2], m4[3]));
        }
        tmax = half_wave_max(tmax) * kScale;                       // kScale > 0: max commutes with the scaling
        // VAR & 1: deferred maximum (see above), decided PER ROW — a row's bits must not depend on the rows that share its wave (the
        // one-query form of the last block == the full attention); -inf + kAttDefer = -inf, so the first tile always sets the maximum.
        // The rescale below is skipped when no row of the wave moved (rows that did not move multiply by exp2(0) = 1 exactly).
        const bool moved = (VAR & 1) ? tmax > mrun + kAttDefer : fmaxf(mrun, tmax) != mrun;
        const float mnew = ((VAR & 1) && !moved) ? mrun : fmaxf(mrun, tmax);    // finite from the first tile on: key 0 is never masked
        const bool grow = __any(moved);
        float psum = 0.f;
        if (VAR & 6) {
            float2_t ps2 = {0.f, 0.f};
            const float2_t ks2 = {kScale, kScale}, nm2 = {-mnew, -mnew};
#pragma unroll
            for (int u = 0; u < NTILE; ++u)
#pragma unroll
                for (int e = 0; e < 16; e += 2) {
                    float2_t v = {st[u][e], st[u][e + 1]};
                    if (VAR & 4) {
                        v = v * ks2 + nm2;                         // v_pk_fma_f32
                        v = float2_t{__builtin_amdgcn_exp2f(v[0]), __builtin_amdgcn_exp2f(v[1])};
                    } else
                        v = float2_t{__builtin_amdgcn_exp2f(fmaf(v[0], kScale, -mnew)), __builtin_amdgcn_exp2f(fmaf(v[1], kScale, -mnew))};
                    st[u][e] = v[0];
                    st[u][e + 1] = v[1];
                    if (VAR & 2) ps2 += v;                         // v_pk_add_f32: two partial sums
                    else { psum += v[0]; psum += v[1]; }
                }
            psum += ps2[0] + ps2[1];
        } else {
#pragma unroll
            for (int u = 0; u < NTILE; ++u)
#pragma unroll
                for (int e = 0; e < 16; ++e) { st[u][e] = __builtin_amdgcn_exp2f(fmaf(st[u][e], kScale, -mnew)); psum += st[u][e]; }
        }
        psum = half_wave_sum(psum);
        if (grow) {
            const float alpha = __builtin_amdgcn_exp2f(mrun - mnew);
            lrun *= alpha;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) o[j][e] *= alpha;
        }
        lrun += psum;
        mrun = mnew;
        if (VBAR && t0 == 0) { pgemm::wait_vm<0>(); pgemm::lds_barrier(); }
#pragma unroll
        for (int u = 0; u < NTILE; ++u)
#pragma unroll
            for (int sidx = 0; sidx < 2; ++sidx) {
                half8_t pf;
#pragma unroll
                for (int e = 0; e < 8; ++e) pf[e] = (half_t)st[u][sidx * 8 + e];
#if defined(__HIP_DEVICE_COMPILE__)
                if (VAR & 8) __builtin_amdgcn_s_setprio(1);
#endif
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const half8_t vf = DEEP ? vpre[u][sidx][j] : v_frag(t0 + u, sidx, j);
                    o[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf, o[j], 0, 0, 0);
                }
#if defined(__HIP_DEVICE_COMPILE__)
                if (VAR & 8) __builtin_amdgcn_s_setprio(0);
#endif
            }
    };
    // A LAST key tile on its own whose keys beyond L are masked (non-causal; ViT-B/16: keys 192 .. 196 of tile 6, ViT-L/14: key 256 alone in tile 8): the groups of
    // eight keys (elements 4g .. 4g + 3 of both half-waves) without a single valid key are not computed at all — no mask, maximum, exponential, sum or conversion
    // for them, and no second contraction over keys 16 .. 31 when those are all masked.  Their probabilities are exact zeros in `tiles` (exp2(-inf)), which add
    // nothing to the sum and to O: same bits (the valid elements keep their order in the maximum chains and the partial sums).
    auto tile_edge = [&](int t0) {
        const int ng = (L - t0 * 32 + 7) >> 3;                          // groups with a valid key: 1 .. 3 (wave-uniform)
        float16_t st;
#pragma unroll
        for (int e = 0; e < 16; ++e) st[e] = 0.f;
#if defined(__HIP_DEVICE_COMPILE__)
        if (VAR & 8) __builtin_amdgcn_s_setprio(1);
#endif
#pragma unroll
        for (int sidx = 0; sidx < 4; ++sidx) st = __builtin_amdgcn_mfma_f32_32x32x16_f16(k_frag(t0, sidx), qf[sidx], st, 0, 0, 0);
#if defined(__HIP_DEVICE_COMPILE__)
        if (VAR & 8) __builtin_amdgcn_s_setprio(0);
#endif
        const int lim = L - t0 * 32 - 4 * hi;
        float m4[4] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
#pragma unroll
        for (int g = 0; g < 3; ++g)
            if (g < ng) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (!(r + 8 * g < lim)) st[4 * g + r] = -__builtin_inff();
                    m4[r] = fmaxf(m4[r], st[4 * g + r]);
                }
            }
        float tmax = fmaxf(fmaxf(m4[0], m4[1]), fmaxf(m4[2], m4[3]));
        tmax = half_wave_max(tmax) * kScale;
        const bool moved = (VAR & 1) ? tmax > mrun + kAttDefer : fmaxf(mrun, tmax) != mrun;
        const float mnew = ((VAR & 1) && !moved) ? mrun : fmaxf(mrun, tmax);
        const bool grow = __any(moved);
        float psum = 0.f;
        float2_t ps2 = {0.f, 0.f};
        const float2_t ks2 = {kScale, kScale}, nm2 = {-mnew, -mnew};
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            if (g < 3 && g < ng) {
#pragma unroll
                for (int e = 4 * g; e < 4 * g + 4; e += 2) {
                    float2_t v = {st[e], st[e + 1]};
                    if (VAR & 6) {
                        if (VAR & 4) {
                            v = v * ks2 + nm2;
                            v = float2_t{__builtin_amdgcn_exp2f(v[0]), __builtin_amdgcn_exp2f(v[1])};
                        } else
                            v = float2_t{__builtin_amdgcn_exp2f(fmaf(v[0], kScale, -mnew)), __builtin_amdgcn_exp2f(fmaf(v[1], kScale, -mnew))};
                        if (VAR & 2) ps2 += v;
                        else { psum += v[0]; psum += v[1]; }
                    } else {
                        v[0] = __builtin_amdgcn_exp2f(fmaf(v[0], kScale, -mnew)); psum += v[0];
                        v[1] = __builtin_amdgcn_exp2f(fmaf(v[1], kScale, -mnew)); psum += v[1];
                    }
                    st[e] = v[0];
                    st[e + 1] = v[1];
                }
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) st[4 * g + r] = 0.f;
            }
        }
        if (VAR & 6) psum += ps2[0] + ps2[1];
        psum = half_wave_sum(psum);
        if (grow) {
            const float alpha = __builtin_amdgcn_exp2f(mrun - mnew);
            lrun *= alpha;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) o[j][e] *= alpha;
        }
        lrun += psum;
        mrun = mnew;
        if (VBAR && t0 == 0) { pgemm::wait_vm<0>(); pgemm::lds_barrier(); }
#pragma unroll
        for (int sidx = 0; sidx < 2; ++sidx)
            if (sidx == 0 || ng > 2) {
                half8_t pf;
#pragma unroll
                for (int e = 0; e < 8; ++e) pf[e] = (half_t)st[sidx * 8 + e];
#if defined(__HIP_DEVICE_COMPILE__)
                if (VAR & 8) __builtin_amdgcn_s_setprio(1);
#endif
#pragma unroll
                for (int j = 0; j < 2; ++j) o[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(v_frag(t0, sidx, j), pf, o[j], 0, 0, 0);
#if defined(__HIP_DEVICE_COMPILE__)
                if (VAR & 8) __builtin_amdgcn_s_setprio(0);
#endif
            }
    };
    int t = 0;
    if (DEEP) k_prefetch(0);
    for (; t + 1 < tend; t += 2) tiles(std::integral_constant<int, 2>{}, t);
    if (t < tend) {
        if (PCLIP_ATT_EDGE && VBAR && !DEEP && !causal && L - t * 32 <= 24) tile_edge(t);      // (the query-first kernels only: measured neutral to - 2 % in the looping eight-wave kernel at L = 257)
        else tiles(std::integral_constant<int, 1>{}, t);
    }
    mrun_io = mrun;
    lrun_io = lrun;
}

// One 32-query tile against every key tile of the sequence resident in LDS (see attn_key_tiles).
template <bool DEEP = false, int VAR = 0, bool VBAR = false>
__device__ __forceinline__ void attn_query_tile(const half_t* Ks, const half_t* Vs, const half8_t (&qf)[4], int q, int qb, int L, int causal,
                                                int NT, int hi, int ql, const int (&voff)[2], float16_t (&o)[2], float& lrun_out) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[j][e] = 0.f;
    float mrun = -__builtin_inff(), lrun = 0.f;
    attn_key_tiles<DEEP, VAR, VBAR>(Ks, Vs, qf, q, qb, L, causal, NT, hi, ql, voff, o, mrun, lrun);
    lrun_out = lrun;
}

// O^T tile -> the query's 128-byte output row segment: lane (ql, hi) holds d = j*32 + 8g + 4hi + (e & 3), i.e. each output row is
// split across the two half-waves in 8-byte pieces.  v_permlane32_swap pairs the pieces of column groups (2k, 2k+1) so that every
// lane owns 16 contiguous bytes: four dwordx4 stores per lane instead of sixteen dwordx2 (the store tail is issue-bound; guide T21).
// `orow` = this lane's output row (+ head offset); every lane executes the swaps, `valid` only predicates the stores.
__device__ __forceinline__ void attn_store_tile(half_t* orow, const float16_t (&o)[2], float lrun, int hi, bool valid) {
    const float inv = 1.f / lrun;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            unsigned a[2], bq[2];
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                const half2_t ha = {(half_t)(o[j][8 * k + 2 * w] * inv), (half_t)(o[j][8 * k + 2 * w + 1] * inv)};          // group g = 2k
                const half2_t hb = {(half_t)(o[j][8 * k + 4 + 2 * w] * inv), (half_t)(o[j][8 * k + 4 + 2 * w + 1] * inv)};  // group g = 2k + 1
                a[w] = __builtin_bit_cast(unsigned, ha);
                bq[w] = __builtin_bit_cast(unsigned, hb);
            }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                const auto r = __builtin_amdgcn_permlane32_swap(a[w], bq[w], false, false);   // upper half of a <-> lower half of b
                a[w] = r[0];
                bq[w] = r[1];
            }
#endif
            // lanes 0-31: [own g=2k | partner's g=2k] = d 16k .. 16k+7; lanes 32-63: [partner's g=2k+1 | own g=2k+1] = d 16k+8 .. 16k+15
            if (valid) *reinterpret_cast<uint4_t*>(orow + j * 32 + 16 * k + 8 * hi) = uint4_t{a[0], a[1], bq[0], bq[1]};
        }
}

// LDS-DMA of one 16-byte piece per lane by inline asm (buffer_load_dwordx4 ... lds; see attention_pipe_kernel for why not the builtin)
__device__ __forceinline__ void attn_dma16(uint4_t rs, int voff, int soff, unsigned lds_addr) {
#if defined(__HIP_DEVICE_COMPILE__)
    unsigned keep;
    asm volatile(
        "s_nop 4\n\t"
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %3\n\t"
        "s_nop 0\n\t"
        "buffer_load_dwordx4 %1, %2, %4 offen lds\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(voff), "s"(rs), "s"(lds_addr), "s"(soff)
        : "memory");
#endif
}
__device__ __forceinline__ uint4_t attn_rsrc(const void* base) {
    const uint64_t addr = (uint64_t)base;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)addr), hi = __builtin_amdgcn_readfirstlane((uint32_t)(addr >> 32));
    return uint4_t{lo, hi & 0xffffu, 0x7fffffffu, 0x00020000u};   // stride 0, num_records 2 GiB, raw 32-bit data format
}

}  // namespace
