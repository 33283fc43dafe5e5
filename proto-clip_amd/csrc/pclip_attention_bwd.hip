// Attention backward of the CLIP towers (the gradient of clip/model.py:183-185, nn.MultiheadAttention with need_weights=False) for the forward's
// resident envelope: dh == 64, 1 <= L <= 288, one workgroup per (sequence, head).
//
//   S = q k^T / 8 (+ causal mask)   P = softmax(S)   O = P v
//   dV = P^T dO      dP = dO V^T      dS = P o (dP - rowsum(dO o O))      dQ = dS K / 8      dK = dS^T Q / 8
//
// Nothing is saved by the forward: S and P are recomputed from qkv.  Q, K, V and dO of the (sequence, head) are staged ONCE into LDS by LDS-DMA
// (4 x LP x 128 B, LP = 32 ceil(L / 32): 147 KB at L = 288) in ONE image per operand — row-major, the 16-byte chunks XOR-swizzled by swz_key(row) —
// that serves the row reads (ds_read_b128: the A operand of S^T and dP^T) and the transposed reads (ds_read_b64_tr_b16: the A operand of the three
// gradient products).  There is no sum across waves or workgroups, hence no atomics and no reduction order that could vary: the kernel walks the
// score matrix twice, once with the QUERY on the MFMA lane and once with the KEY on the lane.
//   pass Q (a wave owns a 32-query tile, walks the key tiles; the own rows' Q / dO fragments are the B operands):
//     sweep 1  S^T = K Q^T and dP^T = V dO^T per key tile; online softmax statistics m (running maximum, log2 domain), l = sum exp2(s - m) and
//              u = sum exp2(s - m) dP, rescaled together when the maximum moves.  delta = u / l.
//     sweep 2  the same two products again, P = exp2(s - m) / l, dS = P (dP - delta); dS rounded to fp16 is the B operand of dQ^T += K^T dS^T.
//     m, 1 / l and delta of every query row go to LDS for pass K.
//   pass K (a wave owns a 32-key tile, walks the query tiles; K / V fragments are the B operands):
//     S = Q K^T and dP = dO V^T per query tile with the row statistics read back from LDS, P and dS as above (bit-identical to sweep 2's: the same
//     fp32 operations on the same MFMA sums), dV^T += dO^T P and dK^T += Q^T dS with P / dS rounded to fp16 as the B operands.
// Nine 32 x 32 x 64 products per pair of tiles where a cross-wave hand-off of dS would need five: the price of the fixed summation order.
//
// ROUNDING POINTS (tests/attention_bwd_ref.py derives the tolerances from exactly these):
//   * q, k, v, dO are fp16; every product runs on v_mfma_f32_32x32x16_f16 with fp32 accumulation.
//   * the scores are scaled in fp32 (s2 = S * 0.125 * log2 e), exponentials are v_exp_f32 (fp32), m, l, 1 / l are fp32.
//   * dP is fp32.  The rowsum term rowsum(dO o O) is formed as delta = sum_k P dP — the same double sum with d contracted first — from the fp32 P and
//     fp32 dP, accumulated in fp32: no fp16 rounding of O enters it.
//   * dS = P (dP - delta) in fp32 from the fp32 P.
//   * P (for dV) and dS (for dQ, dK) are rounded to fp16 ONCE, as they enter their matrix products.
//   * dQ, dK, dV accumulate in fp32; dQ and dK are multiplied by 1/8 (exact) and every output is rounded to fp16 once.
// Rows >= L of the LDS images repeat row L - 1 (finite): every P / dS that involves them is selected to an exact zero, and their outputs are not stored.
#include "pclip_attention_tile.h"

namespace {
constexpr int ABW_MAX_L = 288;
constexpr int ABW_ROW = ATT_DH * 2;                                  // bytes per LDS row
constexpr float kAbwScale = 0.125f * 1.4426950408889634f;

// 16-byte chunk kc (0 .. 7) of a row: the MFMA A / B fragment "row r, k = 8 kc .. 8 kc + 7"
__device__ __forceinline__ half8_t abw_row_frag(const char* M, int row, int kc) {
    return *reinterpret_cast<const half8_t*>(M + row * ABW_ROW + ((kc ^ pgemm::swz_key(row)) << 4));
}

// Transposed-read offsets (see attn_voff; here the image carries swz_key).  For the block of 16 rows at row0 (a multiple of 16) the lane addresses
// row0 + 4 hi + (i16 >> 2) and that row + 8, columns j * 32 + 16 * ((lane >> 4) & 1) + 4 * (i16 & 3) ..+3, and receives column j * 32 + (lane & 31)
// of rows row0 + 4 hi + {0 .. 3} and + 8: the A fragment whose k order matches an accumulator tile used as the B operand.
__device__ __forceinline__ void abw_toff(int lane, int (&toff)[2][2]) {
    const int hi = lane >> 5, i16 = lane & 15, b4 = (lane >> 4) & 1;
    const int r0 = hi * 4 + (i16 >> 2);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int chunk = j * 4 + b4 * 2 + ((i16 & 3) >> 1);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int r = r0 + 8 * u;
            toff[j][u] = r * ABW_ROW + ((chunk ^ pgemm::swz_key(r)) << 4) + 8 * (i16 & 1);
        }
    }
}
__device__ __forceinline__ half8_t abw_tr_frag(const char* M, int row0, const int (&toff)[2][2], int j) {
    const half4_t v0 = tr_read4(M + row0 * ABW_ROW + toff[j][0]);
    const half4_t v1 = tr_read4(M + row0 * ABW_ROW + toff[j][1]);
    return half8_t{v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
}

// [partner row t * 32 + c_e + 4 hi][own row ql] = sum_d M[partner][d] * own[d]
__device__ __forceinline__ float16_t abw_product(const char* M, int t, int ql, int hi, const half8_t (&own)[4]) {
    float16_t c;
#pragma unroll
    for (int e = 0; e < 16; ++e) c[e] = 0.f;
    const int row = t * 32 + ql;
#pragma unroll
    for (int s = 0; s < 4; ++s) c = __builtin_amdgcn_mfma_f32_32x32x16_f16(abw_row_frag(M, row, s * 2 + hi), own[s], c, 0, 0, 0);
    return c;
}

__device__ __forceinline__ half8_t abw_pack(const float16_t& x, int sidx) {
    half8_t r;
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = (half_t)x[sidx * 8 + e];
    return r;
}

template <int NW>
__global__ __launch_bounds__(NW * 64) void attention_bwd_kernel(const half_t* __restrict__ qkv, const half_t* __restrict__ dout,
                                                                 half_t* __restrict__ dqkv, int L, int H, int causal, int NT) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int LP = NT * 32;
    char* Qs = smem;
    char* Ks = Qs + LP * ABW_ROW;
    char* Vs = Ks + LP * ABW_ROW;
    char* Ds = Vs + LP * ABW_ROW;
    float* s_m = reinterpret_cast<float*>(Ds + LP * ABW_ROW);        // [LP] each
    float* s_il = s_m + LP;
    float* s_de = s_il + LP;
    const int b = blockIdx.x / H, h = blockIdx.x % H;
    const int W = H * ATT_DH, ld = 3 * W;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hi = lane >> 5, ql = lane & 31;
    const half_t* qbase = qkv + (size_t)b * L * ld + h * ATT_DH;
    const half_t* dbase = dout + (size_t)b * L * W + h * ATT_DH;
    half_t* gbase = dqkv + (size_t)b * L * ld + h * ATT_DH;

    // staging: 8 rows x 128 B per wave instruction, swizzle on the source chunk (as the forward's K)
    for (int r0 = wave * 8; r0 < LP; r0 += NW * 8) {
        const int r = r0 + (lane >> 3);
        const int c = (lane & 7) ^ pgemm::swz_key(r);
        const int rc = r < L ? r : L - 1;
        const half_t* src = qbase + (size_t)rc * ld + c * 8;
        __builtin_amdgcn_global_load_lds((pgemm::gbl_ptr_t)(src), (pgemm::lds_ptr_t)(Qs + r0 * ABW_ROW), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((pgemm::gbl_ptr_t)(src + W), (pgemm::lds_ptr_t)(Ks + r0 * ABW_ROW), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((pgemm::gbl_ptr_t)(src + 2 * W), (pgemm::lds_ptr_t)(Vs + r0 * ABW_ROW), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((pgemm::gbl_ptr_t)(dbase + (size_t)rc * W + c * 8), (pgemm::lds_ptr_t)(Ds + r0 * ABW_ROW), 16, 0, 0);
    }
    pgemm::wait_vm<0>();
    __syncthreads();

    int toff[2][2];
    abw_toff(lane, toff);

    // ---- pass Q: statistics and dQ, the query on the lane ----------------------------------------------------------------
    for (int qt = wave; qt < NT; qt += NW) {                         // wave-uniform: EXEC stays full for the transposed reads
        const int q = qt * 32 + ql;
        half8_t qf[4], df[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) { qf[s] = abw_row_frag(Qs, q, s * 2 + hi); df[s] = abw_row_frag(Ds, q, s * 2 + hi); }
        const int tend = causal ? qt + 1 : NT;                       // causal: the key tiles beyond the query tile are all masked
        const int kend = causal ? (q + 1 < L ? q + 1 : L) : L;       // key k is valid iff k < kend (>= 1: key 0 is valid for every row)
        float mrun = -__builtin_inff(), lrun = 0.f, urun = 0.f;
        for (int t = 0; t < tend; ++t) {
            float16_t st = abw_product(Ks, t, ql, hi, qf);
            const float16_t dp = abw_product(Vs, t, ql, hi, df);
            const int lim = kend - t * 32 - 4 * hi;
            float tmax = -__builtin_inff();
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                if (!((e & 3) + 8 * (e >> 2) < lim)) st[e] = -__builtin_inff();
                tmax = fmaxf(tmax, st[e]);
            }
            tmax = half_wave_max(tmax) * kAbwScale;
            const float mnew = fmaxf(mrun, tmax);                    // finite from the first tile on
            const float alpha = __builtin_amdgcn_exp2f(mrun - mnew); // exp2(-inf) = 0 on the first tile
            float psum = 0.f, usum = 0.f;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(st[e], kAbwScale, -mnew));      // masked: exp2(-inf) = 0
                psum += p;
                usum = __builtin_fmaf(p, dp[e], usum);
            }
            psum = half_wave_sum(psum);
            usum = half_wave_sum(usum);
            lrun = __builtin_fmaf(lrun, alpha, psum);
            urun = __builtin_fmaf(urun, alpha, usum);
            mrun = mnew;
        }
        const float invl = 1.f / lrun, delta = urun * invl;
        if (hi == 0) { s_m[q] = mrun; s_il[q] = invl; s_de[q] = delta; }
        float16_t acc[2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
        for (int t = 0; t < tend; ++t) {
            float16_t st = abw_product(Ks, t, ql, hi, qf);
            const float16_t dp = abw_product(Vs, t, ql, hi, df);
            const int lim = kend - t * 32 - 4 * hi;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const bool valid = (e & 3) + 8 * (e >> 2) < lim;
                const float p = valid ? __builtin_amdgcn_exp2f(__builtin_fmaf(st[e], kAbwScale, -mrun)) * invl : 0.f;
                st[e] = p * (dp[e] - delta);
            }
#pragma unroll
            for (int sidx = 0; sidx < 2; ++sidx) {
                const half8_t dsf = abw_pack(st, sidx);
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(abw_tr_frag(Ks, t * 32 + sidx * 16, toff, j), dsf, acc[j], 0, 0, 0);
            }
        }
        attn_store_tile(gbase + (size_t)(q < L ? q : 0) * ld, acc, 8.f, hi, q < L);          // dQ = (dS K) / 8
    }
    __syncthreads();

    // ---- pass K: dK and dV, the key on the lane --------------------------------------------------------------------------
    for (int kt = wave; kt < NT; kt += NW) {
        const int k = kt * 32 + ql;
        half8_t kf[4], vf[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) { kf[s] = abw_row_frag(Ks, k, s * 2 + hi); vf[s] = abw_row_frag(Vs, k, s * 2 + hi); }
        float16_t av[2], ak[2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) av[j][e] = ak[j][e] = 0.f;
        for (int t = causal ? kt : 0; t < NT; ++t) {                 // causal: the query tiles before the key tile are all masked
            float16_t st = abw_product(Qs, t, ql, hi, kf);
            const float16_t dp = abw_product(Ds, t, ql, hi, vf);
            float16_t pv;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int q0 = t * 32 + 8 * g + 4 * hi;              // this lane's queries q0 .. q0 + 3 (elements 4 g .. 4 g + 3)
                const float4_t m4 = *reinterpret_cast<const float4_t*>(s_m + q0);
                const float4_t il4 = *reinterpret_cast<const float4_t*>(s_il + q0);
                const float4_t de4 = *reinterpret_cast<const float4_t*>(s_de + q0);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int e = 4 * g + r, qq = q0 + r;
                    const bool valid = qq < L && (!causal || qq >= k);
                    const float p = valid ? __builtin_amdgcn_exp2f(__builtin_fmaf(st[e], kAbwScale, -m4[r])) * il4[r] : 0.f;
                    pv[e] = p;
                    st[e] = p * (dp[e] - de4[r]);
                }
            }
#pragma unroll
            for (int sidx = 0; sidx < 2; ++sidx) {
                const half8_t pf = abw_pack(pv, sidx), dsf = abw_pack(st, sidx);
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    av[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(abw_tr_frag(Ds, t * 32 + sidx * 16, toff, j), pf, av[j], 0, 0, 0);
                    ak[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(abw_tr_frag(Qs, t * 32 + sidx * 16, toff, j), dsf, ak[j], 0, 0, 0);
                }
            }
        }
        half_t* row = gbase + (size_t)(k < L ? k : 0) * ld;
        attn_store_tile(row + W, ak, 8.f, hi, k < L);                // dK = (dS^T Q) / 8
        attn_store_tile(row + 2 * W, av, 1.f, hi, k < L);            // dV = P^T dO
    }
}
}  // namespace

extern "C" int pclip_attention_backward_f16(const void* qkv, const void* dout, void* dqkv, int B, int L, int H, int dh, int causal,
                                            pclip_stream_t stream) {
    PCLIP_REQUIRE(qkv && dout && dqkv, "pclip_attention_backward_f16: null pointer");
    PCLIP_REQUIRE(dh == ATT_DH, "pclip_attention_backward_f16: head dim %d unsupported (must be 64)", dh);
    PCLIP_REQUIRE(B >= 0 && H > 0 && L >= 1 && L <= ABW_MAX_L, "pclip_attention_backward_f16: bad B=%d H=%d L=%d (1 <= L <= %d)", B, H, L, ABW_MAX_L);
    PCLIP_REQUIRE((long)B * H <= 0x7fffffffL, "pclip_attention_backward_f16: B * H = %ld exceeds the grid", (long)B * H);
    PCLIP_REQUIRE(!(((uintptr_t)qkv | (uintptr_t)dout | (uintptr_t)dqkv) & 15), "pclip_attention_backward_f16: operands must be 16-byte aligned");
    PCLIP_REQUIRE(dqkv != qkv && dqkv != dout, "pclip_attention_backward_f16: dqkv must not alias an input");
    if (B == 0) return PCLIP_OK;
    const int NT = ceil_div(L, 32), LP = NT * 32;
    const size_t lds = (size_t)LP * (4 * ABW_ROW + 3 * sizeof(float));       // 150 912 B at L = 288
    static DevOnce attr_set;
    if (int e = pclip_raise_lds(attr_set, {(const void*)attention_bwd_kernel<4>, (const void*)attention_bwd_kernel<8>}, 160 * 1024, "pclip_attention_backward_f16")) return e;
    // up to four tiles: four waves (two workgroups per CU fit the LDS up to L = 128); more: eight waves, one workgroup per CU
    if (NT <= 4)
        attention_bwd_kernel<4><<<B * H, 4 * 64, lds, (hipStream_t)stream>>>((const half_t*)qkv, (const half_t*)dout, (half_t*)dqkv, L, H, causal, NT);
    else
        attention_bwd_kernel<8><<<B * H, 8 * 64, lds, (hipStream_t)stream>>>((const half_t*)qkv, (const half_t*)dout, (half_t*)dqkv, L, H, causal, NT);
    return pclip_check_launch("attention backward");
}
