// Attention of long sequences (clip/model.py:183-185 at L > 288: ViT-L/14@336px, 577 tokens): K / V of the head STREAMED through LDS
// 128 keys at a time instead of resident, so the LDS per workgroup does not depend on L.  Non-causal only (the causal text sequences
// are 77 tokens and stay on pclip_attention.hip).
#include "pclip_attention_tile.h"

namespace {
constexpr int ATT_LONG_MAX_L = 4096;
constexpr int ATT_LONG_NW = 8;                           // waves per workgroup: at most one 32-query tile each
constexpr int ATT_LONG_SROWS = 128;                      // key rows per LDS stage (four key tiles = two pairs of attn_key_tiles)
constexpr int ATT_LONG_SBYTES = 2 * ATT_LONG_SROWS * ATT_DH * 2;      // one stage: K rows | V rows (32 KiB)
constexpr int ATT_LONG_PIECES = ATT_LONG_SROWS / (ATT_LONG_NW * 8);    // LDS-DMA wave instructions (8 rows each) per wave, stage and operand (2)

// A workgroup = (image, head, group of up to eight query tiles); G groups per (image, head) share the query tiles evenly (`per` each).
// Every wave keeps its query fragments in registers and walks the key stages with attn_key_tiles — the per-tile code of the resident
// kernels on the same 32-key tiles in the same order, so for 128 < L <= 288 the bits equal pclip_attention_f16's, and a query row's
// bits do not depend on Lq or on the rows that share its workgroup.  Waves without a query tile only stage.
// Staging: two LDS buffers, one stage in flight.  At the top of stage s a wave waits for its own pieces of stage s (vmcnt(0): nothing
// else is outstanding), the LDS-only barrier makes everyone's visible and tells that every wave is done with stage s - 1, whose buffer
// then receives stage s + 1 by LDS-DMA while stage s is multiplied — one barrier per 128 keys.  LDS-DMA, not registers: the per-tile
// code already fills the 128-VGPR budget of four waves per SIMD, and register staging (16 VGPRs) spilled.  The DMA is inline asm
// (attn_dma16): the builtin would make hipcc drain it in front of the first LDS read of the stage.  8 rows x 128 B per wave
// instruction, lane-linear in LDS with the swizzle on the source chunk: K chunk c of row r at slot c ^ swz_key(r), V at c ^ 4 * ((r >> 1)
// & 1), the layouts attn_key_tiles reads (rows relative to the stage, whose first row is a multiple of 128).  Rows >= L re-read row
// L - 1: their scores are masked and their probabilities exact zeros.
template <int VAR>
__global__ __launch_bounds__(ATT_LONG_NW * 64, ATT_LONG_NW / 2) void attention_long_kernel(const half_t* __restrict__ qp, int ldq, long q_batch,
                                                                                      const half_t* __restrict__ kvp, int ldkv, int k_off, int v_off,
                                                                                      half_t* __restrict__ out, int L, int Lq, int H, int G, int per) {
    __shared__ __attribute__((aligned(16))) char smem[2 * ATT_LONG_SBYTES];
    const int grp = blockIdx.x % G, item = blockIdx.x / G;
    const int b = item / H, h = item - b * H;
    const int W = H * ATT_DH;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hi = lane >> 5, ql = lane & 31;
    const half_t* qbase = qp + (size_t)b * q_batch + h * ATT_DH;
    const int NTq = (Lq + 31) >> 5;
    const int qb = grp * per + wave;                       // this wave's query tile
    const bool has_tile = wave < per && qb < NTq;
    const int q = qb * 32 + ql;                            // this lane's query row
    half8_t qf[4];
    if (has_tile) {
        const int qc = q < Lq ? q : Lq - 1;                // rows beyond Lq: computed, never stored
#pragma unroll
        for (int s = 0; s < 4; ++s) qf[s] = ld_half8(qbase + (size_t)qc * ldq + s * 16 + hi * 8);
    }

    const uint4_t rkv = attn_rsrc(kvp + (size_t)b * L * ldkv + h * ATT_DH);       // byte offsets: row * ldkv * 2 < 2^31 (host check)
    const unsigned lds0 = (unsigned)(size_t)(pgemm::lds_ptr_t)smem;
    auto stage = [&](int st, int buf) {
        const unsigned kb = lds0 + buf * ATT_LONG_SBYTES, vb = kb + ATT_LONG_SROWS * ATT_DH * 2;
#pragma unroll
        for (int i = 0; i < ATT_LONG_PIECES; ++i) {
            const int r0 = wave * 8 + i * (ATT_LONG_NW * 8), rr = r0 + (lane >> 3);
            const int r = st * ATT_LONG_SROWS + rr, rc = r < L ? r : L - 1;
            const int ck = (lane & 7) ^ pgemm::swz_key(rr), cv = (lane & 7) ^ (((rr >> 1) & 1) << 2);
            attn_dma16(rkv, (rc * ldkv + ck * 8) * 2, k_off * 2, kb + r0 * (ATT_DH * 2));
            attn_dma16(rkv, (rc * ldkv + cv * 8) * 2, v_off * 2, vb + r0 * (ATT_DH * 2));
        }
    };

    int voff[2];
    attn_voff(lane, voff);
    float16_t o[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[j][e] = 0.f;
    float mrun = -__builtin_inff(), lrun = 0.f;
    const int NS = (L + ATT_LONG_SROWS - 1) / ATT_LONG_SROWS;
    stage(0, 0);
    for (int st = 0; st < NS; ++st) {
        pgemm::wait_vm<0>();                               // this wave's pieces of stage st (and, at st = 0, its query fragments)
        pgemm::lds_barrier();                              // everyone's; every wave is done with stage st - 1's buffer
        if (st + 1 < NS) stage(st + 1, (st + 1) & 1);
        if (has_tile) {
            const half_t* Ks = reinterpret_cast<const half_t*>(smem + (st & 1) * ATT_LONG_SBYTES);
            const half_t* Vs = Ks + ATT_LONG_SROWS * ATT_DH;
            const int Ls = L - st * ATT_LONG_SROWS;        // keys from this stage's first row on
            const int NTs = Ls >= ATT_LONG_SROWS ? ATT_LONG_SROWS / 32 : (Ls + 31) >> 5;
            attn_key_tiles<false, VAR, false>(Ks, Vs, qf, q, qb, Ls, 0, NTs, hi, ql, voff, o, mrun, lrun);
        }
    }
    if (has_tile) attn_store_tile(out + ((size_t)b * Lq + q) * W + h * ATT_DH, o, lrun, hi, q < Lq);
}
}  // namespace

extern "C" int pclip_attention_long_q_f16(const void* q, int ldq, long q_batch_stride, const void* kv, int ldkv, int k_off, int v_off,
                                          void* out, int B, int L, int Lq, int H, int dh, int causal, pclip_stream_t stream) {
    PCLIP_REQUIRE(q && kv && out, "pclip_attention_long_q_f16: null pointer");
    PCLIP_REQUIRE(dh == ATT_DH, "pclip_attention_long_q_f16: head dim %d unsupported (must be 64)", dh);
    PCLIP_REQUIRE(!causal, "pclip_attention_long_q_f16: causal attention is not supported (causal sequences of up to 288 tokens: pclip_attention_q_f16)");
    PCLIP_REQUIRE(B >= 0 && H > 0 && L > 0 && L <= ATT_LONG_MAX_L && Lq > 0 && Lq <= L,
                  "pclip_attention_long_q_f16: bad B=%d H=%d L=%d Lq=%d (L <= %d, 1 <= Lq <= L)", B, H, L, Lq, ATT_LONG_MAX_L);
    PCLIP_REQUIRE(ldq % 8 == 0 && ldkv % 8 == 0 && k_off % 8 == 0 && v_off % 8 == 0 && q_batch_stride % 8 == 0,
                  "pclip_attention_long_q_f16: strides / offsets must be multiples of 8 halves");
    const int NTq = ceil_div(Lq, 32);
    const int G = ceil_div(NTq, ATT_LONG_NW), per = ceil_div(NTq, G);     // ViT-L/14@336px: 19 query tiles = 7 + 7 + 5
    PCLIP_REQUIRE((long)B * H * G <= 0x7fffffffL, "pclip_attention_long_q_f16: B=%d H=%d too large for one launch", B, H);
    PCLIP_REQUIRE(ldq >= H * ATT_DH && k_off >= 0 && v_off >= 0 && k_off + H * ATT_DH <= ldkv && v_off + H * ATT_DH <= ldkv && (long)L * ldkv * 2 < 0x7fffffffL,
                  "pclip_attention_long_q_f16: bad row layout ldq=%d ldkv=%d k_off=%d v_off=%d for H=%d heads (and L * ldkv < 2^30)", ldq, ldkv, k_off, v_off, H);
    if (B == 0) return PCLIP_OK;
    attention_long_kernel<PCLIP_ATT_VAR_LONG><<<B * H * G, ATT_LONG_NW * 64, 0, (hipStream_t)stream>>>(
        (const half_t*)q, ldq, q_batch_stride, (const half_t*)kv, ldkv, k_off, v_off, (half_t*)out, L, Lq, H, G, per);
    return pclip_check_launch("attention (long sequences)");
}
