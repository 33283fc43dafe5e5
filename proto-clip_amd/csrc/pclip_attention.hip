// Attention of the CLIP towers (clip/model.py:183-185) up to 288 tokens: one workgroup per (image, head), K / V resident in LDS, online softmax in registers
// (per-tile code: pclip_attention_tile.h; longer sequences: pclip_attention_long.hip).
#include "pclip_attention_tile.h"
#include <stdlib.h>
#include <type_traits>

namespace {
constexpr int ATT_MAX_L = 288;

// General operand form: queries q [B][Lq rows, row stride ldq] (the FIRST Lq tokens of each sequence), keys / values in
// kv [B*L rows, row stride ldkv] at column offsets k_off / v_off; the fused-QKV case is q = kv = qkv, ldq = ldkv = 3W,
// k_off = W, v_off = 2W, Lq = L.  Lq < L serves the last vision block, whose output is only read at the class token.
// QF (round 4): every wave has AT MOST ONE query tile (the host guarantees ceil(Lq / 32) <= NW, hence LP <= 256: at most four pieces per wave and operand) and
// requests its query fragments BEFORE the K / V stages, so their round trip passes under the staging instead of opening the compute phase behind the barrier
// (ViT-B/16 354 -> 320 us stand-alone); and the workgroup barrier only waits for K — V is awaited (own pieces + a second LDS-only barrier) between the first
// pair of key tiles' softmax and its second contraction (-> 303 us).  Same bits (profiles/r04_ab_attention_qfirst.txt).  Not for waves that loop over several tiles (ViT-L/14: + 6 %) nor the short causal text sequences (+ 7 %).
template <int NW, int VAR, bool QF = false>   // waves per workgroup (__launch_bounds__'s second argument = waves per SIMD: two workgroups per CU); softmax variant
__global__ __launch_bounds__(NW * 64, NW / 2) void attention_kernel(const half_t* __restrict__ qp, int ldq, long q_batch,
                                                           const half_t* __restrict__ kvp, int ldkv, int k_off, int v_off,
                                                           half_t* __restrict__ out, int L, int Lq, int H, int causal, int NT,
                                                           int /* former V leading dimension: V is kept row-major, always 0 */) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int LP = NT * 32;
    half_t* Ks = reinterpret_cast<half_t*>(smem);             // [LP][64], 16-byte chunks XOR-swizzled by swz_key(row)
    half_t* Vs = Ks + LP * ATT_DH;                            // [LP][64]: V row-major, chunk-swizzled (see the staging loop)
    const int b = blockIdx.x / H, h = blockIdx.x % H;
    const int W = H * ATT_DH;
    const half_t* kbase = kvp + (size_t)b * L * ldkv + h * ATT_DH + k_off;
    const half_t* vbase = kvp + (size_t)b * L * ldkv + h * ATT_DH + v_off;
    const half_t* qbase = qp + (size_t)b * q_batch + h * ATT_DH;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    half8_t qf0[4];
    if (QF) {
        const int q0 = wave * 32 + (lane & 31), qc0 = q0 < Lq ? q0 : Lq - 1;
#pragma unroll
        for (int s_ = 0; s_ < 4; ++s_) qf0[s_] = ld_half8(qbase + (size_t)qc0 * ldq + s_ * 16 + (lane >> 5) * 8);
    }

    // K: global_load_lds, 8 rows x 128 B per wave instruction, swizzle on the source chunk (as the GEMM tiles)
    for (int r0 = wave * 8; r0 < LP; r0 += NW * 8) {
        const int r = r0 + (lane >> 3);
        const int c = (lane & 7) ^ pgemm::swz_key(r);
        const int rc = r < L ? r : L - 1;                     // rows >= L are masked in the scores
        __builtin_amdgcn_global_load_lds((pgemm::gbl_ptr_t)(kbase + (size_t)rc * ldkv + c * 8),
                                         (pgemm::lds_ptr_t)(Ks + r0 * ATT_DH), 16, 0, 0);
    }
    // V: row-major like K, by LDS-DMA (no registers, no transposing ds_writes); the 16-byte chunks of key row r are XORed with
    // 4 * ((r >> 1) & 1) so that the four keys of a transpose-read (ds_read_b64_tr_b16, below) land on 4 x 16 distinct banks.
    // Rows >= L re-read row L-1: their probabilities are exact zeros (masked scores), so they contribute 0 * finite = 0.
    for (int r0 = wave * 8; r0 < LP; r0 += NW * 8) {
        const int r = r0 + (lane >> 3);
        const int c = (lane & 7) ^ (((r >> 1) & 1) << 2);
        const int rc = r < L ? r : L - 1;
        __builtin_amdgcn_global_load_lds((pgemm::gbl_ptr_t)(vbase + (size_t)rc * ldkv + c * 8),
                                         (pgemm::lds_ptr_t)(Vs + r0 * ATT_DH), 16, 0, 0);
    }
#ifndef PCLIP_ATT_VBAR
#define PCLIP_ATT_VBAR 1          // QF kernels: barrier on K alone, V awaited between the first scores and the first second contraction (334.7 -> 303.5 us stand-alone, same bits)
#endif
    constexpr bool VB = PCLIP_ATT_VBAR && QF;
    if (VB) {
        // the wave's V pieces (the youngest operations: rows wave * 8 + NW * 8 k < LP, one to four of them) stay in flight: K and the query fragments have landed
        // once no more than those are outstanding
        const int nv = (LP - wave * 8 + NW * 8 - 1) / (NW * 8);
        // (EXACTLY nv: with "<= 2 -> vmcnt(2)" a wave of the four-wave form that stages ONE piece per operand (L <= 32) went through with its K piece still in flight —
        // caught by a small-tower image -> logits fixture failing in two of four runs)
        if (nv <= 1) pgemm::wait_vm<1>(); else if (nv == 2) pgemm::wait_vm<2>(); else if (nv == 3) pgemm::wait_vm<3>(); else pgemm::wait_vm<4>();
        pgemm::lds_barrier();
    } else
        __syncthreads();

    const int hi = lane >> 5, ql = lane & 31;
    int voff[2];
    attn_voff(lane, voff);
    const int NTq = (Lq + 31) >> 5;
    auto process = [&](int qb, const half8_t (&qf)[4]) {
        const int q = qb * 32 + ql;
        float16_t o[2];
        float lrun;
        attn_query_tile<false, VAR, VB>(Ks, Vs, qf, q, qb, L, causal, NT, hi, ql, voff, o, lrun);
        attn_store_tile(out + ((size_t)b * Lq + q) * W + h * ATT_DH, o, lrun, hi, q < Lq);
    };
    if (QF) {
        if (wave < NTq) process(wave, qf0);
        else if (VB) { pgemm::wait_vm<0>(); pgemm::lds_barrier(); }      // the barrier inside the first pair of key tiles
        return;
    }
    for (int qb = wave; qb < NTq; qb += NW) {
        const int q = qb * 32 + ql;                     // this lane's query row
        const int qc = q < Lq ? q : Lq - 1;
        half8_t qf[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) qf[s] = ld_half8(qbase + (size_t)qc * ldq + s * 16 + hi * 8);
        process(qb, qf);
    }
}

// ---- persistent, double-buffered form of the same attention (whole batches) --------------------------------------------------
// attention_kernel is a chain of dependent phases per (image, head): K/V by LDS-DMA -> barrier -> query loads -> compute -> stores,
// and two co-resident workgroups fall into lockstep, so the memory pipe idles while the SIMDs work and vice versa (ablation,
// the parts ADD).  Here a workgroup walks items (image, head) i, i + G, ...: while item i is multiplied out of LDS
// buffer i & 1, the K/V rows of item i + G arrive in the other buffer and its query rows in a third region, all by LDS-DMA, and
// the output stores of item i drain during item i + G.  Per wave and iteration the vector-memory stream is
//   DMA(next: K, V, Q pieces) | 4 output stores (this)
// so the wait at the top of the next iteration is the counted vmcnt(4): everything but this item's stores.
// The LDS-DMA instructions are INLINE ASM (attn_dma16, pclip_attention_tile.h).  hipcc's wait-count pass treats a pending LDS-DMA it knows about as a pending LDS
// write: it put s_waitcnt vmcnt(0) in front of the first ds_read_b64_tr_b16 of the compute phase (the transpose-read intrinsic
// carries no address it could disambiguate), i.e. it drained the prefetch right where it was meant to overlap.  An asm LDS-DMA
// has no register destination (register-safe, guide §5.7 item 1); its completion is ordered by the explicit vmcnt + barrier
// below.  M0 (the LDS destination) is saved and restored inside the statement; the descriptor and M0 come from readfirstlane,
// hence the leading s_nop 4 (SALU write -> VMEM read of an SGPR).
// One buffer descriptor per item and operand (base = the image's first row at this head) with per-lane byte offsets that are
// the same for every item (row * ld + swizzled chunk) and the K / V column offset in the scalar offset.
// Arithmetic per query tile = attn_query_tile: bit-identical to attention_kernel.
// Requires Lq == L, NT <= NW (one query tile per wave; waves without a tile only stage) and 2 x (K + V) + Q rows <= 160 KiB.
template <int NW, int WPS, int VAR>   // waves per workgroup, waves per SIMD the register budget must allow, softmax variant
__global__ __launch_bounds__(NW * 64, WPS) void attention_pipe_kernel(const half_t* __restrict__ qp, int ldq, long q_batch,
                                                                      const half_t* __restrict__ kvp, int ldkv, int k_off, int v_off,
                                                                      half_t* __restrict__ out, int L, int H, int causal, int NT, int KR,
                                                                      int nitems) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NST = 4;                                    // output stores per wave and item (attn_store_tile)
    constexpr int MAXP = 4;                                   // LDS-DMA pieces (8 rows each) per wave and operand: NT*32 <= NW*8*MAXP
    constexpr int RB = ATT_DH * 2;                            // bytes per row
    const int LP = NT * 32;
    const int BUF = (KR + LP) * RB;                           // bytes per K/V buffer: K rows [0, KR) | V rows [0, LP)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hi = lane >> 5, ql = lane & 31;
    const int W = H * ATT_DH, G = gridDim.x;
    const bool has_tile = wave < NT;
    const unsigned lds0 = (unsigned)(size_t)(pgemm::lds_ptr_t)smem;
    char* Qs = smem + 2 * BUF;                                // [KR rows][64] query rows of the item about to be computed (K swizzle)
    int voff[2];
    attn_voff(lane, voff);
    // per-lane source offsets of this wave's pieces, identical for every item
    int kvo[MAXP], vvo[MAXP], qvo[MAXP];
#pragma unroll
    for (int i = 0; i < MAXP; ++i) {
        const int r = wave * 8 + i * NW * 8 + (lane >> 3);
        const int rc = r < L ? r : L - 1;                     // K / Q rows >= L: masked / never stored; V rows >= L: finite filler (their probabilities are exact zeros)
        const int ck = ((lane & 7) ^ pgemm::swz_key(r)) << 3, cv = ((lane & 7) ^ (((r >> 1) & 1) << 2)) << 3;
        kvo[i] = (rc * ldkv + ck) * 2;
        vvo[i] = (rc * ldkv + cv) * 2;
        qvo[i] = (rc * ldq + ck) * 2;
    }
    const int q = wave * 32 + ql;                             // this lane's query row (has_tile)
    auto stage = [&](int item, int buf) {
        const int b = item / H, h = item - b * H;
        const uint4_t rkv = attn_rsrc(kvp + (size_t)b * L * ldkv + h * ATT_DH);
        const uint4_t rq = attn_rsrc(qp + (size_t)b * q_batch + h * ATT_DH);
        const unsigned kb = lds0 + buf * BUF, vb = kb + KR * RB, qb = lds0 + 2 * BUF;
#pragma unroll
        for (int i = 0; i < MAXP; ++i) {
            const int r0 = wave * 8 + i * NW * 8;
            if (r0 < KR) attn_dma16(rkv, kvo[i], k_off * 2, kb + r0 * RB);
        }
#pragma unroll
        for (int i = 0; i < MAXP; ++i) {
            const int r0 = wave * 8 + i * NW * 8;
            if (r0 < LP) attn_dma16(rkv, vvo[i], v_off * 2, vb + r0 * RB);
        }
#pragma unroll
        for (int i = 0; i < MAXP; ++i) {
            const int r0 = wave * 8 + i * NW * 8;
            if (r0 < KR) attn_dma16(rq, qvo[i], 0, qb + r0 * RB);
        }
    };
    int item = blockIdx.x;
    if (item >= nitems) return;
    stage(item, 0);
    for (int it = 0; item < nitems; item += G, ++it) {
        const int cur = it & 1;
        // this item's K / V / Q pieces have landed (the previous item's stores may still be in flight)
        if (has_tile && it > 0) pgemm::wait_vm<NST>(); else pgemm::wait_vm<0>();
        pgemm::lds_barrier();                                 // everyone's pieces are visible; everyone is done with the other K/V buffer
        half8_t qf[4];
        if (has_tile) {
            const int qr = q < KR ? q : KR - 1;               // rows of the last tile beyond the staged ones: never stored
#pragma unroll
            for (int s = 0; s < 4; ++s)
                qf[s] = *reinterpret_cast<const half8_t*>(Qs + qr * RB + (((s * 2 + hi) ^ pgemm::swz_key(qr)) << 4));
        }
        pgemm::lds_barrier();                                 // every wave holds its query fragments: the Q region is free
#ifndef PCLIP_ATT_ABL
#define PCLIP_ATT_ABL 0          // ablation builds (tools/ablate_attention.py): 1 no prefetch DMA in the loop, 2 no compute, 4 no stores
#endif
        const int next = item + G;
        if (next < nitems && !(PCLIP_ATT_ABL & 1)) stage(next, cur ^ 1);
        if (has_tile) {
            const half_t* Ks = reinterpret_cast<const half_t*>(smem + cur * BUF);
            const half_t* Vs = Ks + KR * ATT_DH;
            float16_t o[2];
            float lrun;
#ifndef PCLIP_ATT_STAGGER
#define PCLIP_ATT_STAGGER 0
#endif
#if PCLIP_ATT_STAGGER && defined(__HIP_DEVICE_COMPILE__)
            if (wave >= NW / 2) __builtin_amdgcn_s_sleep(PCLIP_ATT_STAGGER);     // second wave of each SIMD: start out of phase with the first
#endif
            if (PCLIP_ATT_ABL & 2) {
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int e = 0; e < 16; ++e) o[j][e] = (float)qf[e & 3][e & 7];
                lrun = 1.f;
            } else
                attn_query_tile<true, VAR>(Ks, Vs, qf, q, wave, L, causal, NT, hi, ql, voff, o, lrun);
            const int b = item / H, h = item - b * H;
            attn_store_tile(out + ((size_t)b * L + q) * W + h * ATT_DH, o, lrun, hi, q < L && !(PCLIP_ATT_ABL & 4));
        }
    }
}

}  // namespace

static int att_mode_from_env() {                 // PCLIP_ATT_PIPE=0 / 1: initial mode (A/B runs of whole programs); default automatic
    const char* e = getenv("PCLIP_ATT_PIPE");
    return e && (e[0] == '0' || e[0] == '1') ? e[0] - '0' : -1;
}
static int g_att_mode = att_mode_from_env(), g_att_grid = 0;
extern "C" int pclip_attention_config(int mode, int max_grid) {
    PCLIP_REQUIRE(mode >= -1 && mode <= 1 && max_grid >= 0, "pclip_attention_config: bad mode=%d max_grid=%d", mode, max_grid);
    g_att_mode = mode;
    g_att_grid = max_grid;
    return PCLIP_OK;
}

extern "C" int pclip_attention_q_f16(const void* q, int ldq, long q_batch_stride, const void* kv, int ldkv, int k_off, int v_off,
                                     void* out, int B, int L, int Lq, int H, int dh, int causal, pclip_stream_t stream) {
    PCLIP_REQUIRE(q && kv && out, "pclip_attention_q_f16: null pointer");
    PCLIP_REQUIRE(dh == ATT_DH, "pclip_attention_q_f16: head dim %d unsupported (must be 64)", dh);
    PCLIP_REQUIRE(B >= 0 && H > 0 && L > 0 && L <= ATT_MAX_L && Lq > 0 && Lq <= L, "pclip_attention_q_f16: bad B=%d H=%d L=%d Lq=%d (L <= %d)",
                  B, H, L, Lq, ATT_MAX_L);
    PCLIP_REQUIRE(!causal || Lq == L, "pclip_attention_q_f16: the causal mask needs all queries (Lq == L)");
    PCLIP_REQUIRE(ldq % 8 == 0 && ldkv % 8 == 0 && k_off % 8 == 0 && v_off % 8 == 0 && q_batch_stride % 8 == 0,
                  "pclip_attention_q_f16: strides / offsets must be multiples of 8 halves");
    if (B == 0) return PCLIP_OK;
    const int NT = ceil_div(L, 32), LP = NT * 32;
    // mode 1 only: the persistent double-buffered kernel, one workgroup per CU (short sequences: as many as the LDS holds, at
    // most two: the register budget of the deep-prefetch loop).  Measured: 8 % faster than one workgroup per
    // item in isolation on N(0,1) data (348 vs 377 us, ViT-B/16 B = 1024), no faster inside the encoder (40.3 vs 40.2 ms per
    // step, same-box A/B) — the automatic mode does not select it.
    const long nitems = (long)B * H;
    const int cus = pclip_device_cus();
    const int KR = (L + 7) / 8 * 8;
    const size_t plds = (2 * (size_t)(KR + LP) + KR) * ATT_DH * 2;          // two K/V buffers + the query rows
    if (Lq == L && g_att_mode != 0 && NT <= 8 && plds <= 160 * 1024 && cus > 0 && g_att_mode == 1) {
        static DevOnce pipe_attr;
        if (int e = pclip_raise_lds(pipe_attr, {(const void*)attention_pipe_kernel<4, 2, PCLIP_ATT_VAR_SHORT>, (const void*)attention_pipe_kernel<8, 2, PCLIP_ATT_VAR_LONG>},
                                    160 * 1024, "pclip_attention_f16"))
            return e;
        int per_cu = NT <= 4 ? (int)((160 * 1024) / plds) : 1;
        per_cu = per_cu < 1 ? 1 : (per_cu > 2 ? 2 : per_cu);
        long grid = (long)cus * per_cu;
        if (g_att_grid > 0 && g_att_grid < grid) grid = g_att_grid;
        if (grid > nitems) grid = nitems;
        if (NT <= 4)
            attention_pipe_kernel<4, 2, PCLIP_ATT_VAR_SHORT><<<(int)grid, 256, plds, (hipStream_t)stream>>>((const half_t*)q, ldq, q_batch_stride, (const half_t*)kv, ldkv,
                                                                                      k_off, v_off, (half_t*)out, L, H, causal, NT, KR, (int)nitems);
        else
            attention_pipe_kernel<8, 2, PCLIP_ATT_VAR_LONG><<<(int)grid, 512, plds, (hipStream_t)stream>>>((const half_t*)q, ldq, q_batch_stride, (const half_t*)kv, ldkv,
                                                                                      k_off, v_off, (half_t*)out, L, H, causal, NT, KR, (int)nitems);
        return pclip_check_launch("attention (pipelined)");
    }
    const size_t lds = 2 * (size_t)LP * ATT_DH * 2;
    // The softmax variant follows the SEQUENCE (more than four key tiles: the long form), not the kernel: the one-query form of the
    // last vision block (Lq = 1, four waves) must produce the bits of the full attention over the same keys.
    static DevOnce attr_set;
    if (int e = pclip_raise_lds(attr_set, {(const void*)attention_kernel<8, PCLIP_ATT_VAR_LONG>, (const void*)attention_kernel<4, PCLIP_ATT_VAR_LONG>,
                                           (const void*)attention_kernel<4, PCLIP_ATT_VAR_SHORT>, (const void*)attention_kernel<8, PCLIP_ATT_VAR_LONG, true>,
                                           (const void*)attention_kernel<4, PCLIP_ATT_VAR_SHORT, true>},
                                80 * 1024, "pclip_attention_f16"))
        return e;
    // more than four query tiles (ViT-B/16: 7, ViT-L/14: 9): eight waves, one tile each, two workgroups = four waves per SIMD
    // (VGPRs capped at 128); measured 438 -> 424 us (ViT-B/16), 224 -> 200 us (ViT-L/14), bit-identical.  Short sequences
    // (ViT-B/32: 2 tiles, text: 3) keep the four-wave workgroup, whose idle waves cost less.
#define PCLIP_ATT_LAUNCH(NW, VAR)                                                                                                         \
    attention_kernel<NW, VAR><<<B * H, NW * 64, lds, (hipStream_t)stream>>>((const half_t*)q, ldq, q_batch_stride, (const half_t*)kv, ldkv, k_off, \
                                                                             v_off, (half_t*)out, L, Lq, H, causal, NT, 0)
    static const bool qfirst = pclip_env_on("PCLIP_ATT_QFIRST");      // A/B switch
    // short NON-causal sequences (ViT-B/32: 50 tokens = 2 tiles): every wave of the four-wave workgroup has at most one tile too: 71.9 -> 68.0 us (B = 1024), same bits;
    // the causal text sequences (77 tokens) lose 14 % in this form (489 -> 558 us: their waves' work is triangular) and keep the looping kernel
    if (PCLIP_ATT_QF4 && qfirst && NT <= 4 && Lq == L && !causal)
        attention_kernel<4, PCLIP_ATT_VAR_SHORT, true><<<B * H, 4 * 64, lds, (hipStream_t)stream>>>((const half_t*)q, ldq, q_batch_stride, (const half_t*)kv, ldkv, k_off,
                                                                                                     v_off, (half_t*)out, L, Lq, H, causal, NT, 0);
    else if ((Lq + 31) / 32 > 4 && (Lq + 31) / 32 <= 8 && NT <= 8 && qfirst)      // NT <= 8: the kernel's counted waits assume at most four pieces per wave and operand
        attention_kernel<8, PCLIP_ATT_VAR_LONG, true><<<B * H, 8 * 64, lds, (hipStream_t)stream>>>((const half_t*)q, ldq, q_batch_stride, (const half_t*)kv, ldkv, k_off,
                                                                                                    v_off, (half_t*)out, L, Lq, H, causal, NT, 0);
    else if ((Lq + 31) / 32 > 4) PCLIP_ATT_LAUNCH(8, PCLIP_ATT_VAR_LONG);
    else if (NT > 4) PCLIP_ATT_LAUNCH(4, PCLIP_ATT_VAR_LONG);
    else PCLIP_ATT_LAUNCH(4, PCLIP_ATT_VAR_SHORT);
#undef PCLIP_ATT_LAUNCH
    return pclip_check_launch("attention");
}

extern "C" int pclip_attention_f16(const void* qkv, void* out, int B, int L, int H, int dh, int causal,
                                   pclip_stream_t stream) {
    PCLIP_REQUIRE(qkv && out, "pclip_attention_f16: null pointer");
    PCLIP_REQUIRE(H > 0 && L > 0, "pclip_attention_f16: bad H=%d L=%d", H, L);
    const int W = H * dh;
    return pclip_attention_q_f16(qkv, 3 * W, (long)L * 3 * W, qkv, 3 * W, W, 2 * W, out, B, L, L, H, dh, causal, stream);
}