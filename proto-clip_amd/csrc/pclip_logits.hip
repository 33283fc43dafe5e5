// Cosine-similarity logits: the contrastive forward of CLIP (clip/model.py:356-370) and the zero-shot line `100. * features @ clip_weights`, ragged in M and T.
//   logits[m, t] = r16( sum_d r16(scale * a'[m, d]) * b'[t, d] ),  a' / b' = the rows as given or L2-normalised with the arithmetic of pclip_l2norm_rows_f16.
// The panel walk of pclip_panel_walk.h (staging, operand layout; the one-step-ahead loop over FOUR walked fragments is written out here).  What is this file's own:
// a workgroup (four waves) owns a panel of 16 RF rows of `a` (RF = 1, 2, 4 by M; at most 4 up to D = 1024, 2 up to 2048, 1 beyond) and walks the rows of `b`:
//   * the panel goes to LDS ONCE, already normalised and scaled (one wave per row: the very loads, butterfly and division chain of l2norm_rows_kernel, then
//     r16(scale * .) as an fp32 product rounded to fp16), rows D + 8 halves apart so that ds_read_b128 in the MFMA operand layout (lane = row l & 15, k-chunk
//     l >> 4) spreads over the banks; rows >= M are zeros and never read from memory;
//   * a wave takes blocks of 64 rows of `b` (four 16-row fragments) straight from memory in the MFMA operand layout (16 bytes per lane, the next k-step's
//     fragments in flight under the current one's MFMAs); rows >= T are clamped to row T - 1, their results dropped.  With PCLIP_LOGITS_NORMALIZE_B a first
//     launch writes the normalised rows into `ws` (T D halves: `b` is the small operand) and the walk reads those;
//   * v_mfma_f32_16x16x32_f16 with the rows of `b` as the first operand: a lane ends with 4 consecutive columns t of ONE row m per fragment — an 8-byte store
//     into the row-major logits, and a row's reduction stays inside 4 lanes x 4 waves.  ONE accumulator per element over k = 0, 32, ... D - 32 in that order
//     whatever M, T, RF or the grid: a row's logits do not depend on the rows that travel with it, a column's not on T, bit for bit;
//   * fused argmax / top-k: the rounded fp16 logit and its column make one 32-bit key (order-preserving value bits | 0xFFFF - column: greater = larger value,
//     then lower column; -0 counts as +0); every lane keeps the KMAX >= k best keys of its columns per row SORTED IN REGISTERS (KMAX = 1, 8, 16 compiled;
//     an insertion is a branch-free chain of v_max_u32 / v_min_u32 — per-lane lists in LDS with a threshold test diverged on almost every value: a lane's list
//     sees only T / 16 columns, so a third of them still enter a top-5), and after the walk the lists go to LDS over the dead panel and one thread per row
//     merges the row's 16 lists.  The [M, T] matrix never reaches memory then.
// Only __syncthreads barriers and compiler-counted waits: nothing here for the race-stress build.
// What bounds it: at M >> T every panel re-reads `b` through L2 (M / (16 RF) x T D 2 bytes) — see DESIGN section 3 and profiles/cosine_logits.txt
// (the plain matrix at 50 000 x 1000 is about 30 % slower than a GEMM that stages both operands in LDS).
#include "pclip_panel_walk.h"

namespace {

constexpr int LG_LDS_MAX = 160 * 1024;

template <int NCH, int RF, int KMAX>
__global__ __launch_bounds__(256) void cosine_logits_kernel(const half_t* __restrict__ a, int lda, int M, const half_t* __restrict__ b, int ldb, int T, int D,
                                                            float scale, int norm_a, half_t* __restrict__ logits, int ldl, int32_t* __restrict__ argmax,
                                                            half_t* __restrict__ topk_v, int32_t* __restrict__ topk_i, int k, int keff) {
    extern __shared__ __attribute__((aligned(16))) char lg_smem[];
    half_t* panel = reinterpret_cast<half_t*>(lg_smem);                                      // [16 RF][D + 8]
    const int LDP = D + PW_PAD;
    unsigned* lists = reinterpret_cast<unsigned*>(lg_smem);                                  // after the walk, over the panel: [256 threads][RF][KMAX] keys, descending, 0 = empty
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m0 = blockIdx.x * 16 * RF;

    stage_panel<NCH, 4, true>(panel, LDP, a, lda, M, D, m0, 16 * RF, lane, wave, norm_a, scale);              // normalised, scaled, rounded
    unsigned best[RF][KMAX > 0 ? KMAX : 1];                                                  // this lane's KMAX best keys per row fragment, descending
#pragma unroll
    for (int f = 0; f < RF; ++f)
#pragma unroll
        for (int i = 0; i < (KMAX > 0 ? KMAX : 1); ++i) best[f][i] = 0;
    __syncthreads();

    // ---- the walk over the rows of b ------------------------------------------------------------------------------------------------
    const int lr = lane & 15, lq = lane >> 4;
    const int KS = D >> 5, ncb = (T + 63) >> 6;
    for (int cb = blockIdx.y * 4 + wave; cb < ncb; cb += gridDim.y * 4) {
        const int t0 = cb * 64;
        const half_t* bp[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) bp[c] = walked_row(b, ldb, t0 + 16 * c + lr, T, lq);
        const half_t* ap = panel + (size_t)lr * LDP + lq * 8;
        float4_t acc[RF][4];
#pragma unroll
        for (int f = 0; f < RF; ++f)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[f][c] = float4_t{0.f, 0.f, 0.f, 0.f};
        half8_t bf[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) bf[c] = ld_half8(bp[c]);
        for (int ks = 0; ks < KS; ++ks) {
            half8_t bn[4];
            const int kn = ks + 1 < KS ? ks + 1 : ks;                                        // (the last step re-reads its own fragments: no read past column D)
#pragma unroll
            for (int c = 0; c < 4; ++c) bn[c] = ld_half8(bp[c] + kn * 32);
            half8_t af[RF];
#pragma unroll
            for (int f = 0; f < RF; ++f) af[f] = ld_half8(ap + (size_t)f * 16 * LDP + ks * 32);
#pragma unroll
            for (int f = 0; f < RF; ++f)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[f][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bf[c], af[f], acc[f][c], 0, 0, 0);
#pragma unroll
            for (int c = 0; c < 4; ++c) bf[c] = bn[c];
        }
        // acc[f][c][r] = logit(m0 + 16 f + lr, t0 + 16 c + 4 lq + r)
#pragma unroll
        for (int f = 0; f < RF; ++f) {
            const int m = m0 + 16 * f + lr;
            if (m >= M) continue;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int t = t0 + 16 * c + 4 * lq;
                if (t >= T) continue;
                const half4_t h = {(half_t)acc[f][c][0], (half_t)acc[f][c][1], (half_t)acc[f][c][2], (half_t)acc[f][c][3]};
                if (logits) {
                    half_t* o = logits + (size_t)m * ldl + t;
                    if (t + 3 < T) {
                        *reinterpret_cast<half4_t*>(o) = h;
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (t + r < T) o[r] = h[r];
                    }
                }
                if constexpr (KMAX > 0) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        unsigned key = t + r < T ? logit_key(h[r], t + r) : 0u;              // (0 enters no list)
#pragma unroll
                        for (int i = 0; i < KMAX; ++i) {
                            const unsigned hi = key > best[f][i] ? key : best[f][i];
                            key = key > best[f][i] ? best[f][i] : key;
                            best[f][i] = hi;
                        }
                    }
                }
            }
        }
    }
    if constexpr (KMAX == 0) return;
    __syncthreads();                                                                         // every wave is done with the panel
#pragma unroll
    for (int f = 0; f < RF; ++f)
#pragma unroll
        for (int i = 0; i < (KMAX > 0 ? KMAX : 1); ++i) lists[((size_t)threadIdx.x * RF + f) * KMAX + i] = best[f][i];
    __syncthreads();

    // ---- one thread per row merges the 16 lists of its row: 4 lane groups x 4 waves ---------------------------------------------------
    if (threadIdx.x < 16 * RF) {
        const int f = threadIdx.x >> 4, row = threadIdx.x & 15, m = m0 + threadIdx.x;
        if (m < M) {
            unsigned prev = 0xFFFFFFFFu;
            for (int i = 0; i < keff; ++i) {
                unsigned best = 0;
                for (int src = 0; src < 16; ++src) {
                    const unsigned* L = lists + ((size_t)(src * 16 + row) * RF + f) * KMAX;    // thread src * 16 + row: wave src >> 2, lane group src & 3
                    for (int j = 0; j < KMAX; ++j) {
                        const unsigned key = L[j];
                        if (key < prev) { best = key > best ? key : best; break; }
                    }
                }
                const int idx = (int)(0xFFFFu - (best & 0xFFFFu));
                if (i == 0 && argmax) argmax[m] = idx;
                if (i < k) {
                    topk_v[(size_t)m * k + i] = key_value(best);
                    topk_i[(size_t)m * k + i] = idx;
                }
                prev = best;
            }
        }
    }
}

inline int logits_kmax(int keff) { return keff == 0 ? 0 : (keff == 1 ? 1 : (keff <= 8 ? 8 : 16)); }
inline size_t logits_lds(int D, int RF, int kmax) {                                          // the panel, later the lists over it
    const size_t panel = (size_t)16 * RF * (D + PW_PAD) * 2, lists = (size_t)256 * RF * kmax * 4;
    return panel > lists ? panel : lists;
}

}  // namespace

extern "C" int pclip_cosine_logits_f16(const void* a, int lda, int M, const void* b, int ldb, int T, int D, float scale, int flags, void* logits, int ldl,
                                       int32_t* argmax, void* topk_v, int32_t* topk_i, int k, void* ws, size_t ws_bytes, pclip_stream_t stream) {
    const char* fn = "pclip_cosine_logits_f16";
    PCLIP_REQUIRE(a && b, "%s: null operand", fn);
    PCLIP_REQUIRE(M >= 1 && T >= 1, "%s: M=%d and T=%d must be positive", fn, M, T);
    PCLIP_REQUIRE(D > 0 && D % 64 == 0 && D <= 4096, "%s: D=%d must be a multiple of 64, <= 4096", fn, D);
    PCLIP_REQUIRE((flags & ~(PCLIP_LOGITS_NORMALIZE_A | PCLIP_LOGITS_NORMALIZE_B)) == 0, "%s: unknown flag bits 0x%x", fn, flags);
    PCLIP_REQUIRE_PITCH(fn, lda, D);
    PCLIP_REQUIRE_PITCH(fn, ldb, D);
    PCLIP_REQUIRE(k >= 0 && k <= 16 && k <= T, "%s: k=%d must be in [0, min(16, T=%d)]", fn, k, T);
    PCLIP_REQUIRE((k > 0) == (topk_v != nullptr) && (k > 0) == (topk_i != nullptr), "%s: k=%d needs both top-k outputs, k = 0 neither", fn, k);
    PCLIP_REQUIRE(logits || argmax || k > 0, "%s: no output requested", fn);
    PCLIP_REQUIRE(!logits || (ldl >= T && ldl % 8 == 0), "%s: ldl=%d must be >= T=%d and a multiple of 8 halves", fn, ldl, T);
    const bool fused = argmax || k > 0;
    PCLIP_REQUIRE(!fused || T <= 4096, "%s: argmax / top-k need T=%d <= 4096 (the logits alone have no cap)", fn, T);
    PCLIP_REQUIRE_ALIGNED(fn, (uintptr_t)a | (uintptr_t)b | (uintptr_t)logits, 0);
    const half_t* bw = (const half_t*)b;
    int ldbw = ldb;
    hipStream_t s = (hipStream_t)stream;
    if (flags & PCLIP_LOGITS_NORMALIZE_B) {
        const size_t need = pclip_workspace_bytes(PCLIP_OP_LOGITS, M, T, D);
        PCLIP_REQUIRE(ws != nullptr && (uintptr_t)ws % 16 == 0, "%s: PCLIP_LOGITS_NORMALIZE_B needs a 16-byte aligned workspace", fn);
        if (ws_bytes < need) { pclip_set_error("%s: workspace %zu < %zu", fn, ws_bytes, need); return PCLIP_E_WORKSPACE; }
    }

    // rows per panel: as many fragments as M asks for and the LDS holds next to the top-k lists
    const int keff = k > 0 ? k : (argmax ? 1 : 0);
    const int rfmax = D <= 1024 ? 4 : (D <= 2048 ? 2 : 1);    // what the dispatch below instantiates per register chunk count: the grid, the LDS and the launch share it
    int RF = M <= 16 ? 1 : (M <= 32 ? 2 : 4);
    RF = RF > rfmax ? rfmax : RF;
    const int kmax = logits_kmax(keff);
    while (RF > 1 && logits_lds(D, RF, kmax) > (size_t)LG_LDS_MAX) RF >>= 1;
    const size_t lds = logits_lds(D, RF, kmax);
    PCLIP_REQUIRE(lds <= (size_t)LG_LDS_MAX, "%s: D=%d k=%d does not fit the LDS", fn, D, k);
    const int npanels = ceil_div(M, 16 * RF), ncb = ceil_div(T, 64);
    int ysplit = 1;                                       // the logits alone: few panels share the column blocks between workgroups (a row's bits do not depend on it)
    if (!fused) {
        ysplit = ceil_div(2 * pclip_cus(), npanels);
        const int ymax = ceil_div(ncb, 4);
        ysplit = ysplit > ymax ? ymax : ysplit;
        ysplit = ysplit > 65535 ? 65535 : ysplit;
    }

    if (flags & PCLIP_LOGITS_NORMALIZE_B) {
        if (int e = launch_norm_rows<4096>((const half_t*)b, ldb, (half_t*)ws, T, D, s, "cosine_logits (row norms)")) return e;
        bw = (const half_t*)ws;
        ldbw = D;
    }

    const dim3 grid(npanels, ysplit);
#define PCLIP_LG(NCH, RFV, KM)                                                                                                                     \
    do {                                                                                                                                         \
        static DevOnce attr;                                                                                                                     \
        if (int e = pclip_raise_lds(attr, {(const void*)cosine_logits_kernel<NCH, RFV, KM>}, LG_LDS_MAX, fn)) return e;                          \
        cosine_logits_kernel<NCH, RFV, KM><<<grid, 256, lds, s>>>((const half_t*)a, lda, M, bw, ldbw, T, D, scale, (flags & PCLIP_LOGITS_NORMALIZE_A) ? 1 : 0, \
                                                             (half_t*)logits, ldl, argmax, (half_t*)topk_v, topk_i, k, keff);                   \
    } while (0)
#define PCLIP_LG_K(NCH, RFV)                               \
    do {                                                   \
        if (kmax == 0) PCLIP_LG(NCH, RFV, 0);              \
        else if (kmax == 1) PCLIP_LG(NCH, RFV, 1);         \
        else if (kmax == 8) PCLIP_LG(NCH, RFV, 8);         \
        else PCLIP_LG(NCH, RFV, 16);                       \
    } while (0)
    // (RF <= rfmax above: 4 up to D = 1024, 2 up to 2048, 1 beyond — every (NCH, RF) that can arrive here is compiled, and RF matches `grid` and `lds`)
    // not panel_dispatch: no accumulator panel caps RF here (4 up to D = 1024), D goes on to 4096 (NCH = 8), and every form fans out over KMAX instead of an NDF
    if (D <= 512) { if (RF == 4) PCLIP_LG_K(1, 4); else if (RF == 2) PCLIP_LG_K(1, 2); else PCLIP_LG_K(1, 1); }
    else if (D <= 1024) { if (RF == 4) PCLIP_LG_K(2, 4); else if (RF == 2) PCLIP_LG_K(2, 2); else PCLIP_LG_K(2, 1); }
    else if (D <= 2048) { if (RF == 2) PCLIP_LG_K(4, 2); else if (RF == 1) PCLIP_LG_K(4, 1); else { pclip_set_error("%s: no kernel for D=%d with %d row fragments", fn, D, RF); return PCLIP_E_INVALID; } }
    else { if (RF == 1) PCLIP_LG_K(8, 1); else { pclip_set_error("%s: no kernel for D=%d with %d row fragments", fn, D, RF); return PCLIP_E_INVALID; } }
#undef PCLIP_LG_K
#undef PCLIP_LG
    return pclip_check_launch("cosine_logits");
}
