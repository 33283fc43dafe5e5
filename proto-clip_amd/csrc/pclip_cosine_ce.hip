// Cross-entropy over cosine logits and its gradients, for training on the logits of clip/model.py:356-370 (a text-initialised classifier or an adapter under
// `scale * f' @ w'^T`, CLIP's symmetric contrastive loss, the temperature).  Ragged in M and T; the [M, T] matrix never reaches memory, forward or backward.
//   cos[m, t] = fp32 MFMA accumulation of a'[m, :] . b'[t, :],  s = scale * cos in fp32.  Unlike pclip_logits.hip NOTHING is rounded to fp16 on the way to s.
// The panel walk of pclip_panel_walk.h: the forward is built from its staging and its paired form; the backward calls its second product and gradient store and keeps
// its staging, first product and prefetch written out (the note at ce_bwd_kernel says why).
// Forward (ce_fwd_kernel): the walk of cosine_logits_kernel by eight waves — a panel of 16 RF rows of a' in LDS, the rows of b' streamed in the MFMA operand layout, a lane
//   ending with 4 consecutive columns of one row per fragment — with an online (max, sum-exp) per row in place of the top-k lists and the target logit picked
//   out by comparing the label with the column index (a label is never an index: one outside [0, T) matches nothing).  Symmetric mode: the same tile gives a
//   (max, sum-exp) per column over the panel's valid rows (butterfly over the 16 lanes of a row group) into ws [panel][T]; ce_col_combine_kernel merges the
//   panels in index order.  Rows >= M are -inf before any column statistic, columns >= T before any row statistic.  The mean is one fixed-order fp64 sum.
// Backward (ce_bwd_kernel), "own" = the side whose gradient is produced, "walked" = the other (direction 0: own a, walked b; direction 1 exchanged, i.e. G^T):
//   per 64 walked rows, wave w recomputes the 16 RF x 16 fragment of s for walked rows 16 w .. 16 w + 15 (the panel of own rows in LDS as before), forms
//       E = exp(s - lse_own[i]) + exp(s - lse_walked[j])      (whichever of the two the mode has; both in symmetric mode, so E in [0, 2])
//   in registers, rounds 2^14 E to fp16 (unit 2^-11: the one rounding the gradient tolerance of tests/cosine_ce_ref.py is built on) and puts it in LDS [own][walked];
//   after one barrier every wave reads it as the B operand (own row on the lane, 8 walked rows in the registers) and accumulates E . walked'^T into ITS quarter
//   of the D columns of the fp32 panel: RF D / 16 accumulator registers per lane (128 at the largest RF per D).  The A operand of that product needs the walked
//   rows with the walked index along the registers: a first launch writes them transposed, [D][walked rounded up to 64, zero-filled], into ws, so the operand is
//   again one 16-byte load per lane.  The target term is a second, exact tile Y (-kappa at the target, 0 elsewhere) through the same MFMA into the same
//   accumulator, issued only for tiles where some wave saw a target: weight, scale and the -kappa all act in fp32, so 1 / (2 M) never meets fp16.
//   dscale = sum G o cos from the unrounded E: per-lane fp32, per-panel partials, one fixed-order fp64 sum.  The E tile is double-buffered: one barrier per tile.
//   Under NORMALIZE the panel gradient is chained through x / ||x|| by ce_norm_backward_kernel in fp32 (the fp16 rounding of x' taken as the identity).
// Every workgroup walks ALL walked rows in index order and an element has one accumulator: a row's lse, loss term and gradient do not depend on RF, the grid or
// (labelled, direction 0) the other rows; where the own rows are few panels, the walked tiles are shared between workgroups in fixed chunks (ce_chunks).
// Groups (pclip_cosine_ce_grouped_f16 / _backward_f16, labelled mode): G problems of one shape are the GROUPED instantiations of the same kernels with the
// group as a grid dimension — a base offset in front of the same walk, so a group's bits are the single call's — and every helper pass (row norms, transpose,
// chunk sum, norm backward, the means and dscale sums) is issued once for all groups: the launches of a call do not depend on G.
// Only __syncthreads barriers and compiler-counted waits: nothing here for the race-stress build.
#include "pclip_panel_walk.h"

namespace {

constexpr int CE_LDS_MAX = 152 * 1024;           // dynamic LDS asked for: the forward kernel keeps up to 6 KB of static LDS next to it (the most used is 104 KB)
constexpr int CE_DMAX = 2048;
constexpr int CE_FW = 8;                        // waves of a forward workgroup: each walks every eighth block of 64 columns (a constant: a row's merge order never changes)
// E in [0, 2] enters the fp16 tile as 2^14 E (<= 32768, exact scaling, undone in fp32 with the weight): the relative unit 2^-11 then holds down to E = 2^-28
// instead of 2^-14, and E flushes to zero only below 2^-39 — the rows of a class no sample is near are made of such entries
constexpr float CE_ESCALE = 16384.f;

// (max, sum-exp) pairs; (-inf, 0) is the empty one
__device__ __forceinline__ void lse_merge(float& mx, float& sm, float omx, float osm) {
    const float nm = fmaxf(mx, omx);
    if (nm == -INFINITY) return;
    sm = sm * __expf(mx - nm) + osm * __expf(omx - nm);
    mx = nm;
}

__device__ __forceinline__ long long load_label(const void* labels, int i64, int i) {
    return i64 ? (long long)reinterpret_cast<const int64_t*>(labels)[i] : (long long)reinterpret_cast<const int32_t*>(labels)[i];
}

// ce_bwd_kernel's own staging: stage_panel with the wave count read from blockDim, as that kernel has always had it (see the note at the kernel)
template <int NCH>
__device__ __forceinline__ void load_panel(half_t* panel, int LDP, const half_t* __restrict__ x, int ldx, int R, int D, int r0, int rows, int norm) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    for (int r = wave; r < rows; r += nwaves) {
        const int m = r0 + r;
        RowRegs<NCH> rr;
        if (m < R) {                                                                         // (wave-uniform)
            load_row<NCH>(x + (size_t)m * ldx, D, lane, rr);
            if (norm) normalise_row<NCH>(rr);
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

// element i of a label vector of either width
__device__ __forceinline__ const void* labels_at(const void* labels, int i64, size_t i) {
    return i64 ? (const void*)(reinterpret_cast<const int64_t*>(labels) + i) : (const void*)(reinterpret_cast<const int32_t*>(labels) + i);
}

// GROUPED (pclip_cosine_ce_grouped_f16), launched over grid (panels, 1, G): G labelled forward walks of one shape in one launch.
//   What is walked: by workgroup (p, g), panel p of a_g = a + g gsa ([M, D], rows lda apart) against ALL rows of b_g = b + g gsb ([T, D], rows ldb apart),
//   with the labels, lse, target and loss rows of the group at g M.
//   The order: this kernel's own — 64-column blocks dealt to the CE_FW waves, k ascending, a row's lane groups then its waves merged in a fixed order.
//   The rounding points: those of the list at the head of this file, unchanged (cos an fp32 MFMA accumulation, s = scale * cos in fp32, nothing to fp16).
//   blockIdx.z is the GROUP and nothing else: the bases are advanced once, in size_t, before the walk; no value crosses groups, so group g's numbers are
//   the bits of the ungrouped launch on (a_g, b_g) alone.  The ungrouped instantiation reads neither stride (the habit of pclip_rows.h).
template <int NCH, int RF, bool GROUPED = false>
__global__ __launch_bounds__(64 * CE_FW) void ce_fwd_kernel(const half_t* __restrict__ a, int lda, int M, const half_t* __restrict__ b, int ldb, int T, int D, float scale,
                                                     int norm_a, int symmetric, const void* __restrict__ labels, int lab64, float* __restrict__ lse_row,
                                                     float* __restrict__ tgt, float* __restrict__ row_loss, float2* __restrict__ colpart, size_t gsa, size_t gsb) {
    if (GROUPED) {
        const size_t g = blockIdx.z, r0 = g * M;
        a += g * gsa, b += g * gsb;
        labels = labels_at(labels, lab64, r0);
        lse_row += r0, tgt += r0, row_loss += r0;
    }
    extern __shared__ __attribute__((aligned(16))) char ce_smem[];
    __shared__ float red[CE_FW][RF][16][3];
    half_t* panel = reinterpret_cast<half_t*>(ce_smem);                                      // [16 RF][D + 8]
    const int LDP = D + PW_PAD;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m0 = blockIdx.x * 16 * RF;
    stage_panel<NCH, CE_FW>(panel, LDP, a, lda, M, D, m0, 16 * RF, lane, wave, norm_a);

    const int lr = lane & 15, lq = lane >> 4;
    float mx[RF], sm[RF], tg[RF];
    long long want[RF];                                                                      // the target column of this lane's row per fragment, -1: none
#pragma unroll
    for (int f = 0; f < RF; ++f) {
        const int m = m0 + 16 * f + lr;
        mx[f] = -INFINITY, sm[f] = 0.f, tg[f] = 0.f;
        want[f] = m < M ? (symmetric ? (long long)m : load_label(labels, lab64, m)) : -1;
    }
    __syncthreads();

    const int KS = D >> 5, ncb = (T + 63) >> 6;
    for (int cb = wave; cb < ncb; cb += CE_FW) {
        const int t0 = cb * 64;
        const half_t* bp[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) bp[c] = walked_row(b, ldb, t0 + 16 * c + lr, T, lq);
        float4_t acc[RF][4];
        walk_pairs<RF, 4>(bp, panel + (size_t)lr * LDP + lq * 8, LDP, KS, acc);
        // acc[f][c][r] = cos(m0 + 16 f + lr, t0 + 16 c + 4 lq + r)
#pragma unroll
        for (int f = 0; f < RF; ++f)
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[f][c][r] *= scale;
        // ---- rows: online (max, sum-exp) over this lane's valid columns, the target logit ------------------------------------------------
#pragma unroll
        for (int f = 0; f < RF; ++f) {
            float tmax = -INFINITY;
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int t = t0 + 16 * c + 4 * lq + r;
                    if (t < T) {
                        tmax = fmaxf(tmax, acc[f][c][r]);
                        if ((long long)t == want[f]) tg[f] += acc[f][c][r];
                    }
                }
            if (tmax > -INFINITY) {
                const float nm = fmaxf(mx[f], tmax);
                float add = 0.f;
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int t = t0 + 16 * c + 4 * lq + r;
                        add += t < T ? __expf(acc[f][c][r] - nm) : 0.f;
                    }
                sm[f] = sm[f] * __expf(mx[f] - nm) + add;
                mx[f] = nm;
            }
        }
        // ---- columns (symmetric): (max, sum-exp) over the panel's valid rows: the RF fragments in registers, then the 16 lanes of the group ---
        if (symmetric) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float cm[4], ce[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = -INFINITY;
#pragma unroll
                    for (int f = 0; f < RF; ++f) v = m0 + 16 * f + lr < M ? fmaxf(v, acc[f][c][r]) : v;
                    v = fmaxf(v, lane_xor<1>(v));
                    v = fmaxf(v, lane_xor<2>(v));
                    v = fmaxf(v, lane_xor<4>(v));
                    v = fmaxf(v, lane_xor<8>(v));
                    cm[r] = v;                                                               // (finite: row m0 of the panel exists)
                    float e = 0.f;
#pragma unroll
                    for (int f = 0; f < RF; ++f) e += m0 + 16 * f + lr < M ? __expf(acc[f][c][r] - v) : 0.f;
                    e += lane_xor<1>(e);
                    e += lane_xor<2>(e);
                    e += lane_xor<4>(e);
                    e += lane_xor<8>(e);
                    ce[r] = e;
                }
                if (lr == 0) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int t = t0 + 16 * c + 4 * lq + r;
                        if (t < T) colpart[(size_t)blockIdx.x * T + t] = make_float2(cm[r], ce[r]);
                    }
                }
            }
        }
    }
    // ---- a row's 4 lane groups, then its CE_FW waves, in a fixed order ----------------------------------------------------------------------
#pragma unroll
    for (int f = 0; f < RF; ++f) {
        lse_merge(mx[f], sm[f], lane_xor<16>(mx[f]), lane_xor<16>(sm[f]));
        tg[f] += lane_xor<16>(tg[f]);
        lse_merge(mx[f], sm[f], lane_xor<32>(mx[f]), lane_xor<32>(sm[f]));
        tg[f] += lane_xor<32>(tg[f]);
        if (lq == 0) {
            red[wave][f][lr][0] = mx[f];
            red[wave][f][lr][1] = sm[f];
            red[wave][f][lr][2] = tg[f];
        }
    }
    __syncthreads();
    if (threadIdx.x < 16 * RF) {
        const int f = threadIdx.x >> 4, row = threadIdx.x & 15, m = m0 + threadIdx.x;
        if (m < M) {
            float rm = red[0][f][row][0], rs = red[0][f][row][1], rt = red[0][f][row][2];
            for (int w = 1; w < CE_FW; ++w) {
                lse_merge(rm, rs, red[w][f][row][0], red[w][f][row][1]);
                rt += red[w][f][row][2];
            }
            const float lse = rm + logf(rs);
            lse_row[m] = lse;
            tgt[m] = rt;
            if (!symmetric) row_loss[m] = lse - rt;
        }
    }
}

// symmetric mode: a column's per-panel partials in panel order, then row m's and column m's term
__global__ __launch_bounds__(256) void ce_col_combine_kernel(const float2* __restrict__ colpart, int npanels, int T, const float* __restrict__ lse_row,
                                                             const float* __restrict__ tgt, float* __restrict__ lse_col, float* __restrict__ row_loss) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    float mx = -INFINITY, sm = 0.f;
    for (int p = 0; p < npanels; ++p) {
        const float2 v = colpart[(size_t)p * T + t];
        lse_merge(mx, sm, v.x, v.y);
    }
    const float lc = mx + logf(sm);
    lse_col[t] = lc;
    row_loss[t] = 0.5f * ((lse_row[t] - tgt[t]) + (lc - tgt[t]));
}

// out[0] = mul * sum x[0 .. n), one workgroup, fp64, a fixed order.  GROUPED, launched with G workgroups: out[g] = mul * sum x[g n .. g n + n), each in that order
template <bool GROUPED = false>
__global__ __launch_bounds__(256) void ce_sum_kernel(const float* __restrict__ x, int n, double mul, float* __restrict__ out) {
    if (GROUPED) {
        x += (size_t)blockIdx.x * n;
        out += blockIdx.x;
    }
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

// out = sum over the chunks of part [nchunks][n], in chunk order (n % 4 == 0).  GROUPED, grid (flat, G): part [G][nchunks][n] -> out [G][n], group blockIdx.y
template <bool GROUPED = false>
__global__ __launch_bounds__(256) void ce_sum_chunks_kernel(const float* __restrict__ part, int nchunks, size_t n, float* __restrict__ out) {
    if (GROUPED) {
        part += blockIdx.y * (nchunks * n);
        out += blockIdx.y * n;
    }
    for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += (size_t)gridDim.x * 256 * 4) {
        float4_t s = *reinterpret_cast<const float4_t*>(part + i);
        for (int c = 1; c < nchunks; ++c) s += *reinterpret_cast<const float4_t*>(part + (size_t)c * n + i);
        *reinterpret_cast<float4_t*>(out + i) = s;
    }
}

// NDF: the 16-column fragments of one wave's quarter of D the kernel is compiled for (D / 64 <= NDF of them are live)
// Of the shared skeleton of pclip_panel_walk.h this kernel calls bwd_second_product and store_grad_panel.  Its staging, its first product and its wt0 prefetch are
// written out (the text of bwd_first_product / bwd_prefetch_t): each of them behind the shared function re-rolled the register allocation of the RF = 4 form and
// cost 0.5 - 0.9 % at 32768^2 (profiles/panel_walk_refactor.txt, section 5).  A change to the backward walk is made here and in the header.
//
// GROUPED (pclip_cosine_ce_grouped_backward_f16), launched over grid (panels, chunks, G): G labelled backward walks of one shape in one launch.
//   What is walked: by workgroup (p, c, g), panel p of the own rows of group g against chunk c of THAT group's walked tiles — ce_chunks is a function of
//   (Ro, Rw, D) and so the same for every group — into the group's own gradient panel (or chunk partial) and dscale partial.
//   The order: this kernel's own (walked tiles ascending within a chunk, k ascending, one accumulator per element).
//   The rounding points: those of the list at the head of this file, unchanged (2^14 E to fp16 once; weight, scale and the target term in fp32).
//   blockIdx.z is the GROUP and nothing else: every base is advanced once by g times its stride (CeBwdStrides, size_t) before the walk; nothing is added
//   across groups, so group g's numbers are the bits of the ungrouped launch on that group alone.  The ungrouped instantiation does not read the strides.
struct CeBwdStrides {             // from group g to group g + 1, in elements
    size_t own, walk, walkT;      // halves: the operands as the kernel reads them (the walked one possibly its normalised copy) and the walked transposes
    size_t rows;                  // = M: the labels and the row lse belong to the a side, whichever side is own
    size_t gout, dsc;             // floats: the gradient panels (chunks x Ro x D where the walk is chunked, Ro x D otherwise), the dscale partials
};
template <int NCH, int RF, int NDF, bool GROUPED = false>
__global__ __launch_bounds__(256) void ce_bwd_kernel(const half_t* __restrict__ own, int ldo, int Ro, const half_t* __restrict__ walk, int ldw, int Rw,
                                                     const half_t* __restrict__ walkT, int ldt, int D, float scale, float weight, int norm_own, int symmetric,
                                                     const void* __restrict__ lab_own, const void* __restrict__ lab_walk, int lab64,
                                                     const float* __restrict__ lse_own, const float* __restrict__ lse_walk, float* __restrict__ gout,
                                                     float* __restrict__ dsc_part, CeBwdStrides gs) {
    if (GROUPED) {
        const size_t g = blockIdx.z, r0 = g * gs.rows;
        own += g * gs.own, walk += g * gs.walk, walkT += g * gs.walkT, gout += g * gs.gout;
        if (lab_own) lab_own = labels_at(lab_own, lab64, r0);
        if (lab_walk) lab_walk = labels_at(lab_walk, lab64, r0);
        if (lse_own) lse_own += r0;
        if (lse_walk) lse_walk += r0;
        if (dsc_part) dsc_part += g * gs.dsc;
    }
    extern __shared__ __attribute__((aligned(16))) char ce_smem[];
    const int LDP = D + PW_PAD;
    half_t* panel = reinterpret_cast<half_t*>(ce_smem);                                      // [16 RF][D + 8]
    half_t* etile = panel + (size_t)16 * RF * LDP;                                           // [2][16 RF][PW_PLD]: r16(E), own row x walked row
    half_t* ytile = etile + (size_t)2 * 16 * RF * PW_PLD;                                    // [2][16 RF][PW_PLD]: -kappa at the targets
    int* hitflag = reinterpret_cast<int*>(ytile + (size_t)2 * 16 * RF * PW_PLD);             // [2][4]: wave w saw a target in its fragment of the tile
    float* dsc_red = reinterpret_cast<float*>(hitflag + 8);                                  // [4]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i0 = blockIdx.x * 16 * RF;
    load_panel<NCH>(panel, LDP, own, ldo, Ro, D, i0, 16 * RF, norm_own);

    const int lr = lane & 15, lq = lane >> 4;
    const int ndf = D >> 6, dbase = wave * (D >> 2);
    const float kappa = symmetric ? 2.f : 1.f;
    float lo[RF];
    long long want[RF];                                                                      // direction 0: the walked index that is own row i's target (-1: none)
#pragma unroll
    for (int f = 0; f < RF; ++f) {
        const int i = i0 + 16 * f + lr;
        lo[f] = (lse_own && i < Ro) ? lse_own[i] : 0.f;
        want[f] = -1;
        if (i < Ro) want[f] = symmetric ? (long long)i : (lab_own ? load_label(lab_own, lab64, i) : -1);
    }
    float4_t acc2[RF][NDF];
#pragma unroll
    for (int f = 0; f < RF; ++f)
#pragma unroll
        for (int df = 0; df < NDF; ++df) acc2[f][df] = float4_t{0.f, 0.f, 0.f, 0.f};
    float dsc = 0.f;
    __syncthreads();

    // blockIdx.y: this workgroup's chunk of the walked tiles (gridDim.y > 1: gout is that chunk's partial panel, summed in chunk order by ce_sum_chunks_kernel)
    const int KS = D >> 5, ntiles = (Rw + 63) >> 6, tpc = (ntiles + gridDim.y - 1) / gridDim.y;
    const int tile_end = (int)(blockIdx.y + 1) * tpc < ntiles ? (int)(blockIdx.y + 1) * tpc : ntiles;
    gout += (size_t)blockIdx.y * Ro * D;
    const half_t* wp;                                                                        // this wave's walked row of the tile at hand (clamped), and its first two k-steps
    {
        int jr = (int)blockIdx.y * tpc * 64 + 16 * wave + lr;
        jr = jr < Rw ? jr : Rw - 1;
        wp = walk + (size_t)jr * ldw + lq * 8;
    }
    half8_t c0 = ld_half8(wp), c1 = ld_half8(wp + 32);
    for (int tile = blockIdx.y * tpc; tile < tile_end; ++tile) {
        const int j0 = tile * 64, buf = tile & 1;
        // ---- this wave's fragment of cos: walked rows j0 + 16 wave .. + 15 against the whole panel -------------------------------------
        // k-steps in pairs (KS is even); the pair after the one in the MFMAs is in flight, the first pair of the NEXT tile under the last of this one
        int jn = j0 + 64 + 16 * wave + lr;
        jn = jn < Rw ? jn : Rw - 1;
        const half_t* wpn = walk + (size_t)jn * ldw + lq * 8;
        const half_t* ap = panel + (size_t)lr * LDP + lq * 8;
        float4_t acc[RF];
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
        wp = wpn;
        // the first eight column fragments of the second product's walked operand: in flight under the exponentials and the barrier
        half8_t wt0[8];
#pragma unroll
        for (int u = 0; u < 8; ++u)
            wt0[u] = u < ndf ? ld_half8(walkT + (size_t)(dbase + 16 * u + lr) * ldt + j0 + 8 * lq) : half8_t{};
        // acc[f][r] = cos(own i0 + 16 f + lr, walked j0 + 16 wave + 4 lq + r)
        const int jb = j0 + 16 * wave + 4 * lq;
        float lw[4];
        long long wl[4];                                                                     // direction 1, labelled: the own index that is walked row j's target
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool ok = jb + r < Rw;
            lw[r] = (lse_walk && ok) ? lse_walk[jb + r] : 0.f;
            wl[r] = (lab_walk && ok) ? load_label(lab_walk, lab64, jb + r) : -1;
        }
        bool anyhit = false;
#pragma unroll
        for (int f = 0; f < RF; ++f) {
            const int i = i0 + 16 * f + lr;
            half4_t e16, y16;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float cosv = acc[f][r], s = scale * cosv;
                const bool ok = i < Ro && jb + r < Rw;
                float e = 0.f;
                if (lse_own) e += __expf(s - lo[f]);
                if (lse_walk) e += __expf(s - lw[r]);
                e = ok ? e : 0.f;
                const bool hit = ok && ((long long)(jb + r) == want[f] || wl[r] == (long long)i);
                anyhit = anyhit || hit;
                dsc += (e - (hit ? kappa : 0.f)) * cosv;
                e16[r] = (half_t)(e * CE_ESCALE);
                y16[r] = hit ? (half_t)(-kappa * CE_ESCALE) : (half_t)0.f;
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
    // acc2[f][df][r] = 2^14 sum_j (E - kappa Y)[i0 + 16 f + lr, j] walked'[j, dbase + 16 df + 4 lq + r]
    store_grad_panel<RF, NDF>(gout, i0, Ro, D, dbase, ndf, weight * scale * (1.f / CE_ESCALE), lr, lq, acc2);
    if (dsc_part) {
        dsc = wave_sum(dsc);
        if (lane == 0) dsc_red[wave] = dsc;
        __syncthreads();
        if (threadIdx.x == 0) dsc_part[blockIdx.y * gridDim.x + blockIdx.x] = weight * (((dsc_red[0] + dsc_red[1]) + dsc_red[2]) + dsc_red[3]);
    }
}

// g <- (g - y (y . g)) / ||x||, y = x / ||x|| in fp32: the gradient of x -> x / ||x|| applied to a row of dL/dx' in place (one wave per row)
// GROUPED, launched with gridDim.y = G: the rows of G operands of R rows each, group blockIdx.y's x at x + blockIdx.y gsx, its gradient the dense [R, D] block of g
template <int NCH, bool GROUPED = false>
__global__ __launch_bounds__(256) void ce_norm_backward_kernel(const half_t* __restrict__ x, int ldx, float* __restrict__ g, int R, int D, size_t gsx) {
    if (GROUPED) {
        x += blockIdx.y * gsx;
        g += blockIdx.y * ((size_t)R * D);
    }
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

inline int ce_rf_fwd(int M, int D) {                  // the forward has no other source of workgroups than its panels: smaller ones until there are 256 (a row's bits do not depend on RF)
    int rf = rf_for(M, D);
    while (rf > 1 && ceil_div(M, 16 * rf) < 256) rf >>= 1;
    return rf;
}

struct CeFwdWs {
    size_t bn, colpart, tgt, bytes;
};
inline CeFwdWs ce_fwd_ws(int M, int T, int D) {
    CeFwdWs w;
    size_t off = 0;
    w.bn = off, off += align_up((size_t)T * D * 2, 256);
    const int npanels = ceil_div(M, 16 * ce_rf_fwd(M, D));
    w.colpart = off, off += M == T ? align_up((size_t)npanels * T * sizeof(float2), 256) : 0;   // (symmetric mode needs M == T)
    w.tgt = off, off += align_up((size_t)M * 4, 256);
    w.bytes = off;
    return w;
}
// Few own rows are few panels (dL/db of a 1000-class probe over 50 000 samples: 16): the walked tiles are then shared between up to CE_WG_TARGET / panels
// workgroups, each with a partial fp32 panel in ws, summed in chunk order.  A function of the shape alone, never of the device; the partials stay within
// 4 (M + T) D floats.  Not in labelled mode for dL/da: its rows keep their bits whatever the batch (one accumulator over ALL classes, in order).
constexpr int CE_WG_TARGET = 512;
inline int ce_chunks(int Ro, int Rw, int D, bool split_allowed) {
    if (!split_allowed) return 1;
    const int npanels = ceil_div(Ro, 16 * rf_for(Ro, D)), ntiles = ceil_div(Rw, 64);
    int n = ceil_div(CE_WG_TARGET, npanels);
    const int cap = (int)(4 * ((size_t)Ro + Rw) / Ro);
    n = n > cap ? cap : n;
    n = n > ntiles ? ntiles : n;
    n = n > 65535 ? 65535 : n;
    return n < 1 ? 1 : n;
}
struct CeBwdWs {
    size_t wn, wt, dsc, part, bytes;
};
inline CeBwdWs ce_bwd_ws(int M, int T, int D) {        // either direction fits: sized by the larger side
    const int R = M > T ? M : T;
    const int ca = ce_chunks(M, T, D, true), cb = ce_chunks(T, M, D, true);
    const size_t pa = ca > 1 ? (size_t)ca * M : 0, pb = cb > 1 ? (size_t)cb * T : 0;
    const size_t da = (size_t)ca * ceil_div(M, 16), db = (size_t)cb * ceil_div(T, 16);
    CeBwdWs w;
    size_t off = 0;
    w.wn = off, off += align_up((size_t)R * D * 2, 256);
    w.wt = off, off += align_up((size_t)D * round64(R) * 2, 256);
    w.dsc = off, off += align_up((da > db ? da : db) * 4, 256);
    w.part = off, off += align_up((pa > pb ? pa : pb) * D * 4, 256);
    w.bytes = off;
    return w;
}

int ce_validate(const char* fn, const void* a, int lda, int M, const void* b, int ldb, int T, int D, int flags, const void* labels, const void* ws,
                size_t ws_bytes, size_t need) {
    PCLIP_REQUIRE(a && b, "%s: null operand", fn);
    PCLIP_REQUIRE(M >= 1 && T >= 1, "%s: M=%d and T=%d must be positive", fn, M, T);
    PCLIP_REQUIRE(D > 0 && D % 64 == 0, "%s: D=%d must be a multiple of 64", fn, D);
    PCLIP_REQUIRE(D <= CE_DMAX, "%s: D=%d is past the envelope (D <= %d)", fn, D, CE_DMAX);
    PCLIP_REQUIRE((flags & ~(PCLIP_CE_NORMALIZE_A | PCLIP_CE_NORMALIZE_B | PCLIP_CE_SYMMETRIC | PCLIP_CE_LABELS_I64)) == 0, "%s: unknown flag bits 0x%x", fn, flags);
    if (flags & PCLIP_CE_SYMMETRIC) {
        PCLIP_REQUIRE(M == T, "%s: symmetric mode needs M == T (M=%d, T=%d)", fn, M, T);
        PCLIP_REQUIRE(!labels, "%s: symmetric mode takes no labels (the targets are the diagonal)", fn);
    } else {
        PCLIP_REQUIRE(labels, "%s: labelled mode needs labels", fn);
        PCLIP_REQUIRE((uintptr_t)labels % ((flags & PCLIP_CE_LABELS_I64) ? 8 : 4) == 0, "%s: misaligned labels", fn);
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

size_t pclip_cosine_ce_workspace(int backward, int M, int T, int D) {
    if (M < 1 || T < 1 || D < 1) return 0;
    return backward ? ce_bwd_ws(M, T, D).bytes : ce_fwd_ws(M, T, D).bytes;
}

extern "C" int pclip_cosine_ce_f16(const void* a, int lda, int M, const void* b, int ldb, int T, int D, float scale, int flags, const void* labels,
                                   float* lse_row, float* lse_col, float* row_loss, float* loss, void* ws, size_t ws_bytes, pclip_stream_t stream) {
    const char* fn = "pclip_cosine_ce_f16";
    if (int e = ce_validate(fn, a, lda, M, b, ldb, T, D, flags, labels, ws, ws_bytes, pclip_cosine_ce_workspace(0, M, T, D))) return e;
    const int symmetric = (flags & PCLIP_CE_SYMMETRIC) ? 1 : 0;
    PCLIP_REQUIRE(lse_row && row_loss && loss, "%s: lse_row, row_loss and loss are required", fn);
    PCLIP_REQUIRE(symmetric ? lse_col != nullptr : lse_col == nullptr, "%s: lse_col goes with symmetric mode, and only with it", fn);
    hipStream_t s = (hipStream_t)stream;
    const CeFwdWs w = ce_fwd_ws(M, T, D);
    char* wsb = (char*)ws;
    const half_t* bw = (const half_t*)b;
    int ldbw = ldb;
    if (flags & PCLIP_CE_NORMALIZE_B) {
        if (int e = launch_norm_rows<CE_DMAX>((const half_t*)b, ldb, (half_t*)(wsb + w.bn), T, D, s, "cosine_ce (row norms)")) return e;
        bw = (const half_t*)(wsb + w.bn);
        ldbw = D;
    }
    const int RF = ce_rf_fwd(M, D), npanels = ceil_div(M, 16 * RF);
    const size_t lds = (size_t)16 * RF * (D + PW_PAD) * 2;
    float* tgt = (float*)(wsb + w.tgt);
    float2* colpart = (float2*)(wsb + w.colpart);
    if (int e = panel_dispatch(D, RF, [&](auto nch, auto rf, auto) -> int {
            static DevOnce attr;
            if (int e = pclip_raise_lds(attr, {(const void*)ce_fwd_kernel<nch, rf>}, CE_LDS_MAX, fn)) return e;
            ce_fwd_kernel<nch, rf><<<npanels, 64 * CE_FW, lds, s>>>((const half_t*)a, lda, M, bw, ldbw, T, D, scale, (flags & PCLIP_CE_NORMALIZE_A) ? 1 : 0, symmetric, labels,
                                                                   (flags & PCLIP_CE_LABELS_I64) ? 1 : 0, lse_row, tgt, row_loss, colpart, 0, 0);
            return pclip_check_launch("cosine_ce");
        }))
        return e;
    if (symmetric) {
        ce_col_combine_kernel<<<ceil_div(T, 256), 256, 0, s>>>(colpart, npanels, T, lse_row, tgt, lse_col, row_loss);
        if (int e = pclip_check_launch("cosine_ce (columns)")) return e;
    }
    ce_sum_kernel<><<<1, 256, 0, s>>>(row_loss, M, 1.0 / M, loss);
    return pclip_check_launch("cosine_ce (mean)");
}

extern "C" int pclip_cosine_ce_backward_f16(const void* a, int lda, int M, const void* b, int ldb, int T, int D, float scale, int flags, const void* labels,
                                            const float* lse_row, const float* lse_col, float weight, int direction, float* grad, float* dscale,
                                            void* ws, size_t ws_bytes, pclip_stream_t stream) {
    const char* fn = "pclip_cosine_ce_backward_f16";
    if (int e = ce_validate(fn, a, lda, M, b, ldb, T, D, flags, labels, ws, ws_bytes, pclip_cosine_ce_workspace(1, M, T, D))) return e;
    const int symmetric = (flags & PCLIP_CE_SYMMETRIC) ? 1 : 0;
    PCLIP_REQUIRE(direction == 0 || direction == 1, "%s: direction=%d must be 0 (dL/da) or 1 (dL/db)", fn, direction);
    PCLIP_REQUIRE(lse_row && grad, "%s: lse_row and grad are required", fn);
    PCLIP_REQUIRE(symmetric ? lse_col != nullptr : lse_col == nullptr, "%s: lse_col goes with symmetric mode, and only with it", fn);
    PCLIP_REQUIRE((uintptr_t)grad % 16 == 0, "%s: grad must be 16-byte aligned", fn);
    hipStream_t s = (hipStream_t)stream;
    const CeBwdWs w = ce_bwd_ws(M, T, D);
    char* wsb = (char*)ws;
    // own = the side whose gradient this call produces, walked = the other
    const half_t* own = (const half_t*)(direction ? b : a);
    const half_t* walk = (const half_t*)(direction ? a : b);
    const int ldo = direction ? ldb : lda, Ro = direction ? T : M, Rw = direction ? M : T;
    int ldw = direction ? lda : ldb;
    const int norm_own = (flags & (direction ? PCLIP_CE_NORMALIZE_B : PCLIP_CE_NORMALIZE_A)) ? 1 : 0;
    const int norm_walk = (flags & (direction ? PCLIP_CE_NORMALIZE_A : PCLIP_CE_NORMALIZE_B)) ? 1 : 0;
    const float* lse_own = direction ? lse_col : lse_row;       // (labelled: the row lse is on the a side only)
    const float* lse_walk = direction ? lse_row : lse_col;
    const void* lab_own = (!symmetric && direction == 0) ? labels : nullptr;
    const void* lab_walk = (!symmetric && direction == 1) ? labels : nullptr;
    if (norm_walk) {
        if (int e = launch_norm_rows<CE_DMAX>(walk, ldw, (half_t*)(wsb + w.wn), Rw, D, s, "cosine_ce (row norms)")) return e;
        walk = (const half_t*)(wsb + w.wn);
        ldw = D;
    }
    half_t* walkT = (half_t*)(wsb + w.wt);
    const int ldt = round64(Rw);
    if (int e = launch_transpose(walk, ldw, Rw, D, walkT, ldt, s, "cosine_ce_backward (transpose)")) return e;

    const int RF = rf_for(Ro, D), npanels = ceil_div(Ro, 16 * RF);
    const int nchunks = ce_chunks(Ro, Rw, D, symmetric || direction == 1);
    float* gpanel = nchunks > 1 ? (float*)(wsb + w.part) : grad;
    const dim3 grid(npanels, nchunks);
    const size_t lds = (size_t)16 * RF * (D + PW_PAD) * 2 + (size_t)4 * 16 * RF * PW_PLD * 2 + 8 * sizeof(int) + 4 * sizeof(float);
    float* dsc_part = dscale ? (float*)(wsb + w.dsc) : nullptr;
    if (int e = panel_dispatch(D, RF, [&](auto nch, auto rf, auto ndf) -> int {
            static DevOnce attr;
            if (int e = pclip_raise_lds(attr, {(const void*)ce_bwd_kernel<nch, rf, ndf>}, CE_LDS_MAX, fn)) return e;
            ce_bwd_kernel<nch, rf, ndf><<<grid, 256, lds, s>>>(own, ldo, Ro, walk, ldw, Rw, walkT, ldt, D, scale, weight, norm_own, symmetric, lab_own, lab_walk,
                                                              (flags & PCLIP_CE_LABELS_I64) ? 1 : 0, lse_own, lse_walk, gpanel, dsc_part, CeBwdStrides{});
            return pclip_check_launch("cosine_ce_backward");
        }))
        return e;
    if (nchunks > 1) {
        const size_t n = (size_t)Ro * D;
        size_t g = (n / 4 + 255) / 256;
        g = g > 4096 ? 4096 : g;
        ce_sum_chunks_kernel<><<<(int)g, 256, 0, s>>>(gpanel, nchunks, n, grad);
        if (int e = pclip_check_launch("cosine_ce_backward (chunks)")) return e;
    }
    if (norm_own) {
        int g = ceil_div(Ro, 4);
        g = g > 8192 ? 8192 : g;
        if (D <= 512) ce_norm_backward_kernel<1><<<g, 256, 0, s>>>(own, ldo, grad, Ro, D, 0);
        else if (D <= 1024) ce_norm_backward_kernel<2><<<g, 256, 0, s>>>(own, ldo, grad, Ro, D, 0);
        else ce_norm_backward_kernel<4><<<g, 256, 0, s>>>(own, ldo, grad, Ro, D, 0);
        if (int e = pclip_check_launch("cosine_ce_backward (row norms)")) return e;
    }
    if (dscale) {
        ce_sum_kernel<><<<1, 256, 0, s>>>(dsc_part, npanels * nchunks, 1.0, dscale);
        if (int e = pclip_check_launch("cosine_ce_backward (dscale)")) return e;
    }
    return PCLIP_OK;
}

// ---- G independent labelled problems of one shape in one call: group g is (a + g gsa [M, D], b + g gsb [T, D], labels + g M) ----------------------------
// Every launch below covers all groups (the group is a grid dimension of each), so a call issues the launches of ONE plain call whatever G.  The workspace is the plain call's G times over, region by region: each region holds its G per-group pieces densely, one behind the other.

extern "C" size_t pclip_cosine_ce_grouped_workspace(int backward, int G, int M, int T, int D) {
    if (G < 1) return 0;
    return (size_t)G * pclip_cosine_ce_workspace(backward, M, T, D);
}

namespace {
int ce_grouped_validate(const char* fn, const void* a, int lda, size_t gsa, int M, const void* b, int ldb, size_t gsb, int T, int D, int G, int flags,
                        const void* labels, const void* ws, size_t ws_bytes, int backward) {
    PCLIP_REQUIRE(G >= 1 && G <= 65535, "%s: G=%d must be in 1 .. 65535 (the groups are the grid's z dimension)", fn, G);
    PCLIP_REQUIRE(!(flags & PCLIP_CE_SYMMETRIC), "%s: PCLIP_CE_SYMMETRIC is not supported in groups (labelled mode only)", fn);
    PCLIP_REQUIRE(gsa % 8 == 0 && gsb % 8 == 0, "%s: the group strides gsa=%zu and gsb=%zu must be multiples of 8 halves", fn, gsa, gsb);
    return ce_validate(fn, a, lda, M, b, ldb, T, D, flags, labels, ws, ws_bytes, pclip_cosine_ce_grouped_workspace(backward, G, M, T, D));
}
}  // namespace

extern "C" int pclip_cosine_ce_grouped_f16(const void* a, int lda, size_t gsa, int M, const void* b, int ldb, size_t gsb, int T, int D, int G, float scale,
                                           int flags, const void* labels, float* lse_row, float* row_loss, float* loss, void* ws, size_t ws_bytes,
                                           pclip_stream_t stream) {
    const char* fn = "pclip_cosine_ce_grouped_f16";
    if (int e = ce_grouped_validate(fn, a, lda, gsa, M, b, ldb, gsb, T, D, G, flags, labels, ws, ws_bytes, 0)) return e;
    PCLIP_REQUIRE(lse_row && row_loss && loss, "%s: lse_row, row_loss and loss are required", fn);
    hipStream_t s = (hipStream_t)stream;
    const CeFwdWs w = ce_fwd_ws(M, T, D);
    char* wsb = (char*)ws;
    const half_t* bw = (const half_t*)b;
    int ldbw = ldb;
    size_t gsbw = gsb;
    if (flags & PCLIP_CE_NORMALIZE_B) {
        half_t* bn = (half_t*)(wsb + (size_t)G * w.bn);
        if (int e = launch_norm_rows_grouped<CE_DMAX>((const half_t*)b, ldb, gsb, bn, T, D, G, s, "cosine_ce_grouped (row norms)")) return e;
        bw = bn, ldbw = D, gsbw = (size_t)T * D;
    }
    const int RF = ce_rf_fwd(M, D), npanels = ceil_div(M, 16 * RF);
    const size_t lds = (size_t)16 * RF * (D + PW_PAD) * 2;
    float* tgt = (float*)(wsb + (size_t)G * w.tgt);
    if (int e = panel_dispatch(D, RF, [&](auto nch, auto rf, auto) -> int {
            static DevOnce attr;
            if (int e = pclip_raise_lds(attr, {(const void*)ce_fwd_kernel<nch, rf, true>}, CE_LDS_MAX, fn)) return e;
            ce_fwd_kernel<nch, rf, true><<<dim3(npanels, 1, G), 64 * CE_FW, lds, s>>>((const half_t*)a, lda, M, bw, ldbw, T, D, scale,
                                                                                      (flags & PCLIP_CE_NORMALIZE_A) ? 1 : 0, 0, labels,
                                                                                      (flags & PCLIP_CE_LABELS_I64) ? 1 : 0, lse_row, tgt, row_loss, nullptr, gsa, gsbw);
            return pclip_check_launch("cosine_ce_grouped");
        }))
        return e;
    ce_sum_kernel<true><<<G, 256, 0, s>>>(row_loss, M, 1.0 / M, loss);
    return pclip_check_launch("cosine_ce_grouped (means)");
}

extern "C" int pclip_cosine_ce_grouped_backward_f16(const void* a, int lda, size_t gsa, int M, const void* b, int ldb, size_t gsb, int T, int D, int G,
                                                    float scale, int flags, const void* labels, const float* lse_row, float weight, int direction, float* grad,
                                                    float* dscale, void* ws, size_t ws_bytes, pclip_stream_t stream) {
    const char* fn = "pclip_cosine_ce_grouped_backward_f16";
    if (int e = ce_grouped_validate(fn, a, lda, gsa, M, b, ldb, gsb, T, D, G, flags, labels, ws, ws_bytes, 1)) return e;
    PCLIP_REQUIRE(direction == 0 || direction == 1, "%s: direction=%d must be 0 (dL/da) or 1 (dL/db)", fn, direction);
    PCLIP_REQUIRE(lse_row && grad, "%s: lse_row and grad are required", fn);
    PCLIP_REQUIRE((uintptr_t)grad % 16 == 0, "%s: grad must be 16-byte aligned", fn);
    hipStream_t s = (hipStream_t)stream;
    const CeBwdWs w = ce_bwd_ws(M, T, D);
    char* wsb = (char*)ws;
    // own = the side whose gradient this call produces, walked = the other (as in pclip_cosine_ce_backward_f16, labelled)
    const half_t* own = (const half_t*)(direction ? b : a);
    const half_t* walk = (const half_t*)(direction ? a : b);
    const int ldo = direction ? ldb : lda, Ro = direction ? T : M, Rw = direction ? M : T;
    int ldw = direction ? lda : ldb;
    const size_t gso = direction ? gsb : gsa;
    size_t gsw = direction ? gsa : gsb;
    const int norm_own = (flags & (direction ? PCLIP_CE_NORMALIZE_B : PCLIP_CE_NORMALIZE_A)) ? 1 : 0;
    const int norm_walk = (flags & (direction ? PCLIP_CE_NORMALIZE_A : PCLIP_CE_NORMALIZE_B)) ? 1 : 0;
    const float* lse_own = direction ? nullptr : lse_row;
    const float* lse_walk = direction ? lse_row : nullptr;
    const void* lab_own = direction == 0 ? labels : nullptr;
    const void* lab_walk = direction == 1 ? labels : nullptr;
    if (norm_walk) {
        half_t* wn = (half_t*)(wsb + (size_t)G * w.wn);
        if (int e = launch_norm_rows_grouped<CE_DMAX>(walk, ldw, gsw, wn, Rw, D, G, s, "cosine_ce_grouped (row norms)")) return e;
        walk = wn, ldw = D, gsw = (size_t)Rw * D;
    }
    half_t* walkT = (half_t*)(wsb + (size_t)G * w.wt);
    const int ldt = round64(Rw);
    if (int e = launch_transpose_grouped(walk, ldw, gsw, Rw, D, G, walkT, ldt, s, "cosine_ce_grouped_backward (transpose)")) return e;

    const int RF = rf_for(Ro, D), npanels = ceil_div(Ro, 16 * RF);
    const int nchunks = ce_chunks(Ro, Rw, D, direction == 1);
    const size_t n = (size_t)Ro * D;
    float* gpanel = nchunks > 1 ? (float*)(wsb + (size_t)G * w.part) : grad;
    const size_t lds = (size_t)16 * RF * (D + PW_PAD) * 2 + (size_t)4 * 16 * RF * PW_PLD * 2 + 8 * sizeof(int) + 4 * sizeof(float);
    float* dsc_part = dscale ? (float*)(wsb + (size_t)G * w.dsc) : nullptr;
    const CeBwdStrides gs = {gso, gsw, (size_t)D * ldt, (size_t)M, (size_t)nchunks * n, (size_t)npanels * nchunks};
    if (int e = panel_dispatch(D, RF, [&](auto nch, auto rf, auto ndf) -> int {
            static DevOnce attr;
            if (int e = pclip_raise_lds(attr, {(const void*)ce_bwd_kernel<nch, rf, ndf, true>}, CE_LDS_MAX, fn)) return e;
            ce_bwd_kernel<nch, rf, ndf, true><<<dim3(npanels, nchunks, G), 256, lds, s>>>(own, ldo, Ro, walk, ldw, Rw, walkT, ldt, D, scale, weight, norm_own, 0, lab_own,
                                                                                          lab_walk, (flags & PCLIP_CE_LABELS_I64) ? 1 : 0, lse_own, lse_walk, gpanel,
                                                                                          dsc_part, gs);
            return pclip_check_launch("cosine_ce_grouped_backward");
        }))
        return e;
    if (nchunks > 1) {
        size_t g = (n / 4 + 255) / 256;
        g = g > 4096 ? 4096 : g;
        ce_sum_chunks_kernel<true><<<dim3((int)g, G), 256, 0, s>>>(gpanel, nchunks, n, grad);
        if (int e = pclip_check_launch("cosine_ce_grouped_backward (chunks)")) return e;
    }
    if (norm_own) {
        int g = ceil_div(Ro, 4);
        g = g > 8192 ? 8192 : g;
        if (D <= 512) ce_norm_backward_kernel<1, true><<<dim3(g, G), 256, 0, s>>>(own, ldo, grad, Ro, D, gso);
        else if (D <= 1024) ce_norm_backward_kernel<2, true><<<dim3(g, G), 256, 0, s>>>(own, ldo, grad, Ro, D, gso);
        else ce_norm_backward_kernel<4, true><<<dim3(g, G), 256, 0, s>>>(own, ldo, grad, Ro, D, gso);
        if (int e = pclip_check_launch("cosine_ce_grouped_backward (row norms)")) return e;
    }
    if (dscale) {
        ce_sum_kernel<true><<<G, 256, 0, s>>>(dsc_part, npanels * nchunks, 1.0, dscale);
        if (int e = pclip_check_launch("cosine_ce_grouped_backward (dscale)")) return e;
    }
    return PCLIP_OK;
}
