// Backward of the two embedding stages in front of block 0 (whole-tower fine-tuning): the text embedding x = token_embedding[text] + positional_embedding
// (clip/model.py:342-344) and the token assembly of the vision stem x = [class_embedding ; patches] + positional_embedding (clip/model.py:222-227, in front of
// ln_pre).  Memory-bound gathers and column sums.  No atomics: every sum has one fixed order, so two calls give the same bits.
//
// ROUNDING POINTS
//   * Every input element is an fp16 value, widened exactly to fp32.  Every `+` below is one rounded fp32 addition; every sum starts from +0.
//   * dpos[l][d] = (..((0 + dx[0, l, d]) + dx[1, l, d]) + ..) + dx[B - 1, l, d]: the sequences in ascending order, ONE accumulator (both entry points).
//   * dE (text): the flat ids are sorted stably by the caller (sorted_ids ascending, order[r] = the row of dx that sorted position r came from; equal ids keep
//     their row order).  The sorted positions are cut into chunks of PCLIP_EMBED_BWD_CHUNK = R consecutive positions.  Inside a chunk the rows of a run of equal ids
//     are added in ascending sorted position into one accumulator.  A run that lies inside one chunk IS the row of dE.  A run that crosses a chunk boundary leaves
//     one partial per chunk it touches, and dE[id] = (..(part[c0] + part[c0 + 1]) + ..) + part[c1], the chunks in ascending order, starting from part[c0] itself.
//   * dE rows whose id does not occur are +0 (a memset, not a sum).
//   * dpatch (vision) is a copy: the bits of dt[b, 1 + g, :].
//   * Nothing is rounded to fp16 here: a parameter held in fp16 gets its one rounding from the caller (pclip_cast_f32_f16).
#include "pclip_common.h"

namespace {
constexpr int R = PCLIP_EMBED_BWD_CHUNK;

// One thread per pair of adjacent columns; blockIdx.y walks column groups of 512 (W <= 2048: at most 4).
__device__ __forceinline__ int column_pair(int W) {
    const int col = ((int)blockIdx.y * 256 + (int)threadIdx.x) * 2;
    return col < W ? col : -1;
}

__device__ __forceinline__ void store2(float* p, float a, float b) { *reinterpret_cast<float2*>(p) = make_float2(a, b); }

// ---- positional sums (+ the patch rows of the vision stem) ----------------------------------------------------------------------------------------
// grid.x = L.  dpos[l] = sum_b dx[b, l] in ascending b; COPY: dpatch[b * (L - 1) + l - 1] = dx[b, l] for l >= 1.  dpos may be NULL when COPY.
template <bool COPY>
__global__ __launch_bounds__(256) void embed_pos_sum_kernel(const half_t* __restrict__ dx, int B, int L, int W, float* __restrict__ dpos,
                                                            half_t* __restrict__ dpatch) {
    const int col = column_pair(W);
    if (col < 0) return;
    const int l = blockIdx.x;
    const size_t step = (size_t)L * W;
    const half_t* src = dx + (size_t)l * W + col;
    half_t* dst = COPY && dpatch && l >= 1 ? dpatch + (size_t)(l - 1) * W + col : nullptr;
    const size_t dstep = (size_t)(L - 1) * W;
    float a0 = 0.f, a1 = 0.f;
    int b = 0;
    for (; b + 8 <= B; b += 8) {
        half2_t v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = *reinterpret_cast<const half2_t*>(src + (size_t)(b + j) * step);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            a0 += (float)v[j][0];
            a1 += (float)v[j][1];
            if (COPY && dst) *reinterpret_cast<half2_t*>(dst + (size_t)(b + j) * dstep) = v[j];
        }
    }
    for (; b < B; ++b) {
        const half2_t v = *reinterpret_cast<const half2_t*>(src + (size_t)b * step);
        a0 += (float)v[0];
        a1 += (float)v[1];
        if (COPY && dst) *reinterpret_cast<half2_t*>(dst + (size_t)b * dstep) = v;
    }
    if (dpos) store2(dpos + (size_t)l * W + col, a0, a1);
}

// ---- dE, first pass: one workgroup per chunk of R sorted positions ----------------------------------------------------------------------------------
// part [nchunks][2][W]: slot 0 = the partial of the run that holds the chunk's FIRST position when that run crosses a boundary (it continues from the
// previous chunk, or it fills the whole chunk and continues into the next), slot 1 = the partial of the run that holds the chunk's LAST position when it
// continues into the next chunk and did not start the chunk.  Ids outside [0, V) and rows outside [0, N) (no caller of this library produces them) add
// nothing and write nothing.
__global__ __launch_bounds__(256) void embed_chunk_kernel(const half_t* __restrict__ dx, const int64_t* __restrict__ ids,
                                                          const int64_t* __restrict__ order, size_t N, int W, int V, float* __restrict__ dE,
                                                          float* __restrict__ part) {
    __shared__ int64_t s_id[R];
    __shared__ int64_t s_row[R];
    const size_t c = blockIdx.x;
    const size_t r0 = c * R;
    const int n = (int)(N - r0 < (size_t)R ? N - r0 : (size_t)R);
    for (int i = threadIdx.x; i < n; i += 256) {
        s_id[i] = ids[r0 + i];
        const int64_t p = order[r0 + i];
        s_row[i] = (p >= 0 && (uint64_t)p < N) ? p : -1;
    }
    __syncthreads();
    const int col = column_pair(W);
    if (col < 0) return;
    const bool from_prev = r0 > 0 && ids[r0 - 1] == s_id[0];
    const bool to_next = r0 + n < N && ids[r0 + n] == s_id[n - 1];
    int64_t cur = s_id[0];
    bool first_run = true;
    float a0 = 0.f, a1 = 0.f;
    float* const part_c = part + c * 2 * (size_t)W + col;

    for (int r = 0; r < n; r += 8) {
        half2_t v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int64_t p = r + j < n ? s_row[r + j] : -1;
            v[j] = p >= 0 ? *reinterpret_cast<const half2_t*>(dx + (size_t)p * W + col) : half2_t{(half_t)0.f, (half_t)0.f};
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (r + j >= n) break;
            const int64_t id = s_id[r + j];
            if (id != cur) {                                               // the run of `cur` ends inside this chunk
                if (first_run && from_prev) store2(part_c, a0, a1);
                else if (cur >= 0 && cur < V) store2(dE + (size_t)cur * W + col, a0, a1);
                first_run = false;
                cur = id;
                a0 = a1 = 0.f;
            }
            a0 += (float)v[j][0];
            a1 += (float)v[j][1];
        }
    }
    if ((first_run && from_prev) || to_next) store2(part_c + (first_run ? 0 : W), a0, a1);
    else if (cur >= 0 && cur < V) store2(dE + (size_t)cur * W + col, a0, a1);
}

// ---- dE, second pass: the runs that cross chunk boundaries -----------------------------------------------------------------------------------------
// Workgroup c acts when chunk c holds the START of a run that continues into chunk c + 1: it finds the run's last chunk by bisection of the sorted ids and
// adds the partials in ascending chunk order.
__global__ __launch_bounds__(256) void embed_merge_kernel(const int64_t* __restrict__ ids, size_t N, int W, int V, const float* __restrict__ part,
                                                          float* __restrict__ dE) {
    const int col = column_pair(W);
    if (col < 0) return;
    const size_t c = blockIdx.x;
    const size_t r0 = c * R;
    const size_t r1 = N - r0 < (size_t)R ? N : r0 + R;
    if (r1 >= N) return;
    const int64_t id = ids[r1 - 1];
    if (ids[r1] != id || id < 0 || id >= V) return;                        // nothing continues into the next chunk
    const bool single = ids[r0] == id;                                     // the whole chunk is this id
    if (single && r0 > 0 && ids[r0 - 1] == id) return;                     // ... and the run started earlier
    size_t lo = r1, hi = N;                                                // first position in [r1, N) whose id is larger
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (ids[mid] <= id) lo = mid + 1;
        else hi = mid;
    }
    const size_t c_end = (lo - 1) / R;
    const float* p = part + (c * 2 + (single ? 0 : 1)) * (size_t)W + col;
    float2 acc = *reinterpret_cast<const float2*>(p);
    p = part + (c + 1) * 2 * (size_t)W + col;
#pragma unroll 8
    for (size_t k = c + 1; k <= c_end; ++k, p += 2 * (size_t)W) {
        const float2 v = *reinterpret_cast<const float2*>(p);
        acc.x += v.x;
        acc.y += v.y;
    }
    store2(dE + (size_t)id * W + col, acc.x, acc.y);
}

bool embed_envelope(const char* entry, int B, int L, int W) {
    if (B >= 1 && L >= 1 && L <= 4096 && W >= 64 && W % 64 == 0 && W <= 2048) return true;
    pclip_set_error("%s: B=%d L=%d W=%d outside the envelope (B >= 1, 1 <= L <= 4096, W %% 64 == 0, W <= 2048)", entry, B, L, W);
    return false;
}
}  // namespace

extern "C" int pclip_text_embed_backward(const void* dx, const int64_t* sorted_ids, const int64_t* order, int B, int L, int W, int V, float* dE,
                                         float* dpos, float* part, pclip_stream_t stream) {
    if (!embed_envelope("pclip_text_embed_backward", B, L, W)) return PCLIP_E_INVALID;
    PCLIP_REQUIRE(V >= 1, "pclip_text_embed_backward: V=%d", V);
    PCLIP_REQUIRE(dx && (dE || dpos), "pclip_text_embed_backward: null pointer");
    PCLIP_REQUIRE(!dE || (sorted_ids && order && part), "pclip_text_embed_backward: dE needs sorted_ids, order and the part buffer");
    PCLIP_REQUIRE((((uintptr_t)dx | (uintptr_t)dE | (uintptr_t)dpos | (uintptr_t)part) & 15) == 0, "pclip_text_embed_backward: operands must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const unsigned gy = (unsigned)ceil_div(W, 512);
    if (dpos) embed_pos_sum_kernel<false><<<dim3((unsigned)L, gy), 256, 0, s>>>((const half_t*)dx, B, L, W, dpos, nullptr);
    if (dE) {
        const size_t N = (size_t)B * L;
        const size_t nchunks = (N + R - 1) / R;
        PCLIP_REQUIRE(nchunks <= 0x7fffffffu, "pclip_text_embed_backward: %zu rows are too many chunks", N);
        if (hipMemsetAsync(dE, 0, (size_t)V * W * sizeof(float), s) != hipSuccess) {
            pclip_set_error("pclip_text_embed_backward: cannot clear dE");
            return PCLIP_E_LAUNCH;
        }
        embed_chunk_kernel<<<dim3((unsigned)nchunks, gy), 256, 0, s>>>((const half_t*)dx, sorted_ids, order, N, W, V, dE, part);
        if (nchunks > 1) embed_merge_kernel<<<dim3((unsigned)nchunks - 1, gy), 256, 0, s>>>(sorted_ids, N, W, V, part, dE);
    }
    return pclip_check_launch("text_embed_backward");
}

extern "C" int pclip_vit_embed_backward_f16(const void* dt, int B, int L, int W, float* dpos, void* dpatch, pclip_stream_t stream) {
    if (!embed_envelope("pclip_vit_embed_backward_f16", B, L, W)) return PCLIP_E_INVALID;
    PCLIP_REQUIRE(dt && (dpos || dpatch), "pclip_vit_embed_backward_f16: null pointer");
    PCLIP_REQUIRE((((uintptr_t)dt | (uintptr_t)dpos | (uintptr_t)dpatch) & 15) == 0, "pclip_vit_embed_backward_f16: operands must be 16-byte aligned");
    embed_pos_sum_kernel<true><<<dim3((unsigned)L, (unsigned)ceil_div(W, 512)), 256, 0, (hipStream_t)stream>>>((const half_t*)dt, B, L, W, dpos, (half_t*)dpatch);
    return pclip_check_launch("vit_embed_backward");
}
