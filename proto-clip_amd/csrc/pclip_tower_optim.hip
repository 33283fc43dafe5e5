// Mixed-precision AdamW for the tower parameters (proto_clip_amd/optim.py: TowerAdamW): fp32 master weights and moments, gradient
// unscaling, overflow detection, clipping by the global norm and a dynamic loss scale, in three launches however many tensors there are,
// without a host synchronisation and without atomics (two runs give the same bits).  tests/tower_optim_ref.py restates every sequence
// below in fp32 torch on the CPU; the kernels are graded bit for bit against it.
//
// Operands: a device table of one 64-byte row per tensor (include/pclip.h: PCLIP_TOWER_ROW_*) and a float side table {lr, weight_decay}
// per tensor.  The tensors are cut into chunks of PCLIP_TOWER_CHUNK = 4096 elements; chunk c belongs to the tensor with the greatest
// first_chunk <= c (binary search), and covers its elements [4096 (c - first_chunk), ...).  Inside a chunk, thread t of the 256 owns the two
// groups of eight consecutive elements  e = 2048 j + 8 t + k,  j = 0, 1,  k = 0 .. 7  (one 16-byte load of fp16, two of fp32, per group where
// every base of the tensor is 16-byte aligned — PCLIP_TOWER_ALIGNED; element by element otherwise and in a ragged last group: same owner,
// same order, same bits).
//
// 1. tower_grad_sumsq_kernel: partial[c] = sum of squares of the chunk's RAW (still scaled) gradients in fp32:
//      lane:   s = 0;  for j = 0, 1: for k = 0 .. 7: s = fmaf(g, g, s)              (its elements in index order; absent elements add nothing)
//      wave:   s += s of lane ^ 32, ^ 16, ^ 8, ^ 4, ^ 2, ^ 1                        (butterfly: wave_sum)
//      chunk:  ((w0 + w1) + w2) + w3                                                (the four waves in order)
//    25 roundings on the longest path, all terms non-negative: relative error <= 25 * 2^-24 (to first order).  An Inf or NaN gradient makes
//    its partial non-finite: that is the overflow detector.
// 2. tower_optim_finish_kernel (one workgroup): thread t adds partials [t per, (t + 1) per), per = ceil(nchunks / 256), in index order in
//    double; thread 0 adds the 256 sums in thread order -> total.  found_inf = !isfinite(total).  On a clean step
//      inv_scale = 1.f / scale;  grad_norm = float(sqrt(total) / double(scale))
//      clip_coef = max_norm > 0 ? min(1.f, max_norm / (grad_norm + 1e-6f)) : 1.f;  gmul = clip_coef * inv_scale
//      step += 1;  b1t *= beta1;  b2t *= beta2  (double);  bc1 = float(1 - b1t);  sqrt_bc2 = float(sqrt(1 - b2t))
//      tracker += 1;  if tracker == growth_interval: scale *= growth (kept if that is not finite), tracker = 0          (dynamic scale only)
//    and on overflow  grad_norm = inf, clip_coef = gmul = 0, scale *= backoff, tracker = 0  (dynamic scale only); step, b1t, b2t stay.
// 3. tower_adamw_kernel: nothing when found_inf; otherwise per element, each operation rounded once to fp32 (the file is built with
//    -ffp-contract=off: only the fmaf calls below are fused),
//      g = float(g_raw) * gmul
//      m = fmaf(1 - b1, g, b1 * m)
//      v = fmaf((1 - b2) * g, g, b2 * v)
//      w = master;  if the tensor decays: w = w * (1 - lr * wd)
//      w = w - ((lr / bc1) * m) / (sqrt(v) / sqrt_bc2 + eps)
//    then master, m, v are stored and the parameter: half(w) for an fp16 parameter; an fp32 parameter IS its master (same pointer).
//    b1, 1 - b1, b2, 1 - b2, eps arrive as floats rounded once from the host's doubles.  A tensor without a gradient (g == NULL) has g = 0.
#include "pclip_common.h"

namespace {

constexpr int CH = PCLIP_TOWER_CHUNK;
constexpr int MAX_GRID = 2048;          // memory-bound: a capped grid strides over the chunks

struct Row {
    void* p;
    const void* g;
    float* master;
    float* m;
    float* v;
    long long n, first_chunk, flags;
};
static_assert(sizeof(Row) == PCLIP_TOWER_ROW_BYTES, "table row layout");

struct State {
    double b1t, b2t, total;
    float scale;
    int tracker, step, found_inf;
    float grad_norm, clip_coef, inv_scale, bc1, sqrt_bc2, gmul;
};
static_assert(sizeof(State) == PCLIP_TOWER_STATE_BYTES, "state block layout");

// the tensor that owns `chunk`: the greatest t with first_chunk[t] <= chunk
__device__ __forceinline__ int find_tensor(const Row* __restrict__ rows, int nt, int chunk) {
    int lo = 0, hi = nt - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rows[mid].first_chunk <= chunk) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ void load8_f32(const float* __restrict__ x, int cnt, bool vec, float (&o)[8]) {
    if (vec && cnt == 8) {
        const float4_t a = *reinterpret_cast<const float4_t*>(x), b = *reinterpret_cast<const float4_t*>(x + 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) { o[k] = a[k]; o[4 + k] = b[k]; }
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = k < cnt ? x[k] : 0.f;
    }
}

__device__ __forceinline__ void load8_f16(const half_t* __restrict__ x, int cnt, bool vec, float (&o)[8]) {
    if (vec && cnt == 8) {
        const half8_t a = ld_half8(x);
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = (float)a[k];
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = k < cnt ? (float)x[k] : 0.f;
    }
}

__device__ __forceinline__ void store8_f32(float* __restrict__ x, int cnt, bool vec, const float (&o)[8]) {
    if (vec && cnt == 8) {
        float4_t a, b;
#pragma unroll
        for (int k = 0; k < 4; ++k) { a[k] = o[k]; b[k] = o[4 + k]; }
        *reinterpret_cast<float4_t*>(x) = a;
        *reinterpret_cast<float4_t*>(x + 4) = b;
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (k < cnt) x[k] = o[k];
    }
}

// the raw gradients of one group (zeros where the tensor has no gradient)
__device__ __forceinline__ void load8_grad(const Row& r, long long e, int cnt, bool vec, float (&o)[8]) {
    if (!r.g) {
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = 0.f;
    } else if (r.flags & PCLIP_TOWER_GRAD_F16) {
        load8_f16((const half_t*)r.g + e, cnt, vec, o);
    } else {
        load8_f32((const float*)r.g + e, cnt, vec, o);
    }
}

// elements of `chunk` inside its tensor: [c0, c0 + nc)
__device__ __forceinline__ int chunk_span(const Row& r, int chunk, long long& c0) {
    c0 = (long long)(chunk - r.first_chunk) * CH;
    const long long left = r.n - c0;
    return left < CH ? (left > 0 ? (int)left : 0) : CH;
}

__global__ __launch_bounds__(256) void tower_grad_sumsq_kernel(const Row* __restrict__ rows, int nt, int nchunks, float* __restrict__ partials) {
    __shared__ float red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const Row r = rows[find_tensor(rows, nt, chunk)];
        long long c0;
        const int nc = chunk_span(r, chunk, c0);
        const bool vec = (r.flags & PCLIP_TOWER_ALIGNED) != 0;
        float s = 0.f;
        if (r.g) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int e = j * (CH / 2) + tid * 8;
                const int cnt = nc - e < 8 ? nc - e : 8;
                if (cnt <= 0) continue;
                float g[8];
                load8_grad(r, c0 + e, cnt, vec, g);
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (k < cnt) s = fmaf(g[k], g[k], s);
            }
        }
        s = wave_sum(s);
        if (lane == 0) red[wave] = s;
        __syncthreads();
        if (tid == 0) partials[chunk] = ((red[0] + red[1]) + red[2]) + red[3];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void tower_optim_finish_kernel(const float* __restrict__ partials, int nchunks, State* __restrict__ st, float max_norm,
                                                                 double beta1, double beta2, float growth, float backoff, int growth_interval,
                                                                 int dynamic) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const int per = (nchunks + 255) / 256;
    const int i0 = tid * per, i1 = i0 + per < nchunks ? i0 + per : nchunks;
    double s = 0.0;
    for (int i = i0; i < i1; ++i) s += (double)partials[i];
    red[tid] = s;
    __syncthreads();
    if (tid != 0) return;
    double total = 0.0;
    for (int i = 0; i < 256; ++i) total += red[i];
    const float scale = st->scale;
    const float inv_scale = __fdiv_rn(1.f, scale);
    const bool found = !__builtin_isfinite(total);
    st->total = total;
    st->found_inf = found ? 1 : 0;
    st->inv_scale = inv_scale;
    if (found) {
        st->grad_norm = __builtin_inff();
        st->clip_coef = 0.f;
        st->gmul = 0.f;
        if (dynamic) {
            st->scale = __fmul_rn(scale, backoff);
            st->tracker = 0;
        }
        return;
    }
    const float grad_norm = (float)(sqrt(total) / (double)scale);
    float clip_coef = 1.f;
    if (max_norm > 0.f) {
        clip_coef = __fdiv_rn(max_norm, __fadd_rn(grad_norm, 1e-6f));
        clip_coef = clip_coef < 1.f ? clip_coef : 1.f;
    }
    st->grad_norm = grad_norm;
    st->clip_coef = clip_coef;
    st->gmul = __fmul_rn(clip_coef, inv_scale);
    const double b1t = st->b1t * beta1, b2t = st->b2t * beta2;
    st->b1t = b1t;
    st->b2t = b2t;
    st->step = st->step + 1;
    st->bc1 = (float)(1.0 - b1t);
    st->sqrt_bc2 = (float)sqrt(1.0 - b2t);
    if (dynamic) {
        const int ok = st->tracker + 1;
        if (ok == growth_interval) {
            const float grown = __fmul_rn(scale, growth);
            if (__builtin_isfinite(grown)) st->scale = grown;
            st->tracker = 0;
        } else {
            st->tracker = ok;
        }
    }
}

__global__ __launch_bounds__(256) void tower_adamw_kernel(const Row* __restrict__ rows, const float* __restrict__ hyper, int nt, int nchunks,
                                                          const State* __restrict__ st, float b1, float omb1, float b2, float omb2, float eps) {
    if (st->found_inf) return;
    const float gmul = st->gmul, bc1 = st->bc1, sqrt_bc2 = st->sqrt_bc2;
    const int tid = threadIdx.x;
    for (int chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const int t = find_tensor(rows, nt, chunk);
        const Row r = rows[t];
        long long c0;
        const int nc = chunk_span(r, chunk, c0);
        const bool vec = (r.flags & PCLIP_TOWER_ALIGNED) != 0, decays = (r.flags & PCLIP_TOWER_DECAY) != 0, p16 = (r.flags & PCLIP_TOWER_PARAM_F16) != 0;
        const float lr = hyper[2 * t], wd = hyper[2 * t + 1];
        const float keep = __fsub_rn(1.f, __fmul_rn(lr, wd)), step_size = __fdiv_rn(lr, bc1);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int e0 = j * (CH / 2) + tid * 8;
            const int cnt = nc - e0 < 8 ? nc - e0 : 8;
            if (cnt <= 0) continue;
            const long long e = c0 + e0;
            float g[8], w[8], m[8], v[8];
            load8_grad(r, e, cnt, vec, g);
            load8_f32(r.master + e, cnt, vec, w);
            load8_f32(r.m + e, cnt, vec, m);
            load8_f32(r.v + e, cnt, vec, v);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float gk = __fmul_rn(g[k], gmul);
                m[k] = fmaf(omb1, gk, __fmul_rn(b1, m[k]));
                v[k] = fmaf(__fmul_rn(omb2, gk), gk, __fmul_rn(b2, v[k]));
                float wk = w[k];
                if (decays) wk = __fmul_rn(wk, keep);
                const float den = __fadd_rn(__fdiv_rn(sqrtf(v[k]), sqrt_bc2), eps);
                w[k] = __fsub_rn(wk, __fdiv_rn(__fmul_rn(step_size, m[k]), den));
            }
            store8_f32(r.master + e, cnt, vec, w);
            store8_f32(r.m + e, cnt, vec, m);
            store8_f32(r.v + e, cnt, vec, v);
            if (p16) {
                half_t* p = (half_t*)r.p + e;
                if (vec && cnt == 8) {
                    half8_t h;
#pragma unroll
                    for (int k = 0; k < 8; ++k) h[k] = (half_t)w[k];
                    st_half8(p, h);
                } else {
#pragma unroll
                    for (int k = 0; k < 8; ++k)
                        if (k < cnt) p[k] = (half_t)w[k];
                }
            }
        }
    }
}

inline int chunk_grid(int nchunks) { return nchunks < MAX_GRID ? nchunks : MAX_GRID; }

}  // namespace

extern "C" int pclip_tower_grad_sumsq(const void* table, int ntensors, int nchunks, float* partials, pclip_stream_t stream) {
    PCLIP_REQUIRE(table && partials, "pclip_tower_grad_sumsq: null pointer");
    PCLIP_REQUIRE(ntensors >= 1 && nchunks >= ntensors, "pclip_tower_grad_sumsq: ntensors=%d nchunks=%d (every tensor owns at least one chunk)", ntensors,
                  nchunks);
    tower_grad_sumsq_kernel<<<chunk_grid(nchunks), 256, 0, (hipStream_t)stream>>>((const Row*)table, ntensors, nchunks, partials);
    return pclip_check_launch("tower_grad_sumsq");
}

extern "C" int pclip_tower_optim_finish(const float* partials, int nchunks, void* state, float max_norm, double beta1, double beta2, float growth,
                                        float backoff, int growth_interval, int dynamic, pclip_stream_t stream) {
    PCLIP_REQUIRE(partials && state, "pclip_tower_optim_finish: null pointer");
    PCLIP_REQUIRE(nchunks >= 1, "pclip_tower_optim_finish: nchunks=%d must be >= 1", nchunks);
    PCLIP_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "pclip_tower_optim_finish: betas (%g, %g) outside [0, 1)", beta1, beta2);
    PCLIP_REQUIRE(!dynamic || (growth > 1.f && backoff > 0.f && backoff < 1.f && growth_interval >= 1),
                  "pclip_tower_optim_finish: growth=%g backoff=%g growth_interval=%d", (double)growth, (double)backoff, growth_interval);
    tower_optim_finish_kernel<<<1, 256, 0, (hipStream_t)stream>>>(partials, nchunks, (State*)state, max_norm, beta1, beta2, growth, backoff,
                                                                  growth_interval, dynamic);
    return pclip_check_launch("tower_optim_finish");
}

extern "C" int pclip_tower_adamw(const void* table, const float* hyper, int ntensors, int nchunks, const void* state, double beta1, double beta2,
                                 double eps, pclip_stream_t stream) {
    PCLIP_REQUIRE(table && hyper && state, "pclip_tower_adamw: null pointer");
    PCLIP_REQUIRE(ntensors >= 1 && nchunks >= ntensors, "pclip_tower_adamw: ntensors=%d nchunks=%d (every tensor owns at least one chunk)", ntensors, nchunks);
    PCLIP_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0, "pclip_tower_adamw: betas (%g, %g) eps %g", beta1, beta2, eps);
    tower_adamw_kernel<<<chunk_grid(nchunks), 256, 0, (hipStream_t)stream>>>((const Row*)table, hyper, ntensors, nchunks, (const State*)state, (float)beta1,
                                                                             (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps);
    return pclip_check_launch("tower_adamw");
}
