// Epilogue arithmetic shared by the persistent linear kernels (pclip_encoder.hip: eight waves; pclip_gemm4w.hip: four waves with the asm K-loop):
// the reference's fp16 rounding points of nn.Linear + QuickGELU (clip/model.py:164-166, 176-178) and the output store policy.
//
// ROUNDING POINTS (mirrored in tests/gemm_fwd_ref.py, whose per-element tolerance has one first-order term per line; tests/test_gpu_gemm_forward.py grades every
// GEMM kernel and epilogue against float64 with it).  u11 = 2^-11 (an fp16 rounding), u24 = 2^-24 (an fp32 rounding), 2^-25 absolute in fp16's subnormal range;
// the instructions are what hipcc emits for gfx950 (-ffp-contract=fast).  acc = sum_k a w, z = acc + bias:
//   accumulation   fp32 MFMA over K exact products, the fp32 copy of the bias as the accumulators' INITIAL value: A = (K + 1) u24 (|bias| + sum |a| |w|)
//                  (generic kernel: from zero, the bias added in fp32 behind the K-loop — the same K + 1 additions; split-K: S slabs from zero, added in slice
//                  order from zero, then the bias: K + S + 1)
//   act 0          h = r16(z): ONE rounding (v_cvt_f16_f32), with or without bias — never r16(r16(acc) + bias)
//   act 6          y = r16(res + h): one v_pk_add_f16 of two fp16 values
//   act 2 / 3      c = r16(acc); y = r16(c sc + sh) is ONE v_fma_mixlo/hi_f16: no fp32 rounding of the product or the sum, the exact fma rounded to fp16 once;
//                  ReLU (v_max_f32) exact
//   act 5          y2 = relu(r16(y + res)): one v_add_f16 more, the ReLU behind the add
//   act 1          h = r16(z); t = r16(1.702f h) is ONE v_fma_mixlo_f16 (1.702f is the rounded constant); the exponent's argument fma(t, -log2 e, 0) is one fp32
//                  rounding of a value of size |t| log2 e (v_fma_mix_f32), log2 e itself a rounded fp32 constant; v_exp_f32, 1 + ex (v_pk_add_f32), v_rcp_f32;
//                  s = r16(..); y = r16(h s) is one v_pk_mul_f16.  Where 1.702 |h| leaves fp16's range t = +-inf, s = 1 or 0 exactly, y = h or -0 (never NaN
//                  while h is finite); h = -inf gives -inf x 0 = NaN, as the reference's own fp16 arithmetic does.
//   overflow       every r16 above rounds to infinity from 65520 on, and an infinite intermediate stays infinite
#pragma once
#include "pclip_common.h"

typedef float float2_t __attribute__((ext_vector_type(2)));

// QuickGELU with the reference's three fp16 roundings.  exp / reciprocal use the hardware approximations
// (v_exp_f32, v_rcp_f32: ~1-2 ulp in fp32), far inside the fp16 rounding that follows each step.
__device__ __forceinline__ float quick_gelu16(float v) {
    const float t = r16(1.702f * v);
    const float s = r16(__builtin_amdgcn_rcpf(1.f + __expf(-t)));
    return r16(v * s);
}

// Four at a time with packed fp16 instructions where the arithmetic IS fp16: the two conversions are v_cvt_pk_f16_f32 and the
// final product h * s of two fp16 values is one correctly rounded v_pk_mul_f16 (= r16 of the exact fp32 product).
__device__ __forceinline__ half4_t quick_gelu16x4(float4_t v) {
    const half2_t h01 = __builtin_convertvector(float2_t{v[0], v[1]}, half2_t), h23 = __builtin_convertvector(float2_t{v[2], v[3]}, half2_t);
    const half_t h[4] = {h01[0], h01[1], h23[0], h23[1]};
    // The activation arithmetic is what the c_fc epilogue is bound by (VALU: tools/trace_tile.py), so every instruction counts: the exponent's argument
    // as ONE v_fma_mix_f32 on the fp16 value t (fma(t, -log2 e, 0) == the fp32 product t * -log2 e that __expf(-t) forms, without the separate
    // v_cvt_f32_f16), the "1 +" of two elements as one v_pk_add_f32: 48 instead of 54 issue slots per four elements, same bits.
    float ex[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const half_t t = (half_t)(1.702f * (float)h[e]);
        ex[e] = __builtin_amdgcn_exp2f(__builtin_fmaf((float)t, -1.4426950408889634f, 0.f));
    }
    const float2_t one = {1.f, 1.f};
    const float2_t d01 = float2_t{ex[0], ex[1]} + one, d23 = float2_t{ex[2], ex[3]} + one;
    const float s[4] = {__builtin_amdgcn_rcpf(d01[0]), __builtin_amdgcn_rcpf(d01[1]), __builtin_amdgcn_rcpf(d23[0]), __builtin_amdgcn_rcpf(d23[1])};
    const half2_t s01 = __builtin_convertvector(float2_t{s[0], s[1]}, half2_t), s23 = __builtin_convertvector(float2_t{s[2], s[3]}, half2_t);
    const half2_t y01 = h01 * s01, y23 = h23 * s23;
    return half4_t{y01[0], y01[1], y23[0], y23[1]};
}

// Plain fp32 -> fp16 of four values: the one rounding of r16(acc + bias) (the bias is already inside the accumulators).
__device__ __forceinline__ half4_t cvt16x4(float4_t v) {
    half4_t h;
#pragma unroll
    for (int e = 0; e < 4; ++e) h[e] = (half_t)v[e];
    return h;
}

// eval-mode BatchNorm (+ReLU) on four columns with their scale / shift (clip/model.py:43-52), two roundings: the convolution's output is an fp16 tensor
// (r16(v)), and so is bn's: r16(. * sc + sh) compiles to ONE v_fma_mixlo / mixhi_f16 — the exact fma rounded to fp16 once, no fp32 rounding of the product or the
// sum (list at the top of this file); ReLU is exact.
template <bool RELU>
__device__ __forceinline__ half4_t bn16x4(float4_t v, float4_t sc, float4_t sh) {
    half4_t h;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float y = r16(r16(v[e]) * sc[e] + sh[e]);
        if (RELU) y = fmaxf(y, 0.f);
        h[e] = (half_t)y;
    }
    return h;
}

// Residual add on one 16-byte chunk: r16(x + h) of two fp16 tensors — one rounding: hipcc emits a single v_pk_add_f16 / v_add_f16 for the widened sum, which gives
// the same value — (+ exact ReLU: `out += identity; relu` of a bottleneck).
template <bool RELU>
__device__ __forceinline__ half8_t add_residual16x8(half8_t x, half8_t h) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float y = r16((float)x[j] + (float)h[j]);
        h[j] = (half_t)(RELU ? fmaxf(y, 0.f) : y);
    }
    return h;
}

// Output rows of the persistent linear kernels: non-temporal 16-byte stores (A/B switch PCLIP_NT_STORE) — a c_fc launch writes
// 1.2 GB that nobody re-reads before it has left the 4 MiB L2 anyway; keeping it out leaves the L2 to the operand panels.
#ifndef PCLIP_NT_STORE
#define PCLIP_NT_STORE 1
#endif
typedef float f32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void st_out(half_t* p, half8_t v) {
#if PCLIP_NT_STORE
    __builtin_nontemporal_store(__builtin_bit_cast(f32x4_t, v), reinterpret_cast<f32x4_t*>(p));
#else
    st_half8(p, v);
#endif
}

