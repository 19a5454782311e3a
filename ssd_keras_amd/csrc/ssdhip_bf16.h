// The value helpers every kernel file shares: bf16 / float16 bit conversions, packed-pair operations and the vector types of the MFMA
// operands.  None of them needs an amdgcn-only builtin, so the host pass sees them too (buffer descriptors and LDS-DMA: ssdhip_tile.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ssdhip {

typedef unsigned int u32;                                 // (ssdhip_math.h declares it too; that header also defines a kernel)

typedef unsigned short bf16_t;                           // a bf16 value as its bits
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float bf16_float(u32 h) { return __uint_as_float(h << 16); }
// float32 -> bf16 bits, round to nearest even, NaN stays NaN (as c10::BFloat16).  T: u32, or bf16_t where the value goes to memory as it is
template <typename T = u32>
__device__ __forceinline__ T bf16_bits(float f) {
    const u32 u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (T)((u >> 16) | 0x40u);
    return (T)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

// two float32 -> packed bf16, round to nearest even: one v_cvt_pk_bf16_f32 (the integer formulation, bf16_bits, costs ~6 VALU
// operations per value, and with one wave per SIMD every epilogue instruction is MFMA idle time)
__device__ __forceinline__ u32 pack2_bf16(float a, float b) {
    const f32x2 v = {a, b};
    return __builtin_bit_cast(u32, __builtin_convertvector(v, bf16x2));
}

__device__ __forceinline__ float relu_nan(float v) { return v <= 0.f ? 0.f : v; }       // NaN stays NaN, -0 -> +0

// Two bf16 values at once as signed 16-bit integers (v_pk_max_i16).  On ROUNDED activations this is the whole activation step:
// max(x, 0) sends every value with the sign bit set (negative numbers, -0) to +0 and leaves the others (+NaN included) alone -- the
// same bits as relu_nan before the rounding, because rounding to bf16 is monotonic and keeps the sign; max(x, 0x8000) is the
// identity (no activation).  And on NON-NEGATIVE bf16 values integer order is numeric order, so it is also the pooling maximum.
__device__ __forceinline__ u32 pkmax_i16(u32 a, u32 b) {
    return __builtin_bit_cast(u32, __builtin_elementwise_max(__builtin_bit_cast(s16x2, a), __builtin_bit_cast(s16x2, b)));
}

// The reference-precision (X3) pair of a float32 value: hi = fl16(v), lo = fl16(v - hi).  Two values per word: returns the hi parts,
// lo_out the lo parts.
__device__ __forceinline__ u32 split2_f16(float a, float b, u32& lo_out) {
    const _Float16 ha = (_Float16)a, hb = (_Float16)b;
    const _Float16 la = (_Float16)(a - (float)ha), lb = (_Float16)(b - (float)hb);
    lo_out = (u32)__builtin_bit_cast(unsigned short, la) | ((u32)__builtin_bit_cast(unsigned short, lb) << 16);
    return (u32)__builtin_bit_cast(unsigned short, ha) | ((u32)__builtin_bit_cast(unsigned short, hb) << 16);
}

}  // namespace ssdhip
