// fora_narrow.h -- the element types of the dense operands of the calls on the held rows (PROPAGATE and its transposed and
// valued forms, SCORES (SDDMM), ATTENTION and its backward pass; the paragraph NARROW OPERANDS of include/fora_hip.h): which
// there are, how many bytes each takes, and how a narrow one -- f16, FP8 E4M3, FP8 E5M2 -- widens to f32.  Every narrow
// value is exactly an f32, so a call with a narrow operand gives the bits it gives with that operand widened.
//   narrow_f16_bits / narrow_e4m3_bits / narrow_e5m2_bits   the rule itself: constexpr integer functions from a code to the
//                     f32 bit pattern -- host-compilable, tests/narrow_plan_check.cpp holds them to ldexp on every code.
//   narrow_widen<ET>, narrow_widen_byte<ET>   what the kernels run (HIP only): v_cvt_f32_f16 for f16, and gfx950's FP8
//                     conversions (v_cvt_f32_fp8 for E4M3, v_cvt_f32_bf8 for E5M2), which take a word of four codes and
//                     the number of the byte.  That they keep subnormals and agree with the rule on every code -- OCP
//                     E4M3 with its two NaN codes and no infinity, E5M2 as the high byte of a binary16 -- is what
//                     tests/test_narrow_gpu.py shows on the GPU; the integer functions are the fall-back if a later
//                     target should disagree (DESIGN.md 5.22 has what they cost).
// Integer code up to the HIP part, no context.
#pragma once
#include <stdint.h>

namespace fora {

// the values of FORA_PROP_* (fora_hip.hip holds the two equal); 2 is FORA_PROP_F64, a value type, and 3 is no type
enum : int { ELT_F32 = 0, ELT_BF16 = 1, ELT_F16 = 4, ELT_E4M3 = 5, ELT_E5M2 = 6 };
// a load site that takes its element type at run time (the one-element-per-lane sites of fora_sddmm.h)
constexpr int ELT_ANY = -1;

constexpr bool elt_known(int t) { return t == ELT_F32 || t == ELT_BF16 || t == ELT_F16 || t == ELT_E4M3 || t == ELT_E5M2; }
// the one place that says how many bytes an element takes
constexpr uint32_t elt_bytes(int t) { return t == ELT_F32 ? 4u : (t == ELT_BF16 || t == ELT_F16) ? 2u : 1u; }

// IEEE binary16 (s, e: 5 bits, m: 10 bits) as the f32 with the same value; a NaN code gives a quiet NaN
constexpr uint32_t narrow_f16_bits(uint32_t h) {
    const uint32_t s = (h & 0x8000u) << 16, e = (h >> 10) & 31u;
    uint32_t m = h & 1023u;
    if (e == 31u) return s | 0x7F800000u | (m ? 0x00400000u | (m << 13) : 0u);
    if (e) return s | ((e + 112u) << 23) | (m << 13);  // (1024 + m) * 2^(e - 25) = (1 + m / 1024) * 2^(e - 15)
    if (!m) return s;                                  // +-0
    uint32_t sh = 0;                                   // m * 2^-24: the leading one moved to bit 10
    while (!(m & 1024u)) { m <<= 1; sh++; }
    return s | ((113u - sh) << 23) | ((m & 1023u) << 13);
}
// FP8 E5M2: the binary16 whose bits are byte << 8
constexpr uint32_t narrow_e5m2_bits(uint32_t b) { return narrow_f16_bits((b & 0xFFu) << 8); }
// FP8 E4M3, the OCP "fn" form (s, e: 4 bits, m: 3 bits): 0x7F and 0xFF are NaN, there is no infinity
constexpr uint32_t narrow_e4m3_bits(uint32_t b) {
    const uint32_t s = (b & 0x80u) << 24, e = (b >> 3) & 15u;
    uint32_t m = b & 7u;
    if ((b & 0x7Fu) == 0x7Fu) return s | 0x7FC00000u;
    if (e) return s | ((e + 120u) << 23) | (m << 20);  // (8 + m) * 2^(e - 10) = (1 + m / 8) * 2^(e - 7)
    if (!m) return s;
    uint32_t sh = 0;                                   // m * 2^-9: the leading one moved to bit 3
    while (!(m & 8u)) { m <<= 1; sh++; }
    return s | ((121u - sh) << 23) | ((m & 7u) << 20);
}
// the rule for a type known at run time (host and device): the f32 bits of a code of a narrow type
constexpr uint32_t narrow_bits(int t, uint32_t code) {
    return t == ELT_F16 ? narrow_f16_bits(code) : t == ELT_E4M3 ? narrow_e4m3_bits(code) : narrow_e5m2_bits(code);
}

#if defined(__HIPCC__)
// ---- what the kernels run: code (zero-extended to a word) -> f32, exact
__device__ __forceinline__ float narrow_cvt_f16(uint32_t h) { return (float)__builtin_bit_cast(_Float16, (uint16_t)h); }
// byte `sel` of a word of four FP8 codes: gfx950's own conversions, which select the byte themselves.  sel is a constant
// wherever a caller's loop is unrolled, and the switch folds to the one instruction
template <int ET> __device__ __forceinline__ float narrow_widen_byte(uint32_t word, int sel) {
    static_assert(ET == ELT_E4M3 || ET == ELT_E5M2, "an FP8 type");
    if constexpr (ET == ELT_E4M3) {
        switch (sel) {
        case 0: return __builtin_amdgcn_cvt_f32_fp8((int)word, 0);
        case 1: return __builtin_amdgcn_cvt_f32_fp8((int)word, 1);
        case 2: return __builtin_amdgcn_cvt_f32_fp8((int)word, 2);
        default: return __builtin_amdgcn_cvt_f32_fp8((int)word, 3);
        }
    } else {
        switch (sel) {
        case 0: return __builtin_amdgcn_cvt_f32_bf8((int)word, 0);
        case 1: return __builtin_amdgcn_cvt_f32_bf8((int)word, 1);
        case 2: return __builtin_amdgcn_cvt_f32_bf8((int)word, 2);
        default: return __builtin_amdgcn_cvt_f32_bf8((int)word, 3);
        }
    }
}
template <int ET> __device__ __forceinline__ float narrow_widen(uint32_t code) {
    static_assert(ET == ELT_F16 || ET == ELT_E4M3 || ET == ELT_E5M2, "a narrow type");
    if constexpr (ET == ELT_F16) return narrow_cvt_f16(code);
    else return narrow_widen_byte<ET>(code, 0);
}
#endif

} // namespace fora
