// fora_softmax_exp.h -- exp_def, the exponential of ROW SOFTMAX (the contract is in include/fora_hip.h): defined for t <= 0 and
// t = -inf, every bit of the result defined.  Single IEEE f64 multiplies and adds in a written order, nothing fused -- the
// file that includes this one is compiled with -ffp-contract=off, and the function says so again where the compiler knows
// the pragma.  No HIP types: a CPU program includes it as it stands (tests/softmax_exp_check.cpp), and there the guard below
// is empty.
//   t < -708.0 or t = -inf: +0.0 (so no result is ever subnormal: exp(-708) = 3.3e-308 is still above 2^-1022)
//   k = rint(t * LOG2E), to nearest even;  r = (t - k * LN2_HI) - k * LN2_LO  (LN2_HI has 21 trailing zero bits: k * LN2_HI
//   is exact for |k| <= 1022);  p = sum r^j / j! by Horner from j = 13 down, one multiply and one add per step;
//   result = p * 2^k, one multiply by the double whose biased exponent is k + 1023 (k in [-1021, 0]: always normal).
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define FORA_EXP_HD __host__ __device__
#else
#define FORA_EXP_HD
#endif

namespace fora {

FORA_EXP_HD inline double exp_def(double t) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (!(t >= -708.0)) return 0.0; // (NaN never comes here; it would give +0.0 too)
    const double k = rint(t * 0x1.71547652b82fep+0);
    const double r = (t - k * 0x1.62e42feep-1) - k * 0x1.a39ef35793c76p-33;
    // c_j = 1.0 / (double)(j!): one IEEE division of two exact doubles each, folded by the compiler; literals, not a table
    double p = 1.0 / 6227020800.0;     // 13!
    p = p * r + 1.0 / 479001600.0;     // 12!
    p = p * r + 1.0 / 39916800.0;      // 11!
    p = p * r + 1.0 / 3628800.0;       // 10!
    p = p * r + 1.0 / 362880.0;        // 9!
    p = p * r + 1.0 / 40320.0;         // 8!
    p = p * r + 1.0 / 5040.0;          // 7!
    p = p * r + 1.0 / 720.0;           // 6!
    p = p * r + 1.0 / 120.0;           // 5!
    p = p * r + 1.0 / 24.0;            // 4!
    p = p * r + 1.0 / 6.0;             // 3!
    p = p * r + 1.0 / 2.0;             // 2!
    p = p * r + 1.0;                   // 1!
    p = p * r + 1.0;                   // 0!
    const uint64_t bits = (uint64_t)((int64_t)k + 1023) << 52;
    double two_k;
    __builtin_memcpy(&two_k, &bits, 8);
    return p * two_k;
}

} // namespace fora
