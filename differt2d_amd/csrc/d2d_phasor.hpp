// The phasor of the coherent field (d2d_coherent_field_launch, d2d::FieldSink):  phasor(f, c, s)  gives  c = cos(2 pi f),
// s = sin(2 pi f)  for a phase f in turns, 0 <= f < 1 (the fractional part of path length / wavelength).  This text IS the
// definition: neither the device library's sinf / cosf nor the hardware's sine and cosine match a host libm bit for bit, so the
// phasor is a fixed sequence of fp32 multiplies, adds and compares that compiles for host and device alike (no HIP builtins, no
// library call; the build's -ffp-contract=off keeps one rounding per operation).  tests/native/coherent_field_host.cpp compiles it
// with g++, and tests/test_coherent_field_cpu.py holds it bit for bit to a NumPy restatement and, in accuracy, to float64.
//
//   reduce    t = f * 4                                  exact
//             k = [t >= 0.5] + [t >= 1.5] + [t >= 2.5] + [t >= 3.5]        = floor(4 f + 1/2) in 0..4, the nearest quarter turn
//             g = f - k * 0.25                           exact, |g| <= 0.125
//   scale     x = g * 6.2831853f                         one rounding, |x| <= pi / 4 (+ 1 ulp)
//   evaluate  sin x = x + x * (x^2 * S(x^2)),  cos x = 1 + x^2 * C(x^2)       Taylor through x^9 and x^10, Horner, fixed order
//   rotate    by k quarter turns (k = 4 is k = 0): a swap and sign changes, no arithmetic
//
// k comes from compares, not from floorf(f * 4 + 0.5f): that sum is rounded, and for f = 0.125 - 2^-27 (the fp32 below 1/8) it
// rounds up to 1, whereupon f - 0.25 needs 25 bits and g is no longer exact.  The compares are that floor in exact arithmetic.
// g exact: for k >= 1, f >= 0.125 is a multiple of 2^-26 and so is g, with |g| <= 2^-3: 24 bits.  A NaN f fails every compare
// (k = 0) and comes out as (NaN, NaN); phasor(0) = (1, +0) exactly.
//
// Accuracy over [0, 1), against float64 cos / sin of 2 pi f: the absolute error stays below 2 * 2^-24 (measured maximum
// 1.64 * 2^-24; most of it is the rounding of 2 pi to 6.2831853f and of x, 0.37 and 0.5 units at |x| = pi / 4).
//
// Beside it, the two values every coherent sink forms from a contribution t and its path length r in front of the phasor:
//   field_amp(root, t)      a = root ? copysignf(sqrtf(fabsf(t)), t) : t      the amplitude: sign(t) sqrt|t| in the SQRT mode, t itself in LINEAR
//   turn_fraction(r, inv)   u = r * inv ;  f = u - floorf(u)                  the phase in turns: exact and in [0, 1) for every finite u >= 0, NaN otherwise
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define D2D_PHASOR_FN __host__ __device__ __attribute__((always_inline)) inline
#else
#define D2D_PHASOR_FN __attribute__((always_inline)) inline
#endif

namespace d2d {

D2D_PHASOR_FN float field_amp(bool root, float t) { return root ? copysignf(sqrtf(fabsf(t)), t) : t; }

D2D_PHASOR_FN float turn_fraction(float r, float inv) {
    const float u = r * inv;
    return u - floorf(u);
}

constexpr float PHASOR_TWO_PI = 6.2831853f;
// 1/9!, -1/7!, 1/5!, -1/3!  and  -1/10!, 1/8!, -1/6!, 1/4!, -1/2!  (decimal literals, so that any restatement reads the same fp32)
constexpr float PHASOR_S9 = 2.7557319e-6f, PHASOR_S7 = -1.9841270e-4f, PHASOR_S5 = 8.3333333e-3f, PHASOR_S3 = -1.6666667e-1f;
constexpr float PHASOR_C10 = -2.7557319e-7f, PHASOR_C8 = 2.4801587e-5f, PHASOR_C6 = -1.3888889e-3f, PHASOR_C4 = 4.1666667e-2f,
                PHASOR_C2 = -0.5f;

// the nearest quarter turn of f in [0, 1): 0 .. 4 (0 for NaN)
__attribute__((always_inline)) constexpr float phasor_quarter(float f) {
    const float t = f * 4.0f;
    return ((t >= 0.5f ? 1.0f : 0.0f) + (t >= 1.5f ? 1.0f : 0.0f)) + ((t >= 2.5f ? 1.0f : 0.0f) + (t >= 3.5f ? 1.0f : 0.0f));
}

// f minus its nearest quarter turn, in turns: exact, |g| <= 0.125
__attribute__((always_inline)) constexpr float phasor_reduce(float f, float k) { return f - k * 0.25f; }

// c = cos(2 pi f), s = sin(2 pi f) for 0 <= f < 1
__attribute__((always_inline)) constexpr void phasor(float f, float& c, float& s) {
    const float k = phasor_quarter(f);
    const float g = phasor_reduce(f, k);
    const float x = g * PHASOR_TWO_PI;
    const float z = x * x;
    const float ps = ((PHASOR_S9 * z + PHASOR_S7) * z + PHASOR_S5) * z + PHASOR_S3;
    const float pc = (((PHASOR_C10 * z + PHASOR_C8) * z + PHASOR_C6) * z + PHASOR_C4) * z + PHASOR_C2;
    const float s0 = x + x * (z * ps);
    const float c0 = 1.0f + z * pc;
    // cos(x + k pi/2), sin(x + k pi/2)
    c = k == 1.0f ? -s0 : k == 2.0f ? -c0 : k == 3.0f ? s0 : c0;
    s = k == 1.0f ? c0 : k == 2.0f ? -s0 : k == 3.0f ? -c0 : s0;
}

}  // namespace d2d
