// The per-contribution arithmetic of the frequency response's position adjoint (d2d_field_position_vjp_launch, d2d::PosGradSink):
// dL/dr of one path for one block of POS_CHUNK wavelengths.  For hard validity and image paths a position enters the frequency
// response through the path length r alone (validity is piecewise constant, every fused path function is a function of r), and by
// Fermat's principle the interaction points are stationary:  d r / d p[0] = -unit(p[1] - p[0]),  d r / d p[K+1] = -unit(p[K] - p[K+1]).
// So the gradient with respect to an end point is  -(dL/dr) * unit(direction at that end),  and dL/dr is what this header forms.
// This text IS the definition: a fixed sequence of fp32 multiplies, adds, compares, IEEE sqrt, IEEE division and floor that compiles
// for host and device alike (the build's -ffp-contract=off keeps one rounding per operation; the device build's
// -fhip-fp32-correctly-rounded-divide-sqrt makes sqrt and division IEEE).  tests/native/field_position_vjp_host.cpp compiles it with
// g++, and tests/test_field_position_vjp_cpu.py holds it bit for bit to a NumPy restatement (tests/field_position_vjp_oracle.py).
//
// Per contribution t = valid * fun that is not exactly zero, with path length r, cotangents rb[j], ib[j] and the block's inv[j]:
//
//   a   = posgrad_amp(amplitude, t)         amplitude == SQRT ? copysignf(sqrtf(fabsf(t)), t) : t            // the frequency response's
//   rho = posgrad_rho(fun_id, h2, r)        RECEIVED_POWER, RECEIVED_POWER_PER_OBJECT: -(2.0f*r) / (h2 + r*r)   // (d fun/d r) / fun
//                                           LENGTH_SQUARED: 2.0f / r ;  LENGTH: 1.0f / r ;  ONE (and anything else): +0.0f
//   kr  = posgrad_kr(amplitude, rho)        amplitude == SQRT ? 0.5f * rho : rho                                // (d a/d r) / a
//   g   = +0.0f
//   for j in the block, in order:  g = posgrad_fold(g, kr, r, inv[j], rb[j], ib[j])
//           u = r * inv[j] ; f0 = u - floorf(u) ; (c, s) = phasor(f0) ; w = TWO_PI * inv[j]      // TWO_PI = 6.2831855f
//           pr = kr*c - w*s ;  pi = kr*s + w*c             // d(a e^(-j 2 pi r / lambda))/dr = a (pr - j pi)
//           g  = g + (rb[j]*pr - ib[j]*pi)
//   G   = a * g                                            // dL/dr of this path, this block
//
// Every product and every add above is one stated operation.  A coefficient of RECEIVED_POWER_PER_OBJECT does not depend on r, so
// its rho is RECEIVED_POWER's.  r = 0 (a cell on the fixed end point) gives rho = -0 / h2 for the received powers and an infinite rho
// for the two lengths, whose t is zero there and never comes this far.
#pragma once

#include <cmath>

#include "../../include/d2d.h"
#include "d2d_phasor.hpp"

#if defined(__HIPCC__)
#define D2D_POSGRAD_FN __host__ __device__ __attribute__((always_inline)) inline
#else
#define D2D_POSGRAD_FN __attribute__((always_inline)) inline
#endif

namespace d2d {

constexpr int POS_CHUNK = D2D_POS_CHUNK;  // wavelengths per pass: part of the definition (a block's G is rounded once)
constexpr float POSGRAD_TWO_PI = 6.2831855f;

// the amplitude of a contribution: the frequency response's own
D2D_POSGRAD_FN float posgrad_amp(int amplitude, float t) { return field_amp(amplitude == D2D_FIELD_AMP_SQRT, t); }

// (d fun / d r) / fun of the fused path functions
D2D_POSGRAD_FN float posgrad_rho(int fun_id, float h2, float r) {
    if (fun_id == D2D_FUN_RECEIVED_POWER || fun_id == D2D_FUN_RECEIVED_POWER_PER_OBJECT) {
        const float two_r = 2.0f * r, rr = r * r;
        const float d = h2 + rr;
        return -two_r / d;
    }
    if (fun_id == D2D_FUN_LENGTH_SQUARED) return 2.0f / r;
    if (fun_id == D2D_FUN_LENGTH) return 1.0f / r;
    return 0.0f;
}

// (d a / d r) / a
D2D_POSGRAD_FN float posgrad_kr(int amplitude, float rho) { return amplitude == D2D_FIELD_AMP_SQRT ? 0.5f * rho : rho; }

// one wavelength's step of the fold: g + (rb * pr - ib * pi)
D2D_POSGRAD_FN float posgrad_fold(float g, float kr, float r, float inv, float rb, float ib) {
    float c, s;
    phasor(turn_fraction(r, inv), c, s);
    const float w = POSGRAD_TWO_PI * inv;
    const float krc = kr * c, ws = w * s, krs = kr * s, wc = w * c;
    const float pr = krc - ws, pi = krs + wc;
    const float rp = rb * pr, ip = ib * pi;
    return g + (rp - ip);
}

}  // namespace d2d
