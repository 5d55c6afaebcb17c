// The steering arithmetic of the array response (d2d_array_response_launch, d2d::ArraySink): the channel matrix between a transmit
// array at p[0] and a receive array at p[K+1] under the plane-wave (far-field) model.  This text IS the definition: a fixed sequence
// of fp32 multiplies, adds, compares, IEEE sqrt, IEEE division and floor that compiles for host and device alike (the build's
// -ffp-contract=off keeps one rounding per operation; the device build's -fhip-fp32-correctly-rounded-divide-sqrt makes sqrt and
// division IEEE).  tests/native/array_response_host.cpp compiles it with g++, and tests/test_array_response_cpu.py holds it bit for
// bit to a NumPy restatement.
//
// Per cell, with element offsets etx[nt], erx[nr] (length units, from the terminal's position), all in fp32:
//
//   total = +0.0f ; re[i][j] = im[i][j] = +0.0f
//   for candidates in the sweep's enumeration order:
//       t = valid * fun ; r = path_length(points)          // as the coherent field gets them
//       total = total + t                                   // the fused map bit for bit
//       if (t == 0) continue
//       a  = amplitude == SQRT ? copysignf(sqrtf(fabsf(t)), t) : t
//       u  = r * inv_wavelength ; f0 = u - floorf(u)        // exactly the coherent field's phase
//       (utx, uty, okt) = unit_dir(p[1]-p[0]) ; (urx, ury, okr) = unit_dir(p[K]-p[K+1])
//       if (!(okt && okr)) continue                         // a path without a direction at an end enters no pair (total has it)
//       for j < nt: qt = steer_dot(etx[j], utx, uty)
//         for i < nr: qr = steer_dot(erx[i], urx, ury)
//           f = steer_phase(f0, qt, qr, inv_wavelength)
//           (c, s) = phasor(f)                              // d2d_phasor.hpp
//           re[i][j] = re[i][j] + a * c ; im[i][j] = im[i][j] - a * s
//
//   unit_dir(dx, dy)         n = sqrtf(dx * dx + dy * dy) ;  ok = n > 0 && n <= FLT_MAX ;  ux = dx / n ;  uy = dy / n
//                            (a zero, NaN or infinite n -- squares that overflow included -- gives ok = false; squares that
//                            underflow to a zero n likewise.  ux, uy are then whatever the divisions give and are not used.)
//   steer_dot(ex, ey, ux, uy)      ex * ux + ey * uy           two products, one sum
//   steer_phase(f0, qt, qr, inv)   w = (qt + qr) * inv ;  v = f0 - w ;  f = v - floorf(v) ;  if (f >= 1.0f) f = 0.0f
//                            the phase of the pair in turns, (r - etx . utx - erx . urx) / wavelength mod 1.  v - floorf(v) is in
//                            [0, 1] for every finite v: a v just below zero (f0 = 0, w = 1e-9) gives -tiny + 1, which rounds to 1;
//                            the clamp takes it to 0, the same point of the circle, so that the phasor's 0 <= f < 1 holds.  A NaN
//                            or infinite v gives NaN (and a NaN phasor).
//
// Offsets of (+-0, +-0) at both ends give qt = qr = +-0, w = +-0, v = f0 and f = f0 - floorf(f0) = f0 for f0 in [0, 1): the pair
// is, bit for bit, the coherent field's contribution.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define D2D_STEER_FN __host__ __device__ __attribute__((always_inline)) inline
#else
#define D2D_STEER_FN __attribute__((always_inline)) inline
#endif

namespace d2d {

constexpr float STEER_FLT_MAX = 3.4028235e38f;

// the unit vector of (dx, dy); false where it has none (zero, NaN, infinite or overflowing length)
D2D_STEER_FN bool unit_dir(float dx, float dy, float& ux, float& uy) {
    const float xx = dx * dx, yy = dy * dy;
    const float n = sqrtf(xx + yy);
    ux = dx / n;
    uy = dy / n;
    return n > 0.0f && n <= STEER_FLT_MAX;
}

// an element offset along a unit direction, in length units
D2D_STEER_FN float steer_dot(float ex, float ey, float ux, float uy) {
    const float a = ex * ux, b = ey * uy;
    return a + b;
}

// the phase of one antenna pair in turns, [0, 1) (NaN for a NaN or infinite input)
D2D_STEER_FN float steer_phase(float f0, float qt, float qr, float inv) {
    const float w = (qt + qr) * inv;
    const float v = f0 - w;
    float f = v - floorf(v);
    if (f >= 1.0f) f = 0.0f;
    return f;
}

}  // namespace d2d
