// The Fresnel reflection coefficient of the material response (d2d_material_response_launch, d2d::MaterialSink): what a wall does to
// the complex amplitude of a path that it reflects, as a function of the angle of incidence, the polarisation and the wall's complex
// relative permittivity.  This text IS the definition: a fixed sequence of fp32 multiplies, adds, compares, IEEE sqrt and IEEE
// division that compiles for host and device alike (the build's -ffp-contract=off keeps one rounding per operation; the device
// build's -fhip-fp32-correctly-rounded-divide-sqrt makes sqrt and division IEEE).  tests/native/material_response_host.cpp compiles
// it with g++, and tests/test_material_response_cpu.py holds it bit for bit to a NumPy restatement and, in accuracy, to float64.
//
// The time convention is the library's, e^(-j 2 pi r / lambda): a lossy medium is eps = eps' - j eps'', Im eps <= 0.
//
//   fresnel(er, ei, c, pol) -> (gr, gi)       (er, ei) the permittivity, c the cosine of the angle of incidence in [0, 1],
//                                             pol = D2D_POL_TE (0): E perpendicular to the plane of incidence -- for vertical
//                                             antennas over a 2-D floor plan E out of the plane, the natural case here --
//                                             or D2D_POL_TM (1): E in the plane of incidence
//       if (c > 1) c = 1                                              // a NaN c stays NaN and gives (NaN, NaN)
//       wr = (er - 1) + c*c ; wi = ei                                 // w = eps - sin^2(theta), without forming sin^2
//       m  = sqrtf(wr*wr + wi*wi)
//       if (m == 0)        q = (0, 0)                                 // q = sqrt(w), the branch with Im q <= 0 (the decaying one)
//       else if (wr >= 0)  qr = sqrtf(0.5f*(m + wr)) ; qi = wi / (2.0f*qr)
//       else               qi = -sqrtf(0.5f*(m - wr)) ; qr = wi / (2.0f*qi)      // also for ei = +-0: total reflection, |G| = 1
//       TE: a = (c, 0)            TM: a = (er*c, ei*c)
//       n = a - q ; d = a + q ; den = d.re*d.re + d.im*d.im
//       if (den == 0)      (gr, gi) = (-1, 0)                         // the grazing limit
//       else               gr = (n.re*d.re + n.im*d.im) / den ; gi = (n.im*d.re - n.re*d.im) / den
//
// TE is (cos - sqrt(eps - sin^2)) / (cos + sqrt(eps - sin^2)), TM is (eps cos - sqrt(..)) / (eps cos + sqrt(..)): at normal
// incidence TE = (1 - sqrt(eps)) / (1 + sqrt(eps)) and TM is its negative (the sign convention that keeps TM's field component along
// the wall; TM goes through zero at the Brewster angle, cos = 1 / sqrt(1 + eps), for real eps).  Neither square root sees a
// difference of near-equal numbers: m + wr with wr >= 0 and m - wr with wr < 0 are sums of like signs.
//
// eps - sin^2 is formed as (er - 1) + c*c: 1 - c*c would round at the scale of 1 and then cancel against an er near 1 (errors of
// tens of thousands of units near grazing incidence); er - 1 is exact for er in [0.5, 2].  eps = 1 gives exactly (0, +-0) wherever
// c*c is exact (c = 1, c = 0.5): w = c*c, q = c, n = 0.  er < sin^2 with ei = +-0 gives |G| = 1.
// Components of eps up to 2^50 in magnitude stay finite in both polarisations (the largest intermediate is 2^101).
//
// Accuracy against the float64 formula over er in [1.5, 100], -ei in [0, 1000], c in [1e-3, 1], both polarisations: the absolute
// error of either component stays below 5.25 * 2^-24 (measured maximum 4.79 * 2^-24 over 2^20 seeded points, TE 3.94 and TM 4.79;
// tests/test_material_response_cpu.py).  With er within 1e-3 of 1 and no loss, near grazing incidence -- where 1 - c*c would cancel
// -- the same test reports 2.7 * 2^-24; that corner is reported, not bounded.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define D2D_FRESNEL_FN __host__ __device__ __attribute__((always_inline)) inline
#else
#define D2D_FRESNEL_FN __attribute__((always_inline)) inline
#endif

namespace d2d {

constexpr int POL_TE = 0, POL_TM = 1;  // = D2D_POL_TE / D2D_POL_TM (include/d2d.h)

// q = sqrt(wr + j wi) with Im q <= 0
D2D_FRESNEL_FN void fresnel_root(float wr, float wi, float& qr, float& qi) {
    const float rr = wr * wr, ii = wi * wi;
    const float m = sqrtf(rr + ii);
    if (m == 0.0f) {
        qr = 0.0f;
        qi = 0.0f;
    } else if (wr >= 0.0f) {
        qr = sqrtf(0.5f * (m + wr));
        qi = wi / (2.0f * qr);
    } else {
        qi = -sqrtf(0.5f * (m - wr));
        qr = wi / (2.0f * qi);
    }
}

// the reflection coefficient of a half space of permittivity (er, ei) at cos(angle of incidence) = c
D2D_FRESNEL_FN void fresnel(float er, float ei, float c, int pol, float& gr, float& gi) {
    if (c > 1.0f) c = 1.0f;
    const float cc = c * c;
    const float wr = (er - 1.0f) + cc;
    float qr, qi;
    fresnel_root(wr, ei, qr, qi);
    const float ar = pol == POL_TM ? er * c : c;
    const float ai = pol == POL_TM ? ei * c : 0.0f;
    const float nr = ar - qr, ni = ai - qi;
    const float dr = ar + qr, di = ai + qi;
    const float drr = dr * dr, dii = di * di;
    const float den = drr + dii;
    if (den == 0.0f) {
        gr = -1.0f;
        gi = 0.0f;
    } else {
        const float p0 = nr * dr, p1 = ni * di, p2 = ni * dr, p3 = nr * di;
        gr = (p0 + p1) / den;
        gi = (p2 - p3) / den;
    }
}

// G <- G * g
D2D_FRESNEL_FN void fresnel_fold(float& Gr, float& Gi, float gr, float gi) {
    const float a = Gr * gr, b = Gi * gi, c = Gr * gi, d = Gi * gr;
    Gr = a - b;
    Gi = c + d;
}

// G e^(-j 2 pi f0) = zr - j zs, with (c0, s0) = phasor(f0)
D2D_FRESNEL_FN void fresnel_turn(float Gr, float Gi, float c0, float s0, float& zr, float& zs) {
    const float a = Gr * c0, b = Gi * s0, c = Gr * s0, d = Gi * c0;
    zr = a + b;
    zs = c - d;
}

}  // namespace d2d
