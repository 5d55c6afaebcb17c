// The derivative of the Fresnel reflection coefficient with respect to the wall's complex permittivity, for the permittivity
// adjoint of the material response (d2d_material_eps_vjp_launch, d2d::EpsGradSink).  G(eps) is holomorphic in eps, so the one
// complex number dG/deps carries both dG/dRe eps (= dG/deps) and dG/dIm eps (= j dG/deps).  This text IS the definition, as
// d2d_fresnel.hpp is the coefficient's: a fixed sequence of fp32 multiplies, adds, compares, IEEE sqrt and IEEE division that
// compiles for host and device alike (-ffp-contract=off: one rounding per operation).  tests/native/material_eps_vjp_host.cpp
// compiles it with g++, and tests/test_material_eps_vjp_cpu.py holds it bit for bit to a NumPy restatement and, in accuracy, to
// float64.
//
//   fresnel_grad(er, ei, c, pol) -> (gr, gi, dr, di, ok)
//       if (c > 1) c = 1                                              // a NaN c stays NaN: (NaN, NaN), (NaN, NaN), ok true
//       cc = c*c ; wr = (er - 1) + cc ; wi = ei ; m = sqrtf(wr*wr + wi*wi) ; q = fresnel_root(wr, wi)      // d2d_fresnel.hpp
//       TE: a = (c, 0)            TM: a = (er*c, ei*c)
//       n = a - q ; s = a + q ; den = s.re*s.re + s.im*s.im
//       (gr, gi) = den == 0 ? (-1, 0) : ((n.re*s.re + n.im*s.im) / den, (n.im*s.re - n.re*s.im) / den)   // fresnel()'s operations: its bits
//       ok = !(m == 0) && !(den == 0) ;  if (!ok) (dr, di) = (+0, +0), and what follows is not evaluated
//       id = 1 / den ; u = (s.re*id, -(s.im*id))                      // u = 1 / s
//       u2 = (u.re*u.re - u.im*u.im, 2*(u.re*u.im))                   // 1 / s^2
//       qq = q.re*q.re + q.im*q.im ; iq = 1 / qq ; v = (q.re*iq, -(q.im*iq))      // v = 1 / q
//       TE: num = (-c, 0)         TM: t = (er - 2) + (cc + cc) ; num = (c*t, c*ei)           // c * (eps - 2 + 2 c^2)
//       p = (num.re*v.re - num.im*v.im, num.re*v.im + num.im*v.re)
//       (dr, di) = (p.re*u2.re - p.im*u2.im, p.re*u2.im + p.im*u2.re)
//
// With q = sqrt(eps - 1 + c^2) on fresnel_root's branch Im q <= 0 and dq/deps = 1 / (2 q):
//   TE: G = (c - q) / (c + q)           dG/deps = -c / (q (c + q)^2)
//   TM: G = (eps c - q) / (eps c + q)   dG/deps = c (2 q^2 - eps) / (q (eps c + q)^2) = c (eps - 2 + 2 c^2) / (q (eps c + q)^2)
//
// eps - 2 + 2 c^2 is formed as (er - 2) + (c*c + c*c): er - 2 is exact for er in [1, 4] (the operands are within a factor 2 of
// each other) and the doubling is exact, so the sum's own rounding, relative to the result, is the only one -- nothing is rounded at
// the scale of 1 or of er and then cancelled, against an er near 1 or otherwise.  What remains near the zero of the numerator
// (er = 2 - 2 c^2, inside the domain) is the rounding of c*c itself, which no ordering removes.  (er - 1) + ((c*c - 1) + c*c), the
// forward header's pattern, rounds c*c - 1 at the scale of 1 wherever c*c < 0.5: 29.0 units in the numerator over the points below,
// against 2.8.)
//
// The quotient is taken as num * (1/q) * (1/s)^2 with two reciprocals, not as num / (q s^2): |q s^2|^2 leaves fp32 for |eps| above
// 2^25, the factors do not -- components of eps up to 2^50 in magnitude, what the launch accepts, give finite values in both
// polarisations (1/s^2 is then 2^-100 at the least; the result may underflow to zero, where it is below 2^-126 in truth).
//
// ok is false, and (dr, di) = (+0, +0), where G is defined by a special case and not by the formula: m == 0 (q = 0: G has a
// square-root singularity there, no derivative) and den == 0 (the grazing limit, G = -1).
//
// On the cut (ei = +-0 with er < sin^2: total reflection) q is taken on the branch reached from Im eps <= 0, so the derivative is the
// one-sided one from Im eps <= 0; d2d_material_eps_vjp_launch refuses Im eps > 0 as the forward product does.
//
// Accuracy against the float64 formula over the forward header's domain, er in [1.5, 100], -ei in [0, 1000], c in [1e-3, 1] (q is
// bounded away from 0 there: |q|^2 >= 0.5), both polarisations: |d32 - d64| / |d64| stays below DFRESNEL_BOUND = 14.0 * 2^-24
// (tests/material_eps_vjp_oracle.py; measured maximum 13.28 * 2^-24 over 2^20 seeded points, TE 13.28 and TM 11.95;
// tests/test_material_eps_vjp_cpu.py).  The derivative holds q and s = a + q to the third power together, so it carries about three
// times their error of 3 to 4 units; num / (q s^2) with one division measures the same.
#pragma once

#include "d2d_fresnel.hpp"

namespace d2d {

D2D_FRESNEL_FN void fresnel_grad(float er, float ei, float c, int pol, float& gr, float& gi, float& dr, float& di, bool& ok) {
    if (c > 1.0f) c = 1.0f;
    const float cc = c * c;
    const float wr = (er - 1.0f) + cc;
    const float rr = wr * wr, ii = ei * ei;
    const float m = sqrtf(rr + ii);  // (fresnel_root's own m: the same operations)
    float qr, qi;
    fresnel_root(wr, ei, qr, qi);
    const bool tm = pol == POL_TM;
    const float ar = tm ? er * c : c;
    const float ai = tm ? ei * c : 0.0f;
    const float nr = ar - qr, ni = ai - qi;
    const float sr = ar + qr, si = ai + qi;
    const float srr = sr * sr, sii = si * si;
    const float den = srr + sii;
    dr = 0.0f;
    di = 0.0f;
    if (den == 0.0f) {
        gr = -1.0f;
        gi = 0.0f;
        ok = false;
        return;
    }
    const float p0 = nr * sr, p1 = ni * si, p2 = ni * sr, p3 = nr * si;
    gr = (p0 + p1) / den;
    gi = (p2 - p3) / den;
    ok = !(m == 0.0f);
    if (!ok) return;
    const float id = 1.0f / den;
    const float ur = sr * id, ui = -(si * id);
    const float urr = ur * ur, uii = ui * ui, uri = ur * ui;
    const float u2r = urr - uii, u2i = 2.0f * uri;
    const float qrr = qr * qr, qii = qi * qi;
    const float qq = qrr + qii;
    const float iq = 1.0f / qq;
    const float vr = qr * iq, vi = -(qi * iq);
    float numr, numi;
    if (tm) {
        const float t = (er - 2.0f) + (cc + cc);
        numr = c * t;
        numi = c * ei;
    } else {
        numr = -c;
        numi = 0.0f;
    }
    const float a0 = numr * vr, a1 = numi * vi, a2 = numr * vi, a3 = numi * vr;
    const float pr = a0 - a1, pi = a2 + a3;
    const float b0 = pr * u2r, b1 = pi * u2i, b2 = pr * u2i, b3 = pi * u2r;
    dr = b0 - b1;
    di = b2 + b3;
}

}  // namespace d2d
