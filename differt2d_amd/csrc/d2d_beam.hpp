// The beamforming arithmetic of the beam-space response (d2d_beam_response_launch, d2d::BeamSink): what comes out behind a codebook
// of transmit beams and a codebook of receive beams, y = w_rx^H H w_tx, per cell, wavelength and beam pair, without ever forming the
// channel matrix H.  Under the plane-wave model of d2d_steer.hpp every path's contribution to H has rank one,
//     a e^(-j 2 pi r / lambda) * s_rx s_tx^T      with  s[k] = e^(+j 2 pi q_k / lambda),  q_k = steer_dot(e[k], u),
// so that  w_rx^H H w_tx = sum over paths of  a e^(-j 2 pi r / lambda) * (sum_i conj(w_rx[i]) s_rx[i]) * (sum_j w_tx[j] s_tx[j]):
// nt + nr + 1 phasors per contribution and wavelength where the channel matrix takes nr * nt.  This text IS the definition: a fixed
// sequence of fp32 multiplies, adds, compares and floor that compiles for host and device alike (the build's -ffp-contract=off keeps
// one rounding per operation).  tests/native/beam_response_host.cpp compiles it with g++, and tests/test_beam_response_cpu.py holds
// it bit for bit to a NumPy restatement (tests/beam_response_oracle.py).
//
// Per cell, with element offsets etx[nt], erx[nr], weights tx_weights[nbt][nt], rx_weights[nbr][nr] (complex, (re, im) pairs) and the
// list inv_wavelength[nf], all in fp32, one rounding per operation, no contraction, candidates in the sweep's enumeration order:
//
//   total = +0.0f ; re[f][br][bt] = im[f][br][bt] = +0.0f
//   for candidates:
//       t = valid * fun ; r = path_length(points)            // as the wideband array response gets them
//       total = total + t                                     // the fused map, bit for bit
//       if (t == 0) continue
//       a = amplitude == SQRT ? copysignf(sqrtf(fabsf(t)), t) : t
//       (utx, uty, okt) = unit_dir(p[1]-p[0]) ; (urx, ury, okr) = unit_dir(p[K]-p[K+1])     // d2d_steer.hpp, unchanged
//       if (!(okt && okr)) continue
//       for f < nf:
//           inv = inv_wavelength[f] ; u = r * inv ; f0 = u - floorf(u) ; (c0, s0) = phasor(f0)
//           steer(q):  v = q * inv ; g = v - floorf(v) ; if (g >= 1.0f) g = 0.0f ; (c, s) = phasor(g)      // e^(+j 2 pi q / lambda) = c + j s
//           for bt < nbt:  At = (+0, +0) ; for j < nt in order:  (c, s) = steer(steer_dot(etx[j], utx, uty)) ; w = tx_weights[bt][j]
//                              At.re = At.re + (w.re * c - w.im * s) ;  At.im = At.im + (w.re * s + w.im * c)
//           for br < nbr:  Ar = (+0, +0) ; for i < nr in order:  (c, s) = steer(steer_dot(erx[i], urx, ury)) ; w = rx_weights[br][i]
//                              Ar.re = Ar.re + (w.re * c + w.im * s) ;  Ar.im = Ar.im + (w.re * s - w.im * c)       // conj(w) * steer
//           for (br, bt):  P.re = Ar.re * At.re - Ar.im * At.im ;  P.im = Ar.re * At.im + Ar.im * At.re
//                          zr = P.re * c0 + P.im * s0 ;  zs = P.re * s0 - P.im * c0                                  // P e^(-j 2 pi f0) = zr - j zs
//                          re[f][br][bt] = re[f][br][bt] + a * zr ;  im[f][br][bt] = im[f][br][bt] - a * zs
//
// Every parenthesised product and every add above is one stated operation, so the bits do not depend on how a kernel nests the loops
// or on what it recomputes.
//
// Properties:
//   Total.         total is the fused map, bit for bit.
//   Independence.  Plane (f, br, bt) depends only on inv_wavelength[f], row br of rx_weights, row bt of tx_weights and the two element
//                  lists.  Permuted, duplicated or truncated wavelength or beam lists give permuted, equal or leading planes, bit for
//                  bit.  The element order is part of the definition: the array factors are left folds.
//   One antenna.   nt = nr = nbt = nbr = 1, offsets (+-0, +-0) and weights (1, 0) give the planes of d2d_frequency_response_launch, bit
//                  for bit, wherever no contribution lacks a direction and no contribution is NaN: steer(+-0) is phasor(+0) = (1, +0)
//                  exactly (v = +-0, g = +0), so At = Ar = P = (1, +0), zr = c0 and zs = s0 as values, and an accumulator that starts
//                  at +0 never holds -0, so the signs of zero that the products of zero leave behind are absorbed.
//   Element space. Against the float64 contraction conj(w_rx) . H . w_tx of d2d_array_frequency_response_launch's planes the beam planes
//                  agree within a derived bound (tests/beam_response_oracle.py), not bit for bit: the element-space phase rounds
//                  (qt + qr) * inv once where the three phasors here round f0, qt * inv and qr * inv separately.
#pragma once

#include <cmath>

#include "d2d_phasor.hpp"

#if defined(__HIPCC__)
#define D2D_BEAM_FN __host__ __device__ __attribute__((always_inline)) inline
#else
#define D2D_BEAM_FN __attribute__((always_inline)) inline
#endif

namespace d2d {

// steer: e^(+j 2 pi q * inv) = c + j s for an element's offset q along the path's direction (length units) and inv turns per unit length
D2D_BEAM_FN void beam_steer(float q, float inv, float& c, float& s) {
    const float v = q * inv;
    float g = v - floorf(v);
    if (g >= 1.0f) g = 0.0f;
    phasor(g, c, s);
}

// one step of the transmit fold: At = At + w * (c + j s)
D2D_BEAM_FN void beam_fold_tx(float& at_re, float& at_im, float w_re, float w_im, float c, float s) {
    const float rc = w_re * c, is = w_im * s, rs = w_re * s, ic = w_im * c;
    at_re = at_re + (rc - is);
    at_im = at_im + (rs + ic);
}

// one step of the receive fold: Ar = Ar + conj(w) * (c + j s)
D2D_BEAM_FN void beam_fold_rx(float& ar_re, float& ar_im, float w_re, float w_im, float c, float s) {
    const float rc = w_re * c, is = w_im * s, rs = w_re * s, ic = w_im * c;
    ar_re = ar_re + (rc + is);
    ar_im = ar_im + (rs - ic);
}

// the pair product rotated by the path's phase: P = Ar * At, P e^(-j 2 pi f0) = zr - j zs with (c0, s0) = phasor(f0)
D2D_BEAM_FN void beam_pair(float ar_re, float ar_im, float at_re, float at_im, float c0, float s0, float& zr, float& zs) {
    const float rr = ar_re * at_re, ii = ar_im * at_im, ri = ar_re * at_im, ir = ar_im * at_re;
    const float p_re = rr - ii, p_im = ri + ir;
    const float pc = p_re * c0, qs = p_im * s0, ps = p_re * s0, qc = p_im * c0;
    zr = pc + qs;
    zs = ps - qc;
}

}  // namespace d2d
