// The per-bounce arithmetic of the frequency response's wall adjoint (d2d_field_walls_vjp_launch, d2d::WallGradSink): what one
// bounce of one path adds to the gradient with respect to the two end points of the wall it bounces off.  For hard validity and
// image paths a wall enters the frequency response through the path length r alone (validity is piecewise constant, every fused path
// function is a function of r, per-object coefficients do not depend on geometry), and by Fermat's principle the interaction points
// are stationary: the total derivative with respect to a wall's end points is the partial derivative at a fixed position along the
// wall.  For bounce i on wall w with end points A, B, T = B - A, the unit normal n = normalize((T_y, -T_x)) (what the wall table holds
// in refl[2 w].zw), u_in = unit(p[i] - p[i-1]) and the relative position s = ((p[i] - A) . T) / |T|^2:
//
//     d r / d A = gam (1 - s) n ,   d r / d B = gam s n ,   gam = 2 (u_in . n)
//
// (the reflection law u_in - u_out = 2 (u_in . n) n; the sign of n cancels).  dL/dr of the path for one block of POS_CHUNK wavelengths
// is G of d2d_posgrad.hpp, unchanged.  This text IS the definition: a fixed sequence of fp32 multiplies, adds, IEEE sqrt and IEEE
// division that compiles for host and device alike (the build's -ffp-contract=off keeps one rounding per operation; the device
// build's -fhip-fp32-correctly-rounded-divide-sqrt makes sqrt and division IEEE).  tests/native/field_walls_vjp_host.cpp compiles it
// with g++, and tests/test_field_walls_vjp_cpu.py holds it bit for bit to a NumPy restatement (tests/field_walls_vjp_oracle.py).
//
// Per contribution t = valid * fun that is not exactly zero, of a candidate with walls cand[0..K), K >= 1, and segments
// seg[i] = p[i+1] - p[i] (what MaterialSink gets), with G = posgrad_amp(..) * the fold of posgrad_fold over the block:
//
//   q = p[0]                                   // the transmitter: `fixed` on an RX grid, the cell's (X, Y) on a TX grid
//   for i in 0 .. K-1:                         // wallgrad_bounce, once per bounce
//       q = q + seg[i]                         // componentwise: the bounce point, rebuilt from the hand-outs
//       (ux, uy, ok) = unit_dir(seg[i])        // d2d_steer.hpp, unchanged
//       {ox, oy, nx, ny} = refl[2 w] ; {tx, ty, sq, _} = refl[2 w + 1] ,  w = cand[i]
//       gam = 2.0f * steer_dot(ux, uy, nx, ny)
//       s   = ((q.x - ox)*tx + (q.y - oy)*ty) / sq
//       wa  = G * gam ; Wb = wa * s ; Wa = wa - Wb          // Wa + Wb == wa: a rigid shift along n gets the whole term
//       if (ok) { row[w][0] += Wa ; row[w][1] += Wb }       // a wall that occurs twice in a candidate gets both terms
//
// Every product, add and division above is one stated operation.  A zero-length wall has n = (0, 0) and sq = 1 in the table and
// therefore adds +-0.  A bounce whose incoming segment has no unit vector (ok false) adds nothing; q still advances.
#pragma once

#include <cmath>

#include "d2d_posgrad.hpp"
#include "d2d_steer.hpp"

#if defined(__HIPCC__)
#define D2D_WALLGRAD_FN __host__ __device__ __attribute__((always_inline)) inline
#else
#define D2D_WALLGRAD_FN __attribute__((always_inline)) inline
#endif

namespace d2d {

// One bounce: advances (qx, qy) by the incoming segment (sx, sy) and forms the weights Wa, Wb of the wall's end points A and B
// along the wall's unit normal, from dL/dr = G and the wall's two table rows {ox, oy, nx, ny}, {tx, ty, sq, _}.  Returns ok: the
// incoming segment has a unit vector (the weights count only then).
D2D_WALLGRAD_FN bool wallgrad_bounce(float G, float& qx, float& qy, float sx, float sy, float ox, float oy, float nx, float ny, float tx, float ty,
                                     float sq, float& Wa, float& Wb) {
    qx = qx + sx;
    qy = qy + sy;
    float ux, uy;
    const bool ok = unit_dir(sx, sy, ux, uy);
    const float gam = 2.0f * steer_dot(ux, uy, nx, ny);
    const float dx = qx - ox, dy = qy - oy;
    const float ax = dx * tx, ay = dy * ty;
    const float s = (ax + ay) / sq;
    const float wa = G * gam;
    Wb = wa * s;
    Wa = wa - Wb;
    return ok;
}

}  // namespace d2d
