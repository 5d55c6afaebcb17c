// The direction of the power-angle profile (d2d_power_angle_launch, d2d::AngleSink):  turns(dx, dy)  gives the angle of the vector
// (dx, dy), counter-clockwise from +x, in turns, 0 <= f < 1.  This text IS the definition: no atan2f of any library matches
// another bit for bit, so the angle is a fixed sequence of fp32 compares, multiplies, adds and ONE IEEE division that compiles
// for host and device alike (no HIP builtin, no library call; the build's -ffp-contract=off keeps one rounding per operation).
// tests/native/power_angle_host.cpp compiles it with g++, and tests/test_power_angle_cpu.py holds it bit for bit to a NumPy
// restatement and, in accuracy, to float64.
//
//   magnitudes  ax = |dx|, ay = |dy| by compares (x < 0 ? -x : x == 0 ? +0 : x): -0.0 counts as +0.0
//               mx = max(ax, ay), mn = min(ax, ay);  swap = ay > ax  (the angle is measured from the y axis)
//               mx >= 1e38: both are multiplied by 1/4 (exact for mx; an mn this loses bits of gives q = 0 anyway), so that
//               mx + mn below cannot overflow.  No squares anywhere.
//   reduce      near = mn + mn > mx            (exact compare: q = mn / mx > 1/2, the direction is nearer the diagonal)
//               q = near ? (mx - mn) / (mx + mn) : mn / mx          the one division; q in [0, 1/2] resp. [0, 1/3]
//               (tan(pi/4 - a) = (1 - tan a) / (1 + tan a): the angle from the diagonal)
//   evaluate    p = q * P(q^2) ~ atan(q) / 2 pi,  P of degree 5 in q^2, Horner, fixed order;  0 <= p <= 0.0738
//   rebuild     f = B + p  or  B - p,  B a multiple of 1/8 picked by (swap, near, dx < 0, dy < 0): one rounding, and exact
//               wherever p == 0 -- the axes (mn == 0) and the diagonals (mx == mn).  f >= 1 (B = 1 and p rounded away) is 0.
//
//   first quadrant      !swap, !near: 0 + p      !swap, near: 1/8 - p      swap, near: 1/8 + p      swap, !near: 1/4 - p
//   dx < 0              B -> 1/2 - B, the sign flips;      then dy < 0:  B -> 1 - B, the sign flips
//
// Exact by bits: (+x, +-0) -> 0, (0, +y) -> 0.25, (-x, +-0) -> 0.5, (0, -y) -> 0.75, |dx| == |dy| -> 0.125, 0.375, 0.625, 0.875;
// never 1.0.  (0, 0) and any NaN or infinite component give NaN; every other input, denormals and 1e30 included, a finite result.
//
// Accuracy against float64 atan2 / 2 pi, over 2^24 random directions of all octants (magnitudes 1e-6 .. 1e6), every fp32 q = mn / mx
// of the binades [1/4, 1/2) and [1/2, 1] (the two sides of the reduction boundary, and the diagonal) in all eight octants, and the
// exact cases: the absolute error, taken on the circle (0 for 1 - tiny is near, not a turn away), stays below 0.75 * 2^-24 turn --
// measured maximum 0.701 * 2^-24 (random), 0.677 and 0.664 (the binades), 0.687 (the bit-for-bit input set with its denormals).
// Half a unit is the last rounding of a result in [1/2, 1), the rest the division's and the polynomial's roundings at p <= 0.074;
// the polynomial's own error is 0.05.  4096 bins are 2^-12 turn wide.  The one compiler builtin is the NaN constant.
#pragma once

namespace d2d {

constexpr float ANGLE_HUGE = 1.0e38f;
// P(z) ~ atan(sqrt z) / (2 pi sqrt z) on [0, 1/4]: Chebyshev interpolant of degree 5, highest power first (decimal literals, so
// that any restatement reads the same fp32)
constexpr float ANGLE_P5 = -8.063173853e-03f, ANGLE_P4 = 1.609935798e-02f, ANGLE_P3 = -2.254311182e-02f, ANGLE_P2 = 3.182001412e-02f,
                ANGLE_P1 = -5.305141583e-02f, ANGLE_P0 = 1.591549367e-01f;

// |x| by compares: -0.0 becomes +0.0, NaN stays NaN
__attribute__((always_inline)) constexpr float angle_abs(float x) { return x < 0.0f ? -x : (x == 0.0f ? 0.0f : x); }

// atan(q) / 2 pi for 0 <= q <= 1/2
__attribute__((always_inline)) constexpr float angle_poly(float q) {
    const float z = q * q;
    const float P = ((((ANGLE_P5 * z + ANGLE_P4) * z + ANGLE_P3) * z + ANGLE_P2) * z + ANGLE_P1) * z + ANGLE_P0;
    return q * P;
}

// the angle of (dx, dy) in turns, [0, 1); NaN for (0, 0) and for any NaN or infinite component
__attribute__((always_inline)) constexpr float turns(float dx, float dy) {
    float ax = angle_abs(dx), ay = angle_abs(dy);
    const bool swap = ay > ax;
    float mx = swap ? ay : ax, mn = swap ? ax : ay;
    const bool ok = (ax <= 3.4028235e38f) && (ay <= 3.4028235e38f) && (mx > 0.0f);  // finite, not both zero (NaN fails the compares)
    if (mx >= ANGLE_HUGE) {
        mx = mx * 0.25f;
        mn = mn * 0.25f;
    }
    const bool near = mn + mn > mx;
    const float num = near ? mx - mn : mn;
    const float den = near ? mx + mn : mx;
    const float q = num / den;
    const float p = angle_poly(q);
    // the multiple of 1/8 the small angle p is measured from, and the direction it is measured in
    float B = swap ? (near ? 0.125f : 0.25f) : (near ? 0.125f : 0.0f);
    bool plus = swap == near;
    if (dx < 0.0f) {
        B = 0.5f - B;
        plus = !plus;
    }
    if (dy < 0.0f) {
        B = 1.0f - B;
        plus = !plus;
    }
    float f = plus ? B + p : B - p;
    if (f >= 1.0f) f = 0.0f;
    return ok ? f : __builtin_nanf("");
}

}  // namespace d2d
