// Division of a 32-bit index by a divisor that is fixed when a sweep is launched (patches per grid row, patches per region
// side).  The host prepares the divisor once (make_div), the kernels divide with a shift (powers of two: the default region
// size and every grid whose width is 8 times one) or with one multiply-high and one correction step -- a run-time integer
// division is ~22 scalar instructions and a trip through the vector unit (v_rcp_iflag) on gfx9, per wave.
//
// Exactness (divmod, d not a power of two, so d >= 3): mul = floor(2^32 / d), hence 2^32 / d - 1 < mul <= 2^32 / d and, for
// every n < 2^32,  n / d - 1 < n * mul / 2^32 <= n / d.  The estimate q' = floor(n * mul / 2^32) is therefore q or q - 1
// (q = floor(n / d)), the remainder n - q' d lies in [0, 2 d), and one conditional step mends it.  2 d fits 32 bits for
// d < 2^31; a larger d only ever meets n < d here (q' = 0: mul is 1, and n < 2^32 <= 2 d keeps the remainder in range).
// tests/native/d2d_div_main.cpp holds both paths to the hardware division over the edge values, on the host; the functions
// are constexpr so that the same text compiles for the device.
#pragma once
#include <stdint.h>

namespace d2d {

struct DivU32 {
    uint32_t d;      // the divisor (>= 1)
    uint32_t mul;    // floor(2^32 / d), or 0: d == 1 << shift
    uint32_t shift;
};

constexpr DivU32 make_div(uint32_t d) {
    DivU32 v = {d ? d : 1u, 0u, 0u};
    if ((v.d & (v.d - 1u)) == 0u) {
        while ((1u << v.shift) != v.d) ++v.shift;
    } else {
        v.mul = (uint32_t)((1ull << 32) / v.d);
    }
    return v;
}

// q = n / v.d, r = n % v.d  (always inlined: the operands are wave-uniform scalars in the kernels, which a call would pass in
// vector registers)
__attribute__((always_inline)) constexpr void divmod(const DivU32& v, uint32_t n, uint32_t& q, uint32_t& r) {
    if (v.mul == 0u) {
        q = n >> v.shift;
        r = n & (v.d - 1u);
    } else {
        q = (uint32_t)(((uint64_t)n * v.mul) >> 32);
        r = n - q * v.d;
        if (r >= v.d) {
            ++q;
            r -= v.d;
        }
    }
}

__attribute__((always_inline)) constexpr uint32_t div_by(const DivU32& v, uint32_t n) {
    uint32_t q = 0, r = 0;
    divmod(v, n, q, r);
    return q;
}

}  // namespace d2d
