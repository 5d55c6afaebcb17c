// Stand-alone check of differt2d_amd/csrc/d2d_div.hpp (the sweeps' division by a launch-time divisor) against the hardware
// division, over the values where a reciprocal multiplication can go wrong: indices next to the multiples of the divisor,
// next to the powers of two and at the top of the range, for divisors of both kinds (shift, multiply-high + correction).
// tests/test_host_div.py builds it with g++ -fsanitize=undefined and runs it; it prints DIV-OK and the number of cases.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../differt2d_amd/csrc/d2d_div.hpp"

static unsigned long long n_cases = 0;

static bool check(const d2d::DivU32& v, uint32_t d, uint32_t n) {
    uint32_t q = 0, r = 0;
    d2d::divmod(v, n, q, r);
    ++n_cases;
    if (q != n / d || r != n % d || d2d::div_by(v, n) != n / d) {
        std::printf("FAIL d=%u n=%u: got (%u, %u), want (%u, %u)\n", d, n, q, r, n / d, n % d);
        return false;
    }
    return true;
}

int main() {
    const uint32_t top = 0x7fffffffu;  // indices are below 2^31
    std::vector<uint32_t> ds;
    for (uint32_t d = 1; d <= 4100; ++d) ds.push_back(d);  // every patch-row length up to a 32 800-cell row, every region size
    for (int k = 12; k < 31; ++k)
        for (int o = -2; o <= 2; ++o) ds.push_back((uint32_t)((int64_t)(1u << k) + o));
    for (uint32_t d : {65535u, 65537u, 46340u, 46341u, 0x55555555u, 0x2aaaaaabu, 0x7ffffffdu, 0x7ffffffeu, 0x7fffffffu, 0x80000000u,
                       0x80000001u, 0xfffffffeu, 0xffffffffu})
        ds.push_back(d);
    // constexpr: the functions are usable at compile time (and so by device code)
    static_assert(d2d::make_div(128).mul == 0 && d2d::make_div(128).shift == 7 && d2d::make_div(1).shift == 0, "powers of two shift");
    static_assert(d2d::make_div(3).mul == 0x55555555u && d2d::div_by(d2d::make_div(3), 0x7fffffffu) == 0x2aaaaaaau, "reciprocal");
    static_assert(d2d::make_div(0).d == 1, "a zero divisor cannot divide: treated as 1");
    uint32_t x = 0x9e3779b9u;
    for (uint32_t d : ds) {
        const d2d::DivU32 v = d2d::make_div(d);
        if (v.d != d) return 1;
        if (((d & (d - 1)) == 0) != (v.mul == 0)) return 1;
        // 0, 1, the top of the range, around every power of two, around multiples of d spread over the range
        for (uint32_t n : {0u, 1u, 2u, top - 2, top - 1, top})
            if (!check(v, d, n)) return 1;
        for (int k = 1; k < 31; ++k)
            for (int o = -1; o <= 1; ++o)
                if (!check(v, d, (uint32_t)((int64_t)(1u << k) + o))) return 1;
        const uint32_t qmax = top / d;
        for (int i = 0; i < 48; ++i) {
            x = x * 1664525u + 1013904223u;
            const uint32_t q = i < 4 ? (uint32_t)i : (i < 8 ? qmax - (uint32_t)(i - 4) * (qmax > 4) : (qmax ? x % (qmax + 1u) : 0u));
            const uint64_t base = (uint64_t)q * d;
            for (int o = -2; o <= 2; ++o) {
                const int64_t n = (int64_t)base + o;
                if (n < 0 || n > (int64_t)top) continue;
                if (!check(v, d, (uint32_t)n)) return 1;
            }
        }
        for (int i = 0; i < 16; ++i) {
            x = x * 1664525u + 1013904223u;
            if (!check(v, d, x & top)) return 1;
        }
    }
    // small divisors exhaustively over a dense stretch at the top of the range
    for (uint32_t d : {3u, 5u, 6u, 7u, 11u, 13u, 100u, 128u, 129u, 1000u})
        for (uint32_t n = top - 200000u; n != top + 1u; ++n)
            if (!check(d2d::make_div(d), d, n)) return 1;
    std::printf("DIV-OK %llu\n", n_cases);
    return 0;
}
