// The direction of d2d_power_angle_launch's sink (differt2d_amd/csrc/d2d_angle.hpp: the kernel's own text) and the host's share of
// the launch (d2d_host.hpp: angle_params, outputs_fit with angle_bytes_per_cell), compiled with plain g++ -ffp-contract=off.  Two builds of this file by
// tests/test_power_angle_cpu.py: a shared library driven through ctypes, and -- with -DPA_MAIN -- a stand-alone program that checks
// the host functions, refusals included, and the exact cases of turns; the program is also built with
// -fsanitize=address,undefined and run.  The product compiles the very same headers into libd2d.so with hipcc, where
// d2d::AngleSink::put calls turns once per non-zero contribution and lane.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>

#include "../../differt2d_amd/csrc/d2d_host.hpp"
#include "../../differt2d_amd/csrc/d2d_angle.hpp"

namespace {
constexpr double TWO_PI = 6.283185307179586476925286766559;
// |f - atan2(dy, dx) / 2 pi| on the circle (f = 0 for a direction just below a full turn is near, not a turn away)
double turn_error(float dx, float dy, float f) {
    double want = std::atan2((double)dy, (double)dx) / TWO_PI;
    if (want < 0.0) want += 1.0;
    double e = std::fabs((double)f - want);
    return e > 0.5 ? 1.0 - e : e;
}
float from_bits(uint32_t b) {
    float f;
    std::memcpy(&f, &b, sizeof f);
    return f;
}
}  // namespace

extern "C" {

// out[i] = turns(dx[i], dy[i])
void pa_turns(long long n, const float* dx, const float* dy, float* out) {
    for (long long i = 0; i < n; ++i) out[i] = d2d::turns(dx[i], dy[i]);
}

// The largest circular error of turns against float64 atan2 / 2 pi, in turns, over every fp32 q with bits in [q_lo, q_hi] as the
// smaller component beside a larger one of 1, in all eight octants ((1, q) and (q, 1) with both signs each)
double pa_worst_over_q(uint32_t q_lo, uint32_t q_hi) {
    double worst = 0.0;
    for (uint32_t b = q_lo; b <= q_hi; ++b) {
        const float q = from_bits(b);
        for (int o = 0; o < 8; ++o) {
            const float a = (o & 1) ? -1.0f : 1.0f, c = (o & 2) ? -q : q;
            const float dx = (o & 4) ? c : a, dy = (o & 4) ? a : c;
            const double e = turn_error(dx, dy, d2d::turns(dx, dy));
            if (!(e <= worst)) worst = e;  // (a NaN sticks)
        }
    }
    return worst;
}

// The same over n given directions
double pa_worst_over(long long n, const float* dx, const float* dy) {
    double worst = 0.0;
    for (long long i = 0; i < n; ++i) {
        const double e = turn_error(dx[i], dy[i], d2d::turns(dx[i], dy[i]));
        if (!(e <= worst)) worst = e;
    }
    return worst;
}

// d2d_host.hpp's share of the launch: the status of (end, origin, nbins), and whether 4 * nbins + 4 bytes per cell fit half of the
// free device memory
int pa_angle_params(int end, float origin, int nbins) {
    std::string err;
    const int rc = d2d_host::angle_params(end, origin, nbins, err);
    return (rc == D2D_OK) == err.empty() ? rc : -1000;  // (a refusal always says why)
}
long long pa_bytes_per_cell(int nbins) { return (long long)d2d_host::angle_bytes_per_cell(nbins); }
int pa_angle_fits(long long cells, int nbins, long long mem_free, long long held) {
    return d2d_host::outputs_fit((size_t)cells, d2d_host::angle_bytes_per_cell(nbins), (size_t)mem_free, (size_t)held) ? 1 : 0;
}
}

#ifdef PA_MAIN
static int failures = 0;
#define EXPECT(x)                                                \
    do {                                                         \
        if (!(x)) {                                              \
            std::printf("line %d: %s does not hold\n", __LINE__, #x); \
            ++failures;                                          \
        }                                                        \
    } while (0)

static bool is(float got, float want) { return std::memcmp(&got, &want, sizeof got) == 0; }

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float fmax = std::numeric_limits<float>::max(), tiny = std::numeric_limits<float>::denorm_min();
    // angle_params: what is accepted ...
    EXPECT(pa_angle_params(D2D_ANGLE_AT_TX, 0.0f, 1) == D2D_OK);
    EXPECT(pa_angle_params(D2D_ANGLE_AT_RX, 0.5f, 36) == D2D_OK);
    EXPECT(pa_angle_params(D2D_ANGLE_AT_RX, std::nextafter(1.0f, 0.0f), D2D_ANGLE_BINS_MAX) == D2D_OK);
    EXPECT(pa_angle_params(D2D_ANGLE_AT_TX, -0.0f, 12) == D2D_OK);
    EXPECT(pa_angle_params(D2D_ANGLE_AT_TX, tiny, 12) == D2D_OK);
    // ... and what is refused
    EXPECT(pa_angle_params(2, 0.0f, 12) == D2D_ERR_INVALID);
    EXPECT(pa_angle_params(-1, 0.0f, 12) == D2D_ERR_INVALID);
    EXPECT(pa_angle_params(D2D_ANGLE_AT_TX, 1.0f, 12) == D2D_ERR_INVALID);
    EXPECT(pa_angle_params(D2D_ANGLE_AT_TX, -tiny, 12) == D2D_ERR_INVALID);
    EXPECT(pa_angle_params(D2D_ANGLE_AT_TX, -0.25f, 12) == D2D_ERR_INVALID);
    EXPECT(pa_angle_params(D2D_ANGLE_AT_TX, nan, 12) == D2D_ERR_INVALID);
    EXPECT(pa_angle_params(D2D_ANGLE_AT_TX, inf, 12) == D2D_ERR_INVALID);
    EXPECT(pa_angle_params(D2D_ANGLE_AT_TX, -inf, 12) == D2D_ERR_INVALID);
    EXPECT(pa_angle_params(D2D_ANGLE_AT_TX, 0.0f, 0) == D2D_ERR_INVALID);
    EXPECT(pa_angle_params(D2D_ANGLE_AT_TX, 0.0f, -3) == D2D_ERR_INVALID);
    EXPECT(pa_angle_params(D2D_ANGLE_AT_TX, 0.0f, D2D_ANGLE_BINS_MAX + 1) == D2D_ERR_INVALID);
    {
        std::string err;
        EXPECT(d2d_host::angle_params(5, 0.0f, 12, err) == D2D_ERR_INVALID && err.find("end") != std::string::npos);
        err.clear();
        EXPECT(d2d_host::angle_params(0, nan, 12, err) == D2D_ERR_INVALID && err.find("origin") != std::string::npos);
        err.clear();
        EXPECT(d2d_host::angle_params(0, 0.0f, 5000, err) == D2D_ERR_INVALID && err.find("nbins") != std::string::npos);
    }
    // outputs_fit: nbins planes and total -- 4 * nbins + 4 bytes per cell against half of (free + held), at the edge and one past it
    EXPECT(D2D_ANGLE_BINS_MAX == 4096);
    EXPECT(pa_bytes_per_cell(1) == 8 && pa_bytes_per_cell(36) == 148 && pa_bytes_per_cell(4096) == 16388);
    const long long frees[] = {0, 1ll << 20, 3ll << 30, 288ll << 30}, helds[] = {0, 1ll << 16, 5ll << 30};
    const int bins[] = {1, 12, 36, 4096};
    for (long long mem_free : frees)
        for (long long held : helds)
            for (int nb : bins) {
                const long long edge = (mem_free / 2 + held / 2) / (4ll * nb + 4);
                EXPECT(pa_angle_fits(edge, nb, mem_free, held) == 1);
                EXPECT(pa_angle_fits(edge + 1, nb, mem_free, held) == 0);
            }
    EXPECT(pa_angle_fits(1024 * 1024, 36, 200ll << 30, 0) == 1);
    EXPECT(pa_angle_fits(1024 * 1024, 4096, 200ll << 30, 0) == 1);
    EXPECT(pa_angle_fits(200ll * 1000 * 1000, 4096, 288ll << 30, 0) == 0);  // (over 10^8 cells: what no quick GPU test can hold)
    EXPECT(pa_angle_fits((1ll << 40), 1, 288ll << 30, 0) == 0);
    EXPECT(pa_angle_fits(0, 4096, 0, 0) == 1);
    // turns: the exact cases by bits ...
    const float xs[] = {3.0f, 1.0f, tiny, 1e-30f, 1e30f, fmax};
    for (float x : xs) {
        EXPECT(is(d2d::turns(x, 0.0f), 0.0f) && is(d2d::turns(x, -0.0f), 0.0f));
        EXPECT(is(d2d::turns(0.0f, x), 0.25f) && is(d2d::turns(-0.0f, x), 0.25f));
        EXPECT(is(d2d::turns(-x, 0.0f), 0.5f) && is(d2d::turns(-x, -0.0f), 0.5f));
        EXPECT(is(d2d::turns(0.0f, -x), 0.75f) && is(d2d::turns(-0.0f, -x), 0.75f));
        EXPECT(is(d2d::turns(x, x), 0.125f) && is(d2d::turns(-x, x), 0.375f) && is(d2d::turns(-x, -x), 0.625f) && is(d2d::turns(x, -x), 0.875f));
    }
    // ... never 1: a direction a hair below the +x axis is 0 ...
    EXPECT(is(d2d::turns(1.0f, -tiny), 0.0f) && is(d2d::turns(1.0f, -1e-30f), 0.0f) && is(d2d::turns(fmax, -1.0f), 0.0f));
    EXPECT(d2d::turns(1.0f, -1e-6f) < 1.0f && d2d::turns(1.0f, -1e-6f) > 0.999f);
    // ... NaN for no direction at all ...
    EXPECT(std::isnan(d2d::turns(0.0f, 0.0f)) && std::isnan(d2d::turns(-0.0f, 0.0f)) && std::isnan(d2d::turns(-0.0f, -0.0f)));
    EXPECT(std::isnan(d2d::turns(nan, 1.0f)) && std::isnan(d2d::turns(1.0f, nan)) && std::isnan(d2d::turns(inf, 1.0f)));
    EXPECT(std::isnan(d2d::turns(1.0f, -inf)) && std::isnan(d2d::turns(inf, inf)) && std::isnan(d2d::turns(0.0f, nan)));
    // ... and finite and close everywhere else: a sweep of directions at magnitudes from denormal to the largest fp32
    const float mags[] = {tiny * 1000.0f, 1e-30f, 1e-3f, 1.0f, 1e30f, fmax * 0.7f};
    double worst = 0.0;
    const int steps = 1 << 12;
    for (float mag : mags)
        for (int i = 0; i < steps; ++i) {
            const double th = TWO_PI * (i + 0.37) / steps;
            const float dx = (float)(mag * std::cos(th)), dy = (float)(mag * std::sin(th));
            const float f = d2d::turns(dx, dy);
            EXPECT(f >= 0.0f && f < 1.0f);
            const double e = turn_error(dx, dy, f);
            // (denormal components carry few bits: their own direction is what is measured, so the error stays small all the same)
            if (e > worst) worst = e;
        }
    EXPECT(worst <= 0.75 * std::ldexp(1.0, -24));
    std::printf("power_angle_host: %d failures, worst turns error %.3f * 2^-24 turn\n", failures, worst * std::ldexp(1.0, 24));
    return failures ? 1 : 0;
}
#endif
