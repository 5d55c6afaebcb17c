// The phasor of d2d_coherent_field_launch's sink (differt2d_amd/csrc/d2d_phasor.hpp: the kernel's own text) and the host's share
// of the launch (d2d_host.hpp: field_params, outputs_fit with FIELD_BYTES_PER_CELL), compiled with plain g++ -ffp-contract=off.  Two builds of this file by
// tests/test_coherent_field_cpu.py: a shared library driven through ctypes, and -- with -DCF_MAIN -- a stand-alone program that
// checks the host functions, refusals included, and walks the phasor over a sweep of phases; the program is also built with
// -fsanitize=address,undefined and run.  The product compiles the very same headers into libd2d.so with hipcc, where
// d2d::FieldSink::put calls phasor once per non-zero contribution and lane.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>

#include "../../differt2d_amd/csrc/d2d_host.hpp"
#include "../../differt2d_amd/csrc/d2d_phasor.hpp"

extern "C" {

// c[i] = cos(2 pi f[i]), s[i] = sin(2 pi f[i]); k[i], g[i]: the quarter turn and the reduced phase they come from
void cf_phasor(long long n, const float* f, float* c, float* s, float* k, float* g) {
    for (long long i = 0; i < n; ++i) {
        d2d::phasor(f[i], c[i], s[i]);
        k[i] = d2d::phasor_quarter(f[i]);
        g[i] = d2d::phasor_reduce(f[i], k[i]);
    }
}

// d2d_host.hpp's share of the launch: the status of (inv_wavelength, amplitude), and whether 12 bytes per cell fit half of the
// free device memory
int cf_field_params(float inv_wavelength, int amplitude) {
    std::string err;
    const int rc = d2d_host::field_params(inv_wavelength, amplitude, err);
    return (rc == D2D_OK) == err.empty() ? rc : -1000;  // (a refusal always says why)
}
long long cf_bytes_per_cell() { return (long long)d2d_host::FIELD_BYTES_PER_CELL; }
int cf_field_fits(long long cells, long long mem_free, long long held) {
    return d2d_host::outputs_fit((size_t)cells, d2d_host::FIELD_BYTES_PER_CELL, (size_t)mem_free, (size_t)held) ? 1 : 0;
}
}

#ifdef CF_MAIN
static int failures = 0;
#define EXPECT(x)                                                \
    do {                                                         \
        if (!(x)) {                                              \
            std::printf("line %d: %s does not hold\n", __LINE__, #x); \
            ++failures;                                          \
        }                                                        \
    } while (0)

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // field_params: what is accepted ...
    EXPECT(cf_field_params(0.0f, D2D_FIELD_AMP_SQRT) == D2D_OK);
    EXPECT(cf_field_params(20.0f, D2D_FIELD_AMP_LINEAR) == D2D_OK);
    EXPECT(cf_field_params(std::numeric_limits<float>::max(), D2D_FIELD_AMP_SQRT) == D2D_OK);
    EXPECT(cf_field_params(std::numeric_limits<float>::denorm_min(), D2D_FIELD_AMP_LINEAR) == D2D_OK);
    EXPECT(cf_field_params(-0.0f, D2D_FIELD_AMP_SQRT) == D2D_OK);
    // ... and what is refused
    EXPECT(cf_field_params(-1.0f, D2D_FIELD_AMP_SQRT) == D2D_ERR_INVALID);
    EXPECT(cf_field_params(-std::numeric_limits<float>::denorm_min(), D2D_FIELD_AMP_SQRT) == D2D_ERR_INVALID);
    EXPECT(cf_field_params(nan, D2D_FIELD_AMP_SQRT) == D2D_ERR_INVALID);
    EXPECT(cf_field_params(inf, D2D_FIELD_AMP_LINEAR) == D2D_ERR_INVALID);
    EXPECT(cf_field_params(-inf, D2D_FIELD_AMP_LINEAR) == D2D_ERR_INVALID);
    EXPECT(cf_field_params(20.0f, 2) == D2D_ERR_INVALID);
    EXPECT(cf_field_params(20.0f, -1) == D2D_ERR_INVALID);
    {
        std::string err;
        EXPECT(d2d_host::field_params(nan, 0, err) == D2D_ERR_INVALID && err.find("inv_wavelength") != std::string::npos);
        err.clear();
        EXPECT(d2d_host::field_params(1.0f, 7, err) == D2D_ERR_INVALID && err.find("amplitude") != std::string::npos);
    }
    // outputs_fit: re, im, total -- 12 bytes per cell against half of (free + held), at the edge and one past it
    EXPECT(cf_bytes_per_cell() == 12);
    const long long frees[] = {0, 1ll << 20, 3ll << 30, 288ll << 30}, helds[] = {0, 1ll << 16, 5ll << 30};
    for (long long mem_free : frees)
        for (long long held : helds) {
            const long long edge = (mem_free / 2 + held / 2) / 12;
            EXPECT(cf_field_fits(edge, mem_free, held) == 1);
            EXPECT(cf_field_fits(edge + 1, mem_free, held) == 0);
        }
    EXPECT(cf_field_fits(1024 * 1024, 200ll << 30, 0) == 1);
    EXPECT(cf_field_fits((1ll << 40), 288ll << 30, 0) == 0);
    EXPECT(cf_field_fits(0, 0, 0) == 1);
    // the phasor: exact at 0, on the unit circle and near libm everywhere, NaN in NaN out
    float c = 0.0f, s = 0.0f, k = 0.0f, g = 0.0f;
    float f = 0.0f;
    cf_phasor(1, &f, &c, &s, &k, &g);
    EXPECT(c == 1.0f && s == 0.0f && !std::signbit(s) && k == 0.0f && g == 0.0f);
    f = nan;
    cf_phasor(1, &f, &c, &s, &k, &g);
    EXPECT(std::isnan(c) && std::isnan(s));
    double worst = 0.0;
    const int steps = 1 << 16;
    for (int i = 0; i < steps; ++i) {
        f = (float)i / (float)steps;
        cf_phasor(1, &f, &c, &s, &k, &g);
        EXPECT(k >= 0.0f && k <= 4.0f && std::fabs(g) <= 0.125f && (double)g == (double)f - 0.25 * (double)k);
        const double th = 2.0 * 3.14159265358979323846 * (double)f;
        worst = std::fmax(worst, std::fmax(std::fabs((double)c - std::cos(th)), std::fabs((double)s - std::sin(th))));
    }
    EXPECT(worst <= 2.0 * std::ldexp(1.0, -24));
    std::printf("coherent_field_host: %d failures, worst phasor error %.3f * 2^-24\n", failures, worst * std::ldexp(1.0, 24));
    return failures ? 1 : 0;
}
#endif
