// The host's share of d2d_field_coefs_vjp_launch that is its own (d2d_host.hpp: coef_vjp_fits; the wavelength list and the chunk
// plan are the frequency response's, tests/native/frequency_response_host.cpp), compiled with plain g++ into a stand-alone program by
// tests/test_field_coefs_vjp_cpu.py, which also builds it with -fsanitize=address,undefined and runs it.  The product compiles the
// very same header into libd2d.so with hipcc.  The rule: the cotangents take 8 nf bytes per cell, the partial rows 4 bytes per patch
// and object, and their sum is held against half of (free + held) without a product or a sum that could wrap.
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>

#include "../../differt2d_amd/csrc/d2d_host.hpp"

static int failures = 0;
#define EXPECT(x)                                                     \
    do {                                                              \
        if (!(x)) {                                                   \
            std::printf("line %d: %s does not hold\n", __LINE__, #x); \
            ++failures;                                               \
        }                                                             \
    } while (0)

// the rule in 128-bit arithmetic
static bool rule(size_t cells, int nf, size_t patches, size_t n, size_t mem_free, size_t held) {
    const unsigned __int128 budget = (unsigned __int128)(mem_free / 2) + held / 2;
    const unsigned __int128 planes = (unsigned __int128)cells * 8u * (unsigned)nf;  // < 2^64 * 2^13
    if (planes > budget) return false;
    const unsigned __int128 rows = (unsigned __int128)patches * n;  // < 2^128: the factor 4 goes to the other side
    return rows <= (budget - planes) / 4u;
}

int main() {
    const size_t big = std::numeric_limits<size_t>::max();
    const int NFS[] = {1, 8, 9, 17, 64, 1024};
    const size_t CELLS[] = {0, 1, 273, 1000003, (size_t)1 << 20, (size_t)1 << 31, big / 8, big};
    const size_t PATCHES[] = {0, 1, 6, 16384, (size_t)1 << 25, big / 4, big};
    const size_t NS[] = {0, 1, 8, 50, 4095, big};
    const size_t FREES[] = {0, 1 << 20, (size_t)3 << 30, (size_t)288 << 30, big};
    const size_t HELDS[] = {0, 1 << 16, (size_t)5 << 30, big};
    for (int nf : NFS)
        for (size_t cells : CELLS)
            for (size_t patches : PATCHES)
                for (size_t n : NS)
                    for (size_t mem_free : FREES)
                        for (size_t held : HELDS)
                            EXPECT(d2d_host::coef_vjp_fits(cells, nf, patches, n, mem_free, held) == rule(cells, nf, patches, n, mem_free, held));
    // the boundary byte: need == budget fits, a budget one byte short does not (free counts half: two bytes of it)
    for (int nf : NFS) {
        const size_t cells = 1000003, patches = 15626, n = 50;
        const size_t need = cells * 8 * (size_t)nf + patches * n * 4;
        EXPECT(d2d_host::coef_vjp_fits(cells, nf, patches, n, 2 * need, 0));
        EXPECT(!d2d_host::coef_vjp_fits(cells, nf, patches, n, 2 * need - 2, 0));
        EXPECT(d2d_host::coef_vjp_fits(cells, nf, patches, n, 0, 2 * need));
        EXPECT(!d2d_host::coef_vjp_fits(cells, nf, patches, n, 0, 2 * need - 2));
        // the rows alone can be what does not fit
        EXPECT(d2d_host::coef_vjp_fits(cells, nf, patches, n, 2 * need, 0) && !d2d_host::coef_vjp_fits(cells, nf, patches, n + 1, 2 * need, 0));
    }
    // 1024^2 cells, 64 wavelengths, 50 walls: 512 MiB of cotangents and 3 MiB of rows
    EXPECT(d2d_host::coef_vjp_fits((size_t)1 << 20, 64, 16384, 50, (size_t)200 << 30, 0));
    EXPECT(!d2d_host::coef_vjp_fits((size_t)1 << 20, 64, 16384, 50, (size_t)1 << 30, 0));
    EXPECT(d2d_host::coef_vjp_fits(0, 1, 0, 0, 0, 0));
    std::printf("field_coefs_vjp_host: %d failures\n", failures);
    return failures ? 1 : 0;
}
