// The host's share of d2d_field_position_vjp_launch (d2d_posgrad.hpp: the per-contribution arithmetic, which is the definition;
// d2d_host.hpp: posgrad_params and posgrad_bytes_per_cell), compiled with plain g++ into a stand-alone program by
// tests/test_field_position_vjp_cpu.py, which also builds it with -fsanitize=address,undefined and runs it.  The product compiles
// the very same headers into libd2d.so with hipcc.
//   field_position_vjp_host IN OUT   evaluates the header over a list: IN holds int64 n, int32 fun_id, int32 amplitude and nine fp32
//                                    arrays of n (t, r, h2, inv0, inv1, rb0, rb1, ib0, ib1); OUT receives five (a, rho, kr, g, G),
//                                    g being the fold over (inv0, rb0, ib0) then (inv1, rb1, ib1) from +0 -- d2d_selftest_posgrad's
//   field_position_vjp_host          checks the parameter check and the memory rule, prints "N failures"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../../differt2d_amd/csrc/d2d_host.hpp"
#include "../../differt2d_amd/csrc/d2d_posgrad.hpp"

static int failures = 0;
#define EXPECT(x)                                                     \
    do {                                                              \
        if (!(x)) {                                                   \
            std::printf("line %d: %s does not hold\n", __LINE__, #x); \
            ++failures;                                               \
        }                                                             \
    } while (0)

static int run_list(const char* in_path, const char* out_path) {
    std::FILE* in = std::fopen(in_path, "rb");
    if (!in) return 2;
    int64_t n = 0;
    int32_t fun_id = 0, amplitude = 0;
    if (std::fread(&n, sizeof n, 1, in) != 1 || n < 0 || std::fread(&fun_id, sizeof fun_id, 1, in) != 1 ||
        std::fread(&amplitude, sizeof amplitude, 1, in) != 1) {
        std::fclose(in);
        return 2;
    }
    std::vector<float> v(9 * (size_t)n), out(5 * (size_t)n);
    const bool got = std::fread(v.data(), sizeof(float), v.size(), in) == v.size();
    std::fclose(in);
    if (!got) return 2;
    const size_t N = (size_t)n;
    for (size_t i = 0; i < N; ++i) {
        const float t = v[i], r = v[N + i], h2 = v[2 * N + i];
        const float a = d2d::posgrad_amp(amplitude, t);
        const float rho = d2d::posgrad_rho(fun_id, h2, r);
        const float kr = d2d::posgrad_kr(amplitude, rho);
        float g = 0.0f;
        g = d2d::posgrad_fold(g, kr, r, v[3 * N + i], v[5 * N + i], v[7 * N + i]);
        g = d2d::posgrad_fold(g, kr, r, v[4 * N + i], v[6 * N + i], v[8 * N + i]);
        out[i] = a;
        out[N + i] = rho;
        out[2 * N + i] = kr;
        out[3 * N + i] = g;
        out[4 * N + i] = a * g;
    }
    std::FILE* o = std::fopen(out_path, "wb");
    if (!o) return 2;
    const bool ok = std::fwrite(out.data(), sizeof(float), out.size(), o) == out.size();
    return std::fclose(o) == 0 && ok ? 0 : 2;
}

int main(int argc, char** argv) {
    if (argc == 3) return run_list(argv[1], argv[2]);
    static_assert(d2d_host::POS_CHUNK == 8 && d2d::POS_CHUNK == 8 && D2D_POS_CHUNK == 8, "the block size is part of the definition");
    std::string err;
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    std::vector<float> inv(D2D_FREQ_MAX + 1, 20.0f);
    // nf
    EXPECT(d2d_host::posgrad_params(inv.data(), 1, D2D_FIELD_AMP_SQRT, err) == D2D_OK);
    EXPECT(d2d_host::posgrad_params(inv.data(), D2D_FREQ_MAX, D2D_FIELD_AMP_LINEAR, err) == D2D_OK);
    EXPECT(d2d_host::posgrad_params(inv.data(), 0, D2D_FIELD_AMP_SQRT, err) == D2D_ERR_INVALID && err.find("the position adjoint needs nf in 1 .. 1024, got 0") == 0);
    EXPECT(d2d_host::posgrad_params(nullptr, -3, D2D_FIELD_AMP_SQRT, err) == D2D_ERR_INVALID);  // (the list is not read)
    EXPECT(d2d_host::posgrad_params(inv.data(), D2D_FREQ_MAX + 1, D2D_FIELD_AMP_SQRT, err) == D2D_ERR_INVALID);
    // the entries: 0 is allowed, a negative, NaN or infinite one is named with its index
    inv[3] = 0.0f;
    EXPECT(d2d_host::posgrad_params(inv.data(), 9, D2D_FIELD_AMP_SQRT, err) == D2D_OK);
    const float bad[] = {-1.0f, nan, inf, -inf, -0.5f};
    for (float b : bad) {
        inv[8] = b;
        EXPECT(d2d_host::posgrad_params(inv.data(), 8, D2D_FIELD_AMP_SQRT, err) == D2D_OK);  // (past nf: not read)
        EXPECT(d2d_host::posgrad_params(inv.data(), 9, D2D_FIELD_AMP_SQRT, err) == D2D_ERR_INVALID);
        EXPECT(err.find("the position adjoint needs a finite inv_wavelength >= 0, got ") == 0 && err.find(" at index 8") != std::string::npos);
    }
    inv[8] = -0.0f;  // (>= 0 holds for -0)
    EXPECT(d2d_host::posgrad_params(inv.data(), 9, D2D_FIELD_AMP_SQRT, err) == D2D_OK);
    // the amplitude, after the list
    EXPECT(d2d_host::posgrad_params(inv.data(), 9, 2, err) == D2D_ERR_INVALID && err.find("the position adjoint's amplitude must be") == 0);
    EXPECT(d2d_host::posgrad_params(inv.data(), 9, -1, err) == D2D_ERR_INVALID);
    inv[0] = nan;
    EXPECT(d2d_host::posgrad_params(inv.data(), 9, 2, err) == D2D_ERR_INVALID && err.find(" at index 0") != std::string::npos);
    // memory: 8 nf bytes of cotangents and 16 of planes per cell, against half of (free + held)
    EXPECT(d2d_host::posgrad_bytes_per_cell(1) == 24 && d2d_host::posgrad_bytes_per_cell(8) == 80 && d2d_host::posgrad_bytes_per_cell(1024) == 8208);
    EXPECT(d2d_host::posgrad_bytes_per_cell(0) == 0 && d2d_host::posgrad_bytes_per_cell(-1) == 0 && d2d_host::posgrad_bytes_per_cell(1025) == 0);
    const size_t big = std::numeric_limits<size_t>::max();
    const int NFS[] = {1, 8, 9, 17, 64, 1024};
    const size_t CELLS[] = {0, 1, 273, 1000003, (size_t)1 << 20, (size_t)1 << 31, big / 8, big};
    const size_t FREES[] = {0, 1 << 20, (size_t)3 << 30, (size_t)288 << 30, big};
    const size_t HELDS[] = {0, 1 << 16, (size_t)5 << 30, big};
    for (int nf : NFS)
        for (size_t cells : CELLS)
            for (size_t mem_free : FREES)
                for (size_t held : HELDS) {
                    const unsigned __int128 budget = (unsigned __int128)(mem_free / 2) + held / 2;
                    const unsigned __int128 need = (unsigned __int128)cells * (8u * (unsigned)nf + 16u);
                    EXPECT(d2d_host::outputs_fit(cells, d2d_host::posgrad_bytes_per_cell(nf), mem_free, held) == (need <= budget));
                }
    for (int nf : NFS) {  // the boundary byte (free counts half: two bytes of it)
        const size_t cells = 1000003, need = cells * d2d_host::posgrad_bytes_per_cell(nf);
        EXPECT(d2d_host::outputs_fit(cells, d2d_host::posgrad_bytes_per_cell(nf), 2 * need, 0));
        EXPECT(!d2d_host::outputs_fit(cells, d2d_host::posgrad_bytes_per_cell(nf), 2 * need - 2, 0));
    }
    EXPECT(!d2d_host::outputs_fit(1, d2d_host::posgrad_bytes_per_cell(0), big, big));  // an nf out of range never fits
    // the passes: blocks of POS_CHUNK in list order, the last one partial
    EXPECT(d2d_host::chunks(1, d2d_host::POS_CHUNK) == 1 && d2d_host::chunks(8, d2d_host::POS_CHUNK) == 1 && d2d_host::chunks(9, d2d_host::POS_CHUNK) == 2 &&
           d2d_host::chunks(17, d2d_host::POS_CHUNK) == 3);
    EXPECT(d2d_host::chunk_plan(17, 2, d2d_host::POS_CHUNK).first == 16 && d2d_host::chunk_plan(17, 2, d2d_host::POS_CHUNK).count == 1);
    // the header's values at a point worked by hand: r = 1, h2 = 1, LINEAR received power: rho = -2 / 2 = -1
    EXPECT(d2d::posgrad_rho(D2D_FUN_RECEIVED_POWER, 1.0f, 1.0f) == -1.0f && d2d::posgrad_rho(D2D_FUN_RECEIVED_POWER_PER_OBJECT, 1.0f, 1.0f) == -1.0f);
    EXPECT(d2d::posgrad_rho(D2D_FUN_LENGTH_SQUARED, 0.0f, 4.0f) == 0.5f && d2d::posgrad_rho(D2D_FUN_LENGTH, 0.0f, 4.0f) == 0.25f);
    EXPECT(d2d::posgrad_rho(D2D_FUN_ONE, 1.0f, 1.0f) == 0.0f && !std::signbit(d2d::posgrad_rho(D2D_FUN_ONE, 1.0f, 1.0f)));
    EXPECT(d2d::posgrad_kr(D2D_FIELD_AMP_SQRT, -1.0f) == -0.5f && d2d::posgrad_kr(D2D_FIELD_AMP_LINEAR, -1.0f) == -1.0f);
    EXPECT(d2d::posgrad_amp(D2D_FIELD_AMP_SQRT, -4.0f) == -2.0f && d2d::posgrad_amp(D2D_FIELD_AMP_LINEAR, -4.0f) == -4.0f);
    // inv = 0: phasor(0) = (1, +0), w = 0, so pr = kr, pi = +-0 and the step adds rb * kr: the incoherent limit
    EXPECT(d2d::posgrad_fold(0.0f, -1.0f, 3.0f, 0.0f, 1.0f, 0.0f) == -1.0f);
    // zero cotangents leave g at +0 whatever the phase
    EXPECT(d2d::posgrad_fold(0.0f, -1.0f, 3.3f, 20.0f, 0.0f, 0.0f) == 0.0f && !std::signbit(d2d::posgrad_fold(0.0f, -1.0f, 3.3f, 20.0f, -0.0f, 0.0f)));
    std::printf("field_position_vjp_host: %d failures\n", failures);
    return failures ? 1 : 0;
}
