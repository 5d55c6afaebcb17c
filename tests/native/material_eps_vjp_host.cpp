// The host's share of d2d_material_eps_vjp_launch, compiled with plain g++ into a stand-alone program: the arithmetic of
// d2d_fresnel_grad.hpp (the very text the kernel compiles) and d2d_host.hpp's eps_vjp_fits and the chunk plan with MAT_CHUNK.
// tests/test_material_eps_vjp_cpu.py builds it plain and with -fsanitize=address,undefined and runs both:
//     material_eps_vjp_host                   the checks of the host functions; the exit status counts failures
//     material_eps_vjp_host IN OUT            IN: int64 n, then er[n], ei[n], c[n] (fp32); OUT: gr, gi, dr, di, ok (1 / 0) for TE, then for TM
// Nothing of it is loaded into Python.  The product compiles the very same headers into libd2d.so with hipcc.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../differt2d_amd/csrc/d2d_fresnel_grad.hpp"
#include "../../differt2d_amd/csrc/d2d_host.hpp"

static int failures = 0;
#define EXPECT(x)                                                     \
    do {                                                              \
        if (!(x)) {                                                   \
            std::printf("line %d: %s does not hold\n", __LINE__, #x); \
            ++failures;                                               \
        }                                                             \
    } while (0)

static bool same(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

static int run_list(const char* in_path, const char* out_path) {
    std::FILE* in = std::fopen(in_path, "rb");
    if (!in) return 2;
    int64_t n = 0;
    if (std::fread(&n, sizeof n, 1, in) != 1 || n < 0) return 2;
    std::vector<float> v(3 * (size_t)n), out(10 * (size_t)n);
    if (std::fread(v.data(), sizeof(float), v.size(), in) != v.size()) return 2;
    std::fclose(in);
    const float *er = v.data(), *ei = er + n, *c = ei + n;
    for (int pol = 0; pol < 2; ++pol) {
        float* o = out.data() + (size_t)pol * 5 * (size_t)n;
        for (int64_t k = 0; k < n; ++k) {
            bool ok;
            d2d::fresnel_grad(er[k], ei[k], c[k], pol, o[k], o[n + k], o[2 * n + k], o[3 * n + k], ok);
            o[4 * n + k] = ok ? 1.0f : 0.0f;
        }
    }
    std::FILE* o = std::fopen(out_path, "wb");
    if (!o) return 2;
    const bool ok = std::fwrite(out.data(), sizeof(float), out.size(), o) == out.size();
    std::fclose(o);
    return ok ? 0 : 2;
}

int main(int argc, char** argv) {
    if (argc == 3) return run_list(argv[1], argv[2]);
    const float nan = std::numeric_limits<float>::quiet_NaN();
    const float big = 1125899906842624.0f;  // 2^50
    float gr, gi, dr, di, fr, fi;
    bool ok;
    // ---- the arithmetic: what the definition states outright
    // normal incidence on eps = 4 (q = 2): TE d = -1 / (2 * 3^2) = -1/18, TM d = 1 * (4 - 2 + 2) / (2 * 6^2) = 1/18
    d2d::fresnel_grad(4.0f, -0.0f, 1.0f, D2D_POL_TE, gr, gi, dr, di, ok);
    EXPECT(ok && same(gr, -1.0f / 3.0f) && gi == 0.0f && std::fabs(dr + 1.0f / 18.0f) < 2e-8f && di == 0.0f);
    d2d::fresnel_grad(4.0f, -0.0f, 1.0f, D2D_POL_TM, gr, gi, dr, di, ok);
    EXPECT(ok && same(gr, 1.0f / 3.0f) && gi == 0.0f && std::fabs(dr - 1.0f / 18.0f) < 2e-8f && di == 0.0f);
    d2d::fresnel_grad(4.0f, -0.0f, std::nextafterf(1.0f, 2.0f), D2D_POL_TE, gr, gi, dr, di, ok);  // c just above 1 is 1
    EXPECT(ok && same(gr, -1.0f / 3.0f) && std::fabs(dr + 1.0f / 18.0f) < 2e-8f);
    // (gr, gi) are fresnel()'s bits, also at its special cases
    for (int pol : {D2D_POL_TE, D2D_POL_TM})
        for (float er : {1.0f, 0.25f, 0.0f, 4.0f, 9.0f, big, -big})
            for (float ei : {0.0f, -0.0f, -1.0f, -big})
                for (float c : {0.0f, 1e-3f, 0.5f, 1.0f, 2.0f}) {
                    d2d::fresnel(er, ei, c, pol, fr, fi);
                    d2d::fresnel_grad(er, ei, c, pol, gr, gi, dr, di, ok);
                    EXPECT(same(gr, fr) && same(gi, fi));
                    EXPECT(std::isfinite(dr) && std::isfinite(di));  // components of 2^50 stay finite
                    if (!ok) EXPECT(same(dr, 0.0f) && same(di, 0.0f));
                }
    for (int pol : {D2D_POL_TE, D2D_POL_TM}) {
        // den == 0, the grazing limit: G = -1 by definition, no derivative
        d2d::fresnel_grad(1.0f, 0.0f, 0.0f, pol, gr, gi, dr, di, ok);
        EXPECT(!ok && same(gr, -1.0f) && same(gi, 0.0f) && same(dr, 0.0f) && same(di, 0.0f));
        // m == 0 with den != 0: eps = 1 - c^2 exactly (c = 0.5: w = -0.75 + 0.25 ... er = 0.75), q = 0, G = 1: the square-root singularity
        d2d::fresnel_grad(0.75f, 0.0f, 0.5f, pol, gr, gi, dr, di, ok);
        EXPECT(!ok && same(gr, 1.0f) && gi == 0.0f && same(dr, 0.0f) && same(di, 0.0f));
        d2d::fresnel_grad(0.75f, -0.0f, 0.5f, pol, gr, gi, dr, di, ok);
        EXPECT(!ok && same(dr, 0.0f) && same(di, 0.0f));
        // grazing incidence on a wall: q != 0, den = |q|^2 != 0 for TE and TM alike: the formula holds, d = 0 there (the factor c)
        d2d::fresnel_grad(4.0f, -1.0f, 0.0f, pol, gr, gi, dr, di, ok);
        EXPECT(ok && same(gr, -1.0f) && dr == 0.0f && di == 0.0f);
        // a NaN propagates, ok stays true
        d2d::fresnel_grad(4.0f, -1.0f, nan, pol, gr, gi, dr, di, ok);
        EXPECT(ok && gr != gr && gi != gi && dr != dr && di != di);
        d2d::fresnel_grad(nan, -1.0f, 0.5f, pol, gr, gi, dr, di, ok);
        EXPECT(ok && dr != dr && di != di);
        // lossy: a derivative with both components
        d2d::fresnel_grad(9.0f, -2.0f, 0.3f, pol, gr, gi, dr, di, ok);
        EXPECT(ok && dr != 0.0f && di != 0.0f);
        // total reflection on the cut, from either zero: finite, and |G| = 1
        for (float ei : {0.0f, -0.0f}) {
            d2d::fresnel_grad(0.25f, ei, 0.5f, pol, gr, gi, dr, di, ok);
            EXPECT(ok && std::fabs(gr * gr + gi * gi - 1.0f) < 4e-7f && std::isfinite(dr) && std::isfinite(di) && di != 0.0f);
        }
    }
    {
        // eps - 2 + 2 c^2 without cancellation: at er = 1 + 2^-20 and c = 1 the TM numerator is c * (2^-20 + 1) exactly
        // G = (eps - q) / (eps + q), q = sqrt(eps): d = (eps) / (q (eps + q)^2) -> 1/4 as eps -> 1
        d2d::fresnel_grad(1.0f + 0x1p-20f, -0.0f, 1.0f, D2D_POL_TM, gr, gi, dr, di, ok);
        EXPECT(ok && std::fabs(dr - 0.25f) < 1e-6f && di == 0.0f);
        d2d::fresnel_grad(1.0f + 0x1p-20f, -0.0f, 1.0f, D2D_POL_TE, gr, gi, dr, di, ok);
        EXPECT(ok && std::fabs(dr + 0.25f) < 1e-6f);
    }
    // ---- eps_vjp_fits: 8 nf bytes per cell, 24 nf bytes per object, 64 bytes per patch and object against half of (free + held)
    const unsigned long long all = ~0ull;
    const unsigned long long frees[] = {0, 1ull << 20, 3ull << 30, 288ull << 30, all}, helds[] = {0, 1ull << 16, 5ull << 30, all};
    EXPECT(d2d_host::MAT_CHUNK == 8);
    for (unsigned long long mem_free : frees)
        for (unsigned long long held : helds)
            for (int nf : {1, 9, 1024})
                for (unsigned long long n_obj : {0ull, 7ull, 4095ull})
                    for (unsigned long long patches : {0ull, 1ull, 16384ull}) {
                        const unsigned long long budget = mem_free / 2 + held / 2, per = 8ull * nf;
                        const unsigned long long fixed = 24ull * nf * n_obj + 64ull * patches * n_obj;
                        if (fixed > budget) {
                            EXPECT(!d2d_host::eps_vjp_fits(0, nf, patches, n_obj, mem_free, held));
                            continue;
                        }
                        const unsigned long long edge = (budget - fixed) / per;
                        EXPECT(d2d_host::eps_vjp_fits(edge, nf, patches, n_obj, mem_free, held));
                        EXPECT(!d2d_host::eps_vjp_fits(edge + 1, nf, patches, n_obj, mem_free, held));
                    }
    // the boundary byte: 1024^2 cells of 64 wavelengths need 512 MiB, 50 walls 76 800 bytes and 16384 patches of them 52 428 800:
    // twice that free fits, two bytes less do not
    const unsigned long long need = (512ull << 20) + 24ull * 64 * 50 + 64ull * 16384 * 50;
    EXPECT(d2d_host::eps_vjp_fits(1ull << 20, 64, 16384, 50, 2 * need, 0));
    EXPECT(!d2d_host::eps_vjp_fits(1ull << 20, 64, 16384, 50, 2 * need - 2, 0));
    EXPECT(d2d_host::eps_vjp_fits(1ull << 20, 64, 16384, 50, 0, 2 * need));  // what the buffers hold already counts as free
    EXPECT(!d2d_host::eps_vjp_fits(1ull << 20, 64, 16384, 50, 0, 2 * need - 2));
    // sizes whose products would wrap are refused, not wrapped
    EXPECT(!d2d_host::eps_vjp_fits(all, 1024, 1, 50, 288ull << 30, 0) && !d2d_host::eps_vjp_fits(all / 8 + 2, 1, 0, 0, all, all));
    EXPECT(!d2d_host::eps_vjp_fits(1, 1, 1, all, all, all) && !d2d_host::eps_vjp_fits(1, 1024, 1, all / 24576 + 1, all, all));
    EXPECT(!d2d_host::eps_vjp_fits(1, 1, all, 2, all, all) && !d2d_host::eps_vjp_fits(1, 1, all / 64 + 1, 64, all, all));
    EXPECT(!d2d_host::eps_vjp_fits(1, 1, 1ull << 32, 1ull << 32, all, all));
    EXPECT(!d2d_host::eps_vjp_fits(1, 0, 1, 1, all, all) && !d2d_host::eps_vjp_fits(1, -1, 1, 1, all, all) && d2d_host::eps_vjp_fits(0, 1, 0, 0, 0, 0));
    // ---- the chunks: for every nf they cover 0 .. nf-1 once and in order; the reduction of chunk i takes count * N * 2 entries
    // of rows whose stride is MAT_CHUNK * N * 2 and writes them from first * N * 2 on: the rows of the result are covered once
    const int W = d2d_host::MAT_CHUNK;
    for (int nf = 1; nf <= D2D_FREQ_MAX; ++nf) {
        int next = 0;
        const int n = d2d_host::chunks(nf, W);
        EXPECT(n == (nf + W - 1) / W);
        for (int i = 0; i < n; ++i) {
            const d2d_host::Chunk ch = d2d_host::chunk_plan(nf, i, W);
            EXPECT(ch.first == next && ch.count >= 1 && ch.count <= W);
            next = ch.first + ch.count;
        }
        EXPECT(next == nf);
    }
    for (int nf : {1, W, W + 1, 2 * W + 1}) {
        const d2d_host::Chunk last = d2d_host::chunk_plan(nf, d2d_host::chunks(nf, W) - 1, W);
        EXPECT(last.first + last.count == nf && last.count == (nf % W ? nf % W : W));
    }
    std::printf("material_eps_vjp_host: chunk %d, %d failures\n", W, failures);
    return failures ? 1 : 0;
}
