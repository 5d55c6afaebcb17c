// The host's share of d2d_field_walls_vjp_launch (d2d_wallgrad.hpp: the per-bounce arithmetic, which is the definition;
// d2d_host.hpp: wallgrad_params and wall_vjp_fits), compiled with plain g++ into a stand-alone program by
// tests/test_field_walls_vjp_cpu.py, which also builds it with -fsanitize=address,undefined and runs it.  The product compiles
// the very same headers into libd2d.so with hipcc.
//   field_walls_vjp_host IN OUT   evaluates the header over a list: IN holds int64 n and twelve fp32 arrays of n (G, qx, qy, sx, sy,
//                                 ox, oy, nx, ny, tx, ty, sq); OUT receives five (qx, qy after the bounce, Wa, Wb, ok as 1 / 0) --
//                                 d2d_selftest_wallgrad's
//   field_walls_vjp_host          checks the parameter check and the memory rule, prints "N failures"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../../differt2d_amd/csrc/d2d_host.hpp"
#include "../../differt2d_amd/csrc/d2d_wallgrad.hpp"

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
    if (std::fread(&n, sizeof n, 1, in) != 1 || n < 0) {
        std::fclose(in);
        return 2;
    }
    std::vector<float> v(12 * (size_t)n), out(5 * (size_t)n);
    const bool got = std::fread(v.data(), sizeof(float), v.size(), in) == v.size();
    std::fclose(in);
    if (!got) return 2;
    const size_t N = (size_t)n;
    for (size_t i = 0; i < N; ++i) {
        float qx = v[N + i], qy = v[2 * N + i], Wa, Wb;
        const bool ok = d2d::wallgrad_bounce(v[i], qx, qy, v[3 * N + i], v[4 * N + i], v[5 * N + i], v[6 * N + i], v[7 * N + i], v[8 * N + i], v[9 * N + i],
                                             v[10 * N + i], v[11 * N + i], Wa, Wb);
        out[i] = qx;
        out[N + i] = qy;
        out[2 * N + i] = Wa;
        out[3 * N + i] = Wb;
        out[4 * N + i] = ok ? 1.0f : 0.0f;
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
    EXPECT(d2d_host::wallgrad_params(inv.data(), 1, D2D_FIELD_AMP_SQRT, err) == D2D_OK);
    EXPECT(d2d_host::wallgrad_params(inv.data(), D2D_FREQ_MAX, D2D_FIELD_AMP_LINEAR, err) == D2D_OK);
    EXPECT(d2d_host::wallgrad_params(inv.data(), 0, D2D_FIELD_AMP_SQRT, err) == D2D_ERR_INVALID && err.find("the wall adjoint needs nf in 1 .. 1024, got 0") == 0);
    EXPECT(d2d_host::wallgrad_params(nullptr, -3, D2D_FIELD_AMP_SQRT, err) == D2D_ERR_INVALID);  // (the list is not read)
    EXPECT(d2d_host::wallgrad_params(inv.data(), D2D_FREQ_MAX + 1, D2D_FIELD_AMP_SQRT, err) == D2D_ERR_INVALID);
    // the entries: 0 is allowed, a negative, NaN or infinite one is named with its index
    inv[3] = 0.0f;
    EXPECT(d2d_host::wallgrad_params(inv.data(), 9, D2D_FIELD_AMP_SQRT, err) == D2D_OK);
    const float bad[] = {-1.0f, nan, inf, -inf, -0.5f};
    for (float b : bad) {
        inv[8] = b;
        EXPECT(d2d_host::wallgrad_params(inv.data(), 8, D2D_FIELD_AMP_SQRT, err) == D2D_OK);  // (past nf: not read)
        EXPECT(d2d_host::wallgrad_params(inv.data(), 9, D2D_FIELD_AMP_SQRT, err) == D2D_ERR_INVALID);
        EXPECT(err.find("the wall adjoint needs a finite inv_wavelength >= 0, got ") == 0 && err.find(" at index 8") != std::string::npos);
    }
    inv[8] = -0.0f;  // (>= 0 holds for -0)
    EXPECT(d2d_host::wallgrad_params(inv.data(), 9, D2D_FIELD_AMP_SQRT, err) == D2D_OK);
    // the amplitude, after the list
    EXPECT(d2d_host::wallgrad_params(inv.data(), 9, 2, err) == D2D_ERR_INVALID && err.find("the wall adjoint's amplitude must be") == 0);
    EXPECT(d2d_host::wallgrad_params(inv.data(), 9, -1, err) == D2D_ERR_INVALID);
    inv[0] = nan;
    EXPECT(d2d_host::wallgrad_params(inv.data(), 9, 2, err) == D2D_ERR_INVALID && err.find(" at index 0") != std::string::npos);
    // memory: 8 nf bytes of cotangents per cell and 8 bytes per patch and wall, against half of (free + held)
    const size_t big = std::numeric_limits<size_t>::max();
    const int NFS[] = {1, 8, 9, 17, 1024};
    const size_t CELLS[] = {0, 1, 273, 1000003, (size_t)1 << 31, big / 8, big};
    const size_t TILES[] = {0, 1, 6, 16384, (size_t)1 << 40, big};
    const size_t WALLS[] = {0, 1, 7, 70, 2487, big};
    const size_t FREES[] = {0, 1 << 20, (size_t)3 << 30, (size_t)288 << 30, big};
    const size_t HELDS[] = {0, 1 << 16, big};
    for (int nf : NFS)
        for (size_t cells : CELLS)
            for (size_t tiles : TILES)
                for (size_t walls : WALLS)
                    for (size_t mem_free : FREES)
                        for (size_t held : HELDS) {
                            const unsigned __int128 budget = (unsigned __int128)(mem_free / 2) + held / 2;
                            unsigned __int128 need = (unsigned __int128)cells * (8u * (unsigned)nf);
                            // (tiles * walls * 8 may pass 2^128 at the largest values: compared by quotients where it could)
                            bool fits = need <= budget;
                            if (fits && tiles && walls) {
                                const unsigned __int128 left = (budget - need) / 8;
                                fits = (unsigned __int128)tiles <= left && (unsigned __int128)walls <= left / tiles;
                            }
                            EXPECT(d2d_host::wall_vjp_fits(cells, nf, tiles, walls, mem_free, held) == fits);
                        }
    {  // the boundary byte (free counts half: two bytes of it)
        const size_t cells = 1000003, tiles = 15626, walls = 7, need = cells * 8 * 9 + tiles * walls * 8;
        EXPECT(d2d_host::wall_vjp_fits(cells, 9, tiles, walls, 2 * need, 0));
        EXPECT(!d2d_host::wall_vjp_fits(cells, 9, tiles, walls, 2 * need - 2, 0));
    }
    EXPECT(!d2d_host::wall_vjp_fits(1, 0, 1, 1, big, big));  // an nf out of range never fits
    // the passes: blocks of POS_CHUNK in list order, the last one partial
    EXPECT(d2d_host::chunks(9, d2d_host::POS_CHUNK) == 2 && d2d_host::chunks(17, d2d_host::POS_CHUNK) == 3);
    // the header at points worked by hand.  A wall from (0, 0) to (2, 0): t = (2, 0), n = normalize((0, -2)) = (0, -1), sq = 4.
    // A ray from (0.5, 1) going down-right by (0.5, -1) hits it at (1, 0): s = 0.5; |seg| = sqrt(1.25) is not exact, so take (3, -4) / 4
    // from (0.25, 1): hits (1, 0), u = (0.6, -0.8), u . n = 0.8, gam = 1.6
    {
        float qx = 0.25f, qy = 1.0f, Wa, Wb;
        const bool ok = d2d::wallgrad_bounce(2.0f, qx, qy, 0.75f, -1.0f, 0.0f, 0.0f, 0.0f, -1.0f, 2.0f, 0.0f, 4.0f, Wa, Wb);
        float ux, uy;
        d2d::unit_dir(0.75f, -1.0f, ux, uy);
        const float gam = 2.0f * (ux * 0.0f + uy * -1.0f), wa = 2.0f * gam;
        EXPECT(ok && qx == 1.0f && qy == 0.0f && Wb == wa * 0.5f && Wa == wa - wa * 0.5f && std::fabs(Wa - 1.6f) < 1e-6f);
    }
    {  // s = 0 and s = 1: the whole term goes to one end point
        float qx = 0.0f, qy = 1.0f, Wa, Wb;
        EXPECT(d2d::wallgrad_bounce(1.0f, qx, qy, 0.0f, -1.0f, 0.0f, 0.0f, 0.0f, -1.0f, 2.0f, 0.0f, 4.0f, Wa, Wb) && Wa == 2.0f && Wb == 0.0f);
        qx = 2.0f, qy = 1.0f;
        EXPECT(d2d::wallgrad_bounce(1.0f, qx, qy, 0.0f, -1.0f, 0.0f, 0.0f, 0.0f, -1.0f, 2.0f, 0.0f, 4.0f, Wa, Wb) && Wa == 0.0f && Wb == 2.0f);
    }
    {  // a zero-length wall: n = (0, 0), sq = 1 in the table: +-0
        float qx = 0.0f, qy = 1.0f, Wa, Wb;
        EXPECT(d2d::wallgrad_bounce(3.0f, qx, qy, 0.5f, -1.0f, 0.5f, 0.0f, 0.0f, -0.0f, 0.0f, 0.0f, 1.0f, Wa, Wb) && Wa == 0.0f && Wb == 0.0f);
    }
    {  // a zero segment: no unit vector, q stays where it was plus zero
        float qx = 0.5f, qy = 0.25f, Wa, Wb;
        EXPECT(!d2d::wallgrad_bounce(3.0f, qx, qy, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, -1.0f, 2.0f, 0.0f, 4.0f, Wa, Wb) && qx == 0.5f && qy == 0.25f);
    }
    {  // a NaN G: both weights NaN, ok as the segment says
        float qx = 0.25f, qy = 1.0f, Wa, Wb;
        EXPECT(d2d::wallgrad_bounce(nan, qx, qy, 0.75f, -1.0f, 0.0f, 0.0f, 0.0f, -1.0f, 2.0f, 0.0f, 4.0f, Wa, Wb) && Wa != Wa && Wb != Wb);
    }
    std::printf("field_walls_vjp_host: %d failures\n", failures);
    return failures ? 1 : 0;
}
