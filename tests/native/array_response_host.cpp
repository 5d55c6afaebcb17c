// The steering arithmetic of d2d_array_response_launch's sink (differt2d_amd/csrc/d2d_steer.hpp: the kernel's own text) and the
// host's share of the launch (d2d_host.hpp: array_params, outputs_fit with array_bytes_per_cell), compiled with plain g++ -ffp-contract=off.  Two builds of this
// file by tests/test_array_response_cpu.py: a shared library driven through ctypes, and -- with -DAR_MAIN -- a stand-alone program
// that checks the host functions, refusals included, and the exact cases of the header; the program is also built with
// -fsanitize=address,undefined and run.  The product compiles the very same headers into libd2d.so with hipcc, where
// d2d::ArraySink::put_rd calls them once per non-zero contribution, lane and antenna pair.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../differt2d_amd/csrc/d2d_host.hpp"
#include "../../differt2d_amd/csrc/d2d_steer.hpp"

extern "C" {

// (ux, uy, ok)[i] = unit_dir(dx[i], dy[i])
void ar_unit_dir(long long n, const float* dx, const float* dy, float* ux, float* uy, unsigned char* ok) {
    for (long long i = 0; i < n; ++i) ok[i] = d2d::unit_dir(dx[i], dy[i], ux[i], uy[i]) ? 1 : 0;
}

// out[i] = steer_dot(ex[i], ey[i], ux[i], uy[i])
void ar_steer_dot(long long n, const float* ex, const float* ey, const float* ux, const float* uy, float* out) {
    for (long long i = 0; i < n; ++i) out[i] = d2d::steer_dot(ex[i], ey[i], ux[i], uy[i]);
}

// out[i] = steer_phase(f0[i], qt[i], qr[i], inv[i])
void ar_steer_phase(long long n, const float* f0, const float* qt, const float* qr, const float* inv, float* out) {
    for (long long i = 0; i < n; ++i) out[i] = d2d::steer_phase(f0[i], qt[i], qr[i], inv[i]);
}

// d2d_host.hpp's share of the launch: the status of the counts, lists, wavelength and amplitude (a list pointer may be NULL where
// the count is out of range: it is not read), and whether 8 * nr * nt + 4 bytes per cell fit half of the free device memory.
// `index_out`: the number the message ends in, -1 where it ends in none.
int ar_array_params(int nt, const float* tx, int nr, const float* rx, float inv, int amplitude, int* index_out) {
    std::string err;
    const int rc = d2d_host::array_params(nt, tx, nr, rx, inv, amplitude, err);
    if (index_out) {
        *index_out = -1;
        size_t k = err.size();
        while (k > 0 && err[k - 1] >= '0' && err[k - 1] <= '9') --k;
        if (k < err.size() && err.compare(k >= 10 ? k - 10 : 0, k >= 10 ? 10 : k, " at index ") == 0) *index_out = std::stoi(err.substr(k));
    }
    return (rc == D2D_OK) == err.empty() ? rc : -1000;  // (a refusal always says why)
}
long long ar_bytes_per_cell(int nt, int nr) { return (long long)d2d_host::array_bytes_per_cell(nt, nr); }
int ar_array_fits(unsigned long long cells, int nt, int nr, unsigned long long mem_free, unsigned long long held) {
    return d2d_host::outputs_fit((size_t)cells, d2d_host::array_bytes_per_cell(nt, nr), (size_t)mem_free, (size_t)held) ? 1 : 0;
}
}

#ifdef AR_MAIN
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
    // array_params: both limits of both counts (lists of exactly the size that is read: the sanitizer sees a read past them) ...
    for (int nt : {1, D2D_ARRAY_MAX})
        for (int nr : {1, D2D_ARRAY_MAX}) {
            std::vector<float> tx(2 * (size_t)nt, 0.025f), rx(2 * (size_t)nr, -0.0f);
            int at = 0;
            EXPECT(ar_array_params(nt, tx.data(), nr, rx.data(), 20.0f, D2D_FIELD_AMP_SQRT, &at) == D2D_OK && at == -1);
            EXPECT(ar_array_params(nt, tx.data(), nr, rx.data(), 0.0f, D2D_FIELD_AMP_LINEAR, &at) == D2D_OK);
            // ... every bad position of both lists, with the element's index at the message's end ...
            for (float bad : {nan, inf, -inf}) {
                for (int k = 0; k < 2 * nt; ++k) {
                    std::vector<float> t2 = tx;
                    t2[(size_t)k] = bad;
                    EXPECT(ar_array_params(nt, t2.data(), nr, rx.data(), 20.0f, 0, &at) == D2D_ERR_INVALID && at == k / 2);
                }
                for (int k = 0; k < 2 * nr; ++k) {
                    std::vector<float> r2 = rx;
                    r2[(size_t)k] = bad;
                    EXPECT(ar_array_params(nt, tx.data(), nr, r2.data(), 20.0f, 0, &at) == D2D_ERR_INVALID && at == k / 2);
                }
            }
            // ... the largest finite offsets pass ...
            tx[0] = fmax, rx[1] = -fmax;
            EXPECT(ar_array_params(nt, tx.data(), nr, rx.data(), 20.0f, 0, &at) == D2D_OK);
        }
    {
        // ... counts out of range: no list is read (the pointers are NULL) ...
        const float one[2] = {0.0f, 0.0f};
        int at = 0;
        for (int bad : {0, -1, D2D_ARRAY_MAX + 1, 1 << 30, -(1 << 30)}) {
            EXPECT(ar_array_params(bad, nullptr, 1, nullptr, 20.0f, 0, &at) == D2D_ERR_INVALID && at == -1);
            EXPECT(ar_array_params(1, nullptr, bad, nullptr, 20.0f, 0, &at) == D2D_ERR_INVALID && at == -1);
            EXPECT(ar_array_params(bad, nullptr, bad, nullptr, 20.0f, 0, &at) == D2D_ERR_INVALID);
        }
        // ... wavelength and amplitude ...
        for (float bad : {-1.0f, -tiny, nan, inf, -inf}) EXPECT(ar_array_params(1, one, 1, one, bad, 0, &at) == D2D_ERR_INVALID && at == -1);
        for (int bad : {2, -1}) EXPECT(ar_array_params(1, one, 1, one, 20.0f, bad, &at) == D2D_ERR_INVALID && at == -1);
        std::string err;
        EXPECT(d2d_host::array_params(9, one, 1, one, 20.0f, 0, err) == D2D_ERR_INVALID && err.find("nt") != std::string::npos);
        err.clear();
        EXPECT(d2d_host::array_params(1, one, 0, one, 20.0f, 0, err) == D2D_ERR_INVALID && err.find("nr") != std::string::npos);
        err.clear();
        EXPECT(d2d_host::array_params(1, one, 1, one, nan, 0, err) == D2D_ERR_INVALID && err.find("inv_wavelength") != std::string::npos);
        err.clear();
        EXPECT(d2d_host::array_params(1, one, 1, one, 20.0f, 7, err) == D2D_ERR_INVALID && err.find("amplitude") != std::string::npos);
        err.clear();
        const float badrx[4] = {0.0f, 0.0f, 0.0f, nan};
        EXPECT(d2d_host::array_params(1, one, 2, badrx, 20.0f, 0, err) == D2D_ERR_INVALID && err.find("rx_elems") != std::string::npos &&
               err.size() > 10 && err.compare(err.size() - 10, 10, "at index 1") == 0);
        // ... in the order of the definition: a bad count before a bad element before a bad wavelength before a bad amplitude
        err.clear();
        EXPECT(d2d_host::array_params(1, one, 2, badrx, nan, 7, err) == D2D_ERR_INVALID && err.find("rx_elems") != std::string::npos);
        err.clear();
        EXPECT(d2d_host::array_params(1, one, 1, one, nan, 7, err) == D2D_ERR_INVALID && err.find("inv_wavelength") != std::string::npos);
    }
    // outputs_fit: 8 * nr * nt + 4 bytes per cell against half of (free + held), at the boundary and one past it
    EXPECT(D2D_ARRAY_MAX == 8);
    EXPECT(ar_bytes_per_cell(1, 1) == 12 && ar_bytes_per_cell(4, 3) == 100 && ar_bytes_per_cell(4, 4) == 132 && ar_bytes_per_cell(8, 8) == 516);
    const unsigned long long all = ~0ull;
    const unsigned long long frees[] = {0, 1ull << 20, 3ull << 30, 288ull << 30, all}, helds[] = {0, 1ull << 16, 5ull << 30, all};
    for (unsigned long long mem_free : frees)
        for (unsigned long long held : helds)
            for (int nt : {1, 3, 8})
                for (int nr : {1, 4, 8}) {
                    const unsigned long long edge = (mem_free / 2 + held / 2) / (8ull * nt * nr + 4);
                    EXPECT(ar_array_fits(edge, nt, nr, mem_free, held) == 1);
                    EXPECT(ar_array_fits(edge + 1, nt, nr, mem_free, held) == 0);
                }
    EXPECT(ar_array_fits(1024 * 1024, 8, 8, 200ull << 30, 0) == 1);
    EXPECT(ar_array_fits(2000ull * 1000 * 1000, 8, 8, 288ull << 30, 0) == 0);  // (over 10^9 cells: what no quick GPU test can hold)
    // sizes whose product with the bytes per cell would wrap 64 bits
    EXPECT(ar_array_fits(all, 8, 8, 288ull << 30, 0) == 0 && ar_array_fits(all / 516 + 2, 8, 8, 288ull << 30, 0) == 0);
    EXPECT(ar_array_fits(all / 12 + 2, 1, 1, all, all) == 0 && ar_array_fits(1ull << 62, 1, 1, 1ull << 40, 0) == 0);
    EXPECT(ar_array_fits(0, 8, 8, 0, 0) == 1);
    // unit_dir: exact cases by bits ...
    float ux, uy;
    EXPECT(d2d::unit_dir(3.0f, 4.0f, ux, uy) && is(ux, 0.6f) && is(uy, 0.8f));
    EXPECT(d2d::unit_dir(-2.0f, 0.0f, ux, uy) && is(ux, -1.0f) && is(uy, 0.0f));
    EXPECT(d2d::unit_dir(0.0f, -0.5f, ux, uy) && is(ux, 0.0f) && is(uy, -1.0f));
    EXPECT(d2d::unit_dir(1.0f, -0.0f, ux, uy) && is(ux, 1.0f) && is(uy, -0.0f));
    EXPECT(d2d::unit_dir(1e19f, 0.0f, ux, uy) && is(ux, 1.0f));  // (1e38: the square is still finite)
    // ... and what has no direction: zero, squares that underflow to zero or overflow, NaN, inf
    EXPECT(!d2d::unit_dir(0.0f, 0.0f, ux, uy) && !d2d::unit_dir(-0.0f, 0.0f, ux, uy) && !d2d::unit_dir(-0.0f, -0.0f, ux, uy));
    EXPECT(!d2d::unit_dir(tiny, tiny, ux, uy) && !d2d::unit_dir(1e-30f, 0.0f, ux, uy));
    EXPECT(!d2d::unit_dir(1e30f, 1.0f, ux, uy) && !d2d::unit_dir(fmax, fmax, ux, uy) && !d2d::unit_dir(1.5e19f, 1.5e19f, ux, uy));
    EXPECT(!d2d::unit_dir(nan, 1.0f, ux, uy) && !d2d::unit_dir(1.0f, nan, ux, uy) && !d2d::unit_dir(inf, 1.0f, ux, uy) && !d2d::unit_dir(1.0f, -inf, ux, uy));
    // steer_phase: zero offsets of either sign leave the phase as it is, by bits ...
    const float below1 = std::nextafter(1.0f, 0.0f);
    for (float f0 : {0.0f, tiny, 0.125f, 0.375f, 0.7f, below1})
        for (float z1 : {0.0f, -0.0f})
            for (float z2 : {0.0f, -0.0f})
                for (float inv : {0.0f, 20.0f, 4096.0f}) EXPECT(is(d2d::steer_phase(f0, z1, z2, inv), f0));
    // ... the clamp: f0 = 0 and w = 1e-9 give v = -1e-9, v - floorf(v) = 1 - 1e-9 rounds to 1, and the clamp takes it to 0 ...
    EXPECT(is(d2d::steer_phase(0.0f, 1e-9f, 0.0f, 1.0f), 0.0f) && is(d2d::steer_phase(0.0f, 0.0f, 1e-9f, 1.0f), 0.0f));
    EXPECT(is(d2d::steer_phase(0.0f, tiny, 0.0f, 1.0f), 0.0f) && is(d2d::steer_phase(0.0f, 5e-11f, 0.0f, 20.0f), 0.0f));
    EXPECT(is(-1e-9f - std::floor(-1e-9f), 1.0f));  // (what the clamp is there for)
    // ... known phases ...
    EXPECT(is(d2d::steer_phase(0.5f, 0.25f, 0.0f, 1.0f), 0.25f) && is(d2d::steer_phase(0.25f, 0.5f, 0.0f, 1.0f), 0.75f));
    EXPECT(is(d2d::steer_phase(0.25f, -0.5f, -0.5f, 1.0f), 0.25f) && is(d2d::steer_phase(0.0f, 0.0125f, 0.0125f, 20.0f), 0.5f));
    EXPECT(is(d2d::steer_phase(0.0f, -1e-9f, 0.0f, 1.0f), 1e-9f));
    // ... always in [0, 1) for finite terms, NaN otherwise
    for (float f0 : {0.0f, 0.3f, below1})
        for (float q : {-7.3f, -1e-9f, 1e-9f, 0.011f, 3.0f, 1e30f, -1e30f})
            for (float inv : {1.0f, 20.0f, 1e3f}) {
                const float f = d2d::steer_phase(f0, q, -0.0021f, inv);
                EXPECT(f >= 0.0f && f < 1.0f);
            }
    EXPECT(std::isnan(d2d::steer_phase(nan, 0.0f, 0.0f, 1.0f)) && std::isnan(d2d::steer_phase(0.5f, nan, 0.0f, 1.0f)));
    EXPECT(std::isnan(d2d::steer_phase(0.5f, inf, 0.0f, 1.0f)) && std::isnan(d2d::steer_phase(0.5f, fmax, fmax, 1.0f)));
    // steer_dot: two products, one sum
    EXPECT(is(d2d::steer_dot(0.025f, -0.05f, 0.6f, 0.8f), 0.025f * 0.6f + -0.05f * 0.8f) && is(d2d::steer_dot(-0.0f, 0.0f, 0.6f, 0.8f), 0.0f));
    std::printf("array_response_host: %d failures\n", failures);
    return failures ? 1 : 0;
}
#endif
