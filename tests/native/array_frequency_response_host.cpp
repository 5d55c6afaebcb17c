// The host's share of d2d_array_frequency_response_launch (d2d_host.hpp: wide_params, wide_bytes_per_cell with outputs_fit, and
// chunks / chunk_plan with WIDE_CHUNK), compiled with plain g++.  Two builds of this file by tests/test_array_frequency_response_cpu.py: a shared library
// driven through ctypes, and -- with -DAFR_MAIN -- a stand-alone program that checks the same functions, refusals included; the
// program is also built with -fsanitize=address,undefined and run.  The product compiles the very same header into libd2d.so with
// hipcc.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../differt2d_amd/csrc/d2d_host.hpp"

extern "C" {

// The status of the list, the amplitude, the counts and the element lists (a list pointer may be NULL where its count is out of
// range: it is not read).  `index_out`: the number the message ends in, -1 where it ends in none.  `msg` (may be NULL) receives up
// to msg_len - 1 characters of the message.
int afr_params(const float* inv, int nf, int amplitude, int nt, const float* tx, int nr, const float* rx, int* index_out, char* msg, int msg_len) {
    std::string err;
    const int rc = d2d_host::wide_params(inv, nf, amplitude, nt, tx, nr, rx, err);
    if (index_out) {
        *index_out = -1;
        size_t k = err.size();
        while (k > 0 && err[k - 1] >= '0' && err[k - 1] <= '9') --k;
        if (k < err.size() && err.compare(k >= 10 ? k - 10 : 0, k >= 10 ? 10 : k, " at index ") == 0) *index_out = std::stoi(err.substr(k));
    }
    if (msg && msg_len > 0) {
        std::strncpy(msg, err.c_str(), (size_t)msg_len - 1);
        msg[msg_len - 1] = 0;
    }
    return (rc == D2D_OK) == err.empty() ? rc : -1000;  // (a refusal always says why)
}
long long afr_bytes_per_cell(int nf, int nt, int nr) { return (long long)d2d_host::wide_bytes_per_cell(nf, nt, nr); }
int afr_fits(unsigned long long cells, int nf, int nt, int nr, unsigned long long mem_free, unsigned long long held) {
    return d2d_host::outputs_fit((size_t)cells, d2d_host::wide_bytes_per_cell(nf, nt, nr), (size_t)mem_free, (size_t)held) ? 1 : 0;
}
int afr_chunk_size() { return d2d_host::WIDE_CHUNK; }
int afr_chunks(int nf) { return d2d_host::chunks(nf, d2d_host::WIDE_CHUNK); }
void afr_chunk(int nf, int i, int* first, int* count, int* with_total) {
    const d2d_host::Chunk ch = d2d_host::chunk_plan(nf, i, d2d_host::WIDE_CHUNK);
    *first = ch.first, *count = ch.count, *with_total = ch.with_total ? 1 : 0;
}
}

#ifdef AFR_MAIN
static int failures = 0;
#define EXPECT(x)                                                \
    do {                                                         \
        if (!(x)) {                                              \
            std::printf("line %d: %s does not hold\n", __LINE__, #x); \
            ++failures;                                          \
        }                                                        \
    } while (0)

static bool has(const char* msg, const char* word) { return std::strstr(msg, word) != nullptr; }

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float fmax = std::numeric_limits<float>::max(), tiny = std::numeric_limits<float>::denorm_min();
    char msg[256];
    int at = 0;
    // wide_params: both limits of all three counts (lists of exactly the size that is read: the sanitizer sees a read past them) ...
    for (int nf : {1, 9, D2D_FREQ_MAX})
        for (int nt : {1, D2D_ARRAY_MAX})
            for (int nr : {1, D2D_ARRAY_MAX}) {
                std::vector<float> inv((size_t)nf, 20.0f), tx(2 * (size_t)nt, 0.025f), rx(2 * (size_t)nr, -0.0f);
                inv[(size_t)nf - 1] = 0.0f;  // (an entry 0 is allowed)
                EXPECT(afr_params(inv.data(), nf, D2D_FIELD_AMP_SQRT, nt, tx.data(), nr, rx.data(), &at, msg, 256) == D2D_OK && at == -1);
                EXPECT(afr_params(inv.data(), nf, D2D_FIELD_AMP_LINEAR, nt, tx.data(), nr, rx.data(), &at, msg, 256) == D2D_OK);
                // ... a bad entry at the first, a middle and the last position of the list, with its index at the message's end ...
                for (float bad : {nan, inf, -inf, -1.0f, -tiny})
                    for (int k : {0, nf / 2, nf - 1}) {
                        std::vector<float> v2 = inv;
                        v2[(size_t)k] = bad;
                        EXPECT(afr_params(v2.data(), nf, 0, nt, tx.data(), nr, rx.data(), &at, msg, 256) == D2D_ERR_INVALID && at == k &&
                               has(msg, "inv_wavelength"));
                    }
                // ... every bad position of both element lists, with the element's index at the message's end ...
                for (float bad : {nan, inf, -inf}) {
                    for (int k = 0; k < 2 * nt; ++k) {
                        std::vector<float> t2 = tx;
                        t2[(size_t)k] = bad;
                        EXPECT(afr_params(inv.data(), nf, 0, nt, t2.data(), nr, rx.data(), &at, msg, 256) == D2D_ERR_INVALID && at == k / 2 &&
                               has(msg, "tx_elems"));
                    }
                    for (int k = 0; k < 2 * nr; ++k) {
                        std::vector<float> r2 = rx;
                        r2[(size_t)k] = bad;
                        EXPECT(afr_params(inv.data(), nf, 0, nt, tx.data(), nr, r2.data(), &at, msg, 256) == D2D_ERR_INVALID && at == k / 2 &&
                               has(msg, "rx_elems"));
                    }
                }
                // ... the largest finite values pass
                tx[0] = fmax, rx[1] = -fmax, inv[0] = fmax;
                EXPECT(afr_params(inv.data(), nf, 0, nt, tx.data(), nr, rx.data(), &at, msg, 256) == D2D_OK);
            }
    {
        // counts out of range: the list of that count is not read (the pointers are NULL)
        const float one[2] = {0.0f, 0.0f};
        for (int bad : {0, -1, D2D_FREQ_MAX + 1, 1 << 30, -(1 << 30)})
            EXPECT(afr_params(nullptr, bad, 0, 1, one, 1, one, &at, msg, 256) == D2D_ERR_INVALID && at == -1 && has(msg, "nf in 1 .. 1024"));
        for (int bad : {0, -1, D2D_ARRAY_MAX + 1, 1 << 30, -(1 << 30)}) {
            EXPECT(afr_params(one, 1, 0, bad, nullptr, 1, nullptr, &at, msg, 256) == D2D_ERR_INVALID && at == -1 && has(msg, "nt in 1 .. 8"));
            EXPECT(afr_params(one, 1, 0, 1, nullptr, bad, nullptr, &at, msg, 256) == D2D_ERR_INVALID && at == -1 && has(msg, "nr in 1 .. 8"));
        }
        for (int bad : {2, -1}) EXPECT(afr_params(one, 1, bad, 1, one, 1, one, &at, msg, 256) == D2D_ERR_INVALID && at == -1 && has(msg, "amplitude"));
        // the list's checks come before the element lists'
        const float badinv[3] = {1.0f, 2.0f, nan}, badrx[4] = {0.0f, 0.0f, 0.0f, nan};
        EXPECT(afr_params(badinv, 3, 0, 1, one, 2, badrx, &at, msg, 256) == D2D_ERR_INVALID && at == 2 && has(msg, "inv_wavelength"));
        EXPECT(afr_params(badinv, 2, 0, 1, one, 2, badrx, &at, msg, 256) == D2D_ERR_INVALID && at == 1 && has(msg, "rx_elems"));
    }
    // wide_bytes_per_cell and outputs_fit: 8 * nf * nr * nt + 4 bytes per cell against half of (free + held), at the boundary and one past it
    EXPECT(D2D_FREQ_MAX == 1024 && D2D_ARRAY_MAX == 8);
    EXPECT(afr_bytes_per_cell(1, 1, 1) == 12 && afr_bytes_per_cell(64, 4, 4) == 8196 && afr_bytes_per_cell(9, 4, 3) == 868);
    EXPECT(afr_bytes_per_cell(1024, 8, 8) == 524292);
    const unsigned long long all = ~0ull;
    const unsigned long long frees[] = {0, 1ull << 20, 3ull << 30, 288ull << 30, all}, helds[] = {0, 1ull << 16, 5ull << 30, all};
    for (unsigned long long mem_free : frees)
        for (unsigned long long held : helds)
            for (int nf : {1, 33, 1024})
                for (int nt : {1, 3, 8})
                    for (int nr : {1, 4, 8}) {
                        const unsigned long long per = 8ull * nf * nt * nr + 4;
                        const unsigned long long edge = (mem_free / 2 + held / 2) / per;
                        EXPECT((unsigned long long)afr_bytes_per_cell(nf, nt, nr) == per);
                        EXPECT(afr_fits(edge, nf, nt, nr, mem_free, held) == 1);
                        EXPECT(afr_fits(edge + 1, nf, nt, nr, mem_free, held) == 0);
                    }
    // the boundary byte: 1024^2 cells of 64 wavelengths of a 4 x 4 matrix need 8196 MiB: twice that free fits, two bytes less do not
    EXPECT(afr_fits(1ull << 20, 64, 4, 4, 2 * (8196ull << 20), 0) == 1 && afr_fits(1ull << 20, 64, 4, 4, 2 * (8196ull << 20) - 2, 0) == 0);
    EXPECT(afr_fits(1ull << 20, 64, 4, 4, 0, 2 * (8196ull << 20)) == 1 && afr_fits(1ull << 20, 64, 4, 4, 0, 2 * (8196ull << 20) - 2) == 0);
    EXPECT(afr_fits(1ull << 20, 1024, 8, 8, 288ull << 30, 0) == 0);  // (512 GiB: what no GPU test can hold)
    // sizes whose product with the bytes per cell would wrap 64 bits
    EXPECT(afr_fits(all, 1024, 8, 8, 288ull << 30, 0) == 0 && afr_fits(all / 524292 + 2, 1024, 8, 8, 288ull << 30, 0) == 0);
    EXPECT(afr_fits(all / 12 + 2, 1, 1, 1, all, all) == 0 && afr_fits(1ull << 62, 1, 1, 1, 1ull << 40, 0) == 0);
    EXPECT(afr_fits(0, 1024, 8, 8, 0, 0) == 1);
    // counts out of range (the launch has refused them before): no bytes, nothing fits, no product of the three is formed
    for (int bad : {0, -1, 1 << 30}) {
        EXPECT(afr_bytes_per_cell(bad, 1, 1) == 0 && afr_bytes_per_cell(1, bad, 1) == 0 && afr_bytes_per_cell(1, 1, bad) == 0);
        EXPECT(afr_fits(1, bad, 1, 1, all, all) == 0 && afr_fits(1, 1, bad, 1, all, all) == 0 && afr_fits(1, 1, 1, bad, all, all) == 0);
    }
    EXPECT(afr_bytes_per_cell(1025, 1, 1) == 0 && afr_bytes_per_cell(1, 9, 1) == 0 && afr_bytes_per_cell(1, 1, 9) == 0);
    // the chunks: for every nf they cover 0 .. nf-1 once and in order, only the first carries total, every count is in 1 .. WIDE_CHUNK
    const int W = afr_chunk_size();
    EXPECT(W >= 8 && W <= 64 && (W & (W - 1)) == 0);
    for (int nf = 1; nf <= D2D_FREQ_MAX; ++nf) {
        int next = 0;
        const int n = afr_chunks(nf);
        EXPECT(n == (nf + W - 1) / W);
        for (int i = 0; i < n; ++i) {
            int first = -1, count = -1, with_total = -1;
            afr_chunk(nf, i, &first, &count, &with_total);
            EXPECT(first == next && count >= 1 && count <= W && with_total == (i == 0 ? 1 : 0));
            next = first + count;
        }
        EXPECT(next == nf);
    }
    std::printf("array_frequency_response_host: %d failures\n", failures);
    return failures ? 1 : 0;
}
#endif
