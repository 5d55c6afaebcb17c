// The host's share of d2d_beam_response_launch, compiled with plain g++: the arithmetic of d2d_beam.hpp (beam_steer, the two folds and
// the pair product -- the very text the kernel compiles) and d2d_host.hpp's beam_params and beam_bytes_per_cell with outputs_fit and
// the chunk plan with BEAM_CHUNK.  Two builds of this file by tests/test_beam_response_cpu.py: a shared library driven through
// ctypes, and -- with -DBEAM_MAIN -- a stand-alone program that checks the same functions, refusals included; the program is also
// built with -fsanitize=address,undefined and run.  The product compiles the very same headers into libd2d.so with hipcc.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../differt2d_amd/csrc/d2d_beam.hpp"
#include "../../differt2d_amd/csrc/d2d_host.hpp"

extern "C" {

// d2d_beam.hpp element by element: (c, s) = beam_steer(q, inv); (tx_re, tx_im) = beam_fold_tx from (a_re, a_im) with the weight and
// that phasor; (rx_re, rx_im) = beam_fold_rx likewise; (zr, zs) = beam_pair((a_re, a_im), (b_re, b_im), phasor(f0)).
void beam_arith(const float* q, const float* inv, const float* w_re, const float* w_im, const float* a_re, const float* a_im, const float* b_re,
                const float* b_im, const float* f0, long long n, float* c, float* s, float* tx_re, float* tx_im, float* rx_re, float* rx_im, float* zr,
                float* zs) {
    for (long long k = 0; k < n; ++k) {
        d2d::beam_steer(q[k], inv[k], c[k], s[k]);
        tx_re[k] = rx_re[k] = a_re[k];
        tx_im[k] = rx_im[k] = a_im[k];
        d2d::beam_fold_tx(tx_re[k], tx_im[k], w_re[k], w_im[k], c[k], s[k]);
        d2d::beam_fold_rx(rx_re[k], rx_im[k], w_re[k], w_im[k], c[k], s[k]);
        float c0, s0;
        d2d::phasor(f0[k], c0, s0);
        d2d::beam_pair(a_re[k], a_im[k], b_re[k], b_im[k], c0, s0, zr[k], zs[k]);
    }
}

// The status of beam_params (a list pointer may be NULL where it is not read).  `index_out`: the number the message ends in, -1 where
// it ends in none.  `msg` (may be NULL) receives up to msg_len - 1 characters of the message.
int beam_params(const float* inv, int nf, int amplitude, int nt, const float* tx, int nr, const float* rx, int nbt, const float* wtx, int nbr,
                const float* wrx, int* index_out, char* msg, int msg_len) {
    std::string err;
    const int rc = d2d_host::beam_params(inv, nf, amplitude, nt, tx, nr, rx, nbt, wtx, nbr, wrx, err);
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
long long beam_bytes_per_cell(int nf, int nbt, int nbr) { return (long long)d2d_host::beam_bytes_per_cell(nf, nbt, nbr); }
int beam_fits(unsigned long long cells, int nf, int nbt, int nbr, unsigned long long mem_free, unsigned long long held) {
    return d2d_host::outputs_fit((size_t)cells, d2d_host::beam_bytes_per_cell(nf, nbt, nbr), (size_t)mem_free, (size_t)held) ? 1 : 0;
}
int beam_chunk_size() { return d2d_host::BEAM_CHUNK; }
int beam_chunks(int nf) { return d2d_host::chunks(nf, d2d_host::BEAM_CHUNK); }
void beam_chunk(int nf, int i, int* first, int* count, int* with_total) {
    const d2d_host::Chunk ch = d2d_host::chunk_plan(nf, i, d2d_host::BEAM_CHUNK);
    *first = ch.first, *count = ch.count, *with_total = ch.with_total ? 1 : 0;
}
int beam_max() { return D2D_BEAM_MAX; }
}

#ifdef BEAM_MAIN
static int failures = 0;
#define EXPECT(x)                                                     \
    do {                                                              \
        if (!(x)) {                                                   \
            std::printf("line %d: %s does not hold\n", __LINE__, #x); \
            ++failures;                                               \
        }                                                             \
    } while (0)

static bool has(const char* msg, const char* word) { return std::strstr(msg, word) != nullptr; }
static bool same(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float fmax = std::numeric_limits<float>::max();
    char msg[256];
    int at = 0;
    // ---- the arithmetic: what the definition states outright
    float c, s;
    for (float q : {0.0f, -0.0f})
        for (float inv : {0.0f, 20.0f, fmax}) {
            d2d::beam_steer(q, inv, c, s);
            EXPECT(same(c, 1.0f) && same(s, 0.0f));  // steer(+-0) = phasor(+0) = (1, +0) by bits
        }
    d2d::beam_steer(2.5f, 0.0f, c, s);
    EXPECT(same(c, 1.0f) && same(s, 0.0f));  // a zero inverse wavelength: every phase is 0
    d2d::beam_steer(-1e-9f, 1.0f, c, s);
    EXPECT(same(c, 1.0f) && same(s, 0.0f));  // v just below zero: g rounds to 1 and is taken to 0
    d2d::beam_steer(std::nextafterf(3.0f, 0.0f), 1.0f, c, s);
    EXPECT(c > 0.999f && c <= 1.0f && s < 0.0f && s > -1e-5f);  // q * inv just below an integer: just below a full turn
    d2d::beam_steer(0.0125f, 20.0f, c, s);
    EXPECT(std::fabs(c) < 1e-6f && std::fabs(s - 1.0f) < 1e-6f);  // a quarter turn
    d2d::beam_steer(0.25f, 1.0f, c, s);
    EXPECT(same(c, -0.0f) && same(s, 1.0f));  // an exact quarter turn: the rotation alone (k = 1: c = -s0 = -0)
    for (float bad : {nan, inf, -inf}) {
        d2d::beam_steer(bad, 1.0f, c, s);
        EXPECT(c != c && s != s);
        d2d::beam_steer(1.0f, bad, c, s);
        EXPECT(c != c && s != s);
    }
    {
        // the one-antenna chain: At = Ar = (1, +0), P = (1, +0), zr = c0 and zs = s0 as values
        float atr = 0.0f, ati = 0.0f, arr = 0.0f, ari = 0.0f, zr, zs;
        d2d::beam_fold_tx(atr, ati, 1.0f, 0.0f, 1.0f, 0.0f);
        d2d::beam_fold_rx(arr, ari, 1.0f, 0.0f, 1.0f, 0.0f);
        EXPECT(same(atr, 1.0f) && same(ati, 0.0f) && same(arr, 1.0f) && same(ari, 0.0f));
        for (float f0 : {0.0f, 0.125f, 0.25f, 0.3f, 0.5f, 0.75f, 0.999f}) {
            float c0, s0;
            d2d::phasor(f0, c0, s0);
            d2d::beam_pair(arr, ari, atr, ati, c0, s0, zr, zs);
            EXPECT(zr == c0 && zs == s0);
        }
        // the folds: w * (c + j s) and conj(w) * (c + j s) on exact inputs, added to what was there
        atr = 10.0f, ati = 20.0f, arr = 10.0f, ari = 20.0f;
        d2d::beam_fold_tx(atr, ati, 2.0f, 3.0f, 0.5f, -0.25f);  // (2 + 3j)(0.5 - 0.25j) = 1.75 + 1j
        d2d::beam_fold_rx(arr, ari, 2.0f, 3.0f, 0.5f, -0.25f);  // (2 - 3j)(0.5 - 0.25j) = 0.25 - 2j
        EXPECT(same(atr, 11.75f) && same(ati, 21.0f) && same(arr, 10.25f) && same(ari, 18.0f));
        // the pair: P = (1 + 2j)(3 - 1j) = 5 + 5j; at f0 = 0.25 (c0 = -0, s0 = 1): P e^(-j pi / 2) = 5 - 5j = zr - j zs
        float c0, s0;
        d2d::phasor(0.25f, c0, s0);
        d2d::beam_pair(1.0f, 2.0f, 3.0f, -1.0f, c0, s0, zr, zs);
        EXPECT(zr == 5.0f && zs == 5.0f);
    }
    // ---- beam_params: both limits of all five counts (lists of exactly the size that is read: the sanitizer sees a read past them)
    for (int nf : {1, D2D_FREQ_MAX})
        for (int nt : {1, 3, D2D_ARRAY_MAX})
            for (int nr : {1, D2D_ARRAY_MAX})
                for (int nbt : {1, D2D_BEAM_MAX})
                    for (int nbr : {1, 5, D2D_BEAM_MAX}) {
                        std::vector<float> inv((size_t)nf, 20.0f), tx(2 * (size_t)nt, 0.025f), rx(2 * (size_t)nr, -0.0f);
                        std::vector<float> wtx(2 * (size_t)nbt * nt, 0.5f), wrx(2 * (size_t)nbr * nr, -0.0f);
                        wtx[0] = fmax, wrx[wrx.size() - 1] = -fmax;  // (the largest finite values pass, and so do zeros)
                        EXPECT(beam_params(inv.data(), nf, 0, nt, tx.data(), nr, rx.data(), nbt, wtx.data(), nbr, wrx.data(), &at, msg, 256) == D2D_OK && at == -1);
                        EXPECT(beam_params(inv.data(), nf, 1, nt, tx.data(), nr, rx.data(), nbt, wtx.data(), nbr, wrx.data(), &at, msg, 256) == D2D_OK);
                        // every bad position of both weight tables: the table and the beam named, the element's index at the end
                        for (float bad : {nan, inf, -inf}) {
                            for (size_t k = 0; k < wtx.size(); ++k) {
                                std::vector<float> w2 = wtx;
                                w2[k] = bad;
                                const std::string beam = "beam " + std::to_string(k / 2 / (size_t)nt) + " ";
                                EXPECT(beam_params(inv.data(), nf, 0, nt, tx.data(), nr, rx.data(), nbt, w2.data(), nbr, wrx.data(), &at, msg, 256) == D2D_ERR_INVALID &&
                                       at == (int)(k / 2 % (size_t)nt) && has(msg, "tx_weights") && has(msg, beam.c_str()) && has(msg, k % 2 ? "im" : "re"));
                            }
                            for (size_t k = 0; k < wrx.size(); ++k) {
                                std::vector<float> w2 = wrx;
                                w2[k] = bad;
                                const std::string beam = "beam " + std::to_string(k / 2 / (size_t)nr) + " ";
                                EXPECT(beam_params(inv.data(), nf, 0, nt, tx.data(), nr, rx.data(), nbt, wtx.data(), nbr, w2.data(), &at, msg, 256) == D2D_ERR_INVALID &&
                                       at == (int)(k / 2 % (size_t)nr) && has(msg, "rx_weights") && has(msg, beam.c_str()));
                            }
                        }
                    }
    {
        const float one[2] = {0.0f, 0.0f}, w1[2] = {1.0f, 0.0f};
        // what wide_params refuses comes first and in its order; the weight tables are not read then (NULL)
        for (int bad : {0, -1, D2D_FREQ_MAX + 1})
            EXPECT(beam_params(nullptr, bad, 0, 1, one, 1, one, 1, nullptr, 1, nullptr, &at, msg, 256) == D2D_ERR_INVALID && has(msg, "nf in 1 .. 1024"));
        for (int bad : {0, -1, D2D_ARRAY_MAX + 1, 1 << 30}) {
            EXPECT(beam_params(one, 1, 0, bad, nullptr, 1, nullptr, 1, nullptr, 1, nullptr, &at, msg, 256) == D2D_ERR_INVALID && has(msg, "nt in 1 .. 8"));
            EXPECT(beam_params(one, 1, 0, 1, nullptr, bad, nullptr, 1, nullptr, 1, nullptr, &at, msg, 256) == D2D_ERR_INVALID && has(msg, "nr in 1 .. 8"));
        }
        for (int bad : {2, -1}) EXPECT(beam_params(one, 1, bad, 1, one, 1, one, 1, w1, 1, w1, &at, msg, 256) == D2D_ERR_INVALID && has(msg, "amplitude"));
        const float badinv[2] = {1.0f, nan}, badrx[4] = {0.0f, 0.0f, 0.0f, inf};
        EXPECT(beam_params(badinv, 2, 0, 1, one, 1, one, 0, nullptr, 0, nullptr, &at, msg, 256) == D2D_ERR_INVALID && at == 1 && has(msg, "inv_wavelength"));
        EXPECT(beam_params(badinv, 1, 0, 1, one, 2, badrx, 0, nullptr, 0, nullptr, &at, msg, 256) == D2D_ERR_INVALID && at == 1 && has(msg, "rx_elems"));
        // then nbt, then nbr: neither table is read
        for (int bad : {0, -1, D2D_BEAM_MAX + 1, 1 << 30, -(1 << 30)}) {
            EXPECT(beam_params(one, 1, 0, 1, one, 1, one, bad, nullptr, 1, nullptr, &at, msg, 256) == D2D_ERR_INVALID && at == -1 && has(msg, "nbt in 1 .. 8"));
            EXPECT(beam_params(one, 1, 0, 1, one, 1, one, 1, nullptr, bad, nullptr, &at, msg, 256) == D2D_ERR_INVALID && at == -1 && has(msg, "nbr in 1 .. 8"));
            EXPECT(beam_params(one, 1, 0, 1, one, 1, one, bad, nullptr, bad, nullptr, &at, msg, 256) == D2D_ERR_INVALID && has(msg, "nbt in 1 .. 8"));
        }
        // the transmit table's check comes before the receive table's
        const float badw[2] = {nan, 0.0f};
        EXPECT(beam_params(one, 1, 0, 1, one, 1, one, 1, badw, 1, badw, &at, msg, 256) == D2D_ERR_INVALID && at == 0 && has(msg, "tx_weights"));
        EXPECT(beam_params(one, 1, 0, 1, one, 1, one, 1, w1, 1, badw, &at, msg, 256) == D2D_ERR_INVALID && at == 0 && has(msg, "rx_weights"));
    }
    // ---- beam_bytes_per_cell and outputs_fit: 8 * nf * nbr * nbt + 4 bytes per cell against half of (free + held)
    EXPECT(D2D_BEAM_MAX == 8 && beam_max() == 8);
    EXPECT(beam_bytes_per_cell(1, 1, 1) == 12 && beam_bytes_per_cell(64, 1, 1) == 516 && beam_bytes_per_cell(64, 8, 8) == 32772);
    EXPECT(beam_bytes_per_cell(9, 3, 2) == 436 && beam_bytes_per_cell(1024, 8, 8) == 524292);
    const unsigned long long all = ~0ull;
    const unsigned long long frees[] = {0, 1ull << 20, 3ull << 30, 288ull << 30, all}, helds[] = {0, 1ull << 16, 5ull << 30, all};
    for (unsigned long long mem_free : frees)
        for (unsigned long long held : helds)
            for (int nf : {1, 33, 1024})
                for (int nbt : {1, 3, 8})
                    for (int nbr : {1, 4, 8}) {
                        const unsigned long long per = 8ull * nf * nbt * nbr + 4;
                        const unsigned long long edge = (mem_free / 2 + held / 2) / per;
                        EXPECT((unsigned long long)beam_bytes_per_cell(nf, nbt, nbr) == per);
                        EXPECT(beam_fits(edge, nf, nbt, nbr, mem_free, held) == 1);
                        EXPECT(beam_fits(edge + 1, nf, nbt, nbr, mem_free, held) == 0);
                    }
    // the boundary byte: 1024^2 cells of 64 wavelengths of one beam pair need 516 MiB: twice that free fits, two bytes less do not
    EXPECT(beam_fits(1ull << 20, 64, 1, 1, 2 * (516ull << 20), 0) == 1 && beam_fits(1ull << 20, 64, 1, 1, 2 * (516ull << 20) - 2, 0) == 0);
    EXPECT(beam_fits(1ull << 20, 1024, 8, 8, 288ull << 30, 0) == 0);  // (512 GiB: what no GPU test can hold)
    EXPECT(beam_fits(all, 1024, 8, 8, 288ull << 30, 0) == 0 && beam_fits(all / 524292 + 2, 1024, 8, 8, 288ull << 30, 0) == 0);
    EXPECT(beam_fits(all / 12 + 2, 1, 1, 1, all, all) == 0 && beam_fits(0, 1024, 8, 8, 0, 0) == 1);
    for (int bad : {0, -1, 9, 1 << 30}) {
        EXPECT(beam_bytes_per_cell(1, bad, 1) == 0 && beam_bytes_per_cell(1, 1, bad) == 0);
        EXPECT(beam_fits(1, 1, bad, 1, all, all) == 0 && beam_fits(1, 1, 1, bad, all, all) == 0);
    }
    EXPECT(beam_bytes_per_cell(0, 1, 1) == 0 && beam_bytes_per_cell(1025, 1, 1) == 0);
    // ---- the chunks: for every nf they cover 0 .. nf-1 once and in order, only the first carries total
    const int W = beam_chunk_size();
    EXPECT(W >= 8 && W <= 64 && (W & (W - 1)) == 0);
    for (int nf = 1; nf <= D2D_FREQ_MAX; ++nf) {
        int next = 0;
        const int n = beam_chunks(nf);
        EXPECT(n == (nf + W - 1) / W);
        for (int i = 0; i < n; ++i) {
            int first = -1, count = -1, with_total = -1;
            beam_chunk(nf, i, &first, &count, &with_total);
            EXPECT(first == next && count >= 1 && count <= W && with_total == (i == 0 ? 1 : 0));
            next = first + count;
        }
        EXPECT(next == nf);
    }
    std::printf("beam_response_host: %d failures\n", failures);
    return failures ? 1 : 0;
}
#endif
