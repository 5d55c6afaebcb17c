// Host-only logic of libd2d.so that needs neither a device nor the HIP headers: candidate enumeration (the stand-in for
// differt-core's Rust graph iterator, differt2d/scene.py:153-175), parameter validation, lax.integer_pow, the
// scalar thresholds of a sweep, the bins of the power-delay profile, and the buffer-size arithmetic of the sweep launches (LDS tables, the contribution lists
// of the patches cut in four and their 4 GiB guard).  d2d.hip uses these functions as they are; tests/native/d2d_host_san.cpp compiles the same header with
// g++ -fsanitize=address,undefined and tests/test_host_sanitizers.py drives it (sanitizers run on the CPU build only).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/d2d.h"
#include "d2d_chunks.hpp"

namespace d2d_host {

// lax.integer_pow lowering (square and multiply), fp32
inline float integer_pow(float x, int n) {
    if (n == 0) return 1.0f;
    float acc = 0.0f;
    bool have = false;
    while (n > 0) {
        if (n & 1) {
            acc = have ? acc * x : x;
            have = true;
        }
        n >>= 1;
        if (n > 0) x = x * x;
    }
    return acc;
}

// 64-bit content hash of an fp32 array (bit patterns: -0.0 != 0.0, every NaN payload its own value), four independent
// multiply-xor lanes over 8-byte words so that the loop runs at memory speed.  d2d_set_grid uses it to recognise a grid it
// already holds (a caller of the reference's API passes X, Y with every call: scene.py:1803-1826).
inline uint64_t hash_floats(const float* p, size_t n, uint64_t seed) {
    const uint64_t K0 = 0x9E3779B97F4A7C15ull, K1 = 0xC2B2AE3D27D4EB4Full, K2 = 0x165667B19E3779F9ull, K3 = 0xD6E8FEB86659FD93ull;
    uint64_t h0 = seed ^ K0, h1 = seed ^ K1, h2 = seed ^ K2, h3 = seed ^ K3;
    size_t i = 0;
    auto word = [&](size_t at) {
        uint64_t w;
        __builtin_memcpy(&w, p + at, 8);
        return w;
    };
    for (; i + 8 <= n; i += 8) {
        h0 = (h0 ^ word(i)) * K1;
        h1 = (h1 ^ word(i + 2)) * K2;
        h2 = (h2 ^ word(i + 4)) * K3;
        h3 = (h3 ^ word(i + 6)) * K0;
        h0 ^= h0 >> 29;
        h1 ^= h1 >> 31;
        h2 ^= h2 >> 30;
        h3 ^= h3 >> 28;
    }
    for (; i < n; ++i) {
        uint32_t w;
        __builtin_memcpy(&w, p + i, 4);
        h0 = (h0 ^ (uint64_t)w) * K2;
        h0 ^= h0 >> 31;
    }
    uint64_t h = h0 ^ (h1 * K3) ^ (h2 * K0) ^ (h3 * K1) ^ ((uint64_t)n * K2);
    h ^= h >> 33;
    h *= 0xFF51AFD7ED558CCDull;
    h ^= h >> 33;
    h *= 0xC4CEB9FE1A85EC53ull;
    h ^= h >> 33;
    return h;
}

// candidates of order k over nc allowed objects: nc (nc - 1)^(k-1), 1 for k = 0; saturates at INT64_MAX
inline int64_t count_order(int64_t nc, int k) {
    if (k == 0) return 1;
    if (nc <= 0) return 0;
    int64_t c = nc;
    for (int i = 1; i < k; ++i) {
        if (nc - 1 != 0 && c > INT64_MAX / (nc - 1)) return INT64_MAX;
        c *= (nc - 1);
    }
    return c;
}

// status (D2D_OK or negative) + message
inline int count_candidates(int32_t n_objects, const uint8_t* allowed, int32_t min_order, int32_t max_order, int64_t* count,
                            std::string& err) {
    if (!count) return err = "count is NULL", D2D_ERR_INVALID;
    if (n_objects < 0 || min_order < 0) return err = "negative argument", D2D_ERR_INVALID;
    int64_t nc = 0;
    for (int j = 0; j < n_objects; ++j) nc += (!allowed || allowed[j]) ? 1 : 0;
    int64_t total = 0;
    for (int k = min_order; k <= max_order; ++k) {
        const int64_t ck = count_order(nc, k);
        if (ck > INT64_MAX - total) return err = "the number of candidates overflows int64", D2D_ERR_INVALID;
        total += ck;
    }
    *count = total;
    return D2D_OK;
}

// For each order k ascending, every tuple of k allowed object indices with no two equal neighbours, lexicographic
// (recorded order: docs/source/notebooks/cost20120_helsinki_model.ipynb cell 20).  cand: [count][D2D_MAX_ORDER], -1 padded.
inline int enumerate_candidates(int32_t n_objects, const uint8_t* allowed, int32_t min_order, int32_t max_order, int32_t* cand,
                                int32_t* order, int64_t capacity, std::string& err) {
    if (min_order < 0 || max_order > D2D_MAX_ORDER) return err = "orders must lie in [0, " + std::to_string(D2D_MAX_ORDER) + "]", D2D_ERR_INVALID;
    int64_t total = 0;
    int rc = count_candidates(n_objects, allowed, min_order, max_order, &total, err);
    if (rc) return rc;
    if (capacity < total) return err = "capacity " + std::to_string(capacity) + " < " + std::to_string(total) + " candidates", D2D_ERR_INVALID;
    std::vector<int> cw;
    for (int j = 0; j < n_objects; ++j)
        if (!allowed || allowed[j]) cw.push_back(j);
    const int nc = (int)cw.size();
    int64_t at = 0;
    for (int k = min_order; k <= max_order; ++k) {
        if (k == 0) {
            if (cand) for (int i = 0; i < D2D_MAX_ORDER; ++i) cand[at * D2D_MAX_ORDER + i] = -1;
            if (order) order[at] = 0;
            ++at;
            continue;
        }
        // odometer over positions in the compact list: lexicographic, no equal neighbours
        int pos[D2D_MAX_ORDER];
        int depth = 0;
        pos[0] = -1;
        while (depth >= 0) {
            int p = pos[depth] + 1;
            if (depth > 0 && p == pos[depth - 1]) ++p;
            if (p >= nc) {
                --depth;
                continue;
            }
            pos[depth] = p;
            if (depth == k - 1) {
                if (cand)
                    for (int i = 0; i < D2D_MAX_ORDER; ++i) cand[at * D2D_MAX_ORDER + i] = (i < k) ? cw[pos[i]] : -1;
                if (order) order[at] = k;
                ++at;
            } else {
                ++depth;
                pos[depth] = -1;
            }
        }
    }
    return D2D_OK;
}

inline int check_params(const d2d_params* p, std::string& err) {
    if (!p) return err = "params is NULL", D2D_ERR_INVALID;
    if (p->min_order < 0 || p->max_order > D2D_MAX_ORDER)
        return err = "orders must lie in [0, " + std::to_string(D2D_MAX_ORDER) + "], got [" + std::to_string(p->min_order) + ", " +
                     std::to_string(p->max_order) + "]", D2D_ERR_INVALID;
    if (p->approx && !(p->alpha > 0.0f)) return err = "alpha must be > 0 in approx mode", D2D_ERR_INVALID;
    if (p->approx && p->act != D2D_ACT_HARD_SIGMOID && p->act != D2D_ACT_SIGMOID)
        return err = "activation " + std::to_string(p->act) + " is not one of the native activations", D2D_ERR_UNSUPPORTED;
    if (p->fun_id < 0 || p->fun_id > D2D_FUN_RECEIVED_POWER_PER_OBJECT) return err = "fun_id " + std::to_string(p->fun_id) + " is not a native path function", D2D_ERR_UNSUPPORTED;
    if (p->out_mode != D2D_OUT_OVERWRITE && p->out_mode != D2D_OUT_ADD) return err = "bad out_mode " + std::to_string(p->out_mode), D2D_ERR_INVALID;
    if (p->grid_role != D2D_GRID_RX && p->grid_role != D2D_GRID_TX) return err = "bad grid_role " + std::to_string(p->grid_role), D2D_ERR_INVALID;
    if (!(p->seg_tol >= 0.0f)) return err = "seg_tol must be >= 0", D2D_ERR_INVALID;
    return D2D_OK;
}

// ---- buffer sizes of the forward sweep ----------------------------------------------------------------------------
constexpr size_t LDS_LIMIT = 64 * 1024;  // dynamic LDS the launches that have a choice ask for (of the CU's 160 KB: several workgroups stay resident)
constexpr size_t LDS_MAX = 156 * 1024;    // ... and what a launch without a choice may take: one workgroup per CU (gfx950 grants a workgroup the
                                          // CU's whole 160 KB without an attribute, scripts/probes/lds_limit_probe.hip; 4 KB left for static LDS)
constexpr size_t F4 = 16;                // sizeof(float4)

// one-wave-per-patch kernels: [2N] refl + [N] flt + [N] adjoint table (float4 each) + 1 spare + one 512-byte culling queue
inline size_t tab_lds_bytes(int n_objects) { return (size_t)(4 * (size_t)n_objects + 1) * F4 + 512; }

struct SplitLds {
    size_t base;   // byte offset of the culling queues (16-byte aligned)
    size_t total;  // dynamic LDS of power_fwd_split_kernel
};
// shared-patch kernel (W waves): tables, (W - 1) contribution lists of list_len x 64 floats, their bookkeeping, W queues
inline SplitLds split_lds_bytes(int n_objects, int W, int list_len) {
    SplitLds s;
    s.base = ((tab_lds_bytes(n_objects) - 512 + (size_t)(W - 1) * (size_t)list_len * 64 * sizeof(float) +
               (size_t)((W - 1) * 65 + W + 1) * sizeof(int)) + 15) & ~(size_t)15;
    s.total = s.base + (size_t)W * 512;
    return s;
}

// candidate-sharing kernel (W waves, power_fwd_coop_kernel): tables + the rounds' slots [W][C][64]
inline size_t coop_lds_bytes(int n_objects, int W, int C) {
    return (size_t)(3 * n_objects + 1) * 16 + (size_t)W * (size_t)C * 64 * sizeof(float);
}

struct HeavyPlan {
    long long H = 0;           // patches cut in `parts` (0: none)
    long long cap = 0;         // list entries per lane and part
    long long list_floats = 0; // heavy_list elements
    long long cnt_ints = 0;    // heavy_cnt elements
};
// The dearest `heavy_split` patches of a launch of `tiles` patches (at most a quarter of them) are cut in `parts`; a
// part's list holds as many entries as it has candidates at most (orders 0..2 over Nc allowed walls), and the lists of
// all parts together must stay below 4 GiB (fewer patches are cut to fit; none if one does not fit).
inline HeavyPlan heavy_plan(long long tiles, long long Nc, long long heavy_split, long long parts) {
    HeavyPlan hp;
    if (tiles <= 0 || Nc < 2 || heavy_split <= 0 || parts <= 0) return hp;
    long long H = heavy_split < tiles / 4 ? heavy_split : tiles / 4;
    if (H <= 0) return hp;
    if (Nc > (1ll << 30)) return hp;
    // what one part can push: its range of first walls (enumerating build), or -- region lists, parts by rank, part 0 a
    // smaller share because it also sweeps orders 0 and 1 -- up to 1 / (parts - 1) of all order-2 candidates
    const long long by_walls = ((Nc + parts - 1) / parts + 2) * Nc + Nc + 2;
    const long long by_rank = (Nc * (Nc - 1) + (parts > 1 ? parts - 2 : 0)) / (parts > 1 ? parts - 1 : 1) + Nc + 2;
    const long long cap = by_walls > by_rank ? by_walls : by_rank;
    // H * parts * cap * 64 * 4 bytes <= 4 GiB, evaluated without overflow
    const long long limit = (4ll << 30) / (64 * (long long)sizeof(float));
    if (cap <= 0 || cap > limit / parts) return hp;
    if (H > limit / (parts * cap)) H = limit / (parts * cap);  // as many as fit
    if (H <= 0) return hp;
    hp.H = H;
    hp.cap = cap;
    hp.list_floats = H * parts * cap * 64;
    hp.cnt_ints = H * parts * 64 + H * parts;
    return hp;
}

// ---- bins of the per-cell power-delay profile (d2d_power_profile_launch, d2d::BinSink) ------------------------------
// nbins half-open bins of equal width over [r_min, r_max): a path of length r falls into bin floorf((r - r_min) * inv) with
//     inv = (float)nbins / (r_max - r_min)      fp32: one subtraction, one division
// -- the one place the range is checked and inv is formed (tests/native/power_profile_host.cpp holds it to NumPy's fp32).
// D2D_ERR_INVALID: nbins < 1, a bound that is not finite, r_max <= r_min.
struct ProfileBins {
    float r_min = 0.0f, inv = 0.0f;
    int32_t nbins = 0;
};
inline int profile_bins(float r_min, float r_max, int32_t nbins, ProfileBins& b, std::string& err) {
    if (nbins < 1) return err = "the power profile needs nbins >= 1, got " + std::to_string(nbins), D2D_ERR_INVALID;
    if (!std::isfinite(r_min) || !std::isfinite(r_max)) return err = "the power profile's length range must be finite", D2D_ERR_INVALID;
    if (!(r_max > r_min))
        return err = "the power profile's length range needs r_max > r_min, got [" + std::to_string(r_min) + ", " + std::to_string(r_max) + ")", D2D_ERR_INVALID;
    const volatile float width = r_max - r_min;  // (volatile: rounded to fp32 here, whatever the host compiler's excess precision)
    const volatile float inv = (float)nbins / width;
    b.r_min = r_min;
    b.inv = inv;
    b.nbins = nbins;
    return D2D_OK;
}

// ---- what the products of the sink kernel share on the host -------------------------------------------------------------
// The memory check: a launch is refused when its outputs, bytes_per_cell for each of the grid's cells (a product's
// *_bytes_per_cell below; 0 stands for counts out of range and refuses), exceed half of the device memory that is free, counting
// what the product's buffers hold already as free.  No sum or product is formed that could wrap: cells is held against a quotient.
inline bool outputs_fit(size_t cells, size_t bytes_per_cell, size_t mem_free, size_t held_bytes) {
    if (bytes_per_cell == 0) return false;
    return cells <= (mem_free / 2 + held_bytes / 2) / bytes_per_cell;
}
// D2D_ERR_INVALID: an inverse wavelength that is negative, NaN or infinite (0 is allowed: every phase is 0), an amplitude mode that
// is neither D2D_FIELD_AMP_SQRT nor D2D_FIELD_AMP_LINEAR.  `noun` is the product in the message ("the coherent field").
inline bool inv_wavelength_ok(float v) { return std::isfinite(v) && v >= 0.0f; }
inline int check_inv_wavelength(const char* noun, float v, std::string& err) {
    if (inv_wavelength_ok(v)) return D2D_OK;
    return err = std::string(noun) + " needs a finite inv_wavelength >= 0, got " + std::to_string(v), D2D_ERR_INVALID;
}
inline int check_amplitude(const char* noun, int32_t amplitude, std::string& err) {
    if (amplitude == D2D_FIELD_AMP_SQRT || amplitude == D2D_FIELD_AMP_LINEAR) return D2D_OK;
    return err = std::string(noun) + "'s amplitude must be D2D_FIELD_AMP_SQRT (0) or D2D_FIELD_AMP_LINEAR (1), got " + std::to_string(amplitude),
           D2D_ERR_INVALID;
}
// The launches of a product that takes its wavelengths `chunk` at a time: chunks(nf, chunk) passes of the sink kernel over the same
// prepared sweep.  Pass i takes the entries first .. first + count - 1 of the list, writes their planes from plane (block) `first`
// on, and the first pass alone stores total.
struct Chunk {
    int32_t first = 0, count = 0;
    bool with_total = false;
};
inline int32_t chunks(int32_t nf, int32_t chunk) { return (nf + chunk - 1) / chunk; }
inline Chunk chunk_plan(int32_t nf, int32_t i, int32_t chunk) {
    Chunk ch;
    ch.first = i * chunk;
    ch.count = std::min<int32_t>(chunk, nf - ch.first);
    ch.with_total = i == 0;
    return ch;
}

// ---- outputs of the per-cell strongest paths (d2d_strongest_paths_launch, d2d::TopSink) ------------------------------
// Per cell: k slots of power, length, order (4 bytes each) and D2D_MAX_ORDER wall indices, then total and count.  The launch is
// refused when the outputs exceed half of the device memory that is free, counting what the buffers hold already as free
// (tests/native/strongest_paths_host.cpp: a grid large enough to be refused does not fit a quick test).
inline size_t top_bytes_per_cell(int32_t k) { return (size_t)k * (3 + D2D_MAX_ORDER) * 4 + 8; }

// ---- parameters and outputs of the coherent field (d2d_coherent_field_launch, d2d::FieldSink) -----------------------
// D2D_ERR_INVALID: the inverse wavelength, then the amplitude mode (check_inv_wavelength, check_amplitude).
inline int field_params(float inv_wavelength, int32_t amplitude, std::string& err) {
    if (int rc = check_inv_wavelength("the coherent field", inv_wavelength, err)) return rc;
    return check_amplitude("the coherent field", amplitude, err);
}
// Per cell: re, im and total, 4 bytes each (outputs_fit; tests/native/coherent_field_host.cpp).
constexpr size_t FIELD_BYTES_PER_CELL = 12;

// ---- parameters, outputs and launch plan of the frequency response (d2d_frequency_response_launch, d2d::FreqSink) ---
// D2D_ERR_INVALID: nf outside 1 .. D2D_FREQ_MAX, an entry that is negative, NaN or infinite (the message names its index; 0 is
// allowed), an amplitude mode that is neither D2D_FIELD_AMP_SQRT nor D2D_FIELD_AMP_LINEAR.  The list is not read unless nf is in range.
inline int freq_params(const float* inv_wavelength, int32_t nf, int32_t amplitude, std::string& err) {
    if (nf < 1 || nf > D2D_FREQ_MAX)
        return err = "the frequency response needs nf in 1 .. " + std::to_string(D2D_FREQ_MAX) + ", got " + std::to_string(nf), D2D_ERR_INVALID;
    for (int32_t j = 0; j < nf; ++j)
        if (!inv_wavelength_ok(inv_wavelength[j]))
            return err = "the frequency response needs every inv_wavelength finite and >= 0, got " + std::to_string(inv_wavelength[j]) +
                         " at index " + std::to_string(j),
                   D2D_ERR_INVALID;
    return check_amplitude("the frequency response", amplitude, err);
}
// Per cell: nf planes of re and im and one total, 4 bytes each (outputs_fit; tests/native/frequency_response_host.cpp).
inline size_t freq_bytes_per_cell(int32_t nf) { return 8 * (size_t)nf + 4; }
// One pass of the sink kernel per FREQ_CHUNK wavelengths (chunk_plan).
using d2d::FREQ_CHUNK;

// ---- parameters, outputs and launch plan of the material response (d2d_material_response_launch, d2d::MaterialSink) ---
// D2D_ERR_INVALID, in this order: what freq_params refuses (through it); a polarization that is neither D2D_POL_TE nor D2D_POL_TM; an
// n_objects that is not the scene's; an eps component that is NaN, infinite or above 2^50 in magnitude, or an imaginary part > 0
// (the library's time convention makes a lossy medium eps' - j eps''): the message ends with the wavelength index and the wall index.
// The table is fp32 [nf][n_objects][2] and is not read unless the counts are in range.
constexpr float MAT_EPS_MAX = 1125899906842624.0f;  // 2^50: d2d_fresnel.hpp's squares stay finite
inline int material_params(const float* inv_wavelength, int32_t nf, int32_t amplitude, int32_t polarization, const float* eps, int32_t n_objects,
                           int32_t scene_objects, std::string& err) {
    if (int rc = freq_params(inv_wavelength, nf, amplitude, err)) return rc;
    if (polarization != D2D_POL_TE && polarization != D2D_POL_TM)
        return err = "the material response's polarization must be D2D_POL_TE (0) or D2D_POL_TM (1), got " + std::to_string(polarization), D2D_ERR_INVALID;
    if (n_objects != scene_objects)
        return err = "the material response needs one permittivity per object of the resident scene (" + std::to_string(scene_objects) + "), got n_objects = " +
                     std::to_string(n_objects),
               D2D_ERR_INVALID;
    for (int32_t f = 0; f < nf; ++f)
        for (int32_t w = 0; w < n_objects; ++w) {
            const float er = eps[2 * ((size_t)f * n_objects + w)], ei = eps[2 * ((size_t)f * n_objects + w) + 1];
            const char* what = nullptr;
            if (!std::isfinite(er) || !std::isfinite(ei)) what = "finite";
            else if (std::fabs(er) > MAT_EPS_MAX || std::fabs(ei) > MAT_EPS_MAX) what = "at most 2^50 in magnitude";
            if (what)
                return err = std::string("the material response needs every permittivity component ") + what + ", got (" + std::to_string(er) + ", " +
                             std::to_string(ei) + ") at wavelength index " + std::to_string(f) + ", wall index " + std::to_string(w),
                       D2D_ERR_INVALID;
            if (ei > 0.0f)
                return err = "the material response needs Im eps <= 0 (a lossy medium is eps' - j eps'' under e^(-j 2 pi r / lambda)), got " +
                             std::to_string(ei) + " at wavelength index " + std::to_string(f) + ", wall index " + std::to_string(w),
                       D2D_ERR_INVALID;
        }
    return D2D_OK;
}
// Every row of the table equals row 0 in bits (one permittivity per wall for the whole band): the kernel then forms the product of
// coefficients once per contribution.  Bits, not values: -0 and +0 differ (they choose different signs of zero downstream).
inline bool material_constant_band(const float* eps, int32_t nf, int32_t n_objects) {
    const size_t row = 2 * (size_t)n_objects * sizeof(float);
    for (int32_t f = 1; f < nf; ++f)
        if (row && std::memcmp(eps, reinterpret_cast<const char*>(eps) + (size_t)f * row, row) != 0) return false;
    return true;
}
// Per cell: nf planes of re and im and one total, 4 bytes each; beside them the table, 8 nf bytes per object.  Refused above half
// of the device memory that is free, counting what the buffers hold already as free; no product is formed that could wrap.
inline bool material_fits(size_t cells, int32_t nf, size_t n_objects, size_t mem_free, size_t held_bytes) {
    if (nf < 1) return false;
    const size_t budget = mem_free / 2 + held_bytes / 2;
    const size_t per_object = 8 * (size_t)nf;
    if (n_objects > budget / per_object) return false;
    return cells <= (budget - n_objects * per_object) / freq_bytes_per_cell(nf);
}
// One pass of the sink kernel per MAT_CHUNK wavelengths (chunk_plan).
using d2d::MAT_CHUNK;

// ---- memory of the frequency response's coefficient adjoint (d2d_field_coefs_vjp_launch, d2d::CoefGradSink) -----------
// The cotangent planes take 8 nf bytes per cell and the partial rows 4 bytes per patch and object.  Refused like the frequency
// response: above half of the device memory that is free, counting what the buffers hold already as free.  No product is formed
// that could wrap: each share is held against a quotient of what the budget has left.
inline bool coef_vjp_fits(size_t cells, int32_t nf, size_t patches, size_t n_objects, size_t mem_free, size_t held_bytes) {
    size_t budget = mem_free / 2 + held_bytes / 2;
    const size_t per_cell = 8 * (size_t)nf;
    if (cells > budget / per_cell) return false;
    budget -= cells * per_cell;
    if (patches == 0 || n_objects == 0) return true;
    if (patches > budget / sizeof(float)) return false;
    return n_objects <= budget / sizeof(float) / patches;
}

// ---- parameters and memory of the frequency response's position adjoint (d2d_field_position_vjp_launch, d2d::PosGradSink) ----
// D2D_ERR_INVALID, as the frequency response: nf outside 1 .. D2D_FREQ_MAX, an entry that is negative, NaN or infinite (the message
// names its index; 0 is allowed), an amplitude mode that is neither D2D_FIELD_AMP_SQRT nor D2D_FIELD_AMP_LINEAR.  The list is not
// read unless nf is in range.
inline int posgrad_params(const float* inv_wavelength, int32_t nf, int32_t amplitude, std::string& err) {
    const char* noun = "the position adjoint";
    if (nf < 1 || nf > D2D_FREQ_MAX)
        return err = std::string(noun) + " needs nf in 1 .. " + std::to_string(D2D_FREQ_MAX) + ", got " + std::to_string(nf), D2D_ERR_INVALID;
    for (int32_t j = 0; j < nf; ++j)
        if (int rc = check_inv_wavelength(noun, inv_wavelength[j], err)) return err += " at index " + std::to_string(j), rc;
    return check_amplitude(noun, amplitude, err);
}
// Per cell: nf planes of re_bar and im_bar (8 nf bytes) and the four planes of cell_bar and fixed_terms (16 bytes), 4 bytes each
// (outputs_fit; tests/native/field_position_vjp_host.cpp).  0 for an nf out of range: outputs_fit then refuses.
inline size_t posgrad_bytes_per_cell(int32_t nf) { return nf < 1 || nf > D2D_FREQ_MAX ? 0 : 8 * (size_t)nf + 16; }
// One pass of the sink kernel per POS_CHUNK wavelengths (chunk_plan); the block size is part of the definition (include/d2d.h).
constexpr int32_t POS_CHUNK = D2D_POS_CHUNK;  // = d2d::POS_CHUNK (d2d_posgrad.hpp)

// ---- parameters and memory of the frequency response's wall adjoint (d2d_field_walls_vjp_launch, d2d::WallGradSink) ----
// D2D_ERR_INVALID, as the position adjoint: nf outside 1 .. D2D_FREQ_MAX, an entry that is negative, NaN or infinite (the message
// names its index; 0 is allowed), an amplitude mode that is neither D2D_FIELD_AMP_SQRT nor D2D_FIELD_AMP_LINEAR.  The list is not
// read unless nf is in range.  (The passes are POS_CHUNK's: the block's dL/dr is the position adjoint's.)
inline int wallgrad_params(const float* inv_wavelength, int32_t nf, int32_t amplitude, std::string& err) {
    const char* noun = "the wall adjoint";
    if (nf < 1 || nf > D2D_FREQ_MAX)
        return err = std::string(noun) + " needs nf in 1 .. " + std::to_string(D2D_FREQ_MAX) + ", got " + std::to_string(nf), D2D_ERR_INVALID;
    for (int32_t j = 0; j < nf; ++j)
        if (int rc = check_inv_wavelength(noun, inv_wavelength[j], err)) return err += " at index " + std::to_string(j), rc;
    return check_amplitude(noun, amplitude, err);
}
// The cotangent planes take 8 nf bytes per cell and the partial rows 8 bytes per patch and wall (two floats: the wall's two end
// points).  Refused like the coefficient adjoint: above half of the device memory that is free, counting what the buffers hold
// already as free.  No product is formed that could wrap: each share is held against a quotient of what the budget has left
// (tests/native/field_walls_vjp_host.cpp).  An nf below 1 never fits.
inline bool wall_vjp_fits(size_t cells, int32_t nf, size_t patches, size_t n_objects, size_t mem_free, size_t held_bytes) {
    if (nf < 1) return false;
    size_t budget = mem_free / 2 + held_bytes / 2;
    const size_t per_cell = 8 * (size_t)nf;
    if (cells > budget / per_cell) return false;
    budget -= cells * per_cell;
    if (patches == 0 || n_objects == 0) return true;
    const size_t rows = budget / (2 * sizeof(float));
    if (patches > rows) return false;
    return n_objects <= rows / patches;
}

// ---- memory of the material response's permittivity adjoint (d2d_material_eps_vjp_launch, d2d::EpsGradSink) ------------
// The cotangent planes take 8 nf bytes per cell, the permittivity table 8 nf bytes per object, the partial rows of one chunk
// 4 * MAT_CHUNK * 2 bytes per patch and object and the fp64 result 16 nf bytes per object.  Refused like its siblings: above half of
// the device memory that is free, counting what the buffers hold already as free.  No product is formed that could wrap: each share
// is held against a quotient of what the budget has left.  (The parameters are material_params', the chunks MAT_CHUNK's.)
inline bool eps_vjp_fits(size_t cells, int32_t nf, size_t patches, size_t n_objects, size_t mem_free, size_t held_bytes) {
    if (nf < 1) return false;
    size_t budget = mem_free / 2 + held_bytes / 2;
    const size_t per_cell = 8 * (size_t)nf;
    if (cells > budget / per_cell) return false;
    budget -= cells * per_cell;
    if (n_objects == 0) return true;
    const size_t per_object = 8 * (size_t)nf + 16 * (size_t)nf;  // the table and the result
    if (n_objects > budget / per_object) return false;
    budget -= n_objects * per_object;
    if (patches == 0) return true;
    const size_t per_row = sizeof(float) * (size_t)MAT_CHUNK * 2;  // one patch's partial sums of one object
    if (patches > budget / per_row) return false;
    return n_objects <= budget / per_row / patches;
}

// ---- parameters and outputs of the power-angle profile (d2d_power_angle_launch, d2d::AngleSink) ---------------------
// D2D_ERR_INVALID: an end that is neither D2D_ANGLE_AT_TX nor D2D_ANGLE_AT_RX, an origin that is NaN or outside [0, 1) turns,
// nbins outside 1 .. D2D_ANGLE_BINS_MAX.
inline int angle_params(int32_t end, float origin, int32_t nbins, std::string& err) {
    if (end != D2D_ANGLE_AT_TX && end != D2D_ANGLE_AT_RX)
        return err = "the power-angle profile's end must be D2D_ANGLE_AT_TX (0) or D2D_ANGLE_AT_RX (1), got " + std::to_string(end), D2D_ERR_INVALID;
    if (!(origin >= 0.0f && origin < 1.0f))
        return err = "the power-angle profile needs an origin in [0, 1) turns, got " + std::to_string(origin), D2D_ERR_INVALID;
    if (nbins < 1 || nbins > D2D_ANGLE_BINS_MAX)
        return err = "the power-angle profile needs nbins in 1 .. " + std::to_string(D2D_ANGLE_BINS_MAX) + ", got " + std::to_string(nbins), D2D_ERR_INVALID;
    return D2D_OK;
}
// Per cell: nbins planes and one total, 4 bytes each (outputs_fit; tests/native/power_angle_host.cpp).
inline size_t angle_bytes_per_cell(int32_t nbins) { return 4 * (size_t)nbins + 4; }

// ---- parameters and outputs of the array response (d2d_array_response_launch, d2d::ArraySink) ------------------------
// D2D_ERR_INVALID, in this order: nt, then nr outside 1 .. D2D_ARRAY_MAX; a transmit, then a receive element component that is NaN
// or infinite (the message ends in the element's index); an inverse wavelength that is negative, NaN or infinite; an amplitude mode
// that is neither D2D_FIELD_AMP_SQRT nor D2D_FIELD_AMP_LINEAR.  No list is read unless BOTH counts are in range.
inline int array_params(int32_t nt, const float* tx_elems, int32_t nr, const float* rx_elems, float inv_wavelength, int32_t amplitude, std::string& err) {
    if (nt < 1 || nt > D2D_ARRAY_MAX)
        return err = "the array response needs nt in 1 .. " + std::to_string(D2D_ARRAY_MAX) + ", got " + std::to_string(nt), D2D_ERR_INVALID;
    if (nr < 1 || nr > D2D_ARRAY_MAX)
        return err = "the array response needs nr in 1 .. " + std::to_string(D2D_ARRAY_MAX) + ", got " + std::to_string(nr), D2D_ERR_INVALID;
    for (int side = 0; side < 2; ++side) {
        const float* e = side == 0 ? tx_elems : rx_elems;
        const int32_t n = side == 0 ? nt : nr;
        for (int32_t j = 0; j < n; ++j)
            for (int k = 0; k < 2; ++k)
                if (!std::isfinite(e[2 * j + k]))
                    return err = std::string("the array response needs every element offset finite, got ") + std::to_string(e[2 * j + k]) + " as the " +
                                 (k == 0 ? "x" : "y") + " of " + (side == 0 ? "tx_elems" : "rx_elems") + " at index " + std::to_string(j),
                           D2D_ERR_INVALID;
    }
    if (int rc = check_inv_wavelength("the array response", inv_wavelength, err)) return rc;
    return check_amplitude("the array response", amplitude, err);
}
// Per cell: nr * nt planes of re and im and one total, 4 bytes each (at most 516: the counts are in range; outputs_fit;
// tests/native/array_response_host.cpp).
inline size_t array_bytes_per_cell(int32_t nt, int32_t nr) { return 8 * (size_t)nr * (size_t)nt + 4; }

// ---- parameters, outputs and launch plan of the wideband array response (d2d_array_frequency_response_launch, d2d::ArrayFreqSink) ---
// D2D_ERR_INVALID: what freq_params refuses of the list (nf outside 1 .. D2D_FREQ_MAX, an entry that is negative, NaN or infinite: the
// message names its index; an unknown amplitude), then what array_params refuses of the element lists (a count outside
// 1 .. D2D_ARRAY_MAX, a component that is NaN or infinite: the message ends in the element's index).  No list is read unless its
// count is in range.
inline int wide_params(const float* inv_wavelength, int32_t nf, int32_t amplitude, int32_t nt, const float* tx_elems, int32_t nr, const float* rx_elems,
                       std::string& err) {
    if (int rc = freq_params(inv_wavelength, nf, amplitude, err)) return rc;
    return array_params(nt, tx_elems, nr, rx_elems, 0.0f, amplitude, err);
}
// Per cell: nf * nr * nt planes of re and im and one total, 4 bytes each (at most 524 292 with the counts in range; 0 with a count
// that is not: outputs_fit then refuses; tests/native/array_frequency_response_host.cpp).
inline size_t wide_bytes_per_cell(int32_t nf, int32_t nt, int32_t nr) {
    if (nf < 1 || nf > D2D_FREQ_MAX || nt < 1 || nt > D2D_ARRAY_MAX || nr < 1 || nr > D2D_ARRAY_MAX) return 0;
    return 8 * (size_t)nf * (size_t)nr * (size_t)nt + 4;
}
// One pass of the sink kernel per WIDE_CHUNK wavelengths (chunk_plan), each adding into the plane blocks of its chunk.
using d2d::WIDE_CHUNK;

// ---- parameters, outputs and launch plan of the beam-space response (d2d_beam_response_launch, d2d::BeamSink) ---------
// D2D_ERR_INVALID: what wide_params refuses, in its order (the list, the amplitude, the element counts and lists), then nbt, then nbr
// outside 1 .. D2D_BEAM_MAX, then a transmit, then a receive weight component that is NaN or infinite (the message names the beam and
// ends in the element's index).  The weight tables are fp32 [nbt][nt][2] and [nbr][nr][2]; neither is read unless every count is in
// range.
inline int beam_params(const float* inv_wavelength, int32_t nf, int32_t amplitude, int32_t nt, const float* tx_elems, int32_t nr, const float* rx_elems,
                       int32_t nbt, const float* tx_weights, int32_t nbr, const float* rx_weights, std::string& err) {
    if (int rc = wide_params(inv_wavelength, nf, amplitude, nt, tx_elems, nr, rx_elems, err)) return rc;
    if (nbt < 1 || nbt > D2D_BEAM_MAX)
        return err = "the beam response needs nbt in 1 .. " + std::to_string(D2D_BEAM_MAX) + ", got " + std::to_string(nbt), D2D_ERR_INVALID;
    if (nbr < 1 || nbr > D2D_BEAM_MAX)
        return err = "the beam response needs nbr in 1 .. " + std::to_string(D2D_BEAM_MAX) + ", got " + std::to_string(nbr), D2D_ERR_INVALID;
    for (int side = 0; side < 2; ++side) {
        const float* w = side == 0 ? tx_weights : rx_weights;
        const int32_t nb = side == 0 ? nbt : nbr, n = side == 0 ? nt : nr;
        for (int32_t b = 0; b < nb; ++b)
            for (int32_t j = 0; j < n; ++j)
                for (int k = 0; k < 2; ++k) {
                    const float v = w[2 * (b * n + j) + k];
                    if (!std::isfinite(v))
                        return err = std::string("the beam response needs every weight finite, got ") + std::to_string(v) + " as the " +
                                     (k == 0 ? "re" : "im") + " of " + (side == 0 ? "tx_weights" : "rx_weights") + " of beam " + std::to_string(b) +
                                     " at index " + std::to_string(j),
                               D2D_ERR_INVALID;
                }
    }
    return D2D_OK;
}
// Per cell: nf * nbr * nbt planes of re and im and one total, 4 bytes each (at most 524 292 with the counts in range; 0 with a count
// that is not: outputs_fit then refuses; tests/native/beam_response_host.cpp).
inline size_t beam_bytes_per_cell(int32_t nf, int32_t nbt, int32_t nbr) {
    if (nf < 1 || nf > D2D_FREQ_MAX || nbt < 1 || nbt > D2D_BEAM_MAX || nbr < 1 || nbr > D2D_BEAM_MAX) return 0;
    return 8 * (size_t)nf * (size_t)nbr * (size_t)nbt + 4;
}
// One pass of the sink kernel per BEAM_CHUNK wavelengths (chunk_plan), each adding into the plane blocks of its chunk.
using d2d::BEAM_CHUNK;

// ---- scalar thresholds of a sweep launch (d2d::SweepArgs) -----------------------------------------------------------
enum SweepMode { SWEEP_HARD = 0, SWEEP_HSIG = 1, SWEEP_SIG = 2 };  // = d2d::Mode (d2d_kernels.hpp)
struct SweepThresholds {
    int mode = SWEEP_HARD;
    double widen = 0.0, widen_in = 0.0, widen_flt = 0.0;
    float flt_lo = 0.0f, flt_hi = 0.0f, on_lo = 0.0f, on_hi = 0.0f;
    float loss_skip = -1.0f;
    float fnum[D2D_MAX_ORDER + 1] = {};
    float h2 = 0.0f;
    float sig_l2f = 1e30f;
    int sig_mono = 1;
    bool degenerate_invalid = false;
};
// The thresholds of the culling tests and shortcuts of an ImagePath sweep with parameters p (checked by check_params).
// grad: a value+grad sweep.  coef / allowed / n_objects: the reflection coefficients of D2D_FUN_RECEIVED_POWER_PER_OBJECT and the
// candidate mask (null: all objects) -- without coefficients that function gets no bound (correct, and nothing is skipped).
inline SweepThresholds sweep_thresholds(const d2d_params& p, bool grad, const float* coef = nullptr, const uint8_t* allowed = nullptr,
                                        int n_objects = 0) {
    SweepThresholds t;
    // Filter thresholds: the soft window is where some activation of t is not exactly saturated
    // to "outside": hard -> [-tol, 1+tol]; hard_sigmoid -> widened by 3/alpha; sigmoid -> by 89/alpha
    // (exp(89) overflows fp32, 1/(1+inf) == 0).  1e-5 relative slack covers every rounding in the
    // filter's own arithmetic (a few ulp).
    if (p.approx) {
        t.mode = (p.act == D2D_ACT_HARD_SIGMOID) ? SWEEP_HSIG : SWEEP_SIG;
        t.widen = ((t.mode == SWEEP_HSIG) ? 3.0 : 89.0) / (double)p.alpha;
    }
    t.widen_in = !p.approx ? 0.0 : ((t.mode == SWEEP_HSIG) ? 3.0 : 17.5) / (double)p.alpha * (1.0 + 1e-5);
    // (sigmoid, forward sweeps: an occlusion test only enters the map through 1 - max_j sigmoid(z_j), and sigmoid(z) < 2^-25
    // -- z < -17.33 -- leaves 1 - hit at exactly 1.0f, as no test at all would: the divide-free filter may drop what is
    // certainly below -17.5 instead of what is certainly below -89.  The value+grad build keeps the wide window: it records
    // which test carries the max.)
    t.widen_flt = (t.mode == SWEEP_SIG && !grad) ? 17.5 / (double)p.alpha : t.widen;
    const double lo = -((double)p.seg_tol + t.widen_flt);
    const double hi = 1.0 + (double)p.seg_tol + t.widen_flt;
    t.flt_lo = (float)(lo * (1.0 + 1e-5) - 1e-30);
    t.flt_hi = (float)(hi * (1.0 + 1e-5) + 1e-30);
    // on_objects is exactly 0 / False once s < -widen or s > 1 + widen (same saturation argument)
    t.on_lo = (float)(-t.widen * (1.0 + 1e-5) - 1e-30);
    t.on_hi = (float)((1.0 + t.widen) * (1.0 + 1e-5) + 1e-30);
    // loss certificate threshold (d2d_kernels.hpp): hard -> loss < tol decides; approx -> tol - loss must round to tol
    if (p.tol > 1e-30f && std::isfinite(p.tol)) {
        if (!p.approx) t.loss_skip = p.tol * 0.999f;
        else t.loss_skip = 0.49f * (p.tol - std::nextafterf(p.tol, 0.0f));
    }
    for (int k = 0; k <= D2D_MAX_ORDER; ++k) t.fnum[k] = integer_pow(p.r_coef, k);
    t.h2 = p.height * p.height;
    // sigmoid validity: an upper bound of |fun| lets the kernels skip contributions that cannot change the running sum
    for (int k = p.min_order; k <= p.max_order; ++k) t.sig_mono = t.sig_mono && (t.fnum[k] >= 0.0f || p.fun_id != D2D_FUN_RECEIVED_POWER);
    if (p.fun_id == D2D_FUN_ONE) {
        t.sig_l2f = 0.0f;
    } else if (p.fun_id == D2D_FUN_RECEIVED_POWER && t.h2 > 0.0f && std::isfinite(t.h2)) {
        float fm = 0.0f;  // received_power = r_coef^k / (h^2 + r^2) <= |r_coef|^k / h^2
        bool ok = true;
        for (int k = p.min_order; k <= p.max_order; ++k) {
            const float f = std::fabs(t.fnum[k]) / t.h2;
            ok = ok && std::isfinite(f);
            fm = std::fmax(fm, f);
        }
        if (ok && fm > 0.0f) t.sig_l2f = std::log2(fm) + 1e-3f;
        else if (ok) t.sig_l2f = -1e30f;  // fun == 0 throughout
    }
    if (p.fun_id == D2D_FUN_CUSTOM) t.sig_mono = 0;  // (values of any sign)
    if (p.fun_id == D2D_FUN_RECEIVED_POWER_PER_OBJECT) {
        // |fun| = prod_i |coef[cand_i]| / (h^2 + r^2) <= cmax^k / h^2 with cmax over the objects a candidate may hold; fun >= 0
        // throughout only when none of those coefficients is negative
        t.sig_mono = 0;
        if (coef) {
            float cmax = 0.0f;
            bool nonneg = true;
            for (int j = 0; j < n_objects; ++j) {
                if (allowed && !allowed[j]) continue;
                cmax = std::fmax(cmax, std::fabs(coef[j]));
                nonneg = nonneg && coef[j] >= 0.0f;
            }
            t.sig_mono = (nonneg || p.max_order < 1) ? 1 : 0;
            if (t.h2 > 0.0f && std::isfinite(t.h2)) {
                double fm = 0.0;
                for (int k = p.min_order; k <= p.max_order; ++k) fm = std::fmax(fm, std::pow((double)cmax, k) / (double)t.h2);
                // (1e-3 in log2 units is 7e-4 relative: far above the k roundings of the kernels' fp32 fold)
                if (std::isfinite(fm) && fm > 0.0) t.sig_l2f = (float)std::log2(fm) + 1e-3f;
                else if (std::isfinite(fm)) t.sig_l2f = -1e30f;  // fun == 0 throughout
            }
        }
    }
    // A step of the backward scan with un == 0 (the line to the image parallel to the wall, geometry.py:1105) leaves a
    // zero-length segment, loss >= 1 (0.999 with roundings): is such a path exactly invalid under this tol / activation?
    const double x_deg = (double)p.tol - 0.999;  // tol - loss at best
    t.degenerate_invalid = !p.approx ? (p.tol <= 0.5f)
                                     : (t.mode == SWEEP_HSIG ? ((double)p.alpha * x_deg + 3.0 <= -1e-3) : ((double)p.alpha * x_deg <= -89.5));
    return t;
}

// ---- trajectory store of the reverse-mode MinPath / FermatPath sweep (d2d.hip: opt_traj_store) ----------------------
// Cells per chunk of the grid's `cells` for a store of floats_per_cell floats per cell (all candidates; taken as at least 1):
// the budget is traj_mb MiB ("opt_traj_mb", at least 1), but never more than half of what the device has free (free_bytes,
// plus resident_bytes: the store that is resident already counts as free) -- nor less than 64 MiB by that rule -- when
// mem_known (hipMemGetInfo answered).  Whole waves of 64 cells, at least one, at most the grid rounded up to whole waves.
inline long long opt_chunk_cells(long long cells, long long floats_per_cell, long long traj_mb, bool mem_known, long long free_bytes,
                                 long long resident_bytes) {
    const long long per_cell = std::max<long long>(1, floats_per_cell);
    const long long cells_pad = (cells + 63) / 64 * 64;
    long long budget = std::max<long long>(traj_mb, 1) << 20;
    if (mem_known) budget = std::min<long long>(budget, std::max<long long>((free_bytes + resident_bytes) / 2, 64ll << 20));
    return std::min<long long>(cells_pad, std::max<long long>(64, budget / (4 * per_cell) / 64 * 64));
}

// ---- region candidate lists (region_list_kernel / region_refine_kernel) ----------------------------------------------
struct RegionLevelPlan {
    int R = 0, S = 0;  // region = R x R patches; S lists (slices of first walls) per region
    int regions_x = 0, regions_y = 0;
    long long regions = 0, slots = 0;  // slots = regions * S = lists per order
};
struct RegionPlan {
    bool on = false;
    RegionLevelPlan top, leaf;  // top: listed by enumeration, S slices; leaf: one list per region, refined from top
    long long n_static = 0;     // chunks that are some list's first chunk
    long long max_chunks = 0;   // pool chunks of `chunk` entries
    int k_lo = 2;               // lists exist for the orders [k_lo, max_order]
};
// Lists exist for the orders k in [max(2, min_order), max_order].  R_top is rounded down to a multiple of R_leaf (at
// least R_leaf).  The pool holds budget_bytes worth of 8-byte entries in chunks of `chunk`; every list owns one chunk.
inline RegionPlan region_plan(int tiles_x, int tiles_y, long long Nc, int min_order, int max_order, int R_leaf, int R_top, int S_req,
                              long long budget_bytes, int chunk) {
    RegionPlan rp;
    if (tiles_x <= 0 || tiles_y <= 0 || Nc < 2 || max_order < 2 || R_leaf <= 0 || chunk <= 0 || budget_bytes <= 0) return rp;
    int S = S_req > 0 ? S_req : (int)((Nc + 3) / 4);
    if (S > 1024) S = 1024;
    if (S <= 0) return rp;
    if (R_top < R_leaf) R_top = R_leaf;
    R_top = (R_top / R_leaf) * R_leaf;
    auto level = [&](int R, int Sl) {
        RegionLevelPlan l;
        l.R = R;
        l.S = Sl;
        l.regions_x = (int)(((long long)tiles_x + R - 1) / R);
        l.regions_y = (int)(((long long)tiles_y + R - 1) / R);
        l.regions = (long long)l.regions_x * l.regions_y;  // < 2^62
        l.slots = l.regions > 0x3fffffffLL ? -1 : l.regions * Sl;  // (refused below; S <= 1024: no overflow)
        return l;
    };
    rp.leaf = level(R_leaf, 1);
    rp.top = level(R_top, S);
    if (rp.leaf.slots <= 0 || rp.leaf.slots > 0x3fffffffLL || rp.top.slots <= 0 || rp.top.slots > 0x3fffffffLL) return rp;
    rp.k_lo = min_order > 2 ? min_order : 2;
    if (rp.k_lo > max_order) return rp;
    rp.n_static = (rp.leaf.slots + rp.top.slots) * (max_order - rp.k_lo + 1);
    rp.max_chunks = budget_bytes / ((long long)sizeof(unsigned long long) * chunk);
    if (rp.max_chunks > 0x7fffffffLL) rp.max_chunks = 0x7fffffffLL;
    if (rp.n_static > 0x7fffffffLL || rp.max_chunks < 2 * rp.n_static) return rp;  // not worth having
    rp.on = true;
    return rp;
}

}  // namespace d2d_host
