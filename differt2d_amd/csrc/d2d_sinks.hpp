// The sinks of the culled forward sweep: power_sink_kernel<MODE, MAXK, TXG, Sink>, the contract a Sink keeps, every sink of
// D2D_SINKS (the list at the end of this file) and the launchers' declarations.  Included by d2d.hip and by the sink objects only
// (d2d_sweep_tu.hip with -DD2D_TU_FAMILY=11 -DD2D_TU_SINK=<Sink>: one object per sink and mode); the forward-sweep objects do not
// see it -- sweep_order_culled / sweep_order_culled_txg (d2d_kernels.hpp) reach a sink through their RS parameter alone.
#pragma once

#include "d2d_kernels.hpp"
#include "d2d_chunks.hpp"
#include "d2d_top.hpp"
#include "d2d_phasor.hpp"
#include "d2d_angle.hpp"
#include "d2d_steer.hpp"
#include "d2d_beam.hpp"
#include "d2d_fresnel.hpp"
#include "d2d_fresnel_grad.hpp"
#include "d2d_posgrad.hpp"
#include "d2d_wallgrad.hpp"

namespace d2d {

// A sink of power_sink_kernel: what takes the contributions of the culled forward sweep in acc's place.  The contract:
//     Args                   the sink's kernel argument (by value, behind SweepArgs)
//     begin(args, tile, cell)  fills the lane's sink for patch `tile`; cell = the lane's row-major cell, < 0 for a clamped
//                              duplicate of a lane outside the grid, which never contributes
//     put(t, code, k, r)     one candidate's contribution t (every lane of the wave calls it, zeros included), the candidate's
//                              code (12 bits per wall index, first wall lowest) and order, and -- WANTS_R -- its path length
//     end(args, tile, lane)  after the last order
//     WANTS_DIR              the sink takes put_dir(t, dir) in put's place (sink_put below): dir[4] is what eval_candidate hands out
//                              where it hands out the length, the path's two end directions {p[1] - p[0], p[K] - p[K+1]}
//                              -- or, with WANTS_R as well, put_rd(t, r, dir): the contribution, the length and the directions
//     WANTS_SEG              the sink takes put_seg(t, code, k, r, seg): seg[] holds the segment that reaches every bounce

// ---- pieces that several sinks share: fp32, one rounding per stated operation, no contraction ----
// (the amplitude a of a contribution and the phase f of its path in turns: field_amp, turn_fraction of d2d_phasor.hpp)

// p: this lane's contribution is non-zero or NaN.  True when no lane of the wave has one (wave-uniform), the common case: the sink
// then has nothing to do for the candidate.
__device__ __forceinline__ bool no_contribution(float t, bool& p) {
    p = !(t == 0.0f);
    return __ballot(p) == 0ull;
}

// begin() of an adjoint: the lane's cotangents re_bar[j][cell], im_bar[j][cell] of the chunk's nf planes into registers; zeros past
// nf and for lanes outside the grid (cell < 0), which evaluate a clamped copy of an edge cell and would count it twice
template <int C>
__device__ __forceinline__ void load_cotangents(const float* re_bar, const float* im_bar, long cells, int nf, int cell, float (&rb)[C], float (&ib)[C]) {
    static_for<0, C>([&](auto JJ) {
        constexpr int J = decltype(JJ)::value;
        rb[J] = ib[J] = 0.0f;
        if (J < nf && cell >= 0) {
            const size_t at = (size_t)J * (size_t)cells + (size_t)cell;
            rb[J] = re_bar[at];
            ib[J] = im_bar[at];
        }
    });
}

// end() of a sink whose running sum of every contribution (the fused map, bit for bit) is all it holds in registers: every lane is
// the only writer of its cell, lanes outside the grid (cell < 0) never write
__device__ __forceinline__ void store_total(float* total_out, int cell, float total) {
    if (cell < 0) return;
    total_out[cell] = total;
}

// end() of a sink that holds the chunk's planes in registers: planes 0 .. nf-1 at re / im + j * cells (the host hands every launch
// the planes of its chunk) and total where its pointer is not null (the first chunk's launch); no atomics, no zeroing pass
template <int C>
__device__ __forceinline__ void store_planes(float* re_out, float* im_out, float* total_out, long cells, int nf, int cell, const float (&re)[C],
                                             const float (&im)[C], float total) {
    if (cell < 0) return;
    if (total_out != nullptr) total_out[cell] = total;
    static_for<0, C>([&](auto JJ) {
        constexpr int J = decltype(JJ)::value;
        if (J < nf) {
            const size_t at = (size_t)J * (size_t)cells + (size_t)cell;
            re_out[at] = re[J];
            im_out[at] = im[J];
        }
    });
}

// RecSink (d2d_valid_paths): every (cell, candidate) whose contribution is not exactly zero is handed out as a record
// instead of being added.  Two passes of the same deterministic sweep: with rec == null the wave only counts (cnt is
// wave-uniform: the popcount of the ballot of pushing lanes) and end() writes the patch's number of records to counts; else
// every pushing lane stores its record at base + count so far + the pushing lanes below it, in offs[patch] .. offs[patch + 1] --
// never at or past `limit`, the next patch's offset: a position outside [base, limit) raises the sticky flag instead.  A
// record: {cell (row-major), code bits 0..31, code bits 32..47 | order << 24, the contribution's bits}.
struct RecArgs {
    int* counts;      // [patches]
    const int* offs;  // [patches + 1] exclusive scan of counts
    int4* rec;        // [offs[patches]] or null
    int* flag;        // != 0 afterwards: pass 2 met a position outside its patch's range (the passes disagree: an internal error)
};
struct RecSink {
    using Args = RecArgs;
    static constexpr bool WANTS_R = false, WANTS_DIR = false, WANTS_SEG = false;
    int4* rec;
    int base, limit;
    int cnt;
    int cell;
    int* flag;
    __device__ __forceinline__ void begin(const RecArgs& r, long tile, int lane_cell) {
        rec = r.rec;
        base = r.rec ? r.offs[tile] : 0;
        limit = r.rec ? r.offs[tile + 1] : 0;
        cnt = 0;
        cell = lane_cell;
        flag = r.flag;
    }
    __device__ __forceinline__ void put(float t, unsigned long long code, int k, float /*r*/ = 0.0f) {
        const bool p = cell >= 0 && !(t == 0.0f);
        const unsigned long long m = __ballot(p);
        if (rec != nullptr && p) {
            const int pos = base + cnt + __builtin_popcountll(m & ((1ull << (threadIdx.x & 63)) - 1ull));
            if (pos >= base && pos < limit) rec[pos] = make_int4(cell, (int)(unsigned)(code & 0xffffffffull), (int)(unsigned)(code >> 32) | (k << 24), __float_as_int(t));
            else *flag = 1;
        }
        cnt += __builtin_popcountll(m);
    }
    __device__ __forceinline__ void end(const RecArgs& r, long tile, int lane) const {
        if (r.rec == nullptr && lane == 0) r.counts[tile] = cnt;
    }
};

// BinSink (d2d_power_profile_launch): every contribution that is not exactly zero is added to the bin of its path length instead
// of to acc -- the power-delay profile out[nbins][cells] (include/d2d.h), zeroed on the stream in front of the launch:
//     u = (r - r_min) * inv ;  b = (int)floorf(u) ;  if (u >= 0 && b < nbins) out[b][cell] = out[b][cell] + t
// in fp32 without contraction, candidates in the sweep's order.  A lane is the only writer of its cell's column and reads back
// what it stored itself: plain loads and stores, the same bits run to run.  A NaN length fails u >= 0 and names no bin; lanes
// outside the grid (cell < 0) never write.  (u < 2^31 in front of the conversion: beyond it the conversion is undefined, and
// the bin is past any nbins anyway.)
struct BinArgs {
    float* out;       // [nbins][cells]
    long cells;       // m * n
    float r_min, inv; // the bins: floorf((r - r_min) * inv), d2d_host::profile_bins
    int nbins;
};
struct BinSink {
    using Args = BinArgs;
    static constexpr bool WANTS_R = true, WANTS_DIR = false, WANTS_SEG = false;
    float* out;  // [nbins][cells]
    long cells;
    int cell;
    float r_min, inv;
    int nbins;
    __device__ __forceinline__ void begin(const BinArgs& b, long /*tile*/, int lane_cell) {
        out = b.out;
        cells = b.cells;
        cell = lane_cell;
        r_min = b.r_min;
        inv = b.inv;
        nbins = b.nbins;
    }
    __device__ __forceinline__ void put(float t, unsigned long long /*code*/, int /*k*/, float r) {
        if (cell < 0 || t == 0.0f) return;
        const float d = r - r_min;
        const float u = d * inv;
        if (u >= 0.0f && u < 2147483648.0f) {
            const int b = (int)floorf(u);
            if (b < nbins) {
                float* p = out + (size_t)b * (size_t)cells + (size_t)cell;
                *p = *p + t;
            }
        }
    }
    __device__ __forceinline__ void end(const BinArgs&, long, int) const {}
};

// TopSink (d2d_strongest_paths_launch): the k strongest contributions of every cell instead of their sum alone (include/d2d.h
// holds the definition).  Per lane, in registers: TOP_SLOTS slots of (t, r, code low, code high | order) kept sorted by
// d2d_top.hpp's top_insert, the running fp32 sum of every contribution (the fused map, bit for bit) and the number of
// contributions that are not exactly zero.  The whole insertion is skipped where no_contribution says so.  end() unpacks the codes and stores slots 0 .. k-1: every lane is the only writer
// of its cell and writes all of it, so there are no atomics and no zeroing pass; lanes outside the grid (cell < 0) never write.
struct TopArgs {
    float* power;   // [k][cells]
    float* length;  // [k][cells]
    int* cand;      // [k][cells][D2D_MAX_ORDER]
    int* order;     // [k][cells]
    float* total;   // [cells]
    int* count;     // [cells]
    long cells;     // m * n
    int k;          // 1 .. TOP_SLOTS
};
struct TopSink {
    using Args = TopArgs;
    static constexpr bool WANTS_R = true, WANTS_DIR = false, WANTS_SEG = false;
    static_assert(D2D_MAX_ORDER == 4, "a slot's wall indices are stored as one int4");
    static_assert(TOP_SLOTS == D2D_TOP_MAX, "d2d_top.hpp and include/d2d.h disagree");
    TopSlots s;
    float total;
    int count;
    int cell;
    __device__ __forceinline__ void begin(const TopArgs&, long /*tile*/, int lane_cell) {
        top_clear(s);
        total = 0.0f;
        count = 0;
        cell = lane_cell;
    }
    __device__ __forceinline__ void put(float t, unsigned long long code, int k, float r) {
        total = total + t;
        bool p;
        if (no_contribution(t, p)) return;
        if (p) {
            ++count;
            top_insert(s, (uint32_t)__float_as_int(t), (uint32_t)__float_as_int(r), (uint32_t)(code & 0xffffffffull), (uint32_t)(code >> 32) | ((uint32_t)k << 24));
        }
    }
    __device__ __forceinline__ void end(const TopArgs& x, long, int) const {
        if (cell < 0) return;
        x.total[cell] = total;
        x.count[cell] = count;
        static_for<0, TOP_SLOTS>([&](auto SS) {
            constexpr int S = decltype(SS)::value;
            if (S < x.k) {
                const size_t at = (size_t)S * (size_t)x.cells + (size_t)cell;
                const bool empty = top_key(s.tb[S]) == 0u;
                const int ord = empty ? -1 : (int)(s.hi[S] >> 24);
                const unsigned long long code = ((unsigned long long)(s.hi[S] & 0xffffu) << 32) | s.lo[S];
                int4 w;
                w.x = ord > 0 ? (int)(code & 0xfffull) : -1;
                w.y = ord > 1 ? (int)((code >> 12) & 0xfffull) : -1;
                w.z = ord > 2 ? (int)((code >> 24) & 0xfffull) : -1;
                w.w = ord > 3 ? (int)((code >> 36) & 0xfffull) : -1;
                x.power[at] = __int_as_float((int)s.tb[S]);
                x.length[at] = empty ? __builtin_nanf("") : __int_as_float((int)s.rb[S]);
                x.order[at] = ord;
                reinterpret_cast<int4*>(x.cand)[at] = w;
            }
        });
    }
};

// FieldSink (d2d_coherent_field_launch): the coherent sum of every cell -- each contribution as a complex amplitude with the phase
// of its path length -- beside the incoherent one (include/d2d.h holds the definition).  Per lane, in registers: re, im and the
// running fp32 sum of every contribution (the fused map, bit for bit).  Per contribution that is not exactly zero:
//     a = sqrt mode ? copysignf(sqrtf(fabsf(t)), t) : t ;  u = r * inv_wavelength ;  f = u - floorf(u)
//     (c, s) = phasor(f) ;  re = re + a * c ;  im = im - a * s
// in fp32 without contraction, candidates in the sweep's order; f is exact and in [0, 1) for every finite u >= 0, NaN otherwise.
// phasor (d2d_phasor.hpp, with field_amp and turn_fraction, which form a and f) is plain arithmetic: no sine or cosine of the device
// library or the hardware is involved.  The phasor is skipped where no_contribution says so.  end() stores the
// three values: every lane is the only writer of its cell and writes all of it, so there are no atomics and no zeroing pass; lanes
// outside the grid (cell < 0) never write.
struct FieldArgs {
    float* re;             // [cells]
    float* im;             // [cells]
    float* total;          // [cells]
    long cells;            // m * n
    float inv_wavelength;  // turns per unit length, finite and >= 0
    int amplitude;         // D2D_FIELD_AMP_SQRT / D2D_FIELD_AMP_LINEAR
};
struct FieldSink {
    using Args = FieldArgs;
    static constexpr bool WANTS_R = true, WANTS_DIR = false, WANTS_SEG = false;
    float re, im, total;
    float inv;
    bool root;
    int cell;
    __device__ __forceinline__ void begin(const FieldArgs& x, long /*tile*/, int lane_cell) {
        re = im = total = 0.0f;
        inv = x.inv_wavelength;
        root = x.amplitude == D2D_FIELD_AMP_SQRT;
        cell = lane_cell;
    }
    __device__ __forceinline__ void put(float t, unsigned long long /*code*/, int /*k*/, float r) {
        total = total + t;
        bool p;
        if (no_contribution(t, p)) return;
        if (p) {
            const float a = field_amp(root, t);
            const float f = turn_fraction(r, inv);
            float c, s;
            phasor(f, c, s);
            const float ac = a * c, as = a * s;
            re = re + ac;
            im = im - as;
        }
    }
    __device__ __forceinline__ void end(const FieldArgs& x, long, int) const {
        if (cell < 0) return;
        x.re[cell] = re;
        x.im[cell] = im;
        x.total[cell] = total;
    }
};

// FreqSink (d2d_frequency_response_launch): the coherent sum of every cell at up to FREQ_CHUNK wavelengths of one sweep -- plane j
// is, bit for bit, FieldSink's (re, im) at inv[j] (include/d2d.h holds the definition).  Per lane, in registers: re[C], im[C] and the
// running fp32 sum of every contribution.  Per contribution that is not exactly zero, a is formed once and then, for every j < nf,
//     u = r * inv[j] ;  f = u - floorf(u) ;  (c, s) = phasor(f) ;  re[j] = re[j] + a * c ;  im[j] = im[j] - a * s
// in fp32 without contraction.  j is a compile-time index (static_for) behind the wave-uniform guard j < nf: a register array indexed
// at run time goes to scratch.  inv[] and nf come by value in the kernel argument: scalar loads.  All of it is
// skipped where no_contribution says so.  end() is store_planes.
struct FreqArgs {
    float* re;              // [nf][cells]: this chunk's planes
    float* im;              // [nf][cells]
    float* total;           // [cells] or null
    long cells;             // m * n
    float inv[FREQ_CHUNK];  // turns per unit length, finite and >= 0; entries at and past nf are not read
    int nf;                 // 1 .. FREQ_CHUNK
    int amplitude;          // D2D_FIELD_AMP_SQRT / D2D_FIELD_AMP_LINEAR
};
struct FreqSink {
    using Args = FreqArgs;
    static constexpr bool WANTS_R = true, WANTS_DIR = false, WANTS_SEG = false;
    float re[FREQ_CHUNK], im[FREQ_CHUNK], total;
    float inv[FREQ_CHUNK];
    int nf;
    bool root;
    int cell;
    __device__ __forceinline__ void begin(const FreqArgs& x, long /*tile*/, int lane_cell) {
        static_for<0, FREQ_CHUNK>([&](auto JJ) {
            constexpr int J = decltype(JJ)::value;
            re[J] = im[J] = 0.0f;
            inv[J] = x.inv[J];
        });
        total = 0.0f;
        nf = x.nf;
        root = x.amplitude == D2D_FIELD_AMP_SQRT;
        cell = lane_cell;
    }
    __device__ __forceinline__ void put(float t, unsigned long long /*code*/, int /*k*/, float r) {
        total = total + t;
        bool p;
        if (no_contribution(t, p)) return;
        if (p) {
            const float a = field_amp(root, t);
            static_for<0, FREQ_CHUNK>([&](auto JJ) {
                constexpr int J = decltype(JJ)::value;
                if (J < nf) {
                    const float f = turn_fraction(r, inv[J]);
                    float c, s;
                    phasor(f, c, s);
                    const float ac = a * c, as = a * s;
                    re[J] = re[J] + ac;
                    im[J] = im[J] - as;
                }
            });
        }
    }
    __device__ __forceinline__ void end(const FreqArgs& x, long, int) const { store_planes(x.re, x.im, x.total, x.cells, x.nf, cell, re, im, total); }
};

// CoefGradSink (d2d_field_coefs_vjp_launch): the reverse-mode product of the frequency response with respect to the per-object
// reflection coefficients, for up to FREQ_CHUNK wavelengths of one sweep (include/d2d.h holds the definition).  The host runs the
// sweep with D2D_FUN_RECEIVED_POWER and a numerator of 1, so a contribution is s = valid / (h^2 + r^2): what does not depend on the
// coefficients.  begin() is load_cotangents.  Per candidate that some lane of the wave
// has a non-zero s from: the candidate's coefficients, their left fold num and the products P_i of the OTHER coefficients are formed
// on wave-uniform values (the walls come out of the wave-uniform code, the table is read with scalar loads; nothing is divided by a
// coefficient); per lane g = sum_j (re_bar[j] * c_j - im_bar[j] * s_j) with the frequency response's own phasors, and the weight
// W = g * s (SQRT: g * sqrtf(s)), forced to 0.0f in lanes that do not contribute.  wave_sum(W) runs in uniform control flow, and lane 0
// adds S * Q_i to the patch's row partial[patch][cand[i]] for every position i: one writer per row, candidates in order, plain
// load-add-store, no atomics -- the same bits run to run.  The rows are zeroed on the stream in front of the first chunk's launch,
// accumulate over the chunks' launches and are reduced in patch order into fp64 by vjp_reduce_kernel.  j is a compile-time index
// behind the wave-uniform guard j < nf, as in FreqSink.
struct CoefGradArgs {
    const float* re_bar;    // [nf][cells]: this chunk's cotangent planes
    const float* im_bar;    // [nf][cells]
    const float* coef;      // [N] reflection coefficients (wave-uniform index -> scalar loads)
    float* partial;         // [patches][N] per-patch sums, zeroed in front of the first chunk
    long cells;             // m * n
    float inv[FREQ_CHUNK];  // turns per unit length, finite and >= 0; entries at and past nf are not read
    int nf;                 // 1 .. FREQ_CHUNK
    int amplitude;          // D2D_FIELD_AMP_SQRT / D2D_FIELD_AMP_LINEAR
    int N;                  // objects: the length of a row
};
struct CoefGradSink {
    using Args = CoefGradArgs;
    static constexpr bool WANTS_R = true, WANTS_DIR = false, WANTS_SEG = false;
    float rb[FREQ_CHUNK], ib[FREQ_CHUNK];
    float inv[FREQ_CHUNK];
    const float* coef;
    float* row;  // partial[patch]
    int nf;
    bool root;
    bool live;  // cell >= 0
    __device__ __forceinline__ void begin(const CoefGradArgs& x, long tile, int lane_cell) {
        live = lane_cell >= 0;
        load_cotangents(x.re_bar, x.im_bar, x.cells, x.nf, lane_cell, rb, ib);
        static_for<0, FREQ_CHUNK>([&](auto JJ) { inv[decltype(JJ)::value] = x.inv[decltype(JJ)::value]; });
        coef = x.coef;
        row = x.partial + (size_t)tile * (size_t)x.N;
        nf = x.nf;
        root = x.amplitude == D2D_FIELD_AMP_SQRT;
    }
    __device__ __forceinline__ void put(float t, unsigned long long code, int k, float r) {
        bool p;
        if (k == 0 || no_contribution(t, p)) return;  // (the line of sight holds no coefficient)
        // wave-uniform: the candidate's walls and coefficients, their fold and the products of the others
        int w[D2D_MAX_ORDER];
        float cf[D2D_MAX_ORDER], q[D2D_MAX_ORDER];
        float num = 1.0f;
#pragma unroll
        for (int i = 0; i < D2D_MAX_ORDER; ++i) {
            w[i] = __builtin_amdgcn_readfirstlane((int)((code >> (12 * i)) & 0xfffull));
            cf[i] = 1.0f;
            if (i < k) {
                cf[i] = cmem(coef)[w[i]];
                num = num * cf[i];
            }
        }
        if (root && num == 0.0f) return;  // sign(num) sqrt|num| is not differentiable there: no term
        const float half = root ? 2.0f * sqrtf(fabsf(num)) : 1.0f;
#pragma unroll
        for (int i = 0; i < D2D_MAX_ORDER; ++i) {
            float others = 1.0f;
#pragma unroll
            for (int o = 0; o < D2D_MAX_ORDER; ++o)
                if (o != i && o < k) others = others * cf[o];
            q[i] = root ? others / half : others;
        }
        // per lane: the cotangents against this candidate's phasors
        float g = 0.0f;
        if (p) {
            static_for<0, FREQ_CHUNK>([&](auto JJ) {
                constexpr int J = decltype(JJ)::value;
                if (J < nf) {
                    const float f = turn_fraction(r, inv[J]);
                    float c, s;
                    phasor(f, c, s);
                    const float rc = rb[J] * c, is = ib[J] * s;
                    g = g + (rc - is);
                }
            });
        }
        const float sw = root ? sqrtf(t) : t;
        const float W = (p && live) ? g * sw : 0.0f;
        const float S = wave_sum(W);  // every lane of the wave is here: the exits above are wave-uniform
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int i = 0; i < D2D_MAX_ORDER; ++i)
                if (i < k) row[w[i]] = row[w[i]] + S * q[i];
        }
    }
    __device__ __forceinline__ void end(const CoefGradArgs&, long, int) const {}
};

// PosGradSink (d2d_field_position_vjp_launch): the reverse-mode product of the frequency response with respect to the two end points
// of every path, the cell's and the fixed one, for up to POS_CHUNK wavelengths of one sweep (include/d2d.h holds the definition,
// d2d_posgrad.hpp its per-contribution arithmetic).  Hard validity only: a position then enters through the path length alone, and
// d r / d p[0] = -unit(p[1] - p[0]), d r / d p[K+1] = -unit(p[K] - p[K+1]) (the interaction points are stationary).  CoefGradSink's
// front: begin() is load_cotangents.  A per-lane back: four fp32 accumulators, the gradient with respect to the cell's position and the cell's share of the
// gradient with respect to the fixed end point.  Per candidate that some lane of the wave has a non-zero contribution from, every
// such lane forms G = dL/dr of the path for this block (posgrad_amp / _rho / _kr / _fold) and subtracts G times the unit direction
// at either end, where that end has one (unit_dir of d2d_steer.hpp): no wave reduction, no atomics, no LDS.  fun_id, h2, the
// amplitude mode and inv[] come by value in the kernel argument (scalar loads); j is a compile-time index behind the wave-uniform
// guard j < nf, as in FreqSink.  The four planes cell_bar[2][cells], fixed_terms[2][cells] carry the running values from one
// block's pass to the next: begin() starts from +0.0f in the first pass and from the planes afterwards, end() stores; a lane is the
// only writer of its cell, lanes outside the grid never read or write.  cell < cells, so every address is inside the 2 * cells
// floats of a pair of planes.
struct PosGradArgs {
    const float* re_bar;   // [nf][cells]: this block's cotangent planes
    const float* im_bar;   // [nf][cells]
    float* cell_bar;       // [2][cells]
    float* fixed_terms;    // [2][cells]
    long cells;            // m * n
    float inv[POS_CHUNK];  // turns per unit length, finite and >= 0; entries at and past nf are not read
    int nf;                // 1 .. POS_CHUNK
    int amplitude;         // D2D_FIELD_AMP_SQRT / D2D_FIELD_AMP_LINEAR
    int fun_id;            // the caller's fused path function
    float h2;              // height * height, as the sweep has it
    int txg;               // the cell is the transmitter: its direction is dir[0..1], the fixed end's dir[2..3]
    int first;             // the first block's pass: the accumulators start from +0.0f
};
struct PosGradSink {
    using Args = PosGradArgs;
    static constexpr bool WANTS_R = true, WANTS_DIR = true, WANTS_SEG = false;
    float rb[POS_CHUNK], ib[POS_CHUNK];
    float inv[POS_CHUNK];
    float cx, cy, fx, fy;
    float h2;
    int nf, amplitude, fun_id;
    bool txg;
    int cell;
    __device__ __forceinline__ void begin(const PosGradArgs& x, long /*tile*/, int lane_cell) {
        cell = lane_cell;
        const bool live = lane_cell >= 0;
        load_cotangents(x.re_bar, x.im_bar, x.cells, x.nf, lane_cell, rb, ib);
        static_for<0, POS_CHUNK>([&](auto JJ) { inv[decltype(JJ)::value] = x.inv[decltype(JJ)::value]; });
        cx = cy = fx = fy = 0.0f;
        if (!x.first && live) {
            cx = x.cell_bar[lane_cell];
            cy = x.cell_bar[(size_t)x.cells + (size_t)lane_cell];
            fx = x.fixed_terms[lane_cell];
            fy = x.fixed_terms[(size_t)x.cells + (size_t)lane_cell];
        }
        h2 = x.h2;
        nf = x.nf;
        amplitude = x.amplitude;
        fun_id = x.fun_id;
        txg = x.txg != 0;
    }
    // dir: {p[1] - p[0], p[K] - p[K+1]} of the candidate (stale or zero where its contribution is zero)
    __device__ __forceinline__ void put_rd(float t, float r, const float (&dir)[4]) {
        bool p;
        if (no_contribution(t, p)) return;
        if (!(p && cell >= 0)) return;  // (per lane: nothing below crosses lanes)
        const float a = posgrad_amp(amplitude, t);
        const float kr = posgrad_kr(amplitude, posgrad_rho(fun_id, h2, r));
        float g = 0.0f;
        static_for<0, POS_CHUNK>([&](auto JJ) {
            constexpr int J = decltype(JJ)::value;
            if (J < nf) g = posgrad_fold(g, kr, r, inv[J], rb[J], ib[J]);
        });
        const float G = a * g;
        float ucx, ucy, ufx, ufy;
        const bool okc = unit_dir(txg ? dir[0] : dir[2], txg ? dir[1] : dir[3], ucx, ucy);
        const bool okf = unit_dir(txg ? dir[2] : dir[0], txg ? dir[3] : dir[1], ufx, ufy);
        if (okc) {
            const float gx = G * ucx, gy = G * ucy;
            cx = cx - gx;
            cy = cy - gy;
        }
        if (okf) {
            const float gx = G * ufx, gy = G * ufy;
            fx = fx - gx;
            fy = fy - gy;
        }
    }
    __device__ __forceinline__ void end(const PosGradArgs& x, long, int) const {
        if (cell < 0) return;
        x.cell_bar[cell] = cx;
        x.cell_bar[(size_t)x.cells + (size_t)cell] = cy;
        x.fixed_terms[cell] = fx;
        x.fixed_terms[(size_t)x.cells + (size_t)cell] = fy;
    }
};

// AngleSink (d2d_power_angle_launch): every contribution that is not exactly zero is added to the bin of the direction in which its
// path leaves the transmitter or reaches the receiver -- the power-angle profile out[nbins][cells] (include/d2d.h holds the
// definition), zeroed on the stream in front of the launch -- beside the running fp32 sum of every contribution (the fused map, bit
// for bit), which stays in a register until end():
//     (dx, dy) = end == AT_TX ? dir[0..1] : dir[2..3] ;  f = turns(dx, dy) ;  g = f - origin ;  if (g < 0) g = g + 1
//     u = g * (float)nbins ;  b = (int)floorf(u) ;  if (b >= nbins) b = nbins - 1 ;  if (f == f) out[b][cell] = out[b][cell] + t
// in fp32 without contraction, candidates in the sweep's order.  turns (d2d_angle.hpp) is plain arithmetic with one IEEE division:
// no atan2f of the device library is involved.  All of it is skipped where no_contribution says so.  A lane is the only writer of
// its cell's column and reads back what it stored itself: plain loads and stores, the same bits run to run.  f is in [0, 1) or
// NaN and origin in [0, 1), so 0 <= u <= nbins: the conversion is defined and 0 <= b < nbins after the clamp.  Lanes outside the
// grid (cell < 0) never write.  end, origin and nbins come by value in the kernel argument: scalar loads.
struct AngleArgs {
    float* out;    // [nbins][cells]
    float* total;  // [cells]
    long cells;    // m * n
    float origin;  // turns, in [0, 1)
    int nbins;     // 1 .. D2D_ANGLE_BINS_MAX
    int end;       // D2D_ANGLE_AT_TX / D2D_ANGLE_AT_RX
};
struct AngleSink {
    using Args = AngleArgs;
    static constexpr bool WANTS_R = false, WANTS_DIR = true, WANTS_SEG = false;
    float total;
    float* out;
    long cells;
    float origin, fbins;
    int nbins;
    bool at_rx;
    int cell;
    __device__ __forceinline__ void begin(const AngleArgs& x, long /*tile*/, int lane_cell) {
        total = 0.0f;
        out = x.out;
        cells = x.cells;
        origin = x.origin;
        nbins = x.nbins;
        fbins = (float)x.nbins;
        at_rx = x.end == D2D_ANGLE_AT_RX;
        cell = lane_cell;
    }
    // dir: {p[1] - p[0], p[K] - p[K+1]} of the candidate (stale or zero where its contribution is zero)
    __device__ __forceinline__ void put_dir(float t, const float (&dir)[4]) {
        total = total + t;
        bool p;
        if (no_contribution(t, p)) return;
        if (p && cell >= 0) {
            const float f = turns(at_rx ? dir[2] : dir[0], at_rx ? dir[3] : dir[1]);
            if (f == f) {
                float g = f - origin;
                if (g < 0.0f) g = g + 1.0f;
                const float u = g * fbins;
                int b = (int)floorf(u);
                if (b >= nbins) b = nbins - 1;
                if (b >= 0) {  // (always: see above)
                    float* q = out + (size_t)b * (size_t)cells + (size_t)cell;
                    *q = *q + t;
                }
            }
        }
    }
    __device__ __forceinline__ void end(const AngleArgs& x, long, int) const { store_total(x.total, cell, total); }
};

// ArraySink (d2d_array_response_launch): the coherent sum of every cell for every pair of a transmit element j < nt and a receive
// element i < nr -- the channel matrix re / im [nr][nt][cells] under the plane-wave model (d2d_steer.hpp holds the definition),
// zeroed on the stream in front of the launch -- beside the running fp32 sum of every contribution (the fused map, bit for bit),
// which stays in a register until end().  Per contribution that is not exactly zero, a and f0 are formed once as FieldSink forms
// them, the two unit directions once (dir[] is what eval_candidate hands out through dir_out), and then
//     for j < nt: qt = steer_dot(etx[j], utx, uty)
//       for i < nr: qr = steer_dot(erx[i], urx, ury) ;  f = steer_phase(f0, qt, qr, inv) ;  (c, s) = phasor(f)
//                   re[i][j][cell] = re[i][j][cell] + a * c ;  im[i][j][cell] = im[i][j][cell] - a * s
// in fp32 without contraction, candidates in the sweep's order.  The two loops are wave-uniform run-time loops: no per-element
// register array exists (one indexed at run time goes to scratch); qt is recomputed per j and qr per (i, j) from
// the element offsets, which come by value in the kernel argument with nt and nr and are read by scalar loads.  All of it is skipped
// where no_contribution says so.  A lane is the only writer of its
// cell's column and reads back what it stored itself: plain loads and stores, no atomics, the same bits run to run.  Lanes outside
// the grid (cell < 0) never write.  i * nt + j < 64 and cell < cells, so every address is inside the 2 * nr * nt * cells planes.
struct ArrayArgs {
    float* re;                // [nr][nt][cells]
    float* im;                // [nr][nt][cells]
    float* total;             // [cells]
    long cells;               // m * n
    float inv_wavelength;     // turns per unit length, finite and >= 0
    int amplitude;            // D2D_FIELD_AMP_SQRT / D2D_FIELD_AMP_LINEAR
    int nt, nr;               // 1 .. ARRAY_MAX each
    float etx[ARRAY_MAX][2];  // (ex, ey) of the transmit elements; entries at and past nt are not read
    float erx[ARRAY_MAX][2];  // (ex, ey) of the receive elements; entries at and past nr are not read
};
struct ArraySink {
    using Args = ArrayArgs;
    static constexpr bool WANTS_R = true, WANTS_DIR = true, WANTS_SEG = false;
    float total;
    const ArrayArgs* x;  // the kernel argument: wave-uniform, read where it is used
    int cell;
    __device__ __forceinline__ void begin(const ArrayArgs& xa, long /*tile*/, int lane_cell) {
        total = 0.0f;
        x = &xa;
        cell = lane_cell;
    }
    // dir: {p[1] - p[0], p[K] - p[K+1]} of the candidate (stale or zero where its contribution is zero)
    __device__ __forceinline__ void put_rd(float t, float r, const float (&dir)[4]) {
        total = total + t;
        bool p;
        if (no_contribution(t, p)) return;
        const float inv = x->inv_wavelength;
        const float a = field_amp(x->amplitude == D2D_FIELD_AMP_SQRT, t);
        const float f0 = turn_fraction(r, inv);
        float utx, uty, urx, ury;  // (these five lines stand alike in ArrayFreqSink and BeamSink: as one shared function they compiled to other code)
        const bool okt = unit_dir(dir[0], dir[1], utx, uty);
        const bool okr = unit_dir(dir[2], dir[3], urx, ury);
        const bool go = p && okt && okr && cell >= 0;
        if (!go) return;  // (per lane: the loops below are uniform for the lanes that stay)
        const int nt = x->nt, nr = x->nr;
        const size_t cells = (size_t)x->cells;
        for (int j = 0; j < nt; ++j) {
            const float qt = steer_dot(x->etx[j][0], x->etx[j][1], utx, uty);
            for (int i = 0; i < nr; ++i) {
                const float qr = steer_dot(x->erx[i][0], x->erx[i][1], urx, ury);
                const float f = steer_phase(f0, qt, qr, inv);
                float c, s;
                phasor(f, c, s);
                const float ac = a * c, as = a * s;
                const size_t at = (size_t)(i * nt + j) * cells + (size_t)cell;
                x->re[at] = x->re[at] + ac;
                x->im[at] = x->im[at] - as;
            }
        }
    }
    __device__ __forceinline__ void end(const ArrayArgs& xa, long, int) const { store_total(xa.total, cell, total); }
};

// ArrayFreqSink (d2d_array_frequency_response_launch): ArraySink's channel matrix at up to WIDE_CHUNK wavelengths of one sweep --
// plane block f is, bit for bit, ArraySink's re / im [nr][nt][cells] at inv[f] (include/d2d.h holds the definition).  The planes
// re / im [nf][nr][nt][cells] of the chunk live in memory, zeroed on the stream in front of the passes; the running fp32 sum of
// every contribution stays in a register until end(), which stores it where `total` is not null (the first chunk's pass).  Per
// contribution that is not exactly zero, a and the two unit directions are formed once, and then
//     for f < nf: u = r * inv[f] ;  f0 = u - floorf(u)
//       for j < nt: qt = steer_dot(etx[j], utx, uty)
//         for i < nr: qr = steer_dot(erx[i], urx, ury) ;  ph = steer_phase(f0, qt, qr, inv[f]) ;  (c, s) = phasor(ph)
//                     re[f][i][j][cell] = re[f][i][j][cell] + a * c ;  im[f][i][j][cell] = im[f][i][j][cell] - a * s
// in fp32 without contraction, candidates in the sweep's order.  The three loops are wave-uniform run-time loops over lists that
// come by value in the kernel argument and are read by scalar loads: no per-lane array exists (one indexed at run time goes to
// scratch), so registers do not bound the chunk.  Every plane is its own accumulator: the nesting does not reach
// the result.  All of it is skipped where no_contribution says so.  A lane is the only
// writer of its cell's column and reads back what it stored itself: plain loads and stores, no atomics, the same bits run to run.
// Lanes outside the grid (cell < 0) never write.  (f * nr + i) * nt + j < nf * nr * nt and cell < cells, so every address is
// inside the chunk's 2 * nf * nr * nt * cells planes.
struct ArrayFreqArgs {
    float* re;                // [nf][nr][nt][cells]: this chunk's planes
    float* im;                // [nf][nr][nt][cells]
    float* total;             // [cells] or null
    long cells;               // m * n
    int amplitude;            // D2D_FIELD_AMP_SQRT / D2D_FIELD_AMP_LINEAR
    int nf;                   // 1 .. WIDE_CHUNK
    int nt, nr;               // 1 .. ARRAY_MAX each
    float inv[WIDE_CHUNK];    // turns per unit length, finite and >= 0; entries at and past nf are not read
    float etx[ARRAY_MAX][2];  // (ex, ey) of the transmit elements; entries at and past nt are not read
    float erx[ARRAY_MAX][2];  // (ex, ey) of the receive elements; entries at and past nr are not read
};
static_assert(WIDE_CHUNK >= 8 && WIDE_CHUNK <= 64 && (WIDE_CHUNK & (WIDE_CHUNK - 1)) == 0, "WIDE_CHUNK is a power of two in 8 .. 64");
static_assert(sizeof(SweepArgs) + sizeof(ArrayFreqArgs) <= 4096, "power_sink_kernel's arguments must fit the 4 KiB kernel-argument segment");
struct ArrayFreqSink {
    using Args = ArrayFreqArgs;
    static constexpr bool WANTS_R = true, WANTS_DIR = true, WANTS_SEG = false;
    float total;
    const ArrayFreqArgs* x;  // the kernel argument: wave-uniform, read where it is used
    int cell;
    __device__ __forceinline__ void begin(const ArrayFreqArgs& xa, long /*tile*/, int lane_cell) {
        total = 0.0f;
        x = &xa;
        cell = lane_cell;
    }
    // dir: {p[1] - p[0], p[K] - p[K+1]} of the candidate (stale or zero where its contribution is zero)
    __device__ __forceinline__ void put_rd(float t, float r, const float (&dir)[4]) {
        total = total + t;
        bool p;
        if (no_contribution(t, p)) return;
        const float a = field_amp(x->amplitude == D2D_FIELD_AMP_SQRT, t);
        float utx, uty, urx, ury;
        const bool okt = unit_dir(dir[0], dir[1], utx, uty);
        const bool okr = unit_dir(dir[2], dir[3], urx, ury);
        const bool go = p && okt && okr && cell >= 0;
        if (!go) return;  // (per lane: the loops below are uniform for the lanes that stay)
        const int nf = x->nf, nt = x->nt, nr = x->nr;
        const size_t cells = (size_t)x->cells;
        for (int f = 0; f < nf; ++f) {
            const float inv = x->inv[f];
            const float f0 = turn_fraction(r, inv);
            for (int j = 0; j < nt; ++j) {
                const float qt = steer_dot(x->etx[j][0], x->etx[j][1], utx, uty);
                for (int i = 0; i < nr; ++i) {
                    const float qr = steer_dot(x->erx[i][0], x->erx[i][1], urx, ury);
                    const float ph = steer_phase(f0, qt, qr, inv);
                    float c, s;
                    phasor(ph, c, s);
                    const float ac = a * c, as = a * s;
                    const size_t at = (size_t)((f * nr + i) * nt + j) * cells + (size_t)cell;
                    x->re[at] = x->re[at] + ac;
                    x->im[at] = x->im[at] - as;
                }
            }
        }
    }
    __device__ __forceinline__ void end(const ArrayFreqArgs& xa, long, int) const {
        if (cell < 0 || xa.total == nullptr) return;  // (store_total behind a null test compiled to other code)
        xa.total[cell] = total;
    }
};

// BeamSink (d2d_beam_response_launch): what comes out behind a codebook of nbt transmit beams and one of nbr receive beams,
// y = w_rx^H H w_tx, at up to BEAM_CHUNK wavelengths of one sweep, without the channel matrix H: every contribution to H has rank one
// under the plane-wave model, so its share of y is a e^(-j 2 pi f0) times the two array factors (d2d_beam.hpp holds the definition).
// The planes re / im [nf][nbr][nbt][cells] of the chunk live in memory, zeroed on the stream in front of the passes; the running fp32
// sum of every contribution stays in a register until end(), which stores it where `total` is not null (the first chunk's pass).  Per
// contribution that is not exactly zero, a and the two unit directions are formed once, and then, per wavelength f < nf:
//     (c0, s0) = phasor(f0)
//     for i < nr:   (c, s) = beam_steer(steer_dot(erx[i], urx, ury), inv[f]) ;  for br < nbr: beam_fold_rx(Ar[br], rx_weights[br][i], c, s)
//     for j < nt:   (ct[j], st[j]) = beam_steer(steer_dot(etx[j], utx, uty), inv[f])
//     for bt < nbt: At = fold of beam_fold_tx over j ;  load the nbr planes of this bt ;  for br < nbr: beam_pair, add, store
// -- 1 + nr + nt phasors per wavelength, whatever the codebooks hold; the receive steering is folded into Ar[] and dropped, the
// transmit steering is kept, so that no phasor is formed twice.  The per-lane arrays Ar[BEAM_MAX], (ct, st)[ARRAY_MAX] and the loaded
// planes are indexed at compile time only (a per-lane array indexed at run time goes to scratch): the loops over i, j
// (forming the steering) and bt are wave-uniform run-time loops, the loops that touch an array are unrolled over BEAM_MAX / ARRAY_MAX
// with wave-uniform guards, and the run-time j writes (ct, st)[j] through a chain of selects.  The order of the two folds is the
// definition's (i and j ascending); every other nesting cannot reach the bits, each plane being its own accumulator.  The loads of
// one bt's nbr planes are issued BEAM_LOADS at a time, ahead of their adds.  The lists and the counts come by value in the kernel
// argument and are read by scalar loads; the two weight tables (1 KiB at the limits) live in a device buffer of the result, uploaded
// on the stream in front of the passes, and are read at wave-uniform addresses -- by value they made the compiler copy the whole
// argument to the stack in three of the twelve instances.  All of it is skipped where no_contribution says so.  A lane is the only writer of its cell's column and reads back what it stored itself: plain loads and stores,
// no atomics, the same bits run to run.  Lanes outside the grid (cell < 0) never write.  (f * nbr + br) * nbt + bt < nf * nbr * nbt
// and cell < cells, so every address is inside the chunk's 2 * nf * nbr * nbt * cells planes.
constexpr int BEAM_LOADS = 4;   // planes of one transmit beam whose loads are issued together, ahead of their adds (2 registers each)
struct BeamArgs {
    float* re;                          // [nf][nbr][nbt][cells]: this chunk's planes
    float* im;                          // [nf][nbr][nbt][cells]
    float* total;                       // [cells] or null
    long cells;                         // m * n
    int amplitude;                      // D2D_FIELD_AMP_SQRT / D2D_FIELD_AMP_LINEAR
    int nf;                             // 1 .. BEAM_CHUNK
    int nt, nr;                         // 1 .. ARRAY_MAX each
    int nbt, nbr;                       // 1 .. BEAM_MAX each
    float inv[BEAM_CHUNK];              // turns per unit length, finite and >= 0; entries at and past nf are not read
    float etx[ARRAY_MAX][2];            // (ex, ey) of the transmit elements; entries at and past nt are not read
    float erx[ARRAY_MAX][2];            // (ex, ey) of the receive elements; entries at and past nr are not read
    const float* w;                     // device memory, [2][BEAM_MAX][ARRAY_MAX][2]: (re, im) of transmit beam bt at element j, then of
                                        // receive beam br at element i; rows at and past nbt / nbr, entries at and past nt / nr are not read
};
constexpr int BEAM_TABLE = BEAM_MAX * ARRAY_MAX * 2;  // floats of one weight table
static_assert(BEAM_CHUNK >= 8 && BEAM_CHUNK <= 64 && (BEAM_CHUNK & (BEAM_CHUNK - 1)) == 0, "BEAM_CHUNK is a power of two in 8 .. 64");
static_assert(sizeof(SweepArgs) + sizeof(BeamArgs) <= 4096, "power_sink_kernel's arguments must fit the 4 KiB kernel-argument segment");
struct BeamSink {
    using Args = BeamArgs;
    static constexpr bool WANTS_R = true, WANTS_DIR = true, WANTS_SEG = false;
    float total;
    const BeamArgs* x;  // the kernel argument: wave-uniform, read where it is used
    int cell;
    __device__ __forceinline__ void begin(const BeamArgs& xa, long /*tile*/, int lane_cell) {
        total = 0.0f;
        x = &xa;
        cell = lane_cell;
    }
    // dir: {p[1] - p[0], p[K] - p[K+1]} of the candidate (stale or zero where its contribution is zero)
    __device__ __forceinline__ void put_rd(float t, float r, const float (&dir)[4]) {
        total = total + t;
        bool p;
        if (no_contribution(t, p)) return;
        const float a = field_amp(x->amplitude == D2D_FIELD_AMP_SQRT, t);
        float utx, uty, urx, ury;
        const bool okt = unit_dir(dir[0], dir[1], utx, uty);
        const bool okr = unit_dir(dir[2], dir[3], urx, ury);
        const bool go = p && okt && okr && cell >= 0;
        if (!go) return;  // (per lane: the loops below are uniform for the lanes that stay)
        const int nf = x->nf, nt = x->nt, nr = x->nr, nbt = x->nbt, nbr = x->nbr;
        const size_t cells = (size_t)x->cells;
        const float* const wtx = x->w;
        const float* const wrx = x->w + BEAM_TABLE;
        for (int f = 0; f < nf; ++f) {
            const float inv = x->inv[f];
            const float f0 = turn_fraction(r, inv);
            float c0, s0;
            phasor(f0, c0, s0);
            // the receive array factors of every beam: the steering of element i is folded into them and dropped
            float arr[BEAM_MAX], ari[BEAM_MAX];
#pragma unroll
            for (int b = 0; b < BEAM_MAX; ++b) arr[b] = ari[b] = 0.0f;
            for (int i = 0; i < nr; ++i) {
                float c, s;
                beam_steer(steer_dot(x->erx[i][0], x->erx[i][1], urx, ury), inv, c, s);
#pragma unroll
                for (int b = 0; b < BEAM_MAX; ++b)
                    if (b < nbr) beam_fold_rx(arr[b], ari[b], wrx[(b * ARRAY_MAX + i) * 2], wrx[(b * ARRAY_MAX + i) * 2 + 1], c, s);
            }
            // the transmit steering, kept: (ct, st)[j] through a chain of selects, so that j stays a run-time loop
            float ct[ARRAY_MAX], st[ARRAY_MAX];
#pragma unroll
            for (int k = 0; k < ARRAY_MAX; ++k) ct[k] = st[k] = 0.0f;
            for (int j = 0; j < nt; ++j) {
                float c, s;
                beam_steer(steer_dot(x->etx[j][0], x->etx[j][1], utx, uty), inv, c, s);
#pragma unroll
                for (int k = 0; k < ARRAY_MAX; ++k)
                    if (k == j) ct[k] = c, st[k] = s;
            }
            for (int bt = 0; bt < nbt; ++bt) {
                float atr = 0.0f, ati = 0.0f;
#pragma unroll
                for (int j = 0; j < ARRAY_MAX; ++j)
                    if (j < nt) beam_fold_tx(atr, ati, wtx[(bt * ARRAY_MAX + j) * 2], wtx[(bt * ARRAY_MAX + j) * 2 + 1], ct[j], st[j]);
                // plane (f, br, bt): this bt's nbr planes are loaded together, ahead of the adds
                const size_t first = (size_t)(f * nbr * nbt + bt) * cells + (size_t)cell, step = (size_t)nbt * cells;
#pragma unroll
                for (int g = 0; g < BEAM_MAX; g += BEAM_LOADS) {
                    if (g >= nbr) break;
                    float lre[BEAM_LOADS], lim[BEAM_LOADS];
#pragma unroll
                    for (int k = 0; k < BEAM_LOADS; ++k)
                        if (g + k < nbr) lre[k] = x->re[first + (size_t)(g + k) * step], lim[k] = x->im[first + (size_t)(g + k) * step];
#pragma unroll
                    for (int k = 0; k < BEAM_LOADS; ++k)
                        if (g + k < nbr) {
                            float zr, zs;
                            beam_pair(arr[g + k], ari[g + k], atr, ati, c0, s0, zr, zs);
                            const float azr = a * zr, azs = a * zs;
                            x->re[first + (size_t)(g + k) * step] = lre[k] + azr;
                            x->im[first + (size_t)(g + k) * step] = lim[k] - azs;
                        }
                }
            }
        }
    }
    __device__ __forceinline__ void end(const BeamArgs& xa, long, int) const {
        if (cell < 0 || xa.total == nullptr) return;  // (store_total behind a null test compiled to other code)
        xa.total[cell] = total;
    }
};

// MaterialSink (d2d_material_response_launch): FreqSink's coherent sum with every contribution multiplied by the product of the
// Fresnel reflection coefficients of the walls it bounces off, for up to MAT_CHUNK wavelengths of one sweep (include/d2d.h holds
// the definition, d2d_fresnel.hpp the coefficient).  Per lane, in registers: re[C], im[C] and the running fp32 sum of every
// contribution (the fused map, bit for bit).  Per candidate that some lane has a non-zero contribution from: the walls come out of the
// wave-uniform code (readfirstlane), their unit normals refl[2 w].zw and their permittivities eps[j][w] are read at wave-uniform
// addresses (scalar loads); per lane the cosines c_i = |unit_dir(seg_i) . n_i| of the K angles of incidence, formed once from what
// eval_candidate hands out through seg_out (WANTS_SEG, sink_put), and then for every j < nf
//     G = (1, +0) ; for i < K: G = G * fresnel(eps[j][w_i], c_i, pol) ; u = r * inv[j] ; f0 = u - floorf(u) ; (c0, s0) = phasor(f0)
//     zr = G.re*c0 + G.im*s0 ; zs = G.re*s0 - G.im*c0 ; re[j] = re[j] + a * zr ; im[j] = im[j] - a * zs
// in fp32 without contraction.  With `constant` set (the host found the rows of eps equal in bits) G is formed once, from row 0,
// in front of the loop over j: the same bits by definition.  i and j are compile-time indices (static_for) behind the wave-uniform
// guards i < k and j < nf: a register array indexed at run time goes to scratch.  A lane whose path has a segment
// without a direction, or a NaN cosine, adds nothing to the planes (total has its contribution).  end() is store_planes.  Wall
// indices come from the sweep's own candidates, 0 <= w < N.
struct MaterialArgs {
    float* re;             // [nf][cells]: this chunk's planes
    float* im;             // [nf][cells]
    float* total;          // [cells] or null
    long cells;            // m * n
    const float4* refl;    // the context's wall table: row 2 w = {ox, oy, nx, ny}
    const float* eps;      // device memory, [nf][N][2]: this chunk's rows of (re, im); row 0 alone is read when `constant`
    float inv[MAT_CHUNK];  // turns per unit length, finite and >= 0; entries at and past nf are not read
    int nf;                // 1 .. MAT_CHUNK
    int N;                 // objects: the length of a row of eps
    int amplitude;         // D2D_FIELD_AMP_SQRT / D2D_FIELD_AMP_LINEAR
    int pol;               // D2D_POL_TE / D2D_POL_TM
    int constant;          // != 0: every row of eps equals row 0 in bits
};
static_assert(sizeof(SweepArgs) + sizeof(MaterialArgs) <= 4096, "power_sink_kernel's arguments must fit the 4 KiB kernel-argument segment");
struct MaterialSink {
    using Args = MaterialArgs;
    static constexpr bool WANTS_R = true, WANTS_DIR = false, WANTS_SEG = true;
    static_assert(POL_TE == D2D_POL_TE && POL_TM == D2D_POL_TM, "d2d_fresnel.hpp and include/d2d.h disagree");
    float re[MAT_CHUNK], im[MAT_CHUNK], total;
    const MaterialArgs* x;  // the kernel argument: wave-uniform, read where it is used
    int cell;
    __device__ __forceinline__ void begin(const MaterialArgs& xa, long /*tile*/, int lane_cell) {
        static_for<0, MAT_CHUNK>([&](auto JJ) {
            constexpr int J = decltype(JJ)::value;
            re[J] = im[J] = 0.0f;
        });
        total = 0.0f;
        x = &xa;
        cell = lane_cell;
    }
    // G = prod_i fresnel(row[w_i], ci_i, pol), folded from the left; row and w are wave-uniform
    __device__ __forceinline__ void fold(const float* row, const int (&w)[D2D_MAX_ORDER], const float (&ci)[D2D_MAX_ORDER], int k, int pol, float& Gr,
                                         float& Gi) const {
        Gr = 1.0f;
        Gi = 0.0f;
        static_for<0, D2D_MAX_ORDER>([&](auto II) {
            constexpr int I = decltype(II)::value;
            if (I < k) {
                const float er = cmem(row)[2 * w[I]], ei = cmem(row)[2 * w[I] + 1];
                float gr, gi;
                fresnel(er, ei, ci[I], pol, gr, gi);
                fresnel_fold(Gr, Gi, gr, gi);
            }
        });
    }
    // seg: (p[i+1] - p[i]) for i < k of the candidate (stale or zero where its contribution is zero)
    __device__ __forceinline__ void put_seg(float t, unsigned long long code, int k, float r, const float (&seg)[2 * D2D_MAX_ORDER]) {
        total = total + t;
        bool p;
        if (no_contribution(t, p)) return;
        int w[D2D_MAX_ORDER];
        float ci[D2D_MAX_ORDER];
        bool ok = true;  // (the walls and cosines stand alike in EpsGradSink: as one shared function they compiled to other code in both)
        static_for<0, D2D_MAX_ORDER>([&](auto II) {
            constexpr int I = decltype(II)::value;
            w[I] = 0;
            ci[I] = 0.0f;
            if (I < k) {
                w[I] = __builtin_amdgcn_readfirstlane((int)((code >> (12 * I)) & 0xfffull));
                const float4 n = ldc4(x->refl, 2 * w[I]);
                float ux, uy;
                const bool oki = unit_dir(seg[2 * I], seg[2 * I + 1], ux, uy);
                const float c = fabsf(steer_dot(ux, uy, n.z, n.w));
                ci[I] = c;
                ok = ok && oki && c == c;
            }
        });
        if (!(p && ok)) return;  // (per lane: what follows is uniform for the lanes that stay)
        const float a = field_amp(x->amplitude == D2D_FIELD_AMP_SQRT, t);
        const int nf = x->nf, pol = x->pol;
        const bool constant = x->constant != 0;
        const size_t stride = 2 * (size_t)x->N;
        float G0r = 1.0f, G0i = 0.0f;
        if (constant) fold(x->eps, w, ci, k, pol, G0r, G0i);
        static_for<0, MAT_CHUNK>([&](auto JJ) {
            constexpr int J = decltype(JJ)::value;
            if (J < nf) {
                float Gr = G0r, Gi = G0i;
                if (!constant) fold(x->eps + (size_t)J * stride, w, ci, k, pol, Gr, Gi);
                const float f0 = turn_fraction(r, x->inv[J]);
                float c0, s0, zr, zs;
                phasor(f0, c0, s0);
                fresnel_turn(Gr, Gi, c0, s0, zr, zs);
                const float azr = a * zr, azs = a * zs;
                re[J] = re[J] + azr;
                im[J] = im[J] - azs;
            }
        });
    }
    __device__ __forceinline__ void end(const MaterialArgs& xa, long, int) const { store_planes(xa.re, xa.im, xa.total, xa.cells, xa.nf, cell, re, im, total); }
};

// EpsGradSink (d2d_material_eps_vjp_launch): the reverse-mode product of the material response with respect to the walls'
// permittivities, for up to MAT_CHUNK wavelengths of one sweep (include/d2d.h holds the definition, d2d_fresnel_grad.hpp the
// coefficient's derivative).  It is MaterialSink's front (the walls out of the wave-uniform code, normals and permittivities read
// at wave-uniform addresses, the cosines per lane from seg_out) joined to CoefGradSink's back (load_cotangents; weights forced to 0.0f in lanes that do not contribute; wave_sum in wave-uniform control flow; lane 0 adds
// to the patch's rows with a plain load-add-store: one writer per row, candidates in order, no atomics).  Per lane and j < nf, for
// every position i < k:
//     (g_i, d_i, ok_i) = fresnel_grad(eps[j][w_i], c_i, pol) ;  P_i = (1, +0) folded with g_o for o != i in position order
//     Pd_i = P_i * d_i ;  E = (a*c0, -(a*s0)) ;  D = E * Pd_i ;  Wr = B.re*D.re + B.im*D.im ;  Wi = B.im*D.re - B.re*D.im
// in fp32 without contraction (complex products as fresnel_fold forms them), and partial[tile][j][w_i][0..1] += wave_sum(Wr), wave_sum(Wi).
// With `constant` set g_i, d_i and Pd_i are formed once per contribution from row 0, in front of the loop over j: the same values, so
// the rows are bit-identical to the per-row route.  i and j are compile-time indices behind the wave-uniform guards i < k and j < nf.
// The host zeroes the rows in front of every chunk's pass and reduces them in patch order into fp64 (vjp_reduce_kernel).
struct EpsGradArgs {
    const float* re_bar;   // [nf][cells]: this chunk's cotangent planes
    const float* im_bar;   // [nf][cells]
    const float* eps;      // device memory, [nf][N][2]: this chunk's rows of (re, im); row 0 alone is read when `constant`
    const float4* refl;    // the context's wall table: row 2 w = {ox, oy, nx, ny}
    float* partial;        // [tiles][MAT_CHUNK][N][2] per-patch sums, zeroed in front of the pass
    long cells;            // m * n
    float inv[MAT_CHUNK];  // turns per unit length, finite and >= 0; entries at and past nf are not read
    int nf;                // 1 .. MAT_CHUNK
    int N;                 // objects: the length of a row of eps
    int amplitude;         // D2D_FIELD_AMP_SQRT / D2D_FIELD_AMP_LINEAR
    int pol;               // D2D_POL_TE / D2D_POL_TM
    int constant;          // != 0: every row of eps equals row 0 in bits
};
static_assert(sizeof(SweepArgs) + sizeof(EpsGradArgs) <= 4096, "power_sink_kernel's arguments must fit the 4 KiB kernel-argument segment");
struct EpsGradSink {
    using Args = EpsGradArgs;
    static constexpr bool WANTS_R = true, WANTS_DIR = false, WANTS_SEG = true;
    float rb[MAT_CHUNK], ib[MAT_CHUNK];
    const EpsGradArgs* x;  // the kernel argument: wave-uniform, read where it is used
    float* row;            // partial[tile]
    bool live;             // cell >= 0
    __device__ __forceinline__ void begin(const EpsGradArgs& xa, long tile, int lane_cell) {
        live = lane_cell >= 0;
        load_cotangents(xa.re_bar, xa.im_bar, xa.cells, xa.nf, lane_cell, rb, ib);
        x = &xa;
        row = xa.partial + (size_t)tile * (size_t)MAT_CHUNK * 2 * (size_t)xa.N;
    }
    // Pd_i = (product of the OTHER positions' coefficients) * d_i and ok_i for every position of the candidate, from one row of eps
    __device__ __forceinline__ void factors(const float* erow, const int (&w)[D2D_MAX_ORDER], const float (&ci)[D2D_MAX_ORDER], int k, int pol,
                                            float (&Pdr)[D2D_MAX_ORDER], float (&Pdi)[D2D_MAX_ORDER], bool (&okd)[D2D_MAX_ORDER]) const {
        float gr[D2D_MAX_ORDER], gi[D2D_MAX_ORDER], dr[D2D_MAX_ORDER], di[D2D_MAX_ORDER];
        static_for<0, D2D_MAX_ORDER>([&](auto II) {
            constexpr int I = decltype(II)::value;
            gr[I] = 1.0f;
            gi[I] = dr[I] = di[I] = 0.0f;
            okd[I] = false;
            if (I < k) {
                const float er = cmem(erow)[2 * w[I]], ei = cmem(erow)[2 * w[I] + 1];
                fresnel_grad(er, ei, ci[I], pol, gr[I], gi[I], dr[I], di[I], okd[I]);
            }
        });
        static_for<0, D2D_MAX_ORDER>([&](auto II) {
            constexpr int I = decltype(II)::value;
            Pdr[I] = Pdi[I] = 0.0f;
            if (I < k) {
                float Pr = 1.0f, Pi = 0.0f;
                static_for<0, D2D_MAX_ORDER>([&](auto OO) {
                    constexpr int O = decltype(OO)::value;
                    if (O != I && O < k) fresnel_fold(Pr, Pi, gr[O], gi[O]);
                });
                fresnel_fold(Pr, Pi, dr[I], di[I]);
                Pdr[I] = Pr;
                Pdi[I] = Pi;
            }
        });
    }
    // seg: (p[i+1] - p[i]) for i < k of the candidate (stale or zero where its contribution is zero)
    __device__ __forceinline__ void put_seg(float t, unsigned long long code, int k, float r, const float (&seg)[2 * D2D_MAX_ORDER]) {
        bool p;
        if (k == 0 || no_contribution(t, p)) return;  // wave-uniform (the line of sight holds no coefficient)
        int w[D2D_MAX_ORDER];
        float ci[D2D_MAX_ORDER];
        bool ok = true;
        static_for<0, D2D_MAX_ORDER>([&](auto II) {
            constexpr int I = decltype(II)::value;
            w[I] = 0;
            ci[I] = 0.0f;
            if (I < k) {
                w[I] = __builtin_amdgcn_readfirstlane((int)((code >> (12 * I)) & 0xfffull));
                const float4 n = ldc4(x->refl, 2 * w[I]);
                float ux, uy;
                const bool oki = unit_dir(seg[2 * I], seg[2 * I + 1], ux, uy);
                const float c = fabsf(steer_dot(ux, uy, n.z, n.w));
                ci[I] = c;
                ok = ok && oki && c == c;
            }
        });
        const bool go = p && ok && live;  // (per lane: it becomes zero weights, never an exit)
        const float a = field_amp(x->amplitude == D2D_FIELD_AMP_SQRT, t);
        const int nf = x->nf, pol = x->pol;
        const bool constant = x->constant != 0;
        const size_t stride = 2 * (size_t)x->N;
        const bool lane0 = (threadIdx.x & 63) == 0;
        float Pdr[D2D_MAX_ORDER], Pdi[D2D_MAX_ORDER];
        bool okd[D2D_MAX_ORDER];
        if (constant) factors(x->eps, w, ci, k, pol, Pdr, Pdi, okd);
        static_for<0, MAT_CHUNK>([&](auto JJ) {
            constexpr int J = decltype(JJ)::value;
            if (J < nf) {
                if (!constant) factors(x->eps + (size_t)J * stride, w, ci, k, pol, Pdr, Pdi, okd);
                const float f0 = turn_fraction(r, x->inv[J]);
                float c0, s0;
                phasor(f0, c0, s0);
                const float Er = a * c0, Ei = -(a * s0);
                float* const out = row + (size_t)J * stride;
                static_for<0, D2D_MAX_ORDER>([&](auto II) {
                    constexpr int I = decltype(II)::value;
                    if (I < k) {
                        float Dr = Er, Di = Ei;
                        fresnel_fold(Dr, Di, Pdr[I], Pdi[I]);
                        const float b0 = rb[J] * Dr, b1 = ib[J] * Di, b2 = ib[J] * Dr, b3 = rb[J] * Di;
                        const bool on = go && okd[I];
                        const float Wr = on ? b0 + b1 : 0.0f;
                        const float Wi = on ? b2 - b3 : 0.0f;
                        const float Sr = wave_sum(Wr), Si = wave_sum(Wi);  // every lane of the wave is here: the exits above are wave-uniform
                        if (lane0) {
                            out[2 * w[I]] = out[2 * w[I]] + Sr;
                            out[2 * w[I] + 1] = out[2 * w[I] + 1] + Si;
                        }
                    }
                });
            }
        });
    }
    __device__ __forceinline__ void end(const EpsGradArgs&, long, int) const {}
};

// WallGradSink (d2d_field_walls_vjp_launch): the reverse-mode product of the frequency response with respect to the two end points
// of every wall, for up to POS_CHUNK wavelengths of one sweep (include/d2d.h holds the definition, d2d_wallgrad.hpp its per-bounce
// arithmetic, d2d_posgrad.hpp dL/dr).  Hard validity only: a wall then enters through the path length alone, and
// d r / d A = gam (1 - s) n, d r / d B = gam s n for every bounce on the wall (the interaction points are stationary).  EpsGradSink's
// front: the walls out of the wave-uniform code (readfirstlane), their two table rows refl[2 w], refl[2 w + 1] read at wave-uniform
// addresses (scalar loads), k == 0 || no_contribution as the wave-uniform exit.  PosGradSink's cotangents: begin() is load_cotangents,
// and every contributing lane forms G = dL/dr of the path for this block (posgrad_amp / _rho / _kr / _fold).  CoefGradSink's back: per
// bounce, the lane's weights (wallgrad_bounce; the bounce point q is rebuilt from p[0] and the segments that seg_out hands out)
// forced to 0.0f in lanes that do not contribute, wave_sum in wave-uniform control flow, and lane 0 adds the two sums to the patch's
// row partial[patch][w][0..1] with a plain load-add-store: one writer per row, candidates and bounces in order, no atomics -- the same
// bits run to run.  The rows are zeroed on the stream in front of the first block's launch, accumulate over the blocks' launches and
// are reduced in patch order into fp64 by vjp_reduce_kernel.  i and j are compile-time indices behind the wave-uniform guards i < k
// and j < nf.  p[0] is the transmitter: `fixed` on an RX grid, the lane's cell on a TX grid (begin() loads X[cell], Y[cell]; cell <
// cells).  Wall indices come from the sweep's own candidates, 0 <= w < N, so 2 w + 1 < 2 N: inside the table and inside a row.
struct WallGradArgs {
    const float* re_bar;   // [nf][cells]: this block's cotangent planes
    const float* im_bar;   // [nf][cells]
    const float4* refl;    // the context's wall table: row 2 w = {ox, oy, nx, ny}, row 2 w + 1 = {tx, ty, sq, len}
    const float* X;        // [cells] the grid (read on a TX grid only)
    const float* Y;        // [cells]
    float* partial;        // [patches][N][2] per-patch sums, zeroed in front of the first block
    long cells;            // m * n
    float inv[POS_CHUNK];  // turns per unit length, finite and >= 0; entries at and past nf are not read
    int nf;                // 1 .. POS_CHUNK
    int N;                 // walls: a row holds 2 N floats
    int amplitude;         // D2D_FIELD_AMP_SQRT / D2D_FIELD_AMP_LINEAR
    int fun_id;            // the caller's fused path function
    float h2;              // height * height, as the sweep has it
    int txg;               // the cell is the transmitter
    float fx, fy;          // the fixed end point
};
static_assert(sizeof(SweepArgs) + sizeof(WallGradArgs) <= 4096, "power_sink_kernel's arguments must fit the 4 KiB kernel-argument segment");
struct WallGradSink {
    using Args = WallGradArgs;
    static constexpr bool WANTS_R = true, WANTS_DIR = false, WANTS_SEG = true;
    float rb[POS_CHUNK], ib[POS_CHUNK];
    const WallGradArgs* x;  // the kernel argument: wave-uniform, read where it is used
    float* row;             // partial[tile]
    float px, py;           // p[0] of this lane's paths
    bool live;              // cell >= 0
    __device__ __forceinline__ void begin(const WallGradArgs& xa, long tile, int lane_cell) {
        live = lane_cell >= 0;
        load_cotangents(xa.re_bar, xa.im_bar, xa.cells, xa.nf, lane_cell, rb, ib);
        x = &xa;
        row = xa.partial + (size_t)tile * 2 * (size_t)xa.N;
        px = xa.fx;
        py = xa.fy;
        if (xa.txg != 0 && live) {
            px = xa.X[lane_cell];
            py = xa.Y[lane_cell];
        }
    }
    // seg: (p[i+1] - p[i]) for i < k of the candidate (stale or zero where its contribution is zero)
    __device__ __forceinline__ void put_seg(float t, unsigned long long code, int k, float r, const float (&seg)[2 * D2D_MAX_ORDER]) {
        bool p;
        if (k == 0 || no_contribution(t, p)) return;  // wave-uniform (the line of sight touches no wall)
        // per lane: dL/dr of this path for this block
        float G = 0.0f;
        if (p) {
            const float a = posgrad_amp(x->amplitude, t);
            const float kr = posgrad_kr(x->amplitude, posgrad_rho(x->fun_id, x->h2, r));
            const int nf = x->nf;
            float g = 0.0f;
            static_for<0, POS_CHUNK>([&](auto JJ) {
                constexpr int J = decltype(JJ)::value;
                if (J < nf) g = posgrad_fold(g, kr, r, x->inv[J], rb[J], ib[J]);
            });
            G = a * g;
        }
        const bool go = p && live;  // (per lane: it becomes zero weights, never an exit)
        const bool lane0 = (threadIdx.x & 63) == 0;
        float qx = px, qy = py;
        static_for<0, D2D_MAX_ORDER>([&](auto II) {
            constexpr int I = decltype(II)::value;
            if (I < k) {
                const int w = __builtin_amdgcn_readfirstlane((int)((code >> (12 * I)) & 0xfffull));
                const float4 on = ldc4(x->refl, 2 * w), tt = ldc4(x->refl, 2 * w + 1);
                float Wa, Wb;
                const bool ok = wallgrad_bounce(G, qx, qy, seg[2 * I], seg[2 * I + 1], on.x, on.y, on.z, on.w, tt.x, tt.y, tt.z, Wa, Wb);
                const bool count = go && ok;
                const float Sa = wave_sum(count ? Wa : 0.0f), Sb = wave_sum(count ? Wb : 0.0f);  // every lane of the wave is here: the exits above are wave-uniform
                if (lane0) {
                    row[2 * w] = row[2 * w] + Sa;
                    row[2 * w + 1] = row[2 * w + 1] + Sb;
                }
            }
        });
    }
    __device__ __forceinline__ void end(const WallGradArgs&, long, int) const {}
};

// One candidate into a sink: a WANTS_SEG sink takes put_seg (the contribution, the candidate's code and order, the length and the
// segments that reach its bounces), a sink that wants both the length and the directions takes put_rd, a WANTS_DIR sink the
// contribution with the path's end directions, every other one the contribution with the candidate's code, order and length
template <class S>
__device__ __forceinline__ void sink_put(S& s, float t, unsigned long long code, int k, float r, const float (&dir)[4],
                                         const float (&seg)[2 * D2D_MAX_ORDER]) {
    if constexpr (S::WANTS_SEG) s.put_seg(t, code, k, r, seg);
    else if constexpr (S::WANTS_DIR && S::WANTS_R) s.put_rd(t, r, dir);
    else if constexpr (S::WANTS_DIR) s.put_dir(t, dir);
    else s.put(t, code, k, r);
}

// What a wave that owns patch `tile` starts from: its lane's cell (a lane outside the grid takes the nearest cell inside and gets
// cell < 0), lane_bad, zeroed statistics and the bounding box of the wave's cells for the culling.
__device__ __forceinline__ void wave_prologue(const SweepArgs& a, long tile, int lane, float& cx, float& cy, int& cell, bool& lane_bad,
                                              WaveStats& st, float (&bx)[4], float (&by)[4]) {
    const int tiles_x = (a.n + TILE_W - 1) / TILE_W;
    const int tcol = (int)(tile % tiles_x), trow = (int)(tile / tiles_x);
    const int col = tcol * TILE_W + (lane & (TILE_W - 1));
    const int row = trow * TILE_H + (lane / TILE_W);
    const bool in_range = (col < a.n) && (row < a.m);
    const int ccol = col < a.n ? col : a.n - 1;
    const int crow = row < a.m ? row : a.m - 1;
    const long idx = (long)crow * a.n + ccol;
    cx = a.X[idx];
    cy = a.Y[idx];
    cell = in_range ? (int)idx : -1;
    lane_bad = !(fabsf(cx) < 1e18f) || !(fabsf(cy) < 1e18f) || !(fabsf(a.txx) < 1e18f) || !(fabsf(a.txy) < 1e18f);
#pragma unroll
    for (int i = 0; i < 16; ++i) st.c[i] = 0;
    st.shadow = -1;
    st.work = 0;
    // bounding box of the wave's cells (NaN / inf coordinates make every comparison fail: nothing is culled)
    float x0 = cx, x1 = cx, y0 = cy, y1 = cy;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        x0 = fminf(x0, __shfl_xor(x0, off, 64));
        x1 = fmaxf(x1, __shfl_xor(x1, off, 64));
        y0 = fminf(y0, __shfl_xor(y0, off, 64));
        y1 = fmaxf(y1, __shfl_xor(y1, off, 64));
    }
    const bool box_ok = !wave_any(lane_bad);
    bx[0] = box_ok ? x0 : __builtin_nanf("");
    bx[1] = bx[2] = x1;
    bx[3] = x0;
    by[0] = by[1] = y0;
    by[2] = by[3] = y1;
}

// The culled forward sweep with a sink in acc's place (RecSink: d2d_valid_paths, where the host sets fun_id = D2D_FUN_ONE, so a
// contribution is the validity itself; BinSink: d2d_power_profile_launch with the caller's fused path function): one wave per
// 8 x 8 patch in row-major patch order, no schedule, no cut patches, no region lists.  It touches neither the value map nor the
// work history.  Hard and hard_sigmoid only (the sigmoid sweeps' skips depend on the fused function's sum).
template <int MODE, int MAXK, bool TXG, class Sink>
__global__ void __launch_bounds__(64) power_sink_kernel(SweepArgs a, typename Sink::Args x) {
    const int lane = threadIdx.x & 63;
    extern __shared__ float4 tab[];  // [2N] refl, [N] flt, then (a.cullq_off) the culling queue
    for (int i = lane; i < 2 * a.N; i += 64) tab[i] = ldc4(a.refl, i);
    for (int i = lane; i < a.N; i += 64) tab[2 * a.N + i] = ldc4(a.flt, i);
    __syncthreads();
    const long tile = (long)blockIdx.x;
    float cx, cy, bx[4], by[4];
    int cell;
    bool lane_bad;
    WaveStats st;
    wave_prologue(a, tile, lane, cx, cy, cell, lane_bad, st, bx, by);
    Sink sink;
    sink.begin(x, tile, cell);
    float dummy = 0.0f;
    if (a.min_order <= 0 && a.max_order >= 0) {
        // (sweep_order<0>'s one candidate, with the length handed out where the sink wants it)
        const int cand[D2D_MAX_ORDER] = {-1, -1, -1, -1};
        const float imgx[D2D_MAX_ORDER] = {0.0f, 0.0f, 0.0f, 0.0f}, imgy[D2D_MAX_ORDER] = {0.0f, 0.0f, 0.0f, 0.0f};
        float t = 0.0f, rl = 0.0f, dv[4] = {0.0f, 0.0f, 0.0f, 0.0f}, sg[2 * D2D_MAX_ORDER] = {};
        float* const r_out = Sink::WANTS_R ? &rl : nullptr;
        float* const dir_out = Sink::WANTS_DIR ? dv : nullptr;
        float* const seg_out = Sink::WANTS_SEG ? sg : nullptr;
        if constexpr (TXG) eval_candidate<0, MODE, false, false, true, true>(a, cand, imgx, imgy, cx, cy, a.txx, a.txy, lane_bad, t, st, nullptr, -1.0f, r_out, dir_out, seg_out);
        else eval_candidate<0, MODE, false, false, true, false>(a, cand, imgx, imgy, a.txx, a.txy, cx, cy, lane_bad, t, st, nullptr, -1.0f, r_out, dir_out, seg_out);
        sink_put(sink, t, 0ull, 0, rl, dv, sg);
    }
    static_for<1, MAXK + 1>([&](auto KK) {
        constexpr int K = decltype(KK)::value;
        if (a.min_order <= K && a.max_order >= K) {
            if constexpr (TXG)
                sweep_order_culled_txg<K, MODE, false, false, true>(a, tab, bx, by, cx, cy, lane_bad, dummy, st, nullptr, 0, 0x7fffffff, nullptr, nullptr, 0.0f, &sink);
            else
                sweep_order_culled<K, MODE, false, false, false, false, true>(a, tab, bx, by, cx, cy, lane_bad, dummy, st, nullptr, 0, 0x7fffffff, nullptr, nullptr,
                                                                              nullptr, 0.0f, &sink);
        }
    });
    sink.end(x, tile, lane);
}

#ifdef D2D_AUX_KERNELS  // non-template kernels: defined once, in d2d.hip
// ---- the sinks' arithmetic headers on the device, for comparison with their host builds ----
// phasor (d2d_phasor.hpp) on the device, for comparison with its host build (tests/test_gpu_coherent_field.py)
__global__ void selftest_phasor_kernel(const float* __restrict__ f, float* __restrict__ c, float* __restrict__ s, long n) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) phasor(f[i], c[i], s[i]);
}

// turns (d2d_angle.hpp) on the device, for comparison with its host build (tests/test_gpu_power_angle.py)
__global__ void selftest_angle_kernel(const float* __restrict__ dx, const float* __restrict__ dy, float* __restrict__ out, long n) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = turns(dx[i], dy[i]);
}

// unit_dir and steer_phase (d2d_steer.hpp) on the device, for comparison with their host build (tests/test_gpu_array_response.py):
// in = dx, dy, f0, qt, qr, inv and out = ux, uy, ok (0 / 1), f, n values each
__global__ void selftest_steer_kernel(const float* __restrict__ in, float* __restrict__ out, long n) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float ux, uy;
    const bool ok = unit_dir(in[i], in[n + i], ux, uy);
    out[i] = ux;
    out[n + i] = uy;
    out[2 * n + i] = ok ? 1.0f : 0.0f;
    out[3 * n + i] = steer_phase(in[2 * n + i], in[3 * n + i], in[4 * n + i], in[5 * n + i]);
}

// fresnel (d2d_fresnel.hpp) on the device, for comparison with its host build (tests/test_gpu_material_response.py):
// in = er, ei, c and out = gr, gi, n values each
__global__ void selftest_fresnel_kernel(const float* __restrict__ in, float* __restrict__ out, int pol, long n) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float gr, gi;
    fresnel(in[i], in[n + i], in[2 * n + i], pol, gr, gi);
    out[i] = gr;
    out[n + i] = gi;
}

// fresnel_grad (d2d_fresnel_grad.hpp) on the device, for comparison with its host build (tests/test_gpu_material_eps_vjp.py):
// in = er, ei, c and out = gr, gi, dr, di, ok (1 or 0), n values each
__global__ void selftest_fresnel_grad_kernel(const float* __restrict__ in, float* __restrict__ out, int pol, long n) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float gr, gi, dr, di;
    bool ok;
    fresnel_grad(in[i], in[n + i], in[2 * n + i], pol, gr, gi, dr, di, ok);
    out[i] = gr;
    out[n + i] = gi;
    out[2 * n + i] = dr;
    out[3 * n + i] = di;
    out[4 * n + i] = ok ? 1.0f : 0.0f;
}

// the position adjoint's per-contribution arithmetic (d2d_posgrad.hpp) on the device, for comparison with its host build
// (tests/test_gpu_field_position_vjp.py): in = t, r, h2, inv0, inv1, rb0, rb1, ib0, ib1 and out = a, rho, kr, g, G, n values each,
// g the fold over the two wavelengths in order
__global__ void selftest_posgrad_kernel(const float* __restrict__ in, float* __restrict__ out, int fun_id, int amplitude, long n) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float t = in[i], r = in[n + i], h2 = in[2 * n + i];
    const float a = posgrad_amp(amplitude, t);
    const float rho = posgrad_rho(fun_id, h2, r);
    const float kr = posgrad_kr(amplitude, rho);
    float g = 0.0f;
    g = posgrad_fold(g, kr, r, in[3 * n + i], in[5 * n + i], in[7 * n + i]);
    g = posgrad_fold(g, kr, r, in[4 * n + i], in[6 * n + i], in[8 * n + i]);
    out[i] = a;
    out[n + i] = rho;
    out[2 * n + i] = kr;
    out[3 * n + i] = g;
    out[4 * n + i] = a * g;
}

// the wall adjoint's per-bounce arithmetic (d2d_wallgrad.hpp) on the device, for comparison with its host build
// (tests/test_gpu_field_walls_vjp.py): in = G, qx, qy, sx, sy, ox, oy, nx, ny, tx, ty, sq and out = qx, qy after the bounce, Wa, Wb,
// ok (1 or 0), n values each
__global__ void selftest_wallgrad_kernel(const float* __restrict__ in, float* __restrict__ out, long n) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float qx = in[n + i], qy = in[2 * n + i], Wa, Wb;
    const bool ok = wallgrad_bounce(in[i], qx, qy, in[3 * n + i], in[4 * n + i], in[5 * n + i], in[6 * n + i], in[7 * n + i], in[8 * n + i], in[9 * n + i],
                                    in[10 * n + i], in[11 * n + i], Wa, Wb);
    out[i] = qx;
    out[n + i] = qy;
    out[2 * n + i] = Wa;
    out[3 * n + i] = Wb;
    out[4 * n + i] = ok ? 1.0f : 0.0f;
}
#endif  // D2D_AUX_KERNELS

// ---- the launchers (host) ----
// The sinks, stated once in C++: this list declares the per-mode launchers here, and d2d_sweep_tu.hip defines the one its object is
// compiled for.  The Makefile's SINKS is the second statement of this list (one object per sink and mode): a new sink is one line
// here and one word there.  A sink missing there fails the link of libd2d.so (d2d.hip refers to its launchers), one missing here
// fails its object's compilation.  (Hard and hard_sigmoid only: launch_sink answers hipErrorInvalidValue otherwise.)
#define D2D_SINKS(X)                                                                                          \
    X(RecSink)       /* the record build (d2d_valid_paths) */                                                 \
    X(BinSink)       /* the per-cell power-delay profile */                                                   \
    X(TopSink)       /* the per-cell strongest paths */                                                       \
    X(FieldSink)     /* the coherent field */                                                                 \
    X(FreqSink)      /* the frequency response */                                                             \
    X(CoefGradSink)  /* its adjoint w.r.t. the per-object reflection coefficients */                          \
    X(AngleSink)     /* the power-angle profile */                                                            \
    X(ArraySink)     /* the array response */                                                                 \
    X(ArrayFreqSink) /* the wideband array response */                                                        \
    X(BeamSink)      /* the beam-space response */                                                            \
    X(MaterialSink)  /* the frequency response with Fresnel reflection per wall */                           \
    X(EpsGradSink)   /* its adjoint w.r.t. the walls' permittivities */                                       \
    X(PosGradSink)   /* the frequency response's adjoint w.r.t. the cell's and the fixed end point's position */ \
    X(WallGradSink)  /* the frequency response's adjoint w.r.t. the walls' end points */
template <int MODE, class Sink>
hipError_t launch_sink_m(bool txg, int max_order, dim3 grid, size_t lds, hipStream_t s, const SweepArgs& a, const typename Sink::Args& x);
#define D2D_DECLARE_SINK(S)                                                                                                      \
    template <> hipError_t launch_sink_m<MODE_HARD, S>(bool, int, dim3, size_t, hipStream_t, const SweepArgs&, const S::Args&); \
    template <> hipError_t launch_sink_m<MODE_HSIG, S>(bool, int, dim3, size_t, hipStream_t, const SweepArgs&, const S::Args&);
D2D_SINKS(D2D_DECLARE_SINK)
#undef D2D_DECLARE_SINK
// power_sink_kernel<MODE, MAXK, TXG, Sink> by mode (d2d.hip): the culled sweep into one of D2D_SINKS (any other mode: hipErrorInvalidValue)
template <class Sink>
hipError_t launch_sink(int mode, bool txg, int max_order, dim3 grid, size_t lds, hipStream_t stream, const SweepArgs& a, const typename Sink::Args& x);

}  // namespace d2d
