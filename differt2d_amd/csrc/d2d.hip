// libd2d.so -- host side of the C ABI declared in include/d2d.h (HIP runtime, gfx950 only).
// No CPU fallback lives here: every sweep is a kernel launch.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <cstdlib>
#include <vector>

#include "../../include/d2d.h"
#define D2D_AUX_KERNELS 1  // the non-template kernels are defined in this translation unit
#include "d2d_launch.hpp"
#include "d2d_sinks.hpp"
#include "d2d_host.hpp"
#include "d2d_own.hpp"
#include "d2d_optgrad.hpp"
#include "d2d_optrev.hpp"

// ---- mode dispatch of the sweep-kernel launchers; the per-mode launchers (declared in d2d_launch.hpp too) live in the
// d2d_sweep_tu objects, one per (kernel family, validity mode) ----
namespace d2d {

#define D2D_BY_MODE(fn, ...)                                   \
    switch (mode) {                                            \
        case MODE_HARD: return fn<MODE_HARD>(__VA_ARGS__);     \
        case MODE_HSIG: return fn<MODE_HSIG>(__VA_ARGS__);     \
        default: return fn<MODE_SIG>(__VA_ARGS__);             \
    }

static_assert(d2d_host::SWEEP_HARD == MODE_HARD && d2d_host::SWEEP_HSIG == MODE_HSIG && d2d_host::SWEEP_SIG == MODE_SIG,
              "sweep_thresholds' modes are d2d::Mode");

hipError_t launch_fwd(int mode, bool listed, bool stats, int max_order, dim3 grid, size_t lds, hipStream_t s, const SweepArgs& a) {
    if (listed) { D2D_BY_MODE(launch_fwd_listed_m, stats, max_order, grid, lds, s, a) }
    D2D_BY_MODE(launch_fwd_m, stats, max_order, grid, lds, s, a)
}
hipError_t launch_fwd_grad(int mode, bool listed, int max_order, dim3 grid, size_t lds, hipStream_t s, const SweepArgs& a) {
    if (listed) { D2D_BY_MODE(launch_fwd_grad_listed_m, max_order, grid, lds, s, a) }
    D2D_BY_MODE(launch_fwd_grad_m, max_order, grid, lds, s, a)
}
hipError_t launch_fwd_split(int mode, bool listed, bool stats, int max_order, dim3 grid, size_t lds, hipStream_t s, const SweepArgs& a) {
    if (listed) { D2D_BY_MODE(launch_fwd_split_listed_m, stats, max_order, grid, lds, s, a) }
    D2D_BY_MODE(launch_fwd_split_m, stats, max_order, grid, lds, s, a)
}
hipError_t launch_fwd_coop(int mode, int max_order, int W, dim3 grid, size_t lds, hipStream_t s, const SweepArgs& a) {
    D2D_BY_MODE(launch_fwd_coop_m, max_order, W, grid, lds, s, a)
}
hipError_t launch_txg(int mode, bool listed, bool grad, int max_order, dim3 grid, size_t lds, hipStream_t s, const SweepArgs& a) {
    D2D_BY_MODE(launch_txg_m, listed, grad, max_order, grid, lds, s, a)
}
hipError_t launch_vg(int mode, bool txg, bool grad, dim3 grid, size_t lds, hipStream_t s, const SweepArgs& a) {
    D2D_BY_MODE(launch_vg_m, txg, grad, grid, lds, s, a)
}
template <class Sink>
hipError_t launch_sink(int mode, bool txg, int max_order, dim3 grid, size_t lds, hipStream_t s, const SweepArgs& a, const typename Sink::Args& x) {
    if (mode == MODE_HARD) return launch_sink_m<MODE_HARD, Sink>(txg, max_order, grid, lds, s, a, x);
    if (mode == MODE_HSIG) return launch_sink_m<MODE_HSIG, Sink>(txg, max_order, grid, lds, s, a, x);
    return hipErrorInvalidValue;
}

}  // namespace d2d

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return fail(D2D_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

using d2d_own::DevBuf;
using Event = d2d_own::Unique<hipEvent_t, d2d_own::event_destroy>;
using Stream = d2d_own::Unique<hipStream_t, d2d_own::stream_destroy>;
template <typename T> using Pinned = d2d_own::Unique<T*, d2d_own::pinned_free>;

using d2d_host::integer_pow;

}  // namespace

// the runtime calls behind d2d_own.hpp's owning types: the only places that free or destroy anything
int d2d_own::dev_alloc(void** p, size_t bytes) {
    const hipError_t e = hipMalloc(p, bytes);
    return e == hipSuccess ? D2D_OK : fail(D2D_ERR_HIP, "hipMalloc((void**)&p, count * sizeof(T)) failed: %s", hipGetErrorString(e));
}
void d2d_own::dev_free(void* p) { (void)hipFree(p); }
void d2d_own::pinned_free(void* p) { (void)hipHostFree(p); }
void d2d_own::event_destroy(void* h) { (void)hipEventDestroy((hipEvent_t)h); }
void d2d_own::stream_destroy(void* h) { (void)hipStreamDestroy((hipStream_t)h); }

// Every device buffer, event, stream and the pinned h_meta is an owning member (d2d_own.hpp): ~d2d_ctx drains the streams
// and the members free themselves, in reverse order of declaration.  Invariant: `stream` is declared first, so it dies
// last, after every buffer and event that work on it may still reference; the other streams are declared where they
// belong and are idle by then (the destructor's body has synchronised each of them; d2d_create's failure paths end there too).
struct d2d_ctx {
    int device = 0;
    Stream stream;
    Event ev0, ev1, evk0, evk1;  // evk*: around the dominant kernel of the last sweep ("time_kernel" option)
    bool time_kernel = false, have_kernel_time = false;
    // scene (host copies)
    int N = 0;
    bool have_scene = false;
    std::vector<float> xys;        // [N][2][2]
    std::vector<uint8_t> kind;     // [N]
    std::vector<float> phi;        // [N]
    std::vector<uint8_t> allowed;  // [N]
    std::vector<int> cw;           // compact list of allowed indices
    float occl_patch = NAN;        // patch the occlusion table was built for
    // wall-to-wall masks (pair_shadow_kernel): scene-only, rebuilt when the scene or one of these parameters changes
    DevBuf<unsigned long long> d_pair;
    bool pair_valid = false;
    // last-segment masks of the leaf regions (hidden_region_kernel): scene, grid and validity mode only; built by the second
    // launch in a row that would use them (a one-off map does not pay for them) and kept until one of those changes
    DevBuf<unsigned long long> d_hidden;
    bool hidden_valid = false;
    double hidden_key[12] = {0}, hidden_seen[12] = {0};
    bool use_hidden_masks = true;       // "hidden_masks" option (tests: the reference that never builds them; same results)
    long long hidden_min_tiles = 400;   // ... for launches of at least this many patches ("hidden_min_tiles" option)
    long long hidden_builds = 0;        // diagnostic
    float pair_key[6] = {0, 0, 0, 0, 0, 0};  // patch, seg_tol, approx, act, alpha, dperp
    bool use_pair_masks = true;
    // scene (device)
    DevBuf<float4> d_occl, d_refl, d_flt;
    DevBuf<int> d_cw;
    DevBuf<unsigned char> d_kind;
    DevBuf<float2> d_sincos;
    DevBuf<float4> d_xys;  // raw end points {origin, dest} (gradient sweeps of the optimiser-based solvers)
    // optimiser-based solvers
    DevBuf<float> d_bc1, d_bc2, d_theta0, d_contrib, d_gcontrib, d_traj;
    DevBuf<long long> d_traj_off;
    long long opt_grad_mode = 0;    // gradients through the solvers: 0 reverse mode over the stored trajectory (d2d_optrev.hpp), 1 forward tangents (d2d_optgrad.hpp)
    long long opt_traj_mb = 16384;  // device memory the trajectory store may take; grids that need more are swept in chunks of cells
    bool opt_parallel = true;  // optimiser-based sweeps: candidates side by side (same results as one after the other)
    int bc_steps = -1;
    double bc_b1 = 0.0, bc_b2 = 0.0;    // ... and the decay rates the tabulated bias corrections belong to
    double opt_lr = 0.1, opt_b1 = 0.9, opt_b2 = 0.999, opt_eps = 1e-8;  // d2d_set_optimizer (optax.adam's defaults, optimize.py:83)
    int opt_kind = D2D_OPT_ADAM;  // D2D_OPT_SGD*: opt_b1 holds the momentum, opt_b2 the Nesterov flag (include/d2d.h)
    std::vector<float> theta0;  // [C][D2D_MAX_ORDER] as set by d2d_set_theta0
    DevBuf<int> d_scand, d_sorder;
    // trace scratch
    DevBuf<int> d_tcand, d_torder;
    DevBuf<float> d_ttx, d_trx, d_txys_in, d_tloss_in, d_txys, d_tloss, d_tvalid, d_ton, d_thit, d_tlen;
    // record launch of the culled sweep (d2d_valid_paths): kept between calls, grown when needed, dropped with the grid
    DevBuf<unsigned long long> d_rec_shadow;  // its own shadow masks: the sweeps' rotating sets are not touched
    DevBuf<int> d_rec_counts, d_rec_offs, d_rec_flag, d_rec_cell, d_rec_cand, d_rec_order;
    DevBuf<int4> d_rec;
    DevBuf<float> d_rec_xys, d_rec_loss, d_rec_valid, d_rec_len;
    long long rec_n = -1;  // records the buffers hold (-1: none)
    Event ev_rec[6];  // "time_kernel": around pass 1, pass 2 and the trace
    bool have_rec_time = false;
    // ---- results of the products of the sink kernel: buffers and what they hold, one struct each.  forget() ends the result's
    // validity and keeps the buffers (a launch that is about to change them), drop() releases them as well (another grid).
    struct Planes {  // planes of re and im and the total of every cell
        DevBuf<float> re, im, total;
        size_t bytes() const { return (re.n + im.n + total.n) * sizeof(float); }
        int ensure(size_t planes, size_t cells) {
            int rc;
            return (rc = re.ensure(planes)) || (rc = im.ensure(planes)) ? rc : total.ensure(cells);
        }
        void release() { re.release(); im.release(); total.release(); }
    };
    // per-cell power-delay profile (d2d_power_profile_launch), kept until the next launch
    struct Profile {
        DevBuf<float> out;  // [nbins][m][n]
        int nbins = 0;      // bins the buffer holds a profile of (0: none)
        void forget() { nbins = 0; }
        void drop() { out.release(); forget(); }
    } prof;
    // per-cell strongest paths (d2d_strongest_paths_launch): the first k slots of every cell, kept until the next launch
    struct Top {
        DevBuf<float> power, len, total;  // [k][m][n], [k][m][n], [m][n]
        DevBuf<int> cand, order, count;   // [k][m][n][D2D_MAX_ORDER], [k][m][n], [m][n]
        int k = 0;  // slots per cell the buffers hold a result of (0: none)
        size_t bytes() const { return (power.n + len.n + total.n + cand.n + order.n + count.n) * 4; }
        void forget() { k = 0; }
        void drop() { power.release(); len.release(); total.release(); cand.release(); order.release(); count.release(); forget(); }
    } top;
    // coherent field (d2d_coherent_field_launch): re, im and the incoherent total of every cell, kept until the next launch
    struct Field {
        Planes out;  // [m][n] each
        bool have = false;
        void forget() { have = false; }
        void drop() { out.release(); forget(); }
    } field;
    // frequency response (d2d_frequency_response_launch): nf planes of re and im and the incoherent total, kept until the next launch
    struct Freq {
        Planes out;      // [nf][m][n], [nf][m][n], [m][n]
        int32_t nf = 0;  // planes of the last accepted launch; 0: no result
        void forget() { nf = 0; }
        void drop() { out.release(); forget(); }
    } freq;
    // power-angle profile (d2d_power_angle_launch): nbins planes and the total of every cell, kept until the next accepted launch
    struct Angle {
        DevBuf<float> out, total;  // [nbins][m][n], [m][n]
        int32_t nbins = 0;         // bins of the last accepted launch; 0: no result
        void forget() { nbins = 0; }
        void drop() { out.release(); total.release(); forget(); }
    } angle;
    // array response (d2d_array_response_launch): nr * nt planes of re and im and the total, kept until the next accepted launch
    struct Array {
        Planes out;              // [nr][nt][m][n] twice, [m][n]
        int32_t nt = 0, nr = 0;  // counts of the last accepted launch; 0: no result
        void forget() { nt = nr = 0; }
        void drop() { out.release(); forget(); }
    } array;
    // coefficient adjoint of the frequency response (d2d_field_coefs_vjp_launch): the cotangent planes, the per-patch rows and the
    // reduced result, kept until the next accepted launch; the scene forgets it too
    struct CoefGrad {
        DevBuf<float> re, im;    // [nf][m][n] each: the caller's cotangents
        DevBuf<float> partial;   // [patches][N]
        DevBuf<double> out;      // [N]
        bool have = false;       // out holds the result of an accepted launch for the CURRENT grid and scene
        void forget() { have = false; }
        void drop() { re.release(); im.release(); partial.release(); out.release(); forget(); }
    } cg;
    // wideband array response (d2d_array_frequency_response_launch): nf * nr * nt planes of re and im and the total, kept until
    // the next accepted launch
    struct Wide {
        Planes out;                      // [nf][nr][nt][m][n] twice, [m][n]
        int32_t nf = 0, nt = 0, nr = 0;  // counts of the last accepted launch; 0: no result
        void forget() { nf = nt = nr = 0; }
        void drop() { out.release(); forget(); }
    } wide;
    // beam-space response (d2d_beam_response_launch): nf * nbr * nbt planes of re and im and the total, kept until the next accepted
    // launch
    struct Beam {
        Planes out;                        // [nf][nbr][nbt][m][n] twice, [m][n]
        DevBuf<float> w;                   // [2][BEAM_MAX][ARRAY_MAX][2]: the two weight tables of the launch in flight
        int32_t nf = 0, nbt = 0, nbr = 0;  // counts of the last accepted launch; 0: no result
        void forget() { nf = nbt = nbr = 0; }
        void drop() { out.release(); w.release(); forget(); }
    } beam;
    // material response (d2d_material_response_launch): nf planes of re and im and the total, kept until the next accepted launch;
    // the scene forgets it too (it depends on the walls' count)
    struct Material {
        Planes out;          // [nf][m][n], [nf][m][n], [m][n]
        DevBuf<float> eps;   // [nf][N][2]: the permittivity table of the launch in flight
        int32_t nf = 0;      // planes of the last accepted launch; 0: no result
        size_t bytes() const { return out.bytes() + eps.n * sizeof(float); }
        void forget() { nf = 0; }
        void drop() { out.release(); eps.release(); forget(); }
    } mat;
    // permittivity adjoint of the material response (d2d_material_eps_vjp_launch): the cotangent planes, the permittivity table,
    // one chunk's per-patch rows and the reduced result, kept until the next accepted launch; the scene forgets it too
    struct EpsGrad {
        DevBuf<float> re, im;    // [nf][m][n] each: the caller's cotangents
        DevBuf<float> eps;       // [nf][N][2]: the permittivity table of the launch in flight
        DevBuf<float> partial;   // [patches][MAT_CHUNK][N][2]
        DevBuf<double> out;      // [nf][N][2]
        int32_t nf = 0;          // rows of the last accepted launch for the CURRENT grid and scene; 0: no result
        size_t bytes() const { return (re.n + im.n + eps.n + partial.n) * sizeof(float) + out.n * sizeof(double); }
        void forget() { nf = 0; }
        void drop() { re.release(); im.release(); eps.release(); partial.release(); out.release(); forget(); }
    } eg;
    // position adjoint of the frequency response (d2d_field_position_vjp_launch): the cotangent planes, the four planes the passes
    // carry, the reduction's partial sums and the reduced result, kept until the next accepted launch; the scene forgets it too
    struct PosGrad {
        DevBuf<float> re, im;          // [nf][m][n] each: the caller's cotangents
        DevBuf<float> cell, terms;     // [2][m][n] each: cell_bar, fixed_terms
        DevBuf<double> part, out;      // [2][POS_REDUCE_BLOCKS], [2]: fixed_bar and the sums it is made of
        bool have = false;             // the buffers hold the result of an accepted launch for the CURRENT grid and scene
        size_t bytes() const { return (re.n + im.n + cell.n + terms.n) * sizeof(float); }
        void forget() { have = false; }
        void drop() { re.release(); im.release(); cell.release(); terms.release(); part.release(); out.release(); forget(); }
    } pg;
    // wall adjoint of the frequency response (d2d_field_walls_vjp_launch): the cotangent planes, the per-patch rows and the reduced
    // result, kept until the next accepted launch; the scene forgets it too
    struct WallGrad {
        DevBuf<float> re, im;    // [nf][m][n] each: the caller's cotangents
        DevBuf<float> partial;   // [patches][N][2]
        DevBuf<double> out;      // [N][2]: normal_bar
        bool have = false;       // out holds the result of an accepted launch for the CURRENT grid and scene
        size_t bytes() const { return (re.n + im.n + partial.n) * sizeof(float); }
        void forget() { have = false; }
        void drop() { re.release(); im.release(); partial.release(); out.release(); forget(); }
    } wg;
    void drop_products() {  // every one of them goes with the grid
        prof.drop(); top.drop(); field.drop(); freq.drop(); angle.drop(); array.drop(); cg.drop(); wide.drop(); beam.drop(); mat.drop(); eg.drop(); pg.drop(); wg.drop();
    }
    void drop_records() {
        d_rec_counts.release(); d_rec_offs.release(); d_rec_cell.release(); d_rec_cand.release(); d_rec_order.release();
        d_rec.release(); d_rec_xys.release(); d_rec_loss.release(); d_rec_valid.release(); d_rec_len.release();
        rec_n = -1;
    }
    // grid
    int m = 0, n = 0;
    bool have_grid = false;
    DevBuf<float> d_X, d_Y, d_out;
    DevBuf<unsigned long long> d_stats;
#ifdef D2D_AB_TIMELINE
    DevBuf<unsigned> d_timeline;
    long long timeline_n = 0;
    DevBuf<unsigned long long> d_tl_ring;
    bool tl_ring_on = false;
    long long tl_seq = 0;
#endif
    DevBuf<int> d_sched_override;       // diagnostic: a caller-supplied schedule (d2d_debug_set_schedule)
    long long sched_override_n = 0;
    bool use_cost_history = true;
    long long fwd_waves = 0;            // patches (= waves) per workgroup of the LISTED forward sweep kernel: 1, 4, or 0 = by the table's size
    bool txg_exhaustive = false;        // TX-grid value sweeps with the exhaustive kernel (A/B and tests)
    long long sched_min_tiles = 2048;   // launches with fewer patches keep the identity schedule
    uint64_t grid_token = 0;  // the caller's version token of the resident grid (valid with have_grid; 0: none, see grid_shadow)
    uint64_t grid_fp = 0;                    // strided sample of the resident grid's arrays (checked beside the token)
    std::vector<float> grid_shadow;  // host copy of the resident grid, [X | Y], kept by the token-less d2d_set_grid: equality is
                                     // a byte-for-byte comparison with it (8 B per cell of host memory; empty: not kept)
    int last_shape_waves = 0, last_shape_coop = 0;  // diagnostic: d2d_debug_sweep_shape
    long long txg_fallbacks = 0;  // diagnostic: d2d_debug_txg_fallbacks
    long long grid_reuses = 0;  // d2d_set_grid calls that found their grid resident already (diagnostic: d2d_debug_grid_reuses)
    float grid_absmax = 0.0f;   // max |coordinate| of the grid (host scan at d2d_set_grid)
    bool grid_all_finite = false;  // every cell coordinate is below 1e18 in magnitude (what the kernels call comfortably finite)
    float scene_absmax = 0.0f;  // max |coordinate| of the objects
    // value+grad
    DevBuf<float> d_grad, d_cot, d_partial;
    DevBuf<float> d_cust_f, d_cust_pb;  // d2d_set_path_fun_values: a host-evaluated path function, [C][cells] and [C][cells][NP][2]
    long long cust_C = -1;              // candidates they hold (-1: none); reset by d2d_set_grid
    DevBuf<double> d_vjp;  // [4N] end points, [2] fixed point, [N] phi, [N] reflection coefficients
    // d2d_set_reflection_coefs (D2D_FUN_RECEIVED_POWER_PER_OBJECT): one coefficient per object of the resident scene
    std::vector<float> coef;   // host copy (empty: none set)
    DevBuf<float> d_coef;      // [N], beside refl / occl
    DevBuf<float> d_coef_partial;  // [patches][N] per-patch sums of the coefficient adjoint
    bool vjp_has_coef = false;  // d_vjp[5N+2 .. 6N+2) holds d/d coef (else: identically 0)
    bool have_cot = false;
    bool have_vjp = false;   // d_vjp holds the scene VJP of a sweep of the CURRENT scene (4 N + 2 values)
    bool vjp_has_phi = false;  // d_vjp[4N+2 .. 5N+2) holds d/d phi (optimiser-based sweeps); image sweeps: identically 0
    bool vjp_reduced = false;  // d_vjp has been all-reduced over ranks: it is a global sum, nothing local may be added to it
    bool have_grad = false;  // d_grad holds the per-cell gradient map of a sweep of the CURRENT grid (2 m n values)
    // NaN scan behind the culled value+grad sweeps (d2d_nanscan.hpp): the reference's autodiff NaN positions, all of them
    bool nan_scan = true;               // "nan_scan" option (0: round 3's behaviour -- only the evaluated candidates' NaN; A/B and tests)
    long long nan_scan_mode = 1;        // ... 1: two levels (regions of 4 x 4 patches, then patches), 2: one wave per patch (A/B and tests; same flags)
    bool nan_scan_stats = false;        // "nan_scan_stats" option: count probes / flagged cells / flagged patches (d2d_debug_nan_scan)
    DevBuf<unsigned long long> d_nan_stats;
    size_t lds_max = d2d_host::LDS_MAX;  // dynamic LDS a launch without a choice may take (gfx950: the CU's 160 KB less 4 KB of static LDS, d2d_host.hpp; d2d_create lowers it to what the device reports)
    long long nan_wqcap = 0, nan_rb = 0;  // "nan_scan_wqcap" / "nan_scan_rb": the region scan's queue entries / batches per round in use (0: all; tests)
    Stream scan_stream;  // created at the first use, at the lowest priority
    Event ev_scan_fork, ev_scan_done;
    DevBuf<unsigned long long> d_nan_cells;  // [patches]
    DevBuf<unsigned> d_nan_rows;             // [patches][1 + ceil(N / 32)]
    bool want_wave_cycles = false;
    long long split_max_tiles = -1;     // launches up to this many patches share every patch between 4 waves (-1: by the validity mode)
    long long coop_max_tiles = -1;      // ... and up to this many candidate by candidate (power_fwd_coop_kernel); -1: by the validity mode
    bool split_sigmoid = false;         // sigmoid validity: share patches prefix by prefix like the other modes (slower: A/B and tests)
    long long coop_waves = -1;          // its waves per patch: -1 by the launch's size and mode (16 / 8 / none), 0 never, else 4, 8 or 16
    long long heavy_split = -1;        // bigger launches with a work history: this many of the dearest patches are cut in four (-1: by the launch's size)
    DevBuf<float> d_heavy_list;
    DevBuf<int> d_heavy_cnt, d_heavy_done;
    long long heavy_done_n = 0;
    // region candidate lists (region_list_kernel / region_refine_kernel), rebuilt by every culled RX-grid launch of max_order >= 2
    bool use_region_lists = true;
    long long region_size = 4;         // leaf regions (what the sweep kernels read) are region_size x region_size patches
    long long region_size_top = 16;    // regions listed by enumeration (a multiple of region_size; equal: one level only)
    long long region_slices = 0;       // slices of first walls per enumerated region (0: chosen from the number of allowed walls)
    long long region_budget_mb = 24576; // device memory all list pools together may grow to (one pool per rotating set)
    long long rl_pool_mb = 256;        // its current size: quadrupled (up to the budget) after a launch whose lists did not fit
    bool rl_pool_by_option = false;    // "region_budget_mb" was set by the caller: no automatic first size
    Stream aux_stream;  // the patch schedule's sort runs here, beside the shadow masks and the region lists
    Stream sort_stream; // .. and here when aux_stream carries the whole preparation (pipeline)
    Event ev_fork, ev_join;
    Pinned<int> h_meta;                // pinned: {patches left to the enumerating kernel, pool chunks handed out} of the last launch with lists
    Event ev_meta;
    bool meta_pending = false;
    long long rl_meta_static = 0, rl_meta_chunks = 0;  // n_static / max_chunks of the last launch that built lists
    long long pend_static = 0, pend_chunks = 0;        // ... of the launch the pending h_meta read-back describes
    long long fb_hint = 0;             // patches the last such launch left to the enumerating kernel
    float rl_vkey[6] = {-1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};  // validity parameters of the last launch with lists
    long long rl_launches = 0;         // launches with lists since the plan last changed (the read-back thins out: 1, 2, 3, then every 16th)
    DevBuf<float4> d_rl_box;           // bounding boxes of the leaf regions, then of the top regions (region_box_kernel)
    long long rl_box_key[4] = {-1, 0, 0, 0};  // grid version, leaf R, top R (0: one level) the boxes were built for
    long long grid_version = 0;        // bumped by d2d_set_grid
    d2d_host::RegionPlan rl_plan;      // of the last launch that built lists (rl_plan.on) -- d2d_debug_region_stats
    int rl_max_order = 0;
    // Pipelined preparation.  Everything a launch rebuilds before its sweep kernel (shadow masks, region lists, patch
    // schedule) lives in a PrepSet: `cur` is the set of the current launch, spare_sets[] the others (they rotate at the
    // start of every pipelined sweep launch).  The preparation of launch k+1 runs on aux_stream into its own set while the
    // sweep kernel of launch k still reads another one on the main stream: back-to-back launches (many transmitters, the
    // benchmark) hide it completely.  The work history a schedule is sorted by is then a few launches old instead of one.
    // (a PrepSet moves through its members: the rotation's std::swap hands buffers, event and flags over together)
    struct PrepSet {
        DevBuf<unsigned long long> d_shadow;  // shadow masks, then the schedule sort's histogram and cursors, then the lists' meta
        DevBuf<int> d_sched;                  // patch schedule
        DevBuf<unsigned char> d_sched_key;
        DevBuf<unsigned> d_cost;              // what every patch cost in the last culled sweep of this grid (ticks >> 6)
        long long cost_tiles = 0;             // 0 = no history (scene, grid or candidate mask changed since)
        DevBuf<unsigned long long> d_rl_pool;
        DevBuf<int> d_rl_next;                // [max_chunks]
        DevBuf<int> d_rl_idx;                 // first / cnt arrays of both levels, all orders
        DevBuf<int> d_rl_meta;                // the queue of patches left to the enumerating kernel
        int* rl_meta_ptr = nullptr;           // (inside d_shadow) [0] queue length, [1] pool head, [2 ..) leaf region flags
        DevBuf<d2d::RegionLists> d_rl;        // the descriptor the sweep kernels read
        d2d::RegionLists rl_host;             // what d_rl holds
        bool rl_host_valid = false;
        Event ev_swept;                       // recorded on the main stream behind the sweep that read this set
        bool swept_pending = false;
    };
    PrepSet cur;
    static constexpr int N_SPARE = 2;   // three sets in all: the preparation runs freely ahead on its own streams (with two sets it
                                        // could not start before the sweep before last had finished, i.e. at the very moment the
                                        // previous sweep starts, and the sweep then waited for the tail of the chain: 0.111 ->
                                        // 0.107 ms per step at cfg2 once the sort had left the chain)
    PrepSet spare_sets[N_SPARE];        // [0] the oldest (next to be reused) .. [N_SPARE - 1] the previous launch's
    template <class F> void for_each_set(F f) {
        f(cur);
        for (PrepSet& sp : spare_sets) f(sp);
    }
    Event ev_prep;                      // recorded on aux_stream behind a launch's preparation
    bool pipeline = true;
    long long unpiped_max_tiles = 256; // "unpiped_max_tiles": launches of orders <= 1 over at most this many patches prepare on the sweep's own stream (latency of a small call)
    bool last_small = false;           // ... what the previous launch was (a change of kind drains both streams first)
    // RCCL (one communicator per ctx, collectives run on the ctx stream)
    ncclComm_t comm = nullptr;
    int rank = 0, world = 1;
    DevBuf<float> d_gather[2], d_send[2];  // [0] value map, [1] gradient map: gathered shards / staging copy of the local shard
    // the all-gather of step k runs on its own stream, overlapped with the sweep of step k+1
    Stream comm_stream;
    long long comm_prio = 0;  // "comm_prio" option: priority of comm_stream when it is created
    // every collective runs on comm_stream behind a "ready" event of the main stream; [0] value-map gather, [1] gradient-map
    // gather, [2] scene-VJP all-reduce; the main stream waits for ev_done[i] only where it reuses what collective i touches
    Event ev_ready, ev_done[3];
    bool inflight[3] = {false, false, false};
    DevBuf<double> d_hostred;
    size_t gathered[2] = {0, 0};  // floats per rank in d_gather[what] (0: nothing gathered on this rank)
    ~d2d_ctx();
};

namespace {

int set_device(d2d_ctx* c) {
    HIP_TRY(hipSetDevice(c->device));
    return D2D_OK;
}

// Per-object constants, computed once with the reference's operations (fp32, no contraction):
// t = dest - origin (geometry.py:479-487), n = normalize((t_y, -t_x)) (:561-573, 206-230),
// sq = where(t.t == 0, 1, t.t) (:596-597).
int upload_refl(d2d_ctx* c) {
    std::vector<float4> refl(2 * (size_t)c->N + 2);
    std::vector<float4> flt((size_t)c->N + 1);
    for (int j = 0; j < c->N; ++j) {
        const float* w = &c->xys[4 * (size_t)j];
        float ox = w[0], oy = w[1], dx = w[2], dy = w[3];
        float tx = dx - ox, ty = dy - oy;
        float vx = ty, vy = -tx;
        float len = sqrtf(vx * vx + vy * vy);
        if (len == 0.0f) len = 1.0f;
        float nx = vx / len, ny = vy / len;
        float sq = tx * tx + ty * ty;
        if (sq == 0.0f) sq = 1.0f;
        refl[2 * j] = make_float4(ox, oy, nx, ny);
        refl[2 * j + 1] = make_float4(tx, ty, sq, len);
        // pre-filter constants: 1/sq and the error-bound coefficient (64 ulp of the magnitudes entering s)
        const double rsq = 1.0 / (double)sq;
        flt[j] = make_float4((float)rsq, (float)(64.0 * 1.1920929e-07 * rsq), 0.0f, 0.0f);
    }
    int rc = c->d_refl.ensure(refl.size());
    if (rc) return rc;
    if ((rc = c->d_flt.ensure(flt.size()))) return rc;
    HIP_TRY(hipMemcpyAsync(c->d_flt.p, flt.data(), flt.size() * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    if ((rc = c->d_kind.ensure((size_t)c->N + 1))) return rc;
    if ((rc = c->d_sincos.ensure((size_t)c->N + 1))) return rc;
    if ((rc = c->d_xys.ensure((size_t)c->N + 1))) return rc;
    if (c->N > 0) HIP_TRY(hipMemcpyAsync(c->d_xys.p, c->xys.data(), (size_t)c->N * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    std::vector<float2> sc((size_t)c->N + 1);
    for (int j = 0; j < c->N; ++j) sc[(size_t)j] = make_float2(sinf(c->phi[j]), cosf(c->phi[j]));  // geometry.py:709-710
    HIP_TRY(hipMemcpyAsync(c->d_refl.p, refl.data(), refl.size() * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    if (c->N > 0) {
        HIP_TRY(hipMemcpyAsync(c->d_kind.p, c->kind.data(), (size_t)c->N, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->d_sincos.p, sc.data(), (size_t)c->N * sizeof(float2), hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return D2D_OK;
}

// Patched end points, geometry.py:632-636: P1 = origin - patch*t, P2 = dest + patch*t, A = P2 - P1.
int upload_occl(d2d_ctx* c, float patch) {
    if (c->occl_patch == patch && c->d_occl.p) return D2D_OK;
    // (N rounded up to an even number of rows, and one more pair: the occlusion loop reads the table two adjacent walls at a
    // time, one pair ahead, without clamping an index -- the wall beside the last one of an odd table and the pair behind the
    // last one must exist in memory.  Rows from N on are zero; they are loaded and take no part in any test)
    std::vector<float4> occl((((size_t)c->N + 1) & ~(size_t)1) + 2, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    for (int j = 0; j < c->N; ++j) {
        const float* w = &c->xys[4 * (size_t)j];
        float ox = w[0], oy = w[1], dx = w[2], dy = w[3];
        float tx = dx - ox, ty = dy - oy;
        float ptx = patch * tx, pty = patch * ty;
        float p1x = ox - ptx, p1y = oy - pty;
        float p2x = dx + ptx, p2y = dy + pty;
        occl[j] = make_float4(p1x, p1y, p2x - p1x, p2y - p1y);
    }
    int rc = c->d_occl.ensure(occl.size());
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(c->d_occl.p, occl.data(), occl.size() * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->occl_patch = patch;
    return D2D_OK;
}

int upload_mask(d2d_ctx* c) {
    c->cw.clear();
    for (int j = 0; j < c->N; ++j)
        if (c->allowed[j]) c->cw.push_back(j);
    int rc = c->d_cw.ensure(c->cw.size() + 1);
    if (rc) return rc;
    if (!c->cw.empty()) {
        HIP_TRY(hipMemcpyAsync(c->d_cw.p, c->cw.data(), c->cw.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return D2D_OK;
}

d2d::ObjTables obj_tables(d2d_ctx* c) {
    d2d::ObjTables T;
    T.occl = c->d_occl.p;
    T.refl = c->d_refl.p;
    T.kind = c->d_kind.p;
    T.sincos = c->d_sincos.p;
    T.xys = c->d_xys.p;
    T.N = c->N;
    return T;
}

// optax.adam(0.1) defaults (optimize.py:83): b1 = 0.9, b2 = 0.999, eps = 1e-8 -- or what d2d_set_optimizer said; bias
// corrections 1 - b^t tabulated in double precision and rounded to fp32 (the oracle does the same).  SGD has no tables.
int opt_cfg(d2d_ctx* c, const d2d_params* p, d2d::OptCfg* A) {
    const int steps = p->steps;
    if (steps < 1 || steps > 1000000) return fail(D2D_ERR_INVALID, "steps must lie in 1..1e6, got %d", steps);
    if (p->many < 0 || p->many > 4096) return fail(D2D_ERR_INVALID, "many must lie in 0..4096, got %d", p->many);
    A->solver = p->solver;
    A->steps = steps;
    A->many = p->many > 1 ? p->many : 1;
    // the hyper-parameters are Python floats on the reference's side (weakly typed: rounded to fp32 where they meet an fp32 array)
    A->lr = (float)c->opt_lr;
    if (c->opt_kind != D2D_OPT_ADAM) {  // optax.sgd
        A->sgd = 1;
        A->momentum = (c->opt_kind == D2D_OPT_SGD_MOMENTUM) ? 1 : 0;
        A->nesterov = (A->momentum && c->opt_b2 != 0.0) ? 1 : 0;
        A->decay = A->momentum ? (float)c->opt_b1 : 0.0f;
        return D2D_OK;
    }
    if (c->bc_steps != steps || c->bc_b1 != c->opt_b1 || c->bc_b2 != c->opt_b2) {
        std::vector<float> b1((size_t)steps + 1), b2((size_t)steps + 1);
        for (int t = 1; t <= steps; ++t) {
            b1[(size_t)t - 1] = (float)(1.0 - std::pow(c->opt_b1, (double)t));
            b2[(size_t)t - 1] = (float)(1.0 - std::pow(c->opt_b2, (double)t));
        }
        int rc;
        if ((rc = c->d_bc1.ensure((size_t)steps + 1)) || (rc = c->d_bc2.ensure((size_t)steps + 1))) return rc;
        if (steps > 0) {
            HIP_TRY(hipMemcpyAsync(c->d_bc1.p, b1.data(), (size_t)steps * sizeof(float), hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipMemcpyAsync(c->d_bc2.p, b2.data(), (size_t)steps * sizeof(float), hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
        c->bc_steps = steps;
        c->bc_b1 = c->opt_b1;
        c->bc_b2 = c->opt_b2;
    }
    A->bc1 = c->d_bc1.p;
    A->bc2 = c->d_bc2.p;
    A->b1 = (float)c->opt_b1;
    A->b2 = (float)c->opt_b2;
    A->eps = (float)c->opt_eps;
    A->sgd = 0;
    // optax.scale_by_adam: (1 - decay) is a Python float (double arithmetic) multiplied into an fp32 array
    A->omb1 = (float)(1.0 - c->opt_b1);
    A->omb2 = (float)(1.0 - c->opt_b2);
    return D2D_OK;
}

// the validity chain's parameters of the solver sweeps' arguments (d2d::OptSweepArgs, d2d::TraceArgs)
template <class Args>
void set_validity(Args& a, const d2d_params* p) {
    a.mode = p->approx ? (p->act == D2D_ACT_HARD_SIGMOID ? d2d::MODE_HSIG : d2d::MODE_SIG) : d2d::MODE_HARD;
    a.alpha = p->alpha;
    a.tol = p->tol;
    a.seg_lo = -p->seg_tol;
    a.seg_hi = 1.0f + p->seg_tol;
}

int check_params(const d2d_params* p) {
    std::string err;
    const int rc = d2d_host::check_params(p, err);
    return rc ? fail(rc, "%s", err.c_str()) : D2D_OK;
}

}  // namespace

namespace {

// librccl is resolved at first use (dlopen), so single-GPU users never need it.
struct Rccl {
    void* h = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetVersion) GetVersion = nullptr;
    decltype(&ncclCommCount) CommCount = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    bool ok = false;
};

Rccl& rccl() {
    static Rccl r;
    if (r.h) return r;
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char* n : names) {
        r.h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
        if (r.h) break;
    }
    if (!r.h) return r;
    r.GetUniqueId = (decltype(r.GetUniqueId))dlsym(r.h, "ncclGetUniqueId");
    r.CommInitRank = (decltype(r.CommInitRank))dlsym(r.h, "ncclCommInitRank");
    r.CommDestroy = (decltype(r.CommDestroy))dlsym(r.h, "ncclCommDestroy");
    r.AllGather = (decltype(r.AllGather))dlsym(r.h, "ncclAllGather");
    r.AllReduce = (decltype(r.AllReduce))dlsym(r.h, "ncclAllReduce");
    r.Send = (decltype(r.Send))dlsym(r.h, "ncclSend");
    r.Recv = (decltype(r.Recv))dlsym(r.h, "ncclRecv");
    r.GroupStart = (decltype(r.GroupStart))dlsym(r.h, "ncclGroupStart");
    r.GroupEnd = (decltype(r.GroupEnd))dlsym(r.h, "ncclGroupEnd");
    r.GetErrorString = (decltype(r.GetErrorString))dlsym(r.h, "ncclGetErrorString");
    r.GetVersion = (decltype(r.GetVersion))dlsym(r.h, "ncclGetVersion");
    r.CommCount = (decltype(r.CommCount))dlsym(r.h, "ncclCommCount");
    r.ok = r.GetUniqueId && r.CommInitRank && r.CommDestroy && r.AllGather && r.AllReduce && r.GetErrorString && r.Send &&
           r.Recv && r.GroupStart && r.GroupEnd;
    return r;
}

#define RCCL_TRY(expr)                                                                                     \
    do {                                                                                                   \
        ncclResult_t r_ = (expr);                                                                          \
        if (r_ != ncclSuccess) return fail(D2D_ERR_COMM, "%s failed: %s", #expr, rccl().GetErrorString(r_)); \
    } while (0)

}  // namespace

namespace {

// All collectives of a context run on its communication stream, in issue order (one communicator).  The main stream
// waits for collective `which` ([0] value-map gather, [1] gradient-map gather, [2] scene-VJP all-reduce) only where it is
// about to reuse the buffers that collective reads or writes.
int join_comm(d2d_ctx* c, int which) {
    if (c->inflight[which]) HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_done[which], 0));
    return D2D_OK;
}
int join_all_comm(d2d_ctx* c) {
    for (int w = 0; w < 3; ++w)
        if (int rc = join_comm(c, w)) return rc;
    return D2D_OK;
}
int ensure_comm_stream(d2d_ctx* c) {
    if (c->comm_stream) return D2D_OK;
    // "comm_prio" (set before the first collective): 0 default priority, 1 the highest, -1 the lowest.  The gather runs beside the
    // NEXT step's sweep, and round 4 measured that more busy hardware queues make a sweep's own workgroups start more slowly
    // ("Tried and rejected in round 4"): which priority costs the sweep least is for the first multi-GPU run
    // to measure (bench.py --comm-prio).
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    HIP_TRY(hipStreamCreateWithPriority(c->comm_stream.put(), hipStreamNonBlocking, c->comm_prio > 0 ? prio_hi : (c->comm_prio < 0 ? prio_lo : 0)));
    HIP_TRY(hipEventCreateWithFlags(c->ev_ready.put(), hipEventDisableTiming));
    for (int w = 0; w < 3; ++w) HIP_TRY(hipEventCreateWithFlags(c->ev_done[w].put(), hipEventDisableTiming));
    return D2D_OK;
}
// main stream -> communication stream hand-over: everything enqueued on the main stream so far happens before what is
// enqueued on the communication stream from now on
int comm_after_main(d2d_ctx* c) {
    HIP_TRY(hipEventRecord(c->ev_ready, c->stream));
    HIP_TRY(hipStreamWaitEvent(c->comm_stream, c->ev_ready, 0));
    return D2D_OK;
}

}  // namespace

d2d_ctx::~d2d_ctx() {
    (void)hipSetDevice(device);
    for (hipStream_t st : {(hipStream_t)aux_stream, (hipStream_t)sort_stream, (hipStream_t)stream, (hipStream_t)comm_stream, (hipStream_t)scan_stream})
        if (st) (void)hipStreamSynchronize(st);
    if (comm && rccl().ok) rccl().CommDestroy(comm);
}

extern "C" {

int d2d_abi_version(void) { return D2D_ABI_VERSION; }

const char* d2d_last_error(void) { return g_err.c_str(); }

int d2d_device_count(int* count) {
    if (!count) return fail(D2D_ERR_INVALID, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        n = 0;
    }
    *count = n;
    return D2D_OK;
}

int d2d_device_info(int device, char* name, int cap, int* cus, int64_t* mem_bytes) {
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (name && cap > 0) {
        snprintf(name, (size_t)cap, "%s (%s)", prop.name, prop.gcnArchName);
    }
    if (cus) *cus = prop.multiProcessorCount;
    if (mem_bytes) *mem_bytes = (int64_t)prop.totalGlobalMem;
    return D2D_OK;
}

int d2d_create(int device, d2d_ctx** out) {
    if (!out) return fail(D2D_ERR_INVALID, "ctx out-pointer is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return fail(D2D_ERR_NO_DEVICE, "no HIP device visible (%s); libd2d has no CPU fallback",
                    e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
    }
    if (device < 0 || device >= n) return fail(D2D_ERR_NO_DEVICE, "device %d out of range (0..%d)", device, n - 1);
    d2d_ctx* c = new d2d_ctx();
    c->device = device;
    hipError_t e1 = hipSetDevice(device);
    if (e1 == hipSuccess) {
        // The kernels are gfx950 code objects and size their LDS for a CU with 160 KB: say so HERE, in words, instead of failing a
        // launch later with a generic HIP error.
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
            if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
                delete c;
                return fail(D2D_ERR_UNSUPPORTED, "device %d is %s; libd2d is built for gfx950 (MI355X) only", device, prop.gcnArchName);
            }
            // (gfx950 / ROCm 7.2 reports sharedMemPerBlock = 163 840 and grants it without an attribute: scripts/probes/lds_limit_probe.hip,
            // profiles/r06_lds_probe.txt.  A runtime that reports less lowers the limit: D2D_ERR_UNSUPPORTED then names the object count)
            if (prop.sharedMemPerBlock >= 64 * 1024 && prop.sharedMemPerBlock < d2d_host::LDS_MAX + 4096)
                c->lds_max = prop.sharedMemPerBlock - 4096;  // (4 KB left for the kernels' static LDS)
        } else {
            (void)hipGetLastError();
        }
    }
    if (e1 == hipSuccess) e1 = hipStreamCreateWithFlags(c->stream.put(), hipStreamNonBlocking);
    for (Event* e : {&c->ev0, &c->ev1, &c->evk0, &c->evk1})
        if (e1 == hipSuccess) e1 = hipEventCreate(e->put());
    if (e1 == hipSuccess) e1 = hipEventCreateWithFlags(c->ev_meta.put(), hipEventDisableTiming);
    if (e1 == hipSuccess) {
        // the side stream carries short dependent chains that run beside a sweep kernel which fills the chip: highest priority
        int prio_lo = 0, prio_hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
        e1 = hipStreamCreateWithPriority(c->aux_stream.put(), hipStreamNonBlocking, prio_hi);
        if (e1 == hipSuccess) e1 = hipStreamCreateWithPriority(c->sort_stream.put(), hipStreamNonBlocking, prio_hi);
    }
    for (Event* e : {&c->ev_fork, &c->ev_join, &c->ev_prep})
        if (e1 == hipSuccess) e1 = hipEventCreateWithFlags(e->put(), hipEventDisableTiming | hipEventDisableSystemFence);
    c->for_each_set([&](d2d_ctx::PrepSet& sp) {
        if (e1 == hipSuccess) e1 = hipEventCreateWithFlags(sp.ev_swept.put(), hipEventDisableTiming | hipEventDisableSystemFence);
    });
    if (e1 == hipSuccess) e1 = hipHostMalloc(reinterpret_cast<void**>(c->h_meta.put()), 2 * sizeof(int), hipHostMallocDefault);
    if (e1 != hipSuccess) {
        delete c;
        return fail(D2D_ERR_HIP, "context creation failed: %s", hipGetErrorString(e1));
    }
    *out = c;
    return D2D_OK;
}

void d2d_destroy(d2d_ctx* c) {
    if (c) delete c;
}

int d2d_synchronize(d2d_ctx* c) {
    if (!c) return fail(D2D_ERR_INVALID, "ctx is NULL");
    int rc = set_device(c);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->scan_stream) HIP_TRY(hipStreamSynchronize(c->scan_stream));  // (joined by every launch that forks it; a failed launch may have left it running)
    for (int w = 0; w < 3; ++w)
        if (c->inflight[w]) {
            HIP_TRY(hipEventSynchronize(c->ev_done[w]));
            c->inflight[w] = false;
        }
    return D2D_OK;
}

int d2d_set_scene(d2d_ctx* c, const float* xys, const uint8_t* kind, const float* phi, int32_t n_objects) {
    if (!c) return fail(D2D_ERR_INVALID, "ctx is NULL");
    // validate everything before touching the context: a rejected call leaves the previous scene in place
    if (n_objects < 0 || (n_objects > 0 && !xys)) return fail(D2D_ERR_INVALID, "bad scene arguments");
    for (size_t i = 0; i < 4 * (size_t)n_objects; ++i)
        if (!(std::fabs(xys[i]) < 1e18f)) return fail(D2D_ERR_INVALID, "object coordinate %zu is not finite (or >= 1e18)", i);
    if (kind)
        for (int j = 0; j < n_objects; ++j)
            if (kind[j] > D2D_VERTEX) return fail(D2D_ERR_INVALID, "object %d has unknown kind %d", j, (int)kind[j]);
    if (phi)
        for (int j = 0; j < n_objects; ++j)
            if (!std::isfinite(phi[j])) return fail(D2D_ERR_INVALID, "phi[%d] is not finite", j);
    int rc = set_device(c);
    if (rc) return rc;
    // The scene that is resident already (a caller of the reference's API hands the objects over with every call): nothing
    // to upload, and the wall-to-wall masks and the work history stay valid.  Only the candidate mask is reset, as always.
    if (c->have_scene && c->N == n_objects && (n_objects == 0 || std::memcmp(c->xys.data(), xys, 4 * (size_t)n_objects * sizeof(float)) == 0)) {
        bool same = true;
        for (int j = 0; j < n_objects && same; ++j) {
            same = c->kind[(size_t)j] == (kind ? kind[j] : (uint8_t)D2D_WALL);
            const float ph = phi ? phi[j] : 0.78539816339744830962f;
            same = same && std::memcmp(&c->phi[(size_t)j], &ph, sizeof(float)) == 0;
        }
        if (same) {
            // what a d2d_set_scene has always meant for the results held by the context: a scene VJP summed so far (D2D_OUT_ADD)
            // is closed -- a caller who sets the scene again starts a new sum -- and the last launch's kernel time is stale
            c->have_vjp = false;
            c->vjp_reduced = false;
            c->have_kernel_time = false;
            bool all = true;
            for (int j = 0; j < n_objects; ++j) all = all && c->allowed[(size_t)j] != 0;
            if (all) return D2D_OK;
            return d2d_set_candidate_mask(c, nullptr);
        }
    }
    // from here on the old scene is gone: a failed upload leaves the context without a scene, never with half of one
    c->have_scene = false;
    c->coef.clear();              // (the reflection coefficients belong to the objects of the previous scene)
    c->cust_C = -1;               // (a host-evaluated path function's rows belong to the paths of the previous scene)
    c->have_vjp = false;          // d_vjp was sized for (and computed from) the previous scene
    c->cg.forget();               // (... and so was the frequency response's coefficient adjoint)
    c->mat.forget();              // (... and the material response, whose table has one entry per wall)
    c->eg.forget();               // (... and its permittivity adjoint)
    c->pg.forget();               // (... and the frequency response's position adjoint: its paths are the previous scene's)
    c->wg.forget();               // (... and its wall adjoint: one row per wall of the previous scene)
    c->have_kernel_time = false;
    c->for_each_set([](d2d_ctx::PrepSet& sp) { sp.cost_tiles = 0; });  // the patch-cost history describes another sweep
    c->pair_valid = false;
    c->hidden_valid = false;
    c->hidden_seen[0] = -1.0;
    c->occl_patch = NAN;
    c->N = n_objects;
    c->xys.assign(xys, xys + 4 * (size_t)n_objects);
    c->scene_absmax = 0.0f;
    for (size_t i = 0; i < 4 * (size_t)n_objects; ++i) c->scene_absmax = std::fmax(c->scene_absmax, std::fabs(xys[i]));
    c->kind.assign((size_t)n_objects, (uint8_t)D2D_WALL);
    if (kind) c->kind.assign(kind, kind + n_objects);
    c->phi.assign((size_t)n_objects, 0.78539816339744830962f);
    if (phi) c->phi.assign(phi, phi + n_objects);
    c->allowed.assign((size_t)n_objects, (uint8_t)1);
    rc = upload_refl(c);
    if (rc) return rc;
    rc = upload_mask(c);
    if (rc) return rc;
    c->have_scene = true;
    return D2D_OK;
}

int d2d_set_reflection_coefs(d2d_ctx* c, const float* coef, int32_t n) {
    if (!c) return fail(D2D_ERR_INVALID, "ctx is NULL");
    if (!c->have_scene) return fail(D2D_ERR_STATE, "d2d_set_scene must come first");
    if (!coef || n == 0) {
        if (coef || n != 0) return fail(D2D_ERR_INVALID, "d2d_set_reflection_coefs: NULL with n = 0 drops the coefficients; got %s with n = %d", coef ? "an array" : "NULL", n);
        c->coef.clear();
        return D2D_OK;
    }
    if (n != c->N) return fail(D2D_ERR_INVALID, "d2d_set_reflection_coefs: %d coefficients for a scene of %d objects", n, c->N);
    for (int j = 0; j < n; ++j)
        if (!std::isfinite(coef[j])) return fail(D2D_ERR_INVALID, "reflection coefficient %d is not finite", j);
    if ((int)c->coef.size() == n && c->d_coef.p && std::memcmp(c->coef.data(), coef, (size_t)n * sizeof(float)) == 0) return D2D_OK;  // resident already
    int rc = set_device(c);
    if (rc) return rc;
    c->coef.clear();  // (a failed upload leaves the context without coefficients, never with stale ones)
    if ((rc = c->d_coef.ensure((size_t)n + 1))) return rc;
    // (stream order: the sweeps that read the previous values are in front of this copy)
    HIP_TRY(hipMemcpyAsync(c->d_coef.p, coef, (size_t)n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->coef.assign(coef, coef + n);
    return D2D_OK;
}

int d2d_get_reflection_coefs_vjp(d2d_ctx* c, float* coef_bar) {
    if (!c || !coef_bar) return fail(D2D_ERR_INVALID, "NULL argument");
    if (!c->have_vjp) return fail(D2D_ERR_STATE, "no scene-VJP sweep has run");
    for (int j = 0; j < c->N; ++j) coef_bar[j] = 0.0f;
    if (!c->vjp_has_coef || c->N == 0) return D2D_OK;  // none of the sweeps used D2D_FUN_RECEIVED_POWER_PER_OBJECT
    int rc = set_device(c);
    if (rc) return rc;
    if ((rc = join_comm(c, 2))) return rc;  // an all-reduce of the VJP in flight lands first
    std::vector<double> h((size_t)c->N);
    HIP_TRY(hipMemcpyAsync(h.data(), c->d_vjp.p + 5 * (size_t)c->N + 2, (size_t)c->N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int j = 0; j < c->N; ++j) coef_bar[j] = (float)h[(size_t)j];
    return D2D_OK;
}

int d2d_set_candidate_mask(d2d_ctx* c, const uint8_t* allowed) {
    if (!c) return fail(D2D_ERR_INVALID, "ctx is NULL");
    if (!c->have_scene) return fail(D2D_ERR_STATE, "d2d_set_scene must come first");
    {
        bool same = (int)c->allowed.size() == c->N && c->d_cw.p != nullptr;
        for (int j = 0; j < c->N && same; ++j) same = (c->allowed[(size_t)j] != 0) == (allowed ? allowed[j] != 0 : true);
        if (same) return D2D_OK;  // the mask in place already
    }
    c->cust_C = -1;     // (... and to the candidates of the previous mask)
    c->for_each_set([](d2d_ctx::PrepSet& sp) { sp.cost_tiles = 0; });  // the patch-cost history describes another sweep
    int rc = set_device(c);
    if (rc) return rc;
    if (allowed) c->allowed.assign(allowed, allowed + c->N);
    else c->allowed.assign((size_t)c->N, (uint8_t)1);
    return upload_mask(c);
}

int d2d_count_candidates(int32_t n_objects, const uint8_t* allowed, int32_t min_order, int32_t max_order, int64_t* count) {
    std::string err;
    const int rc = d2d_host::count_candidates(n_objects, allowed, min_order, max_order, count, err);
    return rc ? fail(rc, "%s", err.c_str()) : D2D_OK;
}

int d2d_enumerate_candidates(int32_t n_objects, const uint8_t* allowed, int32_t min_order, int32_t max_order, int32_t* cand,
                             int32_t* order, int64_t capacity) {
    std::string err;
    const int rc = d2d_host::enumerate_candidates(n_objects, allowed, min_order, max_order, cand, order, capacity, err);
    return rc ? fail(rc, "%s", err.c_str()) : D2D_OK;
}

int d2d_num_candidates(d2d_ctx* c, int32_t min_order, int32_t max_order, int64_t* count) {
    if (!c || !count) return fail(D2D_ERR_INVALID, "NULL argument");
    if (!c->have_scene) return fail(D2D_ERR_STATE, "d2d_set_scene must come first");
    return d2d_count_candidates(c->N, c->allowed.data(), min_order, max_order, count);
}

int d2d_list_candidates(d2d_ctx* c, int32_t min_order, int32_t max_order, int32_t* cand, int32_t* order, int64_t capacity) {
    if (!c) return fail(D2D_ERR_INVALID, "ctx is NULL");
    if (!c->have_scene) return fail(D2D_ERR_STATE, "d2d_set_scene must come first");
    return d2d_enumerate_candidates(c->N, c->allowed.data(), min_order, max_order, cand, order, capacity);
}

// token != 0: the caller vouches that equal tokens mean equal contents (an immutable array it has passed before); 0: the
// contents are hashed.  A grid that is resident already is not uploaded again, and everything keyed to it -- the regions'
// bounding boxes, the work history behind the patch schedule -- stays valid: a caller of the reference's API, which passes
// X and Y with every call (scene.py:1803-1826, examples/plot_power_optimize.py:78-93), then runs at the resident rate.
static int set_grid_impl(d2d_ctx* c, const float* X, const float* Y, int32_t m, int32_t n, uint64_t token) {
    if (!c || !X || !Y) return fail(D2D_ERR_INVALID, "NULL argument");
    if (m <= 0 || n <= 0) return fail(D2D_ERR_INVALID, "grid must be at least 1 x 1, got %d x %d", m, n);
    int rc = set_device(c);
    if (rc) return rc;
    size_t cells = (size_t)m * (size_t)n;
    bool same = c->have_grid && c->m == m && c->n == n && c->d_X.p && c->d_Y.p && c->d_out.p;
    // a strided sample of both arrays (<= 2 x 509 words): the caller's version token says "the same immutable arrays", but an
    // owning array's flag can be flipped, written through and flipped back -- the sample catches what a token cannot
    uint64_t fp = ((uint64_t)(uint32_t)m << 32) | (uint32_t)n;
    {
        const size_t step = cells > 509 ? cells / 509 : 1;
        for (size_t i = 0; i < cells; i += step) {
            uint32_t a, b;
            std::memcpy(&a, X + i, 4);
            std::memcpy(&b, Y + i, 4);
            fp = (fp ^ (((uint64_t)a << 32) | b)) * 0x9E3779B97F4A7C15ull;
            fp ^= fp >> 29;
        }
        if (cells) {
            uint32_t a, b;
            std::memcpy(&a, X + cells - 1, 4);
            std::memcpy(&b, Y + cells - 1, 4);
            fp = (fp ^ (((uint64_t)a << 32) | b)) * 0xC2B2AE3D27D4EB4Full;
        }
    }
    if (token != 0) {
        same = same && c->grid_token == token && c->grid_fp == fp;
    } else {
        // byte for byte against the host copy of what is resident (bit patterns: -0.0 != 0.0, a NaN equals itself) -- exact,
        // and cheaper than a hash of both arrays (ADVICE / VERDICT r4: a 64-bit hash collision was a silently stale map)
        same = same && c->grid_fp == fp && c->grid_shadow.size() == 2 * cells &&
               std::memcmp(c->grid_shadow.data(), X, cells * sizeof(float)) == 0 &&
               std::memcmp(c->grid_shadow.data() + cells, Y, cells * sizeof(float)) == 0;
    }
    if (same) {
        c->grid_reuses += 1;
    } else {
        c->have_grid = false;
        c->for_each_set([](d2d_ctx::PrepSet& sp) { sp.cost_tiles = 0; });  // the patch-cost history describes another sweep
        c->grid_version += 1;  // ... and the regions' bounding boxes another grid
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->drop_records();  // ... and the records' cells
        c->drop_products(); // ... and the results of the sink kernel's products
        if ((rc = c->d_X.ensure(cells))) return rc;
        if ((rc = c->d_Y.ensure(cells))) return rc;
        if ((rc = c->d_out.ensure(cells))) return rc;
        // (sweeps of the previous grid may still be in flight on the main stream: the copies are ordered behind them)
        HIP_TRY(hipMemcpyAsync(c->d_X.p, X, cells * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->d_Y.p, Y, cells * sizeof(float), hipMemcpyHostToDevice, c->stream));
        c->grid_absmax = 0.0f;
        c->grid_all_finite = true;
        for (size_t i = 0; i < cells; ++i) {
            const float ax = std::fabs(X[i]), ay = std::fabs(Y[i]);
            c->grid_all_finite = c->grid_all_finite && (ax < 1e18f) && (ay < 1e18f);
            if (ax > c->grid_absmax) c->grid_absmax = ax;  // NaN compares false: such cells are handled by the kernel
            if (ay > c->grid_absmax) c->grid_absmax = ay;
        }
        c->grid_token = token;
        c->grid_fp = fp;
        if (token == 0) {
            try {
                c->grid_shadow.resize(2 * cells);
                std::memcpy(c->grid_shadow.data(), X, cells * sizeof(float));
                std::memcpy(c->grid_shadow.data() + cells, Y, cells * sizeof(float));
            } catch (const std::bad_alloc&) {
                std::vector<float>().swap(c->grid_shadow);  // (no copy: the next call uploads again)
            }
        } else {
            std::vector<float>().swap(c->grid_shadow);
        }
    }
    HIP_TRY(hipMemsetAsync(c->d_out.p, 0, cells * sizeof(float), c->stream));
    if (!same) HIP_TRY(hipStreamSynchronize(c->stream));  // the caller's buffers may go away
    c->m = m;
    c->n = n;
    c->have_grid = true;
    c->have_cot = false;
    c->cust_C = -1;
    c->have_vjp = false;
    c->have_grad = false;  // d_grad (if any) was sized for the previous grid
    c->gathered[0] = c->gathered[1] = 0;
    return D2D_OK;
}

int d2d_set_grid(d2d_ctx* c, const float* X, const float* Y, int32_t m, int32_t n) { return set_grid_impl(c, X, Y, m, n, 0); }

int d2d_set_grid_versioned(d2d_ctx* c, const float* X, const float* Y, int32_t m, int32_t n, uint64_t version) {
    return set_grid_impl(c, X, Y, m, n, version);
}

int d2d_debug_sweep_shape(d2d_ctx* c, int32_t* waves_per_patch, int32_t* candidates) {
    if (!c || !waves_per_patch || !candidates) return fail(D2D_ERR_INVALID, "NULL argument");
    *waves_per_patch = c->last_shape_waves;
    *candidates = c->last_shape_coop;
    return D2D_OK;
}

int d2d_debug_txg_fallbacks(d2d_ctx* c, int64_t* count) {
    if (!c || !count) return fail(D2D_ERR_INVALID, "NULL argument");
    *count = c->txg_fallbacks;
    return D2D_OK;
}

int d2d_debug_hidden_masks(d2d_ctx* c, int64_t* builds, int32_t* valid) {
    if (!c || !builds || !valid) return fail(D2D_ERR_INVALID, "NULL argument");
    *builds = c->hidden_builds;
    *valid = c->hidden_valid ? 1 : 0;
    return D2D_OK;
}

int d2d_debug_grid_reuses(d2d_ctx* c, int64_t* count) {
    if (!c || !count) return fail(D2D_ERR_INVALID, "NULL argument");
    *count = c->grid_reuses;
    return D2D_OK;
}

}  // extern "C"

namespace {

// ---- MinPath / FermatPath sweeps: opt_sweep_launch and its steps; an explicit candidate list, theta0 per candidate ---
// What the steps of one launch share: opt_sweep_launch sets the inputs, the steps the rest.
struct OptSweep {
    const d2d_params* p;
    const float* tx;
    int grad_mode;                    // 0 values; 1 + per-cell gradient; 2 + scene VJP
    int64_t C = 0;
    std::vector<int32_t> cand, order;  // [C][D2D_MAX_ORDER], [C]: by ascending order
    unsigned blocks = 0;              // 64-lane workgroups over the grid
    int n_elem = 0;                   // scene VJP row: [4N] object end points, [2] fixed end point, [N] phi
    d2d::OptSweepArgs a;
    d2d::OptGradArgs g;               // value+grad sweeps
    d2d::OptRevArgs ra;               // ... in reverse mode (option opt_grad_mode 0)
    long long chunk_cells = 0;        // reverse mode: cells per launch (the trajectory store holds that many)
};

// enumerate the candidates; check theta0 and upload both
static int opt_candidates(d2d_ctx* c, OptSweep& s) {
    const d2d_params* p = s.p;
    int rc;
    int64_t C = 0;
    if ((rc = d2d_count_candidates(c->N, c->allowed.data(), p->min_order, p->max_order, &C))) return rc;
    if (C > (1 << 22)) return fail(D2D_ERR_UNSUPPORTED, "%lld candidates are too many for an optimiser-based sweep", (long long)C);
    std::vector<int32_t>& cand = s.cand;
    std::vector<int32_t>& order = s.order;
    cand.assign((size_t)C * D2D_MAX_ORDER + 1, 0);
    order.assign((size_t)C + 1, 0);
    if ((rc = d2d_enumerate_candidates(c->N, c->allowed.data(), p->min_order, p->max_order, cand.data(), order.data(), C))) return rc;
    s.C = C;
    bool need_theta = false;
    for (int64_t i = 0; i < C; ++i)
        for (int q = 0; q < order[(size_t)i]; ++q)
            if (c->kind[cand[(size_t)i * D2D_MAX_ORDER + q]] != D2D_VERTEX) need_theta = true;
    const int64_t many = p->many > 1 ? p->many : 1;
    if (need_theta && (int64_t)c->theta0.size() != C * many * D2D_MAX_ORDER)
        return fail(D2D_ERR_STATE, "d2d_set_theta0 must provide %lld x %lld x %d initial guesses for this sweep (got %zu values)",
                    (long long)C, (long long)many, D2D_MAX_ORDER, c->theta0.size());
    std::vector<float> th((size_t)(C * many) * D2D_MAX_ORDER + 1, 0.0f);
    if ((int64_t)c->theta0.size() == C * many * D2D_MAX_ORDER) std::copy(c->theta0.begin(), c->theta0.end(), th.begin());
    if ((rc = c->d_scand.ensure(cand.size())) || (rc = c->d_sorder.ensure(order.size())) || (rc = c->d_theta0.ensure(th.size()))) return rc;
    HIP_TRY(hipMemcpyAsync(c->d_scand.p, cand.data(), cand.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_sorder.p, order.data(), order.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_theta0.p, th.data(), th.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // th goes out of scope
    return D2D_OK;
}

static int opt_args(d2d_ctx* c, OptSweep& s) {
    const d2d_params* p = s.p;
    d2d::OptSweepArgs& a = s.a;
    memset(&a, 0, sizeof a);
    a.T = obj_tables(c);
    if (int rc = opt_cfg(c, p, &a.A)) return rc;
    a.cand = c->d_scand.p;
    a.order = c->d_sorder.p;
    a.theta0 = c->d_theta0.p;
    a.C = (int)s.C;
    a.X = c->d_X.p;
    a.Y = c->d_Y.p;
    a.out = c->d_out.p;
    a.cells = (long)c->m * c->n;
    a.txx = s.tx[0];
    a.txy = s.tx[1];
    a.grid_is_tx = (p->grid_role == D2D_GRID_TX) ? 1 : 0;
    set_validity(a, p);
    for (int k = 0; k <= D2D_MAX_ORDER; ++k) a.fnum[k] = integer_pow(p->r_coef, k);
    a.h2 = p->height * p->height;
    a.fun_id = p->fun_id;
    a.out_mode = p->out_mode;
    if (p->fun_id == D2D_FUN_CUSTOM) {
        // a host-evaluated path function: rows in this enumeration's order, chained through the reverse pass over the stored
        // trajectory (the forward-tangent variant carries no seed for them)
        if (!s.grad_mode || c->opt_grad_mode != 0)
            return fail(D2D_ERR_UNSUPPORTED, "fun_id D2D_FUN_CUSTOM with an optimiser-based solver needs the reverse-mode value+grad sweep (option opt_grad_mode 0)");
        if (c->cust_C != (long long)s.C)
            return fail(D2D_ERR_STATE, "d2d_set_path_fun_values holds %lld candidates, this sweep walks %lld", c->cust_C, (long long)s.C);
        a.cust_f = c->d_cust_f.p;
        a.cust_pb = c->d_cust_pb.p;
    }
    s.blocks = (unsigned)((a.cells + 63) / 64);
    s.n_elem = 5 * c->N + 2;
    return D2D_OK;
}

// no candidate at all (order 2 in a scene of one object): the map, its gradient and the scene VJP are zero -- the
// reference's loop over no candidates (scene.py:1892-1918); found by scripts/fuzz_opt.py
static int opt_grad_zero(d2d_ctx* c, const OptSweep& s) {
    const d2d_params* p = s.p;
    int rc;
    if (p->out_mode == D2D_OUT_ADD && !c->have_grad) return fail(D2D_ERR_STATE, "D2D_OUT_ADD needs a previous value+grad sweep on this grid");
    if ((rc = c->d_grad.ensure(2 * (size_t)s.a.cells))) return rc;
    c->have_grad = true;
    HIP_TRY(d2d::launch_opt_grad_reduce(nullptr, nullptr, 0, s.a.cells, c->d_out.p, c->d_grad.p, p->out_mode, c->stream));
    if (s.grad_mode == 2) {
        if ((rc = c->d_vjp.ensure((size_t)s.n_elem))) return rc;
        if ((rc = join_comm(c, 2))) return rc;
        if (!(p->out_mode == D2D_OUT_ADD && c->have_vjp)) {
            HIP_TRY(hipMemsetAsync(c->d_vjp.p, 0, (size_t)s.n_elem * sizeof(double), c->stream));
            c->vjp_has_phi = true;
            c->vjp_has_coef = false;
            c->vjp_reduced = false;
        }
        c->have_vjp = true;
    }
    return D2D_OK;
}

// the D2D_OUT_ADD state checks; per-candidate scratch (value, per-cell gradient, VJP partial sums), reduced in candidate order
static int opt_grad_buffers(d2d_ctx* c, OptSweep& s) {
    const d2d_params* p = s.p;
    int rc;
    if (p->out_mode == D2D_OUT_ADD && !c->have_grad) return fail(D2D_ERR_STATE, "D2D_OUT_ADD needs a previous value+grad sweep on this grid");
    if (s.grad_mode == 2 && p->out_mode == D2D_OUT_ADD && c->have_vjp) {
        if (!c->vjp_has_phi)
            return fail(D2D_ERR_STATE, "D2D_OUT_ADD: the resident scene VJP comes from an ImagePath sweep; a MinPath / FermatPath sweep cannot be added to it");
        if (c->vjp_reduced)
            return fail(D2D_ERR_STATE, "D2D_OUT_ADD: the resident scene VJP has been all-reduced over ranks; fetch it, then start a new sum (D2D_OUT_OVERWRITE)");
    }
    const size_t C = (size_t)s.C, cells = (size_t)s.a.cells;
    if ((rc = c->d_contrib.ensure(C * cells))) return rc;
    if ((rc = c->d_gcontrib.ensure(2 * C * cells))) return rc;
    if ((rc = c->d_grad.ensure(2 * cells))) return rc;
    d2d::OptGradArgs& g = s.g;
    memset(&g, 0, sizeof g);
    g.s = s.a;
    g.patch = p->patch;
    g.cot = c->have_cot ? c->d_cot.p : nullptr;
    g.contrib = c->d_contrib.p;
    g.gcontrib = c->d_gcontrib.p;
    g.partial = nullptr;
    if (s.grad_mode == 2) {
        if ((rc = c->d_partial.ensure(C * s.blocks * (size_t)s.n_elem))) return rc;
        if ((rc = c->d_vjp.ensure((size_t)s.n_elem))) return rc;
        g.partial = c->d_partial.p;
        if (p->out_mode == D2D_OUT_OVERWRITE) c->have_vjp = false;
    }
    c->have_grad = true;
    return D2D_OK;
}

// reverse mode: the solver's trajectories go through HBM, in chunks of cells (d2d_host::opt_chunk_cells); when even the
// first chunk cannot be had, chunks of half the cells, down to one wave's worth, before giving up
static int opt_traj_store(d2d_ctx* c, OptSweep& s) {
    const int64_t C = s.C;
    std::vector<long long> off((size_t)C + 1, 0);
    for (int64_t i = 0; i < C; ++i) {
        int nu = 0;
        for (int q = 0; q < s.order[(size_t)i]; ++q) nu += c->kind[s.cand[(size_t)i * D2D_MAX_ORDER + q]] != D2D_VERTEX ? 1 : 0;
        off[(size_t)i + 1] = off[(size_t)i] + (long long)d2d::traj_floats_per_step(s.a.A.sgd != 0) * s.p->steps * nu;
    }
    const long long per_cell = std::max<long long>(1, off[(size_t)C]);  // floats per cell, all candidates
    size_t free_b = 0, total_b = 0;
    const bool mem_known = hipMemGetInfo(&free_b, &total_b) == hipSuccess;
    if (!mem_known) (void)hipGetLastError();
    long long& chunk_cells = s.chunk_cells;
    chunk_cells = d2d_host::opt_chunk_cells(s.a.cells, per_cell, c->opt_traj_mb, mem_known, (long long)free_b, (long long)(c->d_traj.n * sizeof(float)));
    while (c->d_traj.ensure((size_t)(chunk_cells * per_cell)) != D2D_OK) {
        (void)hipGetLastError();
        if (chunk_cells <= 64) return fail(D2D_ERR_HIP, "the solver's trajectory store does not fit the device even for 64 cells (%lld floats per cell)", per_cell);
        chunk_cells = std::max<long long>(64, chunk_cells / 2 / 64 * 64);
    }
    int rc;
    if ((rc = c->d_traj_off.ensure((size_t)C + 1))) return rc;
    HIP_TRY(hipMemcpyAsync(c->d_traj_off.p, off.data(), ((size_t)C + 1) * sizeof(long long), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // (the host vector goes out of scope)
    d2d::OptRevArgs& ra = s.ra;
    memset(&ra, 0, sizeof ra);
    ra.g = s.g;
    ra.traj = c->d_traj.p;
    ra.traj_off = c->d_traj_off.p;
    ra.total_blocks = s.blocks;
    return D2D_OK;
}

// the value+grad kernels (reverse mode: chunk x order launches), then the reduction of values and per-cell gradients
static int opt_grad_launch(d2d_ctx* c, OptSweep& s) {
    const size_t lds = (size_t)s.n_elem * sizeof(float);
    if (c->time_kernel) HIP_TRY(hipEventRecord(c->evk0, c->stream));
    if (c->opt_grad_mode == 0) {
        d2d::OptRevArgs& ra = s.ra;
        for (long long cell0 = 0; cell0 < (long long)s.a.cells; cell0 += s.chunk_cells) {
            ra.cell0 = (long)cell0;
            ra.chunk_cells = (long)std::min<long long>(s.chunk_cells, (long long)s.a.cells - cell0);
            ra.stride = (long)((ra.chunk_cells + 63) / 64 * 64);
            for (int64_t c0 = 0; c0 < s.C;) {  // one launch per order: a contiguous range of the enumeration
                int64_t c1 = c0 + 1;
                while (c1 < s.C && s.order[(size_t)c1] == s.order[(size_t)c0]) ++c1;
                HIP_TRY(d2d::launch_opt_rev(s.order[(size_t)c0], ra, (int)c0, dim3((unsigned)(ra.stride / 64), (unsigned)(c1 - c0)), lds, c->stream));
                c0 = c1;
            }
        }
    } else {
        HIP_TRY(d2d::launch_opt_grad(s.g, dim3(s.blocks, (unsigned)s.C), lds, c->stream));
    }
    if (c->time_kernel) {
        HIP_TRY(hipEventRecord(c->evk1, c->stream));
        c->have_kernel_time = true;
    }
    HIP_TRY(d2d::launch_opt_grad_reduce(c->d_contrib.p, c->d_gcontrib.p, (int)s.C, s.a.cells, c->d_out.p, c->d_grad.p, s.p->out_mode, c->stream));
    return D2D_OK;
}

// the scene VJP: the workgroups' partial sums, reduced in a fixed order
static int opt_vjp_reduce(d2d_ctx* c, const OptSweep& s) {
    if (int rc = join_comm(c, 2)) return rc;  // the previous step's all-reduce has finished with d_vjp
    // a VJP accumulated over several transmitters (D2D_OUT_ADD) must come from sweeps of one kind (the image-method
    // sweeps have no phi part) and must still be this rank's own partial sum
    const int accumulate = (s.p->out_mode == D2D_OUT_ADD && c->have_vjp) ? 1 : 0;
    c->vjp_reduced = false;
    hipLaunchKernelGGL(d2d::vjp_reduce_kernel, dim3((unsigned)s.n_elem), dim3(256), 0, c->stream, c->d_partial.p, (long)((size_t)s.C * s.blocks),
                       s.n_elem, c->d_vjp.p, accumulate);
    HIP_TRY(hipGetLastError());
    c->have_vjp = true;
    c->vjp_has_phi = true;
    c->vjp_has_coef = false;  // (the optimiser-based sweeps refuse the per-object function)
    return D2D_OK;
}

// values only: the candidates side by side while the contributions fit a modest scratch buffer (and the grid's y dimension)
static int opt_value_launch(d2d_ctx* c, const OptSweep& s) {
    const d2d::OptSweepArgs& a = s.a;
    const int64_t C = s.C;
    const bool side_by_side = c->opt_parallel && C >= 2 && C <= 65535 && (long long)C * a.cells <= (1ll << 26);
    if (!side_by_side) {
        HIP_TRY(d2d::launch_opt(a, dim3(s.blocks), nullptr, c->stream));
        return D2D_OK;
    }
    if (int rc = c->d_contrib.ensure((size_t)C * (size_t)a.cells)) return rc;
    HIP_TRY(d2d::launch_opt(a, dim3(s.blocks, (unsigned)C), c->d_contrib.p, c->stream));
    hipLaunchKernelGGL(d2d::opt_reduce_kernel, dim3((unsigned)((a.cells + 255) / 256)), dim3(256), 0, c->stream, c->d_contrib.p, (int)C, a.cells,
                       c->d_out.p, s.p->out_mode);
    HIP_TRY(hipGetLastError());
    return D2D_OK;
}

static int opt_sweep_launch(d2d_ctx* c, const d2d_params* p, const float* tx, int grad_mode) {
    OptSweep s;
    s.p = p;
    s.tx = tx;
    s.grad_mode = grad_mode;
    int rc;
    if ((rc = set_device(c)) || (rc = upload_occl(c, p->patch)) || (rc = opt_candidates(c, s)) || (rc = opt_args(c, s))) return rc;
    if (!grad_mode) return opt_value_launch(c, s);
    if (s.C > 65535 || (long long)s.C * s.a.cells > (1ll << 28))
        return fail(D2D_ERR_UNSUPPORTED, "%lld candidates x %lld cells exceed the gradient sweep's scratch (2^28 contributions)",
                    (long long)s.C, (long long)s.a.cells);
    if (s.C == 0) return opt_grad_zero(c, s);
    if ((rc = opt_grad_buffers(c, s))) return rc;
    if (c->opt_grad_mode == 0 && (rc = opt_traj_store(c, s))) return rc;
    if ((rc = opt_grad_launch(c, s))) return rc;
    return grad_mode == 2 ? opt_vjp_reduce(c, s) : D2D_OK;
}

// ---- ImagePath sweeps: sweep_launch and its steps ------------------------------------------------------------------
// What the steps of one launch share.  The constructor sets the inputs; take_prep_set (or prep_sink_sweep) and sweep_args the rest.
struct Sweep {
    const d2d_params* p;
    const float* tx;
    unsigned long long* d_stats;  // instrumented build (d2d_power_map_stats): its counters
    int grad_mode;                // 0 values, 1 value+grad, 2 ... and the scene VJP
    int tiles_x, tiles_y;
    long long tiles;
    Sweep(const d2d_ctx* c, const d2d_params* p, const float* tx, unsigned long long* d_stats = nullptr, int grad_mode = 0)
        : p(p), tx(tx), d_stats(d_stats), grad_mode(grad_mode), tiles_x((c->n + d2d::TILE_W - 1) / d2d::TILE_W),
          tiles_y((c->m + d2d::TILE_H - 1) / d2d::TILE_H), tiles((long long)tiles_x * tiles_y) {}
    bool piped = false;           // the preparation runs on aux_stream into a rotated set
    bool set_was_swept = false;   // the set this launch takes was read by a sweep that may still be running (its ev_swept says when)
    hipStream_t ps = nullptr;     // where this launch's preparation runs
    d2d_host::SweepThresholds th;
    bool txg = false, txg_culled = false;
    bool txg_fallback = false;    // a TX-grid sweep that would be culled if a degenerate path could not count: whoever runs it exhaustively counts it
    dim3 grid_patches;            // one single-wave workgroup per 8 x 8 patch
    d2d::SweepArgs a;
};
// The window of the shadow masks (certainly hit, parametric bins); the hidden masks reuse it.
struct MaskWindow {
    bool ok = false;
    double in_lo = 0.0, in_hi = 0.0, dom_lo = 0.0, dom_w = 0.0;
};
// What the preparation steps found out.
struct Prep {
    bool zeroed = false;              // d_shadow's counters and list meta were zeroed with the shadow masks
    MaskWindow win;
    bool queue_impossible = false;    // no patch can be left to the enumerating kernel (the queue walker is not launched)
    bool sched_from_history = false;  // the schedule's keys are measured (work history or list lengths), not the proxy
};

// a host-evaluated path function (d2d_set_path_fun_values): the exhaustive value+grad kernel walks every candidate in the
// reference's order, which is the order the host's rows come in
static int custom_fun_params(d2d_ctx* c, const d2d_params* p, d2d_params* out) {
    long long want = 0;
    for (int k = p->min_order; k <= p->max_order; ++k) {
        long long ck = 1;
        for (int i = 0; i < k; ++i) ck *= (i == 0) ? (long long)c->cw.size() : (long long)c->cw.size() - 1;
        want += ck;
    }
    if (c->cust_C != want)
        return fail(D2D_ERR_STATE, "d2d_set_path_fun_values holds %lld candidates, this sweep walks %lld", c->cust_C, want);
    *out = *p;
    out->strict_nan = 1;
    return D2D_OK;
}

// what an ImagePath sweep refuses from its arguments alone
static int check_image_sweep(d2d_ctx* c, const d2d_params* p, const unsigned long long* d_stats) {
    if (p->solver != D2D_SOLVER_IMAGE) return fail(D2D_ERR_INVALID, "unknown solver %d", p->solver);
    if (p->max_order >= 1)
        for (int j = 0; j < c->N; ++j)
            if (c->allowed[j] && c->kind[j] != D2D_WALL)
                return fail(D2D_ERR_UNSUPPORTED,
                            "ImagePath needs homogeneous Wall objects (reference: stack_leaves raises on mixed types); "
                            "object %d has kind %d", j, (int)c->kind[j]);
    for (int j = 0; j < c->N; ++j)
        if (c->kind[j] == D2D_VERTEX) return fail(D2D_ERR_UNSUPPORTED, "Vertex objects need the MinPath/FermatPath solver");
    if (p->grid_role == D2D_GRID_TX && d_stats) return fail(D2D_ERR_UNSUPPORTED, "the instrumented build covers the RX-grid kernel only");
    return D2D_OK;
}

// Pipelined preparation (see d2d_ctx::PrepSet): this launch takes the set the launch before the previous one used,
// and builds into it on the side stream, which first waits for the sweep that read it last.
// (instrumented launches prepare on the main stream: their counters are zeroed there, and the list kernels add to them)
// (a lone call has no previous sweep to hide its preparation behind; preparing on the sweep stream whenever that stream is idle
// was measured: launch -> synchronise 0.146 -> 0.137 ms at 300^2, but back-to-back launches whose host runs ahead of the GPU
// only now and then lose 4-8 %: not kept)
// Small launches without region lists ("unpiped_max_tiles", orders <= 1): a grid of a few patches is all launch latency; its one
// preparation kernel (the shadow masks) takes microseconds and gains nothing from running beside a previous sweep, while the fork
// to the side stream and the join back cost two cross-stream events per launch.  They prepare on the sweep's own stream: the
// reference's own benchmark workload (basic_scene, scene.grid(n <= 50), orders 0..1) 45 -> 37.5 us launch -> synchronise, back-to-back
// launches unchanged at 24 us (scripts/small_launch_ab.py).  With lists (orders >= 2) a lone call gains the same 8 us but
// back-to-back launches lose 30 - 40 us (71 -> 104 us at 128^2): those stay pipelined.  A context that changes kind drains its
// streams once, like the "pipeline" option does.
static int take_prep_set(d2d_ctx* c, Sweep& s) {
    const bool small = c->pipeline && s.p->max_order <= 1 && s.tiles <= c->unpiped_max_tiles;
    if (small != c->last_small) {
        if (c->stream) HIP_TRY(hipStreamSynchronize(c->stream));
        if (c->aux_stream) HIP_TRY(hipStreamSynchronize(c->aux_stream));
        if (c->sort_stream) HIP_TRY(hipStreamSynchronize(c->sort_stream));
        c->for_each_set([](d2d_ctx::PrepSet& sp) { sp.swept_pending = false; });
        c->last_small = small;
    }
    s.piped = c->pipeline && c->aux_stream != nullptr && s.d_stats == nullptr && !small;
    if (s.piped) {
        // rotate: the oldest set becomes the current one, the current one the newest spare
        std::swap(c->cur, c->spare_sets[0]);
        for (int i = 0; i + 1 < d2d_ctx::N_SPARE; ++i) std::swap(c->spare_sets[i], c->spare_sets[i + 1]);
        s.set_was_swept = c->cur.swept_pending;
        if (c->cur.swept_pending) HIP_TRY(hipStreamWaitEvent(c->aux_stream, c->cur.ev_swept, 0));
        c->cur.swept_pending = false;
    }
    s.ps = s.piped ? c->aux_stream : c->stream;
    return D2D_OK;
}

// the scalar SweepArgs: buffers of the scene and the grid, parameters, thresholds
static int sweep_args(d2d_ctx* c, Sweep& s) {
    const d2d_params* p = s.p;
    d2d::SweepArgs& a = s.a;
    memset(&a, 0, sizeof a);
    a.occl = c->d_occl.p;
    a.refl = c->d_refl.p;
    a.flt = c->d_flt.p;
    a.cw = c->d_cw.p;
    a.N = c->N;
    a.Nc = (int)c->cw.size();
    a.X = c->d_X.p;
    a.Y = c->d_Y.p;
    a.out = c->d_out.p;
    a.m = c->m;
    a.n = c->n;
    a.tiles_x_div = d2d::make_div((uint32_t)s.tiles_x);
    a.txx = s.tx[0];
    a.txy = s.tx[1];
    a.min_order = p->min_order;
    a.max_order = p->max_order;
    a.alpha = p->alpha;
    a.tol = p->tol;
    a.seg_lo = -p->seg_tol;
    a.seg_hi = 1.0f + p->seg_tol;
    const bool per_object = p->fun_id == D2D_FUN_RECEIVED_POWER_PER_OBJECT;
    s.th = d2d_host::sweep_thresholds(*p, s.grad_mode != 0, per_object ? c->coef.data() : nullptr, c->allowed.data(), c->N);
    a.coef = per_object ? c->d_coef.p : nullptr;
    a.flt_lo = s.th.flt_lo;
    a.flt_hi = s.th.flt_hi;
    a.on_lo = s.th.on_lo;
    a.on_hi = s.th.on_hi;
    a.loss_skip = s.th.loss_skip;
    for (int k = 0; k <= D2D_MAX_ORDER; ++k) a.fnum[k] = s.th.fnum[k];
    a.h2 = s.th.h2;
    a.sig_l2f = s.th.sig_l2f;
    a.sig_mono = s.th.sig_mono;
    a.fun_id = p->fun_id;
    a.cust_f = c->d_cust_f.p;
    a.cust_pb = c->d_cust_pb.p;
    a.cust_cells = (long)c->m * c->n;
    a.out_mode = p->out_mode;
    a.patch = p->patch;
    a.stats = s.d_stats;
    a.wave_cycles = (s.d_stats && c->want_wave_cycles) ? s.d_stats + D2D_NUM_STATS : nullptr;
    if (s.tiles > 0x7fffffffLL) return fail(D2D_ERR_INVALID, "grid too large: %lld tiles", s.tiles);
    s.grid_patches = dim3((unsigned)s.tiles);
    s.txg = p->grid_role == D2D_GRID_TX;
    // TX grid: culled kernels -- unless a degenerate path can count.  Their culling walks the chain from the FIXED end (images of
    // the receiver, first the wall next to the cell), which is the exact chain's LAST step: where an earlier exact step hits
    // un == 0 the exact points are not the geometric ones the culling reasons about (RX grids cull along the exact chain's own
    // order and stop at its poles).  Found by scripts/fuzz_parity.py (seed 4003, case 1295: sigmoid, alpha = 10, tol = 0.5 --
    // a zero-length segment still leaves sigmoid(-5) -- walls on a lattice); tests/test_gpu_forward.py keeps the case.
    const bool txg_cullable = s.txg && !c->txg_exhaustive && !(s.grad_mode && p->strict_nan);
    s.txg_culled = txg_cullable && s.th.degenerate_invalid;
    s.txg_fallback = txg_cullable && !s.th.degenerate_invalid;
    return D2D_OK;
}

// (a sweep that reads the old masks may still be in flight on the main stream)
static int wait_spare_sweeps(d2d_ctx* c, hipStream_t st) {
    for (d2d_ctx::PrepSet& sp : c->spare_sets)
        if (sp.swept_pending) HIP_TRY(hipStreamWaitEvent(st, sp.ev_swept, 0));
    return D2D_OK;
}

// wall-to-wall masks for the segments between two interaction points (orders >= 2): no end point involved,
// so they depend on the scene and the validity mode only and are kept until one of those changes
static int prep_pair_masks(d2d_ctx* c, Sweep& s, const MaskWindow& w, float ext) {
    const d2d_params* p = s.p;
    d2d::SweepArgs& a = s.a;
    int rc;
    bool pair_ext_ok = false;
    if (p->max_order >= 2 && c->N >= 3 && c->N <= 256 && c->use_pair_masks && std::isfinite(c->scene_absmax) && c->scene_absmax > 0.0f) {
        const float pdperp = 4096.0f * 1.1920929e-07f * c->scene_absmax * (float)(D2D_MAX_ORDER + 1);
        const float key[6] = {p->patch, p->seg_tol, (float)p->approx, (float)p->act, p->alpha, pdperp};
        if (!c->pair_valid || std::memcmp(key, c->pair_key, sizeof(key)) != 0) {
            const size_t n2 = (size_t)c->N * c->N;
            if ((rc = c->d_pair.ensure(n2))) return rc;
            if (s.piped && (rc = wait_spare_sweeps(c, s.ps))) return rc;
            HIP_TRY(hipMemsetAsync(c->d_pair.p, 0, n2 * sizeof(unsigned long long), s.ps));
            const long long waves = (long long)c->N * c->N * c->N;
            hipLaunchKernelGGL(d2d::pair_shadow_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s.ps, c->d_occl.p,
                               c->d_refl.p, c->d_kind.p, c->N, (float)(w.in_lo + 1e-4), (float)(w.in_hi - 1e-4), pdperp,
                               (float)w.dom_lo, (float)(w.dom_w * 8.0), c->d_pair.p);
            HIP_TRY(hipGetLastError());
            std::memcpy(c->pair_key, key, sizeof(key));
            c->pair_valid = true;
        }
        a.pair = c->d_pair.p;
        a.pair_dperp = pdperp;
        pair_ext_ok = ext <= 8.0f * c->scene_absmax;  // interaction points of a valid path stay within pdperp of their walls
    }
    // a candidate with un == 0 in some step has a zero-length segment, loss >= 1: is it exactly invalid?
    a.shadow_prefix_ok = s.th.degenerate_invalid ? 1 : 0;
    a.pair_prefix_ok = (a.pair && pair_ext_ok && a.shadow_prefix_ok) ? 1 : 0;
    return D2D_OK;
}

// first-segment shadow coverage (RX grids: the fixed end point is the transmitter) and the pair masks
// (`own`: a record launch's masks go to a buffer of its own -- nothing behind them to zero, no fork event -- so that the
// rotating sets stay what the sweeps left)
static int prep_masks(d2d_ctx* c, Sweep& s, Prep& pr, DevBuf<unsigned long long>* own = nullptr) {
    const d2d_params* p = s.p;
    d2d::SweepArgs& a = s.a;
    int rc;
    if (!((!s.txg || s.txg_culled) && c->N >= 2 && p->max_order >= 1)) return D2D_OK;
    DevBuf<unsigned long long>& buf = own ? *own : c->cur.d_shadow;
    // [N] masks, then the {histogram, cursors} of the patch schedule's counting sort, then what the region lists need
    // zeroed per launch ({queue length, pool head}, one flag per leaf region): one memset for all of it
    const size_t rl_regions = (size_t)((s.tiles_x + c->region_size - 1) / c->region_size) * (size_t)((s.tiles_y + c->region_size - 1) / c->region_size);
    // (a multiple of 256 bytes: the runtime fills odd tails with a second kernel)
    const size_t zero_words = own ? (size_t)c->N : ((size_t)c->N + d2d::SCHED_KEYS + (2 + rl_regions + 1) / 2 + 31) & ~(size_t)31;
    if ((rc = buf.ensure(zero_words))) return rc;
    pr.zeroed = !own;
    // window where a test is certainly "hit" (hard) / exactly saturated to 1 (approx): shrink [-tol, 1+tol] by widen
    MaskWindow& w = pr.win;
    w.in_lo = -(double)p->seg_tol + s.th.widen_in;
    w.in_hi = 1.0 + (double)p->seg_tol - s.th.widen_in;
    const float ext = std::fmax(std::fmax(c->scene_absmax, c->grid_absmax), std::fmax(std::fabs(s.tx[0]), std::fabs(s.tx[1])));
    w.ok = w.in_hi > w.in_lo + 1e-3 && std::isfinite(ext) && ext > 0.0f;
    // bins span the parametric window in which on_objects is not exactly 0 (+ a little)
    w.dom_lo = (double)a.on_lo - 2e-3;
    const double dom_hi = (double)a.on_hi + 2e-3;
    w.dom_w = (dom_hi - w.dom_lo) / 64.0;
    const float dperp = 4096.0f * 1.1920929e-07f * (w.ok ? ext : 1.0f) * (float)(p->max_order + 1);
    // one kernel: the masks (stored, not OR-ed: nothing to zero in front) and the zeroing of everything behind them
    const long n_zero = (long)zero_words - c->N;
    hipLaunchKernelGGL(d2d::shadow_fill_kernel, dim3((unsigned)(c->N + (n_zero + 255) / 256)), dim3(256), 0, s.ps, c->d_occl.p, c->d_refl.p,
                       c->d_kind.p, c->N, s.tx[0], s.tx[1], (float)(w.in_lo + 1e-4), (float)(w.in_hi - 1e-4), dperp, (float)w.dom_lo,
                       (float)w.dom_w, w.ok ? 1 : 0, buf.p, buf.p + c->N, n_zero);
    HIP_TRY(hipGetLastError());
    if (!own) HIP_TRY(hipEventRecord(c->ev_fork, s.ps));  // (the sort of a big launch needs its counters zeroed: it may start here)
    if (!w.ok) return D2D_OK;
    a.shadow = buf.p;
    a.shadow_dperp = dperp;
    a.shadow_lo = (float)w.dom_lo;
    a.shadow_inv = (float)(1.0 / w.dom_w);
    return prep_pair_masks(c, s, w, ext);
}

// last-segment masks: which bins of which wall are hidden from a whole leaf region (forward RX-grid sweeps)
// (launches of a few hundred patches are latency-bound: one more dependent load per culling step costs them more than
// the masks save -- 64^2 cells: 0.085 -> 0.097 ms with them, 128^2 0.072 -> 0.076, 200^2 equal, 300^2 0.091 -> 0.086)
static int prep_hidden_masks(d2d_ctx* c, Sweep& s, const Prep& pr, const d2d_host::RegionPlan& rp, d2d::RegionLevel& leaf) {
    const d2d_params* p = s.p;
    const MaskWindow& w = pr.win;
    int rc;
    if (!(w.ok && s.a.shadow && c->use_hidden_masks && s.tiles >= c->hidden_min_tiles && std::isfinite(c->scene_absmax) &&
          std::isfinite(c->grid_absmax) && (size_t)rp.leaf.regions * (size_t)c->N <= ((size_t)1 << 28)))
        return D2D_OK;
    const float hdperp = 4096.0f * 1.1920929e-07f * std::fmax(c->scene_absmax, c->grid_absmax) * (float)(D2D_MAX_ORDER + 1);
    const double key[12] = {(double)c->grid_version, (double)rp.leaf.R, (double)c->m, (double)c->n, (double)p->patch, (double)p->seg_tol,
                            (double)(p->approx * 4 + p->act + (s.txg ? 16 : 0)), (double)p->alpha, (double)hdperp, w.dom_lo, w.dom_w, (double)c->N};
    if (hdperp > 0.0f && !(c->hidden_valid && std::memcmp(key, c->hidden_key, sizeof key) == 0)) {
        if (std::memcmp(key, c->hidden_seen, sizeof key) == 0) {  // the second launch in a row with this key: build
            const size_t nh = (size_t)rp.leaf.regions * (size_t)c->N;
            if ((rc = c->d_hidden.ensure(nh))) return rc;
            if (s.piped && (rc = wait_spare_sweeps(c, s.ps))) return rc;
            hipLaunchKernelGGL(d2d::hidden_region_kernel, dim3((unsigned)nh), dim3(64), 0, s.ps, c->d_occl.p, c->d_refl.p, c->d_kind.p, c->N,
                               c->d_rl_box.p, (float)(w.in_lo + 1e-4), (float)(w.in_hi - 1e-4), hdperp, (float)w.dom_lo, (float)w.dom_w,
                               c->d_hidden.p, s.txg ? 1 : 0);
            HIP_TRY(hipGetLastError());
            std::memcpy(c->hidden_key, key, sizeof key);
            c->hidden_valid = true;
            c->hidden_builds += 1;
        } else {
            std::memcpy(c->hidden_seen, key, sizeof key);
            c->hidden_valid = false;
        }
    }
    if (c->hidden_valid && std::memcmp(key, c->hidden_key, sizeof key) == 0) {
        leaf.hidden = c->d_hidden.p;
        leaf.hidden_dperp = hdperp;
    }
    return D2D_OK;
}

// region candidate lists (orders >= 2): the culled RX-grid kernels (forward, instrumented, value+grad) read them
static int prep_region_lists(d2d_ctx* c, Sweep& s, Prep& pr) {
    const d2d_params* p = s.p;
    d2d::SweepArgs& a = s.a;
    d2d_ctx::PrepSet& cur = c->cur;
    int rc;
    if (!((!s.txg || s.txg_culled) && c->use_region_lists && p->max_order >= 2 && c->cw.size() >= 2 && c->N <= 4095 &&
          !(s.grad_mode && p->strict_nan)))
        return D2D_OK;
    // "region_budget_mb" bounds the device memory of ALL list pools: the pipeline keeps one per rotating set
    const long long pool_cap_mb = std::max<long long>(1, c->region_budget_mb / (s.piped ? 1 + d2d_ctx::N_SPARE : 1));
    // how the previous launch's lists fared (read back without waiting: a launch or two late is early enough)
    if (c->meta_pending && hipEventQuery(c->ev_meta) == hipSuccess) {
        c->meta_pending = false;
        c->fb_hint = c->h_meta[0];
        if ((long long)c->h_meta[1] + c->pend_static > c->pend_chunks && c->rl_pool_mb < pool_cap_mb)
            c->rl_pool_mb = std::min(pool_cap_mb, c->rl_pool_mb * 4);  // the pool ran out: a bigger one from now on
    }
    // third-order lists over a big scene start with 1 GB per set: configs[3]'s hard_sigmoid lists are 577 MB, and the ONE launch
    // that finds a 256 MB pool too small takes 8.7 s instead of 0.04 (its patches enumerate) -- 288 GB of HBM are there to be used
    if (!c->rl_pool_by_option && p->max_order >= 3 && c->cw.size() >= 64 && c->rl_pool_mb < 1024) c->rl_pool_mb = 1024;
    if (c->rl_pool_mb > pool_cap_mb) c->rl_pool_mb = pool_cap_mb;
    d2d_host::RegionPlan rp =
        d2d_host::region_plan(s.tiles_x, s.tiles_y, (long long)c->cw.size(), p->min_order, p->max_order, (int)c->region_size,
                              (int)c->region_size_top, (int)c->region_slices, c->rl_pool_mb << 20, d2d::RL_CHUNK);
    const size_t lds_l = (size_t)(3 * c->N + 1) * sizeof(float4) + 512;                                         // tables + culling queue
    const size_t lds_r = (size_t)(3 * c->N + 1) * sizeof(float4) + (size_t)d2d::RL_GATHER * sizeof(unsigned long long);  // tables + gather buffer
    if (!rp.on || lds_l > d2d_host::LDS_LIMIT || lds_r > d2d_host::LDS_LIMIT) return D2D_OK;
    // the pool is the one big allocation of the library: when the device cannot give it, this launch enumerates
    // (same results) and later launches ask for a quarter
    if (cur.d_rl_pool.ensure((size_t)rp.max_chunks * d2d::RL_CHUNK) != D2D_OK || cur.d_rl_next.ensure((size_t)rp.max_chunks) != D2D_OK) {
        (void)hipGetLastError();
        cur.d_rl_pool.release();
        cur.d_rl_next.release();
        c->rl_pool_mb = std::max<long long>(1, c->rl_pool_mb / 4);
        return D2D_OK;
    }
    const int orders = p->max_order - rp.k_lo + 1;
    const size_t per_order = (size_t)rp.leaf.slots + (size_t)rp.top.slots;
    if ((rc = cur.d_rl_idx.ensure(per_order * (size_t)orders))) return rc;
    // meta (zeroed with the shadow masks above): [0] queue length, [1] pool head, [2 ..) leaf region flags
    int* const meta = reinterpret_cast<int*>(cur.d_shadow.p + c->N + d2d::SCHED_KEYS);
    cur.rl_meta_ptr = meta;
    if ((rc = cur.d_rl_meta.ensure((size_t)s.tiles))) return rc;  // the queue of patches left to the enumerating kernel
    if ((rc = cur.d_rl.ensure(1))) return rc;
    {
        // the regions' bounding boxes depend on the grid only
        const long long key[4] = {c->grid_version, rp.leaf.R, rp.top.R, (long long)c->m * 0x100000000ll + c->n};
        const size_t nbox = (size_t)rp.leaf.regions + (size_t)rp.top.regions;
        if (std::memcmp(key, c->rl_box_key, sizeof key) != 0 || c->d_rl_box.n < nbox) {
            if ((rc = c->d_rl_box.ensure(nbox))) return rc;
            hipLaunchKernelGGL(d2d::region_box_kernel, dim3((unsigned)rp.leaf.regions), dim3(256), 0, s.ps, c->d_X.p, c->d_Y.p,
                               c->m, c->n, rp.leaf.R, rp.leaf.regions_x, c->d_rl_box.p);
            hipLaunchKernelGGL(d2d::region_box_kernel, dim3((unsigned)rp.top.regions), dim3(256), 0, s.ps, c->d_X.p, c->d_Y.p,
                               c->m, c->n, rp.top.R, rp.top.regions_x, c->d_rl_box.p + rp.leaf.regions);
            HIP_TRY(hipGetLastError());
            std::memcpy(c->rl_box_key, key, sizeof key);
        }
    }
    auto fill = [](d2d::RegionLevel& l, const d2d_host::RegionLevelPlan& lp_) {
        l.S = lp_.S;
        l.R = lp_.R;
        l.R_div = d2d::make_div((uint32_t)lp_.R);
        l.regions_x = lp_.regions_x;
        l.regions_y = lp_.regions_y;
    };
    d2d::RegionLists rl;
    d2d::RegionLevel top;
    memset(&rl, 0, sizeof rl);
    memset(&top, 0, sizeof top);
    fill(rl.leaf, rp.leaf);
    fill(top, rp.top);
    rl.leaf.box = c->d_rl_box.p;
    top.box = c->d_rl_box.p + rp.leaf.regions;
    if ((rc = prep_hidden_masks(c, s, pr, rp, rl.leaf))) return rc;
    int* at = cur.d_rl_idx.p;
    int chunk_at = 0;
    for (int k = rp.k_lo; k <= p->max_order; ++k) {
        rl.leaf.cnt[k] = at; at += rp.leaf.slots;
        rl.leaf.chunk0[k] = chunk_at; chunk_at += (int)rp.leaf.slots;
        top.cnt[k] = at; at += rp.top.slots;
        top.chunk0[k] = chunk_at; chunk_at += (int)rp.top.slots;
    }
    rl.lp.pool = cur.d_rl_pool.p;
    rl.lp.next = cur.d_rl_next.p;
    rl.lp.head = meta + 1;
    rl.lp.n_static = (int)rp.n_static;
    rl.lp.max_chunks = (int)rp.max_chunks;
    rl.flag = meta + 2;
    a.fb_n = meta;
    a.fb_list = cur.d_rl_meta.p;
    if (!cur.rl_host_valid || std::memcmp(&rl, &cur.rl_host, sizeof rl) != 0) {
        // written by a kernel that takes the descriptor by value: stream-ordered, and nothing reads host memory
        // after this call returns (a copy from a pageable member would be staged synchronously and drain `ps`)
        cur.rl_host = rl;
        cur.rl_host_valid = true;
        hipLaunchKernelGGL(d2d::write_region_lists_kernel, dim3(1), dim3(1), 0, s.ps, cur.d_rl.p, rl);
        HIP_TRY(hipGetLastError());
    }
    d2d::SweepArgs al = a;
    al.fb_n = nullptr;
    al.cullq_off = (int)((size_t)(3 * c->N + 1) * sizeof(float4));
    for (int k = rp.k_lo; k <= p->max_order; ++k) {
        HIP_TRY(d2d::launch_region_lists(k, s.txg, dim3((unsigned)rp.top.slots), lds_l, s.ps, al, top, rl.lp));
        HIP_TRY(d2d::launch_region_refine(k, s.txg, dim3((unsigned)rp.leaf.regions), lds_r, s.ps, al, rl.leaf, top, rl.lp, rl.flag));
    }
    a.rl = cur.d_rl.p;
    c->rl_plan = rp;
    c->rl_max_order = p->max_order;
    // (the lists' lengths follow the validity parameters as much as the plan: a context that goes from hard to hard_sigmoid
    // validity on the same grid -- bench.py's configs[3] legs -- must look at its first launches again: without this the
    // overflow of the hard_sigmoid lists was noticed sixteen launches late, each of them seconds long)
    const float vkey[6] = {(float)s.th.mode, p->alpha, p->tol, p->patch, p->seg_tol, (float)(p->min_order * 16 + p->max_order)};
    const bool same_params = std::memcmp(vkey, c->rl_vkey, sizeof vkey) == 0;
    std::memcpy(c->rl_vkey, vkey, sizeof vkey);
    c->rl_launches = (same_params && c->rl_meta_static == rp.n_static && c->rl_meta_chunks == rp.max_chunks) ? c->rl_launches + 1 : 1;
    c->rl_meta_static = rp.n_static;
    c->rl_meta_chunks = rp.max_chunks;
    // Can a patch be left to the enumerating kernel at all?  Only a cell or end point that is not comfortably
    // finite or a list that does not fit can do that; if even "every candidate survives everywhere" fits the
    // pool, the queue stays empty and the launch that would walk it is not made.
    double worst = 0.0;  // entries of all lists of one region
    for (int k = rp.k_lo; k <= p->max_order; ++k) worst += (double)c->cw.size() * std::pow((double)c->cw.size() - 1.0, k - 1);
    const double worst_chunks = worst * (double)(rp.leaf.regions + rp.top.regions) / d2d::RL_CHUNK + 2.0 * (double)rp.n_static;
    pr.queue_impossible = c->grid_all_finite && std::fabs(s.tx[0]) < 1e18f && std::fabs(s.tx[1]) < 1e18f &&
                          worst_chunks < (double)rp.max_chunks;
    return D2D_OK;
}

// dearest-first patch schedule for the culled kernels; then which work history the sweep writes
static int prep_schedule(d2d_ctx* c, Sweep& s, Prep& pr) {
    const d2d_params* p = s.p;
    d2d::SweepArgs& a = s.a;
    d2d_ctx::PrepSet& cur = c->cur;
    const long long tiles = s.tiles;
    int rc;
    if ((!s.txg || s.txg_culled) && !(s.grad_mode && p->strict_nan) && p->max_order >= 2 && c->cw.size() >= 2 && tiles >= c->sched_min_tiles) {
        if ((rc = cur.d_sched.ensure((size_t)tiles))) return rc;
        if ((rc = cur.d_sched_key.ensure((size_t)tiles))) return rc;
        if (!pr.zeroed) {
            if ((rc = cur.d_shadow.ensure((size_t)c->N + d2d::SCHED_KEYS))) return rc;
            HIP_TRY(hipMemsetAsync(cur.d_shadow.p + c->N, 0, d2d::SCHED_KEYS * sizeof(unsigned long long), s.ps));
        }
        int* hist = reinterpret_cast<int*>(cur.d_shadow.p + c->N);  // [SCHED_KEYS] counts, [SCHED_KEYS] cursors
        // cost key: what the patch cost last time, when this context has swept the same grid before (optimisation
        // loops, repeated maps); otherwise a proxy computed from the geometry
        const bool from_history = cur.cost_tiles == tiles && c->use_cost_history;
        // no (usable) history: the lengths of the region lists this launch has just built, if any, else the geometric proxy
        const bool from_lists = !from_history && a.rl != nullptr;
        pr.sched_from_history = from_history || from_lists;
        if (!from_history && !from_lists)
            hipLaunchKernelGGL(d2d::patch_cost_kernel, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, s.ps, a, cur.d_sched_key.p);
        // keys from the work history depend on nothing this launch has built: the sort then runs on the side stream,
        // beside the shadow masks and the region lists, behind the memset of its counters
        const bool one_wg = tiles <= d2d::SORT1_MAX;  // the whole sort in one workgroup's LDS: nothing zeroed, nothing to wait for
        const bool side = from_history && (pr.zeroed || (one_wg && s.piped)) && (s.piped ? c->sort_stream : c->aux_stream) != nullptr;
        hipStream_t ss = side ? (s.piped ? c->sort_stream : c->aux_stream) : s.ps;
        // (ev_fork sits on `ps` behind the zeroing; without the pipeline `ps` is the main stream, i.e. also behind the
        // previous sweep, whose work counters the sort reads)
        if (side && (!one_wg || !s.piped)) HIP_TRY(hipStreamWaitEvent(ss, c->ev_fork, 0));
        // (the one-workgroup sort waits for nothing this launch builds -- only for the sweep that last read this set's schedule)
        if (side && one_wg && s.piped && s.set_was_swept) HIP_TRY(hipStreamWaitEvent(ss, cur.ev_swept, 0));
        const unsigned* cost_in = from_history ? cur.d_cost.p : (const unsigned*)nullptr;
        const d2d::RegionLists* lists_in = from_lists ? a.rl : (const d2d::RegionLists*)nullptr;
        if (one_wg) {
            hipLaunchKernelGGL(d2d::patch_sort_kernel, dim3(1), dim3(d2d::SORT1_THREADS), 0, ss, cur.d_sched_key.p, cost_in, cur.d_sched.p,
                               (long)tiles, lists_in, s.tiles_x, c->rl_plan.k_lo, p->max_order);
        } else {
            const unsigned sort_blocks = (unsigned)((tiles + 256 * d2d::SCHED_PER_THREAD - 1) / (256 * d2d::SCHED_PER_THREAD));
            hipLaunchKernelGGL(d2d::patch_hist_kernel, dim3(sort_blocks), dim3(256), 0, ss, cur.d_sched_key.p, cost_in, hist, (long)tiles,
                               lists_in, s.tiles_x, c->rl_plan.k_lo, p->max_order);
            hipLaunchKernelGGL(d2d::patch_order_kernel, dim3(sort_blocks), dim3(256), 0, ss, cur.d_sched_key.p, hist,
                               hist + d2d::SCHED_KEYS, cur.d_sched.p, (long)tiles);
        }
        if (side) {
            HIP_TRY(hipEventRecord(c->ev_join, ss));
            HIP_TRY(hipStreamWaitEvent(s.ps, c->ev_join, 0));
        }
        HIP_TRY(hipGetLastError());
        a.sched = cur.d_sched.p;
    }
    if (c->sched_override_n == tiles && !s.txg) a.sched = c->d_sched_override.p;
    if (a.sched && !s.d_stats) {
        if ((rc = cur.d_cost.ensure((size_t)tiles))) return rc;
        a.cost_out = cur.d_cost.p;  // the kernels launched below count the work of every patch
        cur.cost_tiles = tiles;     // (stream order: the next launch's key kernel runs after this sweep)
    }
    return D2D_OK;
}

// behind a LISTED launch: how the lists fared, read back without waiting (see prep_region_lists)
static int read_back_meta(d2d_ctx* c) {
    if (!c->meta_pending && c->h_meta && (c->rl_launches <= 3 || c->rl_launches % 16 == 0)) {
        HIP_TRY(hipMemcpyAsync(c->h_meta, c->cur.rl_meta_ptr, 2 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipEventRecord(c->ev_meta, c->stream));
        c->meta_pending = true;
        c->pend_static = c->rl_meta_static;  // the plan THIS launch's counters belong to
        c->pend_chunks = c->rl_meta_chunks;
    }
    return D2D_OK;
}

// The sweep kernel, launch(a, grid); behind a LISTED one (a.rl) the patches it left to the enumerating build (usually none):
// a few workgroups walk the queue, launch(args without lists, schedule or cut patches, their grid); then the read-back of
// how the lists fared.
template <class Launch>
static int sweep_and_walk(d2d_ctx* c, const Sweep& s, const Prep& pr, const d2d::SweepArgs& a, dim3 grid, Launch launch) {
    HIP_TRY(launch(a, grid));
    if (!a.rl || pr.queue_impossible) return D2D_OK;
    d2d::SweepArgs af = a;
    af.rl = nullptr; af.sched = nullptr; af.n_heavy = 0;
    HIP_TRY(launch(af, dim3((unsigned)std::min<long long>(s.tiles, std::max<long long>(256, c->fb_hint)))));
    return read_back_meta(c);
}

// everything before this is preparation (memsets, shadow masks, schedule); what follows is the sweep kernel itself
static int sweep_begin(d2d_ctx* c, const Sweep& s) {
    if (s.piped) {
        // the sweep waits for this launch's preparation; the set is busy until the sweep is through (sweep_done)
        HIP_TRY(hipEventRecord(c->ev_prep, s.ps));
        HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_prep, 0));
    }
    c->have_kernel_time = false;
    if (c->time_kernel) HIP_TRY(hipEventRecord(c->evk0, c->stream));
    return D2D_OK;
}

// behind the sweep kernel(s)
static int sweep_done(d2d_ctx* c) {
    if (c->time_kernel) {
        HIP_TRY(hipEventRecord(c->evk1, c->stream));
        c->have_kernel_time = true;
    }
    if (c->pipeline && c->aux_stream != nullptr) {
        // (also behind a launch that prepared on the sweep stream: a later pipelined launch may take its set)
        HIP_TRY(hipEventRecord(c->cur.ev_swept, c->stream));
        c->cur.swept_pending = true;
    }
    return D2D_OK;
}

// TX grid, values only: culled, or exhaustive (the "txg_exhaustive" option, or a degenerate path can count)
static int launch_txg_values(d2d_ctx* c, Sweep& s, const Prep& pr) {
    const int mode = s.th.mode, max_order = s.p->max_order;
    int rc;
    if (s.txg_culled) {
        const size_t lds_t = (size_t)(3 * c->N + 1) * sizeof(float4);
        if (lds_t > c->lds_max) return fail(D2D_ERR_UNSUPPORTED, "%d objects exceed the kernel's LDS table", c->N);
        rc = sweep_and_walk(c, s, pr, s.a, s.grid_patches, [&](const d2d::SweepArgs& x, dim3 g) {
            return d2d::launch_txg(mode, x.rl != nullptr, false, max_order, g, lds_t, c->stream, x);
        });
        if (rc) return rc;
    } else {
        // the per-lane-image code path without the adjoint
        const size_t lds0 = (size_t)(4 * c->N + 4) * sizeof(float);
        HIP_TRY(d2d::launch_vg(mode, true, false, s.grid_patches, lds0, c->stream, s.a));
    }
    return sweep_done(c);
}

// The NaN scan (d2d_nanscan.hpp) on stream st
static int launch_scan(d2d_ctx* c, const Sweep& s, hipStream_t st, const d2d::SweepArgs& as) {
    // two levels (a workgroup of 16 waves per region of 4 x 4 patches) when the region's list fits beside the tables
    const size_t lds_r = (size_t)(3 * c->N) * sizeof(float4) + (size_t)d2d::NAN_LCAP * sizeof(unsigned long long) +
                         (size_t)(2 * d2d::NAN_W + 1) * (size_t)((c->N + 31) / 32) * sizeof(unsigned) + 16;
    // (+ the kernel's static LDS: boxes, counters, the region's probe queue, its cells and their flag words)
    const size_t lds_static = 512 + (size_t)d2d::NAN_WQCAP * sizeof(unsigned long long) + (size_t)d2d::NAN_W * (64 * sizeof(float2) + 16);
    const bool regions = c->nan_scan_mode != 2 && lds_r + lds_static <= d2d_host::LDS_LIMIT && c->N <= 4095;
    const size_t lds_n = regions ? lds_r : (size_t)(3 * c->N) * sizeof(float4) + (size_t)c->N * sizeof(int) + 16;
    if (lds_n > c->lds_max) return fail(D2D_ERR_UNSUPPORTED, "%d objects exceed the NaN scan's LDS table", c->N);
    unsigned long long* ns = nullptr;
    if (c->nan_scan_stats) {
        int rc;
        if ((rc = c->d_nan_stats.ensure(8))) return rc;
        HIP_TRY(hipMemsetAsync(c->d_nan_stats.p, 0, 8 * sizeof(unsigned long long), st));
        ns = c->d_nan_stats.p;
    }
    const dim3 grid_regions((unsigned)(((s.tiles_x + d2d::NAN_R - 1) / d2d::NAN_R) * ((s.tiles_y + d2d::NAN_RY - 1) / d2d::NAN_RY)));
    d2d::SweepArgs ac = as;
    ac.nan_wqcap = c->nan_wqcap > 0 ? (int)c->nan_wqcap : d2d::NAN_WQCAP;  // (the kernel takes them as they are: never 0)
    ac.nan_rb = c->nan_rb > 0 ? (int)c->nan_rb : d2d::NAN_RB;
    // (the region kernel's debug instance -- run-time buffer sizes, counters -- only when a test asked for either)
    const bool dbg = c->nan_wqcap > 0 || c->nan_rb > 0 || c->nan_scan_stats;
    HIP_TRY(d2d::launch_nan_scan(s.p->approx != 0, s.txg, s.p->max_order, regions, dbg, regions ? grid_regions : s.grid_patches, lds_n, st, ac, ns));
    return D2D_OK;
}

// Value + gradient (+ the scene VJP's partial sums and their reduction, grad_mode 2)
static int launch_value_grad(d2d_ctx* c, Sweep& s, const Prep& pr) {
    const d2d_params* p = s.p;
    d2d::SweepArgs& a = s.a;
    const int mode = s.th.mode, grad_mode = s.grad_mode;
    const bool txg = s.txg;
    int rc = D2D_OK;
    const size_t cells = (size_t)c->m * c->n;
    if (p->out_mode == D2D_OUT_ADD && !c->have_grad) return fail(D2D_ERR_STATE, "D2D_OUT_ADD needs a previous value+grad sweep on this grid");
    if (grad_mode == 2 && p->out_mode == D2D_OUT_ADD && c->have_vjp) {
        // a scene VJP accumulated over several transmitters must come from sweeps of one kind (an ImagePath sweep has no
        // phi part) and must still be this rank's own partial sum
        if (c->vjp_has_phi)
            return fail(D2D_ERR_STATE, "D2D_OUT_ADD: the resident scene VJP comes from a MinPath / FermatPath sweep; an ImagePath sweep cannot be added to it");
        if (c->vjp_reduced)
            return fail(D2D_ERR_STATE, "D2D_OUT_ADD: the resident scene VJP has been all-reduced over ranks; fetch it, then start a new sum (D2D_OUT_OVERWRITE)");
    }
    if ((rc = c->d_grad.ensure(2 * cells))) return rc;
    c->have_grad = true;
    a.grad = c->d_grad.p;
    a.cot = c->have_cot ? c->d_cot.p : nullptr;
    const int n_elem = 4 * c->N + 2;
    if (grad_mode == 2) {
        if ((rc = c->d_partial.ensure((size_t)s.tiles * n_elem))) return rc;
        if ((rc = c->d_vjp.ensure((size_t)n_elem + 2 * (size_t)c->N))) return rc;  // [4N] end points, [2] fixed point, [N] phi, [N] coef
        a.partial = c->d_partial.p;
    }
    // the coefficient adjoint of the per-object function: N more floats of LDS per wave behind everything else, one row per patch
    const bool coef_vjp = grad_mode == 2 && p->fun_id == D2D_FUN_RECEIVED_POWER_PER_OBJECT && c->N > 0;
    const size_t lds_coef = coef_vjp ? (size_t)c->N * sizeof(float) : 0;
    if (coef_vjp) {
        if ((rc = c->d_coef_partial.ensure((size_t)s.tiles * (size_t)c->N))) return rc;
        a.coef_partial = c->d_coef_partial.p;
    }
    if (p->out_mode == D2D_OUT_OVERWRITE) c->have_vjp = false;
    // (hard validity with fun = 1: nothing is differentiated through the path; order 0 alone: only path_length's own trap)
    const bool scan = !p->strict_nan && (!txg || s.txg_culled) && c->nan_scan && (p->approx || p->fun_id != D2D_FUN_ONE) &&
                      ((p->max_order >= 1 && !c->cw.empty()) || (p->min_order <= 0 && p->fun_id != D2D_FUN_ONE));
    // The culled sweep writes the gradients of the candidates it evaluates; the reference's autodiff NaN positions -- an exact
    // zero in the backward scan of ANY candidate, valid or not -- come from a pass of their own (d2d_nanscan.hpp), which
    // poisons the cells and the patches' rows of VJP partial sums the way the exhaustive kernel (strict_nan) would have
    // written them.  It reads the scene's tables and the grid only: it runs BESIDE the sweep on a stream of its own and
    // leaves flags that nan_apply_kernel applies once both are through.
    // Every size check of the sweeps below comes BEFORE the scan is forked onto its own stream: nothing may fail between the
    // fork and the join (a scan left running would read tables that a later d2d_set_scene rewrites).
    const bool culled_rx = !txg && !p->strict_nan;
    const size_t lds_tab = (size_t)(4 * c->N + 1) * sizeof(float4);  // tables, adjoint table
    const size_t lds_culled = culled_rx ? lds_tab + 512 : lds_tab;    // (+ the culling queue)
    if ((culled_rx || s.txg_culled) && lds_culled + lds_coef > c->lds_max) return fail(D2D_ERR_UNSUPPORTED, "%d objects exceed the kernel's LDS table", c->N);
    const size_t lds_vg = (size_t)(4 * c->N + 4) * sizeof(float);  // the exhaustive kernel's wall adjoints
    if (coef_vjp && !culled_rx && !s.txg_culled && lds_vg + lds_coef > c->lds_max) return fail(D2D_ERR_UNSUPPORTED, "%d objects exceed the kernel's LDS table", c->N);
    if (coef_vjp) a.coef_lds_off = (int)((culled_rx || s.txg_culled) ? lds_culled : lds_vg);
    // ... and should a launch fail behind the fork all the same (a HIP error), the scan is waited for before the error is returned
    struct ScanJoin {
        d2d_ctx* c;
        bool armed = false;
        ~ScanJoin() {
            if (armed && c->scan_stream) (void)hipStreamSynchronize(c->scan_stream);
        }
    } scan_join{c};
    const int rw = 1 + (c->N + 31) / 32;
    if (scan) {
        if (c->scan_stream == nullptr) {
            int prio_lo = 0, prio_hi = 0;
            (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
            HIP_TRY(hipStreamCreateWithPriority(c->scan_stream.put(), hipStreamNonBlocking, prio_lo));
        }
        if (!c->ev_scan_fork) HIP_TRY(hipEventCreateWithFlags(c->ev_scan_fork.put(), hipEventDisableTiming | hipEventDisableSystemFence));
        if (!c->ev_scan_done) HIP_TRY(hipEventCreateWithFlags(c->ev_scan_done.put(), hipEventDisableTiming | hipEventDisableSystemFence));
        if ((rc = c->d_nan_cells.ensure((size_t)s.tiles))) return rc;
        if (grad_mode == 2 && (rc = c->d_nan_rows.ensure((size_t)s.tiles * rw))) return rc;
        d2d::SweepArgs as = a;
        as.nan_cell_bits = c->d_nan_cells.p;
        as.nan_row_bits = grad_mode == 2 ? c->d_nan_rows.p : nullptr;
        as.nan_row_words = rw;
        // (the previous launch's nan_apply_kernel has read the flags: stream order through the fork event)
        HIP_TRY(hipEventRecord(c->ev_scan_fork, c->stream));
        HIP_TRY(hipStreamWaitEvent(c->scan_stream, c->ev_scan_fork, 0));
        scan_join.armed = true;
        if ((rc = launch_scan(c, s, c->scan_stream, as))) return rc;
        HIP_TRY(hipEventRecord(c->ev_scan_done, c->scan_stream));
    }
    if (culled_rx) {
        // culled value+grad sweep (default)
        a.cullq_off = (int)lds_tab;
        rc = sweep_and_walk(c, s, pr, a, s.grid_patches, [&](const d2d::SweepArgs& x, dim3 g) {
            return d2d::launch_fwd_grad(mode, x.rl != nullptr, p->max_order, g, lds_culled + lds_coef, c->stream, x);
        });
    } else if (s.txg_culled) {
        // TX grid, culled value+grad sweep
        rc = sweep_and_walk(c, s, pr, a, s.grid_patches, [&](const d2d::SweepArgs& x, dim3 g) {
            return d2d::launch_txg(mode, x.rl != nullptr, true, p->max_order, g, lds_culled + lds_coef, c->stream, x);
        });
    } else {
        HIP_TRY(d2d::launch_vg(mode, txg, true, s.grid_patches, lds_vg + lds_coef, c->stream, a));
    }
    if (rc) return rc;
    if (scan) {
        d2d::SweepArgs as = a;
        as.nan_cell_bits = c->d_nan_cells.p;
        as.nan_row_bits = grad_mode == 2 ? c->d_nan_rows.p : nullptr;
        as.nan_row_words = rw;
        HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_scan_done, 0));
        scan_join.armed = false;  // joined: the main stream is behind the scan from here on
        HIP_TRY(d2d::launch_nan_apply(c->stream, as, (long)s.tiles));
    }
    if ((rc = sweep_done(c))) return rc;
    if (grad_mode == 2) {
        const long rows = (long)s.tiles;  // one row of partials per patch
        if ((rc = join_comm(c, 2))) return rc;  // the previous step's all-reduce has finished with d_vjp
        const int accumulate = (p->out_mode == D2D_OUT_ADD && c->have_vjp) ? 1 : 0;
        c->vjp_has_phi = false;
        c->vjp_reduced = false;
        hipLaunchKernelGGL(d2d::vjp_reduce_kernel, dim3((unsigned)n_elem), dim3(256), 0, c->stream, c->d_partial.p,
                           rows, n_elem, c->d_vjp.p, accumulate);
        HIP_TRY(hipGetLastError());
        if (!accumulate) c->vjp_has_coef = false;  // a new sum
        if (coef_vjp) {
            // the fourth block, behind a phi block that an ImagePath sweep leaves at zero (d2d_comm_allreduce_vjp covers both by length)
            double* const phi_block = c->d_vjp.p + n_elem;
            const int acc_coef = (accumulate && c->vjp_has_coef) ? 1 : 0;
            if (!acc_coef) HIP_TRY(hipMemsetAsync(phi_block, 0, (size_t)c->N * sizeof(double), c->stream));
            hipLaunchKernelGGL(d2d::vjp_reduce_kernel, dim3((unsigned)c->N), dim3(256), 0, c->stream, c->d_coef_partial.p, rows, c->N,
                               phi_block + c->N, acc_coef);
            HIP_TRY(hipGetLastError());
            c->vjp_has_coef = true;
        }
        c->have_vjp = true;
    }
    return D2D_OK;
}

// RX grid, values (or the instrumented build): candidate by candidate (coop), every patch shared by 4 waves (split), or
// one wave per patch with the dearest patches cut in four
static int launch_rx_values(d2d_ctx* c, Sweep& s, const Prep& pr) {
    const d2d_params* p = s.p;
    d2d::SweepArgs& a = s.a;
    const int mode = s.th.mode;
    const long long tiles = s.tiles;
    const bool stats = s.d_stats != nullptr;
    int rc;
    const size_t tab_lds = d2d_host::tab_lds_bytes(c->N);  // tables (+ adjoint table) + one culling queue
    if (tab_lds > c->lds_max) return fail(D2D_ERR_UNSUPPORTED, "%d objects exceed the kernel's LDS table (max ~2400)", c->N);
    // Launches that hold only a few patches per SIMD are bound by their dearest patch: share every patch between
    // SPLIT_W waves there (power_fwd_split_kernel).  Big grids are throughput-bound: one wave per patch.
    const d2d_host::SplitLds sl = d2d_host::split_lds_bytes(c->N, d2d::SPLIT_W, d2d::SPLIT_LIST);  // ... + one culling queue per wave
    // (sigmoid validity: a wave that adds to a list instead of the running sum loses the sum's absorption shortcut, sig_zc_of --
    // measured at 64^2 .. 640^2 cells of cfg2's scene the shared patches take 7.5 .. 11.6 ms, one wave per patch 5.4 .. 7.8)
    // (measured with the last-segment masks in place, sweep kernel, ms -- 4 waves per patch / one: hard 512^2 0.068 / 0.072,
    // 640^2 0.080 / 0.065; hard_sigmoid 384^2 0.141 / 0.123 (8 waves candidate by candidate: 0.104), 512^2 0.136 / 0.121,
    // 640^2 0.117 / 0.097: hard launches share their patches up to 5120 of them, hard_sigmoid ones only candidate by candidate)
    const long long split_lim = c->split_max_tiles >= 0 ? c->split_max_tiles : (mode == d2d::MODE_HARD ? 5120 : 0);
    const bool split = p->max_order >= 2 && c->cw.size() >= 2 && sl.total <= d2d_host::LDS_LIMIT && tiles <= split_lim &&
                       (mode != d2d::MODE_SIG || c->split_sigmoid);
    // the smallest launches (the grids of the reference's own examples): W waves per patch, candidate by candidate
    // (power_fwd_coop_kernel).  Measured on cfg2's scene, ms per sweep kernel, best other kernel first:
    //   hard  128^2 0.096 -> 0.072 (16 waves)   200^2 0.093 -> 0.085 (8)   256^2 0.091 / 0.097 (8): none from there on
    //   hsig  128^2 0.204 -> 0.119 (16)         320^2 0.180 -> 0.163 (8)   384^2 0.136 -> 0.106 (8)   448^2 0.138 / 0.134
    //   sig   128^2 6.48 -> 1.28 (16)   200^2 6.26 -> 1.93 (16)   320^2 6.20 -> 3.07 (8)   512^2 5.35 -> 4.35 (4)   640^2 5.6 / 6.3
    int coop_w = 0;
    if (p->max_order >= 2 && c->cw.size() >= 2 && a.rl != nullptr && !stats && c->coop_waves != 0) {
        const bool sig = mode == d2d::MODE_SIG;
        const long long lim = c->coop_max_tiles >= 0 ? c->coop_max_tiles : (mode == d2d::MODE_HARD ? 640 : (sig ? 4096 : 2304));
        if (c->coop_waves > 0) coop_w = (int)c->coop_waves;
        else if (sig) coop_w = tiles <= 640 ? 16 : (tiles <= 1600 ? 8 : 4);
        else coop_w = tiles <= 256 ? 16 : 8;
        // ("split_max_tiles" = 0 asks for one wave per patch whatever the size: honoured unless the waves are forced)
        if (d2d_host::coop_lds_bytes(c->N, coop_w, d2d::COOP_C) + 4096 > d2d_host::LDS_LIMIT ||  /* (+ the kernel's static LDS: masks, chunks, floor) */ tiles > lim || (c->coop_waves < 0 && c->split_max_tiles >= 0 && tiles > c->split_max_tiles)) coop_w = 0;
    }
    // the dearest patches of a bigger launch are cut in four (see power_fwd_kernel); they are only known with a work history
    dim3 grid_fwd = s.grid_patches;
    if (!split && !coop_w && !stats && p->max_order == 2 && c->cw.size() >= 2 && a.sched == c->cur.d_sched.p && pr.sched_from_history && c->heavy_split != 0) {
        const long long P = d2d::HEAVY_PARTS;
        // -1 (default): launches that are only a few patch latencies long (fewer than 4 patches per wave slot of the chip)
        // are bound by their dearest patches: one patch in 93 is cut there (measured best at 1024^2), else 64 patches
        long long hs = c->heavy_split;
        if (hs < 0) {
            int cus = 256;
            (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device);
            // 3 patches in 32 (1536 at cfg2; round 2 cut 1 in 93, the best figure before the last-segment masks thinned the cheap
            // patches out): the launch stays bound by its dear patches far down the ranking -- hard_sigmoid 0.177 -> 0.134 ms
            // (1024 cut patches: 0.148, 2048: 0.138); hard, same transmitter every launch: 0.085 either way, a different one
            // every launch (a work history three positions old ranks the patches less well): 0.158 -> 0.104 ms per step
            hs = (tiles < 4ll * cus * 4 * 6) ? std::max<long long>(64, tiles * 3 / 32) : 64;
            // sigmoid: a part adds to a list, not to the running sum, and cannot drop the contributions that sum would
            // absorb (sig_zc_of) -- the dearest patches would lose their best shortcut (cfg2: 11.2 ms cut, 10.9 uncut)
            if (mode == d2d::MODE_SIG && a.sig_mono) hs = 0;
        }
        const d2d_host::HeavyPlan hp = d2d_host::heavy_plan(tiles, (long long)c->cw.size(), hs, P);
        const long long H = hp.H, cap = hp.cap;
        if (H > 0) {
            if ((rc = c->d_heavy_list.ensure((size_t)hp.list_floats))) return rc;
            if ((rc = c->d_heavy_cnt.ensure((size_t)hp.cnt_ints))) return rc;
            if (c->heavy_done_n < H) {
                if ((rc = c->d_heavy_done.ensure((size_t)H))) return rc;
                HIP_TRY(hipMemsetAsync(c->d_heavy_done.p, 0, (size_t)H * sizeof(int), c->stream));  // the kernel re-zeroes it
                c->heavy_done_n = H;
            }
            a.n_heavy = (int)H;
            a.heavy_cap = (int)cap;
            a.heavy_list = c->d_heavy_list.p;
            a.heavy_cnt = c->d_heavy_cnt.p;
            a.heavy_done = c->d_heavy_done.p;
            grid_fwd = dim3((unsigned)(tiles + (P - 1) * H));
        }
    }
    a.cullq_off = (int)(split ? sl.base : (size_t)(4 * c->N + 1) * sizeof(float4));
    c->last_shape_waves = coop_w ? coop_w : (split ? 4 : 1);
    c->last_shape_coop = coop_w ? 1 : 0;
    // one patch per wave, fwd_waves waves per workgroup (fewer, bigger workgroups are dispatched faster)
    // (0: 4 when a single-wave workgroup's LDS would keep a CU below 32 waves, else 1; STATS and the enumerating build: 1)
    const unsigned wpb_listed = c->fwd_waves > 0 ? (unsigned)c->fwd_waves : ((tab_lds * 32 > 160 * 1024) ? 4u : 1u);
#ifdef D2D_AB_TIMELINE  // diagnostic build: one start / end stamp per workgroup, read back by d2d_debug_get_work
    if (!coop_w && !split) {
        if (c->tl_ring_on) {
            // ... or only the first start / the end of every launch (an unperturbed pipelined sequence: scripts/launch_gaps.py)
            a.tl_ring = c->d_tl_ring.p;
            a.tl_seq = (int)(c->tl_seq++);
        } else {
            if ((rc = c->d_timeline.ensure(2 * (size_t)grid_fwd.x + 64))) return rc;
            HIP_TRY(hipMemsetAsync(c->d_timeline.p, 0, (2 * (size_t)grid_fwd.x + 64) * sizeof(unsigned), c->stream));
            c->timeline_n = 2 * (long long)grid_fwd.x;
            if (!stats) a.grad = reinterpret_cast<float*>(c->d_timeline.p);
        }
    }
#endif
    // (the queue walker -- x without lists -- is the split or the one-wave-per-patch kernel)
    rc = sweep_and_walk(c, s, pr, a, grid_fwd, [&](const d2d::SweepArgs& x, dim3 g) {
        const bool listed = x.rl != nullptr;
        if (coop_w && listed) return d2d::launch_fwd_coop(mode, p->max_order, coop_w, g, d2d_host::coop_lds_bytes(c->N, coop_w, d2d::COOP_C), c->stream, x);
        if (split) return d2d::launch_fwd_split(mode, listed, stats, p->max_order, g, sl.total, c->stream, x);
        const unsigned wpb = (listed && !stats) ? wpb_listed : 1u;
        const hipError_t e = d2d::launch_fwd(mode, listed, stats, p->max_order, dim3((g.x + wpb - 1) / wpb, wpb), tab_lds + (wpb - 1) * 512, c->stream, x);
#ifdef D2D_AB_TIMELINE
        if (c->tl_ring_on && &x == &a) hipLaunchKernelGGL(d2d::tl_end_kernel, dim3(1), dim3(1), 0, c->stream, c->d_tl_ring.p, a.tl_seq);
#endif
        return e;
    });
    if (rc) return rc;
    return sweep_done(c);
}

static int sweep_launch(d2d_ctx* c, const d2d_params* p, const float* tx, unsigned long long* d_stats, int grad_mode = 0) {
    if (!c || !tx) return fail(D2D_ERR_INVALID, "NULL argument");
    int rc = check_params(p);
    if (rc) return rc;
    if (!c->have_scene) return fail(D2D_ERR_STATE, "d2d_set_scene must come before a sweep");
    if (!c->have_grid) return fail(D2D_ERR_STATE, "d2d_set_grid must come before a sweep");
    c->have_kernel_time = false;  // whatever this launch turns out to be, the previous launch's kernel time is stale
    if (p->fun_id == D2D_FUN_CUSTOM && !grad_mode) return fail(D2D_ERR_UNSUPPORTED, "fun_id D2D_FUN_CUSTOM is for d2d_power_map_vg_launch only");
    if (p->fun_id == D2D_FUN_RECEIVED_POWER_PER_OBJECT) {
        if (p->solver == D2D_SOLVER_MINPATH || p->solver == D2D_SOLVER_FERMAT)
            return fail(D2D_ERR_UNSUPPORTED, "fun_id D2D_FUN_RECEIVED_POWER_PER_OBJECT (received_power_per_object) is fused for ImagePath sweeps only, not for the MinPath / FermatPath solvers");
        if (d_stats) return fail(D2D_ERR_UNSUPPORTED, "fun_id D2D_FUN_RECEIVED_POWER_PER_OBJECT (received_power_per_object) has no instrumented build");
        if ((int)c->coef.size() != c->N || (c->N > 0 && !c->d_coef.p))
            return fail(D2D_ERR_STATE, "fun_id D2D_FUN_RECEIVED_POWER_PER_OBJECT needs d2d_set_reflection_coefs for the resident scene");
    }
    if (p->solver == D2D_SOLVER_MINPATH || p->solver == D2D_SOLVER_FERMAT) {
        if (d_stats) return fail(D2D_ERR_UNSUPPORTED, "the optimiser-based solvers have no instrumented build");
        return opt_sweep_launch(c, p, tx, grad_mode);
    }
    d2d_params p_custom;
    if (p->fun_id == D2D_FUN_CUSTOM) {
        if ((rc = custom_fun_params(c, p, &p_custom))) return rc;
        p = &p_custom;
    }
    if ((rc = check_image_sweep(c, p, d_stats))) return rc;
    if ((rc = set_device(c))) return rc;
    if ((rc = upload_occl(c, p->patch))) return rc;

    Sweep s(c, p, tx, d_stats, grad_mode);
    Prep pr;
    if ((rc = take_prep_set(c, s)) || (rc = sweep_args(c, s))) return rc;
    if (s.txg_fallback) ++c->txg_fallbacks;
    if ((rc = prep_masks(c, s, pr)) || (rc = prep_region_lists(c, s, pr))) return rc;
    if (!s.a.rl) c->rl_plan.on = false;
    if ((rc = prep_schedule(c, s, pr)) || (rc = sweep_begin(c, s))) return rc;
    if (grad_mode) return launch_value_grad(c, s, pr);
    if (s.txg) return launch_txg_values(c, s, pr);
    return launch_rx_values(c, s, pr);
}

// What every launch of the sink kernel shares (d2d_valid_paths and the products below: `who` in the messages), from the validity mode on.
// Every refusal that the arguments and the context decide comes first, before anything is uploaded or enqueued; a TX grid is swept
// by the culled kernels only, and refusing one is not a fall-back.  Then the launch is prepared on the main stream, behind whatever
// the context has in flight, with masks of its own: the sweeps' rotating sets, work history, schedule and value map are not touched.
static int prep_sink_sweep(d2d_ctx* c, Sweep& s, const char* who, size_t& lds) {
    const d2d_params* p = s.p;
    int rc;
    if (p->approx && p->act != D2D_ACT_HARD_SIGMOID)
        return fail(D2D_ERR_UNSUPPORTED, "%s covers hard and hard_sigmoid validity: the sigmoid sweeps skip candidates by the fused function's running sum", who);
    if ((rc = check_image_sweep(c, p, nullptr))) return rc;
    if (c->N > 4095) return fail(D2D_ERR_UNSUPPORTED, "%s: %d objects exceed the 12-bit object indices of the culling queue and the records", who, c->N);
    if ((long long)c->m * c->n > 0x7fffffffLL) return fail(D2D_ERR_UNSUPPORTED, "%s: the grid exceeds 31-bit cell indices", who);
    lds = d2d_host::tab_lds_bytes(c->N);  // tables + one culling queue
    if (lds > c->lds_max) return fail(D2D_ERR_UNSUPPORTED, "%s: %d objects exceed the kernel's LDS table (max ~2400)", who, c->N);
    if (p->grid_role == D2D_GRID_TX && (c->txg_exhaustive || !d2d_host::sweep_thresholds(*p, false).degenerate_invalid))
        return fail(D2D_ERR_UNSUPPORTED, "%s: a TX-grid sweep with these parameters is not culled (%s)", who,
                    c->txg_exhaustive ? "the \"txg_exhaustive\" option is set" : "a degenerate path is not exactly invalid under tol / alpha");
    if ((rc = set_device(c))) return rc;
    if ((rc = upload_occl(c, p->patch))) return rc;
    s.ps = c->stream;
    if ((rc = sweep_args(c, s))) return rc;
    if (s.txg && !s.txg_culled) return fail(D2D_ERR_STATE, "%s: the TX-grid sweep is not culled after all (an internal error)", who);
    Prep pr;
    if ((rc = prep_masks(c, s, pr, &c->d_rec_shadow))) return rc;
    s.a.out = nullptr;  // never written by a sink
    s.a.cullq_off = (int)((size_t)(4 * c->N + 1) * sizeof(float4));
    return D2D_OK;
}

// One pass of the sink kernel over the prepared sweep `s` (prep_sink_sweep gave `lds`), on the main stream.
template <class Sink>
static hipError_t sink_pass(const d2d_ctx* c, const Sweep& s, size_t lds, const typename Sink::Args& x) {
    return d2d::launch_sink<Sink>(s.th.mode, s.txg, s.p->max_order, s.grid_patches, lds, c->stream, s.a, x);
}

// Record launch of the culled forward sweep: pass 1 counts the (cell, candidate) pairs with valid != 0 per patch, the host scans
// the counts, pass 2 writes the records, trace_rec_kernel solves their paths.
static int valid_paths(d2d_ctx* c, const d2d_params* p_in, const float* fixed, int64_t* count) {
    if (!c || !fixed || !count) return fail(D2D_ERR_INVALID, "NULL argument");
    *count = 0;
    int rc = check_params(p_in);
    if (rc) return rc;
    if (!c->have_scene) return fail(D2D_ERR_STATE, "d2d_set_scene must come before d2d_valid_paths");
    if (!c->have_grid) return fail(D2D_ERR_STATE, "d2d_set_grid must come before d2d_valid_paths");
    if (p_in->solver != D2D_SOLVER_IMAGE) return fail(D2D_ERR_UNSUPPORTED, "d2d_valid_paths covers ImagePath only (solver %d)", p_in->solver);
    c->rec_n = -1;  // whatever this call turns out to be, the previous records are gone
    c->have_rec_time = false;
    d2d_params pp = *p_in;
    pp.fun_id = D2D_FUN_ONE;  // a contribution is then the validity itself
    pp.out_mode = D2D_OUT_OVERWRITE;
    pp.strict_nan = 0;
    const d2d_params* p = &pp;
    Sweep s(c, p, fixed);
    size_t lds = 0;
    if ((rc = prep_sink_sweep(c, s, "d2d_valid_paths", lds))) return rc;
    const size_t tiles = (size_t)s.tiles;
    if ((rc = c->d_rec_counts.ensure(tiles)) || (rc = c->d_rec_offs.ensure(tiles + 1)) || (rc = c->d_rec_flag.ensure(1))) return rc;
    const bool timed = c->time_kernel;
    if (timed)
        for (Event& e : c->ev_rec)
            if (!e) HIP_TRY(hipEventCreate(e.put()));
    HIP_TRY(hipMemsetAsync(c->d_rec_flag.p, 0, sizeof(int), c->stream));
    d2d::RecArgs r;
    r.counts = c->d_rec_counts.p;
    r.offs = c->d_rec_offs.p;
    r.rec = nullptr;
    r.flag = c->d_rec_flag.p;
    // pass 1: count
    if (timed) HIP_TRY(hipEventRecord(c->ev_rec[0], c->stream));
    HIP_TRY(sink_pass<d2d::RecSink>(c, s, lds, r));
    if (timed) HIP_TRY(hipEventRecord(c->ev_rec[1], c->stream));
    std::vector<int> offs(tiles + 1);
    HIP_TRY(hipMemcpyAsync(offs.data() + 1, c->d_rec_counts.p, tiles * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    // exclusive scan on the host (4 bytes per patch; the call is synchronous anyway)
    long long total = 0;
    offs[0] = 0;
    for (size_t i = 1; i <= tiles; ++i) {
        if (offs[i] < 0) return fail(D2D_ERR_STATE, "d2d_valid_paths: patch %zu counted %d records", i - 1, offs[i]);
        total += offs[i];
        offs[i] = (int)std::min<long long>(total, 0x7fffffffLL);
    }
    // what the records and their paths take: 16 B + cell, cand[4], order + xys[6][2], loss, valid, length
    constexpr size_t NPTS = D2D_MAX_ORDER + 2;
    const size_t per_record = sizeof(int4) + (2 + D2D_MAX_ORDER) * sizeof(int) + (NPTS * 2 + 3) * sizeof(float);
    size_t mem_free = 0, mem_total = 0;
    HIP_TRY(hipMemGetInfo(&mem_free, &mem_total));
    // (half of what is free, plus what the buffers hold already; 2^30 records: positions are 32-bit)
    const size_t held = c->d_rec.n * per_record;
    *count = total;
    if (total > (1ll << 30) || (size_t)total * per_record > (mem_free + held) / 2)
        return fail(D2D_ERR_UNSUPPORTED, "d2d_valid_paths: %lld records (%zu bytes each) exceed half of the free device memory (%zu bytes free)",
                    total, per_record, mem_free);
    if (total == 0) {
        c->rec_n = 0;
        return D2D_OK;
    }
    const size_t n = (size_t)total;
    if ((rc = c->d_rec.ensure(n)) || (rc = c->d_rec_cell.ensure(n)) || (rc = c->d_rec_cand.ensure(n * D2D_MAX_ORDER)) ||
        (rc = c->d_rec_order.ensure(n)) || (rc = c->d_rec_xys.ensure(n * NPTS * 2)) || (rc = c->d_rec_loss.ensure(n)) ||
        (rc = c->d_rec_valid.ensure(n)) || (rc = c->d_rec_len.ensure(n)))
        return rc;
    // (c->rec_n stays -1 until everything below is through)
    HIP_TRY(hipMemcpyAsync(c->d_rec_offs.p, offs.data(), (tiles + 1) * sizeof(int), hipMemcpyHostToDevice, c->stream));
    // a slot pass 2 does not write names no cell: trace_rec_kernel flags it instead of reading through it
    HIP_TRY(hipMemsetAsync(c->d_rec.p, 0xff, n * sizeof(int4), c->stream));
    // pass 2: the same sweep, writing
    r.rec = c->d_rec.p;
    if (timed) HIP_TRY(hipEventRecord(c->ev_rec[2], c->stream));
    HIP_TRY(sink_pass<d2d::RecSink>(c, s, lds, r));
    if (timed) HIP_TRY(hipEventRecord(c->ev_rec[3], c->stream));
    // stage 2: the paths of the records
    d2d::TraceArgs t;
    memset(&t, 0, sizeof t);
    t.T = obj_tables(c);
    t.solver = D2D_SOLVER_IMAGE;
    t.xys = c->d_rec_xys.p;
    t.loss = c->d_rec_loss.p;
    t.valid = c->d_rec_valid.p;
    t.length = c->d_rec_len.p;
    set_validity(t, p);
    d2d::RecTraceArgs q;
    q.rec = c->d_rec.p;
    q.n = (long)n;
    q.X = c->d_X.p;
    q.Y = c->d_Y.p;
    q.cells = (long)c->m * c->n;
    q.fx = fixed[0];
    q.fy = fixed[1];
    q.txg = s.txg ? 1 : 0;
    q.cell = c->d_rec_cell.p;
    q.cand = c->d_rec_cand.p;
    q.order = c->d_rec_order.p;
    q.flag = c->d_rec_flag.p;
    if (timed) HIP_TRY(hipEventRecord(c->ev_rec[4], c->stream));
    hipLaunchKernelGGL(d2d::trace_rec_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c->stream, t, q);
    HIP_TRY(hipGetLastError());
    if (timed) HIP_TRY(hipEventRecord(c->ev_rec[5], c->stream));
    int flag = 0;
    HIP_TRY(hipMemcpyAsync(&flag, c->d_rec_flag.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (flag) return fail(D2D_ERR_STATE, "d2d_valid_paths: the two passes of the record launch disagree (%lld records counted)", total);
    c->rec_n = total;
    c->have_rec_time = timed;
    return D2D_OK;
}

// ---- the products of the sink kernel ---------------------------------------------------------------------------------
// Every product is one more sink of power_sink_kernel behind the same host path; DESIGN.md ("Adding a product of the sink kernel")
// says what a new one writes and where.
struct SinkProduct {
    const char* who;           // the launch's name in the messages
    const char* custom_route;  // how check_fused_sink's refusal of D2D_FUN_CUSTOM ends: what to do instead
    const char* add_why;       // ... and its refusal of D2D_OUT_ADD
    bool early_discard;        // when a launch forgets the previous result (below)
};
// Discard timing is behaviour, and it differs for historical reasons only: the four older products forget the previous result as
// soon as the state checks pass (EARLY: any later refusal leaves nothing to get), the five newer ones when the launch is accepted
// and the buffers are about to change (LATE: a refused launch leaves the previous result readable).  Callers may rely on either.
constexpr bool EARLY = true, LATE = false;
constexpr SinkProduct PROFILE = {"d2d_power_profile_launch", "a host function's profile: bin the records of d2d_valid_paths", "a profile is always overwritten", EARLY};
constexpr SinkProduct TOP = {"d2d_strongest_paths_launch", "a host function's strongest paths: sort the records of d2d_valid_paths", "the slots are always overwritten", EARLY};
constexpr SinkProduct FIELD = {"d2d_coherent_field_launch", "a host function's field: add the phasors of the records of d2d_valid_paths", "the field is always overwritten", EARLY};
constexpr SinkProduct FREQ = {"d2d_frequency_response_launch", "a host function's response: add the phasors of the records of d2d_valid_paths", "the response is always overwritten", EARLY};
constexpr SinkProduct COEF_VJP = {"d2d_field_coefs_vjp_launch", "a host function has no coefficients", "the gradient is always overwritten", LATE};
constexpr SinkProduct ANGLE = {"d2d_power_angle_launch", "a host function's profile: bin the paths that d2d_trace_paths gives for the records of d2d_valid_paths", "a profile is always overwritten", LATE};
constexpr SinkProduct ARRAY = {"d2d_array_response_launch", "a host function's channel matrix: add the steered phasors of the paths that d2d_trace_paths gives for the records of d2d_valid_paths", "the channel matrix is always overwritten", LATE};
constexpr SinkProduct WIDE = {"d2d_array_frequency_response_launch", "a host function's channel matrices: add the steered phasors of the paths that d2d_trace_paths gives for the records of d2d_valid_paths", "the channel matrices are always overwritten", LATE};
constexpr SinkProduct MATERIAL = {"d2d_material_response_launch", "a host function's response: add the phasors of the paths that d2d_trace_paths gives for the records of d2d_valid_paths, each times its walls' Fresnel coefficients", "the response is always overwritten", LATE};
constexpr SinkProduct EPS_VJP = {"d2d_material_eps_vjp_launch", "a host function has no permittivities", "the gradient is always overwritten", LATE};
constexpr SinkProduct POS_VJP = {"d2d_field_position_vjp_launch", "a host function's derivative with respect to the path length is not known to the library", "the gradient is always overwritten", LATE};
constexpr SinkProduct WALL_VJP = {"d2d_field_walls_vjp_launch", "a host function's derivative with respect to the path length is not known to the library", "the gradient is always overwritten", LATE};
constexpr SinkProduct BEAM = {"d2d_beam_response_launch", "a host function's beam response: add the beamformed phasors of the paths that d2d_trace_paths gives for the records of d2d_valid_paths", "the beam response is always overwritten", LATE};

// What the products refuse of the caller's parameters before prep_sink_sweep's share.
static int check_fused_sink(d2d_ctx* c, const d2d_params* p, const SinkProduct& pr) {
    if (p->solver == D2D_SOLVER_MINPATH || p->solver == D2D_SOLVER_FERMAT)
        return fail(D2D_ERR_UNSUPPORTED, "%s covers ImagePath only, not the MinPath / FermatPath solvers (solver %d)", pr.who, p->solver);
    if (p->fun_id == D2D_FUN_CUSTOM)
        return fail(D2D_ERR_UNSUPPORTED, "%s: fun_id D2D_FUN_CUSTOM is for d2d_power_map_vg_launch only (%s)", pr.who, pr.custom_route);
    if (p->out_mode == D2D_OUT_ADD) return fail(D2D_ERR_UNSUPPORTED, "%s: D2D_OUT_ADD is not supported, %s", pr.who, pr.add_why);
    if (p->fun_id == D2D_FUN_RECEIVED_POWER_PER_OBJECT && ((int)c->coef.size() != c->N || (c->N > 0 && !c->d_coef.p)))
        return fail(D2D_ERR_STATE, "fun_id D2D_FUN_RECEIVED_POWER_PER_OBJECT needs d2d_set_reflection_coefs for the resident scene");
    return D2D_OK;
}

// One launch of a product, whose result is the context's `r`: the stages every product walks in the same order, with the product's
// own steps between them (the NULL-argument check comes before a SinkLaunch exists).  Every check comes before anything is
// enqueued; the launches are asynchronous.
//   begin    check_params, the state checks, the EARLY discard, the product's pre-check if it has one, check_fused_sink
//            -- the product's parameter check --
//   device   set_device and the free device memory, for
//            -- the product's memory check (fits: the rule and the message that five products share) --
//   prepare  the sweep's preparation (prep_sink_sweep), then the LATE discard
//            -- ensure the buffers, zero what the sink adds into, the passes, mark the result --
template <class Result>
struct SinkLaunch {
    d2d_ctx* const c;
    const SinkProduct& pr;
    Result& r;
    d2d_params pp;  // the caller's parameters with strict_nan = 0; a product may substitute more between begin and prepare
    // Built before any check, and from pp while it is still zero: sound only because Sweep's constructor reads nothing but the
    // grid's shape (c->m, c->n: s.tiles, for a memory check that needs the patch count) and STORES the pointer to the parameters.
    // A constructor that ever read *p would have to move into begin, behind the state checks.
    Sweep s;
    const size_t cells;
    size_t lds = 0, mem_free = 0;
    SinkLaunch(d2d_ctx* c, const SinkProduct& pr, Result& r, const float* fixed)
        : c(c), pr(pr), r(r), pp(), s(c, &pp, fixed), cells((size_t)c->m * (size_t)c->n) {}
    SinkLaunch(const SinkLaunch&) = delete;  // (s points at pp)

    template <class Pre>
    int begin(const d2d_params* p_in, Pre pre) {
        int rc = check_params(p_in);
        if (rc) return rc;
        if (!c->have_scene) return fail(D2D_ERR_STATE, "d2d_set_scene must come before %s", pr.who);
        if (!c->have_grid) return fail(D2D_ERR_STATE, "d2d_set_grid must come before %s", pr.who);
        if (pr.early_discard) r.forget();  // whatever this launch turns out to be, the previous result is gone
        if ((rc = pre()) || (rc = check_fused_sink(c, p_in, pr))) return rc;
        pp = *p_in;
        pp.strict_nan = 0;
        return D2D_OK;
    }
    int begin(const d2d_params* p_in) { return begin(p_in, [] { return D2D_OK; }); }
    int device() {
        if (int rc = set_device(c)) return rc;
        size_t mem_total = 0;
        HIP_TRY(hipMemGetInfo(&mem_free, &mem_total));
        return D2D_OK;
    }
    int fits(size_t bytes_per_cell, size_t held) const {
        if (d2d_host::outputs_fit(cells, bytes_per_cell, mem_free, held)) return D2D_OK;
        return fail(D2D_ERR_UNSUPPORTED, "%s: %zu cells (%zu bytes per cell) exceed half of the free device memory (%zu bytes free)", pr.who, cells,
                    bytes_per_cell, mem_free);
    }
    int prepare() {
        if (int rc = prep_sink_sweep(c, s, pr.who, lds)) return rc;
        if (!pr.early_discard) r.forget();  // from here on the buffers change
        return D2D_OK;
    }
    template <class Sink>
    hipError_t pass(const typename Sink::Args& x) const {
        return sink_pass<Sink>(c, s, lds, x);
    }
};

// The getters: no result without a context, a grid and an accepted launch (`holds`; `goes_with` ends the message) ...
static int result_state(const d2d_ctx* c, bool holds, const SinkProduct& pr, const char* goes_with = "result goes with the grid") {
    if (!c) return fail(D2D_ERR_INVALID, "ctx is NULL");
    if (!c->have_grid) return fail(D2D_ERR_STATE, "no grid set");
    if (!holds) return fail(D2D_ERR_STATE, "%s must come first (its %s)", pr.who, goes_with);
    return D2D_OK;
}
// ... then the copies the caller asked for (dst not NULL), behind whatever is in flight, and one synchronisation.
struct CopyOut {
    void* dst;
    const void* src;
    size_t bytes;
};
static int copy_out(d2d_ctx* c, std::initializer_list<CopyOut> copies) {
    if (int rc = set_device(c)) return rc;
    for (const CopyOut& x : copies)
        if (x.dst) HIP_TRY(hipMemcpyAsync(x.dst, x.src, x.bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return D2D_OK;
}

static_assert(d2d_host::POS_CHUNK == d2d::POS_CHUNK, "d2d_host.hpp and d2d_posgrad.hpp disagree");  // (the other chunks: d2d_chunks.hpp, stated once)

}  // namespace

extern "C" {

// Bin build: ONE pass into the zeroed profile.  (Its memory check keeps arithmetic of its own: (free + held) / 2 against a
// product of quotients, where outputs_fit halves both terms.)
int d2d_power_profile_launch(d2d_ctx* c, const d2d_params* p, const float* fixed, float r_min, float r_max, int32_t nbins) {
    if (!c || !fixed) return fail(D2D_ERR_INVALID, "NULL argument");
    SinkLaunch<d2d_ctx::Profile> L(c, PROFILE, c->prof, fixed);
    d2d_host::ProfileBins bins;
    std::string err;
    int rc;
    if ((rc = L.begin(p))) return rc;
    if ((rc = d2d_host::profile_bins(r_min, r_max, nbins, bins, err))) return fail(rc, "%s", err.c_str());
    if ((rc = L.device())) return rc;
    const size_t budget = (L.mem_free + c->prof.out.n * sizeof(float)) / 2;  // (half of what is free, plus what the buffer holds already)
    if (L.cells > 0 && (size_t)nbins > budget / sizeof(float) / L.cells)
        return fail(D2D_ERR_UNSUPPORTED, "d2d_power_profile_launch: %d bins of %zu cells (4 bytes each) exceed half of the free device memory (%zu bytes free)",
                    nbins, L.cells, L.mem_free);
    if ((rc = L.prepare()) || (rc = c->prof.out.ensure((size_t)nbins * L.cells))) return rc;
    d2d::BinArgs b;
    b.out = c->prof.out.p;
    b.cells = (long)L.cells;
    b.r_min = bins.r_min;
    b.inv = bins.inv;
    b.nbins = bins.nbins;
    HIP_TRY(hipMemsetAsync(c->prof.out.p, 0, (size_t)nbins * L.cells * sizeof(float), c->stream));
    if (L.s.tiles > 0) HIP_TRY(L.pass<d2d::BinSink>(b));
    c->prof.nbins = nbins;
    return D2D_OK;
}

int d2d_get_power_profile(d2d_ctx* c, float* out) {
    if (!c || !out) return fail(D2D_ERR_INVALID, "NULL argument");
    if (int rc = result_state(c, c->prof.nbins >= 1 && c->prof.out.p, PROFILE, "profile goes with the grid")) return rc;
    return copy_out(c, {{out, c->prof.out.p, (size_t)c->prof.nbins * (size_t)c->m * c->n * sizeof(float)}});
}

// Top-k build: ONE pass, every lane writing the whole of its cell (no zeroing in front).
int d2d_strongest_paths_launch(d2d_ctx* c, const d2d_params* p, const float* fixed, int32_t k) {
    if (!c || !fixed) return fail(D2D_ERR_INVALID, "NULL argument");
    SinkLaunch<d2d_ctx::Top> L(c, TOP, c->top, fixed);
    d2d_ctx::Top& r = c->top;
    int rc;
    if ((rc = L.begin(p))) return rc;
    if (k < 1 || k > D2D_TOP_MAX) return fail(D2D_ERR_INVALID, "d2d_strongest_paths_launch: k = %d is outside 1..D2D_TOP_MAX (%d)", k, D2D_TOP_MAX);
    if ((rc = L.device())) return rc;
    if (!d2d_host::outputs_fit(L.cells, d2d_host::top_bytes_per_cell(k), L.mem_free, r.bytes()))
        return fail(D2D_ERR_UNSUPPORTED, "d2d_strongest_paths_launch: %d slots of %zu cells (%zu bytes per cell) exceed half of the free device memory (%zu bytes free)",
                    k, L.cells, d2d_host::top_bytes_per_cell(k), L.mem_free);
    if ((rc = L.prepare())) return rc;
    const size_t kc = (size_t)k * L.cells;
    if ((rc = r.power.ensure(kc)) || (rc = r.len.ensure(kc)) || (rc = r.cand.ensure(kc * D2D_MAX_ORDER)) || (rc = r.order.ensure(kc)) ||
        (rc = r.total.ensure(L.cells)) || (rc = r.count.ensure(L.cells)))
        return rc;
    d2d::TopArgs t;
    t.power = r.power.p;
    t.length = r.len.p;
    t.cand = r.cand.p;
    t.order = r.order.p;
    t.total = r.total.p;
    t.count = r.count.p;
    t.cells = (long)L.cells;
    t.k = k;
    if (L.s.tiles > 0) HIP_TRY(L.pass<d2d::TopSink>(t));
    r.k = k;
    return D2D_OK;
}

int d2d_get_strongest_paths(d2d_ctx* c, float* power, float* length, int32_t* cand, int32_t* order, float* total, int32_t* count) {
    if (int rc = result_state(c, c && c->top.k >= 1 && c->top.power.p, TOP)) return rc;
    const d2d_ctx::Top& r = c->top;
    const size_t cells = (size_t)c->m * (size_t)c->n, kc = (size_t)r.k * cells;
    return copy_out(c, {{power, r.power.p, kc * sizeof(float)}, {length, r.len.p, kc * sizeof(float)}, {cand, r.cand.p, kc * D2D_MAX_ORDER * sizeof(int)},
                        {order, r.order.p, kc * sizeof(int)}, {total, r.total.p, cells * sizeof(float)}, {count, r.count.p, cells * sizeof(int)}});
}

// Coherent-field build: ONE pass, every lane writing the three values of its cell (no zeroing in front).
int d2d_coherent_field_launch(d2d_ctx* c, const d2d_params* p, const float* fixed, float inv_wavelength, int32_t amplitude) {
    if (!c || !fixed) return fail(D2D_ERR_INVALID, "NULL argument");
    SinkLaunch<d2d_ctx::Field> L(c, FIELD, c->field, fixed);
    d2d_ctx::Planes& o = c->field.out;
    std::string err;
    int rc;
    if ((rc = L.begin(p))) return rc;
    if ((rc = d2d_host::field_params(inv_wavelength, amplitude, err))) return fail(rc, "d2d_coherent_field_launch: %s", err.c_str());
    if ((rc = L.device()) || (rc = L.fits(d2d_host::FIELD_BYTES_PER_CELL, o.bytes())) || (rc = L.prepare()) || (rc = o.ensure(L.cells, L.cells))) return rc;
    d2d::FieldArgs f;
    f.re = o.re.p;
    f.im = o.im.p;
    f.total = o.total.p;
    f.cells = (long)L.cells;
    f.inv_wavelength = inv_wavelength;
    f.amplitude = amplitude;
    if (L.s.tiles > 0) HIP_TRY(L.pass<d2d::FieldSink>(f));
    c->field.have = true;
    return D2D_OK;
}

int d2d_get_coherent_field(d2d_ctx* c, float* re, float* im, float* total) {
    if (int rc = result_state(c, c && c->field.have && c->field.out.re.p, FIELD)) return rc;
    const d2d_ctx::Planes& o = c->field.out;
    const size_t bytes = (size_t)c->m * (size_t)c->n * sizeof(float);
    return copy_out(c, {{re, o.re.p, bytes}, {im, o.im.p, bytes}, {total, o.total.p, bytes}});
}

// Frequency-response build: ONE preparation, then one pass per chunk of FREQ_CHUNK wavelengths over the same SweepArgs (as
// d2d_valid_paths launches its two passes: the sink kernel writes nothing that a later pass reads), every lane writing its cell's
// planes of the chunk and, in the first pass, the total.
int d2d_frequency_response_launch(d2d_ctx* c, const d2d_params* p, const float* fixed, const float* inv_wavelength, int32_t nf, int32_t amplitude) {
    if (!c || !fixed || !inv_wavelength) return fail(D2D_ERR_INVALID, "NULL argument");
    SinkLaunch<d2d_ctx::Freq> L(c, FREQ, c->freq, fixed);
    d2d_ctx::Planes& o = c->freq.out;
    std::string err;
    int rc;
    if ((rc = L.begin(p))) return rc;
    if ((rc = d2d_host::freq_params(inv_wavelength, nf, amplitude, err))) return fail(rc, "d2d_frequency_response_launch: %s", err.c_str());
    if ((rc = L.device()) || (rc = L.fits(d2d_host::freq_bytes_per_cell(nf), o.bytes())) || (rc = L.prepare()) || (rc = o.ensure((size_t)nf * L.cells, L.cells)))
        return rc;
    if (L.s.tiles > 0)
        for (int32_t i = 0; i < d2d_host::chunks(nf, d2d::FREQ_CHUNK); ++i) {
            const d2d_host::Chunk ch = d2d_host::chunk_plan(nf, i, d2d::FREQ_CHUNK);
            d2d::FreqArgs f;
            f.re = o.re.p + (size_t)ch.first * L.cells;
            f.im = o.im.p + (size_t)ch.first * L.cells;
            f.total = ch.with_total ? o.total.p : nullptr;
            f.cells = (long)L.cells;
            for (int32_t j = 0; j < d2d::FREQ_CHUNK; ++j) f.inv[j] = j < ch.count ? inv_wavelength[ch.first + j] : 0.0f;
            f.nf = ch.count;
            f.amplitude = amplitude;
            HIP_TRY(L.pass<d2d::FreqSink>(f));
        }
    c->freq.nf = nf;
    return D2D_OK;
}

int d2d_get_frequency_response(d2d_ctx* c, float* re, float* im, float* total) {
    if (int rc = result_state(c, c && c->freq.nf >= 1 && c->freq.out.re.p, FREQ)) return rc;
    const d2d_ctx::Planes& o = c->freq.out;
    const size_t bytes = (size_t)c->m * (size_t)c->n * sizeof(float);
    return copy_out(c, {{re, o.re.p, bytes * (size_t)c->freq.nf}, {im, o.im.p, bytes * (size_t)c->freq.nf}, {total, o.total.p, bytes}});
}

// Coefficient adjoint of the frequency response: ONE preparation of the culled sweep with the coefficient-free contribution
// valid / (h^2 + r^2) (D2D_FUN_RECEIVED_POWER with a numerator of 1, as d2d_valid_paths substitutes D2D_FUN_ONE), one pass per
// chunk of FREQ_CHUNK wavelengths into the zeroed per-patch rows, then the fixed-order fp64 reduction of the rows.  The cotangents
// are copied before the call returns.
int d2d_field_coefs_vjp_launch(d2d_ctx* c, const d2d_params* p, const float* fixed, const float* inv_wavelength, int32_t nf, int32_t amplitude,
                               const float* re_bar, const float* im_bar) {
    if (!c || !fixed || !inv_wavelength || !re_bar || !im_bar) return fail(D2D_ERR_INVALID, "NULL argument");
    SinkLaunch<d2d_ctx::CoefGrad> L(c, COEF_VJP, c->cg, fixed);
    d2d_ctx::CoefGrad& r = c->cg;
    std::string err;
    int rc;
    if ((rc = L.begin(p, [&] {
            if (p->fun_id == D2D_FUN_RECEIVED_POWER_PER_OBJECT) return (int)D2D_OK;
            return fail(D2D_ERR_UNSUPPORTED, "%s: fun_id %d has no reflection coefficient per object to differentiate by (D2D_FUN_RECEIVED_POWER_PER_OBJECT only)",
                        COEF_VJP.who, p->fun_id);
        })))
        return rc;
    if ((rc = d2d_host::freq_params(inv_wavelength, nf, amplitude, err))) return fail(rc, "%s: %s", COEF_VJP.who, err.c_str());
    if ((rc = L.device())) return rc;
    L.pp.fun_id = D2D_FUN_RECEIVED_POWER;  // with a numerator of 1: a contribution is then valid / (h^2 + r^2)
    L.pp.r_coef = 1.0f;
    const size_t cells = L.cells, N = (size_t)c->N, tiles = (size_t)L.s.tiles;
    if (!d2d_host::coef_vjp_fits(cells, nf, tiles, N, L.mem_free, (r.re.n + r.im.n + r.partial.n) * sizeof(float)))
        return fail(D2D_ERR_UNSUPPORTED, "%s: cotangents of %zu cells (%zu bytes per cell) and %zu rows of %zu partial sums exceed half of the free device memory (%zu bytes free)",
                    COEF_VJP.who, cells, 8 * (size_t)nf, tiles, N, L.mem_free);
    if ((rc = L.prepare())) return rc;
    const size_t planes = (size_t)nf * cells;
    if ((rc = r.re.ensure(planes)) || (rc = r.im.ensure(planes)) || (rc = r.partial.ensure(tiles * N)) || (rc = r.out.ensure(N))) return rc;
    HIP_TRY(hipMemcpyAsync(r.re.p, re_bar, planes * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(r.im.p, im_bar, planes * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // the caller's arrays are free again when the call returns
    if (N > 0 && tiles > 0) {
        HIP_TRY(hipMemsetAsync(r.partial.p, 0, tiles * N * sizeof(float), c->stream));
        for (int32_t i = 0; i < d2d_host::chunks(nf, d2d::FREQ_CHUNK); ++i) {
            const d2d_host::Chunk ch = d2d_host::chunk_plan(nf, i, d2d::FREQ_CHUNK);
            d2d::CoefGradArgs g;
            g.re_bar = r.re.p + (size_t)ch.first * cells;
            g.im_bar = r.im.p + (size_t)ch.first * cells;
            g.coef = c->d_coef.p;
            g.partial = r.partial.p;
            g.cells = (long)cells;
            for (int32_t j = 0; j < d2d::FREQ_CHUNK; ++j) g.inv[j] = j < ch.count ? inv_wavelength[ch.first + j] : 0.0f;
            g.nf = ch.count;
            g.amplitude = amplitude;
            g.N = c->N;
            HIP_TRY(L.pass<d2d::CoefGradSink>(g));
        }
        hipLaunchKernelGGL(d2d::vjp_reduce_kernel, dim3((unsigned)N), dim3(256), 0, c->stream, r.partial.p, (long)tiles, c->N, r.out.p, 0);
        HIP_TRY(hipGetLastError());
    } else {
        HIP_TRY(hipMemsetAsync(r.out.p, 0, (N ? N : 1) * sizeof(double), c->stream));
    }
    r.have = true;
    return D2D_OK;
}

int d2d_get_field_coefs_vjp(d2d_ctx* c, double* coef_bar) {
    if (int rc = result_state(c, c && c->have_scene && c->cg.have && c->cg.out.p, COEF_VJP, "result goes with the grid and the scene")) return rc;
    if (!coef_bar) return fail(D2D_ERR_INVALID, "coef_bar is NULL");
    return copy_out(c, {{coef_bar, c->cg.out.p, (size_t)c->N * sizeof(double)}});
}

// Position adjoint of the frequency response: ONE preparation of the culled sweep with the caller's own path function, one pass per
// block of POS_CHUNK wavelengths -- every lane carries its cell's four running values from pass to pass through the planes, the
// first pass starting from +0 -- then the fixed-order fp64 sums of the two fixed_terms planes.  The cotangents are copied before
// the call returns.
constexpr unsigned POS_REDUCE_BLOCKS = 1024;  // most partial sums per plane of the reduction's first stage
int d2d_field_position_vjp_launch(d2d_ctx* c, const d2d_params* p, const float* fixed, const float* inv_wavelength, int32_t nf, int32_t amplitude,
                                  const float* re_bar, const float* im_bar) {
    if (!c || !fixed || !inv_wavelength || !re_bar || !im_bar) return fail(D2D_ERR_INVALID, "NULL argument");
    SinkLaunch<d2d_ctx::PosGrad> L(c, POS_VJP, c->pg, fixed);
    d2d_ctx::PosGrad& r = c->pg;
    std::string err;
    int rc;
    if ((rc = L.begin(p, [&] {
            if (!p->approx) return (int)D2D_OK;
            return fail(D2D_ERR_UNSUPPORTED,
                        "%s covers hard validity only: a smoothed validity (hard_sigmoid, sigmoid) depends on the positions itself, and its term needs the "
                        "reverse chain of the value+grad sweep (d2d_power_map_vg_launch); a gradient without that term is not offered",
                        POS_VJP.who);
        })))
        return rc;
    if ((rc = d2d_host::posgrad_params(inv_wavelength, nf, amplitude, err))) return fail(rc, "%s: %s", POS_VJP.who, err.c_str());
    if ((rc = L.device()) || (rc = L.fits(d2d_host::posgrad_bytes_per_cell(nf), r.bytes())) || (rc = L.prepare())) return rc;
    const size_t cells = L.cells, planes = (size_t)nf * cells;
    const unsigned blocks = (unsigned)std::min<size_t>(POS_REDUCE_BLOCKS, std::max<size_t>(1, (cells + 255) / 256));
    if ((rc = r.re.ensure(planes)) || (rc = r.im.ensure(planes)) || (rc = r.cell.ensure(2 * cells)) || (rc = r.terms.ensure(2 * cells)) ||
        (rc = r.part.ensure(2 * (size_t)POS_REDUCE_BLOCKS)) || (rc = r.out.ensure(2)))
        return rc;
    HIP_TRY(hipMemcpyAsync(r.re.p, re_bar, planes * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(r.im.p, im_bar, planes * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // the caller's arrays are free again when the call returns
    if (L.s.tiles > 0 && cells > 0) {
        for (int32_t i = 0; i < d2d_host::chunks(nf, d2d::POS_CHUNK); ++i) {
            const d2d_host::Chunk ch = d2d_host::chunk_plan(nf, i, d2d::POS_CHUNK);
            d2d::PosGradArgs g;
            g.re_bar = r.re.p + (size_t)ch.first * cells;
            g.im_bar = r.im.p + (size_t)ch.first * cells;
            g.cell_bar = r.cell.p;
            g.fixed_terms = r.terms.p;
            g.cells = (long)cells;
            for (int32_t j = 0; j < d2d::POS_CHUNK; ++j) g.inv[j] = j < ch.count ? inv_wavelength[ch.first + j] : 0.0f;
            g.nf = ch.count;
            g.amplitude = amplitude;
            g.fun_id = L.pp.fun_id;
            g.h2 = L.s.a.h2;
            g.txg = L.s.txg ? 1 : 0;
            g.first = i == 0 ? 1 : 0;
            HIP_TRY(L.pass<d2d::PosGradSink>(g));
        }
        hipLaunchKernelGGL(d2d::plane_sum_kernel<float>, dim3(blocks, 2), dim3(256), 0, c->stream, r.terms.p, (long)cells, r.part.p);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(d2d::plane_sum_kernel<double>, dim3(1, 2), dim3(256), 0, c->stream, r.part.p, (long)blocks, r.out.p);
        HIP_TRY(hipGetLastError());
    } else {  // a sweep without contributions
        if (cells > 0) {
            HIP_TRY(hipMemsetAsync(r.cell.p, 0, 2 * cells * sizeof(float), c->stream));
            HIP_TRY(hipMemsetAsync(r.terms.p, 0, 2 * cells * sizeof(float), c->stream));
        }
        HIP_TRY(hipMemsetAsync(r.out.p, 0, 2 * sizeof(double), c->stream));
    }
    r.have = true;
    return D2D_OK;
}

int d2d_get_field_position_vjp(d2d_ctx* c, float* cell_bar, float* fixed_terms, double* fixed_bar) {
    if (int rc = result_state(c, c && c->have_scene && c->pg.have && c->pg.out.p, POS_VJP, "result goes with the grid and the scene")) return rc;
    const d2d_ctx::PosGrad& r = c->pg;
    const size_t bytes = 2 * (size_t)c->m * (size_t)c->n * sizeof(float);
    return copy_out(c, {{cell_bar, r.cell.p, bytes}, {fixed_terms, r.terms.p, bytes}, {fixed_bar, r.out.p, 2 * sizeof(double)}});
}

// Wall adjoint of the frequency response: ONE preparation of the culled sweep with the caller's own path function, one pass per
// block of POS_CHUNK wavelengths into the per-patch rows -- zeroed in front of the first pass, carried from pass to pass -- then the
// fixed-order fp64 reduction of the rows.  The cotangents are copied before the call returns.
int d2d_field_walls_vjp_launch(d2d_ctx* c, const d2d_params* p, const float* fixed, const float* inv_wavelength, int32_t nf, int32_t amplitude,
                               const float* re_bar, const float* im_bar) {
    if (!c || !fixed || !inv_wavelength || !re_bar || !im_bar) return fail(D2D_ERR_INVALID, "NULL argument");
    SinkLaunch<d2d_ctx::WallGrad> L(c, WALL_VJP, c->wg, fixed);
    d2d_ctx::WallGrad& r = c->wg;
    std::string err;
    int rc;
    if ((rc = L.begin(p, [&] {
            if (!p->approx) return (int)D2D_OK;
            return fail(D2D_ERR_UNSUPPORTED,
                        "%s covers hard validity only: a smoothed validity (hard_sigmoid, sigmoid) depends on the walls' end points itself, and its term needs "
                        "the reverse chain of the value+grad sweep (d2d_power_map_vg_launch); a gradient without that term is not offered",
                        WALL_VJP.who);
        })))
        return rc;
    if ((rc = d2d_host::wallgrad_params(inv_wavelength, nf, amplitude, err))) return fail(rc, "%s: %s", WALL_VJP.who, err.c_str());
    if ((rc = L.device())) return rc;
    const size_t cells = L.cells, N = (size_t)c->N, tiles = (size_t)L.s.tiles;
    if (!d2d_host::wall_vjp_fits(cells, nf, tiles, N, L.mem_free, r.bytes()))
        return fail(D2D_ERR_UNSUPPORTED, "%s: cotangents of %zu cells (%zu bytes per cell) and %zu rows of %zu pairs of partial sums exceed half of the free device memory (%zu bytes free)",
                    WALL_VJP.who, cells, 8 * (size_t)nf, tiles, N, L.mem_free);
    if ((rc = L.prepare())) return rc;
    const size_t planes = (size_t)nf * cells, row = 2 * N;
    if ((rc = r.re.ensure(planes)) || (rc = r.im.ensure(planes)) || (rc = r.partial.ensure(tiles * row)) || (rc = r.out.ensure(row))) return rc;
    HIP_TRY(hipMemcpyAsync(r.re.p, re_bar, planes * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(r.im.p, im_bar, planes * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // the caller's arrays are free again when the call returns
    if (N > 0 && tiles > 0 && cells > 0) {
        HIP_TRY(hipMemsetAsync(r.partial.p, 0, tiles * row * sizeof(float), c->stream));
        for (int32_t i = 0; i < d2d_host::chunks(nf, d2d::POS_CHUNK); ++i) {
            const d2d_host::Chunk ch = d2d_host::chunk_plan(nf, i, d2d::POS_CHUNK);
            d2d::WallGradArgs g;
            g.re_bar = r.re.p + (size_t)ch.first * cells;
            g.im_bar = r.im.p + (size_t)ch.first * cells;
            g.refl = c->d_refl.p;
            g.X = c->d_X.p;
            g.Y = c->d_Y.p;
            g.partial = r.partial.p;
            g.cells = (long)cells;
            for (int32_t j = 0; j < d2d::POS_CHUNK; ++j) g.inv[j] = j < ch.count ? inv_wavelength[ch.first + j] : 0.0f;
            g.nf = ch.count;
            g.N = c->N;
            g.amplitude = amplitude;
            g.fun_id = L.pp.fun_id;
            g.h2 = L.s.a.h2;
            g.txg = L.s.txg ? 1 : 0;
            g.fx = fixed[0];
            g.fy = fixed[1];
            HIP_TRY(L.pass<d2d::WallGradSink>(g));
        }
        hipLaunchKernelGGL(d2d::vjp_reduce_kernel, dim3((unsigned)row), dim3(256), 0, c->stream, r.partial.p, (long)tiles, (int)row, r.out.p, 0);
        HIP_TRY(hipGetLastError());
    } else {  // a sweep without a patch, or a scene without walls
        HIP_TRY(hipMemsetAsync(r.out.p, 0, (row ? row : 1) * sizeof(double), c->stream));
    }
    r.have = true;
    return D2D_OK;
}

int d2d_get_field_walls_vjp(d2d_ctx* c, double* walls_bar, double* normal_bar) {
    if (int rc = result_state(c, c && c->have_scene && c->wg.have && c->wg.out.p, WALL_VJP, "result goes with the grid and the scene")) return rc;
    const size_t N = (size_t)c->N;
    if (N == 0 || (!walls_bar && !normal_bar)) return copy_out(c, {});
    // normal_bar, then walls_bar[w][e][d] = normal_bar[w][e] * (double)n_w[d] + 0.0 from the fp32 normals of the device's wall table
    std::vector<double> nb(2 * N);
    std::vector<float4> refl(walls_bar ? 2 * N : 0);
    if (int rc = copy_out(c, {{nb.data(), c->wg.out.p, 2 * N * sizeof(double)}, {walls_bar ? refl.data() : nullptr, c->d_refl.p, 2 * N * sizeof(float4)}})) return rc;
    if (normal_bar) memcpy(normal_bar, nb.data(), 2 * N * sizeof(double));
    if (walls_bar)
        for (size_t w = 0; w < N; ++w)
            for (int e = 0; e < 2; ++e) {
                walls_bar[4 * w + 2 * e] = nb[2 * w + e] * (double)refl[2 * w].z + 0.0;  // (+ 0.0: a zero product is +0.0)
                walls_bar[4 * w + 2 * e + 1] = nb[2 * w + e] * (double)refl[2 * w].w + 0.0;
            }
    return D2D_OK;
}

// Power-angle build: ONE pass into the zeroed planes, every lane storing its cell's total at the end.
int d2d_power_angle_launch(d2d_ctx* c, const d2d_params* p, const float* fixed, int32_t end, float origin, int32_t nbins) {
    if (!c || !fixed) return fail(D2D_ERR_INVALID, "NULL argument");
    SinkLaunch<d2d_ctx::Angle> L(c, ANGLE, c->angle, fixed);
    d2d_ctx::Angle& r = c->angle;
    std::string err;
    int rc;
    if ((rc = L.begin(p))) return rc;
    if ((rc = d2d_host::angle_params(end, origin, nbins, err))) return fail(rc, "d2d_power_angle_launch: %s", err.c_str());
    if ((rc = L.device()) || (rc = L.fits(d2d_host::angle_bytes_per_cell(nbins), (r.out.n + r.total.n) * sizeof(float))) || (rc = L.prepare())) return rc;
    const size_t planes = (size_t)nbins * L.cells;
    if ((rc = r.out.ensure(planes)) || (rc = r.total.ensure(L.cells))) return rc;
    d2d::AngleArgs g;
    g.out = r.out.p;
    g.total = r.total.p;
    g.cells = (long)L.cells;
    g.origin = origin;
    g.nbins = nbins;
    g.end = end;
    HIP_TRY(hipMemsetAsync(r.out.p, 0, planes * sizeof(float), c->stream));
    if (L.s.tiles > 0) HIP_TRY(L.pass<d2d::AngleSink>(g));
    else HIP_TRY(hipMemsetAsync(r.total.p, 0, L.cells * sizeof(float), c->stream));
    r.nbins = nbins;
    return D2D_OK;
}

int d2d_get_power_angle(d2d_ctx* c, float* out, float* total) {
    if (int rc = result_state(c, c && c->angle.nbins >= 1 && c->angle.out.p, ANGLE)) return rc;
    const size_t bytes = (size_t)c->m * (size_t)c->n * sizeof(float);
    return copy_out(c, {{out, c->angle.out.p, bytes * (size_t)c->angle.nbins}, {total, c->angle.total.p, bytes}});
}

// Array-response build: ONE pass into the zeroed planes, every lane storing its cell's total at the end.
int d2d_array_response_launch(d2d_ctx* c, const d2d_params* p, const float* fixed, float inv_wavelength, int32_t amplitude, int32_t nt,
                              const float* tx_elems, int32_t nr, const float* rx_elems) {
    if (!c || !fixed || !tx_elems || !rx_elems) return fail(D2D_ERR_INVALID, "NULL argument");
    SinkLaunch<d2d_ctx::Array> L(c, ARRAY, c->array, fixed);
    d2d_ctx::Planes& o = c->array.out;
    std::string err;
    int rc;
    if ((rc = L.begin(p))) return rc;
    if ((rc = d2d_host::array_params(nt, tx_elems, nr, rx_elems, inv_wavelength, amplitude, err))) return fail(rc, "d2d_array_response_launch: %s", err.c_str());
    const size_t planes = (size_t)nr * (size_t)nt * L.cells;
    if ((rc = L.device()) || (rc = L.fits(d2d_host::array_bytes_per_cell(nt, nr), o.bytes())) || (rc = L.prepare()) || (rc = o.ensure(planes, L.cells))) return rc;
    d2d::ArrayArgs g = {};
    g.re = o.re.p;
    g.im = o.im.p;
    g.total = o.total.p;
    g.cells = (long)L.cells;
    g.inv_wavelength = inv_wavelength;
    g.amplitude = amplitude;
    g.nt = nt;
    g.nr = nr;
    for (int32_t j = 0; j < nt; ++j) g.etx[j][0] = tx_elems[2 * j], g.etx[j][1] = tx_elems[2 * j + 1];
    for (int32_t i = 0; i < nr; ++i) g.erx[i][0] = rx_elems[2 * i], g.erx[i][1] = rx_elems[2 * i + 1];
    HIP_TRY(hipMemsetAsync(o.re.p, 0, planes * sizeof(float), c->stream));
    HIP_TRY(hipMemsetAsync(o.im.p, 0, planes * sizeof(float), c->stream));
    if (L.s.tiles > 0) HIP_TRY(L.pass<d2d::ArraySink>(g));
    else HIP_TRY(hipMemsetAsync(o.total.p, 0, L.cells * sizeof(float), c->stream));
    c->array.nt = nt;
    c->array.nr = nr;
    return D2D_OK;
}

int d2d_get_array_response(d2d_ctx* c, float* re, float* im, float* total) {
    if (int rc = result_state(c, c && c->array.nt >= 1 && c->array.nr >= 1 && c->array.out.re.p, ARRAY)) return rc;
    const d2d_ctx::Planes& o = c->array.out;
    const size_t bytes = (size_t)c->m * (size_t)c->n * sizeof(float), pairs = (size_t)c->array.nt * (size_t)c->array.nr;
    return copy_out(c, {{re, o.re.p, bytes * pairs}, {im, o.im.p, bytes * pairs}, {total, o.total.p, bytes}});
}

// Wideband array-response build: ONE preparation, then one pass per chunk of WIDE_CHUNK wavelengths over the same SweepArgs (as
// d2d_frequency_response_launch does), every pass adding into the zeroed plane blocks of its chunk and the first storing the total.
int d2d_array_frequency_response_launch(d2d_ctx* c, const d2d_params* p, const float* fixed, const float* inv_wavelength, int32_t nf, int32_t amplitude,
                                        int32_t nt, const float* tx_elems, int32_t nr, const float* rx_elems) {
    if (!c || !fixed || !inv_wavelength || !tx_elems || !rx_elems) return fail(D2D_ERR_INVALID, "NULL argument");
    SinkLaunch<d2d_ctx::Wide> L(c, WIDE, c->wide, fixed);
    d2d_ctx::Planes& o = c->wide.out;
    std::string err;
    int rc;
    if ((rc = L.begin(p))) return rc;
    if ((rc = d2d_host::wide_params(inv_wavelength, nf, amplitude, nt, tx_elems, nr, rx_elems, err))) return fail(rc, "%s: %s", WIDE.who, err.c_str());
    const size_t block = (size_t)nr * (size_t)nt * L.cells;  // one wavelength's planes
    const size_t planes = (size_t)nf * block;
    if ((rc = L.device()) || (rc = L.fits(d2d_host::wide_bytes_per_cell(nf, nt, nr), o.bytes())) || (rc = L.prepare()) || (rc = o.ensure(planes, L.cells))) return rc;
    HIP_TRY(hipMemsetAsync(o.re.p, 0, planes * sizeof(float), c->stream));
    HIP_TRY(hipMemsetAsync(o.im.p, 0, planes * sizeof(float), c->stream));
    if (L.s.tiles > 0)
        for (int32_t i = 0; i < d2d_host::chunks(nf, d2d::WIDE_CHUNK); ++i) {
            const d2d_host::Chunk ch = d2d_host::chunk_plan(nf, i, d2d::WIDE_CHUNK);
            d2d::ArrayFreqArgs g = {};
            g.re = o.re.p + (size_t)ch.first * block;
            g.im = o.im.p + (size_t)ch.first * block;
            g.total = ch.with_total ? o.total.p : nullptr;
            g.cells = (long)L.cells;
            g.amplitude = amplitude;
            g.nf = ch.count;
            g.nt = nt;
            g.nr = nr;
            for (int32_t f = 0; f < ch.count; ++f) g.inv[f] = inv_wavelength[ch.first + f];
            for (int32_t j = 0; j < nt; ++j) g.etx[j][0] = tx_elems[2 * j], g.etx[j][1] = tx_elems[2 * j + 1];
            for (int32_t k = 0; k < nr; ++k) g.erx[k][0] = rx_elems[2 * k], g.erx[k][1] = rx_elems[2 * k + 1];
            HIP_TRY(L.pass<d2d::ArrayFreqSink>(g));
        }
    else HIP_TRY(hipMemsetAsync(o.total.p, 0, L.cells * sizeof(float), c->stream));
    c->wide.nf = nf;
    c->wide.nt = nt;
    c->wide.nr = nr;
    return D2D_OK;
}

int d2d_get_array_frequency_response(d2d_ctx* c, int32_t first, int32_t count, float* re, float* im, float* total) {
    if (int rc = result_state(c, c && c->wide.nf >= 1 && c->wide.out.re.p, WIDE)) return rc;
    if (first < 0 || count < 1 || count > c->wide.nf - first)
        return fail(D2D_ERR_INVALID, "d2d_get_array_frequency_response: first %d and count %d are no range of the result's %d wavelengths", first, count, c->wide.nf);
    const d2d_ctx::Planes& o = c->wide.out;
    const size_t cells = (size_t)c->m * (size_t)c->n, block = (size_t)c->wide.nr * (size_t)c->wide.nt * cells;
    const size_t bytes = (size_t)count * block * sizeof(float);
    return copy_out(c, {{re, o.re.p + (size_t)first * block, bytes}, {im, o.im.p + (size_t)first * block, bytes}, {total, o.total.p, cells * sizeof(float)}});
}

// Beam-response build: ONE preparation, then one pass per chunk of BEAM_CHUNK wavelengths over the same SweepArgs (as
// d2d_array_frequency_response_launch does), every pass adding into the zeroed plane blocks of its chunk and the first storing the
// total.  The lists travel by value in the kernel argument, the two weight tables in a device buffer of the result (copied from the
// caller's during the call).
int d2d_beam_response_launch(d2d_ctx* c, const d2d_params* p, const float* fixed, const float* inv_wavelength, int32_t nf, int32_t amplitude, int32_t nt,
                             const float* tx_elems, int32_t nr, const float* rx_elems, int32_t nbt, const float* tx_weights, int32_t nbr,
                             const float* rx_weights) {
    if (!c || !fixed || !inv_wavelength || !tx_elems || !rx_elems || !tx_weights || !rx_weights) return fail(D2D_ERR_INVALID, "NULL argument");
    SinkLaunch<d2d_ctx::Beam> L(c, BEAM, c->beam, fixed);
    d2d_ctx::Planes& o = c->beam.out;
    std::string err;
    int rc;
    if ((rc = L.begin(p))) return rc;
    if ((rc = d2d_host::beam_params(inv_wavelength, nf, amplitude, nt, tx_elems, nr, rx_elems, nbt, tx_weights, nbr, rx_weights, err)))
        return fail(rc, "%s: %s", BEAM.who, err.c_str());
    const size_t block = (size_t)nbr * (size_t)nbt * L.cells;  // one wavelength's planes
    const size_t planes = (size_t)nf * block;
    if ((rc = L.device()) || (rc = L.fits(d2d_host::beam_bytes_per_cell(nf, nbt, nbr), o.bytes())) || (rc = L.prepare()) || (rc = o.ensure(planes, L.cells)) ||
        (rc = c->beam.w.ensure(2 * d2d::BEAM_TABLE)))
        return rc;
    // the two weight tables, padded to the limits, behind whatever pass still reads the previous launch's
    float w[2 * d2d::BEAM_TABLE] = {};
    for (int32_t b = 0; b < nbt; ++b)
        for (int32_t j = 0; j < 2 * nt; ++j) w[b * 2 * d2d::ARRAY_MAX + j] = tx_weights[b * 2 * nt + j];
    for (int32_t b = 0; b < nbr; ++b)
        for (int32_t k = 0; k < 2 * nr; ++k) w[d2d::BEAM_TABLE + b * 2 * d2d::ARRAY_MAX + k] = rx_weights[b * 2 * nr + k];
    HIP_TRY(hipMemcpyAsync(c->beam.w.p, w, sizeof w, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(o.re.p, 0, planes * sizeof(float), c->stream));
    HIP_TRY(hipMemsetAsync(o.im.p, 0, planes * sizeof(float), c->stream));
    if (L.s.tiles > 0)
        for (int32_t i = 0; i < d2d_host::chunks(nf, d2d::BEAM_CHUNK); ++i) {
            const d2d_host::Chunk ch = d2d_host::chunk_plan(nf, i, d2d::BEAM_CHUNK);
            d2d::BeamArgs g = {};
            g.re = o.re.p + (size_t)ch.first * block;
            g.im = o.im.p + (size_t)ch.first * block;
            g.total = ch.with_total ? o.total.p : nullptr;
            g.cells = (long)L.cells;
            g.amplitude = amplitude;
            g.nf = ch.count;
            g.nt = nt;
            g.nr = nr;
            g.nbt = nbt;
            g.nbr = nbr;
            for (int32_t f = 0; f < ch.count; ++f) g.inv[f] = inv_wavelength[ch.first + f];
            for (int32_t j = 0; j < nt; ++j) g.etx[j][0] = tx_elems[2 * j], g.etx[j][1] = tx_elems[2 * j + 1];
            for (int32_t k = 0; k < nr; ++k) g.erx[k][0] = rx_elems[2 * k], g.erx[k][1] = rx_elems[2 * k + 1];
            g.w = c->beam.w.p;
            HIP_TRY(L.pass<d2d::BeamSink>(g));
        }
    // (No patch at all: as in the siblings above, what a sweep without contributions would leave.  d2d_set_grid refuses a grid of
    // less than 1 x 1, so tiles == 0 cannot arise today and no test reaches this line; it stands for a context that ever holds an
    // empty share of a grid.)
    else HIP_TRY(hipMemsetAsync(o.total.p, 0, L.cells * sizeof(float), c->stream));
    c->beam.nf = nf;
    c->beam.nbt = nbt;
    c->beam.nbr = nbr;
    return D2D_OK;
}

int d2d_get_beam_response(d2d_ctx* c, int32_t first, int32_t count, float* re, float* im, float* total) {
    if (int rc = result_state(c, c && c->beam.nf >= 1 && c->beam.out.re.p, BEAM)) return rc;
    if (first < 0 || count < 1 || count > c->beam.nf - first)
        return fail(D2D_ERR_INVALID, "d2d_get_beam_response: first %d and count %d are no range of the result's %d wavelengths", first, count, c->beam.nf);
    const d2d_ctx::Planes& o = c->beam.out;
    const size_t cells = (size_t)c->m * (size_t)c->n, block = (size_t)c->beam.nbr * (size_t)c->beam.nbt * cells;
    const size_t bytes = (size_t)count * block * sizeof(float);
    return copy_out(c, {{re, o.re.p + (size_t)first * block, bytes}, {im, o.im.p + (size_t)first * block, bytes}, {total, o.total.p, cells * sizeof(float)}});
}

// Material-response build: ONE preparation, then one pass per chunk of MAT_CHUNK wavelengths over the same SweepArgs (as
// d2d_frequency_response_launch does), every lane writing its cell's planes of the chunk and, in the first pass, the total.  The
// permittivity table lives in a device buffer of the result, copied from the caller's during the call and uploaded on the stream in
// front of the passes; the wall normals are the context's own table.
int d2d_material_response_launch(d2d_ctx* c, const d2d_params* p, const float* fixed, const float* inv_wavelength, int32_t nf, int32_t amplitude,
                                 int32_t polarization, const float* eps, int32_t n_objects) {
    if (!c || !fixed || !inv_wavelength || !eps) return fail(D2D_ERR_INVALID, "NULL argument");
    SinkLaunch<d2d_ctx::Material> L(c, MATERIAL, c->mat, fixed);
    d2d_ctx::Planes& o = c->mat.out;
    std::string err;
    int rc;
    if ((rc = L.begin(p))) return rc;
    if ((rc = d2d_host::material_params(inv_wavelength, nf, amplitude, polarization, eps, n_objects, c->N, err))) return fail(rc, "%s: %s", MATERIAL.who, err.c_str());
    if ((rc = L.device())) return rc;
    if (!d2d_host::material_fits(L.cells, nf, (size_t)n_objects, L.mem_free, c->mat.bytes()))
        return fail(D2D_ERR_UNSUPPORTED, "%s: %zu cells (%zu bytes per cell) and a table of %zu bytes exceed half of the free device memory (%zu bytes free)",
                    MATERIAL.who, L.cells, d2d_host::freq_bytes_per_cell(nf), 8 * (size_t)nf * (size_t)n_objects, L.mem_free);
    const size_t table = 2 * (size_t)nf * (size_t)n_objects;  // floats
    if ((rc = L.prepare()) || (rc = o.ensure((size_t)nf * L.cells, L.cells)) || (rc = c->mat.eps.ensure(table + 2))) return rc;
    const bool constant = d2d_host::material_constant_band(eps, nf, n_objects);
    // behind whatever pass still reads the previous launch's table (the copy leaves the caller's memory during the call: pageable)
    if (table > 0) HIP_TRY(hipMemcpyAsync(c->mat.eps.p, eps, table * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (L.s.tiles > 0)
        for (int32_t i = 0; i < d2d_host::chunks(nf, d2d::MAT_CHUNK); ++i) {
            const d2d_host::Chunk ch = d2d_host::chunk_plan(nf, i, d2d::MAT_CHUNK);
            d2d::MaterialArgs g = {};
            g.re = o.re.p + (size_t)ch.first * L.cells;
            g.im = o.im.p + (size_t)ch.first * L.cells;
            g.total = ch.with_total ? o.total.p : nullptr;
            g.cells = (long)L.cells;
            g.refl = c->d_refl.p;
            g.eps = c->mat.eps.p + (size_t)ch.first * 2 * (size_t)n_objects;
            for (int32_t j = 0; j < ch.count; ++j) g.inv[j] = inv_wavelength[ch.first + j];
            g.nf = ch.count;
            g.N = n_objects;
            g.amplitude = amplitude;
            g.pol = polarization;
            g.constant = constant ? 1 : 0;
            HIP_TRY(L.pass<d2d::MaterialSink>(g));
        }
    c->mat.nf = nf;
    return D2D_OK;
}

int d2d_get_material_response(d2d_ctx* c, float* re, float* im, float* total) {
    if (int rc = result_state(c, c && c->mat.nf >= 1 && c->mat.out.re.p, MATERIAL, "result goes with the grid and the scene")) return rc;
    const d2d_ctx::Planes& o = c->mat.out;
    const size_t bytes = (size_t)c->m * (size_t)c->n * sizeof(float);
    return copy_out(c, {{re, o.re.p, bytes * (size_t)c->mat.nf}, {im, o.im.p, bytes * (size_t)c->mat.nf}, {total, o.total.p, bytes}});
}

// Permittivity adjoint of the material response: d2d_material_response_launch's front half (the same parameter checks, the table
// copied during the call) and d2d_field_coefs_vjp_launch's back half (the cotangents copied before the call returns, per-patch rows,
// the fixed-order fp64 reduction).  Per chunk of MAT_CHUNK wavelengths: zero the rows, one pass, one reduction of the chunk's
// count * N * 2 entries (the rows keep the stride of a full chunk) into the chunk's rows of the result.  Any fused fun: the
// amplitude does not depend on eps.
int d2d_material_eps_vjp_launch(d2d_ctx* c, const d2d_params* p, const float* fixed, const float* inv_wavelength, int32_t nf, int32_t amplitude,
                                int32_t polarization, const float* eps, int32_t n_objects, const float* re_bar, const float* im_bar) {
    if (!c || !fixed || !inv_wavelength || !eps || !re_bar || !im_bar) return fail(D2D_ERR_INVALID, "NULL argument");
    SinkLaunch<d2d_ctx::EpsGrad> L(c, EPS_VJP, c->eg, fixed);
    d2d_ctx::EpsGrad& r = c->eg;
    std::string err;
    int rc;
    if ((rc = L.begin(p))) return rc;
    if ((rc = d2d_host::material_params(inv_wavelength, nf, amplitude, polarization, eps, n_objects, c->N, err))) return fail(rc, "%s: %s", EPS_VJP.who, err.c_str());
    if ((rc = L.device())) return rc;
    const size_t cells = L.cells, N = (size_t)n_objects, tiles = (size_t)L.s.tiles;
    if (!d2d_host::eps_vjp_fits(cells, nf, tiles, N, L.mem_free, r.bytes()))
        return fail(D2D_ERR_UNSUPPORTED, "%s: cotangents of %zu cells (%zu bytes per cell), a table and a result of %zu bytes and %zu rows of %zu partial sums exceed half of the free device memory (%zu bytes free)",
                    EPS_VJP.who, cells, 8 * (size_t)nf, 24 * (size_t)nf * N, tiles, (size_t)d2d::MAT_CHUNK * 2 * N, L.mem_free);
    if ((rc = L.prepare())) return rc;
    const size_t planes = (size_t)nf * cells, table = 2 * (size_t)nf * N, chunk_row = (size_t)d2d::MAT_CHUNK * 2 * N;
    if ((rc = r.re.ensure(planes)) || (rc = r.im.ensure(planes)) || (rc = r.eps.ensure(table + 2)) || (rc = r.partial.ensure(tiles * chunk_row)) ||
        (rc = r.out.ensure(table)))
        return rc;
    const bool constant = d2d_host::material_constant_band(eps, nf, n_objects);
    HIP_TRY(hipMemcpyAsync(r.re.p, re_bar, planes * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(r.im.p, im_bar, planes * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (table > 0) HIP_TRY(hipMemcpyAsync(r.eps.p, eps, table * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // the caller's arrays are free again when the call returns
    if (N > 0 && tiles > 0) {
        for (int32_t i = 0; i < d2d_host::chunks(nf, d2d::MAT_CHUNK); ++i) {
            const d2d_host::Chunk ch = d2d_host::chunk_plan(nf, i, d2d::MAT_CHUNK);
            d2d::EpsGradArgs g = {};
            g.re_bar = r.re.p + (size_t)ch.first * cells;
            g.im_bar = r.im.p + (size_t)ch.first * cells;
            g.eps = r.eps.p + (size_t)ch.first * 2 * N;
            g.refl = c->d_refl.p;
            g.partial = r.partial.p;
            g.cells = (long)cells;
            for (int32_t j = 0; j < ch.count; ++j) g.inv[j] = inv_wavelength[ch.first + j];
            g.nf = ch.count;
            g.N = n_objects;
            g.amplitude = amplitude;
            g.pol = polarization;
            g.constant = constant ? 1 : 0;
            HIP_TRY(hipMemsetAsync(r.partial.p, 0, tiles * chunk_row * sizeof(float), c->stream));
            HIP_TRY(L.pass<d2d::EpsGradSink>(g));
            // (n_elem is the stride between rows: a full chunk's, whatever this chunk's count)
            hipLaunchKernelGGL(d2d::vjp_reduce_kernel, dim3((unsigned)((size_t)ch.count * 2 * N)), dim3(256), 0, c->stream, r.partial.p, (long)tiles, (int)chunk_row,
                               r.out.p + (size_t)ch.first * 2 * N, 0);
            HIP_TRY(hipGetLastError());
        }
    } else {
        HIP_TRY(hipMemsetAsync(r.out.p, 0, (table ? table : 1) * sizeof(double), c->stream));
    }
    r.nf = nf;
    return D2D_OK;
}

int d2d_get_material_eps_vjp(d2d_ctx* c, double* eps_bar) {
    if (int rc = result_state(c, c && c->have_scene && c->eg.nf >= 1 && c->eg.out.p, EPS_VJP, "result goes with the grid and the scene")) return rc;
    if (!eps_bar) return fail(D2D_ERR_INVALID, "eps_bar is NULL");
    return copy_out(c, {{eps_bar, c->eg.out.p, (size_t)c->eg.nf * 2 * (size_t)c->N * sizeof(double)}});
}

int d2d_valid_paths(d2d_ctx* c, const d2d_params* p, const float* fixed, int64_t* count) { return valid_paths(c, p, fixed, count); }

int d2d_get_valid_paths(d2d_ctx* c, int64_t capacity, int32_t* cell, int32_t* cand, int32_t* order, float* xys, float* loss, float* valid,
                        float* length) {
    if (!c) return fail(D2D_ERR_INVALID, "ctx is NULL");
    if (c->rec_n < 0) return fail(D2D_ERR_STATE, "d2d_valid_paths must come first (its records go with the grid)");
    if (capacity < c->rec_n) return fail(D2D_ERR_INVALID, "capacity %lld is less than the %lld records held", (long long)capacity, c->rec_n);
    const size_t n = (size_t)c->rec_n;
    if (n == 0) return D2D_OK;
    constexpr size_t NPTS = D2D_MAX_ORDER + 2;
    return copy_out(c, {{cell, c->d_rec_cell.p, n * sizeof(int)}, {cand, c->d_rec_cand.p, n * D2D_MAX_ORDER * sizeof(int)}, {order, c->d_rec_order.p, n * sizeof(int)},
                        {xys, c->d_rec_xys.p, n * NPTS * 2 * sizeof(float)}, {loss, c->d_rec_loss.p, n * sizeof(float)}, {valid, c->d_rec_valid.p, n * sizeof(float)},
                        {length, c->d_rec_len.p, n * sizeof(float)}});
}

int d2d_debug_valid_paths_ms(d2d_ctx* c, float* ms) {
    if (!c || !ms) return fail(D2D_ERR_INVALID, "NULL argument");
    if (!c->have_rec_time) return fail(D2D_ERR_STATE, "no timed d2d_valid_paths yet (set the \"time_kernel\" option; a call without records has no pass 2)");
    HIP_TRY(hipEventElapsedTime(&ms[0], c->ev_rec[0], c->ev_rec[1]));
    HIP_TRY(hipEventElapsedTime(&ms[1], c->ev_rec[2], c->ev_rec[3]));
    HIP_TRY(hipEventElapsedTime(&ms[2], c->ev_rec[4], c->ev_rec[5]));
    return D2D_OK;
}

int d2d_power_map_launch(d2d_ctx* c, const d2d_params* p, const float* tx) { return sweep_launch(c, p, tx, nullptr); }

int d2d_set_cotangent(d2d_ctx* c, const float* cot) {
    if (!c) return fail(D2D_ERR_INVALID, "ctx is NULL");
    if (!c->have_grid) return fail(D2D_ERR_STATE, "d2d_set_grid must come first");
    int rc = set_device(c);
    if (rc) return rc;
    if (!cot) {
        c->have_cot = false;
        return D2D_OK;
    }
    const size_t cells = (size_t)c->m * c->n;
    if ((rc = c->d_cot.ensure(cells))) return rc;
    HIP_TRY(hipMemcpyAsync(c->d_cot.p, cot, cells * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->have_cot = true;
    return D2D_OK;
}

int d2d_set_path_fun_values(d2d_ctx* c, const float* f, const float* xys_bar, int64_t n_candidates) {
    if (!c) return fail(D2D_ERR_INVALID, "ctx is NULL");
    if (!c->have_grid) return fail(D2D_ERR_STATE, "d2d_set_grid must come first");
    if (!f || !xys_bar || n_candidates <= 0) {
        c->cust_C = -1;
        return (f || xys_bar || n_candidates > 0) ? fail(D2D_ERR_INVALID, "f, xys_bar and n_candidates > 0 go together") : D2D_OK;
    }
    int rc = set_device(c);
    if (rc) return rc;
    const size_t rows = (size_t)n_candidates * (size_t)c->m * (size_t)c->n;
    const size_t np2 = 2 * (size_t)(D2D_MAX_ORDER + 2);
    c->cust_C = -1;
    if ((rc = c->d_cust_f.ensure(rows))) return rc;
    if ((rc = c->d_cust_pb.ensure(rows * np2))) return rc;
    HIP_TRY(hipMemcpyAsync(c->d_cust_f.p, f, rows * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_cust_pb.p, xys_bar, rows * np2 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->cust_C = n_candidates;
    return D2D_OK;
}

int d2d_power_map_vg_launch(d2d_ctx* c, const d2d_params* p, const float* tx, int32_t want_scene_vjp) {
    return sweep_launch(c, p, tx, nullptr, want_scene_vjp ? 2 : 1);
}

int d2d_get_grad_rx(d2d_ctx* c, float* out) {
    if (!c || !out) return fail(D2D_ERR_INVALID, "NULL argument");
    if (!c->have_grid || !c->have_grad) return fail(D2D_ERR_STATE, "no value+grad sweep has run on this grid");
    int rc = set_device(c);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out, c->d_grad.p, 2 * (size_t)c->m * c->n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return D2D_OK;
}

int d2d_get_scene_vjp(d2d_ctx* c, float* tx_bar, float* xys_bar, float* phi_bar) {
    if (!c || !tx_bar) return fail(D2D_ERR_INVALID, "NULL argument");
    if (!c->have_vjp) return fail(D2D_ERR_STATE, "no scene-VJP sweep has run");
    int rc = set_device(c);
    if (rc) return rc;
    const int n_elem = 4 * c->N + 2;
    std::vector<double> h((size_t)n_elem);
    if ((rc = join_comm(c, 2))) return rc;  // an all-reduce of the VJP in flight lands first
    HIP_TRY(hipMemcpyAsync(h.data(), c->d_vjp.p, (size_t)n_elem * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (xys_bar)
        for (int i = 0; i < 4 * c->N; ++i) xys_bar[i] = (float)h[(size_t)i];
    tx_bar[0] = (float)h[(size_t)4 * c->N];
    tx_bar[1] = (float)h[(size_t)4 * c->N + 1];
    if (phi_bar) {
        // ImagePath sweeps interact with Wall objects only (RIS / Vertex objects need MinPath / FermatPath): the map does not
        // depend on any phi
        for (int j = 0; j < c->N; ++j) phi_bar[j] = 0.0f;
        if (c->vjp_has_phi) {
            std::vector<double> hp((size_t)c->N);
            HIP_TRY(hipMemcpyAsync(hp.data(), c->d_vjp.p + n_elem, (size_t)c->N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            for (int j = 0; j < c->N; ++j) phi_bar[j] = (float)hp[(size_t)j];
        }
    }
    return D2D_OK;
}

int d2d_selftest_div(d2d_ctx* c, const float* x, const float* y, int64_t n, float* q_fast, float* q_ref, float* q_hostr) {
    if (!c || !x || !y || !q_fast || !q_ref || !q_hostr || n <= 0) return fail(D2D_ERR_INVALID, "bad argument");
    int rc = set_device(c);
    if (rc) return rc;
    DevBuf<float> dx, dy, dr, d1, d2, d3;
    std::vector<float> ry((size_t)n);
    for (int64_t i = 0; i < n; ++i) ry[(size_t)i] = 1.0f / y[i];
    if ((rc = dx.ensure(n)) || (rc = dy.ensure(n)) || (rc = dr.ensure(n)) || (rc = d1.ensure(n)) || (rc = d2.ensure(n)) || (rc = d3.ensure(n))) return rc;
    HIP_TRY(hipMemcpy(dx.p, x, n * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dy.p, y, n * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dr.p, ry.data(), n * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(d2d::selftest_div_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, dx.p, dy.p, d1.p, d2.p, d3.p, dr.p, (long)n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(q_fast, d1.p, n * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(q_ref, d2.p, n * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(q_hostr, d3.p, n * sizeof(float), hipMemcpyDeviceToHost));
    return D2D_OK;
}

int d2d_selftest_expf(d2d_ctx* c, const float* x, int64_t n, float* y) {
    if (!c || !x || !y || n <= 0) return fail(D2D_ERR_INVALID, "bad argument");
    int rc = set_device(c);
    if (rc) return rc;
    DevBuf<float> dx, dy;
    if ((rc = dx.ensure((size_t)n)) || (rc = dy.ensure((size_t)n))) return rc;
    HIP_TRY(hipMemcpy(dx.p, x, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(d2d::selftest_expf_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, dx.p, dy.p, (long)n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(y, dy.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return D2D_OK;
}

int d2d_selftest_phasor(d2d_ctx* c, const float* f, int64_t n, float* cs, float* sn) {
    if (!c || !f || !cs || !sn || n <= 0) return fail(D2D_ERR_INVALID, "bad argument");
    int rc = set_device(c);
    if (rc) return rc;
    DevBuf<float> df, dc, ds;
    if ((rc = df.ensure((size_t)n)) || (rc = dc.ensure((size_t)n)) || (rc = ds.ensure((size_t)n))) return rc;
    HIP_TRY(hipMemcpy(df.p, f, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(d2d::selftest_phasor_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, df.p, dc.p, ds.p, (long)n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(cs, dc.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(sn, ds.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return D2D_OK;
}

int d2d_selftest_angle(d2d_ctx* c, const float* dx, const float* dy, int64_t n, float* out) {
    if (!c || !dx || !dy || !out || n <= 0) return fail(D2D_ERR_INVALID, "bad argument");
    int rc = set_device(c);
    if (rc) return rc;
    DevBuf<float> ddx, ddy, dout;
    if ((rc = ddx.ensure((size_t)n)) || (rc = ddy.ensure((size_t)n)) || (rc = dout.ensure((size_t)n))) return rc;
    HIP_TRY(hipMemcpy(ddx.p, dx, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ddy.p, dy, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(d2d::selftest_angle_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, ddx.p, ddy.p, dout.p, (long)n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out, dout.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return D2D_OK;
}

int d2d_selftest_steer(d2d_ctx* c, const float* dx, const float* dy, const float* f0, const float* qt, const float* qr, const float* inv, int64_t n,
                       float* ux, float* uy, float* ok, float* f) {
    if (!c || !dx || !dy || !f0 || !qt || !qr || !inv || !ux || !uy || !ok || !f || n <= 0) return fail(D2D_ERR_INVALID, "bad argument");
    int rc = set_device(c);
    if (rc) return rc;
    DevBuf<float> din, dout;  // six inputs, four outputs, n each
    if ((rc = din.ensure(6 * (size_t)n)) || (rc = dout.ensure(4 * (size_t)n))) return rc;
    const float* in[6] = {dx, dy, f0, qt, qr, inv};
    for (int k = 0; k < 6; ++k) HIP_TRY(hipMemcpy(din.p + (size_t)k * (size_t)n, in[k], (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(d2d::selftest_steer_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, din.p, dout.p, (long)n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    float* out[4] = {ux, uy, ok, f};
    for (int k = 0; k < 4; ++k) HIP_TRY(hipMemcpy(out[k], dout.p + (size_t)k * (size_t)n, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return D2D_OK;
}

int d2d_selftest_fresnel(d2d_ctx* c, const float* er, const float* ei, const float* cs, int32_t pol, int64_t n, float* gr, float* gi) {
    if (!c || !er || !ei || !cs || !gr || !gi || n <= 0 || (pol != D2D_POL_TE && pol != D2D_POL_TM)) return fail(D2D_ERR_INVALID, "bad argument");
    int rc = set_device(c);
    if (rc) return rc;
    DevBuf<float> din, dout;  // three inputs, two outputs, n each
    if ((rc = din.ensure(3 * (size_t)n)) || (rc = dout.ensure(2 * (size_t)n))) return rc;
    const float* in[3] = {er, ei, cs};
    for (int k = 0; k < 3; ++k) HIP_TRY(hipMemcpy(din.p + (size_t)k * (size_t)n, in[k], (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(d2d::selftest_fresnel_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, din.p, dout.p, (int)pol, (long)n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    float* out[2] = {gr, gi};
    for (int k = 0; k < 2; ++k) HIP_TRY(hipMemcpy(out[k], dout.p + (size_t)k * (size_t)n, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return D2D_OK;
}

int d2d_selftest_fresnel_grad(d2d_ctx* c, const float* er, const float* ei, const float* cs, int32_t pol, int64_t n, float* gr, float* gi, float* dr, float* di,
                              float* ok) {
    if (!c || !er || !ei || !cs || !gr || !gi || !dr || !di || !ok || n <= 0 || (pol != D2D_POL_TE && pol != D2D_POL_TM)) return fail(D2D_ERR_INVALID, "bad argument");
    int rc = set_device(c);
    if (rc) return rc;
    DevBuf<float> din, dout;  // three inputs, five outputs, n each
    if ((rc = din.ensure(3 * (size_t)n)) || (rc = dout.ensure(5 * (size_t)n))) return rc;
    const float* in[3] = {er, ei, cs};
    for (int k = 0; k < 3; ++k) HIP_TRY(hipMemcpy(din.p + (size_t)k * (size_t)n, in[k], (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(d2d::selftest_fresnel_grad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, din.p, dout.p, (int)pol, (long)n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    float* out[5] = {gr, gi, dr, di, ok};
    for (int k = 0; k < 5; ++k) HIP_TRY(hipMemcpy(out[k], dout.p + (size_t)k * (size_t)n, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return D2D_OK;
}

int d2d_selftest_posgrad(d2d_ctx* c, int32_t fun_id, int32_t amplitude, const float* t, const float* r, const float* h2, const float* inv0, const float* inv1,
                         const float* rb0, const float* rb1, const float* ib0, const float* ib1, int64_t n, float* a, float* rho, float* kr, float* g, float* G) {
    if (!c || !t || !r || !h2 || !inv0 || !inv1 || !rb0 || !rb1 || !ib0 || !ib1 || !a || !rho || !kr || !g || !G || n <= 0)
        return fail(D2D_ERR_INVALID, "bad argument");
    int rc = set_device(c);
    if (rc) return rc;
    DevBuf<float> din, dout;  // nine inputs, five outputs, n each
    if ((rc = din.ensure(9 * (size_t)n)) || (rc = dout.ensure(5 * (size_t)n))) return rc;
    const float* in[9] = {t, r, h2, inv0, inv1, rb0, rb1, ib0, ib1};
    for (int k = 0; k < 9; ++k) HIP_TRY(hipMemcpy(din.p + (size_t)k * (size_t)n, in[k], (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(d2d::selftest_posgrad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, din.p, dout.p, (int)fun_id, (int)amplitude,
                       (long)n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    float* out[5] = {a, rho, kr, g, G};
    for (int k = 0; k < 5; ++k) HIP_TRY(hipMemcpy(out[k], dout.p + (size_t)k * (size_t)n, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return D2D_OK;
}

int d2d_selftest_wallgrad(d2d_ctx* c, const float* const* in, int64_t n, float* qx, float* qy, float* Wa, float* Wb, float* ok) {
    if (!c || !in || !qx || !qy || !Wa || !Wb || !ok || n <= 0) return fail(D2D_ERR_INVALID, "bad argument");
    for (int k = 0; k < 12; ++k)
        if (!in[k]) return fail(D2D_ERR_INVALID, "bad argument");
    int rc = set_device(c);
    if (rc) return rc;
    DevBuf<float> din, dout;  // twelve inputs, five outputs, n each
    if ((rc = din.ensure(12 * (size_t)n)) || (rc = dout.ensure(5 * (size_t)n))) return rc;
    for (int k = 0; k < 12; ++k) HIP_TRY(hipMemcpy(din.p + (size_t)k * (size_t)n, in[k], (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(d2d::selftest_wallgrad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, din.p, dout.p, (long)n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    float* out[5] = {qx, qy, Wa, Wb, ok};
    for (int k = 0; k < 5; ++k) HIP_TRY(hipMemcpy(out[k], dout.p + (size_t)k * (size_t)n, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return D2D_OK;
}

int d2d_set_option(d2d_ctx* c, const char* name, int64_t value) {
    if (!c || !name) return fail(D2D_ERR_INVALID, "d2d_set_option: NULL argument");
    if (!strcmp(name, "split_max_tiles")) c->split_max_tiles = value;
    else if (!strcmp(name, "coop_max_tiles")) c->coop_max_tiles = value;
    else if (!strcmp(name, "hidden_masks")) c->use_hidden_masks = value != 0;
    else if (!strcmp(name, "hidden_min_tiles")) c->hidden_min_tiles = value;
    else if (!strcmp(name, "split_sigmoid")) c->split_sigmoid = value != 0;
    else if (!strcmp(name, "coop_waves")) {
        if (value != -1 && value != 0 && value != 4 && value != 8 && value != 16) return fail(D2D_ERR_INVALID, "coop_waves must be -1, 0, 4, 8 or 16, got %lld", (long long)value);
        c->coop_waves = value;
    }
    else if (!strcmp(name, "sched_min_tiles")) c->sched_min_tiles = value;
    else if (!strcmp(name, "heavy_split")) c->heavy_split = value;
    else if (!strcmp(name, "time_kernel")) c->time_kernel = value != 0;
    else if (!strcmp(name, "cost_history")) c->use_cost_history = value != 0;
    else if (!strcmp(name, "pipeline")) {
        // (the two sets must not be mixed up by a switch in mid-flight)
        if (c->stream) HIP_TRY(hipStreamSynchronize(c->stream));
        if (c->aux_stream) HIP_TRY(hipStreamSynchronize(c->aux_stream));
        c->for_each_set([](d2d_ctx::PrepSet& sp) { sp.swept_pending = false; });
        c->pipeline = value != 0;
    }
    else if (!strcmp(name, "unpiped_max_tiles")) {
        if (value < 0) return fail(D2D_ERR_INVALID, "unpiped_max_tiles must be >= 0, got %lld", (long long)value);
        c->unpiped_max_tiles = value;
    }
    else if (!strcmp(name, "fwd_waves")) {
        if (value != 0 && value != 1 && value != 4) return fail(D2D_ERR_INVALID, "fwd_waves must be 0, 1 or 4, got %lld", (long long)value);
        c->fwd_waves = value;
    }
    else if (!strcmp(name, "pair_masks")) c->use_pair_masks = value != 0;
#ifdef D2D_AB_TIMELINE
    else if (!strcmp(name, "tl_ring")) {
        c->tl_ring_on = value != 0;
        c->tl_seq = 0;
        if (c->tl_ring_on) {
            int rc2 = c->d_tl_ring.ensure(512);
            if (rc2) return rc2;
            std::vector<unsigned long long> init(512);
            for (int i = 0; i < 256; ++i) { init[2 * i] = ~0ull; init[2 * i + 1] = 0ull; }
            HIP_TRY(hipMemcpy(c->d_tl_ring.p, init.data(), 512 * sizeof(unsigned long long), hipMemcpyHostToDevice));
        }
    }
#endif
    else if (!strcmp(name, "nan_scan")) {
        if (value < 0 || value > 2) return fail(D2D_ERR_INVALID, "nan_scan must be 0 (off), 1 (two levels) or 2 (one wave per patch), got %lld", (long long)value);
        c->nan_scan = value != 0;
        if (value) c->nan_scan_mode = value;
    }
    else if (!strcmp(name, "nan_scan_stats")) c->nan_scan_stats = value != 0;
    else if (!strcmp(name, "comm_prio")) {
        if (c->comm_stream) return fail(D2D_ERR_STATE, "comm_prio must be set before the first collective creates the communication stream");
        c->comm_prio = value > 0 ? 1 : (value < 0 ? -1 : 0);
    }
    else if (!strcmp(name, "nan_scan_wqcap")) {
        if (value < 0 || value > d2d::NAN_WQCAP) return fail(D2D_ERR_INVALID, "nan_scan_wqcap must be in [0, %d], got %lld", d2d::NAN_WQCAP, (long long)value);
        c->nan_wqcap = value;
    } else if (!strcmp(name, "nan_scan_rb")) {
        if (value < 0 || value > d2d::NAN_RB) return fail(D2D_ERR_INVALID, "nan_scan_rb must be in [0, %d], got %lld", d2d::NAN_RB, (long long)value);
        c->nan_rb = value;
    }
    else if (!strcmp(name, "opt_parallel")) c->opt_parallel = value != 0;
    else if (!strcmp(name, "opt_grad_mode")) {
        if (value != 0 && value != 1) return fail(D2D_ERR_INVALID, "opt_grad_mode must be 0 (reverse mode) or 1 (forward tangents), got %lld", (long long)value);
        c->opt_grad_mode = value;
    } else if (!strcmp(name, "opt_traj_mb")) {
        if (value < 1 || value > (256ll << 10)) return fail(D2D_ERR_INVALID, "opt_traj_mb must lie in 1..262144, got %lld", (long long)value);
        c->opt_traj_mb = value;
    }
    else if (!strcmp(name, "txg_exhaustive")) c->txg_exhaustive = value != 0;
    else if (!strcmp(name, "region_lists")) c->use_region_lists = value != 0;
    else if (!strcmp(name, "region_size")) {
        if (value < 1 || value > 64) return fail(D2D_ERR_INVALID, "region_size must lie in 1..64, got %lld", (long long)value);
        c->region_size = value;
    } else if (!strcmp(name, "region_size_top")) {
        if (value < 1 || value > 1024) return fail(D2D_ERR_INVALID, "region_size_top must lie in 1..1024, got %lld", (long long)value);
        c->region_size_top = value;
    } else if (!strcmp(name, "region_slices")) {
        if (value < 0 || value > 1024) return fail(D2D_ERR_INVALID, "region_slices must lie in 0..1024, got %lld", (long long)value);
        c->region_slices = value;
    } else if (!strcmp(name, "region_budget_mb")) {
        if (value < 1 || value > (256ll << 10)) return fail(D2D_ERR_INVALID, "region_budget_mb must lie in 1..262144, got %lld", (long long)value);
        c->region_budget_mb = value;
        c->rl_pool_mb = std::min<long long>(256, value);
        c->rl_pool_by_option = true;
    }
    else return fail(D2D_ERR_INVALID, "d2d_set_option: unknown option '%s'", name);
    return D2D_OK;
}

int d2d_debug_set_schedule(d2d_ctx* c, const int32_t* order, int64_t n) {
    if (!c || (n > 0 && !order)) return fail(D2D_ERR_INVALID, "NULL argument");
    int rc = set_device(c);
    if (rc) return rc;
    c->sched_override_n = 0;
    if (n <= 0) return D2D_OK;
    std::vector<char> seen((size_t)n, 0);
    for (int64_t i = 0; i < n; ++i) {
        if (order[i] < 0 || order[i] >= n || seen[(size_t)order[i]]) return fail(D2D_ERR_INVALID, "schedule is not a permutation of 0..%lld", (long long)n - 1);
        seen[(size_t)order[i]] = 1;
    }
    if ((rc = c->d_sched_override.ensure((size_t)n))) return rc;
    HIP_TRY(hipMemcpyAsync(c->d_sched_override.p, order, (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->sched_override_n = n;
    return D2D_OK;
}

int d2d_debug_get_work(d2d_ctx* c, uint32_t* work, int64_t n) {
    if (!c || !work) return fail(D2D_ERR_INVALID, "NULL argument");
    int rc = set_device(c);
    if (rc) return rc;
#ifdef D2D_AB_TIMELINE
    if (n == -7) {  // the launches' ring: 256 x {first start, end} as 1024 words
        if (!c->d_tl_ring.p) return fail(D2D_ERR_STATE, "tl_ring is off");
        HIP_TRY(hipMemcpyAsync(work, c->d_tl_ring.p, 512 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return (int)0;
    }
    if (n < 0) {  // the stamps of the last forward launch's workgroups (work[0 .. min(-n, timeline_n))
        const long long m = std::min<long long>(-n, c->timeline_n);
        HIP_TRY(hipMemcpyAsync(work, c->d_timeline.p, (size_t)m * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return (int)0;
    }
#endif
    if (!c->cur.d_cost.p || c->cur.cost_tiles != n) return fail(D2D_ERR_STATE, "no work history of %lld patches", (long long)n);
    HIP_TRY(hipMemcpyAsync(work, c->cur.d_cost.p, (size_t)n * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return D2D_OK;
}

int d2d_debug_nan_scan(d2d_ctx* c, int64_t* out) {
    if (!c || !out) return fail(D2D_ERR_INVALID, "NULL argument");
    int rc = set_device(c);
    if (rc) return rc;
    for (int i = 0; i < 6; ++i) out[i] = 0;
    if (!c->d_nan_stats.p) return D2D_OK;
    unsigned long long h[8];
    HIP_TRY(hipStreamSynchronize(c->stream));  // (the launch joined the scan's stream)
    HIP_TRY(hipMemcpy(h, c->d_nan_stats.p, sizeof h, hipMemcpyDeviceToHost));
    for (int i = 0; i < 6; ++i) out[i] = (int64_t)h[i];
    return D2D_OK;
}

int d2d_debug_region_stats(d2d_ctx* c, int64_t* out) {
    if (!c || !out) return fail(D2D_ERR_INVALID, "NULL argument");
    int rc = set_device(c);
    if (rc) return rc;
    for (int i = 0; i < 8; ++i) out[i] = 0;
    if (!c->rl_plan.on) return D2D_OK;
    const d2d_host::RegionPlan& rp = c->rl_plan;
    std::vector<int> meta(2 + (size_t)rp.leaf.regions);
    HIP_TRY(hipMemcpyAsync(meta.data(), c->cur.rl_meta_ptr, meta.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    const int orders = c->rl_max_order - rp.k_lo + 1;
    const size_t per_order = (size_t)rp.leaf.slots + (size_t)rp.top.slots;
    std::vector<int> idx(per_order * (size_t)orders);
    HIP_TRY(hipMemcpyAsync(idx.data(), c->cur.d_rl_idx.p, idx.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    out[0] = meta[1] + rp.n_static;
    out[1] = rp.max_chunks;
    out[2] = meta[0];
    for (long long r = 0; r < rp.leaf.regions; ++r) out[3] += meta[2 + (size_t)r] != 0;
    for (int k = rp.k_lo; k <= c->rl_max_order && k <= 4; ++k) {
        const int* cnt = idx.data() + per_order * (size_t)(k - rp.k_lo);
        for (long long i = 0; i < rp.leaf.slots; ++i) out[2 + k] += cnt[i] > 0 ? cnt[i] : 0;
    }
    out[7] = rp.leaf.regions;
    return D2D_OK;
}

int d2d_debug_get_schedule(d2d_ctx* c, int32_t* order, uint8_t* key, int64_t n) {
    if (!c || !order || !key) return fail(D2D_ERR_INVALID, "NULL argument");
    int rc = set_device(c);
    if (rc) return rc;
    if (!c->cur.d_sched.p || !c->cur.d_sched_key.p || (size_t)n > c->cur.d_sched.n) return fail(D2D_ERR_STATE, "no schedule of %lld patches has been built", (long long)n);
    HIP_TRY(hipMemcpyAsync(order, c->cur.d_sched.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(key, c->cur.d_sched_key.p, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return D2D_OK;
}

int d2d_power_map_wave_cycles(d2d_ctx* c, const d2d_params* p, const float* tx, uint64_t* cycles, int64_t capacity, int64_t* n_waves) {
    if (!c || !cycles || !n_waves) return fail(D2D_ERR_INVALID, "NULL argument");
    if (!c->have_grid) return fail(D2D_ERR_STATE, "no grid set");
    int rc = set_device(c);
    if (rc) return rc;
    const int64_t waves = (int64_t)((c->n + d2d::TILE_W - 1) / d2d::TILE_W) * ((c->m + d2d::TILE_H - 1) / d2d::TILE_H);
    *n_waves = waves;
    if (capacity < waves) return fail(D2D_ERR_INVALID, "capacity %lld < %lld waves", (long long)capacity, (long long)waves);
    if ((rc = c->d_stats.ensure((size_t)D2D_NUM_STATS + (size_t)waves))) return rc;
    HIP_TRY(hipMemsetAsync(c->d_stats.p, 0, ((size_t)D2D_NUM_STATS + (size_t)waves) * sizeof(unsigned long long), c->stream));
    c->want_wave_cycles = true;
    rc = sweep_launch(c, p, tx, c->d_stats.p);
    c->want_wave_cycles = false;
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(cycles, c->d_stats.p + D2D_NUM_STATS, (size_t)waves * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return D2D_OK;
}

int d2d_power_map_stats(d2d_ctx* c, const d2d_params* p, const float* tx, uint64_t* stats) {
    if (!c || !stats) return fail(D2D_ERR_INVALID, "NULL argument");
    int rc = set_device(c);
    if (rc) return rc;
    if ((rc = c->d_stats.ensure(D2D_NUM_STATS))) return rc;
    HIP_TRY(hipMemsetAsync(c->d_stats.p, 0, D2D_NUM_STATS * sizeof(unsigned long long), c->stream));
    if ((rc = sweep_launch(c, p, tx, c->d_stats.p))) return rc;
    unsigned long long h[D2D_NUM_STATS];
    HIP_TRY(hipMemcpyAsync(h, c->d_stats.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int i = 0; i < D2D_NUM_STATS; ++i) stats[i] = h[i];
    return D2D_OK;
}

int d2d_set_theta0(d2d_ctx* c, const float* theta0, int64_t n_rows) {
    if (!c) return fail(D2D_ERR_INVALID, "ctx is NULL");
    if (n_rows < 0 || (n_rows > 0 && !theta0)) return fail(D2D_ERR_INVALID, "bad theta0 arguments");
    c->theta0.assign(theta0, theta0 + n_rows * D2D_MAX_ORDER);
    return D2D_OK;
}

int d2d_set_optimizer(d2d_ctx* c, int32_t kind, double learning_rate, double b1, double b2, double eps) {
    if (!c) return fail(D2D_ERR_INVALID, "ctx is NULL");
    if (kind == D2D_OPT_SGD || kind == D2D_OPT_SGD_MOMENTUM) {
        if (!std::isfinite(learning_rate)) return fail(D2D_ERR_INVALID, "SGD needs a finite learning rate (got %g)", learning_rate);
        if (kind == D2D_OPT_SGD_MOMENTUM && (!(b1 >= 0.0 && b1 < 1.0) || !(b2 == 0.0 || b2 == 1.0)))
            return fail(D2D_ERR_INVALID, "SGD with momentum needs a momentum in [0, 1) and a Nesterov flag of 0 or 1 (got %g, %g)", b1, b2);
        c->opt_kind = kind;
        c->opt_lr = learning_rate;
        c->opt_b1 = (kind == D2D_OPT_SGD_MOMENTUM) ? b1 : 0.0;
        c->opt_b2 = (kind == D2D_OPT_SGD_MOMENTUM) ? b2 : 0.0;
        c->opt_eps = 0.0;
        return D2D_OK;
    }
    if (kind != D2D_OPT_ADAM)
        return fail(D2D_ERR_UNSUPPORTED, "optimizer kind %d is not native (D2D_OPT_ADAM, D2D_OPT_SGD and D2D_OPT_SGD_MOMENTUM are)", (int)kind);
    if (!std::isfinite(learning_rate) || !(b1 >= 0.0 && b1 < 1.0) || !(b2 >= 0.0 && b2 < 1.0) || !(eps >= 0.0) || !std::isfinite(eps))
        return fail(D2D_ERR_INVALID, "Adam needs a finite learning rate, decay rates in [0, 1) and eps >= 0 (got %g, %g, %g, %g)", learning_rate, b1,
                    b2, eps);
    c->opt_kind = kind;
    c->opt_lr = learning_rate;
    c->opt_b1 = b1;
    c->opt_b2 = b2;
    c->opt_eps = eps;
    return D2D_OK;
}

int d2d_trace_paths(d2d_ctx* c, const d2d_params* p, const float* tx, const float* rx, int32_t P, const int32_t* cand,
                    const int32_t* order, int32_t C, const float* theta0, int64_t theta0_rows, const float* xys_in,
                    const float* loss_in, float* xys, float* loss, float* valid, float* on, float* hit, float* length) {
    if (!c || !tx || !rx || !cand || !order || !xys || !loss || !valid) return fail(D2D_ERR_INVALID, "NULL argument");
    int rc = check_params(p);
    if (rc) return rc;
    if (!c->have_scene) return fail(D2D_ERR_STATE, "d2d_set_scene must come first");
    if (P < 0 || C < 0) return fail(D2D_ERR_INVALID, "negative sizes");
    const bool opt = (p->solver == D2D_SOLVER_MINPATH || p->solver == D2D_SOLVER_FERMAT) && !xys_in;
    if (opt && theta0 && theta0_rows != (int64_t)C * (p->many > 1 ? p->many : 1))
        return fail(D2D_ERR_INVALID, "theta0 must hold %lld rows (candidates x max(1, many)), got %lld",
                    (long long)C * (p->many > 1 ? p->many : 1), (long long)theta0_rows);
    if (p->solver < D2D_SOLVER_IMAGE || p->solver > D2D_SOLVER_FERMAT) return fail(D2D_ERR_INVALID, "unknown solver %d", p->solver);
    for (int i = 0; i < C; ++i) {
        if (order[i] < 0 || order[i] > D2D_MAX_ORDER) return fail(D2D_ERR_INVALID, "candidate %d has order %d", i, order[i]);
        for (int q = 0; q < order[i]; ++q) {
            int w = cand[(size_t)i * D2D_MAX_ORDER + q];
            if (w < 0 || w >= c->N) return fail(D2D_ERR_INVALID, "candidate %d references object %d of %d", i, w, c->N);
            if (!xys_in && !opt && c->kind[w] != D2D_WALL)
                return fail(D2D_ERR_UNSUPPORTED, "ImagePath needs Wall objects; object %d has kind %d", w, (int)c->kind[w]);
            if (opt && !theta0 && c->kind[w] != D2D_VERTEX)
                return fail(D2D_ERR_INVALID, "theta0 is required by the optimiser-based solvers");
        }
    }
    const size_t n = (size_t)P * (size_t)C;
    if (n == 0) return D2D_OK;
    if ((rc = set_device(c))) return rc;
    if ((rc = upload_occl(c, p->patch))) return rc;
    constexpr size_t NP = D2D_MAX_ORDER + 2;
    if ((rc = c->d_tcand.ensure((size_t)C * D2D_MAX_ORDER))) return rc;
    if ((rc = c->d_torder.ensure((size_t)C))) return rc;
    if ((rc = c->d_ttx.ensure(2 * (size_t)P))) return rc;
    if ((rc = c->d_trx.ensure(2 * (size_t)P))) return rc;
    if ((rc = c->d_txys.ensure(n * NP * 2))) return rc;
    if ((rc = c->d_tloss.ensure(n))) return rc;
    if ((rc = c->d_tvalid.ensure(n))) return rc;
    if ((rc = c->d_ton.ensure(n))) return rc;
    if ((rc = c->d_thit.ensure(n))) return rc;
    if ((rc = c->d_tlen.ensure(n))) return rc;
    HIP_TRY(hipMemcpyAsync(c->d_tcand.p, cand, (size_t)C * D2D_MAX_ORDER * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_torder.p, order, (size_t)C * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_ttx.p, tx, 2 * (size_t)P * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_trx.p, rx, 2 * (size_t)P * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (xys_in) {
        if ((rc = c->d_txys_in.ensure(n * NP * 2))) return rc;
        HIP_TRY(hipMemcpyAsync(c->d_txys_in.p, xys_in, n * NP * 2 * sizeof(float), hipMemcpyHostToDevice, c->stream));
        if (loss_in) {
            if ((rc = c->d_tloss_in.ensure(n))) return rc;
            HIP_TRY(hipMemcpyAsync(c->d_tloss_in.p, loss_in, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
        }
    }
    d2d::TraceArgs a;
    memset(&a, 0, sizeof a);
    a.T = obj_tables(c);
    a.solver = p->solver;
    if (opt) {
        if ((rc = opt_cfg(c, p, &a.A))) return rc;
        const size_t nth = (size_t)C * (size_t)a.A.many * D2D_MAX_ORDER;
        if ((rc = c->d_theta0.ensure(nth + 1))) return rc;
        if (theta0) HIP_TRY(hipMemcpyAsync(c->d_theta0.p, theta0, nth * sizeof(float), hipMemcpyHostToDevice, c->stream));
        else HIP_TRY(hipMemsetAsync(c->d_theta0.p, 0, nth * sizeof(float), c->stream));
        a.theta0 = c->d_theta0.p;
    }
    a.cand = c->d_tcand.p;
    a.order = c->d_torder.p;
    a.C = C;
    a.tx = c->d_ttx.p;
    a.rx = c->d_trx.p;
    a.P = P;
    a.xys_in = xys_in ? c->d_txys_in.p : nullptr;
    a.loss_in = (xys_in && loss_in) ? c->d_tloss_in.p : nullptr;
    a.xys = c->d_txys.p;
    a.loss = c->d_tloss.p;
    a.valid = c->d_tvalid.p;
    a.on = c->d_ton.p;
    a.hit = c->d_thit.p;
    a.length = c->d_tlen.p;
    set_validity(a, p);
    HIP_TRY(d2d::launch_trace(a, dim3((unsigned)((n + 63) / 64)), c->stream));
    HIP_TRY(hipMemcpyAsync(xys, c->d_txys.p, n * NP * 2 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(loss, c->d_tloss.p, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(valid, c->d_tvalid.p, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (on) HIP_TRY(hipMemcpyAsync(on, c->d_ton.p, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (hit) HIP_TRY(hipMemcpyAsync(hit, c->d_thit.p, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (length) HIP_TRY(hipMemcpyAsync(length, c->d_tlen.p, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return D2D_OK;
}

int d2d_get_map(d2d_ctx* c, float* out) {
    if (!c || !out) return fail(D2D_ERR_INVALID, "NULL argument");
    if (!c->have_grid) return fail(D2D_ERR_STATE, "no grid set");
    int rc = set_device(c);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out, c->d_out.p, (size_t)c->m * c->n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return D2D_OK;
}

int d2d_power_map(d2d_ctx* c, const d2d_params* p, const float* tx, const float* X, const float* Y, int32_t m, int32_t n,
                  float* out) {
    int rc = d2d_set_grid(c, X, Y, m, n);
    if (rc) return rc;
    if ((rc = d2d_power_map_launch(c, p, tx))) return rc;
    return d2d_get_map(c, out);
}

/* ---- RCCL --------------------------------------------------------------------------------- */

int d2d_comm_unique_id(uint8_t* id) {
    if (!id) return fail(D2D_ERR_INVALID, "id is NULL");
    if (!rccl().ok) {
        const char* why = dlerror();  // (a second call would return NULL: dlerror clears its state)
        return fail(D2D_ERR_COMM, "librccl could not be loaded: %s", why ? why : "missing symbols");
    }
    ncclUniqueId u;
    RCCL_TRY(rccl().GetUniqueId(&u));
    static_assert(sizeof(u) == D2D_COMM_ID_BYTES, "ncclUniqueId size");
    memcpy(id, &u, sizeof u);
    return D2D_OK;
}

int d2d_comm_init(d2d_ctx* c, const uint8_t* id, int32_t rank, int32_t world) {
    if (!c || !id) return fail(D2D_ERR_INVALID, "NULL argument");
    if (world < 1 || rank < 0 || rank >= world) return fail(D2D_ERR_INVALID, "bad rank %d of %d", rank, world);
    if (!rccl().ok) return fail(D2D_ERR_COMM, "librccl could not be loaded");
    int rc = set_device(c);
    if (rc) return rc;
    if (c->comm) {
        rccl().CommDestroy(c->comm);
        c->comm = nullptr;
    }
    ncclUniqueId u;
    memcpy(&u, id, sizeof u);
    RCCL_TRY(rccl().CommInitRank(&c->comm, world, u, rank));
    c->rank = rank;
    c->world = world;
    return D2D_OK;
}

int d2d_comm_count(d2d_ctx* c, int32_t* ranks) {
    if (!c || !ranks) return fail(D2D_ERR_INVALID, "NULL argument");
    if (!c->comm) return fail(D2D_ERR_STATE, "d2d_comm_init must come first");
    if (!rccl().CommCount) return fail(D2D_ERR_COMM, "librccl has no ncclCommCount");
    int n = 0;
    RCCL_TRY(rccl().CommCount(c->comm, &n));
    *ranks = n;
    return D2D_OK;
}

int d2d_comm_destroy(d2d_ctx* c) {
    if (!c) return fail(D2D_ERR_INVALID, "ctx is NULL");
    if (c->comm) {
        (void)set_device(c);
        (void)hipStreamSynchronize(c->stream);
        if (c->comm_stream) (void)hipStreamSynchronize(c->comm_stream);
        c->inflight[0] = c->inflight[1] = c->inflight[2] = false;
        rccl().CommDestroy(c->comm);
        c->comm = nullptr;
    }
    c->world = 1;
    c->rank = 0;
    return D2D_OK;
}

// Common part of the two map collectives.  root < 0: all-gather (every rank receives the whole map); root >= 0: gather
// to that rank only -- what a single-process caller of the reference gets (one assembled array, scene.py:1927-1953):
// ncclSend from every other rank, world - 1 ncclRecv on the root inside one group, N x fewer bytes on the wire than the
// all-gather and nothing to receive on the other ranks.
static int gather_map(d2d_ctx* c, int32_t what, int32_t root) {
    if (!c) return fail(D2D_ERR_INVALID, "ctx is NULL");
    if (!c->comm) return fail(D2D_ERR_STATE, "d2d_comm_init must come first");
    if (!c->have_grid) return fail(D2D_ERR_STATE, "no grid set");
    if (what != 0 && what != 1) return fail(D2D_ERR_INVALID, "what must be 0 (value map) or 1 (grad map)");
    if (what == 1 && !c->have_grad) return fail(D2D_ERR_STATE, "no value+grad sweep has run on this grid");
    if (root >= c->world) return fail(D2D_ERR_INVALID, "root %d is not a rank of this communicator (world %d)", root, c->world);
    int rc = set_device(c);
    if (rc) return rc;
    const size_t per_rank = (size_t)c->m * c->n * (what ? 2 : 1);
    const bool receives = root < 0 || root == c->rank;
    DevBuf<float>& gbuf = c->d_gather[what];
    DevBuf<float>& sbuf = c->d_send[what];
    if (receives && (rc = gbuf.ensure(per_rank * (size_t)c->world))) return rc;
    if ((rc = sbuf.ensure(per_rank))) return rc;
    if ((rc = ensure_comm_stream(c))) return rc;
    // main stream: (the previous gather of this map has finished reading the staging copy) -> copy this step's shard;
    // communication stream: -> collective -> done.  The next sweep on the main stream does not wait for `done`.
    if ((rc = join_comm(c, what))) return rc;
    HIP_TRY(hipMemcpyAsync(sbuf.p, what ? c->d_grad.p : c->d_out.p, per_rank * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    if ((rc = comm_after_main(c))) return rc;
    if (root < 0) {
        RCCL_TRY(rccl().AllGather(sbuf.p, gbuf.p, per_rank, ncclFloat32, c->comm, c->comm_stream));
    } else if (root == c->rank) {
        RCCL_TRY(rccl().GroupStart());
        for (int r = 0; r < c->world; ++r)
            if (r != root) RCCL_TRY(rccl().Recv(gbuf.p + (size_t)r * per_rank, per_rank, ncclFloat32, r, c->comm, c->comm_stream));
        RCCL_TRY(rccl().GroupEnd());
        HIP_TRY(hipMemcpyAsync(gbuf.p + (size_t)root * per_rank, sbuf.p, per_rank * sizeof(float), hipMemcpyDeviceToDevice, c->comm_stream));
    } else {
        RCCL_TRY(rccl().Send(sbuf.p, per_rank, ncclFloat32, root, c->comm, c->comm_stream));
    }
    HIP_TRY(hipEventRecord(c->ev_done[what], c->comm_stream));
    c->inflight[what] = true;
    c->gathered[what] = receives ? per_rank : 0;
    return D2D_OK;
}

int d2d_comm_allgather_map(d2d_ctx* c, int32_t what) { return gather_map(c, what, -1); }

int d2d_comm_gather_map(d2d_ctx* c, int32_t what, int32_t root) {
    if (root < 0) return fail(D2D_ERR_INVALID, "root must be a rank (>= 0)");
    return gather_map(c, what, root);
}

int d2d_comm_get_gathered(d2d_ctx* c, int32_t what, float* out, int64_t capacity) {
    if (!c || !out) return fail(D2D_ERR_INVALID, "NULL argument");
    if (what != 0 && what != 1) return fail(D2D_ERR_INVALID, "what must be 0 (value map) or 1 (grad map)");
    if (!c->gathered[what])
        return fail(D2D_ERR_STATE, "no %s map has been gathered on this rank (after d2d_comm_gather_map only the root holds it)",
                    what ? "gradient" : "value");
    const size_t total = c->gathered[what] * (size_t)c->world;
    if (capacity != (int64_t)total)
        return fail(D2D_ERR_INVALID, "the gathered map holds %lld floats (%d ranks), the buffer %lld", (long long)total, c->world, (long long)capacity);
    int rc = set_device(c);
    if (rc) return rc;
    if ((rc = join_comm(c, what))) return rc;
    HIP_TRY(hipMemcpyAsync(out, c->d_gather[what].p, total * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return D2D_OK;
}

int d2d_comm_allreduce_vjp(d2d_ctx* c) {
    if (!c) return fail(D2D_ERR_INVALID, "ctx is NULL");
    if (!c->comm) return fail(D2D_ERR_STATE, "d2d_comm_init must come first");
    if (!c->have_vjp) return fail(D2D_ERR_STATE, "no scene-VJP sweep has run");
    int rc = set_device(c);
    if (rc) return rc;
    if ((rc = ensure_comm_stream(c))) return rc;
    // on the communication stream like the gathers (collectives of one communicator execute in issue order), behind the
    // reduction kernel that produced d_vjp; d2d_get_scene_vjp and the next sweep's reduction wait for it
    if ((rc = comm_after_main(c))) return rc;
    const size_t n = (size_t)(4 * c->N + 2) + (c->vjp_has_coef ? 2 * (size_t)c->N : (c->vjp_has_phi ? (size_t)c->N : 0));
    RCCL_TRY(rccl().AllReduce(c->d_vjp.p, c->d_vjp.p, n, ncclFloat64, ncclSum, c->comm, c->comm_stream));
    HIP_TRY(hipEventRecord(c->ev_done[2], c->comm_stream));
    c->inflight[2] = true;
    c->vjp_reduced = true;
    return D2D_OK;
}

int d2d_comm_allreduce_host(d2d_ctx* c, double* values, int32_t n, int32_t op) {
    if (!c || !values) return fail(D2D_ERR_INVALID, "NULL argument");
    if (!c->comm) return fail(D2D_ERR_STATE, "d2d_comm_init must come first");
    if (n <= 0 || n > 4096) return fail(D2D_ERR_INVALID, "n must lie in 1..4096");
    if (op != 0 && op != 1) return fail(D2D_ERR_INVALID, "op must be 0 (sum) or 1 (max)");
    int rc = set_device(c);
    if (rc) return rc;
    if ((rc = c->d_hostred.ensure((size_t)n))) return rc;
    if ((rc = join_all_comm(c))) return rc;  // this one runs on the main stream: behind every collective in flight
    HIP_TRY(hipMemcpyAsync(c->d_hostred.p, values, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    RCCL_TRY(rccl().AllReduce(c->d_hostred.p, c->d_hostred.p, (size_t)n, ncclFloat64, op ? ncclMax : ncclSum, c->comm, c->stream));
    HIP_TRY(hipMemcpyAsync(values, c->d_hostred.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return D2D_OK;
}

int d2d_last_kernel_ms(d2d_ctx* c, float* ms) {
    if (!c || !ms) return fail(D2D_ERR_INVALID, "NULL argument");
    if (!c->have_kernel_time) return fail(D2D_ERR_INVALID, "no timed sweep: set the \"time_kernel\" option, then launch");
    int rc = set_device(c);
    if (rc) return rc;
    HIP_TRY(hipEventSynchronize(c->evk1));
    HIP_TRY(hipEventElapsedTime(ms, c->evk0, c->evk1));
    return D2D_OK;
}

int d2d_timer_begin(d2d_ctx* c) {
    if (!c) return fail(D2D_ERR_INVALID, "ctx is NULL");
    int rc = set_device(c);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    return D2D_OK;
}

int d2d_timer_end(d2d_ctx* c, float* ms) {
    if (!c || !ms) return fail(D2D_ERR_INVALID, "NULL argument");
    int rc = set_device(c);
    if (rc) return rc;
    if ((rc = join_all_comm(c))) return rc;  // the timed region ends when the last collective has landed
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    HIP_TRY(hipEventSynchronize(c->ev1));
    HIP_TRY(hipEventElapsedTime(ms, c->ev0, c->ev1));
    return D2D_OK;
}

}  // extern "C"
