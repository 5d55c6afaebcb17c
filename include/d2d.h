/*
 * d2d.h -- C ABI of libd2d.so, the MI355X (gfx950) drop-in for DiffeRT2d's hot path.
 *
 * DiffeRT2d (v0.4.0) is pure Python on JAX: it has no FFI, its extension points are Python
 * protocols.  This header is the boundary a maintainer would bind with ctypes/cffi from
 * differt2d/scene.py (see INTEGRATION.md for the stub).  Each entry point cites the
 * reference interface it replaces (paths relative to the DiffeRT2d checkout).
 *
 * Conventions
 *   - every function returns D2D_OK (0) or a negative d2d_status; nothing throws across the
 *     ABI; d2d_last_error() returns a thread-local, human-readable message for the last failure;
 *   - the caller owns all host buffers (C-contiguous fp32 / int32 / uint8); the library owns
 *     every device buffer inside d2d_ctx; one ctx = one GPU + one HIP stream; calls on one ctx
 *     are serialised by the caller, different ctxs may be driven from different threads;
 *   - all floating point is IEEE fp32 with one rounding per operation (no fma contraction,
 *     correctly rounded divide/sqrt), operations in the order the reference writes them;
 *   - there is NO CPU fallback: without a usable gfx950 device d2d_create fails.
 */
#ifndef D2D_H
#define D2D_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D2D_MAX_ORDER 4 /* highest interaction order a sweep accepts */
#define D2D_ABI_VERSION 12 /* (d2d_power_profile_launch / d2d_get_power_profile, d2d_strongest_paths_launch /
                              d2d_get_strongest_paths, d2d_coherent_field_launch / d2d_get_coherent_field,
                              d2d_frequency_response_launch / d2d_get_frequency_response and d2d_power_angle_launch /
                              d2d_get_power_angle, d2d_array_response_launch / d2d_get_array_response,
                              d2d_array_frequency_response_launch / d2d_get_array_frequency_response,
                              d2d_beam_response_launch / d2d_get_beam_response, d2d_material_response_launch /
                              d2d_get_material_response, d2d_material_eps_vjp_launch / d2d_get_material_eps_vjp,
                              d2d_field_position_vjp_launch / d2d_get_field_position_vjp and
                              d2d_field_walls_vjp_launch / d2d_get_field_walls_vjp are
                              additive: no struct, enum or existing entry point changed with them, so the version did not) */

typedef enum d2d_status {
    D2D_OK = 0,
    D2D_ERR_INVALID = -1,     /* bad argument (NULL, negative size, order > D2D_MAX_ORDER, alpha <= 0 ...) */
    D2D_ERR_HIP = -2,         /* a HIP runtime call failed */
    D2D_ERR_NO_DEVICE = -3,   /* no gfx950 device visible */
    D2D_ERR_UNSUPPORTED = -4, /* feature outside the native closed set (e.g. ImagePath with RIS objects) */
    D2D_ERR_STATE = -5,       /* call order violated (e.g. sweep before d2d_set_scene / d2d_set_grid) */
    D2D_ERR_COMM = -6         /* RCCL failure */
} d2d_status;

/* Object kinds, differt2d/geometry.py:542-721 (Wall), :683-721 (RIS), :352-431 (Vertex). */
enum { D2D_WALL = 0, D2D_RIS = 1, D2D_VERTEX = 2 };

/* Path solver = `path_cls`, differt2d/scene.py:1814 (ImagePath geometry.py:1013-1114,
 * MinPath :1207-1288, FermatPath :1117-1204). */
enum { D2D_SOLVER_IMAGE = 0, D2D_SOLVER_MINPATH = 1, D2D_SOLVER_FERMAT = 2 };

/* Activation = `function` kwarg of differt2d/logic.py:258-312. */
enum { D2D_ACT_HARD_SIGMOID = 0, D2D_ACT_SIGMOID = 1 };

/* Natively fused `fun` (PathFun, differt2d/scene.py:51):
 *   RECEIVED_POWER  differt2d/utils.py:17-54        r_coef**n / (height^2 + length^2)
 *   LENGTH_SQUARED  tests/test_scene.py:444-445     path.length() ** 2
 *   LENGTH          differt2d/geometry.py:811-819   path.length()
 *   ONE             1.0 (the map then counts valid paths -- "intersection counts")
 *   RECEIVED_POWER_PER_OBJECT   the `interacting_objects` argument of PathFun put to use (differt2d/scene.py:51, 1136-1154): one
 *                   reflection coefficient per object (d2d_set_reflection_coefs) instead of one for all,
 *                       num = 1;  for o in interacting_objects (candidate order):  num = num * coef[o]     (fp32, left fold)
 *                       f   = num / (height^2 + length^2)
 *                   Order 0 has num = 1.  With every coefficient equal to c this is RECEIVED_POWER(r_coef = c) bit for bit for the
 *                   orders 0..3 (lax.integer_pow's square-and-multiply and the left fold coincide there); at order 4 the two may
 *                   differ by an ulp, and the left fold is the definition.  d2d_params.r_coef is ignored. */
enum {
    D2D_FUN_RECEIVED_POWER = 0,
    D2D_FUN_LENGTH_SQUARED = 1,
    D2D_FUN_LENGTH = 2,
    D2D_FUN_ONE = 3,
    D2D_FUN_CUSTOM = 4, /* values and derivatives supplied per (candidate, cell): d2d_set_path_fun_values; value+grad launches only */
    D2D_FUN_RECEIVED_POWER_PER_OBJECT = 5 /* ImagePath sweeps only; needs d2d_set_reflection_coefs */
};

/* Which end of the paths the grid cells are. */
enum { D2D_GRID_RX = 0, D2D_GRID_TX = 1 };

/* How a sweep combines with what the output map already holds. */
enum {
    D2D_OUT_OVERWRITE = 0, /* Z  = facc                                              */
    D2D_OUT_ADD = 1        /* Z  = Z + facc   (reduce_all over transmitters, differt2d/scene.py:1939-1952) */
};

/* Everything Scene.accumulate_on_receivers_grid_over_paths threads down to Path.is_valid and
 * `fun` (differt2d/scene.py:1803-1826; kwargs -> differt2d/geometry.py:910-919, logic.py:258-267). */
typedef struct d2d_params {
    int32_t min_order;  /* differt2d/scene.py:1817 */
    int32_t max_order;  /* differt2d/scene.py:1818 */
    int32_t approx;     /* 0 = jnp.logical_*, 1 = min/max/activation (differt2d/logic.py:315-537) */
    int32_t act;        /* D2D_ACT_* */
    float alpha;        /* differt2d/defaults.py:3 (100.0) */
    float tol;          /* differt2d/geometry.py:915 (1e-2): loss tolerance of is_valid */
    float patch;        /* differt2d/geometry.py:916 / defaults.py:7 (0.0) */
    float seg_tol;      /* differt2d/geometry.py:89 (0.005); not reachable from the reference's sweep kwargs */
    int32_t fun_id;     /* D2D_FUN_* */
    float r_coef;       /* differt2d/defaults.py:12 (0.5) */
    float height;       /* differt2d/defaults.py:15 (0.1) */
    int32_t solver;     /* D2D_SOLVER_* */
    int32_t steps;      /* differt2d/optimize.py:50 (100): Adam steps of MinPath / FermatPath */
    int32_t out_mode;   /* D2D_OUT_* */
    int32_t grid_role;  /* D2D_GRID_RX: the grid cells are receivers and `tx` is the transmitter
                           (accumulate_on_receivers_grid_over_paths, differt2d/scene.py:1803-1953);
                           D2D_GRID_TX: the grid cells are transmitters and the `tx` argument of the launch is the
                           fixed RECEIVER (accumulate_on_transmitters_grid_over_paths, differt2d/scene.py:1489-1648);
                           the per-cell gradient is then taken w.r.t. the transmitter (scene.py:1617-1620).
                           TX grids run the culled kernels only while a path with a zero-length segment (a step of the backward
                           scan with un == 0, loss >= 0.999) is EXACTLY invalid under `tol` / `alpha` / the activation: hard
                           tol <= 0.5; hard_sigmoid alpha (tol - 0.999) + 3 <= 0; sigmoid alpha (tol - 0.999) <= -89.5 (e.g.
                           NOT sigmoid with alpha = 10).  Otherwise every (cell, candidate) is evaluated -- correct, tens of
                           times slower, and counted by d2d_debug_txg_fallbacks */
    int32_t strict_nan; /* value+grad sweeps only.  The reference's reverse-mode autodiff returns NaN for a cell whenever the
                           backward scan of ANY candidate -- valid or not -- hits un == 0 (differt2d/geometry.py:1105) or, in
                           the approx modes, a zero-length segment (normalize, :227-228).  0 (default): candidates that tile
                           culling proves invalid are not evaluated; a separate NaN scan (conservative test per 8 x 8 patch and
                           candidate, then the backward scan itself for the few survivors) finds every such cell and poisons
                           the gradient map and the scene VJP exactly as the exhaustive evaluation does.  1: every candidate of
                           every cell is evaluated in full (about 40x slower; the cross-check the tests hold 0 against) */
    int32_t many;       /* differt2d/optimize.py:142: random starts per candidate of MinPath / FermatPath, best recorded loss
                           wins (0 or 1 = one start; the path classes default to 1, differt2d/geometry.py:1198, 1282) */
    int32_t reserved[1];
} d2d_params;

typedef struct d2d_ctx d2d_ctx;

/* ---- library / device ------------------------------------------------------------------ */

int d2d_abi_version(void);
const char* d2d_last_error(void);
/* Number of visible HIP devices (0 is not an error). */
int d2d_device_count(int* count);
/* Fills name (<= cap bytes), number of CUs and total global memory of a device. */
int d2d_device_info(int device, char* name, int cap, int* cus, int64_t* mem_bytes);

/* One context per GPU. Fails with D2D_ERR_NO_DEVICE when `device` does not exist. */
int d2d_create(int device, d2d_ctx** ctx);
void d2d_destroy(d2d_ctx* ctx);
int d2d_synchronize(d2d_ctx* ctx);

/* ---- scene (replaces Scene.objects / Scene.from_walls_array, differt2d/scene.py:191, 413-426) -- */

/* objects: xys[N][2][2] (origin, dest; a Vertex stores its point in both rows), kind[N]
 * (D2D_WALL / D2D_RIS / D2D_VERTEX, NULL = all walls), phi[N] (RIS angle, NULL = pi/4).
 * Size: the image-method sweeps keep per-object tables in LDS -- up to ~1 300 objects in 64 KB with several workgroups per CU,
 * up to ~2 400 with one workgroup per CU (156 of gfx950's 160 KB); a sweep over a bigger scene returns D2D_ERR_UNSUPPORTED.
 * Scenes above 4 095 objects sweep without region lists (12-bit object indices in the list entries). */
int d2d_set_scene(d2d_ctx* ctx, const float* xys, const uint8_t* kind, const float* phi, int32_t n_objects);
/* (A scene that is resident already -- bit-identical arguments -- is recognised: nothing is uploaded and the scene-only
 * masks and the schedule's work history stay valid; the candidate mask is reset to "all" as always.) */

/* filter_objects of Scene.all_path_candidates (differt2d/scene.py:1089-1134): allowed[i] != 0
 * means object i may appear in a path candidate; NULL = all. Filtered objects still occlude. */
int d2d_set_candidate_mask(d2d_ctx* ctx, const uint8_t* allowed);

/* Reflection coefficient of every object for D2D_FUN_RECEIVED_POWER_PER_OBJECT: coef[n], n = the scene's number of objects
 * (D2D_ERR_INVALID otherwise, and for a value that is not finite; negative values and zero are allowed).  A host array, copied
 * before the call returns.  The values belong to the resident scene: a d2d_set_scene that uploads another scene drops them,
 * one that recognises the resident scene keeps them.  Setting the values that are set already uploads nothing; NULL / 0 drops
 * them.  A sweep with fun_id D2D_FUN_RECEIVED_POWER_PER_OBJECT returns D2D_ERR_STATE without coefficients and
 * D2D_ERR_UNSUPPORTED (naming the function) with the MinPath / FermatPath solvers or through the instrumented build
 * (d2d_power_map_stats, d2d_power_map_wave_cycles); d2d_power_map_launch and d2d_power_map_vg_launch run it in both grid roles,
 * all three validity modes, orders 0..D2D_MAX_ORDER, with D2D_OUT_ADD, the candidate mask, cotangents and either strict_nan.
 * d2d_valid_paths / d2d_trace_paths ignore fun_id as ever. */
int d2d_set_reflection_coefs(d2d_ctx* ctx, const float* coef, int32_t n);

/* Context-free candidate enumeration (pure host integer code, replaces the Rust
 * differt_core.rt.CompleteGraph / DiGraph.all_paths calls at differt2d/scene.py:153-175): for each order
 * k ascending, every tuple of k allowed object indices with no two equal neighbours, lexicographic
 * (recorded order: docs/source/notebooks/cost20120_helsinki_model.ipynb cell 20). cand is row-major
 * [count][D2D_MAX_ORDER], -1 padded; either output pointer may be NULL. */
int d2d_count_candidates(int32_t n_objects, const uint8_t* allowed, int32_t min_order, int32_t max_order, int64_t* count);
int d2d_enumerate_candidates(int32_t n_objects, const uint8_t* allowed, int32_t min_order, int32_t max_order, int32_t* cand,
                             int32_t* order, int64_t capacity);

/* Number of path candidates sum_k |{tuples of length k, no equal neighbours}| for the current
 * scene and mask (differt2d/scene.py:122-175; differt-core 0.0.31 CompleteGraph.all_paths). */
int d2d_num_candidates(d2d_ctx* ctx, int32_t min_order, int32_t max_order, int64_t* count);

/* Writes the candidate list itself (row-major [count][D2D_MAX_ORDER], -1 padded) and each
 * candidate's order, in the reference's enumeration order. Either pointer may be NULL. */
int d2d_list_candidates(d2d_ctx* ctx, int32_t min_order, int32_t max_order, int32_t* cand, int32_t* order,
                        int64_t capacity);

/* ---- grid sweep (replaces Scene.accumulate_on_receivers_grid_over_paths, differt2d/scene.py:1803-1953,
 *      for one transmitter at a time; X, Y as produced by Plottable.grid, differt2d/abc.py:57-81) -------- */

/* Uploads the receiver grid (row-major [m][n], any coordinates) and (re)allocates the resident
 * output maps; the value map is zeroed.  A grid that is resident already (same m, n and bit patterns, compared byte for
 * byte with a host copy the context keeps: 8 bytes of host memory per cell) is not uploaded again and keeps everything
 * keyed to it (the regions' bounding boxes, the work history of the patch schedule): the reference's callers pass X, Y with
 * every call (differt2d/scene.py:1803-1826). */
int d2d_set_grid(d2d_ctx* ctx, const float* X, const float* Y, int32_t m, int32_t n);
/* The same with a caller-supplied version token instead of the content hash: version != 0 asserts that equal versions
 * mean equal contents (an immutable array the caller has passed before, like the reference's JAX arrays); 0 = hash.  A strided
 * sample of ~500 cells of both arrays is compared beside the token (an array whose read-only flag was flipped, written through
 * and flipped back has the same token: a change that misses every sampled cell is not seen). */
int d2d_set_grid_versioned(d2d_ctx* ctx, const float* X, const float* Y, int32_t m, int32_t n, uint64_t version);
/* Diagnostic: how many d2d_set_grid / d2d_set_grid_versioned calls found their grid resident already. */
int d2d_debug_grid_reuses(d2d_ctx* ctx, int64_t* count);
/* Diagnostic: the launch shape of the last RX-grid value sweep -- waves_per_patch = 1 (one wave per patch, the dearest
 * patches cut in parts), 4 (patches shared by 4 waves prefix by prefix) or, with candidates = 1, the 4 / 8 / 16 waves of
 * the kernel that shares a patch candidate by candidate (options coop_waves, coop_max_tiles); 0 before any sweep. */
int d2d_debug_sweep_shape(d2d_ctx* ctx, int32_t* waves_per_patch, int32_t* candidates);
/* Diagnostic: how many TX-grid sweeps of this context ran the EXHAUSTIVE kernel although culling was asked for (no
 * strict_nan, no "txg_exhaustive" option), because a degenerate path is not exactly invalid under their parameters (see
 * d2d_params.grid_role) -- so that a bench or a profile does not misattribute that time. */
int d2d_debug_txg_fallbacks(d2d_ctx* ctx, int64_t* count);
/* Diagnostic: how often the last-segment masks of the leaf regions ("hidden_masks" option) were built, and whether the
 * context holds valid ones now. */
int d2d_debug_hidden_masks(d2d_ctx* ctx, int64_t* builds, int32_t* valid);

/* Initial guesses of the optimiser-based solvers for the NEXT sweeps: theta0[n_candidates * many][D2D_MAX_ORDER]
 * (n_rows = n_candidates * max(1, params->many)), candidates in enumeration order, the `many` starts of one candidate
 * consecutive (unused entries ignored); every RX cell starts from the same guesses, as in the reference
 * (differt2d/scene.py:1887-1890, optimize.py:132, 174-178). */
int d2d_set_theta0(d2d_ctx* ctx, const float* theta0, int64_t n_rows);

/* The optimiser of the MinPath / FermatPath solvers for the NEXT sweeps and traces (differt2d/optimize.py:44-51: any
 * optax.GradientTransformation; default optax.adam(learning_rate=0.1), optimize.py:83).  Native: Adam with any
 * hyper-parameters (optax.adam(learning_rate, b1, b2, eps), eps_root = 0) -- they are Python floats on the reference's
 * side, hence doubles here; the gradients through the solver (reverse mode and forward tangents) follow them.
 *   D2D_OPT_ADAM           optax.adam(learning_rate, b1, b2, eps): decay rates in [0, 1), eps >= 0 and finite.
 *   D2D_OPT_SGD            optax.sgd(learning_rate) (momentum=None: x += -lr * g, no state); b1, b2, eps are ignored.
 *   D2D_OPT_SGD_MOMENTUM   optax.sgd(learning_rate, momentum=b1, nesterov=b2): b1 = the momentum in [0, 1) (0 included: a
 *                          trace of decay 0 still carries a NaN forward, unlike D2D_OPT_SGD), b2 = the Nesterov flag, 0 or
 *                          1; eps is ignored.
 * The learning rate must be finite.  Any other kind: D2D_ERR_UNSUPPORTED. */
#define D2D_OPT_ADAM 0
#define D2D_OPT_SGD 1
#define D2D_OPT_SGD_MOMENTUM 2
int d2d_set_optimizer(d2d_ctx* ctx, int32_t kind, double learning_rate, double b1, double b2, double eps);

/* Launches the fused forward sweep for transmitter tx[2] on the ctx stream (asynchronous).
 * Inputs and outputs stay resident in HBM. params->solver selects ImagePath (fused image-method kernel) or
 * MinPath / FermatPath (per-cell optimiser loop of params->steps iterations, hand-derived gradient). */
int d2d_power_map_launch(d2d_ctx* ctx, const d2d_params* params, const float* tx);

/* ---- value + gradient (replaces grad=True / value_and_grad=True of the sweep, differt2d/scene.py:1920-1923,
 *      and the user-side jax.value_and_grad over scene parameters, examples/plot_power_optimize.py:78-93) ---- */

/* Cotangent of the value map for the scene-parameter VJP: cot[m*n], or NULL for all ones (the gradient of
 * sum(Z)). Reset by d2d_set_grid. */
int d2d_set_cotangent(d2d_ctx* ctx, const float* cot);

/* Gradient of a sweep whose path function `fun` is an arbitrary host callable (the reference differentiates any JAX
 * callable, differt2d/scene.py:1892-1923: d/d cell of sum_c valid_c * fun_c).  The host traces the paths
 * (d2d_trace_paths), evaluates fun and its derivative on them and hands both over:
 *   f[n_candidates][m*n]                          fun of (candidate, cell),
 *   xys_bar[n_candidates][m*n][D2D_MAX_ORDER+2][2] d fun / d path points (rows 0 .. order+1 of a candidate are read; a
 *                                                 derivative w.r.t. tx.xy / rx.xy as arguments of fun is added to rows 0 / order+1),
 * candidates in the sweep's order (orders min_order..max_order, lexicographic over the allowed objects -- the order of
 * d2d_trace_paths' candidate list built by the reference's all_path_candidates).  A following d2d_power_map_vg_launch with
 * params->fun_id == D2D_FUN_CUSTOM (image solver: every candidate of every cell is evaluated, as under strict_nan;
 * MinPath / FermatPath: the reverse pass over the stored trajectory, option "opt_grad_mode" 0, with the theta0 rows the
 * paths were traced with) then
 * chains them through the hand-derived adjoint of the validity and of the path method: d2d_get_map returns
 * sum_c valid_c * f_c and d2d_get_grad_rx its derivative w.r.t. the cell, d2d_get_scene_vjp the pull-back to the fixed
 * end point and the wall end points THROUGH THE PATHS (fun's own dependence on the objects is the caller's).
 * Host arrays, copied before the call returns; NULL / 0 drops them; dropped by d2d_set_grid, by a different scene and by
 * a different candidate mask.  D2D_ERR_STATE from the launch
 * when n_candidates is not the number of candidates the sweep walks. */
int d2d_set_path_fun_values(d2d_ctx* ctx, const float* f, const float* xys_bar, int64_t n_candidates);

/* Value+grad sweep.  ImagePath: fused, hand-derived reverse mode.  MinPath / FermatPath (differt2d/geometry.py:1117-1288):
 * hand-derived reverse mode through the reference's lax.scan of Adam steps (differt2d/optimize.py:83-97): the solver writes its
 * trajectory to HBM and the steps are walked backwards (d2d_optrev.hpp; 16 bytes per step and unknown, grids whose
 * trajectories exceed "opt_traj_mb" are swept in chunks of cells), for Wall, RIS (incl. phi, geometry.py:698-711) and Vertex
 * objects; "opt_grad_mode" = 1 selects the older forward-tangent kernel (d2d_optgrad.hpp), kept as an independent
 * cross-check.  Writes the value map exactly as
 * d2d_power_map_launch does, the per-cell gradient d Z[i,j] / d rx[i,j] (resident, [m][n][2]) and, when
 * want_scene_vjp != 0, the VJP of the map w.r.t. the transmitter position and every object end point,
 * contracted with the cotangent. out_mode D2D_OUT_ADD accumulates all of them (reduce_all). Asynchronous. */
int d2d_power_map_vg_launch(d2d_ctx* ctx, const d2d_params* params, const float* tx, int32_t want_scene_vjp);

/* Synchronises and copies the per-cell gradient map to out[m*n*2] (last axis d/dx, d/dy). */
int d2d_get_grad_rx(d2d_ctx* ctx, float* out);

/* Synchronises and copies the scene-parameter VJP: tx_bar[2] (the fixed end point), xys_bar[N][2][2] (object end points;
 * may be NULL) and phi_bar[N] (RIS angles, differt2d/geometry.py:683-721; may be NULL; identically 0 after an ImagePath
 * sweep, whose candidates hold Wall objects only). */
int d2d_get_scene_vjp(d2d_ctx* ctx, float* tx_bar, float* xys_bar, float* phi_bar);

/* Synchronises and copies <cot, d Z / d coef> [N] of the last scene-VJP sweep(s) (d2d_power_map_vg_launch with
 * want_scene_vjp != 0): the derivative of the objective w.r.t. the reflection coefficients of
 * D2D_FUN_RECEIVED_POWER_PER_OBJECT,  coef_bar[o] = sum over cells and candidates, once per occurrence i of o in the candidate, of
 * cot * valid * (prod_{q != i} coef[cand_q]) / (height^2 + length^2)  -- the product of the OTHER coefficients is formed explicitly,
 * nothing is divided by a coefficient (zero is a legal value).  It accumulates over D2D_OUT_ADD launches exactly as tx_bar /
 * xys_bar do, is all zeros when none of the accumulated sweeps used that function, and D2D_ERR_STATE without a scene-VJP sweep.
 * The reference's reverse-mode NaN traps sit on the way from the path points back to the geometry, and the coefficients are not
 * on that way: cells whose grad_rx is NaN (d2d_params.strict_nan) poison tx_bar / xys_bar, never coef_bar.
 * Stored as a fourth block of the resident VJP ([4N] end points, [2] fixed point, [N] phi, [N] coef), which
 * d2d_comm_allreduce_vjp then covers by length -- that path has NEVER run on more than one rank. */
int d2d_get_reflection_coefs_vjp(d2d_ctx* ctx, float* coef_bar /* [N] */);

/* Same sweep through the instrumented build of the kernel (same results, not for timing): fills
 * stats[D2D_NUM_STATS] with executed-work counters summed over waves (one count = one 64-lane wave):
 *   [0] candidates evaluated (interaction points + on_objects)   [1] ... that reached the loss stage
 *   [2] ... that reached the occlusion loop                      [3] ... with a non-zero validity (valid * fun evaluated)
 *   [4] segment/wall tests evaluated                             [5] tests that took the exact-divide path
 *   [6] sum of k over [0]    [7] sum of k over the candidates whose loss was evaluated exactly    [8] sum of (k+1) over [3]
 *   [9] tile-culling levels evaluated (one count = 64 candidates x 4 vertex evaluations)
 *   [10..14] shader-clock ticks summed over waves: patch prologue, order 0, order 1, order 2, exact evaluation of survivors
 * bench.py prices these with SURVEY.md section 8(d)'s per-unit FLOP figures. */
#define D2D_NUM_STATS 16
int d2d_power_map_stats(d2d_ctx* ctx, const d2d_params* params, const float* tx, uint64_t* stats);

/* Diagnostic (instrumented build): shader-clock ticks each 64-lane wave (= one 8 x 8 patch of cells, row-major over
 * patches) spent in the sweep -- the load-balance picture behind the roofline numbers. */
int d2d_power_map_wave_cycles(d2d_ctx* ctx, const d2d_params* params, const float* tx, uint64_t* cycles, int64_t capacity,
                              int64_t* n_waves);

/* Launch-shape tuning of a context; never changes a result bit (tests sweep these to cover every kernel variant).
 *   "split_max_tiles": launches of at most this many 8 x 8 patches share every patch between 4 waves (0 = never; default -1:
 *                  5120 with hard validity, never with hard_sigmoid -- those share candidate by candidate, "coop_waves", or
 *                  run one wave per patch; never with sigmoid validity unless "split_sigmoid" is non-zero)
 *   "coop_waves": the smallest launches share every patch between this many waves CANDIDATE BY CANDIDATE, wave 0 adding the
 *                  contributions in the reference's order (4, 8 or 16; 0 = never; default -1: by the launch's size and
 *                  validity mode -- 16 waves up to 256 patches and 8 up to 640 (hard) / 2304 (hard_sigmoid), 16 / 8 / 4 up
 *                  to 640 / 1600 / 4096 patches with sigmoid validity, and never more than "split_max_tiles");
 *                  "coop_max_tiles": replaces the upper limit (-1)
 *   "hidden_masks": non-zero (default) = forward RX-grid sweeps with region lists keep, per leaf region and wall, a 64-bin mask
 *                  of where the wall is certainly hidden from the WHOLE region (scene, grid and validity mode only: built
 *                  by the second launch in a row that would use it, kept until the scene, the grid or the mode changes);
 *                  candidates whose last interaction point can only lie in hidden bins leave the region's list, and order-1
 *                  candidates the patch's culling (same results); "hidden_min_tiles": only launches of at least this many
 *                  patches use them (default 400: smaller ones are latency-bound and lose more to the extra load than they gain)
 *   "sched_min_tiles": launches of at least this many patches start their dearest patches first (default 2048)
 *   "heavy_split": with a work history and max_order == 2, this many of the dearest patches of a launch that is too big to
 *                  share every patch are cut in four parts swept by separate workgroups (0 = none, at most a quarter of the
 *                  patches; default -1: 3 patches in 32 when the launch holds fewer than 4 patches per wave slot of the
 *                  chip, else 64)
 *   "cost_history": non-zero (default) = a launch that sweeps the same grid as the previous one orders its patches by the
 *                   work each took then (counted by the kernels); zero = always by the geometric proxy
 *   "pair_masks": zero = do not build / use the wall-to-wall occlusion masks (A/B and tests; same results)
 *   "nan_scan": the pass beside a culled value+grad sweep that finds the reference's autodiff NaN cells (d2d_params.strict_nan):
 *                  1 (default) = one workgroup of 16 waves per region of 4 x 4 patches, 2 = one wave per patch (same flags),
 *                  0 = off (round 3's behaviour: NaN only inside the candidates the sweep evaluates; A/B);
 *                  "nan_scan_stats": non-zero = count its work (d2d_debug_nan_scan; slows the scan down)
 *                  (it runs on a stream of its own at the lowest priority and leaves flags that a small kernel applies once
 *                  both are through)
 *                  "nan_scan_wqcap" / "nan_scan_rb": entries of a region's probe queue / batches per round of its list that the
 *                  two-level scan USES (0 = default: all it has; tests set them small so that a full queue and a full list are the
 *                  rule instead of a rare event -- same flags whatever the values).  Any of these two, or "nan_scan_stats", selects the
 *                  region kernel's debug instance (run-time sizes, counters through LDS); the product instance has neither
 *   "comm_prio": priority of the stream the RCCL collectives run on beside the next sweep: -1 lowest, 0 (default) normal, 1 highest;
 *                  set it BEFORE the first collective (D2D_ERR_STATE afterwards)
 *   "opt_parallel": zero = MinPath / FermatPath sweeps walk the candidates one after the other in every lane (same results)
 *   "opt_grad_mode": gradients through the MinPath / FermatPath solvers: 0 (default) reverse mode over the stored trajectory,
 *                   1 forward tangents carried through the loop (same derivative; NaN only where a local partial derivative
 *                   is infinite vs. also where an accumulated tangent overflowed); "opt_traj_mb": device memory the
 *                   trajectory store of the reverse mode may take (default 16384)
 *   "txg_exhaustive": non-zero = TX-grid value sweeps use the exhaustive kernel instead of the culled one (same results)
 *   "region_lists": zero = no region candidate lists: every patch enumerates the prefixes of its candidates itself
 *                   (default non-zero: culled RX-grid launches of max_order >= 2 build, per launch, for every region of
 *                   patches the list of candidates that the tile culling cannot drop for the region's bounding box, and
 *                   the patches only test and evaluate those; same results)
 *   "region_size" / "region_size_top": leaf regions are region_size x region_size patches (default 4, 1..64); their
 *                   lists are refined from those of regions of region_size_top patches a side (default 16, rounded down to
 *                   a multiple of region_size), which are built by enumeration
 *   "region_slices": lists per top region = slices of first walls = waves that enumerate it (default 0: a quarter of
 *                   the allowed objects); "region_budget_mb": device memory of ALL list pools (default 24576: an upper bound; the pipeline keeps one pool per
 *                   rotating set, three in all, so a pool may grow to a third of it); a list
 *                   that does not fit is marked as not listed and the patches of its region enumerate (same results)
 *   "pipeline": non-zero (default) = everything a launch rebuilds (shadow masks, region lists, the schedule's sort) lives
 *                   in three rotating sets and is built on side streams beside the previous launches' sweeps; the work
 *                   history a schedule is sorted by is then three launches old instead of one; zero = on the
 *                   launch's own stream, in front of its sweep (same results)
 *   "unpiped_max_tiles": launches of orders <= 1 over at most this many 8 x 8 patches (default 256) prepare on the sweep's own
 *                   stream whatever "pipeline" says: a small call is launch latency, and the side stream's fork and join cost it
 *                   8 us of 45 (same results); 0 = never
 *   "fwd_waves": patches per workgroup
 *                   of the sweep with region lists (0 default: 4 when the per-wall LDS table is big, else 1)
 *   "region_budget_mb" also bounds the growth of the list pool: it starts at 256 MB and is quadrupled (up to the budget,
 *                   a third of it per pool) when a launch's lists did not fit (read back without waiting); when the device cannot
 *                   provide the pool, the launch enumerates instead (same results) and later launches ask for a quarter
 *   "time_kernel": non-zero = bracket the sweep kernel of every launch with HIP events (see d2d_last_kernel_ms)
 * No reference counterpart (XLA picks its own launch shapes). Returns D2D_ERR_INVALID for an unknown name. */
int d2d_set_option(d2d_ctx* ctx, const char* name, int64_t value);

/* Diagnostics of the patch schedule (the order in which the culled kernels start their 8 x 8 patches; it changes
 * speed, never results): d2d_debug_get_schedule copies the order built by the last scheduled launch and its cost keys
 * (n = number of patches); d2d_debug_set_schedule makes later launches of exactly n patches use `order` (a permutation
 * of 0..n-1) instead; n = 0 removes the override. */
int d2d_debug_set_schedule(d2d_ctx* ctx, const int32_t* order, int64_t n);
int d2d_debug_get_schedule(d2d_ctx* ctx, int32_t* order, uint8_t* key, int64_t n);
/* Region candidate lists of the last launch that built any (all zeros otherwise): out[0] pool chunks handed out,
 * [1] pool chunks available, [2] patches left to the enumerating kernel, [3] leaf regions with a list that is not listed,
 * [4] / [5] / [6] entries of the leaf lists of order 2 / 3 / 4, [7] leaf regions.  Waits for the stream. */
int d2d_debug_region_stats(d2d_ctx* ctx, int64_t* out /* [8] */);
/* Counters of the last value+grad launch's NaN scan (option "nan_scan_stats" = 1; zeros otherwise): out[0] (patch, candidate)
 * pairs whose backward scan was probed cell by cell, [1] cells flagged NaN, [2] patches with a flagged cell; two-level scan only:
 * [3] probes a wave made itself because its region's queue was full, [4] queue items refused because they named no patch of the
 * region or no object of the scene (an internal error: always 0), [5] rounds of the regions' lists.  Waits for the stream. */
int d2d_debug_nan_scan(d2d_ctx* ctx, int64_t* out /* [6] */);

/* The work history behind the schedule: what each of the n patches took in the last culled sweep (units of ~25
 * wave-instructions, counted by the kernels). */
int d2d_debug_get_work(d2d_ctx* ctx, uint32_t* work, int64_t n);

/* Duration of the sweep kernel proper of the last launch on this context -- without the preparation kernels in front
 * of it (shadow masks, patch schedule) and the VJP reduction behind it -- from HIP events recorded on the context's
 * stream; needs the "time_kernel" option. Waits for that kernel. This is the figure bench.py's roofline uses. */
int d2d_last_kernel_ms(d2d_ctx* ctx, float* ms);

/* Diagnostic: evaluates x[i] / y[i] on the GPU three ways -- q_fast: the kernels' bare fma chain on a refined
 * v_rcp; q_ref: the compiler's generic correctly rounded expansion; q_hostr: the bare chain on a host-computed
 * reciprocal. For operands in [2^-62, 2^62] (or x == 0) all three must be bit-identical. */
int d2d_selftest_div(d2d_ctx* ctx, const float* x, const float* y, int64_t n, float* q_fast, float* q_ref, float* q_hostr);

/* Diagnostic: the device's expf as the sigmoid activation uses it (the algorithm of glibc's expf, in double, rounded once:
 * d2d_kernels.hpp expf_libm) on x[n] -> y[n]; must equal the host C library's expf bit for bit. */
int d2d_selftest_expf(d2d_ctx* ctx, const float* x, int64_t n, float* y);

/* Diagnostic: the coherent field's phasor (differt2d_amd/csrc/d2d_phasor.hpp) on the device, f[n] (turns, in [0, 1)) -> c[n] =
 * cos(2 pi f), s[n] = sin(2 pi f); must equal the header's host build bit for bit. */
int d2d_selftest_phasor(d2d_ctx* ctx, const float* f, int64_t n, float* c, float* s);

/* Diagnostic: the power-angle profile's direction (differt2d_amd/csrc/d2d_angle.hpp) on the device, (dx[n], dy[n]) -> out[n] =
 * turns(dx, dy), the angle in turns in [0, 1) (NaN for (0, 0), NaN and inf); must equal the header's host build bit for bit. */
int d2d_selftest_angle(d2d_ctx* ctx, const float* dx, const float* dy, int64_t n, float* out);

/* Synchronises and copies the resident value map to out[m*n]. */
int d2d_get_map(d2d_ctx* ctx, float* out);

/* Convenience: d2d_set_grid + d2d_power_map_launch + d2d_get_map. */
int d2d_power_map(d2d_ctx* ctx, const d2d_params* params, const float* tx, const float* X, const float* Y,
                  int32_t m, int32_t n, float* out);

/* ---- individual paths (replaces Scene.all_paths / all_valid_paths / accumulate_over_paths,
 *      differt2d/scene.py:1156-1334; ImagePath.from_tx_objects_rx, differt2d/geometry.py:1013-1114;
 *      Path.on_objects / intersects_with_objects / is_valid / length, differt2d/geometry.py:811-963) ---- */

/* For each of the P (tx, rx) pairs and each of the C candidates (cand[C][D2D_MAX_ORDER] object
 * indices, order[C] their lengths) solves the path (or, when xys_in != NULL, takes the given points
 * xys_in[P][C][D2D_MAX_ORDER+2][2] and losses loss_in[P][C] (NULL = 0)) and evaluates it against the
 * current scene. Outputs (row-major, [P][C] leading): xys[..][D2D_MAX_ORDER+2][2] (unused rows NaN),
 * loss, valid (is_valid after nan_to_num; 0/1 in hard mode), and optionally on (on_objects),
 * hit (intersects_with_objects) and length (path_length). theta0[C * max(1, many)][D2D_MAX_ORDER] = initial parametric
 * coordinates of the optimiser-based solvers (MinPath geometry.py:1207-1288, FermatPath :1117-1204; the reference
 * draws them from a per-candidate PRNG key shared by all pairs, scene.py:1887-1890), theta0_rows = the number of rows the
 * caller provides (checked against C * max(1, many)); NULL / 0 for ImagePath. Synchronous. */
int d2d_trace_paths(d2d_ctx* ctx, const d2d_params* params, const float* tx, const float* rx, int32_t P,
                    const int32_t* cand, const int32_t* order, int32_t C, const float* theta0, int64_t theta0_rows,
                    const float* xys_in, const float* loss_in, float* xys, float* loss, float* valid, float* on, float* hit,
                    float* length);

/* ---- valid paths of a whole grid, sparse (the plug-in point for an arbitrary host `fun` on grids too big to trace densely:
 *      differt2d/scene.py:1892-1918 adds valid * fun(...), and valid is exactly 0 for nearly every (cell, candidate)) ---- */

/* Record launch of the culled forward sweep (ImagePath; hard or hard_sigmoid validity; the current scene, candidate mask and
 * grid; params->grid_role says which end the cells are, `fixed` is the other end; params->fun_id and out_mode are ignored):
 * finds every (cell, candidate of orders min_order..max_order) whose validity is not exactly zero and solves its path.
 * Two passes of the same sweep -- count per 8 x 8 patch, host scan, write -- then one thread per record for the path: no
 * global atomics.  Synchronous.  *count = how many there are; the library keeps them (grown when needed, dropped by a
 * d2d_set_grid of another grid) until the next call.  The resident value / gradient maps, the work history and the
 * schedule of the fused sweeps are not touched.
 * D2D_ERR_UNSUPPORTED: sigmoid validity (its sweeps skip candidates by the fused function's running sum), MinPath / FermatPath,
 * a TX grid whose sweep would not be culled (d2d_params.grid_role), more than 4 095 objects -- all decided before anything is
 * enqueued -- or a total that would take more than half of the free device memory (100 bytes per record; the message holds the
 * count) -- decided before the second pass.
 * D2D_ERR_STATE: the second pass disagreed with the first (an internal error; nothing is stored out of bounds). */
int d2d_valid_paths(d2d_ctx* ctx, const d2d_params* params, const float* fixed /* [2] */, int64_t* count);
/* Copies the records of the last d2d_valid_paths out: cell[n] (row-major index into the grid), cand[n][D2D_MAX_ORDER]
 * (-1 padded), order[n], xys[n][D2D_MAX_ORDER+2][2] (unused rows NaN), loss[n], valid[n], length[n] -- what d2d_trace_paths
 * returns for the same (pair, candidate), bit for bit.  Any pointer may be NULL; capacity (in records) must be at least the
 * count; the order of the records is unspecified. */
int d2d_get_valid_paths(d2d_ctx* ctx, int64_t capacity, int32_t* cell, int32_t* cand, int32_t* order, float* xys, float* loss,
                        float* valid, float* length);
/* Diagnostic ("time_kernel" option): kernel times of the last d2d_valid_paths that found records -- ms[0] pass 1 (count),
 * ms[1] pass 2 (write), ms[2] the paths of the records. */
int d2d_debug_valid_paths_ms(d2d_ctx* ctx, float* ms /* [3] */);

/* ---- per-cell power-delay profile: the fused sweep binned by path length (no reference counterpart: the reference reduces every
 *      cell to one number, differt2d/scene.py:1892-1918; mean excess delay and RMS delay spread follow from the profile) ---- */

/* Launches the bin build of the culled forward sweep for the fixed end point `fixed` on the ctx stream (asynchronous): the
 * profile out[nbins][m][n], fp32, of the current scene, candidate mask and grid.  `params` as for d2d_power_map_launch
 * (params->grid_role says which end the cells are), r_min, r_max fp32 and finite with r_max > r_min, nbins >= 1.  Definition:
 *
 *     inv = (float)nbins / (r_max - r_min)          // host, fp32: one subtraction, one division
 *     for candidates in the sweep's enumeration order:
 *         t = valid * fun                             // exactly the fused sweep's contribution (nan_to_num rules included)
 *         r = path_length(points)                     // the fp32 value the path function is evaluated with
 *         u = (r - r_min) * inv ;  b = (int)floorf(u) // fp32, no contraction
 *         if (u >= 0 && b < nbins) out[b][cell] = out[b][cell] + t    // NaN r / u: no bin
 *
 *   - Contributions that are exactly zero may be skipped; the sums are never -0.0.
 *   - Bins are half-open.  Anything outside [r_min, r_max) is dropped.
 *   - With nbins == 1 and a range that covers every path, out[0] equals the fused map bit for bit.
 *   - For any nbins over a covering range, the bins of a cell sum to the fused value up to fp32 summation order.
 *
 * One pass of one kernel (one wave per 8 x 8 patch, every lane the only writer of its cell: no atomics, the same bits run to
 * run) behind a zeroing of the profile on the same stream.  The resident value / gradient maps, the work history and the
 * schedule of the fused sweeps are not touched.  Every fused function but D2D_FUN_CUSTOM; D2D_FUN_RECEIVED_POWER_PER_OBJECT
 * with the coefficients of d2d_set_reflection_coefs, D2D_ERR_STATE without them.
 * D2D_ERR_INVALID: nbins < 1, r_max <= r_min, a bound that is not finite.
 * D2D_ERR_UNSUPPORTED (the message names the reason): sigmoid validity (its sweeps skip candidates by the fused function's
 * running sum), MinPath / FermatPath, D2D_FUN_CUSTOM, D2D_OUT_ADD, a TX grid whose sweep would not be culled
 * (d2d_params.grid_role; not counted by d2d_debug_txg_fallbacks), more than 4 095 objects, or nbins * m * n * 4 bytes above
 * half of the free device memory -- all decided before anything is enqueued. */
int d2d_power_profile_launch(d2d_ctx* ctx, const d2d_params* params, const float* fixed /* [2] */, float r_min, float r_max,
                             int32_t nbins);
/* Synchronises and copies the profile of the last d2d_power_profile_launch to out[nbins][m][n].  D2D_ERR_STATE before a launch,
 * after a launch that was refused, and after a d2d_set_grid of another grid (the profile goes with the grid). */
int d2d_get_power_profile(d2d_ctx* ctx, float* out /* [nbins][m][n] */);

/* ---- per-cell strongest paths: the k largest contributions of the fused sweep, with their lengths and wall sequences (no
 *      reference counterpart: the reference reduces every cell to one number; the dominant path, the share of the power that
 *      the few strongest paths carry, and channel taps follow from the slots) ---- */

#define D2D_TOP_MAX 8
/* Launches the top-k build of the culled forward sweep for the fixed end point `fixed` on the ctx stream (asynchronous), for
 * the current scene, candidate mask and grid.  `params` as for d2d_power_map_launch (params->grid_role says which end the
 * cells are); k lies in 1..D2D_TOP_MAX.  Definition, per cell:
 *
 *     slots empty;  total = +0.0f;  count = 0
 *     for candidates in the sweep's enumeration order:
 *         t = valid * fun            // exactly the fused sweep's contribution (nan_to_num rules included)
 *         r = path_length(points)    // the fp32 value the path function is evaluated with (what the profile bins by)
 *         total = total + t          // fp32: hence the fused map bit for bit
 *         if (t == 0) continue       // exact zeros of either sign take no slot
 *         count += 1
 *         key = bit pattern of fabsf(t), compared as uint32   // a total order; NaN ranks above inf
 *         insert (t, r, candidate) in front of the first slot whose key is STRICTLY smaller; the (k+1)-th falls off
 *
 *   - Slots are therefore sorted by key, descending.  Among equal keys the earlier candidate in enumeration order comes first
 *     and survives the cut.
 *   - "Strongest" means largest |t|.  A negative per-object coefficient gives negative contributions, and those compete by
 *     magnitude.
 *
 * Outputs, cell axes last:
 *     power   fp32  [k][m][n]                  the slot's t
 *     length  fp32  [k][m][n]                  the slot's r
 *     cand    int32 [k][m][n][D2D_MAX_ORDER]   wall indices of the path, -1 padded
 *     order   int32 [k][m][n]                  order of the path
 *     total   fp32  [m][n]                     the running sum over all candidates
 *     count   int32 [m][n]                     how many non-zero contributions the cell had
 *
 *   - count > k means something was cut.
 *   - An empty slot holds power = +0.0, length = NaN, order = -1 and cand = -1.
 *   - The top-k of the top-8 is the top-k under this rule: the kernel keeps D2D_TOP_MAX slots and stores the first k.
 *
 * One pass of one kernel (one wave per 8 x 8 patch, a lane's slots in registers, every lane the only writer of its cell and
 * writing all of it: no atomics, no zeroing, the same bits run to run).  The resident value / gradient maps, the work history,
 * the schedule of the fused sweeps, the records of d2d_valid_paths and the profile are not touched.  Every fused function but
 * D2D_FUN_CUSTOM; D2D_FUN_RECEIVED_POWER_PER_OBJECT with the coefficients of d2d_set_reflection_coefs, D2D_ERR_STATE without
 * them.  The interaction points of a kept path: d2d_trace_paths with its `cand`.
 * D2D_ERR_INVALID: k outside 1..D2D_TOP_MAX.
 * D2D_ERR_UNSUPPORTED (the message names the reason): sigmoid validity, MinPath / FermatPath, D2D_FUN_CUSTOM, D2D_OUT_ADD, a TX
 * grid whose sweep would not be culled (d2d_params.grid_role; not counted by d2d_debug_txg_fallbacks), more than 4 095 objects,
 * or outputs above half of the free device memory -- all decided before anything is enqueued. */
int d2d_strongest_paths_launch(d2d_ctx* ctx, const d2d_params* params, const float* fixed /* [2] */, int32_t k);
/* Synchronises and copies the result of the last d2d_strongest_paths_launch (its k) to the arrays that are not NULL.
 * D2D_ERR_STATE before a launch, after a launch that was refused, and after a d2d_set_grid of another grid (the result goes with
 * the grid). */
int d2d_get_strongest_paths(d2d_ctx* ctx, float* power, float* length, int32_t* cand, int32_t* order, float* total, int32_t* count);

/* ---- coherent field: the per-cell sum of complex amplitudes at one wavelength (no reference counterpart: every grid product
 *      of the reference adds powers; interference fringes, small-scale fading and coherent coverage follow from re and im) ---- */

#define D2D_FIELD_AMP_SQRT 0   /* the fused function is a power: its amplitude is the square root, its sign a pi flip */
#define D2D_FIELD_AMP_LINEAR 1 /* the fused function is the amplitude itself */
/* Launches the coherent-field build of the culled forward sweep for the fixed end point `fixed` on the ctx stream
 * (asynchronous), for the current scene, candidate mask and grid.  `params` as for d2d_power_map_launch (params->grid_role says
 * which end the cells are).  inv_wavelength: fp32, finite and >= 0, in turns per unit length (1 / lambda); amplitude:
 * D2D_FIELD_AMP_SQRT or D2D_FIELD_AMP_LINEAR.  Definition, per cell:
 *
 *     re = im = total = +0.0f
 *     for candidates in the sweep's enumeration order:
 *         t = valid * fun            // exactly the fused sweep's contribution (nan_to_num rules included)
 *         r = path_length(points)    // the fp32 value the path function is evaluated with (what the profile bins by)
 *         total = total + t          // fp32: hence the fused map bit for bit
 *         if (t == 0) continue       // exact zeros of either sign add no phasor (culled candidates are such zeros)
 *         a = amplitude == SQRT ? copysignf(sqrtf(fabsf(t)), t) : t       // IEEE sqrtf
 *         u = r * inv_wavelength     // fp32, turns
 *         f = u - floorf(u)          // exact; in [0, 1) for u >= 0; a NaN or infinite r gives NaN
 *         (c, s) = phasor(f)         // cos(2 pi f), sin(2 pi f) as d2d::phasor of differt2d_amd/csrc/d2d_phasor.hpp computes
 *                                    // them: fp32 multiplies, adds and compares, within 2 * 2^-24 of the true values
 *         re = re + a * c ;  im = im - a * s                              // e^(-j 2 pi r / lambda); fp32, no contraction
 *
 * Outputs: re, im and total, each fp32 [m][n].
 *
 *   - SQRT treats the fused function as a power.  Its sign becomes a pi flip of the amplitude, which is what a negative
 *     coefficient of D2D_FUN_RECEIVED_POWER_PER_OBJECT means here.  re^2 + im^2 is then a power again, and equals |t| where a
 *     cell has one path.
 *   - LINEAR takes the fused function as the amplitude itself.
 *   - With inv_wavelength == 0 and LINEAR, re equals the fused map bit for bit and im is +0.0 wherever total is finite.
 *   - The phase resolution is ulp(r / lambda) turns: 2 pi * 7.6e-6 rad at 64 wavelengths of path.  At r / lambda >= 2^24 every
 *     phase is 0.  This is documented, not refused.
 *
 * One pass of one kernel (one wave per 8 x 8 patch, three registers per lane, every lane the only writer of its cell and writing
 * all of it: no atomics, no zeroing, the same bits run to run).  The resident value / gradient maps, the work history, the
 * schedule of the fused sweeps, the records of d2d_valid_paths, the profile and the strongest paths are not touched.  Every fused
 * function but D2D_FUN_CUSTOM; D2D_FUN_RECEIVED_POWER_PER_OBJECT with the coefficients of d2d_set_reflection_coefs, D2D_ERR_STATE
 * without them.
 * D2D_ERR_INVALID: inv_wavelength negative, NaN or infinite; an unknown amplitude.
 * D2D_ERR_UNSUPPORTED (the message names the reason): sigmoid validity, MinPath / FermatPath, D2D_FUN_CUSTOM, D2D_OUT_ADD, a TX
 * grid whose sweep would not be culled (d2d_params.grid_role; not counted by d2d_debug_txg_fallbacks), more than 4 095 objects,
 * or outputs (12 bytes per cell) above half of the free device memory -- all decided before anything is enqueued. */
int d2d_coherent_field_launch(d2d_ctx* ctx, const d2d_params* params, const float* fixed /* [2] */, float inv_wavelength,
                              int32_t amplitude);
/* Synchronises and copies the result of the last d2d_coherent_field_launch to the arrays that are not NULL ([m][n] each).
 * D2D_ERR_STATE before a launch, after a launch that was refused, and after a d2d_set_grid of another grid (the result goes with
 * the grid). */
int d2d_get_coherent_field(d2d_ctx* ctx, float* re, float* im, float* total);

/* ---- channel frequency response: the coherent field at many wavelengths per sweep (no reference counterpart: H(f_j) per cell;
 *      frequency-selective fading, subcarrier gains, frequency-averaged coverage and, through an inverse FFT, a coherent impulse
 *      response follow from it) ---- */

#define D2D_FREQ_MAX 1024 /* most wavelengths of one d2d_frequency_response_launch (128 kernel launches) */
/* Launches the frequency-response build of the culled forward sweep for the fixed end point `fixed` on the ctx stream
 * (asynchronous), for the current scene, candidate mask and grid.  Definition:
 *
 * `params`, `fixed`, the grid role and `amplitude` are as for `d2d_coherent_field_launch`. The wavelengths are
 * `inv_wavelength[nf]`: fp32, each finite and `>= 0`, with `nf` in `1..D2D_FREQ_MAX`. Per cell and for every `j < nf`, the pair
 * `(re[j], im[j])` is the `(re, im)` of the coherent-field definition evaluated with `inv_wavelength[j]`. It uses the same loop,
 * the same skip of exact zeros, the same `a`, `u = r * inv_wavelength[j]`, `f = u − floorf(u)` and `phasor(f)`, and the same fp32
 * adds without contraction. `total` is the coherent field's `total`, which is the fused map bit for bit.
 *
 * The outputs are `re` and `im`, fp32 `[nf][m][n]`, and `total`, fp32 `[m][n]`.
 *
 *   - Planes do not depend on the order, the number or the duplication of the other entries of the list.
 *   - An entry `0` with `LINEAR` gives the fused map in `re[j]` and `+0.0` in `im[j]`.
 *   - Plane j is therefore, bit for bit, what d2d_coherent_field_launch gives for inv_wavelength[j]: one call of this function
 *     replaces nf of those, and the culled sweep (occlusion masks, culling, every candidate's evaluation, the path length) runs
 *     once per 8 entries instead of once per entry.
 *
 * One preparation and ceil(nf / 8) passes of one kernel over it (one wave per 8 x 8 patch; per lane up to 8 (re, im) pairs and the
 * total in registers; every lane the only writer of its cell and writing all of it: no atomics, no zeroing, the same bits run to
 * run; the 8 is internal).  The list is copied during the call.  The resident value / gradient maps, the work history, the
 * schedule of the fused sweeps, the records of d2d_valid_paths, the profile, the strongest paths and the coherent field of
 * d2d_coherent_field_launch are not touched.  Fused functions as for d2d_coherent_field_launch.
 * D2D_ERR_INVALID: nf outside 1 .. D2D_FREQ_MAX; an entry that is negative, NaN or infinite (the message names its index); an
 * unknown amplitude.
 * D2D_ERR_UNSUPPORTED (the message names the reason): what d2d_coherent_field_launch refuses, with outputs of 8 * nf + 4 bytes per
 * cell held against half of the free device memory -- all decided before anything is enqueued.  A refused launch leaves no result. */
int d2d_frequency_response_launch(d2d_ctx* ctx, const d2d_params* params, const float* fixed /* [2] */,
                                  const float* inv_wavelength /* [nf] */, int32_t nf, int32_t amplitude);
/* Synchronises and copies the result of the last d2d_frequency_response_launch to the arrays that are not NULL (re, im: [nf][m][n]
 * with that launch's nf; total: [m][n]).  D2D_ERR_STATE before a launch, after a launch that was refused, and after a d2d_set_grid
 * of another grid (the result goes with the grid). */
int d2d_get_frequency_response(d2d_ctx* ctx, float* re, float* im, float* total);

/* ---- calibrating reflection coefficients: the reverse-mode product of the frequency response with respect to the per-object
 *      coefficients (no reference counterpart: fit one coefficient per wall to a measured complex channel H_meas(f_j, cell)) ---- */

/* Launches the coefficient adjoint of the frequency response for the fixed end point `fixed` on the ctx stream, for the current
 * scene, candidate mask, grid and reflection coefficients.  Inputs: the cotangent planes re_bar, im_bar (host arrays, fp32
 * [nf][m][n], copied before the call returns; the kernels that follow are asynchronous).  Output (d2d_get_field_coefs_vjp):
 *     coef_bar[N] = sum_j sum_cells (re_bar * d re / d coef + im_bar * d im / d coef)
 * where re and im are those of d2d_frequency_response_launch with fun_id = D2D_FUN_RECEIVED_POWER_PER_OBJECT.
 * K3-G `d2d::CoefGradSink`, definition:
 *
 * - `params`, `fixed`, the grid role, `inv_wavelength[nf]` and `amplitude` are as for `d2d_frequency_response_launch`. `nf` lies in `1..D2D_FREQ_MAX`.
 * - `params.fun_id` must be `D2D_FUN_RECEIVED_POWER_PER_OBJECT`.
 * - Coefficients must be set with `d2d_set_reflection_coefs`. Without them the call returns `D2D_ERR_STATE`, as the sweeps do.
 *
 * Per cell, and per patch in the kernel:
 *
 *     for candidates in the sweep's enumeration order (walls cand[0..K)):
 *         s = valid * (1 / (h² + r²))        // fp32: the sweep's own contribution for received_power with numerator 1
 *                                             // (host: fun_id = RECEIVED_POWER, fnum[] = 1, the caller's h2 -- the way
 *                                             //  d2d_valid_paths substitutes D2D_FUN_ONE); r = the fp32 path length the sinks get
 *         if (s == 0) continue                // exact zeros of either sign; culled candidates are such zeros
 *         num = left fold of coef over cand ; P_i = product of the coefficients at the OTHER positions, formed explicitly (K <= 4)
 *         LINEAR:  Q_i = P_i                              // a = s*num ; d a / d coef[cand[i]] = s * P_i.  A zero coefficient is legal and HAS a gradient
 *         SQRT:    if (num == 0) continue                 // a = sign(num) sqrt(s) sqrt|num| is not differentiable there: defined as no term
 *                  Q_i = P_i / (2 sqrtf(|num|)) ; s := sqrtf(s)
 *         g = sum_{j<nf} ( re_bar[j][cell] * c_j - im_bar[j][cell] * s_j )   with (c_j, s_j) = phasor(frac(r * inv_wavelength[j]))
 *                                             // since re += a c and im -= a s
 *         for every position i:  coef_bar[cand[i]] += g * s * Q_i          // a wall that occurs twice gets both terms
 *
 * - Nothing is ever divided by a coefficient.
 * - `coef_bar` is fp64 `[N]`. Walls that no contributing candidate touches are exactly `+0.0`.
 * - A NaN contribution makes the entries of that candidate's walls NaN and no others.
 *
 * Unlike the forward products this is a sum over cells: it is not defined bit for bit against an oracle but to a derived bound
 * (tests/field_coefs_vjp_oracle.py).  What is exact: the same call gives the same bits run to run and whatever ran before it on the
 * context; all-zero cotangents give all +0.0; cotangents scaled by 2 give exactly doubled entries.
 *
 * In the kernel the arithmetic above is fp32 without contraction: g is a left fold over j, the lanes' weights g * s are summed over
 * the wave's 64 lanes (cells outside the grid weigh 0.0f), and one lane adds S * Q_i to the patch's row of a [patches][N] fp32 buffer
 * -- one writer per row, candidates in order, chunks of 8 wavelengths in order, plain loads and stores, no atomics -- which a
 * fixed-order reduction sums in patch order into fp64.  One preparation of the culled sweep and ceil(nf / 8) passes of one kernel,
 * exactly as the frequency response does it.  The launch touches none of: the resident value / gradient maps, the scene VJP of
 * d2d_power_map_vg_launch (d2d_get_reflection_coefs_vjp is unaffected), the work history, the other products' results.
 * D2D_ERR_INVALID: nf outside 1 .. D2D_FREQ_MAX; an inv_wavelength entry that is negative, NaN or infinite (the message names its
 * index); an unknown amplitude.  Non-finite cotangents are NOT refused: they propagate.
 * D2D_ERR_UNSUPPORTED (the message names the reason): any other fun_id, sigmoid validity, MinPath / FermatPath, D2D_OUT_ADD, a TX
 * grid whose sweep would not be culled, more than 4 095 objects, or cotangents (8 * nf bytes per cell) plus partial rows
 * (4 * patches * N bytes) above half of the free device memory -- all decided before anything is enqueued.  A refused launch
 * leaves the previous result readable. */
int d2d_field_coefs_vjp_launch(d2d_ctx* ctx, const d2d_params* params, const float* fixed /* [2] */,
                               const float* inv_wavelength /* [nf] */, int32_t nf, int32_t amplitude,
                               const float* re_bar /* [nf][m][n] */, const float* im_bar /* [nf][m][n] */);
/* Synchronises and copies the result of the last accepted d2d_field_coefs_vjp_launch to coef_bar (fp64 [N]).  D2D_ERR_STATE before
 * a launch and after a d2d_set_grid / d2d_set_scene of another grid or scene (the result goes with both). */
int d2d_get_field_coefs_vjp(d2d_ctx* ctx, double* coef_bar /* [N] */);

/* ---- power-angle profile: the fused sweep binned by the direction in which a path leaves the transmitter or reaches the
 *      receiver (no reference counterpart: angle-of-departure / angle-of-arrival spectra, angular spread, sector selection and
 *      the power a directional antenna receives follow from it) ---- */

#define D2D_ANGLE_AT_TX 0 /* bin by the direction of departure: from the transmitter towards the first interaction point */
#define D2D_ANGLE_AT_RX 1 /* bin by the direction of arrival: from the receiver towards the last interaction point */
#define D2D_ANGLE_BINS_MAX 4096
/* Launches the power-angle build of the culled forward sweep for the fixed end point `fixed` on the ctx stream (asynchronous),
 * for the current scene, candidate mask and grid.  `params`, `fixed` and the grid role are as for d2d_power_profile_launch.
 * end: D2D_ANGLE_AT_TX or D2D_ANGLE_AT_RX; origin: fp32, in turns, 0 <= origin < 1 (where bin 0 begins, counter-clockwise from
 * +x); nbins: in 1 .. D2D_ANGLE_BINS_MAX.
 *
 * A path's points are p[0] = TX, p[1..K], p[K+1] = RX: the fp32 points the path function's length is computed from.  They are
 * the same in both grid roles: in a TX grid the cell is p[0].  Definition, per cell:
 *
 *     total = +0.0f ; out[0..nbins) = +0.0f
 *     for candidates in the sweep's enumeration order:
 *         t = valid * fun                     // exactly the fused sweep's contribution (nan_to_num rules included)
 *         total = total + t                   // fp32: hence the fused map bit for bit
 *         if (t == 0) continue                // exact zeros of either sign name no bin
 *         (dx, dy) = end == AT_TX ? p[1] - p[0] : p[K] - p[K+1]
 *                                             // fp32 differences, no D2D_EPS: the direction in which that terminal SEES the path
 *                                             // (departure direction at TX; at RX the direction towards the last interaction
 *                                             // point, i.e. where the wave comes from)
 *         f = turns(dx, dy)                   // angle of (dx, dy) in turns, [0, 1), as d2d::turns of
 *                                             // differt2d_amd/csrc/d2d_angle.hpp computes it: fp32 compares, multiplies, adds and
 *                                             // one division, within 0.75 * 2^-24 turn of atan2; NaN for dx == dy == 0 and for
 *                                             // any NaN / inf component
 *         g = f - origin ; if (g < 0) g = g + 1.0f          // fp32, one rounding each
 *         u = g * (float)nbins ; b = (int)floorf(u) ; if (b >= nbins) b = nbins - 1     // (g + 1 may round to 1.0: last bin)
 *         if (f == f) out[b][cell] = out[b][cell] + t      // NaN f: no bin (total still has it)
 *
 * Outputs: out, fp32 [nbins][m][n], and total, fp32 [m][n].
 *
 *   - With nbins == 1, out[0] equals total bit for bit wherever no contribution has a zero or non-finite direction.  The dropped
 *     share is the only difference.
 *   - For any nbins, a cell's bins sum to that same value up to fp32 summation order.
 *   - AT_TX over an RX grid and AT_RX over a TX grid bin the direction at the FIXED end point.
 *   - The other two combinations bin at the cell.
 *
 * One pass of one kernel (one wave per 8 x 8 patch; out is zeroed on the stream in front of it, every lane is the only writer of
 * its cell's column: plain loads and stores, no atomics, the same bits run to run).  The result is kept with the grid until the
 * next such launch.  The resident value / gradient maps, the work history, the schedule of the fused sweeps, the records of
 * d2d_valid_paths, the delay profile, the strongest paths, the coherent field and the frequency response are not touched.  Every
 * fused function but D2D_FUN_CUSTOM; D2D_FUN_RECEIVED_POWER_PER_OBJECT with the coefficients of d2d_set_reflection_coefs,
 * D2D_ERR_STATE without them.
 * D2D_ERR_INVALID: an unknown end; an origin that is NaN or outside [0, 1); nbins outside 1 .. D2D_ANGLE_BINS_MAX.
 * D2D_ERR_UNSUPPORTED (the message names the reason): what d2d_power_profile_launch refuses, with outputs of 4 * nbins + 4 bytes
 * per cell held against half of the free device memory -- all decided before anything is enqueued.  A refused launch leaves the
 * previous result as it was. */
int d2d_power_angle_launch(d2d_ctx* ctx, const d2d_params* params, const float* fixed /* [2] */, int32_t end, float origin,
                           int32_t nbins);
/* Synchronises and copies the result of the last d2d_power_angle_launch that was accepted to the arrays that are not NULL
 * (out: [nbins][m][n] with that launch's nbins, total: [m][n]).  D2D_ERR_STATE before a launch and after a d2d_set_grid of
 * another grid (the result goes with the grid). */
int d2d_get_power_angle(d2d_ctx* ctx, float* out, float* total);

/* ---- array response: the coherent field for every pair of a transmit and a receive antenna element (no reference counterpart:
 *      the nr x nt channel matrix H per cell; beamforming gain, MIMO rank and capacity maps and spatial correlation follow from
 *      it) ---- */

#define D2D_ARRAY_MAX 8 /* most elements of either array of one d2d_array_response_launch */
/* Launches the array-response build of the culled forward sweep for the fixed end point `fixed` on the ctx stream (asynchronous),
 * for the current scene, candidate mask and grid.  `params`, `fixed`, the grid role, `inv_wavelength` and `amplitude` are exactly
 * as for d2d_coherent_field_launch.  tx_elems: fp32 [nt][2], rx_elems: fp32 [nr][2]: element offsets (ex, ey) in length units
 * from the terminal's position, every component finite; nt and nr each in 1 .. D2D_ARRAY_MAX.  The transmit array sits at p[0]
 * and the receive array at p[K+1] in both grid roles (the points of d2d_power_angle_launch: in a TX grid the cell is p[0]).
 * Definition, per cell:
 *
 *     total = +0.0f ; re[i][j] = im[i][j] = +0.0f
 *     for candidates in the sweep's enumeration order:
 *         t = valid * fun ; r = path_length(points)          // as d2d_coherent_field_launch gets them
 *         total = total + t                                   // the fused map bit for bit
 *         if (t == 0) continue
 *         a  = amplitude == SQRT ? copysignf(sqrtf(fabsf(t)), t) : t
 *         u  = r * inv_wavelength ; f0 = u - floorf(u)        // exactly the coherent field's phase
 *         (utx, uty, okt) = unit(p[1]-p[0]) ; (urx, ury, okr) = unit(p[K]-p[K+1])
 *             // unit(dx,dy): n = sqrtf(dx*dx + dy*dy) ; ok = n > 0 && n <= FLT_MAX ; ux = dx / n ; uy = dy / n   (IEEE sqrt and division)
 *         if (!(okt && okr)) continue                         // a path without a direction at an end enters no pair (total has it)
 *         for j < nt: qt = etx[j].x * utx + etx[j].y * uty
 *           for i < nr: qr = erx[i].x * urx + erx[i].y * ury
 *             w = (qt + qr) * inv_wavelength ; v = f0 - w ; f = v - floorf(v) ; if (f >= 1.0f) f = 0.0f   // (-tiny + 1 rounds to 1)
 *             (c, s) = phasor(f)
 *             re[i][j] = re[i][j] + a * c ; im[i][j] = im[i][j] - a * s
 *
 * All arithmetic is fp32 with one rounding per operation and no contraction; differt2d_amd/csrc/d2d_steer.hpp holds unit and the
 * pair's phase for host and device.  Outputs: re and im, fp32 [nr][nt][m][n], and total, fp32 [m][n].
 *
 *   - Entry (i, j) depends only on etx[j] and erx[i]: permuted, duplicated or truncated element lists give permuted, equal or
 *     leading planes, bit for bit.
 *   - A pair whose two offsets are (+-0, +-0) equals d2d_coherent_field_launch bit for bit wherever no contribution lacks a
 *     direction at an end (the line of sight of a cell that IS the fixed end point is such a contribution).
 *   - This is the plane-wave (far-field) model: the phase of pair (i, j) is (r - etx[j] . u_tx - erx[i] . u_rx) / lambda, and the
 *     neglected spherical-wave phase is about pi |e_perp|^2 / (lambda r) for an offset e_perp across the path.
 *   - The phase resolution is that of the coherent field: ulp(r / lambda) turns.
 *
 * One pass of one kernel (one wave per 8 x 8 patch; re and im are zeroed on the stream in front of it, every lane is the only writer
 * of its cell's column: plain loads and stores, no atomics, the same bits run to run).  The element lists are copied during the
 * call.  The result is kept with the grid until the next such launch.  The resident value / gradient maps, the work history, the
 * schedule of the fused sweeps, the records of d2d_valid_paths and every other product (delay profile, strongest paths, coherent
 * field, frequency response, power-angle profile) are not touched.  Fused functions as for d2d_coherent_field_launch.
 * D2D_ERR_INVALID: nt or nr outside 1 .. D2D_ARRAY_MAX; an element component that is NaN or infinite (the message ends in its
 * index); inv_wavelength negative, NaN or infinite; an unknown amplitude.  No list is read unless its count is in range.
 * D2D_ERR_UNSUPPORTED (the message names the reason): what d2d_coherent_field_launch refuses, with outputs of 8 * nr * nt + 4
 * bytes per cell held against half of the free device memory -- all decided before anything is enqueued.  A refused launch leaves
 * the previous result as it was. */
int d2d_array_response_launch(d2d_ctx* ctx, const d2d_params* params, const float* fixed /* [2] */, float inv_wavelength,
                              int32_t amplitude, int32_t nt, const float* tx_elems /* [nt][2] */, int32_t nr,
                              const float* rx_elems /* [nr][2] */);
/* Synchronises and copies the result of the last d2d_array_response_launch that was accepted to the arrays that are not NULL
 * (re, im: [nr][nt][m][n] with that launch's counts, total: [m][n]).  D2D_ERR_STATE before a launch and after a d2d_set_grid of
 * another grid (the result goes with the grid). */
int d2d_get_array_response(d2d_ctx* ctx, float* re, float* im, float* total);
/* ---- K3-W, wideband array response: the channel matrices at many wavelengths from one preparation of the culled sweep (the
 *      nf x nr x nt channel tensor per cell: per-subcarrier capacity, wideband beamforming, spatial correlation across a band) ---- */

/* Launches the wideband array-response build of the culled forward sweep for the fixed end point `fixed` on the ctx stream
 * (asynchronous), for the current scene, candidate mask and grid.
 *
 * - `params`, `fixed`, the grid role, `amplitude`, `tx_elems`, `rx_elems`, `nt` and `nr` are exactly as for
 *   d2d_array_response_launch.
 * - `inv_wavelength[nf]` and `nf` are exactly as for d2d_frequency_response_launch: `1..D2D_FREQ_MAX`, each entry finite and `>= 0`.
 * - Per cell and for every `f < nf`, the planes `(re[f][i][j], im[f][i][j])` are the `(re[i][j], im[i][j])` of the array-response
 *   definition evaluated with `inv_wavelength[f]`.
 * - That means the same loop over candidates in the sweep's order and the same skip of exact zeros.
 * - It means the same `a`, and `f0 = u - floorf(u)` with `u = r * inv_wavelength[f]`.
 * - It means the same `unit_dir`, `steer_dot`, `steer_phase(f0, qt, qr, inv_wavelength[f])` and `phasor`.
 * - It means the same fp32 adds without contraction.
 * - `total` is the array response's `total`: the fused map, bit for bit.
 * - Outputs are `re` and `im`, fp32 `[nf][nr][nt][m][n]`, and `total`, fp32 `[m][n]`.
 *
 * These properties follow from the definition:
 *
 * - Independence.  Plane `(f, i, j)` depends on `inv_wavelength[f]`, `etx[j]` and `erx[i]` only.  Permuted, duplicated or
 *   truncated lists on any of the three axes give permuted, equal or leading planes, bit for bit.
 * - Slice.  Plane block `f` equals d2d_array_response_launch at `inv_wavelength[f]`, bit for bit.
 * - Zero offsets.  A pair of `(+-0, +-0)` offsets gives the planes of d2d_frequency_response_launch, bit for bit, wherever no
 *   contribution lacks a direction.
 * - Zero entry.  An entry `0` with `LINEAR` and zero offsets gives the fused map in `re` and `+0.0` in `im`.
 *
 * One preparation of the sweep, then one kernel pass per chunk of wavelengths (the chunk's size is internal) over the same
 * arguments; re and im are zeroed on the stream in front of the passes, every lane is the only writer of its cell's column: plain
 * loads and stores, no atomics, the same bits run to run.  The lists are copied during the call.  The result is kept with the grid
 * until the next such launch.  The launch touches no other product's result: not the resident value / gradient maps, not the
 * results of d2d_array_response_launch, d2d_frequency_response_launch or d2d_coherent_field_launch, nor any other.
 * D2D_ERR_INVALID: what d2d_frequency_response_launch refuses of the list and the amplitude (nf outside 1 .. D2D_FREQ_MAX; an entry
 * that is negative, NaN or infinite: the message names its index), then what d2d_array_response_launch refuses of the element
 * lists (nt or nr outside 1 .. D2D_ARRAY_MAX; a component that is NaN or infinite: the message ends in its index).  No list is
 * read unless its count is in range.
 * D2D_ERR_UNSUPPORTED (the message names the reason): what d2d_array_response_launch refuses (sigmoid validity, MinPath /
 * FermatPath, D2D_OUT_ADD, a function that is not fused -- the message names d2d_valid_paths and d2d_trace_paths --, a TX grid
 * whose sweep is not culled), with outputs of 8 * nf * nr * nt + 4 bytes per cell held against half of the free device memory --
 * all decided before anything is enqueued.  A refused launch leaves the previous result as it was. */
int d2d_array_frequency_response_launch(d2d_ctx* ctx, const d2d_params* params, const float* fixed /* [2] */,
                                        const float* inv_wavelength /* [nf] */, int32_t nf, int32_t amplitude, int32_t nt,
                                        const float* tx_elems /* [nt][2] */, int32_t nr, const float* rx_elems /* [nr][2] */);
/* Synchronises and copies wavelengths first .. first + count - 1 of the result of the last d2d_array_frequency_response_launch
 * that was accepted to the arrays that are not NULL (re, im: [count][nr][nt][m][n] with that launch's counts; total: [m][n], may
 * be NULL).  0 <= first, count >= 1 and first + count <= nf; anything else is D2D_ERR_INVALID.  The range exists so that a
 * result far larger than host memory can be read block by block: at 1024^2, 64 wavelengths of a 4 x 4 matrix are 8 GiB.
 * D2D_ERR_STATE before a launch and after a d2d_set_grid of another grid (the result goes with the grid). */
int d2d_get_array_frequency_response(d2d_ctx* ctx, int32_t first, int32_t count, float* re /* [count][nr][nt][m][n] */,
                                     float* im /* same */, float* total /* [m][n] or NULL */);

/* ---- K3-B, beam-space response: codebook beamforming fused into the culled sweep (y = w_rx^H H w_tx per cell, wavelength and
 *      beam pair without the channel matrix: beam-sweep coverage maps, the best beam pair per cell, beamformed wideband power) ---- */

#define D2D_BEAM_MAX 8 /* most beams of either codebook of one d2d_beam_response_launch */

/* Launches the beam-response build of the culled forward sweep for the fixed end point `fixed` on the ctx stream (asynchronous),
 * for the current scene, candidate mask and grid.
 *
 * Existing arguments:
 *
 * - `params`, `fixed`, the grid role and `amplitude` are exactly as for `d2d_array_frequency_response_launch`.
 * - So are `inv_wavelength[nf]` (`1..D2D_FREQ_MAX`, each finite and `>= 0`), `tx_elems[nt][2]` and `rx_elems[nr][2]`
 *   (`1..D2D_ARRAY_MAX` each).
 *
 * New arguments:
 *
 * - `tx_weights`: fp32 `[nbt][nt][2]`, the `(re, im)` of transmit beam `bt` at element `j`.
 * - `rx_weights`: fp32 `[nbr][nr][2]`.
 * - Every component must be finite.
 * - `nbt` and `nbr` each lie in `1..D2D_BEAM_MAX`, with `D2D_BEAM_MAX = 8`. A larger codebook is several calls, which the
 *   independence property below makes exact.
 *
 * Per cell, all in fp32, one rounding per operation, no contraction, candidates in the sweep's enumeration order:
 *
 *   total = +0.0f ; re[f][br][bt] = im[f][br][bt] = +0.0f
 *   for candidates:
 *       t = valid * fun ; r = path_length(points)            // as ArrayFreqSink gets them
 *       total = total + t                                     // the fused map, bit for bit
 *       if (t == 0) continue
 *       a = amplitude == SQRT ? copysignf(sqrtf(fabsf(t)), t) : t
 *       (utx, uty, okt) = unit_dir(p[1]-p[0]) ; (urx, ury, okr) = unit_dir(p[K]-p[K+1])     // d2d_steer.hpp, unchanged
 *       if (!(okt && okr)) continue
 *       for f < nf:
 *           inv = inv_wavelength[f] ; u = r * inv ; f0 = u - floorf(u) ; (c0, s0) = phasor(f0)
 *           steer(q):  v = q * inv ; g = v - floorf(v) ; if (g >= 1.0f) g = 0.0f ; (c, s) = phasor(g)      // e^(+j 2 pi q / lambda) = c + j s
 *           for bt < nbt:  At = (+0, +0) ; for j < nt in order:  (c, s) = steer(steer_dot(etx[j], utx, uty)) ; w = tx_weights[bt][j]
 *                              At.re = At.re + (w.re * c - w.im * s) ;  At.im = At.im + (w.re * s + w.im * c)
 *           for br < nbr:  Ar = (+0, +0) ; for i < nr in order:  (c, s) = steer(steer_dot(erx[i], urx, ury)) ; w = rx_weights[br][i]
 *                              Ar.re = Ar.re + (w.re * c + w.im * s) ;  Ar.im = Ar.im + (w.re * s - w.im * c)       // conj(w) * steer
 *           for (br, bt):  P.re = Ar.re * At.re - Ar.im * At.im ;  P.im = Ar.re * At.im + Ar.im * At.re
 *                          zr = P.re * c0 + P.im * s0 ;  zs = P.re * s0 - P.im * c0                                  // P e^(-j 2 pi f0) = zr - j zs
 *                          re[f][br][bt] = re[f][br][bt] + a * zr ;  im[f][br][bt] = im[f][br][bt] - a * zs
 *
 * Outputs:
 *
 * - `re` and `im`: fp32 `[nf][nbr][nbt][m][n]`.
 * - `total`: fp32 `[m][n]`.
 * - This is `y = w_rx^H H w_tx` with the conjugate on the receive weights, the convention of `utils.beamformed_power`.
 *
 * The arithmetic is that of differt2d_amd/csrc/d2d_beam.hpp (steer, the two folds and the pair product), host and device alike;
 * its text is the definition. Because every parenthesised product and every add above is one stated operation, the bits do not
 * depend on how the kernel nests or recomputes things.
 *
 * Properties:
 *
 * - Total. `total` is the fused map, bit for bit.
 * - Independence. Plane `(f, br, bt)` depends only on `inv_wavelength[f]`, row `br` of `rx_weights`, row `bt` of `tx_weights` and
 *   the two element lists. Permuted, duplicated or truncated wavelength or beam lists give permuted, equal or leading planes, bit
 *   for bit. The element order is part of the definition, because it is a left fold.
 * - One antenna. Take `nt = nr = nbt = nbr = 1`, offsets `(+-0, +-0)` and weights `(1, 0)`. The planes then equal
 *   `d2d_frequency_response_launch`'s, bit for bit, wherever no contribution lacks a direction and no contribution is NaN:
 *   `phasor(0) = (1, +0)` exactly, so `At = Ar = P = (1, +0)`, `zr = c0` and `zs = s0` as values, and the accumulation absorbs
 *   signs of zero.
 * - Element space. Against the float64 contraction `conj(w_rx) . H . w_tx` of `d2d_array_frequency_response_launch`'s planes, the
 *   beam planes agree within a derived bound (tests/beam_response_oracle.py), not bit for bit.
 *
 * One preparation of the sweep, then one kernel pass per chunk of wavelengths (the chunk's size is internal) over the same
 * arguments; re and im are zeroed on the stream in front of the passes, every lane is the only writer of its cell's column: plain
 * loads and stores, no atomics, the same bits run to run.  The lists and the weights are copied during the call.  The result is
 * kept with the grid until the next such launch; d2d_set_grid of another grid drops it.  The launch touches no other product's
 * result, and no other product's launch touches this one.
 * D2D_ERR_INVALID: a NULL argument; what d2d_array_frequency_response_launch refuses of the list, the amplitude and the element
 * lists, in its order; then nbt, then nbr outside 1 .. D2D_BEAM_MAX; then a weight component that is NaN or infinite (the message
 * names the table and the beam and ends in the element's index).  No list is read unless its count is in range.
 * D2D_ERR_UNSUPPORTED (the message names the reason): what d2d_array_frequency_response_launch refuses (sigmoid validity, MinPath /
 * FermatPath, D2D_OUT_ADD, a function that is not fused -- the message names d2d_valid_paths and d2d_trace_paths --, a TX grid
 * whose sweep is not culled), with outputs of 8 * nf * nbr * nbt + 4 bytes per cell held against half of the free device memory --
 * all decided before anything is enqueued.  A refused launch leaves the previous result as it was. */
int d2d_beam_response_launch(d2d_ctx* ctx, const d2d_params* params, const float* fixed /* [2] */,
                             const float* inv_wavelength /* [nf] */, int32_t nf, int32_t amplitude, int32_t nt,
                             const float* tx_elems /* [nt][2] */, int32_t nr, const float* rx_elems /* [nr][2] */, int32_t nbt,
                             const float* tx_weights /* [nbt][nt][2] */, int32_t nbr, const float* rx_weights /* [nbr][nr][2] */);
/* Synchronises and copies wavelengths first .. first + count - 1 of the result of the last d2d_beam_response_launch that was
 * accepted to the arrays that are not NULL (re, im: [count][nbr][nbt][m][n] with that launch's counts; total: [m][n], may be
 * NULL).  0 <= first, count >= 1 and first + count <= nf; anything else is D2D_ERR_INVALID.  D2D_ERR_STATE before a launch and
 * after a d2d_set_grid of another grid (the result goes with the grid). */
int d2d_get_beam_response(d2d_ctx* ctx, int32_t first, int32_t count, float* re /* [count][nbr][nbt][m][n] */, float* im /* same */,
                          float* total /* [m][n] or NULL */);

/* unit_dir and steer_phase of d2d_steer.hpp on the device, for comparison with their host build: ok[i] = unit_dir(dx[i], dy[i]) as
 * 0 / 1 with ux[i], uy[i], and f[i] = steer_phase(f0[i], qt[i], qr[i], inv[i]). */
int d2d_selftest_steer(d2d_ctx* ctx, const float* dx, const float* dy, const float* f0, const float* qt, const float* qr,
                       const float* inv, int64_t n, float* ux, float* uy, float* ok, float* f);

/* ---- material response: the frequency response with Fresnel reflection per wall ------------------------------------------------
 *
 * d2d_frequency_response_launch with every contribution multiplied by the product of the complex Fresnel reflection coefficients of
 * the walls it bounces off: the coefficient depends on the angle of incidence, the polarisation and the wall's complex relative
 * permittivity, goes through zero at the Brewster angle (TM), tends to -1 at grazing incidence and carries a phase of its own where
 * the material is lossy.  One preparation of the culled sweep, one pass per chunk of wavelengths.
 *
 * - `params`, `fixed`, the grid role, `inv_wavelength[nf]` (`1..D2D_FREQ_MAX`, each finite and `>= 0`) and `amplitude` are as for
 *   d2d_frequency_response_launch.  Pass a path function that holds no reflection loss of its own (D2D_FUN_RECEIVED_POWER with
 *   r_coef = 1, or D2D_FUN_ONE), so that walls are not counted twice.
 * - `polarization`: D2D_POL_TE (E perpendicular to the plane of incidence; for vertical antennas over a 2-D floor plan E out of the
 *   plane, the natural case here) or D2D_POL_TM (E in the plane of incidence).
 * - `eps[nf][n_objects][2]`: fp32 (re, im) of the complex relative permittivity of every object at every wavelength.  The time
 *   convention is the library's, e^(-j 2 pi r / lambda): a lossy medium is eps = eps' - j eps'', so Im eps <= 0.  `n_objects` is
 *   the resident scene's.  Rows that are all equal in bits (one permittivity for the whole band, the common case) are detected and
 *   the product of coefficients is then formed once per contribution: the same bits by definition.
 *
 * The coefficient (differt2d_amd/csrc/d2d_fresnel.hpp is the definition; fp32, one rounding per operation, IEEE sqrt and division):
 *
 *   fresnel(er, ei, c, pol) -> (gr, gi)
 *       if (c > 1) c = 1                                              // a NaN c stays NaN and gives (NaN, NaN)
 *       wr = (er - 1) + c*c ; wi = ei                                 // w = eps - sin^2(theta), without forming sin^2
 *       m  = sqrtf(wr*wr + wi*wi)
 *       if (m == 0)        q = (0, 0)                                 // q = sqrt(w), the branch with Im q <= 0 (the decaying one)
 *       else if (wr >= 0)  qr = sqrtf(0.5f*(m + wr)) ; qi = wi / (2.0f*qr)
 *       else               qi = -sqrtf(0.5f*(m - wr)) ; qr = wi / (2.0f*qi)      // also for ei = +-0: total reflection, |G| = 1
 *       TE: a = (c, 0)            TM: a = (er*c, ei*c)
 *       n = a - q ; d = a + q ; den = d.re*d.re + d.im*d.im
 *       if (den == 0)      (gr, gi) = (-1, 0)                         // the grazing limit
 *       else               gr = (n.re*d.re + n.im*d.im) / den ; gi = (n.im*d.re - n.re*d.im) / den
 *
 * Per cell, candidates in the sweep's enumeration order, p[0] = TX and p[K+1] = RX in both grid roles, walls cand[0..K):
 *
 *   total = +0.0f ; re[f] = im[f] = +0.0f
 *   for candidates:
 *       t = valid * fun ; r = path_length(points)          // as d2d_frequency_response_launch gets them
 *       total = total + t                                   // the fused map, bit for bit
 *       if (t == 0) continue
 *       a = amplitude == SQRT ? copysignf(sqrtf(fabsf(t)), t) : t
 *       for i < K:  (ux, uy, ok_i) = unit_dir(p[i+1] - p[i])                 // d2d_steer.hpp
 *                   (nx, ny) = unit normal of wall cand[i]                   // normalize((t_y, -t_x)) of t = dest - origin, fp32
 *                   c_i = fabsf(ux*nx + uy*ny)                                // cos of the angle of incidence
 *       if (any !ok_i or any c_i is NaN) continue           // no incidence angle: the path enters no plane (total has it)
 *       for f < nf:
 *           G = (1, +0) ; for i < K in order:  g = fresnel(eps[f][cand[i]], c_i, polarization)
 *                                              G = (G.re*g.re - G.im*g.im, G.re*g.im + G.im*g.re)
 *           u = r * inv_wavelength[f] ; f0 = u - floorf(u) ; (c0, s0) = phasor(f0)
 *           zr = G.re*c0 + G.im*s0 ; zs = G.re*s0 - G.im*c0                  // G e^(-j 2 pi f0) = zr - j zs
 *           re[f] = re[f] + a*zr ; im[f] = im[f] - a*zs
 *
 * `total` is the fused map bit for bit.  Plane f depends on inv_wavelength[f] and row f of eps alone; the eps of a wall that no
 * contributing candidate touches does not matter.  With max_order = 0 the planes are d2d_frequency_response_launch's bit for bit
 * wherever no contribution is NaN.  Values only, one GPU: no gradients with respect to the geometry (d2d_material_eps_vjp_launch has those with respect to eps), no array or beam variant,
 * no transmission through walls, no slabs of finite thickness, no roughness; RIS objects reflect like walls of their permittivity.
 *
 * D2D_ERR_INVALID: what d2d_frequency_response_launch refuses of the list and the amplitude; a polarization other than 0 / 1; an
 * n_objects that is not the resident scene's; an eps component that is NaN, infinite or above 2^50 in magnitude, or Im eps > 0 (the
 * message ends with the wavelength index and the wall index).
 * D2D_ERR_UNSUPPORTED (the message names the reason): what d2d_frequency_response_launch refuses (sigmoid validity, MinPath /
 * FermatPath, D2D_OUT_ADD, a function that is not fused -- the message names d2d_valid_paths and d2d_trace_paths --, a TX grid
 * whose sweep is not culled), with outputs of 8 * nf + 4 bytes per cell plus 8 * nf * n_objects bytes for the table held against
 * half of the free device memory -- all decided before anything is enqueued.  A refused launch leaves the previous result as it was. */
#define D2D_POL_TE 0
#define D2D_POL_TM 1
int d2d_material_response_launch(d2d_ctx* ctx, const d2d_params* params, const float* fixed /* [2] */,
                                 const float* inv_wavelength /* [nf] */, int32_t nf, int32_t amplitude, int32_t polarization,
                                 const float* eps /* [nf][n_objects][2]: (re, im) */, int32_t n_objects);
/* Synchronises and copies the result of the last d2d_material_response_launch that was accepted to the arrays that are not NULL
 * (re, im: [nf][m][n]; total: [m][n]).  D2D_ERR_STATE before a launch, after a d2d_set_grid of another grid and after a
 * d2d_set_scene of another scene (the result goes with the grid and the walls). */
int d2d_get_material_response(d2d_ctx* ctx, float* re /* [nf][m][n] or NULL */, float* im /* same */, float* total /* [m][n] or NULL */);

/* fresnel of d2d_fresnel.hpp on the device, for comparison with its host build: (gr[i], gi[i]) = fresnel(er[i], ei[i], c[i], pol). */
int d2d_selftest_fresnel(d2d_ctx* ctx, const float* er, const float* ei, const float* c, int32_t pol, int64_t n, float* gr, float* gi);

/* ---- material calibration: the material response's gradient with respect to the walls' permittivities (K3-E) --------------------
 *
 * The reverse-mode product of d2d_material_response_launch: given the cotangents re_bar, im_bar [nf][m][n] of its planes
 * (dL = sum re_bar * dre + im_bar * dim; utils.field_misfit returns them for a least-squares misfit), eps_bar[nf][n_objects][2] =
 * (dL/dRe eps, dL/dIm eps) of every wall at every wavelength, in fp64.  G(eps) is holomorphic, so one complex derivative per bounce
 * (differt2d_amd/csrc/d2d_fresnel_grad.hpp is its definition) carries both components.  One preparation of the culled sweep; per
 * chunk of 8 wavelengths one pass into per-patch rows (one writer per row, no atomics) and one fixed-order fp64 reduction of the
 * rows: the same bits run to run.  eps <- eps - rate * (eps_bar.re + j eps_bar.im) is gradient descent.
 *
 * Every argument up to `n_objects` is d2d_material_response_launch's, with its checks and messages; `re_bar` and `im_bar` are
 * copied before the call returns.  Any fused path function is accepted: the amplitude does not depend on eps.
 *
 *   eps_bar[f][w] = (+0.0, +0.0) for all f, w                    // fp64 [nf][n_objects][2]
 *   for cells, for candidates in the sweep's enumeration order (walls cand[0..K), K >= 1):
 *       t = valid * fun ; r ; seg[i] = p[i+1] - p[i]              // as d2d_material_response_launch gets them
 *       if (t == 0) continue
 *       c_i = |unit_dir(seg[i]) . n(cand[i])| ;  if any segment lacks a direction or any c_i is NaN: continue   // the forward's rule
 *       a = amplitude == SQRT ? copysignf(sqrtf(fabsf(t)), t) : t
 *       for f < nf:
 *           (g_i, d_i, ok_i) = fresnel_grad(eps[f][cand[i]], c_i, polarization)   for i < K       // d2d_fresnel_grad.hpp
 *           (c0, s0) = phasor(frac(r * inv_wavelength[f])) ;  E = a * (c0 - j s0)
 *           B = re_bar[f][cell] + j im_bar[f][cell]
 *           for i < K with ok_i:
 *               P_i = product of g_o over the OTHER positions o != i, in position order, formed explicitly (K <= 4; nothing is divided by a g)
 *               D   = E * (P_i * d_i)
 *               eps_bar[f][cand[i]].re += B.re*D.re + B.im*D.im                  // dL/dRe eps
 *               eps_bar[f][cand[i]].im += B.im*D.re - B.re*D.im                  // dL/dIm eps
 *
 * The terms are formed in fp32 and summed per 8 x 8 patch in fp32 (a wave's butterfly, then the patch's row), the rows in fp64: the
 * result is the definition's up to the rounding that tests/material_eps_vjp_oracle.py bounds, not bit for bit.  A wall that occurs
 * twice in a candidate gets both terms; the line of sight holds no coefficient and adds nothing; ok_i is false where G is defined by
 * a special case (q = 0, the grazing limit) and has no derivative.  Row f depends on inv_wavelength[f], row f of eps and the
 * cotangent planes f alone; a wall that no contributing candidate touches has (+0.0, +0.0).  `total` is not produced.  One GPU; no
 * gradients with respect to the geometry, the wavelengths or the fixed end point, no array or beam variant.
 *
 * D2D_ERR_INVALID and D2D_ERR_UNSUPPORTED: what d2d_material_response_launch refuses, with its messages under this function's name,
 * and NULL cotangents.  The memory rule holds the cotangents (8 * nf bytes per cell), the table and the result (24 * nf * n_objects
 * bytes) and one chunk's rows (64 * n_objects bytes per patch) against half of the free device memory.  All decided before anything
 * is enqueued: a refused launch leaves the previous result as it was. */
int d2d_material_eps_vjp_launch(d2d_ctx* ctx, const d2d_params* params, const float* fixed /* [2] */,
                                const float* inv_wavelength /* [nf] */, int32_t nf, int32_t amplitude, int32_t polarization,
                                const float* eps /* [nf][n_objects][2]: (re, im) */, int32_t n_objects,
                                const float* re_bar /* [nf][m][n] */, const float* im_bar /* [nf][m][n] */);
/* Synchronises and copies the result of the last d2d_material_eps_vjp_launch that was accepted.  D2D_ERR_STATE before a launch,
 * after a d2d_set_grid of another grid and after a d2d_set_scene of another scene (the result goes with the grid and the scene). */
int d2d_get_material_eps_vjp(d2d_ctx* ctx, double* eps_bar /* [nf][n_objects][2] */);

/* fresnel_grad of d2d_fresnel_grad.hpp on the device, for comparison with its host build:
 * (gr[i], gi[i], dr[i], di[i], ok[i]) = fresnel_grad(er[i], ei[i], c[i], pol), ok as 1 / 0. */
int d2d_selftest_fresnel_grad(d2d_ctx* ctx, const float* er, const float* ei, const float* c, int32_t pol, int64_t n, float* gr, float* gi,
                              float* dr, float* di, float* ok);

/* ---- position gradients of the frequency response: its reverse-mode product with respect to the cell's position and the fixed
 *      end point (K3-X; localisation against a measured complex channel H_meas(f_j, cell), transmitter placement for coherent
 *      wideband coverage; additive entry points, the ABI version did not change) -------------------------------------------- */

#define D2D_POS_CHUNK 8 /* wavelengths per pass of d2d_field_position_vjp_launch: part of its definition (a block's dL/dr rounds once) */
/* Launches the position adjoint of the frequency response for the fixed end point `fixed` on the ctx stream, for the current
 * scene, candidate mask and grid.  For hard validity and image paths a position enters the response through the path length r
 * alone (validity is piecewise constant, every fused path function is a function of r), and the interaction points are stationary
 * (Fermat's principle): d r / d p[0] = -unit(p[1] - p[0]), d r / d p[K+1] = -unit(p[K] - p[K+1]).
 * K3-X `d2d::PosGradSink`, definition:
 *
 * - `params`, `fixed`, the role of the grid, `inv_wavelength[nf]` (`1..D2D_FREQ_MAX` entries, each finite and `>= 0`) and `amplitude` are exactly as for `d2d_frequency_response_launch`.
 * - The cotangent planes `re_bar`, `im_bar` are host arrays, fp32 `[nf][m][n]`. They are copied before the call returns.
 * - The validity must be hard (`params.approx == 0`). Every fused `fun_id` is accepted.
 * - The result is the gradient of `L`, for `dL = Σ (re_bar·dre + im_bar·dim)` with `re`, `im` those of `d2d_frequency_response_launch` for the same arguments. There are three outputs.
 * - `cell_bar[2][m][n]`, fp32: the gradient with respect to the position of every cell. On an RX grid that is the receiver of that cell; on a TX grid the transmitter.
 * - `fixed_terms[2][m][n]`, fp32: what each cell contributes to the gradient with respect to the fixed end point.
 * - `fixed_bar[2]`, fp64: the sum of `fixed_terms` over the cells.
 *
 * All arithmetic is fp32, one rounding per stated operation, no contraction. `POS_CHUNK = D2D_POS_CHUNK = 8` is the number of wavelengths per pass. It is part of the definition. Per cell:
 *
 *     cell_bar = fixed_terms = (+0.0f, +0.0f)
 *     for blocks of POS_CHUNK wavelengths, in list order:
 *       for candidates in the sweep's enumeration order:
 *         t = valid * fun ; r = path_length(points) ; dir = {p[1]-p[0], p[K]-p[K+1]}      // as the array response gets them
 *         if (t == 0) continue                                                             // exact zeros of either sign
 *         a   = amplitude == SQRT ? copysignf(sqrtf(fabsf(t)), t) : t
 *         rho = RECEIVED_POWER, RECEIVED_POWER_PER_OBJECT: -(2.0f*r) / (h2 + r*r)          // (d fun/d r) / fun ; h2 as the sweep has it
 *               LENGTH_SQUARED: 2.0f / r ;  LENGTH: 1.0f / r ;  ONE: +0.0f
 *         kr  = amplitude == SQRT ? 0.5f * rho : rho                                       // (d a/d r) / a
 *         g = +0.0f
 *         for j in the block, in order:
 *             u = r * inv[j] ; f0 = u - floorf(u) ; (c, s) = phasor(f0) ; w = TWO_PI * inv[j]     // TWO_PI = 6.2831855f
 *             pr = kr*c - w*s ;  pi = kr*s + w*c            // d(a e^(-j2πr/λ))/dr = a (pr - j pi)
 *             g  = g + (re_bar[j][cell]*pr - im_bar[j][cell]*pi)
 *         G = a * g                                         // dL/dr of this path, this block
 *         (ucx, ucy, okc) = unit_dir(direction at the cell's end) ; (ufx, ufy, okf) = unit_dir(direction at the fixed end)   // d2d_steer.hpp, unchanged
 *         if (okc) { cell_bar.x    = cell_bar.x    - G*ucx ;  cell_bar.y    = cell_bar.y    - G*ucy }
 *         if (okf) { fixed_terms.x = fixed_terms.x - G*ufx ;  fixed_terms.y = fixed_terms.y - G*ufy }
 *     fixed_bar[d] = sum over cells of (double)fixed_terms[d][cell]      // fp64, a fixed order, no atomics
 *
 * - The direction at the cell's end is `dir[2..3]` on an RX grid and `dir[0..1]` on a TX grid. The fixed end takes the other pair.
 * - The per-contribution arithmetic (`a`, `rho`, `kr`, the fold over `j`, `G`) is the text of `differt2d_amd/csrc/d2d_posgrad.hpp`.
 * - A cell that no path reaches holds exactly `+0.0` in all four entries. A path without a direction at an end adds nothing at that end.
 * - Non-finite cotangents are not refused. A NaN contribution makes that cell's entries NaN, and thereby `fixed_bar`, and no other cell's.
 *
 * cell_bar and fixed_terms are defined bit for bit (tests/field_position_vjp_oracle.py restates them in NumPy); fixed_bar is a fixed-
 * order fp64 sum: the same bits run to run and whatever ran before on the context, within (cells - 1) * 2^-53 * sum |terms| of any
 * other summation order.  All-zero cotangents give +0.0 in every bit of the three outputs, cotangents scaled by 2 exactly doubled
 * outputs, and appending a wavelength whose two planes are zero changes no bit.
 *
 * One preparation of the culled sweep and ceil(nf / D2D_POS_CHUNK) passes of one kernel, as the frequency response does it: the
 * cotangents of a block sit in registers, every lane keeps four accumulators that the four planes carry from one pass to the next,
 * and a fixed-order reduction sums the two fixed_terms planes.  The launch touches none of: the resident value / gradient maps, the
 * scene VJP of d2d_power_map_vg_launch, the work history, the other products' results.
 * D2D_ERR_INVALID: a NULL argument; nf outside 1 .. D2D_FREQ_MAX; an inv_wavelength entry that is negative, NaN or infinite (the
 * message names its index); an unknown amplitude.
 * D2D_ERR_UNSUPPORTED (the message names the reason): hard_sigmoid and sigmoid validity -- a smoothed validity depends on the
 * positions itself, and its term needs the reverse chain of the value+grad sweep (d2d_power_map_vg_launch); a gradient that silently
 * left that term out would be a trap, so it is refused, not approximated -- and what d2d_frequency_response_launch refuses, with
 * 8 * nf + 16 bytes per cell held against half of the free device memory.  All decided before anything is enqueued; a refused launch
 * leaves the previous result readable.
 * Not computed: hard_sigmoid validity, the array, beam and material variants (where the angle of incidence also moves), gradients
 * with respect to the wavelengths, more than one GPU.  (Gradients with respect to wall end points: d2d_field_walls_vjp_launch.) */
int d2d_field_position_vjp_launch(d2d_ctx* ctx, const d2d_params* params, const float* fixed /* [2] */,
                                  const float* inv_wavelength /* [nf] */, int32_t nf, int32_t amplitude,
                                  const float* re_bar /* [nf][m][n] */, const float* im_bar /* [nf][m][n] */);
/* Synchronises and copies the result of the last accepted d2d_field_position_vjp_launch to the arrays that are not NULL.
 * D2D_ERR_STATE before a launch and after a d2d_set_grid / d2d_set_scene of another grid or scene (the result goes with both). */
int d2d_get_field_position_vjp(d2d_ctx* ctx, float* cell_bar /* [2][m][n] or NULL */, float* fixed_terms /* [2][m][n] or NULL */,
                               double* fixed_bar /* [2] or NULL */);
/* The per-contribution arithmetic of d2d_posgrad.hpp on the device, for comparison with its host build: for every i,
 * a = posgrad_amp(amplitude, t), rho = posgrad_rho(fun_id, h2, r), kr = posgrad_kr(amplitude, rho), g = the fold of posgrad_fold
 * over (inv0, rb0, ib0) then (inv1, rb1, ib1) from +0, and G = a * g. */
int d2d_selftest_posgrad(d2d_ctx* ctx, int32_t fun_id, int32_t amplitude, const float* t, const float* r, const float* h2, const float* inv0,
                         const float* inv1, const float* rb0, const float* rb1, const float* ib0, const float* ib1, int64_t n, float* a,
                         float* rho, float* kr, float* g, float* G);

/* ---- wall end-point gradients of the frequency response: its reverse-mode product with respect to the two end points of every
 *      wall (K3-V; scene reconstruction and wall localisation against a measured complex channel H_meas(f_j, cell); additive
 *      entry points, the ABI version did not change) --------------------------------------------------------------------------- */

/* Launches the wall adjoint of the frequency response for the fixed end point `fixed` on the ctx stream, for the current scene,
 * candidate mask and grid.
 * K3-V `d2d::WallGradSink`, definition:
 *
 * - The arguments of the wall adjoint are exactly those of `d2d_field_position_vjp_launch`: `params`, `fixed[2]`, the role of the grid, `inv_wavelength[nf]` (`nf` in `1..D2D_FREQ_MAX`, each entry finite and `>= 0`), `amplitude`, and the cotangent planes `re_bar`, `im_bar`.
 * - The cotangents are host arrays, fp32 `[nf][m][n]`. They are copied before the call returns.
 * - Validity is hard only (`params.approx == 0`). Every fused `fun_id` is accepted; `RECEIVED_POWER_PER_OBJECT` needs its coefficients set.
 * - For hard validity and image paths a wall enters the response through the path length `r` alone: validity is piecewise constant, every fused `fun` depends on `r` only, and per-object coefficients do not depend on geometry.
 * - The interaction points are stationary (Fermat), so the total derivative with respect to a wall's end points is the partial derivative at a fixed position along the wall.
 * - Take bounce `i` on wall `w` with end points `A`, `B`, `T = B − A`, and unit normal `n = normalize((T_y, −T_x))`, which is `refl[2w].zw` of the wall table. With `u_in = unit(p[i] − p[i−1])` and the relative position `s = ((p[i] − A)·T)/|T|²`: `∂r/∂A = γ (1 − s) n`, `∂r/∂B = γ s n`, `γ = 2 (u_in · n)`. The sign of `n` cancels.
 * - The result is for `dL = Σ (re_bar·dre + im_bar·dim)`, with `re`, `im` those of `d2d_frequency_response_launch` for the same arguments. There are two outputs.
 * - `normal_bar[w][0..1]`, fp64: `Σ_cells Σ_paths Σ_bounces on w` of `G·γ·(1−s)` and of `G·γ·s`. This is the sensitivity of `L` to moving end point `A` or `B` of wall `w` along the wall's unit normal.
 * - `walls_bar[w][e][d] = normal_bar[w][e] · (double)n_w[d]`, fp64 `[N][2][2]`. This is the layout of `d2d_get_scene_vjp`'s `xys_bar`. The getter forms it in fp64 from the fp32 normals of the wall table, and adds `+ 0.0`: a zero product is `+0.0` whatever the normal's sign.
 *
 * All arithmetic is fp32, one rounding per stated operation, no contraction. Blocks hold `D2D_POS_CHUNK = 8` wavelengths. `G` rounds once per block, as in K3-X. Per contribution:
 *
 *     for blocks of POS_CHUNK wavelengths, in list order:
 *       for candidates in the sweep's enumeration order (walls cand[0..K), K >= 1; the line of sight adds nothing):
 *         t = valid * fun ; r = path_length(points) ; seg[i] = p[i+1] − p[i], i < K      // what MaterialSink gets
 *         if (t == 0) continue
 *         G = posgrad_amp(..) * fold of posgrad_fold over the block                      // d2d_posgrad.hpp, unchanged: dL/dr
 *         q = p[0]                                   // the transmitter: `fixed` on an RX grid, the cell's (X, Y) on a TX grid
 *         for i in 0..K-1:
 *             q = q + seg[i]                         // componentwise: the bounce point, rebuilt from the hand-outs
 *             (ux, uy, ok) = unit_dir(seg[i])        // d2d_steer.hpp, unchanged
 *             {ox, oy, nx, ny} = refl[2w] ; {tx, ty, sq, _} = refl[2w+1] ,  w = cand[i]
 *             gam = 2.0f * steer_dot(ux, uy, nx, ny)
 *             s   = ((q.x − ox)*tx + (q.y − oy)*ty) / sq
 *             wa  = G * gam ; Wb = wa * s ; Wa = wa − Wb          // Wa + Wb == wa: a rigid shift along n gets the whole term
 *             if (ok) { row[w][0] += Wa ; row[w][1] += Wb }       // a wall that occurs twice in a candidate gets both terms
 *     normal_bar = fixed-order fp64 sum of the per-patch rows
 *
 * - The bounce arithmetic (`q`, `gam`, `s`, `wa`, `Wa`, `Wb`, `ok`) is the text of `differt2d_amd/csrc/d2d_wallgrad.hpp`, which compiles for host and device.
 * - A row is one 8 x 8 patch's fp32 sums: the contributing lanes' weights of one bounce are added over the patch's wave, and that sum is added to the row, candidates and bounces in order.
 * - A zero-length wall has `n = (0,0)` in the table and therefore adds `±0`.
 * - A bounce whose incoming segment has no unit vector adds nothing; `q` still advances.
 * - Being a sum over cells, the result is defined to a derived bound against a float64 oracle, like K3-G and K3-E. It is not defined bit for bit.
 * - The same call gives the same bits run to run, whatever ran before on the context.
 * - All-zero cotangents give `+0.0` in every entry. Cotangents ×2 give exactly doubled entries. Appending a wavelength with zero planes changes no bit.
 * - Walls that no contributing candidate touches are exactly `+0.0`. A sweep of order 0 alone gives all zeros.
 * - A NaN contribution makes the entries of that candidate's walls NaN and no others.
 *
 * One preparation of the culled sweep and ceil(nf / D2D_POS_CHUNK) passes of one kernel: the cotangents of a block sit in registers,
 * lane 0 of every patch's wave is the only writer of the patch's row [N][2], the rows are zeroed in front of the first pass and carried
 * from pass to pass, and one fixed-order reduction sums them into fp64.  A sweep without a patch and a scene without walls leave zeros.
 * The launch touches none of: the resident value / gradient maps, the scene VJP of d2d_power_map_vg_launch, the work history, the
 * other products' results.
 * D2D_ERR_INVALID: a NULL argument; nf outside 1 .. D2D_FREQ_MAX; an inv_wavelength entry that is negative, NaN or infinite (the
 * message names its index); an unknown amplitude.
 * D2D_ERR_UNSUPPORTED (the message names the reason): hard_sigmoid and sigmoid validity -- a smoothed validity depends on the walls'
 * end points itself, and its term needs the reverse chain of the value+grad sweep (d2d_power_map_vg_launch, whose objects_bar has it
 * for the incoherent map) -- and what d2d_frequency_response_launch refuses, with 8 * nf bytes per cell plus 8 bytes per patch and
 * wall held against half of the free device memory.  All decided before anything is enqueued; a refused launch leaves the previous
 * result readable.
 * Not computed: hard_sigmoid / sigmoid validity, the array, beam and material variants (where the angle of incidence also moves),
 * RIS angles, more than one GPU, D2D_OUT_ADD. */
int d2d_field_walls_vjp_launch(d2d_ctx* ctx, const d2d_params* params, const float* fixed /* [2] */,
                               const float* inv_wavelength /* [nf] */, int32_t nf, int32_t amplitude,
                               const float* re_bar /* [nf][m][n] */, const float* im_bar /* [nf][m][n] */);
/* Synchronises and copies the result of the last accepted d2d_field_walls_vjp_launch to the arrays that are not NULL.
 * D2D_ERR_STATE before a launch and after a d2d_set_grid / d2d_set_scene of another grid or scene (the result goes with both). */
int d2d_get_field_walls_vjp(d2d_ctx* ctx, double* walls_bar /* [N][2][2] or NULL */, double* normal_bar /* [N][2] or NULL */);
/* The per-bounce arithmetic of d2d_wallgrad.hpp on the device, for comparison with its host build: in[12] = G, qx, qy, sx, sy, ox,
 * oy, nx, ny, tx, ty, sq (n values each); for every i, wallgrad_bounce gives qx, qy after the bounce, Wa, Wb and ok as 1 / 0. */
int d2d_selftest_wallgrad(d2d_ctx* ctx, const float* const* in /* [12] */, int64_t n, float* qx, float* qy, float* Wa, float* Wb,
                          float* ok);

/* ---- multi-GPU (one process per GPU; the reference has no multi-device code: its only batching is jax.vmap
 *      over the grid, differt2d/scene.py:1927-1932; RX rows are sharded over ranks and maps are assembled with one
 *      RCCL all-gather on the ctx stream; the scene VJP with one all-reduce) ------------------------------------- */

#define D2D_COMM_ID_BYTES 128
/* Rank 0 creates the id (ncclGetUniqueId) and ships it to the other ranks out of band. */
int d2d_comm_unique_id(uint8_t* id /* [D2D_COMM_ID_BYTES] */);
/* Collective: ncclCommInitRank on the ctx's device. */
int d2d_comm_init(d2d_ctx* ctx, const uint8_t* id, int32_t rank, int32_t world);
int d2d_comm_destroy(d2d_ctx* ctx);
/* Ranks of the communicator as RCCL itself reports them (ncclCommCount): what bench.py prints as `rccl_ranks`. */
int d2d_comm_count(d2d_ctx* ctx, int32_t* ranks);
/* Collective, asynchronous: all-gathers this rank's resident map (what = 0: value map, m*n floats; what = 1:
 * grad_rx map, m*n*2 floats; every rank must hold the same m, n) into a resident buffer [world][...]. The map is
 * first copied aside on the ctx stream and the all-gather runs on a second stream behind that copy, so the NEXT sweep
 * on this ctx overlaps with it; d2d_synchronize, d2d_timer_end, d2d_comm_get_gathered and d2d_comm_allreduce_host wait
 * for the collectives in flight. */
int d2d_comm_allgather_map(d2d_ctx* ctx, int32_t what);
/* Collective, asynchronous: the same maps gathered to ONE rank -- what the reference's single-process caller receives
 * (one assembled m x n (x 2) array, differt2d/scene.py:1927-1953): ncclSend from every other rank, world - 1 ncclRecv on
 * `root` (xGMI is point to point: 7 direct links into the root, 1/world of the all-gather's bytes per GPU).  Same staging
 * copy, second stream and overlap as the all-gather; only `root` may call d2d_comm_get_gathered afterwards. */
int d2d_comm_gather_map(d2d_ctx* ctx, int32_t what, int32_t root);
/* Synchronises and copies the gathered map (what = 0 / 1 as above; the two are kept in separate buffers, so a step may
 * gather both) to out[world * per_rank]; capacity (in floats) must be exactly that. */
int d2d_comm_get_gathered(d2d_ctx* ctx, int32_t what, float* out, int64_t capacity);
/* Collective, asynchronous: sums the resident scene VJP (fp64, 4N+2 values, + N for phi, + N for the reflection coefficients) over ranks in place, on the
 * communication stream behind the reduction that produced it; d2d_get_scene_vjp waits for it. */
int d2d_comm_allreduce_vjp(d2d_ctx* ctx);

/* Collective, synchronous: all-reduces n host doubles over ranks through the GPUs (op 0 = sum, 1 = max).
 * A sum of one value is the barrier; a max is how bench.py takes the slowest rank's time. */
int d2d_comm_allreduce_host(d2d_ctx* ctx, double* values, int32_t n, int32_t op);

/* ---- timing on the ctx stream (HIP events) -------------------------------------------------- */

int d2d_timer_begin(d2d_ctx* ctx);
int d2d_timer_end(d2d_ctx* ctx, float* elapsed_ms); /* synchronises on the end event */

#ifdef __cplusplus
}
#endif
#endif /* D2D_H */
