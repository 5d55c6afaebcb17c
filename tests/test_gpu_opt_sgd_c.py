"""
GPU tests of the MinPath / FermatPath solvers with SGD (differt2d_amd.optimize.sgd) against the C solver oracle
(oracle/d2d_oracle_opt.c with an orc_opt_optimizer of SGD / SGD with a trace, pinned to oracle/ref.py by
tests/test_oracle_opt_c.py): every SGD instance of the solver kernels -- the forward sweep one lane per cell and side by side,
the trace, the forward-tangent gradient, the reverse sweep for every order and for a host-evaluated `fun` -- at orders 0..3,
both grid roles, every validity mode, every SGD kind (plain, momentum, Nesterov, momentum 0.0), and the reverse sweep's
trajectory store cut into chunks, for SGD and Adam.

Bars: values and per-cell gradients on the cells the ORACLE calls well conditioned (CO.opt_conditioning), at the rule of
tests/test_gpu_opt.py::test_cfg5_full_map_against_the_c_oracle; the scene VJP against reverse-mode autodiff of ref.py at
_tight's bar; launch variants bit for bit.
"""

import time

import numpy as np
import pytest

from test_gpu_opt import _odd_host, _odd_oracle, _opt_case, _oracle_objs, _oracle_stable, _ris_scene, _scene_tables, _tight
from test_oracle_opt_c import SGD_SPECS, _sgd_spec

pytestmark = pytest.mark.gpu

F = np.float32
MODES = {"hard": dict(approx=False), "hard_sigmoid": dict(approx=True, function="hard_sigmoid"), "sigmoid": dict(approx=True, function="sigmoid")}


def _sgd(name, solver):
    from differt2d_amd.optimize import sgd

    lr, momentum, nesterov = _sgd_spec(name, solver)
    return sgd(lr, momentum=momentum, nesterov=nesterov)


def _co_kw(name, solver):
    from oracle import c_oracle as CO

    return CO.sgd_kwargs(*_sgd_spec(name, solver))


def _three_object_scene():
    """Two walls and a RIS facing each other across the unit square: every order-3 candidate (3 x 2 x 2 of them) has a solve."""
    xys = np.array([[[0.1, 0.05], [0.9, 0.1]], [[0.95, 0.2], [0.9, 0.85]], [[0.8, 0.95], [0.1, 0.9]]], F)
    kind = np.array([0, 1, 0], np.uint8)
    phi = np.array([0.0, 0.3, 0.0], F)
    return xys, kind, phi


def _theta0(kind, cands, seed):
    rng = np.random.default_rng(seed)
    full = [rng.random(4, dtype=F) for _ in cands]
    th = [t[: sum(int(kind[int(i)]) != 2 for i in c)] for c, t in zip(cands, full)]
    return full, th


def _ref_yardstick(kind, xys, phi, fixed, X, Y, cands, th, spec, **okw):
    """cells [n, 2] -> per-cell gradients (fp64, fp32) of reverse-mode autodiff of ref.py through sgd_minimize on those cells."""
    from oracle import ref as R

    def run(cells):
        Xc, Yc = X[cells[:, 0], cells[:, 1]][None], Y[cells[:, 0], cells[:, 1]][None]  # (one batched call per precision)
        with R.sgd_hyper(*spec):
            return tuple(R.opt_value_and_grads(kind, np.asarray(xys, np.float64), phi, fixed, Xc, Yc, cands, th, dtype=dt, **okw)["grad_cell"][0]
                         for dt in ("float64", "float32"))

    return run


def _check_against_the_oracle(got_v, got_g, cond, name, yardstick=None):
    """Values on the well-conditioned cells within 1e-5 of the map's scale (+ 1e-5 relative) of the fp64 oracle or twice the
    oracle's own fp32 distance; per-cell gradients (where the oracle's derivative through the loop is itself well conditioned:
    its fp32 run and its run from a cell one ulp away within 1e-2 of the cell's scale of fp64) within max(1e-5, twice what the
    oracle's own fp32 runs lose) of the cell's scale; NaN positions of the gradient those of the oracle's fp32 run.  A few
    offenders go to test_cfg5_full_map_against_the_c_oracle's second yardstick, the reference chain's own fp32 REVERSE mode
    through the loop (`yardstick`, ref.py under torch): within max(1e-5, twice its distance from fp64) of the cell's scale --
    forward-mode probes of the oracle do not see what summing an adjoint over the loop in fp32 loses."""
    stable, v64, scale = cond["stable"], cond["value64"], cond["scale"]
    assert stable.mean() >= 0.7, f"{name}: only {int(stable.sum())} of {stable.size} cells well conditioned in the oracle"
    bar = np.maximum(1e-5 * scale + 1e-5 * np.abs(v64), 2.0 * cond["dist"])
    err = np.abs(got_v.astype(np.float64) - v64)
    assert (err <= bar)[stable].all(), f"{name}: value beyond the bar on {int((err > bar)[stable].sum())} of {int(stable.sum())} cells"
    if got_g is None:
        return 0
    g, g64, g32, g32t, g32n = got_g.astype(np.float64), cond["grad64"], cond["grad32"], cond["grad32t"], cond["grad32n"]
    assert np.array_equal(np.isnan(g)[stable], np.isnan(g32)[stable]), f"{name}: NaN positions of the per-cell gradient"
    fin = np.isfinite(g64).all(-1) & np.isfinite(g32).all(-1) & np.isfinite(g32n).all(-1) & stable
    if not fin.any():
        return 0
    gs = np.maximum(np.abs(np.nan_to_num(g64)).max(-1), np.median(np.abs(g64[fin]).max(-1)))[..., None] + 1e-30
    with np.errstate(invalid="ignore"):
        fin &= (np.abs(g32 - g64) <= 1e-2 * gs).all(-1) & (np.abs(g32n - g64) <= 1e-2 * gs).all(-1)
        gerr = np.abs(g - g64) / gs
        gref = np.maximum(np.maximum(np.abs(g32 - g64), np.nan_to_num(np.abs(g32t - g64))), np.abs(g32n - g64)) / gs
        bad = fin & ~(gerr <= np.maximum(1e-5, 2.0 * gref)).all(-1)
    if bad.any() and yardstick is not None and bad.sum() <= 16:
        wb = np.argwhere(bad)
        t64, t32 = yardstick(wb)
        for i, w in enumerate(map(tuple, wb)):
            if np.isfinite(t32[i]).all() and (np.abs(g[w] - t64[i]) / gs[w] <= np.maximum(1e-5, 2.0 * np.abs(t32[i] - t64[i]) / gs[w])).all():
                bad[w] = False
        print(f"   {name}: {len(wb)} cells to the reverse-mode yardstick, {int(bad.sum())} still beyond")
    assert not bad.any(), (f"{name}: per-cell gradient beyond the bar on {int(bad.sum())} of {int(fin.sum())} cells, worst "
                           f"{float(gerr[bad].max()):.2e} of the cell's scale (oracle fp32: {float(gref[bad].max()):.2e}): {np.argwhere(bad)[:4].tolist()}")
    return int(fin.sum())


# ---- the matrix: solver x SGD kind x grid role x validity mode x gradient kernel, orders 0..2 -------------------------------


@pytest.mark.parametrize("name", list(SGD_SPECS))
@pytest.mark.parametrize("solver", ["min", "fermat"])
def test_sgd_values_and_per_cell_gradients_match_the_c_oracle(solver, name):
    """RIS + walls + vertices, orders 0..2 (1 + 7 + 42 candidates: power_opt_rev_kernel<1|2, false, true>), both grid roles, hard
    / hard_sigmoid (approx) / sigmoid validity: the value map of the forward sweep, and value and per-cell gradient of both
    gradient kernels (opt_grad_mode 0: reverse mode over the stored trajectory, 1: forward tangents)."""
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import default_context
    from oracle import c_oracle as CO

    steps = 24
    scene, xys, kind, phi, X, Y, _, _ = _opt_case(steps, solver, True, grid=(7, 5))
    cands = L.enumerate_candidates(len(kind), 0, 2, None)
    theta0, th = _theta0(kind, cands, 17)
    fixed = scene.transmitters["tx"].xy
    ctx = default_context()
    ctx.set_scene(xys, kind, phi)
    ctx.set_theta0(theta0)
    n_grad = 0
    try:
        ctx.set_optimizer(_sgd(name, solver))
        for role in ("rx", "tx"):
            for mode, mkw in MODES.items():
                # (a few dozen cells: a handful of threads -- a wide OpenMP team costs more to wake than the work)
                cond = CO.opt_conditioning(kind, xys, phi, fixed, X, Y, cands, th, steps, with_grad=True, solver=solver, grid_role=role,
                                           nthreads=8, **mkw, **_co_kw(name, solver))
                yard = _ref_yardstick(kind, xys, phi, fixed, X, Y, cands, th, _sgd_spec(name, solver), solver=solver, steps=steps, grid_role=role, **mkw)
                gkw = dict(solver=solver, steps=steps, min_order=0, max_order=2, grid_role=L.GRID_TX if role == "tx" else L.GRID_RX, **mkw)
                fwd = ctx.power_map(fixed, X, Y, **gkw)
                _check_against_the_oracle(fwd, None, cond, f"{name} {role} {mode} forward")
                for grad_mode in (0, 1):
                    ctx.set_option("opt_grad_mode", grad_mode)
                    out = ctx.value_and_grads(fixed, X, Y, **gkw)
                    assert np.array_equal(out["value"], fwd, equal_nan=True), f"{name} {role} {mode} mode {grad_mode}: value map of the gradient sweep"
                    n_grad += _check_against_the_oracle(out["value"], out["grad_rx"], cond, f"{name} {role} {mode} mode {grad_mode}", yard)
                ctx.set_option("opt_grad_mode", 0)
    finally:
        ctx.set_option("opt_grad_mode", 0)
        ctx.set_optimizer(None)
    assert n_grad > 0
    print(f"{solver} {name}: {n_grad} per-cell gradients compared")


@pytest.mark.parametrize("solver", ["min", "fermat"])
def test_sgd_order_3_matches_the_c_oracle(solver):
    """Three objects, order 3 (power_opt_rev_kernel<3, false, true>) with Nesterov, hard_sigmoid validity: values and per-cell
    gradients of both gradient kernels, both grid roles.  The fixed point is one where a quarter to a half of the cells have a
    valid order-3 path in every solver and role: a map left in the sigmoid's tail (values ~1e-6) holds nothing but the fp32
    rounding of the activation's argument, alpha ulp(1) ~ 1e-5 relative, which no two fp32 evaluations share."""
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import default_context
    from oracle import c_oracle as CO

    steps = 30
    xys, kind, phi = _three_object_scene()
    X, Y = np.meshgrid(np.linspace(0.2, 0.8, 8).astype(F), np.linspace(0.25, 0.75, 6).astype(F))
    fixed = np.array([0.3, 0.6], F)
    cands = L.enumerate_candidates(len(kind), 3, 3, None)
    assert len(cands) == 12
    theta0, th = _theta0(kind, cands, 23)
    ctx = default_context()
    ctx.set_scene(xys, kind, phi)
    ctx.set_theta0(theta0)
    try:
        ctx.set_optimizer(_sgd("nesterov", solver))
        for role in ("rx", "tx"):
            mkw = MODES["hard_sigmoid"]
            cond = CO.opt_conditioning(kind, xys, phi, fixed, X, Y, cands, th, steps, with_grad=True, solver=solver, grid_role=role,
                                       nthreads=8, **mkw, **_co_kw("nesterov", solver))
            yard = _ref_yardstick(kind, xys, phi, fixed, X, Y, cands, th, _sgd_spec("nesterov", solver), solver=solver, steps=steps, grid_role=role, **mkw)
            gkw = dict(solver=solver, steps=steps, min_order=3, max_order=3, grid_role=L.GRID_TX if role == "tx" else L.GRID_RX, **mkw)
            for grad_mode in (0, 1):
                ctx.set_option("opt_grad_mode", grad_mode)
                out = ctx.value_and_grads(fixed, X, Y, **gkw)
                _check_against_the_oracle(out["value"], out["grad_rx"], cond, f"order 3 {role} mode {grad_mode}", yard)
                assert np.abs(out["value"]).max() > 0 and np.abs(np.nan_to_num(out["grad_rx"])).max() > 0
    finally:
        ctx.set_option("opt_grad_mode", 0)
        ctx.set_optimizer(None)


@pytest.mark.parametrize("solver", ["min", "fermat"])
def test_sgd_order_2_scene_vjp_matches_autodiff_of_the_oracle(solver):
    """The scene VJP (fixed end point, object end points, phi) of an order-2 SGD sweep (momentum) against reverse-mode autodiff
    of ref.py through sgd_minimize -- the C oracle has no VJP -- with the cotangent masked to the cells where ref.py is well
    conditioned, at _tight's bar; per-cell gradients too."""
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import default_context
    from oracle import ref as R

    steps = 30
    xys, kind, phi = _three_object_scene()
    X, Y = np.meshgrid(np.linspace(0.2, 0.8, 6).astype(F), np.linspace(0.25, 0.75, 5).astype(F))
    fixed = np.array([0.35, 0.4], F)
    cands = L.enumerate_candidates(len(kind), 2, 2, None)
    theta0, th = _theta0(kind, cands, 29)
    cot = (np.random.default_rng(5).random(X.shape) + 0.5).astype(F)
    okw = dict(solver=solver, steps=steps, grid_role="rx", approx=True)
    with R.sgd_hyper(*_sgd_spec("momentum", solver)):
        w64 = R.opt_value_and_grads(kind, xys, phi, fixed, X, Y, cands, th, dtype="float64", cotangent=cot, **okw)
        w32 = R.opt_value_and_grads(kind, xys, phi, fixed, X, Y, cands, th, dtype="float32", cotangent=cot, **okw)
        stable = _oracle_stable(w64["value"], w32["value"], w64["grad_cell"], w32["grad_cell"])
        assert stable.mean() >= 0.8
        cot_m = (cot * stable).astype(F)
        if not stable.all():
            w64 = R.opt_value_and_grads(kind, xys, phi, fixed, X, Y, cands, th, dtype="float64", cotangent=cot_m, **okw)
            w32 = R.opt_value_and_grads(kind, xys, phi, fixed, X, Y, cands, th, dtype="float32", cotangent=cot_m, **okw)
    ctx = default_context()
    ctx.set_scene(xys, kind, phi)
    ctx.set_theta0(theta0)
    try:
        ctx.set_optimizer(_sgd("momentum", solver))
        g = ctx.value_and_grads(fixed, X, Y, cotangent=cot_m, solver=solver, steps=steps, min_order=2, max_order=2, approx=True, grid_role=L.GRID_RX)
    finally:
        ctx.set_optimizer(None)
    _tight(g["grad_rx"][stable], w64["grad_cell"][stable], w32["grad_cell"][stable], f"{solver} order 2 per-cell gradient")
    _tight(g["tx_bar"], w64["fixed_bar"], w32["fixed_bar"], f"{solver} order 2 fixed end point")
    _tight(g["walls_bar"], w64["xys_bar"], w32["xys_bar"], f"{solver} order 2 object end points")
    _tight(g["phi_bar"], w64["phi_bar"], w32["phi_bar"], f"{solver} order 2 phi")
    assert np.abs(w64["xys_bar"]).max() > 0


# ---- trajectories -------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("steps", [1, 10, 50])
@pytest.mark.parametrize("solver", ["min", "fermat"])
def test_sgd_trajectory_matches_the_c_oracle_after_few_steps(solver, steps):
    """trace_paths (trace_kernel<true>) after 1, 10 and 50 SGD steps, every SGD kind: interaction points within 1e-6 of the
    fp64 oracle, or four times the oracle's own fp32 distance; recorded losses within rtol 1e-4 / atol 1e-6 of fp64 or four
    times the oracle's own fp32 distance (test_gpu_opt.py's trajectory test with the C oracle as the yardstick)."""
    from differt2d_amd.engine import default_context, make_params
    from oracle import c_oracle as CO

    scene = _ris_scene()
    xys, kind, phi = _scene_tables(scene)
    objs = _oracle_objs(scene)
    cands = [np.array(c, np.int32) for c in ([0], [1], [2], [3], [4], [5], [0, 4], [4, 1], [3, 5], [2, 0, 4])]
    rng = np.random.default_rng(11)
    th = [rng.random(sum(objs[int(i)].parameters_count() for i in c), dtype=F) for c in cands]
    tx = np.array([[0.2, 0.2], [0.31, 0.77], [0.9, 0.12]], F)
    rx = np.array([[0.8, 0.6], [0.62, 0.18], [0.15, 0.85]], F)
    ctx = default_context()
    ctx.set_scene(xys, kind, phi)
    p = make_params(min_order=0, max_order=4, solver=solver, steps=steps, approx=True)
    worst = 0.0
    try:
        for name in SGD_SPECS:
            ctx.set_optimizer(_sgd(name, solver))
            got = ctx.trace_paths(p, tx, rx, cands, theta0=[np.pad(t, (0, 4 - len(t))) for t in th])
            for i in range(tx.shape[0]):
                res = {dt: CO.opt_power_map(kind, xys, phi, tx[i], rx[i, :1], rx[i, 1:], cands, th, dtype=dt, with_paths=True, steps=steps,
                                            solver=solver, approx=True, nthreads=1, **_co_kw(name, solver)) for dt in ("float64", "float32")}
                p64, l64 = res["float64"][1][0, :, 0], res["float64"][2][0]
                p32, l32 = res["float32"][1][0, :, 0], res["float32"][2][0]
                for ci, c in enumerate(cands):
                    k = len(c)
                    g = got["xys"][i, ci, 1 : k + 1].astype(np.float64)
                    ref_err = float(np.abs(p32[ci, :k] - p64[ci, :k]).max())
                    err = float(np.abs(g - p64[ci, :k]).max())
                    worst = max(worst, err)
                    assert err <= max(1e-6, 4.0 * ref_err), f"{name} pair {i} candidate {c.tolist()} after {steps} steps: {err:.2e} (oracle fp32: {ref_err:.2e})"
                    lerr, lref = abs(float(got["loss"][i, ci]) - l64[ci]), abs(l32[ci] - l64[ci])
                    assert lerr <= max(1e-4 * abs(l64[ci]) + 1e-6, 4.0 * lref), f"{name} pair {i} candidate {c.tolist()}: loss {got['loss'][i, ci]} vs {l64[ci]}"
    finally:
        ctx.set_optimizer(None)
    print(f"{solver} {steps} steps: max |points - C oracle (fp64)| = {worst:.2e}")
    if steps == 1:
        assert worst <= 1e-6


# ---- the chunked reverse sweep --------------------------------------------------------------------------------------------


def _chunks(per_cell_floats, cells, traj_mb):
    """d2d_host::opt_chunk_cells (differt2d_amd/csrc/d2d_host.hpp): cells per chunk for a trajectory budget of traj_mb MiB."""
    cells_pad = (cells + 63) // 64 * 64
    return min(cells_pad, max(64, (traj_mb << 20) // (4 * per_cell_floats) // 64 * 64))


@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
def test_chunked_reverse_sweep_equals_one_chunk(optimizer):
    """opt_traj_mb = 1: the reverse sweep runs over the grid in at least three chunks, the last a partial one whose cell count
    is not a multiple of 64 (SGD stores 1 float per step and unknown, Adam 4: the steps differ so that both cut the grid
    similarly).  Against the one-chunk sweep on the same context: values, per-cell gradients and the scene VJP bit for bit.
    The VJP can be bit for bit: every workgroup writes its partial sums to the row of its GLOBAL block index
    (cell0 / 64 + blockIdx.x, and a chunk starts on a multiple of 64 cells), and vjp_reduce_kernel then sums those rows in
    the same fixed order however many launches wrote them."""
    from differt2d_amd.engine import default_context
    from differt2d_amd.optimize import adam, sgd

    steps = 200 if optimizer == "sgd" else 50
    scene, xys, kind, phi, X, Y, cands, theta0 = _opt_case(steps, "min", True, grid=(30, 27))
    fixed = scene.transmitters["tx"].xy
    per_cell = (1 if optimizer == "sgd" else 4) * steps * sum(int(kind[int(i)]) != 2 for c in cands for i in c)
    chunk = _chunks(per_cell, X.size, 1)
    n_chunks = -(-X.size // chunk)
    assert n_chunks >= 3 and (X.size % chunk) % 64 != 0, (chunk, n_chunks)
    cot = (np.random.default_rng(5).random(X.shape) + 0.5).astype(F)
    ctx = default_context()
    ctx.set_scene(xys, kind, phi)
    ctx.set_theta0([np.pad(np.asarray(t, F), (0, 4 - len(t))) for t in theta0])
    kw = dict(solver="min", steps=steps, min_order=0, max_order=1, approx=True)
    try:
        ctx.set_optimizer(sgd(0.005, momentum=0.3) if optimizer == "sgd" else adam(0.05))
        one = ctx.value_and_grads(fixed, X, Y, cotangent=cot, **kw)
        ctx.set_option("opt_traj_mb", 1)
        cut = ctx.value_and_grads(fixed, X, Y, cotangent=cot, **kw)
    finally:
        ctx.set_option("opt_traj_mb", 16384)
        ctx.set_optimizer(None)
    for k in ("value", "grad_rx", "tx_bar", "walls_bar", "phi_bar"):
        assert np.array_equal(one[k], cut[k], equal_nan=True), f"{optimizer}: {k} differs between {n_chunks} chunks of {chunk} cells and one chunk"
    assert np.isfinite(one["grad_rx"]).mean() > 0.8 and np.abs(one["walls_bar"]).max() > 0
    print(f"{optimizer}: {X.size} cells in {n_chunks} chunks of {chunk} (last {X.size - (n_chunks - 1) * chunk})")


# ---- launch variants --------------------------------------------------------------------------------------------------


def test_sgd_candidates_side_by_side_equal_one_after_the_other():
    """power_opt_cand_kernel<true> (candidates side by side) against power_opt_kernel<true> (one lane per cell): bit for bit."""
    from differt2d_amd.engine import default_context

    scene, xys, kind, phi, X, Y, cands, theta0 = _opt_case(60, "min", True, grid=(40, 33))
    fixed = scene.transmitters["tx"].xy
    ctx = default_context()
    ctx.set_scene(xys, kind, phi)
    ctx.set_theta0([np.pad(np.asarray(t, F), (0, 4 - len(t))) for t in theta0])
    try:
        for solver in ("min", "fermat"):
            ctx.set_optimizer(_sgd("nesterov", solver))
            kw = dict(solver=solver, steps=60, min_order=0, max_order=1, approx=True)
            a = ctx.power_map(fixed, X, Y, **kw)
            ctx.set_option("opt_parallel", 0)
            b = ctx.power_map(fixed, X, Y, **kw)
            ctx.set_option("opt_parallel", 1)
            assert np.array_equal(a, b, equal_nan=True) and np.isfinite(a).all() and (a > 0).any(), solver
    finally:
        ctx.set_option("opt_parallel", 1)
        ctx.set_optimizer(None)


def test_sgd_many_random_starts():
    """many = 3 with SGD: three identical starts give many = 1's value map and gradients bit for bit; three distinct starts of
    one candidate (the others' starts identical) give, cell by cell, the single-start sweep whose start has the smallest
    recorded loss (the first on ties; trace_kernel<true> with many = 3 picks the same)."""
    from differt2d_amd.engine import default_context, make_params

    steps = 40
    scene, xys, kind, phi, X, Y, cands, theta0 = _opt_case(steps, "min", True, grid=(9, 7))
    fixed = scene.transmitters["tx"].xy
    th1 = [np.pad(np.asarray(t, F), (0, 4 - len(t))) for t in theta0]
    ctx = default_context()
    ctx.set_scene(xys, kind, phi)
    kw = dict(solver="min", steps=steps, min_order=0, max_order=1, approx=True)
    try:
        ctx.set_optimizer(_sgd("momentum", "min"))
        ctx.set_theta0(th1)
        one = ctx.value_and_grads(fixed, X, Y, **kw)
        ctx.set_theta0([t for t in th1 for _ in range(3)])
        three = ctx.value_and_grads(fixed, X, Y, many=3, **kw)
        for k in ("value", "grad_rx"):
            assert np.array_equal(one[k], three[k], equal_nan=True), k
        rng = np.random.default_rng(4)
        P = X.size
        txp, rxp = np.broadcast_to(fixed, (P, 2)), np.stack([X.reshape(-1), Y.reshape(-1)], -1)
        for ci in (1, 5):  # a wall, the RIS
            starts = [rng.random(4, dtype=F) for _ in range(3)]
            singles, losses = [], []
            for s in starts:
                th = [s if i == ci else t for i, t in enumerate(th1)]
                ctx.set_theta0(th)
                singles.append(ctx.power_map(fixed, X, Y, **kw))
                losses.append(ctx.trace_paths(make_params(**kw), txp, rxp, cands, theta0=th)["loss"][:, ci].reshape(X.shape))
            multi_th = [x for i, t in enumerate(th1) for x in (starts if i == ci else [t, t, t])]
            ctx.set_theta0(multi_th)
            got = ctx.power_map(fixed, X, Y, many=3, **kw)
            tr = ctx.trace_paths(make_params(many=3, **kw), txp, rxp, cands, theta0=multi_th)
            L_ = np.stack(losses)
            best = np.where(np.isnan(L_).any(0), np.argmax(np.isnan(L_), 0), np.argmin(np.where(np.isnan(L_), np.inf, L_), 0))
            want = np.choose(best, singles)
            assert np.array_equal(got, want, equal_nan=True), f"candidate {ci}: {int((got != want).sum())} cells"
            assert np.array_equal(tr["loss"][:, ci].reshape(X.shape), np.choose(best, L_), equal_nan=True)
            assert len(set(best.reshape(-1).tolist())) > 1  # the starts do compete
    finally:
        ctx.set_theta0(th1)
        ctx.set_optimizer(None)


@pytest.mark.parametrize("role", ["rx", "tx"])
def test_sgd_gradient_of_a_host_evaluated_fun_through_the_solver(role):
    """The SGD twin of test_gpu_opt.py::test_gradient_of_a_host_evaluated_fun_through_the_solver (power_opt_rev_kernel<1, true,
    true>): a `fun` only the host can evaluate, chained through the reverse pass over the stored SGD trajectory, against
    reverse-mode autodiff of ref.py through sgd_minimize with the same function, at the image-method bar."""
    from differt2d_amd.geometry import MinPath, Point
    from oracle import ref as R

    steps, solver = 40, "min"
    spec = _sgd_spec("momentum", solver)
    scene, xys, kind, phi, X, Y, cands, theta0 = _opt_case(steps, solver, True, grid=(8, 6), role=role)
    fixed = scene.transmitters["tx"].xy
    if role == "rx":
        sweep = scene.accumulate_on_receivers_grid_over_paths
    else:
        scene = scene.with_transmitters().with_receivers(rx=Point(xy=fixed))
        sweep = scene.accumulate_on_transmitters_grid_over_paths
    kw = dict(path_cls=MinPath, min_order=0, max_order=1, approx=True, reduce_all=True, value_and_grad=True,
              path_cls_kwargs={"steps": steps, "theta0": theta0, "optimizer": _sgd("momentum", solver)})
    Z, G = sweep(X, Y, fun=_odd_host, fun_kwargs=dict(w=0.25), **kw)
    okw = dict(solver=solver, steps=steps, grid_role=role, approx=True, fun=_odd_oracle, fun_kwargs=dict(w=0.25))
    with R.sgd_hyper(*spec):
        w64 = R.opt_value_and_grads(kind, xys, phi, fixed, X, Y, cands, theta0, dtype="float64", **okw)
        w32 = R.opt_value_and_grads(kind, xys, phi, fixed, X, Y, cands, theta0, dtype="float32", **okw)
    stable = _oracle_stable(w64["value"], w32["value"], w64["grad_cell"], w32["grad_cell"])
    assert stable.mean() >= 0.8
    _tight(Z[stable], w64["value"][stable], w32["value"][stable], f"{role} host fun: value")
    _tight(G[stable], w64["grad_cell"][stable], w32["grad_cell"][stable], f"{role} host fun: per-cell gradient")


def test_sgd_momentum_zero_equals_plain_sgd_without_nan():
    """D2D_OPT_SGD_MOMENTUM with momentum 0.0: m' = g + 0 m = g wherever m is finite, so the map, the per-cell gradient and the
    trajectories equal plain SGD's bit for bit -- the kind exists for the NaN a decay-0 trace carries forward, which no cell
    of this sweep meets."""
    from differt2d_amd.engine import default_context
    from differt2d_amd.optimize import sgd

    steps = 60
    scene, xys, kind, phi, X, Y, cands, theta0 = _opt_case(steps, "fermat", True, grid=(20, 16))
    fixed = scene.transmitters["tx"].xy
    ctx = default_context()
    ctx.set_scene(xys, kind, phi)
    ctx.set_theta0([np.pad(np.asarray(t, F), (0, 4 - len(t))) for t in theta0])
    out = {}
    try:
        for solver in ("min", "fermat"):
            lr = _sgd_spec("plain", solver)[0]
            kw = dict(solver=solver, steps=steps, min_order=0, max_order=1, approx=True)
            for k, o in (("plain", sgd(lr)), ("zero", sgd(lr, momentum=0.0))):
                ctx.set_optimizer(o)
                out[k] = ctx.value_and_grads(fixed, X, Y, **kw)
            assert np.isfinite(out["plain"]["value"]).all() and np.isfinite(out["plain"]["grad_rx"]).all(), solver
            for k in ("value", "grad_rx", "tx_bar", "walls_bar", "phi_bar"):
                assert np.array_equal(out["plain"][k], out["zero"][k]), (solver, k)
    finally:
        ctx.set_optimizer(None)


# ---- a configs[4]-sized SGD map ----------------------------------------------------------------------------------------


def test_cfg5_sized_sgd_map_against_the_c_oracle():
    """The configs[4] scene (tests/golden/cfg5_samples.npz: square + RIS + its two vertices, 7 order-1 candidates, MinPath,
    hard_sigmoid) with SGD + momentum on a 160 x 160 grid (400 launch blocks): values on every cell against the C oracle on its
    well-conditioned cells; per-cell gradients through the reverse sweep on four sampled rows."""
    import os

    from differt2d_amd.engine import default_context
    from oracle import c_oracle as CO
    from oracle import ref as R

    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "cfg5_samples.npz"))
    xys, kind, phi, tx = z["xys"], z["kind"], z["phi"], z["tx"]
    theta0 = [np.array([t, 0, 0, 0], F) if np.isfinite(t) else np.zeros(4, F) for t in z["theta0"]]
    th = [np.array([t], F) if np.isfinite(t) else np.zeros(0, F) for t in z["theta0"]]
    cands = R.all_path_candidates(7, order=1)
    steps = 200
    x = np.linspace(0.0, 1.0, 160).astype(F)
    X, Y = np.meshgrid(x, x)
    co = dict(solver="min", approx=True, **_co_kw("momentum", "min"))
    ctx = default_context()
    ctx.set_scene(xys, kind, phi)
    ctx.set_theta0(theta0)
    try:
        ctx.set_optimizer(_sgd("momentum", "min"))
        full = ctx.value_and_grads(tx, X, Y, min_order=1, max_order=1, approx=True, solver="min", steps=steps)
    finally:
        ctx.set_optimizer(None)
    t0 = time.time()
    cond = CO.opt_conditioning(kind, xys, phi, tx, X, Y, cands, th, steps, **co)
    _check_against_the_oracle(full["value"], None, cond, "cfg5 SGD map")
    t1 = time.time()
    rows = np.arange(13, 160, 40)
    cg = CO.opt_conditioning(kind, xys, phi, tx, X[rows], Y[rows], cands, th, steps, with_grad=True, **co)
    yard = _ref_yardstick(kind, xys, phi, tx, X[rows], Y[rows], cands, th, _sgd_spec("momentum", "min"), solver="min", steps=steps, approx=True)
    n = _check_against_the_oracle(full["value"][rows], full["grad_rx"][rows], cg, "cfg5 SGD rows", yard)
    assert n >= 0.7 * rows.size * X.shape[1]
    print(f"cfg5 SGD, {X.size} cells: {int(cond['stable'].sum())} well conditioned, oracle {t1 - t0:.1f} s; {n} per-cell gradients on "
          f"{rows.size} rows, oracle {time.time() - t1:.1f} s")
