"""
GPU tests of the MinPath / FermatPath solvers with SGD (differt2d_amd.optimize.sgd: optax 0.2.4's optax.sgd, plain, momentum
and Nesterov) -- the forward solver, the reverse sweep over its stored trajectory and the forward-tangent cross-check --
against the autodiff oracle (oracle/ref.py) with its Adam loop replaced by an SGD restatement (below).  The bars are those
of tests/test_gpu_opt.py, whose helpers these tests share.
"""

import numpy as np
import pytest

from test_gpu_opt import _gpu_opt_grads, _opt_case, _oracle_objs, _oracle_stable, _ris_scene, _scene_tables, _tight

from oracle.ref import sgd_minimize

pytestmark = pytest.mark.gpu

F = np.float32

# (learning_rate, momentum, nesterov): plain, trace, Nesterov.  Chosen where the reference chain is well conditioned on these
# grids: its fp32 gradients within 2e-6 of its fp64 ones, and moved by < 2e-6 when theta0 moves by one ulp.  (At lr 0.01 with
# momentum 0.8, MinPath's iteration is chaotic on some cells: a one-ulp change of theta0 moves the oracle's own fp32 gradient
# by orders of magnitude there, and no fp32 evaluation can be held to the _tight bar.)
SPECS = {"plain": (0.01, None, False), "momentum": (0.005, 0.3, False), "nesterov": (0.005, 0.5, True)}


def _sgd_oracle(monkeypatch, name):
    """The oracle's solvers (opt_path, opt_path_diff and with them opt_value_and_grads) run SGD `name`; returns the spec."""
    from differt2d_amd.optimize import sgd
    from oracle import ref as R

    lr, momentum, nesterov = SPECS[name]
    monkeypatch.setattr(R, "adam_minimize", sgd_minimize)
    monkeypatch.setattr(R, "_ADAM", dict(lr=lr, momentum=momentum, nesterov=nesterov))
    return sgd(lr, momentum=momentum, nesterov=nesterov)


@pytest.mark.parametrize("name", list(SPECS))
@pytest.mark.parametrize("solver", ["min", "fermat"])
def test_sgd_trajectory_matches_the_oracle(solver, name, monkeypatch):
    """The interaction points after 20 SGD steps agree with the oracle's (fp64, same update)."""
    from differt2d_amd.engine import default_context, make_params
    from oracle import ref as R

    spec = _sgd_oracle(monkeypatch, name)
    scene = _ris_scene()
    xys, kind, phi = _scene_tables(scene)
    objs = _oracle_objs(scene)
    cands = [np.array(c, np.int32) for c in ([0], [4], [5], [0, 4], [3, 5])]
    rng = np.random.default_rng(13)
    theta0 = [rng.random(sum(objs[int(i)].parameters_count() for i in c), dtype=F) for c in cands]
    tx = np.array([[0.2, 0.2], [0.31, 0.77]], F)
    rx = np.array([[0.8, 0.6], [0.62, 0.18]], F)
    ctx = default_context()
    ctx.set_scene(xys, kind, phi)
    p = make_params(min_order=0, max_order=4, solver=solver, steps=20, approx=True)
    th = [np.pad(t, (0, 4 - len(t))) for t in theta0]
    try:
        ctx.set_optimizer(spec)
        got = ctx.trace_paths(p, tx, rx, cands, theta0=th)
        ctx.set_optimizer(None)
        adam = ctx.trace_paths(p, tx, rx, cands, theta0=th)
    finally:
        ctx.set_optimizer(None)
    for ci, c in enumerate(cands):
        inter64 = [R.Obj(objs[int(i)].kind, np.asarray(objs[int(i)].xys, np.float64), objs[int(i)].phi) for i in c]
        pts64, loss64 = R.opt_path(solver, tx.astype(np.float64), inter64, rx.astype(np.float64), theta0[ci], 20, R.NUMPY64)
        n = len(c) + 2
        np.testing.assert_allclose(got["xys"][:, ci, :n], np.stack(pts64, axis=1), rtol=0, atol=2e-5, err_msg=f"{name} {c.tolist()}")
        np.testing.assert_allclose(got["loss"][:, ci], np.broadcast_to(loss64, (2,)), rtol=1e-4, atol=1e-6)
    assert np.nanmax(np.abs(got["xys"] - adam["xys"])) > 1e-2  # not Adam's solution


@pytest.mark.parametrize("name", list(SPECS))
@pytest.mark.parametrize("solver", ["min", "fermat"])
def test_sgd_gradients_through_the_solver_match_the_oracle(solver, name, monkeypatch):
    """Per-cell gradient, fixed end point, every object's end points and phi from both gradient kernels (reverse mode over
    the stored trajectory, forward tangents) against reverse-mode autodiff of the oracle through its SGD loop, on the cells
    where the oracle is well conditioned (the cotangent is masked to them on both sides)."""
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import default_context
    from oracle import ref as R

    spec = _sgd_oracle(monkeypatch, name)
    scene, xys, kind, phi, X, Y, cands, theta0 = _opt_case(30, solver, True)
    tx = scene.transmitters["tx"].xy
    cot = (np.random.default_rng(5).random(X.shape) + 0.5).astype(F)
    okw = dict(solver=solver, steps=30, grid_role="rx", approx=True)
    w64 = R.opt_value_and_grads(kind, xys, phi, tx, X, Y, cands, theta0, dtype="float64", cotangent=cot, **okw)
    w32 = R.opt_value_and_grads(kind, xys, phi, tx, X, Y, cands, theta0, dtype="float32", cotangent=cot, **okw)
    stable = _oracle_stable(w64["value"], w32["value"], w64["grad_cell"], w32["grad_cell"])
    assert stable.mean() >= 0.8, f"only {int(stable.sum())} of {stable.size} cells are well conditioned in the oracle"
    cot_m = (cot * stable).astype(F)
    if not stable.all():
        w64 = R.opt_value_and_grads(kind, xys, phi, tx, X, Y, cands, theta0, dtype="float64", cotangent=cot_m, **okw)
        w32 = R.opt_value_and_grads(kind, xys, phi, tx, X, Y, cands, theta0, dtype="float32", cotangent=cot_m, **okw)
    ctx = default_context()
    kw = dict(solver=solver, steps=30, grid_role=L.GRID_RX, min_order=0, max_order=1, approx=True)
    try:
        for grad_mode in (0, 1):
            ctx.set_option("opt_grad_mode", grad_mode)
            ctx.set_optimizer(spec)
            g = _gpu_opt_grads(xys, kind, phi, tx, X, Y, cands, theta0, cot_m, **kw)
            fwd = ctx.power_map(tx, X, Y, **kw)  # the value map of the gradient sweep is the forward sweep's, bit for bit
            assert np.array_equal(g["value"], fwd, equal_nan=True)
            np.testing.assert_allclose(g["value"][stable], w64["value"][stable], rtol=2e-3, atol=2e-3 * np.abs(w64["value"]).max())
            assert np.array_equal(np.isnan(g["grad_rx"]), np.isnan(w32["grad_cell"]))
            _tight(g["grad_rx"][stable], w64["grad_cell"][stable], w32["grad_cell"][stable], f"{name} mode {grad_mode} per-cell gradient")
            _tight(g["tx_bar"], w64["fixed_bar"], w32["fixed_bar"], f"{name} mode {grad_mode} fixed end point")
            _tight(g["walls_bar"], w64["xys_bar"], w32["xys_bar"], f"{name} mode {grad_mode} object end points")
            _tight(g["phi_bar"], w64["phi_bar"], w32["phi_bar"], f"{name} mode {grad_mode} phi")
    finally:
        ctx.set_option("opt_grad_mode", 0)
        ctx.set_optimizer(None)


@pytest.mark.parametrize("name", list(SPECS))
def test_sgd_gradient_on_the_ris_line_matches_the_oracle(name, monkeypatch):
    """Receivers on the RIS's supporting line: the RIS residual is constant in theta there.  Adam's sqrt(nu_hat) turns that
    into NaN gradients (tests/test_gpu_opt.py); SGD has no square root -- whatever the oracle's fp32 chain says there (NaN
    positions) and its fp64 chain (values), the GPU says too."""
    from differt2d_amd.engine import default_context
    from oracle import ref as R

    spec = _sgd_oracle(monkeypatch, name)
    scene, xys, kind, phi, X, Y, cands, theta0 = _opt_case(30, "min", True, grid=(7, 5))
    line = X == F(0.5)
    assert line.sum() == X.shape[0]
    tx = scene.transmitters["tx"].xy
    okw = dict(solver="min", steps=30, approx=True)
    w64 = R.opt_value_and_grads(kind, xys, phi, tx, X, Y, cands, theta0, dtype="float64", **okw)
    w32 = R.opt_value_and_grads(kind, xys, phi, tx, X, Y, cands, theta0, dtype="float32", **okw)
    ctx = default_context()
    try:
        ctx.set_optimizer(spec)
        got = _gpu_opt_grads(xys, kind, phi, tx, X, Y, cands, theta0, None, min_order=0, max_order=1, **okw)
    finally:
        ctx.set_optimizer(None)
    assert np.isfinite(got["value"]).all()
    assert np.array_equal(np.isnan(got["grad_rx"][line]), np.isnan(w32["grad_cell"][line]))
    _tight(got["grad_rx"][line], w64["grad_cell"][line], w32["grad_cell"][line], f"{name} per-cell gradient on the RIS line")
    print(f"{name}: {int(np.isfinite(got['grad_rx'][line]).all(-1).sum())} of {int(line.sum())} cells on the RIS line have a finite gradient")


def test_sgd_through_the_scene_api():
    """`path_cls_kwargs=dict(optimizer=sgd(...))`: each SGD variant gives its own map, none of them Adam's, and asking for no
    optimiser afterwards gives Adam's map back bit for bit."""
    from differt2d_amd.geometry import MinPath
    from differt2d_amd.optimize import sgd
    from differt2d_amd.utils import received_power

    scene = _ris_scene()
    x = np.linspace(0.05, 0.95, 12).astype(F)
    X, Y = np.meshgrid(x, x)
    cands = scene.all_path_candidates(min_order=1, max_order=1)
    rng = np.random.default_rng(2)
    theta0 = [rng.random(sum(o.parameters_count() for o in scene.get_interacting_objects(c)), dtype=F) for c in cands]
    kw = dict(fun=received_power, path_cls=MinPath, min_order=1, max_order=1, approx=True, reduce_all=True)

    def run(**o):
        return scene.accumulate_on_receivers_grid_over_paths(X, Y, path_cls_kwargs=dict(steps=40, theta0=theta0, **o), **kw)

    adam = run()
    maps = [run(optimizer=sgd(*SPECS[n][:2], nesterov=SPECS[n][2])) for n in SPECS]
    back = run()
    assert np.array_equal(back, adam, equal_nan=True)
    for i, m in enumerate(maps):
        assert np.isfinite(m).all() and not np.array_equal(m, adam, equal_nan=True)
        for j in range(i):
            assert not np.array_equal(m, maps[j], equal_nan=True)


def test_sgd_optimizer_kinds_are_validated():
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import default_context

    ctx = default_context()
    lib, c = ctx._lib, ctx._ctx
    try:
        L.check(lib.d2d_set_optimizer(c, L.D2D_OPT_SGD, 0.1, 0.0, 0.0, 0.0))
        L.check(lib.d2d_set_optimizer(c, L.D2D_OPT_SGD_MOMENTUM, 0.1, 0.0, 0.0, 0.0))
        L.check(lib.d2d_set_optimizer(c, L.D2D_OPT_SGD_MOMENTUM, 0.1, 0.9, 1.0, 0.0))
        for args in ((L.D2D_OPT_SGD, float("nan"), 0.0, 0.0, 0.0), (L.D2D_OPT_SGD_MOMENTUM, float("inf"), 0.5, 0.0, 0.0),
                     (L.D2D_OPT_SGD_MOMENTUM, 0.1, 1.0, 0.0, 0.0), (L.D2D_OPT_SGD_MOMENTUM, 0.1, -0.1, 0.0, 0.0),
                     (L.D2D_OPT_SGD_MOMENTUM, 0.1, float("nan"), 0.0, 0.0), (L.D2D_OPT_SGD_MOMENTUM, 0.1, 0.5, 0.5, 0.0),
                     (L.D2D_OPT_SGD_MOMENTUM, 0.1, 0.5, 2.0, 0.0)):
            with pytest.raises(L.D2DError):
                L.check(lib.d2d_set_optimizer(c, *args))
        with pytest.raises(L.D2DUnsupported):
            L.check(lib.d2d_set_optimizer(c, 3, 0.1, 0.0, 0.0, 0.0))
        with pytest.raises(L.D2DUnsupported):
            ctx.set_optimizer("sgd")
        with pytest.raises(L.D2DUnsupported):
            ctx.set_optimizer(object())
    finally:
        ctx.set_optimizer(None)
