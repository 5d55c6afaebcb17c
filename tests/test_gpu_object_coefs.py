"""
GPU: ``received_power_per_object`` (D2D_FUN_RECEIVED_POWER_PER_OBJECT) -- one reflection coefficient per wall, fused.

    num = 1;  for o in interacting_objects (candidate order):  num = num * coef[o]      (fp32, left fold)
    f   = num / (h * h + r * r)

The oracle is the loop of ``tests/object_coefs_oracle.py`` over ``oracle/ref.py``'s public pieces (pinned on the CPU by
``tests/test_object_coefs_cpu.py``), run under ``LibmBackend``: NumpyBackend with the C library's expf, the one operation in which
NumPy's fp32 arithmetic is not the C oracle's and the device's.  Bars are the project's own: hard and hard_sigmoid maps bit for bit, sigmoid maps within
rtol 1e-6 / atol 1e-9 and bit-equal in >= 99.9 % of the cells (tests/test_gpu_forward.py); per-cell gradients with torch's fp32
NaN positions and within max(1e-5 * scale, 2 |fp32 - fp64|) of torch's fp64 run (tests/test_gpu_api.py); the scene VJP -- and the
coefficient block, which is reduced the same way: fp32 per-patch partial rows, then the fixed-order fp64 sum -- within rtol 2e-5,
atol 2e-5 * max|.| (tests/test_gpu_api.py).
"""

import dataclasses
import functools

import numpy as np
import pytest

from conftest import random_scene, unit_grid
from object_coefs_oracle import LibmBackend, coef_map, coef_value_and_grads

pytestmark = pytest.mark.gpu

F = np.float32
MODES = [(False, "hard_sigmoid"), (True, "hard_sigmoid"), (True, "sigmoid")]
MODE_IDS = ["hard", "hsig", "sig"]
FUN = "received_power_per_object"
# the oracle loop's NumPy backend with libm's expf for the sigmoid (NumPy's own fp32 exp is a SIMD routine an ulp off libm's in a
# third of the arguments: allclose holds, bit equality cannot; hard and hard_sigmoid validity never call exp)
LIBM = LibmBackend()

# every forward launch shape the library has: the two fixtures of tests/test_gpu_forward.py, the default of
# tests/test_gpu_coop.py (patches shared candidate by candidate), and the enumerating kernels (no region lists)
SHAPES = {
    "shared_patches": dict(coop_waves=0, split_max_tiles=8192, split_sigmoid=1),
    "one_wave_per_patch_scheduled": dict(split_max_tiles=0, sched_min_tiles=1),
    "coop_default": dict(),
    "no_region_lists": dict(region_lists=0),
    "no_region_lists_one_wave": dict(region_lists=0, split_max_tiles=0, sched_min_tiles=1),
}


@pytest.fixture(scope="module", params=list(SHAPES))
def shaped(request):
    from differt2d_amd.engine import Context

    with Context(0) as c:
        for k, v in SHAPES[request.param].items():
            c.set_option(k, v)
        yield c


@pytest.fixture(scope="module")
def ctx():
    from differt2d_amd.engine import Context

    with Context(0) as c:
        yield c


def _role(role):
    from differt2d_amd import _lib as L

    return L.GRID_TX if role == "tx" else L.GRID_RX


def _coefs(n, seed):
    return (0.2 + 0.7 * np.random.default_rng(seed).random(n)).astype(F)


def _same(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


def _compare(got, want, function):
    assert got.shape == want.shape and got.dtype == np.float32
    if function == "sigmoid":
        np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-9)
        assert _same(got, want).mean() >= 0.999, f"{int((~_same(got, want)).sum())} of {got.size} cells differ in some bit"
    else:
        bad = ~_same(got, want)
        assert not bad.any(), f"{bad.sum()} of {bad.size} cells differ; max abs {np.nanmax(np.abs(got - want))}"


# ---- 1. forward against the oracle loop --------------------------------------------------------------------------------------
# (scene, seed, grid, candidate mask, (min_order, max_order))
FWD_CASES = {
    "12w_o0-2": (12, 11, (37, 29), None, (0, 2)),  # the ragged grid of tests/test_gpu_forward.py: walls 2, 5, 10 reach 236 / 132 / 187 cells
    "8w_masked_o1-2": (8, 21, (24, 24), [1, 0, 1, 1, 0, 1, 1, 1], (1, 2)),
    "6w_o3": (6, 5, (16, 9), None, (3, 3)),
    "6w_o0-3": (6, 5, (16, 9), None, (0, 3)),
    "6w_o4": (6, 5, (16, 9), None, (4, 4)),
}


@functools.lru_cache(maxsize=None)
def _fwd_oracle(case, role, approx, function, height):
    n, seed, (gx, gy), mask, (lo, hi) = FWD_CASES[case]
    fixed, walls = random_scene(n, seed=seed)
    X, Y = unit_grid(gx, gy)
    off = None if mask is None else {j for j, a in enumerate(mask) if not a}
    want = coef_map(walls, _coefs(n, seed + 1000), fixed, X, Y, min_order=lo, max_order=hi, height=height, approx=approx,
                    function=function, grid_role=role, filter_nodes=off, xp=LIBM)
    want.setflags(write=False)
    return want


@pytest.mark.parametrize("case", list(FWD_CASES))
@pytest.mark.parametrize("height", [0.1, 0.25])
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("approx,function", MODES, ids=MODE_IDS)
def test_forward_against_the_oracle_loop(shaped, case, height, role, approx, function):
    n, seed, (gx, gy), mask, (lo, hi) = FWD_CASES[case]
    fixed, walls = random_scene(n, seed=seed)
    X, Y = unit_grid(gx, gy)
    shaped.set_scene(walls)
    shaped.set_reflection_coefs(_coefs(n, seed + 1000))
    if mask is not None:
        shaped.set_candidate_mask(mask)
    got = shaped.power_map(fixed, X, Y, min_order=lo, max_order=hi, approx=approx, function=function, fun=FUN, height=height,
                           grid_role=_role(role))
    want = _fwd_oracle(case, role, approx, function, height)
    assert np.count_nonzero(want) > 0 or (lo == 3 and not approx)  # (no valid order-3 path under hard validity in this scene)
    _compare(got, want, function)


# ---- 2. uniform coefficients are received_power, bit for bit ------------------------------------------------------------------
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("approx,function", MODES, ids=MODE_IDS)
def test_uniform_coefficients_equal_received_power(ctx, role, approx, function):
    """Orders 0..3 (there the left fold and lax.integer_pow's square-and-multiply coincide): only the numerator's source differs,
    so the maps AND the per-cell gradients of the value+grad sweep are the same bits, NaN positions included."""
    from differt2d_amd.engine import make_params

    fixed, walls = random_scene(6, seed=5)
    X, Y = unit_grid(16, 9)
    ctx.set_scene(walls)
    ctx.set_reflection_coefs(np.full(6, 0.35, F))
    ctx.set_grid(X, Y)
    ctx.set_cotangent(None)
    kw = dict(min_order=0, max_order=3, approx=approx, function=function, height=0.25, grid_role=_role(role))
    out = {}
    for fun in ("received_power", FUN):
        ctx.launch(make_params(fun=fun, r_coef=0.35, **kw), fixed)
        value = ctx.get_map()
        ctx.launch_vg(make_params(fun=fun, r_coef=0.35, **kw), fixed, scene_vjp=True)
        out[fun] = (value, ctx.get_map(), ctx.get_grad_rx(), *ctx.get_scene_vjp())
    for a, b in zip(out["received_power"], out[FUN]):
        assert np.array_equal(a, b, equal_nan=True)
    assert np.count_nonzero(out[FUN][0]) > 0 and np.count_nonzero(np.nan_to_num(out[FUN][2])) > 0


# ---- 3. coefficients in {0, c}: the zeroed walls drop out of the candidates ------------------------------------------------------
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("approx,function", MODES[:2], ids=MODE_IDS[:2])
def test_zeroed_walls_equal_received_power_without_them(ctx, role, approx, function):
    """The mapping object index -> coefficient, independently of the oracle loop: walls 2 and 10 at zero contribute +0 to every
    cell, which is what masking them out of the candidates does.  Values only: a zero-coefficient candidate still runs into the
    reverse-mode NaN rules, a masked one is never enumerated."""
    fixed, walls = random_scene(12, seed=11)
    X, Y = unit_grid(37, 29)
    coef = np.full(12, 0.6, F)
    coef[[2, 10]] = 0.0
    kw = dict(min_order=0, max_order=2, approx=approx, function=function, grid_role=_role(role))
    ctx.set_scene(walls)
    ctx.set_reflection_coefs(coef)
    got = ctx.power_map(fixed, X, Y, fun=FUN, **kw)
    full = ctx.power_map(fixed, X, Y, fun="received_power", r_coef=0.6, **kw)
    ctx.set_candidate_mask([0 if j in (2, 10) else 1 for j in range(12)])
    want = ctx.power_map(fixed, X, Y, fun="received_power", r_coef=0.6, **kw)
    ctx.set_candidate_mask(None)
    assert np.array_equal(got, want, equal_nan=True)
    assert not np.array_equal(full, want, equal_nan=True)


# ---- 4. value+grad and the VJP against torch autodiff of the oracle loop ------------------------------------------------------
def _vg(c, walls, coef, fixed, X, Y, cot, **kw):
    from differt2d_amd.engine import make_params

    c.set_scene(walls)
    c.set_reflection_coefs(coef)
    c.set_grid(X, Y)
    c.set_cotangent(cot)
    c.launch_vg(make_params(fun=FUN, **kw), fixed, scene_vjp=True)
    tx_bar, walls_bar = c.get_scene_vjp()
    return {"value": c.get_map(), "grad_rx": c.get_grad_rx(), "tx_bar": tx_bar, "walls_bar": walls_bar,
            "coef_bar": c.get_reflection_coefs_vjp()}


def _vjp_inputs():
    fixed, walls = random_scene(7, seed=77)
    X, Y = unit_grid(21, 13)
    rng = np.random.default_rng(770)
    return fixed, walls, X, Y, _coefs(7, 771), rng.standard_normal(X.shape).astype(F)


@functools.lru_cache(maxsize=None)
def _vjp_oracle(role, approx, function, dtype):
    fixed, walls, X, Y, coef, cot = _vjp_inputs()
    return coef_value_and_grads(walls, coef, fixed, X, Y, cotangent=cot, dtype=dtype, min_order=0, max_order=2, approx=approx,
                                function=function, grid_role=role)


@functools.lru_cache(maxsize=None)
def _vjp_value(role, approx, function):
    fixed, walls, X, Y, coef, _ = _vjp_inputs()
    return coef_map(walls, coef, fixed, X, Y, min_order=0, max_order=2, approx=approx, function=function, grid_role=role, xp=LIBM)


def _check_against_autodiff(got, want64, want32, tag):
    assert np.array_equal(np.isnan(got["grad_rx"]), np.isnan(want32["grad_rx"])), f"{tag}: NaN positions of grad_rx"
    scale = float(np.nanmax(np.abs(want64["grad_rx"])))
    err = np.abs(got["grad_rx"] - want64["grad_rx"])
    bar = np.maximum(1e-5 * scale, 2.0 * np.abs(want32["grad_rx"] - want64["grad_rx"]))
    if np.isfinite(err).any():
        assert np.nanmax(err - bar) <= 0.0, f"{tag}: grad_rx max err {np.nanmax(err):.3e} at scale {scale:.3e}"
    for k in ("tx_bar", "walls_bar", "coef_bar"):
        w = want64[k]
        fin = np.isfinite(w)
        top = float(np.abs(w[fin]).max()) if fin.any() else 0.0
        with np.errstate(invalid="ignore"):
            print(f"{tag}: {k} max |got - fp64| = {np.nanmax(np.abs(got[k] - w)) if fin.any() else 0.0:.3e} at max |.| = {top:.3e}")
        np.testing.assert_allclose(got[k], w, rtol=2e-5, atol=2e-5 * top, err_msg=f"{tag}: {k}")


@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("approx,function", MODES, ids=MODE_IDS)
def test_value_grad_and_vjp_against_autodiff_of_the_oracle_loop(ctx, role, approx, function):
    fixed, walls, X, Y, coef, cot = _vjp_inputs()
    want64, want32 = _vjp_oracle(role, approx, function, "float64"), _vjp_oracle(role, approx, function, "float32")
    kw = dict(min_order=0, max_order=2, approx=approx, function=function, grid_role=_role(role))
    runs = {}
    for strict in (False, True):
        got = _vg(ctx, walls, coef, fixed, X, Y, cot, strict_nan=strict, **kw)
        tag = f"{role} {function if approx else 'hard'} {'strict' if strict else 'culled'}"
        _compare(got["value"], _vjp_value(role, approx, function), function)
        _check_against_autodiff(got, want64, want32, tag)
        assert np.isfinite(got["coef_bar"]).all() and np.count_nonzero(got["coef_bar"]) >= 3, got["coef_bar"]
        again = _vg(ctx, walls, coef, fixed, X, Y, cot, strict_nan=strict, **kw)
        for k in got:  # reproducible run to run, the coefficient block like the rest of the VJP
            assert np.array_equal(got[k], again[k], equal_nan=True), f"{tag}: {k} differs between two launches"
        runs[strict] = got
    # the culled sweep (with its NaN scan) and the exhaustive kernel agree
    a, b = runs[False], runs[True]
    assert np.array_equal(a["value"], b["value"], equal_nan=True)
    for k in ("grad_rx", "tx_bar", "walls_bar", "coef_bar"):
        assert np.array_equal(np.isnan(a[k]), np.isnan(b[k])), f"NaN positions of {k} differ"
        fin = ~np.isnan(b[k])
        if k == "grad_rx":
            assert np.array_equal(a[k][fin], b[k][fin])
        elif fin.any():
            np.testing.assert_allclose(a[k][fin], b[k][fin], rtol=1e-5, atol=1e-6 * float(np.abs(b[k][fin]).max()), err_msg=k)


def test_coefficient_vjp_accumulates_over_out_add_launches(ctx):
    """D2D_OUT_ADD adds the coefficient block as it adds tx_bar / xys_bar; a sweep with another function adds nothing to it."""
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import make_params

    fixed, walls, X, Y, coef, cot = _vjp_inputs()
    kw = dict(min_order=0, max_order=2, approx=True)
    one = _vg(ctx, walls, coef, fixed, X, Y, cot, **kw)
    other = fixed[::-1].copy()
    two = _vg(ctx, walls, coef, other, X, Y, cot, **kw)
    _vg(ctx, walls, coef, fixed, X, Y, cot, **kw)
    ctx.launch_vg(make_params(fun=FUN, out_mode=L.OUT_ADD, **kw), other, scene_vjp=True)
    both = ctx.get_reflection_coefs_vjp()
    want = one["coef_bar"].astype(np.float64) + two["coef_bar"]
    np.testing.assert_allclose(both, want, rtol=1e-6, atol=1e-6 * float(np.abs(want).max()))
    assert np.count_nonzero(both) >= 3
    ctx.launch_vg(make_params(fun="received_power", out_mode=L.OUT_ADD, **kw), other, scene_vjp=True)
    assert np.array_equal(ctx.get_reflection_coefs_vjp(), both)


# ---- 5. NaN cells do not reach the coefficients -----------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [False, True], ids=["culled", "strict"])
def test_nan_cells_do_not_reach_the_coefficients(ctx, strict):
    """The reference's reverse-mode NaN traps sit between the path points and the geometry; the coefficients are not on that way:
    with 18 of 20 cells' grad_rx NaN (and every wall's adjoint), torch's coefficient gradient is finite -- and so is ours."""
    from oracle import ref as R

    walls, fixed = R.square_scene_with_wall_walls(), np.array([0.2, 0.5], F)
    X, Y = np.meshgrid(np.array([0.0, 0.2, 0.5, 1.0], F), np.array([0.0, 0.2, 0.5, 0.8, 1.0], F))
    coef = _coefs(5, 55)
    kw = dict(min_order=0, max_order=2, approx=True, function="hard_sigmoid")
    want64 = coef_value_and_grads(walls, coef, fixed, X, Y, dtype="float64", **kw)
    want32 = coef_value_and_grads(walls, coef, fixed, X, Y, dtype="float32", **kw)
    got = _vg(ctx, walls, coef, fixed, X, Y, None, strict_nan=strict, **kw)
    nan_cells = np.isnan(want32["grad_rx"]).any(axis=-1)
    assert int(nan_cells.sum()) == 18 and np.isnan(want32["walls_bar"]).all()
    assert np.array_equal(np.isnan(got["grad_rx"]), np.isnan(want32["grad_rx"]))
    assert np.isfinite(want32["coef_bar"]).all() and np.count_nonzero(want32["coef_bar"]) > 0
    assert np.isfinite(got["coef_bar"]).all()
    top = float(np.abs(want64["coef_bar"]).max())
    print(f"coef_bar max |got - fp64| = {np.abs(got['coef_bar'] - want64['coef_bar']).max():.3e} at max |.| = {top:.3e}")
    np.testing.assert_allclose(got["coef_bar"], want64["coef_bar"], rtol=2e-5, atol=2e-5 * top)


# ---- 6. the mirror ---------------------------------------------------------------------------------------------------------------------
def _coated_scene(n_receivers=0):
    from differt2d_amd.geometry import Point, Wall
    from differt2d_amd.scene import Scene

    @dataclasses.dataclass(frozen=True, eq=False)
    class CoatedWall(Wall):
        r_coef: float = 0.5

    tx, walls = random_scene(7, seed=77)
    coef = _coefs(7, 771)
    # walls 1 and 4 are plain Walls: they take the keyword's value
    objects = [Wall(xys=w) if j in (1, 4) else CoatedWall(xys=w, r_coef=float(coef[j])) for j, w in enumerate(walls)]
    scene = Scene(objects=objects).with_transmitters(tx=Point(xy=tx), tx2=Point(xy=tx[::-1].copy()))
    rng = np.random.default_rng(5)
    rx = {f"rx_{i}": Point(xy=rng.random(2).astype(F)) for i in range(max(n_receivers, 1))}
    coef[[1, 4]] = 0.45
    return scene.with_receivers(**rx), walls, coef


def _host_route(transmitter, receiver, path, interacting_objects, r_coef=0.5, height=0.1):
    from differt2d_amd.utils import received_power_per_object

    return received_power_per_object(transmitter, receiver, path, interacting_objects, r_coef=r_coef, height=height)


_host_route._d2d_native = False  # the dense host route: GPU trace, this function on the host


def _close_values(fused, host):
    assert np.array_equal(np.asarray(host) == 0, np.asarray(fused) == 0)
    np.testing.assert_allclose(host, fused, rtol=2e-6, atol=1e-9)


def _close_grads(fused, host):
    assert np.array_equal(np.isnan(fused), np.isnan(host))
    np.testing.assert_allclose(np.nan_to_num(fused), np.nan_to_num(host), rtol=0, atol=1e-5 * float(np.nanmax(np.abs(host))))


@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("approx", [False, True], ids=["hard", "hsig"])
def test_mirror_grid_sweeps_against_the_host_route(role, approx):
    from differt2d_amd.utils import received_power_per_object

    scene, walls, coef = _coated_scene(2)
    X, Y = unit_grid(21, 13)
    sweep = scene.accumulate_on_receivers_grid_over_paths if role == "rx" else scene.accumulate_on_transmitters_grid_over_paths
    kw = dict(fun_kwargs=dict(r_coef=0.45, height=0.25), min_order=0, max_order=2, approx=approx)
    fused = sweep(X, Y, fun=received_power_per_object, reduce_all=True, **kw)
    _close_values(fused, sweep(X, Y, fun=_host_route, reduce_all=True, **kw))
    assert np.count_nonzero(fused) > 0
    # the keyword reaches the objects without the attribute: another value, another map
    other = sweep(X, Y, fun=received_power_per_object, reduce_all=True, **{**kw, "fun_kwargs": dict(r_coef=0.9, height=0.25)})
    assert not np.array_equal(other, fused)
    per_fused = dict(sweep(X, Y, fun=received_power_per_object, **kw))
    per_host = dict(sweep(X, Y, fun=_host_route, **kw))
    assert list(per_fused) == list(per_host) and len(per_fused) == 2
    for k in per_fused:
        _close_values(per_fused[k], per_host[k])
    Zf, Gf = sweep(X, Y, fun=received_power_per_object, reduce_all=True, value_and_grad=True, **kw)
    Zh, Gh = sweep(X, Y, fun=_host_route, reduce_all=True, value_and_grad=True, **kw)
    assert np.array_equal(Zf, fused)
    _close_values(Zf, Zh)
    _close_grads(Gf, Gh)


def test_mirror_pairwise_and_vjps():
    from differt2d_amd.utils import received_power, received_power_per_object

    scene, walls, coef = _coated_scene(3)
    kw = dict(fun_kwargs=dict(r_coef=0.45), min_order=0, max_order=2, approx=True)
    fused = {(a, b): v for a, b, v in scene.accumulate_over_paths(received_power_per_object, **kw)}
    host = {(a, b): v for a, b, v in scene.accumulate_over_paths(_host_route, **kw)}
    assert list(fused) == list(host) and len(fused) == 6
    _close_values([fused[k] for k in fused], [host[k] for k in fused])

    # pairwise VJP against torch autodiff of the oracle loop (receivers as a 1 x R grid, default cotangent = ones)
    values, vjp = scene.accumulate_over_paths_value_and_vjp(received_power_per_object, **kw)
    assert all(values[k] == fused[k] for k in fused)
    rx = np.stack([r.xy for r in scene.receivers.values()])
    want = np.zeros(7)
    for t in scene.transmitters.values():
        o = coef_value_and_grads(walls, coef, t.xy, rx[None, :, 0], rx[None, :, 1], dtype="float64", min_order=0, max_order=2, approx=True)
        want = want + o["coef_bar"]
    assert vjp["r_coefs"].shape == (7,) and np.count_nonzero(vjp["r_coefs"]) >= 3
    np.testing.assert_allclose(vjp["r_coefs"], want, rtol=2e-5, atol=2e-5 * float(np.abs(want).max()))
    _, plain = scene.accumulate_over_paths_value_and_vjp(received_power, min_order=0, max_order=2, approx=True)
    assert sorted(plain) == ["objects", "phi", "receivers", "transmitters"]  # the other functions keep their keys

    # grid VJP
    X, Y = unit_grid(21, 13)
    cot = np.random.default_rng(770).standard_normal(X.shape).astype(F)
    outs = dict(scene.receivers_grid_value_and_vjp(X, Y, received_power_per_object, fun_kwargs=dict(r_coef=0.45), cotangent=cot,
                                                   min_order=0, max_order=2, approx=True))
    for name, t in scene.transmitters.items():
        o = coef_value_and_grads(walls, coef, t.xy, X, Y, cotangent=cot, dtype="float64", min_order=0, max_order=2, approx=True)
        got = outs[name]["r_coef_bar"]
        np.testing.assert_allclose(got, o["coef_bar"], rtol=2e-5, atol=2e-5 * float(np.abs(o["coef_bar"]).max()))
        np.testing.assert_allclose(outs[name]["objects_bar"], o["walls_bar"], rtol=2e-5, atol=2e-5 * float(np.abs(o["walls_bar"]).max()))
    plain = dict(scene.receivers_grid_value_and_vjp(X, Y, received_power, min_order=0, max_order=1))
    assert sorted(plain["tx"]) == ["grad_rx", "objects_bar", "phi_bar", "tx_bar", "value"]


# ---- 7. loud edges ---------------------------------------------------------------------------------------------------------------------
def test_loud_edges(ctx):
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import make_params
    from differt2d_amd.geometry import MinPath, Point
    from differt2d_amd.scene import Scene
    from differt2d_amd.utils import received_power_per_object

    fixed, walls = random_scene(6, seed=5)
    _, walls_b = random_scene(6, seed=6)
    X, Y = unit_grid(16, 9)
    coef = _coefs(6, 1)
    p = make_params(fun=FUN, max_order=2)

    def status(call):
        with pytest.raises(L.D2DError) as e:
            call()
        return e.value.status

    ctx.set_scene(walls_b)
    ctx.set_scene(walls)  # (a new scene: nothing set)
    ctx.set_grid(X, Y)
    assert status(lambda: ctx.launch(p, fixed)) == -5  # D2D_ERR_STATE: no coefficients
    assert status(lambda: ctx.launch_vg(p, fixed, scene_vjp=True)) == -5
    assert status(lambda: ctx.set_reflection_coefs(coef[:5])) == -1  # D2D_ERR_INVALID: wrong n
    bad = coef.copy()
    bad[3] = np.nan
    assert status(lambda: ctx.set_reflection_coefs(bad)) == -1
    bad[3] = np.inf
    assert status(lambda: ctx.set_reflection_coefs(bad)) == -1
    assert status(lambda: ctx.get_reflection_coefs_vjp()) == -5  # no scene-VJP sweep yet
    neg = coef.copy()
    neg[2] = -0.5  # negative values are allowed
    ctx.set_reflection_coefs(neg)
    ctx.set_reflection_coefs(coef)
    ctx.launch(p, fixed)
    first = ctx.get_map()
    with pytest.raises(L.D2DUnsupported, match="received_power_per_object"):
        ctx.launch(make_params(fun=FUN, max_order=1, solver="min"), fixed)
    with pytest.raises(L.D2DUnsupported, match="received_power_per_object"):
        ctx.launch_stats(p, fixed)
    ctx.set_scene(walls)  # the resident scene again: the coefficients stay
    ctx.launch(p, fixed)
    assert np.array_equal(ctx.get_map(), first)
    ctx.set_reflection_coefs(None)  # dropped
    assert status(lambda: ctx.launch(p, fixed)) == -5
    ctx.set_reflection_coefs(coef)
    ctx.set_scene(walls_b)  # another scene drops them
    assert status(lambda: ctx.launch(p, fixed)) == -5
    ctx.set_scene(walls)
    ctx.set_cotangent(None)
    ctx.launch_vg(make_params(fun="received_power", max_order=2), fixed, scene_vjp=True)
    assert np.array_equal(ctx.get_reflection_coefs_vjp(), np.zeros(6, F))  # zeros after a sweep with another function

    scene = Scene.from_walls_array(walls).with_transmitters(tx=Point(xy=fixed))
    with pytest.raises(L.D2DUnsupported, match="received_power_per_object"):
        scene.accumulate_on_receivers_grid_over_paths(X, Y, fun=received_power_per_object, reduce_all=True, path_cls=MinPath,
                                                      key=np.random.default_rng(0))


# ---- 8. one full-size case -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("approx", [False, True], ids=["hard", "hsig"])
def test_cfg2_full_size(ctx, approx):
    """BASELINE.json configs[1]: 50 walls, seed 1234, 1024 x 1024 cells, orders 0..2."""
    tx, walls = random_scene(50, seed=1234)
    x = np.linspace(0.0, 1.0, 1024).astype(F)
    X, Y = np.meshgrid(x, x)
    kw = dict(min_order=0, max_order=2, approx=approx)
    ctx.set_scene(walls)
    want = ctx.power_map(tx, X, Y, fun="received_power", r_coef=0.5, **kw)
    ctx.set_reflection_coefs(np.full(50, 0.5, F))
    assert np.array_equal(ctx.power_map(tx, X, Y, fun=FUN, **kw), want)
    ctx.set_reflection_coefs(_coefs(50, 50))
    got = ctx.power_map(tx, X, Y, fun=FUN, **kw)
    assert np.array_equal(got == 0, want == 0) and not np.array_equal(got, want)
