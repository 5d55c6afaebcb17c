"""The per-cell power-delay profile (include/d2d.h: d2d_power_profile_launch; power_sink_kernel, BinSink): the fused sweep's contributions
binned by path length.  Held bit for bit to the oracle recipe of ``tests/power_profile_oracle.py`` (which
``tests/test_power_profile_cpu.py`` pins to ``R.power_map``), to the consequences of the definition against the fused sweep itself,
and to its state rules and refusals."""

import functools

import numpy as np
import pytest

from conftest import random_scene, unit_grid
from power_profile_oracle import profile_map

pytestmark = pytest.mark.gpu

F = np.float32
MODES = {"hard": dict(approx=False), "hsig": dict(approx=True, function="hard_sigmoid")}
# nbins -> the range it is taken over: one covering bin; bins that the longest paths overshoot; more bins than a patch has cells
RANGES = {1: (0.0, 8.0), 24: (0.0, 3.0), 257: (0.0, 4.5)}
# (of the 7-wall scene's walls only 2, 3 and 6 carry single reflections: the negative and the zero coefficient sit on two of them)
COEF7 = np.array([0.3, 0.4, -0.7, 0.6, 0.7, 0.5, 0.0], F)


@pytest.fixture(scope="module")
def ctx():
    from differt2d_amd.engine import Context

    with Context(0) as c:
        yield c


def _role_id(role):
    from differt2d_amd import _lib as L

    return L.GRID_RX if role == "rx" else L.GRID_TX


@functools.lru_cache(maxsize=None)
def _case(scene):
    """(walls, fixed end point, X, Y)"""
    from oracle import ref as R

    if scene == "random7":  # 21 x 13: partial patches on both sides, 3 x 2 patches
        fixed, walls = random_scene(7, seed=77)
        return walls, fixed, *unit_grid(21, 13)
    if scene == "obstacle":
        return R.square_scene_with_obstacle_walls(), np.array([0.2, 0.2], F), *unit_grid(16, 9)
    if scene == "square4":  # order 3: the MAXK = 3 instance
        return R.square_scene_walls(), np.array([0.3, 0.4], F), *unit_grid(9, 9)
    raise KeyError(scene)


@functools.lru_cache(maxsize=None)
def _oracle(scene, mode, role, fun, nbins, rng, lo=0, hi=2, masked=()):
    walls, fixed, X, Y = _case(scene)
    kw = dict(min_order=lo, max_order=hi, grid_role=role, filter_nodes=set(masked) or None, **MODES[mode])
    if fun == "received_power_per_object":
        kw.update(coef=COEF7, fun_kwargs=dict(height=0.25))
    out = profile_map(walls, fixed, X, Y, rng[0], rng[1], nbins, fun=fun, **kw)
    out.setflags(write=False)
    return out


def _gpu(ctx, scene, mode, role, fun, nbins, rng, lo=0, hi=2, **extra):
    from differt2d_amd.engine import make_params

    walls, fixed, X, Y = _case(scene)
    ctx.set_scene(walls)
    if fun == "received_power_per_object":
        ctx.set_reflection_coefs(COEF7)
        extra["height"] = 0.25
    ctx.set_grid(X, Y)
    params = make_params(min_order=lo, max_order=hi, fun=fun, grid_role=_role_id(role), **MODES[mode], **extra)
    return ctx.power_profile(params, fixed, rng[0], rng[1], nbins), params


def _same_bits(got, want):
    assert got.dtype == np.float32 and got.shape == want.shape
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), f"{bad.sum()} of {bad.size} entries differ, first at {tuple(np.argwhere(bad)[0])}"


# ---- 1. bit for bit against the oracle recipe ---------------------------------------------------------------------------------
@pytest.mark.parametrize("nbins", [1, 24, 257])
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
@pytest.mark.parametrize("scene", ["random7", "obstacle"])
def test_profile_equals_the_oracle_recipe(ctx, scene, mode, role, nbins):
    got, _ = _gpu(ctx, scene, mode, role, "received_power", nbins, RANGES[nbins])
    want = _oracle(scene, mode, role, "received_power", nbins, RANGES[nbins])
    _same_bits(got, want)
    occupied = np.count_nonzero(want.reshape(nbins, -1).any(axis=1))
    print(f"{scene} {mode} {role} {nbins} bins: {occupied} occupied, {np.count_nonzero(want)} non-zero entries")
    assert occupied >= min(nbins, 12)


@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
@pytest.mark.parametrize("fun", ["one", "received_power_per_object"])
def test_profile_of_the_other_fused_functions(ctx, fun, mode, role):
    """``one``: the profile counts valid paths per bin.  The per-object function: a zero coefficient (exact zeros that are
    skipped) and a negative one (contributions of either sign in one bin)."""
    got, _ = _gpu(ctx, "random7", mode, role, fun, 24, RANGES[24])
    want = _oracle("random7", mode, role, fun, 24, RANGES[24])
    _same_bits(got, want)
    if fun == "received_power_per_object":
        assert (want < 0).any() and (want > 0).any()
    elif mode == "hard":
        assert np.array_equal(want, np.round(want)) and want.max() >= 2
    ctx.set_reflection_coefs(None)


@pytest.mark.parametrize("mode,role", [("hard", "rx"), ("hsig", "tx")])
def test_profile_order_3(ctx, mode, role):
    got, _ = _gpu(ctx, "square4", mode, role, "received_power", 24, (0.0, 5.0), 0, 3)
    want = _oracle("square4", mode, role, "received_power", 24, (0.0, 5.0), 0, 3)
    _same_bits(got, want)
    assert np.count_nonzero(want.reshape(24, -1).any(axis=1)) >= 12


@pytest.mark.parametrize("role", ["rx", "tx"])
def test_profile_honours_the_candidate_mask(ctx, role):
    walls, fixed, X, Y = _case("random7")
    allowed = np.ones(7, np.uint8)
    allowed[[2, 5]] = 0
    ctx.set_scene(walls)
    ctx.set_candidate_mask(allowed)
    try:
        from differt2d_amd.engine import make_params

        ctx.set_grid(X, Y)
        got = ctx.power_profile(make_params(min_order=0, max_order=2, grid_role=_role_id(role)), fixed, 0.0, 3.0, 24)
    finally:
        ctx.set_candidate_mask(None)
    _same_bits(got, _oracle("random7", "hard", role, "received_power", 24, (0.0, 3.0), 0, 2, (2, 5)))
    assert not np.array_equal(got, _oracle("random7", "hard", role, "received_power", 24, (0.0, 3.0)))


@pytest.mark.parametrize("mode", ["hard", "hsig"])
def test_a_range_that_cuts_off_both_ends(ctx, mode):
    """Half-open bins over [0.4, 1.1): the shortest (line of sight next to the fixed point) and the longest paths are dropped, so
    the bins hold less than the fused map does."""
    got, params = _gpu(ctx, "random7", mode, "rx", "received_power", 5, (0.4, 1.1))
    want = _oracle("random7", mode, "rx", "received_power", 5, (0.4, 1.1))
    _same_bits(got, want)
    full = _oracle("random7", mode, "rx", "received_power", 1, RANGES[1])[0]
    below = _oracle("random7", mode, "rx", "received_power", 1, (0.0, 0.4))[0]
    above = _oracle("random7", mode, "rx", "received_power", 1, (1.1, 8.0))[0]
    assert below.any() and above.any() and got.any()
    np.testing.assert_allclose(got.astype(np.float64).sum(0) + below + above, full, rtol=1e-5, atol=1e-6 * float(full.max()))


# ---- 2. consequences of the definition, against the fused sweep itself ------------------------------------------------------
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
@pytest.mark.parametrize("scene", ["random7", "obstacle"])
def test_one_covering_bin_is_the_fused_map_and_the_bins_sum_to_it(ctx, scene, mode, role):
    _, fixed, X, Y = _case(scene)
    one, params = _gpu(ctx, scene, mode, role, "received_power", 1, (0.0, 8.0))
    ctx.launch(params, fixed)
    fused = ctx.get_map()
    _same_bits(one[0], fused)
    assert np.count_nonzero(fused) > fused.size // 4
    many, _ = _gpu(ctx, scene, mode, role, "received_power", 257, (0.0, 8.0))
    # at most 62 fp32 additions per cell (51 / 61 candidates and the bins they fall into) of non-negative terms: <= 4e-6 relative
    err = np.abs(many.astype(np.float64).sum(0) - fused.astype(np.float64)).max()
    print(f"{scene} {mode} {role}: max |sum of bins - fused| = {err:.3g} (map max {fused.max():.3g})")
    np.testing.assert_allclose(many.astype(np.float64).sum(0), fused, rtol=1e-5, atol=1e-6 * float(fused.max()))


# ---- 3. state ------------------------------------------------------------------------------------------------------------------
def test_profile_launch_leaves_the_fused_sweeps_alone_and_repeats_itself(ctx):
    from differt2d_amd.engine import make_params

    walls, fixed, X, Y = _case("random7")
    ctx.set_scene(walls)
    ctx.set_grid(X, Y)
    fused_params = make_params(min_order=0, max_order=2, fun="length")
    ctx.launch(fused_params, fixed)
    before = ctx.get_map()
    prof_params = make_params(min_order=0, max_order=2, **MODES["hsig"])
    p1 = ctx.power_profile(prof_params, fixed, 0.0, 3.0, 24)
    _same_bits(ctx.get_map(), before)  # the value map is still the previous sweep's
    p2 = ctx.power_profile(prof_params, fixed, 0.0, 3.0, 24)
    _same_bits(p2, p1)
    ctx.launch(fused_params, fixed)
    _same_bits(ctx.get_map(), before)
    assert p1.any() and before.any()
    # fewer bins, then another grid size on the same context: partial patches on the other side, more patches
    p3 = ctx.power_profile(prof_params, fixed, 0.0, 3.0, 3)
    np.testing.assert_allclose(p3.astype(np.float64).sum(0), p1.astype(np.float64).sum(0), rtol=1e-5, atol=1e-6 * float(p1.sum(0).max()))
    X2, Y2 = unit_grid(35, 18)
    ctx.set_grid(X2, Y2)
    q = ctx.power_profile(prof_params, fixed, 0.0, 8.0, 1)
    ctx.launch(prof_params, fixed)
    assert q.shape == (1, 18, 35)
    _same_bits(q[0], ctx.get_map())


# ---- 4. loud edges -------------------------------------------------------------------------------------------------------------
def _refused(ctx, status, word, params, fixed, r_min=0.0, r_max=3.0, nbins=8):
    from differt2d_amd import _lib as L

    with pytest.raises(L.D2DError, match=word) as e:
        ctx.power_profile(params, fixed, r_min, r_max, nbins)
    assert e.value.status == status, (e.value.status, str(e.value))
    assert isinstance(e.value, L.D2DUnsupported) == (status == -4)
    # ... and a refused launch leaves no profile behind
    out = np.zeros((nbins if 0 < nbins < 1000 else 1,) + tuple(ctx.shape), F)
    assert ctx._lib.d2d_get_power_profile(ctx._ctx, out) == -5


def test_loud_edges(ctx):
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import make_params

    walls, fixed, X, Y = _case("random7")
    ctx.set_scene(walls)
    ctx.set_reflection_coefs(None)
    ctx.set_grid(*unit_grid(19, 11))  # a grid this context has not seen: no profile yet
    ctx.set_grid(X, Y)
    out = np.zeros((8,) + X.shape, F)
    assert ctx._lib.d2d_get_power_profile(ctx._ctx, out) == -5 and b"d2d_power_profile_launch" in ctx._lib.d2d_last_error()
    kw = dict(min_order=0, max_order=2)
    _refused(ctx, -4, "sigmoid", make_params(approx=True, function="sigmoid", **kw), fixed)
    _refused(ctx, -4, "MinPath / FermatPath", make_params(solver="min", **kw), fixed)
    _refused(ctx, -4, "MinPath / FermatPath", make_params(solver="fermat", **kw), fixed)
    _refused(ctx, -4, "D2D_FUN_CUSTOM", make_params(fun="custom", **kw), fixed)
    _refused(ctx, -4, "D2D_OUT_ADD", make_params(out_mode=L.OUT_ADD, **kw), fixed)
    # a TX grid whose sweep is not culled: refused, and not counted as a fall-back
    n0 = ctx.txg_fallbacks()
    _refused(ctx, -4, "not culled", make_params(grid_role=L.GRID_TX, tol=0.6, **kw), fixed)
    ctx.set_option("txg_exhaustive", 1)
    try:
        _refused(ctx, -4, "txg_exhaustive", make_params(grid_role=L.GRID_TX, **kw), fixed)
    finally:
        ctx.set_option("txg_exhaustive", 0)
    assert ctx.txg_fallbacks() == n0
    # the per-object function: D2D_ERR_STATE without coefficients, works with them
    per_object = make_params(fun="received_power_per_object", **kw)
    _refused(ctx, -5, "d2d_set_reflection_coefs", per_object, fixed)
    ctx.set_reflection_coefs(COEF7)
    assert ctx.power_profile(per_object, fixed, 0.0, 3.0, 8).any()
    ctx.set_reflection_coefs(None)
    # the range
    ok = make_params(**kw)
    _refused(ctx, -1, "nbins", ok, fixed, nbins=0)
    _refused(ctx, -1, "r_max > r_min", ok, fixed, r_min=1.0, r_max=1.0)
    _refused(ctx, -1, "r_max > r_min", ok, fixed, r_min=2.0, r_max=1.0)
    _refused(ctx, -1, "finite", ok, fixed, r_max=float("inf"))
    _refused(ctx, -1, "finite", ok, fixed, r_min=float("nan"))
    # more bins than half of the free device memory holds (2^31 - 1 bins of 273 cells: 2.3 TB)
    _refused(ctx, -4, "free device memory", ok, fixed, nbins=2**31 - 1)
    # ... after all of which the context still works, and the grid's change drops the profile
    assert ctx.power_profile(ok, fixed, 0.0, 3.0, 8).any()
    assert ctx._lib.d2d_get_power_profile(ctx._ctx, out) == 0
    ctx.set_grid(*unit_grid(19, 11))
    assert ctx._lib.d2d_get_power_profile(ctx._ctx, np.zeros((8, 11, 19), F)) == -5


# ---- 5. the Scene methods ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("role", ["rx", "tx"])
def test_scene_methods_mirror_the_context(ctx, role):
    from differt2d_amd import utils
    from differt2d_amd.engine import make_params
    from differt2d_amd.geometry import Point
    from differt2d_amd.scene import Scene

    walls, fixed, X, Y = _case("random7")
    pts = {"a": Point(xy=fixed), "b": Point(xy=(F(1.0) - fixed).astype(F))}
    scene = Scene.from_walls_array(walls)
    scene = scene.with_transmitters(**pts) if role == "rx" else scene.with_receivers(**pts)
    method = scene.power_delay_profile_on_receivers_grid if role == "rx" else scene.power_delay_profile_on_transmitters_grid
    got = dict(method(X, Y, utils.received_power, dict(r_coef=0.4, height=0.2), length_range=(0.0, 3.0), nbins=24, min_order=0,
                      max_order=2, approx=True, function="hard_sigmoid", filter_objects=lambda o: o is not scene.objects[3]))
    assert list(got) == ["a", "b"]
    allowed = np.ones(7, np.uint8)
    allowed[3] = 0
    ctx.set_scene(walls)
    ctx.set_candidate_mask(allowed)
    ctx.set_grid(X, Y)
    params = make_params(min_order=0, max_order=2, r_coef=0.4, height=0.2, grid_role=_role_id(role), **MODES["hsig"])
    for name, pt in pts.items():
        _same_bits(got[name], ctx.power_profile(params, pt.xy, 0.0, 3.0, 24))
        assert got[name].any()
    ctx.set_candidate_mask(None)
    assert not np.array_equal(got["a"], got["b"])
    total, mean, rms = utils.delay_statistics(got["a"], (0.0, 3.0))
    lit = total > 0
    assert lit.any() and np.isfinite(mean[lit]).all() and (mean[lit] > 0).all() and (rms[lit] >= 0).all() and np.isnan(mean[~lit]).all()
