"""The power-angle profile (include/d2d.h: d2d_power_angle_launch; power_sink_kernel, AngleSink): per cell the fused sweep's
contributions binned by the direction of departure or arrival.  Held bit for bit to the oracle recipe of
``tests/power_angle_oracle.py`` (which ``tests/test_power_angle_cpu.py`` pins to ``R.power_map``, to the g++ build of the direction
header and to float64), to the fused map, to the straight line of sight, and to its state rules and refusals.  The scenes are those
of ``tests/test_gpu_strongest_paths.py``; the directed contributions are computed once per session."""

import functools
import subprocess

import numpy as np
import pytest

from conftest import unit_grid
from power_angle_oracle import AT_RX, AT_TX, PowerAngleProfile, directed_contributions, fold, turns, turns_inputs
from test_gpu_strongest_paths import COEF7, MODES, _case, _role_id

pytestmark = pytest.mark.gpu

F = np.float32
ENDS = {"tx": AT_TX, "rx": AT_RX}
FUSED_FUNS = ["received_power", "length_squared", "length", "one", "received_power_per_object"]
ORIGIN_ODD = F(0.3)  # no multiple of 1/12 or 1/8


@pytest.fixture(scope="module")
def ctx():
    from differt2d_amd.engine import Context

    with Context(0) as c:
        yield c


@functools.lru_cache(maxsize=None)
def _directed(scene, mode, role, fun, lo=0, hi=2, masked=()):
    walls, fixed, X, Y = _case(scene)
    kw = dict(min_order=lo, max_order=hi, grid_role=role, filter_nodes=set(masked) or None, **MODES[mode])
    if fun == "received_power_per_object":
        kw.update(coef=COEF7, fun_kwargs=dict(height=0.25))
    out = directed_contributions(walls, fixed, X, Y, fun=fun, **kw)
    for a in out[1:]:
        a.setflags(write=False)
    return out


def _oracle(scene, mode, role, fun, end, origin, nbins, lo=0, hi=2, masked=()):
    _, T, D = _directed(scene, mode, role, fun, lo, hi, masked)
    shape = _case(scene)[2].shape
    out, total = fold(T, D, ENDS[end], origin, nbins)
    return PowerAngleProfile(out.reshape((nbins,) + shape), total.reshape(shape))


def _params(mode, role, fun, lo=0, hi=2, **extra):
    from differt2d_amd.engine import make_params

    if fun == "received_power_per_object":
        extra["height"] = 0.25
    return make_params(min_order=lo, max_order=hi, fun=fun, grid_role=_role_id(role), **MODES[mode], **extra)


def _setup(ctx, scene, fun="received_power"):
    walls, fixed, X, Y = _case(scene)
    ctx.set_scene(walls)
    if fun == "received_power_per_object":
        ctx.set_reflection_coefs(COEF7)
    ctx.set_grid(X, Y)
    return fixed


def _same(got, want):
    for name, g, w in zip(want._fields, got, want):
        assert g.dtype == w.dtype == np.float32 and g.shape == w.shape, (name, g.dtype, g.shape, w.dtype, w.shape)
        bad = np.ascontiguousarray(g).view(np.uint32) != np.ascontiguousarray(w).view(np.uint32)
        assert not bad.any(), f"{name}: {bad.sum()} of {bad.size} entries differ, first at {tuple(np.argwhere(bad)[0])}: {g[bad][0]!r} != {w[bad][0]!r}"


def _dropped(T, D, end):
    """[C, cells]: non-zero contributions whose direction at ``end`` names no bin."""
    o = 0 if ENDS[end] == AT_TX else 2
    return (T != 0) & np.isnan(turns(D[:, :, o], D[:, :, o + 1]))


# ---- 1. bit for bit against the oracle recipe ---------------------------------------------------------------------------------
@pytest.mark.parametrize("end", ["tx", "rx"])
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
@pytest.mark.parametrize("scene", ["random7", "obstacle", "square_centre"])
def test_profile_equals_the_oracle_recipe(ctx, scene, mode, role, end):
    """Twelve bins and eight (which put the diagonals on edges), origin 0 and one that is no bin multiple."""
    _, T, D = _directed(scene, mode, role, "received_power")
    want12 = _oracle(scene, mode, role, "received_power", end, 0.0, 12)
    # (so that the comparison does not pass on empty ground)
    spread = ((want12.bins != 0).sum(axis=0) >= 2).mean()
    dropped = _dropped(T, D, end)
    o = 0 if end == "tx" else 2
    f = turns(D[:, :, o], D[:, :, o + 1])
    on_edge = int(((T != 0) & (f * F(12) == np.floor(f * F(12)))).sum())
    print(f"{scene} {mode} {role} at {end}: {spread:.2f} of the cells have power in two or more bins, {(want12.bins != 0).any(axis=(1, 2)).sum()} "
          f"bins in use, {dropped.sum()} contributions without a direction, {on_edge} on a bin edge")
    if scene == "random7":
        assert spread > 1 / 4 and not dropped.any()
    elif scene == "obstacle":
        assert spread > 1 / 2 and (want12.bins != 0).any(axis=(1, 2)).all()
    else:  # the cell that is the fixed end point has a line of sight without a direction; the axes lie on bin edges
        assert spread >= 0.6 and dropped.sum() == 1 and dropped[0].reshape(9, 9)[4, 4]
        # 69 (hard) and 81 (hard_sigmoid) non-zero contributions run along the axes through the fixed point: the one without a
        # direction, which atan2 would put at 0, and 68 / 80 whose direction is a multiple of a quarter turn, an edge of twelve bins
        assert on_edge + dropped.sum() == (69 if mode == "hard" else 81)
    fixed = _setup(ctx, scene)
    params = _params(mode, role, "received_power")
    for nbins, origin in ((12, 0.0), (8, 0.0), (12, ORIGIN_ODD), (8, ORIGIN_ODD)):
        got = ctx.power_angle(params, fixed, end, origin, nbins)
        want = _oracle(scene, mode, role, "received_power", end, origin, nbins)
        assert got.bins.shape == (nbins, *want.total.shape) and np.count_nonzero(got.bins) > 0
        _same(got, want)
        if scene == "square_centre":
            # the bins miss exactly what has no direction: one cell, beyond any reordering of an fp32 sum (at most 17 terms)
            s = got.bins.astype(np.float64).sum(axis=0)
            differ = np.abs(s - got.total) > 17 * 2.0**-24 * np.abs(got.bins).astype(np.float64).sum(axis=0)
            assert differ.sum() == 1 and differ[4, 4]


# ---- 2. identities --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
@pytest.mark.parametrize("fun", FUSED_FUNS)
def test_total_and_one_bin_are_the_fused_map_and_the_line_of_sight_points_at_the_other_end(ctx, fun, mode, role):
    walls, fixed, X, Y = _case("random7")
    params = _params(mode, role, fun)
    los = _params(mode, role, fun, 0, 0)
    # over an RX grid the transmitter is the fixed point: AT_TX looks from it to the cell; over a TX grid AT_RX does
    fixed_end = "tx" if role == "rx" else "rx"
    try:
        _setup(ctx, "random7", fun)
        got = ctx.power_angle(params, fixed, "rx", 0.0, 12)
        one = ctx.power_angle(params, fixed, "tx", ORIGIN_ODD, 1)
        ctx.launch(params, fixed)
        fused = ctx.get_map()
        sight = ctx.power_angle(los, fixed, fixed_end, 0.0, 12)
        ctx.launch(los, fixed)
        fused_los = ctx.get_map()
    finally:
        ctx.set_reflection_coefs(None)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    assert np.isfinite(fused).all() and np.count_nonzero(fused) > fused.size // 3
    assert np.array_equal(bits(got.total), bits(fused)) and np.array_equal(bits(one.total), bits(fused))
    assert one.bins.shape == (1, *fused.shape) and np.array_equal(bits(one.bins[0]), bits(fused))  # (no direction is dropped here)
    assert ((got.bins != 0).sum(axis=0) >= 2).mean() > 1 / 4
    # the line of sight alone: every cell's power sits in the bin of atan2(cell - fixed), known in float64
    f = np.mod(np.arctan2(Y.astype(np.float64) - float(fixed[1]), X.astype(np.float64) - float(fixed[0])) / (2 * np.pi), 1.0)
    assert (np.abs(f * 12 - np.round(f * 12)) > 1e-4).all()  # (no cell on a bin edge)
    want = np.zeros_like(sight.bins)
    np.put_along_axis(want, np.floor(f * 12).astype(int)[None], fused_los[None], axis=0)
    assert np.count_nonzero(fused_los) > fused_los.size // 3 and np.array_equal(bits(sight.total), bits(fused_los))
    assert np.array_equal(bits(sight.bins), bits(want))
    if fun == "received_power_per_object":  # the negative and the zero coefficient are exercised
        cands, T, _ = _directed("random7", mode, role, fun)
        through = lambda w: np.array([w in c for c in cands])
        assert (T[through(2)] < 0).any() and not T[through(6)].any() and (_directed("random7", mode, role, "one")[1][through(6)] != 0).any()
        assert (got.bins < 0).any()
        _same(got, _oracle("random7", mode, role, fun, "rx", 0.0, 12))


# ---- 3. the highest order and the bin counts at the limits --------------------------------------------------------------------------
@pytest.mark.parametrize("end", ["tx", "rx"])
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
def test_orders_up_to_three_on_the_square(ctx, mode, role, end):
    fixed = _setup(ctx, "square_centre")
    got = ctx.power_angle(_params(mode, role, "received_power", 0, 3), fixed, end, ORIGIN_ODD, 12)
    want = _oracle("square_centre", mode, role, "received_power", end, ORIGIN_ODD, 12, 0, 3)
    third = _oracle("square_centre", mode, role, "received_power", end, ORIGIN_ODD, 12, 3, 3)
    assert np.count_nonzero(third.bins) > 81  # (the third order is there)
    _same(got, want)


@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
@pytest.mark.parametrize("nbins", [1, 4096])
def test_one_bin_and_the_most_bins(ctx, nbins, mode, role):
    fixed = _setup(ctx, "random7")
    got = ctx.power_angle(_params(mode, role, "received_power"), fixed, "rx", ORIGIN_ODD, nbins)
    want = _oracle("random7", mode, role, "received_power", "rx", ORIGIN_ODD, nbins)
    _same(got, want)
    if nbins == 4096:
        assert (got.bins != 0).any(axis=(1, 2)).sum() > 200


# ---- 4. the direction on the device ----------------------------------------------------------------------------------------------
def test_selftest_angle_equals_the_host_builds_bit_for_bit(ctx, tmp_path):
    from test_power_angle_cpu import GXX, SRC, load_host

    dx, dy = turns_inputs()
    keep = np.r_[0 : 10**5 - 15, dx.size - 15 : dx.size]  # the exact cases and the head of the random ones, then what gives NaN
    dx, dy = np.ascontiguousarray(dx[keep]), np.ascontiguousarray(dy[keep])
    assert dx.size == 10**5
    got = ctx.selftest_angle(dx, dy)
    so = str(tmp_path / "libpa_host.so")
    subprocess.check_call(GXX + ["-shared", "-fPIC", "-o", so, SRC])
    host = np.empty_like(dx)
    load_host(so).pa_turns(dx.size, dx, dy, host)
    nan = np.isnan(host)
    assert nan.sum() == 15 and np.array_equal(np.isnan(got), nan)
    for name, want in (("g++", host), ("NumPy", turns(dx, dy))):
        bad = (got.view(np.uint32) != want.view(np.uint32)) & ~nan
        assert not bad.any(), f"{name}: {bad.sum()} of {bad.size} differ, first at ({dx[bad][0]!r}, {dy[bad][0]!r}): {got[bad][0]!r} != {want[bad][0]!r}"
    assert (np.maximum(np.abs(dx), np.abs(dy))[~nan] < 1e-38).any()  # (denormals took part)


# ---- 5. the candidate mask and min_order ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("role", ["rx", "tx"])
def test_profile_honours_the_candidate_mask_and_min_order(ctx, role):
    from differt2d_amd.engine import make_params

    walls, fixed, X, Y = _case("random7")
    allowed = np.ones(7, np.uint8)
    allowed[[2, 5]] = 0
    ctx.set_scene(walls)
    ctx.set_candidate_mask(allowed)
    try:
        ctx.set_grid(X, Y)
        got = ctx.power_angle(make_params(min_order=0, max_order=2, grid_role=_role_id(role)), fixed, "rx", 0.0, 12)
    finally:
        ctx.set_candidate_mask(None)
    everything = _oracle("random7", "hard", role, "received_power", "rx", 0.0, 12)
    _same(got, _oracle("random7", "hard", role, "received_power", "rx", 0.0, 12, 0, 2, (2, 5)))
    assert not np.array_equal(got.bins, everything.bins)
    # min_order = 1: the line of sight is left out
    _setup(ctx, "random7")
    got = ctx.power_angle(_params("hsig", role, "received_power", 1, 2), fixed, "tx", 0.0, 12)
    _same(got, _oracle("random7", "hsig", role, "received_power", "tx", 0.0, 12, 1, 2))
    assert got.bins.any() and not np.array_equal(got.total, _oracle("random7", "hsig", role, "received_power", "tx", 0.0, 12).total)


# ---- 6. state and refusals ---------------------------------------------------------------------------------------------------------
def test_launch_leaves_the_other_results_alone_and_repeats_itself(ctx):
    from differt2d_amd.engine import make_params

    walls, fixed, X, Y = _case("random7")
    ctx.set_scene(walls)
    ctx.set_grid(X, Y)
    fused_params = make_params(min_order=0, max_order=2, fun="length")
    ctx.launch(fused_params, fixed)
    before = ctx.get_map()
    params = make_params(min_order=0, max_order=2, **MODES["hsig"])
    profile = ctx.power_profile(params, fixed, 0.0, 3.0, 24)
    rec = ctx.valid_paths(params, fixed)
    top = ctx.strongest_paths(params, fixed, 8)
    cf = ctx.coherent_field(params, fixed, 20.0, "sqrt")
    pa = ctx.power_angle(params, fixed, "rx", ORIGIN_ODD, 12)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    assert np.array_equal(bits(ctx.get_map()), bits(before)) and before.any()  # still the previous sweep's map
    assert np.array_equal(bits(ctx.get_profile(24)), bits(profile)) and profile.any()
    n = len(rec["cell"])
    again = {"cell": np.empty(n, np.int32), "valid": np.empty(n, F), "length": np.empty(n, F)}
    vp = lambda a: a.ctypes.data
    assert ctx._lib.d2d_get_valid_paths(ctx._ctx, n, vp(again["cell"]), None, None, None, None, vp(again["valid"]), vp(again["length"])) == 0
    assert n > 0 and all(np.array_equal(again[f].view(np.uint32), rec[f].view(np.uint32)) for f in again)
    top2 = ctx.get_strongest_paths()
    assert all(np.array_equal(a, b, equal_nan=a.dtype == np.float32) for a, b in zip(top, top2)) and top.power.any()
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(ctx.get_coherent_field(), cf)) and cf.im.any()
    _same(ctx.power_angle(params, fixed, "rx", ORIGIN_ODD, 12), pa)  # two launches give the same bits
    _same(ctx.get_power_angle(), pa)
    assert pa.bins.any() and np.array_equal(bits(pa.total), bits(top.total))
    # either pointer may be NULL
    only_total = np.empty(ctx.shape, F)
    assert ctx._lib.d2d_get_power_angle(ctx._ctx, None, vp(only_total)) == 0 and np.array_equal(bits(only_total), bits(pa.total))
    # the other sinks leave the profile alone in their turn
    ctx.strongest_paths(params, fixed, 2)
    ctx.coherent_field(params, fixed, 20.0, "linear")
    ctx.power_profile(params, fixed, 0.0, 3.0, 8)
    ctx.launch(fused_params, fixed)
    _same(ctx.get_power_angle(), pa)
    # fewer bins after more: the result has the new launch's planes
    few = ctx.power_angle(params, fixed, "rx", ORIGIN_ODD, 3)
    assert few.bins.shape == (3, *ctx.shape)
    _same(few, _oracle("random7", "hsig", "rx", "received_power", "rx", ORIGIN_ODD, 3))
    # another grid size on the same context: the result goes with the grid
    X2, Y2 = unit_grid(35, 18)
    ctx.set_grid(X2, Y2)
    with pytest.raises(Exception) as e:
        ctx.get_power_angle()
    assert getattr(e.value, "status", None) == -5
    q = ctx.power_angle(params, fixed, "tx", 0.0, 5)
    ctx.launch(params, fixed)
    assert q.bins.shape == (5, 18, 35) and q.total.shape == (18, 35)
    assert np.array_equal(bits(q.total), bits(ctx.get_map()))
    _, T, D = directed_contributions(walls, fixed, X2, Y2, min_order=0, max_order=2, **MODES["hsig"])
    out, total = fold(T, D, AT_TX, 0.0, 5)
    _same(q, PowerAngleProfile(out.reshape(5, 18, 35), total.reshape(18, 35)))


def _nothing_to_get(ctx):
    bufs = [np.zeros((4096,) + tuple(ctx.shape), F), np.zeros(ctx.shape, F)]
    rc = ctx._lib.d2d_get_power_angle(ctx._ctx, *(b.ctypes.data for b in bufs))
    return rc == -5 and b"d2d_power_angle_launch" in ctx._lib.d2d_last_error()


def _refused(ctx, previous, status, word, params, fixed, end="rx", origin=0.0, nbins=12):
    """The launch is refused with ``status`` and a message that has ``word``, and the previous result is still there to get."""
    from differt2d_amd import _lib as L

    with pytest.raises(L.D2DError, match=word) as e:
        ctx.power_angle(params, fixed, end, origin, nbins)
    assert e.value.status == status, (e.value.status, str(e.value))
    assert isinstance(e.value, L.D2DUnsupported) == (status == -4)
    _same(ctx.get_power_angle(), previous)


def test_loud_edges(ctx):
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import make_params

    walls, fixed, X, Y = _case("random7")
    ctx.set_scene(walls)
    ctx.set_reflection_coefs(None)
    ctx.set_grid(*unit_grid(19, 11))  # a grid this context has not seen: no result yet
    ctx.set_grid(X, Y)
    assert _nothing_to_get(ctx)
    with pytest.raises(L.D2DError) as e:
        ctx.get_power_angle()
    assert e.value.status == -5
    kw = dict(min_order=0, max_order=2)
    ok = make_params(**kw)
    # a refusal before any launch leaves nothing to get
    with pytest.raises(L.D2DUnsupported, match="sigmoid"):
        ctx.power_angle(make_params(approx=True, function="sigmoid", **kw), fixed, "rx", 0.0, 12)
    assert _nothing_to_get(ctx)
    previous = ctx.power_angle(ok, fixed, "rx", ORIGIN_ODD, 12)
    assert previous.bins.any()
    n0 = ctx.txg_fallbacks()
    _refused(ctx, previous, -4, "sigmoid", make_params(approx=True, function="sigmoid", **kw), fixed)
    _refused(ctx, previous, -4, "MinPath / FermatPath", make_params(solver="min", **kw), fixed)
    _refused(ctx, previous, -4, "MinPath / FermatPath", make_params(solver="fermat", **kw), fixed)
    _refused(ctx, previous, -4, "D2D_FUN_CUSTOM", make_params(fun="custom", **kw), fixed)
    _refused(ctx, previous, -4, "D2D_OUT_ADD", make_params(out_mode=L.OUT_ADD, **kw), fixed)
    _refused(ctx, previous, -4, "not culled", make_params(grid_role=L.GRID_TX, tol=0.6, **kw), fixed)
    _refused(ctx, previous, -5, "d2d_set_reflection_coefs", make_params(fun="received_power_per_object", **kw), fixed)
    for end in (2, -1, "up"):
        _refused(ctx, previous, -1, "end", ok, fixed, end=end)
    for origin in (1.0, -1e-30, -0.25, float("nan"), float("inf"), float("-inf")):
        _refused(ctx, previous, -1, "origin", ok, fixed, origin=origin)
    for nbins in (0, -1, 4097):
        _refused(ctx, previous, -1, "nbins", ok, fixed, nbins=nbins)
    assert ctx.txg_fallbacks() == n0
    # ... after all of which the context still works (the library's constants are taken as well as the names), and the grid's
    # change drops the result
    a = ctx.power_angle(ok, fixed, L.D2D_ANGLE_AT_TX, 0.0, 4096)
    _same(a, ctx.power_angle(ok, fixed, "tx", 0.0, 4096))
    assert a.bins.any() and not _nothing_to_get(ctx)
    ctx.set_grid(*unit_grid(19, 11))
    assert _nothing_to_get(ctx)


# ---- 7. the Scene methods ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("role", ["rx", "tx"])
def test_scene_methods_mirror_the_context(ctx, role):
    from differt2d_amd import utils
    from differt2d_amd.engine import PowerAngleProfile as PA, make_params
    from differt2d_amd.geometry import Point
    from differt2d_amd.scene import Scene
    from power_angle_oracle import origin_turns

    walls, fixed, X, Y = _case("random7")
    pts = {"a": Point(xy=fixed), "b": Point(xy=(F(1.0) - fixed).astype(F))}
    scene = Scene.from_walls_array(walls)
    scene = scene.with_transmitters(**pts) if role == "rx" else scene.with_receivers(**pts)
    method = scene.power_angle_profile_on_receivers_grid if role == "rx" else scene.power_angle_profile_on_transmitters_grid
    common = dict(min_order=0, max_order=2, approx=True, function="hard_sigmoid", filter_objects=lambda o: o is not scene.objects[3])
    origin = -np.pi / 5
    arr = dict(method(X, Y, utils.received_power, dict(r_coef=0.4, height=0.2), at="rx", nbins=12, origin=origin, **common))
    dep = dict(method(X, Y, utils.received_power, dict(r_coef=0.4, height=0.2), at="tx", nbins=36, **common))
    assert list(arr) == list(dep) == ["a", "b"]
    allowed = np.ones(7, np.uint8)
    allowed[3] = 0
    ctx.set_scene(walls)
    ctx.set_candidate_mask(allowed)
    ctx.set_grid(X, Y)
    params = make_params(min_order=0, max_order=2, r_coef=0.4, height=0.2, grid_role=_role_id(role), **MODES["hsig"])
    assert origin_turns(origin) == F(0.9)
    for name, pt in pts.items():
        assert isinstance(arr[name], PA)
        _same(arr[name], ctx.power_angle(params, pt.xy, "rx", origin_turns(origin), 12))
        _same(dep[name], ctx.power_angle(params, pt.xy, "tx", 0.0, 36))
        assert arr[name].bins.any() and dep[name].bins.shape == (36, 13, 21)
    ctx.set_candidate_mask(None)
    assert not np.array_equal(arr["a"].bins, arr["b"].bins)
    with pytest.raises(Exception, match="at="):
        next(iter(method(X, Y, utils.received_power, at="up")))
    # angular_statistics / pattern_power on the result: the binned power is the total up to fp32 summation order, the spread lies in
    # [0, 1], and an isotropic pattern receives the binned power
    a = arr["a"]
    st = utils.angular_statistics(a, origin=origin)
    lit = a.total > 0
    assert lit.any() and np.isnan(st.mean[~lit]).all() and np.isnan(st.spread[~lit]).all()
    assert np.abs(st.power[lit] / a.total[lit] - 1).max() < 57 * 2.0**-23
    assert (st.spread[lit] >= 0).all() and (st.spread[lit] <= 1).all() and (st.spread[lit] > 0.3).any() and (st.spread[lit] < 1e-6).any()
    assert np.array_equal(utils.pattern_power(a, np.ones(12)), st.power)
