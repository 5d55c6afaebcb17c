"""The frequency response's wall adjoint on the GPU (include/d2d.h: d2d_field_walls_vjp_launch; power_sink_kernel, WallGradSink):
``normal_bar`` within the derived bound of the float64 oracle of ``tests/field_walls_vjp_oracle.py``, ``walls_bar`` as its exact fp64
product with the fp32 normals, the header on the device against its host build, the same bits run to run, the exact rules, the
incoherent limit against the value+grad sweep's ``objects_bar``, the state rules and every refusal, the ``Scene`` methods, the
wall-fitting loop of ``tests/test_field_walls_vjp_cpu.py`` and one case of 70 walls."""

import ctypes as C
import functools

import numpy as np
import pytest

import field_walls_vjp_oracle as WO
from conftest import unit_grid
from test_field_position_vjp_cpu import AMPS, HEIGHT, INV_20, bars, inv_list
from test_field_walls_vjp_cpu import FIT, ORACLE_RATIO, fitting_inputs, segment_case
from test_gpu_strongest_paths import COEF7, MODES, _case, _role_id

pytestmark = pytest.mark.gpu

F = np.float32
RAGGED = (13, 19)  # partial patches on both sides, lanes outside the grid in every patch row


@pytest.fixture(scope="module")
def ctx():
    from differt2d_amd.engine import Context

    with Context(0) as c:
        yield c


def grid_of(scene, grid=None):
    walls, fixed, X, Y = _case(scene)
    if grid is not None:
        X, Y = unit_grid(*grid)
    return walls, fixed, X, Y


@functools.lru_cache(maxsize=None)
def _bars(scene, nf, seed=0, grid=None):
    shape = grid_of(scene, grid)[2].shape
    rb, ib = bars(nf, shape, 3000 + 31 * seed + nf)
    rb.setflags(write=False)
    ib.setflags(write=False)
    return rb, ib


def _gpu(ctx, scene, role, fun, inv, rb, ib, amp, lo=0, hi=2, allowed=None, grid=None):
    from differt2d_amd.engine import make_params

    walls, fixed, X, Y = grid_of(scene, grid)
    ctx.set_scene(walls)
    if allowed is not None:
        ctx.set_candidate_mask(allowed)
    extra = {}
    if fun == "received_power_per_object":
        ctx.set_reflection_coefs(COEF7)
        extra["height"] = HEIGHT
    elif fun == "received_power":
        extra.update(r_coef=0.5, height=HEIGHT)
    ctx.set_grid(X, Y)
    params = make_params(min_order=lo, max_order=hi, fun=fun, grid_role=_role_id(role), **MODES["hard"], **extra)
    try:
        return ctx.field_walls_vjp(params, fixed, inv, rb, ib, amp), params
    finally:
        if allowed is not None:
            ctx.set_candidate_mask(None)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64)


def _walls_bar_is_the_product(got, walls, tag):
    """``walls_bar == normal_bar * n`` in fp64, exactly."""
    assert got.normal_bar.dtype == got.walls_bar.dtype == np.float64, tag
    assert got.normal_bar.shape == (len(walls), 2) and got.walls_bar.shape == (len(walls), 2, 2), tag
    want = WO.walls_bar_of(got.normal_bar, walls)
    both_nan = np.isnan(want) & np.isnan(got.walls_bar)
    assert ((_bits(got.walls_bar) == _bits(want)) | both_nan).all(), tag


def _check(ctx, scene, role, fun, amp, nf, lo=0, hi=2, masked=(), grid=None, need_twice=False):
    """One launch against the float64 oracle: every entry within its bound, untouched walls exactly ``+0.0``; returns the worst
    fraction of the bound."""
    walls = grid_of(scene, grid)[0]
    cands, T, Rl, S, p0 = segment_case(scene, role, fun, lo, hi, masked, grid)
    rb, ib = _bars(scene, nf, grid=grid)
    inv = inv_list(nf)
    ph = WO.physics(cands, T, Rl, S, walls, p0, fun, HEIGHT, inv, rb, ib, AMPS[amp])
    WO.guards(cands, T, ph, max_order=hi - lo, need_twice=need_twice)
    allowed = None
    if masked:
        allowed = np.ones(len(walls), np.uint8)
        allowed[list(masked)] = 0
    got, _ = _gpu(ctx, scene, role, fun, inv, rb, ib, amp, lo, hi, allowed, grid)
    tag = f"{scene} {grid or ''} {role} {fun} {amp} nf={nf} orders {lo}-{hi} masked {masked}"
    _walls_bar_is_the_product(got, walls, tag)
    err = np.abs(got.normal_bar - ph.normal_bar)
    touched = ph.scale > 0
    frac = float((err[touched] / ph.bound[touched]).max())
    print(f"{tag}: worst error / bound = {frac:.3f} on {int(touched.sum())} touched walls, worst bound / scale = "
          f"{(ph.bound[touched] / ph.scale[touched, None]).max():.2e}")
    assert (err <= ph.bound).all(), (tag, frac)
    assert not _bits(got.normal_bar[~touched]).any() and not _bits(got.walls_bar[~touched]).any(), tag  # exactly +0.0
    return frac


# ---- 1. within the bound of the float64 oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", [1, 8, 9, 17])
@pytest.mark.parametrize("amp", ["sqrt", "linear"])
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("scene", ["obstacle", "random7"])
def test_normal_bar_within_the_bound_of_the_float64_oracle(ctx, scene, role, amp, nf):
    """nf: a partial block, a full one, a full one plus one, two plus one."""
    _check(ctx, scene, role, "received_power", amp, nf)


@pytest.mark.parametrize("amp", ["sqrt", "linear"])
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("fun", ["received_power_per_object", "length", "one", "length_squared"])
def test_within_the_bound_for_every_fused_function(ctx, fun, role, amp):
    """``received_power_per_object`` with ``COEF7`` (a negative and a zero coefficient: the zero one's candidates contribute nothing),
    ``length``, ``one`` and ``length_squared``; ``received_power`` is the test above."""
    _check(ctx, "random7", role, fun, amp, 9)


@pytest.mark.parametrize("role", ["rx", "tx"])
def test_within_the_bound_at_orders_0_to_3_under_a_mask_and_on_a_ragged_grid(ctx, role):
    """Orders 0-3 on ``obstacle``, where ``(0, 2, 0)`` between the square's facing walls visits a wall twice (both terms go to its
    row); orders 1-2 alone; a candidate mask that takes contributions away; the ragged 13 x 19 grid, where every patch row and column
    ends in lanes outside the grid that must not be counted."""
    _check(ctx, "obstacle", role, "received_power", "sqrt", 9, 0, 3, need_twice=True)
    _check(ctx, "random7", role, "received_power", "linear", 9, 1, 2)
    everything = segment_case("random7", role)[1]
    masked = segment_case("random7", role, masked=(2, 5))[1]
    assert (~(everything == 0)).sum() > (~(masked == 0)).sum() > 0  # (the mask takes contributions away)
    _check(ctx, "random7", role, "received_power", "linear", 9, masked=(2, 5))
    for nf in (8, 17):
        _check(ctx, "random7", role, "received_power", "sqrt", nf, grid=RAGGED)


def test_header_on_the_device_equals_its_host_build(ctx):
    """d2d_wallgrad.hpp on the device against the NumPy restatement (which the CPU test holds the g++ build to), bit for bit over the
    generated list and the special values."""
    cols = WO.header_inputs()
    got = ctx.selftest_wallgrad(*cols)
    want = WO.bounce(*cols)
    for name, g, w in zip("qx qy Wa Wb".split(), got, want):
        w = np.ascontiguousarray(w, F)
        both_nan = np.isnan(g) & np.isnan(w)
        bad = (_bits(g) != _bits(w)) & ~both_nan
        assert not bad.any(), (name, int(bad.sum()), int(np.flatnonzero(bad)[0]))
    assert np.array_equal(got[4] != 0, want[4]) and set(np.unique(got[4])) == {0.0, 1.0}


# ---- 2. the same bits ---------------------------------------------------------------------------------------------------------------------
def test_same_bits_run_to_run_and_after_other_products(ctx):
    from differt2d_amd.engine import make_params

    nf = 17
    rb, ib = _bars("random7", nf)
    first, params = _gpu(ctx, "random7", "rx", "received_power", inv_list(nf), rb, ib, "sqrt")
    assert first.normal_bar.any()
    again, _ = _gpu(ctx, "random7", "rx", "received_power", inv_list(nf), rb, ib, "sqrt")
    walls, fixed, X, Y = _case("random7")
    ctx.frequency_response(params, fixed, inv_list(3))
    ctx.field_position_vjp(params, fixed, inv_list(nf), rb, ib, "sqrt")
    ctx.strongest_paths(params, fixed, 3)
    ctx.launch(make_params(min_order=0, max_order=2), fixed)
    ctx.get_map()
    ctx.field_walls_vjp(params, fixed, inv_list(2), rb[:2], ib[:2], "linear")  # (another call of the same product in between)
    third = ctx.field_walls_vjp(params, fixed, inv_list(nf), rb, ib, "sqrt")
    for other in (again, third):
        for a, b in zip(first, other):
            assert np.array_equal(_bits(a), _bits(b))


# ---- 3. exact rules -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("role", ["rx", "tx"])
def test_exact_rules(ctx, role):
    scene = "random7"
    rb17, ib17 = (a.copy() for a in _bars(scene, 17))
    touched = WO.physics(*segment_case(scene, role)[:4], _case(scene)[0], segment_case(scene, role)[4], "received_power", HEIGHT, inv_list(8),
                         rb17[:8], ib17[:8], WO.AMP_SQRT).scale > 0
    assert 0 < touched.sum() < touched.size
    for nf in (8, 16):  # appending a wavelength whose planes are zero changes no bit: a new block, and one that crosses a block edge
        rb, ib = rb17[: nf + 1].copy(), ib17[: nf + 1].copy()
        rb[nf] = ib[nf] = 0
        short, _ = _gpu(ctx, scene, role, "received_power", inv_list(nf), rb[:nf], ib[:nf], "sqrt")
        more, _ = _gpu(ctx, scene, role, "received_power", inv_list(nf + 1), rb, ib, "sqrt")
        twice, _ = _gpu(ctx, scene, role, "received_power", inv_list(nf), 2 * rb[:nf], 2 * ib[:nf], "sqrt")
        zero, _ = _gpu(ctx, scene, role, "received_power", inv_list(nf), 0 * rb[:nf], F(-0.0) * ib[:nf], "sqrt")
        for s, m, t2, z in zip(short, more, twice, zero):
            assert s[touched].any() and np.array_equal(_bits(s), _bits(m))
            assert np.array_equal(_bits(2.0 * s), _bits(t2))
            assert not _bits(z).any()  # +0.0 in every bit of both outputs
            assert not _bits(s[~touched]).any()  # walls that no contributing candidate touches
    # a sweep of order 0 alone gives all zeros
    los, _ = _gpu(ctx, scene, role, "received_power", inv_list(9), rb17[:9], ib17[:9], "linear", 0, 0)
    assert not _bits(los.normal_bar).any() and not _bits(los.walls_bar).any() and los.normal_bar.shape == (7, 2)


@pytest.mark.parametrize("role", ["rx", "tx"])
def test_a_nan_reaches_the_walls_of_its_candidates_and_no_others(ctx, role):
    """A NaN cotangent in one cell makes ``G`` NaN for every candidate that contributes there: the walls those candidates bounce off
    become NaN, every other wall keeps its bits."""
    nf = 9
    cands, T, Rl, S, p0 = segment_case("random7", role)
    reach = np.array([[(~(T[ci] == 0)) for ci, c in enumerate(cands) if w in [int(x) for x in c]] for w in range(7)], bool).any(axis=1)  # [wall, cell]
    counts = reach.sum(axis=0)
    cell = int(np.flatnonzero((counts > 0) & (counts < reach.any(axis=1).sum()))[0])  # it reaches some touched walls, not all
    rb, ib = (a.copy() for a in _bars("random7", nf))
    clean, _ = _gpu(ctx, "random7", role, "received_power", inv_list(nf), rb, ib, "linear")
    ib.reshape(nf, -1)[8, cell] = np.nan  # one cell, one plane, in the second block
    got, _ = _gpu(ctx, "random7", role, "received_power", inv_list(nf), rb, ib, "linear")
    hit = reach[:, cell]
    assert hit.any() and np.isfinite(clean.normal_bar).all() and clean.normal_bar[~hit].any()
    assert np.isnan(got.normal_bar[hit]).all() and np.array_equal(_bits(got.normal_bar[~hit]), _bits(clean.normal_bar[~hit]))
    _walls_bar_is_the_product(got, _case("random7")[0], "nan")


# ---- 4. against the value+grad sweep in the incoherent limit -----------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["obstacle", "random7"])
def test_incoherent_limit_is_the_objects_bar_of_the_value_and_grad_sweep(ctx, scene):
    """LINEAR, ``inv = [0]``, ``re_bar = 1``, ``im_bar = 0``: ``re`` is the power map, so ``walls_bar`` agrees with ``objects_bar`` of
    ``launch_vg(..., scene_vjp=True)`` for a cotangent of ones in hard mode, within 1e-5 of the wall's summed term magnitude of the
    float64 oracle, every entry finite."""
    walls, fixed, X, Y = _case(scene)
    cands, T, Rl, S, p0 = segment_case(scene, "rx")
    ones, zeros = np.ones((1,) + X.shape, F), np.zeros((1,) + X.shape, F)
    ph = WO.physics(cands, T, Rl, S, walls, p0, "received_power", HEIGHT, [0.0], ones, zeros, WO.AMP_LINEAR)
    got, params = _gpu(ctx, scene, "rx", "received_power", np.zeros(1, F), ones, zeros, "linear")
    ctx.set_cotangent(None)
    ctx.launch_vg(params, fixed, scene_vjp=True)
    _, objects_bar = ctx.get_scene_vjp()
    objects_bar = np.asarray(objects_bar, np.float64).reshape(len(walls), 2, 2)
    assert np.isfinite(objects_bar).all() and np.isfinite(got.walls_bar).all()
    mag = ph.mag.sum(axis=1)
    touched = mag > 0
    err = np.abs(got.walls_bar - objects_bar).max(axis=(1, 2))
    print(f"{scene}: worst |walls_bar - objects_bar| / magnitude = {(err[touched] / mag[touched]).max():.3g} over {touched.sum()} walls")
    assert touched.sum() >= 3 and (err[touched] <= 1e-5 * mag[touched]).all() and objects_bar[touched].any(axis=(1, 2)).all()
    assert (np.abs(objects_bar[~touched]) <= 1e-5 * mag.max()).all()


# ---- 5. state rules and refusals ---------------------------------------------------------------------------------------------------------
def test_state_rules_and_refusals(ctx):
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import make_params

    walls, fixed, X, Y = _case("random7")
    nf = 9
    inv = inv_list(nf)
    rb, ib = _bars("random7", nf)
    kw = dict(min_order=0, max_order=2, r_coef=0.5, height=HEIGHT)
    ok = make_params(fun="received_power", **kw)
    who = "d2d_field_walls_vjp_launch"

    def nothing_to_get():
        rc = ctx._lib.d2d_get_field_walls_vjp(ctx._ctx, None, None)
        return rc == -5 and who.encode() in ctx._lib.d2d_last_error()

    ctx.set_scene(walls)
    ctx.set_grid(*unit_grid(19, 11))  # a grid this context has not seen: no result yet
    ctx.set_grid(X, Y)
    assert nothing_to_get()
    with pytest.raises(L.D2DError, match=who) as e:
        ctx.get_field_walls_vjp()
    assert e.value.status == -5
    want = ctx.field_walls_vjp(ok, fixed, inv, rb, ib)
    assert want.normal_bar.any()
    # NULL outputs in any combination
    for mask in range(4):
        bufs = [np.full((7, 2, 2), 7, np.float64), np.full((7, 2), 7, np.float64)]
        args = [b.ctypes.data if mask >> i & 1 else None for i, b in enumerate(bufs)]
        assert ctx._lib.d2d_get_field_walls_vjp(ctx._ctx, *args) == 0
        for i, (b, w) in enumerate(zip(bufs, want)):
            assert np.array_equal(_bits(b), _bits(w)) if mask >> i & 1 else (b == 7).all()
    # the other results it must leave alone
    ctx.set_reflection_coefs(COEF7)
    per_object = make_params(fun="received_power_per_object", min_order=0, max_order=2, height=HEIGHT)
    fr = ctx.frequency_response(ok, fixed, inv_list(3))
    cg = ctx.field_coefs_vjp(per_object, fixed, inv, rb, ib)
    pg = ctx.field_position_vjp(ok, fixed, inv, rb, ib)
    ctx.launch(make_params(min_order=0, max_order=2), fixed)
    before = ctx.get_map()
    n0 = ctx.txg_fallbacks()
    assert np.array_equal(_bits(ctx.field_walls_vjp(ok, fixed, inv, rb, ib).normal_bar), _bits(want.normal_bar))

    def untouched():
        for a, b in zip(ctx.get_field_walls_vjp(), want):
            assert np.array_equal(_bits(a), _bits(b))
        assert np.array_equal(_bits(ctx.get_map()), _bits(before)) and before.any()
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(ctx.get_frequency_response(), fr)) and fr.re.any()
        assert np.array_equal(_bits(ctx.get_field_coefs_vjp()), _bits(cg)) and cg.any()
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(ctx.get_field_position_vjp(), pg)) and pg.fixed_bar.any()

    untouched()

    def refused(status, word, params, inv_=inv, amp="sqrt", bars_=(rb, ib)):
        with pytest.raises(L.D2DError, match=word) as e:
            ctx.field_walls_vjp(params, fixed, inv_, *bars_, amp)
        assert e.value.status == status, (e.value.status, str(e.value))
        assert isinstance(e.value, L.D2DUnsupported) == (status == -4)
        assert who in str(e.value)
        untouched()  # a refused launch leaves the previous result readable, and everything else as it was

    # a smoothed validity, with the reason
    for extra in (dict(approx=True, function="hard_sigmoid"), dict(approx=True, function="sigmoid")):
        refused(-4, "covers hard validity only: a smoothed validity .hard_sigmoid, sigmoid. depends on the walls' end points itself, and its "
                    "term needs the reverse chain of the value.grad sweep", make_params(fun="received_power", **extra, **kw))
    # everything the frequency response refuses
    refused(-4, "D2D_FUN_CUSTOM", make_params(fun="custom", min_order=0, max_order=2))
    for solver in ("min", "fermat"):
        refused(-4, "MinPath / FermatPath", make_params(fun="received_power", solver=solver, **kw))
    refused(-4, "D2D_OUT_ADD", make_params(fun="received_power", out_mode=L.OUT_ADD, **kw))
    refused(-4, "not culled", make_params(fun="received_power", grid_role=L.GRID_TX, tol=0.6, **kw))
    ctx.set_option("txg_exhaustive", 1)
    try:
        refused(-4, "txg_exhaustive", make_params(fun="received_power", grid_role=L.GRID_TX, **kw))
    finally:
        ctx.set_option("txg_exhaustive", 0)
    empty = np.zeros((0,) + X.shape, F)
    refused(-1, "the wall adjoint needs nf in 1 .. 1024, got 0", ok, inv_=np.zeros(0, F), bars_=(empty, empty))
    many = np.zeros((L.D2D_FREQ_MAX + 1,) + X.shape, F)
    refused(-1, "nf in 1 .. 1024, got 1025", ok, inv_=np.full(L.D2D_FREQ_MAX + 1, INV_20, F), bars_=(many, many))
    for at in (0, 8):  # in the first block and in the second: the message names the index
        for bad in (-1.0, float("nan"), float("inf")):
            v = inv.copy()
            v[at] = bad
            refused(-1, f"the wall adjoint needs a finite inv_wavelength >= 0, got .* at index {at}$", ok, inv_=v)
    for amp in (2, -1):
        refused(-1, "the wall adjoint's amplitude must be", ok, amp=amp)
    with pytest.raises(L.D2DError, match="amplitude") as e:  # (an unknown name is refused by the Python layer)
        ctx.field_walls_vjp(ok, fixed, inv, rb, ib, "power")
    assert e.value.status == -1
    with pytest.raises(L.D2DError, match="shape") as e:  # (... and so are cotangents of another shape)
        ctx.field_walls_vjp(ok, fixed, inv, rb[:3], ib[:3])
    assert e.value.status == -1
    # NULL cotangents (the Python layer always hands pointers: the library itself)
    keep = np.ascontiguousarray(inv)
    for a, b in ((None, ib.ctypes.data), (rb.ctypes.data, None), (None, None)):
        rc = ctx._lib.d2d_field_walls_vjp_launch(ctx._ctx, C.byref(ok), np.ascontiguousarray(fixed, F), keep.ctypes.data, nf, 0, a, b)
        assert rc == -1 and b"NULL argument" in ctx._lib.d2d_last_error()
    # per-object coefficients that are not set: D2D_ERR_STATE, as the sweeps answer
    ctx.set_reflection_coefs(None)
    with pytest.raises(L.D2DError, match="d2d_set_reflection_coefs") as e:
        ctx.field_walls_vjp(per_object, fixed, inv, rb, ib)
    assert e.value.status == -5
    for a, b in zip(ctx.get_field_walls_vjp(), want):
        assert np.array_equal(_bits(a), _bits(b))
    assert ctx.txg_fallbacks() == n0
    # non-finite cotangents are not refused: they propagate
    inf_bar = rb.copy()
    inf_bar[0] = np.inf
    assert not np.isfinite(ctx.field_walls_vjp(ok, fixed, inv, inf_bar, ib).normal_bar).all()
    # the library's constants are taken as well as the names; an accepted launch replaces the previous result
    a = ctx.field_walls_vjp(ok, fixed, inv, rb, ib, L.D2D_FIELD_AMP_LINEAR)
    b = ctx.field_walls_vjp(ok, fixed, inv, rb, ib, "linear")
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b)) and not np.array_equal(a.normal_bar, want.normal_bar)
    # another grid drops the result, and so does another scene
    ctx.set_grid(*unit_grid(19, 11))
    assert nothing_to_get()
    ctx.set_grid(X, Y)
    ctx.field_walls_vjp(ok, fixed, inv, rb, ib)
    assert not nothing_to_get()
    rng = np.random.default_rng(3)
    ctx.set_scene(rng.random((5, 2, 2)).astype(F))
    assert nothing_to_get()
    ctx.set_scene(rng.random((4096, 2, 2)).astype(F))  # 4 096 objects exceed the 12-bit wall indices
    with pytest.raises(L.D2DUnsupported, match="4096 objects") as e:
        ctx.field_walls_vjp(make_params(fun="received_power", min_order=0, max_order=1, r_coef=0.5, height=HEIGHT), fixed, inv, rb, ib)
    assert e.value.status == -4 and who in str(e.value) and nothing_to_get()
    ctx.set_scene(walls)


# ---- 6. the Scene methods and the wall-fitting loop --------------------------------------------------------------------------------------
@pytest.mark.parametrize("role", ["rx", "tx"])
def test_scene_methods_mirror_the_context(ctx, role):
    from differt2d_amd import utils
    from differt2d_amd.engine import make_params
    from differt2d_amd.geometry import Point, Wall
    from differt2d_amd.scene import Scene

    walls, fixed, X, Y = _case("random7")
    pts = {"a": Point(xy=fixed), "b": Point(xy=(F(1.0) - fixed).astype(F))}
    scene = Scene(objects=[Wall(xys=w) for w in walls])
    scene = scene.with_transmitters(**pts) if role == "rx" else scene.with_receivers(**pts)
    method = (scene.frequency_response_walls_vjp_on_receivers_grid if role == "rx"
              else scene.frequency_response_walls_vjp_on_transmitters_grid)
    nf = 9
    inv = inv_list(nf)
    rb, ib = _bars("random7", nf)
    rb2, ib2 = _bars("random7", nf, seed=2)
    common = dict(min_order=0, max_order=2, approx=False)
    fk = dict(r_coef=0.5, height=HEIGHT)
    got = dict(method(X, Y, utils.received_power, fk, rb, ib, inv_wavelengths=inv, **common))
    per = dict(method(X, Y, utils.received_power, fk, {"a": rb, "b": rb2}, {"a": ib, "b": ib2}, inv_wavelengths=inv, amplitude="linear", **common))
    assert list(got) == list(per) == ["a", "b"]  # one result per fixed end point, in order
    ctx.set_scene(walls)
    ctx.set_grid(X, Y)
    params = make_params(min_order=0, max_order=2, fun="received_power", grid_role=_role_id(role), **MODES["hard"], **fk)
    for name, pt in pts.items():
        want = ctx.field_walls_vjp(params, pt.xy, inv, rb, ib, "sqrt")
        assert all(np.array_equal(_bits(g), _bits(w)) for g, w in zip(got[name], want)) and want.normal_bar.any()
        pair = (rb, ib) if name == "a" else (rb2, ib2)
        assert all(np.array_equal(_bits(g), _bits(w)) for g, w in zip(per[name], ctx.field_walls_vjp(params, pt.xy, inv, *pair, "linear")))
    assert not np.array_equal(got["a"].normal_bar, got["b"].normal_bar) and not np.array_equal(got["a"].normal_bar, per["a"].normal_bar)
    ws = [0.05, 0.03, 0.07]  # wavelengths=[w] is inv_wavelengths=[float32(1) / float32(w)]
    by_w = dict(method(X, Y, utils.received_power, fk, rb[:3], ib[:3], wavelengths=ws, **common))
    by_inv = dict(method(X, Y, utils.received_power, fk, rb[:3], ib[:3], inv_wavelengths=F(1) / np.asarray(ws, F), **common))
    assert all(np.array_equal(_bits(by_w[k].normal_bar), _bits(by_inv[k].normal_bar)) for k in pts) and by_w["a"].normal_bar.any()
    # received_power_per_object with its coefficients: the objects' r_coef
    import dataclasses

    @dataclasses.dataclass(frozen=True, eq=False)
    class CoatedWall(Wall):
        r_coef: float = 0.5

    coated = Scene(objects=[CoatedWall(xys=w, r_coef=float(c)) for w, c in zip(walls, COEF7)])
    coated = coated.with_transmitters(**pts) if role == "rx" else coated.with_receivers(**pts)
    method = (coated.frequency_response_walls_vjp_on_receivers_grid if role == "rx"
              else coated.frequency_response_walls_vjp_on_transmitters_grid)
    (_, po), _ = method(X, Y, utils.received_power_per_object, dict(height=HEIGHT), rb, ib, inv_wavelengths=inv, **common)
    cands, T, Rl, S, p0 = segment_case("random7", role, "received_power_per_object")
    ph = WO.physics(cands, T, Rl, S, walls, p0, "received_power_per_object", HEIGHT, inv, rb, ib, WO.AMP_SQRT)
    assert (np.abs(po.normal_bar - ph.normal_bar) <= ph.bound).all() and po.normal_bar.any()


def test_wall_fitting_loop(ctx):
    """The loop of ``tests/test_field_walls_vjp_cpu.py`` through the ``Scene`` methods: the target is the GPU's frequency response with
    the wall where it belongs, every step is one forward call, ``utils.field_misfit`` and one adjoint call, at the fixed rate.  The
    misfit falls at every step and ends below 10 x the ratio the float64 oracle reached (``ORACLE_RATIO``; times 10 for fp32)."""
    from differt2d_amd import utils
    from differt2d_amd.geometry import Point, Wall
    from differt2d_amd.scene import Scene

    truth, walls, fixed, X, Y, inv = fitting_inputs()
    common = dict(min_order=0, max_order=2, approx=False)
    fk = dict(r_coef=0.5, height=HEIGHT)

    def forward(w):
        scene = Scene(objects=[Wall(xys=x) for x in w]).with_transmitters(tx=Point(xy=fixed))
        (_, fr), = scene.frequency_response_on_receivers_grid(X, Y, utils.received_power, fk, inv_wavelengths=inv, amplitude="linear", **common)
        return scene, fr

    target = utils.frequency_response(forward(truth)[1])
    losses = []
    for _ in range(FIT["steps"]):
        scene, fr = forward(walls)
        loss, rb, ib = utils.field_misfit(fr, target)
        losses.append(loss)
        (name, wg), = scene.frequency_response_walls_vjp_on_receivers_grid(X, Y, utils.received_power, fk, rb, ib, inv_wavelengths=inv,
                                                                           amplitude="linear", **common)
        assert name == "tx" and np.isfinite(wg.walls_bar).all()
        walls = walls.copy()
        walls[FIT["wall"]] = (walls[FIT["wall"]].astype(np.float64) - FIT["rate"] * wg.walls_bar[FIT["wall"]]).astype(F)
    losses.append(utils.field_misfit(forward(walls)[1], target)[0])
    print("misfit:", " ".join(f"{v:.4g}" for v in losses), "ratio", losses[-1] / losses[0], "wall", walls[FIT["wall"]].tolist())
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    assert losses[-1] <= 10 * ORACLE_RATIO * losses[0], losses[-1] / losses[0]
    assert np.abs(walls[FIT["wall"]] - truth[FIT["wall"]]).max() <= 0.02 * abs(FIT["shift"])


# ---- 7. many walls ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("role", ["rx", "tx"])
def test_seventy_walls_within_the_bound(ctx, role):
    """``random70`` of ``tests/many_walls_cases.py``: two chunks of last walls, wall indices at and past 64, 4 830 order-2 candidates
    (the culling queue flushes between prefixes), against the same oracle within the same bound."""
    import many_walls_cases as MW
    from differt2d_amd.engine import make_params

    name = "random70"
    walls, fixed, X, Y = MW.scene_of(name)
    inp = MW.inputs_of(name, "hard", role)
    nf = 9
    inv = inv_list(nf)
    rb, ib = bars(nf, X.shape, 3070)
    p0 = WO.first_point(fixed, X, Y, role)
    ph = WO.physics(inp.cands, inp.T, inp.Rl, inp.S, walls, p0, "received_power", MW.HEIGHT, inv, rb, ib, WO.AMP_SQRT)
    WO.guards(inp.cands, inp.T, ph)
    assert (ph.scale[64:] > 0).any()  # a wall of the second chunk carries bounces
    ctx.set_scene(walls)
    ctx.set_grid(X, Y)
    params = make_params(min_order=0, max_order=2, fun="received_power", grid_role=_role_id(role), **MODES["hard"], **MW.FUN_KW)
    got = ctx.field_walls_vjp(params, fixed, inv, rb, ib, "sqrt")
    _walls_bar_is_the_product(got, walls, name)
    err = np.abs(got.normal_bar - ph.normal_bar)
    touched = ph.scale > 0
    print(f"{name} {role}: worst error / bound = {(err[touched] / ph.bound[touched]).max():.3f} on {int(touched.sum())} touched walls")
    assert (err <= ph.bound).all() and not _bits(got.normal_bar[~touched]).any()
