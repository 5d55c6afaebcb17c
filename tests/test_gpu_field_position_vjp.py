"""The frequency response's position adjoint on the GPU (include/d2d.h: d2d_field_position_vjp_launch; power_sink_kernel,
PosGradSink): ``cell_bar`` and ``fixed_terms`` bit for bit against the NumPy restatement of ``tests/field_position_vjp_oracle.py``,
``fixed_bar`` against the float64 sum of the call's own planes, both within the derived bound of the float64 oracle, against the
value+grad sweep in the incoherent limit, its exact rules, its state rules and every refusal, the ``Scene`` methods and the
localisation loop of ``tests/test_field_position_vjp_cpu.py``."""

import ctypes as C
import functools

import numpy as np
import pytest

import field_position_vjp_oracle as PO
from conftest import unit_grid
from test_field_position_vjp_cpu import AMPS, HEIGHT, INV_20, LOC, bars, directed_case, inv_list, localisation_inputs
from test_gpu_strongest_paths import COEF7, MODES, _case, _role_id

pytestmark = pytest.mark.gpu

F = np.float32
RAGGED = (13, 19)  # the ragged grid of the adjoint tests: partial patches on both sides, lanes outside the grid in every patch row


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
    rb, ib = bars(nf, shape, 2000 + 31 * seed + nf)
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
        return ctx.field_position_vjp(params, fixed, inv, rb, ib, amp), params
    finally:
        if allowed is not None:
            ctx.set_candidate_mask(None)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64)


def _same_planes(got, want, shape, tag):
    """``cell_bar`` and ``fixed_terms`` of a :class:`PositionGradient` against the restatement's ``[cells, 2]`` planes, by bits."""
    for name, g, w in (("cell_bar", got.cell_bar, want.cell_bar), ("fixed_terms", got.fixed_terms, want.fixed_terms)):
        assert g.dtype == F and g.shape == tuple(shape) + (2,), (tag, name, g.dtype, g.shape)
        bad = _bits(g.reshape(-1, 2)) != _bits(w)
        assert not bad.any(), f"{tag} {name}: {bad.sum()} of {bad.size} entries differ, first at {tuple(np.argwhere(bad)[0])}"
    assert np.any(want.cell_bar) and np.any(want.fixed_terms), tag


def _fixed_bar_is_the_sum(got, tag):
    total, bound = PO.fixed_bar_bound(got.fixed_terms)
    assert got.fixed_bar.dtype == np.float64 and got.fixed_bar.shape == (2,)
    assert (np.abs(got.fixed_bar - total) <= bound).all(), (tag, got.fixed_bar, total, bound)


def _check(ctx, scene, role, fun, amp, nf, lo=0, hi=2, masked=(), grid=None):
    cands, T, Rl, D = directed_case(scene, role, fun, lo, hi, masked, grid)
    rb, ib = _bars(scene, nf, grid=grid)
    inv = inv_list(nf)
    want = PO.restate(T, Rl, D, fun, HEIGHT, inv, rb, ib, AMPS[amp], role)
    allowed = None
    if masked:
        allowed = np.ones(len(_case(scene)[0]), np.uint8)
        allowed[list(masked)] = 0
    got, _ = _gpu(ctx, scene, role, fun, inv, rb, ib, amp, lo, hi, allowed, grid)
    tag = f"{scene} {grid or ''} {role} {fun} {amp} nf={nf} orders {lo}-{hi} masked {masked}"
    _same_planes(got, want, grid_of(scene, grid)[2].shape, tag)
    _fixed_bar_is_the_sum(got, tag)
    return got, want


# ---- 1. bit for bit against the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", [1, 8, 9, 17])
@pytest.mark.parametrize("amp", ["sqrt", "linear"])
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("scene", ["obstacle", "random7"])
def test_planes_equal_the_restatement(ctx, scene, role, amp, nf):
    """nf: a partial block, a full one, a full one plus one, two plus one."""
    _check(ctx, scene, role, "received_power", amp, nf)


@pytest.mark.parametrize("amp", ["sqrt", "linear"])
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("fun", ["received_power_per_object", "length", "one", "length_squared"])
def test_planes_equal_the_restatement_for_every_fused_function(ctx, fun, role, amp):
    """``received_power_per_object`` with ``COEF7`` (a negative and a zero coefficient), ``length``, ``one`` -- and ``length_squared``,
    the fourth branch of ``rho``."""
    _check(ctx, "random7", role, fun, amp, 9)


@pytest.mark.parametrize("role", ["rx", "tx"])
def test_planes_equal_the_restatement_at_orders_0_to_3_and_under_a_mask(ctx, role):
    _check(ctx, "random7", role, "received_power", "sqrt", 9, 0, 3)
    everything = directed_case("random7", role)[1]
    masked = directed_case("random7", role, masked=(2, 5))[1]
    assert (~(everything == 0)).sum() > (~(masked == 0)).sum() > 0  # (the mask takes contributions away)
    _check(ctx, "random7", role, "received_power", "linear", 9, masked=(2, 5))


@pytest.mark.parametrize("nf", [8, 17])
@pytest.mark.parametrize("role", ["rx", "tx"])
def test_ragged_grid_no_clamped_lane_is_counted_or_written(ctx, role, nf):
    """13 x 19: every patch row and column ends in lanes outside the grid.  They evaluate a clamped copy of an edge cell; if one were
    written, an edge cell's planes would differ from the restatement (a block's pass would add its terms twice), and if one were
    counted, ``fixed_bar`` would differ from the sum of the planes."""
    _check(ctx, "random7", role, "received_power", "sqrt", nf, grid=RAGGED)


@pytest.mark.parametrize("role", ["rx", "tx"])
def test_a_cell_on_the_fixed_end_point_adds_nothing_there(ctx, role):
    """``square_centre``: the grid passes through the fixed end point; that cell's line of sight contributes (``t = 1 / h^2``) and has
    no direction at either end."""
    cands, T, Rl, D = directed_case("square_centre", role)
    _, _, ok = PO.unit_dir(D[0, :, 0], D[0, :, 1])
    assert (~(T[0] == 0) & ~ok).sum() == 1
    _check(ctx, "square_centre", role, "received_power", "sqrt", 9)


def test_header_on_the_device_equals_its_host_build(ctx):
    """d2d_posgrad.hpp on the device against the NumPy restatement (which the CPU test holds the g++ build to), every fun_id and both
    amplitudes over the generated list."""
    t, r, h2, inv, rb, ib = PO.header_inputs()
    for fun, fid in PO.FUN_IDS.items():
        for amp in ("sqrt", "linear"):
            got = ctx.selftest_posgrad(fid, amp, t, r, h2, inv, rb, ib)
            want = PO.header(fun, AMPS[amp], t, r, h2, inv, rb, ib)
            for name, g, w in zip("a rho kr g G".split(), got, want):
                both_nan = np.isnan(g) & np.isnan(w)
                bad = (_bits(g) != _bits(np.ascontiguousarray(w, F))) & ~both_nan
                assert not bad.any(), (fun, amp, name, int(bad.sum()), int(np.flatnonzero(bad)[0]))


# ---- 2. fixed_bar ------------------------------------------------------------------------------------------------------------------------
def test_fixed_bar_repeats_bit_for_bit_and_after_other_products(ctx):
    from differt2d_amd.engine import make_params

    nf = 17
    rb, ib = _bars("random7", nf)
    first, params = _gpu(ctx, "random7", "rx", "received_power", inv_list(nf), rb, ib, "sqrt")
    _fixed_bar_is_the_sum(first, "first")
    assert first.fixed_bar.all()
    again, _ = _gpu(ctx, "random7", "rx", "received_power", inv_list(nf), rb, ib, "sqrt")
    walls, fixed, X, Y = _case("random7")
    ctx.frequency_response(params, fixed, inv_list(3))
    ctx.strongest_paths(params, fixed, 3)
    ctx.launch(make_params(min_order=0, max_order=2), fixed)
    ctx.get_map()
    ctx.field_position_vjp(params, fixed, inv_list(2), rb[:2], ib[:2], "linear")  # (another call of the same product in between)
    third = ctx.field_position_vjp(params, fixed, inv_list(nf), rb, ib, "sqrt")
    for other in (again, third):
        for a, b in zip(first, other):
            assert np.array_equal(_bits(a), _bits(b))


# ---- 3. float64 physics ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("amp", ["sqrt", "linear"])
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("scene", ["obstacle", "random7"])
def test_planes_within_the_bound_of_the_float64_oracle(ctx, scene, role, amp):
    nf = 17
    cands, T, Rl, D = directed_case(scene, role)
    rb, ib = _bars(scene, nf)
    ph = PO.physics(T, Rl, D, "received_power", HEIGHT, inv_list(nf), rb, ib, AMPS[amp], role)
    PO.guards(T, Rl, D, role, ph)
    got, _ = _gpu(ctx, scene, role, "received_power", inv_list(nf), rb, ib, amp)
    worst = 0.0
    for e, (g, w) in enumerate(((got.cell_bar, ph.cell_bar), (got.fixed_terms, ph.fixed_terms))):
        err = np.abs(g.reshape(-1, 2).astype(np.float64) - w)
        lit = ph.bound[e] > 0
        assert (err <= ph.bound[e]).all(), (e, float((err[lit] / ph.bound[e][lit]).max()))
        assert not _bits(g.reshape(-1, 2)[~lit]).any()  # nothing reaches it: exactly +0.0
        worst = max(worst, float((err[lit] / ph.bound[e][lit]).max()))
    print(f"{scene} {role} {amp}: worst error / bound = {worst:.3f}, worst bound / magnitude = "
          f"{max(float((ph.bound[e][ph.mag[e] > 0] / ph.mag[e][ph.mag[e] > 0]).max()) for e in range(2)):.2e}")


# ---- 4. against the value+grad sweep in the incoherent limit -----------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["obstacle", "random7"])
def test_incoherent_limit_is_the_value_and_grad_sweep(ctx, scene):
    """LINEAR, ``inv = [0]``, ``re_bar = 1``, ``im_bar = 0``: ``re`` is the power map.  ``cell_bar`` on an RX grid agrees with
    ``get_grad_rx`` of the value+grad sweep (hard validity) within 1e-5 of the cell's gradient scale -- the summed term magnitude of
    the float64 oracle -- on every finite cell, and ``fixed_bar`` with its ``tx_bar`` for a cotangent of ones within the sum of the
    per-cell tolerances."""
    from differt2d_amd.engine import make_params

    walls, fixed, X, Y = _case(scene)
    cands, T, Rl, D = directed_case(scene, "rx")
    ones, zeros = np.ones((1,) + X.shape, F), np.zeros((1,) + X.shape, F)
    ph = PO.physics(T, Rl, D, "received_power", HEIGHT, [0.0], ones, zeros, PO.AMP_LINEAR, "rx")
    got, params = _gpu(ctx, scene, "rx", "received_power", np.zeros(1, F), ones, zeros, "linear")
    ctx.set_cotangent(None)
    ctx.launch_vg(params, fixed, scene_vjp=True)
    grad = ctx.get_grad_rx().reshape(-1, 2).astype(np.float64)
    tx_bar, _ = ctx.get_scene_vjp()
    finite = np.isfinite(grad).all(axis=1)
    assert finite.all(), int((~finite).sum())  # hard validity: every cell
    scale_c, scale_f = ph.mag[0].sum(axis=1), ph.mag[1].sum(axis=1)
    err = np.abs(got.cell_bar.reshape(-1, 2) - grad).max(axis=1)
    lit = scale_c > 0
    print(f"{scene}: worst |cell_bar - grad_rx| / scale = {(err[lit] / scale_c[lit]).max():.3g} over {lit.sum()} cells; "
          f"|fixed_bar - tx_bar| / tolerance = {(np.abs(got.fixed_bar - tx_bar) / (1e-5 * scale_f.sum())).max():.3g}")
    assert lit.sum() >= 0.5 * lit.size and (err <= 1e-5 * scale_c).all()
    assert (np.abs(got.fixed_bar - tx_bar.astype(np.float64)) <= 1e-5 * scale_f.sum()).all() and tx_bar.all()


# ---- 5. exact rules ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("role", ["rx", "tx"])
def test_exact_rules(ctx, role):
    scene = "random7"
    rb17, ib17 = (a.copy() for a in _bars(scene, 17))
    for nf in (8, 16):  # appending a wavelength whose planes are zero changes no bit: a new block, and one that crosses a block edge
        rb, ib = rb17[: nf + 1].copy(), ib17[: nf + 1].copy()
        rb[nf] = ib[nf] = 0
        short, _ = _gpu(ctx, scene, role, "received_power", inv_list(nf), rb[:nf], ib[:nf], "sqrt")
        more, _ = _gpu(ctx, scene, role, "received_power", inv_list(nf + 1), rb, ib, "sqrt")
        twice, _ = _gpu(ctx, scene, role, "received_power", inv_list(nf), 2 * rb[:nf], 2 * ib[:nf], "sqrt")
        zero, _ = _gpu(ctx, scene, role, "received_power", inv_list(nf), 0 * rb[:nf], F(-0.0) * ib[:nf], "sqrt")
        for s, m, t2, z in zip(short, more, twice, zero):
            assert s.any() and np.array_equal(_bits(s), _bits(m))
            assert np.array_equal(_bits(s.dtype.type(2) * s), _bits(t2))
            assert not _bits(z).any()  # +0.0 in every bit of all three outputs


@pytest.mark.parametrize("role", ["rx", "tx"])
def test_a_nan_cotangent_reaches_its_cell_and_fixed_bar_only(ctx, role):
    nf = 9
    cands, T, Rl, D = directed_case("obstacle", role)
    n = _case("obstacle")[2].shape[1]
    lit = np.flatnonzero((~(T == 0)).any(axis=0))
    cell = int(next((c for c in lit[::-1] if c % n == n - 1), lit[-1]))  # in the last column where there is one: a partial patch's edge
    rb, ib = (a.copy() for a in _bars("obstacle", nf))
    clean, _ = _gpu(ctx, "obstacle", role, "received_power", inv_list(nf), rb, ib, "linear")
    ib.reshape(nf, -1)[8, cell] = np.nan  # one cell, one plane, in the second block
    got, _ = _gpu(ctx, "obstacle", role, "received_power", inv_list(nf), rb, ib, "linear")
    others = np.arange(T.shape[1]) != cell
    for g, c in ((got.cell_bar, clean.cell_bar), (got.fixed_terms, clean.fixed_terms)):
        g, c = g.reshape(-1, 2), c.reshape(-1, 2)
        assert np.isnan(g[cell]).all() and np.isfinite(c).all()
        assert np.array_equal(_bits(g[others]), _bits(c[others]))
    assert np.isnan(got.fixed_bar).all() and np.isfinite(clean.fixed_bar).all()


# ---- 6. state rules and refusals ---------------------------------------------------------------------------------------------------------
def test_state_rules_and_refusals(ctx):
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import make_params

    walls, fixed, X, Y = _case("random7")
    nf = 9
    inv = inv_list(nf)
    rb, ib = _bars("random7", nf)
    kw = dict(min_order=0, max_order=2, r_coef=0.5, height=HEIGHT)
    ok = make_params(fun="received_power", **kw)
    who = "d2d_field_position_vjp_launch"

    def nothing_to_get():
        rc = ctx._lib.d2d_get_field_position_vjp(ctx._ctx, None, None, None)
        return rc == -5 and who.encode() in ctx._lib.d2d_last_error()

    ctx.set_scene(walls)
    ctx.set_grid(*unit_grid(19, 11))  # a grid this context has not seen: no result yet
    ctx.set_grid(X, Y)
    assert nothing_to_get()
    with pytest.raises(L.D2DError, match=who) as e:
        ctx.get_field_position_vjp()
    assert e.value.status == -5
    want = ctx.field_position_vjp(ok, fixed, inv, rb, ib)
    cands, T, Rl, D = directed_case("random7", "rx")
    _same_planes(want, PO.restate(T, Rl, D, "received_power", HEIGHT, inv, rb, ib, PO.AMP_SQRT, "rx"), X.shape, "state")
    # NULL outputs in any combination
    shape2 = (2,) + X.shape
    for mask in range(8):
        bufs = [np.full(shape2, 7, F), np.full(shape2, 7, F), np.full(2, 7, np.float64)]
        args = [b.ctypes.data if mask >> i & 1 else None for i, b in enumerate(bufs)]
        assert ctx._lib.d2d_get_field_position_vjp(ctx._ctx, *args) == 0
        for i, (b, w) in enumerate(zip(bufs, (np.moveaxis(want.cell_bar, -1, 0), np.moveaxis(want.fixed_terms, -1, 0), want.fixed_bar))):
            assert np.array_equal(_bits(b), _bits(np.ascontiguousarray(w))) if mask >> i & 1 else (b == 7).all()
    # the other results it must leave alone
    ctx.set_reflection_coefs(COEF7)
    per_object = make_params(fun="received_power_per_object", min_order=0, max_order=2, height=HEIGHT)
    fr = ctx.frequency_response(ok, fixed, inv_list(3))
    cg = ctx.field_coefs_vjp(per_object, fixed, inv, rb, ib)
    ctx.launch(make_params(min_order=0, max_order=2), fixed)
    before = ctx.get_map()
    n0 = ctx.txg_fallbacks()
    assert np.array_equal(_bits(ctx.field_position_vjp(ok, fixed, inv, rb, ib).fixed_bar), _bits(want.fixed_bar))

    def untouched():
        for a, b in zip(ctx.get_field_position_vjp(), want):
            assert np.array_equal(_bits(a), _bits(b))
        assert np.array_equal(_bits(ctx.get_map()), _bits(before)) and before.any()
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(ctx.get_frequency_response(), fr)) and fr.re.any()
        assert np.array_equal(_bits(ctx.get_field_coefs_vjp()), _bits(cg)) and cg.any()

    untouched()

    def refused(status, word, params, inv_=inv, amp="sqrt", bars_=(rb, ib)):
        with pytest.raises(L.D2DError, match=word) as e:
            ctx.field_position_vjp(params, fixed, inv_, *bars_, amp)
        assert e.value.status == status, (e.value.status, str(e.value))
        assert isinstance(e.value, L.D2DUnsupported) == (status == -4)
        assert who in str(e.value)
        untouched()  # a refused launch leaves the previous result readable, and everything else as it was

    # a smoothed validity, with the reason
    for extra in (dict(approx=True, function="hard_sigmoid"), dict(approx=True, function="sigmoid")):
        refused(-4, "covers hard validity only: a smoothed validity .hard_sigmoid, sigmoid. depends on the positions itself, and its term "
                    "needs the reverse chain of the value.grad sweep", make_params(fun="received_power", **extra, **kw))
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
    refused(-1, "the position adjoint needs nf in 1 .. 1024, got 0", ok, inv_=np.zeros(0, F), bars_=(empty, empty))
    many = np.zeros((L.D2D_FREQ_MAX + 1,) + X.shape, F)
    refused(-1, "nf in 1 .. 1024, got 1025", ok, inv_=np.full(L.D2D_FREQ_MAX + 1, INV_20, F), bars_=(many, many))
    for at in (0, 8):  # in the first block and in the second: the message names the index
        for bad in (-1.0, float("nan"), float("inf")):
            v = inv.copy()
            v[at] = bad
            refused(-1, f"the position adjoint needs a finite inv_wavelength >= 0, got .* at index {at}$", ok, inv_=v)
    for amp in (2, -1):
        refused(-1, "the position adjoint's amplitude must be", ok, amp=amp)
    with pytest.raises(L.D2DError, match="amplitude") as e:  # (an unknown name is refused by the Python layer)
        ctx.field_position_vjp(ok, fixed, inv, rb, ib, "power")
    assert e.value.status == -1
    with pytest.raises(L.D2DError, match="shape") as e:  # (... and so are cotangents of another shape)
        ctx.field_position_vjp(ok, fixed, inv, rb[:3], ib[:3])
    assert e.value.status == -1
    # NULL cotangents (the Python layer always hands pointers: the library itself)
    keep = np.ascontiguousarray(inv)
    for a, b in ((None, ib.ctypes.data), (rb.ctypes.data, None), (None, None)):
        rc = ctx._lib.d2d_field_position_vjp_launch(ctx._ctx, C.byref(ok), np.ascontiguousarray(fixed, F), keep.ctypes.data, nf, 0, a, b)
        assert rc == -1 and b"NULL argument" in ctx._lib.d2d_last_error()
    # per-object coefficients that are not set: D2D_ERR_STATE, as the sweeps answer
    ctx.set_reflection_coefs(None)
    with pytest.raises(L.D2DError, match="d2d_set_reflection_coefs") as e:
        ctx.field_position_vjp(per_object, fixed, inv, rb, ib)
    assert e.value.status == -5
    for a, b in zip(ctx.get_field_position_vjp(), want):
        assert np.array_equal(_bits(a), _bits(b))
    assert ctx.txg_fallbacks() == n0
    # non-finite cotangents are not refused: they propagate
    inf_bar = rb.copy()
    inf_bar[0] = np.inf
    assert not np.isfinite(ctx.field_position_vjp(ok, fixed, inv, inf_bar, ib).fixed_bar).all()
    # the library's constants are taken as well as the names; an accepted launch replaces the previous result
    a = ctx.field_position_vjp(ok, fixed, inv, rb, ib, L.D2D_FIELD_AMP_LINEAR)
    b = ctx.field_position_vjp(ok, fixed, inv, rb, ib, "linear")
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b)) and not np.array_equal(a.cell_bar, want.cell_bar)
    # another grid drops the result, and so does another scene
    ctx.set_grid(*unit_grid(19, 11))
    assert nothing_to_get()
    ctx.set_grid(X, Y)
    ctx.field_position_vjp(ok, fixed, inv, rb, ib)
    assert not nothing_to_get()
    rng = np.random.default_rng(3)
    ctx.set_scene(rng.random((5, 2, 2)).astype(F))
    assert nothing_to_get()
    ctx.set_scene(rng.random((4096, 2, 2)).astype(F))  # 4 096 objects exceed the 12-bit wall indices
    with pytest.raises(L.D2DUnsupported, match="4096 objects") as e:
        ctx.field_position_vjp(make_params(fun="received_power", min_order=0, max_order=1, r_coef=0.5, height=HEIGHT), fixed, inv, rb, ib)
    assert e.value.status == -4 and who in str(e.value) and nothing_to_get()
    ctx.set_scene(walls)


# ---- 7. the Scene methods and the localisation loop --------------------------------------------------------------------------------------
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
    method = (scene.frequency_response_position_vjp_on_receivers_grid if role == "rx"
              else scene.frequency_response_position_vjp_on_transmitters_grid)
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
        want = ctx.field_position_vjp(params, pt.xy, inv, rb, ib, "sqrt")
        assert all(np.array_equal(_bits(g), _bits(w)) for g, w in zip(got[name], want)) and want.fixed_bar.any()
        pair = (rb, ib) if name == "a" else (rb2, ib2)
        assert all(np.array_equal(_bits(g), _bits(w)) for g, w in zip(per[name], ctx.field_position_vjp(params, pt.xy, inv, *pair, "linear")))
    assert not np.array_equal(got["a"].cell_bar, got["b"].cell_bar) and not np.array_equal(got["a"].cell_bar, per["a"].cell_bar)
    ws = [0.05, 0.03, 0.07]  # wavelengths=[w] is inv_wavelengths=[float32(1) / float32(w)]
    by_w = dict(method(X, Y, utils.received_power, fk, rb[:3], ib[:3], wavelengths=ws, **common))
    by_inv = dict(method(X, Y, utils.received_power, fk, rb[:3], ib[:3], inv_wavelengths=F(1) / np.asarray(ws, F), **common))
    assert all(np.array_equal(_bits(by_w[k].cell_bar), _bits(by_inv[k].cell_bar)) for k in pts) and by_w["a"].cell_bar.any()
    # received_power_per_object with its coefficients: the objects' r_coef
    import dataclasses

    @dataclasses.dataclass(frozen=True, eq=False)
    class CoatedWall(Wall):
        r_coef: float = 0.5

    coated = Scene(objects=[CoatedWall(xys=w, r_coef=float(c)) for w, c in zip(walls, COEF7)])
    coated = coated.with_transmitters(**pts) if role == "rx" else coated.with_receivers(**pts)
    method = (coated.frequency_response_position_vjp_on_receivers_grid if role == "rx"
              else coated.frequency_response_position_vjp_on_transmitters_grid)
    (_, po), _ = method(X, Y, utils.received_power_per_object, dict(height=HEIGHT), rb, ib, inv_wavelengths=inv, **common)
    cands, T, Rl, D = directed_case("random7", role, "received_power_per_object")
    _same_planes(po, PO.restate(T, Rl, D, "received_power_per_object", HEIGHT, inv, rb, ib, PO.AMP_SQRT, role), X.shape, f"scene {role} per object")


def test_localisation_loop(ctx):
    """The loop of ``tests/test_field_position_vjp_cpu.py`` through the ``Scene`` methods: the target is the GPU's frequency response
    at the displaced transmitter, every step is one forward call, ``utils.field_misfit`` and one adjoint call, at the fixed rate.
    The misfit falls at every step and ends below ``LOC["gpu_fraction"]`` of its start."""
    from differt2d_amd import utils
    from differt2d_amd.geometry import Point, Wall
    from differt2d_amd.scene import Scene

    walls, X, Y, inv, truth, pos = localisation_inputs()
    common = dict(min_order=0, max_order=2, approx=False)
    fk = dict(r_coef=0.5, height=HEIGHT)
    objects = [Wall(xys=w) for w in walls]

    def forward(xy):
        scene = Scene(objects=objects).with_transmitters(tx=Point(xy=xy))
        (_, fr), = scene.frequency_response_on_receivers_grid(X, Y, utils.received_power, fk, inv_wavelengths=inv, amplitude="linear", **common)
        return scene, fr

    target = utils.frequency_response(forward(truth)[1])
    losses = []
    for _ in range(LOC["steps"]):
        scene, fr = forward(pos)
        loss, rb, ib = utils.field_misfit(fr, target)
        losses.append(loss)
        (name, pg), = scene.frequency_response_position_vjp_on_receivers_grid(X, Y, utils.received_power, fk, rb, ib, inv_wavelengths=inv,
                                                                              amplitude="linear", **common)
        assert name == "tx" and np.isfinite(pg.fixed_bar).all()
        pos = (pos.astype(np.float64) - LOC["rate"] * pg.fixed_bar).astype(F)
    losses.append(utils.field_misfit(forward(pos)[1], target)[0])
    print("misfit:", " ".join(f"{v:.4g}" for v in losses), "position", pos, "truth", truth)
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    assert losses[-1] <= LOC["gpu_fraction"] * losses[0], losses[-1] / losses[0]
    assert np.abs(pos - truth).max() < 1e-4
