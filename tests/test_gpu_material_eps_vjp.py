"""The permittivity adjoint of the material response (include/d2d.h: d2d_material_eps_vjp_launch; power_sink_kernel, EpsGradSink):
``eps_bar[f, w] = dL/dRe eps[f, w] + j dL/dIm eps[f, w]`` for ``dL = sum (re_bar * d re + im_bar * d im)``.  A sum over cells, so it
is held to the float64 oracle of ``tests/material_eps_vjp_oracle.py`` within that module's derived bound per entry and component
(never relative to ``|eps_bar|``: gradients cancel), to the rules that ARE exact (same bits run to run, zero and doubled cotangents,
rows alone, the constant band), to its NaN rule, its state rules and refusals, through the Scene methods, and in a calibration loop.
Scenes and grids are those of ``tests/test_gpu_strongest_paths.py``; the wavelength lists are the forward tests' ``inv_list(nf)``;
the permittivities are lossy, different per wall and row; cotangents are seeded standard normals.  Every comparison first asserts the
oracle's guards (``material_eps_vjp_oracle.guards``)."""

import dataclasses
import functools

import numpy as np
import pytest

import material_eps_vjp_oracle as EO
import material_response_oracle as MO
from conftest import unit_grid
from test_gpu_strongest_paths import MODES, _case as _case3, _role_id
from test_material_eps_vjp_cpu import eps_table, run_header

pytestmark = pytest.mark.gpu

F = np.float32
AMPS = {"sqrt": EO.AMP_SQRT, "linear": EO.AMP_LINEAR}
POLS = {"te": MO.POL_TE, "tm": MO.POL_TM}
NF_MAX = 17


def inv_list(nf):
    return (F(20) * (F(1) + np.arange(nf, dtype=F) / F(64))).astype(F)


@pytest.fixture(scope="module")
def ctx():
    from differt2d_amd.engine import Context

    with Context(0) as c:
        yield c


@functools.lru_cache(maxsize=None)
def _case(scene):
    """(walls, fixed end point, X, Y): the strongest-paths cases, and random7 on a 13 x 19 grid whose ragged patches have clamped
    lanes on both sides."""
    if scene == "random7_13x19":
        walls, fixed, _, _ = _case3("random7")
        return walls, fixed, *unit_grid(13, 19)
    return _case3(scene)


@functools.lru_cache(maxsize=None)
def _contributions(scene, mode, role, lo=0, hi=2, masked=()):
    walls, fixed, X, Y = _case(scene)
    out = MO.segment_contributions(walls, fixed, X, Y, min_order=lo, max_order=hi, grid_role=role, filter_nodes=set(masked) or None, **MODES[mode])
    assert not np.isnan(out[1]).any()
    for a in out[1:]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _bars(scene, nf, seed=0):
    shape = _case(scene)[2].shape
    rng = np.random.default_rng(2000 + 31 * seed + nf)
    rb, ib = rng.standard_normal((nf,) + shape).astype(F), rng.standard_normal((nf,) + shape).astype(F)
    rb.setflags(write=False)
    ib.setflags(write=False)
    return rb, ib


def _eps(scene, nf):
    return eps_table(NF_MAX, len(_case(scene)[0]))[:nf]


@functools.lru_cache(maxsize=None)
def _oracle(scene, mode, role, pol, amp, nf, lo=0, hi=2, masked=()):
    """Computed once per case and shared; the guards are asserted here, in front of every comparison."""
    walls = _case(scene)[0]
    con = _contributions(scene, mode, role, lo, hi, masked)
    eg = EO.eps_grad(*con, MO.wall_normals(walls), inv_list(nf), _eps(scene, nf), *_bars(scene, nf), POLS[pol], AMPS[amp])
    EO.guards(eg, con[0], need_repeat=hi >= 3)
    return eg


def _params(mode, role, lo=0, hi=2, **extra):
    from differt2d_amd.engine import make_params

    return make_params(min_order=lo, max_order=hi, grid_role=_role_id(role), **MODES[mode], **extra)


def _gpu(ctx, scene, mode, role, inv, eps, rb, ib, pol, amp, lo=0, hi=2, allowed=None):
    walls, fixed, X, Y = _case(scene)
    ctx.set_scene(walls)
    if allowed is not None:
        ctx.set_candidate_mask(allowed)
    ctx.set_grid(X, Y)
    params = _params(mode, role, lo, hi)
    try:
        return ctx.material_eps_vjp(params, fixed, inv, eps, rb, ib, pol, amp), params
    finally:
        if allowed is not None:
            ctx.set_candidate_mask(None)


def _bits(a):
    return np.ascontiguousarray(a, np.complex128).view(np.uint64)


def _within(got, eg, tag):
    assert got.dtype == np.complex128 and got.shape == eg.eps_bar.shape, (got.dtype, got.shape)
    lit = eg.mag > 0
    err = np.maximum(np.abs(got.real - eg.eps_bar.real), np.abs(got.imag - eg.eps_bar.imag))
    with np.errstate(divide="ignore", invalid="ignore"):
        print(f"{tag}: walls {np.flatnonzero(lit.any(axis=0)).tolist()}, max err / bound {np.max(err[lit] / eg.bound[lit]):.3f}, "
              f"max bound / mag {np.max(eg.bound[lit] / eg.mag[lit]):.2e}, min |eps_bar| / mag {np.min(np.abs(eg.eps_bar[lit]) / eg.mag[lit]):.1e}")
    EO.within(got, eg)
    assert not _bits(got[~lit]).any(), (tag, got[~lit])  # untouched walls: exactly (+0.0, +0.0)


# ---- 1. against the float64 oracle, within its bound ---------------------------------------------------------------------------
@pytest.mark.parametrize("nf", [1, 8, 9, 17])
@pytest.mark.parametrize("amp", ["sqrt", "linear"])
@pytest.mark.parametrize("pol", ["te", "tm"])
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
@pytest.mark.parametrize("scene", ["obstacle", "random7"])
def test_gradient_within_the_oracle_bound(ctx, scene, mode, role, pol, amp, nf):
    """nf: a partial chunk, a full chunk, a full chunk plus one, two full chunks plus one."""
    eg = _oracle(scene, mode, role, pol, amp, nf)
    got, _ = _gpu(ctx, scene, mode, role, inv_list(nf), _eps(scene, nf), *_bars(scene, nf), pol, amp)
    _within(got, eg, f"{scene} {mode} {role} {pol} {amp} nf={nf}")


@pytest.mark.parametrize("pol", ["te", "tm"])
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
def test_ragged_grid_counts_no_lane_twice(ctx, mode, role, pol):
    """13 x 19: the last patch of every row and column has clamped lanes, which evaluate a copy of an edge cell."""
    eg = _oracle("random7_13x19", mode, role, pol, "sqrt", 9)
    got, _ = _gpu(ctx, "random7_13x19", mode, role, inv_list(9), _eps("random7_13x19", 9), *_bars("random7_13x19", 9), pol, "sqrt")
    _within(got, eg, f"random7 13 x 19 {mode} {role} {pol}")


@pytest.mark.parametrize("pol", ["te", "tm"])
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
def test_repeated_walls_at_order_three(ctx, mode, role, pol):
    """The square with the fixed end point at its centre, orders 0-3 (the MAXK = 3 instance): candidates (a, b, a) contribute, so a
    wall receives two terms of one candidate (the oracle's guard asserts that such a candidate contributes)."""
    eg = _oracle("square_centre", mode, role, pol, "linear", 9, 0, 3)
    got, _ = _gpu(ctx, "square_centre", mode, role, inv_list(9), _eps("square_centre", 9), *_bars("square_centre", 9), pol, "linear", 0, 3)
    _within(got, eg, f"square_centre {mode} {role} {pol} orders 0-3")


@pytest.mark.parametrize("role", ["rx", "tx"])
def test_gradient_honours_min_order_and_the_candidate_mask(ctx, role):
    rb, ib = _bars("random7", 9)
    eps = _eps("random7", 9)
    # min_order = 1 (the line of sight holds no coefficient: the same gradient as with it, from a sweep without it)
    eg = _oracle("random7", "hsig", role, "te", "linear", 9, 1, 2)
    got, _ = _gpu(ctx, "random7", "hsig", role, inv_list(9), eps, rb, ib, "te", "linear", 1, 2)
    _within(got, eg, f"random7 hsig {role} min_order=1")
    # a candidate mask: walls 2 and 5 are out, wall 2 carries terms without the mask and none with it
    allowed = np.ones(7, np.uint8)
    allowed[[2, 5]] = 0
    eg = _oracle("random7", "hard", role, "te", "linear", 9, 0, 2, (2, 5))
    everything = _oracle("random7", "hard", role, "te", "linear", 9)
    assert (everything.mag[:, 2] > 0).all() and not eg.mag[:, 2].any()
    got, _ = _gpu(ctx, "random7", "hard", role, inv_list(9), eps, rb, ib, "te", "linear", allowed=allowed)
    _within(got, eg, f"random7 hard {role} masked")


# ---- 2. what is exact ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
def test_exact_rules(ctx, mode, role):
    from differt2d_amd.engine import make_params

    nf = NF_MAX
    inv = inv_list(nf)
    eps = _eps("obstacle", nf)
    rb, ib = _bars("obstacle", nf)
    eg = _oracle("obstacle", mode, role, "tm", "sqrt", nf)
    got, params = _gpu(ctx, "obstacle", mode, role, inv, eps, rb, ib, "tm", "sqrt")
    _within(got, eg, f"obstacle {mode} {role} tm sqrt")
    fixed = _case("obstacle")[1]
    run = lambda *a: ctx.material_eps_vjp(params, fixed, *a, "tm", "sqrt")
    # two launches give the same bits, also after other products ran on the same context
    assert np.array_equal(_bits(run(inv, eps, rb, ib)), _bits(got))
    ctx.frequency_response(make_params(min_order=0, max_order=1, **MODES[mode]), fixed, inv[:3], "linear")
    ctx.material_response(params, fixed, inv[:3], eps[:3], "te", "linear")
    assert np.array_equal(_bits(ctx.get_material_eps_vjp()), _bits(got))  # the result is still there ...
    assert np.array_equal(_bits(run(inv, eps, rb, ib)), _bits(got))
    # zero cotangents: all +0.0
    zero = np.zeros_like(rb)
    assert not _bits(run(inv, eps, zero, zero)).any()
    # doubled cotangents: exactly doubled
    twice = run(inv, eps, F(2) * rb, F(2) * ib)
    assert np.array_equal(_bits(twice), _bits(2.0 * got)) and got.any()
    # max_order = 0: the line of sight holds no coefficient
    los = ctx.material_eps_vjp(_params(mode, role, 0, 0), fixed, inv, eps, rb, ib, "tm", "sqrt")
    assert los.shape == got.shape and not _bits(los).any()
    # row f depends on inv[f], eps[f] and the cotangent planes f alone: the list reversed across the chunk borders gives the rows reversed
    back = run(inv[::-1], eps[::-1], rb[::-1], ib[::-1])
    assert np.array_equal(_bits(back), _bits(got[::-1]))
    # ... and a chunk's rows alone are the rows of the whole
    for lo, hi in ((0, 8), (8, 16), (16, 17), (3, 4)):
        alone = run(inv[lo:hi], eps[lo:hi], rb[lo:hi], ib[lo:hi])
        assert np.array_equal(_bits(alone), _bits(got[lo:hi])) and alone.any(), (lo, hi)
    # the constant band (one row for the band: the factors formed once per contribution) equals the per-row route's rows bit for bit:
    # a table whose first 8 rows are equal and whose ninth differs is not constant
    mixed = np.concatenate([np.broadcast_to(eps[0], (8, eps.shape[1])), eps[8:9]])
    per_row = run(inv[:9], mixed, rb[:9], ib[:9])
    band = run(inv[:8], eps[0], rb[:8], ib[:8])
    assert band.shape == (8, eps.shape[1]) and np.array_equal(_bits(band), _bits(per_row[:8])) and band.any()
    assert np.array_equal(_bits(per_row[8]), _bits(got[8]))
    assert np.array_equal(_bits(run(inv[:8], np.broadcast_to(eps[0], (8, eps.shape[1])), rb[:8], ib[:8])), _bits(band))


@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
def test_a_nan_cotangent_reaches_row_f_of_the_walls_of_that_cells_candidates_only(ctx, mode, role):
    nf = 9
    eg = _oracle("obstacle", mode, role, "te", "linear", nf)
    cands = _contributions("obstacle", mode, role)[0]
    lit = np.flatnonzero(eg.mag.any(axis=0))
    walls_of = {}
    for ci, go in eg.touched.items():
        for cell in np.flatnonzero(go):
            walls_of.setdefault(int(cell), set()).update(int(o) for o in cands[ci])
    # a cell whose candidates touch some of the walls that have a gradient, not all of them (the last column where there is one:
    # a partial patch's edge, which the lanes outside the grid copy)
    n = _case("obstacle")[2].shape[1]
    some = [c for c, ws in sorted(walls_of.items()) if 0 < len(ws) < len(lit)]
    assert some
    cell = next((c for c in some if c % n == n - 1), some[0])
    rb, ib = (a.copy() for a in _bars("obstacle", nf))
    eps = _eps("obstacle", nf)
    clean, _ = _gpu(ctx, "obstacle", mode, role, inv_list(nf), eps, rb, ib, "te", "linear")
    ib.reshape(nf, -1)[8, cell] = np.nan  # in the second chunk
    got, _ = _gpu(ctx, "obstacle", mode, role, inv_list(nf), eps, rb, ib, "te", "linear")
    hit = np.zeros(clean.shape, bool)
    hit[8, sorted(walls_of[cell])] = True
    print(f"{mode} {role}: cell {cell}, NaN walls {sorted(walls_of[cell])} of {lit.tolist()}")
    assert np.isnan(got.real[hit]).all() and np.isnan(got.imag[hit]).all() and np.isfinite(clean).all()
    assert np.array_equal(_bits(got[~hit]), _bits(clean[~hit]))


# ---- 3. the derivative's header on the device -----------------------------------------------------------------------------------
def test_selftest_fresnel_grad_equals_the_host_build(ctx, tmp_path):
    """d2d_selftest_fresnel_grad over the forward header's input list: the device's fresnel_grad equals the g++ build's bits."""
    import os
    import subprocess

    from test_material_eps_vjp_cpu import GXX, SRC

    exe = str(tmp_path / "material_eps_vjp_host")
    subprocess.check_call(GXX + ["-o", exe, SRC])
    er, ei, c = MO.fresnel_inputs()
    host = run_header(exe, tmp_path, er, ei, c)
    assert os.path.exists(exe) and er.size > 60000
    for k, pol in enumerate(("te", "tm")):
        gr, gi, dr, di, ok = ctx.selftest_fresnel_grad(er, ei, c, pol)
        for name, g, w in zip(("gr", "gi", "dr", "di"), (gr, gi, dr, di), host[k, :4]):
            same = MO.same_bits(g, w)
            assert same.all(), (pol, name, int((~same).sum()), int(np.flatnonzero(~same)[0]))
        assert np.array_equal(ok, host[k, 4] != 0) and not ok.all() and np.isnan(dr).any()


# ---- 4. state rules and refusals ----------------------------------------------------------------------------------------------------
def test_state_rules_and_refusals(ctx):
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import make_params

    walls, fixed, X, Y = _case("random7")
    nf = 9
    inv, eps = inv_list(nf), _eps("random7", nf)
    rb, ib = _bars("random7", nf)
    kw = dict(min_order=0, max_order=2)
    ok = make_params(**kw)

    def nothing_to_get():
        rc = ctx._lib.d2d_get_material_eps_vjp(ctx._ctx, None)
        return rc == -5 and b"d2d_material_eps_vjp_launch" in ctx._lib.d2d_last_error()

    ctx.set_scene(walls)
    ctx.set_reflection_coefs(None)
    ctx.set_grid(*unit_grid(19, 11))  # a grid this context has not seen: no result yet
    ctx.set_grid(X, Y)
    assert nothing_to_get()
    with pytest.raises(L.D2DError) as e:
        ctx.get_material_eps_vjp()
    assert e.value.status == -5
    want = ctx.material_eps_vjp(ok, fixed, inv, eps, rb, ib)
    _within(want, _oracle("random7", "hard", "rx", "te", "sqrt", nf), "random7 hard rx te sqrt")
    # the forward product's and the coefficient adjoint's results are not touched by this launch, nor this one by theirs
    fwd = ctx.material_response(ok, fixed, inv[:3], eps[:3], "tm", "linear")
    ctx.set_reflection_coefs(np.full(7, 0.5, F))
    per_object = make_params(fun="received_power_per_object", height=0.25, **kw)
    cv = ctx.field_coefs_vjp(per_object, fixed, inv, rb, ib)
    assert np.array_equal(_bits(ctx.get_material_eps_vjp()), _bits(want))
    assert np.array_equal(_bits(ctx.material_eps_vjp(ok, fixed, inv, eps, rb, ib)), _bits(want))
    again = ctx.get_material_response()
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(again, fwd)) and fwd.re.any()
    assert np.array_equal(ctx.get_field_coefs_vjp(), cv) and cv.any()
    ctx.set_reflection_coefs(None)
    ctx.launch(ok, fixed)
    before = ctx.get_map()
    n0 = ctx.txg_fallbacks()

    def refused(status, word, params=ok, inv=inv, eps=eps, pol="te", amp="sqrt", bars=(rb, ib)):
        with pytest.raises(L.D2DError, match=word) as e:
            ctx.material_eps_vjp(params, fixed, inv, eps, *bars, pol, amp)
        assert e.value.status == status, (e.value.status, str(e.value))
        assert isinstance(e.value, L.D2DUnsupported) == (status == -4)
        # a refused launch leaves the previous result readable, and the value map as it was
        assert np.array_equal(_bits(ctx.get_material_eps_vjp()), _bits(want))
        assert np.array_equal(ctx.get_map().view(np.uint32), before.view(np.uint32)) and before.any()
        return str(e.value)

    # everything material_response refuses, with its messages under the new prefix
    assert "d2d_material_eps_vjp_launch" in refused(-4, "sigmoid", make_params(approx=True, function="sigmoid", **kw))
    for solver in ("min", "fermat"):
        assert "d2d_material_eps_vjp_launch" in refused(-4, "MinPath / FermatPath", make_params(solver=solver, **kw))
    assert "d2d_material_eps_vjp_launch" in refused(-4, "D2D_FUN_CUSTOM", make_params(fun="custom", **kw))
    assert "d2d_material_eps_vjp_launch" in refused(-4, "D2D_OUT_ADD", make_params(out_mode=L.OUT_ADD, **kw))
    refused(-5, "d2d_set_reflection_coefs", per_object)
    assert "d2d_material_eps_vjp_launch" in refused(-4, "not culled", make_params(grid_role=L.GRID_TX, tol=0.6, **kw))
    ctx.set_option("txg_exhaustive", 1)
    try:
        refused(-4, "txg_exhaustive", make_params(grid_role=L.GRID_TX, **kw))
    finally:
        ctx.set_option("txg_exhaustive", 0)
    empty = np.zeros((0,) + X.shape, F)
    refused(-1, "d2d_material_eps_vjp_launch: .*nf in 1 .. 1024", inv=np.zeros(0, F), eps=eps[0], bars=(empty, empty))
    many = np.zeros((L.D2D_FREQ_MAX + 1,) + X.shape, F)
    refused(-1, "nf in 1 .. 1024", inv=np.full(L.D2D_FREQ_MAX + 1, 20.0, F), eps=eps[0], bars=(many, many))
    for at in (0, 8):
        for bad in (-1.0, float("nan"), float("inf")):
            b = inv.copy()
            b[at] = bad
            refused(-1, f"d2d_material_eps_vjp_launch: .*inv_wavelength.* at index {at}$", inv=b)
    for amp in (2, -1):
        refused(-1, "amplitude", amp=amp)
    for pol in (2, -1):
        refused(-1, "the material response's polarization", pol=pol)
    refused(-1, "n_objects", eps=eps_table(nf, 6))
    refused(-1, "n_objects", eps=eps_table(nf, 8))
    for f, w in ((0, 0), (7, 6), (8, 3)):
        for bad in (np.nan, np.inf, 2.0**51):
            b = eps.copy()
            b[f, w] = complex(bad, b[f, w].imag)
            refused(-1, f"permittivity.* at wavelength index {f}, wall index {w}$", eps=b)
        b = eps.copy()
        b[f, w] = b[f, w].real + 0.25j
        refused(-1, f"d2d_material_eps_vjp_launch: the material response needs Im eps <= 0.* at wavelength index {f}, wall index {w}$", eps=b)
    # NULL arguments: the list, the table and either cotangent (the adjoint's checks)
    table = np.ascontiguousarray(eps).view(F)
    ptrs = [inv.ctypes.data, table.ctypes.data, rb.ctypes.data, ib.ctypes.data]
    for k in range(4):
        p = list(ptrs)
        p[k] = None
        rc = ctx._lib.d2d_material_eps_vjp_launch(ctx._ctx, ok, np.ascontiguousarray(fixed, F), p[0], nf, 0, 0, p[1], 7, p[2], p[3])
        assert rc == -1 and b"NULL" in ctx._lib.d2d_last_error(), k
    assert ctx._lib.d2d_get_material_eps_vjp(ctx._ctx, None) == -1 and b"eps_bar is NULL" in ctx._lib.d2d_last_error()
    assert np.array_equal(_bits(ctx.get_material_eps_vjp()), _bits(want))
    # the Python layer refuses unknown names and shapes ahead of the library
    for call in (lambda: ctx.material_eps_vjp(ok, fixed, inv, eps, rb, ib, "circular"), lambda: ctx.material_eps_vjp(ok, fixed, inv, eps, rb, ib, "te", "power"),
                 lambda: ctx.material_eps_vjp(ok, fixed, inv, eps[:3], rb, ib), lambda: ctx.material_eps_vjp(ok, fixed, inv, eps, rb[:3], ib[:3])):
        with pytest.raises(L.D2DError) as e:
            call()
        assert e.value.status == -1
    assert np.array_equal(_bits(ctx.get_material_eps_vjp()), _bits(want))
    assert ctx.txg_fallbacks() == n0
    # any fused fun is accepted (the amplitude does not depend on eps); non-finite cotangents propagate; the limits pass
    for fun in ("one", "length", "length_squared"):
        assert np.isfinite(ctx.material_eps_vjp(make_params(fun=fun, **kw), fixed, inv, eps, rb, ib)).all()
    inf_bar = rb.copy()
    inf_bar[0] = np.inf
    assert not np.isfinite(ctx.material_eps_vjp(ok, fixed, inv, eps, inf_bar, ib)).all()
    edge = eps.copy()
    edge[0, 0] = 2.0**50 - 2.0**50 * 1j
    edge[1, 1] = 3 + 0j
    assert np.isfinite(ctx.material_eps_vjp(ok, fixed, inv, edge, rb, ib, L.D2D_POL_TM, L.D2D_FIELD_AMP_LINEAR)).all()
    # another grid drops the result, and so does another scene
    ctx.set_grid(*unit_grid(19, 11))
    assert nothing_to_get()
    ctx.set_grid(X, Y)
    ctx.material_eps_vjp(ok, fixed, inv, eps, rb, ib)
    assert not nothing_to_get() or b"eps_bar is NULL" in ctx._lib.d2d_last_error()
    assert np.array_equal(_bits(ctx.get_material_eps_vjp()), _bits(want))
    rng = np.random.default_rng(3)
    ctx.set_scene(rng.random((5, 2, 2)).astype(F))
    assert nothing_to_get()
    ctx.set_scene(walls)


# ---- 5. the Scene methods -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("role", ["rx", "tx"])
def test_scene_methods_mirror_the_context(ctx, role):
    from differt2d_amd import utils
    from differt2d_amd.engine import make_params
    from differt2d_amd.geometry import Point, Wall
    from differt2d_amd.scene import Scene

    walls, fixed, X, Y = _case("random7")
    pts = {"a": Point(xy=fixed), "b": Point(xy=(F(1.0) - fixed).astype(F))}
    scene = Scene.from_walls_array(walls)
    scene = scene.with_transmitters(**pts) if role == "rx" else scene.with_receivers(**pts)
    name_of = "material_response_permittivity_vjp_on_receivers_grid" if role == "rx" else "material_response_permittivity_vjp_on_transmitters_grid"
    method = getattr(scene, name_of)
    nf = 9
    inv, eps = inv_list(nf), _eps("random7", nf)
    rb, ib = _bars("random7", nf)
    rb2, ib2 = _bars("random7", nf, seed=2)
    common = dict(min_order=0, max_order=2, approx=True, function="hard_sigmoid")
    fk = dict(r_coef=1.0, height=0.2)
    got = dict(method(X, Y, utils.received_power, fk, rb, ib, inv_wavelengths=inv, permittivity=eps, polarization="tm", **common))
    band = dict(method(X, Y, utils.received_power, fk, {"a": rb, "b": rb2}, {"a": ib, "b": ib2}, inv_wavelengths=inv, permittivity=eps[0],
                       amplitude="linear", **common))
    assert list(got) == list(band) == ["a", "b"]
    ctx.set_scene(walls)
    ctx.set_grid(X, Y)
    params = make_params(min_order=0, max_order=2, r_coef=1.0, height=0.2, grid_role=_role_id(role), **MODES["hsig"])
    for name, pt in pts.items():
        want = ctx.material_eps_vjp(params, pt.xy, inv, eps, rb, ib, "tm", "sqrt")
        assert got[name].dtype == np.complex128 and got[name].shape == (nf, 7)
        assert np.array_equal(_bits(got[name]), _bits(want)) and want.any()
        bars = (rb, ib) if name == "a" else (rb2, ib2)
        rows = ctx.material_eps_vjp(params, pt.xy, inv, eps[0], *bars, "te", "linear")
        assert band[name].shape == (7,) and np.array_equal(_bits(band[name]), _bits(rows.sum(axis=0)))  # the rows' sum, in float64
    assert not np.array_equal(got["a"], got["b"])
    # wavelengths=[w] is inv_wavelengths=[float32(1) / float32(w)]
    ws = [0.05, 0.03, 0.07]
    by_w = dict(method(X, Y, utils.received_power, fk, rb[:3], ib[:3], wavelengths=ws, permittivity=eps[:3], **common))
    by_inv = dict(method(X, Y, utils.received_power, fk, rb[:3], ib[:3], inv_wavelengths=F(1) / np.asarray(ws, F), permittivity=eps[:3], **common))
    assert all(np.array_equal(_bits(by_w[k]), _bits(by_inv[k])) for k in pts) and by_w["a"].any()
    # permittivity=None: read from the objects' attributes, a scalar or one value per wavelength
    @dataclasses.dataclass(frozen=True, eq=False)
    class Material(Wall):
        permittivity: object = None

    objs = [Material(xys=o.xys, permittivity=complex(eps[0, j]) if j % 2 else eps[:, j].copy()) for j, o in enumerate(scene.objects)]
    with_eps = dataclasses.replace(scene, objects=objs)
    table = eps.copy()
    table[:, 1::2] = eps[0, 1::2]
    attr = dict(getattr(with_eps, name_of)(X, Y, utils.received_power, fk, rb, ib, inv_wavelengths=inv, polarization="tm", **common))
    explicit = dict(method(X, Y, utils.received_power, fk, rb, ib, inv_wavelengths=inv, permittivity=table, polarization="tm", **common))
    for name in pts:
        assert attr[name].shape == (nf, 7) and np.array_equal(_bits(attr[name]), _bits(explicit[name])) and attr[name].any()


# ---- 6. calibration -----------------------------------------------------------------------------------------------------------------
def _descend(forward, grad, eps0, target, rate, steps=10):
    """Gradient descent with step halving on utils.field_misfit, as the coefficient adjoint's calibration test does: returns the
    losses of the accepted steps."""
    from differt2d_amd import utils

    eps = eps0
    fr = forward(eps)
    loss, rb, ib = utils.field_misfit(fr, target)
    losses = [loss]
    step = rate
    for it in range(steps):
        g = grad(eps, rb, ib)
        assert g.shape == eps.shape and np.isfinite(g).all() and g.any()
        for halvings in range(31):
            trial = eps.astype(np.complex128) - step * g
            trial = (trial.real + 1j * np.minimum(trial.imag, 0.0)).astype(np.complex64)  # (the launch refuses Im eps > 0)
            fr_t = forward(trial)
            loss_t, rb_t, ib_t = utils.field_misfit(fr_t, target)
            if loss_t < loss:
                break
            step *= 0.5
        else:
            pytest.fail(f"step {it}: no decrease after 30 halvings (loss {loss:.6e})")
        print(f"  step {it}: loss {loss:.6e} -> {loss_t:.6e} after {halvings} halvings (step {step:.3e})")
        assert loss_t < loss
        eps, loss, rb, ib = trial, loss_t, rb_t, ib_t
        losses.append(loss)
        step *= 2.0
    return losses


RATE = 1.0  # the first trial step; halved until the loss falls, doubled after every accepted step


def test_gradient_descent_calibrates_the_permittivities(ctx):
    """Planes generated by material_response with a true eps on random7 (16 x 24 grid, 9 wavelengths, LINEAR, TE); ten steps of
    descent with step halving on utils.field_misfit from 1 + 0.5 (eps - 1): every accepted step lowers the loss and the final loss is
    below half of the initial one.  The half is a condition, not a measurement: RATE was chosen so that the same descent on the
    float64 oracle, run on the CPU here, ends below a quarter (both ratios are printed)."""
    from differt2d_amd import utils
    from differt2d_amd.engine import FrequencyResponse, make_params

    walls, fixed, _, _ = _case("random7")
    X, Y = unit_grid(16, 24)
    nf = 9
    inv = inv_list(nf)
    true = eps_table(nf, 7, seed=21)
    start = (1 + 0.5 * (true.astype(np.complex128) - 1)).astype(np.complex64)
    params = make_params(min_order=0, max_order=2)
    ctx.set_scene(walls)
    ctx.set_grid(X, Y)
    target = utils.frequency_response(ctx.material_response(params, fixed, inv, true, "te", "linear"))
    print("GPU:")
    gpu = _descend(lambda e: ctx.material_response(params, fixed, inv, e, "te", "linear"),
                   lambda e, rb, ib: ctx.material_eps_vjp(params, fixed, inv, e, rb, ib, "te", "linear"), start, target, RATE)
    # the same descent on the float64 oracle
    con = MO.segment_contributions(walls, fixed, X, Y, min_order=0, max_order=2)
    normals = MO.wall_normals(walls)

    def forward64(e):
        H = EO.forward(*con, normals, inv, e.astype(np.complex128), MO.POL_TE, EO.AMP_LINEAR).reshape((nf,) + X.shape)
        return FrequencyResponse(re=H.real, im=H.imag, total=None)

    target64 = EO.forward(*con, normals, inv, true.astype(np.complex128), MO.POL_TE, EO.AMP_LINEAR).reshape((nf,) + X.shape)
    print("float64 oracle:")
    cpu = _descend(forward64, lambda e, rb, ib: EO.eps_grad(*con, normals, inv, e, rb, ib, MO.POL_TE, EO.AMP_LINEAR).eps_bar, start, target64, RATE)
    print(f"final / initial loss: GPU {gpu[-1] / gpu[0]:.4f}, float64 oracle {cpu[-1] / cpu[0]:.4f}")
    assert cpu[-1] < 0.25 * cpu[0], (cpu[0], cpu[-1])
    assert gpu[-1] < 0.5 * gpu[0], (gpu[0], gpu[-1])
