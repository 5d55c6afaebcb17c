"""The coefficient adjoint of the frequency response (include/d2d.h: d2d_field_coefs_vjp_launch; power_sink_kernel, CoefGradSink):
``coef_bar[w] = sum_j sum_cells (re_bar * d re / d coef[w] + im_bar * d im / d coef[w])`` for the per-object reflection coefficients.
A sum over cells, so it is held to the float64 oracle of ``tests/field_coefs_vjp_oracle.py`` within that module's derived bound per
wall (never relative to ``|coef_bar|``: a wall's gradient cancels to a fraction of a percent of its terms' magnitude), to the rules
that ARE exact (same bits run to run, zero and doubled cotangents, chunks alone), to the forward product users get, to the incoherent
coefficient adjoint of the value+grad kernel, to its NaN rule, its state rules and refusals, and through the Scene methods.  Scenes and
grids are those of ``tests/test_gpu_strongest_paths.py``; the wavelength lists are ``inv_list(nf)`` of the frequency-response tests;
cotangents are seeded standard normals.  Every comparison first asserts the oracle's guards (``field_coefs_vjp_oracle.guards``)."""

import dataclasses
import functools

import numpy as np
import pytest

from conftest import unit_grid
from coherent_field_oracle import AMP_LINEAR, AMP_SQRT
from field_coefs_vjp_oracle import coef_grad, guards, scale_contributions
from frequency_response_oracle import physics_list
from strongest_paths_oracle import contributions
from test_gpu_strongest_paths import COEF7, MODES, _case, _role_id

pytestmark = pytest.mark.gpu

F = np.float32
AMPS = {"sqrt": AMP_SQRT, "linear": AMP_LINEAR}
INV_20 = F(1) / F(0.05)
HEIGHT = 0.25
COEF8 = np.array([0.3, 0.4, -0.7, 0.6, 0.7, 0.5, 0.0, 0.45], F)
assert np.array_equal(COEF8[:7], COEF7)
FUN = "received_power_per_object"


def inv_list(nf):
    return (INV_20 * (F(1) + np.arange(nf, dtype=F) / F(64))).astype(F)


def coefs_of(scene):
    return COEF8[: len(_case(scene)[0])].copy()


@pytest.fixture(scope="module")
def ctx():
    from differt2d_amd.engine import Context

    with Context(0) as c:
        yield c


@functools.lru_cache(maxsize=None)
def _scale(scene, mode, role, lo=0, hi=2, masked=()):
    walls, fixed, X, Y = _case(scene)
    out = scale_contributions(walls, fixed, X, Y, HEIGHT, min_order=lo, max_order=hi, grid_role=role, filter_nodes=set(masked) or None,
                              **MODES[mode])
    assert not np.isnan(out[1]).any()
    for a in out[1:]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _bars(scene, nf, seed=0):
    shape = _case(scene)[2].shape
    rng = np.random.default_rng(1000 + 31 * seed + nf)
    rb, ib = rng.standard_normal((nf,) + shape).astype(F), rng.standard_normal((nf,) + shape).astype(F)
    rb.setflags(write=False)
    ib.setflags(write=False)
    return rb, ib


@functools.lru_cache(maxsize=None)
def _oracle(scene, mode, role, amp, nf, lo=0, hi=2, masked=()):
    cands, S, Rl = _scale(scene, mode, role, lo, hi, masked)
    rb, ib = _bars(scene, nf)
    coef = coefs_of(scene)
    cg = coef_grad(cands, S, Rl, coef, inv_list(nf), rb, ib, AMPS[amp])
    guards(cg, coef if not masked else np.ones_like(coef), AMPS[amp], scene if (lo, hi, masked) == (0, 2, ()) else None, cands,
           need_repeat=hi >= 3)
    return cg


def _gpu(ctx, scene, mode, role, inv, rb, ib, amp, lo=0, hi=2, coef=None, allowed=None):
    from differt2d_amd.engine import make_params

    walls, fixed, X, Y = _case(scene)
    ctx.set_scene(walls)
    if allowed is not None:
        ctx.set_candidate_mask(allowed)
    ctx.set_reflection_coefs(coefs_of(scene) if coef is None else coef)
    ctx.set_grid(X, Y)
    params = make_params(min_order=lo, max_order=hi, fun=FUN, height=HEIGHT, grid_role=_role_id(role), **MODES[mode])
    try:
        return ctx.field_coefs_vjp(params, fixed, inv, rb, ib, amp), params
    finally:
        if allowed is not None:
            ctx.set_candidate_mask(None)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _within(got, cg, tag):
    assert got.dtype == np.float64 and got.shape == cg.coef_bar.shape
    err = np.abs(got - cg.coef_bar)
    lit = cg.mag > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        print(f"{tag}: walls {np.flatnonzero(lit).tolist()}, max err / bound {np.max(err[lit] / cg.bound[lit]):.3f}, "
              f"max bound / mag {np.max(cg.bound[lit] / cg.mag[lit]):.2e}, min |coef_bar| / mag {np.min(np.abs(cg.coef_bar[lit]) / cg.mag[lit]):.1e}")
    assert (err <= cg.bound).all(), (tag, err, cg.bound)
    assert not _bits(got[~lit]).any(), (tag, got[~lit])  # untouched walls: exactly +0.0


# ---- 1. against the float64 oracle, within its bound ---------------------------------------------------------------------------
@pytest.mark.parametrize("nf", [1, 8, 9, 17])
@pytest.mark.parametrize("amp", ["sqrt", "linear"])
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
@pytest.mark.parametrize("scene", ["obstacle", "random7"])
def test_gradient_within_the_oracle_bound(ctx, scene, mode, role, amp, nf):
    """nf: a partial chunk, a full chunk, a full chunk plus one, two full chunks plus one."""
    cg = _oracle(scene, mode, role, amp, nf)
    got, _ = _gpu(ctx, scene, mode, role, inv_list(nf), *_bars(scene, nf), amp)
    _within(got, cg, f"{scene} {mode} {role} {amp} nf={nf}")


@pytest.mark.parametrize("amp", ["sqrt", "linear"])
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
def test_repeated_walls_at_order_three(ctx, mode, role, amp):
    """The square with the fixed end point at its centre, orders 0-3 (the MAXK = 3 instance): candidates (a, b, a) contribute, so a
    wall receives two terms of one candidate (the oracle's guard asserts that such a candidate contributes)."""
    cg = _oracle("square_centre", mode, role, amp, 9, 0, 3)
    got, _ = _gpu(ctx, "square_centre", mode, role, inv_list(9), *_bars("square_centre", 9), amp, 0, 3)
    _within(got, cg, f"square_centre {mode} {role} {amp} orders 0-3")


@pytest.mark.parametrize("role", ["rx", "tx"])
def test_gradient_honours_min_order_and_the_candidate_mask(ctx, role):
    rb, ib = _bars("random7", 9)
    # min_order = 1 (the line of sight holds no coefficient: the same gradient as with it, from a sweep without it)
    cg = _oracle("random7", "hsig", role, "linear", 9, 1, 2)
    got, _ = _gpu(ctx, "random7", "hsig", role, inv_list(9), rb, ib, "linear", 1, 2)
    _within(got, cg, f"random7 hsig {role} min_order=1")
    # a candidate mask: walls 2 and 5 are out, wall 2 carries terms without the mask and none with it
    allowed = np.ones(7, np.uint8)
    allowed[[2, 5]] = 0
    cg = _oracle("random7", "hard", role, "linear", 9, 0, 2, (2, 5))
    everything = _oracle("random7", "hard", role, "linear", 9)
    assert everything.mag[2] > 0 and cg.mag[2] == 0
    got, _ = _gpu(ctx, "random7", "hard", role, inv_list(9), rb, ib, "linear", allowed=allowed)
    _within(got, cg, f"random7 hard {role} masked")


# ---- 2. what is exact ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
def test_exact_rules(ctx, mode, role):
    from differt2d_amd.engine import make_params

    nf = 17
    inv = inv_list(nf)
    rb, ib = _bars("obstacle", nf)
    cg = _oracle("obstacle", mode, role, "sqrt", nf)
    got, params = _gpu(ctx, "obstacle", mode, role, inv, rb, ib, "sqrt")
    _within(got, cg, f"obstacle {mode} {role} sqrt")
    fixed = _case("obstacle")[1]
    # two launches give the same bits, also after an unrelated frequency response and a value+grad launch on the same context
    again = ctx.field_coefs_vjp(params, fixed, inv, rb, ib, "sqrt")
    assert np.array_equal(_bits(again), _bits(got))
    ctx.frequency_response(make_params(min_order=0, max_order=1, **MODES[mode]), fixed, inv[:3], "linear")
    ctx.set_cotangent(np.ones(ctx.shape, F))
    ctx.launch_vg(make_params(min_order=0, max_order=2, fun=FUN, height=HEIGHT, **MODES[mode]), fixed, scene_vjp=True)
    k2 = ctx.get_reflection_coefs_vjp()
    assert np.array_equal(_bits(ctx.get_field_coefs_vjp()), _bits(got))  # the result is still there ...
    assert np.array_equal(_bits(ctx.field_coefs_vjp(params, fixed, inv, rb, ib, "sqrt")), _bits(got))
    assert np.array_equal(ctx.get_reflection_coefs_vjp(), k2) and k2.any()  # ... and the value+grad kernel's block was not touched
    # zero cotangents: all +0.0
    zero = np.zeros_like(rb)
    assert not _bits(ctx.field_coefs_vjp(params, fixed, inv, zero, zero, "sqrt")).any()
    # doubled cotangents: exactly doubled
    twice = ctx.field_coefs_vjp(params, fixed, inv, F(2) * rb, F(2) * ib, "sqrt")
    assert np.array_equal(_bits(twice), _bits(2.0 * got)) and got.any()
    # cotangents that are zero outside one chunk: the bits of the call with that chunk's 8 wavelengths alone
    for lo, hi in ((0, 8), (8, 16), (16, 17)):
        rz, iz = np.zeros_like(rb), np.zeros_like(ib)
        rz[lo:hi], iz[lo:hi] = rb[lo:hi], ib[lo:hi]
        whole = ctx.field_coefs_vjp(params, fixed, inv, rz, iz, "sqrt")
        alone = ctx.field_coefs_vjp(params, fixed, inv[lo:hi], rb[lo:hi], ib[lo:hi], "sqrt")
        assert np.array_equal(_bits(whole), _bits(alone)) and alone.any(), (lo, hi)


# ---- 3. against the forward product users get -----------------------------------------------------------------------------------
def _forward(ctx, params, fixed, coef, inv):
    ctx.set_reflection_coefs(coef)
    fr = ctx.frequency_response(params, fixed, inv, "linear")
    return fr.re.astype(np.float64), fr.im.astype(np.float64)


@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
@pytest.mark.parametrize("scene", ["obstacle", "random7"])
def test_gradient_is_the_difference_of_two_forward_calls(ctx, scene, mode, role):
    """At orders <= 2 no wall repeats in a candidate, so with LINEAR ``H`` is affine in each coefficient and ``coef_bar[w] = <bar,
    H(c + e_w) - H(c)>`` exactly in real arithmetic.  The right-hand side is formed in float64 from two GPU frequency responses; the
    two sides agree within ``bound_w + sum |bar| (b0 + b1)``, with ``b0``, ``b1`` the two forward calls' ``physics_list`` bounds, summed
    over the cells in which wall ``w`` contributes (elsewhere the two forward calls execute the same operations on the same values:
    their planes are equal in bits and the difference is exactly zero, which the test asserts).  The guard wants that tolerance below
    ``2^-10 mag_w``; a wall that misses it at nf = 17 is run at nf = 1 instead, and a wall that misses it at
    both (a wall with a handful of weak terms beside a strong line of sight) is left to test 1 -- the zero-coefficient wall and at
    least three walls in all must be run."""
    walls, fixed, X, Y = _case(scene)
    coef = coefs_of(scene)
    kw = dict(min_order=0, max_order=2, grid_role=role, **MODES[mode])
    ran, zero_ran = [], False
    for nf in (17, 1):
        inv = inv_list(nf)
        rb, ib = _bars(scene, nf)
        cg = _oracle(scene, mode, role, "linear", nf)
        cands, S, Rl = _scale(scene, mode, role)
        todo = [w for w in np.flatnonzero(cg.mag > 0) if w not in ran]
        if not todo:
            break
        got, params = _gpu(ctx, scene, mode, role, inv, rb, ib, "linear")
        _, T0, Rl0, _ = contributions(walls, fixed, X, Y, fun=FUN, coef=coef, fun_kwargs=dict(height=HEIGHT), **kw)
        _, b0 = physics_list(T0, Rl0, inv, AMP_LINEAR)
        re0, im0 = _forward(ctx, params, fixed, coef, inv)
        absbar = (np.abs(rb) + np.abs(ib)).reshape(nf, -1).astype(np.float64)
        for w in todo:
            c1 = coef.copy()
            c1[w] += F(1)
            _, T1, Rl1, _ = contributions(walls, fixed, X, Y, fun=FUN, coef=c1, fun_kwargs=dict(height=HEIGHT), **kw)
            _, b1 = physics_list(T1, Rl1, inv, AMP_LINEAR)
            cells = np.zeros(S.shape[1], bool)
            for ci, nz in cg.touched.items():
                if w in [int(o) for o in cands[ci]]:
                    cells |= nz
            tol = cg.bound[w] + (absbar * (b0 + b1))[:, cells].sum()
            if not tol < 2.0**-10 * cg.mag[w]:
                continue
            re1, im1 = _forward(ctx, params, fixed, c1, inv)
            dre, dim = (re1 - re0).reshape(nf, -1), (im1 - im0).reshape(nf, -1)
            assert not dre[:, ~cells].any() and not dim[:, ~cells].any()
            rhs = float((rb.reshape(nf, -1).astype(np.float64) * dre + ib.reshape(nf, -1).astype(np.float64) * dim).sum())
            print(f"{scene} {mode} {role} nf={nf} wall {w}: |gpu - rhs| / tol {abs(got[w] - rhs) / tol:.3f}, tol / mag {tol / cg.mag[w]:.2e}")
            assert abs(got[w] - rhs) <= tol, (w, got[w], rhs, tol)
            ran.append(int(w))
            zero_ran = zero_ran or coef[w] == 0
    ctx.set_reflection_coefs(coef)
    assert len(ran) >= 3 and zero_ran, ran


# ---- 4. against the value+grad kernel's coefficient adjoint ---------------------------------------------------------------------
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
def test_zero_wavenumber_is_the_incoherent_coefficient_adjoint(ctx, mode, role):
    """inv_wavelength = [0], LINEAR, im_bar = 0, re_bar = cot: every phasor is (1, 0), re is the fused map, and the result is what
    d2d_get_reflection_coefs_vjp gives after d2d_set_cotangent(cot) and a value+grad launch with the scene VJP -- two kernels that
    share nothing but the sweep.  Both sum fp32 per-patch rows in fp64; the other one returns fp32.  Tolerance: this oracle's bound
    for either kernel (the same count of operations covers both) plus the fp32 rounding of the other's result."""
    from differt2d_amd.engine import make_params

    walls, fixed, X, Y = _case("obstacle")
    coef = coefs_of("obstacle")
    cot, _ = _bars("obstacle", 1, seed=4)
    cands, S, Rl = _scale("obstacle", mode, role)
    inv = np.zeros(1, F)
    cg = coef_grad(cands, S, Rl, coef, inv, cot, np.zeros_like(cot), AMP_LINEAR)
    guards(cg, coef, AMP_LINEAR, "obstacle", cands)
    got, _ = _gpu(ctx, "obstacle", mode, role, inv, cot, np.zeros_like(cot), "linear")
    _within(got, cg, f"obstacle {mode} {role} inv=0")
    ctx.set_cotangent(cot[0])
    ctx.launch_vg(make_params(min_order=0, max_order=2, fun=FUN, height=HEIGHT, grid_role=_role_id(role), **MODES[mode]), fixed, scene_vjp=True)
    k2 = ctx.get_reflection_coefs_vjp().astype(np.float64)
    tol = 2 * cg.bound + 2.0**-24 * np.abs(cg.coef_bar)
    print(f"{mode} {role}: max |this - value+grad| / tol {np.max(np.abs(got - k2)[cg.mag > 0] / tol[cg.mag > 0]):.3f}")
    assert (np.abs(got - k2) <= tol).all() and np.count_nonzero(k2) >= 3


# ---- 5. NaN -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
def test_a_nan_cotangent_reaches_the_walls_of_that_cells_candidates_only(ctx, mode, role):
    nf = 9
    cg = _oracle("obstacle", mode, role, "linear", nf)
    cands, S, Rl = _scale("obstacle", mode, role)
    lit = np.flatnonzero(cg.mag > 0)
    walls_of = {}
    for ci, nz in cg.touched.items():
        for cell in np.flatnonzero(nz):
            walls_of.setdefault(int(cell), set()).update(int(o) for o in cands[ci])
    # a cell whose candidates touch some of the walls that have a gradient, not all of them (the last column where there is one:
    # a partial patch's edge, which the lanes outside the grid copy)
    n = _case("obstacle")[2].shape[1]
    some = [c for c, ws in sorted(walls_of.items()) if 0 < len(ws) < len(lit)]
    assert some
    cell = next((c for c in some if c % n == n - 1), some[0])
    rb, ib = (a.copy() for a in _bars("obstacle", nf))
    clean, _ = _gpu(ctx, "obstacle", mode, role, inv_list(nf), rb, ib, "linear")
    rb.reshape(nf, -1)[8, cell] = np.nan  # in the second chunk
    got, _ = _gpu(ctx, "obstacle", mode, role, inv_list(nf), rb, ib, "linear")
    hit = np.zeros(len(clean), bool)
    hit[sorted(walls_of[cell])] = True
    print(f"{mode} {role}: cell {cell}, NaN walls {np.flatnonzero(hit).tolist()} of {lit.tolist()}")
    assert np.isnan(got[hit]).all() and np.array_equal(_bits(got[~hit]), _bits(clean[~hit])) and np.isfinite(clean).all()


# ---- 6. state rules and refusals ----------------------------------------------------------------------------------------------------
def test_state_rules_and_refusals(ctx):
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import make_params

    walls, fixed, X, Y = _case("random7")
    nf = 9
    inv = inv_list(nf)
    rb, ib = _bars("random7", nf)
    kw = dict(min_order=0, max_order=2, height=HEIGHT)
    ok = make_params(fun=FUN, **kw)

    def nothing_to_get():
        rc = ctx._lib.d2d_get_field_coefs_vjp(ctx._ctx, None)
        return rc == -5 and b"d2d_field_coefs_vjp_launch" in ctx._lib.d2d_last_error()

    ctx.set_scene(walls)
    ctx.set_reflection_coefs(None)
    ctx.set_grid(*unit_grid(19, 11))  # a grid this context has not seen: no result yet
    ctx.set_grid(X, Y)
    assert nothing_to_get()
    with pytest.raises(L.D2DError) as e:
        ctx.get_field_coefs_vjp()
    assert e.value.status == -5
    # without coefficients: D2D_ERR_STATE, as the sweeps answer
    with pytest.raises(L.D2DError, match="d2d_set_reflection_coefs") as e:
        ctx.field_coefs_vjp(ok, fixed, inv, rb, ib)
    assert e.value.status == -5 and nothing_to_get()
    ctx.set_reflection_coefs(COEF7)
    want = ctx.field_coefs_vjp(ok, fixed, inv, rb, ib)
    _within(want, _oracle("random7", "hard", "rx", "sqrt", nf), "random7 hard rx sqrt")
    ctx.launch(make_params(min_order=0, max_order=2), fixed)
    before = ctx.get_map()
    n0 = ctx.txg_fallbacks()

    def refused(status, word, params, inv_=inv, amp="sqrt", bars=(rb, ib)):
        with pytest.raises(L.D2DError, match=word) as e:
            ctx.field_coefs_vjp(params, fixed, inv_, *bars, amp)
        assert e.value.status == status, (e.value.status, str(e.value))
        assert isinstance(e.value, L.D2DUnsupported) == (status == -4)
        assert "d2d_field_coefs_vjp_launch" in str(e.value)
        # a refused launch leaves the previous result readable, and the value map as it was
        assert np.array_equal(_bits(ctx.get_field_coefs_vjp()), _bits(want))
        assert np.array_equal(ctx.get_map().view(np.uint32), before.view(np.uint32)) and before.any()

    for fun in ("received_power", "one", "length", "length_squared", "custom"):
        refused(-4, "D2D_FUN_RECEIVED_POWER_PER_OBJECT", make_params(fun=fun, min_order=0, max_order=2))
    refused(-4, "sigmoid", make_params(fun=FUN, approx=True, function="sigmoid", **kw))
    for solver in ("min", "fermat"):
        refused(-4, "MinPath / FermatPath", make_params(fun=FUN, solver=solver, **kw))
    refused(-4, "D2D_OUT_ADD", make_params(fun=FUN, out_mode=L.OUT_ADD, **kw))
    refused(-4, "not culled", make_params(fun=FUN, grid_role=L.GRID_TX, tol=0.6, **kw))
    ctx.set_option("txg_exhaustive", 1)
    try:
        refused(-4, "txg_exhaustive", make_params(fun=FUN, grid_role=L.GRID_TX, **kw))
    finally:
        ctx.set_option("txg_exhaustive", 0)
    # nf of 0 and of D2D_FREQ_MAX + 1
    empty = np.zeros((0,) + X.shape, F)
    refused(-1, "nf in 1 .. 1024", ok, inv_=np.zeros(0, F), bars=(empty, empty))
    many = np.zeros((L.D2D_FREQ_MAX + 1,) + X.shape, F)
    refused(-1, "nf in 1 .. 1024", ok, inv_=np.full(L.D2D_FREQ_MAX + 1, INV_20, F), bars=(many, many))
    # a negative, a NaN and an infinite entry, in the first chunk and in the second: the message names the index
    for at in (0, 8):
        for bad in (-1.0, float("nan"), float("inf")):
            v = inv.copy()
            v[at] = bad
            refused(-1, f"inv_wavelength.* at index {at}$", ok, inv_=v)
    for amp in (2, -1):
        refused(-1, "amplitude", ok, amp=amp)
    with pytest.raises(L.D2DError, match="amplitude") as e:  # (an unknown name is refused by the Python layer)
        ctx.field_coefs_vjp(ok, fixed, inv, rb, ib, "power")
    assert e.value.status == -1
    with pytest.raises(L.D2DError, match="shape") as e:  # (... and so are cotangents of another shape)
        ctx.field_coefs_vjp(ok, fixed, inv, rb[:3], ib[:3])
    assert e.value.status == -1
    assert np.array_equal(_bits(ctx.get_field_coefs_vjp()), _bits(want))
    assert ctx.txg_fallbacks() == n0
    # non-finite cotangents are not refused: they propagate
    inf_bar = rb.copy()
    inf_bar[0] = np.inf
    assert not np.isfinite(ctx.field_coefs_vjp(ok, fixed, inv, inf_bar, ib)).all()
    # the library's constants are taken as well as the names; the result of the accepted launch replaces the previous one
    a = ctx.field_coefs_vjp(ok, fixed, inv, rb, ib, L.D2D_FIELD_AMP_LINEAR)
    assert np.array_equal(_bits(a), _bits(ctx.field_coefs_vjp(ok, fixed, inv, rb, ib, "linear"))) and not np.array_equal(a, want)
    # another grid drops the result, and so does another scene
    ctx.set_grid(*unit_grid(19, 11))
    assert nothing_to_get()
    ctx.set_grid(X, Y)
    ctx.field_coefs_vjp(ok, fixed, inv, rb, ib)
    assert not nothing_to_get()
    rng = np.random.default_rng(3)
    ctx.set_scene(rng.random((5, 2, 2)).astype(F))
    assert nothing_to_get()
    # 4 096 objects exceed the 12-bit wall indices
    ctx.set_scene(rng.random((4096, 2, 2)).astype(F))
    ctx.set_reflection_coefs(np.full(4096, 0.5, F))
    with pytest.raises(L.D2DUnsupported, match="4096 objects") as e:
        ctx.field_coefs_vjp(make_params(fun=FUN, min_order=0, max_order=1, height=HEIGHT), fixed, inv, rb, ib)
    assert e.value.status == -4 and "d2d_field_coefs_vjp_launch" in str(e.value) and nothing_to_get()
    ctx.set_scene(walls)


# ---- 7. the Scene methods -----------------------------------------------------------------------------------------------------------
def _coated(walls, coef):
    from differt2d_amd.geometry import Wall

    @dataclasses.dataclass(frozen=True, eq=False)
    class CoatedWall(Wall):
        r_coef: float = 0.5

    return [CoatedWall(xys=w, r_coef=float(c)) for w, c in zip(walls, coef)]


@pytest.mark.parametrize("role", ["rx", "tx"])
def test_scene_methods_mirror_the_context(ctx, role):
    from differt2d_amd.engine import make_params
    from differt2d_amd.geometry import Point
    from differt2d_amd.scene import Scene

    walls, fixed, X, Y = _case("random7")
    pts = {"a": Point(xy=fixed), "b": Point(xy=(F(1.0) - fixed).astype(F))}
    scene = Scene(objects=_coated(walls, COEF7))
    scene = scene.with_transmitters(**pts) if role == "rx" else scene.with_receivers(**pts)
    method = scene.frequency_response_coefs_vjp_on_receivers_grid if role == "rx" else scene.frequency_response_coefs_vjp_on_transmitters_grid
    nf = 9
    inv = inv_list(nf)
    rb, ib = _bars("random7", nf)
    rb2, ib2 = _bars("random7", nf, seed=2)
    common = dict(min_order=0, max_order=2, approx=True, function="hard_sigmoid")
    fk = dict(height=HEIGHT)
    got = dict(method(X, Y, fk, rb, ib, inv_wavelengths=inv, **common))
    per = dict(method(X, Y, fk, {"a": rb, "b": rb2}, {"a": ib, "b": ib2}, inv_wavelengths=inv, amplitude="linear", **common))
    assert list(got) == list(per) == ["a", "b"]
    ctx.set_scene(walls)
    ctx.set_reflection_coefs(COEF7)
    ctx.set_grid(X, Y)
    params = make_params(min_order=0, max_order=2, fun=FUN, height=HEIGHT, grid_role=_role_id(role), **MODES["hsig"])
    for name, pt in pts.items():
        want = ctx.field_coefs_vjp(params, pt.xy, inv, rb, ib, "sqrt")
        assert got[name].dtype == np.float64 and np.array_equal(_bits(got[name]), _bits(want)) and want.any()
        bars = (rb, ib) if name == "a" else (rb2, ib2)
        assert np.array_equal(_bits(per[name]), _bits(ctx.field_coefs_vjp(params, pt.xy, inv, *bars, "linear")))
    _within(got["a"], _oracle("random7", "hsig", role, "sqrt", nf), f"scene method {role}")
    assert not np.array_equal(got["a"], got["b"]) and not np.array_equal(got["a"], per["a"])
    # wavelengths=[w] is inv_wavelengths=[float32(1) / float32(w)]
    ws = [0.05, 0.03, 0.07]
    by_w = dict(method(X, Y, fk, rb[:3], ib[:3], wavelengths=ws, **common))
    by_inv = dict(method(X, Y, fk, rb[:3], ib[:3], inv_wavelengths=F(1) / np.asarray(ws, F), **common))
    assert all(np.array_equal(_bits(by_w[k]), _bits(by_inv[k])) for k in pts) and by_w["a"].any()
    with pytest.raises(ValueError, match="exactly one"):
        method(X, Y, fk, rb, ib, **common)
    with pytest.raises(ValueError, match="exactly one"):
        method(X, Y, fk, rb, ib, wavelengths=ws, inv_wavelengths=inv, **common)


def test_gradient_descent_calibrates_the_coefficients(ctx):
    """Ten steps of gradient descent with step halving on utils.field_misfit, from 0.5 * COEF towards planes generated with COEF on
    the obstacle scene: every accepted step lowers the loss recomputed by the forward call, and no step needs more than 30 halvings."""
    from differt2d_amd import utils
    from differt2d_amd.geometry import Point
    from differt2d_amd.scene import Scene

    walls, fixed, X, Y = _case("obstacle")
    inv = inv_list(9)
    common = dict(min_order=0, max_order=2)
    fk = dict(height=HEIGHT)

    def forward(coef):
        scene = Scene(objects=_coated(walls, coef)).with_transmitters(tx=Point(xy=fixed))
        (_, fr), = scene.frequency_response_on_receivers_grid(X, Y, utils.received_power_per_object, fk, inv_wavelengths=inv,
                                                              amplitude="linear", **common)
        return scene, fr

    _, measured = forward(COEF8)
    target = utils.frequency_response(measured)
    coef = (F(0.5) * COEF8).astype(F)
    scene, fr = forward(coef)
    loss, rb, ib = utils.field_misfit(fr, target)
    first = loss
    assert loss > 0
    step = 1.0
    for it in range(10):
        (_, g), = scene.frequency_response_coefs_vjp_on_receivers_grid(X, Y, fk, rb, ib, inv_wavelengths=inv, amplitude="linear", **common)
        assert g.shape == (8,) and np.isfinite(g).all() and g.any()
        for halvings in range(31):
            trial = (coef.astype(np.float64) - step * g).astype(F)
            scene_t, fr_t = forward(trial)
            loss_t, rb_t, ib_t = utils.field_misfit(fr_t, target)
            if loss_t < loss:
                break
            step *= 0.5
        else:
            pytest.fail(f"step {it}: no decrease after 30 halvings (loss {loss:.6e})")
        print(f"step {it}: loss {loss:.6e} -> {loss_t:.6e} after {halvings} halvings (step {step:.3e})")
        coef, scene, loss, rb, ib = trial, scene_t, loss_t, rb_t, ib_t
        step *= 2.0
    assert loss < 0.5 * first, (first, loss)
