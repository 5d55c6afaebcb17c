"""The coherent field (include/d2d.h: d2d_coherent_field_launch; power_sink_kernel, FieldSink): per cell the sum of the fused
sweep's contributions as complex amplitudes with the phase of their path length.  Held bit for bit to the oracle recipe of
``tests/coherent_field_oracle.py`` (which ``tests/test_coherent_field_cpu.py`` pins to ``R.power_map``, to the g++ build of the
phasor header and to float64), to the fused map, to the float64 physics, and to its state rules and refusals.  The scenes and the
cached contributions are those of ``tests/test_gpu_strongest_paths.py`` (computed once per session)."""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import unit_grid
from coherent_field_oracle import AMP_LINEAR, AMP_SQRT, CoherentField, fold, phasor, phasor_inputs, physics
from test_gpu_strongest_paths import COEF7, MODES, _case, _contributions, _role_id

pytestmark = pytest.mark.gpu

F = np.float32
AMPS = {"sqrt": AMP_SQRT, "linear": AMP_LINEAR}
INV_20 = F(1) / F(0.05)  # wavelength 0.05: what Scene.coherent_field_on_*_grid hands to the library
FUSED_FUNS = ["received_power", "length_squared", "length", "one", "received_power_per_object"]


@pytest.fixture(scope="module")
def ctx():
    from differt2d_amd.engine import Context

    with Context(0) as c:
        yield c


def _oracle(scene, mode, role, fun, inv, amp, lo=0, hi=2, masked=()):
    _, T, Rl, _ = _contributions(scene, mode, role, fun, lo, hi, masked)
    shape = _case(scene)[2].shape
    return CoherentField(*(a.reshape(shape) for a in fold(T, Rl, inv, AMPS[amp])))


def _gpu(ctx, scene, mode, role, fun, inv, amp, lo=0, hi=2, **extra):
    from differt2d_amd.engine import make_params

    walls, fixed, X, Y = _case(scene)
    ctx.set_scene(walls)
    if fun == "received_power_per_object":
        ctx.set_reflection_coefs(COEF7)
        extra["height"] = 0.25
    ctx.set_grid(X, Y)
    params = make_params(min_order=lo, max_order=hi, fun=fun, grid_role=_role_id(role), **MODES[mode], **extra)
    return ctx.coherent_field(params, fixed, inv, amp), params


def _same(got, want):
    for name, g, w in zip(want._fields, got, want):
        assert g.dtype == w.dtype == np.float32 and g.shape == w.shape, (name, g.dtype, g.shape, w.dtype, w.shape)
        bad = np.ascontiguousarray(g).view(np.uint32) != np.ascontiguousarray(w).view(np.uint32)
        assert not bad.any(), f"{name}: {bad.sum()} of {bad.size} cells differ, first at {tuple(np.argwhere(bad)[0])}: {g[bad][0]!r} != {w[bad][0]!r}"


# ---- 1. bit for bit against the oracle recipe ---------------------------------------------------------------------------------
@pytest.mark.parametrize("amp", ["sqrt", "linear"])
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
@pytest.mark.parametrize("scene,inv", [("random7", INV_20), ("obstacle", INV_20), ("random7", F(4096))],
                         ids=["random7-wl0.05", "obstacle-wl0.05", "random7-inv4096"])
def test_field_equals_the_oracle_recipe(ctx, scene, inv, mode, role, amp):
    """inv = 4096: u = r / lambda in the thousands, so the phase resolves 2^-12 .. 2^-11 turns only (coarse, and still by bits)."""
    _, T, Rl, _ = _contributions(scene, mode, role, "received_power")
    want = _oracle(scene, mode, role, "received_power", inv, amp)
    # (so that the comparison does not pass on empty ground)
    count = (T != 0).sum(axis=0)
    lit = count >= 1
    print(f"{scene} {mode} {role} {amp} inv={float(inv):g}: {(count >= 2).mean():.2f} of the cells, {(count >= 2).sum() / lit.sum():.2f} of the "
          f"lit cells have two or more paths, at most {count.max()}; im != 0 in {np.count_nonzero(want.im)} cells")
    if scene == "obstacle":
        assert (count >= 2).mean() > 0.5
    else:  # (7 random walls leave half of the 21 x 13 cells dark and a third with two or more paths: 0.34 hard, 0.37 hard_sigmoid)
        assert (count >= 2).sum() > lit.sum() / 2 and (count >= 2).mean() > 1 / 3
    assert np.count_nonzero(want.im) > want.im.size // 3 and np.count_nonzero(want.re) > want.re.size // 3
    got, _ = _gpu(ctx, scene, mode, role, "received_power", inv, amp)
    assert np.count_nonzero(got.im) > 0
    _same(got, want)


# ---- 2. identities --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
@pytest.mark.parametrize("fun", FUSED_FUNS)
def test_total_is_the_fused_map_and_zero_wavelength_linear_is_it_too(ctx, fun, mode, role):
    walls, fixed, X, Y = _case("random7")
    try:
        got, params = _gpu(ctx, "random7", mode, role, fun, 0.0, "linear")
        ctx.launch(params, fixed)
        fused = ctx.get_map()
        wl, _ = _gpu(ctx, "random7", mode, role, fun, INV_20, "sqrt")
    finally:
        ctx.set_reflection_coefs(None)
    assert np.isfinite(fused).all() and np.count_nonzero(fused) > fused.size // 3
    assert np.array_equal(got.total.view(np.uint32), fused.view(np.uint32))
    assert np.array_equal(got.re.view(np.uint32), fused.view(np.uint32))  # every phasor is (1, +0)
    assert not got.im.view(np.uint32).any()  # +0.0, not -0.0
    assert np.array_equal(wl.total.view(np.uint32), fused.view(np.uint32)) and np.count_nonzero(wl.im) > 0
    if fun == "received_power_per_object":  # the negative and the zero coefficient are exercised
        cands, T, _, _ = _contributions("random7", mode, role, fun)
        through = lambda w: np.array([w in c for c in cands])
        assert (T[through(2)] < 0).any() and not T[through(6)].any() and (_contributions("random7", mode, role, "one")[1][through(6)] != 0).any()
        _same(wl, _oracle("random7", mode, role, fun, INV_20, "sqrt"))
        _same(got, _oracle("random7", mode, role, fun, 0.0, "linear"))


@pytest.mark.parametrize("amp", ["sqrt", "linear"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
def test_mirrored_paths_add_and_never_cancel(ctx, mode, amp):
    """The square with the fixed end point at its centre: mirrored candidates have the same length and the same contribution bit
    for bit, hence the same phasor -- their sum is twice one of them, whatever the wavelength."""
    _, T, Rl, _ = _contributions("square_centre", mode, "rx", "received_power")
    tb, rb = T.view(np.uint32), Rl.view(np.uint32)
    twins = 0
    for i in range(len(T)):
        for j in range(i + 1, len(T)):
            both = (T[i] != 0) & (tb[i] == tb[j]) & (rb[i] == rb[j])
            if both.any():
                twins += 1
                a = fold(T[[i, j]][:, both], Rl[[i, j]][:, both], INV_20, AMPS[amp])
                b = fold(T[[i]][:, both], Rl[[i]][:, both], INV_20, AMPS[amp])
                assert np.array_equal(a[0], b[0] + b[0]) and np.array_equal(a[1], b[1] + b[1])
    assert twins >= 4
    got, _ = _gpu(ctx, "square_centre", mode, "rx", "received_power", INV_20, amp)
    _same(got, _oracle("square_centre", mode, "rx", "received_power", INV_20, amp))


# ---- 3. against physics in float64 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("amp", ["sqrt", "linear"])
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
@pytest.mark.parametrize("scene,inv", [("random7", INV_20), ("obstacle", INV_20), ("random7", F(4096))],
                         ids=["random7-wl0.05", "obstacle-wl0.05", "random7-inv4096"])
def test_field_against_the_float64_sum_of_phasors(ctx, scene, inv, mode, role, amp):
    """sum a_i e^(-j 2 pi r_i / lambda) in float64 from the oracle's fp32 contributions and lengths; per cell the difference is at
    most 2 * sum |a_i| (pi ulp(u_i) + 2 * 2^-24 + 2^-23 + N 2^-24) (coherent_field_oracle.physics says which term is what)."""
    _, T, Rl, _ = _contributions(scene, mode, role, "received_power")
    field, bound = physics(T, Rl, inv, AMPS[amp])
    got, _ = _gpu(ctx, scene, mode, role, "received_power", inv, amp)
    err = np.abs(got.re.reshape(-1).astype(np.float64) + 1j * got.im.reshape(-1).astype(np.float64) - field)
    lit = bound > 0
    print(f"{scene} {mode} {role} {amp} inv={float(inv):g}: max error / bound {np.max(err[lit] / bound[lit]):.3f}")
    assert lit.sum() > lit.size // 3 and (err <= bound).all()
    assert np.abs(field).max() > 0 and (np.abs(field.imag) > 0).sum() > lit.size // 3


# ---- 4. the candidate mask and min_order ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("role", ["rx", "tx"])
def test_field_honours_the_candidate_mask_and_min_order(ctx, role):
    from differt2d_amd.engine import make_params

    walls, fixed, X, Y = _case("random7")
    allowed = np.ones(7, np.uint8)
    allowed[[2, 5]] = 0
    ctx.set_scene(walls)
    ctx.set_candidate_mask(allowed)
    try:
        ctx.set_grid(X, Y)
        got = ctx.coherent_field(make_params(min_order=0, max_order=2, grid_role=_role_id(role)), fixed, INV_20, "sqrt")
    finally:
        ctx.set_candidate_mask(None)
    everything = _oracle("random7", "hard", role, "received_power", INV_20, "sqrt")
    _same(got, _oracle("random7", "hard", role, "received_power", INV_20, "sqrt", 0, 2, (2, 5)))
    assert not np.array_equal(got.re, everything.re)
    # min_order = 1: the line of sight is left out
    got, _ = _gpu(ctx, "random7", "hsig", role, "received_power", INV_20, "linear", 1, 2)
    _same(got, _oracle("random7", "hsig", role, "received_power", INV_20, "linear", 1, 2))
    assert got.re.any() and not np.array_equal(got.total, _oracle("random7", "hsig", role, "received_power", INV_20, "linear").total)


# ---- 5. state and refusals ---------------------------------------------------------------------------------------------------------
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
    cf = ctx.coherent_field(params, fixed, INV_20, "sqrt")
    assert np.array_equal(ctx.get_map().view(np.uint32), before.view(np.uint32)) and before.any()  # still the previous sweep's map
    assert np.array_equal(ctx.get_profile(24).view(np.uint32), profile.view(np.uint32)) and profile.any()
    n = len(rec["cell"])
    again = {"cell": np.empty(n, np.int32), "valid": np.empty(n, F), "length": np.empty(n, F)}
    vp = lambda a: a.ctypes.data
    assert ctx._lib.d2d_get_valid_paths(ctx._ctx, n, vp(again["cell"]), None, None, None, None, vp(again["valid"]), vp(again["length"])) == 0
    assert n > 0 and all(np.array_equal(again[f].view(np.uint32), rec[f].view(np.uint32)) for f in again)
    top2 = ctx.get_strongest_paths()
    assert all(np.array_equal(a, b, equal_nan=a.dtype == np.float32) for a, b in zip(top, top2)) and top.power.any()
    _same(ctx.coherent_field(params, fixed, INV_20, "sqrt"), cf)  # two launches give the same bits
    _same(ctx.get_coherent_field(), cf)
    assert cf.re.any() and cf.im.any()
    assert np.array_equal(cf.total.view(np.uint32), top.total.view(np.uint32))
    # any of the three pointers may be NULL
    only_im = np.empty(ctx.shape, F)
    assert ctx._lib.d2d_get_coherent_field(ctx._ctx, None, vp(only_im), None) == 0 and np.array_equal(only_im, cf.im)
    # the other sinks leave the field alone in their turn
    ctx.strongest_paths(params, fixed, 2)
    ctx.launch(fused_params, fixed)
    _same(ctx.get_coherent_field(), cf)
    # another grid size on the same context: the result goes with the grid
    X2, Y2 = unit_grid(35, 18)
    ctx.set_grid(X2, Y2)
    with pytest.raises(Exception) as e:
        ctx.get_coherent_field()
    assert getattr(e.value, "status", None) == -5
    q = ctx.coherent_field(params, fixed, INV_20, "linear")
    ctx.launch(params, fixed)
    assert q.re.shape == q.im.shape == q.total.shape == (18, 35)
    assert np.array_equal(q.total.view(np.uint32), ctx.get_map().view(np.uint32))
    from strongest_paths_oracle import contributions

    _, T, Rl, _ = contributions(walls, fixed, X2, Y2, min_order=0, max_order=2, **MODES["hsig"])
    _same(q, CoherentField(*(a.reshape(X2.shape) for a in fold(T, Rl, INV_20, AMP_LINEAR))))


def _nothing_to_get(ctx):
    bufs = [np.zeros(ctx.shape, F) for _ in range(3)]
    rc = ctx._lib.d2d_get_coherent_field(ctx._ctx, *(b.ctypes.data for b in bufs))
    return rc == -5 and b"d2d_coherent_field_launch" in ctx._lib.d2d_last_error()


def _refused(ctx, status, word, params, fixed, inv=INV_20, amp="sqrt"):
    from differt2d_amd import _lib as L

    with pytest.raises(L.D2DError, match=word) as e:
        ctx.coherent_field(params, fixed, inv, amp)
    assert e.value.status == status, (e.value.status, str(e.value))
    assert isinstance(e.value, L.D2DUnsupported) == (status == -4)
    assert "d2d_coherent_field_launch" in str(e.value) or status == -5
    assert _nothing_to_get(ctx)  # ... and a refused launch leaves nothing to get


def test_loud_edges(ctx):
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import make_params

    walls, fixed, X, Y = _case("random7")
    ctx.set_scene(walls)
    ctx.set_reflection_coefs(None)
    ctx.set_grid(*unit_grid(19, 11))  # a grid this context has not seen: no result yet
    ctx.set_grid(X, Y)
    assert _nothing_to_get(ctx)
    kw = dict(min_order=0, max_order=2)
    ok = make_params(**kw)
    n0 = ctx.txg_fallbacks()
    _refused(ctx, -4, "sigmoid", make_params(approx=True, function="sigmoid", **kw), fixed)
    _refused(ctx, -4, "MinPath / FermatPath", make_params(solver="min", **kw), fixed)
    _refused(ctx, -4, "MinPath / FermatPath", make_params(solver="fermat", **kw), fixed)
    _refused(ctx, -4, "D2D_FUN_CUSTOM", make_params(fun="custom", **kw), fixed)
    _refused(ctx, -4, "D2D_OUT_ADD", make_params(out_mode=L.OUT_ADD, **kw), fixed)
    _refused(ctx, -4, "not culled", make_params(grid_role=L.GRID_TX, tol=0.6, **kw), fixed)
    ctx.set_option("txg_exhaustive", 1)
    try:
        _refused(ctx, -4, "txg_exhaustive", make_params(grid_role=L.GRID_TX, **kw), fixed)
    finally:
        ctx.set_option("txg_exhaustive", 0)
    # the per-object function: D2D_ERR_STATE without coefficients, works with them
    per_object = make_params(fun="received_power_per_object", **kw)
    _refused(ctx, -5, "d2d_set_reflection_coefs", per_object, fixed)
    ctx.set_reflection_coefs(COEF7)
    assert ctx.coherent_field(per_object, fixed, INV_20).re.any()
    ctx.set_reflection_coefs(None)
    # inv_wavelength and amplitude: each refusal after a launch that succeeded, so that it is seen to drop the result
    for inv in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf")):
        assert ctx.coherent_field(ok, fixed, INV_20).re.any() and not _nothing_to_get(ctx)
        _refused(ctx, -1, "inv_wavelength", ok, fixed, inv=inv)
    for amp in (2, -1):
        _refused(ctx, -1, "amplitude", ok, fixed, amp=amp)
    with pytest.raises(L.D2DError, match="amplitude") as e:
        ctx.coherent_field(ok, fixed, INV_20, "power")
    assert e.value.status == -1 and _nothing_to_get(ctx)
    assert ctx.txg_fallbacks() == n0
    # ... after all of which the context still works (the library's constants are taken as well as the names), and the grid's
    # change drops the result
    a = ctx.coherent_field(ok, fixed, INV_20, L.D2D_FIELD_AMP_LINEAR)
    _same(a, ctx.coherent_field(ok, fixed, INV_20, "linear"))
    assert a.re.any() and not _nothing_to_get(ctx)
    ctx.set_grid(*unit_grid(19, 11))
    assert _nothing_to_get(ctx)


# ---- 6. the phasor on the device ---------------------------------------------------------------------------------------------------
def test_selftest_phasor_equals_the_host_builds_bit_for_bit(ctx, tmp_path):
    f = np.concatenate([phasor_inputs(), np.array([np.nan], F)])
    c, s = ctx.selftest_phasor(f)
    wc, ws = phasor(f)
    # the g++ build of the same header (tests/native/coherent_field_host.cpp)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = str(tmp_path / "libcf_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                           os.path.join(root, "tests", "native", "coherent_field_host.cpp")])
    lib = C.CDLL(so)
    fp = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
    lib.cf_phasor.argtypes = [C.c_longlong, fp, fp, fp, fp, fp]
    lib.cf_phasor.restype = None
    hc, hs, hk, hg = (np.empty_like(f) for _ in range(4))
    lib.cf_phasor(f.size, f, hc, hs, hk, hg)
    ok = ~np.isnan(f)
    for name, got, want in (("cos / NumPy", c, wc), ("sin / NumPy", s, ws), ("cos / g++", c, hc), ("sin / g++", s, hs)):
        bad = got[ok].view(np.uint32) != want[ok].view(np.uint32)
        assert not bad.any(), f"{name}: {bad.sum()} of {bad.size} differ, first at f = {f[ok][bad][0]!r}"
    assert np.isnan(c[~ok]).all() and np.isnan(s[~ok]).all()
    assert c[f == 0].view(np.uint32).tolist() == [F(1).view(np.uint32)] * int((f == 0).sum()) and not s[f == 0].view(np.uint32).any()


# ---- 7. the Scene methods ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("role", ["rx", "tx"])
def test_scene_methods_mirror_the_context(ctx, role):
    from differt2d_amd import utils
    from differt2d_amd.engine import CoherentField as CF, make_params
    from differt2d_amd.geometry import Point
    from differt2d_amd.scene import Scene

    walls, fixed, X, Y = _case("random7")
    pts = {"a": Point(xy=fixed), "b": Point(xy=(F(1.0) - fixed).astype(F))}
    scene = Scene.from_walls_array(walls)
    scene = scene.with_transmitters(**pts) if role == "rx" else scene.with_receivers(**pts)
    method = scene.coherent_field_on_receivers_grid if role == "rx" else scene.coherent_field_on_transmitters_grid
    got = dict(method(X, Y, utils.received_power, dict(r_coef=0.4, height=0.2), wavelength=0.05, min_order=0, max_order=2, approx=True,
                      function="hard_sigmoid", filter_objects=lambda o: o is not scene.objects[3]))
    lin = dict(method(X, Y, utils.received_power, dict(r_coef=0.4, height=0.2), wavelength=0.05, amplitude="linear", min_order=0,
                      max_order=2, approx=True, function="hard_sigmoid", filter_objects=lambda o: o is not scene.objects[3]))
    assert list(got) == list(lin) == ["a", "b"]
    allowed = np.ones(7, np.uint8)
    allowed[3] = 0
    ctx.set_scene(walls)
    ctx.set_candidate_mask(allowed)
    ctx.set_grid(X, Y)
    params = make_params(min_order=0, max_order=2, r_coef=0.4, height=0.2, grid_role=_role_id(role), **MODES["hsig"])
    for name, pt in pts.items():
        assert isinstance(got[name], CF)
        _same(got[name], ctx.coherent_field(params, pt.xy, INV_20, "sqrt"))
        _same(lin[name], ctx.coherent_field(params, pt.xy, INV_20, "linear"))
        assert got[name].re.any() and got[name].im.any()
    ctx.set_candidate_mask(None)
    assert not np.array_equal(got["a"].re, got["b"].re) and not np.array_equal(got["a"].re, lin["a"].re)
    # field_power / fading_gain on the result: float64 re^2 + im^2, its ratio to the incoherent sum; received_power is never
    # negative, so with SQRT |field|^2 <= (sum sqrt t_i)^2 <= N sum t_i (Cauchy-Schwarz; N <= 57 candidates, fp32 roundings within 1e-5)
    a = got["a"]
    power, gain = utils.field_power(a), utils.fading_gain(a)
    assert power.dtype == gain.dtype == np.float64 and power.shape == gain.shape == a.total.shape
    assert np.array_equal(power, a.re.astype(np.float64) ** 2 + a.im.astype(np.float64) ** 2)
    lit = a.total > 0
    assert lit.any() and np.isnan(gain[a.total == 0]).all()
    assert np.array_equal(gain[lit], power[lit] / a.total[lit].astype(np.float64))
    assert (gain[lit] >= 0).all() and (gain[lit] <= 57 * (1 + 1e-5)).all()
    assert (gain[lit] > 1.05).any() and (gain[lit] < 0.95).any()  # paths interfere: in phase here, out of phase there
