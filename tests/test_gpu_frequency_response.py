"""The channel frequency response (include/d2d.h: d2d_frequency_response_launch; power_sink_kernel, FreqSink): per cell the coherent
field at every wavelength of a list, from one preparation of the culled sweep and one kernel pass per 8 entries.  Held bit for bit to
the oracle of ``tests/frequency_response_oracle.py`` (the coherent field's recipe, stacked per entry), to the existing single-wavelength
kernel plane by plane, to the fused map, to the float64 physics, and to its state rules and refusals.  The scenes and the cached
contributions are those of ``tests/test_gpu_strongest_paths.py`` (computed once per session); the frequency lists are
``inv_j = INV_20 * (1 + j / 64)``, and every comparison first asserts on the oracle's planes that they differ pairwise in bits and
that more than a third of every plane's ``im`` is non-zero (``frequency_response_oracle.guard``), so that a wrong chunk offset or a
reused wavelength cannot pass."""

import functools

import numpy as np
import pytest

from conftest import unit_grid
from coherent_field_oracle import AMP_LINEAR, AMP_SQRT
from frequency_response_oracle import FrequencyResponse, fold_list, guard, physics_list, wideband_physics
from test_gpu_strongest_paths import COEF7, MODES, _case, _contributions, _role_id

pytestmark = pytest.mark.gpu

F = np.float32
AMPS = {"sqrt": AMP_SQRT, "linear": AMP_LINEAR}
INV_20 = F(1) / F(0.05)
NF_MAX = 17
FUSED_FUNS = ["received_power", "length_squared", "length", "one", "received_power_per_object"]


def inv_list(nf):
    return (INV_20 * (F(1) + np.arange(nf, dtype=F) / F(64))).astype(F)


@pytest.fixture(scope="module")
def ctx():
    from differt2d_amd.engine import Context

    with Context(0) as c:
        yield c


@functools.lru_cache(maxsize=None)
def _oracle17(scene, mode, role, fun, amp, lo=0, hi=2, masked=()):
    """The oracle on the 17-entry list, guarded.  A plane is one fold of its own entry, so the planes of a shorter list, a permuted one
    or one with duplicates are these planes picked by entry (``_oracle``)."""
    _, T, Rl, _ = _contributions(scene, mode, role, fun, lo, hi, masked)
    shape = _case(scene)[2].shape
    re, im, total = fold_list(T, Rl, inv_list(NF_MAX), AMPS[amp])
    fr = FrequencyResponse(re.reshape((-1,) + shape), im.reshape((-1,) + shape), total.reshape(shape))
    guard(fr.re, fr.im)
    for a in fr:
        a.setflags(write=False)
    return fr


def _oracle(scene, mode, role, fun, amp, entries, **kw):
    """The oracle's planes for the entries ``inv_list(17)[entries]`` (a count means the first so many)."""
    fr = _oracle17(scene, mode, role, fun, amp, **kw)
    pick = np.arange(entries) if isinstance(entries, int) else np.asarray(entries)
    return FrequencyResponse(fr.re[pick], fr.im[pick], fr.total)


def _gpu(ctx, scene, mode, role, fun, inv, amp, lo=0, hi=2, **extra):
    from differt2d_amd.engine import make_params

    walls, fixed, X, Y = _case(scene)
    ctx.set_scene(walls)
    if fun == "received_power_per_object":
        ctx.set_reflection_coefs(COEF7)
        extra["height"] = 0.25
    ctx.set_grid(X, Y)
    params = make_params(min_order=lo, max_order=hi, fun=fun, grid_role=_role_id(role), **MODES[mode], **extra)
    return ctx.frequency_response(params, fixed, inv, amp), params


def _same(got, want):
    for name, g, w in zip(want._fields, got, want):
        assert g.dtype == w.dtype == np.float32 and g.shape == w.shape, (name, g.dtype, g.shape, w.dtype, w.shape)
        bad = np.ascontiguousarray(g).view(np.uint32) != np.ascontiguousarray(w).view(np.uint32)
        assert not bad.any(), f"{name}: {bad.sum()} of {bad.size} entries differ, first at {tuple(np.argwhere(bad)[0])}: {g[bad][0]!r} != {w[bad][0]!r}"


# ---- 1. bit for bit against the oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", [1, 8, 9, 17])
@pytest.mark.parametrize("amp", ["sqrt", "linear"])
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
@pytest.mark.parametrize("scene", ["random7", "obstacle"])
def test_planes_equal_the_oracle(ctx, scene, mode, role, amp, nf):
    """nf: a partial chunk, a full chunk, a full chunk plus one, two full chunks plus one."""
    want = _oracle(scene, mode, role, "received_power", amp, nf)
    got, _ = _gpu(ctx, scene, mode, role, "received_power", inv_list(nf), amp)
    assert got.re.shape == got.im.shape == (nf,) + want.total.shape
    _same(got, want)


# ---- 2. against the existing kernel, the fused map, the zero entry ----------------------------------------------------------------
@pytest.mark.parametrize("amp", ["sqrt", "linear"])
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
def test_every_plane_equals_the_single_wavelength_kernel(ctx, mode, role, amp):
    _oracle17("obstacle", mode, role, "received_power", amp)  # (the guard)
    inv = inv_list(NF_MAX)
    got, params = _gpu(ctx, "obstacle", mode, role, "received_power", inv, amp)
    fixed = _case("obstacle")[1]
    for j in range(NF_MAX):
        cf = ctx.coherent_field(params, fixed, inv[j], amp)
        _same(FrequencyResponse(got.re[j], got.im[j], got.total), FrequencyResponse(*cf))
    _same(ctx.get_frequency_response(), got)  # (which the 17 launches of the other sink did not touch)


@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
@pytest.mark.parametrize("fun", FUSED_FUNS)
def test_total_is_the_fused_map_and_a_zero_entry_with_linear_is_it_too(ctx, fun, mode, role):
    walls, fixed, X, Y = _case("random7")
    _oracle17("random7", mode, role, fun, "linear")  # (the guard, on this function's planes)
    inv = inv_list(NF_MAX).copy()
    inv[3] = inv[9] = 0.0  # one zero entry in the first chunk, one in the second
    try:
        got, params = _gpu(ctx, "random7", mode, role, fun, inv, "linear")
        ctx.launch(params, fixed)
        fused = ctx.get_map()
        root, _ = _gpu(ctx, "random7", mode, role, fun, inv_list(NF_MAX), "sqrt")
    finally:
        ctx.set_reflection_coefs(None)
    assert np.isfinite(fused).all() and np.count_nonzero(fused) > fused.size // 3
    for fr in (got, root):
        assert np.array_equal(fr.total.view(np.uint32), fused.view(np.uint32))
    for j in (3, 9):
        assert np.array_equal(got.re[j].view(np.uint32), fused.view(np.uint32))  # every phasor is (1, +0)
        assert not got.im[j].view(np.uint32).any()  # +0.0, not -0.0
    keep = [j for j in range(NF_MAX) if j not in (3, 9)]
    want = _oracle("random7", mode, role, fun, "linear", keep)
    _same(FrequencyResponse(got.re[keep], got.im[keep], got.total), want)
    if fun == "received_power_per_object":  # the negative and the zero coefficient are exercised
        cands, T, _, _ = _contributions("random7", mode, role, fun)
        through = lambda w: np.array([w in c for c in cands])
        assert (T[through(2)] < 0).any() and not T[through(6)].any()
        _same(root, _oracle("random7", mode, role, fun, "sqrt", NF_MAX))


# ---- 3. independence of the planes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
def test_planes_do_not_depend_on_the_rest_of_the_list(ctx, mode, role):
    inv = inv_list(NF_MAX)
    full, _ = _gpu(ctx, "obstacle", mode, role, "received_power", inv, "sqrt")
    _same(full, _oracle("obstacle", mode, role, "received_power", "sqrt", NF_MAX))
    # a permuted list gives permuted planes (a fixed permutation that moves every entry and crosses the chunks)
    perm = np.random.default_rng(5).permutation(NF_MAX)
    assert (perm != np.arange(NF_MAX)).sum() >= NF_MAX - 2 and (perm[:8] >= 8).any() and (perm[16] != 16)
    got, _ = _gpu(ctx, "obstacle", mode, role, "received_power", inv[perm], "sqrt")
    _same(got, FrequencyResponse(full.re[perm], full.im[perm], full.total))
    # duplicated entries give equal planes, within a chunk and across chunks
    dup = np.array([0, 5, 5, 2, 0, 7, 16, 16, 5, 0, 11, 2, 5, 16, 0, 0, 11])
    got, _ = _gpu(ctx, "obstacle", mode, role, "received_power", inv[dup], "sqrt")
    _same(got, FrequencyResponse(full.re[dup], full.im[dup], full.total))
    # a list's first 8 planes equal the 8-entry launch
    got, _ = _gpu(ctx, "obstacle", mode, role, "received_power", inv[:8], "sqrt")
    _same(got, FrequencyResponse(full.re[:8], full.im[:8], full.total))


# ---- 4. against physics in float64 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("amp", ["sqrt", "linear"])
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
@pytest.mark.parametrize("scene", ["random7", "obstacle"])
def test_planes_and_wideband_power_against_the_float64_sum_of_phasors(ctx, scene, mode, role, amp):
    """Every plane within coherent_field_oracle.physics' bound of sum a_i e^(-j 2 pi r_i inv_j) in float64; utils.wideband_power
    within the mean of b_j (2 |field_j| + b_j) of the float64 mean of |field_j|^2 (frequency_response_oracle.wideband_physics)."""
    from differt2d_amd.utils import frequency_response, wideband_power

    _oracle17(scene, mode, role, "received_power", amp)  # (the guard)
    _, T, Rl, _ = _contributions(scene, mode, role, "received_power")
    inv = inv_list(NF_MAX)
    field, bound = physics_list(T, Rl, inv, AMPS[amp])
    got, _ = _gpu(ctx, scene, mode, role, "received_power", inv, amp)
    h = frequency_response(got)
    assert h.dtype == np.complex64 and h.shape == got.re.shape
    err = np.abs(h.reshape(NF_MAX, -1).astype(np.complex128) - field)
    lit = bound > 0
    print(f"{scene} {mode} {role} {amp}: max error / bound {np.max(err[lit] / bound[lit]):.3f}")
    assert lit.sum() > lit.size // 3 and (err <= bound).all()
    assert (np.abs(field.imag) > 0).sum() > lit.size // 3
    power, pbound = wideband_physics(T, Rl, inv, AMPS[amp])
    wide = wideband_power(got).reshape(-1)
    assert wide.dtype == np.float64 and (np.abs(wide - power) <= pbound).all() and power.any()


# ---- 5. the candidate mask and min_order, one case per role -----------------------------------------------------------------------
@pytest.mark.parametrize("role", ["rx", "tx"])
def test_response_honours_the_candidate_mask_and_min_order(ctx, role):
    from differt2d_amd.engine import make_params

    walls, fixed, X, Y = _case("random7")
    inv = inv_list(9)
    allowed = np.ones(7, np.uint8)
    allowed[[2, 5]] = 0
    ctx.set_scene(walls)
    ctx.set_candidate_mask(allowed)
    try:
        ctx.set_grid(X, Y)
        got = ctx.frequency_response(make_params(min_order=0, max_order=2, grid_role=_role_id(role)), fixed, inv, "sqrt")
    finally:
        ctx.set_candidate_mask(None)
    everything = _oracle("random7", "hard", role, "received_power", "sqrt", 9)
    _same(got, _oracle("random7", "hard", role, "received_power", "sqrt", 9, lo=0, hi=2, masked=(2, 5)))
    assert not np.array_equal(got.re, everything.re)
    # min_order = 1: the line of sight is left out
    got, _ = _gpu(ctx, "random7", "hsig", role, "received_power", inv, "linear", 1, 2)
    _same(got, _oracle("random7", "hsig", role, "received_power", "linear", 9, lo=1, hi=2))
    assert got.re.any() and not np.array_equal(got.total, _oracle("random7", "hsig", role, "received_power", "linear", 9).total)


# ---- 6. state -----------------------------------------------------------------------------------------------------------------------
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
    top = ctx.strongest_paths(params, fixed, 8)
    cf = ctx.coherent_field(params, fixed, INV_20, "sqrt")
    inv = inv_list(NF_MAX)
    fr = ctx.frequency_response(params, fixed, inv, "sqrt")
    _same(fr, _oracle("random7", "hsig", "rx", "received_power", "sqrt", NF_MAX))
    assert np.array_equal(ctx.get_map().view(np.uint32), before.view(np.uint32)) and before.any()  # still the previous sweep's map
    assert np.array_equal(ctx.get_profile(24).view(np.uint32), profile.view(np.uint32)) and profile.any()
    top2 = ctx.get_strongest_paths()
    assert all(np.array_equal(a, b, equal_nan=a.dtype == np.float32) for a, b in zip(top, top2)) and top.power.any()
    cf2 = ctx.get_coherent_field()
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(cf, cf2)) and cf.im.any()
    _same(ctx.frequency_response(params, fixed, inv, "sqrt"), fr)  # two launches give the same bits
    _same(ctx.get_frequency_response(), fr)
    # any of the three pointers may be NULL
    vp = lambda a: a.ctypes.data
    only_im = np.empty((NF_MAX,) + tuple(ctx.shape), F)
    assert ctx._lib.d2d_get_frequency_response(ctx._ctx, None, vp(only_im), None) == 0 and np.array_equal(only_im, fr.im)
    only_total = np.empty(ctx.shape, F)
    assert ctx._lib.d2d_get_frequency_response(ctx._ctx, None, None, vp(only_total)) == 0 and np.array_equal(only_total, fr.total)
    # the other sinks leave the response alone in their turn
    ctx.strongest_paths(params, fixed, 2)
    ctx.coherent_field(params, fixed, INV_20, "linear")
    ctx.launch(fused_params, fixed)
    _same(ctx.get_frequency_response(), fr)
    # a launch with a smaller nf after a larger one returns the smaller shape
    small = ctx.frequency_response(params, fixed, inv[:3], "sqrt")
    assert small.re.shape == small.im.shape == (3,) + tuple(ctx.shape)
    _same(small, FrequencyResponse(fr.re[:3], fr.im[:3], fr.total))
    _same(ctx.get_frequency_response(), small)
    # another grid size on the same context: the result goes with the grid
    X2, Y2 = unit_grid(35, 18)
    ctx.set_grid(X2, Y2)
    with pytest.raises(Exception) as e:
        ctx.get_frequency_response()
    assert getattr(e.value, "status", None) == -5
    q = ctx.frequency_response(params, fixed, inv[:9], "linear")
    ctx.launch(params, fixed)
    assert q.re.shape == q.im.shape == (9, 18, 35) and q.total.shape == (18, 35)
    assert np.array_equal(q.total.view(np.uint32), ctx.get_map().view(np.uint32))
    from strongest_paths_oracle import contributions

    _, T, Rl, _ = contributions(walls, fixed, X2, Y2, min_order=0, max_order=2, **MODES["hsig"])
    re, im, total = fold_list(T, Rl, inv[:9], AMP_LINEAR)
    guard(re, im)
    _same(q, FrequencyResponse(re.reshape(9, 18, 35), im.reshape(9, 18, 35), total.reshape(18, 35)))


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------
def _nothing_to_get(ctx):
    # (no buffers: the state is answered before anything is copied, and a result, where there is one, has its own launch's nf planes)
    rc = ctx._lib.d2d_get_frequency_response(ctx._ctx, None, None, None)
    return rc == -5 and b"d2d_frequency_response_launch" in ctx._lib.d2d_last_error()


def _refused(ctx, status, word, params, fixed, inv=None, amp="sqrt"):
    from differt2d_amd import _lib as L

    ctx.launch(params_ok(), fixed)
    before = ctx.get_map()
    with pytest.raises(L.D2DError, match=word) as e:
        ctx.frequency_response(params, fixed, inv_list(9) if inv is None else inv, amp)
    assert e.value.status == status, (e.value.status, str(e.value))
    assert isinstance(e.value, L.D2DUnsupported) == (status == -4)
    assert "d2d_frequency_response_launch" in str(e.value) or status == -5
    assert _nothing_to_get(ctx)  # a refused launch leaves nothing to get ...
    assert np.array_equal(ctx.get_map().view(np.uint32), before.view(np.uint32)) and before.any()  # ... and the previous map as it was
    with pytest.raises(L.D2DError) as e:
        ctx.get_frequency_response()
    assert e.value.status == -5


def params_ok():
    from differt2d_amd.engine import make_params

    return make_params(min_order=0, max_order=2)


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
        ctx.get_frequency_response()
    assert e.value.status == -5
    kw = dict(min_order=0, max_order=2)
    ok = params_ok()
    want = _oracle("random7", "hard", "rx", "received_power", "sqrt", 9)
    n0 = ctx.txg_fallbacks()

    def launched():  # every refusal comes after a launch that succeeded, so that it is seen to drop the result
        _same(ctx.frequency_response(ok, fixed, inv_list(9)), want)
        assert not _nothing_to_get(ctx)

    for bad in (make_params(approx=True, function="sigmoid", **kw), ):
        launched()
        _refused(ctx, -4, "sigmoid", bad, fixed)
    for solver in ("min", "fermat"):
        launched()
        _refused(ctx, -4, "MinPath / FermatPath", make_params(solver=solver, **kw), fixed)
    launched()
    _refused(ctx, -4, "D2D_FUN_CUSTOM", make_params(fun="custom", **kw), fixed)
    launched()
    _refused(ctx, -4, "D2D_OUT_ADD", make_params(out_mode=L.OUT_ADD, **kw), fixed)
    # the per-object function: D2D_ERR_STATE without coefficients, works with them
    per_object = make_params(fun="received_power_per_object", **kw)
    launched()
    _refused(ctx, -5, "d2d_set_reflection_coefs", per_object, fixed)
    ctx.set_reflection_coefs(COEF7)
    assert ctx.frequency_response(per_object, fixed, inv_list(9)).re.any()
    ctx.set_reflection_coefs(None)
    # nf of 0 and of D2D_FREQ_MAX + 1
    assert L.D2D_FREQ_MAX == 1024
    for inv in (np.zeros(0, F), np.full(L.D2D_FREQ_MAX + 1, INV_20, F)):
        launched()
        _refused(ctx, -1, "nf in 1 .. 1024", ok, fixed, inv=inv)
    # a negative, a NaN and an infinite entry at index 0, at index 7 and at index 8 (the second chunk): the message names the index
    for at in (0, 7, 8):
        for bad in (-1.0, float("nan"), float("inf")):
            inv = inv_list(NF_MAX).copy()
            inv[at] = bad
            launched()
            _refused(ctx, -1, f"inv_wavelength.* at index {at}$", ok, fixed, inv=inv)
    # an unknown amplitude
    for amp in (2, -1):
        launched()
        _refused(ctx, -1, "amplitude", ok, fixed, amp=amp)
    launched()  # (an unknown name is refused by the Python layer, ahead of the library: its get then refuses as well)
    with pytest.raises(L.D2DError, match="amplitude") as e:
        ctx.frequency_response(ok, fixed, inv_list(9), "power")
    assert e.value.status == -1
    with pytest.raises(L.D2DError) as e:
        ctx.get_frequency_response()
    assert e.value.status == -5
    assert ctx.txg_fallbacks() == n0
    # ... after all of which the context still works (the library's constants are taken as well as the names), D2D_FREQ_MAX entries
    # are accepted (128 launches; the first and the last plane are entry 0's and entry 16's), and the grid's change drops the result
    a = ctx.frequency_response(ok, fixed, inv_list(9), L.D2D_FIELD_AMP_LINEAR)
    _same(a, ctx.frequency_response(ok, fixed, inv_list(9), "linear"))
    most = np.resize(inv_list(NF_MAX), L.D2D_FREQ_MAX)
    big = ctx.frequency_response(ok, fixed, most, "sqrt")
    full = _oracle("random7", "hard", "rx", "received_power", "sqrt", NF_MAX)
    pick = np.arange(L.D2D_FREQ_MAX) % NF_MAX
    _same(big, FrequencyResponse(full.re[pick], full.im[pick], full.total))
    assert not _nothing_to_get(ctx)
    ctx.set_grid(*unit_grid(19, 11))
    assert _nothing_to_get(ctx)


# ---- 8. the Scene methods -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("role", ["rx", "tx"])
def test_scene_methods_mirror_the_context(ctx, role):
    from differt2d_amd import utils
    from differt2d_amd.engine import FrequencyResponse as FR, make_params
    from differt2d_amd.geometry import Point
    from differt2d_amd.scene import Scene

    walls, fixed, X, Y = _case("random7")
    pts = {"a": Point(xy=fixed), "b": Point(xy=(F(1.0) - fixed).astype(F))}
    scene = Scene.from_walls_array(walls)
    scene = scene.with_transmitters(**pts) if role == "rx" else scene.with_receivers(**pts)
    response = scene.frequency_response_on_receivers_grid if role == "rx" else scene.frequency_response_on_transmitters_grid
    field = scene.coherent_field_on_receivers_grid if role == "rx" else scene.coherent_field_on_transmitters_grid
    common = dict(min_order=0, max_order=2, approx=True, function="hard_sigmoid", filter_objects=lambda o: o is not scene.objects[3])
    fk = dict(r_coef=0.4, height=0.2)
    inv = inv_list(9)
    got = dict(response(X, Y, utils.received_power, fk, inv_wavelengths=inv, **common))
    lin = dict(response(X, Y, utils.received_power, fk, inv_wavelengths=inv, amplitude="linear", **common))
    assert list(got) == list(lin) == ["a", "b"]
    allowed = np.ones(7, np.uint8)
    allowed[3] = 0
    ctx.set_scene(walls)
    ctx.set_candidate_mask(allowed)
    ctx.set_grid(X, Y)
    params = make_params(min_order=0, max_order=2, r_coef=0.4, height=0.2, grid_role=_role_id(role), **MODES["hsig"])
    for name, pt in pts.items():
        assert isinstance(got[name], FR)
        want = ctx.frequency_response(params, pt.xy, inv, "sqrt")
        if name == "a":
            guard(want.re, want.im)
        else:  # (from b, 34 of the 273 cells see a path at all: the planes still differ pairwise, and there im is not zero)
            planes = {want.re[j].tobytes() + want.im[j].tobytes() for j in range(len(inv))}
            assert len(planes) == len(inv) and 30 < np.count_nonzero(want.total) < 40
            assert all(np.count_nonzero(want.im[j]) == np.count_nonzero(want.total) for j in range(len(inv)))
        _same(got[name], want)
        _same(lin[name], ctx.frequency_response(params, pt.xy, inv, "linear"))
    ctx.set_candidate_mask(None)
    assert not np.array_equal(got["a"].re, got["b"].re) and not np.array_equal(got["a"].re, lin["a"].re)
    # wavelengths=[w] is coherent_field_on_*_grid(wavelength=w) bit for bit (float32(1) / float32(w), as the coherent field does);
    # a list of them is the single ones stacked
    ws = [0.05, 0.03, 0.07]
    many = dict(response(X, Y, utils.received_power, fk, wavelengths=ws, **common))
    for j, w in enumerate(ws):
        one = dict(response(X, Y, utils.received_power, fk, wavelengths=[w], **common))
        cf = dict(field(X, Y, utils.received_power, fk, wavelength=w, **common))
        for name in pts:
            assert one[name].re.shape == (1,) + X.shape and cf[name].im.any()
            _same(FR(one[name].re[0], one[name].im[0], one[name].total), FR(*cf[name]))
            _same(FR(many[name].re[j], many[name].im[j], many[name].total), FR(*cf[name]))
    # giving both lists or neither raises
    with pytest.raises(ValueError, match="exactly one"):
        response(X, Y, utils.received_power, fk, **common)
    with pytest.raises(ValueError, match="exactly one"):
        response(X, Y, utils.received_power, fk, wavelengths=ws, inv_wavelengths=inv, **common)
