"""The material response (include/d2d.h: d2d_material_response_launch; power_sink_kernel, MaterialSink): the frequency response with
every contribution multiplied by the Fresnel reflection coefficients of the walls it bounces off, from one preparation of the culled
sweep and one kernel pass per 8 wavelengths.  Held bit for bit to the oracle of ``tests/material_response_oracle.py`` (a NumPy
restatement of ``d2d_fresnel.hpp`` and of the definition's loop), to the fused map, to ``Context.frequency_response`` on the line of
sight, to its independence properties, to a closed form in float64 that does not go through the oracle, and to its state rules and
refusals.  The scenes are those of ``tests/test_gpu_strongest_paths.py`` plus the 5-wall and the 4-wall square (orders up to 3 and 4);
the lists are ``inv_j = 20 * (1 + j / 64)`` and the permittivities are lossy and differ per wall and per wavelength.  Every comparison
first asserts on the ORACLE's planes that the case can fail: the planes differ pairwise in bits, TE and TM differ, more than a third of
``im`` is non-zero and every order present contributes somewhere."""

import functools

import numpy as np
import pytest

import material_response_oracle as MO
from conftest import unit_grid
from frequency_response_oracle import guard
from test_gpu_strongest_paths import COEF7, MODES, _role_id
from test_gpu_strongest_paths import _case as _case3

pytestmark = pytest.mark.gpu

F = np.float32
AMPS = {"sqrt": MO.AMP_SQRT, "linear": MO.AMP_LINEAR}
POLS = {"te": MO.POL_TE, "tm": MO.POL_TM}
C = 8  # the chunk (asserted against the host's in tests/test_material_response_cpu.py)
NF_MAX = 2 * C + 1
NFS = [1, C, C + 1, 2 * C + 1]
FUSED_FUNS = ["received_power", "length_squared", "length", "one", "received_power_per_object"]
ORDERS = {"random7": (0, 2), "obstacle": (0, 2), "wall5": (0, 3), "square4": (0, 4)}
MR = MO.MaterialResponse


def inv_list(nf):
    return (F(20) * (F(1) + np.arange(nf, dtype=F) / F(64))).astype(F)


def eps_table(nf, n, shift=0.0):
    """Lossy, different per wall and per wavelength: complex64 ``[nf, n]``."""
    f, w = np.arange(nf)[:, None], np.arange(n)[None, :]
    return ((2.5 + 0.7 * w + 0.11 * f + shift) - 1j * (0.05 + 0.3 * w + 0.02 * f)).astype(np.complex64)


@pytest.fixture(scope="module")
def ctx():
    from differt2d_amd.engine import Context

    with Context(0) as c:
        yield c


@functools.lru_cache(maxsize=None)
def _case(scene):
    """(walls, fixed end point, X, Y): grids of 21 x 13 and 16 x 24 (edge patches with lanes outside the grid) and two small ones."""
    from oracle import ref as R

    if scene == "random7":
        return _case3("random7")  # 21 x 13
    if scene == "obstacle":
        return R.square_scene_with_obstacle_walls(), np.array([0.2, 0.2], F), *unit_grid(16, 24)
    if scene == "wall5":
        return R.square_scene_with_wall_walls(), np.array([0.2, 0.45], F), *unit_grid(11, 9)
    if scene == "square4":  # orders up to 4: the segment array is full
        return R.square_scene_walls(), np.array([0.3, 0.4], F), *unit_grid(10, 7)
    raise KeyError(scene)


@functools.lru_cache(maxsize=None)
def _contributions(scene, mode, role, fun="received_power", lo=None, hi=None, masked=()):
    walls, fixed, X, Y = _case(scene)
    lo = ORDERS[scene][0] if lo is None else lo
    hi = ORDERS[scene][1] if hi is None else hi
    out = MO.segment_contributions(walls, fixed, X, Y, min_order=lo, max_order=hi, fun=fun, grid_role=role, filter_nodes=set(masked) or None,
                                   **MODES[mode])
    for a in out[1:]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _oracle17(scene, mode, role, amp, pol, fun="received_power", lo=None, hi=None, masked=()):
    walls, _, X, _ = _case(scene)
    fr = MO.material_response(walls, None, X, None, inv_list(NF_MAX), eps_table(NF_MAX, len(walls)), POLS[pol], AMPS[amp],
                              contributions=_contributions(scene, mode, role, fun, lo, hi, masked))
    for a in fr:
        a.setflags(write=False)
    return fr


def _oracle(scene, mode, role, amp, pol, entries, **kw):
    fr = _oracle17(scene, mode, role, amp, pol, **kw)
    pick = np.arange(entries) if isinstance(entries, int) else np.asarray(entries)
    return MR(fr.re[pick], fr.im[pick], fr.total)


def _params(scene, mode, role, fun="received_power", lo=None, hi=None, **extra):
    from differt2d_amd.engine import make_params

    lo = ORDERS[scene][0] if lo is None else lo
    hi = ORDERS[scene][1] if hi is None else hi
    return make_params(min_order=lo, max_order=hi, fun=fun, grid_role=_role_id(role), **MODES[mode], **extra)


def _gpu(ctx, scene, mode, role, inv, eps, amp, pol, fun="received_power", **kw):
    walls, fixed, X, Y = _case(scene)
    ctx.set_scene(walls)
    extra = {}
    if fun == "received_power_per_object":
        ctx.set_reflection_coefs(COEF7)
        extra["height"] = 0.25
    ctx.set_grid(X, Y)
    params = _params(scene, mode, role, fun, **kw, **extra)
    return ctx.material_response(params, fixed, inv, eps, pol, amp), params


def _same(got, want):
    for name, g, w in zip(want._fields, got, want):
        assert g.dtype == w.dtype == np.float32 and g.shape == w.shape, (name, g.dtype, g.shape, w.dtype, w.shape)
        bad = np.ascontiguousarray(g).view(np.uint32) != np.ascontiguousarray(w).view(np.uint32)
        assert not bad.any(), f"{name}: {bad.sum()} of {bad.size} entries differ, first at {tuple(np.argwhere(bad)[0])}: {g[bad][0]!r} != {w[bad][0]!r}"


def _can_fail(scene, mode, role, amp):
    """On the oracle's planes: they differ pairwise, TE and TM differ, im is mostly non-zero, every order present contributes."""
    te, tm = (_oracle17(scene, mode, role, amp, pol) for pol in ("te", "tm"))
    for fr in (te, tm):
        guard(fr.re, fr.im)
        assert np.isfinite(fr.re).all() and np.isfinite(fr.im).all()
    assert (te.re != tm.re).sum() > te.re.size // 3 and np.array_equal(te.total.view(np.uint32), tm.total.view(np.uint32))
    cands, T, _, _ = _contributions(scene, mode, role)
    orders = np.array([len(c) for c in cands])
    for k in range(ORDERS[scene][0], ORDERS[scene][1] + 1):
        assert (T[orders == k] != 0).any(), (scene, k)


# ---- 1. bit for bit against the oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("amp", ["sqrt", "linear"])
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
@pytest.mark.parametrize("scene", ["random7", "obstacle", "wall5", "square4"])
def test_planes_equal_the_oracle(ctx, scene, mode, role, amp):
    """Both polarisations; nf: a partial chunk, a full chunk, a full chunk plus one, two full chunks plus one."""
    _can_fail(scene, mode, role, amp)
    n = len(_case(scene)[0])
    for pol in ("te", "tm"):
        for nf in NFS:
            want = _oracle(scene, mode, role, amp, pol, nf)
            got, _ = _gpu(ctx, scene, mode, role, inv_list(nf), eps_table(NF_MAX, n)[:nf], amp, pol)
            assert got.re.shape == got.im.shape == (nf,) + want.total.shape
            _same(got, want)


# ---- 2. the fused map, the line of sight --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
@pytest.mark.parametrize("fun", FUSED_FUNS)
def test_total_is_the_fused_map(ctx, fun, mode, role):
    walls, fixed, X, Y = _case("random7")
    try:
        got, params = _gpu(ctx, "random7", mode, role, inv_list(C + 1), eps_table(C + 1, 7), "linear", "tm", fun=fun)
        ctx.launch(params, fixed)
        fused = ctx.get_map()
    finally:
        ctx.set_reflection_coefs(None)
    assert np.isfinite(fused).all() and np.count_nonzero(fused) > fused.size // 3
    assert np.array_equal(got.total.view(np.uint32), fused.view(np.uint32)) and got.im.any()
    if fun in ("length_squared", "length", "one"):  # (test_planes_equal_the_oracle has received_power; the oracle folds no coefficients)
        _same(got, _oracle("random7", mode, role, "linear", "tm", C + 1, fun=fun))


@pytest.mark.parametrize("amp", ["sqrt", "linear"])
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
def test_line_of_sight_equals_the_frequency_response(ctx, mode, role, amp):
    """max_order = 0: G = (1, +0), so the planes are Context.frequency_response's bit for bit, whatever the table and the polarisation."""
    inv = inv_list(NF_MAX)
    for scene in ("random7", "obstacle"):
        n = len(_case(scene)[0])
        for pol in ("te", "tm"):
            got, params = _gpu(ctx, scene, mode, role, inv, eps_table(NF_MAX, n), amp, pol, lo=0, hi=0)
            want = ctx.frequency_response(params, _case(scene)[1], inv, amp)
            guard(want.re, want.im)
            _same(got, MR(*want))


# ---- 3. independence ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
def test_planes_depend_on_their_own_wavelength_and_row_alone(ctx, mode, role):
    inv, eps = inv_list(NF_MAX), eps_table(NF_MAX, 8)
    full, _ = _gpu(ctx, "obstacle", mode, role, inv, eps, "sqrt", "te")
    _same(full, _oracle("obstacle", mode, role, "sqrt", "te", NF_MAX))
    # a permuted list, its rows moved along, gives permuted planes (the permutation moves every entry and crosses the chunks)
    perm = np.random.default_rng(5).permutation(NF_MAX)
    assert (perm != np.arange(NF_MAX)).sum() >= NF_MAX - 2 and (perm[:8] >= 8).any()
    got, _ = _gpu(ctx, "obstacle", mode, role, inv[perm], eps[perm], "sqrt", "te")
    _same(got, MR(full.re[perm], full.im[perm], full.total))
    # duplicated entries give equal planes, within a chunk and across chunks
    dup = np.array([0, 5, 5, 2, 0, 7, 16, 16, 5, 0, 11, 2, 5, 16, 0, 0, 11])
    got, _ = _gpu(ctx, "obstacle", mode, role, inv[dup], eps[dup], "sqrt", "te")
    _same(got, MR(full.re[dup], full.im[dup], full.total))
    # a truncated list gives the leading planes
    got, _ = _gpu(ctx, "obstacle", mode, role, inv[:C], eps[:C], "sqrt", "te")
    _same(got, MR(full.re[:C], full.im[:C], full.total))
    # the wavelength moved without its row is another plane: the rows matter
    got, _ = _gpu(ctx, "obstacle", mode, role, inv[perm], eps, "sqrt", "te")
    assert not np.array_equal(got.re, full.re[perm])


@pytest.mark.parametrize("role", ["rx", "tx"])
def test_the_permittivity_of_an_untouched_wall_does_not_matter(ctx, role):
    """Walls 2 and 5 masked out of the candidates (they still occlude): their rows may hold anything allowed."""
    walls, fixed, X, Y = _case("random7")
    inv, eps = inv_list(C + 1), eps_table(NF_MAX, 7)[:C + 1]
    allowed = np.ones(7, np.uint8)
    allowed[[2, 5]] = 0
    other = eps.copy()
    other[:, 2] = 2.0**50 - 2.0**50 * 1j
    other[:, 5] = -3.0
    ctx.set_scene(walls)
    ctx.set_candidate_mask(allowed)
    try:
        ctx.set_grid(X, Y)
        params = _params("random7", "hsig", role)
        a = ctx.material_response(params, fixed, inv, eps, "tm", "sqrt")
        b = ctx.material_response(params, fixed, inv, other, "tm", "sqrt")
    finally:
        ctx.set_candidate_mask(None)
    _same(a, _oracle("random7", "hsig", role, "sqrt", "tm", C + 1, masked=(2, 5)))
    _same(b, a)
    everything, _ = _gpu(ctx, "random7", "hsig", role, inv, eps, "sqrt", "tm")
    assert not np.array_equal(a.re, everything.re)
    cands, T, _, _ = _contributions("random7", "hsig", role)
    w = next(int(c[0]) for c, t in zip(cands, T) if len(c) and t.any())  # a wall that some contributing candidate touches
    touched = eps.copy()
    touched[:, w] = -3.0
    c, _ = _gpu(ctx, "random7", "hsig", role, inv, touched, "sqrt", "tm")
    assert not np.array_equal(c.re, everything.re)  # (a wall that IS touched matters)


@pytest.mark.parametrize("pol", ["te", "tm"])
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
def test_constant_band_equals_per_row_tables_of_equal_rows(ctx, mode, role, pol):
    """One permittivity per wall for the whole band ([N], or equal rows: the host detects it and the kernel forms G once) against
    the per-row path: a table whose last row alone differs is not constant, and its leading planes are the same bits."""
    for scene in ("obstacle", "square4"):
        n = len(_case(scene)[0])
        inv = inv_list(NF_MAX)
        row = eps_table(1, n)[0]
        const, _ = _gpu(ctx, scene, mode, role, inv, row, "sqrt", pol)  # [N]
        rows = np.tile(row, (NF_MAX, 1))
        again, _ = _gpu(ctx, scene, mode, role, inv, rows, "sqrt", pol)  # [nf, N], equal rows
        _same(again, const)
        rows[-1] = eps_table(2, n)[1]
        mixed, _ = _gpu(ctx, scene, mode, role, inv, rows, "sqrt", pol)  # the per-row path
        _same(MR(mixed.re[:-1], mixed.im[:-1], mixed.total), MR(const.re[:-1], const.im[:-1], const.total))
        assert not np.array_equal(mixed.re[-1], const.re[-1])
        # a row that differs in the sign of a zero alone is another table
        real = np.tile(np.full(n, 4 - 0j, np.complex64), (C + 1, 1))
        a, _ = _gpu(ctx, scene, mode, role, inv[:C + 1], real, "sqrt", pol)
        signed = real.copy()
        signed.imag[C] = -0.0
        b, _ = _gpu(ctx, scene, mode, role, inv[:C + 1], signed, "sqrt", pol)
        _same(MR(b.re[:C], b.im[:C], b.total), MR(a.re[:C], a.im[:C], a.total))
        # and the oracle has the constant band too
        cands = _contributions(scene, mode, role)
        want = MO.material_response(_case(scene)[0], None, _case(scene)[2], None, inv, np.tile(row, (NF_MAX, 1)), POLS[pol], MO.AMP_SQRT,
                                    contributions=cands)
        _same(const, want)


# ---- 4. the header on the device ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pol", ["te", "tm"])
def test_selftest_fresnel_equals_the_restatement_by_bits(ctx, pol):
    er, ei, c = MO.fresnel_inputs()
    gr, gi = ctx.selftest_fresnel(er, ei, c, pol)
    wr, wi = MO.fresnel(er, ei, c, POLS[pol])
    assert er.size > 60000 and np.isnan(wr).any()
    for name, g, w in (("gr", gr, wr), ("gi", gi, wi)):
        ok = MO.same_bits(g, w)
        assert ok.all(), (name, int((~ok).sum()), int(np.flatnonzero(~ok)[0]))


# ---- 5. a closed form, independent of the oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pol", ["te", "tm"])
@pytest.mark.parametrize("role", ["rx", "tx"])
def test_one_wall_closed_form_in_float64(ctx, role, pol):
    """One wall, order 1 alone, fun = one, LINEAR, hard validity: every lit cell holds G(theta) e^(-j 2 pi r / lambda), compared with
    utils.fresnel_coefficient on float64 geometry within the bound that material_response_oracle's docstring derives (observed on
    an MI355X: max error / bound 0.07 - 0.12 over the four cases)."""
    from differt2d_amd.engine import make_params
    from differt2d_amd.utils import fresnel_coefficient

    walls = np.array([[[0.0, 0.0], [1.0, 0.0]]], F)
    fixed = np.array([0.3, 0.5], F)
    X, Y = unit_grid(21, 13)
    Y = (Y * F(0.9) + F(0.1)).astype(F)  # off the wall
    inv = inv_list(C + 1)
    eps = np.array([[5.31 - 0.59j * (1 + 0.1 * j)] for j in range(C + 1)], np.complex64)
    ctx.set_scene(walls)
    ctx.set_grid(X, Y)
    params = make_params(min_order=1, max_order=1, fun="one", grid_role=_role_id(role))
    got = ctx.material_response(params, fixed, inv, eps, pol, "linear")
    lit = got.total == 1
    assert lit.sum() > lit.size // 2 and set(np.unique(got.total)) <= {F(0), F(1)}
    # float64 geometry: the image of the fixed point in y = 0
    x0, y0 = fixed.astype(np.float64)
    gx, gy = X.astype(np.float64), Y.astype(np.float64)
    r = np.hypot(gx - x0, gy + y0)
    cos = (gy + y0) / r
    hit_x = x0 + (gx - x0) * y0 / (gy + y0)
    d_in = np.hypot(hit_x - (x0 if role == "rx" else gx), y0 if role == "rx" else gy)  # TX -> wall
    e64 = eps.astype(np.complex128)[:, 0]
    worst = 0.0
    for j in range(C + 1):
        want = fresnel_coefficient(e64[j], cos, pol) * np.exp(-2j * np.pi * r * float(inv[j]))
        bound = MO.closed_form_bound(r, float(inv[j]), d_in, 1.0, MO.dg_dc(e64[j], cos, POLS[pol]))
        err = np.maximum(np.abs(got.re[j] - want.real), np.abs(got.im[j] - want.imag))
        worst = max(worst, float((err / bound)[lit].max()))
        assert (err[lit] <= bound[lit]).all(), (j, float((err / bound)[lit].max()))
        assert not got.re[j][~lit].any() and not got.im[j][~lit].any()
    print(f"closed form {role} {pol}: max error / bound {worst:.3f}")
    assert np.abs(got.im[0][lit]).min() >= 0 and np.count_nonzero(got.im[0]) > lit.sum() // 2


# ---- 6. state -----------------------------------------------------------------------------------------------------------------------
def test_launch_leaves_the_other_results_alone_and_repeats_itself(ctx):
    from differt2d_amd.engine import make_params

    walls, fixed, X, Y = _case("random7")
    ctx.set_scene(walls)
    ctx.set_grid(X, Y)
    fused_params = make_params(min_order=0, max_order=2, fun="length")
    ctx.launch(fused_params, fixed)
    before = ctx.get_map()
    params = _params("random7", "hsig", "rx")
    inv, eps = inv_list(NF_MAX), eps_table(NF_MAX, 7)
    top = ctx.strongest_paths(params, fixed, 8)
    cf = ctx.coherent_field(params, fixed, 20.0, "sqrt")
    fr = ctx.frequency_response(params, fixed, inv, "sqrt")
    mr = ctx.material_response(params, fixed, inv, eps, "te", "sqrt")
    _same(mr, _oracle("random7", "hsig", "rx", "sqrt", "te", NF_MAX))
    assert not np.array_equal(mr.re, fr.re) and np.array_equal(mr.total.view(np.uint32), fr.total.view(np.uint32))
    # the other products' results are still readable and unchanged
    assert np.array_equal(ctx.get_map().view(np.uint32), before.view(np.uint32)) and before.any()
    assert all(np.array_equal(a, b, equal_nan=a.dtype == np.float32) for a, b in zip(top, ctx.get_strongest_paths())) and top.power.any()
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(cf, ctx.get_coherent_field()))
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(fr, ctx.get_frequency_response()))
    # the same launch gives the same bits twice, and after other products ran on the context
    _same(ctx.material_response(params, fixed, inv, eps, "te", "sqrt"), mr)
    ctx.strongest_paths(params, fixed, 2)
    ctx.frequency_response(params, fixed, inv[:3], "linear")
    ctx.launch(fused_params, fixed)
    _same(ctx.get_material_response(), mr)
    _same(ctx.material_response(params, fixed, inv, eps, "te", "sqrt"), mr)
    # any of the three pointers may be NULL
    vp = lambda a: a.ctypes.data
    only_im = np.empty((NF_MAX,) + tuple(ctx.shape), F)
    assert ctx._lib.d2d_get_material_response(ctx._ctx, None, vp(only_im), None) == 0 and np.array_equal(only_im, mr.im)
    only_total = np.empty(ctx.shape, F)
    assert ctx._lib.d2d_get_material_response(ctx._ctx, None, None, vp(only_total)) == 0 and np.array_equal(only_total, mr.total)
    # a smaller nf after a larger one returns the smaller shape
    small = ctx.material_response(params, fixed, inv[:3], eps[:3], "te", "sqrt")
    _same(small, MR(mr.re[:3], mr.im[:3], mr.total))
    # the resident scene set again keeps the result; another scene drops it (it depends on the walls), and so does another grid
    ctx.set_scene(walls)
    _same(ctx.get_material_response(), small)
    ctx.set_scene(walls[:6])
    with pytest.raises(Exception) as e:
        ctx.get_material_response()
    assert getattr(e.value, "status", None) == -5 and "d2d_material_response_launch" in str(e.value)
    ctx.set_scene(walls)
    with pytest.raises(Exception) as e:
        ctx.get_material_response()
    assert getattr(e.value, "status", None) == -5
    _same(ctx.material_response(params, fixed, inv[:3], eps[:3], "te", "sqrt"), small)
    ctx.set_grid(*unit_grid(35, 18))
    with pytest.raises(Exception) as e:
        ctx.get_material_response()
    assert getattr(e.value, "status", None) == -5
    q = ctx.material_response(params, fixed, inv[:C + 1], eps[:C + 1], "tm", "linear")
    ctx.launch(params, fixed)
    assert q.re.shape == q.im.shape == (C + 1, 18, 35) and np.array_equal(q.total.view(np.uint32), ctx.get_map().view(np.uint32))


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------
def test_loud_edges(ctx):
    """Every refusal by status and a word of its reason; a refused launch leaves the previous result readable and unchanged."""
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import make_params

    walls, fixed, X, Y = _case("random7")
    ctx.set_scene(walls)
    ctx.set_reflection_coefs(None)
    ctx.set_grid(*unit_grid(19, 11))  # a grid this context has not seen: no result yet
    ctx.set_grid(X, Y)
    rc = ctx._lib.d2d_get_material_response(ctx._ctx, None, None, None)
    assert rc == -5 and b"d2d_material_response_launch" in ctx._lib.d2d_last_error()
    kw = dict(min_order=0, max_order=2)
    ok = make_params(**kw)
    inv, eps = inv_list(C + 1), eps_table(NF_MAX, 7)[:C + 1]
    want = _oracle("random7", "hard", "rx", "sqrt", "te", C + 1)
    _same(ctx.material_response(ok, fixed, inv, eps, "te", "sqrt"), want)
    n0 = ctx.txg_fallbacks()

    def refused(status, word, params=ok, inv=inv, eps=eps, pol="te", amp="sqrt"):
        with pytest.raises(L.D2DError, match=word) as e:
            ctx.material_response(params, fixed, inv, eps, pol, amp)
        assert e.value.status == status, (e.value.status, str(e.value))
        assert isinstance(e.value, L.D2DUnsupported) == (status == -4)
        _same(ctx.get_material_response(), want)  # the previous result is still there

    refused(-4, "sigmoid", make_params(approx=True, function="sigmoid", **kw))
    for solver in ("min", "fermat"):
        refused(-4, "MinPath / FermatPath", make_params(solver=solver, **kw))
    refused(-4, "D2D_FUN_CUSTOM.*d2d_trace_paths", make_params(fun="custom", **kw))
    refused(-4, "D2D_OUT_ADD", make_params(out_mode=L.OUT_ADD, **kw))
    refused(-5, "d2d_set_reflection_coefs", make_params(fun="received_power_per_object", **kw))
    for bad in (np.zeros(0, F), np.full(L.D2D_FREQ_MAX + 1, 20.0, F)):
        refused(-1, "nf in 1 .. 1024", inv=bad, eps=eps_table(1, 7)[0])
    for at in (0, C - 1, C):
        for bad in (-1.0, float("nan"), float("inf")):
            b = inv.copy()
            b[at] = bad
            refused(-1, f"inv_wavelength.* at index {at}$", inv=b)
    for amp in (2, -1):
        refused(-1, "amplitude", amp=amp)
    for pol in (2, -1):
        refused(-1, "polarization", pol=pol)
    refused(-1, "n_objects", eps=eps_table(C + 1, 6))
    refused(-1, "n_objects", eps=eps_table(C + 1, 8))
    for f, w in ((0, 0), (C - 1, 6), (C, 3)):
        for bad in (np.nan, np.inf, -np.inf, 2.0**51, -2.0**51):
            for part in ("re", "im"):
                b = eps.copy()
                if part == "re":
                    b[f, w] = complex(bad, b[f, w].imag)
                else:  # (a finite imaginary part is kept negative, so that its magnitude is what is refused)
                    b[f, w] = complex(b[f, w].real, -abs(bad) if np.isfinite(bad) else bad)
                refused(-1, f"permittivity.* at wavelength index {f}, wall index {w}$", eps=b)
        b = eps.copy()
        b[f, w] = b[f, w].real + 0.25j
        refused(-1, f"Im eps <= 0.* at wavelength index {f}, wall index {w}$", eps=b)
    rc = ctx._lib.d2d_material_response_launch(ctx._ctx, ok, fixed, inv.ctypes.data, C + 1, 0, 0, None, 7)
    assert rc == -1 and b"NULL" in ctx._lib.d2d_last_error()
    _same(ctx.get_material_response(), want)
    # the Python layer refuses unknown names and shapes ahead of the library
    for call in (lambda: ctx.material_response(ok, fixed, inv, eps, "circular"), lambda: ctx.material_response(ok, fixed, inv, eps, "te", "power"),
                 lambda: ctx.material_response(ok, fixed, inv, eps[:3])):
        with pytest.raises(L.D2DError) as e:
            call()
        assert e.value.status == -1
    _same(ctx.get_material_response(), want)
    assert ctx.txg_fallbacks() == n0
    # ... after all of which the context still works; the limits pass: components of 2^50, +0 imaginary parts, D2D_FREQ_MAX entries
    edge = eps.copy()
    edge[0, 0] = 2.0**50 - 2.0**50 * 1j
    edge[1, 1] = 3 + 0j
    assert np.isfinite(ctx.material_response(ok, fixed, inv, edge, L.D2D_POL_TM, L.D2D_FIELD_AMP_LINEAR).re).all()
    most = np.resize(inv_list(NF_MAX), L.D2D_FREQ_MAX)
    pick = np.arange(L.D2D_FREQ_MAX) % NF_MAX
    big = ctx.material_response(ok, fixed, most, eps_table(NF_MAX, 7)[pick], "te", "sqrt")
    full = _oracle("random7", "hard", "rx", "sqrt", "te", NF_MAX)
    _same(big, MR(full.re[pick], full.im[pick], full.total))


# ---- 8. the Scene methods -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("role", ["rx", "tx"])
def test_scene_methods_mirror_the_context(ctx, role):
    import dataclasses

    from differt2d_amd import utils
    from differt2d_amd.engine import FrequencyResponse as FR, make_params
    from differt2d_amd.geometry import Point, Wall
    from differt2d_amd.scene import Scene

    walls, fixed, X, Y = _case("random7")
    pts = {"a": Point(xy=fixed), "b": Point(xy=(F(1.0) - fixed).astype(F))}
    scene = Scene.from_walls_array(walls)
    scene = scene.with_transmitters(**pts) if role == "rx" else scene.with_receivers(**pts)
    response = scene.material_response_on_receivers_grid if role == "rx" else scene.material_response_on_transmitters_grid
    common = dict(min_order=0, max_order=2, approx=True, function="hard_sigmoid", filter_objects=lambda o: o is not scene.objects[3])
    fk = dict(r_coef=1.0, height=0.2)
    inv = inv_list(C + 1)
    eps = eps_table(C + 1, 7)
    got = dict(response(X, Y, utils.received_power, fk, inv_wavelengths=inv, permittivity=eps, polarization="tm", **common))
    band = dict(response(X, Y, utils.received_power, fk, inv_wavelengths=inv, permittivity=eps[0], amplitude="linear", **common))
    assert list(got) == list(band) == ["a", "b"]
    allowed = np.ones(7, np.uint8)
    allowed[3] = 0
    ctx.set_scene(walls)
    ctx.set_candidate_mask(allowed)
    ctx.set_grid(X, Y)
    params = make_params(min_order=0, max_order=2, r_coef=1.0, height=0.2, grid_role=_role_id(role), **MODES["hsig"])
    try:
        for name, pt in pts.items():
            assert isinstance(got[name], FR)
            _same(got[name], ctx.material_response(params, pt.xy, inv, eps, "tm", "sqrt"))
            _same(band[name], ctx.material_response(params, pt.xy, inv, eps[0], "te", "linear"))
        assert got["a"].im.any() and not np.array_equal(got["a"].re, got["b"].re)
        # wavelengths= becomes float32(1) / float32(w), as the frequency response does
        ws = [0.05, 0.03, 0.07]
        many = dict(response(X, Y, utils.received_power, fk, wavelengths=ws, permittivity=eps[0], **common))
        _same(many["a"], ctx.material_response(params, pts["a"].xy, F(1) / np.asarray(ws, F), eps[0], "te", "sqrt"))
    finally:
        ctx.set_candidate_mask(None)
    # permittivity=None: read from the objects' attributes, a scalar or one value per wavelength
    @dataclasses.dataclass(frozen=True, eq=False)
    class Material(Wall):
        permittivity: object = None

    objs = [Material(xys=o.xys, permittivity=complex(eps[0, j]) if j % 2 else eps[:, j].copy()) for j, o in enumerate(scene.objects)]
    with_eps = dataclasses.replace(scene, objects=objs)
    response2 = with_eps.material_response_on_receivers_grid if role == "rx" else with_eps.material_response_on_transmitters_grid
    table = eps.copy()
    table[:, 1::2] = eps[0, 1::2]
    common2 = dict(common, filter_objects=lambda o: o is not with_eps.objects[3])
    attr = dict(response2(X, Y, utils.received_power, fk, inv_wavelengths=inv, polarization="tm", **common2))
    explicit = dict(response(X, Y, utils.received_power, fk, inv_wavelengths=inv, permittivity=table, polarization="tm", **common))
    for name in pts:
        _same(attr[name], explicit[name])
    bare = dataclasses.replace(with_eps, objects=objs[:4] + [Wall(xys=objs[4].xys)] + objs[5:])
    response3 = bare.material_response_on_receivers_grid if role == "rx" else bare.material_response_on_transmitters_grid
    with pytest.raises(ValueError, match="object 4 .*no permittivity"):
        next(iter(response3(X, Y, utils.received_power, fk, inv_wavelengths=inv, **common)))
