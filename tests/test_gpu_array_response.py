"""The array response (include/d2d.h: d2d_array_response_launch; power_sink_kernel, ArraySink): per cell the nr x nt channel matrix,
every contribution of the fused sweep as a complex amplitude whose phase is steered per antenna pair by the plane-wave model.  Held
bit for bit to the oracle recipe of ``tests/array_response_oracle.py`` (which ``tests/test_array_response_cpu.py`` pins to the
coherent field's recipe and to the g++ build of the steering header), to ``Context.coherent_field``, to the fused map, to the float64
physics, and to its state rules and refusals.  The scenes and the cached contributions are those of
``tests/test_gpu_strongest_paths.py`` and ``tests/test_gpu_power_angle.py`` (computed once per session)."""

import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from array_response_oracle import AMP_LINEAR, AMP_SQRT, ArrayResponse, directed, fold, physics, steer_inputs, steer_phase, unit_dir
from conftest import unit_grid
from test_gpu_power_angle import _directed
from test_gpu_strongest_paths import COEF7, MODES, _case, _contributions, _role_id

pytestmark = pytest.mark.gpu

F = np.float32
AMPS = {"sqrt": AMP_SQRT, "linear": AMP_LINEAR}
WL = F(0.05)
INV_20 = F(1) / WL  # wavelength 0.05: what Scene.array_response_on_*_grid hands to the library
FUSED_FUNS = ["received_power", "length_squared", "length", "one", "received_power_per_object"]


def _elements(n, seed):
    """``n`` offsets of a fraction of the wavelength to two wavelengths, the first one zero, no two alike."""
    rng = np.random.default_rng(seed)
    r = rng.uniform(0.1, 2.0, n) * float(WL)
    th = rng.uniform(0, 2 * np.pi, n)
    e = np.stack([r * np.cos(th), r * np.sin(th)], axis=1).astype(F)
    e[0] = 0
    return e


# nr x nt: 1 x 1 (the zero pair alone), 3 x 4 and 8 x 8 (both limits)
SHAPES = {"1x1": (_elements(1, 1), _elements(1, 2)), "3x4": (_elements(4, 3), _elements(3, 4)), "8x8": (_elements(8, 5), _elements(8, 6))}


@pytest.fixture(scope="module")
def ctx():
    from differt2d_amd.engine import Context

    with Context(0) as c:
        yield c


def _joined(scene, mode, role, fun="received_power", lo=0, hi=2, masked=()):
    _, T, Rl, _ = _contributions(scene, mode, role, fun, lo, hi, masked)
    _, T2, D = _directed(scene, mode, role, fun, lo, hi, masked)
    assert np.array_equal(T.view(np.uint32), T2.view(np.uint32))
    return T, Rl, D


@functools.lru_cache(maxsize=None)
def _oracle(scene, mode, role, fun, amp, shape, lo=0, hi=2, masked=()):
    T, Rl, D = _joined(scene, mode, role, fun, lo, hi, masked)
    etx, erx = SHAPES[shape]
    grid = _case(scene)[2].shape
    re, im, total = fold(T, Rl, D, INV_20, AMPS[amp], etx, erx)
    out = ArrayResponse(re.reshape(re.shape[:2] + grid), im.reshape(im.shape[:2] + grid), total.reshape(grid))
    for a in out:
        a.setflags(write=False)
    return out


def _setup(ctx, scene, fun="received_power"):
    walls, fixed, X, Y = _case(scene)
    ctx.set_scene(walls)
    if fun == "received_power_per_object":
        ctx.set_reflection_coefs(COEF7)
    ctx.set_grid(X, Y)
    return fixed


def _params(mode, role, fun="received_power", lo=0, hi=2, **extra):
    from differt2d_amd.engine import make_params

    if fun == "received_power_per_object":
        extra["height"] = 0.25
    return make_params(min_order=lo, max_order=hi, fun=fun, grid_role=_role_id(role), **MODES[mode], **extra)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, want):
    for name, g, w in zip(want._fields, got, want):
        assert g.dtype == w.dtype == np.float32 and g.shape == w.shape, (name, g.dtype, g.shape, w.dtype, w.shape)
        bad = _bits(g) != _bits(w)
        assert not bad.any(), f"{name}: {bad.sum()} of {bad.size} values differ, first at {tuple(np.argwhere(bad)[0])}: {g[bad][0]!r} != {w[bad][0]!r}"


# ---- 0. the oracle alone: the comparison below does not pass on empty ground -------------------------------------------------------
@pytest.mark.parametrize("scene", ["random7", "obstacle"])
def test_oracle_planes_differ_pairwise_and_carry_phase(scene):
    want = _oracle(scene, "hard", "rx", "received_power", "sqrt", "3x4")
    nr, nt = want.re.shape[:2]
    planes = [(i, j) for i in range(nr) for j in range(nt)]
    for a in range(len(planes)):
        for b in range(a + 1, len(planes)):
            pa, pb = planes[a], planes[b]
            assert not np.array_equal(_bits(want.re[pa]), _bits(want.re[pb])) and not np.array_equal(_bits(want.im[pa]), _bits(want.im[pb])), (pa, pb)
    for i, j in planes[1:]:
        assert np.count_nonzero(want.im[i, j]) > want.im[i, j].size // 3, (i, j)


# ---- 1. bit for bit against the oracle recipe -----------------------------------------------------------------------------------
@pytest.mark.parametrize("amp", ["sqrt", "linear"])
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
@pytest.mark.parametrize("scene,shape", [("random7", "1x1"), ("random7", "3x4"), ("obstacle", "3x4"), ("random7", "8x8"), ("square_centre", "3x4")])
def test_matrix_equals_the_oracle_recipe(ctx, scene, shape, mode, role, amp):
    want = _oracle(scene, mode, role, "received_power", amp, shape)
    etx, erx = SHAPES[shape]
    assert np.count_nonzero(want.im) > want.im.size // 3 and np.count_nonzero(want.re) > want.re.size // 3
    fixed = _setup(ctx, scene)
    got = ctx.array_response(_params(mode, role), fixed, INV_20, etx, erx, amp)
    assert got.re.shape == (erx.shape[0], etx.shape[0]) + _case(scene)[2].shape
    _same(got, want)


# ---- 2. identities ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("amp", ["sqrt", "linear"])
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
@pytest.mark.parametrize("scene", ["random7", "obstacle", "square_centre"])
def test_zero_offset_pair_is_the_coherent_field(ctx, scene, mode, role, amp):
    """Offsets of (+-0, +-0) at both ends: Context.coherent_field bit for bit wherever no contribution lacks a direction -- everywhere
    in random7 and obstacle; in square_centre the cell that IS the fixed end point, [4, 4], has a line of sight without one, and
    exactly that cell's re differs."""
    fixed = _setup(ctx, scene)
    params = _params(mode, role)
    etx = np.array([[0.03, 0.01], [-0.0, 0.0]], F)
    erx = np.array([[0.0, -0.0], [0.02, -0.07], [-0.0, -0.0]], F)
    got = ctx.array_response(params, fixed, INV_20, etx, erx, amp)
    cf = ctx.coherent_field(params, fixed, INV_20, amp)
    assert np.array_equal(_bits(got.total), _bits(cf.total)) and cf.im.any()
    for i in (0, 2):
        dre, dim = _bits(got.re[i, 1]) != _bits(cf.re), _bits(got.im[i, 1]) != _bits(cf.im)
        if scene == "square_centre":
            assert np.argwhere(dre).tolist() == [[4, 4]] and np.argwhere(dre | dim).tolist() == [[4, 4]]
        else:
            assert not dre.any() and not dim.any()
    assert not np.array_equal(_bits(got.im[1, 1]), _bits(cf.im)) and not np.array_equal(_bits(got.im[0, 0]), _bits(cf.im))


@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
@pytest.mark.parametrize("fun", FUSED_FUNS)
def test_total_is_the_fused_map_for_every_fused_function(ctx, fun, mode, role):
    etx, erx = SHAPES["3x4"]
    try:
        fixed = _setup(ctx, "random7", fun)
        params = _params(mode, role, fun)
        got = ctx.array_response(params, fixed, INV_20, etx, erx, "sqrt")
        ctx.launch(params, fixed)
        fused = ctx.get_map()
    finally:
        ctx.set_reflection_coefs(None)
    assert np.isfinite(fused).all() and np.count_nonzero(fused) > fused.size // 3
    assert np.array_equal(_bits(got.total), _bits(fused)) and np.count_nonzero(got.im) > 0
    if fun != "received_power":  # (the signed and the zero coefficient included)
        _same(got, _oracle("random7", mode, role, fun, "sqrt", "3x4"))


@pytest.mark.parametrize("role", ["rx", "tx"])
def test_entries_depend_on_their_own_elements_only(ctx, role):
    """Permuted, duplicated and truncated element lists give permuted, equal and leading planes, bit for bit."""
    etx, erx = SHAPES["3x4"]
    fixed = _setup(ctx, "random7")
    params = _params("hsig", role)
    base = ctx.array_response(params, fixed, INV_20, etx, erx, "sqrt")
    pt, pr = [2, 0, 3, 1], [1, 2, 0]
    perm = ctx.array_response(params, fixed, INV_20, etx[pt], erx[pr], "sqrt")
    _same(perm, ArrayResponse(base.re[pr][:, pt], base.im[pr][:, pt], base.total))
    dup = ctx.array_response(params, fixed, INV_20, etx[[1, 3, 1, 1, 0, 3, 2, 1]], erx[[2, 2]], "sqrt")
    _same(dup, ArrayResponse(base.re[[2, 2]][:, [1, 3, 1, 1, 0, 3, 2, 1]], base.im[[2, 2]][:, [1, 3, 1, 1, 0, 3, 2, 1]], base.total))
    cut = ctx.array_response(params, fixed, INV_20, etx[:2], erx[:1], "sqrt")
    _same(cut, ArrayResponse(base.re[:1, :2], base.im[:1, :2], base.total))
    assert not np.array_equal(_bits(base.re[0, 1]), _bits(base.re[0, 2]))


# ---- 3. against physics in float64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("amp", ["sqrt", "linear"])
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
@pytest.mark.parametrize("scene", ["random7", "obstacle"])
def test_every_plane_against_the_float64_sum_of_steered_phasors(ctx, scene, mode, role, amp):
    """sum a_k e^(-j 2 pi (r_k - e_tx[j] . u_tx - e_rx[i] . u_rx) / lambda) in float64 from the oracle's fp32 contributions, lengths
    and directions; per cell and pair the difference is within the bound that array_response_oracle.physics derives term by term."""
    etx, erx = SHAPES["3x4"]
    T, Rl, D = _joined(scene, mode, role)
    H, bound = physics(T, Rl, D, INV_20, AMPS[amp], etx, erx)
    fixed = _setup(ctx, scene)
    got = ctx.array_response(_params(mode, role), fixed, INV_20, etx, erx, amp)
    err = np.abs(got.re.astype(np.float64) + 1j * got.im.astype(np.float64) - H.reshape(got.re.shape))
    bound = bound.reshape(err.shape)
    lit = bound > 0
    print(f"{scene} {mode} {role} {amp}: max error / bound {np.max(err[lit] / bound[lit]):.3f}")
    assert lit.mean() > 1 / 3 and (err <= bound).all()
    assert (np.abs(H.imag) > 0).mean() > 1 / 3
    # the steering moves the phases: the off-origin planes are not the origin's
    assert np.abs(H[1, 1] - H[0, 0]).max() > 0.1 * np.abs(H[0, 0]).max()


# ---- 4. the candidate mask and min_order ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("role", ["rx", "tx"])
def test_matrix_honours_the_candidate_mask_and_min_order(ctx, role):
    etx, erx = SHAPES["3x4"]
    walls, fixed, X, Y = _case("random7")
    allowed = np.ones(7, np.uint8)
    allowed[[2, 5]] = 0
    ctx.set_scene(walls)
    ctx.set_candidate_mask(allowed)
    try:
        ctx.set_grid(X, Y)
        got = ctx.array_response(_params("hard", role), fixed, INV_20, etx, erx, "sqrt")
    finally:
        ctx.set_candidate_mask(None)
    everything = _oracle("random7", "hard", role, "received_power", "sqrt", "3x4")
    _same(got, _oracle("random7", "hard", role, "received_power", "sqrt", "3x4", 0, 2, (2, 5)))
    assert not np.array_equal(got.re, everything.re)
    # min_order = 1: the line of sight is left out
    got = ctx.array_response(_params("hsig", role, lo=1), fixed, INV_20, etx, erx, "linear")
    _same(got, _oracle("random7", "hsig", role, "received_power", "linear", "3x4", 1, 2))
    assert got.re.any() and not np.array_equal(got.total, _oracle("random7", "hsig", role, "received_power", "linear", "3x4").total)


# ---- 5. state and refusals -------------------------------------------------------------------------------------------------------------
def test_launch_leaves_the_other_results_alone_and_repeats_itself(ctx):
    from differt2d_amd.engine import make_params

    etx, erx = SHAPES["3x4"]
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
    fr = ctx.frequency_response(params, fixed, [INV_20, F(7.0), F(0.0)], "sqrt")
    pa = ctx.power_angle(params, fixed, "rx", 0.3, 12)
    ar = ctx.array_response(params, fixed, INV_20, etx, erx, "sqrt")
    assert np.array_equal(_bits(ctx.get_map()), _bits(before)) and before.any()  # still the previous sweep's map
    assert np.array_equal(_bits(ctx.get_profile(24)), _bits(profile)) and profile.any()
    n = len(rec["cell"])
    again = {"cell": np.empty(n, np.int32), "valid": np.empty(n, F), "length": np.empty(n, F)}
    vp = lambda a: a.ctypes.data
    assert ctx._lib.d2d_get_valid_paths(ctx._ctx, n, vp(again["cell"]), None, None, None, None, vp(again["valid"]), vp(again["length"])) == 0
    assert n > 0 and all(np.array_equal(again[f].view(np.uint32), rec[f].view(np.uint32)) for f in again)
    top2 = ctx.get_strongest_paths()
    assert all(np.array_equal(a, b, equal_nan=a.dtype == np.float32) for a, b in zip(top, top2)) and top.power.any()
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(ctx.get_coherent_field(), cf)) and cf.im.any()
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(ctx.get_frequency_response(), fr)) and fr.im.any()
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(ctx.get_power_angle(), pa)) and pa.bins.any()
    _same(ctx.array_response(params, fixed, INV_20, etx, erx, "sqrt"), ar)  # two launches give the same bits
    _same(ctx.get_array_response(), ar)
    _same(ar, _oracle("random7", "hsig", "rx", "received_power", "sqrt", "3x4"))
    assert np.array_equal(_bits(ar.total), _bits(top.total))
    # any of the three pointers may be NULL
    only_im = np.empty(ar.im.shape, F)
    assert ctx._lib.d2d_get_array_response(ctx._ctx, None, vp(only_im), None) == 0 and np.array_equal(_bits(only_im), _bits(ar.im))
    # the other sinks leave the matrix alone in their turn
    ctx.strongest_paths(params, fixed, 2)
    ctx.coherent_field(params, fixed, INV_20, "linear")
    ctx.frequency_response(params, fixed, [INV_20], "linear")
    ctx.power_angle(params, fixed, "tx", 0.0, 5)
    ctx.power_profile(params, fixed, 0.0, 3.0, 8)
    ctx.launch(fused_params, fixed)
    _same(ctx.get_array_response(), ar)
    # a smaller matrix after a larger one: the result has the new launch's planes
    few = ctx.array_response(params, fixed, INV_20, etx[:2], erx[:1], "sqrt")
    assert few.re.shape == (1, 2, *ctx.shape)
    _same(few, ArrayResponse(ar.re[:1, :2], ar.im[:1, :2], ar.total))
    # another grid size on the same context: the result goes with the grid
    X2, Y2 = unit_grid(35, 18)
    ctx.set_grid(X2, Y2)
    with pytest.raises(Exception) as e:
        ctx.get_array_response()
    assert getattr(e.value, "status", None) == -5
    q = ctx.array_response(params, fixed, INV_20, etx[:2], erx[:2], "linear")
    ctx.launch(params, fixed)
    assert q.re.shape == q.im.shape == (2, 2, 18, 35) and q.total.shape == (18, 35)
    assert np.array_equal(_bits(q.total), _bits(ctx.get_map()))
    _, T, Rl, D = directed(walls, fixed, X2, Y2, min_order=0, max_order=2, **MODES["hsig"])
    re, im, total = fold(T, Rl, D, INV_20, AMP_LINEAR, etx[:2], erx[:2])
    _same(q, ArrayResponse(re.reshape(2, 2, 18, 35), im.reshape(2, 2, 18, 35), total.reshape(18, 35)))


def _nothing_to_get(ctx):
    bufs = [np.zeros((8, 8) + tuple(ctx.shape), F), np.zeros((8, 8) + tuple(ctx.shape), F), np.zeros(ctx.shape, F)]
    rc = ctx._lib.d2d_get_array_response(ctx._ctx, *(b.ctypes.data for b in bufs))
    return rc == -5 and b"d2d_array_response_launch" in ctx._lib.d2d_last_error()


def _refused(ctx, previous, status, word, params, fixed, inv=INV_20, etx=None, erx=None, amp="sqrt"):
    """The launch is refused with ``status`` and a message that has ``word``, and the previous result is still there to get."""
    from differt2d_amd import _lib as L

    etx = SHAPES["3x4"][0] if etx is None else etx
    erx = SHAPES["3x4"][1] if erx is None else erx
    with pytest.raises(L.D2DError, match=word) as e:
        ctx.array_response(params, fixed, inv, etx, erx, amp)
    assert e.value.status == status, (e.value.status, str(e.value))
    assert isinstance(e.value, L.D2DUnsupported) == (status == -4)
    _same(ctx.get_array_response(), previous)
    return str(e.value)


def test_loud_edges(ctx):
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import make_params

    etx, erx = SHAPES["3x4"]
    walls, fixed, X, Y = _case("random7")
    ctx.set_scene(walls)
    ctx.set_reflection_coefs(None)
    ctx.set_grid(*unit_grid(19, 11))  # a grid this context has not seen: no result yet
    ctx.set_grid(X, Y)
    assert _nothing_to_get(ctx)
    with pytest.raises(L.D2DError) as e:
        ctx.get_array_response()
    assert e.value.status == -5
    kw = dict(min_order=0, max_order=2)
    ok = make_params(**kw)
    # a refusal before any launch leaves nothing to get
    with pytest.raises(L.D2DUnsupported, match="sigmoid"):
        ctx.array_response(make_params(approx=True, function="sigmoid", **kw), fixed, INV_20, etx, erx)
    assert _nothing_to_get(ctx)
    previous = ctx.array_response(ok, fixed, INV_20, etx, erx)
    assert previous.re.any() and previous.im.any()
    n0 = ctx.txg_fallbacks()
    _refused(ctx, previous, -4, "sigmoid", make_params(approx=True, function="sigmoid", **kw), fixed)
    _refused(ctx, previous, -4, "MinPath / FermatPath", make_params(solver="min", **kw), fixed)
    _refused(ctx, previous, -4, "MinPath / FermatPath", make_params(solver="fermat", **kw), fixed)
    _refused(ctx, previous, -4, "D2D_FUN_CUSTOM", make_params(fun="custom", **kw), fixed)
    _refused(ctx, previous, -4, "D2D_OUT_ADD", make_params(out_mode=L.OUT_ADD, **kw), fixed)
    _refused(ctx, previous, -4, "not culled", make_params(grid_role=L.GRID_TX, tol=0.6, **kw), fixed)
    ctx.set_option("txg_exhaustive", 1)
    try:
        _refused(ctx, previous, -4, "txg_exhaustive", make_params(grid_role=L.GRID_TX, **kw), fixed)
    finally:
        ctx.set_option("txg_exhaustive", 0)
    _refused(ctx, previous, -5, "d2d_set_reflection_coefs", make_params(fun="received_power_per_object", **kw), fixed)
    # the counts: 0 and 9 of either list
    nine = np.zeros((9, 2), F)
    none = np.zeros((0, 2), F)
    for bad in (none, nine):
        assert "d2d_array_response_launch" in _refused(ctx, previous, -1, "nt in 1 .. 8", ok, fixed, etx=bad)
        _refused(ctx, previous, -1, "nr in 1 .. 8", ok, fixed, erx=bad)
    # a non-finite element: the message ends in its index
    for value in (np.nan, np.inf, -np.inf):
        for k in range(etx.size):
            e2 = etx.copy()
            e2.reshape(-1)[k] = value
            assert _refused(ctx, previous, -1, "tx_elems", ok, fixed, etx=e2).endswith(f"at index {k // 2}")
        for k in range(erx.size):
            e2 = erx.copy()
            e2.reshape(-1)[k] = value
            assert _refused(ctx, previous, -1, "rx_elems", ok, fixed, erx=e2).endswith(f"at index {k // 2}")
    for inv in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf")):
        _refused(ctx, previous, -1, "inv_wavelength", ok, fixed, inv=inv)
    for amp in (2, -1, "power"):
        _refused(ctx, previous, -1, "amplitude", ok, fixed, amp=amp)
    # NULL lists
    fx = np.ascontiguousarray(fixed, F)
    raw = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p)(
        C.cast(ctx._lib.d2d_array_response_launch, C.c_void_p).value)
    assert raw(ctx._ctx, C.addressof(ok), fx.ctypes.data, float(INV_20), 0, 1, None, 1, erx.ctypes.data) == -1
    assert raw(ctx._ctx, C.addressof(ok), fx.ctypes.data, float(INV_20), 0, 1, etx.ctypes.data, 1, None) == -1
    _same(ctx.get_array_response(), previous)
    assert ctx.txg_fallbacks() == n0
    # ... after all of which the context still works (the library's constants are taken as well as the names), and the grid's
    # change drops the result
    a = ctx.array_response(ok, fixed, INV_20, etx, erx, L.D2D_FIELD_AMP_LINEAR)
    _same(a, ctx.array_response(ok, fixed, INV_20, etx, erx, "linear"))
    assert a.re.any() and not _nothing_to_get(ctx)
    # finite offsets are accepted whatever their size, and so is a zero inverse wavelength
    big = np.array([[np.finfo(F).max, 0.0]], F)
    z = ctx.array_response(ok, fixed, 0.0, big, big, "linear")
    assert np.array_equal(_bits(z.total), _bits(a.total))
    ctx.set_grid(*unit_grid(19, 11))
    assert _nothing_to_get(ctx)


# ---- 6. the steering header on the device ------------------------------------------------------------------------------------------------
def test_selftest_steer_equals_the_host_builds_bit_for_bit(ctx, tmp_path):
    dx, dy, f0, qt, qr, inv = steer_inputs()
    ux, uy, ok, f = ctx.selftest_steer(dx, dy, f0, qt, qr, inv)
    wx, wy, wok = unit_dir(dx, dy)
    wf = steer_phase(f0, qt, qr, inv)
    # the g++ build of the same header (tests/native/array_response_host.cpp)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = str(tmp_path / "libar_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                           os.path.join(root, "tests", "native", "array_response_host.cpp")])
    lib = C.CDLL(so)
    fp = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
    lib.ar_unit_dir.argtypes = [C.c_longlong, fp, fp, fp, fp, np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")]
    lib.ar_unit_dir.restype = None
    lib.ar_steer_phase.argtypes = [C.c_longlong, fp, fp, fp, fp, fp]
    lib.ar_steer_phase.restype = None
    hx, hy, hok, hf = np.empty_like(dx), np.empty_like(dx), np.empty(dx.size, np.uint8), np.empty_like(dx)
    lib.ar_unit_dir(dx.size, dx, dy, hx, hy, hok)
    lib.ar_steer_phase(dx.size, f0, qt, qr, inv, hf)
    assert np.array_equal(ok, wok) and np.array_equal(ok, hok.astype(bool)) and ok.sum() > 2 * 10**5 and (~ok).sum() > 300
    for name, got, want in (("ux / NumPy", ux, wx), ("uy / NumPy", uy, wy), ("ux / g++", ux, hx), ("uy / g++", uy, hy)):
        bad = _bits(got[ok]) != _bits(want[ok])  # (without a direction the quotients are not used)
        assert not bad.any(), f"{name}: {bad.sum()} of {bad.size} differ, first at ({dx[ok][bad][0]!r}, {dy[ok][bad][0]!r})"
    nan = np.isnan(wf)
    assert np.array_equal(np.isnan(f), nan) and np.array_equal(np.isnan(hf), nan) and nan.sum() > 100
    for name, want in (("NumPy", wf), ("g++", hf)):
        bad = _bits(f[~nan]) != _bits(want[~nan])
        assert not bad.any(), f"steer_phase / {name}: {bad.sum()} of {bad.size} differ"
    assert (f[~nan] >= 0).all() and (f[~nan] < 1).all()
    clamp = (f0 == 0) & (qt == F(1e-9)) & (qr == 0) & (inv == 1)
    assert clamp.any() and not _bits(f[clamp]).any()  # the clamp case: +0.0


# ---- 7. the Scene methods ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("role", ["rx", "tx"])
def test_scene_methods_mirror_the_context(ctx, role):
    from differt2d_amd import utils
    from differt2d_amd.engine import ArrayResponse as AR, make_params
    from differt2d_amd.geometry import Point
    from differt2d_amd.scene import Scene

    walls, fixed, X, Y = _case("random7")
    pts = {"a": Point(xy=fixed), "b": Point(xy=(F(1.0) - fixed).astype(F))}
    scene = Scene.from_walls_array(walls)
    scene = scene.with_transmitters(**pts) if role == "rx" else scene.with_receivers(**pts)
    method = scene.array_response_on_receivers_grid if role == "rx" else scene.array_response_on_transmitters_grid
    etx, erx = utils.ula(4, 0.025), utils.ula(3, 0.025, np.pi / 3)
    common = dict(wavelength=0.05, tx_elements=etx, rx_elements=erx, min_order=0, max_order=2, approx=True, function="hard_sigmoid",
                  filter_objects=lambda o: o is not scene.objects[3])
    got = dict(method(X, Y, utils.received_power, dict(r_coef=0.4, height=0.2), **common))
    lin = dict(method(X, Y, utils.received_power, dict(r_coef=0.4, height=0.2), amplitude="linear", **common))
    assert list(got) == list(lin) == ["a", "b"]
    allowed = np.ones(7, np.uint8)
    allowed[3] = 0
    ctx.set_scene(walls)
    ctx.set_candidate_mask(allowed)
    ctx.set_grid(X, Y)
    params = make_params(min_order=0, max_order=2, r_coef=0.4, height=0.2, grid_role=_role_id(role), **MODES["hsig"])
    for name, pt in pts.items():
        assert isinstance(got[name], AR) and got[name].re.shape == (3, 4, 13, 21)
        _same(got[name], ctx.array_response(params, pt.xy, INV_20, etx, erx, "sqrt"))
        _same(lin[name], ctx.array_response(params, pt.xy, INV_20, etx, erx, "linear"))
        assert got[name].re.any() and got[name].im.any()
    ctx.set_candidate_mask(None)
    assert not np.array_equal(got["a"].re, got["b"].re) and not np.array_equal(got["a"].re, lin["a"].re)
    # the utils on the result: H, its singular values and the capacity; no pair of unit-norm beamformers beats the largest singular
    # value, and the matched ones of a one-path cell reach nr * nt * |a|^2 = nr * nt * total up to the fp32 roundings
    a = got["a"]
    h = utils.channel_matrix(a)
    s = utils.singular_values(a)
    cap = utils.mimo_capacity(a, 1e4)
    assert h.shape == (3, 4, 13, 21) and s.shape == (3, 13, 21) and cap.shape == (13, 21)
    lit = a.total > 0
    assert lit.any() and (s[0][lit] > 0).all() and not s[:, ~lit].any() and not cap[~lit].any() and (cap[lit] > 0).all()
    wr, wt = np.ones(3) / np.sqrt(3), np.ones(4) / np.sqrt(4)
    assert (utils.beamformed_power(a, wr, wt) <= s[0] ** 2 * (1 + 1e-9) + 1e-30).all()
    assert (s[1][lit] > 1e-3 * s[0][lit]).any()  # multipath: some cells have rank above one
