"""The wideband array response (include/d2d.h: d2d_array_frequency_response_launch; power_sink_kernel, ArrayFreqSink): per cell the
nf x nr x nt channel tensor from one preparation of the culled sweep.  Held bit for bit to the oracle recipe of
``tests/array_frequency_response_oracle.py`` (a loop of the array response's recipe over the list), to ``Context.array_response`` per
wavelength, to ``Context.frequency_response`` for zero offsets, to the fused map, and to its state rules and refusals.  The wavelength
counts 1, 9, 33 and 70 cross a chunk boundary for every chunk size the kernel may be built with (8, 16, 32, 64).  The scenes and the
cached contributions are those of ``tests/test_gpu_strongest_paths.py`` and ``tests/test_gpu_power_angle.py``."""

import ctypes as C
import functools

import numpy as np
import pytest

from array_frequency_response_oracle import ArrayFrequencyResponse, array_frequency_response, fold_list, guard
from array_response_oracle import AMP_LINEAR, AMP_SQRT
from conftest import unit_grid
from test_gpu_power_angle import _directed
from test_gpu_strongest_paths import COEF7, MODES, _case, _contributions, _role_id

pytestmark = pytest.mark.gpu

F = np.float32
AMPS = {"sqrt": AMP_SQRT, "linear": AMP_LINEAR}
WL = F(0.05)
FUSED_FUNS = ["received_power", "length_squared", "length", "one", "received_power_per_object"]


def _elements(n, seed):
    """``n`` offsets of a fraction of the wavelength to two wavelengths, the first one zero, no two alike (the lists of
    tests/test_gpu_array_response.py: the same seeds)."""
    rng = np.random.default_rng(seed)
    r = rng.uniform(0.1, 2.0, n) * float(WL)
    th = rng.uniform(0, 2 * np.pi, n)
    e = np.stack([r * np.cos(th), r * np.sin(th)], axis=1).astype(F)
    e[0] = 0
    return e


# nr x nt: 1 x 1 (the zero pair alone), 3 x 4 and 8 x 8 (both limits)
SHAPES = {"1x1": (_elements(1, 1), _elements(1, 2)), "3x4": (_elements(4, 3), _elements(3, 4)), "8x8": (_elements(8, 5), _elements(8, 6))}


def _inv_list(nf):
    """``nf`` inverse wavelengths, ``float32(1) / float32(w)`` with ``w`` drawn from 0.03 .. 0.2 (seeded; every list is a prefix of the
    longest) and entry 0 equal to 0.05."""
    w = np.random.default_rng(20261019).uniform(0.03, 0.2, 70).astype(F)
    w[0] = WL
    inv = (F(1) / w)[:nf]
    assert inv.dtype == F and np.unique(inv).size == nf
    return inv


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
def _oracle(scene, mode, role, fun, amp, shape, nf, lo=0, hi=2):
    T, Rl, D = _joined(scene, mode, role, fun, lo, hi)
    etx, erx = SHAPES[shape]
    grid = _case(scene)[2].shape
    re, im, total = fold_list(T, Rl, D, _inv_list(nf), AMPS[amp], etx, erx)
    out = ArrayFrequencyResponse(re.reshape(re.shape[:3] + grid), im.reshape(im.shape[:3] + grid), total.reshape(grid))
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


# ---- 1. the oracle alone: the comparisons below do not pass on empty ground -------------------------------------------------------------
@pytest.mark.parametrize("scene,shape,nf", [("random7", "3x4", 9), ("obstacle", "3x4", 33)])
def test_oracle_blocks_differ_pairwise_and_carry_phase(scene, shape, nf):
    want = _oracle(scene, "hard", "rx", "received_power", "sqrt", shape, nf)
    guard(want.re, want.im)


# ---- 2. bit for bit against the oracle recipe -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("amp", ["sqrt", "linear"])
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
@pytest.mark.parametrize("scene,shape,nf", [("random7", "1x1", 1), ("random7", "3x4", 9), ("obstacle", "3x4", 33), ("random7", "8x8", 9),
                                            ("square_centre", "3x4", 9)])
def test_tensor_equals_the_oracle_recipe(ctx, scene, shape, nf, mode, role, amp):
    want = _oracle(scene, mode, role, "received_power", amp, shape, nf)
    etx, erx = SHAPES[shape]
    assert np.count_nonzero(want.im) > want.im.size // 3 and np.count_nonzero(want.re) > want.re.size // 3
    fixed = _setup(ctx, scene)
    got = ctx.array_frequency_response(_params(mode, role), fixed, _inv_list(nf), etx, erx, amp)
    assert got.re.shape == (nf, erx.shape[0], etx.shape[0]) + _case(scene)[2].shape
    _same(got, want)


def test_seventy_wavelengths_equal_the_oracle_recipe(ctx):
    """More than one pass for every chunk size up to 64, the last pass a partial one."""
    want = _oracle("random7", "hard", "rx", "received_power", "sqrt", "3x4", 70)
    guard(want.re[::7], want.im[::7])
    etx, erx = SHAPES["3x4"]
    fixed = _setup(ctx, "random7")
    _same(ctx.array_frequency_response(_params("hard", "rx"), fixed, _inv_list(70), etx, erx, "sqrt"), want)


# ---- 3. every block is the array response at its wavelength ----------------------------------------------------------------------------
def _slice_list():
    """Nine entries in descending order with a duplicate and an entry 0."""
    v = np.sort(_inv_list(7))[::-1]
    inv = np.concatenate([v[:3], v[2:3], v[3:], [F(0)]]).astype(F)
    assert inv.size == 9 and (np.diff(inv) <= 0).all() and inv[2] == inv[3] and inv[8] == 0
    return inv


@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
def test_every_block_is_the_array_response_at_its_wavelength(ctx, mode, role):
    etx, erx = SHAPES["3x4"]
    inv = _slice_list()
    fixed = _setup(ctx, "random7")
    params = _params(mode, role)
    base = ctx.array_frequency_response(params, fixed, inv, etx, erx, "sqrt")
    for f in range(inv.size):
        ar = ctx.array_response(params, fixed, inv[f], etx, erx, "sqrt")
        _same(ArrayFrequencyResponse(base.re[f], base.im[f], base.total), ArrayFrequencyResponse(*ar))
    assert base.im[0].any() and np.array_equal(_bits(base.re[2]), _bits(base.re[3])) and not np.array_equal(_bits(base.re[0]), _bits(base.re[1]))
    # permuted and truncated lists give permuted and leading blocks
    pf = [4, 8, 0, 3, 7, 1, 6, 2, 5]
    _same(ctx.array_frequency_response(params, fixed, inv[pf], etx, erx, "sqrt"), ArrayFrequencyResponse(base.re[pf], base.im[pf], base.total))
    _same(ctx.array_frequency_response(params, fixed, inv[:4], etx, erx, "sqrt"), ArrayFrequencyResponse(base.re[:4], base.im[:4], base.total))
    # permuted element lists give permuted planes
    pt, pr = [2, 0, 3, 1], [1, 2, 0]
    perm = ctx.array_frequency_response(params, fixed, inv, etx[pt], erx[pr], "sqrt")
    _same(perm, ArrayFrequencyResponse(base.re[:, pr][:, :, pt], base.im[:, pr][:, :, pt], base.total))
    assert not np.array_equal(_bits(base.re[0, 0, 1]), _bits(base.re[0, 0, 2]))
    # total is the fused map
    ctx.launch(params, fixed)
    fused = ctx.get_map()
    assert np.array_equal(_bits(base.total), _bits(fused)) and np.count_nonzero(fused) > fused.size // 3


# ---- 4. zero offsets: the frequency response ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("amp", ["sqrt", "linear"])
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
@pytest.mark.parametrize("scene", ["random7", "obstacle", "square_centre"])
def test_zero_offset_pair_is_the_frequency_response(ctx, scene, mode, role, amp):
    """Offsets of (+-0, +-0) at both ends: Context.frequency_response bit for bit wherever no contribution lacks a direction --
    everywhere in random7 and obstacle; in square_centre the cell that IS the fixed end point, [4, 4], has a line of sight without one,
    and exactly that cell differs."""
    fixed = _setup(ctx, scene)
    params = _params(mode, role)
    inv = _inv_list(9)
    etx = np.array([[0.03, 0.01], [-0.0, 0.0]], F)
    erx = np.array([[0.0, -0.0], [0.02, -0.07], [-0.0, -0.0]], F)
    got = ctx.array_frequency_response(params, fixed, inv, etx, erx, amp)
    fr = ctx.frequency_response(params, fixed, inv, amp)
    assert np.array_equal(_bits(got.total), _bits(fr.total)) and np.count_nonzero(fr.im) > fr.im.size // 3
    for i in (0, 2):
        for f in range(inv.size):
            dre, dim = _bits(got.re[f, i, 1]) != _bits(fr.re[f]), _bits(got.im[f, i, 1]) != _bits(fr.im[f])
            if scene == "square_centre":
                assert np.argwhere(dre | dim).tolist() == [[4, 4]], (i, f)
            else:
                assert not dre.any() and not dim.any(), (i, f)
    assert not np.array_equal(_bits(got.im[:, 1, 1]), _bits(fr.im)) and not np.array_equal(_bits(got.im[:, 0, 0]), _bits(fr.im))


# ---- 5. an entry 0 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
def test_zero_entry_linear_zero_offsets_is_the_fused_map(ctx, mode, role):
    fixed = _setup(ctx, "random7")
    params = _params(mode, role)
    inv = _inv_list(9).copy()
    inv[5] = 0
    z = np.zeros((1, 2), F)
    got = ctx.array_frequency_response(params, fixed, inv, z, np.array([[-0.0, 0.0]], F), "linear")
    ctx.launch(params, fixed)
    fused = ctx.get_map()
    assert np.count_nonzero(fused) > fused.size // 3
    assert np.array_equal(_bits(got.re[5, 0, 0]), _bits(fused)) and np.array_equal(_bits(got.total), _bits(fused))
    assert not _bits(got.im[5]).any()  # +0.0 by bits
    assert got.im[4].any() and got.im[6].any() and not np.array_equal(_bits(got.re[4, 0, 0]), _bits(fused))


# ---- 6. every fused function ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fun", FUSED_FUNS)
def test_every_fused_function(ctx, fun):
    etx, erx = SHAPES["3x4"]
    try:
        fixed = _setup(ctx, "random7", fun)
        params = _params("hsig", "rx", fun)
        got = ctx.array_frequency_response(params, fixed, _inv_list(9), etx, erx, "sqrt")
        ctx.launch(params, fixed)
        fused = ctx.get_map()
    finally:
        ctx.set_reflection_coefs(None)
    assert np.isfinite(fused).all() and np.count_nonzero(fused) > fused.size // 3
    assert np.array_equal(_bits(got.total), _bits(fused)) and np.count_nonzero(got.im) > 0
    _same(got, _oracle("random7", "hsig", "rx", fun, "sqrt", "3x4", 9))  # (the signed and the zero coefficient included)


# ---- 7. min_order, 8. max_order = 3 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("role", ["rx", "tx"])
def test_min_order_one_leaves_the_line_of_sight_out(ctx, role):
    etx, erx = SHAPES["3x4"]
    fixed = _setup(ctx, "random7")
    got = ctx.array_frequency_response(_params("hsig", role, lo=1), fixed, _inv_list(9), etx, erx, "linear")
    _same(got, _oracle("random7", "hsig", role, "received_power", "linear", "3x4", 9, 1, 2))
    everything = _oracle("random7", "hsig", role, "received_power", "linear", "3x4", 9)
    assert got.re.any() and not np.array_equal(got.total, everything.total) and not np.array_equal(got.re, everything.re)


@pytest.mark.parametrize("shape", ["1x1", "3x4"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
def test_max_order_three(ctx, mode, shape):
    """The MAXK = 3 instance of the kernel."""
    etx, erx = SHAPES[shape]
    fixed = _setup(ctx, "random7")
    got = ctx.array_frequency_response(_params(mode, "rx", hi=3), fixed, _inv_list(9), etx, erx, "sqrt")
    _same(got, _oracle("random7", mode, "rx", "received_power", "sqrt", shape, 9, 0, 3))
    assert not np.array_equal(got.total, _oracle("random7", mode, "rx", "received_power", "sqrt", shape, 9).total)


# ---- 9. a grid of its own -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("role", ["rx", "tx"])
def test_a_grid_of_its_own_from_the_walls(ctx, role):
    """19 x 11: 3 x 2 patches, the last column and row of patches with clamped lanes."""
    etx, erx = SHAPES["3x4"]
    walls, fixed, _, _ = _case("random7")
    X, Y = unit_grid(19, 11)
    inv = _inv_list(9)
    ctx.set_scene(walls)
    ctx.set_grid(X, Y)
    got = ctx.array_frequency_response(_params("hsig", role), fixed, inv, etx, erx, "sqrt")
    want = array_frequency_response(walls, fixed, X, Y, inv, AMP_SQRT, etx, erx, min_order=0, max_order=2, grid_role=role, **MODES["hsig"])
    assert got.re.shape == (9, 3, 4, 11, 19) and np.count_nonzero(want.im) > want.im.size // 3
    _same(got, want)


# ---- 10. the get ---------------------------------------------------------------------------------------------------------------------------------
def test_get_reads_ranges_of_wavelengths(ctx):
    from differt2d_amd import _lib as L

    etx, erx = SHAPES["3x4"]
    nf = 9
    walls, fixed, X, Y = _case("random7")
    ctx.set_scene(walls)
    ctx.set_grid(*unit_grid(19, 11))  # a grid this context has not a result of
    ctx.set_grid(X, Y)
    for args in ((), (0, 1)):
        with pytest.raises(L.D2DError, match="d2d_array_frequency_response_launch") as e:
            ctx.get_array_frequency_response(*args)
        assert e.value.status == -5
    assert ctx._lib.d2d_get_array_frequency_response(ctx._ctx, 0, 1, None, None, None) == -5
    whole = ctx.array_frequency_response(_params("hsig", "rx"), fixed, _inv_list(nf), etx, erx, "sqrt")
    _same(whole, _oracle("random7", "hsig", "rx", "received_power", "sqrt", "3x4", nf))
    for first, count in ((0, nf), (3, 1), (nf - 1, 1), (2, 5)):
        part = ctx.get_array_frequency_response(first, count)
        assert part.re.shape == (count, 3, 4) + tuple(ctx.shape)
        _same(part, ArrayFrequencyResponse(whole.re[first:first + count], whole.im[first:first + count], whole.total))
    _same(ctx.get_array_frequency_response(4), ArrayFrequencyResponse(whole.re[4:], whole.im[4:], whole.total))  # count=None: to the end
    # total=None is accepted, and so is any other pointer
    part = ctx.get_array_frequency_response(3, 2, with_total=False)
    assert part.total is None and np.array_equal(_bits(part.re), _bits(whole.re[3:5])) and np.array_equal(_bits(part.im), _bits(whole.im[3:5]))
    only_im = np.full(whole.im[6:7].shape, np.nan, F)
    assert ctx._lib.d2d_get_array_frequency_response(ctx._ctx, 6, 1, None, only_im.ctypes.data, None) == 0
    assert np.array_equal(_bits(only_im), _bits(whole.im[6:7]))
    # ranges outside the result
    for first, count in ((-1, 1), (0, 0), (nf - 1, 2), (nf, 1), (0, nf + 1), (0, -1), (2**31 - 1, 2**31 - 1)):
        with pytest.raises(L.D2DError, match="d2d_get_array_frequency_response") as e:
            ctx.get_array_frequency_response(first, count)
        assert e.value.status == -1, (first, count)
    _same(ctx.get_array_frequency_response(), whole)
    # the result goes with the grid
    ctx.set_grid(*unit_grid(19, 11))
    with pytest.raises(L.D2DError) as e:
        ctx.get_array_frequency_response()
    assert e.value.status == -5


# ---- 11. state ---------------------------------------------------------------------------------------------------------------------------------
def test_launch_leaves_the_other_results_alone_and_repeats_itself(ctx):
    from differt2d_amd.engine import make_params

    etx, erx = SHAPES["3x4"]
    inv = _inv_list(9)
    walls, fixed, X, Y = _case("random7")
    ctx.set_scene(walls)
    ctx.set_grid(X, Y)
    fused_params = make_params(min_order=0, max_order=2, fun="length")
    ctx.launch(fused_params, fixed)
    before = ctx.get_map()
    params = make_params(min_order=0, max_order=2, **MODES["hsig"])
    cf = ctx.coherent_field(params, fixed, inv[0], "sqrt")
    fr = ctx.frequency_response(params, fixed, inv[:3], "sqrt")
    ar = ctx.array_response(params, fixed, inv[1], etx, erx, "sqrt")
    afr = ctx.array_frequency_response(params, fixed, inv, etx, erx, "sqrt")
    _same(afr, _oracle("random7", "hsig", "rx", "received_power", "sqrt", "3x4", 9))
    # the results taken before the launch are still there, bit for bit
    assert np.array_equal(_bits(ctx.get_map()), _bits(before)) and before.any()
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(ctx.get_coherent_field(), cf)) and cf.im.any()
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(ctx.get_frequency_response(), fr)) and fr.im.any()
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(ctx.get_array_response(), ar)) and ar.im.any()
    # the same call twice gives the same bits, also with other launches in between
    _same(ctx.array_frequency_response(params, fixed, inv, etx, erx, "sqrt"), afr)
    ctx.coherent_field(params, fixed, inv[2], "linear")
    ctx.array_response(params, fixed, inv[3], etx[:2], erx, "linear")
    ctx.frequency_response(params, fixed, inv[4:6], "linear")
    ctx.launch_vg(params, fixed)
    ctx.get_grad_rx()
    _same(ctx.get_array_frequency_response(), afr)  # they leave the tensor alone in their turn
    _same(ctx.array_frequency_response(params, fixed, inv, etx, erx, "sqrt"), afr)
    # a smaller tensor after a larger one: the result has the new launch's planes
    few = ctx.array_frequency_response(params, fixed, inv[:2], etx[:2], erx[:1], "sqrt")
    assert few.re.shape == (2, 1, 2, *ctx.shape)
    _same(few, ArrayFrequencyResponse(afr.re[:2, :1, :2], afr.im[:2, :1, :2], afr.total))


# ---- 12. refusals ------------------------------------------------------------------------------------------------------------------------------
def _refused(ctx, previous, status, word, params, fixed, inv=None, etx=None, erx=None, amp="sqrt"):
    """The launch is refused with ``status`` and a message that has ``word``, and the previous result is still there to get."""
    from differt2d_amd import _lib as L

    inv = _inv_list(9) if inv is None else inv
    etx = SHAPES["3x4"][0] if etx is None else etx
    erx = SHAPES["3x4"][1] if erx is None else erx
    with pytest.raises(L.D2DError, match=word) as e:
        ctx.array_frequency_response(params, fixed, inv, etx, erx, amp)
    assert e.value.status == status, (e.value.status, str(e.value))
    assert isinstance(e.value, L.D2DUnsupported) == (status == -4)
    _same(ctx.get_array_frequency_response(), previous)
    return str(e.value)


def test_loud_edges(ctx):
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import make_params

    etx, erx = SHAPES["3x4"]
    inv = _inv_list(9)
    walls, fixed, X, Y = _case("random7")
    ctx.set_scene(walls)
    ctx.set_reflection_coefs(None)
    ctx.set_grid(*unit_grid(19, 11))
    ctx.set_grid(X, Y)
    kw = dict(min_order=0, max_order=2)
    ok = make_params(**kw)
    # a refusal before any launch leaves nothing to get
    with pytest.raises(L.D2DUnsupported, match="sigmoid"):
        ctx.array_frequency_response(make_params(approx=True, function="sigmoid", **kw), fixed, inv, etx, erx)
    assert ctx._lib.d2d_get_array_frequency_response(ctx._ctx, 0, 1, None, None, None) == -5
    previous = ctx.array_frequency_response(ok, fixed, inv, etx, erx)
    assert previous.re.any() and previous.im.any()
    n0 = ctx.txg_fallbacks()
    _refused(ctx, previous, -4, "sigmoid", make_params(approx=True, function="sigmoid", **kw), fixed)
    _refused(ctx, previous, -4, "MinPath / FermatPath", make_params(solver="min", **kw), fixed)
    _refused(ctx, previous, -4, "MinPath / FermatPath", make_params(solver="fermat", **kw), fixed)
    msg = _refused(ctx, previous, -4, "D2D_FUN_CUSTOM", make_params(fun="custom", **kw), fixed)
    assert "d2d_valid_paths" in msg and "d2d_trace_paths" in msg
    _refused(ctx, previous, -4, "D2D_OUT_ADD", make_params(out_mode=L.OUT_ADD, **kw), fixed)
    _refused(ctx, previous, -4, "not culled", make_params(grid_role=L.GRID_TX, tol=0.6, **kw), fixed)
    # nf 0 and 1025
    for bad in (np.zeros(0, F), np.full(1025, 3.0, F)):
        assert "d2d_array_frequency_response_launch" in _refused(ctx, previous, -1, "nf in 1 .. 1024", ok, fixed, inv=bad)
    # an entry that is negative, NaN or infinite: the index named
    for value in (-1.0, -1e-30, np.nan, np.inf, -np.inf):
        for k in (0, 4, 8):
            v = inv.copy()
            v[k] = value
            assert _refused(ctx, previous, -1, "inv_wavelength", ok, fixed, inv=v).endswith(f"at index {k}")
    # the counts: 0 and 9 of either list
    for bad in (np.zeros((0, 2), F), np.zeros((9, 2), F)):
        _refused(ctx, previous, -1, "nt in 1 .. 8", ok, fixed, etx=bad)
        _refused(ctx, previous, -1, "nr in 1 .. 8", ok, fixed, erx=bad)
    # a non-finite element: the message ends in its index
    for value in (np.nan, np.inf, -np.inf):
        for k in (0, 3, etx.size - 1):
            e2 = etx.copy()
            e2.reshape(-1)[k] = value
            assert _refused(ctx, previous, -1, "tx_elems", ok, fixed, etx=e2).endswith(f"at index {k // 2}")
        for k in (1, erx.size - 2):
            e2 = erx.copy()
            e2.reshape(-1)[k] = value
            assert _refused(ctx, previous, -1, "rx_elems", ok, fixed, erx=e2).endswith(f"at index {k // 2}")
    for amp in (2, -1, "power"):
        _refused(ctx, previous, -1, "amplitude", ok, fixed, amp=amp)
    # NULL lists
    fx = np.ascontiguousarray(fixed, F)
    raw = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p)(
        C.cast(ctx._lib.d2d_array_frequency_response_launch, C.c_void_p).value)
    assert raw(ctx._ctx, C.addressof(ok), fx.ctypes.data, None, 1, 0, 1, etx.ctypes.data, 1, erx.ctypes.data) == -1
    assert raw(ctx._ctx, C.addressof(ok), fx.ctypes.data, inv.ctypes.data, 1, 0, 1, None, 1, erx.ctypes.data) == -1
    assert raw(ctx._ctx, C.addressof(ok), fx.ctypes.data, inv.ctypes.data, 1, 0, 1, etx.ctypes.data, 1, None) == -1
    _same(ctx.get_array_frequency_response(), previous)
    assert ctx.txg_fallbacks() == n0
    # ... after all of which the context still works (the library's constants are taken as well as the names)
    a = ctx.array_frequency_response(ok, fixed, inv, etx, erx, L.D2D_FIELD_AMP_LINEAR)
    _same(a, ctx.array_frequency_response(ok, fixed, inv, etx, erx, "linear"))
    assert a.re.any() and not np.array_equal(_bits(a.re), _bits(previous.re))


# ---- 13. the Scene methods and the utils --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("role", ["rx", "tx"])
def test_scene_methods_mirror_the_context(ctx, role):
    from differt2d_amd import utils
    from differt2d_amd.engine import ArrayFrequencyResponse as AFR, make_params
    from differt2d_amd.geometry import Point
    from differt2d_amd.scene import Scene

    walls, fixed, X, Y = _case("random7")
    pts = {"a": Point(xy=fixed), "b": Point(xy=(F(1.0) - fixed).astype(F))}
    scene = Scene.from_walls_array(walls)
    scene = scene.with_transmitters(**pts) if role == "rx" else scene.with_receivers(**pts)
    method = scene.array_frequency_response_on_receivers_grid if role == "rx" else scene.array_frequency_response_on_transmitters_grid
    etx, erx = utils.ula(4, 0.025), utils.ula(3, 0.025, np.pi / 3)
    wl = np.array([0.05, 0.0625, 0.11], F)
    common = dict(tx_elements=etx, rx_elements=erx, min_order=0, max_order=2, approx=True, function="hard_sigmoid")
    got = dict(method(X, Y, utils.received_power, dict(r_coef=0.4, height=0.2), wavelengths=wl, **common))
    inv = dict(method(X, Y, utils.received_power, dict(r_coef=0.4, height=0.2), inv_wavelengths=F(1) / wl, amplitude="linear", **common))
    assert list(got) == list(inv) == ["a", "b"]
    ctx.set_scene(walls)
    ctx.set_grid(X, Y)
    params = make_params(min_order=0, max_order=2, r_coef=0.4, height=0.2, grid_role=_role_id(role), **MODES["hsig"])
    for name, pt in pts.items():
        assert isinstance(got[name], AFR) and got[name].re.shape == (3, 3, 4, 13, 21)
        _same(got[name], ctx.array_frequency_response(params, pt.xy, F(1) / wl, etx, erx, "sqrt"))
        _same(inv[name], ctx.array_frequency_response(params, pt.xy, F(1) / wl, etx, erx, "linear"))
        assert got[name].re.any() and got[name].im.any()
    a = got["a"]
    assert utils.channel_tensor(a).shape == (3, 3, 4, 13, 21)
    ar = utils.array_response_at(a, 1)
    _same(ArrayFrequencyResponse(*ar), ArrayFrequencyResponse(*ctx.array_response(params, pts["a"].xy, F(1) / wl[1], etx, erx, "sqrt")))
    cap = utils.wideband_capacity(a, 1e4)
    lit = a.total > 0
    assert cap.shape == (13, 21) and lit.any() and (cap[lit] > 0).all() and not cap[~lit].any()
    assert np.allclose(cap, np.mean([utils.mimo_capacity(utils.array_response_at(a, f), 1e4) for f in range(3)], axis=0))
