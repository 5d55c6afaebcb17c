"""The beam-space response (include/d2d.h: d2d_beam_response_launch; power_sink_kernel, BeamSink): per cell, wavelength and beam pair
``y = w_rx^H H w_tx`` from one preparation of the culled sweep, without the channel matrix.  Held bit for bit to the oracle recipe
of ``tests/beam_response_oracle.py`` (a NumPy restatement of ``d2d_beam.hpp``), to ``Context.frequency_response`` for one antenna, to
the fused map, within the derived element-space bound to the float64 contraction of ``Context.array_frequency_response``, and to its
independence properties, state rules and refusals.  The wavelength counts 1, 9, 33 and 70 cross a chunk boundary for every chunk size
the kernel may be built with (8, 16, 32, 64).  The scenes and the cached contributions are those of
``tests/test_gpu_strongest_paths.py`` and ``tests/test_gpu_power_angle.py``."""

import ctypes as C
import functools

import numpy as np
import pytest

import beam_response_oracle as BO
from array_response_oracle import AMP_LINEAR, AMP_SQRT
from beam_response_oracle import BeamResponse
from conftest import unit_grid
from test_gpu_power_angle import _directed
from test_gpu_strongest_paths import COEF7, MODES, _case, _contributions, _role_id

pytestmark = pytest.mark.gpu

F = np.float32
AMPS = {"sqrt": AMP_SQRT, "linear": AMP_LINEAR}
WL = F(0.05)
FUSED_FUNS = ["received_power", "length_squared", "length", "one", "received_power_per_object"]


def _elements(n, seed):
    """The element lists of tests/test_gpu_array_frequency_response.py (the same seeds)."""
    rng = np.random.default_rng(seed)
    r = rng.uniform(0.1, 2.0, n) * float(WL)
    th = rng.uniform(0, 2 * np.pi, n)
    e = np.stack([r * np.cos(th), r * np.sin(th)], axis=1).astype(F)
    e[0] = 0
    return e


def _codebook(nb, n, seed, zero=None, one_hot=None):
    """``nb`` beams of seeded complex weights over ``n`` elements; beam ``zero`` all zero, beam ``one_hot`` 1 at one element."""
    rng = np.random.default_rng(seed)
    w = (rng.normal(size=(nb, n)) + 1j * rng.normal(size=(nb, n))).astype(np.complex64)
    if zero is not None:
        w[zero] = 0
    if one_hot is not None:
        w[one_hot] = 0
        w[one_hot, n // 2] = 1
    return w


# nr x nt: 1 x 1 (the zero pair alone), 3 x 4 and 8 x 8 (both limits)
SHAPES = {"1x1": (_elements(1, 1), _elements(1, 2)), "3x4": (_elements(4, 3), _elements(3, 4)), "8x8": (_elements(8, 5), _elements(8, 6))}
# nbr x nbt: 1 x 1, 2 x 3 and 8 x 8; from two beams on, one transmit beam is all zero and one receive beam one-hot
BOOK_SIZES = {"1x1": (1, 1), "2x3": (2, 3), "8x8": (8, 8)}


def _book(book, shape):
    """``(tx_weights [nbt, nt], rx_weights [nbr, nr])`` of codebook ``book`` over the elements of ``shape``."""
    nbr, nbt = BOOK_SIZES[book]
    nt, nr = SHAPES[shape][0].shape[0], SHAPES[shape][1].shape[0]
    return (_codebook(nbt, nt, 100 + 8 * nbt + nt, zero=None if nbt == 1 else nbt - 2),
            _codebook(nbr, nr, 200 + 8 * nbr + nr, one_hot=None if nbr == 1 else nbr - 1))


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


def _joined(scene, mode, role, fun="received_power", lo=0, hi=2):
    _, T, Rl, _ = _contributions(scene, mode, role, fun, lo, hi)
    _, T2, D = _directed(scene, mode, role, fun, lo, hi)
    assert np.array_equal(T.view(np.uint32), T2.view(np.uint32))
    return T, Rl, D


@functools.lru_cache(maxsize=None)
def _oracle(scene, mode, role, fun, amp, shape, book, nf, lo=0, hi=2):
    T, Rl, D = _joined(scene, mode, role, fun, lo, hi)
    etx, erx = SHAPES[shape]
    wtx, wrx = _book(book, shape)
    grid = _case(scene)[2].shape
    re, im, total = BO.fold_list(T, Rl, D, _inv_list(nf), AMPS[amp], etx, erx, wtx, wrx)
    out = BeamResponse(re.reshape(re.shape[:3] + grid), im.reshape(im.shape[:3] + grid), total.reshape(grid))
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


def _launch(ctx, params, fixed, nf, shape, book, amp="sqrt"):
    etx, erx = SHAPES[shape]
    wtx, wrx = _book(book, shape)
    return ctx.beam_response(params, fixed, _inv_list(nf), etx, erx, wtx, wrx, amp)


# ---- 1. the oracle alone: the comparisons below do not pass on empty ground -------------------------------------------------------------
@pytest.mark.parametrize("scene,nf", [("random7", 9), ("obstacle", 33)])
def test_oracle_planes_differ_pairwise_and_carry_phase(scene, nf):
    want = _oracle(scene, "hard", "rx", "received_power", "sqrt", "3x4", "2x3", nf)
    keep = [0, 2]  # (transmit beam 1 is the all-zero one: +0.0 by bits in every plane)
    assert not _bits(want.re[:, :, 1]).any() and not _bits(want.im[:, :, 1]).any()
    BO.guard(want.re[:, :, keep], want.im[:, :, keep])


# ---- 2. bit for bit against the oracle recipe -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("amp", ["sqrt", "linear"])
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
@pytest.mark.parametrize("scene,shape,book,nf", [("random7", "1x1", "1x1", 1), ("random7", "3x4", "2x3", 9), ("obstacle", "3x4", "2x3", 33),
                                                 ("random7", "8x8", "8x8", 9), ("random7", "3x4", "8x8", 1), ("square_centre", "8x8", "2x3", 9)])
def test_planes_equal_the_oracle_recipe(ctx, scene, shape, book, nf, mode, role, amp):
    want = _oracle(scene, mode, role, "received_power", amp, shape, book, nf)
    assert np.count_nonzero(want.im) > want.im.size // 3 or nf == 1
    fixed = _setup(ctx, scene)
    got = _launch(ctx, _params(mode, role), fixed, nf, shape, book, amp)
    assert got.re.shape == (nf,) + BOOK_SIZES[book] + _case(scene)[2].shape
    _same(got, want)


def test_seventy_wavelengths_equal_the_oracle_recipe(ctx):
    """More than one pass for every chunk size up to 64, the last pass a partial one."""
    want = _oracle("random7", "hard", "rx", "received_power", "sqrt", "3x4", "2x3", 70)
    BO.guard(want.re[::7, :, [0, 2]], want.im[::7, :, [0, 2]])
    fixed = _setup(ctx, "random7")
    _same(_launch(ctx, _params("hard", "rx"), fixed, 70, "3x4", "2x3"), want)


# ---- 3. total, one antenna ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("amp", ["sqrt", "linear"])
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
@pytest.mark.parametrize("scene", ["random7", "obstacle", "square_centre"])
def test_one_antenna_is_the_frequency_response_and_total_the_fused_map(ctx, scene, mode, role, amp):
    """nt = nr = nbt = nbr = 1, offsets (+-0, +-0), weights (1, 0): Context.frequency_response bit for bit wherever no contribution lacks
    a direction -- everywhere in random7 and obstacle; in square_centre the cell that IS the fixed end point, [4, 4], has a line of
    sight without one, and exactly that cell differs."""
    fixed = _setup(ctx, scene)
    params = _params(mode, role)
    inv = _inv_list(9)
    got = ctx.beam_response(params, fixed, inv, np.array([[-0.0, 0.0]], F), np.array([[0.0, -0.0]], F), [1 + 0j], [[1 + 0j]], amp)
    fr = ctx.frequency_response(params, fixed, inv, amp)
    ctx.launch(params, fixed)
    fused = ctx.get_map()
    assert np.array_equal(_bits(got.total), _bits(fused)) and np.array_equal(_bits(got.total), _bits(fr.total))
    assert np.count_nonzero(fr.im) > fr.im.size // 3 and np.count_nonzero(fused) > fused.size // 3
    assert got.re.shape == (9, 1, 1) + fused.shape
    for f in range(inv.size):
        diff = (_bits(got.re[f, 0, 0]) != _bits(fr.re[f])) | (_bits(got.im[f, 0, 0]) != _bits(fr.im[f]))
        assert np.argwhere(diff).tolist() == ([[4, 4]] if scene == "square_centre" else []), f


# ---- 4. element space ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
@pytest.mark.parametrize("shape,book", [("3x4", "2x3"), ("8x8", "8x8")])
def test_element_space_within_the_derived_bound(ctx, shape, book, mode, role):
    """A general codebook with a one-hot receive beam against the float64 contraction of Context.array_frequency_response, and
    utils.beam_power against utils.beamformed_power, within the bound of tests/beam_response_oracle.py."""
    from differt2d_amd import utils

    etx, erx = SHAPES[shape]
    wtx, wrx = _book(book, shape)
    inv = _inv_list(4)
    fixed = _setup(ctx, "random7")
    params = _params(mode, role)
    got = ctx.beam_response(params, fixed, inv, etx, erx, wtx, wrx, "sqrt")
    afr = ctx.array_frequency_response(params, fixed, inv, etx, erx, "sqrt")
    T, Rl, D = _joined("random7", mode, role)
    bnd = BO.bound(T, Rl, D, inv, AMP_SQRT, etx, erx, wtx, wrx).reshape(got.re.shape)
    y = BO.contract(afr.re, afr.im, wtx, wrx)
    err = np.abs(utils.beam_response(got).astype(np.complex128) - y)
    lit = bnd > 0
    print(f"{shape} {book} {mode} {role}: max error / bound = {(err[lit] / bnd[lit]).max():.4f}")
    assert (err <= bnd).all() and lit.sum() > lit.size // 3 and np.abs(y).max() > 0.1
    # the one-hot receive beam: w_rx^H H is row n // 2 of H, and with it y = H[i] . w_tx
    hot, i = wrx.shape[0] - 1, erx.shape[0] // 2
    row = np.einsum("fj...,tj->ft...", afr.re[:, i].astype(np.float64) + 1j * afr.im[:, i], wtx.astype(np.complex128))
    assert (np.abs(utils.beam_response(got)[:, hot] - row) <= bnd[:, hot]).all()
    # powers: |y|^2 against beamformed_power per wavelength and pair, d|y|^2 <= (2 |y| + bound) * bound
    power = utils.beam_power(got)
    for f in (0, 3):
        for br, bt in ((0, 0), (wrx.shape[0] - 1, wtx.shape[0] - 1)):
            ref = utils.beamformed_power(utils.array_response_at(afr, f), wrx[br], wtx[bt])
            slack = (2 * np.abs(y[f, br, bt]) + bnd[f, br, bt]) * bnd[f, br, bt]
            assert (np.abs(power[f, br, bt] - ref) <= slack + 1e-12 * ref).all()


# ---- 5. independence -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
def test_independence_under_permuted_duplicated_and_truncated_lists(ctx, mode, role):
    etx, erx = SHAPES["3x4"]
    wtx, wrx = _codebook(3, 4, 21), _codebook(2, 3, 22)
    inv = _inv_list(9)
    fixed = _setup(ctx, "random7")
    params = _params(mode, role)
    base = ctx.beam_response(params, fixed, inv, etx, erx, wtx, wrx)
    BO.guard(base.re, base.im)
    pf, pt, pr = [4, 8, 0, 3, 7, 1, 6, 2, 5], [2, 0, 1], [1, 0]
    _same(ctx.beam_response(params, fixed, inv[pf], etx, erx, wtx[pt], wrx[pr]),
          BeamResponse(base.re[pf][:, pr][:, :, pt], base.im[pf][:, pr][:, :, pt], base.total))
    dup = ctx.beam_response(params, fixed, inv[[1, 1, 5]], etx, erx, wtx[[0, 2, 0, 0, 1, 2, 2, 1]], wrx[[1, 1, 0]])
    _same(dup, BeamResponse(base.re[[1, 1, 5]][:, [1, 1, 0]][:, :, [0, 2, 0, 0, 1, 2, 2, 1]], base.im[[1, 1, 5]][:, [1, 1, 0]][:, :, [0, 2, 0, 0, 1, 2, 2, 1]],
                            base.total))
    _same(ctx.beam_response(params, fixed, inv[:4], etx, erx, wtx[:1], wrx[0]), BeamResponse(base.re[:4, :1, :1], base.im[:4, :1, :1], base.total))
    # a codebook of 16 transmit beams is two calls
    many = _codebook(16, 4, 23)
    whole = [ctx.beam_response(params, fixed, inv[:2], etx, erx, many[k:k + 8], wrx) for k in (0, 8)]
    odd = ctx.beam_response(params, fixed, inv[:2], etx, erx, many[[3, 12]], wrx)
    assert np.array_equal(_bits(odd.re[:, :, 0]), _bits(whole[0].re[:, :, 3])) and np.array_equal(_bits(odd.im[:, :, 1]), _bits(whole[1].im[:, :, 4]))


# ---- 6. every fused function ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fun", FUSED_FUNS)
def test_every_fused_function(ctx, fun):
    try:
        fixed = _setup(ctx, "random7", fun)
        params = _params("hsig", "rx", fun)
        got = _launch(ctx, params, fixed, 9, "3x4", "2x3")
        ctx.launch(params, fixed)
        fused = ctx.get_map()
    finally:
        ctx.set_reflection_coefs(None)
    assert np.isfinite(fused).all() and np.count_nonzero(fused) > fused.size // 3
    assert np.array_equal(_bits(got.total), _bits(fused)) and np.count_nonzero(got.im) > 0
    _same(got, _oracle("random7", "hsig", "rx", fun, "sqrt", "3x4", "2x3", 9))  # (the signed and the zero coefficient included)


# ---- 7. min_order, max_order = 3, a grid of its own ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("role", ["rx", "tx"])
def test_min_order_one_leaves_the_line_of_sight_out(ctx, role):
    fixed = _setup(ctx, "random7")
    got = _launch(ctx, _params("hsig", role, lo=1), fixed, 9, "3x4", "2x3", "linear")
    _same(got, _oracle("random7", "hsig", role, "received_power", "linear", "3x4", "2x3", 9, 1, 2))
    everything = _oracle("random7", "hsig", role, "received_power", "linear", "3x4", "2x3", 9)
    assert got.re.any() and not np.array_equal(got.total, everything.total) and not np.array_equal(got.re, everything.re)


@pytest.mark.parametrize("shape,book", [("1x1", "1x1"), ("3x4", "2x3")])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
def test_max_order_three(ctx, mode, shape, book):
    """The MAXK = 3 instance of the kernel."""
    fixed = _setup(ctx, "random7")
    got = _launch(ctx, _params(mode, "rx", hi=3), fixed, 9, shape, book)
    _same(got, _oracle("random7", mode, "rx", "received_power", "sqrt", shape, book, 9, 0, 3))
    assert not np.array_equal(got.total, _oracle("random7", mode, "rx", "received_power", "sqrt", shape, book, 9).total)


@pytest.mark.parametrize("role", ["rx", "tx"])
def test_a_grid_of_its_own_from_the_walls(ctx, role):
    """19 x 11: 3 x 2 patches, the last column and row of patches with clamped lanes."""
    etx, erx = SHAPES["3x4"]
    wtx, wrx = _book("2x3", "3x4")
    walls, fixed, _, _ = _case("random7")
    X, Y = unit_grid(19, 11)
    inv = _inv_list(9)
    ctx.set_scene(walls)
    ctx.set_grid(X, Y)
    got = ctx.beam_response(_params("hsig", role), fixed, inv, etx, erx, wtx, wrx)
    want = BO.beam_response(walls, fixed, X, Y, inv, AMP_SQRT, etx, erx, wtx, wrx, min_order=0, max_order=2, grid_role=role, **MODES["hsig"])
    assert got.re.shape == (9, 2, 3, 11, 19) and np.count_nonzero(want.im) > want.im.size // 3
    _same(got, want)


# ---- 8. the get ---------------------------------------------------------------------------------------------------------------------------------
def test_get_reads_ranges_of_wavelengths(ctx):
    from differt2d_amd import _lib as L

    nf = 9
    walls, fixed, X, Y = _case("random7")
    ctx.set_scene(walls)
    ctx.set_grid(*unit_grid(19, 11))  # a grid this context has not a result of
    ctx.set_grid(X, Y)
    for args in ((), (0, 1)):
        with pytest.raises(L.D2DError, match="d2d_beam_response_launch") as e:
            ctx.get_beam_response(*args)
        assert e.value.status == -5
    assert ctx._lib.d2d_get_beam_response(ctx._ctx, 0, 1, None, None, None) == -5
    whole = _launch(ctx, _params("hsig", "rx"), fixed, nf, "3x4", "2x3")
    _same(whole, _oracle("random7", "hsig", "rx", "received_power", "sqrt", "3x4", "2x3", nf))
    for first, count in ((0, nf), (3, 1), (nf - 1, 1), (2, 5)):
        part = ctx.get_beam_response(first, count)
        assert part.re.shape == (count, 2, 3) + tuple(ctx.shape)
        _same(part, BeamResponse(whole.re[first:first + count], whole.im[first:first + count], whole.total))
    _same(ctx.get_beam_response(4), BeamResponse(whole.re[4:], whole.im[4:], whole.total))  # count=None: to the end
    part = ctx.get_beam_response(3, 2, with_total=False)
    assert part.total is None and np.array_equal(_bits(part.re), _bits(whole.re[3:5])) and np.array_equal(_bits(part.im), _bits(whole.im[3:5]))
    only_im = np.full(whole.im[6:7].shape, np.nan, F)
    assert ctx._lib.d2d_get_beam_response(ctx._ctx, 6, 1, None, only_im.ctypes.data, None) == 0
    assert np.array_equal(_bits(only_im), _bits(whole.im[6:7]))
    # ranges outside the result
    for first, count in ((-1, 1), (0, 0), (nf - 1, 2), (nf, 1), (0, nf + 1), (0, -1), (2**31 - 1, 2**31 - 1)):
        with pytest.raises(L.D2DError, match="d2d_get_beam_response") as e:
            ctx.get_beam_response(first, count)
        assert e.value.status == -1, (first, count)
    _same(ctx.get_beam_response(), whole)
    # set_grid drops it: the result goes with the grid
    ctx.set_grid(*unit_grid(19, 11))
    with pytest.raises(L.D2DError) as e:
        ctx.get_beam_response()
    assert e.value.status == -5


# ---- 9. state ---------------------------------------------------------------------------------------------------------------------------------
def test_launch_leaves_the_other_results_alone_and_repeats_itself(ctx):
    from differt2d_amd.engine import make_params

    etx, erx = SHAPES["3x4"]
    wtx, wrx = _book("2x3", "3x4")
    inv = _inv_list(9)
    walls, fixed, X, Y = _case("random7")
    ctx.set_scene(walls)
    ctx.set_reflection_coefs(COEF7)
    ctx.set_grid(X, Y)
    try:
        fused_params = make_params(min_order=0, max_order=2, fun="length")
        ctx.launch(fused_params, fixed)
        before = ctx.get_map()
        params = make_params(min_order=0, max_order=2, **MODES["hsig"])
        per_object = make_params(min_order=0, max_order=2, fun="received_power_per_object", height=0.25, **MODES["hsig"])
        # the other nine results
        others = {
            "power_profile": (lambda: ctx.power_profile(params, fixed, 0.0, 3.0, 8), lambda: ctx.get_profile(8)),
            "strongest_paths": (lambda: ctx.strongest_paths(params, fixed, 3), ctx.get_strongest_paths),
            "coherent_field": (lambda: ctx.coherent_field(params, fixed, inv[0], "sqrt"), ctx.get_coherent_field),
            "frequency_response": (lambda: ctx.frequency_response(params, fixed, inv[:3], "sqrt"), ctx.get_frequency_response),
            "power_angle": (lambda: ctx.power_angle(params, fixed, "rx", 0.0, 12), ctx.get_power_angle),
            "array_response": (lambda: ctx.array_response(params, fixed, inv[1], etx, erx, "sqrt"), ctx.get_array_response),
            "array_frequency_response": (lambda: ctx.array_frequency_response(params, fixed, inv[:3], etx, erx, "sqrt"), ctx.get_array_frequency_response),
        }
        held = {name: launch() for name, (launch, _) in others.items()}
        records = ctx.valid_paths(params, fixed)

        def records_again():
            out = {k: np.empty_like(v) for k, v in records.items()}
            vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
            assert ctx._lib.d2d_get_valid_paths(ctx._ctx, records["cell"].size, *(vp(out[k]) for k in ("cell", "cand", "order", "xys", "loss", "valid", "length"))) == 0
            return out

        cot = np.ones((3,) + X.shape, F)
        vjp = ctx.field_coefs_vjp(per_object, fixed, inv[:3], cot, cot, "sqrt")
        got = ctx.beam_response(params, fixed, inv, etx, erx, wtx, wrx)
        _same(got, _oracle("random7", "hsig", "rx", "received_power", "sqrt", "3x4", "2x3", 9))

        def equal(a, b):
            a, b = (tuple(x) if isinstance(x, tuple) else (x,) for x in (a, b))
            return len(a) == len(b) and all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)) for x, y in zip(a, b))

        # the results taken before the launch are still there, bit for bit
        assert np.array_equal(_bits(ctx.get_map()), _bits(before)) and before.any()
        for name, (_, get) in others.items():
            assert equal(get(), held[name]), name
        again = records_again()
        assert records["cell"].size > 0 and all(equal(again[k], records[k]) for k in records)
        assert np.array_equal(ctx.get_field_coefs_vjp(), vjp) and np.any(vjp)
        # the same call twice gives the same bits, also with every other launch in between
        _same(ctx.beam_response(params, fixed, inv, etx, erx, wtx, wrx), got)
        for launch, _ in others.values():
            launch()
        ctx.valid_paths(params, fixed)
        ctx.field_coefs_vjp(per_object, fixed, inv[:3], cot, cot, "sqrt")
        ctx.launch_vg(params, fixed)
        ctx.get_grad_rx()
        _same(ctx.get_beam_response(), got)  # they leave the planes alone in their turn
        # a smaller result after a larger one: the result has the new launch's planes
        few = ctx.beam_response(params, fixed, inv[:2], etx, erx, wtx[:2], wrx[:1])
        assert few.re.shape == (2, 1, 2, *ctx.shape)
        _same(few, BeamResponse(got.re[:2, :1, :2], got.im[:2, :1, :2], got.total))
    finally:
        ctx.set_reflection_coefs(None)


# ---- 10. refusals ------------------------------------------------------------------------------------------------------------------------------
def _refused(ctx, previous, status, word, params, fixed, inv=None, etx=None, erx=None, wtx=None, wrx=None, amp="sqrt"):
    """The launch is refused with ``status`` and a message that has ``word``, and the previous result is still there to get."""
    from differt2d_amd import _lib as L

    book = _book("2x3", "3x4")
    inv = _inv_list(9) if inv is None else inv
    etx = SHAPES["3x4"][0] if etx is None else etx
    erx = SHAPES["3x4"][1] if erx is None else erx
    wtx = book[0] if wtx is None else wtx
    wrx = book[1] if wrx is None else wrx
    with pytest.raises(L.D2DError, match=word) as e:
        ctx.beam_response(params, fixed, inv, etx, erx, wtx, wrx, amp)
    assert e.value.status == status, (e.value.status, str(e.value))
    assert isinstance(e.value, L.D2DUnsupported) == (status == -4)
    _same(ctx.get_beam_response(), previous)
    return str(e.value)


def test_loud_edges(ctx):
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import make_params

    etx, erx = SHAPES["3x4"]
    wtx, wrx = _book("2x3", "3x4")
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
        ctx.beam_response(make_params(approx=True, function="sigmoid", **kw), fixed, inv, etx, erx, wtx, wrx)
    assert ctx._lib.d2d_get_beam_response(ctx._ctx, 0, 1, None, None, None) == -5
    previous = ctx.beam_response(ok, fixed, inv, etx, erx, wtx, wrx)
    assert previous.re.any() and previous.im.any()
    n0 = ctx.txg_fallbacks()
    _refused(ctx, previous, -4, "sigmoid", make_params(approx=True, function="sigmoid", **kw), fixed)
    _refused(ctx, previous, -4, "MinPath / FermatPath", make_params(solver="min", **kw), fixed)
    _refused(ctx, previous, -4, "MinPath / FermatPath", make_params(solver="fermat", **kw), fixed)
    msg = _refused(ctx, previous, -4, "D2D_FUN_CUSTOM", make_params(fun="custom", **kw), fixed)
    assert "d2d_valid_paths" in msg and "d2d_trace_paths" in msg and "d2d_beam_response_launch" in msg
    _refused(ctx, previous, -4, "D2D_OUT_ADD", make_params(out_mode=L.OUT_ADD, **kw), fixed)
    _refused(ctx, previous, -4, "not culled", make_params(grid_role=L.GRID_TX, tol=0.6, **kw), fixed)
    _refused(ctx, previous, -5, "d2d_set_reflection_coefs", make_params(fun="received_power_per_object", height=0.25, **kw), fixed)  # missing coefficients
    # what the wideband array response refuses of the lists
    for bad in (np.zeros(0, F), np.full(1025, 3.0, F)):
        assert "d2d_beam_response_launch" in _refused(ctx, previous, -1, "nf in 1 .. 1024", ok, fixed, inv=bad)
    v = inv.copy()
    v[4] = np.nan
    assert _refused(ctx, previous, -1, "inv_wavelength", ok, fixed, inv=v).endswith("at index 4")
    _refused(ctx, previous, -1, "nt in 1 .. 8", ok, fixed, etx=np.zeros((9, 2), F), wtx=np.ones((2, 9)))
    _refused(ctx, previous, -1, "nr in 1 .. 8", ok, fixed, erx=np.zeros((0, 2), F), wrx=np.ones((2, 0)))
    for amp in (2, -1, "power"):
        _refused(ctx, previous, -1, "amplitude", ok, fixed, amp=amp)
    # the codebooks: nbt = 0, nbr = 9 (and the other way round), a weight that is not finite
    _refused(ctx, previous, -1, "nbt in 1 .. 8", ok, fixed, wtx=np.zeros((0, 4), np.complex64))
    _refused(ctx, previous, -1, "nbr in 1 .. 8", ok, fixed, wrx=np.ones((9, 3), np.complex64))
    _refused(ctx, previous, -1, "nbt in 1 .. 8", ok, fixed, wtx=np.ones((9, 4), np.complex64))
    _refused(ctx, previous, -1, "nbr in 1 .. 8", ok, fixed, wrx=np.zeros((0, 3), np.complex64))
    for value in (np.nan, np.inf, -np.inf, complex(0, np.nan), complex(1, -np.inf)):
        w = wtx.copy()
        w[2, 1] = value
        msg = _refused(ctx, previous, -1, "tx_weights of beam 2", ok, fixed, wtx=w)
        assert msg.endswith("at index 1") and "every weight finite" in msg
        w = wrx.copy()
        w[0, 2] = value
        assert _refused(ctx, previous, -1, "rx_weights of beam 0", ok, fixed, wrx=w).endswith("at index 2")
    _refused(ctx, previous, -1, "tx_weights must be complex", ok, fixed, wtx=np.ones((2, 5)))  # (refused by the binding: the shape)
    # NULL arguments
    fx = np.ascontiguousarray(fixed, F)
    wt, wr = np.ascontiguousarray(wtx[:1, :1]).view(F), np.ascontiguousarray(wrx[:1, :1]).view(F)
    raw = C.CFUNCTYPE(C.c_int, *([C.c_void_p] * 4), C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                      C.c_void_p)(C.cast(ctx._lib.d2d_beam_response_launch, C.c_void_p).value)
    ptrs = [C.addressof(ok), fx.ctypes.data, inv.ctypes.data, etx.ctypes.data, erx.ctypes.data, wt.ctypes.data, wr.ctypes.data]
    for k in range(len(ptrs)):
        p = [None if j == k else v for j, v in enumerate(ptrs)]
        assert raw(ctx._ctx, p[0], p[1], p[2], 1, 0, 1, p[3], 1, p[4], 1, p[5], 1, p[6]) == -1, k
    assert raw(None, *ptrs[:3], 1, 0, 1, ptrs[3], 1, ptrs[4], 1, ptrs[5], 1, ptrs[6]) == -1
    assert raw(ctx._ctx, *ptrs[:3], 1, 0, 1, ptrs[3], 1, ptrs[4], 1, ptrs[5], 1, ptrs[6]) == 0  # (the same call with every pointer: accepted)
    one = np.full((1, 1, 1) + tuple(ctx.shape), np.nan, F)
    assert ctx._lib.d2d_get_beam_response(ctx._ctx, 0, 1, one.ctypes.data, None, None) == 0 and np.isfinite(one).all() and one.any()
    assert ctx._lib.d2d_get_beam_response(ctx._ctx, 0, 2, one.ctypes.data, None, None) == -1  # (that launch had one wavelength)
    previous = ctx.beam_response(ok, fixed, inv, etx, erx, wtx, wrx)
    _refused(ctx, previous, -4, "sigmoid", make_params(approx=True, function="sigmoid", **kw), fixed)
    assert ctx.txg_fallbacks() == n0
    # ... after all of which the context still works (the library's constants are taken as well as the names)
    a = ctx.beam_response(ok, fixed, inv, etx, erx, wtx, wrx, L.D2D_FIELD_AMP_LINEAR)
    _same(a, ctx.beam_response(ok, fixed, inv, etx, erx, wtx, wrx, "linear"))
    assert a.re.any()


# ---- 11. the Scene methods and the utils ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("role", ["rx", "tx"])
def test_scene_methods_mirror_the_context(ctx, role):
    from differt2d_amd import utils
    from differt2d_amd.engine import BeamResponse as BR, make_params
    from differt2d_amd.geometry import Point
    from differt2d_amd.scene import Scene

    walls, fixed, X, Y = _case("random7")
    pts = {"a": Point(xy=fixed), "b": Point(xy=(F(1.0) - fixed).astype(F))}
    scene = Scene.from_walls_array(walls)
    scene = scene.with_transmitters(**pts) if role == "rx" else scene.with_receivers(**pts)
    method = scene.beam_response_on_receivers_grid if role == "rx" else scene.beam_response_on_transmitters_grid
    etx, erx = utils.ula(4, 0.025), utils.ula(3, 0.025, np.pi / 3)
    wtx = utils.steering_weights(etx, np.linspace(0, np.pi, 5), 0.05)
    wrx = utils.steering_weights(erx, [0.3, 2.0], 0.05)
    wl = np.array([0.05, 0.0625, 0.11], F)
    common = dict(tx_elements=etx, rx_elements=erx, tx_weights=wtx, rx_weights=wrx, min_order=0, max_order=2, approx=True, function="hard_sigmoid")
    got = dict(method(X, Y, utils.received_power, dict(r_coef=0.4, height=0.2), wavelengths=wl, **common))
    inv = dict(method(X, Y, utils.received_power, dict(r_coef=0.4, height=0.2), inv_wavelengths=F(1) / wl, amplitude="linear", **common))
    assert list(got) == list(inv) == ["a", "b"]
    ctx.set_scene(walls)
    ctx.set_grid(X, Y)
    params = make_params(min_order=0, max_order=2, r_coef=0.4, height=0.2, grid_role=_role_id(role), **MODES["hsig"])
    for name, pt in pts.items():
        assert isinstance(got[name], BR) and got[name].re.shape == (3, 2, 5, 13, 21)
        _same(got[name], ctx.beam_response(params, pt.xy, F(1) / wl, etx, erx, wtx, wrx, "sqrt"))
        _same(inv[name], ctx.beam_response(params, pt.xy, F(1) / wl, etx, erx, wtx, wrx, "linear"))
        assert got[name].re.any() and got[name].im.any()
    a = got["a"]
    assert utils.beam_response(a).shape == utils.beam_power(a).shape == (3, 2, 5, 13, 21)
    rx, tx, power = utils.best_beam(a)
    lit = a.total > 0
    assert rx.shape == (13, 21) and lit.any() and (power[lit] > 0).all() and (rx >= 0).all() and (tx < 5).all()
    mean = utils.beam_power(a).mean(axis=0)
    assert np.array_equal(power, mean.reshape(10, 13, 21).max(axis=0))
    assert np.unique(tx[lit]).size > 1  # a beam sweep picks different beams in different places
