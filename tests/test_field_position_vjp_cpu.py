"""Host side of the frequency response's position adjoint (no GPU): ``d2d_posgrad.hpp`` and the host's parameter check through a
stand-alone g++ program (plain and with sanitizers), the header bit for bit against the NumPy restatement of
``tests/field_position_vjp_oracle.py``, the float64 oracle against central differences of its own forward sum at displaced end
points and -- in the incoherent limit -- against the project's forward-mode C oracle, the oracle's exact rules and its guards on
the GPU tests' inputs, ``utils.wideband_power_cotangent``, the bindings, the ``Scene`` refusals, the definition block in the three
documents, and the localisation loop on the float64 oracle."""

import functools
import os
import re
import subprocess

import numpy as np
import pytest

import field_position_vjp_oracle as PO
from coherent_field_oracle import AMP_LINEAR, AMP_SQRT
from test_gpu_strongest_paths import COEF7, MODES, _case

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "field_position_vjp_host.cpp")
GXX = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror"]
INV_20 = F(1) / F(0.05)
HEIGHT = 0.25
AMPS = {"sqrt": AMP_SQRT, "linear": AMP_LINEAR}


def inv_list(nf):
    return (INV_20 * (F(1) + np.arange(nf, dtype=F) / F(64))).astype(F)


def bars(nf, shape, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nf,) + tuple(shape)).astype(F), rng.standard_normal((nf,) + tuple(shape)).astype(F)


def fun_kw(fun):
    """The keywords of ``contributions()`` for a fused function of the tests."""
    if fun == "received_power_per_object":
        return dict(fun=fun, coef=COEF7, fun_kwargs=dict(height=HEIGHT))
    if fun == "received_power":
        return dict(fun=fun, fun_kwargs=dict(r_coef=0.5, height=HEIGHT))
    return dict(fun=fun)


@functools.lru_cache(maxsize=None)
def directed_case(scene, role, fun="received_power", lo=0, hi=2, masked=(), grid=None):
    """``(cands, T, Rl, D)`` of a case of ``tests/test_gpu_strongest_paths.py`` in hard mode, read-only; ``grid``: another ``(n, m)`` of
    ``unit_grid``."""
    from conftest import unit_grid

    walls, fixed, X, Y = _case(scene)
    if grid is not None:
        X, Y = unit_grid(*grid)
    out = PO.directed(walls, fixed, X, Y, min_order=lo, max_order=hi, grid_role=role, filter_nodes=set(masked) or None, **MODES["hard"],
                      **fun_kw(fun))
    for a in out[1:]:
        a.setflags(write=False)
    return out


# ---- 1. the stand-alone host build ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """The stand-alone program, plain and with sanitizers linked in by the compiler (nothing is preloaded, nothing is loaded into
    Python)."""
    d = tmp_path_factory.mktemp("pv_host")
    out = {}
    for name, extra in (("plain", []), ("asan_ubsan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])):
        out[name] = str(d / f"pv_host_{name}")
        subprocess.check_call(GXX + extra + ["-o", out[name], SRC])
    return out


@pytest.mark.parametrize("build", ["plain", "asan_ubsan"])
def test_stand_alone_host_program(programs, build):
    """posgrad_params (nf, the entries with their index, the amplitude, in that order), the memory rule against 128-bit arithmetic and
    at its boundary byte, the chunk plan and the header at points worked by hand."""
    done = subprocess.run([programs[build]], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(done.stdout)
    assert done.returncode == 0, done.stdout
    assert "0 failures" in done.stdout


def _run_header(exe, tmp_path, fun_id, amplitude, cols):
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    n = cols[0].size
    with open(inp, "wb") as f:
        f.write(np.int64(n).tobytes() + np.int32(fun_id).tobytes() + np.int32(amplitude).tobytes())
        for c in cols:
            f.write(np.ascontiguousarray(c, F).tobytes())
    subprocess.run([exe, inp, outp], check=True, timeout=300)
    return np.fromfile(outp, F).reshape(5, n)


def flat_inputs():
    t, r, h2, inv, rb, ib = PO.header_inputs()
    return (t, r, h2, inv[0], inv[1], rb[0], rb[1], ib[0], ib[1]), (t, r, h2, inv, rb, ib)


@pytest.mark.parametrize("build", ["plain", "asan_ubsan"])
def test_header_equals_the_numpy_restatement_bit_for_bit(programs, tmp_path, build):
    """Every fun_id, both amplitudes, ``r`` across 1e-3 .. 1e3 and the special values: ``a``, ``rho``, ``kr``, the two-step fold ``g``
    and ``G`` of the g++ build equal the restatement in every bit (any NaN equals any NaN)."""
    cols, args = flat_inputs()
    r = cols[1]
    fin = np.isfinite(r) & (r > 0)
    assert r[fin].min() <= 1.001e-3 and r[fin].max() >= 0.999e3 and cols[0].size > 60000
    for fun, fid in PO.FUN_IDS.items():
        for amplitude in (AMP_SQRT, AMP_LINEAR):
            got = _run_header(programs[build], tmp_path, fid, amplitude, cols)
            want = PO.header(fun, amplitude, *args)
            for name, g, w in zip("a rho kr g G".split(), got, want):
                both_nan = np.isnan(g) & np.isnan(w)
                bad = (g.view(np.uint32) != np.ascontiguousarray(w, F).view(np.uint32)) & ~both_nan
                assert not bad.any(), (fun, amplitude, name, int(bad.sum()), int(np.flatnonzero(bad)[0]))
            assert np.isfinite(got[4]).mean() > 0.99  # (the list is not NaN all over)
    assert len(PO.FUN_IDS) == 5


# ---- 2. the float64 oracle against central differences -----------------------------------------------------------------------------------
H_STEP = 1e-6


def _loss_cells(H, rb, ib):
    nf = H.shape[0]
    return (rb.reshape(nf, -1).astype(np.float64) * H.real + ib.reshape(nf, -1).astype(np.float64) * H.imag).sum(axis=0)


@functools.lru_cache(maxsize=None)
def _stable_cells(scene, role):
    """Cells whose visibility -- which candidates contribute -- is the same with either end displaced by ``+-H_STEP`` along either
    axis (fp32 positions, the oracle's own validity).  Every cell strictly inside the unit square must be among them: that is the
    assertion that the visibility is unchanged at ``+-h``.  A cell ON a wall of the bounding square sees its paths appear and vanish
    as it crosses the wall; the response is not differentiable there and such a cell is not compared."""
    from conftest import unit_grid  # noqa: F401

    walls, fixed, X, Y = _case(scene)
    base = directed_case(scene, role)[1]
    nz0 = ~(base == 0)
    stable = np.ones(X.size, bool)
    h = F(H_STEP)
    for axis in (0, 1):
        for sign in (-1, 1):
            f2 = np.array(fixed, F).copy()
            f2[axis] = F(f2[axis] + sign * h)
            X2, Y2 = (X + sign * h if axis == 0 else X).astype(F), (Y + sign * h if axis == 1 else Y).astype(F)
            for fx, gx, gy in ((f2, X, Y), (fixed, X2, Y2)):
                _, T, _, _ = PO.contributions(walls, fx, gx, gy, min_order=0, max_order=2, grid_role=role, **MODES["hard"], **fun_kw("received_power"))
                stable &= ((~(T == 0)) == nz0).all(axis=0)
    inside = ((X > 0) & (X < 1) & (Y > 0) & (Y < 1)).reshape(-1)
    assert stable[inside].all(), int((~stable[inside]).sum())
    assert stable.mean() > 0.6
    return stable


@pytest.mark.parametrize("amplitude", ["sqrt", "linear"])
@pytest.mark.parametrize("role", ["rx", "tx"])
def test_oracle_is_the_central_difference_of_its_forward_sum(role, amplitude):
    """Both ends, both roles, both amplitudes, orders 0-2 on ``obstacle``: per cell, the oracle's ``cell_bar`` and ``fixed_terms``
    against central differences of ``sum_j (rb_j Re H_j + ib_j Im H_j)`` with the path lengths recomputed in float64 by mirror images at
    end points displaced by ``+-h`` and the candidates' visibility frozen.

    The tolerance follows from the step.  One term is ``f(r(x))`` with ``f = a(r) e^(-j kappa r)``, ``kappa = 2 pi / lambda``; with
    ``Lam = kappa + 3 / rho0`` (``rho0 = sqrt(h2 + r^2)``: the n-th logarithmic derivative of the received power's amplitude is below
    ``(n / rho0)^n``) and ``|r'| <= 1``, ``|r''| <= 1 / r``, ``|r'''| <= 3 / r^2``, the third derivative is below ``A (Lam + 1 / r)^3``
    with ``A = |a| (|rb| + |ib|)``, so the central difference is off by at most ``h^2 / 6`` times that; the rounding of the two float64
    sums, each of magnitude ``sum A``, adds ``n 2^-52 sum A / (2 h)``.  The oracle takes its amplitude from the fp32 ``T`` (the
    forward sum evaluates ``fun`` in float64: up to 6 roundings) and its directions from the fp32 ``D`` (the subtraction of two fp32
    points and, for an image, the roundings of the mirror chain: a few units on components of magnitude up to 4):
    ``16 * 2^-24 A Lam`` covers them with margin.  Cells within ``1e-3`` of the fixed end point (the cell on it:
    ``1 / r`` has no bound there) are not compared; there is at most one."""
    amp = AMPS[amplitude]
    walls, fixed, X, Y = _case("obstacle")
    cands, T, Rl, D = directed_case("obstacle", role)
    nf = 9
    inv = inv_list(nf)
    rb, ib = bars(nf, X.shape, 31)
    ph = PO.physics(T, Rl, D, "received_power", HEIGHT, inv, rb, ib, amp, role)
    PO.guards(T, Rl, D, role, ph)
    stable = _stable_cells("obstacle", role)
    mirror = PO.Mirror(walls)
    grid = np.stack([X.reshape(-1), Y.reshape(-1)], axis=1).astype(np.float64)
    fx = np.asarray(fixed, np.float64)
    ends = {"rx": lambda f, g: (f, g), "tx": lambda f, g: (g, f)}[role]  # (tx, rx) from (fixed, grid)

    tx0, rx0 = ends(fx, grid)

    def loss(f, g):
        tx, rx = ends(f, g)
        return _loss_cells(PO.forward(mirror, cands, T, Rl, "received_power", HEIGHT, 0.5, inv, amp, tx, rx, tx0, rx0), rb, ib)

    # the mirror's lengths are the oracle's fp32 lengths to fp32 accuracy wherever a candidate contributes
    for ci, cand in enumerate(cands):
        nz = ~(T[ci] == 0)
        if nz.any():
            r = np.broadcast_to(mirror.lengths(cand, tx0, rx0), nz.shape)
            assert np.abs(r[nz] - Rl[ci][nz]).max() <= 8 * 2.0**-24 * 4.0, (ci, np.abs(r[nz] - Rl[ci][nz]).max())
    # the step's tolerance per cell
    nz = ~(T == 0)
    r64 = np.where(nz, Rl.astype(np.float64), np.inf)
    near = (r64 < 1e-3).any(axis=0)
    assert near.sum() <= 1
    a = np.abs(np.where(nz, T.astype(np.float64), 0.0))
    a = np.sqrt(a) if amp == AMP_SQRT else a
    A = a * (np.abs(rb) + np.abs(ib)).reshape(nf, -1).astype(np.float64).sum(axis=0)[None, :]
    kappa = 2 * np.pi * float(inv.max())
    lam = kappa + 3.0 / np.sqrt(HEIGHT * HEIGHT + r64 * r64) + 1.0 / r64
    h = H_STEP
    lam = np.where(nz, lam, 0.0)
    tol = (h * h / 6.0) * (A * lam**3).sum(axis=0) + (len(cands) * nf) * 2.0**-52 * A.sum(axis=0) / (2 * h) + 16 * 2.0**-24 * (A * lam).sum(axis=0)
    use = stable & ~near & (tol > 0)
    assert use.sum() >= 0.6 * use.size and np.isfinite(tol[use]).all()
    worst = 0.0
    for axis in (0, 1):
        e = np.zeros(2)
        e[axis] = h
        for name, want, fd in (("cell_bar", ph.cell_bar, (loss(fx, grid + e) - loss(fx, grid - e)) / (2 * h)),
                               ("fixed_terms", ph.fixed_terms, (loss(fx + e, grid) - loss(fx - e, grid)) / (2 * h))):
            err = np.abs(fd - want[:, axis])
            worst = max(worst, float((err[use] / tol[use]).max()))
            assert (err[use] <= tol[use]).all(), (name, axis, float((err[use] / tol[use]).max()))
            lit = use & (np.abs(want[:, axis]) > 0)
            assert lit.sum() >= 0.5 * use.size  # (the comparison is not of zeros)
            assert (tol[lit] <= 1e-5 * ph.mag[0 if name == "cell_bar" else 1][lit, :].sum(axis=1)).all()  # ... and the tolerance binds
    print(f"central differences, {role} grid, {amplitude}: worst error / tolerance = {worst:.3g}")


# ---- 3. the incoherent limit against the forward-mode C oracle ---------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["obstacle", "random7"])
def test_incoherent_limit_is_the_power_map_gradient_of_the_c_oracle(scene):
    """LINEAR, one entry ``inv = 0``, ``re_bar = 1``, ``im_bar = 0``: ``re`` is the power map, so ``cell_bar`` on an RX grid is its
    gradient -- ``oracle.c_oracle.power_map_grad`` (hard, orders 0-2), within 1e-5 of the cell's summed term magnitude (the
    project's tolerance for K2's gradients), on every cell where that oracle is finite and a contribution exists; no cell is left out."""
    from oracle import c_oracle as CO

    walls, fixed, X, Y = _case(scene)
    cands, T, Rl, D = directed_case(scene, "rx")
    ones, zeros = np.ones((1,) + X.shape, F), np.zeros((1,) + X.shape, F)
    ph = PO.physics(T, Rl, D, "received_power", HEIGHT, [0.0], ones, zeros, AMP_LINEAR, "rx")
    _, grad = CO.power_map_grad(walls, fixed, X, Y, min_order=0, max_order=2, approx=False, fun="received_power", r_coef=0.5, height=HEIGHT)
    grad = grad.reshape(-1, 2)
    mag = ph.mag[0].sum(axis=1)  # the cell's summed term magnitude, both components
    have = (ph.n_terms > 0) & (mag > 0)
    finite = np.isfinite(grad).all(axis=1)
    assert finite.all(), int((~finite).sum())  # 100 % of the cells in hard mode: nothing is left out
    assert have.sum() >= 0.5 * have.size  # (cells on the bounding walls, inside the obstacle or behind every wall see nothing)
    err =np.abs(ph.cell_bar - grad).max(axis=1)
    print(f"{scene}: worst |cell_bar - C oracle| / magnitude = {(err[have] / mag[have]).max():.3g} over {have.sum()} of {have.size} cells")
    assert (err[have] <= 1e-5 * mag[have]).all(), float((err[have] / mag[have]).max())
    assert not grad[~have].any()  # a cell without a contribution has no gradient either


# ---- 4. rules and guards -----------------------------------------------------------------------------------------------------------------
def test_oracle_rules():
    """Zero cotangents give zeros of sign plus in every bit, doubled cotangents exactly doubled planes, an appended wavelength with
    zero cotangents changes no bit (within a block and across a block edge), and the restatement lies within the bound of the float64
    evaluation."""
    cands, T, Rl, D = directed_case("obstacle", "rx")
    cells = T.shape[1]
    for nf in (8, 16):
        inv = inv_list(nf + 1)
        rb, ib = bars(nf + 1, (cells,), 41)
        rb[nf] = ib[nf] = 0
        for amp in (AMP_SQRT, AMP_LINEAR):
            short = PO.restate(T, Rl, D, "received_power", HEIGHT, inv[:nf], rb[:nf], ib[:nf], amp, "rx")
            more = PO.restate(T, Rl, D, "received_power", HEIGHT, inv, rb, ib, amp, "rx")
            twice = PO.restate(T, Rl, D, "received_power", HEIGHT, inv[:nf], 2 * rb[:nf], 2 * ib[:nf], amp, "rx")
            zero = PO.restate(T, Rl, D, "received_power", HEIGHT, inv[:nf], 0 * rb[:nf], F(-0.0) * ib[:nf], amp, "rx")
            for s, m, t2, z in zip(short, more, twice, zero):
                assert np.array_equal(s.view(np.uint32), m.view(np.uint32))
                assert np.array_equal((F(2) * s).view(np.uint32), t2.view(np.uint32))
                assert not z.view(np.uint32).any()
                assert s.any()
            ph = PO.physics(T, Rl, D, "received_power", HEIGHT, inv[:nf], rb[:nf], ib[:nf], amp, "rx")
            PO.guards(T, Rl, D, "rx", ph)
            for got, want, bound in ((short.cell_bar, ph.cell_bar, ph.bound[0]), (short.fixed_terms, ph.fixed_terms, ph.bound[1])):
                assert (np.abs(got.astype(np.float64) - want) <= bound).all()
    # the zero-cotangent wavelength inside a block changes nothing either
    inv = inv_list(3)
    rb, ib = bars(3, (cells,), 42)
    rb[1] = ib[1] = 0
    a = PO.restate(T, Rl, D, "length", HEIGHT, inv, rb, ib, AMP_LINEAR, "tx")
    b = PO.restate(T, Rl, D, "length", HEIGHT, inv[[0, 2]], rb[[0, 2]], ib[[0, 2]], AMP_LINEAR, "tx")
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


GPU_CASES = [("obstacle", None), ("random7", None), ("random7", (13, 19)), ("square_centre", None)]


@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("scene,grid", GPU_CASES)
def test_oracle_guards_on_the_gpu_tests_inputs(scene, grid, role):
    """The comparisons of ``tests/test_gpu_field_position_vjp.py`` do not pass on empty ground: contributions of every order, both
    ends lit in most cells, the bound small against the scale, and on ``square_centre`` -- the one grid that passes through the fixed
    end point -- a contributing line of sight without a direction."""
    cands, T, Rl, D = directed_case(scene, role, grid=grid)
    nf = 9
    cells = T.shape[1]
    rb, ib = bars(nf, (cells,), 43)
    ph = PO.physics(T, Rl, D, "received_power", HEIGHT, inv_list(nf), rb, ib, AMP_SQRT, role)
    orders = {len(c) for ci, c in enumerate(cands) if (~(T[ci] == 0)).any()}
    assert orders == {0, 1, 2}, orders
    PO.guards(T, Rl, D, role, ph, need_no_direction=scene == "square_centre")


def test_a_cell_on_the_fixed_end_point_has_no_direction_and_adds_nothing():
    """A grid through the fixed end point: the line of sight of that cell has length zero and no direction at either end; with
    ``one`` as the path function it still contributes (``t = 1``) and the definition leaves it out at both ends, bit for bit and in the
    float64 evaluation alike."""
    from oracle import ref as R

    walls = R.square_scene_walls()
    fixed = np.array([0.5, 0.5], F)
    x = np.linspace(0, 1, 5).astype(F)
    X, Y = np.meshgrid(x, x)
    cands, T, Rl, D = PO.directed(walls, fixed, X, Y, min_order=0, max_order=1, grid_role="rx", approx=False, fun="one")
    centre = 12
    assert len(cands[0]) == 0 and T[0, centre] == 1 and Rl[0, centre] < 1e-6  # (the reference adds eps to every segment's components)
    _, _, ok = PO.unit_dir(D[0, :, 0], D[0, :, 1])
    assert not ok[centre] and ok.sum() == ok.size - 1
    rb, ib = bars(2, (25,), 44)
    inv = inv_list(2)
    got = PO.restate(T, Rl, D, "one", HEIGHT, inv, rb, ib, AMP_LINEAR, "rx")
    los_only = PO.restate(T[:1], Rl[:1], D[:1], "one", HEIGHT, inv, rb, ib, AMP_LINEAR, "rx")
    assert not los_only.cell_bar[centre].view(np.uint32).any() and not los_only.fixed_terms[centre].view(np.uint32).any()
    others = ~(T[0] == 0) & (np.arange(25) != centre)
    assert others.sum() >= 8 and los_only.cell_bar[others].any(axis=1).all() and los_only.fixed_terms[others].any(axis=1).all()
    assert np.isfinite(got.cell_bar).all() and np.isfinite(got.fixed_terms).all() and got.cell_bar[others].any(axis=1).all()


def test_wideband_power_cotangent_against_numpy():
    from differt2d_amd.engine import FrequencyResponse
    from differt2d_amd.utils import wideband_power, wideband_power_cotangent

    rng = np.random.default_rng(45)
    shape = (5, 3, 4)
    re, im = rng.standard_normal(shape).astype(F), rng.standard_normal(shape).astype(F)
    fr = FrequencyResponse(re, im, np.zeros(shape[1:], F))
    J, rb, ib = wideband_power_cotangent(fr)
    assert isinstance(J, float) and abs(J - wideband_power(fr).sum()) <= 1e-12 * J
    assert rb.dtype == ib.dtype == F and rb.shape == ib.shape == shape
    assert np.array_equal(rb, (2.0 / 5 * re.astype(np.float64)).astype(F)) and np.array_equal(ib, (2.0 / 5 * im.astype(np.float64)).astype(F))
    w = rng.random(shape[1:])
    Jw, rbw, ibw = wideband_power_cotangent(fr, w)
    assert abs(Jw - (w * wideband_power(fr)).sum()) <= 1e-12 * Jw
    # the cotangents are the objective's derivatives (it is quadratic: the difference is the derivative plus w step^2 / nf, exactly)
    bumped = FrequencyResponse(re.copy(), im.copy(), fr.total)
    bumped.im[2, 1, 3] += F(1e-3)
    step = float(bumped.im[2, 1, 3]) - float(im[2, 1, 3])
    assert abs((wideband_power_cotangent(bumped, w)[0] - Jw - w[1, 3] * step * step / 5) / step - float(ibw[2, 1, 3])) <= 1e-6


def test_bindings_and_abi_version():
    from differt2d_amd import _lib as L
    from differt2d_amd import utils
    from differt2d_amd.engine import Context, PositionGradient
    from differt2d_amd.scene import Scene

    assert L.D2D_ABI_VERSION == 12 and L.D2D_POS_CHUNK == PO.POS_CHUNK == 8
    names = [s[0] for s in L.SYMBOLS]
    for name in ("d2d_field_position_vjp_launch", "d2d_get_field_position_vjp", "d2d_selftest_posgrad"):
        assert name in names
    assert callable(Context.field_position_vjp) and callable(Context.launch_field_position_vjp) and callable(Context.get_field_position_vjp)
    assert callable(Scene.frequency_response_position_vjp_on_receivers_grid) and callable(Scene.frequency_response_position_vjp_on_transmitters_grid)
    assert callable(utils.wideband_power_cotangent) and PositionGradient._fields == ("cell_bar", "fixed_terms", "fixed_bar")
    header = open(os.path.join(ROOT, "include", "d2d.h")).read()
    assert "#define D2D_ABI_VERSION 12" in header and "#define D2D_POS_CHUNK 8" in header
    for decl in ("int d2d_field_position_vjp_launch(", "int d2d_get_field_position_vjp(", "int d2d_selftest_posgrad("):
        assert decl in header
    lib = L.load()  # (the library exports them: getattr raises otherwise)
    assert lib.d2d_field_position_vjp_launch and lib.d2d_get_field_position_vjp and lib.d2d_selftest_posgrad and lib.d2d_abi_version() == 12


def test_scene_refusals_without_a_launch():
    """What the ``Scene`` methods refuse themselves, before a context exists: both or neither of the wavelength arguments, a function
    that is not fused, another path class, a smoothed validity."""
    from differt2d_amd import _lib as L
    from differt2d_amd.geometry import MinPath
    from differt2d_amd.scene import Scene
    from differt2d_amd.utils import received_power

    scene = Scene.square_scene()
    x = np.linspace(0.1, 0.9, 4).astype(F)
    X, Y = np.meshgrid(x, x)
    rb = ib = np.zeros((2, 4, 4), F)
    for method in (scene.frequency_response_position_vjp_on_receivers_grid, scene.frequency_response_position_vjp_on_transmitters_grid):
        with pytest.raises(ValueError, match="exactly one of wavelengths= and inv_wavelengths="):
            method(X, Y, received_power, None, rb, ib, approx=False)
        with pytest.raises(ValueError, match="exactly one of wavelengths= and inv_wavelengths="):
            method(X, Y, received_power, None, rb, ib, wavelengths=[0.05, 0.06], inv_wavelengths=[20, 21], approx=False)
        with pytest.raises(L.D2DUnsupported, match="is not fused natively: the position adjoint needs the path function's derivative"):
            method(X, Y, lambda path: 1.0, None, rb, ib, wavelengths=[0.05, 0.06], approx=False)
        with pytest.raises(L.D2DUnsupported, match="the position adjoint covers ImagePath only, not path_cls=MinPath"):
            method(X, Y, received_power, None, rb, ib, wavelengths=[0.05, 0.06], path_cls=MinPath, approx=False)
        for kw in (dict(approx=True), dict(approx=True, function="sigmoid")):
            with pytest.raises(L.D2DUnsupported, match="hard validity only .approx=False.: a smoothed validity depends on the positions itself"):
                method(X, Y, received_power, None, rb, ib, wavelengths=[0.05, 0.06], **kw)


def _definition(text):
    """The definition block of K3-X ``d2d::PosGradSink`` in a document: from the line that names ``params``, ``fixed`` and the role of
    the grid to the line about NaN contributions, with comment prefixes, Markdown's code fences and all white space taken out."""
    lines = text.splitlines()
    first = next(i for i, line in enumerate(lines) if "`params`, `fixed`, the role of the grid, `inv_wavelength[nf]`" in line)
    last = next(i for i in range(first, len(lines)) if "and thereby `fixed_bar`, and no other cell's." in lines[i])
    block = [re.sub(r"^\s*\*( |$)", "", line) for line in lines[first:last + 1] if line.strip() != "```"]
    return re.sub(r"\s+", "", "\n".join(block))


def test_definition_reads_the_same_in_the_header_the_design_and_the_readme():
    docs = {name: open(os.path.join(ROOT, *name.split("/"))).read() for name in ("include/d2d.h", "DESIGN.md", "README.md")}
    for name, text in docs.items():
        assert "K3-X `d2d::PosGradSink`" in text, name
    blocks = {name: _definition(text) for name, text in docs.items()}
    want = blocks["include/d2d.h"]
    assert len(want) > 2000 and "G=a*g" in want and "pr=kr*c-w*s;pi=kr*s+w*c" in want and "POS_CHUNK=D2D_POS_CHUNK=8" in want
    assert "if(okf){fixed_terms.x=fixed_terms.x-G*ufx;fixed_terms.y=fixed_terms.y-G*ufy}" in want
    for name, got in blocks.items():
        assert got == want, name
    # the header's own text states the same arithmetic
    hpp = open(os.path.join(ROOT, "differt2d_amd", "csrc", "d2d_posgrad.hpp")).read()
    assert "pr = kr*c - w*s ;  pi = kr*s + w*c" in hpp and "6.2831855f" in hpp


# ---- 5. the localisation loop on the float64 oracle --------------------------------------------------------------------------------------
# The truth lies 0.0036 from the start: 0.45 rad of phase at these wavelengths, inside the misfit's basin (it is periodic in the path
# lengths: a quarter wavelength, 0.0125, is where the basin ends).  The rate is 1 / curvature to within a factor of 2: the first
# gradient is 2.3e6 at that distance, a curvature of 6e8.
LOC = dict(scene="obstacle", nf=8, start=(0.2, 0.2), truth=(0.203, 0.198), steps=10, rate=2e-9, gpu_fraction=1e-3)


def localisation_inputs():
    walls, _, X, Y = _case(LOC["scene"])
    return walls, X, Y, inv_list(LOC["nf"]), np.array(LOC["truth"], F), np.array(LOC["start"], F)


def test_localisation_loop_on_the_float64_oracle():
    """``obstacle``, ``nf = 8``, LINEAR: the target is the float64 response at a displaced transmitter; from the start, gradient
    descent on ``utils.field_misfit`` with the oracle's ``fixed_bar`` at a fixed rate.  The misfit falls at every step and ends below
    a tenth of the fraction of its start that the GPU test asserts (``LOC["gpu_fraction"]``): the reference alone holds the condition
    with a margin of 10 x.  Every step re-derives the contributions at the current transmitter (the visibility is the oracle's own)."""
    from differt2d_amd.engine import FrequencyResponse
    from differt2d_amd.utils import field_misfit

    walls, X, Y, inv, truth, pos = localisation_inputs()
    nf = inv.size

    def response(fixed):
        cands, T, Rl, D = PO.directed(walls, fixed, X, Y, min_order=0, max_order=2, grid_role="rx", **MODES["hard"], **fun_kw("received_power"))
        a = T.astype(np.float64)
        u = Rl.astype(np.float64)[None] * inv.astype(np.float64)[:, None, None]
        H = (np.where(T == 0, 0.0, a)[None] * np.exp(-2j * np.pi * u)).sum(axis=1)
        return (T, Rl, D), H.reshape((nf,) + X.shape)

    _, target = response(truth)
    losses = []
    for _ in range(LOC["steps"]):
        geo, H = response(pos)
        fr = FrequencyResponse(H.real.astype(F), H.imag.astype(F), np.zeros(X.shape, F))
        loss, rb, ib = field_misfit(fr, target)
        losses.append(loss)
        ph = PO.physics(*geo, "received_power", HEIGHT, inv, rb, ib, AMP_LINEAR, "rx")
        pos = (pos.astype(np.float64) - LOC["rate"] * ph.fixed_terms.sum(axis=0)).astype(F)
    losses.append(field_misfit(FrequencyResponse(*(lambda H: (H.real.astype(F), H.imag.astype(F)))(response(pos)[1]), np.zeros(X.shape, F)), target)[0])
    print("misfit:", " ".join(f"{v:.4g}" for v in losses), "position", pos)
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    assert losses[-1] <= 0.1 * LOC["gpu_fraction"] * losses[0], (losses[-1] / losses[0])
