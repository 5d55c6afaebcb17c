"""Host side of the frequency response's wall adjoint (no GPU): ``d2d_wallgrad.hpp`` and the host's parameter check and memory rule
through a stand-alone g++ program (plain and with sanitizers), the header bit for bit against the NumPy restatement of
``tests/field_walls_vjp_oracle.py``, the float64 oracle against central differences of the frozen-visibility forward sum on displaced
walls and -- in the incoherent limit -- against torch autodiff of the reference's own chain, the exact rules on the restatement, the
oracle's guards on the GPU tests' inputs, the bindings, the ``Scene`` refusals, the definition block in the three documents, and a
wall-fitting loop on the float64 oracle."""

import functools
import os
import re
import subprocess

import numpy as np
import pytest

import field_position_vjp_oracle as PO
import field_walls_vjp_oracle as WO
from coherent_field_oracle import AMP_LINEAR, AMP_SQRT
from test_field_position_vjp_cpu import AMPS, HEIGHT, bars, fun_kw, inv_list
from test_gpu_strongest_paths import MODES, _case

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "field_walls_vjp_host.cpp")
GXX = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror"]


@functools.lru_cache(maxsize=None)
def segment_case(scene, role, fun="received_power", lo=0, hi=2, masked=(), grid=None):
    """``(cands, T, Rl, S, p0)`` of a case of ``tests/test_gpu_strongest_paths.py`` in hard mode, read-only; ``grid``: another ``(n, m)``
    of ``unit_grid``.  ``received_power_per_object`` takes its ``T`` from ``strongest_paths_oracle.contributions`` (the left fold of the
    coefficients), the lengths and segments do not depend on the path function."""
    from conftest import unit_grid

    walls, fixed, X, Y = _case(scene)
    if grid is not None:
        X, Y = unit_grid(*grid)
    common = dict(min_order=lo, max_order=hi, grid_role=role, filter_nodes=set(masked) or None, **MODES["hard"])
    if fun == "received_power_per_object":
        cands, _, Rl, S = WO.segment_contributions(walls, fixed, X, Y, fun="one", **common)
        cands2, T, Rl2, _ = PO.contributions(walls, fixed, X, Y, **common, **fun_kw(fun))
        assert [tuple(c) for c in cands] == [tuple(c) for c in cands2] and np.array_equal(Rl, Rl2, equal_nan=True)
    else:
        kw = fun_kw(fun)
        cands, T, Rl, S = WO.segment_contributions(walls, fixed, X, Y, fun=kw["fun"], fun_kwargs=kw.get("fun_kwargs"), **common)
    p0 = WO.first_point(fixed, X, Y, role)
    for a in (T, Rl, S, p0):
        a.setflags(write=False)
    return cands, T, Rl, S, p0


# ---- 1. the stand-alone host build ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """The stand-alone program, plain and with sanitizers linked in by the compiler (nothing is preloaded, nothing is loaded into
    Python)."""
    d = tmp_path_factory.mktemp("wv_host")
    out = {}
    for name, extra in (("plain", []), ("asan_ubsan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])):
        out[name] = str(d / f"wv_host_{name}")
        subprocess.check_call(GXX + extra + ["-o", out[name], SRC])
    return out


@pytest.mark.parametrize("build", ["plain", "asan_ubsan"])
def test_stand_alone_host_program(programs, build):
    """wallgrad_params (nf, the entries with their index, the amplitude, in that order), the memory rule against 128-bit arithmetic and
    at its boundary byte, the chunk plan and the header at points worked by hand (``s`` at 0 and 1, a zero-length wall, a zero
    segment, a NaN)."""
    done = subprocess.run([programs[build]], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(done.stdout)
    assert done.returncode == 0, done.stdout
    assert "0 failures" in done.stdout


def _run_header(exe, tmp_path, cols):
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    n = cols[0].size
    with open(inp, "wb") as f:
        f.write(np.int64(n).tobytes())
        for c in cols:
            f.write(np.ascontiguousarray(c, F).tobytes())
    subprocess.run([exe, inp, outp], check=True, timeout=300)
    return np.fromfile(outp, F).reshape(5, n)


@pytest.mark.parametrize("build", ["plain", "asan_ubsan"])
def test_header_equals_the_numpy_restatement_bit_for_bit(programs, tmp_path, build):
    """Seeded walls, points and segments and the special values (a zero-length wall, a zero segment, ``s`` at 0 and 1, NaN and
    infinities): ``q`` after the bounce, ``Wa``, ``Wb`` and ``ok`` of the g++ build equal the restatement in every bit (any NaN equals
    any NaN)."""
    cols = WO.header_inputs()
    assert cols[0].size > 60000
    got = _run_header(programs[build], tmp_path, cols)
    want = WO.bounce(*cols)
    for name, g, w in zip("qx qy Wa Wb ok".split(), got, want):
        w = np.ascontiguousarray(w, F)
        both_nan = np.isnan(g) & np.isnan(w)
        bad = (g.view(np.uint32) != w.view(np.uint32)) & ~both_nan
        assert not bad.any(), (name, int(bad.sum()), int(np.flatnonzero(bad)[0]))
    assert np.isfinite(got[2]).mean() > 0.99 and 0 < got[4].mean() < 1  # (the list is not NaN all over, and ok takes both values)
    # the special rows: s at exactly 0 and 1 hands the whole term to one end, a zero-length wall adds zeros, a zero segment is not ok
    n = cols[0].size - 18
    assert got[2][n + 1] == 2 and got[3][n + 1] == 0 and got[2][n + 2] == 0 and got[3][n + 2] == 2
    assert got[2][n + 3] == 0 and got[3][n + 3] == 0 and got[4][n + 3] == 1
    assert got[4][n + 4] == 0 and got[4][n + 5] == 0 and got[0][n + 4] == F(0.5) and got[1][n + 4] == F(0.25)
    assert np.isnan(got[2][n + 6]) and np.isnan(got[3][n + 6]) and got[4][n + 6] == 1


# ---- 2. the float64 oracle against central differences on displaced walls ----------------------------------------------------------------
H_STEP = 1e-6


def _loss_cells(H, rb, ib):
    nf = H.shape[0]
    return rb.reshape(nf, -1).astype(np.float64) * H.real + ib.reshape(nf, -1).astype(np.float64) * H.imag


@pytest.mark.parametrize("amplitude", ["sqrt", "linear"])
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("scene", ["obstacle", "random7"])
def test_oracle_is_the_central_difference_of_the_forward_sum_on_displaced_walls(scene, role, amplitude):
    """Every wall of the scene, all four coordinates of its two end points, each displaced by ``+h`` and ``-h`` (eight scenes per wall):
    the oracle's ``walls_bar[w][e][d] = normal_bar[w][e] n_w[d]`` against central differences of ``sum_cells sum_j (rb_j Re H_j + ib_j Im
    H_j)`` of ``field_position_vjp_oracle.forward``, with the path lengths recomputed in float64 by mirror images on the displaced walls
    and the candidates' visibility frozen.  A displacement along the wall moves no image: those components are zero on both sides,
    which the comparison holds too.  Only the candidates that visit the wall enter a difference (the others cancel exactly and would
    only add rounding), and the differences are taken per cell and wavelength before they are summed.

    The tolerance follows from the step, as in ``tests/test_field_position_vjp_cpu.py``.  One term is ``f(r(x))`` with ``f = a(r) e^(-j
    kappa r)`` and ``Lam = kappa + 3 / rho0`` bounding its logarithmic derivatives; with respect to an end-point coordinate ``|r'| <= 2``
    (``gam (1 - s)``, the bounce lies on the wall), and every further derivative gains at most a factor ``kap = 1 / L_w + 1 / r`` (the
    normal turns by ``dx / L_w``; the length is the distance from the last image to the receiver, a straight line of length ``r``,
    and a distance at range ``r`` curves by ``1 / r``), so the third derivative is below ``A (2 Lam + 8 kap)^3`` with ``A = |a| sum_j (|rb_j| + |ib_j|)`` and the
    central difference is off by ``h^2 / 6`` times that.  The rounding of the two float64 sums of a cell adds ``n_j 2^-52 A / (2 h)``
    per term.  The oracle takes its amplitude from the fp32 ``T`` (up to 6 roundings), ``gam`` from the fp32 segment and the fp32 normal
    (10 units, absolute) and ``s`` from the fp32 segments' sum and the fp32 table (``(i + 1) qabs sqrt(2) / L_w + 4`` units): ``(40 + 3
    K qabs / L_w) 2^-24 A Lam`` covers them with ``|gam| <= 2``.  The mirror's float64 lengths differ from the fp32 ``Rl`` by fp32
    rounding, which moves ``1 / rho0`` and ``1 / r`` by parts in 1e7: no term.

    Cells ON a wall of the bounding square carry zero cotangents here.  On a TX grid such a cell is a transmitter on the wall: the
    segment that reaches its bounce has a length of rounding noise and its fp32 direction -- the definition's ``u_in`` -- is noise
    too, while the path itself appears and vanishes as the cell crosses the wall: the response is not differentiable there
    (``tests/test_field_position_vjp_cpu.py`` leaves the same cells out)."""
    amp = AMPS[amplitude]
    walls, fixed, X, Y = _case(scene)
    cands, T, Rl, S, p0 = segment_case(scene, role)
    nf = 9
    inv = inv_list(nf)
    rb, ib = bars(nf, X.shape, 131)
    inside = (X > 0) & (X < 1) & (Y > 0) & (Y < 1)
    assert inside.mean() > 0.6
    rb, ib = rb * inside, ib * inside  # (a cell ON a wall of the bounding square: see the docstring)
    ph = WO.physics(cands, T, Rl, S, walls, p0, "received_power", HEIGHT, inv, rb, ib, amp)
    WO.guards(cands, T, ph)
    wb = WO.walls_bar_of(ph.normal_bar, walls)
    grid = np.stack([X.reshape(-1), Y.reshape(-1)], axis=1).astype(np.float64)
    fx = np.asarray(fixed, np.float64)
    tx0, rx0 = (fx, grid) if role == "rx" else (grid, fx)
    w64 = np.asarray(walls, np.float64)
    h = H_STEP
    kappa = 2 * np.pi * float(inv.max())
    bsum = (np.abs(rb) + np.abs(ib)).reshape(nf, -1).astype(np.float64).sum(axis=0)
    qabs = max(float(np.abs(w64).max()), float(np.abs(grid).max()), float(np.abs(fx).max()))
    worst, compared = 0.0, 0
    for w in range(len(walls)):
        sel = [ci for ci, c in enumerate(cands) if w in [int(x) for x in c]]
        sub = [cands[ci] for ci in sel]
        Tw, Rw, Sw = T[sel], Rl[sel], S[sel]
        Lw = float(np.hypot(*(w64[w, 1] - w64[w, 0])))
        tol = 0.0
        for cand, t, r, s in zip(sub, Tw, Rw, Sw):
            nz = ~(t == 0)
            if not nz.any():
                continue
            K = len(cand)
            r64 = np.where(nz, r.astype(np.float64), 1.0)
            a = np.abs(np.where(nz, t.astype(np.float64), 0.0))
            A = (np.sqrt(a) if amp == AMP_SQRT else a) * bsum
            lam = kappa + 3.0 / np.sqrt(HEIGHT * HEIGHT + r64 * r64)
            kap = 1.0 / Lw + 1.0 / r64
            hits = sum(1 for x in cand if int(x) == w)
            tol += hits * ((h * h / 6.0) * (A * (2 * lam + 8 * kap) ** 3).sum() + nf * 2.0**-52 * A.sum() / (2 * h)
                           + (40 + 3 * K * qabs / Lw) * 2.0**-24 * (A * lam).sum())
        assert np.isfinite(tol)
        for e in range(2):
            for d in range(2):
                def loss(sign):
                    moved = w64.copy()
                    moved[w, e, d] += sign * h
                    H = PO.forward(WO.displaced(moved, w64), sub, Tw, Rw, "received_power", HEIGHT, 0.5, inv, amp, tx0, rx0, tx0, rx0)
                    return _loss_cells(H, rb, ib)
                fd = ((loss(+1) - loss(-1)) / (2 * h)).sum() if sub else 0.0
                err = abs(fd - wb[w, e, d])
                if ph.scale[w] > 0:
                    worst = max(worst, err / tol)
                    compared += 1
                    assert tol <= 1e-4 * ph.scale[w], (w, tol / ph.scale[w])  # the tolerance binds
                assert err <= tol, (w, e, d, fd, wb[w, e, d], err / tol if tol else np.inf)
    touched = ph.scale > 0
    assert compared == 4 * touched.sum() >= 8 and np.abs(wb[touched]).max(axis=(1, 2)).all()
    print(f"central differences, {scene}, {role} grid, {amplitude}: {touched.sum()} touched walls, worst error / tolerance = {worst:.3g}")


# ---- 3. the incoherent limit against torch autodiff of the reference's own chain ---------------------------------------------------------
@pytest.mark.parametrize("scene", ["obstacle", "random7"])
def test_incoherent_limit_is_the_walls_bar_of_the_reference_chain(scene):
    """LINEAR, one entry ``inv = 0``, ``re_bar = 1``, ``im_bar = 0``: ``re`` is the power map, so ``walls_bar`` is the gradient of its
    sum over the cells with respect to the walls -- ``oracle.ref.power_map_value_and_grads(..., dtype="float64")["walls_bar"]`` (hard,
    orders 0-2), torch autodiff of the reference's own chain and independent of the closed form.  K3-X's rule for the same comparison:
    within 1e-5 of the summed term magnitude, every entry finite."""
    from oracle import ref as R

    walls, fixed, X, Y = _case(scene)
    cands, T, Rl, S, p0 = segment_case(scene, "rx")
    ones, zeros = np.ones((1,) + X.shape, F), np.zeros((1,) + X.shape, F)
    ph = WO.physics(cands, T, Rl, S, walls, p0, "received_power", HEIGHT, [0.0], ones, zeros, AMP_LINEAR)
    want = R.power_map_value_and_grads(walls, fixed, X, Y, dtype="float64", min_order=0, max_order=2, approx=False, fun="received_power",
                                       fun_kwargs=dict(r_coef=0.5, height=HEIGHT))["walls_bar"]
    got = WO.walls_bar_of(ph.normal_bar, walls)
    assert want.shape == got.shape == (len(walls), 2, 2) and np.isfinite(want).all() and np.isfinite(got).all()
    mag = ph.mag.sum(axis=1)  # the wall's summed term magnitude, both ends
    touched = mag > 0
    err = np.abs(got - want).max(axis=(1, 2))
    print(f"{scene}: worst |walls_bar - autodiff| / magnitude = {(err[touched] / mag[touched]).max():.3g} over {touched.sum()} of {touched.size} walls")
    assert touched.sum() >= 3 and (err[touched] <= 1e-5 * mag[touched]).all(), float((err[touched] / mag[touched]).max())
    assert (np.abs(want[~touched]) <= 1e-5 * mag.max()).all()  # a wall without a bounce has no gradient either


# ---- 4. rules and guards -----------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_oracle_rules():
    """On the restatement: zero cotangents give ``+0.0`` in every entry, doubled cotangents exactly doubled entries, an appended
    wavelength with zero cotangents changes no bit (a new block, and one that crosses a block edge), walls that no contributing
    candidate touches are exactly ``+0.0``, order 0 alone gives all zeros, a NaN contribution reaches its candidate's walls and no
    others -- and the restatement lies within the bound of the float64 evaluation."""
    walls = _case("obstacle")[0]
    cands, T, Rl, S, p0 = segment_case("obstacle", "rx")
    cells = T.shape[1]
    args = (cands, T, Rl, S, walls, p0, "received_power", HEIGHT)
    for nf in (8, 16):
        inv = inv_list(nf + 1)
        rb, ib = bars(nf + 1, (cells,), 141)
        rb[nf] = ib[nf] = 0
        for amp in (AMP_SQRT, AMP_LINEAR):
            short = WO.restate(*args, inv[:nf], rb[:nf], ib[:nf], amp)
            more = WO.restate(*args, inv, rb, ib, amp)
            twice = WO.restate(*args, inv[:nf], 2 * rb[:nf], 2 * ib[:nf], amp)
            zero = WO.restate(*args, inv[:nf], 0 * rb[:nf], F(-0.0) * ib[:nf], amp)
            assert short.any() and np.array_equal(_bits(short), _bits(more))
            assert np.array_equal(_bits(2.0 * short), _bits(twice))
            assert not _bits(zero).any()
            ph = WO.physics(*args, inv[:nf], rb[:nf], ib[:nf], amp)
            WO.guards(cands, T, ph)
            assert (np.abs(short - ph.normal_bar) <= ph.bound).all(), float((np.abs(short - ph.normal_bar) / np.maximum(ph.bound, 1e-300)).max())
            assert not _bits(short[ph.scale == 0]).any()
    inv = inv_list(3)
    rb, ib = bars(3, (cells,), 142)
    los = [ci for ci, c in enumerate(cands) if len(c) == 0]
    assert len(los) == 1 and (~(T[los[0]] == 0)).any()
    only0 = WO.restate([cands[los[0]]], T[los], Rl[los], S[los], walls, p0, "received_power", HEIGHT, inv, rb, ib, AMP_SQRT)
    assert not _bits(only0).any()
    # a NaN contribution of one candidate in one cell
    ci = next(ci for ci, c in enumerate(cands) if len(c) == 2 and (~(T[ci] == 0)).any())
    cell = int(np.flatnonzero(~(T[ci] == 0))[0])
    Tn = T.copy()
    Tn[ci, cell] = np.nan
    clean = WO.restate(*args, inv, rb, ib, AMP_LINEAR)
    dirty = WO.restate(cands, Tn, Rl, S, walls, p0, "received_power", HEIGHT, inv, rb, ib, AMP_LINEAR)
    hit = np.zeros(len(walls), bool)
    hit[[int(x) for x in cands[ci]]] = True
    assert np.isnan(dirty[hit]).all() and np.array_equal(_bits(dirty[~hit]), _bits(clean[~hit])) and np.isfinite(clean).all()


GPU_CASES = [("obstacle", None, 2), ("random7", None, 2), ("random7", (13, 19), 2), ("obstacle", None, 3)]


@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("scene,grid,hi", GPU_CASES)
def test_oracle_guards_on_the_gpu_tests_inputs(scene, grid, hi, role):
    """The comparisons of ``tests/test_gpu_field_walls_vjp.py`` do not pass on empty ground: contributions of every order, a bound that
    is small against the scale on every touched wall, and at order 3 (``obstacle``: the square's facing walls) a contributing candidate that visits a wall twice, ``(0, 2, 0)``."""
    walls = _case(scene)[0]
    cands, T, Rl, S, p0 = segment_case(scene, role, hi=hi, grid=grid)
    nf = 9
    rb, ib = bars(nf, (T.shape[1],), 143)
    ph = WO.physics(cands, T, Rl, S, walls, p0, "received_power", HEIGHT, inv_list(nf), rb, ib, AMP_SQRT)
    orders = {len(c) for ci, c in enumerate(cands) if (~(T[ci] == 0)).any()}
    assert orders == set(range(hi + 1)), orders
    WO.guards(cands, T, ph, max_order=hi, need_twice=hi == 3)
    print(f"{scene} {grid} {role} orders 0-{hi}: {int((ph.scale > 0).sum())} touched walls, worst bound / scale = "
          f"{(ph.bound[ph.scale > 0] / ph.scale[ph.scale > 0, None]).max():.2e}")


def test_bindings_and_abi_version():
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import Context, WallGradient
    from differt2d_amd.scene import Scene

    assert L.D2D_ABI_VERSION == 12 and L.D2D_POS_CHUNK == WO.POS_CHUNK == 8
    names = [s[0] for s in L.SYMBOLS]
    for name in ("d2d_field_walls_vjp_launch", "d2d_get_field_walls_vjp", "d2d_selftest_wallgrad"):
        assert name in names
    assert callable(Context.field_walls_vjp) and callable(Context.launch_field_walls_vjp) and callable(Context.get_field_walls_vjp)
    assert callable(Scene.frequency_response_walls_vjp_on_receivers_grid) and callable(Scene.frequency_response_walls_vjp_on_transmitters_grid)
    assert WallGradient._fields == ("walls_bar", "normal_bar")
    header = open(os.path.join(ROOT, "include", "d2d.h")).read()
    assert "#define D2D_ABI_VERSION 12" in header
    for decl in ("int d2d_field_walls_vjp_launch(", "int d2d_get_field_walls_vjp(", "int d2d_selftest_wallgrad("):
        assert decl in header
    lib = L.load()  # (the library exports them: getattr raises otherwise)
    assert lib.d2d_field_walls_vjp_launch and lib.d2d_get_field_walls_vjp and lib.d2d_selftest_wallgrad and lib.d2d_abi_version() == 12


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
    for method in (scene.frequency_response_walls_vjp_on_receivers_grid, scene.frequency_response_walls_vjp_on_transmitters_grid):
        with pytest.raises(ValueError, match="exactly one of wavelengths= and inv_wavelengths="):
            method(X, Y, received_power, None, rb, ib, approx=False)
        with pytest.raises(ValueError, match="exactly one of wavelengths= and inv_wavelengths="):
            method(X, Y, received_power, None, rb, ib, wavelengths=[0.05, 0.06], inv_wavelengths=[20, 21], approx=False)
        with pytest.raises(L.D2DUnsupported, match="is not fused natively: the wall adjoint needs the path function's derivative"):
            method(X, Y, lambda path: 1.0, None, rb, ib, wavelengths=[0.05, 0.06], approx=False)
        with pytest.raises(L.D2DUnsupported, match="the wall adjoint covers ImagePath only, not path_cls=MinPath"):
            method(X, Y, received_power, None, rb, ib, wavelengths=[0.05, 0.06], path_cls=MinPath, approx=False)
        for kw in (dict(approx=True), dict(approx=True, function="sigmoid")):
            with pytest.raises(L.D2DUnsupported, match="hard validity only .approx=False.: a smoothed validity depends on the walls' end points itself"):
                method(X, Y, received_power, None, rb, ib, wavelengths=[0.05, 0.06], **kw)


def _definition(text):
    """The definition block of K3-V ``d2d::WallGradSink`` in a document: from the line that names the arguments to the line about NaN
    contributions, with comment prefixes, Markdown's code fences and all white space taken out."""
    lines = text.splitlines()
    first = next(i for i, line in enumerate(lines) if "The arguments of the wall adjoint are exactly those of `d2d_field_position_vjp_launch`" in line)
    last = next(i for i in range(first, len(lines)) if "makes the entries of that candidate's walls NaN and no others." in lines[i])
    block = [re.sub(r"^\s*\*( |$)", "", line) for line in lines[first:last + 1] if line.strip() != "```"]
    return re.sub(r"\s+", "", "\n".join(block))


def test_definition_reads_the_same_in_the_header_the_design_and_the_readme():
    docs = {name: open(os.path.join(ROOT, *name.split("/"))).read() for name in ("include/d2d.h", "DESIGN.md", "README.md")}
    for name, text in docs.items():
        assert "K3-V `d2d::WallGradSink`" in text, name
    blocks = {name: _definition(text) for name, text in docs.items()}
    want = blocks["include/d2d.h"]
    assert len(want) > 2000 and "wa=G*gam;Wb=wa*s;Wa=wa−Wb" in want and "gam=2.0f*steer_dot(ux,uy,nx,ny)" in want
    assert "if(ok){row[w][0]+=Wa;row[w][1]+=Wb}" in want and "D2D_POS_CHUNK=8" in want
    for name, got in blocks.items():
        assert got == want, name
    # the header's own text states the same arithmetic
    hpp = open(os.path.join(ROOT, "differt2d_amd", "csrc", "d2d_wallgrad.hpp")).read()
    assert "wa  = G * gam ; Wb = wa * s ; Wa = wa - Wb" in hpp and "gam = 2.0f * steer_dot(ux, uy, nx, ny)" in hpp


# ---- 5. the wall-fitting loop on the float64 oracle --------------------------------------------------------------------------------------
# The face of `obstacle`'s inner square that looks at the transmitter (wall 4) is displaced along its normal by 0.001, into the
# obstacle: 0.02 wavelengths (a fifth of 0.1 lambda, 0.25 rad of phase per bounce: inside the misfit's basin).  On that side the
# visibility of every cell is the truth's; on the other side the face leaves gaps at the obstacle's corners and the misfit jumps
# (17 at 0.0005 against 0.36 on this side), so the rate stays where the descent does not cross: the misfit is 1.4e6 d^2 along the
# shift d, a curvature of 2.8e6, and the rate is 1.1 / curvature.  The far end point carries a third of the gradient and converges
# last: 40 steps.
FIT = dict(scene="obstacle", nf=8, wall=4, shift=-0.001, steps=40, rate=4e-7)


def fitting_inputs():
    walls, fixed, X, Y = _case(FIT["scene"])
    truth = np.array(walls, F).copy()
    n = WO.wall_table(truth)[1][FIT["wall"]]
    start = truth.copy()
    start[FIT["wall"]] = (truth[FIT["wall"]].astype(np.float64) + FIT["shift"] * n.astype(np.float64)[None, :]).astype(F)
    return truth, start, fixed, X, Y, inv_list(FIT["nf"])


def oracle_fitting_loop():
    """``(losses, walls)``: fixed-rate descent of ``utils.field_misfit`` on the end points of the displaced wall with the float64
    oracle's ``walls_bar``; the forward model (contributions, lengths, segments: the oracle's own visibility) is recomputed at every
    step on the current fp32 walls."""
    from differt2d_amd.engine import FrequencyResponse
    from differt2d_amd.utils import field_misfit

    truth, walls, fixed, X, Y, inv = fitting_inputs()
    nf = inv.size
    kw = fun_kw("received_power")

    def response(w):
        cands, T, Rl, S = WO.segment_contributions(w, fixed, X, Y, min_order=0, max_order=2, grid_role="rx", fun=kw["fun"],
                                                   fun_kwargs=kw["fun_kwargs"], **MODES["hard"])
        u = Rl.astype(np.float64)[None] * inv.astype(np.float64)[:, None, None]
        H = (np.where(T == 0, 0.0, T.astype(np.float64))[None] * np.exp(-2j * np.pi * u)).sum(axis=1)
        return (cands, T, Rl, S), H.reshape((nf,) + X.shape)

    def as_fr(H):
        return FrequencyResponse(H.real.astype(F), H.imag.astype(F), np.zeros(X.shape, F))

    _, target = response(truth)
    p0 = WO.first_point(fixed, X, Y, "rx")
    losses = []
    for _ in range(FIT["steps"]):
        geo, H = response(walls)
        loss, rb, ib = field_misfit(as_fr(H), target)
        losses.append(loss)
        ph = WO.physics(*geo, walls, p0, "received_power", HEIGHT, inv, rb, ib, AMP_LINEAR)
        step = FIT["rate"] * WO.walls_bar_of(ph.normal_bar, walls)[FIT["wall"]]
        walls = walls.copy()
        walls[FIT["wall"]] = (walls[FIT["wall"]].astype(np.float64) - step).astype(F)
    losses.append(field_misfit(as_fr(response(walls)[1]), target)[0])
    return losses, walls


ORACLE_RATIO = 5.4e-6  # final / initial misfit the float64 loop reached (5.32e-6), rounded up; the GPU test asserts 10 x this for fp32


def test_wall_fitting_loop_on_the_float64_oracle():
    """The misfit falls at every step and ends below ``ORACLE_RATIO`` of its start; the wall is back within a hundredth of the
    displacement."""
    losses, walls = oracle_fitting_loop()
    truth = fitting_inputs()[0]
    print("misfit:", " ".join(f"{v:.4g}" for v in losses), "ratio", losses[-1] / losses[0], "wall", walls[FIT["wall"]].tolist())
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    assert losses[-1] <= ORACLE_RATIO * losses[0], losses[-1] / losses[0]
    assert np.abs(walls[FIT["wall"]] - truth[FIT["wall"]]).max() <= 0.01 * abs(FIT["shift"]) + 2.0**-23
