"""Host side of the material response's permittivity adjoint (no GPU): ``d2d_fresnel_grad.hpp``'s arithmetic and the host's memory
rule through a stand-alone g++ program (plain and with sanitizers; nothing of it is loaded into Python), the header against the NumPy
restatement of ``tests/material_eps_vjp_oracle.py`` bit for bit and against float64 in accuracy, the oracle against central
differences of its own float64 forward, its guards on the inputs the GPU tests use, ``utils.material_parameters_vjp``, the bindings,
the definition block in the three documents and the ``Scene`` methods' refusals."""

import os
import re
import subprocess

import numpy as np
import pytest

import material_eps_vjp_oracle as EO
import material_response_oracle as MO
from conftest import unit_grid
from test_gpu_strongest_paths import _case

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "material_eps_vjp_host.cpp")
GXX = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
U = 2.0**-24


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """tests/native/material_eps_vjp_host.cpp as a program of its own, plain and with sanitizers (linked against their run times by
    the compiler: nothing is preloaded)."""
    d = tmp_path_factory.mktemp("material_eps_vjp_host")
    out = {}
    for name, extra in (("plain", []), ("asan_ubsan", SANITIZE)):
        out[name] = str(d / f"material_eps_vjp_host_{name}")
        subprocess.check_call(GXX + extra + ["-o", out[name], SRC])
    return out


def run_header(exe, tmp_path, er, ei, c):
    """``[2 (TE, TM), 5 (gr, gi, dr, di, ok), n]`` of the header's g++ build over a list."""
    n = er.size
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(np.int64(n).tobytes())
        for a in (er, ei, c):
            f.write(np.ascontiguousarray(a, F).tobytes())
    subprocess.run([exe, inp, outp], check=True, timeout=300)
    out = np.fromfile(outp, F)
    assert out.size == 10 * n
    return out.reshape(2, 5, n)


# ---- the stand-alone program ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", ["plain", "asan_ubsan"])
def test_stand_alone_host_program(programs, build):
    """The header's stated values, ok false at m == 0 and den == 0, the memory rule at its boundary byte and with sizes that would
    wrap, the chunk plan."""
    done = subprocess.run([programs[build]], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(done.stdout)
    assert done.returncode == 0, done.stdout
    assert "material_eps_vjp_host: chunk 8, 0 failures" in done.stdout


@pytest.mark.parametrize("build", ["plain", "asan_ubsan"])
def test_header_equals_fresnel_and_the_numpy_restatement_by_bits(programs, tmp_path, build):
    """Over the forward header's input list: (gr, gi) are fresnel's bits everywhere, (dr, di) and ok the restatement's (NaN
    results compare as NaN); finite inputs, components of 2^50 included, give a finite derivative; both special cases occur."""
    er, ei, c = MO.fresnel_inputs()
    got = run_header(programs[build], tmp_path, er, ei, c)
    assert er.size > 60000
    finite = np.isfinite(er) & np.isfinite(ei) & np.isfinite(c)
    for k, pol in enumerate((MO.POL_TE, MO.POL_TM)):
        gr, gi = MO.fresnel(er, ei, c, pol)
        assert MO.same_bits(got[k, 0], gr).all() and MO.same_bits(got[k, 1], gi).all()
        want = EO.fresnel_grad(er, ei, c, pol)
        for name, g, w in zip(("gr", "gi", "dr", "di"), got[k, :4], want[:4]):
            ok = MO.same_bits(g, w)
            assert ok.all(), (pol, name, int((~ok).sum()), int(np.flatnonzero(~ok)[0]))
        assert np.array_equal(got[k, 4] != 0, want[4])
        off = ~want[4]
        assert off.any() and not got[k, 2][off].view(np.uint32).any() and not got[k, 3][off].view(np.uint32).any()  # (+0, +0)
        assert (off & (got[k, 0] == -1)).any()  # den == 0 ...
        assert pol == MO.POL_TM or (off & (got[k, 0] == 1)).any()  # ... and m == 0 alone (eps = 0 at c = 1: TE's a + q is 1, TM's 0)
        assert np.isfinite(got[k, 2][finite]).all() and np.isfinite(got[k, 3][finite]).all()
        nan_c = np.isnan(c) & np.isfinite(er) & np.isfinite(ei)
        assert nan_c.any() and np.isnan(got[k, 2][nan_c]).all() and (got[k, 4][nan_c] != 0).all()  # a NaN c propagates, ok true


def test_header_accuracy_against_float64(programs, tmp_path):
    """The g++ build of the header against the float64 formula on the forward header's domain, eps' in [1.5, 100], eps'' in [0, 1000],
    cos in [1e-3, 1], 2^20 seeded points: |d32 - d64| / |d64| measured 13.28 * 2^-24 (TE 13.28, TM 11.95; printed), asserted below
    DFRESNEL_BOUND = 14.0 (the maximum plus 5 %, rounded up to a multiple of 0.25)."""
    rng = np.random.default_rng(20261022)
    n = 1 << 20
    er = rng.uniform(1.5, 100, n).astype(F)
    ei = (-rng.uniform(0, 1000, n)).astype(F)
    ei[: n // 4] = (-rng.uniform(0, 1, n // 4)).astype(F)  # weakly lossy too
    c = rng.uniform(1e-3, 1, n).astype(F)
    got = run_header(programs["plain"], tmp_path, er, ei, c)
    worst = 0.0
    for k, pol in enumerate((MO.POL_TE, MO.POL_TM)):
        _, d = EO.dfresnel64(er.astype(np.float64) + 1j * ei.astype(np.float64), c.astype(np.float64), pol)
        d32 = got[k, 2].astype(np.float64) + 1j * got[k, 3].astype(np.float64)
        err = float((np.abs(d32 - d) / np.abs(d)).max() / U)
        print(f"fresnel_grad vs float64, pol {pol}: max |d32 - d64| / |d64| = {err:.3f} * 2^-24")
        assert (got[k, 4] != 0).all()
        worst = max(worst, err)
    assert worst < EO.DFRESNEL_BOUND
    assert EO.DFRESNEL_BOUND == 14.0 == np.ceil(13.28 * 1.05 / 0.25) * 0.25
    text = open(os.path.join(ROOT, "differt2d_amd", "csrc", "d2d_fresnel_grad.hpp")).read()
    assert "DFRESNEL_BOUND = 14.0 * 2^-24" in text and "measured maximum 13.28 * 2^-24" in text


def test_analytic_derivative_is_the_derivative_of_the_float64_coefficient():
    """dfresnel64's d against a central difference of utils.fresnel_coefficient in eps, along the real and the imaginary axis (G is
    holomorphic: both give the same complex number)."""
    rng = np.random.default_rng(5)
    eps = rng.uniform(2, 9, 4096) - 1j * rng.uniform(0, 3, 4096)
    c = rng.uniform(0.02, 1, 4096)
    h = 1e-6
    for pol in (MO.POL_TE, MO.POL_TM):
        _, d = EO.dfresnel64(eps, c, pol)
        for step in (h, 1j * h):
            fd = (EO.dfresnel64(eps + step, c, pol)[0] - EO.dfresnel64(eps - step, c, pol)[0]) / (2 * step)
            assert np.abs(fd - d).max() < 1e-8 * max(1.0, np.abs(d).max())


# ---- the oracle against itself -------------------------------------------------------------------------------------------------------
def eps_table(nf, N, seed=7):
    """Lossy, different per wall and row: eps in [2, 9] - j [0, 3] (complex64, the kernel's table)."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(2, 9, (nf, N)) - 1j * rng.uniform(0, 3, (nf, N))).astype(np.complex64)


@pytest.fixture(scope="module")
def random7():
    walls, fixed, X, Y = _case("random7")
    con = MO.segment_contributions(walls, fixed, X, Y, min_order=0, max_order=2, approx=False)
    return walls, con, MO.wall_normals(walls), X.shape


@pytest.mark.parametrize("amp", [EO.AMP_SQRT, EO.AMP_LINEAR])
@pytest.mark.parametrize("pol", [MO.POL_TE, MO.POL_TM])
def test_oracle_is_the_gradient_of_its_own_forward(random7, pol, amp):
    """<eps_bar, delta> against the central difference of L(eps +- h delta) of the oracle's float64 forward, h = 1e-6, random complex
    delta: within 1e-6 * sum mag |delta| (q is bounded away from 0 on these inputs: the truncation is O(h^2), the rounding 1e-16 / h).
    The guards hold on these inputs: the oracle alone stays inside the cap."""
    walls, con, normals, shape = random7
    N, nf = len(walls), 3
    inv = (F(20) * (F(1) + np.arange(nf, dtype=F) / F(64))).astype(F)
    eps = eps_table(nf, N)
    rng = np.random.default_rng(100 + 2 * pol + amp)
    rb, ib = rng.standard_normal((nf,) + shape).astype(F), rng.standard_normal((nf,) + shape).astype(F)
    eg = EO.eps_grad(*con, normals, inv, eps, rb, ib, pol, amp)
    EO.guards(eg)
    print(f"pol {pol} amp {amp}: max bound / mag {(eg.bound[eg.mag > 0] / eg.mag[eg.mag > 0]).max():.2e} (cap {2.0**-12:.2e}), terms {eg.n_terms.sum()}")
    delta = rng.standard_normal((nf, N)) + 1j * rng.standard_normal((nf, N))
    h = 1e-6
    e64 = eps.astype(np.complex128)
    up = EO.loss(EO.forward(*con, normals, inv, e64 + h * delta, pol, amp), rb, ib)
    dn = EO.loss(EO.forward(*con, normals, inv, e64 - h * delta, pol, amp), rb, ib)
    fd = (up - dn) / (2 * h)
    inner = float((eg.eps_bar.real * delta.real + eg.eps_bar.imag * delta.imag).sum())
    tol = 1e-6 * float((eg.mag * np.abs(delta)).sum())
    print(f"  <eps_bar, delta> {inner:.9e}, central difference {fd:.9e}, |difference| / tolerance {abs(inner - fd) / tol:.3f}")
    assert abs(inner - fd) <= tol and abs(inner) > 100 * tol
    # the oracle's forward is the forward oracle's, up to fp32 rounding of the latter
    mr = MO.material_response(walls, None, np.zeros(shape), None, inv, eps, pol, amp, contributions=con)
    H = EO.forward(*con, normals, inv, e64, pol, amp).reshape((nf,) + shape)
    assert np.abs(H.real - mr.re).max() < 1e-4 * np.abs(H).max() and np.abs(H.imag - mr.im).max() < 1e-4 * np.abs(H).max()


def test_oracle_rules(random7):
    """A wall occurring twice gets both terms (order 2: (a, b) with a != b only, so the square at order 3 is the GPU test's);
    row f depends on row f alone; the constant band equals equal rows; the line of sight adds nothing."""
    walls, con, normals, shape = random7
    N, nf = len(walls), 3
    inv = np.array([20.0, 21.5, 20.0], F)
    eps = eps_table(nf, N)
    rng = np.random.default_rng(9)
    rb, ib = rng.standard_normal((nf,) + shape).astype(F), rng.standard_normal((nf,) + shape).astype(F)
    eg = EO.eps_grad(*con, normals, inv, eps, rb, ib, MO.POL_TE, EO.AMP_SQRT)
    perm = [2, 0, 1]
    p = EO.eps_grad(*con, normals, inv[perm], eps[perm], rb[perm], ib[perm], MO.POL_TE, EO.AMP_SQRT)
    assert np.array_equal(p.eps_bar, eg.eps_bar[perm])
    one = EO.eps_grad(*con, normals, inv[1:2], eps[1:2], rb[1:2], ib[1:2], MO.POL_TE, EO.AMP_SQRT)
    assert np.array_equal(one.eps_bar[0], eg.eps_bar[1])
    band = EO.eps_grad(*con, normals, inv, eps[0], rb, ib, MO.POL_TE, EO.AMP_SQRT)
    rows = EO.eps_grad(*con, normals, inv, np.broadcast_to(eps[0], (nf, N)), rb, ib, MO.POL_TE, EO.AMP_SQRT)
    assert np.array_equal(band.eps_bar, rows.eps_bar) and band.eps_bar.shape == (nf, N)
    cands, T, Rl, S = con
    los = [k for k, cand in enumerate(cands) if len(cand) == 0]
    only = EO.eps_grad([cands[k] for k in los], T[los], Rl[los], S[los], normals, inv, eps, rb, ib, MO.POL_TE, EO.AMP_SQRT)
    assert los and not only.eps_bar.any() and not only.mag.any()
    tm = EO.eps_grad(*con, normals, inv, eps, rb, ib, MO.POL_TM, EO.AMP_SQRT)
    assert not np.allclose(tm.eps_bar, eg.eps_bar)


# ---- utils.material_parameters_vjp ---------------------------------------------------------------------------------------------------
def test_material_parameters_vjp_against_a_finite_difference():
    from differt2d_amd import utils

    rng = np.random.default_rng(4)
    nf, N = 5, 6
    freq = np.linspace(2.0e9, 3.0e9, nf)
    eps_r, sigma = rng.uniform(2, 9, N), rng.uniform(0.01, 0.3, N)
    eps_bar = rng.standard_normal((nf, N)) + 1j * rng.standard_normal((nf, N))

    def L(er, sg):  # a loss whose gradient with respect to eps is eps_bar: linear in (Re eps, Im eps)
        e = utils.complex_permittivity(er[None, :], sg[None, :], freq[:, None])
        return float((eps_bar.real * e.real + eps_bar.imag * e.imag).sum())

    er_bar, sg_bar = utils.material_parameters_vjp(eps_bar, freq)
    assert er_bar.shape == sg_bar.shape == (N,) and er_bar.dtype == sg_bar.dtype == np.float64
    for k in range(N):
        d = np.zeros(N)
        d[k] = 1.0
        assert np.isclose((L(eps_r + 1e-3 * d, sigma) - L(eps_r - 1e-3 * d, sigma)) / 2e-3, er_bar[k], rtol=1e-9)
        assert np.isclose((L(eps_r, sigma + 1e-4 * d) - L(eps_r, sigma - 1e-4 * d)) / 2e-4, sg_bar[k], rtol=1e-9)
    assert np.allclose(er_bar, eps_bar.real.sum(axis=0))
    assert np.allclose(sg_bar, (-eps_bar.imag / (2 * np.pi * freq[:, None] * utils.VACUUM_PERMITTIVITY)).sum(axis=0))
    with pytest.raises(ValueError, match="row per frequency"):
        utils.material_parameters_vjp(eps_bar[0], freq)
    with pytest.raises(ValueError, match="row per frequency"):
        utils.material_parameters_vjp(eps_bar, freq[:3])


# ---- bindings, documents and refusals ------------------------------------------------------------------------------------------------
def _definition_block(text):
    """The lines from ``eps_bar[f][w] = (+0.0, +0.0)`` to the line that adds to ``.im``, without the comment leader and the
    indentation that the three documents differ in."""
    lines = text.splitlines()
    starts = [k for k, ln in enumerate(lines) if "eps_bar[f][w] = (+0.0, +0.0) for all f, w" in ln]
    assert len(starts) == 1, len(starts)
    out = []
    for ln in lines[starts[0]:]:
        out.append(re.sub(r"\s+", " ", re.sub(r"^\s*\*?\s*", "", ln)).strip())
        if "eps_bar[f][cand[i]].im +=" in ln:
            return out
    raise AssertionError("the block has no end")


def test_bindings_abi_version_and_the_definition_in_three_documents():
    from differt2d_amd import _lib as L
    from differt2d_amd import utils
    from differt2d_amd.engine import Context
    from differt2d_amd.scene import Scene

    assert L.D2D_ABI_VERSION == 12
    names = [s[0] for s in L.SYMBOLS]
    assert all(n in names for n in ("d2d_material_eps_vjp_launch", "d2d_get_material_eps_vjp", "d2d_selftest_fresnel_grad"))
    for name in ("material_eps_vjp", "launch_material_eps_vjp", "get_material_eps_vjp", "selftest_fresnel_grad"):
        assert callable(getattr(Context, name))
    assert callable(Scene.material_response_permittivity_vjp_on_receivers_grid)
    assert callable(Scene.material_response_permittivity_vjp_on_transmitters_grid)
    assert callable(utils.material_parameters_vjp)
    header = open(os.path.join(ROOT, "include", "d2d.h")).read()
    assert "#define D2D_ABI_VERSION 12" in header
    for name in ("int d2d_material_eps_vjp_launch(", "int d2d_get_material_eps_vjp(", "int d2d_selftest_fresnel_grad("):
        assert name in header
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    block = _definition_block(header)
    assert len(block) == 15 and block == _definition_block(design) == _definition_block(readme)
    assert "K3-E" in design and "Calibrating materials" in readme
    for text in (header, readme):
        assert "no gradients with respect to eps or the geometry" not in text and "gradients with respect to `ε` or the geometry" not in text
        assert "gradients with respect to the geometry" in text
    # the derivative's header states the operations that the ABI header names it for
    grad = open(os.path.join(ROOT, "differt2d_amd", "csrc", "d2d_fresnel_grad.hpp")).read()
    assert "TM: t = (er - 2) + (cc + cc)" in grad and "ok = !(m == 0) && !(den == 0)" in grad
    lib = L.load()
    assert lib.d2d_material_eps_vjp_launch and lib.d2d_get_material_eps_vjp and lib.d2d_selftest_fresnel_grad and lib.d2d_abi_version() == 12


def test_scene_refusals_without_a_launch():
    from differt2d_amd import _lib as L
    from differt2d_amd.scene import Scene
    from differt2d_amd.utils import received_power

    scene = Scene.square_scene_with_obstacle()
    n = len(scene.objects)
    X, Y = unit_grid(4, 3)
    rb = ib = np.zeros((2, 4, 3), F)

    def step(tx, rx, path, objs):
        return (path.length() < 1.0).astype(F)

    for method in (scene.material_response_permittivity_vjp_on_receivers_grid, scene.material_response_permittivity_vjp_on_transmitters_grid):
        with pytest.raises(L.D2DUnsupported, match="valid_paths") as e:
            next(iter(method(X, Y, step, None, rb, ib, wavelengths=[0.05, 0.06], permittivity=np.full(n, 4 - 1j))))
        assert "trace_paths" in str(e.value) and "material response" in str(e.value)
        with pytest.raises(ValueError, match="exactly one"):
            method(X, Y, received_power, None, rb, ib, permittivity=np.full(n, 4 - 1j))
        with pytest.raises(ValueError, match="exactly one"):
            method(X, Y, received_power, None, rb, ib, wavelengths=[0.05], inv_wavelengths=[20.0])
        with pytest.raises(ValueError, match="object 0 .*no permittivity"):
            next(iter(method(X, Y, received_power, None, rb, ib, wavelengths=[0.05, 0.06])))
        with pytest.raises(ValueError, match=rf"\[{n}\]"):
            next(iter(method(X, Y, received_power, None, rb, ib, wavelengths=[0.05, 0.06], permittivity=np.ones((3, n)))))
        from differt2d_amd.geometry import MinPath

        with pytest.raises(L.D2DUnsupported, match="ImagePath only"):
            method(X, Y, received_power, None, rb, ib, wavelengths=[0.05, 0.06], permittivity=np.full(n, 4 - 1j), path_cls=MinPath)


def test_oracle_guards_hold_on_the_gpu_tests_inputs():
    """Every case of tests/test_gpu_material_eps_vjp.py: at least three walls carry terms at every wavelength and the oracle's own
    bound stays below 2^-12 of the terms' magnitude, so the GPU comparisons stand on ground that can fail (checked here, without a GPU)."""
    import itertools

    import test_gpu_material_eps_vjp as T

    worst = 0.0
    for scene, mode, role, pol, amp, nf in itertools.product(("obstacle", "random7"), ("hard", "hsig"), ("rx", "tx"), ("te", "tm"), ("sqrt", "linear"),
                                                             (1, 8, 9, 17)):
        eg = T._oracle(scene, mode, role, pol, amp, nf)  # (asserts the guards)
        lit = eg.mag > 0
        worst = max(worst, float((eg.bound[lit] / eg.mag[lit]).max()))
    for mode, role, pol in itertools.product(("hard", "hsig"), ("rx", "tx"), ("te", "tm")):
        T._oracle("random7_13x19", mode, role, pol, "sqrt", 9)
        T._oracle("square_centre", mode, role, pol, "linear", 9, 0, 3)  # (... and that a candidate (a, b, a) contributes)
    print(f"largest bound / mag over the cases: {worst:.2e} (cap {2.0**-12:.2e})")
    assert worst <= 2.0**-12
