"""Host side of the material response (no GPU): ``d2d_fresnel.hpp``'s arithmetic and the host's parameter and memory checks through a
stand-alone g++ program (plain and with sanitizers; nothing of it is loaded into Python), the header against the NumPy restatement
of ``tests/material_response_oracle.py`` bit for bit and against float64 in accuracy, the physics of ``utils.fresnel_coefficient``
and ``utils.complex_permittivity``, the oracle's own line-of-sight and independence properties, the bindings and the ``Scene``
methods' refusals."""

import os
import subprocess

import numpy as np
import pytest

import frequency_response_oracle as FRO
import material_response_oracle as MO
from conftest import unit_grid
from test_gpu_strongest_paths import _case

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "material_response_host.cpp")
GXX = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
U = 2.0**-24


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """tests/native/material_response_host.cpp as a program of its own, plain and with sanitizers (linked against their run times by
    the compiler: nothing is preloaded)."""
    d = tmp_path_factory.mktemp("material_host")
    out = {}
    for name, extra in (("plain", []), ("asan_ubsan", SANITIZE)):
        out[name] = str(d / f"material_host_{name}")
        subprocess.check_call(GXX + extra + ["-o", out[name], SRC])
    return out


def _run_header(exe, tmp_path, er, ei, c):
    """``(gr_te, gi_te, gr_tm, gi_tm)`` of the header's g++ build over a list."""
    n = er.size
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(np.int64(n).tobytes())
        for a in (er, ei, c):
            f.write(np.ascontiguousarray(a, F).tobytes())
    subprocess.run([exe, inp, outp], check=True, timeout=300)
    out = np.fromfile(outp, F)
    assert out.size == 4 * n
    return out.reshape(4, n)


# ---- the stand-alone program ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", ["plain", "asan_ubsan"])
def test_stand_alone_host_program(programs, build):
    """The header's stated values, every refusal of material_params, the memory rule at its boundary byte and with sizes that would
    wrap, the chunk plan and the constant-band detection (rows that differ in the sign of a zero included)."""
    done = subprocess.run([programs[build]], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(done.stdout)
    assert done.returncode == 0, done.stdout
    assert "material_response_host: chunk 8, 0 failures" in done.stdout


@pytest.mark.parametrize("build", ["plain", "asan_ubsan"])
def test_header_equals_the_numpy_restatement_by_bits(programs, tmp_path, build):
    """The shared input list: seeded random permittivities and cosines, eps near 1, total reflection, c of 0, 1, above 1 and NaN,
    components of 2^50, NaN and inf in every position (NaN results compare as NaN: their payload is not part of the definition)."""
    er, ei, c = MO.fresnel_inputs()
    got = _run_header(programs[build], tmp_path, er, ei, c)
    assert er.size > 60000
    seen_nan = seen_graze = False
    for k, pol in enumerate((MO.POL_TE, MO.POL_TM)):
        want = MO.fresnel(er, ei, c, pol)
        for name, g, w in zip(("gr", "gi"), got[2 * k:2 * k + 2], want):
            ok = MO.same_bits(g, w)
            assert ok.all(), (pol, name, int((~ok).sum()), int(np.flatnonzero(~ok)[0]))
        seen_nan |= bool(np.isnan(want[0]).any())
        seen_graze |= bool((want[0] == -1).any())
        finite = np.isfinite(er) & np.isfinite(ei) & np.isfinite(c)
        assert np.isfinite(want[0][finite]).all() and np.isfinite(want[1][finite]).all()  # components up to 2^50 stay finite
    assert seen_nan and seen_graze


def test_restatement_at_the_special_points():
    for pol in (MO.POL_TE, MO.POL_TM):
        for ei in (0.0, -0.0):
            for c in (1.0, 0.5):
                gr, gi = MO.fresnel(F(1), F(ei), F(c), pol)
                assert gr == 0 and gi == 0  # eps = 1: exactly no reflection
            gr, gi = MO.fresnel(F(0.25), F(ei), np.array([0.1, 0.5, 0.8], F), pol)
            assert np.allclose(gr.astype(np.float64) ** 2 + gi.astype(np.float64) ** 2, 1, atol=1e-6)  # total reflection
        gr, gi = MO.fresnel(F(4), F(-1), F(0), pol)
        assert _bits(gr) == _bits(F(-1)) and gi == 0  # grazing
        gr, gi = MO.fresnel(F(4), F(-1), F(np.nan), pol)
        assert np.isnan(gr) and np.isnan(gi)
    gr, gi = MO.fresnel(F(4), F(-0.0), np.array([1.0, np.nextafter(F(1), F(2)), 7.0], F), MO.POL_TE)
    assert (_bits(gr) == _bits(F(-1) / F(3))).all() and (gi == 0).all()  # c above 1 is 1
    gr, gi = MO.fresnel(F(4), F(-0.0), F(1), MO.POL_TM)
    assert _bits(gr) == _bits(F(1) / F(3))


# ---- accuracy against float64 ---------------------------------------------------------------------------------------------------------
def _float64(er, ei, c, pol):
    from differt2d_amd.utils import fresnel_coefficient

    return fresnel_coefficient(er.astype(np.float64) + 1j * ei.astype(np.float64), c.astype(np.float64), "tm" if pol == MO.POL_TM else "te")


def test_header_accuracy_against_float64(programs, tmp_path):
    """The g++ build of the header against the float64 formula on the stated domain, eps' in [1.5, 100], eps'' in [0, 1000], cos in
    [1e-3, 1], 2^20 seeded points: measured 4.792 * 2^-24 per component (printed), asserted below 5.25.  The corner eps' within 1e-3 of 1
    without loss, where a 1 - cos^2 would cancel against eps', is reported only (2.7 * 2^-24 with the header's (eps' - 1) + cos^2)."""
    rng = np.random.default_rng(20261021)
    n = 1 << 20
    er = rng.uniform(1.5, 100, n).astype(F)
    ei = (-rng.uniform(0, 1000, n)).astype(F)
    ei[: n // 4] = (-rng.uniform(0, 1, n // 4)).astype(F)  # weakly lossy too
    c = rng.uniform(1e-3, 1, n).astype(F)
    got = _run_header(programs["plain"], tmp_path, er, ei, c)
    worst = 0.0
    for k, pol in enumerate((MO.POL_TE, MO.POL_TM)):
        ref = _float64(er, ei, c, pol)
        err = max(np.abs(got[2 * k] - ref.real).max(), np.abs(got[2 * k + 1] - ref.imag).max()) / U
        print(f"fresnel vs float64, pol {pol}: max error {err:.3f} * 2^-24")
        worst = max(worst, err)
    assert worst < 5.25
    assert MO.FRESNEL_BOUND == 5.25  # what the closed-form bound of the GPU test takes
    # the corner, reported
    er1 = (1 + 1e-3 * rng.random(n)).astype(F)
    ei1 = np.full(n, -0.0, F)
    got = _run_header(programs["plain"], tmp_path, er1, ei1, c)
    for k, pol in enumerate((MO.POL_TE, MO.POL_TM)):
        ref = _float64(er1, ei1, c, pol)
        err = max(np.abs(got[2 * k] - ref.real).max(), np.abs(got[2 * k + 1] - ref.imag).max()) / U
        print(f"fresnel vs float64 near eps' = 1, pol {pol}: max error {err:.1f} * 2^-24 (reported, not bounded)")
        assert np.isfinite(got).all()


# ---- the physics of utils.fresnel_coefficient -----------------------------------------------------------------------------------------
def test_fresnel_coefficient_physics():
    from differt2d_amd.utils import fresnel_coefficient

    eps = np.array([2.0, 4.0, 5.31 - 0.5j, 9 - 20j, 1.0001], np.complex128)
    root = np.sqrt(eps)
    te, tm = fresnel_coefficient(eps, 1.0, "te"), fresnel_coefficient(eps, 1.0, "tm")
    assert np.allclose(te, (1 - root) / (1 + root), rtol=0, atol=1e-15)  # normal incidence
    assert np.allclose(tm, -te, rtol=0, atol=1e-15)  # ... up to TM's sign convention (the docstring states it)
    for e in (2.0, 4.0, 30.0):  # Brewster: TM vanishes at cos = 1 / sqrt(1 + eps) for real eps
        assert abs(fresnel_coefficient(e, 1 / np.sqrt(1 + e), "tm")) < 1e-15
        assert abs(fresnel_coefficient(e, 1 / np.sqrt(1 + e), "te")) > 0.1
    rng = np.random.default_rng(3)
    e = rng.uniform(0.1, 50, 4096) - 1j * rng.uniform(0, 200, 4096)
    c = rng.uniform(0, 1, 4096)
    for pol in ("te", "tm"):
        assert (np.abs(fresnel_coefficient(e, c, pol)) <= 1 + 1e-12).all()  # passive for Im eps <= 0
        assert np.allclose(fresnel_coefficient(e, 0.0, pol), -1)  # grazing
    assert np.allclose(np.abs(fresnel_coefficient(0.25, np.array([0.1, 0.5, 0.8]), "te")), 1)  # total reflection
    assert np.allclose(np.abs(fresnel_coefficient(0.25 - 0.0j, np.array([0.1, 0.5, 0.8]), "tm")), 1)
    big = np.array([1e12, -1e12j, 1e12 - 1e12j])
    assert np.allclose(fresnel_coefficient(big, 0.3, "te"), -1, atol=1e-5)  # a perfect conductor
    assert np.allclose(fresnel_coefficient(big, 0.3, "tm"), +1, atol=1e-5)
    assert fresnel_coefficient(1.0, 0.4, "te") == 0 and fresnel_coefficient(1.0, 0.4, "tm") == 0
    assert fresnel_coefficient(eps[:, None], np.linspace(0, 1, 7)[None, :]).shape == (5, 7)
    with pytest.raises(ValueError, match="polarization"):
        fresnel_coefficient(2.0, 0.5, "circular")
    # the lossy branch decays: Im q <= 0 means the TE coefficient of a lossy wall has a NEGATIVE imaginary part's conjugate convention
    g = fresnel_coefficient(4 - 2j, 0.5, "te")
    c_, q = 0.5, np.sqrt(4 - 2j - 0.75)
    assert q.imag < 0 and np.isclose(g, (c_ - q) / (c_ + q))


def test_complex_permittivity_against_a_hand_computed_value():
    from differt2d_amd.utils import complex_permittivity

    # concrete-like: eps_r = 5.31, sigma = 0.0326 S/m at 1 GHz: 0.0326 / (2 pi * 1e9 * 8.8541878128e-12) = 0.585993...
    e = complex_permittivity(5.31, 0.0326, 1e9)
    assert e.real == 5.31 and abs(e.imag + 0.0326 / (2 * np.pi * 1e9 * 8.8541878128e-12)) < 1e-15
    assert abs(e.imag + 0.58599) < 1e-4
    band = complex_permittivity(5.31, 0.0326, np.array([1e9, 2e9]))
    assert band.shape == (2,) and np.isclose(band[1].imag, e.imag / 2) and (band.imag < 0).all()
    assert complex_permittivity(3.0, 0.0, 1e9) == 3.0


# ---- the oracle's own properties (NumPy alone) -------------------------------------------------------------------------------------------
def test_oracle_line_of_sight_is_the_frequency_response_recipe_by_bits():
    walls, fixed, X, Y = _case("random7")
    inv = np.array([20.0, 7.0, 0.0], F)
    eps = np.array([[3 - 1j * k - 0.5j * j for j in range(len(walls))] for k in range(3)], np.complex64)
    kw = dict(min_order=0, max_order=0, approx=True, function="hard_sigmoid")
    got = MO.material_response(walls, fixed, X, Y, inv, eps, MO.POL_TM, MO.AMP_SQRT, **kw)
    want = FRO.frequency_response(walls, fixed, X, Y, inv, MO.AMP_SQRT, **kw)
    for g, w in zip(got, want):
        assert np.array_equal(_bits(g), _bits(w))


def test_oracle_independence_and_polarisations_differ():
    walls, fixed, _, _ = _case("random7")
    X, Y = unit_grid(7, 5)
    N = len(walls)
    con = MO.segment_contributions(walls, fixed, X, Y, min_order=0, max_order=2, approx=False)
    inv = np.array([20.0, 21.5, 20.0], F)
    rng = np.random.default_rng(11)
    eps = (rng.uniform(2, 9, (3, N)) - 1j * rng.uniform(0, 3, (3, N))).astype(np.complex64)
    te = MO.material_response(walls, fixed, X, Y, inv, eps, MO.POL_TE, MO.AMP_SQRT, contributions=con)
    tm = MO.material_response(walls, fixed, X, Y, inv, eps, MO.POL_TM, MO.AMP_SQRT, contributions=con)
    assert (te.re != tm.re).any() and np.array_equal(_bits(te.total), _bits(tm.total))
    assert (te.re[0] != te.re[2]).any()  # equal wavelengths, different rows of eps
    perm = [2, 0, 1]
    p = MO.material_response(walls, fixed, X, Y, inv[perm], eps[perm], MO.POL_TE, MO.AMP_SQRT, contributions=con)
    assert np.array_equal(_bits(p.re), _bits(te.re[perm])) and np.array_equal(_bits(p.im), _bits(te.im[perm]))
    one = MO.material_response(walls, fixed, X, Y, inv[1:2], eps[1:2], MO.POL_TE, MO.AMP_SQRT, contributions=con)
    assert np.array_equal(_bits(one.re[0]), _bits(te.re[1])) and np.array_equal(_bits(one.im[0]), _bits(te.im[1]))
    assert (np.count_nonzero(te.im) > te.im.size // 3) and np.isfinite(te.re).all()


# ---- bindings and refusals ----------------------------------------------------------------------------------------------------------------
def test_bindings_and_abi_version():
    from differt2d_amd import _lib as L
    from differt2d_amd import utils
    from differt2d_amd.engine import POLARIZATIONS, Context, FrequencyResponse
    from differt2d_amd.scene import Scene

    assert L.D2D_ABI_VERSION == 12 and (L.D2D_POL_TE, L.D2D_POL_TM) == (0, 1) == (MO.POL_TE, MO.POL_TM)
    assert POLARIZATIONS == {"te": 0, "tm": 1}
    names = [s[0] for s in L.SYMBOLS]
    assert all(n in names for n in ("d2d_material_response_launch", "d2d_get_material_response", "d2d_selftest_fresnel"))
    assert callable(Context.material_response) and callable(Context.launch_material_response) and callable(Context.get_material_response)
    assert callable(Context.selftest_fresnel)
    assert callable(Scene.material_response_on_receivers_grid) and callable(Scene.material_response_on_transmitters_grid)
    assert FrequencyResponse._fields == MO.MaterialResponse._fields == ("re", "im", "total")
    assert callable(utils.complex_permittivity) and callable(utils.fresnel_coefficient)
    header = open(os.path.join(ROOT, "include", "d2d.h")).read()
    assert "#define D2D_ABI_VERSION 12" in header and "#define D2D_POL_TE 0" in header and "#define D2D_POL_TM 1" in header
    assert "int d2d_material_response_launch(" in header and "int d2d_get_material_response(" in header and "int d2d_selftest_fresnel(" in header
    # the header holds the definition, in the words of d2d_fresnel.hpp
    fres = open(os.path.join(ROOT, "differt2d_amd", "csrc", "d2d_fresnel.hpp")).read()
    for line in ("m  = sqrtf(wr*wr + wi*wi)", "else if (wr >= 0)  qr = sqrtf(0.5f*(m + wr)) ; qi = wi / (2.0f*qr)",
                 "if (den == 0)      (gr, gi) = (-1, 0)"):
        assert line in header and line in fres
    lib = L.load()  # the library has all three
    assert lib.d2d_material_response_launch and lib.d2d_get_material_response and lib.d2d_selftest_fresnel and lib.d2d_abi_version() == 12


def test_scene_refusals_without_a_launch():
    from differt2d_amd import _lib as L
    from differt2d_amd.scene import Scene
    from differt2d_amd.utils import received_power

    scene = Scene.square_scene_with_obstacle()
    n = len(scene.objects)
    X, Y = unit_grid(4, 3)

    def step(tx, rx, path, objs):
        return (path.length() < 1.0).astype(F)

    for method in (scene.material_response_on_receivers_grid, scene.material_response_on_transmitters_grid):
        with pytest.raises(L.D2DUnsupported, match="valid_paths") as e:
            next(iter(method(X, Y, step, wavelengths=[0.05, 0.06], permittivity=np.full(n, 4 - 1j))))
        assert "trace_paths" in str(e.value) and "material response" in str(e.value)
        with pytest.raises(ValueError, match="exactly one"):
            method(X, Y, received_power, permittivity=np.full(n, 4 - 1j))
        with pytest.raises(ValueError, match="exactly one"):
            method(X, Y, received_power, wavelengths=[0.05], inv_wavelengths=[20.0])
        # no permittivity anywhere: the first object without one is named
        with pytest.raises(ValueError, match="object 0 .*no permittivity"):
            next(iter(method(X, Y, received_power, wavelengths=[0.05])))
        with pytest.raises(ValueError, match=rf"\[{n}\]"):
            next(iter(method(X, Y, received_power, wavelengths=[0.05, 0.06], permittivity=np.ones((3, n)))))
    # read from the objects' attributes: a scalar for the band, or one value per wavelength
    table = scene._permittivity_table(np.arange(n) + 2 - 1j, 3)
    assert table.shape == (n,) and table.dtype == np.complex64


def test_context_refuses_unknown_names():
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import _polarization_id

    assert _polarization_id("x", "TE") == 0 and _polarization_id("x", "tm") == 1 and _polarization_id("x", 1) == 1
    with pytest.raises(L.D2DError, match="polarization"):
        _polarization_id("material_response", "circular")
