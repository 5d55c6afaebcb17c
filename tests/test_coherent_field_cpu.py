"""Host side of the coherent field (no GPU): the phasor header (``d2d_phasor.hpp``) through a plain g++ build against its NumPy
restatement (bit for bit) and against float64 (accuracy), the oracle recipe of ``tests/coherent_field_oracle.py`` against
``R.power_map`` and against known answers (which the GPU tests then hold the kernel to), the host's parameter and memory checks
through a stand-alone g++ program, plain and with sanitizers, ``utils.field_power`` / ``fading_gain``, and the bindings."""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import random_scene, unit_grid
from coherent_field_oracle import (AMP_LINEAR, AMP_SQRT, CoherentField, coherent_field, fold, phasor, phasor_inputs, phasor_quarter,
                                   phasor_reduce, physics)
from strongest_paths_oracle import contributions

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "coherent_field_host.cpp")
GXX = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror"]
COEF7 = np.array([0.3, 0.4, -0.7, 0.6, 0.7, 0.5, 0.0], F)  # (tests/test_gpu_strongest_paths.py: walls 2, 3 and 6 carry reflections)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """d2d_phasor.hpp and d2d_host.hpp's field checks, compiled for the host (tests/native/coherent_field_host.cpp)."""
    so = str(tmp_path_factory.mktemp("cf_host") / "libcf_host.so")
    subprocess.check_call(GXX + ["-shared", "-fPIC", "-o", so, SRC])
    lib = C.CDLL(so)
    fp = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
    lib.cf_phasor.argtypes = [C.c_longlong, fp, fp, fp, fp, fp]
    lib.cf_phasor.restype = None
    lib.cf_field_params.argtypes = [C.c_float, C.c_int]
    lib.cf_field_params.restype = C.c_int
    lib.cf_bytes_per_cell.restype = C.c_longlong
    lib.cf_field_fits.argtypes = [C.c_longlong, C.c_longlong, C.c_longlong]
    lib.cf_field_fits.restype = C.c_int
    return lib


def host_phasor(host, f):
    f = np.ascontiguousarray(f, F)
    c, s, k, g = (np.empty_like(f) for _ in range(4))
    host.cf_phasor(f.size, f, c, s, k, g)
    return c, s, k, g


# ---- the phasor header -----------------------------------------------------------------------------------------------------------
def test_phasor_header_equals_its_numpy_restatement_bit_for_bit(host):
    f = phasor_inputs()
    assert f.size == (1 << 20) + 4096 + 16 + 3
    c, s, k, g = host_phasor(host, f)
    wc, ws = phasor(f)
    wk = phasor_quarter(f)
    for name, got, want in (("cos", c, wc), ("sin", s, ws), ("k", k, wk), ("g", g, phasor_reduce(f, wk))):
        bad = got.view(np.uint32) != want.view(np.uint32)
        assert not bad.any(), f"{name}: {bad.sum()} of {bad.size} differ, first at f = {f[bad][0]!r}"
    # the reduction: k in 0..4 and all five taken, g exact (against float64) and at most an eighth of a turn
    assert set(np.unique(k)) == {0.0, 1.0, 2.0, 3.0, 4.0}
    assert np.array_equal(g.astype(np.float64), f.astype(np.float64) - 0.25 * k.astype(np.float64))
    assert np.abs(g).max() <= 0.125
    # k is floor(4 f + 1/2) in exact arithmetic (float64 holds 4 f + 1/2 exactly) ...
    assert np.array_equal(k.astype(np.float64), np.floor(4.0 * f.astype(np.float64) + 0.5))
    # ... which the fp32 sum is not: it rounds up for the fp32 below 1/8, and f - 0.25 then needs 25 bits
    below = np.nextafter(F(0.125), F(0))
    assert np.floor(below * F(4) + F(0.5)) == 1 and float(F(below - F(0.25))) != float(below) - 0.25
    assert below in f and host_phasor(host, [below])[2][0] == 0
    # 0 and NaN
    c0, s0, _, _ = host_phasor(host, [0.0])
    assert c0.view(np.uint32)[0] == F(1).view(np.uint32) and s0.view(np.uint32)[0] == 0
    cn, sn, _, _ = host_phasor(host, [np.nan])
    assert np.isnan(cn[0]) and np.isnan(sn[0]) and all(np.isnan(v[0]) for v in phasor(np.array([np.nan], F)))


def test_phasor_accuracy_against_float64(host):
    """|error| <= 2 * 2^-24 against float64 cos / sin of 2 pi f over the input set.  The budget: x = g * 6.2831853f carries the
    constant's error (2.8e-8 relative: 0.37 * 2^-24 at |x| = pi / 4) and its own rounding (half an ulp: 0.5 * 2^-24 there), the
    result's last rounding another 0.5 * 2^-24, the polynomial's inner roundings the rest.  Measured: 1.64 * 2^-24."""
    f = phasor_inputs()
    c, s, _, _ = host_phasor(host, f)
    th = 2.0 * np.pi * f.astype(np.float64)
    ec = np.abs(c.astype(np.float64) - np.cos(th)).max() * 2.0**24
    es = np.abs(s.astype(np.float64) - np.sin(th)).max() * 2.0**24
    print(f"phasor: max |cos error| {ec:.3f} * 2^-24, max |sin error| {es:.3f} * 2^-24")
    assert ec <= 2.0 and es <= 2.0


# ---- the host checks, through the stand-alone program ----------------------------------------------------------------------------
def test_host_checks_through_ctypes(host):
    assert host.cf_field_params(0.0, AMP_SQRT) == 0 and host.cf_field_params(20.0, AMP_LINEAR) == 0
    for inv in (-1.0, -1e-30, np.nan, np.inf, -np.inf):
        assert host.cf_field_params(inv, AMP_SQRT) == -1, inv
    for amp in (-1, 2, 7):
        assert host.cf_field_params(20.0, amp) == -1, amp
    assert host.cf_bytes_per_cell() == 12
    for free in (0, 1 << 20, 3 << 30, 288 << 30):
        for held in (0, 1 << 16, 5 << 30):
            edge = (free // 2 + held // 2) // 12
            assert host.cf_field_fits(edge, free, held) == 1 and host.cf_field_fits(edge + 1, free, held) == 0
    assert host.cf_field_fits(1024 * 1024, 200 << 30, 0) == 1 and host.cf_field_fits(1 << 40, 288 << 30, 0) == 0


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_stand_alone_host_program(tmp_path, sanitize):
    """field_params, field_fits (refusals included) and the phasor in a program of their own; with sanitizers it is the same
    program, linked against the sanitizers' run times by the compiler (nothing is preloaded, nothing is loaded into Python)."""
    exe = str(tmp_path / "cf_host")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(GXX + extra + ["-DCF_MAIN", "-o", exe, SRC])
    done = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(done.stdout)
    assert done.returncode == 0, done.stdout
    assert "0 failures" in done.stdout


# ---- the oracle recipe -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid_role", ["rx", "tx"])
@pytest.mark.parametrize("approx", [False, True])
def test_recipe_total_is_the_power_map_and_zero_wavelength_linear_is_it_too(approx, grid_role):
    from oracle import ref as R

    walls = R.square_scene_with_obstacle_walls()
    fixed = np.array([0.2, 0.2], F)
    X, Y = unit_grid(16, 9)
    kw = dict(min_order=0, max_order=2, approx=approx, function="hard_sigmoid", grid_role=grid_role)
    want = np.asarray(R.power_map(walls, fixed, X, Y, **kw), F)
    _, T, Rl, _ = contributions(walls, fixed, X, Y, **kw)
    for amp in (AMP_SQRT, AMP_LINEAR):
        re, im, total = fold(T, Rl, 20.0, amp)
        assert total.dtype == np.float32
        assert np.array_equal(total.reshape(want.shape).view(np.uint32), want.view(np.uint32))
        assert np.count_nonzero(im) > im.size // 2 and np.count_nonzero(re) > re.size // 2
    assert np.count_nonzero(want) > want.size // 2
    # inv = 0, LINEAR: every phasor is (1, +0), so re is the incoherent sum by bits and im is +0.0 everywhere
    re, im, total = fold(T, Rl, 0.0, AMP_LINEAR)
    assert np.array_equal(re.view(np.uint32), total.view(np.uint32)) and not im.view(np.uint32).any()
    # ... while SQRT adds amplitudes: sum sqrt(t) >= sqrt(sum t) for non-negative terms (fp32 roundings: 62 terms of 2^-24 each)
    re, im, _ = fold(T, Rl, 0.0, AMP_SQRT)
    assert not im.view(np.uint32).any()
    assert (re.astype(np.float64) ** 2 >= total.astype(np.float64) * (1 - 62 * 2.0**-23)).all()
    cf = coherent_field(walls, fixed, X, Y, 20.0, AMP_SQRT, **kw)
    assert isinstance(cf, CoherentField) and cf.re.shape == cf.im.shape == cf.total.shape == (9, 16)


@pytest.mark.parametrize("amp", [AMP_SQRT, AMP_LINEAR])
def test_recipe_on_the_line_of_sight_alone(amp):
    """Orders 0..0 in the empty square: one path per cell, so the field's power is the path's own -- |t| with SQRT (within 4 ulp:
    the phasor's c^2 + s^2 and the roundings of the root and the two products), t^2 with LINEAR -- and its phase is the path
    length's: re + j im = a e^(-j 2 pi r / lambda) with r the distance, known in float64."""
    from differt2d_amd.utils import fading_gain, field_power
    from oracle import ref as R

    walls = R.square_scene_walls()
    fixed = np.array([0.3, 0.4], F)
    X, Y = unit_grid(9, 9)
    inv = F(1) / F(0.05)
    cf = coherent_field(walls, fixed, X, Y, inv, amp, min_order=0, max_order=0)
    lit = cf.total != 0
    assert lit.sum() >= 49
    t = cf.total[lit]
    p = field_power(cf)[lit]
    if amp == AMP_SQRT:
        err = np.abs(p - np.abs(t).astype(np.float64)) / np.spacing(np.abs(t)).astype(np.float64)
        print(f"line of sight: field_power within {err.max():.2f} ulp of |t|")
        assert err.max() <= 4
        gain = fading_gain(cf)
        assert np.abs(gain[lit] - 1).max() <= 4 * 2.0**-23 and np.isnan(gain[~lit]).all()
    else:
        assert np.abs(p / t.astype(np.float64) ** 2 - 1).max() <= 4 * 2.0**-23
    # the phase is that of the path length (the convention e^(-j 2 pi r / lambda)): from the oracle's fp32 length, which is the
    # distance, u = r / lambda in float64 differs from the fp32 product by half an ulp (pi ulp(u) radians); the phasor, the root and
    # the product add 2 * 2^-24 + 2^-23
    _, _, Rl, _ = contributions(walls, fixed, X, Y, min_order=0, max_order=0)
    r = Rl[0].reshape(X.shape)[lit].astype(np.float64)
    d = np.hypot(X.astype(np.float64) - float(fixed[0]), Y.astype(np.float64) - float(fixed[1]))[lit]
    assert np.abs(r - d).max() < 1e-6
    a = np.sqrt(t.astype(np.float64)) if amp == AMP_SQRT else t.astype(np.float64)
    u = r * float(inv)
    want = a * np.exp(-2j * np.pi * u)
    got = cf.re[lit].astype(np.float64) + 1j * cf.im[lit].astype(np.float64)
    tol = a * (np.pi * np.spacing(u.astype(F)).astype(np.float64) + 2 * 2.0**-24 + 2.0**-23)
    assert (np.abs(got - want) <= tol).all(), (np.abs(got - want) / tol).max()
    assert u.max() > 10 and np.count_nonzero(cf.im) > lit.sum() // 2  # (several turns of phase; a whole number of them has im = 0)


@pytest.mark.parametrize("amp", [AMP_SQRT, AMP_LINEAR])
def test_recipe_negative_coefficient_flips_the_sign_of_that_paths_phasor(amp):
    fixed, walls = random_scene(7, seed=77)
    X, Y = unit_grid(21, 13)
    kw = dict(min_order=0, max_order=1, fun="received_power_per_object", fun_kwargs=dict(height=0.25))
    flipped = COEF7.copy()
    flipped[2] = -flipped[2]
    cands, T, Rl, _ = contributions(walls, fixed, X, Y, coef=COEF7, **kw)
    _, Tf, Rlf, _ = contributions(walls, fixed, X, Y, coef=flipped, **kw)
    ci = [tuple(int(w) for w in c) for c in cands].index((2,))
    inv = F(20.0)
    assert (T[ci] < 0).any() and not (T[ci] > 0).any() and np.array_equal(Tf[ci], -T[ci]) and np.array_equal(Rl, Rlf)
    # the path alone: the same phasor with the opposite sign, bit for bit
    re_n, im_n, _ = fold(T[ci : ci + 1], Rl[ci : ci + 1], inv, amp)
    re_p, im_p, _ = fold(Tf[ci : ci + 1], Rl[ci : ci + 1], inv, amp)
    on = T[ci] != 0
    assert on.sum() > 10 and np.array_equal(re_n[on], -re_p[on]) and np.array_equal(im_n[on], -im_p[on]) and re_n[on].any() and im_n[on].any()
    # in the cell's sum: flipping the coefficient moves the field by twice that path's phasor (float64 physics and its bound)
    field_n, bound_n = physics(T, Rl, inv, amp)
    field_p, bound_p = physics(Tf, Rl, inv, amp)
    one = re_p.astype(np.float64) + 1j * im_p.astype(np.float64)
    assert (np.abs((field_p - field_n) - 2 * one) <= bound_n + bound_p).all()
    re, im, _ = fold(T, Rl, inv, amp)
    assert (np.abs(re + 1j * im.astype(np.float64) - field_n) <= bound_n).all()
    # the zero coefficient (wall 6) adds no phasor at all
    c6 = [tuple(int(w) for w in c) for c in cands].index((6,))
    assert not T[c6].any() and not any(a.view(np.uint32).any() for a in fold(T[c6 : c6 + 1], Rl[c6 : c6 + 1], inv, amp))


def test_recipe_respects_the_float64_physics_with_many_paths():
    from oracle import ref as R

    walls = R.square_scene_with_obstacle_walls()
    fixed = np.array([0.2, 0.2], F)
    X, Y = unit_grid(16, 9)
    _, T, Rl, _ = contributions(walls, fixed, X, Y, min_order=0, max_order=2, approx=True, function="hard_sigmoid")
    assert ((T != 0).sum(axis=0) >= 2).mean() > 0.5
    for amp in (AMP_SQRT, AMP_LINEAR):
        for inv in (20.0, 4096.0):
            re, im, _ = fold(T, Rl, inv, amp)
            field, bound = physics(T, Rl, inv, amp)
            err = np.abs(re.astype(np.float64) + 1j * im.astype(np.float64) - field)
            assert (err <= bound).all(), (amp, inv, (err / bound).max())
    # interference is there to be seen: the coherent power is above the incoherent one in some cells and below it in others
    re, im, total = fold(T, Rl, 20.0, AMP_SQRT)
    gain = (re.astype(np.float64) ** 2 + im.astype(np.float64) ** 2)[total > 0] / total[total > 0]
    assert gain.max() > 1.5 and gain.min() < 0.5


# ---- utils and bindings ----------------------------------------------------------------------------------------------------------
def test_field_power_and_fading_gain_known_answers():
    from differt2d_amd.utils import fading_gain, field_power

    cf = CoherentField(np.array([[3.0, 0.0], [1.0, 0.0]], F), np.array([[4.0, -2.0], [1.0, 0.0]], F), np.array([[5.0, 8.0], [-2.0, 0.0]], F))
    p, g = field_power(cf), fading_gain(cf)
    assert p.dtype == g.dtype == np.float64 and p.shape == g.shape == (2, 2)
    assert np.array_equal(p, [[25.0, 4.0], [2.0, 0.0]])
    assert g[0, 0] == 5.0 and g[0, 1] == 0.5 and g[1, 0] == -1.0 and np.isnan(g[1, 1])


def test_bindings_and_abi_version():
    from differt2d_amd import _lib as L
    from differt2d_amd import utils
    from differt2d_amd.engine import CoherentField as CF, Context
    from differt2d_amd.scene import Scene

    assert L.D2D_ABI_VERSION == 12
    assert (L.D2D_FIELD_AMP_SQRT, L.D2D_FIELD_AMP_LINEAR) == (AMP_SQRT, AMP_LINEAR) == (0, 1)
    names = [s[0] for s in L.SYMBOLS]
    assert "d2d_coherent_field_launch" in names and "d2d_get_coherent_field" in names and "d2d_selftest_phasor" in names
    assert callable(Context.coherent_field) and callable(Context.launch_coherent_field) and callable(Context.get_coherent_field)
    assert callable(Context.selftest_phasor)
    assert callable(Scene.coherent_field_on_receivers_grid) and callable(Scene.coherent_field_on_transmitters_grid)
    assert CF._fields == CoherentField._fields == ("re", "im", "total")
    assert callable(utils.field_power) and callable(utils.fading_gain)
    header = open(os.path.join(ROOT, "include", "d2d.h")).read()
    assert "#define D2D_FIELD_AMP_SQRT 0" in header and "#define D2D_FIELD_AMP_LINEAR 1" in header


def test_scene_refuses_a_fun_that_is_not_fused_and_names_the_sparse_route():
    from differt2d_amd import _lib as L
    from differt2d_amd.scene import Scene

    scene = Scene.square_scene_with_obstacle()
    X, Y = unit_grid(4, 3)

    def step(tx, rx, path, objs):
        return (path.length() < 1.0).astype(F)

    for method in (scene.coherent_field_on_receivers_grid, scene.coherent_field_on_transmitters_grid):
        with pytest.raises(L.D2DUnsupported, match="valid_paths"):
            next(iter(method(X, Y, step, wavelength=0.05)))
