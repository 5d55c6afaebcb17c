"""Host side of the channel frequency response (no GPU): the oracle of ``tests/frequency_response_oracle.py`` pinned to the coherent
field's for single entries (the GPU tests then hold the kernel to it), the host's parameter checks, memory check and chunk plan
through a stand-alone g++ program, plain and with sanitizers, ``utils.frequency_response`` / ``wideband_power`` /
``impulse_response``, and the bindings."""

import os
import subprocess

import numpy as np
import pytest

from conftest import unit_grid
from coherent_field_oracle import AMP_LINEAR, AMP_SQRT, coherent_field
from frequency_response_oracle import FrequencyResponse, fold_list, frequency_response, guard, wideband_physics
from strongest_paths_oracle import contributions

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "frequency_response_host.cpp")
GXX = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror"]
INV_20 = F(1) / F(0.05)


def inv_list(nf):
    """``inv_j = INV_20 * (1 + j / 64)``, fp32."""
    return (INV_20 * (F(1) + np.arange(nf, dtype=F) / F(64))).astype(F)


# ---- the oracle ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid_role", ["rx", "tx"])
@pytest.mark.parametrize("approx", [False, True])
def test_oracle_planes_are_the_coherent_field_oracle_entry_by_entry(approx, grid_role):
    from oracle import ref as R

    walls = R.square_scene_with_obstacle_walls()
    fixed = np.array([0.2, 0.2], F)
    X, Y = unit_grid(16, 9)
    kw = dict(min_order=0, max_order=2, approx=approx, function="hard_sigmoid", grid_role=grid_role)
    inv = inv_list(9)
    for amp in (AMP_SQRT, AMP_LINEAR):
        fr = frequency_response(walls, fixed, X, Y, inv, amp, **kw)
        assert isinstance(fr, FrequencyResponse) and fr.re.shape == fr.im.shape == (9, 9, 16) and fr.total.shape == (9, 16)
        assert fr.re.dtype == fr.im.dtype == fr.total.dtype == np.float32
        guard(fr.re, fr.im)
        for j in (0, 4, 8):
            cf = coherent_field(walls, fixed, X, Y, inv[j], amp, **kw)
            one = frequency_response(walls, fixed, X, Y, [inv[j]], amp, **kw)
            for a, b, c in ((fr.re[j], cf.re, one.re[0]), (fr.im[j], cf.im, one.im[0]), (fr.total, cf.total, one.total)):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(a.view(np.uint32), c.view(np.uint32))
    want = np.asarray(R.power_map(walls, fixed, X, Y, **kw), F)
    assert np.array_equal(fr.total.view(np.uint32), want.view(np.uint32)) and np.count_nonzero(want) > want.size // 2
    # an entry 0 with LINEAR: the fused map in re, +0.0 in im, whatever its neighbours in the list are
    fr = frequency_response(walls, fixed, X, Y, [inv[1], 0.0, inv[2]], AMP_LINEAR, **kw)
    assert np.array_equal(fr.re[1].view(np.uint32), want.view(np.uint32)) and not fr.im[1].view(np.uint32).any()


def test_oracle_guard_catches_a_reused_wavelength_and_an_empty_plane():
    from oracle import ref as R

    walls = R.square_scene_with_obstacle_walls()
    X, Y = unit_grid(8, 5)
    _, T, Rl, _ = contributions(walls, np.array([0.2, 0.2], F), X, Y, min_order=0, max_order=1)
    re, im, _ = fold_list(T, Rl, inv_list(3), AMP_SQRT)
    guard(re, im)
    with pytest.raises(AssertionError):
        guard(re[[0, 1, 0]], im[[0, 1, 0]])
    with pytest.raises(AssertionError):
        guard(*fold_list(T, Rl, [INV_20, 0.0], AMP_SQRT)[:2])  # the entry 0 has im = +0 everywhere


# ---- the host checks, through the stand-alone program ----------------------------------------------------------------------------
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_stand_alone_host_program(tmp_path, sanitize):
    """freq_params (every bad entry position, both nf limits), freq_fits (boundary byte, sizes that would wrap 64 bits) and the chunk
    plan for nf in {1, 7, 8, 9, 16, 17, 1024} in a program of their own; with sanitizers it is the same program, linked against the
    sanitizers' run times by the compiler (nothing is preloaded, nothing is loaded into Python)."""
    exe = str(tmp_path / "fr_host")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(GXX + extra + ["-o", exe, SRC])
    done = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(done.stdout)
    assert done.returncode == 0, done.stdout
    assert "0 failures" in done.stdout


# ---- utils -----------------------------------------------------------------------------------------------------------------------
def test_frequency_response_assembles_the_planes():
    from differt2d_amd.utils import frequency_response as H

    rng = np.random.default_rng(7)
    re, im = rng.standard_normal((5, 3, 4)).astype(F), rng.standard_normal((5, 3, 4)).astype(F)
    h = H(FrequencyResponse(re, im, np.zeros((3, 4), F)))
    assert h.dtype == np.complex64 and h.shape == (5, 3, 4)
    assert np.array_equal(h.real.view(np.uint32), re.view(np.uint32)) and np.array_equal(h.imag.view(np.uint32), im.view(np.uint32))
    assert np.array_equal(h[2, 1, 3], np.complex64(complex(re[2, 1, 3], im[2, 1, 3])))


def test_wideband_power_of_a_two_path_cell_is_the_closed_form():
    """Two paths a1, r1 and a2, r2 on nf wavelengths: |H_j|^2 = a1^2 + a2^2 + 2 a1 a2 cos(2 pi (r2 - r1) inv_j), whose mean over j
    is the closed form.  The planes are formed in float64 and rounded to fp32 once; wideband_power squares those fp32 values in
    float64, so it equals the float64 mean of their squares up to the order of the additions, and the closed form within the rounding of
    the planes: 2 * 2^-24 relative on a power of at most (|a1| + |a2|)^2, plus float64 roundings (a factor 2 of margin)."""
    from differt2d_amd.utils import wideband_power

    a1, a2, r1, r2 = 0.75, -0.5, 1.25, 2.0625
    nf = 16
    inv = inv_list(nf).astype(np.float64)
    h = a1 * np.exp(-2j * np.pi * r1 * inv) + a2 * np.exp(-2j * np.pi * r2 * inv)
    dark = np.zeros(nf)
    fr = FrequencyResponse(np.stack([h.real, dark], 1).reshape(nf, 1, 2).astype(F), np.stack([h.imag, dark], 1).reshape(nf, 1, 2).astype(F),
                           np.array([[a1 * a1 + a2 * a2, 0.0]], F))
    p = wideband_power(fr)
    assert p.dtype == np.float64 and p.shape == (1, 2)
    assert p[0, 1] == 0.0
    # (the same float64 squares, summed in another order: nf additions of 2^-53 relative each)
    assert abs(p[0, 0] - (fr.re[:, 0, 0].astype(np.float64) ** 2 + fr.im[:, 0, 0].astype(np.float64) ** 2).mean()) <= nf * 2.0**-53 * p[0, 0]
    closed = a1 * a1 + a2 * a2 + 2 * a1 * a2 * np.cos(2 * np.pi * (r2 - r1) * inv).mean()
    assert abs(p[0, 0] - closed) <= 2 * (2 * 2.0**-24) * (abs(a1) + abs(a2)) ** 2
    # ... and the cross term is there: 16 entries span 4 turns of r2 - r1, which leaves 0.007 of it
    assert abs(closed - (a1 * a1 + a2 * a2)) > 1e-3


@pytest.mark.parametrize("nf,r", [(64, 1.3), (64, 7.9), (17, 0.4), (2, 0.6)])
def test_impulse_response_of_a_single_path_peaks_at_its_tap(nf, r):
    """H_j = a e^(-j 2 pi r (inv_0 + j step)): the inverse DFT along j peaks at tap round(r nf step) mod nf, and the taps are
    1 / (nf step) of path length apart."""
    from differt2d_amd.utils import impulse_response

    step, inv0, a = 1.0 / 3.2, 20.0, 0.8
    inv = inv0 + step * np.arange(nf)
    h = a * np.exp(-2j * np.pi * r * inv)
    cells = np.zeros((nf, 2, 3), np.complex128)
    cells[:, 1, 2] = h
    fr = FrequencyResponse(cells.real.astype(F), cells.imag.astype(F), np.zeros((2, 3), F))
    taps, spacing = impulse_response(fr, step)
    assert taps.shape == (nf, 2, 3) and np.iscomplexobj(taps)
    assert spacing == 1.0 / (nf * step)
    assert np.allclose(taps, np.fft.ifft(cells.real.astype(F) + 1j * cells.imag.astype(F), axis=0), rtol=0, atol=1e-6)
    peak = int(np.argmax(np.abs(taps[:, 1, 2])))
    assert peak == int(round(r * nf * step)) % nf
    assert not taps[:, 0, 0].any()
    # the peak's path length, tap * spacing, is r up to half a tap and the aliasing period 1 / step
    assert abs((peak * spacing - r + 0.5 / step) % (1.0 / step) - 0.5 / step) <= spacing / 2 + 1e-12


def test_impulse_response_refuses_fewer_than_two_frequencies_and_a_bad_step():
    from differt2d_amd.utils import impulse_response

    one = FrequencyResponse(np.ones((1, 2, 2), F), np.zeros((1, 2, 2), F), np.ones((2, 2), F))
    with pytest.raises(ValueError, match="nf"):
        impulse_response(one, 0.25)
    two = FrequencyResponse(np.ones((2, 2, 2), F), np.zeros((2, 2, 2), F), np.ones((2, 2), F))
    for step in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="step"):
            impulse_response(two, step)
    taps, spacing = impulse_response(two, 0.25)
    assert spacing == 2.0 and np.array_equal(taps[:, 0, 0], [1.0, 0.0])


def test_wideband_physics_bound_holds_for_the_oracle_itself():
    """The bound the GPU test holds utils.wideband_power to, first met by the oracle's own fp32 planes."""
    from differt2d_amd.utils import wideband_power
    from oracle import ref as R

    walls = R.square_scene_with_obstacle_walls()
    X, Y = unit_grid(8, 5)
    _, T, Rl, _ = contributions(walls, np.array([0.2, 0.2], F), X, Y, min_order=0, max_order=2)
    inv = inv_list(17)
    for amp in (AMP_SQRT, AMP_LINEAR):
        re, im, total = fold_list(T, Rl, inv, amp)
        power, bound = wideband_physics(T, Rl, inv, amp)
        got = wideband_power(FrequencyResponse(re, im, total)).reshape(-1)
        assert (np.abs(got - power) <= bound).all() and power.any()


# ---- bindings --------------------------------------------------------------------------------------------------------------------
def test_bindings_and_abi_version():
    from differt2d_amd import _lib as L
    from differt2d_amd import utils
    from differt2d_amd.engine import Context, FrequencyResponse as FR
    from differt2d_amd.scene import Scene

    assert L.D2D_ABI_VERSION == 12 and L.D2D_FREQ_MAX == 1024
    names = [s[0] for s in L.SYMBOLS]
    assert "d2d_frequency_response_launch" in names and "d2d_get_frequency_response" in names
    assert callable(Context.frequency_response) and callable(Context.launch_frequency_response) and callable(Context.get_frequency_response)
    assert callable(Scene.frequency_response_on_receivers_grid) and callable(Scene.frequency_response_on_transmitters_grid)
    assert FR._fields == FrequencyResponse._fields == ("re", "im", "total")
    assert callable(utils.frequency_response) and callable(utils.wideband_power) and callable(utils.impulse_response)
    header = open(os.path.join(ROOT, "include", "d2d.h")).read()
    assert "#define D2D_FREQ_MAX 1024" in header and "#define D2D_ABI_VERSION 12" in header
    assert "int d2d_frequency_response_launch(" in header and "int d2d_get_frequency_response(" in header


def test_scene_refuses_a_fun_that_is_not_fused_and_wants_exactly_one_list():
    from differt2d_amd import _lib as L
    from differt2d_amd import utils
    from differt2d_amd.scene import Scene

    scene = Scene.square_scene_with_obstacle()
    X, Y = unit_grid(4, 3)

    def step(tx, rx, path, objs):
        return (path.length() < 1.0).astype(F)

    for method in (scene.frequency_response_on_receivers_grid, scene.frequency_response_on_transmitters_grid):
        with pytest.raises(L.D2DUnsupported, match="valid_paths"):
            next(iter(method(X, Y, step, wavelengths=[0.05])))
        with pytest.raises(ValueError, match="exactly one"):
            method(X, Y, utils.received_power)
        with pytest.raises(ValueError, match="exactly one"):
            method(X, Y, utils.received_power, wavelengths=[0.05], inv_wavelengths=[20.0])
