"""Host side of the power-angle profile (no GPU): the direction header (``d2d_angle.hpp``) through a plain g++ build against its
NumPy restatement (bit for bit) and against float64 (accuracy), the oracle recipe of ``tests/power_angle_oracle.py`` against
``R.power_map`` and against known answers (which the GPU tests then hold the kernel to), the host's parameter and memory checks
through a stand-alone g++ program, plain and with sanitizers, ``utils.angular_statistics`` / ``pattern_power``, and the bindings."""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import random_scene, unit_grid
from power_angle_oracle import (AT_RX, AT_TX, BINS_MAX, PowerAngleProfile, bin_of, directed_contributions, fold, origin_turns,
                                power_angle, turns, turns_inputs)

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "power_angle_host.cpp")
GXX = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror"]
# What d2d_angle.hpp's comment and DESIGN.md K3-A record as measured: 0.701 * 2^-24 turn.  The bound is the next round figure
# above it (0.75 <= 1.25 * 0.701).
TURNS_ERROR_BOUND = 0.75  # units of 2^-24 turn


def load_host(so):
    lib = C.CDLL(so)
    fp = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
    lib.pa_turns.argtypes = [C.c_longlong, fp, fp, fp]
    lib.pa_turns.restype = None
    lib.pa_worst_over_q.argtypes = [C.c_uint32, C.c_uint32]
    lib.pa_worst_over_q.restype = C.c_double
    lib.pa_worst_over.argtypes = [C.c_longlong, fp, fp]
    lib.pa_worst_over.restype = C.c_double
    lib.pa_angle_params.argtypes = [C.c_int, C.c_float, C.c_int]
    lib.pa_angle_params.restype = C.c_int
    lib.pa_bytes_per_cell.argtypes = [C.c_int]
    lib.pa_bytes_per_cell.restype = C.c_longlong
    lib.pa_angle_fits.argtypes = [C.c_longlong, C.c_int, C.c_longlong, C.c_longlong]
    lib.pa_angle_fits.restype = C.c_int
    return lib


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """d2d_angle.hpp and d2d_host.hpp's angle checks, compiled for the host (tests/native/power_angle_host.cpp)."""
    so = str(tmp_path_factory.mktemp("pa_host") / "libpa_host.so")
    subprocess.check_call(GXX + ["-shared", "-fPIC", "-o", so, SRC])
    return load_host(so)


def host_turns(host, dx, dy):
    dx, dy = np.ascontiguousarray(dx, F), np.ascontiguousarray(dy, F)
    out = np.empty_like(dx)
    host.pa_turns(dx.size, dx, dy, out)
    return out


def _bits(x):
    return int(np.array(x, F).view(np.uint32))


# ---- the direction header --------------------------------------------------------------------------------------------------------
def test_turns_header_equals_its_numpy_restatement_bit_for_bit(host):
    dx, dy = turns_inputs()
    assert dx.size > 10**6
    got, want = host_turns(host, dx, dy), turns(dx, dy)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and nan.sum() == 15
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~nan
    assert not bad.any(), f"{bad.sum()} of {bad.size} differ, first at ({dx[bad][0]!r}, {dy[bad][0]!r}): {got[bad][0]!r} != {want[bad][0]!r}"
    # in [0, 1), never 1; every octant and both reduction branches are there
    ok = ~nan
    assert (got[ok] >= 0).all() and (got[ok] < 1).all()
    assert set(np.floor(got[ok] * 8).astype(int)) == set(range(8))
    ax, ay = np.abs(dx[ok]), np.abs(dy[ok])
    near = 2 * np.minimum(ax, ay).astype(np.float64) > np.maximum(ax, ay)
    assert 0.3 < near.mean() < 0.5
    # denormals, 1e30 and the largest fp32 took part, and came out finite
    assert (np.maximum(ax, ay) < 1e-38).any() and (np.maximum(ax, ay) >= 1e30).any() and np.isfinite(got[ok]).all()


def test_turns_exact_cases_by_bits(host):
    tiny, fmax = np.nextafter(F(0), F(1)), np.finfo(F).max
    for x in (F(3), F(1), tiny, F(1e-30), F(1e30), fmax):
        for z in (F(0.0), F(-0.0)):
            cases = [((x, z), 0.0), ((z, x), 0.25), ((-x, z), 0.5), ((z, -x), 0.75)]
            for (dx, dy), want in cases:
                for f in (host_turns(host, [dx], [dy])[0], turns([dx], [dy])[0]):
                    assert _bits(f) == _bits(want), (dx, dy, f)
        for (sx, sy), want in (((1, 1), 0.125), ((-1, 1), 0.375), ((-1, -1), 0.625), ((1, -1), 0.875)):
            for f in (host_turns(host, [sx * x], [sy * x])[0], turns([sx * x], [sy * x])[0]):
                assert _bits(f) == _bits(want), (sx, sy, x, f)
    # what would round to 1 is 0; a little further below the axis it is just under 1
    assert _bits(host_turns(host, [1.0], [-tiny])[0]) == 0 and _bits(host_turns(host, [1.0], [-1e-30])[0]) == 0
    assert 0.999 < host_turns(host, [1.0], [-1e-6])[0] < 1.0
    # no direction: NaN
    bad = [(0, 0), (-0.0, 0), (0, -0.0), (np.nan, 1), (1, np.nan), (np.inf, 1), (1, -np.inf), (np.inf, np.inf), (0, np.inf)]
    dx, dy = np.array(bad, F).T
    assert np.isnan(host_turns(host, dx, dy)).all() and np.isnan(turns(dx, dy)).all()


def test_turns_accuracy_against_float64(host):
    """|error| on the circle against float64 atan2 / 2 pi, in units of 2^-24 turn, over 2^24 seeded random directions of all octants
    (magnitudes 1e-6 .. 1e6), every fp32 q = min / max of the binades [1/4, 1/2) and [1/2, 1] -- the two sides of the reduction
    boundary q = 1/2 and the diagonal -- in all eight octants, and the input set of the bit-for-bit test.  The budget: half a unit is
    the last rounding of a result in [1/2, 1); the division and the polynomial's roundings give p a relative error of a few 2^-24
    at p <= 0.074, another 0.2; the polynomial's own error is 0.05.  Measured: 0.701 (random), 0.677 and 0.664 (binades), 0.687."""
    rng = np.random.default_rng(20261019)
    n = 1 << 24
    ang = rng.random(n) * (2 * np.pi)
    mag = 10.0 ** rng.uniform(-6, 6, n)
    dx, dy = (mag * np.cos(ang)).astype(F), (mag * np.sin(ang)).astype(F)
    octants = np.bincount((ang / (np.pi / 4)).astype(int), minlength=8)
    assert (octants > n // 9).all()
    e_random = host.pa_worst_over(n, dx, dy) * 2.0**24
    e_below = host.pa_worst_over_q(_bits(0.25), _bits(0.5) - 1) * 2.0**24
    e_above = host.pa_worst_over_q(_bits(0.5), _bits(1.0)) * 2.0**24
    sx, sy = turns_inputs()
    ok = ~np.isnan(turns(sx, sy))
    e_set = host.pa_worst_over(int(ok.sum()), np.ascontiguousarray(sx[ok]), np.ascontiguousarray(sy[ok])) * 2.0**24
    print(f"turns: max |error| {e_random:.3f} (2^24 random), {e_below:.3f} (q in [1/4, 1/2)), {e_above:.3f} (q in [1/2, 1]), "
          f"{e_set:.3f} (input set), in units of 2^-24 turn")
    assert max(e_random, e_below, e_above, e_set) <= TURNS_ERROR_BOUND
    assert TURNS_ERROR_BOUND * 2.0**-24 < 2.0**-20  # (4096 bins are 2^-12 turn wide)


# ---- the host checks, through ctypes and through the stand-alone program ---------------------------------------------------------
def test_host_checks_through_ctypes(host):
    assert host.pa_angle_params(AT_TX, 0.0, 1) == 0 and host.pa_angle_params(AT_RX, 0.5, BINS_MAX) == 0
    assert host.pa_angle_params(AT_RX, float(np.nextafter(F(1), F(0))), 36) == 0 and host.pa_angle_params(AT_TX, -0.0, 36) == 0
    for end in (-1, 2, 7):
        assert host.pa_angle_params(end, 0.0, 36) == -1, end
    for origin in (1.0, -1e-30, -0.25, 2.5, np.nan, np.inf, -np.inf):
        assert host.pa_angle_params(AT_TX, origin, 36) == -1, origin
    for nbins in (0, -1, BINS_MAX + 1, 1 << 30):
        assert host.pa_angle_params(AT_TX, 0.0, nbins) == -1, nbins
    assert [host.pa_bytes_per_cell(nb) for nb in (1, 36, 4096)] == [8, 148, 16388]
    for free in (0, 1 << 20, 3 << 30, 288 << 30):
        for held in (0, 1 << 16, 5 << 30):
            for nb in (1, 36, 4096):
                edge = (free // 2 + held // 2) // (4 * nb + 4)
                assert host.pa_angle_fits(edge, nb, free, held) == 1 and host.pa_angle_fits(edge + 1, nb, free, held) == 0
    # 4096 bins of 2 * 10^8 cells are 3.3 TB: refused on any device (no quick GPU test could hold such a grid)
    assert host.pa_angle_fits(1024 * 1024, 4096, 200 << 30, 0) == 1 and host.pa_angle_fits(2 * 10**8, 4096, 288 << 30, 0) == 0


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_stand_alone_host_program(tmp_path, sanitize):
    """angle_params, angle_fits (refusals included) and turns in a program of their own; with sanitizers it is the same program,
    linked against the sanitizers' run times by the compiler (nothing is preloaded, nothing is loaded into Python)."""
    exe = str(tmp_path / "pa_host")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(GXX + extra + ["-DPA_MAIN", "-o", exe, SRC])
    done = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(done.stdout)
    assert done.returncode == 0, done.stdout
    assert "0 failures" in done.stdout


# ---- the oracle recipe -----------------------------------------------------------------------------------------------------------
def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("grid_role", ["rx", "tx"])
@pytest.mark.parametrize("approx", [False, True])
def test_recipe_total_and_one_bin_are_the_power_map_and_origin_rolls_the_planes(approx, grid_role):
    from oracle import ref as R

    walls = R.square_scene_with_obstacle_walls()
    fixed = np.array([0.2, 0.2], F)
    X, Y = unit_grid(16, 9)
    kw = dict(min_order=0, max_order=2, approx=approx, function="hard_sigmoid", grid_role=grid_role)
    want = np.asarray(R.power_map(walls, fixed, X, Y, **kw), F)
    assert np.count_nonzero(want) > want.size // 2
    _, T, D = directed_contributions(walls, fixed, X, Y, **kw)
    for end in (AT_TX, AT_RX):
        o = 0 if end == AT_TX else 2
        named = ~np.isnan(turns(D[:, :, o], D[:, :, o + 1]))
        assert (named | (T == 0)).all()  # no contribution of this scene has a zero direction
        out12, total = fold(T, D, end, 0.0, 12)
        assert total.dtype == np.float32 and _same_bits(total.reshape(want.shape), want)
        # one bin: the fused map by bits
        out1, total1 = fold(T, D, end, 0.0, 1)
        assert _same_bits(out1[0], total) and _same_bits(total1, total)
        out1, _ = fold(T, D, end, F(0.7), 1)
        assert _same_bits(out1[0], total)
        # twelve bins: the bins of a cell add up to its total (fp32 summation order: at most 62 terms of 2^-24 each), and more
        # than one bin is in use in most cells
        s = out12.astype(np.float64).sum(axis=0)
        assert (np.abs(s - total) <= 62 * 2.0**-24 * np.abs(out12).astype(np.float64).sum(axis=0)).all()
        assert ((out12 != 0).sum(axis=0) >= 2).mean() > 0.5
        assert (out12 != 0).any(axis=1).sum() >= (6 if end == AT_TX and grid_role == "rx" or end == AT_RX and grid_role == "tx" else 12)
        # eight bins: an origin of one bin width, which fp32 holds exactly, rolls the planes by one
        out8, _ = fold(T, D, end, 0.0, 8)
        rot8, _ = fold(T, D, end, F(0.125), 8)
        assert _same_bits(rot8, np.roll(out8, -1, axis=0)) and not _same_bits(rot8, out8)
    pa = power_angle(walls, fixed, X, Y, AT_RX, 0.0, 12, **kw)
    assert isinstance(pa, PowerAngleProfile) and pa.bins.shape == (12, 9, 16) and pa.total.shape == (9, 16)


@pytest.mark.parametrize("grid_role", ["rx", "tx"])
def test_recipe_on_the_line_of_sight_alone(grid_role):
    """Orders 0..0 in the empty square: one path per cell, and its direction is the straight line between the two end points --
    known in float64.  AT_TX sees the receiver, AT_RX the transmitter, whichever of them the cells are."""
    from oracle import ref as R

    walls = R.square_scene_walls()
    fixed = np.array([0.3, 0.4], F)
    X, Y = unit_grid(9, 9)
    nbins = 12
    cx, cy = X.astype(np.float64) - float(fixed[0]), Y.astype(np.float64) - float(fixed[1])  # fixed -> cell
    for end in (AT_TX, AT_RX):
        pa = power_angle(walls, fixed, X, Y, end, 0.0, nbins, min_order=0, max_order=0, grid_role=grid_role)
        lit = pa.total != 0
        assert lit.sum() >= 49
        # the terminal the direction is taken at looks towards the other one
        from_fixed = (end == AT_TX) == (grid_role == "rx")
        f = np.mod(np.arctan2(cy if from_fixed else -cy, cx if from_fixed else -cx) / (2 * np.pi), 1.0)
        edge = np.abs(f * nbins - np.round(f * nbins))
        assert (edge[lit] > 1e-4).all()  # (no cell of this grid sits on a bin edge: the float64 bin is the bin)
        b = np.floor(f * nbins).astype(int)
        want = np.zeros_like(pa.bins)
        np.put_along_axis(want, b[None], pa.total[None], axis=0)
        assert _same_bits(pa.bins, want) and len(np.unique(b[lit])) == nbins


def test_recipe_drops_a_zero_direction_from_the_bins_only():
    """The cell that IS the fixed end point: its line of sight has no direction, (0, 0) -- total has the contribution, no bin does."""
    from oracle import ref as R

    walls = R.square_scene_walls()
    fixed = np.array([0.5, 0.5], F)
    X, Y = unit_grid(9, 9)
    pa = power_angle(walls, fixed, X, Y, AT_RX, 0.0, 1, min_order=0, max_order=1)
    differ = pa.bins[0].view(np.uint32) != pa.total.view(np.uint32)
    assert differ.sum() == 1 and differ[4, 4] and pa.total[4, 4] > pa.bins[0][4, 4] > 0


def test_bin_of_follows_the_definition_at_its_edges():
    # the last fp32 below 1 with 4096 bins; g + 1 rounding to 1.0 lands in the last bin; NaN names none
    f = np.array([0.0, np.nextafter(F(1), F(0)), 0.25, np.nextafter(F(0.25), F(0)), np.nan, 1e-9], F)
    b, named = bin_of(f, 0.0, 4096)
    assert b.tolist() == [0, 4095, 1024, 1023, 0, 0] and named.tolist() == [True, True, True, True, False, True]
    b, named = bin_of(f, F(0.25), 4)
    assert b.tolist() == [3, 2, 0, 3, 0, 3] and named[5]
    assert F(F(1e-9) - F(0.25)) + F(1) == F(0.75)
    b, _ = bin_of(np.array([1e-9], F), np.nextafter(F(0), F(1)), 7)  # (g = f - origin >= 0: no wrap)
    assert b.tolist() == [0]
    b, _ = bin_of(np.array([0.0], F), F(1e-9), 7)  # g = -1e-9 + 1 rounds to 1.0: u = nbins, clamped to the last bin
    assert b.tolist() == [6]
    assert origin_turns(0.0) == 0 and origin_turns(2 * np.pi) == 0 and origin_turns(-1e-12) == 0 and origin_turns(np.pi) == F(0.5)
    assert origin_turns(-np.pi / 2) == F(0.75) and origin_turns(np.pi / 4).dtype == F and 0 <= origin_turns(123.456) < 1


def test_recipe_with_signed_and_zero_coefficients():
    fixed, walls = random_scene(7, seed=77)
    X, Y = unit_grid(21, 13)
    coef = np.array([0.3, 0.4, -0.7, 0.6, 0.7, 0.5, 0.0], F)  # (tests/test_gpu_strongest_paths.py: COEF7)
    kw = dict(min_order=0, max_order=1, fun="received_power_per_object", fun_kwargs=dict(height=0.25), coef=coef)
    cands, T, D = directed_contributions(walls, fixed, X, Y, **kw)
    ci = [tuple(int(w) for w in c) for c in cands].index((2,))
    assert (T[ci] < 0).any() and not T[[tuple(int(w) for w in c) for c in cands].index((6,))].any()
    out, total = fold(T, D, AT_RX, 0.0, 12)
    assert (out < 0).any() and (out > 0).any()
    assert np.abs(out.astype(np.float64).sum(axis=0) - total).max() <= 8 * 2.0**-24 * np.abs(T).astype(np.float64).sum(axis=0).max()


# ---- utils and bindings ----------------------------------------------------------------------------------------------------------
def test_angular_statistics_and_pattern_power_known_answers():
    from differt2d_amd.utils import AngularStatistics, angular_statistics, pattern_power

    nbins = 8
    bins = np.zeros((nbins, 2, 2), F)
    bins[2, 0, 0] = 3.0                    # one occupied bin
    bins[1, 0, 1] = bins[5, 0, 1] = 2.0    # two equal opposite bins
    bins[0, 1, 0], bins[2, 1, 0] = 1.0, 1.0  # two equal bins a quarter turn apart
    pa = PowerAngleProfile(bins, bins.sum(axis=0))
    st = angular_statistics(pa)
    assert isinstance(st, AngularStatistics) and all(a.dtype == np.float64 and a.shape == (2, 2) for a in st)
    assert np.array_equal(st.power, [[3.0, 4.0], [2.0, 0.0]])
    centre = lambda b: 2 * np.pi * (b + 0.5) / nbins
    assert abs(st.mean[0, 0] - centre(2)) < 1e-12 and st.spread[0, 0] < 1e-7
    assert abs(st.spread[0, 1] - 1.0) < 1e-12
    assert abs(st.mean[1, 0] - centre(1)) < 1e-12 and abs(st.spread[1, 0] - np.sqrt(0.5)) < 1e-12
    assert np.isnan(st.mean[1, 1]) and np.isnan(st.spread[1, 1])
    # the profile's origin moves the centres with it
    st = angular_statistics(pa, origin=np.pi / 3)
    assert abs(np.mod(st.mean[0, 0] - (centre(2) + np.pi / 3) + np.pi, 2 * np.pi) - np.pi) < 1e-12 and st.spread[0, 0] < 1e-7
    # pattern_power: unit gains give the binned power, a one-bin sector gives that bin
    assert np.array_equal(pattern_power(pa, np.ones(nbins)), angular_statistics(pa).power)
    g = np.zeros(nbins)
    g[5] = 0.5
    assert np.array_equal(pattern_power(pa, g), [[0.0, 1.0], [0.0, 0.0]]) and pattern_power(pa, g).dtype == np.float64
    with pytest.raises(ValueError, match="one gain per bin"):
        pattern_power(pa, np.ones(7))


def test_bindings_and_abi_version():
    from differt2d_amd import _lib as L
    from differt2d_amd import utils
    from differt2d_amd.engine import ANGLE_ENDS, Context, PowerAngleProfile as PA
    from differt2d_amd.scene import Scene

    assert L.D2D_ABI_VERSION == 12
    assert (L.D2D_ANGLE_AT_TX, L.D2D_ANGLE_AT_RX) == (AT_TX, AT_RX) == (0, 1) and L.D2D_ANGLE_BINS_MAX == BINS_MAX == 4096
    assert ANGLE_ENDS == {"tx": 0, "rx": 1}
    names = [s[0] for s in L.SYMBOLS]
    assert "d2d_power_angle_launch" in names and "d2d_get_power_angle" in names and "d2d_selftest_angle" in names
    assert callable(Context.power_angle) and callable(Context.launch_power_angle) and callable(Context.get_power_angle)
    assert callable(Context.selftest_angle)
    assert callable(Scene.power_angle_profile_on_receivers_grid) and callable(Scene.power_angle_profile_on_transmitters_grid)
    assert PA._fields == PowerAngleProfile._fields == ("bins", "total")
    assert callable(utils.angular_statistics) and callable(utils.pattern_power)
    header = open(os.path.join(ROOT, "include", "d2d.h")).read()
    assert "#define D2D_ANGLE_AT_TX 0" in header and "#define D2D_ANGLE_AT_RX 1" in header and "#define D2D_ANGLE_BINS_MAX 4096" in header
    assert "#define D2D_ABI_VERSION 12" in header


def test_scene_refuses_a_fun_that_is_not_fused_and_names_the_sparse_route():
    from differt2d_amd import _lib as L
    from differt2d_amd.scene import Scene

    scene = Scene.square_scene_with_obstacle()
    X, Y = unit_grid(4, 3)

    def step(tx, rx, path, objs):
        return (path.length() < 1.0).astype(F)

    for method in (scene.power_angle_profile_on_receivers_grid, scene.power_angle_profile_on_transmitters_grid):
        with pytest.raises(L.D2DUnsupported, match="valid_paths"):
            next(iter(method(X, Y, step, at="rx", nbins=12)))
