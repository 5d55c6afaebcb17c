"""Host side of the per-cell power-delay profile (no GPU): the oracle recipe of ``tests/power_profile_oracle.py`` against
``R.power_map`` (which the GPU tests then hold the kernel to), ``utils.delay_statistics`` on known answers, the range function of
``d2d_host.hpp`` through a plain g++ build, and the bindings."""

import numpy as np
import pytest

from conftest import random_scene, unit_grid
from power_profile_oracle import bins_inv, profile_map

F = np.float32
MODES = [(False, "hard_sigmoid"), (True, "hard_sigmoid")]


@pytest.mark.parametrize("grid_role", ["rx", "tx"])
@pytest.mark.parametrize("approx,function", MODES)
def test_recipe_with_one_covering_bin_is_the_power_map(approx, function, grid_role):
    from oracle import ref as R

    walls = R.square_scene_with_obstacle_walls()
    fixed = np.array([0.2, 0.2], F)
    X, Y = unit_grid(16, 9)
    kw = dict(min_order=0, max_order=2, approx=approx, function=function, grid_role=grid_role)
    want = R.power_map(walls, fixed, X, Y, **kw)
    one = profile_map(walls, fixed, X, Y, 0.0, 8.0, 1, **kw)
    assert one.dtype == np.float32 and one.shape == (1, 9, 16)
    assert np.array_equal(one[0].view(np.uint32), np.asarray(want, F).view(np.uint32))
    assert np.count_nonzero(want) > want.size // 2
    # 24 bins over [0, 3): the power spreads over (nearly) all of them, and the bins of a cell sum to its fused value up to
    # fp32 summation order: at most 62 additions per cell (61 candidates + the bins' sum) of non-negative terms, each within
    # 2^-24 relative of the running sum -- 62 * 6e-8 = 4e-6 of the cell's own value, hence of the map's maximum
    many = profile_map(walls, fixed, X, Y, 0.0, 3.0, 24, **kw)
    assert np.count_nonzero(many.reshape(24, -1).any(axis=1)) > 12  # (sanity: the range is resolved, not one bin)
    err = np.abs(many.astype(np.float64).sum(0) - want.astype(np.float64)).max()
    assert err <= 4e-6 * float(want.max()), err


def test_recipe_bins_are_half_open_and_drop_what_lies_outside():
    """Order 0 on a clear square: the length is the distance, so the bins can be told from the geometry (eps of path_length:
    1.2e-7, far from any edge used here)."""
    from oracle import ref as R

    walls = R.square_scene_walls()
    fixed = np.array([0.5, 0.5], F)
    X, Y = unit_grid(9, 9)
    d = np.hypot(X.astype(np.float64) - 0.5, Y.astype(np.float64) - 0.5)
    interior = (X > 0) & (X < 1) & (Y > 0) & (Y < 1)  # (a cell ON a wall is hidden by it)
    got = profile_map(walls, fixed, X, Y, 0.1, 0.6, 5, min_order=0, max_order=0, fun="one")
    for b in range(5):
        inside = interior & (d >= 0.1 + 0.1 * b + 1e-5) & (d < 0.1 + 0.1 * (b + 1) - 1e-5)
        assert inside.any()
        assert (got[b][inside] == 1).all()
    far = (d < 0.1 - 1e-5) | (d >= 0.6 + 1e-5)  # the centre cell (shorter than r_min) and the corners (longer than r_max)
    assert far.any() and (got[:, far] == 0).all()
    assert (got.sum(0) <= 1).all() and got.sum() < 81


def test_delay_statistics_known_answers():
    from differt2d_amd.utils import delay_statistics

    nb, lo, hi = 10, 1.0, 6.0
    w = (hi - lo) / nb
    P = np.zeros((nb, 2, 3), F)
    P[4, 0, 0] = 0.25               # one occupied bin
    P[2, 0, 1] = P[7, 0, 1] = 3.0   # two equal bins k = 5 apart
    P[0, 0, 2], P[9, 0, 2] = 1.0, 3.0
    total, mean, rms = delay_statistics(P, (lo, hi))
    assert total.dtype == mean.dtype == rms.dtype == np.float64 and total.shape == (2, 3)
    assert total[0, 0] == 0.25 and abs(mean[0, 0] - (lo + 4.5 * w)) < 1e-14 and abs(rms[0, 0]) < 1e-14
    assert total[0, 1] == 6.0 and abs(mean[0, 1] - (lo + 5.0 * w)) < 1e-14 and abs(rms[0, 1] - 5 * w / 2) < 1e-14
    # weights 1 : 3 at centres c0, c9: mean = c0 + 0.75 * 9 w, variance = 0.25 * 0.75 * (9 w)^2
    assert abs(mean[0, 2] - (lo + 0.5 * w + 0.75 * 9 * w)) < 1e-14 and abs(rms[0, 2] - np.sqrt(0.1875) * 9 * w) < 1e-14
    # empty cells
    assert (total[1] == 0).all() and np.isnan(mean[1]).all() and np.isnan(rms[1]).all()
    # a profile without cell axes, and one bin
    t1, m1, s1 = delay_statistics(np.array([2.0], F), (0.0, 4.0))
    assert t1 == 2.0 and m1 == 2.0 and s1 == 0.0
    with pytest.raises(ValueError):
        delay_statistics(np.float32(1.0), (0.0, 1.0))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """d2d_host.hpp's share of the feature, compiled for the host (tests/native/power_profile_host.cpp)."""
    import ctypes as C
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = str(tmp_path_factory.mktemp("pp_host") / "libpp_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-o", so, os.path.join(root, "tests", "native", "power_profile_host.cpp")])
    lib = C.CDLL(so)
    lib.pp_profile_bins.argtypes = [C.c_float, C.c_float, C.c_int32, C.c_void_p, C.c_char_p, C.c_int]
    lib.pp_profile_bins.restype = C.c_int
    return lib


def _bins(host, r_min, r_max, nbins):
    import ctypes as C

    out = np.zeros(3, F)
    msg = C.create_string_buffer(256)
    rc = host.pp_profile_bins(float(r_min), float(r_max), int(nbins), out.ctypes.data_as(C.c_void_p), msg, 256)
    return rc, out, msg.value.decode()


def test_host_range_function(host):
    rng = np.random.default_rng(7)
    cases = [(0.0, 4.0, 32), (0.0, 3.0, 24), (0.0, 8.0, 1), (0.3, 1.7, 257), (-1.5, 0.25, 7), (1e-3, 1e3, 1000), (0.1, 0.1000001, 3)]
    cases += [(float(a), float(a + b), int(n)) for a, b, n in zip(rng.random(50, F), rng.random(50, F) + F(1e-3), rng.integers(1, 5000, 50))]
    for lo, hi, n in cases:
        rc, out, msg = _bins(host, lo, hi, n)
        assert rc == 0 and msg == "", (lo, hi, n, msg)
        want = bins_inv(lo, hi, n)
        assert out[0].view(np.uint32) == F(lo).view(np.uint32) and out[2] == n
        assert out[1].view(np.uint32) == want.view(np.uint32), (lo, hi, n, out[1], want)
    for lo, hi, n, word in [(0.0, 1.0, 0, "nbins"), (0.0, 1.0, -3, "nbins"), (1.0, 1.0, 4, "r_max > r_min"), (2.0, 1.0, 4, "r_max > r_min"),
                            (np.nan, 1.0, 4, "finite"), (0.0, np.inf, 4, "finite"), (-np.inf, 0.0, 4, "finite"), (0.0, np.nan, 4, "finite")]:
        rc, _, msg = _bins(host, lo, hi, n)
        assert rc == -1 and word in msg, (lo, hi, n, rc, msg)


def test_bindings_and_abi_version():
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import Context
    from differt2d_amd.scene import Scene

    assert L.D2D_ABI_VERSION == 12
    names = [s[0] for s in L.SYMBOLS]
    assert "d2d_power_profile_launch" in names and "d2d_get_power_profile" in names
    assert callable(Context.power_profile)
    assert callable(Scene.power_delay_profile_on_receivers_grid) and callable(Scene.power_delay_profile_on_transmitters_grid)


def test_scene_refuses_a_fun_that_is_not_fused_and_names_the_sparse_route():
    from differt2d_amd import _lib as L
    from differt2d_amd.scene import Scene

    scene = Scene.square_scene_with_obstacle()
    X, Y = unit_grid(4, 3)

    def step(tx, rx, path, objs):
        return (path.length() < 1.0).astype(F)

    with pytest.raises(L.D2DUnsupported, match="valid_paths"):
        next(iter(scene.power_delay_profile_on_receivers_grid(X, Y, step, length_range=(0.0, 4.0), nbins=4)))
