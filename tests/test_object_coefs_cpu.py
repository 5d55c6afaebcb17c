"""Host side of ``received_power_per_object`` (no GPU): the host function against the closed form, the attribute fallback, the
native tag and its kwargs, the host thresholds' optional coefficient argument, and the two identities that pin the oracle recipe
of ``tests/object_coefs_oracle.py`` (which the GPU tests hold the kernels to)."""

import dataclasses

import numpy as np
import pytest

from conftest import random_scene, unit_grid
from object_coefs_oracle import LibmBackend, coef_map

F = np.float32


@dataclasses.dataclass(frozen=True, eq=False)
class CoatedWall:
    """(stands in for a ``Wall`` subclass: the function reads nothing but ``r_coef``)"""
    r_coef: float = 0.5


class Bare:
    pass


def _paths():
    from differt2d_amd.geometry import Path

    pts = np.array([[0.1, 0.2], [0.4, 0.9], [0.8, 0.3], [0.25, 0.15], [0.6, 0.7]], F)
    return [Path(xys=pts[[0] + list(range(1, k + 1)) + [4]], loss=F(0.0)) for k in range(4)]


@pytest.mark.parametrize("height", [0.1, 0.25])
def test_host_function_is_the_left_fold_over_the_objects(height):
    from differt2d_amd import utils

    coefs = [0.3, 0.7, 0.9]
    for k, path in enumerate(_paths()):
        objs = [CoatedWall(c) for c in coefs[:k]]
        got = utils.received_power_per_object(None, None, path, objs, height=height)
        num = F(1.0)
        for c in coefs[:k]:
            num = F(num * F(c))
        r = path.length()
        want = F(num / (F(height) * F(height) + r * r))
        assert got.dtype == np.float32 and got == want, (k, got, want)
        # all coefficients equal: received_power, bit for bit (orders 0..3)
        same = utils.received_power_per_object(None, None, path, [CoatedWall(0.4)] * k, height=height)
        assert same == utils.received_power(None, None, path, [None] * k, r_coef=0.4, height=height)


def test_objects_without_the_attribute_take_the_keyword():
    from differt2d_amd import utils

    path = _paths()[2]
    got = utils.received_power_per_object(None, None, path, [Bare(), CoatedWall(0.8)], r_coef=0.25)
    want = utils.received_power_per_object(None, None, path, [CoatedWall(0.25), CoatedWall(0.8)])
    assert got == want and got != utils.received_power_per_object(None, None, path, [Bare(), CoatedWall(0.8)])


def test_native_tag_and_kwargs():
    from differt2d_amd import _lib as L
    from differt2d_amd import utils
    from differt2d_amd.engine import FUN_IDS, make_params
    from differt2d_amd.scene import _native_fun

    assert utils.received_power_per_object._d2d_native == "received_power_per_object"
    assert _native_fun(utils.received_power_per_object, (), {}) == ("received_power_per_object", {})
    assert _native_fun(utils.received_power_per_object, (), {"r_coef": 0.3, "height": 0.2}) == (
        "received_power_per_object", {"r_coef": 0.3, "height": 0.2})
    assert _native_fun(utils.received_power_per_object, (), {"colour": 1}) is None
    assert _native_fun(utils.received_power_per_object, (0.3,), {}) is None
    assert FUN_IDS["received_power_per_object"] == L.FUN_RECEIVED_POWER_PER_OBJECT == 5
    assert make_params(fun="received_power_per_object", height=0.2).fun_id == 5
    assert L.D2D_ABI_VERSION == 12


def test_a_callable_that_reads_r_coef_is_not_recognised():
    from differt2d_amd.scene import _native_fun

    def fun(tx, rx, path, objs):
        num = F(1.0)
        for o in objs:
            num = F(num * F(o.r_coef))
        return num / (F(0.01) + path.length() ** 2)

    assert _native_fun(fun, (), {}) is None  # the synthetic probes' objects have no r_coef: left to the host, as before


MODES = [(False, "hard_sigmoid"), (True, "hard_sigmoid")]


@pytest.mark.parametrize("approx,function", MODES)
def test_recipe_with_uniform_coefficients_is_received_power(approx, function):
    from oracle import ref as R

    tx, walls = random_scene(6, seed=5)
    X, Y = unit_grid(16, 9)
    kw = dict(min_order=0, max_order=3, approx=approx, function=function)
    got = coef_map(walls, np.full(6, 0.35, F), tx, X, Y, height=0.25, **kw)
    want = R.power_map(walls, tx, X, Y, fun_kwargs=dict(r_coef=0.35, height=0.25), **kw)
    assert got.dtype == np.float32 and np.array_equal(got, want, equal_nan=True)
    assert np.count_nonzero(got) > got.size // 4
    got_tx = coef_map(walls, np.full(6, 0.35, F), tx, X, Y, height=0.25, grid_role="tx", **kw)
    want_tx = R.power_map(walls, tx, X, Y, fun_kwargs=dict(r_coef=0.35, height=0.25), grid_role="tx", **kw)
    assert np.array_equal(got_tx, want_tx, equal_nan=True)


@pytest.mark.parametrize("approx,function", MODES)
def test_recipe_with_zeroed_walls_is_received_power_without_them(approx, function):
    from oracle import ref as R

    tx, walls = random_scene(12, seed=11)
    X, Y = unit_grid(37, 29)
    coef = np.full(12, 0.6, F)
    coef[[2, 10]] = 0.0
    kw = dict(min_order=0, max_order=2, approx=approx, function=function)
    got = coef_map(walls, coef, tx, X, Y, **kw)
    want = R.power_map(walls, tx, X, Y, fun_kwargs=dict(r_coef=0.6), filter_nodes={2, 10}, **kw)
    assert np.array_equal(got, want, equal_nan=True)
    full = R.power_map(walls, tx, X, Y, fun_kwargs=dict(r_coef=0.6), **kw)
    assert not np.array_equal(full, want)  # (the two walls do carry paths here)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """d2d_host.hpp's share of the feature, compiled for the host (tests/native/object_coefs_host.cpp)."""
    import ctypes as C
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = str(tmp_path_factory.mktemp("oc_host") / "liboc_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-o", so, os.path.join(root, "tests", "native", "object_coefs_host.cpp")])
    return C.CDLL(so)


def _thresholds(host, params, coef=None, allowed=None, grad=False):
    import ctypes as C

    out = np.zeros(4, F)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    host.oc_sweep_thresholds.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    host.oc_sweep_thresholds.restype = None
    host.oc_sweep_thresholds(C.byref(params), int(grad), vp(coef), vp(allowed), 0 if coef is None else coef.size, vp(out))
    return float(out[0]), int(out[1])


def test_host_accepts_the_function_and_bounds_it(host):
    """check_params takes fun_id 5 and still refuses 6, 9 and -1; sweep_thresholds' bound for the sigmoid sweeps is
    log2(max_j |coef_j| ^ k / h^2) over the ALLOWED objects and the launch's orders, and the running sum is monotone exactly when
    every allowed coefficient is >= 0.  Without coefficients: no bound, not monotone (correct, nothing skipped)."""
    import ctypes as C

    from differt2d_amd.engine import make_params

    host.oc_check_params.argtypes = [C.c_void_p]
    p = make_params(fun="received_power_per_object", approx=True, function="sigmoid", min_order=0, max_order=2, height=0.25)
    assert host.oc_check_params(C.byref(p)) == 0
    for bad in (6, 9, -1):
        q = make_params()
        q.fun_id = bad
        assert host.oc_check_params(C.byref(q)) == -4
    l2f, mono = _thresholds(host, p)
    assert l2f > 1e29 and mono == 0
    coef = np.array([0.2, -3.0, 0.5], F)
    h2 = float(F(0.25) * F(0.25))
    # the negative (and largest) coefficient is masked out: bound from 0.5, order 0 dominates, monotone
    l2f, mono = _thresholds(host, p, coef, np.array([1, 0, 1], np.uint8))
    assert mono == 1 and abs(l2f - (np.log2(1.0 / h2) + 1e-3)) < 1e-4
    # every object allowed: |-3|^2 / h^2, not monotone
    l2f, mono = _thresholds(host, p, coef, None)
    assert mono == 0 and abs(l2f - (np.log2(9.0 / h2) + 1e-3)) < 1e-4
    # orders 1..2 only: the bound no longer holds the order-0 term
    p12 = make_params(fun="received_power_per_object", approx=True, function="sigmoid", min_order=1, max_order=2, height=0.25)
    l2f, mono = _thresholds(host, p12, coef, np.array([1, 0, 1], np.uint8))
    assert mono == 1 and abs(l2f - (np.log2(0.5 / h2) + 1e-3)) < 1e-4
    # all-zero coefficients, orders >= 1: fun == 0 throughout
    l2f, mono = _thresholds(host, p12, np.zeros(3, F), None)
    assert mono == 1 and l2f < -1e29
    # the other functions do not look at the extra arguments
    rp = make_params(fun="received_power", approx=True, function="sigmoid", min_order=0, max_order=2, r_coef=0.5, height=0.25)
    assert _thresholds(host, rp, coef, None) == _thresholds(host, rp)


def test_the_oracle_backends_expf_is_the_c_librarys():
    """The sigmoid maps of the GPU tests come from the oracle loop under ``LibmBackend``: its ``exp`` must be libm's expf bit for
    bit (NumPy's own fp32 exp is not), special values included, and must leave every other mode's map alone."""
    import ctypes
    import ctypes.util

    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.expf.restype, libm.expf.argtypes = ctypes.c_float, [ctypes.c_float]
    rng = np.random.default_rng(0)
    x = np.concatenate([(rng.random(5000) * (hi - lo) + lo).astype(F) for lo, hi in ((-104.5, 89.5), (-20, 20), (-1, 1), (-104, -86))]
                       + [np.array([np.inf, -np.inf, 0.0, -0.0, 1e30, -1e30, 88.7228, 88.73, -103.97, -103.98, -104.0], F)])
    want = np.array([libm.expf(float(v)) for v in x], F)
    xp = LibmBackend()
    got = xp.exp(x)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.isnan(xp.exp(np.array([np.nan], F))[0]) and isinstance(xp.exp(F(1.0)), np.float32)
    tx, walls = random_scene(6, seed=5)
    X, Y = unit_grid(16, 9)
    kw = dict(min_order=0, max_order=2, approx=True, function="hard_sigmoid")
    assert np.array_equal(coef_map(walls, np.full(6, 0.4, F), tx, X, Y, xp=xp, **kw), coef_map(walls, np.full(6, 0.4, F), tx, X, Y, **kw))
    # the sigmoid maps of the two backends agree to rounding, not to the bit
    kw["function"] = "sigmoid"
    a, b = coef_map(walls, np.full(6, 0.4, F), tx, X, Y, xp=xp, **kw), coef_map(walls, np.full(6, 0.4, F), tx, X, Y, **kw)
    np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-9)
