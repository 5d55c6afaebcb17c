"""Scenes, grids and oracle-side conditions of ``tests/test_gpu_irregular_grids.py``: grids that are no axis-aligned mesh.

``include/d2d.h`` takes a row-major ``[m][n]`` grid of ANY coordinates; on a ``np.meshgrid`` the corner lanes of a patch and the
corner cells of a region are the extremes of their boxes, neighbouring patches have disjoint boxes of positive extent, rows are
monotone and no two cells coincide.  The families here break each of these in turn (``FAMILIES``).  Scene R is the room with clutter
of ``test_shared_geometry_serves_the_bits_of_the_loop_cpu``; the lattice scenes L3, L5, L6, L8 are the recipe of
``test_lattice_scenes_against_the_c_gradient_oracle`` at 7 walls on a 33 x 21 mesh, and supply NaN gradients on lines that a
scrambled grid scatters over unrelated patches.

Every oracle is per cell, so none is restated; ``oracle_vg`` and ``oracle_forward`` compute each reference once per session and
hand it out read-only.  ``conditions`` asserts on the oracle alone that a comparison cannot pass on empty ground."""

import functools

import numpy as np

import many_walls_cases as MW
from conftest import unit_grid

F = np.float32
MODES = {"hard": dict(approx=False, function="hard_sigmoid"), "hsig": dict(approx=True, function="hard_sigmoid"),
         "sigmoid": dict(approx=True, function="sigmoid")}
ROLES = ("rx", "tx")
FAMILIES = ("mesh", "scrambled", "sheared", "polar", "track_row", "track_col", "collapsed", "flipped")
LATTICES = {"L3": 3, "L5": 5, "L6": 6, "L8": 8}
# (scene, grid) pairs of the value + gradient tests
VG_GRIDS = [("R", f) for f in FAMILIES] + [(s, g) for s in LATTICES for g in ("mesh", "scrambled")]
# NaN-gradient cells of the lattice scenes out of 693, (rx hard, rx hsig, tx hard, tx hsig), as measured with the C oracle
LATTICE_NANS = {"L3": (220, 291, 114, 178), "L5": (27, 118, 92, 162), "L6": (131, 587, 215, 669), "L8": (224, 338, 395, 449)}
SCRAMBLE_SEED = 5


@functools.lru_cache(maxsize=None)
def scene(name):
    """``(fixed end point, walls)``, read-only."""
    if name == "R":
        fixed, walls = MW.room_with_clutter(14, 9, 0.3, (1, 4, 8, 12, 13))
    else:
        rng = np.random.default_rng(LATTICES[name])
        walls = (np.round(rng.random((7, 2, 2)) * 4) / 4).astype(F)
        walls[(walls[:, 0] == walls[:, 1]).all(-1)] += F(0.125)
        fixed = (np.round(rng.random(2) * 8) / 8).astype(F)
    fixed, walls = np.ascontiguousarray(fixed, F), np.ascontiguousarray(walls, F)
    fixed.setflags(write=False)
    walls.setflags(write=False)
    return fixed, walls


def _mesh(name):
    if name == "R":
        return unit_grid(43, 29)  # 29 rows, 43 columns: 4 x 6 patches, ragged on both sides
    xs = np.linspace(0, 1, 33).astype(F)
    return np.meshgrid(xs, xs[:21])


def permutation(n):
    """The scramble of an ``n``-cell grid: ``scrambled.reshape(-1) == mesh.reshape(-1)[permutation(n)]``."""
    return np.random.default_rng(SCRAMBLE_SEED).permutation(n)


def warp(X, Y, family, fixed=None):
    """``(X, Y)`` of a family from the mesh ``X, Y`` (``polar`` and the tracks keep only its shape)."""
    X, Y = np.asarray(X, F), np.asarray(Y, F)
    if family == "mesh":
        x, y = X, Y
    elif family == "scrambled":
        p = permutation(X.size)
        x, y = X.reshape(-1)[p].reshape(X.shape), Y.reshape(-1)[p].reshape(Y.shape)
    elif family == "sheared":
        u, v = X.astype(np.float64) - 0.5, Y.astype(np.float64) - 0.5
        c, s = np.cos(np.pi / 6), np.sin(np.pi / 6)
        x, y = 0.5 + 0.8 * (c * u - s * v + 0.3 * v), 0.5 + 0.8 * (s * u + c * v)
    elif family == "polar":
        r, th = np.linspace(0.02, 0.6, X.shape[1])[None, :], np.linspace(0, 2 * np.pi, X.shape[0])[:, None]
        x, y = float(fixed[0]) + r * np.cos(th), float(fixed[1]) + r * np.sin(th)
    elif family in ("track_row", "track_col"):
        p = np.cumsum(np.random.default_rng(9).normal(0, 0.02, (150, 2)), axis=0) + 0.5
        p = np.abs(p)
        p = 1 - np.abs(1 - p)
        shape = (1, 150) if family == "track_row" else (150, 1)
        x, y = p[:, 0].reshape(shape), p[:, 1].reshape(shape)
    elif family == "collapsed":
        x, y = X.copy(), Y.copy()
        x[8:16, :], y[8:16, :] = X[11, 13], Y[11, 13]
    elif family == "flipped":
        x, y = X[::-1, ::-1], Y[::-1, ::-1]
    else:
        raise KeyError(family)
    return np.ascontiguousarray(x, F), np.ascontiguousarray(y, F)


@functools.lru_cache(maxsize=None)
def grid(scene_name, family):
    """``(X, Y)`` float32, C-contiguous, read-only."""
    X, Y = warp(*_mesh(scene_name), family, scene(scene_name)[0])
    X, Y = X.copy(), Y.copy()  # (own their memory: read-only all the way down)
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y


def to_mesh_order(a, scene_name, family):
    """What the mesh's result ``a`` (cells on the leading axes) looks like on ``family``'s grid, for the two families that are a
    re-indexing of the mesh."""
    shape = _mesh(scene_name)[0].shape
    a = np.asarray(a)
    if family == "flipped":
        return a[::-1, ::-1]
    assert family == "scrambled"
    return a.reshape((-1,) + a.shape[2:])[permutation(shape[0] * shape[1])].reshape(a.shape)


# ---- the oracles, once per session ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_forward(scene_name, family, mode, role, lo, hi):
    from oracle import c_oracle as CO

    fixed, walls = scene(scene_name)
    X, Y = grid(scene_name, family)
    want = CO.power_map(walls, fixed, X, Y, prune=True, grid_role=role, min_order=lo, max_order=hi, **MODES[mode])
    want.setflags(write=False)
    return want


VG = ("value", "grad", "gabs", "kink", "stable")


@functools.lru_cache(maxsize=None)
def oracle_vg(scene_name, family, mode, role):
    """``dict(value, grad, gabs, kink, stable)`` of ``CO.power_map_grad`` at orders 0..2, ``stable`` by the one-ulp rule of
    ``test_lattice_scenes_against_the_c_gradient_oracle``."""
    from oracle import c_oracle as CO
    from test_gpu_grad import _stable_under_one_ulp

    fixed, walls = scene(scene_name)
    X, Y = grid(scene_name, family)
    kw = dict(min_order=0, max_order=2, **MODES[mode])
    value, grad, gabs, kink = CO.power_map_grad(walls, fixed, X, Y, grid_role=role, with_gabs=True, with_kink=True, **kw)
    stable = _stable_under_one_ulp(walls, fixed, X, Y, value, grad, gabs, role, kw)
    out = dict(zip(VG, (value, grad, gabs, kink, stable)))
    for a in out.values():
        a.setflags(write=False)
    return out


# ---- what must hold of the oracle before any comparison ---------------------------------------------------------------------------
def conditions(scene_name, family, mode, role):
    """Asserts on the oracle alone that no comparison on this (scene, grid, mode, role) passes on empty ground; returns the
    figures for printing."""
    o = oracle_vg(scene_name, family, mode, role)
    value, grad = o["value"], o["grad"]
    nan = np.isnan(grad).any(-1)
    compared = np.isfinite(grad).all(-1) & ~o["kink"] & o["stable"]
    figures = dict(cells=value.size, nan=int(nan.sum()), compared=round(float(compared.mean()), 3), kink=round(float(o["kink"].mean()), 3))
    tag = (scene_name, family, mode, role, figures)
    if scene_name == "R":
        if mode != "sigmoid":
            lit = float((value != 0).mean())
            differs = float((value != oracle_forward("R", family, mode, role, 0, 1)).mean())
            figures.update(lit=round(lit, 3), order2=round(differs, 3))
            assert lit >= 0.7 and differs >= 0.7, tag
            assert np.array_equal(value, oracle_forward("R", family, mode, role, 0, 2), equal_nan=True), tag  # the two C oracles agree
        if family == "polar":
            assert figures["nan"] > 50, tag  # (measured: 129 in every mode and both roles)
        if family in ("mesh", "scrambled", "collapsed", "flipped") and mode != "hard" and role == "rx":
            assert figures["nan"] > 50, tag  # (measured: 86)
        floor = {"hard": 0.85, "hsig": 0.60 if family == "collapsed" else 0.80, "sigmoid": 0.0}[mode]
        assert compared.mean() >= floor, tag
    else:
        assert 20 < figures["nan"] < value.size, tag
        if mode != "sigmoid":
            want = LATTICE_NANS[scene_name][2 * ROLES.index(role) + ("hard", "hsig").index(mode)]
            figures.update(nan_measured=want)
    return figures
