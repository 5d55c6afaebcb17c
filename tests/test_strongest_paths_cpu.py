"""Host side of the per-cell strongest paths (no GPU): the oracle recipe of ``tests/strongest_paths_oracle.py`` against
``R.power_map`` (which the GPU tests then hold the kernel to) and against geometric known answers, the kernel's insertion
(``d2d_top.hpp``) through a plain g++ build against NumPy's stable sort, ``utils.strongest_share``, and the bindings."""

import numpy as np
import pytest

from conftest import unit_grid
from strongest_paths_oracle import StrongestPaths, contributions, keys_of, strongest_paths, top_k

F = np.float32
MODES = [(False, "hard_sigmoid"), (True, "hard_sigmoid")]


@pytest.mark.parametrize("grid_role", ["rx", "tx"])
@pytest.mark.parametrize("approx,function", MODES)
def test_recipe_total_is_the_power_map_and_all_slots_sum_to_it(approx, function, grid_role):
    from differt2d_amd import _lib as L
    from oracle import ref as R

    walls = R.square_scene_with_obstacle_walls()
    fixed = np.array([0.2, 0.2], F)
    X, Y = unit_grid(16, 9)
    kw = dict(min_order=0, max_order=2, approx=approx, function=function, grid_role=grid_role)
    want = np.asarray(R.power_map(walls, fixed, X, Y, **kw), F)
    cands, T, Rl, total = contributions(walls, fixed, X, Y, **kw)
    sp = top_k(cands, T, Rl, total, 3, X.shape)
    assert sp.total.dtype == np.float32 and sp.total.shape == (9, 16)
    assert np.array_equal(sp.total.view(np.uint32), want.view(np.uint32))
    assert np.count_nonzero(want) > want.size // 2
    assert sp.power.shape == sp.length.shape == sp.order.shape == (3, 9, 16) and sp.cand.shape == (3, 9, 16, 4)
    assert sp.count.max() > L.D2D_TOP_MAX == 8  # (what makes this scene evict in the kernel's eight slots)
    # with k >= count.max() the slots hold every non-zero contribution: their sum is the cell's value up to fp32 summation order
    # -- at most 62 additions per cell (61 candidates + the slots' sum) of non-negative terms, each within 2^-24 relative of the
    # running sum: 62 * 6e-8 = 4e-6 of the cell's own value, hence of the map's maximum (test_power_profile_cpu.py's bound)
    k = int(sp.count.max())
    full = top_k(cands, T, Rl, total, k, X.shape)
    assert np.array_equal((full.order >= 0).sum(axis=0), full.count)
    err = np.abs(full.power.astype(np.float64).sum(0) - want.astype(np.float64)).max()
    assert err <= 4e-6 * float(want.max()), err
    # the cut is a prefix, and the keys never increase
    assert all(np.array_equal(a[:3].view(np.uint32), b.view(np.uint32)) for a, b in zip(full[:4], sp[:4]))
    key = keys_of(full.power).reshape(full.power.shape).astype(np.int64)
    assert (np.diff(key, axis=0) <= 0).all()
    # a k above the number of candidates pads with empty slots
    big = top_k(cands, T, Rl, total, len(cands) + 2, X.shape)
    assert (big.order[-2:] == -1).all() and np.isnan(big.length[-2:]).all() and (big.power[-2:].view(np.uint32) == 0).all()
    assert (big.cand[-2:] == -1).all()


def test_recipe_on_a_clear_square_names_the_line_of_sight():
    """Orders 0-1 in the empty square: with ``received_power`` (decreasing in the length) the strongest path of every lit interior
    cell is the line of sight, the shortest path there is; with ``fun="length"`` slot 0 is the longest path instead."""
    from differt2d_amd.utils import strongest_share
    from oracle import ref as R

    walls = R.square_scene_walls()
    fixed = np.array([0.3, 0.4], F)
    X, Y = unit_grid(9, 9)
    interior = (X > 0) & (X < 1) & (Y > 0) & (Y < 1)  # (a cell ON a wall is hidden by it)
    sp = strongest_paths(walls, fixed, X, Y, 5, min_order=0, max_order=1)
    lit = interior & (sp.count > 0)
    assert lit.sum() == interior.sum() == 49
    assert (sp.order[0][lit] == 0).all() and (sp.cand[0][lit] == -1).all()
    d = np.hypot(X.astype(np.float64) - 0.3, Y.astype(np.float64) - 0.4)
    assert np.abs(sp.length[0][lit] - d[lit]).max() < 1e-6
    assert (sp.count[lit] == 5).all() and (sp.order[1:][:, lit] == 1).all()  # line of sight + one bounce off each wall
    assert (sp.length[0][lit] < sp.length[1:][:, lit].min(axis=0)).all()  # strongest = shortest
    # nothing is cut at k = 5, so the slots carry the whole cell: a share of 1 up to the rounding of five fp32 additions
    share = strongest_share(sp)
    assert np.abs(share[lit] - 1.0).max() <= 5 * 2.0**-24 and np.isnan(share[sp.total == 0]).all()
    one = strongest_share(strongest_paths(walls, fixed, X, Y, 1, min_order=0, max_order=1))
    assert (one[lit] > 0.2).all() and (one[lit] < 1.0).all()  # the line of sight alone: the largest of five terms, not all of them
    lp = strongest_paths(walls, fixed, X, Y, 5, min_order=0, max_order=1, fun="length")
    assert (lp.order[0][lit] == 1).all() and (lp.order[4][lit] == 0).all()
    assert np.array_equal(lp.power[:, lit].view(np.uint32), lp.length[:, lit].view(np.uint32))
    assert np.array_equal(lp.length[0][lit], sp.length[:, lit].max(axis=0)) and np.array_equal(lp.length[4][lit], sp.length[0][lit])


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """d2d_top.hpp, the kernel's insertion, compiled for the host (tests/native/strongest_paths_host.cpp)."""
    import ctypes as C
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = str(tmp_path_factory.mktemp("sp_host") / "libsp_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so,
                           os.path.join(root, "tests", "native", "strongest_paths_host.cpp")])
    lib = C.CDLL(so)
    fp = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
    lib.sp_top_stream.argtypes = [C.c_int, fp, fp, fp, fp, np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")]
    lib.sp_top_stream.restype = C.c_int
    lib.sp_top_slots.restype = C.c_int
    lib.sp_bytes_per_cell.argtypes = [C.c_int]
    lib.sp_bytes_per_cell.restype = C.c_longlong
    lib.sp_top_fits.argtypes = [C.c_longlong, C.c_int, C.c_longlong, C.c_longlong]
    lib.sp_top_fits.restype = C.c_int
    return lib


def test_host_memory_check(host):
    """Outputs above half of the free device memory are refused: a grid that large does not fit a quick GPU test, so the
    function that decides is held to the rule here."""
    for k in range(1, 9):
        per = k * (4 + 4 + 4 + 4 * 4) + 4 + 4  # power, length, order, cand[4] per slot; total and count
        assert host.sp_bytes_per_cell(k) == per
        for free in (0, 1 << 20, 3 << 30, 288 << 30):
            for held in (0, 1 << 16, 5 << 30):
                edge = (free // 2 + held // 2) // per
                assert host.sp_top_fits(edge, k, free, held) == 1
                assert host.sp_top_fits(edge + 1, k, free, held) == 0
    assert host.sp_top_fits(1024 * 1024, 8, 200 << 30, 0) == 1 and host.sp_top_fits(2**31 - 1, 8, 288 << 30, 0) == 0


def test_insertion_header_against_a_stable_sort(host):
    from differt2d_amd import _lib as L

    assert host.sp_top_slots() == L.D2D_TOP_MAX == 8
    rng = np.random.default_rng(11)
    # few magnitudes, so that most streams repeat them; both signs; both zeros; inf and NaN of both signs
    pool = np.array([0.0, -0.0, 0.25, 0.5, 0.5, 1.0, 1.0, 1.0, 2.0, 3.5, 1e-30, np.inf, np.nan], F)
    ties_across_the_cut = np.zeros(9, int)
    streams = 0
    for n in list(range(0, 41)) * 12:
        t = rng.choice(pool, n).astype(F) * rng.choice(np.array([1.0, -1.0], F), n)
        if n and rng.random() < 0.3:
            t[:] = np.abs(t[rng.integers(n)])  # every item the same: order alone decides
        r = rng.random(n).astype(F)
        to, ro, tag = np.zeros(8, F), np.zeros(8, F), np.zeros(8, np.int32)
        count = host.sp_top_stream(n, t, r, to, ro, tag)
        nz = np.flatnonzero(~(t == 0))
        assert count == nz.size
        want = nz[np.argsort(-keys_of(t[nz]).astype(np.int64), kind="stable")]
        for k in range(1, 9):  # the first k slots of the eight are the top k
            w = want[:k]
            assert np.array_equal(tag[: w.size], w), (n, k, t, tag, want)
            assert (tag[w.size:k] == -1).all() and (to[w.size:k].view(np.uint32) == 0).all()
            assert np.array_equal(to[: w.size].view(np.uint32), t[w].view(np.uint32))
            assert np.array_equal(ro[: w.size].view(np.uint32), r[w].view(np.uint32))
            if want.size > k and keys_of(t[want[k - 1 : k]])[0] == keys_of(t[want[k : k + 1]])[0]:
                ties_across_the_cut[k] += 1
                assert tag[k - 1] < want[k]  # the earlier item is the one kept
        streams += 1
    assert streams == 492 and (ties_across_the_cut[1:] > 20).all(), ties_across_the_cut


def test_strongest_share_known_answers():
    from differt2d_amd.utils import strongest_share

    power = np.zeros((3, 2, 2), F)
    power[:, 0, 0] = [0.5, 0.25, 0.0]      # nothing cut: the share is 1
    power[:, 0, 1] = [4.0, 2.0, 1.0]       # total 8: one unit was cut
    power[:, 1, 0] = [-3.0, 2.0, 0.0]      # signs compete by magnitude and cancel in the sum
    total = np.array([[0.75, 8.0], [-1.0, 0.0]], F)
    sp = StrongestPaths(power, np.full((3, 2, 2), np.nan, F), np.full((3, 2, 2, 4), -1, np.int32), np.full((3, 2, 2), -1, np.int32),
                        total, np.array([[2, 4], [2, 0]], np.int32))
    share = strongest_share(sp)
    assert share.dtype == np.float64 and share.shape == (2, 2)
    assert share[0, 0] == 1.0 and share[0, 1] == 0.875 and share[1, 0] == 1.0 and np.isnan(share[1, 1])


def test_bindings_and_abi_version():
    from differt2d_amd import _lib as L
    from differt2d_amd import utils
    from differt2d_amd.engine import Context, StrongestPaths as SP
    from differt2d_amd.scene import Scene

    assert L.D2D_ABI_VERSION == 12
    names = [s[0] for s in L.SYMBOLS]
    assert "d2d_strongest_paths_launch" in names and "d2d_get_strongest_paths" in names
    assert callable(Context.strongest_paths) and callable(Context.launch_strongest_paths) and callable(Context.get_strongest_paths)
    assert callable(Scene.strongest_paths_on_receivers_grid) and callable(Scene.strongest_paths_on_transmitters_grid)
    assert SP._fields == StrongestPaths._fields == ("power", "length", "cand", "order", "total", "count")
    assert callable(utils.strongest_share)


def test_scene_refuses_a_fun_that_is_not_fused_and_names_the_sparse_route():
    from differt2d_amd import _lib as L
    from differt2d_amd.scene import Scene

    scene = Scene.square_scene_with_obstacle()
    X, Y = unit_grid(4, 3)

    def step(tx, rx, path, objs):
        return (path.length() < 1.0).astype(F)

    for method in (scene.strongest_paths_on_receivers_grid, scene.strongest_paths_on_transmitters_grid):
        with pytest.raises(L.D2DUnsupported, match="valid_paths"):
            next(iter(method(X, Y, step, k=3)))
