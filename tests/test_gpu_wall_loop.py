"""
GPU: the occlusion loop's walk over the wall table and the patch prologue's index arithmetic change speed, never a bit.

* The loop of eval_candidate (hard and hard_sigmoid validity) tests the cached occluder, then walls 0, 1, 2, ... two adjacent
  table rows per trip, the candidate's own walls handled by the trips that hold them.  Scenes of 1 .. 9 walls leave many cells
  lit, so full-length loops run over odd and even tables (the last trip of an odd one has no second wall), the own walls
  include rows 0, N - 2 and N - 1, and later launches start from a cached occluder.  Orders 3 and 4 run the same loop with
  four and five segments.
* The prologue of a patch divides by the patches per grid row and by the region size with a shift or a host-made reciprocal
  (d2d_div.hpp; tests/test_host_div.py proves the arithmetic): ragged grids whose row lengths and region sizes take both paths,
  lists on against lists off, whole patches and patches cut in parts.

Maps are compared bit for bit, NaN positions included, with the C oracle or with the same sweep enumerating every prefix in
whole patches (region_lists = 0, heavy_split = 0).
"""

import functools

import numpy as np
import pytest

from conftest import random_scene, unit_grid

pytestmark = pytest.mark.gpu

F = np.float32
ONE_WAVE = {"split_max_tiles": 0, "sched_min_tiles": 1}
SHAPES = {"default": {}, "one_wave_per_patch": ONE_WAVE}


def _ctx(**opts):
    from differt2d_amd.engine import Context

    c = Context(0)
    for k, v in opts.items():
        c.set_option(k, v)
    return c


def _same(a, b):
    return bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


@functools.lru_cache(maxsize=None)
def _oracle(n_walls, approx, lo, hi):
    from oracle import c_oracle as CO

    tx, walls = random_scene(n_walls, seed=40 + n_walls)
    X, Y = unit_grid(24)
    want = CO.power_map(walls, tx, X, Y, min_order=lo, max_order=hi, approx=approx, function="hard_sigmoid")
    want.setflags(write=False)
    return tx, walls, X, Y, want


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("approx", [False, True])
@pytest.mark.parametrize("n_walls", [1, 2, 3, 4, 5, 8, 9])
def test_pairs_and_padding_against_the_oracle(n_walls, approx, shape):
    from differt2d_amd.engine import make_params

    tx, walls, X, Y, want = _oracle(n_walls, approx, 0, 2)
    # the premise: a lit cell has a valid path, and a valid candidate has run the loop to its end (10 % of the cells with 9
    # walls, over 80 % with one)
    assert (want > 0).mean() > 0.05
    p = make_params(min_order=0, max_order=2, approx=approx, function="hard_sigmoid")
    with _ctx(**SHAPES[shape]) as c:
        c.set_scene(walls)
        got = c.power_map(tx, X, Y, min_order=0, max_order=2, approx=approx, function="hard_sigmoid")
        assert _same(got, want), f"launch 0: {(got != want).sum()} cells differ"
        for i in (1, 2):  # work history, and a cached occluder from the first candidates on
            c.launch(p, tx)
            got = c.get_map()
            assert _same(got, want), f"launch {i}: {(got != want).sum()} cells differ"


@pytest.mark.parametrize("approx", [False, True])
@pytest.mark.parametrize("n_walls", [5, 8])
def test_orders_three_and_four(n_walls, approx):
    tx, walls, X, Y, want = _oracle(n_walls, approx, 3, 4)
    assert np.nanmax(np.abs(want)) > 0
    for opts in SHAPES.values():
        with _ctx(**opts) as c:
            c.set_scene(walls)
            for _ in range(2):
                got = c.power_map(tx, X, Y, min_order=3, max_order=4, approx=approx, function="hard_sigmoid")
                assert _same(got, want), opts


@pytest.mark.parametrize("region_size,region_size_top", [(1, 1), (3, 6), (4, 16), (8, 64)])
@pytest.mark.parametrize("n,m", [(83, 61), (8, 200)])
def test_divisions_on_ragged_grids(n, m, region_size, region_size_top):
    """83 cells per row: 11 patches, 8: one patch -- with regions of 3 and of 1, 4, 8 patches both the reciprocal and the shift
    divide rows and regions; heavy_split = 8 cuts patches from the second launch on."""
    from differt2d_amd.engine import make_params

    tx, walls = random_scene(12, seed=17)
    X, Y = unit_grid(n, m)
    for approx in (False, True):
        kw = dict(min_order=0, max_order=2, approx=approx, function="hard_sigmoid")
        with _ctx(region_lists=0, heavy_split=0, **ONE_WAVE) as off:
            off.set_scene(walls)
            want = off.power_map(tx, X, Y, **kw)
            assert off.debug_region_stats()["leaf_regions"] == 0
        assert np.nanmax(np.abs(want)) > 0
        with _ctx(region_size=region_size, region_size_top=region_size_top, heavy_split=8, **ONE_WAVE) as on:
            on.set_scene(walls)
            got = on.power_map(tx, X, Y, **kw)
            st = on.debug_region_stats()
            tiles_x, tiles_y = -(-n // 8), -(-m // 8)
            assert st["leaf_regions"] == -(-tiles_x // region_size) * -(-tiles_y // region_size), st
            assert st["patches_enumerated"] == 0 and st["regions_not_listed"] == 0, st
            assert _same(got, want), f"{(got != want).sum()} cells differ"
            for i in range(2):
                on.launch(make_params(**kw), tx)
                got = on.get_map()
                st = on.debug_region_stats()
                assert st["patches_enumerated"] == 0 and st["regions_not_listed"] == 0, st
                assert _same(got, want), f"launch {i + 1}: {(got != want).sum()} cells differ"


@pytest.mark.parametrize("approx", [False, True])
@pytest.mark.parametrize("n_walls", [14, 24, 40])
@pytest.mark.parametrize("n,m", [(96, 72), (192, 160)])
def test_cut_patches_take_their_ranks(n, m, n_walls, approx):
    """The parts of a cut patch (the item, part and list indices of fwd_patch; the ranks of sweep_order_listed): one patch cut,
    eight, all of them; four launches, so that the schedule comes from a work history."""
    from differt2d_amd.engine import make_params

    tx, walls = random_scene(n_walls, seed=5 + n_walls)
    X, Y = unit_grid(n, m)
    kw = dict(min_order=0, max_order=2, approx=approx, function="hard_sigmoid")
    with _ctx(region_lists=0, heavy_split=0, **ONE_WAVE) as ref:
        ref.set_scene(walls)
        want = ref.power_map(tx, X, Y, **kw)
    patches = -(-n // 8) * -(-m // 8)
    for cut in (1, 8, patches):
        with _ctx(heavy_split=cut, **ONE_WAVE) as c:
            c.set_scene(walls)
            c.set_grid(X, Y)
            for i in range(4):
                c.launch(make_params(**kw), tx)
                got = c.get_map()
                st = c.debug_region_stats()
                assert st["patches_enumerated"] == 0 and st["regions_not_listed"] == 0, st
                assert _same(got, want), (cut, i)


@pytest.mark.parametrize("approx", [False, True])
def test_cut_patches_with_a_moving_transmitter(approx):
    from differt2d_amd.engine import make_params

    tx, walls = random_scene(24, seed=33)
    X, Y = unit_grid(96, 72)
    txs = [tx, (tx + F([0.017, -0.011])).astype(F), (F([0.8, 0.15]) - tx * F(0.5)).astype(F)]
    kw = dict(min_order=0, max_order=2, approx=approx, function="hard_sigmoid")
    with _ctx(region_lists=0, heavy_split=0, **ONE_WAVE) as ref:
        ref.set_scene(walls)
        want = [ref.power_map(t, X, Y, **kw) for t in txs]
    for cut in (8, 108):
        with _ctx(heavy_split=cut, **ONE_WAVE) as c:
            c.set_scene(walls)
            c.set_grid(X, Y)
            for i in range(9):
                c.launch(make_params(**kw), txs[i % 3])
                got = c.get_map()
                st = c.debug_region_stats()
                assert st["patches_enumerated"] == 0 and st["regions_not_listed"] == 0, st
                assert _same(got, want[i % 3]), (cut, i)
