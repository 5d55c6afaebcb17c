"""
GPU: the wall loop's segment filters compute every lane and every trip's second wall, and mask afterwards.

The filters of eval_candidate (hard and hard_sigmoid validity) no longer run under the mask of the undecided lanes: a lane the
loop has already decided, a lane outside a ragged grid and a lane whose cell is not finite all compute the K + 1 bilinear forms
of every wall on whatever their registers hold, and one select behind the filter drops their bits.  The wall beside the last
one of an odd table -- a spare row -- is filtered too and dropped by a scalar select.  None of that may reach a result bit:

* lanes of one patch decided at different trips (shadow edges that cross the 8 x 8 patches obliquely),
* lanes that never vote (cells outside a ragged grid; NaN, +inf and 1e19 cells beside lit ones),
* odd tables whose full-length loops reach the trip with the phantom wall, three and four segments per wall,
* the instrumented build, whose counter adds sit inside the filters.

Every map is compared bit for bit, NaN positions included, with the C oracle; three launches per context, so that the later
ones start from a cached occluder and a work history; in whole patches, one wave per patch, without region lists, and with
the cells as transmitters.
"""

import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32
SHAPES = {
    "default": {},
    "one_wave_per_patch": {"split_max_tiles": 0, "sched_min_tiles": 1},
    "no_region_lists": {"region_lists": 0},
    "tx_grid": {},
}
MIXED_SEEDS = {3: 74, 5: 151, 8: 135}    # chosen on the CPU: most patches with lit and dark cells among seeds 0..199
RAGGED_SEEDS = {3: 74, 4: 82, 7: 129}
LIT_SEEDS = {1: 0, 3: 1, 5: 7}           # chosen on the CPU: the most cells lit among seeds 0..11


def _scene(n_walls, seed):
    """Walls of half-length 0.12 .. 0.42 at any angle about a centre in the unit square: long enough to cast shadows over
    many patches, oblique to the grid."""
    r = np.random.default_rng(seed)
    tx = r.random(2, dtype=F)
    mid = r.random((n_walls, 2), dtype=F)
    ang = r.random(n_walls, dtype=F) * F(np.pi)
    half = F(0.12) + F(0.3) * r.random(n_walls, dtype=F)
    d = np.stack([np.cos(ang), np.sin(ang)], -1).astype(F) * half[:, None]
    return tx, np.stack([mid - d, mid + d], 1).astype(F)


def _grid(n, m):
    x = np.linspace(0.0, 1.0, n).astype(F)
    y = np.linspace(0.0, 1.0, m).astype(F)
    X, Y = np.meshgrid(x, y)
    return X.copy(), Y.copy()


def _ctx(**opts):
    from differt2d_amd.engine import Context

    c = Context(0)
    for k, v in opts.items():
        c.set_option(k, v)
    return c


def _same(a, b):
    return bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def _want(walls, fixed, X, Y, shape, **kw):
    from oracle import c_oracle as CO

    want = CO.power_map(walls, fixed, X, Y, grid_role="tx" if shape == "tx_grid" else "rx", function="hard_sigmoid", **kw)
    want.setflags(write=False)
    return want


def _three_launches(walls, fixed, X, Y, want, shape, **kw):
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import make_params

    p = make_params(function="hard_sigmoid", grid_role=L.GRID_TX if shape == "tx_grid" else L.GRID_RX, **kw)
    with _ctx(**SHAPES[shape]) as c:
        c.set_scene(walls)
        c.set_grid(X, Y)
        for i in range(3):
            c.launch(p, fixed)
            got = c.get_map()
            print(f"{shape} launch {i}: {int((~((got == want) | (np.isnan(got) & np.isnan(want)))).sum())} of {got.size} cells differ")
            assert _same(got, want), f"{shape}, launch {i}"


def _patches(a):
    m, n = a.shape
    return [a[i : i + 8, j : j + 8] for i in range(0, m, 8) for j in range(0, n, 8)]


# ---- 1. lanes decided at different trips ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mixed(n_walls, approx, shape):
    tx, walls = _scene(n_walls, MIXED_SEEDS[n_walls])
    X, Y = _grid(72, 40)
    return tx, walls, X, Y, _want(walls, tx, X, Y, shape, min_order=0, max_order=2, approx=approx)


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("approx", [False, True])
@pytest.mark.parametrize("n_walls", sorted(MIXED_SEEDS))
def test_lanes_decided_at_different_trips(n_walls, approx, shape):
    tx, walls, X, Y, want = _mixed(n_walls, approx, shape)
    # the premise: in at least a quarter of the patches some lanes are occluded -- by different walls, at different trips --
    # while others run the loop to its end
    mixed = [bool((p > 0).any() and (p == 0).any()) for p in _patches(want)]
    assert 4 * sum(mixed) >= len(mixed), (sum(mixed), len(mixed))
    _three_launches(walls, tx, X, Y, want, shape, min_order=0, max_order=2, approx=approx)


# ---- 2. lanes that never vote --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ragged(n, m, n_walls, approx, shape):
    tx, walls = _scene(n_walls, RAGGED_SEEDS[n_walls])
    X, Y = _grid(n, m)
    kw = dict(min_order=0, max_order=2, approx=approx)
    clean = _want(walls, tx, X, Y, shape, **kw)
    # the last patch in reading order that has lanes outside the grid and at least six lit cells: three of its cells stop
    # being finite (or sane), three or more stay lit
    spots = [(i, j) for i in range(0, m, 8) for j in range(0, n, 8)
             if (i + 8 > m or j + 8 > n) and (clean[i : i + 8, j : j + 8] > 0).sum() >= 6]
    assert spots, "no ragged patch with lit cells"
    i, j = spots[-1]
    cells = [(i + a, j + b) for a in range(min(8, m - i)) for b in range(min(8, n - j)) if clean[i + a, j + b] > 0]
    (a0, b0), (a1, b1), (a2, b2) = cells[0], cells[len(cells) // 2], cells[-1]
    X[a0, b0] = np.nan
    Y[a1, b1] = np.inf
    X[a2, b2] = 1e19
    want = _want(walls, tx, X, Y, shape, **kw)
    return tx, walls, X, Y, want, (i, j)


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("approx", [False, True])
@pytest.mark.parametrize("n_walls", sorted(RAGGED_SEEDS))
@pytest.mark.parametrize("n,m", [(27, 13), (20, 12)])
def test_lanes_that_never_vote(n, m, n_walls, approx, shape):
    tx, walls, X, Y, want, (i, j) = _ragged(n, m, n_walls, approx, shape)
    patch = want[i : i + 8, j : j + 8]
    # the premise: lanes outside the grid, cells that are not finite and lit cells share one patch
    assert patch.size < 64 and (patch > 0).any() and not np.isfinite(X[i : i + 8, j : j + 8]).all()
    _three_launches(walls, tx, X, Y, want, shape, min_order=0, max_order=2, approx=approx)


# ---- 3. odd tables: the phantom second wall of the last trip -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _odd(n_walls, max_order, approx, shape):
    tx, walls = _scene(n_walls, LIT_SEEDS[n_walls])
    X, Y = _grid(40, 24)
    return tx, walls, X, Y, _want(walls, tx, X, Y, shape, min_order=0, max_order=max_order, approx=approx)


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("approx", [False, True])
@pytest.mark.parametrize("max_order", [2, 3])
@pytest.mark.parametrize("n_walls", sorted(LIT_SEEDS))
def test_odd_table_phantom_wall(n_walls, max_order, approx, shape):
    tx, walls, X, Y, want = _odd(n_walls, max_order, approx, shape)
    # the premise: a lit cell has a valid path, whose loop ran over the whole table and met the trip without a second wall
    assert (want > 0).mean() > 0.5
    _three_launches(walls, tx, X, Y, want, shape, min_order=0, max_order=max_order, approx=approx)


# ---- 4. the instrumented build -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("approx", [False, True])
@pytest.mark.parametrize("n_walls", sorted(MIXED_SEEDS))
def test_instrumented_build_computes_the_same_map(n_walls, approx):
    from differt2d_amd.engine import make_params

    tx, walls, X, Y, want = _mixed(n_walls, approx, "default")
    p = make_params(min_order=0, max_order=2, approx=approx, function="hard_sigmoid")
    with _ctx() as c:
        c.set_scene(walls)
        c.set_grid(X, Y)
        c.launch(p, tx)
        product = c.get_map().copy()
        st = c.launch_stats(p, tx)
        counted = c.get_map()
    assert st[0] > 0 and st[4] > 0
    assert _same(counted, product) and _same(product, want)
