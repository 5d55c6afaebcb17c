"""The sparse emit route: Python path functions on grids too big to trace densely (Scene._emit_grid above EMIT_LIMIT).

Stage 1 is a record build of the culled forward sweep (d2d_valid_paths: one record per (cell, candidate) whose validity is
not exactly zero), stage 2 the paths of the records; the host evaluates `fun` on the records only.  Small scenes hold the
records to the dense trace (d2d_trace_paths) and to the C oracle's count map, and the sparse sweeps to the dense route bit for
bit; the full-size cases -- the ones the dense route refuses -- are held to the fused sweeps."""

import os

import numpy as np
import pytest

from conftest import random_scene, unit_grid

pytestmark = pytest.mark.gpu

F = np.float32
MODES = {"hard": dict(approx=False), "hsig": dict(approx=True, function="hard_sigmoid")}
# (scene walls, seed, min_order, max_order): 12 walls / orders 0-2 = 145 candidates; 6 walls / orders 0-3 = 1 + 6 + 30 + 150
SMALL = [(12, 31, 0, 2), (12, 32, 0, 2), (6, 33, 0, 3)]


@pytest.fixture(scope="module")
def ctx():
    from differt2d_amd.engine import Context

    with Context(0) as c:
        yield c


def _role_id(role):
    from differt2d_amd import _lib as L

    return L.GRID_RX if role == "rx" else L.GRID_TX


# ---- 3. the records against the dense trace and the oracle's count map ------------------------------------------------------
@pytest.mark.parametrize("n_walls,seed,lo,hi", SMALL)
@pytest.mark.parametrize("mode", ["hard", "hsig"])
@pytest.mark.parametrize("role", ["rx", "tx"])
def test_records_equal_the_nonzero_entries_of_the_dense_trace(ctx, role, mode, n_walls, seed, lo, hi):
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import make_params
    from oracle import c_oracle as CO

    fixed, walls = random_scene(n_walls, seed=seed)
    X, Y = unit_grid(64)
    cells = X.size
    cands = L.enumerate_candidates(n_walls, lo, hi)
    ctx.set_scene(walls)
    ctx.set_grid(X, Y)
    rec = ctx.valid_paths(make_params(min_order=lo, max_order=hi, grid_role=_role_id(role), **MODES[mode]), fixed)
    n = rec["cell"].size
    assert rec["cand"].shape == (n, L.D2D_MAX_ORDER) and rec["xys"].shape == (n, L.D2D_MAX_ORDER + 2, 2)

    grid = np.stack([X.reshape(-1), Y.reshape(-1)], -1)
    other = np.broadcast_to(fixed, grid.shape)
    txs, rxs = (other, grid) if role == "rx" else (grid, other)
    dense = ctx.trace_paths(make_params(min_order=0, max_order=L.D2D_MAX_ORDER, **MODES[mode]), txs, rxs, cands)

    rank = L.candidate_rank(rec["cand"], rec["order"], n_walls, None, lo, hi)
    assert rank.min(initial=0) >= 0 and rank.max(initial=0) < len(cands)
    assert np.array_equal(rec["order"], np.array([len(c) for c in cands], np.int32)[rank])
    assert np.all((rec["cell"] >= 0) & (rec["cell"] < cells))
    key = rec["cell"].astype(np.int64) * len(cands) + rank
    assert np.unique(key).size == n, "a (cell, candidate) pair occurs twice"
    want_cell, want_rank = np.nonzero(dense["valid"])
    print(f"{role} {mode} {n_walls} walls orders {lo}-{hi}: {n} records, {want_cell.size} non-zero dense entries of {dense['valid'].size}")
    assert np.array_equal(np.sort(key), want_cell.astype(np.int64) * len(cands) + want_rank), "the records are not exactly the valid != 0 set"
    assert n > 0
    # every record's path is the dense trace's entry, bit for bit (NaN rows included)
    for name in ("xys", "loss", "valid", "length"):
        got, want = rec[name], dense[name][rec["cell"], rank]
        assert got.dtype == F and np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
    if mode == "hard":
        _, count = CO.power_and_count_maps(walls, fixed, X, Y, min_order=lo, max_order=hi, grid_role=role, **MODES[mode])
        assert np.array_equal(np.bincount(rec["cell"], minlength=cells).reshape(X.shape), count.astype(np.int64))


def test_record_launch_leaves_the_resident_map_and_honours_the_mask(ctx):
    """d2d_get_map after a record launch still returns the last sweep's map; filtered objects occlude but never interact; a
    second call on the same context replaces the records; min_order > 0."""
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import make_params

    tx, walls = random_scene(12, seed=31)
    X, Y = unit_grid(61, 45)  # sides that are not multiples of 8
    ctx.set_scene(walls)
    ctx.set_grid(X, Y)
    ctx.launch(make_params(min_order=0, max_order=2), tx)
    before = ctx.get_map()
    allowed = np.ones(12, np.uint8)
    allowed[[2, 7]] = 0
    ctx.set_candidate_mask(allowed)
    rec = ctx.valid_paths(make_params(min_order=1, max_order=2, fun="length"), tx)
    assert np.array_equal(ctx.get_map(), before)
    assert rec["order"].min() >= 1 and not np.isin(rec["cand"], [2, 7]).any()
    ctx.launch(make_params(min_order=1, max_order=2, fun="one"), tx)
    assert np.array_equal(np.bincount(rec["cell"], minlength=X.size).reshape(X.shape), ctx.get_map().astype(np.int64))
    rec0 = ctx.valid_paths(make_params(min_order=0, max_order=0), tx)
    assert rec0["order"].max(initial=0) == 0 and np.all(rec0["cand"] == -1) and 0 < rec0["cell"].size <= X.size
    ctx.set_candidate_mask(None)


# ---- 4. the sweeps: sparse route == dense route -----------------------------------------------------------------------------
def _odd_fun(transmitter, receiver, path, interacting_objects, w=0.3):
    """tests/test_gpu_api.py's _odd_fun restated with + - * / sqrt only: the length, both end points, an interior path point."""
    r = path.length()
    dx = receiver.xy[..., 0] - transmitter.xy[..., 0]
    return F(w) * r * np.sqrt(r) + dx * dx + path.xys[..., -2, 0] * receiver.xy[..., 1]


_odd_fun._d2d_native = False


def _gain_and_loss_fun(scene):
    gains = {id(o): F(0.5 + 0.125 * i) for i, o in enumerate(scene.objects)}

    def fun(transmitter, receiver, path, interacting_objects):
        """A per-object gain looked up by identity, and the solver's loss."""
        g = F(1.0)
        for o in interacting_objects:
            g = F(g * gains[id(o)])
        return g / ((F(1.0) + path.length()) * (F(1.0) + path.loss))

    fun._d2d_native = False
    return fun


def _scene(role, n_walls, seed, two=False):
    from differt2d_amd.geometry import Point
    from differt2d_amd.scene import Scene

    p, walls = random_scene(n_walls, seed=seed)
    pts = {"a": Point(xy=p)}
    if two:
        pts["b"] = Point(xy=(F(1.0) - p).astype(F))
    scene = Scene.from_walls_array(walls)
    if role == "rx":
        scene = scene.with_transmitters(**pts)
        return scene, scene.accumulate_on_receivers_grid_over_paths
    scene = scene.with_receivers(**pts)
    return scene, scene.accumulate_on_transmitters_grid_over_paths


@pytest.mark.parametrize("mode", ["hard", "hsig"])
@pytest.mark.parametrize("role", ["rx", "tx"])
def test_sparse_sweeps_equal_the_dense_route_bit_for_bit(monkeypatch, role, mode):
    import differt2d_amd.scene as S

    scene, sweep = _scene(role, 12, 31, two=True)
    X, Y = unit_grid(64)
    Xo, Yo = unit_grid(61, 45)
    not_first = lambda o: o is not scene.objects[0] and o is not scene.objects[5]  # noqa: E731
    cases = [
        (X, Y, _odd_fun, dict(fun_kwargs=dict(w=0.25), reduce_all=True, min_order=0, max_order=2)),
        (X, Y, _gain_and_loss_fun(scene), dict(reduce_all=False, min_order=0, max_order=2)),
        (X, Y, _gain_and_loss_fun(scene), dict(reduce_all=True, min_order=0, max_order=2, filter_objects=not_first)),
        (X, Y, _odd_fun, dict(reduce_all=False, order=2)),
        (Xo, Yo, _odd_fun, dict(reduce_all=True, min_order=0, max_order=2)),
    ]
    for Xc, Yc, fun, kw in cases:
        kw = dict(kw, **MODES[mode])
        monkeypatch.setattr(S, "EMIT_LIMIT", 8_000_000)
        dense = sweep(Xc, Yc, fun=fun, **kw)
        dense = dense if kw["reduce_all"] else list(dense)
        monkeypatch.setattr(S, "EMIT_LIMIT", 0)
        sparse = sweep(Xc, Yc, fun=fun, **kw)
        if kw["reduce_all"]:
            assert sparse.shape == Xc.shape and sparse.dtype == F
            assert np.array_equal(sparse, dense) and np.count_nonzero(dense) > 0
        else:
            sparse = list(sparse)
            assert [k for k, _ in sparse] == [k for k, _ in dense] == ["a", "b"]
            for (_, zs), (_, zd) in zip(sparse, dense):
                assert np.array_equal(zs, zd)
            nonzero = sum(int(np.count_nonzero(zd)) for _, zd in dense)
            print(f"{role} {mode} {sorted(k for k in kw if k != 'fun_kwargs')}: {nonzero} non-zero cells over both fixed points")
            # (second-order paths alone are rare in a 12-wall scene: that case may be all zeros for a fixed point)
            assert nonzero > 0 or kw.get("order") == 2


def test_sparse_sweep_orders_0_to_3(monkeypatch):
    import differt2d_amd.scene as S

    scene, sweep = _scene("rx", 6, 33)
    X, Y = unit_grid(64)
    kw = dict(fun=_gain_and_loss_fun(scene), reduce_all=True, min_order=0, max_order=3, approx=True)
    dense = sweep(X, Y, **kw)
    monkeypatch.setattr(S, "EMIT_LIMIT", 0)
    assert np.array_equal(sweep(X, Y, **kw), dense) and np.count_nonzero(dense) > 0


# ---- 5. full size: what the dense route refuses -----------------------------------------------------------------------------
def _one_host(transmitter, receiver, path, interacting_objects):
    return F(1.0)


_one_host._d2d_native = False


def _power_like(transmitter, receiver, path, interacting_objects, r_coef=0.5, height=0.1):
    """received_power written with operators only (tests/test_gpu_api.py)."""
    r = path.length()
    n = path.xys.shape[-2] - 2
    return (r_coef ** n) / (height * height + r * r)


_power_like._d2d_native = False


def _full_size_checks(sweep, X, Y, mode):
    from differt2d_amd.utils import one, received_power

    kw = dict(reduce_all=True, min_order=0, max_order=2, **MODES[mode])
    fused_one = sweep(X, Y, fun=one, **kw)
    assert np.array_equal(sweep(X, Y, fun=_one_host, **kw), fused_one) and np.count_nonzero(fused_one) > 0
    fused = sweep(X, Y, fun=received_power, **kw)
    host = sweep(X, Y, fun=_power_like, **kw)
    assert np.array_equal(host == 0, fused == 0)
    np.testing.assert_allclose(host, fused, rtol=2e-6, atol=1e-9)


@pytest.mark.parametrize("mode", ["hard", "hsig"])
def test_cfg2_full_size_host_functions(mode):
    """BASELINE.json configs[1]: 50 walls, 1024 x 1024 cells, orders 0..2 = 2.6e9 (cell, candidate) pairs."""
    from differt2d_amd.geometry import Point
    from differt2d_amd.scene import Scene

    tx, walls = random_scene(50, seed=1234)
    x = np.linspace(0.0, 1.0, 1024).astype(F)
    X, Y = np.meshgrid(x, x)
    scene = Scene.from_walls_array(walls).with_transmitters(tx=Point(xy=tx))
    _full_size_checks(scene.accumulate_on_receivers_grid_over_paths, X, Y, mode)


@pytest.mark.parametrize("mode", ["hard", "hsig"])
@pytest.mark.parametrize("role", ["rx", "tx"])
def test_geojson_scene_300x300_host_functions(role, mode):
    """The notebook's scene (28 walls): 90 000 cells x 785 candidates = 70 M pairs."""
    from differt2d_amd.scene import Scene

    scene = Scene.from_geojson(open(os.path.join(os.path.dirname(__file__), "golden", "example.geojson")).read())
    X, Y = scene.grid(300)
    sweep = scene.accumulate_on_receivers_grid_over_paths if role == "rx" else scene.accumulate_on_transmitters_grid_over_paths
    _full_size_checks(sweep, X, Y, mode)


# ---- 6. the edge of the feature stays loud ----------------------------------------------------------------------------------
def test_above_the_limit_the_rest_is_still_refused(monkeypatch):
    import differt2d_amd.scene as S
    from differt2d_amd import _lib as L
    from differt2d_amd import logic
    from differt2d_amd.geometry import MinPath

    scene, sweep = _scene("rx", 6, 33)
    X, Y = unit_grid(16)
    monkeypatch.setattr(S, "EMIT_LIMIT", 0)
    with pytest.raises(L.D2DUnsupported, match="sigmoid"):
        sweep(X, Y, fun=_odd_fun, reduce_all=True, max_order=1, approx=True, function=logic.sigmoid)
    with pytest.raises(L.D2DUnsupported, match="MinPath"):
        sweep(X, Y, fun=_odd_fun, reduce_all=True, max_order=1, path_cls=MinPath, key=np.random.default_rng(0))
    with pytest.raises(L.D2DUnsupported, match="grad"):
        sweep(X, Y, fun=_odd_fun, reduce_all=True, max_order=1, grad=True)
    with pytest.raises(L.D2DUnsupported, match="grad"):
        sweep(X, Y, fun=_odd_fun, reduce_all=True, max_order=1, value_and_grad=True)


def test_the_library_refuses_what_the_record_launch_does_not_cover(ctx):
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import make_params

    tx, walls = random_scene(6, seed=33)
    ctx.set_scene(walls)
    ctx.set_grid(*unit_grid(16))
    with pytest.raises(L.D2DUnsupported):
        ctx.valid_paths(make_params(max_order=1, approx=True, function="sigmoid"), tx)
    with pytest.raises(L.D2DUnsupported):
        ctx.valid_paths(make_params(max_order=1, solver="min"), tx)
    with pytest.raises(L.D2DUnsupported):  # a TX grid whose sweep would fall back to the exhaustive kernel (tol > 0.5, hard)
        ctx.valid_paths(make_params(max_order=1, tol=0.75, grid_role=L.GRID_TX), tx)
    before = ctx.txg_fallbacks()
    with pytest.raises(L.D2DUnsupported):
        ctx.valid_paths(make_params(max_order=1, tol=0.75, grid_role=L.GRID_TX), tx)
    assert ctx.txg_fallbacks() == before


def test_a_refused_record_launch_comes_before_anything_is_enqueued(ctx):
    """A record launch that is refused for a reason its arguments and the context decide -- a TX grid whose sweep is not culled,
    more objects than the kernel's LDS table holds -- returns D2D_ERR_UNSUPPORTED without having built a mask, counted a
    fall-back or touched the resident map.  Both refusals drop the previous records (they always did: the call that replaces
    the records starts by giving them up)."""
    import ctypes as C

    from differt2d_amd import _lib as L
    from differt2d_amd.engine import make_params

    tx, walls = random_scene(6, seed=33)
    ctx.set_scene(walls)
    ctx.set_grid(*unit_grid(16))
    p = make_params(min_order=0, max_order=2)
    ctx.launch(p, tx)
    resident = ctx.get_map()
    assert np.count_nonzero(resident) > 0
    lib, handle, fixed, null = ctx._lib, ctx._ctx, np.ascontiguousarray(tx, F), [None] * 7

    def refused(params, word):
        assert lib.d2d_get_valid_paths(handle, 1 << 20, *null) == 0  # records to lose
        before = (ctx.hidden_masks(), ctx.txg_fallbacks())
        n = C.c_int64(-1)
        assert lib.d2d_valid_paths(handle, C.byref(params), fixed, C.byref(n)) == -4 and n.value == 0
        message = lib.d2d_last_error().decode()
        assert word in message and "d2d_valid_paths" in message
        assert (ctx.hidden_masks(), ctx.txg_fallbacks()) == before
        assert np.array_equal(ctx.get_map(), resident)
        assert lib.d2d_get_valid_paths(handle, 1 << 20, *null) == -5  # the previous records are gone

    assert ctx.valid_paths(p, tx)["cell"].size > 0
    ctx.set_option("txg_exhaustive", 1)
    try:
        refused(make_params(min_order=0, max_order=2, grid_role=L.GRID_TX), "txg_exhaustive")
    finally:
        ctx.set_option("txg_exhaustive", 0)
    # 2600 walls: (4 * 2600 + 1) * 16 + 512 bytes of tables and queue, above the CU's 160 KB (the records of the small scene are
    # still held when the call comes: they go with the grid, not with the scene)
    assert ctx.valid_paths(p, tx)["cell"].size > 0
    ctx.set_scene(random_scene(2600, seed=34)[1])
    refused(make_params(min_order=0, max_order=1), "LDS")
