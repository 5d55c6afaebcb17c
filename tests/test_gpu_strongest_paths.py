"""The per-cell strongest paths (include/d2d.h: d2d_strongest_paths_launch; power_sink_kernel, TopSink): the k largest contributions
of the fused sweep per cell, with their lengths and wall sequences.  Held bit for bit to the oracle recipe of
``tests/strongest_paths_oracle.py`` (which ``tests/test_strongest_paths_cpu.py`` pins to ``R.power_map``), to the routes that exist
(the fused map, the records of ``d2d_valid_paths``), and to its state rules and refusals."""

import functools

import numpy as np
import pytest

from conftest import random_scene, unit_grid
from strongest_paths_oracle import contributions, keys_of, top_k

pytestmark = pytest.mark.gpu

F = np.float32
MODES = {"hard": dict(approx=False), "hsig": dict(approx=True, function="hard_sigmoid")}
# (of the 7-wall scene's walls only 2, 3 and 6 carry single reflections: the negative and the zero coefficient sit on two of them)
COEF7 = np.array([0.3, 0.4, -0.7, 0.6, 0.7, 0.5, 0.0], F)


@pytest.fixture(scope="module")
def ctx():
    from differt2d_amd.engine import Context

    with Context(0) as c:
        yield c


def _role_id(role):
    from differt2d_amd import _lib as L

    return L.GRID_RX if role == "rx" else L.GRID_TX


@functools.lru_cache(maxsize=None)
def _case(scene):
    """(walls, fixed end point, X, Y)"""
    from oracle import ref as R

    if scene == "random7":  # 21 x 13: partial patches on both sides, 3 x 2 patches
        fixed, walls = random_scene(7, seed=77)
        return walls, fixed, *unit_grid(21, 13)
    if scene == "obstacle":
        return R.square_scene_with_obstacle_walls(), np.array([0.2, 0.2], F), *unit_grid(16, 9)
    if scene == "square_centre":  # the fixed end point on both axes of symmetry: mirrored paths tie bit for bit
        return R.square_scene_walls(), np.array([0.5, 0.5], F), *unit_grid(9, 9)
    raise KeyError(scene)


@functools.lru_cache(maxsize=None)
def _contributions(scene, mode, role, fun, lo=0, hi=2, masked=()):
    walls, fixed, X, Y = _case(scene)
    kw = dict(min_order=lo, max_order=hi, grid_role=role, filter_nodes=set(masked) or None, **MODES[mode])
    if fun == "received_power_per_object":
        kw.update(coef=COEF7, fun_kwargs=dict(height=0.25))
    out = contributions(walls, fixed, X, Y, fun=fun, **kw)
    for a in out[1:]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _oracle(scene, mode, role, fun, k, lo=0, hi=2, masked=()):
    sp = top_k(*_contributions(scene, mode, role, fun, lo, hi, masked), k, _case(scene)[2].shape)
    for a in sp:
        a.setflags(write=False)
    return sp


def _gpu(ctx, scene, mode, role, fun, k, lo=0, hi=2, **extra):
    from differt2d_amd.engine import make_params

    walls, fixed, X, Y = _case(scene)
    ctx.set_scene(walls)
    if fun == "received_power_per_object":
        ctx.set_reflection_coefs(COEF7)
        extra["height"] = 0.25
    ctx.set_grid(X, Y)
    params = make_params(min_order=lo, max_order=hi, fun=fun, grid_role=_role_id(role), **MODES[mode], **extra)
    return ctx.strongest_paths(params, fixed, k), params


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want):
    """power, length and total by bits (NaN lengths of empty slots included); cand, order and count exactly."""
    for name, g, w in zip(want._fields, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, g.shape, w.dtype, w.shape)
        if name == "length":  # (an empty slot's length is a NaN: any NaN will do)
            both_nan = np.isnan(g) & np.isnan(w)
            bad = (_bits(g) != _bits(w)) & ~both_nan
        else:
            bad = _bits(g) != _bits(w)
        assert not bad.any(), f"{name}: {bad.sum()} of {bad.size} entries differ, first at {tuple(np.argwhere(bad)[0])}"


def _cut_ties(sp_more, k):
    """Cells whose k-th and (k+1)-th keys are equal and not empty, from an oracle with more than k slots."""
    key = keys_of(sp_more.power).reshape(sp_more.power.shape)
    return (key[k - 1] == key[k]) & (key[k] != 0)


# ---- 1. bit for bit against the oracle recipe ---------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
@pytest.mark.parametrize("scene", ["random7", "obstacle"])
def test_slots_equal_the_oracle_recipe(ctx, scene, mode, role, k):
    got, _ = _gpu(ctx, scene, mode, role, "received_power", k)
    want = _oracle(scene, mode, role, "received_power", k)
    print(f"{scene} {mode} {role} k={k}: count max {want.count.max()}, {(want.count > k).sum()} of {want.count.size} cells cut")
    # (so that the comparison does not pass on empty ground)
    if scene == "random7":
        assert 1 < want.count.max() <= 5  # empty slots at k = 8, evictions at k = 1 and 3
    else:
        assert want.count.max() > 8 and (want.count > 8).sum() > 80  # k = 8 and k = 3 both evict
    _same(got, want)


# ---- 2. ties --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 8])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
def test_ties_across_the_cut_keep_the_earlier_candidate(ctx, mode, k):
    """The square with the fixed end point at its centre, orders 0-3 (the MAXK = 3 instance): mirrored paths have the same bits."""
    want = _oracle("square_centre", mode, "rx", "received_power", k, 0, 3)
    ties = _cut_ties(_oracle("square_centre", mode, "rx", "received_power", k + 1, 0, 3), k)
    print(f"{mode} k={k}: {ties.sum()} cells tie across the cut")
    assert ties.sum() >= 1
    got, _ = _gpu(ctx, "square_centre", mode, "rx", "received_power", k, 0, 3)
    _same(got, want)


@pytest.mark.parametrize("k", [3, 8])
def test_all_keys_tie_with_fun_one_in_hard_mode(ctx, k):
    """``fun="one"``, hard validity: every contribution is 1.0, so the slots are the first k valid candidates in enumeration order."""
    cands, T, _, _ = _contributions("square_centre", "hard", "rx", "one", 0, 3)
    assert set(np.unique(T)) == {F(0.0), F(1.0)}
    want = _oracle("square_centre", "hard", "rx", "one", k, 0, 3)
    got, _ = _gpu(ctx, "square_centre", "hard", "rx", "one", k, 0, 3)
    _same(got, want)
    cells = T.shape[1]
    first = np.full((k, cells, 4), -1, np.int32)
    for c in range(cells):
        for s, ci in enumerate(np.flatnonzero(T[:, c])[:k]):
            first[s, c, : len(cands[ci])] = cands[ci]
    assert np.array_equal(got.cand.reshape(k, cells, 4), first)
    assert (got.count > k).any()


# ---- 3. sign and zeros -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
def test_negative_contributions_compete_by_magnitude_and_zeros_take_no_slot(ctx, mode, role):
    want = _oracle("random7", mode, role, "received_power_per_object", 3)
    assert (want.power < 0).any() and (want.power > 0).any()
    # contributions through the zero coefficient (wall 6) are exact zeros: no slot, not counted
    cands, T, _, _ = _contributions("random7", mode, role, "received_power_per_object")
    _, T_one, _, _ = _contributions("random7", mode, role, "one")
    through6 = np.array([6 in c for c in cands])
    assert (T_one[through6] != 0).any() and (T[through6] == 0).all()
    assert np.array_equal(want.count, (T[~through6] != 0).sum(axis=0).reshape(want.count.shape))
    assert not (want.cand == 6).any()
    try:
        got, _ = _gpu(ctx, "random7", mode, role, "received_power_per_object", 3)
    finally:
        ctx.set_reflection_coefs(None)
    _same(got, want)


# ---- 4. the candidate mask -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("role", ["rx", "tx"])
def test_slots_honour_the_candidate_mask(ctx, role):
    from differt2d_amd.engine import make_params

    walls, fixed, X, Y = _case("random7")
    allowed = np.ones(7, np.uint8)
    allowed[[2, 5]] = 0
    ctx.set_scene(walls)
    ctx.set_candidate_mask(allowed)
    try:
        ctx.set_grid(X, Y)
        got = ctx.strongest_paths(make_params(min_order=0, max_order=2, grid_role=_role_id(role)), fixed, 3)
    finally:
        ctx.set_candidate_mask(None)
    _same(got, _oracle("random7", "hard", role, "received_power", 3, 0, 2, (2, 5)))
    assert not np.array_equal(got.cand, _oracle("random7", "hard", role, "received_power", 3).cand)
    assert not np.isin(got.cand, [2, 5]).any()


# ---- 5. against the routes that exist --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("scene", ["random7", "obstacle"])
def test_against_the_fused_map_and_the_records(ctx, scene, role):
    from oracle import ref as R

    walls, fixed, X, Y = _case(scene)
    got, params = _gpu(ctx, scene, "hsig", role, "one", 8)
    ctx.launch(params, fixed)
    fused = ctx.get_map()
    assert np.array_equal(got.total.view(np.uint32), fused.view(np.uint32)) and np.count_nonzero(fused) > fused.size // 4
    rec = ctx.valid_paths(params, fixed)
    cells = X.size
    assert np.array_equal(got.count.reshape(-1), np.bincount(rec["cell"], minlength=cells))
    # every cell's slots are its records ordered by (key descending, enumeration rank)
    rank_of = {tuple(int(w) for w in c): i for i, c in enumerate(R.all_path_candidates(len(walls), 0, 2))}
    rank = np.array([rank_of[tuple(int(w) for w in c[:o])] for c, o in zip(rec["cand"], rec["order"])], np.int64)
    key = keys_of(rec["valid"]).astype(np.int64)
    by = np.lexsort((rank, -key, rec["cell"]))
    cell_s = rec["cell"][by]
    slot = np.arange(by.size) - np.searchsorted(cell_s, cell_s, side="left")
    keep = slot < 8
    want_p = np.zeros((8, cells), F)
    want_l = np.full((8, cells), np.nan, F)
    want_c = np.full((8, cells, 4), -1, np.int32)
    want_o = np.full((8, cells), -1, np.int32)
    at = (slot[keep], cell_s[keep])
    want_p[at] = rec["valid"][by][keep]
    want_l[at] = rec["length"][by][keep]
    want_c[at] = rec["cand"][by][keep]
    want_o[at] = rec["order"][by][keep]
    assert np.array_equal(got.power.reshape(8, cells).view(np.uint32), want_p.view(np.uint32))
    assert np.array_equal(got.order.reshape(8, cells), want_o) and np.array_equal(got.cand.reshape(8, cells, 4), want_c)
    full = want_o >= 0
    assert np.array_equal(got.length.reshape(8, cells)[full].view(np.uint32), want_l[full].view(np.uint32))
    assert np.isnan(got.length.reshape(8, cells)[~full]).all()
    # the keys within a cell's slots never increase
    k8 = keys_of(got.power).reshape(8, cells).astype(np.int64)
    assert (np.diff(k8, axis=0) <= 0).all()
    if scene == "obstacle":
        assert (got.count > 8).any()
    assert len(np.unique(rec["valid"])) > 2  # (hard_sigmoid: keys that differ, not only ties)


# ---- 6. state --------------------------------------------------------------------------------------------------------------------
def test_launch_leaves_the_other_results_alone_and_repeats_itself(ctx):
    from differt2d_amd.engine import make_params

    walls, fixed, X, Y = _case("random7")
    ctx.set_scene(walls)
    ctx.set_grid(X, Y)
    fused_params = make_params(min_order=0, max_order=2, fun="length")
    ctx.launch(fused_params, fixed)
    before = ctx.get_map()
    top_params = make_params(min_order=0, max_order=2, **MODES["hsig"])
    profile = ctx.power_profile(top_params, fixed, 0.0, 3.0, 24)
    rec = ctx.valid_paths(top_params, fixed)
    s8 = ctx.strongest_paths(top_params, fixed, 8)
    assert np.array_equal(ctx.get_map().view(np.uint32), before.view(np.uint32))  # the value map is still the previous sweep's
    assert np.array_equal(ctx.get_profile(24).view(np.uint32), profile.view(np.uint32)) and profile.any()
    n = len(rec["cell"])
    again = {"cell": np.empty(n, np.int32), "valid": np.empty(n, F), "length": np.empty(n, F)}
    vp = lambda a: a.ctypes.data
    assert ctx._lib.d2d_get_valid_paths(ctx._ctx, n, vp(again["cell"]), None, None, None, None, vp(again["valid"]), vp(again["length"])) == 0
    assert n > 0 and all(np.array_equal(again[f].view(np.uint32), rec[f].view(np.uint32)) for f in again)
    _same(ctx.strongest_paths(top_params, fixed, 8), s8)  # two launches give the same bits
    assert s8.power.any() and before.any()
    # k = 2 after k = 8 on the same context: the first two slots of the former
    s2 = ctx.strongest_paths(top_params, fixed, 2)
    _same(s2, type(s8)(s8.power[:2], s8.length[:2], s8.cand[:2], s8.order[:2], s8.total, s8.count))
    ctx.launch(fused_params, fixed)
    assert np.array_equal(ctx.get_map().view(np.uint32), before.view(np.uint32))
    # another grid size on the same context: partial patches on the other side, more patches
    X2, Y2 = unit_grid(35, 18)
    ctx.set_grid(X2, Y2)
    with pytest.raises(Exception) as e:  # set_grid of another grid drops the result
        ctx.get_strongest_paths()
    assert getattr(e.value, "status", None) == -5
    q = ctx.strongest_paths(top_params, fixed, 4)
    ctx.launch(top_params, fixed)
    assert q.power.shape == (4, 18, 35) and q.cand.shape == (4, 18, 35, 4)
    assert np.array_equal(q.total.view(np.uint32), ctx.get_map().view(np.uint32))
    cands, T, Rl, total = contributions(walls, fixed, X2, Y2, min_order=0, max_order=2, **MODES["hsig"])
    _same(q, top_k(cands, T, Rl, total, 4, X2.shape))


# ---- 7. loud edges ---------------------------------------------------------------------------------------------------------------
def _nothing_to_get(ctx):
    bufs = [np.zeros((8,) + tuple(ctx.shape) + tail, dt) for tail, dt in (((), F), ((), F), ((4,), np.int32), ((), np.int32))]
    bufs += [np.zeros(ctx.shape, F), np.zeros(ctx.shape, np.int32)]
    rc = ctx._lib.d2d_get_strongest_paths(ctx._ctx, *(b.ctypes.data for b in bufs))
    return rc == -5 and b"d2d_strongest_paths_launch" in ctx._lib.d2d_last_error()


def _refused(ctx, status, word, params, fixed, k=3):
    from differt2d_amd import _lib as L

    with pytest.raises(L.D2DError, match=word) as e:
        ctx.strongest_paths(params, fixed, k)
    assert e.value.status == status, (e.value.status, str(e.value))
    assert isinstance(e.value, L.D2DUnsupported) == (status == -4)
    assert "d2d_strongest_paths_launch" in str(e.value) or status == -5
    assert _nothing_to_get(ctx)  # ... and a refused launch leaves nothing to get


def test_loud_edges(ctx):
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import make_params

    walls, fixed, X, Y = _case("random7")
    ctx.set_scene(walls)
    ctx.set_reflection_coefs(None)
    ctx.set_grid(*unit_grid(19, 11))  # a grid this context has not seen: no result yet
    ctx.set_grid(X, Y)
    assert _nothing_to_get(ctx)
    kw = dict(min_order=0, max_order=2)
    n0 = ctx.txg_fallbacks()
    _refused(ctx, -4, "sigmoid", make_params(approx=True, function="sigmoid", **kw), fixed)
    _refused(ctx, -4, "MinPath / FermatPath", make_params(solver="min", **kw), fixed)
    _refused(ctx, -4, "MinPath / FermatPath", make_params(solver="fermat", **kw), fixed)
    _refused(ctx, -4, "D2D_FUN_CUSTOM", make_params(fun="custom", **kw), fixed)
    _refused(ctx, -4, "D2D_OUT_ADD", make_params(out_mode=L.OUT_ADD, **kw), fixed)
    # a TX grid whose sweep is not culled: refused, and not counted as a fall-back
    _refused(ctx, -4, "not culled", make_params(grid_role=L.GRID_TX, tol=0.6, **kw), fixed)
    ctx.set_option("txg_exhaustive", 1)
    try:
        _refused(ctx, -4, "txg_exhaustive", make_params(grid_role=L.GRID_TX, **kw), fixed)
    finally:
        ctx.set_option("txg_exhaustive", 0)
    # the per-object function: D2D_ERR_STATE without coefficients, works with them
    per_object = make_params(fun="received_power_per_object", **kw)
    _refused(ctx, -5, "d2d_set_reflection_coefs", per_object, fixed)
    ctx.set_reflection_coefs(COEF7)
    assert ctx.strongest_paths(per_object, fixed, 3).power.any()
    ctx.set_reflection_coefs(None)
    # k
    ok = make_params(**kw)
    for k in (0, 9, -1):
        _refused(ctx, -1, "D2D_TOP_MAX", ok, fixed, k=k)
    assert ctx.txg_fallbacks() == n0
    # ... after all of which the context still works, and the grid's change drops the result
    assert ctx.strongest_paths(ok, fixed, 8).power.any()
    assert not _nothing_to_get(ctx)
    ctx.set_grid(*unit_grid(19, 11))
    assert _nothing_to_get(ctx)


def test_more_objects_than_the_codes_hold(ctx):
    """4 096 objects exceed the 12-bit wall indices.  (The last refusal, outputs above half of the free device memory, needs a grid
    of over 10^8 cells: tests/test_strongest_paths_cpu.py holds the host function that decides it to the rule instead.)"""
    from differt2d_amd.engine import make_params

    rng = np.random.default_rng(5)
    many = rng.random((4096, 2, 2)).astype(F)
    fixed = np.array([0.5, 0.5], F)
    ctx.set_scene(many)
    ctx.set_grid(*unit_grid(9, 9))
    _refused(ctx, -4, "4096 objects", make_params(min_order=0, max_order=1), fixed)
    walls = _case("random7")[0]
    ctx.set_scene(walls)
    assert ctx.strongest_paths(make_params(min_order=0, max_order=1), fixed, 2).power.shape == (2, 9, 9)


# ---- 8. the Scene methods --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("role", ["rx", "tx"])
def test_scene_methods_mirror_the_context(ctx, role):
    from differt2d_amd import utils
    from differt2d_amd.engine import StrongestPaths, make_params
    from differt2d_amd.geometry import Point
    from differt2d_amd.scene import Scene

    walls, fixed, X, Y = _case("random7")
    pts = {"a": Point(xy=fixed), "b": Point(xy=(F(1.0) - fixed).astype(F))}
    scene = Scene.from_walls_array(walls)
    scene = scene.with_transmitters(**pts) if role == "rx" else scene.with_receivers(**pts)
    method = scene.strongest_paths_on_receivers_grid if role == "rx" else scene.strongest_paths_on_transmitters_grid
    got = dict(method(X, Y, utils.received_power, dict(r_coef=0.4, height=0.2), k=2, min_order=0, max_order=2, approx=True,
                      function="hard_sigmoid", filter_objects=lambda o: o is not scene.objects[3]))
    assert list(got) == ["a", "b"]
    allowed = np.ones(7, np.uint8)
    allowed[3] = 0
    ctx.set_scene(walls)
    ctx.set_candidate_mask(allowed)
    ctx.set_grid(X, Y)
    params = make_params(min_order=0, max_order=2, r_coef=0.4, height=0.2, grid_role=_role_id(role), **MODES["hsig"])
    for name, pt in pts.items():
        assert isinstance(got[name], StrongestPaths)
        _same(got[name], ctx.strongest_paths(params, pt.xy, 2))
        assert got[name].power.any() and (got[name].count > 2).any() and not (got[name].cand == 3).any()
    ctx.set_candidate_mask(None)
    assert not np.array_equal(got["a"].power, got["b"].power)
    share = utils.strongest_share(got["a"])
    lit = got["a"].total > 0
    # received_power is never negative: the kept slots are part of the cell's terms, so their float64 sum is at most the fp32 total
    # up to its rounding (at most 51 additions of 2^-24 relative each: 4e-6)
    assert lit.any() and (share[lit] > 0).all() and (share[lit] <= 1 + 4e-6).all() and (share[lit] < 0.999).any()
    assert np.isnan(share[got["a"].total == 0]).all()
