"""The host half of the sparse emit route (Scene._emit_grid above EMIT_LIMIT), without a GPU: the rank of a wall tuple in the
reference's enumeration, and the accumulation over sparse valid-path records against the dense loop on the same arrays."""

import numpy as np
import pytest

F = np.float32


@pytest.mark.parametrize("n_objects", [1, 2, 5, 13])
@pytest.mark.parametrize("mask", ["all", "some", "single"])
def test_candidate_rank_inverts_the_enumeration(n_objects, mask):
    """rank(enumerated[i]) == i for every i, fed in shuffled order: orders 0..4 and every sub-range of them, with and without
    an `allowed` mask (one of them leaves a single object)."""
    from differt2d_amd import _lib as L

    rng = np.random.default_rng(100 + n_objects)
    allowed = None
    if mask == "some":
        allowed = (rng.random(n_objects) < 0.6).astype(np.uint8)
        allowed[rng.integers(n_objects)] = 1
    elif mask == "single":
        allowed = np.zeros(n_objects, np.uint8)
        allowed[n_objects // 2] = 1
    checked = 0
    for lo in range(5):
        for hi in range(lo, 5):
            if L.count_candidates(n_objects, lo, hi, allowed) > 40_000:
                continue  # (13 objects, order 4 alone: 22 464 tuples -- kept; the ranges that add the lower orders to it are not)
            en = L.enumerate_candidates(n_objects, lo, hi, allowed)
            if not en:
                continue
            cand = np.full((len(en), L.D2D_MAX_ORDER), -1, np.int32)
            order = np.array([len(e) for e in en], np.int32)
            for i, e in enumerate(en):
                cand[i, : len(e)] = e
            perm = rng.permutation(len(en))
            rank = L.candidate_rank(cand[perm], order[perm], n_objects, allowed, lo, hi)
            assert rank.dtype == np.int64 and np.array_equal(rank, perm), (n_objects, mask, lo, hi)
            checked += len(en)
    assert checked > 0
    if n_objects == 13 and mask == "all":
        assert L.count_candidates(13, 4, 4, None) == 13 * 12 ** 3  # (the order-4 range was among those checked)


def test_candidate_rank_refuses_what_the_enumeration_does_not_hold():
    from differt2d_amd import _lib as L

    with pytest.raises(ValueError):
        L.candidate_rank([[1, 1, -1, -1]], [2], 3)  # equal neighbours
    with pytest.raises(ValueError):
        L.candidate_rank([[0, -1, -1, -1]], [1], 3, allowed=[0, 1, 1])  # a filtered object
    with pytest.raises(ValueError):
        L.candidate_rank([[0, 1, -1, -1]], [2], 3, None, 0, 1)  # an order outside the range
    assert L.candidate_rank(np.zeros((0, 4)), [], 3).shape == (0,)


def _gain_fun(objects):
    gains = {id(o): F(0.5 + 0.25 * i) for i, o in enumerate(objects)}

    def fun(transmitter, receiver, path, interacting_objects, w=0.3):
        """The path's points, both end points, the interacting objects (by identity) and the solver's loss; + - * / sqrt only."""
        r = path.length()
        dx = receiver.xy[..., 0] - transmitter.xy[..., 0]
        g = F(1.0)
        for o in interacting_objects:
            g = F(g * gains[id(o)])
        return (F(w) * r * np.sqrt(r) + dx * dx + path.xys[..., -2, 0] * receiver.xy[..., 1]) * g / (F(1.0) + path.loss)

    return fun


@pytest.mark.parametrize("grid_is_rx", [True, False])
@pytest.mark.parametrize("density", [0.0, 0.02, 0.5])
def test_sparse_accumulation_equals_the_dense_loop_bit_for_bit(density, grid_is_rx):
    """Synthetic records made by masking a random dense valid[cells][C] array (random xys and losses), fed in a random
    permutation, give exactly what the dense loop of _emit_grid gives on the same arrays."""
    from differt2d_amd import _lib as L
    from differt2d_amd.geometry import ImagePath, Point, Wall
    from differt2d_amd.scene import _accumulate_dense, _accumulate_sparse

    rng = np.random.default_rng(7)
    n_objects, shape = 5, (9, 13)
    objects = [Wall(xys=rng.random((2, 2), dtype=F)) for _ in range(n_objects)]
    allowed = np.array([1, 1, 0, 1, 1], np.uint8)
    lo, hi = 0, 3
    candidates = L.enumerate_candidates(n_objects, lo, hi, allowed)
    cells, C, NP = shape[0] * shape[1], len(candidates), L.D2D_MAX_ORDER + 2
    xys = rng.random((cells, C, NP, 2), dtype=F)
    for c, cand in enumerate(candidates):
        xys[:, c, len(cand) + 2 :] = np.nan  # unused rows, as the trace leaves them
    loss = (rng.random((cells, C), dtype=F) * F(0.01)).astype(F)
    valid = np.where(rng.random((cells, C)) < density, rng.random((cells, C), dtype=F), F(0.0)).astype(F)
    grid = rng.random((cells, 2), dtype=F)
    fixed = Point(xy=np.array([0.3, 0.6], F))
    fun = _gain_fun(objects)
    interacting = lambda cand: [objects[int(i)] for i in cand]
    dense = _accumulate_dense(shape, grid, fixed, grid_is_rx, Point, ImagePath, candidates, interacting, xys, loss, valid, fun, (),
                              dict(w=0.25))

    cell_i, cand_i = np.nonzero(valid)
    perm = rng.permutation(cell_i.size)
    cell_i, cand_i = cell_i[perm], cand_i[perm]
    cand_arr = np.full((C, L.D2D_MAX_ORDER), -1, np.int32)
    for c, cand in enumerate(candidates):
        cand_arr[c, : len(cand)] = cand
    order_arr = np.array([len(c) for c in candidates], np.int32)
    records = {"cell": cell_i.astype(np.int32), "cand": cand_arr[cand_i], "order": order_arr[cand_i], "xys": xys[cell_i, cand_i],
               "loss": loss[cell_i, cand_i], "valid": valid[cell_i, cand_i]}
    rank = L.candidate_rank(records["cand"], records["order"], n_objects, allowed, lo, hi)
    assert np.array_equal(rank, cand_i)
    calls = []

    def counting(*a, **k):
        calls.append(a[2].xys.shape)
        return fun(*a, **k)

    sparse = _accumulate_sparse(shape, grid, fixed, grid_is_rx, Point, ImagePath, records, rank, interacting, counting, (), dict(w=0.25))
    assert sparse.dtype == F and sparse.shape == shape
    assert np.array_equal(sparse, dense)
    if density:
        assert np.count_nonzero(dense) > 0
    # fun once per candidate that has records, on 1-D batches of exactly its records
    assert len(calls) == np.unique(cand_i).size
    assert sorted(s[0] for s in calls) == sorted(np.bincount(cand_i)[np.unique(cand_i)].tolist())
    assert all(len(s) == 3 and s[2] == 2 for s in calls)
