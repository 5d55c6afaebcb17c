"""The oracle of the per-cell strongest paths (include/d2d.h: d2d_strongest_paths_launch), built from ``oracle/ref.py``'s public
pieces (the oracle itself is not edited): loop over ``R.all_path_candidates``, take ``valid * fun`` and the path's points from
``R.accumulate_candidate``, the length from ``R.path_length``, keep the fp32 running ``total``, and per cell sort the
contributions that are not exactly zero by

    key = bit pattern of |t| as uint32, descending; equal keys in candidate order (a stable sort)

and keep the first ``k`` -- any ``k``, values above the kernel's 8 slots included.  ``tests/test_strongest_paths_cpu.py`` pins
the recipe (``total`` is ``R.power_map`` bit for bit); ``tests/test_gpu_strongest_paths.py`` holds the kernel to it."""

from collections import namedtuple

import numpy as np

from oracle import ref as R

F = np.float32
MAX_ORDER = 4  # D2D_MAX_ORDER: the width of ``cand``

StrongestPaths = namedtuple("StrongestPaths", "power length cand order total count")


def keys_of(t):
    """The sort key of fp32 contributions: the bits of ``|t|`` as uint32 (NaN above inf; the sign does not count)."""
    return np.ascontiguousarray(t, F).view(np.uint32) & np.uint32(0x7FFFFFFF)


def contributions(walls, fixed, Xg, Yg, min_order=0, max_order=1, fun="received_power", fun_kwargs=None, coef=None, approx=False,
                  grid_role="rx", filter_nodes=None, **kw):
    """``(cands, T[C, cells], Rl[C, cells], total[cells])``: every candidate's contribution and path length per cell, fp32, in
    enumeration order, and the sequential fp32 sum.  ``fun``: a name of ``R.FUNS``, or ``"received_power_per_object"`` with
    ``coef`` (fp32, one per wall; ``fun_kwargs`` may hold ``height``) -- the left fold of ``tests/object_coefs_oracle.py``."""
    xp = R.NUMPY
    objs = R.walls_to_objs(walls, xp)
    cands = R.all_path_candidates(len(objs), min_order, max_order, filter_nodes=filter_nodes)
    grid = R.vec(xp.asarray(Xg), xp.asarray(Yg), xp)
    fixed = xp.asarray(fixed)
    a, b = (fixed, grid) if grid_role == "rx" else (grid, fixed)
    shape = np.shape(Xg)
    cells = int(np.prod(shape))
    T = np.zeros((len(cands), cells), F)
    Rl = np.zeros((len(cands), cells), F)
    total = np.zeros(cells, F)
    for ci, cand in enumerate(cands):
        if fun == "received_power_per_object":
            num = xp.c(1.0)
            for o in cand:
                num = num * coef[int(o)]  # fp32, left fold, candidate order
            h = xp.c((fun_kwargs or {}).get("height", R.DEFAULT_HEIGHT))

            def f(pts, xp=xp, num=num, h=h):
                r = R.path_length(pts, xp)
                return num / (h * h + r * r)

            valid, val, pts, _ = R.accumulate_candidate(a, objs, cand, b, f, None, "image", approx, xp, **kw)
        else:
            valid, val, pts, _ = R.accumulate_candidate(a, objs, cand, b, fun, fun_kwargs, "image", approx, xp, **kw)
        with np.errstate(all="ignore"):
            T[ci] = np.broadcast_to(np.asarray(xp.to_float(valid) * val, F), shape).reshape(-1)
            Rl[ci] = np.broadcast_to(np.asarray(R.path_length(pts, xp), F), shape).reshape(-1)
            total = (total + T[ci]).astype(F)
    return cands, T, Rl, total


def top_k(cands, T, Rl, total, k, shape):
    """The definition's slots from the contributions: a stable sort per cell, zeros last and never kept."""
    C, cells = T.shape
    nz = ~(T == 0)  # non-zero or NaN
    key = np.where(nz, keys_of(T).astype(np.int64), -1)
    rank = np.argsort(-key, axis=0, kind="stable")  # [C, cells]: candidates by key descending, ties in enumeration order
    k = int(k)
    power = np.zeros((k, cells), F)
    length = np.full((k, cells), np.nan, F)
    cand = np.full((k, cells, MAX_ORDER), -1, np.int32)
    order = np.full((k, cells), -1, np.int32)
    cw = np.full((C, MAX_ORDER), -1, np.int32)
    co = np.zeros(C, np.int32)
    for ci, c in enumerate(cands):
        cw[ci, : len(c)] = np.asarray(c, np.int32)
        co[ci] = len(c)
    col = np.arange(cells)
    for s in range(min(k, C)):
        ci = rank[s]
        kept = nz[ci, col]
        power[s] = np.where(kept, T[ci, col], F(0.0))
        length[s] = np.where(kept, Rl[ci, col], F(np.nan))
        cand[s] = np.where(kept[:, None], cw[ci], -1)
        order[s] = np.where(kept, co[ci], -1)
    shape = tuple(shape)
    return StrongestPaths(power.reshape((k,) + shape), length.reshape((k,) + shape), cand.reshape((k,) + shape + (MAX_ORDER,)),
                          order.reshape((k,) + shape), total.reshape(shape), nz.sum(axis=0).astype(np.int32).reshape(shape))


def strongest_paths(walls, fixed, Xg, Yg, k, **kw):
    """``StrongestPaths(power[k, m, n], length[k, m, n], cand[k, m, n, 4], order[k, m, n], total[m, n], count[m, n])``."""
    cands, T, Rl, total = contributions(walls, fixed, Xg, Yg, **kw)
    return top_k(cands, T, Rl, total, k, np.shape(Xg))
