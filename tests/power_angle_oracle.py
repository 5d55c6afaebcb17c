"""The oracle of the per-cell power-angle profile (include/d2d.h: d2d_power_angle_launch), built from ``oracle/ref.py``'s public
pieces exactly as ``tests/power_profile_oracle.py`` is (the oracle itself is not edited): loop over ``R.all_path_candidates``, take
``valid``, ``fun`` and the path's points ``[tx, p1..pK, rx]`` from ``R.accumulate_candidate``, the direction at the chosen end from
``pts[1] - pts[0]`` (AT_TX) or ``pts[-2] - pts[-1]`` (AT_RX), and add ``valid * fun`` to the bin of that direction -- one sequential
fp32 sum per bin, in candidate order, every operation one NumPy fp32 operation (IEEE single, no contraction):

    f = turns(dx, dy) ;  g = f - origin ;  if g < 0: g = g + 1
    u = g * fp32(nbins) ;  b = floor(u) ;  if b >= nbins: b = nbins - 1 ;  if f == f: out[b][cell] = out[b][cell] + t

``turns`` is a NumPy restatement of ``differt2d_amd/csrc/d2d_angle.hpp``, written from the header's description;
``tests/test_power_angle_cpu.py`` holds the header's g++ build to it bit for bit, and both to float64, and pins the recipe (``total``
is ``R.power_map`` bit for bit); ``tests/test_gpu_power_angle.py`` holds the kernel to it."""

from collections import namedtuple

import numpy as np

from oracle import ref as R

F = np.float32
AT_TX, AT_RX = 0, 1  # D2D_ANGLE_AT_TX, D2D_ANGLE_AT_RX
BINS_MAX = 4096  # D2D_ANGLE_BINS_MAX

PowerAngleProfile = namedtuple("PowerAngleProfile", "bins total")

HUGE = F(1.0e38)
FLT_MAX = F(3.4028235e38)
# P(z) ~ atan(sqrt z) / (2 pi sqrt z) on [0, 1/4], highest power first
POLY = [F(-8.063173853e-03), F(1.609935798e-02), F(-2.254311182e-02), F(3.182001412e-02), F(-5.305141583e-02), F(1.591549367e-01)]


def angle_abs(x):
    """``|x|`` by compares: -0.0 becomes +0.0, NaN stays NaN."""
    x = np.asarray(x, F)
    return np.where(x < 0, -x, np.where(x == 0, F(0), x))


def angle_poly(q):
    z = q * q
    p = np.full_like(z, POLY[0])
    for c in POLY[1:]:
        p = p * z + c
    return q * p


def turns(dx, dy):
    """The angle of ``(dx, dy)`` in turns, fp32 in [0, 1), as d2d_angle.hpp computes it; NaN for (0, 0), NaN and inf."""
    dx, dy = np.asarray(dx, F), np.asarray(dy, F)
    with np.errstate(all="ignore"):
        ax, ay = angle_abs(dx), angle_abs(dy)
        swap = ay > ax
        mx, mn = np.where(swap, ay, ax), np.where(swap, ax, ay)
        ok = (ax <= FLT_MAX) & (ay <= FLT_MAX) & (mx > 0)
        huge = mx >= HUGE
        mx, mn = np.where(huge, mx * F(0.25), mx), np.where(huge, mn * F(0.25), mn)
        near = mn + mn > mx
        num = np.where(near, mx - mn, mn)
        den = np.where(near, mx + mn, mx)
        p = angle_poly(num / den)
        B = np.where(swap, np.where(near, F(0.125), F(0.25)), np.where(near, F(0.125), F(0)))
        plus = swap == near
        neg_x, neg_y = dx < 0, dy < 0
        B = np.where(neg_x, F(0.5) - B, B)
        plus = plus ^ neg_x
        B = np.where(neg_y, F(1) - B, B)
        plus = plus ^ neg_y
        f = np.where(plus, B + p, B - p)
        f = np.where(f >= 1, F(0), f)
        f = np.where(ok, f, F(np.nan))
    assert f.dtype == F
    return f


def turns_inputs(n_random=1 << 20):
    """``(dx, dy)`` the header is checked on: the exact cases (axes and diagonals, with both zeros), ``n_random`` seeded random
    directions over all octants and magnitudes from 1e-6 to 1e6, both fp32 neighbours of the diagonals and of the reduction boundary
    ``mn / mx = 1/2`` in every octant, denormals, 1e30 and the largest fp32, and (0, 0), NaN and inf (which give NaN)."""
    rng = np.random.default_rng(20261019)
    ang = rng.random(n_random) * 2 * np.pi
    mag = 10.0 ** rng.uniform(-6, 6, n_random)
    rnd = np.stack([mag * np.cos(ang), mag * np.sin(ang)], axis=1).astype(F)
    one, up, dn = F(1), np.nextafter(F(1), F(2)), np.nextafter(F(1), F(0))
    half, hup, hdn = F(0.5), np.nextafter(F(0.5), F(1)), np.nextafter(F(0.5), F(0))
    first = [(3, 0), (3, -0.0), (0, 2), (-0.0, 2), (1, 1), (7, 7), (one, up), (one, dn), (up, one), (dn, one),
             (one, half), (one, hup), (one, hdn), (half, one), (hup, one), (hdn, one)]
    tiny, den = np.nextafter(F(0), F(1)), F(1e-41)
    first += [(tiny, 0), (tiny, tiny), (den, tiny), (tiny, den), (den, 3 * den), (1e30, 1e30), (1e30, 1), (1, 1e30), (1e30, 3e29),
              (FLT_MAX, FLT_MAX), (FLT_MAX, 1e38), (1e38, FLT_MAX), (FLT_MAX, tiny), (FLT_MAX, 1e-30), (1e-30, FLT_MAX), (1, tiny), (1, 1e-30)]
    exact = np.array([(sx * a, sy * b) for a, b in first for sx in (1, -1) for sy in (1, -1)], F)
    nan, inf = np.nan, np.inf
    bad = np.array([(0, 0), (-0.0, 0), (0, -0.0), (-0.0, -0.0), (nan, 1), (1, nan), (nan, nan), (inf, 1), (1, inf), (-inf, 1), (1, -inf),
                    (inf, inf), (inf, nan), (0, nan), (0, inf)], F)
    d = np.concatenate([exact, rnd, bad])
    assert d.dtype == F
    return np.ascontiguousarray(d[:, 0]), np.ascontiguousarray(d[:, 1])


def bin_of(f, origin, nbins):
    """``(b, named)``: the definition's bin index of directions ``f`` (turns) and whether a bin is named at all (``f`` not NaN)."""
    f = np.asarray(f, F)
    with np.errstate(invalid="ignore"):
        g = f - F(origin)
        g = np.where(g < 0, g + F(1), g)
        u = g * F(nbins)
        assert g.dtype == u.dtype == F
        named = f == f
        b = np.where(named, np.floor(u), 0).astype(np.int64)
    return np.minimum(b, int(nbins) - 1), named


def origin_turns(origin_radians):
    """What the Scene methods hand to the library for an ``origin`` in radians: ``float32((origin / 2 pi) mod 1)`` computed in
    float64, a result of 1.0 becoming 0.0."""
    o = F(np.mod(np.float64(origin_radians) / (2.0 * np.pi), 1.0))
    return F(0) if o >= 1 else o


def directed_contributions(walls, fixed, Xg, Yg, min_order=0, max_order=1, fun="received_power", fun_kwargs=None, coef=None,
                           approx=False, grid_role="rx", filter_nodes=None, **kw):
    """``(cands, T[C, cells], D[C, cells, 4])``: every candidate's contribution ``valid * fun`` and its two end directions
    ``(p[1] - p[0], p[K] - p[K+1])`` per cell, fp32, in enumeration order.  ``fun``: a name of ``R.FUNS``, or
    ``"received_power_per_object"`` with ``coef`` (fp32, one per wall; ``fun_kwargs`` may hold ``height``)."""
    xp = R.NUMPY
    objs = R.walls_to_objs(walls, xp)
    cands = R.all_path_candidates(len(objs), min_order, max_order, filter_nodes=filter_nodes)
    grid = R.vec(xp.asarray(Xg), xp.asarray(Yg), xp)
    fixed = xp.asarray(fixed)
    a, b = (fixed, grid) if grid_role == "rx" else (grid, fixed)
    shape = np.shape(Xg)
    cells = int(np.prod(shape))
    T = np.zeros((len(cands), cells), F)
    D = np.zeros((len(cands), cells, 4), F)
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
            p = [np.broadcast_to(np.asarray(q, F), shape + (2,)).reshape(-1, 2) for q in (pts[0], pts[1], pts[-2], pts[-1])]
            D[ci, :, 0:2] = p[1] - p[0]
            D[ci, :, 2:4] = p[2] - p[3]
    assert D.dtype == F
    return cands, T, D


def fold(T, D, end, origin, nbins):
    """``(out[nbins, cells], total[cells])`` of contributions ``T[C, cells]`` with directions ``D[C, cells, 4]``: the definition's
    loop."""
    nbins = int(nbins)
    cells = T.shape[1]
    out = np.zeros((nbins, cells), F)
    total = np.zeros(cells, F)
    cell = np.arange(cells)
    o = 0 if end == AT_TX else 2
    with np.errstate(all="ignore"):
        for t, d in zip(T, D):
            total = total + t
            nz = ~(t == 0)  # non-zero or NaN
            if not nz.any():
                continue
            b, named = bin_of(turns(d[:, o], d[:, o + 1]), origin, nbins)
            ok = nz & named
            idx, bi = cell[ok], b[ok]
            out[bi, idx] = out[bi, idx] + t[ok]  # one (bin, cell) per cell: no index repeats within a candidate
    assert out.dtype == total.dtype == F
    return out, total


def power_angle(walls, fixed, Xg, Yg, end, origin, nbins, **kw):
    """``PowerAngleProfile(bins[nbins, m, n], total[m, n])``; ``kw`` as for ``directed_contributions``."""
    _, T, D = directed_contributions(walls, fixed, Xg, Yg, **kw)
    out, total = fold(T, D, end, origin, nbins)
    shape = tuple(np.shape(Xg))
    return PowerAngleProfile(out.reshape((int(nbins),) + shape), total.reshape(shape))
