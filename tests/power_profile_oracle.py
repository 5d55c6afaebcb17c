"""The oracle of the per-cell power-delay profile (include/d2d.h: d2d_power_profile_launch), built from ``oracle/ref.py``'s public
pieces (the oracle itself is not edited): loop over ``R.all_path_candidates``, take ``valid``, ``fun`` and the path's points from
``R.accumulate_candidate``, the length from ``R.path_length``, and add ``valid * fun`` to the bin of the length -- one sequential
fp32 sum per bin, in candidate order:

    inv = fp32(nbins) / (r_max - r_min)
    u = (r - r_min) * inv ;  b = floor(u) ;  if u >= 0 and b < nbins: out[b][cell] = out[b][cell] + t

``tests/test_power_profile_cpu.py`` pins the recipe (one covering bin is ``R.power_map`` bit for bit);
``tests/test_gpu_power_profile.py`` holds the kernel to it."""

import numpy as np

from oracle import ref as R

F = np.float32


def bins_inv(r_min, r_max, nbins):
    """``inv`` of the definition: fp32, one subtraction, one division."""
    return F(F(nbins) / F(F(r_max) - F(r_min)))


def profile_map(walls, fixed, Xg, Yg, r_min, r_max, nbins, min_order=0, max_order=1, fun="received_power", fun_kwargs=None,
                coef=None, approx=False, grid_role="rx", filter_nodes=None, **kw):
    """``out[nbins, m, n]`` fp32.  ``fun``: a name of ``R.FUNS``, or ``"received_power_per_object"`` with ``coef`` (fp32, one per
    wall; ``fun_kwargs`` may hold ``height``) -- the left fold of ``tests/object_coefs_oracle.py``."""
    xp = R.NUMPY
    objs = R.walls_to_objs(walls, xp)
    cands = R.all_path_candidates(len(objs), min_order, max_order, filter_nodes=filter_nodes)
    grid = R.vec(xp.asarray(Xg), xp.asarray(Yg), xp)
    fixed = xp.asarray(fixed)
    a, b = (fixed, grid) if grid_role == "rx" else (grid, fixed)
    shape = np.shape(Xg)
    cells = int(np.prod(shape))
    r_min = F(r_min)
    inv = bins_inv(r_min, r_max, nbins)
    out = np.zeros((int(nbins), cells), F)
    cell = np.arange(cells)
    for cand in cands:
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
            t = np.broadcast_to(np.asarray(xp.to_float(valid) * val, F), shape).reshape(-1)
            r = np.broadcast_to(np.asarray(R.path_length(pts, xp), F), shape).reshape(-1)
            u = ((r - r_min).astype(F) * inv).astype(F)
            fl = np.floor(u)
            ok = (u >= 0) & (fl < nbins) & ~(t == 0)  # (NaN u: no bin; adding an exact zero changes no sum: they are never -0.0)
        idx = cell[ok]
        bi = fl[ok].astype(np.int64)
        out[bi, idx] = (out[bi, idx] + t[ok]).astype(F)  # one (bin, cell) per cell: no index repeats within a candidate
    return out.reshape((int(nbins),) + tuple(shape))
