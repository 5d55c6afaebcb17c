"""The oracle of the frequency response's wall adjoint (include/d2d.h: d2d_field_walls_vjp_launch; K3-V ``d2d::WallGradSink``), built
from ``segment_contributions()`` of ``tests/material_response_oracle.py`` (every candidate's ``T = valid * fun``, path length ``Rl`` and
incoming segments ``S[.., i] = p[i+1] - p[i]`` per cell in fp32, from ``oracle/ref.py``; the oracle itself is not edited), the wall
table as the library builds it, and the definition.  Three things:

``bounce`` / ``restate``  ``differt2d_amd/csrc/d2d_wallgrad.hpp`` in NumPy fp32, one NumPy operation per stated operation, written from
             the header's description (``tests/test_field_walls_vjp_cpu.py`` holds the header's g++ build to ``bounce`` bit for bit),
             and the definition's loop around it: every lane's fp32 weights, summed over the cells in float64.  The product is a sum
             over cells and is not defined bit for bit; the exact rules (zeros, doubling, an appended zero plane, untouched walls)
             hold for this sum as they do for the kernel's.
``physics``  the same formula in float64 from the fp32 ``(T, Rl, S)``, the fp32 wall table and ``p[0]`` -- amplitude, ``rho``, the
             phases, the unit vectors, ``s`` and every sum in float64 -- with the scale ``mag`` and the bound below.
``displaced``  an adapter that lets ``field_position_vjp_oracle.forward`` evaluate the frozen-visibility forward sum on displaced
             walls, for central differences.

The bound, per wall ``w`` and end ``e``.  One *term* is one bounce on ``w`` of one contributing candidate in one cell.  With
``W_j = |a| (|rb_j| + |ib_j|) (|kr| + w_j)`` as in ``field_position_vjp_oracle`` (it bounds the share of wavelength ``j`` in ``|G|``
whatever the phase), ``W = sum_j W_j``, ``c_0 = |1 - s|``, ``c_1 = |s|`` and ``eps = 2^-24`` (half an ulp, relative), the fp32 weight of
a term differs from float64 by at most

    E_e = sum_j W_j pi ulp(u_j) |gam| c_e                # the phase: u = r * inv[j] is half an ulp of turns off
        + W (13 + nf_b) eps |gam| c_e                     # G: K3-X's flat count of 17 less the unit vector (3) and G * u (1), and the
                                                          #   adds of g over a block's wavelengths
        + W 10 eps c_e                                    # gam, ABSOLUTE: the unit vector (3 per component), the two products and the
                                                          #   sum of steer_dot (2) on |ux nx| + |uy ny| <= 1, times 2.0f (exact)
        + W |gam| es                                      # s, absolute (below)
        + W |gam| 3 eps (1 + |s|)                         # wa = G * gam, Wb = wa * s, Wa = wa - Wb: one rounding each
    es  = eps * (((i + 1) qabs (|tx| + |ty|) + 3 (|dx tx| + |dy ty|)) / sq + |s|)

``es``: ``q`` is rebuilt with ``i + 1`` adds per component, each rounding a partial sum of magnitude at most ``qabs`` (the largest
coordinate magnitude along the way); ``dx = q.x - ox`` rounds once more, the products and their sum once each (3 on ``|dx tx| + |dy
ty|``), the division once.  Then the rows: the 64 lanes of a patch are added by a butterfly of 6 levels, each rounding partial sums
that the patch's ``sum |terms|`` bounds, and the sum is added to the patch's fp32 row -- one add per (candidate, bounce on ``w``) pair
with a contribution anywhere and block, ``n_pairs[w] * n_blocks`` at most, each rounding a partial sum that the patch's ``sum
|terms|`` bounds; over the patches that is ``(6 + n_pairs[w] n_blocks) eps mag[w][e]``.  The fp64 reduction over the patches adds at
most ``cells 2^-53 mag[w][e]``.

    bound[w][e] = 2 * (sum_terms E_e + (6 + n_pairs[w] * n_blocks) eps mag[w][e] + cells 2^-53 mag[w][e])

The factor 2 in front is margin, in the style of ``coherent_field_oracle.physics``.  ``T``, ``Rl``, ``S``, the table and ``p[0]`` are
the kernel's own fp32 values, so they carry no error."""

from collections import namedtuple

import numpy as np

import field_position_vjp_oracle as PO
from array_response_oracle import steer_dot, unit_dir
from coherent_field_oracle import AMP_LINEAR, AMP_SQRT  # noqa: F401
from material_response_oracle import segment_contributions, wall_normals  # noqa: F401

F = np.float32
POS_CHUNK = PO.POS_CHUNK
G_OPS = 13  # the flat count of the module's docstring

WallGrad64 = namedtuple("WallGrad64", "normal_bar mag bound scale n_pairs n_terms")


def wall_table(walls):
    """``(o[N, 2], n[N, 2], t[N, 2], sq[N])`` in fp32 as the library builds its wall table: ``t = dest - origin``, ``n =
    normalize((t_y, -t_x))`` (a zero length divides by 1), ``sq = t . t`` (1 where it is 0)."""
    w = np.asarray(walls, F).reshape(-1, 2, 2)
    o = w[:, 0].copy()
    t = w[:, 1] - w[:, 0]
    sq = t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]
    sq = np.where(sq == 0, F(1), sq)
    n = wall_normals(w)
    assert o.dtype == n.dtype == t.dtype == sq.dtype == F
    return o, n, t, sq


def walls_bar_of(normal_bar, walls):
    """``walls_bar[w][e][d] = normal_bar[w][e] * (double)n_w[d] + 0.0``: what the getter forms (a zero product is ``+0.0``)."""
    n = wall_table(walls)[1].astype(np.float64)
    return np.asarray(normal_bar, np.float64)[:, :, None] * n[:, None, :] + 0.0


def first_point(fixed, Xg, Yg, role):
    """``p[0]`` per cell, fp32 ``[cells, 2]``: the transmitter -- ``fixed`` on an RX grid, the cell on a TX grid."""
    cells = int(np.size(Xg))
    if role == "rx":
        return np.broadcast_to(np.asarray(fixed, F).reshape(1, 2), (cells, 2)).copy()
    return np.stack([np.asarray(Xg, F).reshape(-1), np.asarray(Yg, F).reshape(-1)], axis=1)


# ---- d2d_wallgrad.hpp in NumPy fp32 -----------------------------------------------------------------------------------------------------
def bounce(G, qx, qy, sx, sy, ox, oy, nx, ny, tx, ty, sq):
    """``(qx, qy, Wa, Wb, ok)``: one bounce."""
    G, qx, qy, sx, sy, ox, oy, nx, ny, tx, ty, sq = (np.asarray(a, F) for a in (G, qx, qy, sx, sy, ox, oy, nx, ny, tx, ty, sq))
    with np.errstate(all="ignore"):
        qx = qx + sx
        qy = qy + sy
        ux, uy, ok = unit_dir(sx, sy)
        a, b = ux * nx, uy * ny  # steer_dot(ux, uy, nx, ny)
        gam = F(2) * (a + b)
        dx, dy = qx - ox, qy - oy
        ax, ay = dx * tx, dy * ty
        s = (ax + ay) / sq
        wa = G * gam
        Wb = wa * s
        Wa = wa - Wb
    assert qx.dtype == qy.dtype == Wa.dtype == Wb.dtype == F
    return qx, qy, Wa, Wb, ok


def header_inputs(n_random=1 << 16):
    """The twelve columns ``(G, qx, qy, sx, sy, ox, oy, nx, ny, tx, ty, sq)`` the header is checked on: seeded walls of lengths 1e-3 ..
    1e1 with the table's own normals, points and segments of a unit-sized scene, ``G`` of both signs over 1e-6 .. 1e6; then the special
    values: a zero-length wall (``n = (0, -0)``, ``sq = 1``), a zero segment, ``s`` at exactly 0 and 1, NaN and infinite inputs."""
    rng = np.random.default_rng(20261021)
    A = rng.uniform(-1, 2, (n_random, 2)).astype(F)
    L = (10.0 ** rng.uniform(-3, 1, n_random))
    ang = rng.uniform(0, 2 * np.pi, n_random)
    B = (A + (L[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1))).astype(F)
    o, n, t, sq = wall_table(np.stack([A, B], axis=1))
    q = rng.uniform(-1, 2, (n_random, 2)).astype(F)
    seg = (rng.standard_normal((n_random, 2)) * 10.0 ** rng.uniform(-3, 0.5, (n_random, 1))).astype(F)
    G = (10.0 ** rng.uniform(-6, 6, n_random) * rng.choice([-1.0, 1.0], n_random)).astype(F)
    nan, inf = np.nan, np.inf
    special = np.array([
        # G, qx, qy, sx, sy, ox, oy, nx, ny, tx, ty, sq
        (2, 0.25, 1, 0.75, -1, 0, 0, 0, -1, 2, 0, 4), (1, 0, 1, 0, -1, 0, 0, 0, -1, 2, 0, 4), (1, 2, 1, 0, -1, 0, 0, 0, -1, 2, 0, 4),
        (3, 0, 1, 0.5, -1, 0.5, 0, 0, -0.0, 0, 0, 1), (3, 0.5, 0.25, 0, 0, 0, 0, 0, -1, 2, 0, 4), (3, 0.5, 0.25, -0.0, 0, 0, 0, 0, -1, 2, 0, 4),
        (nan, 0.25, 1, 0.75, -1, 0, 0, 0, -1, 2, 0, 4), (inf, 0.25, 1, 0.75, -1, 0, 0, 0, -1, 2, 0, 4), (1, nan, 1, 0.75, -1, 0, 0, 0, -1, 2, 0, 4),
        (1, 0.25, 1, nan, -1, 0, 0, 0, -1, 2, 0, 4), (1, 0.25, 1, inf, -1, 0, 0, 0, -1, 2, 0, 4), (1, 0.25, 1, 1e-30, 1e-30, 0, 0, 0, -1, 2, 0, 4),
        (1, 0.25, 1, 1e30, -1e30, 0, 0, 0, -1, 2, 0, 4), (0, 0.25, 1, 0.75, -1, 0, 0, 0, -1, 2, 0, 4), (-0.0, 0.25, 1, 0.75, -1, 0, 0, 0, -1, 2, 0, 4),
        (1, 0.25, 1, 0.75, -1, 0, 0, nan, -1, 2, 0, 4), (1, 0.25, 1, 0.75, -1, 0, 0, 0, -1, 2, 0, 0), (5, 1, 1, 1, 0, 2, 0, 1, 0, 0, 2, 4),
    ], F)
    cols = (G, q[:, 0], q[:, 1], seg[:, 0], seg[:, 1], o[:, 0], o[:, 1], n[:, 0], n[:, 1], t[:, 0], t[:, 1], sq)
    return tuple(np.ascontiguousarray(np.concatenate([c, special[:, k]]), F) for k, c in enumerate(cols))


# ---- the definition ----------------------------------------------------------------------------------------------------------------------
def _block_G(t, r, fun, h2, inv, rb, ib, amplitude, block):
    a = PO.amp(amplitude, t)
    k = PO.kr(amplitude, PO.rho(fun, h2, r))
    g = np.zeros(t.shape, F)
    for j in block:
        g = PO.fold(g, k, r, inv[j], rb[j], ib[j])
    with np.errstate(all="ignore"):
        return a * g


def restate(cands, T, Rl, S, walls, p0, fun, height, inv_wavelengths, re_bar, im_bar, amplitude):
    """``normal_bar[N, 2]`` float64: the definition's loop with every lane's weights in fp32, summed over cells, candidates, bounces
    and blocks in float64 (``+ 0.0`` at the end: a sum of nothing but negative zeros is the kernel's ``+0.0``)."""
    inv = np.asarray(inv_wavelengths, F).reshape(-1)
    nf, cells = inv.size, T.shape[1]
    rb = np.asarray(re_bar, F).reshape(nf, cells)
    ib = np.asarray(im_bar, F).reshape(nf, cells)
    h2 = PO.h2_of(height)
    o, n, tt, sq = wall_table(walls)
    p0 = np.asarray(p0, F).reshape(cells, 2)
    out = np.zeros((len(o), 2), np.float64)
    for first in range(0, nf, POS_CHUNK):
        block = range(first, min(first + POS_CHUNK, nf))
        for cand, t, r, s in zip(cands, T, Rl, S):
            nz = ~(t == 0)  # non-zero or NaN
            if len(cand) == 0 or not nz.any():
                continue
            G = _block_G(t, r, fun, h2, inv, rb, ib, amplitude, block)
            qx, qy = p0[:, 0], p0[:, 1]
            for i, w in enumerate(cand):
                w = int(w)
                qx, qy, Wa, Wb, ok = bounce(G, qx, qy, s[:, i, 0], s[:, i, 1], o[w, 0], o[w, 1], n[w, 0], n[w, 1], tt[w, 0], tt[w, 1], sq[w])
                go = nz & ok
                out[w, 0] += np.where(go, Wa, F(0)).astype(np.float64).sum()
                out[w, 1] += np.where(go, Wb, F(0)).astype(np.float64).sum()
    return out + 0.0


def physics(cands, T, Rl, S, walls, p0, fun, height, inv_wavelengths, re_bar, im_bar, amplitude, per_cell=False):
    """``WallGrad64(normal_bar[N, 2], mag[N, 2], bound[N, 2], scale[N], n_pairs[N], n_terms)``: the formula in float64 from the fp32
    inputs (a bounce whose fp32 segment has no unit vector adds nothing, as the definition says), ``mag[w][e] = sum_terms W |gam| c_e``,
    the module docstring's ``bound``, ``scale[w] = sum_terms W |gam|``, the number of (candidate, bounce on ``w``) pairs with a
    contribution anywhere, and the number of contributing candidates per cell.  ``per_cell``: ``normal_bar`` and ``mag`` keep the cells'
    axis, ``[N, 2, cells]`` (and ``bound`` is None)."""
    inv32 = np.asarray(inv_wavelengths, F).reshape(-1)
    inv = inv32.astype(np.float64)
    nf, cells = inv.size, T.shape[1]
    rb = np.asarray(re_bar, F).reshape(nf, cells).astype(np.float64)
    ib = np.asarray(im_bar, F).reshape(nf, cells).astype(np.float64)
    h2 = float(PO.h2_of(height))
    n_blocks = -(-nf // POS_CHUNK)
    nf_b = min(nf, POS_CHUNK)
    eps = 2.0**-24
    o, n, tt, sq = (a.astype(np.float64) for a in wall_table(walls))
    N = len(o)
    p0 = np.asarray(p0, F).reshape(cells, 2).astype(np.float64)
    shape = (N, 2, cells) if per_cell else (N, 2)
    out, mag, err = np.zeros(shape), np.zeros(shape), np.zeros((N, 2))
    scale, n_pairs = np.zeros(N), np.zeros(N, np.int64)
    n_terms = np.zeros(cells, np.int64)
    red = (lambda x: x) if per_cell else (lambda x: x.sum())
    with np.errstate(all="ignore"):
        for cand, t, r, s in zip(cands, T, Rl, S):
            nz = ~(t == 0)
            if not nz.any():
                continue
            n_terms += nz
            if len(cand) == 0:
                continue
            r64 = r.astype(np.float64)
            a = PO._amp64(t.astype(np.float64), amplitude)
            k = PO._rho64(fun, h2, r64) * (0.5 if amplitude == AMP_SQRT else 1.0)
            u = r64[None, :] * inv[:, None]  # [nf, cells]
            ulp_u = np.spacing(np.abs((r[None, :] * inv32[:, None]).astype(F))).astype(np.float64)
            wj = 2.0 * np.pi * inv[:, None]
            c, sn = np.cos(2 * np.pi * u), np.sin(2 * np.pi * u)
            pr, pi = k[None, :] * c - wj * sn, k[None, :] * sn + wj * c
            G = a * (rb * pr - ib * pi).sum(axis=0)
            Wj = np.abs(a)[None, :] * (np.abs(rb) + np.abs(ib)) * (np.abs(k)[None, :] + wj)
            W, Wp = Wj.sum(axis=0), (Wj * np.pi * ulp_u).sum(axis=0)
            q = p0.copy()
            qabs = np.abs(q).max(axis=1)
            for i, w in enumerate(cand):
                w = int(w)
                seg32 = s[:, i]
                _, _, ok = unit_dir(seg32[:, 0], seg32[:, 1])
                go = nz & ok
                if go.any():
                    n_pairs[w] += 1
                seg = seg32.astype(np.float64)
                q = q + seg
                qabs = np.maximum(qabs, np.abs(q).max(axis=1))
                un = seg / np.hypot(seg[:, 0], seg[:, 1])[:, None]
                gam = 2.0 * (un[:, 0] * n[w, 0] + un[:, 1] * n[w, 1])
                d = q - o[w]
                sv = (d[:, 0] * tt[w, 0] + d[:, 1] * tt[w, 1]) / sq[w]
                es = eps * (((i + 1) * qabs * (abs(tt[w, 0]) + abs(tt[w, 1])) + 3.0 * (np.abs(d[:, 0] * tt[w, 0]) + np.abs(d[:, 1] * tt[w, 1]))) / sq[w]
                            + np.abs(sv))
                ag = np.abs(gam)
                scale[w] += np.where(go, W * ag, 0.0).sum()
                for e, (wt, ce) in enumerate(((1.0 - sv, np.abs(1.0 - sv)), (sv, np.abs(sv)))):
                    out[w, e] += red(np.where(go, G * gam * wt, 0.0))
                    mag[w, e] += red(np.where(go, W * ag * ce, 0.0))
                    E = Wp * ag * ce + W * ((G_OPS + nf_b) * eps * ag * ce + 10.0 * eps * ce + ag * es + ag * 3.0 * eps * (1.0 + np.abs(sv)))
                    err[w, e] += np.where(go, E, 0.0).sum()
    if per_cell:
        return WallGrad64(out, mag, None, scale, n_pairs, n_terms)
    rows = (6 + n_pairs * n_blocks)[:, None] * eps * mag + cells * 2.0**-53 * mag
    return WallGrad64(out, mag, 2.0 * (err + rows), scale, n_pairs, n_terms)


def guards(cands, T, ph, max_order=2, need_twice=False):
    """What every comparison asserts of the oracle first, so that it cannot pass on empty ground: contributions of at least
    ``max_order + 1`` candidates, at least one wall with a bounce, a bound that is small against the terms' scale on every touched wall,
    finite values -- and, ``need_twice`` (order 3), a contributing candidate that visits a wall twice, such as ``(a, b, a)``."""
    nz = ~(T == 0)
    assert nz.any(axis=1).sum() >= max_order + 1
    touched = ph.scale > 0
    assert touched.any() and (ph.n_pairs[touched] > 0).all() and not ph.n_pairs[~touched].any()
    assert (ph.bound[touched] <= 2.0**-10 * ph.scale[touched, None]).all(), (ph.bound[touched] / ph.scale[touched, None]).max()
    assert not ph.bound[~touched].any() and not ph.normal_bar[~touched].any()
    assert np.isfinite(ph.normal_bar).all() and np.abs(ph.normal_bar[touched]).max() > 0
    if need_twice:
        twice = [ci for ci, c in enumerate(cands) if len(set(int(x) for x in c)) < len(c) and nz[ci].any()]
        assert twice, "no contributing candidate visits a wall twice"


# ---- central differences on displaced walls ----------------------------------------------------------------------------------------------
class displaced:
    """What ``field_position_vjp_oracle.forward`` takes as its mirror, for walls that move while both end points stay: ``forward`` asks
    for the lengths twice per candidate, first at the displaced end points and then at the undisplaced ones, and forms ``r = Rl +
    (first - second)``; this adapter answers the first call from a ``Mirror`` built on the displaced walls and the second from one built
    on the walls as they are, so that ``r = Rl + (mirror_displaced - mirror_base)`` at the same end points."""

    def __init__(self, moved_walls, base_walls):
        self.pair = (PO.Mirror(moved_walls), PO.Mirror(base_walls))
        self.calls = 0

    def lengths(self, cand, tx, rx):
        m = self.pair[self.calls % 2]
        self.calls += 1
        return m.lengths(cand, tx, rx)
