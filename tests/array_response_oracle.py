"""The oracle of the array response (include/d2d.h: d2d_array_response_launch), built from ``contributions()`` of
``tests/strongest_paths_oracle.py`` (every candidate's ``valid * fun`` and path length per cell) and ``directed_contributions()`` of
``tests/power_angle_oracle.py`` (the same contributions with the path's two end directions) -- both from ``oracle/ref.py``, which is
not edited; the two ``T`` must agree in bits -- plus the definition: a left fold over the candidates in enumeration order, every
operation one NumPy fp32 operation (IEEE single, no contraction).  ``unit_dir``, ``steer_dot`` and ``steer_phase`` are a NumPy
restatement of ``differt2d_amd/csrc/d2d_steer.hpp``, written from the header's description; ``tests/test_array_response_cpu.py``
holds the header's g++ build to it bit for bit.  The phasor and the amplitude are the coherent field's
(``tests/coherent_field_oracle.py``)."""

from collections import namedtuple

import numpy as np

from coherent_field_oracle import AMP_LINEAR, AMP_SQRT, amplitude_of, phasor  # noqa: F401
from power_angle_oracle import directed_contributions
from strongest_paths_oracle import contributions

F = np.float32
ARRAY_MAX = 8  # D2D_ARRAY_MAX
FLT_MAX = F(3.4028235e38)

ArrayResponse = namedtuple("ArrayResponse", "re im total")


def unit_dir(dx, dy):
    """``(ux, uy, ok)``: the unit vector of ``(dx, dy)`` in fp32 as d2d_steer.hpp computes it, and whether there is one."""
    dx, dy = np.asarray(dx, F), np.asarray(dy, F)
    with np.errstate(all="ignore"):
        xx, yy = dx * dx, dy * dy
        n = np.sqrt(xx + yy)
        ux, uy = dx / n, dy / n
        ok = (n > 0) & (n <= FLT_MAX)
    assert ux.dtype == uy.dtype == n.dtype == F
    return ux, uy, ok


def steer_dot(ex, ey, ux, uy):
    with np.errstate(all="ignore"):
        a, b = F(ex) * np.asarray(ux, F), F(ey) * np.asarray(uy, F)
        q = a + b
    assert q.dtype == F
    return q


def steer_phase(f0, qt, qr, inv):
    """The pair's phase in turns, [0, 1): ``w = (qt + qr) * inv; v = f0 - w; f = v - floor(v); f >= 1 -> 0``."""
    f0, qt, qr, inv = (np.asarray(a, F) for a in (f0, qt, qr, inv))
    with np.errstate(all="ignore"):
        w = (qt + qr) * inv
        v = f0 - w
        f = v - np.floor(v)
        f = np.where(f >= 1, F(0), f)
    assert f.dtype == F
    return f


def steer_inputs(n_random=1 << 18):
    """``(dx, dy, f0, qt, qr, inv)`` the header is checked on, one size: seeded random directions of magnitudes 1e-6 .. 1e6 with random
    phases, offsets up to a few length units and inverse wavelengths up to 100; then the special directions (zero with both signs,
    denormal, squares that underflow or overflow, the largest fp32, NaN, inf) and the special phases (the clamp case ``f0 = 0``,
    ``w = 1e-9``, its neighbours, zero offsets of both signs, NaN and infinite terms), each special direction with each special phase."""
    rng = np.random.default_rng(20261019)
    ang = rng.random(n_random) * 2 * np.pi
    mag = 10.0 ** rng.uniform(-6, 6, n_random)
    rnd = np.stack([mag * np.cos(ang), mag * np.sin(ang), rng.random(n_random), rng.uniform(-3, 3, n_random), rng.uniform(-3, 3, n_random),
                    10.0 ** rng.uniform(-2, 2, n_random)], axis=1).astype(F)
    rnd[:, 2] = np.minimum(rnd[:, 2], np.nextafter(F(1), F(0)))
    tiny, fmax, nan, inf = np.nextafter(F(0), F(1)), np.finfo(F).max, np.nan, np.inf
    dirs = [(0, 0), (-0.0, 0), (0, -0.0), (-0.0, -0.0), (tiny, 0), (tiny, tiny), (1e-30, 1e-30), (1e-23, 1e-23), (1e-19, 0), (3, 4), (-3, 4),
            (1, -0.0), (0, -2), (1e19, 1e19), (1.5e19, 1e19), (1e30, 1), (fmax, 0), (fmax, fmax), (-fmax, 1), (nan, 1), (1, nan), (inf, 1),
            (1, -inf), (inf, inf), (nan, nan), (0, nan)]
    below1 = np.nextafter(F(1), F(0))
    phases = [(0, 1e-9, 0, 1), (0, 0, 1e-9, 1), (0, 1e-9, 0, 20), (tiny, 1e-9, 0, 1), (0, -1e-9, 0, 1), (0, tiny, 0, 1), (0, 0, 0, 20),
              (0, -0.0, -0.0, 20), (0.375, -0.0, 0, 20), (0.375, 0, -0.0, 0), (below1, 0, 0, 20), (below1, -1e-9, 0, 1), (below1, 1e-9, 0, 1),
              (0.5, 0.025, -0.0125, 20), (0.25, 3, 4, 20), (0.25, -3, -4, 20), (0.75, 1e30, 1e30, 1e30), (0.5, fmax, fmax, 1), (0.5, 1, 1, inf),
              (nan, 0, 0, 20), (0.5, nan, 0, 20), (0.5, 0, inf, 20), (0.5, inf, -inf, 20), (0.5, 0.01, 0.01, 0), (0.5, 1e-3, 1e-3, tiny)]
    special = np.array([d + p for d in dirs for p in phases], F)
    x = np.concatenate([rnd, special])
    assert x.dtype == F
    return tuple(np.ascontiguousarray(x[:, k]) for k in range(6))


def elements(e):
    e = np.ascontiguousarray(e, F).reshape(-1, 2)
    assert 1 <= e.shape[0] <= ARRAY_MAX
    return e


def fold(T, Rl, D, inv_wavelength, amplitude, etx, erx):
    """``(re[nr, nt, cells], im[nr, nt, cells], total[cells])`` of contributions ``T[C, cells]`` with lengths ``Rl[C, cells]`` and end
    directions ``D[C, cells, 4]``: the definition's loop."""
    inv = F(inv_wavelength)
    etx, erx = elements(etx), elements(erx)
    nt, nr = etx.shape[0], erx.shape[0]
    cells = T.shape[1]
    re, im, total = np.zeros((nr, nt, cells), F), np.zeros((nr, nt, cells), F), np.zeros(cells, F)
    with np.errstate(all="ignore"):
        for t, r, d in zip(T, Rl, D):
            total = total + t
            nz = ~(t == 0)  # non-zero or NaN
            if not nz.any():
                continue
            a = amplitude_of(t, amplitude)
            u = r * inv
            f0 = u - np.floor(u)
            utx, uty, okt = unit_dir(d[:, 0], d[:, 1])
            urx, ury, okr = unit_dir(d[:, 2], d[:, 3])
            go = nz & okt & okr
            for j in range(nt):
                qt = steer_dot(etx[j, 0], etx[j, 1], utx, uty)
                for i in range(nr):
                    qr = steer_dot(erx[i, 0], erx[i, 1], urx, ury)
                    c, s = phasor(steer_phase(f0, qt, qr, inv))
                    re[i, j] = np.where(go, re[i, j] + a * c, re[i, j])
                    im[i, j] = np.where(go, im[i, j] - a * s, im[i, j])
    assert re.dtype == im.dtype == total.dtype == F
    return re, im, total


def directed(walls, fixed, Xg, Yg, **kw):
    """``(cands, T, Rl, D)``: the two oracles' contributions joined; their ``T`` agree in bits."""
    cands, T, Rl, _ = contributions(walls, fixed, Xg, Yg, **kw)
    cands2, T2, D = directed_contributions(walls, fixed, Xg, Yg, **kw)
    assert len(cands) == len(cands2) and all(np.array_equal(a, b) for a, b in zip(cands, cands2))
    assert np.array_equal(T.view(np.uint32), T2.view(np.uint32))
    return cands, T, Rl, D


def array_response(walls, fixed, Xg, Yg, inv_wavelength, amplitude, etx, erx, **kw):
    """``ArrayResponse(re[nr, nt, m, n], im[nr, nt, m, n], total[m, n])``; ``kw`` as for ``contributions``."""
    _, T, Rl, D = directed(walls, fixed, Xg, Yg, **kw)
    re, im, total = fold(T, Rl, D, inv_wavelength, amplitude, etx, erx)
    shape = tuple(np.shape(Xg))
    return ArrayResponse(re.reshape(re.shape[:2] + shape), im.reshape(im.shape[:2] + shape), total.reshape(shape))


def physics(T, Rl, D, inv_wavelength, amplitude, etx, erx):
    """``(H [nr, nt, cells] complex128, bound [nr, nt, cells])``: the float64 sum of
    ``a_k e^(-j 2 pi (r_k - e_tx[j] . u_tx,k - e_rx[i] . u_rx,k) / lambda)`` from the fp32 ``T``, ``Rl`` and ``D`` (amplitude, unit
    vectors, dot products and the product with ``1 / lambda`` in float64; a contribution whose fp32 direction has no unit vector is
    left out, as the definition leaves it out), and the bound on what the fp32 definition may differ by.  With ``e = 2^-24`` (the
    unit roundoff), ``E = |ex| + |ey|`` of an element and ``W = (E_tx[j] + E_rx[i]) / lambda``, the phase of one contribution is off
    by at most, in turns:

      - ``ulp(u) / 2``: the rounding of ``u = r / lambda``; ``f0 = u - floor(u)`` is exact;
      - the unit vector: ``dx^2``, ``dy^2`` and their sum round once each (``2 e`` relative on ``n^2``, ``e`` on ``n``), the square
        root and the division once each: every component is within ``3 e`` (components are at most 1);
      - ``q = ex ux + ey uy``: each product rounds once (``e``), the sum once: within ``5 e E`` with the unit vector's share;
      - ``w = (qt + qr) * inv``: the sum and the product round once each: with the two q, within ``7 e W``;
      - ``v = f0 - w``: one rounding, ``e |v| <= e (1 + W)``;
      - ``f = v - floor(v)``: exact for ``v >= 0``; for ``v < 0`` it is ``v + k`` rounded once, a result of at most 1: ``e``
        (and ``f = 1 -> 0`` is the same point of the circle);

    in all ``ulp(u) / 2 + e (8 W + 2)`` turns, ``2 pi`` times that in radians.  To it come, as in
    ``coherent_field_oracle.physics``, the phasor's error ``2 * 2^-24``, the roundings of the square root and the product ``2^-23`` and
    ``N`` fp32 additions ``N 2^-24``; all of it times ``|a_k|``, summed, with a factor 2 of margin."""
    etx, erx = elements(etx), elements(erx)
    nt, nr = etx.shape[0], erx.shape[0]
    e = 2.0**-24
    inv64 = float(F(inv_wavelength))
    T64, R64, D64 = T.astype(np.float64), Rl.astype(np.float64), D.astype(np.float64)
    _, _, okt = unit_dir(D[:, :, 0], D[:, :, 1])
    _, _, okr = unit_dir(D[:, :, 2], D[:, :, 3])
    go = (T != 0) & okt & okr
    a = np.where(go, np.sign(T64) * np.sqrt(np.abs(T64)) if amplitude == AMP_SQRT else T64, 0.0)
    with np.errstate(all="ignore"):
        nrm_t = np.hypot(D64[:, :, 0], D64[:, :, 1])
        nrm_r = np.hypot(D64[:, :, 2], D64[:, :, 3])
        ut = np.where(go[..., None], D64[:, :, 0:2] / nrm_t[..., None], 0.0)
        ur = np.where(go[..., None], D64[:, :, 2:4] / nrm_r[..., None], 0.0)
        ulp_u = np.spacing(np.abs((Rl * F(inv_wavelength)).astype(F))).astype(np.float64)
    u = R64 * inv64
    n = go.sum(axis=0)
    cells = T.shape[1]
    H = np.zeros((nr, nt, cells), np.complex128)
    bound = np.zeros((nr, nt, cells))
    for j in range(nt):
        qt = ut @ etx[j].astype(np.float64)
        for i in range(nr):
            qr = ur @ erx[i].astype(np.float64)
            H[i, j] = (a * np.exp(-2j * np.pi * (u - (qt + qr) * inv64))).sum(axis=0)
            W = (np.abs(etx[j]).astype(np.float64).sum() + np.abs(erx[i]).astype(np.float64).sum()) * inv64
            per = np.pi * ulp_u + 2 * np.pi * e * (8 * W + 2) + 2 * 2.0**-24 + 2.0**-23 + n[None, :] * 2.0**-24
            bound[i, j] = 2 * (np.abs(a) * per).sum(axis=0)
    return H, bound
