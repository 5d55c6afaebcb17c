"""The oracle of the beam-space response (include/d2d.h: d2d_beam_response_launch): a NumPy restatement of
``differt2d_amd/csrc/d2d_beam.hpp`` (``steer``, the two folds, the pair product), written from the header's description, folded over
the cached contributions, lengths and end directions that ``tests/test_gpu_strongest_paths.py::_contributions`` and
``tests/test_gpu_power_angle.py::_directed`` provide -- every operation one NumPy fp32 operation (IEEE single, no contraction),
candidates in enumeration order, elements in list order.  ``unit_dir`` and ``steer_dot`` are the array response's
(``tests/array_response_oracle.py``), the phasor and the amplitude the coherent field's (``tests/coherent_field_oracle.py``).
Nothing of the kernel's chunking or nesting is restated here: the wavelengths are one more NumPy axis.

``bound`` is the derived element-space bound: how far the beam planes may be from the float64 contraction
``conj(w_rx) . H . w_tx`` of the wideband array response's fp32 planes ``H``.  On the test scenes (random7, obstacle and
square_centre; hard and hsig; both roles; both amplitudes; 3 x 4 elements with a 2 x 3 codebook and 8 x 8 with 8 x 8, four
wavelengths) the two NumPy oracles stay inside it with an observed ``max error / bound`` of 0.062 at most (0.022 .. 0.062 over the 32 cases)
(``tests/test_beam_response_cpu.py::test_element_space_bound_between_the_two_oracles`` prints the figure of every case)."""

from collections import namedtuple

import numpy as np

from array_response_oracle import elements, steer_dot, unit_dir
from coherent_field_oracle import AMP_LINEAR, AMP_SQRT, amplitude_of, phasor  # noqa: F401

F = np.float32
BEAM_MAX = 8  # D2D_BEAM_MAX

BeamResponse = namedtuple("BeamResponse", "re im total")


# ---- d2d_beam.hpp, restated ------------------------------------------------------------------------------------------------------------
def steer(q, inv):
    """``(c, s)`` of ``e^(+j 2 pi q inv)``: ``v = q * inv; g = v - floor(v); g >= 1 -> 0; phasor(g)``."""
    q, inv = np.asarray(q, F), np.asarray(inv, F)
    with np.errstate(all="ignore"):
        v = q * inv
        g = v - np.floor(v)
        g = np.where(g >= 1, F(0), g)
    assert g.dtype == F
    return phasor(g)


def fold_tx(at_re, at_im, w_re, w_im, c, s):
    """One step of the transmit fold: ``At + w * (c + j s)``."""
    w_re, w_im = F(w_re), F(w_im)
    with np.errstate(all="ignore"):
        rc, i_s, rs, ic = w_re * c, w_im * s, w_re * s, w_im * c
        re, im = at_re + (rc - i_s), at_im + (rs + ic)
    assert re.dtype == im.dtype == F
    return re, im


def fold_rx(ar_re, ar_im, w_re, w_im, c, s):
    """One step of the receive fold: ``Ar + conj(w) * (c + j s)``."""
    w_re, w_im = F(w_re), F(w_im)
    with np.errstate(all="ignore"):
        rc, i_s, rs, ic = w_re * c, w_im * s, w_re * s, w_im * c
        re, im = ar_re + (rc + i_s), ar_im + (rs - ic)
    assert re.dtype == im.dtype == F
    return re, im


def pair(ar_re, ar_im, at_re, at_im, c0, s0):
    """``(zr, zs)``: ``P = Ar * At`` rotated by the path's phase, ``P e^(-j 2 pi f0) = zr - j zs``."""
    ar_re, ar_im, at_re, at_im, c0, s0 = (np.asarray(a, F) for a in (ar_re, ar_im, at_re, at_im, c0, s0))
    with np.errstate(all="ignore"):
        rr, ii, ri, ir = ar_re * at_re, ar_im * at_im, ar_re * at_im, ar_im * at_re
        p_re, p_im = rr - ii, ri + ir
        pc, qs, ps, qc = p_re * c0, p_im * s0, p_re * s0, p_im * c0
        zr, zs = pc + qs, ps - qc
    assert zr.dtype == zs.dtype == F
    return zr, zs


def weights(w, n):
    """A codebook as complex64 ``[nb, n]`` (``[n]`` is one beam)."""
    w = np.asarray(w)
    w = np.ascontiguousarray(w.reshape(1, -1) if w.ndim == 1 else w, np.complex64)
    assert w.ndim == 2 and 1 <= w.shape[0] <= BEAM_MAX and w.shape[1] == n, (w.shape, n)
    return w


def beam_inputs(n_random=1 << 16):
    """``(q, inv, w_re, w_im, a_re, a_im, b_re, b_im, f0)`` the header is checked on, one size: seeded random offsets up to a few length
    units, inverse wavelengths up to 100, weights and array factors of magnitudes 1e-3 .. 1e3 and phases in [0, 1); then the specials:
    ``q * inv`` just below an integer (and just above, and negative ones), exact quarter turns, ``+-0`` offsets, a zero inverse
    wavelength, and NaN / inf in every position."""
    rng = np.random.default_rng(20261020)
    mag = lambda: (10.0 ** rng.uniform(-3, 3, n_random)) * rng.choice([-1.0, 1.0], n_random)  # noqa: E731
    rnd = np.stack([rng.uniform(-3, 3, n_random), 10.0 ** rng.uniform(-2, 2, n_random), mag(), mag(), mag(), mag(), mag(), mag(),
                    rng.random(n_random)], axis=1).astype(F)
    rnd[:, 8] = np.minimum(rnd[:, 8], np.nextafter(F(1), F(0)))
    below = lambda k: np.nextafter(F(k), F(-np.inf))  # noqa: E731
    above = lambda k: np.nextafter(F(k), F(np.inf))  # noqa: E731
    nan, inf, tiny, fmax = np.nan, np.inf, np.nextafter(F(0), F(1)), np.finfo(F).max
    qi = [(below(1), 1), (below(3), 1), (above(3), 1), (below(-2), 1), (above(-2), 1), (-1e-9, 1), (1e-9, 1), (-tiny, 1), (0.0125, 20),
          (0.025, 20), (0.0375, 20), (0.05, 20), (-0.0125, 20), (0.25, 1), (0.5, 1), (0.75, 1), (-0.25, 1), (3, 0.25), (0.0, 20),
          (-0.0, 20), (0.0, 0.0), (-0.0, 0.0), (2.5, 0.0), (1e30, 1e30), (fmax, 1), (-fmax, fmax), (nan, 1), (1, nan), (inf, 1),
          (-inf, 1), (1, inf), (inf, 0.0), (0.3, 7.5), (-1.7, 33.25)]
    ws = [(1, 0), (0, 1), (-1, 0), (0, -1), (0, 0), (-0.0, 0), (0, -0.0), (0.6, -0.8), (1e-3, 1e3), (fmax, fmax), (nan, 1), (1, nan),
          (inf, 1), (1, -inf), (tiny, -tiny)]
    f0s = [0.0, 0.25, 0.5, 0.75, 0.125, below(1), tiny, 0.3, nan]
    special = np.array([q + w + a + b + (f0,) for q in qi for w in ws for a in ((1, 0), (0.5, -2.0), (-0.0, 0.0), (inf, nan))
                        for b in ((0, 0), (-3.0, 0.25)) for f0 in f0s], F)
    x = np.concatenate([rnd, special])
    assert x.dtype == F
    return tuple(np.ascontiguousarray(x[:, k]) for k in range(9))


# ---- the definition's loop -----------------------------------------------------------------------------------------------------------------
def fold_list(T, Rl, D, inv_wavelengths, amplitude, etx, erx, wtx, wrx):
    """``(re[nf, nbr, nbt, cells], im[nf, nbr, nbt, cells], total[cells])`` of contributions ``T[C, cells]`` with lengths
    ``Rl[C, cells]`` and end directions ``D[C, cells, 4]``: the definition's loop, the wavelengths as a NumPy axis."""
    inv = np.asarray(inv_wavelengths, F).reshape(-1, 1)
    etx, erx = elements(etx), elements(erx)
    nt, nr = etx.shape[0], erx.shape[0]
    wtx, wrx = weights(wtx, nt), weights(wrx, nr)
    nbt, nbr, nf, cells = wtx.shape[0], wrx.shape[0], inv.shape[0], T.shape[1]
    assert nf >= 1
    re, im, total = np.zeros((nf, nbr, nbt, cells), F), np.zeros((nf, nbr, nbt, cells), F), np.zeros(cells, F)
    zero = np.zeros((nf, cells), F)
    with np.errstate(all="ignore"):
        for t, r, d in zip(T, Rl, D):
            total = total + t
            nz = ~(t == 0)  # non-zero or NaN
            if not nz.any():
                continue
            a = amplitude_of(t, amplitude)
            utx, uty, okt = unit_dir(d[:, 0], d[:, 1])
            urx, ury, okr = unit_dir(d[:, 2], d[:, 3])
            go = nz & okt & okr
            u = r[None, :] * inv
            c0, s0 = phasor(u - np.floor(u))
            stx = [steer(steer_dot(etx[j, 0], etx[j, 1], utx, uty)[None, :], inv) for j in range(nt)]
            srx = [steer(steer_dot(erx[i, 0], erx[i, 1], urx, ury)[None, :], inv) for i in range(nr)]
            At, Ar = [], []
            for bt in range(nbt):
                acc = (zero, zero)
                for j in range(nt):
                    acc = fold_tx(*acc, wtx[bt, j].real, wtx[bt, j].imag, *stx[j])
                At.append(acc)
            for br in range(nbr):
                acc = (zero, zero)
                for i in range(nr):
                    acc = fold_rx(*acc, wrx[br, i].real, wrx[br, i].imag, *srx[i])
                Ar.append(acc)
            for br in range(nbr):
                for bt in range(nbt):
                    zr, zs = pair(*Ar[br], *At[bt], c0, s0)
                    re[:, br, bt] = np.where(go, re[:, br, bt] + a * zr, re[:, br, bt])
                    im[:, br, bt] = np.where(go, im[:, br, bt] - a * zs, im[:, br, bt])
    assert re.dtype == im.dtype == total.dtype == F
    return re, im, total


def beam_response(walls, fixed, Xg, Yg, inv_wavelengths, amplitude, etx, erx, wtx, wrx, **kw):
    """``BeamResponse(re[nf, nbr, nbt, m, n], im[nf, nbr, nbt, m, n], total[m, n])``; ``kw`` as for ``contributions``."""
    from array_response_oracle import directed

    _, T, Rl, D = directed(walls, fixed, Xg, Yg, **kw)
    re, im, total = fold_list(T, Rl, D, inv_wavelengths, amplitude, etx, erx, wtx, wrx)
    shape = tuple(np.shape(Xg))
    return BeamResponse(re.reshape(re.shape[:3] + shape), im.reshape(im.shape[:3] + shape), total.reshape(shape))


# ---- element space ------------------------------------------------------------------------------------------------------------------------
def contract(H_re, H_im, wtx, wrx):
    """``y[nf, nbr, nbt, ...] = conj(w_rx) . H . w_tx`` in complex128 from planes ``H[nf, nr, nt, ...]``."""
    H = np.asarray(H_re, np.float64) + 1j * np.asarray(H_im, np.float64)
    wt = weights(wtx, H.shape[2]).astype(np.complex128)
    wr = weights(wrx, H.shape[1]).astype(np.complex128)
    return np.einsum("ri,fij...,tj->frt...", wr.conj(), H, wt)


def bound(T, Rl, D, inv_wavelengths, amplitude, etx, erx, wtx, wrx):
    """``[nf, nbr, nbt, cells]``: what the fp32 beam planes may differ by from ``contract`` of the fp32 planes of the wideband array
    response (``array_frequency_response_oracle.fold_list``), per cell.  Both start from the same fp32 ``a``, ``r``, unit vectors and
    ``qt[j] = steer_dot(etx[j], utx)``, ``qr[i]``, bit for bit; the exact share of a contribution in pair ``(i, j)`` is
    ``a e^(-j 2 pi (r - qt[j] - qr[i]) inv)``.  With ``e = 2^-24`` (the unit roundoff), ``Qt = max_j |qt[j]|``, ``Qr = max_i |qr[i]|``
    and ``W = (Qt + Qr) inv``, the phase of one contribution is off by at most, in turns:

      - element space (d2d_steer.hpp): ``ulp(u) / 2`` for ``u = r * inv`` (``f0 = u - floor(u)`` is exact); the sum ``qt + qr``
        rounds once, ``e |qt + qr| inv <= ulp(W)``, and its product with ``inv`` once, ``ulp(W) / 2``; ``v = f0 - w`` rounds once,
        ``e (1 + W) <= e + ulp(W)``; ``f = v - floor(v)`` once for ``v < 0``, ``e / 2``: in all ``ulp(u) / 2 + 2.5 ulp(W) + 1.5 e``;
      - beam space (d2d_beam.hpp): ``ulp(u) / 2`` again; ``qt * inv`` and ``qr * inv`` round once each, ``ulp(Qt inv) / 2`` and
        ``ulp(Qr inv) / 2``; ``g = v - floor(v)`` once each for ``v < 0``, ``e / 2`` each: in all
        ``ulp(u) / 2 + ulp(Qt inv) / 2 + ulp(Qr inv) / 2 + e``;

    together ``ulp(u) + ulp(Qt inv) / 2 + ulp(Qr inv) / 2 + 2.5 ulp(W) + 2.5 e`` turns, ``2 pi`` times that in radians (the common
    rounding of ``u`` is counted on both sides although it cancels: the bound does not lean on that).  To it come, in units of ``e``
    and relative to ``|a| |w_rx|_1 |w_tx|_1`` (``|.|_1`` the sum of the weights' magnitudes): the four phasors at
    ``1.64 sqrt(2)`` each (one in element space, the two steerings and ``(c0, s0)`` here: 9.3); the products and inner sums of a fold
    step, ``4`` per end (8), and ``sqrt(2)`` per fold addition (``2 (nt + nr)`` taken); the pair product and the rotation, ``4``
    each (8); ``a * c`` in element space and ``a * z`` here, ``sqrt(2)`` each (2.9); and ``N`` fp32 additions per component on
    either side (``3 N`` taken, ``N`` the contributions of the cell): ``C = 32`` covers the constants.  All of it times
    ``|a_k| |w_rx|_1 |w_tx|_1``, summed over the contributions.  Everything above is first order in ``e``; the terms left out are
    products of two of the relative errors above, each below ``(32 + 2 (nt + nr) + 3 N + 2 pi (ulps) / e) e < 2^-12`` for the counts
    that exist (``N <= 2501`` candidates), so that a factor ``1 + 2^-10`` on the whole covers them (``|At| <= |w|_1 (1 + nt e)``
    included).  No other margin is taken."""
    inv = np.asarray(inv_wavelengths, F).reshape(-1, 1, 1).astype(np.float64)  # [nf, 1, 1]
    etx, erx = elements(etx), elements(erx)
    nt, nr = etx.shape[0], erx.shape[0]
    wtx, wrx = weights(wtx, nt), weights(wrx, nr)
    e = 2.0**-24
    utx, uty, okt = unit_dir(D[:, :, 0], D[:, :, 1])
    urx, ury, okr = unit_dir(D[:, :, 2], D[:, :, 3])
    go = (T != 0) & okt & okr
    T64 = T.astype(np.float64)
    a = np.where(go, np.sqrt(np.abs(T64)) if amplitude == AMP_SQRT else np.abs(T64), 0.0)  # [C, cells]
    with np.errstate(all="ignore"):
        Qt = np.max([np.abs(steer_dot(etx[j, 0], etx[j, 1], utx, uty)) for j in range(nt)], axis=0).astype(np.float64)
        Qr = np.max([np.abs(steer_dot(erx[i, 0], erx[i, 1], urx, ury)) for i in range(nr)], axis=0).astype(np.float64)
    Qt, Qr = np.where(go, Qt, 0.0), np.where(go, Qr, 0.0)
    ulp = lambda x: np.spacing(np.abs(x).astype(F)).astype(np.float64)  # noqa: E731
    with np.errstate(all="ignore"):
        turns = ulp(np.where(go, Rl, 0).astype(np.float64)[None] * inv) + ulp(Qt[None] * inv) / 2 + ulp(Qr[None] * inv) / 2 \
            + 2.5 * ulp((Qt + Qr)[None] * inv) + 2.5 * e  # [nf, C, cells]
    n = go.sum(axis=0)  # [cells]
    per = 2 * np.pi * turns + (32 + 2 * (nt + nr) + 3 * n[None, None, :]) * e
    cell = (1 + 2.0**-10) * (a[None] * per).sum(axis=1)  # [nf, cells]
    l1t, l1r = np.abs(wtx.astype(np.complex128)).sum(axis=1), np.abs(wrx.astype(np.complex128)).sum(axis=1)
    return cell[:, None, None, :] * l1r[None, :, None, None] * l1t[None, None, :, None]


def guard(re, im):
    """What the comparisons assert of the oracle's planes first, so that a wrong plane offset or a reused beam or wavelength cannot
    pass: more than a third of ``re`` and of ``im`` is non-zero, and the planes ``(f, br, bt)`` differ pairwise in bits (``re`` and
    ``im`` both)."""
    assert np.count_nonzero(re) > re.size // 3, (np.count_nonzero(re), re.size)
    assert np.count_nonzero(im) > im.size // 3, (np.count_nonzero(im), im.size)
    planes = re.shape[0] * re.shape[1] * re.shape[2]
    rb = np.ascontiguousarray(re).view(np.uint32).reshape(planes, -1)
    ib = np.ascontiguousarray(im).view(np.uint32).reshape(planes, -1)
    for a in range(planes):
        differ = (rb[a + 1:] != rb[a]).any(axis=1) & (ib[a + 1:] != ib[a]).any(axis=1)
        assert differ.all(), (a, np.flatnonzero(~differ) + a + 1)
