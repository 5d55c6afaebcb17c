"""The oracle of the frequency response's coefficient adjoint (include/d2d.h: d2d_field_coefs_vjp_launch; K3-G ``d2d::CoefGradSink``),
built from ``contributions()`` of ``tests/strongest_paths_oracle.py`` (every candidate's ``S = valid / (h^2 + r^2)`` and path length
``Rl`` per cell in fp32, from ``oracle/ref.py``; the oracle itself is not edited) plus the definition, evaluated in float64 with
``numpy.cos`` / ``numpy.sin``.

The adjoint is a sum over cells, so the kernel is not held to it bit for bit but to a derived bound, per wall ``w``:

    bound_w = 2 * sum_terms sum_j |term_j| * (pi * ulp(u_j) + (16 + K + nf + 6 + n_row) * 2^-24)

where a *term* is one (cell, contributing candidate, position ``i`` with ``cand[i] == w``) and ``term_j = (re_bar[j] c_j - im_bar[j]
s_j) * s * Q_i`` its share of wavelength ``j`` (the term itself is ``sum_j term_j``).  ``mag_w = sum_terms sum_j |term_j|`` is the
scale the bound is relative to: a wall's gradient cancels down to a fraction of a percent of it, so nothing here is ever compared
relative to ``|coef_bar|``.  Where the count comes from, per ``term_j``, in units of ``2^-24`` (half an ulp, relative) unless said
otherwise:

  - ``pi * ulp(u_j)``: the kernel forms ``u = r * inv_wavelength[j]`` in fp32, half an ulp of turns off the float64 product, which
    is ``pi * ulp(u)`` radians of phase (``frac`` is exact);
  - 16: the phasor's 1.64 (absolute, on values of magnitude <= 1), the two products ``re_bar * c`` and ``im_bar * s`` and their
    difference (3), the square roots of SQRT (``sqrtf(s)``, ``sqrtf|num|``: 2), the doubling is exact, the division of ``Q_i`` (1),
    the products ``g * s`` and ``S * Q_i`` (2), the conversion of the coefficients is exact; 16 rounds this up with room for the
    phase-dependent ratio of the phasor's absolute error to ``|term_j|``;
  - K: the K - 1 products of the fold ``num`` and the K - 2 of ``P_i``, at most K together in any one ``Q_i``;
  - nf: the adds of ``g`` over the wavelengths of a chunk (at most 8 per launch; ``nf`` covers every chunk length);
  - 6: the six levels of the wave's butterfly sum;
  - n_row: the adds into the patch's row entry, one per contributing (candidate, position) that names the wall and per chunk
    launch: ``n_row_w = ceil(nf / 8) * #{(candidate, i): cand[i] == w, the candidate contributes in some cell}``, which no patch
    exceeds.  The fp64 reduction over the patches adds 2^-53 per row: nothing;
  - the factor 2 in front is margin, in the style of ``coherent_field_oracle.physics``.

``S`` and ``Rl`` are the kernel's own fp32 values (the forward products are held to them bit for bit), so they carry no error."""

from collections import namedtuple

import numpy as np

from coherent_field_oracle import AMP_LINEAR, AMP_SQRT
from strongest_paths_oracle import contributions

F = np.float32
CHUNK = 8  # wavelengths per kernel launch: enters n_row only

CoefGrad = namedtuple("CoefGrad", "coef_bar mag bound n_terms touched")


def scale_contributions(walls, fixed, Xg, Yg, height, **kw):
    """``(cands, S[C, cells], Rl[C, cells])``: ``S = valid * (1 / (h^2 + r^2))`` in fp32 -- received_power with a numerator of 1."""
    cands, S, Rl, _ = contributions(walls, fixed, Xg, Yg, fun="received_power", fun_kwargs=dict(r_coef=1.0, height=height), **kw)
    return cands, S, Rl


def _factors(cand, coef, amplitude):
    """``(num fp32 left fold, Q[K] float64)`` of one candidate, or ``None`` where SQRT defines no term."""
    cf32 = [F(coef[int(o)]) for o in cand]
    num = F(1.0)
    for c in cf32:
        num = F(num * c)
    cf = np.array(cf32, np.float64)
    P = np.array([np.prod(np.delete(cf, i)) for i in range(len(cf))], np.float64)
    if amplitude == AMP_LINEAR:
        return num, P
    if num == 0:
        return None
    return num, P / (2.0 * np.sqrt(abs(float(np.prod(cf)))))


def forward(cands, S, Rl, coef, inv_wavelengths, amplitude):
    """The float64 forward sum ``H[nf, cells]`` (complex128) the adjoint belongs to: ``a e^(-j 2 pi r inv)`` with ``a = s * num``
    (LINEAR) or ``sign(num) sqrt(s) sqrt|num|`` (SQRT), candidates whose ``s`` is exactly zero left out."""
    inv = np.asarray(inv_wavelengths, F).astype(np.float64).reshape(-1)
    coef = np.asarray(coef, np.float64)
    H = np.zeros((inv.size, S.shape[1]), np.complex128)
    for ci, cand in enumerate(cands):
        nz = ~(S[ci] == 0)
        if not nz.any():
            continue
        num = float(np.prod([coef[int(o)] for o in cand])) if len(cand) else 1.0
        s64 = np.where(nz, S[ci].astype(np.float64), 0.0)
        a = s64 * num if amplitude == AMP_LINEAR else np.sign(num) * np.sqrt(s64) * np.sqrt(abs(num))
        u = Rl[ci].astype(np.float64)[None, :] * inv[:, None]
        H += np.where(nz[None, :], a[None, :] * np.exp(-2j * np.pi * u), 0.0)
    return H


def coef_grad(cands, S, Rl, coef, inv_wavelengths, re_bar, im_bar, amplitude, n_objects=None):
    """``CoefGrad(coef_bar[N], mag[N], bound[N], n_terms[N], touched)``: the definition in float64, the scale, the bound of the
    module's docstring, the number of terms per wall and, per candidate index that contributes, the cells it contributes in
    (``touched[ci]`` = boolean ``[cells]``).  ``re_bar`` / ``im_bar``: ``[nf, cells]`` (any shape that reshapes to it)."""
    inv32 = np.asarray(inv_wavelengths, F).reshape(-1)
    nf = inv32.size
    cells = S.shape[1]
    rb = np.asarray(re_bar, F).reshape(nf, cells).astype(np.float64)
    ib = np.asarray(im_bar, F).reshape(nf, cells).astype(np.float64)
    coef = np.asarray(coef, F)
    N = len(coef) if n_objects is None else n_objects
    coef_bar, mag, phase = np.zeros(N), np.zeros(N), np.zeros(N)
    flat = np.zeros(N)  # sum |term_j| * (16 + K + nf + 6), without n_row
    n_terms = np.zeros(N, np.int64)
    n_adds = np.zeros(N, np.int64)
    touched = {}
    chunks = -(-nf // CHUNK)
    with np.errstate(all="ignore"):
        for ci, cand in enumerate(cands):
            K = len(cand)
            nz = ~(S[ci] == 0)  # non-zero or NaN
            if K == 0 or not nz.any():
                continue
            fac = _factors(cand, coef, amplitude)
            if fac is None:
                continue
            _, Q = fac
            touched[ci] = nz
            s64 = S[ci].astype(np.float64)
            sw = s64 if amplitude == AMP_LINEAR else np.sqrt(s64)
            u = Rl[ci].astype(np.float64)[None, :] * inv32.astype(np.float64)[:, None]  # [nf, cells]
            ulp_u = np.spacing(np.abs((Rl[ci][None, :] * inv32[:, None]).astype(F))).astype(np.float64)
            gj = rb * np.cos(2 * np.pi * u) - ib * np.sin(2 * np.pi * u)  # [nf, cells]
            for i, o in enumerate(cand):
                w = int(o)
                tj = gj * (sw * Q[i])[None, :]  # term_j [nf, cells]
                tj = np.where(nz[None, :], tj, 0.0)
                coef_bar[w] += tj.sum()
                a = np.abs(tj)
                mag[w] += a.sum()
                phase[w] += (a * np.pi * ulp_u).sum()
                flat[w] += a.sum() * (16 + K + nf + 6)
                n_terms[w] += int(nz.sum())
                n_adds[w] += chunks
    bound = 2.0 * (phase + (flat + mag * n_adds) * 2.0**-24)
    return CoefGrad(coef_bar, mag, bound, n_terms, touched)


def guards(cg, coef, amplitude, scene=None, cands=None, need_repeat=False):
    """What every comparison asserts of the oracle first, so that it cannot pass on empty ground."""
    lit = cg.mag > 0
    if scene == "obstacle":
        assert lit.sum() >= 3, cg.mag
    zero = np.flatnonzero(np.asarray(coef) == 0)
    if amplitude == AMP_LINEAR and zero.size and scene in ("obstacle", "random7"):
        assert (cg.mag[zero] > 0).all(), (zero, cg.mag[zero])  # a zero coefficient HAS a gradient
    if amplitude == AMP_SQRT:
        assert not cg.mag[zero].any()
    if need_repeat:
        assert any(len(set(map(int, cands[ci]))) < len(cands[ci]) for ci in cg.touched), "no contributing candidate repeats a wall"
    assert lit.any() and (cg.bound[lit] <= 2.0**-12 * cg.mag[lit]).all(), (cg.bound[lit] / cg.mag[lit]).max()
    assert np.isfinite(cg.coef_bar).all()
