"""Utilities (reference ``differt2d/utils.py``): the path functions the kernels fuse natively.

Each function here works on host ``Path`` objects (so user code can call it directly) and carries a
``_d2d_native`` tag: when it is passed as ``fun`` to a ``Scene`` sweep it is recognised and evaluated
inside the HIP kernel instead of being called from Python."""

from __future__ import annotations

from typing import NamedTuple

import numpy as np

from .defaults import DEFAULT_HEIGHT, DEFAULT_R_COEF
from .geometry import Path, Point

P0: float = 100.0
"""Received power at zero distance with the default parameters (reference utils.py:12)."""

F = np.float32


def _integer_pow(x, n: int):
    """x ** n by square-and-multiply in fp32 (the lowering of ``lax.integer_pow``)."""
    x = F(x)
    if n == 0:
        return F(1.0)
    acc = None
    while n > 0:
        if n & 1:
            acc = x if acc is None else F(acc * x)
        n >>= 1
        if n > 0:
            x = F(x * x)
    return acc


def received_power(transmitter, receiver, path: Path, interacting_objects, r_coef: float = DEFAULT_R_COEF,
                   height: float = DEFAULT_HEIGHT):
    """``r_coef ** n / (height**2 + length**2)`` with ``n`` the number of interactions (reference utils.py:17-54)."""
    r = path.length()
    n = path.xys.shape[-2] - 2
    h = F(height)
    return (_integer_pow(r_coef, n) / (h * h + r * r)).astype(F)


def received_power_per_object(transmitter, receiver, path: Path, interacting_objects, r_coef: float = DEFAULT_R_COEF,
                              height: float = DEFAULT_HEIGHT):
    """``prod_o coef(o) / (height**2 + length**2)`` over the interacting objects, ``coef(o) = getattr(o, "r_coef", r_coef)``: a
    reflection coefficient per wall -- a ``Wall`` subclass with an ``r_coef`` field or class attribute is all a user writes
    (the reference hands ``interacting_objects`` to every path function for this, scene.py:51, 1136-1154).  The product is
    folded from the left in fp32, in the candidate's order; with equal coefficients it is :func:`received_power`."""
    r = path.length()
    h = F(height)
    num = F(1.0)
    for o in interacting_objects:
        num = F(num * F(getattr(o, "r_coef", r_coef)))
    return (num / (h * h + r * r)).astype(F)


def path_length_squared(transmitter, receiver, path: Path, interacting_objects):
    """``path.length() ** 2`` -- the function the reference's accumulate tests use (tests/test_scene.py:444)."""
    r = path.length()
    return (r * r).astype(F)


def path_length_fun(transmitter, receiver, path: Path, interacting_objects):
    """``path.length()``."""
    return path.length()


def one(transmitter, receiver, path: Path, interacting_objects):
    """Constant 1: sweeps then count valid paths per cell."""
    return np.ones(path.xys.shape[:-2], F)


def delay_statistics(profile, length_range):
    """Total power, mean path length and RMS length spread per cell of a power-delay profile ``[nbins, ...]``
    (``Scene.power_delay_profile_on_receivers_grid``, ``Context.power_profile``) whose bins are ``nbins`` equal parts of
    ``length_range = (r_min, r_max)``.  On the host, in float64, every bin taken at its centre ``c_b``:

        total = sum_b P_b        mean_length = sum_b P_b c_b / total        rms_spread = sqrt(sum_b P_b (c_b - mean_length)^2 / total)

    Returns ``(total, mean_length, rms_spread)``, each of the profile's shape without its first axis; ``mean_length`` and
    ``rms_spread`` are NaN where ``total == 0`` (no path in range).  Divide lengths by the wave speed for the mean delay and the
    RMS delay spread; subtract the first occupied bin's centre for the mean EXCESS delay."""
    P = np.asarray(profile, dtype=np.float64)
    if P.ndim < 1 or P.shape[0] < 1:
        raise ValueError("profile must have the bins on its first axis")
    r_min, r_max = float(length_range[0]), float(length_range[1])
    nbins = P.shape[0]
    width = (r_max - r_min) / nbins
    centres = (r_min + (np.arange(nbins, dtype=np.float64) + 0.5) * width).reshape((nbins,) + (1,) * (P.ndim - 1))
    total = P.sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(total == 0.0, np.nan, (P * centres).sum(axis=0) / total)
        var = (P * (centres - mean) ** 2).sum(axis=0) / total
        rms = np.where(total == 0.0, np.nan, np.sqrt(var))
    return total, mean, rms


def strongest_share(sp):
    """The share of every cell's sum that its kept strongest paths carry: the sum of the slots' ``power`` divided by ``total``,
    for a ``StrongestPaths`` (``Scene.strongest_paths_on_receivers_grid``, ``Context.strongest_paths``) or any object with
    ``power`` ``[k, ...]`` and ``total`` ``[...]``.  On the host, in float64 (empty slots hold +0.0 and add nothing); NaN where
    ``total == 0``.  With a path function that is never negative the share lies in [0, 1], and 1 where nothing was cut."""
    kept = np.asarray(sp.power, dtype=np.float64).sum(axis=0)
    total = np.asarray(sp.total, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(total == 0.0, np.nan, kept / total)


def field_power(cf):
    """The power of a coherent field, ``re**2 + im**2`` per cell, for a ``CoherentField``
    (``Scene.coherent_field_on_receivers_grid``, ``Context.coherent_field``) or any object with ``re`` and ``im``.  On the host, in
    float64.  With ``amplitude="sqrt"`` it is a power in the units of the fused function, and equals ``|total|`` where a cell has
    one path."""
    re = np.asarray(cf.re, dtype=np.float64)
    im = np.asarray(cf.im, dtype=np.float64)
    return re * re + im * im


def fading_gain(cf):
    """The gain of the coherent sum over the incoherent one, ``field_power(cf) / total`` per cell: 1 where a cell has one path,
    above 1 where its paths add in phase, towards 0 where they cancel (small-scale fading).  On the host, in float64; NaN where
    ``total == 0``."""
    total = np.asarray(cf.total, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(total == 0.0, np.nan, field_power(cf) / total)


def frequency_response(fr):
    """The complex channel frequency response ``H = re + 1j * im``, complex64 ``[nf, m, n]``, of a ``FrequencyResponse``
    (``Scene.frequency_response_on_receivers_grid``, ``Context.frequency_response``) or any object with ``re`` and ``im``."""
    re = np.asarray(fr.re, dtype=np.float32)
    im = np.asarray(fr.im, dtype=np.float32)
    h = np.empty(re.shape, np.complex64)
    h.real = re
    h.imag = im
    return h


def wideband_power(fr):
    """The frequency-averaged coverage of a ``FrequencyResponse``: the mean over the wavelengths ``j`` of ``re[j]**2 + im[j]**2`` per
    cell, ``[m, n]``.  On the host, in float64.  The cross terms of two paths average out once the band spans many turns of their
    length difference, so with ``amplitude="sqrt"`` it tends to ``total`` as the band widens."""
    re = np.asarray(fr.re, dtype=np.float64)
    im = np.asarray(fr.im, dtype=np.float64)
    return (re * re + im * im).mean(axis=0)


def impulse_response(fr, inv_wavelength_step):
    """The coherent impulse response of a ``FrequencyResponse`` taken on a UNIFORM grid ``inv_wavelength[j] = inv_0 + j * step``:
    ``numpy.fft.ifft`` of ``H`` along the frequency axis.  Returns ``(taps, spacing)``: ``taps`` complex ``[nf, m, n]`` and the tap
    spacing in path length, ``1 / (nf * step)``.  A path of length ``r`` (``H[j] = a * exp(-2j pi r * inv_wavelength[j])``) peaks at
    tap ``round(r * nf * step) mod nf``: path lengths alias with period ``1 / step``.  ``inv_wavelength_step`` is the caller's grid
    spacing (it is not recovered from the result); ``nf < 2`` is refused."""
    h = frequency_response(fr)
    nf = h.shape[0]
    if nf < 2:
        raise ValueError(f"impulse_response needs at least 2 frequencies, got nf={nf}")
    step = float(inv_wavelength_step)
    if not (np.isfinite(step) and step > 0.0):
        raise ValueError(f"impulse_response needs a finite inv_wavelength_step > 0, got {inv_wavelength_step!r}")
    return np.fft.ifft(h, axis=0), 1.0 / (nf * step)


def field_misfit(fr, target, weights=None):
    """The least-squares misfit of a ``FrequencyResponse`` to a measured complex channel, and its cotangents:
    ``L = 1/2 * sum w * |H - target|**2`` over every plane and cell, with ``H = re + 1j * im``.  ``target`` is complex
    ``[nf, m, n]`` (or broadcasts to it), ``weights`` real and non-negative with a shape that broadcasts too (``None``: 1).  Returns
    ``(loss, re_bar, im_bar)``: the loss in float64 and ``d L / d re = w * (re - target.real)``, ``d L / d im = w * (im -
    target.imag)`` as fp32 ``[nf, m, n]`` -- what ``Context.field_coefs_vjp``,
    ``Scene.frequency_response_coefs_vjp_on_receivers_grid`` and ``Context.material_eps_vjp`` take.  On the host, in float64, rounded to fp32 once."""
    re = np.asarray(fr.re, dtype=np.float64)
    im = np.asarray(fr.im, dtype=np.float64)
    t = np.broadcast_to(np.asarray(target, dtype=np.complex128), re.shape)
    w = np.ones(re.shape) if weights is None else np.broadcast_to(np.asarray(weights, dtype=np.float64), re.shape)
    dr, di = re - t.real, im - t.imag
    loss = 0.5 * float(np.sum(w * (dr * dr + di * di)))
    return loss, np.ascontiguousarray(w * dr, dtype=np.float32), np.ascontiguousarray(w * di, dtype=np.float32)


def wideband_power_cotangent(fr, weights=None):
    """The coherent wideband coverage of a ``FrequencyResponse`` as an objective, and its cotangents:
    ``J = sum_cells w * mean_j |H_j|**2`` with ``H = re + 1j * im`` (:func:`wideband_power` summed over the cells), ``weights`` real
    ``[m, n]`` (or a shape that broadcasts to it; ``None``: 1).  Returns ``(objective, re_bar, im_bar)``: ``J`` in float64 and
    ``d J / d re = 2 w re / nf``, ``d J / d im = 2 w im / nf`` as fp32 ``[nf, m, n]`` -- what ``Context.field_position_vjp`` and
    ``Scene.frequency_response_position_vjp_on_receivers_grid`` take: their ``fixed_bar`` is then the direction in which to move the
    transmitter to RAISE the coverage.  On the host, in float64, rounded to fp32 once."""
    re = np.asarray(fr.re, dtype=np.float64)
    im = np.asarray(fr.im, dtype=np.float64)
    nf = re.shape[0]
    w = np.ones(re.shape[1:]) if weights is None else np.broadcast_to(np.asarray(weights, dtype=np.float64), re.shape[1:])
    objective = float(np.sum(w * (re * re + im * im).mean(axis=0)))
    scale = (2.0 / nf) * w
    return objective, np.ascontiguousarray(scale * re, dtype=np.float32), np.ascontiguousarray(scale * im, dtype=np.float32)


VACUUM_PERMITTIVITY = 8.8541878128e-12  # F/m


def complex_permittivity(eps_r, conductivity, frequency_hz):
    """The complex relative permittivity of a material of real relative permittivity ``eps_r`` and conductivity ``sigma`` (S/m) at
    ``frequency_hz``: ``eps_r - 1j * sigma / (2 pi f eps_0)`` with ``eps_0 = 8.8541878128e-12`` F/m.  The sign is the library's time
    convention, ``e^(-j 2 pi r / lambda)``: loss is a NEGATIVE imaginary part, what ``Context.material_response`` takes.  The
    arguments broadcast; complex128."""
    f = np.asarray(frequency_hz, dtype=np.float64)
    loss = np.asarray(conductivity, dtype=np.float64) / (2.0 * np.pi * f * VACUUM_PERMITTIVITY)
    return np.asarray(eps_r, dtype=np.float64) - 1j * loss


def material_parameters_vjp(eps_bar, frequency_hz):
    """The chain rule through :func:`complex_permittivity` for one ``eps_r`` and one conductivity per wall: ``eps_bar`` is the
    per-wavelength gradient ``dL/dRe eps + 1j * dL/dIm eps``, complex ``[nf, N]`` (``Context.material_eps_vjp``,
    ``Scene.material_response_permittivity_vjp_on_receivers_grid`` with a table ``[nf, N]``), ``frequency_hz`` the ``nf``
    frequencies the rows of the table were formed at.  Returns ``(eps_r_bar, conductivity_bar)``, float64 ``[N]`` each:
    ``eps_r_bar = sum_f Re eps_bar`` and ``conductivity_bar = sum_f -Im eps_bar / (2 pi f eps_0)``."""
    bar = np.asarray(eps_bar, dtype=np.complex128)
    f = np.asarray(frequency_hz, dtype=np.float64).reshape(-1)
    if bar.ndim != 2 or bar.shape[0] != f.size:
        raise ValueError(f"material_parameters_vjp needs eps_bar [nf, N] with a row per frequency (nf = {f.size}), got shape {tuple(bar.shape)}")
    return bar.real.sum(axis=0), (-bar.imag / (2.0 * np.pi * f[:, None] * VACUUM_PERMITTIVITY)).sum(axis=0)


def fresnel_coefficient(eps, cos_theta, polarization="te"):
    """The Fresnel reflection coefficient of a half space of complex relative permittivity ``eps`` (``Im eps <= 0`` for a lossy
    medium: the library's time convention) seen from vacuum at the cosine ``cos_theta`` of the angle of incidence, in complex128:
    the reference formula of ``Context.material_response`` (differt2d_amd/csrc/d2d_fresnel.hpp is its fp32 definition), and
    what one plots.  With ``q = sqrt(eps - sin(theta)**2)``, the root with ``Im q <= 0`` (the wave that decays into the wall),

    * ``"te"`` (E perpendicular to the plane of incidence): ``(cos - q) / (cos + q)``;
    * ``"tm"`` (E in the plane of incidence): ``(eps cos - q) / (eps cos + q)``.

    At normal incidence TE is ``(1 - sqrt(eps)) / (1 + sqrt(eps))`` and TM is its negative: the convention that measures TM's
    field by its component along the wall, under which TM tends to +1 and TE to -1 as ``|eps|`` grows.  TM vanishes at the
    Brewster angle, ``cos_theta = 1 / sqrt(1 + eps)`` for real ``eps``; both tend to -1 at grazing incidence.  The arguments
    broadcast."""
    pol = str(polarization).lower()
    if pol not in ("te", "tm"):
        raise ValueError(f"polarization must be 'te' or 'tm', got {polarization!r}")
    eps = np.asarray(eps, dtype=np.complex128)
    c = np.minimum(np.asarray(cos_theta, dtype=np.float64), 1.0)
    q = np.sqrt((eps - 1.0) + c * c)
    # the decaying branch, Im q <= 0: the principal root has it for Im eps <= 0, except +j|q| for a real eps below sin^2 with Im = +0
    q = np.where(q.imag > 0.0, -q, q)
    a = eps * c if pol == "tm" else c + 0j
    with np.errstate(divide="ignore", invalid="ignore"):
        g = (a - q) / (a + q)
    return np.where(a + q == 0, -1.0 + 0j, g)


class AngularStatistics(NamedTuple):
    """Result of :func:`angular_statistics`: float64 ``[m, n]`` each."""

    power: np.ndarray   # the binned power, the sum of the bins
    mean: np.ndarray    # the mean direction in radians, in (-pi, pi], counter-clockwise from +x; NaN where power is 0
    spread: np.ndarray  # the circular spread sqrt(1 - |sum p_b e^(j theta_b)|^2 / (sum p_b)^2), 0 .. 1; NaN where power is 0


def angular_statistics(profile, origin=0.0):
    """The binned power, the mean direction and the angular spread per cell of a ``PowerAngleProfile``
    (``Scene.power_angle_profile_on_receivers_grid``, ``Context.power_angle``) or any object with ``bins`` ``[nbins, m, n]``; ``origin``
    is the profile's, in radians.  From the bin centres ``theta_b = origin + 2 pi (b + 1/2) / nbins``, on the host, in float64: the
    power is ``sum_b bins[b]``, the mean direction the angle of ``sum_b bins[b] e^(j theta_b)``, and the circular spread
    ``sqrt(1 - |sum_b bins[b] e^(j theta_b)|^2 / (sum_b bins[b])^2)`` -- 0 when all power sits in one bin, 1 when it is balanced
    around the circle.  Mean and spread are NaN where the power is 0.  Returns an :class:`AngularStatistics`."""
    bins = np.asarray(profile.bins, dtype=np.float64)
    nbins = bins.shape[0]
    theta = float(origin) + 2.0 * np.pi * (np.arange(nbins, dtype=np.float64) + 0.5) / nbins
    phase = np.exp(1j * theta).reshape((nbins,) + (1,) * (bins.ndim - 1))
    power = bins.sum(axis=0)
    first = (bins * phase).sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        lit = power != 0.0
        mean = np.where(lit, np.angle(first), np.nan)
        spread = np.where(lit, np.sqrt(np.clip(1.0 - np.abs(first) ** 2 / power**2, 0.0, None)), np.nan)
    return AngularStatistics(power, mean, spread)


def pattern_power(profile, gains):
    """The power a directional antenna receives: ``sum_b gains[b] * bins[b]`` per cell, for a ``PowerAngleProfile`` (or any object
    with ``bins`` ``[nbins, m, n]``) and the antenna's power pattern sampled at the bin centres, ``gains[nbins]`` (linear, not dB).  On
    the host, in float64; unit gains give the binned power."""
    bins = np.asarray(profile.bins, dtype=np.float64)
    g = np.asarray(gains, dtype=np.float64).reshape(-1)
    if g.size != bins.shape[0]:
        raise ValueError(f"pattern_power needs one gain per bin, got {g.size} gains for {bins.shape[0]} bins")
    return np.tensordot(g, bins, axes=(0, 0))


def ula(n, spacing, orientation=0.0):
    """The element offsets of a uniform linear array of ``n`` elements ``spacing`` apart (length units), centred on the terminal, along
    the direction ``orientation`` (radians, counter-clockwise from +x): fp32 ``[n, 2]``, element ``k`` at
    ``(k - (n - 1) / 2) * spacing * (cos, sin)(orientation)``.  Computed in float64 and rounded once; what
    ``Scene.array_response_on_receivers_grid`` and ``Context.array_response`` take as ``tx_elements`` / ``rx_elements``."""
    n = int(n)
    if n < 1:
        raise ValueError(f"ula needs n >= 1, got {n}")
    k = (np.arange(n, dtype=np.float64) - (n - 1) / 2.0) * float(spacing)
    return np.stack([k * np.cos(float(orientation)), k * np.sin(float(orientation))], axis=1).astype(np.float32)


def channel_matrix(ar):
    """The complex channel matrix ``H = re + 1j * im``, complex64 ``[nr, nt, m, n]``, of an ``ArrayResponse``
    (``Scene.array_response_on_receivers_grid``, ``Context.array_response``) or any object with ``re`` and ``im``."""
    re = np.asarray(ar.re, dtype=np.float32)
    im = np.asarray(ar.im, dtype=np.float32)
    h = np.empty(re.shape, np.complex64)
    h.real = re
    h.imag = im
    return h


def _cells_last(ar):
    """H of an ArrayResponse as complex128 [..., nr, nt]: the cells in front, one matrix per cell."""
    return np.moveaxis(channel_matrix(ar).astype(np.complex128), (0, 1), (-2, -1))


def beamformed_power(ar, w_rx, w_tx):
    """The power behind two beamformers, ``|w_rx^H H w_tx|**2`` per cell, ``[m, n]``, for an ``ArrayResponse`` and the complex weights
    ``w_rx[nr]`` and ``w_tx[nt]`` (not normalised here).  On the host, in float64 / complex128."""
    h = _cells_last(ar)
    wr = np.asarray(w_rx, dtype=np.complex128).reshape(-1)
    wt = np.asarray(w_tx, dtype=np.complex128).reshape(-1)
    if wr.size != h.shape[-2] or wt.size != h.shape[-1]:
        raise ValueError(f"beamformed_power needs {h.shape[-2]} receive and {h.shape[-1]} transmit weights, got {wr.size} and {wt.size}")
    y = np.einsum("i,...ij,j->...", wr.conj(), h, wt)
    return y.real**2 + y.imag**2


def singular_values(ar):
    """The singular values of every cell's channel matrix, descending: float64 ``[min(nr, nt), m, n]``, for an ``ArrayResponse``.  A
    cell with a non-finite entry gives NaN."""
    h = _cells_last(ar)
    bad = ~np.isfinite(h).all(axis=(-2, -1))
    s = np.linalg.svd(np.where(bad[..., None, None], 0.0, h), compute_uv=False)
    s[bad] = np.nan
    return np.moveaxis(s, -1, 0)


def mimo_capacity(ar, snr):
    """The capacity of every cell's channel with equal power per transmit element and no channel knowledge at the transmitter,
    ``log2 det(I + snr / nt * H H^H)`` in bit/s/Hz, float64 ``[m, n]``, for an ``ArrayResponse``; ``snr`` is linear (not dB), relative
    to the units of ``|H|**2``.  From the singular values: ``sum_k log2(1 + snr / nt * s_k**2)``."""
    s = singular_values(ar)
    nt = np.asarray(ar.re).shape[1]
    return np.log2(1.0 + float(snr) / nt * s * s).sum(axis=0)


def channel_tensor(afr):
    """The complex channel tensor ``H = re + 1j * im``, complex64 ``[nf, nr, nt, m, n]``, of an ``ArrayFrequencyResponse``
    (``Scene.array_frequency_response_on_receivers_grid``, ``Context.array_frequency_response``) or any object with ``re`` and ``im``."""
    return channel_matrix(afr)


def array_response_at(afr, f):
    """Wavelength ``f`` of an ``ArrayFrequencyResponse`` as an ``engine.ArrayResponse`` of views (``re`` and ``im`` ``[nr, nt, m, n]``,
    nothing is copied), so that ``beamformed_power``, ``singular_values`` and ``mimo_capacity`` apply per wavelength unchanged."""
    from .engine import ArrayResponse

    return ArrayResponse(re=afr.re[f], im=afr.im[f], total=afr.total)


def wideband_capacity(afr, snr):
    """The capacity of every cell averaged over the band: the mean over the wavelengths ``f`` of ``mimo_capacity`` of
    ``array_response_at(afr, f)``, float64 ``[m, n]`` in bit/s/Hz, for an ``ArrayFrequencyResponse`` and a linear ``snr``.  NaN where
    any plane of the cell is not finite."""
    nf = np.asarray(afr.re).shape[0]
    acc = mimo_capacity(array_response_at(afr, 0), snr)
    for f in range(1, nf):
        acc = acc + mimo_capacity(array_response_at(afr, f), snr)
    return acc / nf


def steering_weights(elements, angles, wavelength):
    """Matched (conjugate-steering) beam weights of an array: complex64 ``[len(angles), n]``,
    ``w[k, i] = exp(+2j pi e[i] . u(angles[k]) / wavelength) / sqrt(n)`` with ``u(a) = (cos a, sin a)``, for ``elements`` ``[n, 2]``
    (offsets in length units, :func:`ula`) and ``angles`` in radians counter-clockwise from +x.  Computed in float64 and rounded once.

    The same function serves either end of ``y = w_rx^H H w_tx`` (``Context.beam_response``, :func:`beamformed_power`), but ``angle``
    means something else at each.  The receive weights are conjugated by the product, so as ``rx_weights`` the beam points AT
    ``angle``: it is matched to a wave that the receiver sees along ``angle``, the direction from the receiver towards the last
    interaction point (where the wave comes from).  The transmit weights are not conjugated, so as ``tx_weights`` the beam points at
    ``angle + pi``: a transmit beam towards the direction of departure ``d`` (from the transmitter towards the first interaction
    point) is built from ``angle = d + pi``.  With both ends matched to a path, that path contributes ``sqrt(nt * nr)`` times its
    amplitude."""
    e = np.asarray(elements, dtype=np.float64).reshape(-1, 2)
    a = np.asarray(angles, dtype=np.float64).reshape(-1)
    q = np.cos(a)[:, None] * e[None, :, 0] + np.sin(a)[:, None] * e[None, :, 1]
    return (np.exp(2j * np.pi * q / float(wavelength)) / np.sqrt(e.shape[0])).astype(np.complex64)


def beam_response(br):
    """The complex beam-space response ``y = re + 1j * im``, complex64 ``[nf, nbr, nbt, m, n]``, of a ``BeamResponse``
    (``Scene.beam_response_on_receivers_grid``, ``Context.beam_response``) or any object with ``re`` and ``im``."""
    return channel_matrix(br)


def beam_power(br):
    """The power behind every beam pair, ``|y|**2 = re**2 + im**2``, float64 ``[nf, nbr, nbt, m, n]``, for a ``BeamResponse``."""
    re = np.asarray(br.re, dtype=np.float64)
    im = np.asarray(br.im, dtype=np.float64)
    return re * re + im * im


def best_beam(br):
    """The best beam pair of every cell: ``(rx_beam, tx_beam, power)`` with the ``(br, bt)`` of the largest mean of
    :func:`beam_power` over the wavelengths (int64 ``[m, n]`` each) and that mean (float64 ``[m, n]``), for a ``BeamResponse``.  Ties
    go to the lowest flat index ``br * nbt + bt``.  A cell with a non-finite plane gives ``-1``, ``-1`` and NaN."""
    p = beam_power(br)
    nbr, nbt = p.shape[1], p.shape[2]
    bad = ~np.isfinite(p).all(axis=(0, 1, 2))
    mean = np.where(bad, 0.0, p).mean(axis=0).reshape((nbr * nbt,) + p.shape[3:])
    flat = mean.argmax(axis=0)  # (the first of equal maxima)
    power = np.where(bad, np.nan, np.take_along_axis(mean, flat[None], axis=0)[0])
    return np.where(bad, -1, flat // nbt), np.where(bad, -1, flat % nbt), power


received_power._d2d_native = "received_power"
received_power_per_object._d2d_native = "received_power_per_object"
path_length_squared._d2d_native = "length_squared"
path_length_fun._d2d_native = "length"
one._d2d_native = "one"
