"""The oracle of the channel frequency response (include/d2d.h: d2d_frequency_response_launch): plane ``j`` is the coherent-field
recipe ``coherent_field_oracle.fold`` at ``inv_wavelength[j]``, one fold per entry of the list, stacked -- nothing of the kernel's
chunking is restated here.  ``tests/test_frequency_response_cpu.py`` pins it to ``coherent_field_oracle.coherent_field`` for single
entries."""

from collections import namedtuple

import numpy as np

from coherent_field_oracle import fold, physics
from strongest_paths_oracle import contributions

F = np.float32

FrequencyResponse = namedtuple("FrequencyResponse", "re im total")


def fold_list(T, Rl, inv_wavelengths, amplitude):
    """``(re[nf, cells], im[nf, cells], total[cells])`` of contributions ``T[C, cells]`` with lengths ``Rl[C, cells]``."""
    inv = np.asarray(inv_wavelengths, F).reshape(-1)
    assert inv.size >= 1
    planes = [fold(T, Rl, v, amplitude) for v in inv]
    total = planes[0][2]
    for p in planes[1:]:  # (the incoherent sum does not know the wavelength)
        assert np.array_equal(p[2].view(np.uint32), total.view(np.uint32))
    re, im = np.stack([p[0] for p in planes]), np.stack([p[1] for p in planes])
    assert re.dtype == im.dtype == total.dtype == F
    return re, im, total


def frequency_response(walls, fixed, Xg, Yg, inv_wavelengths, amplitude, **kw):
    """``FrequencyResponse(re[nf, m, n], im[nf, m, n], total[m, n])``; ``kw`` as for ``contributions``."""
    _, T, Rl, total = contributions(walls, fixed, Xg, Yg, **kw)
    re, im, tot = fold_list(T, Rl, inv_wavelengths, amplitude)
    assert np.array_equal(tot.view(np.uint32), total.view(np.uint32))
    shape = tuple(np.shape(Xg))
    return FrequencyResponse(re.reshape((-1,) + shape), im.reshape((-1,) + shape), tot.reshape(shape))


def guard(re, im):
    """What every comparison asserts of the oracle's planes first, so that a wrong chunk offset or a reused wavelength cannot pass:
    all planes differ pairwise in bits, and more than a third of the ``im`` entries of every plane are non-zero."""
    nf = re.shape[0]
    rb = np.ascontiguousarray(re).view(np.uint32).reshape(nf, -1)
    ib = np.ascontiguousarray(im).view(np.uint32).reshape(nf, -1)
    for i in range(nf):
        assert np.count_nonzero(im[i]) > im[i].size // 3, (i, np.count_nonzero(im[i]), im[i].size)
        for j in range(i + 1, nf):
            assert (rb[i] != rb[j]).any() and (ib[i] != ib[j]).any(), (i, j)


def physics_list(T, Rl, inv_wavelengths, amplitude):
    """``(field[nf, cells] complex128, bound[nf, cells])``: ``coherent_field_oracle.physics`` per entry of the list."""
    both = [physics(T, Rl, v, amplitude) for v in np.asarray(inv_wavelengths, F).reshape(-1)]
    return np.stack([b[0] for b in both]), np.stack([b[1] for b in both])


def wideband_physics(T, Rl, inv_wavelengths, amplitude):
    """``(power[cells], bound[cells])``: the float64 mean over the list of ``|field_j|^2`` and what the mean of the fp32 planes'
    ``re^2 + im^2`` may differ from it by.  With ``|got_j - field_j| <= b_j``:  ``||got_j|^2 - |field_j|^2| <= b_j (2 |field_j| +
    b_j)``, and the mean of the bounds bounds the mean (the float64 squares and the mean itself add roundings of 2^-53 relative,
    covered by a factor ``1 + 2^-40``)."""
    field, bound = physics_list(T, Rl, inv_wavelengths, amplitude)
    mag = np.abs(field)
    return (mag * mag).mean(axis=0), (bound * (2 * mag + bound)).mean(axis=0) * (1 + 2.0**-40) + (mag * mag).mean(axis=0) * 2.0**-40
