"""The oracle of the wideband array response (include/d2d.h: d2d_array_frequency_response_launch): plane block ``f`` is the
array-response recipe ``array_response_oracle.fold`` at ``inv_wavelength[f]``, one fold per entry of the list, stacked -- no new
arithmetic, and nothing of the kernel's chunking is restated here.  ``tests/test_array_frequency_response_cpu.py`` pins its
zero-offset pair to ``frequency_response_oracle``."""

from collections import namedtuple

import numpy as np

from array_response_oracle import directed, fold

F = np.float32

ArrayFrequencyResponse = namedtuple("ArrayFrequencyResponse", "re im total")


def fold_list(T, Rl, D, inv_wavelengths, amplitude, etx, erx):
    """``(re[nf, nr, nt, cells], im[nf, nr, nt, cells], total[cells])`` of contributions ``T[C, cells]`` with lengths ``Rl[C, cells]``
    and end directions ``D[C, cells, 4]``."""
    inv = np.asarray(inv_wavelengths, F).reshape(-1)
    assert inv.size >= 1
    blocks = [fold(T, Rl, D, v, amplitude, etx, erx) for v in inv]
    total = blocks[0][2]
    for b in blocks[1:]:  # (the incoherent sum does not know the wavelength)
        assert np.array_equal(b[2].view(np.uint32), total.view(np.uint32))
    re, im = np.stack([b[0] for b in blocks]), np.stack([b[1] for b in blocks])
    assert re.dtype == im.dtype == total.dtype == F
    return re, im, total


def array_frequency_response(walls, fixed, Xg, Yg, inv_wavelengths, amplitude, etx, erx, **kw):
    """``ArrayFrequencyResponse(re[nf, nr, nt, m, n], im[nf, nr, nt, m, n], total[m, n])``; ``kw`` as for ``contributions``."""
    _, T, Rl, D = directed(walls, fixed, Xg, Yg, **kw)
    re, im, total = fold_list(T, Rl, D, inv_wavelengths, amplitude, etx, erx)
    shape = tuple(np.shape(Xg))
    return ArrayFrequencyResponse(re.reshape(re.shape[:3] + shape), im.reshape(im.shape[:3] + shape), total.reshape(shape))


def guard(re, im):
    """What the comparisons assert of the oracle's planes first, so that a wrong chunk offset or a reused wavelength cannot pass: the
    plane blocks differ pairwise in bits (``re`` and ``im`` both), and more than a third of ``im`` is non-zero."""
    nf = re.shape[0]
    rb = np.ascontiguousarray(re).view(np.uint32).reshape(nf, -1)
    ib = np.ascontiguousarray(im).view(np.uint32).reshape(nf, -1)
    assert np.count_nonzero(im) > im.size // 3, (np.count_nonzero(im), im.size)
    for a in range(nf):
        for b in range(a + 1, nf):
            assert (rb[a] != rb[b]).any() and (ib[a] != ib[b]).any(), (a, b)
