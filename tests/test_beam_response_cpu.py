"""Host side of the beam-space response (no GPU): ``d2d_beam.hpp``'s arithmetic and the host's parameter and memory checks through a
plain g++ build (ctypes, and a stand-alone program, plain and with sanitizers), the oracle recipe of ``tests/beam_response_oracle.py``
against the frequency response's (one antenna) and the wideband array response's (element space, within the derived bound), its
independence properties, a known answer, ``utils.steering_weights`` / ``beam_power`` / ``best_beam`` on hand-made planes, the
bindings and the ``Scene`` methods' refusals."""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import array_frequency_response_oracle as AFO
import beam_response_oracle as BO
import frequency_response_oracle as FRO
from array_response_oracle import AMP_LINEAR, AMP_SQRT, unit_dir
from conftest import unit_grid
from test_gpu_power_angle import _directed
from test_gpu_strongest_paths import _case, _contributions

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "beam_response_host.cpp")
GXX = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror"]
WL = F(0.05)
INV_LIST = np.array([F(1) / WL, 7.0, 0.0, 12.5], F)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _elements(n, seed):
    """The element lists of tests/test_gpu_array_frequency_response.py (the same seeds)."""
    rng = np.random.default_rng(seed)
    r = rng.uniform(0.1, 2.0, n) * float(WL)
    th = rng.uniform(0, 2 * np.pi, n)
    e = np.stack([r * np.cos(th), r * np.sin(th)], axis=1).astype(F)
    e[0] = 0
    return e


def _codebook(nb, n, seed, zero=None, one_hot=None):
    """``nb`` beams of seeded complex weights over ``n`` elements; beam ``zero`` all zero, beam ``one_hot`` 1 at one element."""
    rng = np.random.default_rng(seed)
    w = (rng.normal(size=(nb, n)) + 1j * rng.normal(size=(nb, n))).astype(np.complex64)
    if zero is not None:
        w[zero] = 0
    if one_hot is not None:
        w[one_hot] = 0
        w[one_hot, n // 2] = 1
    return w


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """d2d_beam.hpp and d2d_host.hpp's beam checks, compiled for the host (tests/native/beam_response_host.cpp)."""
    so = str(tmp_path_factory.mktemp("beam_host") / "libbeam_host.so")
    subprocess.check_call(GXX + ["-shared", "-fPIC", "-o", so, SRC])
    lib = C.CDLL(so)
    lib.beam_arith.argtypes = [C.c_void_p] * 9 + [C.c_longlong] + [C.c_void_p] * 8
    lib.beam_arith.restype = None
    lib.beam_params.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                C.POINTER(C.c_int), C.c_char_p, C.c_int]
    lib.beam_params.restype = C.c_int
    lib.beam_bytes_per_cell.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.beam_bytes_per_cell.restype = C.c_longlong
    lib.beam_fits.argtypes = [C.c_ulonglong, C.c_int, C.c_int, C.c_int, C.c_ulonglong, C.c_ulonglong]
    lib.beam_fits.restype = C.c_int
    lib.beam_chunk_size.restype = C.c_int
    lib.beam_max.restype = C.c_int
    return lib


# ---- the header's arithmetic ---------------------------------------------------------------------------------------------------------
def test_header_arithmetic_equals_the_numpy_restatement_by_bits(host):
    """steer, the two folds and the pair product on seeded random inputs and on the specials: q * inv just below an integer, exact
    quarter turns, +-0 offsets, NaN and inf (NaN results compare as NaN: their payload is not part of the definition)."""
    q, inv, w_re, w_im, a_re, a_im, b_re, b_im, f0 = BO.beam_inputs()
    n = q.size
    out = [np.empty(n, F) for _ in range(8)]
    host.beam_arith(*(x.ctypes.data for x in (q, inv, w_re, w_im, a_re, a_im, b_re, b_im, f0)), n, *(x.ctypes.data for x in out))
    c, s = BO.steer(q, inv)
    want = [c, s]
    with np.errstate(all="ignore"):
        # the folds take the weight of one step as a scalar: element by element here
        rc, i_s, rs, ic = w_re * c, w_im * s, w_re * s, w_im * c
        want += [a_re + (rc - i_s), a_im + (rs + ic), a_re + (rc + i_s), a_im + (rs - ic)]
    want += list(BO.pair(a_re, a_im, b_re, b_im, *BO.phasor(f0)))
    assert n > 60000 and np.isnan(c).any() and (c == 1).any()
    for name, g, w in zip(("c", "s", "tx_re", "tx_im", "rx_re", "rx_im", "zr", "zs"), out, want):
        assert w.dtype == F
        nan = np.isnan(w)
        assert np.array_equal(np.isnan(g), nan), name
        bad = (_bits(g) != _bits(w)) & ~nan
        assert not bad.any(), (name, int(bad.sum()), int(np.flatnonzero(bad)[0]))
    # the scalar folds of the oracle are the same expressions
    k = 12345
    assert all(np.array_equal(_bits(x), _bits(y[k])) for x, y in zip(BO.fold_tx(a_re[k], a_im[k], w_re[k], w_im[k], c[k], s[k]), want[2:4]))
    assert all(np.array_equal(_bits(x), _bits(y[k])) for x, y in zip(BO.fold_rx(a_re[k], a_im[k], w_re[k], w_im[k], c[k], s[k]), want[4:6]))


def test_steer_at_the_special_points():
    one, zero = F(1).view(np.uint32), F(0).view(np.uint32)
    for q in (0.0, -0.0):
        for inv in (0.0, 20.0, 3e38):
            c, s = BO.steer(F(q), F(inv))
            assert c.view(np.uint32) == one and s.view(np.uint32) == zero  # (1, +0) by bits
    c, s = BO.steer(F(-1e-9), F(1))  # g rounds to 1 and is taken to 0
    assert c.view(np.uint32) == one and s.view(np.uint32) == zero
    c, s = BO.steer(np.nextafter(F(3), F(0)), F(1))
    assert 0.999 < c <= 1 and -1e-5 < s < 0
    c, s = BO.steer(F(0.25), F(1))
    assert c == 0 and np.signbit(c) and s == 1
    # accuracy against float64 on ordinary inputs: the phase rounding plus the phasor's 2 * 2^-24
    rng = np.random.default_rng(5)
    q, inv = rng.uniform(-0.2, 0.2, 4096).astype(F), rng.uniform(5, 40, 4096).astype(F)
    c, s = BO.steer(q, inv)
    v = q.astype(np.float64) * inv.astype(np.float64)
    err = np.abs((c + 1j * s) - np.exp(2j * np.pi * v))
    assert (err <= 2 * np.pi * np.spacing(np.abs(q * inv)) + 4 * 2.0**-24).all()


# ---- parameter checks ----------------------------------------------------------------------------------------------------------------
def _params(host, inv, tx, rx, wtx, wrx, amp=0, nbt=None, nbr=None):
    arr = [None if a is None else np.ascontiguousarray(a, F) for a in (inv, tx, rx)]
    wt = None if wtx is None else np.ascontiguousarray(wtx, np.complex64)
    wr = None if wrx is None else np.ascontiguousarray(wrx, np.complex64)
    nbt = wt.shape[0] if nbt is None else nbt
    nbr = wr.shape[0] if nbr is None else nbr
    at = C.c_int(0)
    msg = C.create_string_buffer(256)
    rc = host.beam_params(arr[0].ctypes.data, arr[0].size, amp, arr[1].size // 2, arr[1].ctypes.data, arr[2].size // 2, arr[2].ctypes.data, nbt,
                          None if wt is None else wt.ctypes.data, nbr, None if wr is None else wr.ctypes.data, C.byref(at), msg, 256)
    return rc, at.value, msg.value.decode()


def test_beam_params_refusals_in_order(host):
    inv = np.array([20.0, 5.0, 0.0], F)
    tx, rx = _elements(4, 3), _elements(3, 4)
    wtx, wrx = _codebook(3, 4, 1, zero=1), _codebook(2, 3, 2, one_hot=0)
    assert _params(host, inv, tx, rx, wtx, wrx)[:2] == (0, -1) and _params(host, inv, tx, rx, wtx, wrx, 1)[:2] == (0, -1)
    assert host.beam_max() == 8
    assert _params(host, inv, tx, rx, _codebook(8, 4, 3), _codebook(8, 3, 4))[:2] == (0, -1)
    # what the wideband array response refuses comes first: the tables are not read (NULL)
    bad_inv = inv.copy()
    bad_inv[1] = np.nan
    rc, at, msg = _params(host, bad_inv, tx, rx, None, None, nbt=0, nbr=0)
    assert (rc, at) == (-1, 1) and "inv_wavelength" in msg
    rc, at, msg = _params(host, inv, np.zeros((9, 2), F), rx, None, None, nbt=0, nbr=0)
    assert rc == -1 and "nt in 1 .. 8" in msg
    rc, at, msg = _params(host, inv, tx, rx, None, None, amp=2, nbt=0, nbr=0)
    assert rc == -1 and "amplitude" in msg
    # the counts: nbt before nbr, neither table read
    for bad in (0, -1, 9, 2**30, -(2**30)):
        rc, at, msg = _params(host, inv, tx, rx, None, None, nbt=bad, nbr=bad)
        assert (rc, at) == (-1, -1) and "the beam response needs nbt in 1 .. 8" in msg and msg.endswith(f"got {bad}")
        rc, at, msg = _params(host, inv, tx, rx, None, None, nbt=1, nbr=bad)
        assert (rc, at) == (-1, -1) and "the beam response needs nbr in 1 .. 8" in msg and msg.endswith(f"got {bad}")
    # every position of both tables: the table, the beam and the part named, the element's index at the end
    for value in (np.nan, np.inf, -np.inf):
        for k in range(2 * wtx.size):
            w = wtx.copy()
            w.view(F).reshape(-1)[k] = value
            rc, at, msg = _params(host, inv, tx, rx, w, wrx)
            assert (rc, at) == (-1, k // 2 % 4) and f"tx_weights of beam {k // 8} " in msg and ("im" if k % 2 else "re") in msg
        for k in range(2 * wrx.size):
            w = wrx.copy()
            w.view(F).reshape(-1)[k] = value
            rc, at, msg = _params(host, inv, tx, rx, wtx, w)
            assert (rc, at) == (-1, k // 2 % 3) and f"rx_weights of beam {k // 6} " in msg
    both = wtx.copy()
    both[2, 3] = np.nan
    bad_rx = wrx.copy()
    bad_rx[0, 0] = np.inf
    assert "tx_weights" in _params(host, inv, tx, rx, both, bad_rx)[2]  # the transmit table first


def test_beam_fits_at_the_boundary_byte_and_with_sizes_that_would_wrap(host):
    assert [host.beam_bytes_per_cell(*p) for p in ((1, 1, 1), (9, 3, 2), (64, 1, 1), (64, 8, 8), (1024, 8, 8))] == [12, 436, 516, 32772, 524292]
    top = 2**64 - 1
    for mem_free in (0, 2**20, 288 * 2**30, top):
        for held in (0, 5 * 2**30, top):
            for nf, nbt, nbr in ((1, 1, 1), (9, 3, 2), (64, 8, 8), (1024, 8, 8)):
                per = 8 * nf * nbt * nbr + 4
                edge = (mem_free // 2 + held // 2) // per
                assert host.beam_fits(edge, nf, nbt, nbr, mem_free, held) == 1 and host.beam_fits(edge + 1, nf, nbt, nbr, mem_free, held) == 0
    assert host.beam_fits(2**20, 64, 1, 1, 2 * 516 * 2**20, 0) == 1 and host.beam_fits(2**20, 64, 1, 1, 2 * 516 * 2**20 - 2, 0) == 0
    assert host.beam_fits(top // 524292 + 2, 1024, 8, 8, 288 * 2**30, 0) == 0 and host.beam_fits(top, 1024, 8, 8, 288 * 2**30, 0) == 0
    for bad in (0, -1, 9, 2**30):
        assert host.beam_fits(1, 1, bad, 1, top, top) == 0 and host.beam_fits(1, 1, 1, bad, top, top) == 0
    assert host.beam_chunk_size() in (8, 16, 32, 64)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_stand_alone_host_program(tmp_path, sanitize):
    """The header's arithmetic, beam_params, the memory rule (refusals included) and the chunk plan in a program of their own; with
    sanitizers it is the same program, linked against the sanitizers' run times by the compiler (nothing is preloaded, nothing is
    loaded into Python)."""
    exe = str(tmp_path / "beam_host")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(GXX + extra + ["-DBEAM_MAIN", "-o", exe, SRC])
    done = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(done.stdout)
    assert done.returncode == 0, done.stdout
    assert "beam_response_host: 0 failures" in done.stdout


# ---- the oracle recipe ---------------------------------------------------------------------------------------------------------------
def _joined(scene, mode, role, lo=0, hi=2):
    _, T, Rl, _ = _contributions(scene, mode, role, "received_power", lo, hi)
    _, T2, D = _directed(scene, mode, role, "received_power", lo, hi)
    assert np.array_equal(T.view(np.uint32), T2.view(np.uint32))  # the two oracles' contributions agree in bits
    return T, Rl, D


@pytest.mark.parametrize("amp", [AMP_SQRT, AMP_LINEAR], ids=["sqrt", "linear"])
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
@pytest.mark.parametrize("scene", ["random7", "obstacle", "square_centre"])
def test_one_antenna_is_the_frequency_response_recipe_by_bits(scene, mode, role, amp):
    """nt = nr = nbt = nbr = 1, offsets (+-0, +-0), weights (1, 0): the frequency response BIT FOR BIT (signs of zero do not survive
    the accumulation) wherever no contribution lacks a direction: every cell of random7 and obstacle; in square_centre the line of
    sight of the cell that IS the fixed end point has none, and exactly [4, 4] differs."""
    T, Rl, D = _joined(scene, mode, role)
    assert np.isfinite(T).all()
    fre, fim, ftotal = FRO.fold_list(T, Rl, INV_LIST, amp)
    shape = _case(scene)[2].shape
    _, _, okt = unit_dir(D[:, :, 0], D[:, :, 1])
    _, _, okr = unit_dir(D[:, :, 2], D[:, :, 3])
    lacking = ((T != 0) & ~(okt & okr)).any(axis=0).reshape(shape)
    assert np.argwhere(lacking).tolist() == ([[4, 4]] if scene == "square_centre" else [])
    assert np.count_nonzero(fim) > fim.size // 3
    for etx, erx in (([[0.0, -0.0]], [[-0.0, 0.0]]), ([[-0.0, -0.0]], [[0.0, 0.0]])):
        re, im, total = BO.fold_list(T, Rl, D, INV_LIST, amp, np.array(etx, F), np.array(erx, F), [1 + 0j], [[1 + 0j]])
        assert re.shape == (4, 1, 1, T.shape[1]) and np.array_equal(_bits(total), _bits(ftotal))
        diff = (_bits(re[:, 0, 0]) != _bits(fre)) | (_bits(im[:, 0, 0]) != _bits(fim))
        for f in range(INV_LIST.size):
            assert np.argwhere(diff[f].reshape(shape)).tolist() == ([[4, 4]] if scene == "square_centre" else []), f
    # any other weight is not the frequency response
    re2, im2, _ = BO.fold_list(T, Rl, D, INV_LIST, amp, np.zeros((1, 2), F), np.zeros((1, 2), F), [0.6 - 0.8j], [1 + 0j])
    assert not np.array_equal(_bits(im2[:, 0, 0]), _bits(fim))


SHAPES = {"3x4": (_elements(4, 3), _elements(3, 4)), "8x8": (_elements(8, 5), _elements(8, 6))}
BOOKS = {"3x4": (_codebook(3, 4, 11, zero=1), _codebook(2, 3, 12, one_hot=0)), "8x8": (_codebook(8, 8, 13, zero=6), _codebook(8, 8, 14, one_hot=3))}


@pytest.mark.parametrize("amp", [AMP_SQRT, AMP_LINEAR], ids=["sqrt", "linear"])
@pytest.mark.parametrize("role", ["rx", "tx"])
@pytest.mark.parametrize("mode", ["hard", "hsig"])
@pytest.mark.parametrize("scene,shape", [("random7", "3x4"), ("obstacle", "3x4"), ("square_centre", "3x4"), ("random7", "8x8")])
def test_element_space_bound_between_the_two_oracles(scene, shape, mode, role, amp):
    """The beam planes against the float64 contraction of the wideband array response's planes, both from NumPy: inside the derived
    bound in every cell, plane and wavelength -- and not equal in bits, which is why the bound exists."""
    T, Rl, D = _joined(scene, mode, role)
    etx, erx = SHAPES[shape]
    wtx, wrx = BOOKS[shape]
    re, im, total = BO.fold_list(T, Rl, D, INV_LIST, amp, etx, erx, wtx, wrx)
    hre, him, htotal = AFO.fold_list(T, Rl, D, INV_LIST, amp, etx, erx)
    assert np.array_equal(_bits(total), _bits(htotal))
    y = BO.contract(hre, him, wtx, wrx)
    bnd = BO.bound(T, Rl, D, INV_LIST, amp, etx, erx, wtx, wrx)
    assert y.shape == bnd.shape == re.shape and np.isfinite(bnd).all()
    err = np.abs((re.astype(np.float64) + 1j * im.astype(np.float64)) - y)
    lit = bnd > 0
    ratio = float((err[lit] / bnd[lit]).max())
    print(f"{scene} {shape} {mode} {role} amp={amp}: max error / bound = {ratio:.4f}, max error = {err.max():.3e}, max |y| = {np.abs(y).max():.3e}")
    assert (err <= bnd).all() and not err[~lit].any()
    assert ratio > 1e-4  # (the bound is not vacuous: the planes are not the contraction's bits)
    # the bound is small against the signal where there is one
    assert np.median(bnd[lit]) < 1e-3 * np.abs(y).max()
    # a zero beam gives +0.0 by bits, a one-hot receive beam is the conjugate-free row of H contracted with the transmit beams
    zero_bt = 1 if shape == "3x4" else 6
    assert not _bits(re[:, :, zero_bt]).any() and not _bits(im[:, :, zero_bt]).any()


def test_independence_under_permuted_duplicated_and_truncated_lists():
    T, Rl, D = _joined("random7", "hsig", "rx")
    etx, erx = SHAPES["3x4"]
    wtx, wrx = _codebook(3, 4, 21), _codebook(2, 3, 22)
    base = BO.fold_list(T, Rl, D, INV_LIST, AMP_SQRT, etx, erx, wtx, wrx)
    BO.guard(base[0][[0, 1, 3]], base[1][[0, 1, 3]])  # (the entry 0 has no phase of its own in the elements)
    pf, pt, pr = [2, 0, 3, 1], [2, 0, 1], [1, 0]
    perm = BO.fold_list(T, Rl, D, INV_LIST[pf], AMP_SQRT, etx, erx, wtx[pt], wrx[pr])
    for k in (0, 1):
        assert np.array_equal(_bits(perm[k]), _bits(base[k][pf][:, pr][:, :, pt]))
    dup = BO.fold_list(T, Rl, D, INV_LIST[[1, 1]], AMP_SQRT, etx, erx, wtx[[0, 2, 0]], wrx[[1, 1]])
    for k in (0, 1):
        assert np.array_equal(_bits(dup[k]), _bits(base[k][[1, 1]][:, [1, 1]][:, :, [0, 2, 0]]))
    cut = BO.fold_list(T, Rl, D, INV_LIST[:2], AMP_SQRT, etx, erx, wtx[:1], wrx[:1])
    for k in (0, 1):
        assert np.array_equal(_bits(cut[k]), _bits(base[k][:2, :1, :1]))
    # the element order IS part of the definition: permuting elements and weights together changes bits somewhere (a left fold)
    pe = [3, 1, 0, 2]
    moved = BO.fold_list(T, Rl, D, INV_LIST, AMP_SQRT, etx[pe], erx, wtx[:, pe], wrx)
    assert not np.array_equal(_bits(moved[0]), _bits(base[0])) and np.allclose(moved[0], base[0], atol=1e-4)


def test_known_answer_matched_beams_on_a_single_path():
    """Orders 0..0 on a scene whose walls block nothing: every cell has exactly one path, its line of sight.  With steering_weights
    aimed along that cell's own line of sight at both ends, |y|^2 = nt * nr * |t| at that cell within the bound; with any other beam
    it is no larger."""
    from differt2d_amd.utils import steering_weights, ula

    walls, fixed, X, Y = _case("square_centre")
    T, Rl, D = _joined("square_centre", "hard", "rx", 0, 0)
    assert T.shape[0] == 1
    shape = X.shape
    lit = (T[0] != 0) & unit_dir(D[0, :, 0], D[0, :, 1])[2]
    assert lit.sum() == 48  # (the cells on the walls have no valid path, the centre cell's has no direction)
    nt, nr = 4, 3
    etx, erx = ula(nt, float(WL) / 2), ula(nr, float(WL) / 2, np.pi / 3)
    inv = np.array([F(1) / WL], F)
    cells = [(1, 2), (7, 3), (2, 7), (6, 5)]
    assert all(lit.reshape(shape)[c] for c in cells)
    dep = np.arctan2(D[0, :, 1].astype(np.float64), D[0, :, 0].astype(np.float64)).reshape(shape)  # departure, from the transmitter
    arr = np.arctan2(D[0, :, 3].astype(np.float64), D[0, :, 2].astype(np.float64)).reshape(shape)  # arrival, from the receiver
    wtx = steering_weights(etx, [dep[c] + np.pi for c in cells], WL)  # a transmit beam towards d is built from d + pi
    wrx = steering_weights(erx, [arr[c] for c in cells], WL)
    assert wtx.shape == (4, nt) and wrx.shape == (4, nr) and wtx.dtype == np.complex64
    re, im, total = BO.fold_list(T, Rl, D, inv, AMP_SQRT, etx, erx, wtx, wrx)
    bnd = BO.bound(T, Rl, D, inv, AMP_SQRT, etx, erx, wtx, wrx)[0].reshape((4, 4) + shape)
    power = (re.astype(np.float64) ** 2 + im.astype(np.float64) ** 2)[0].reshape((4, 4) + shape)
    t = np.abs(T[0].astype(np.float64)).reshape(shape)
    for k, c in enumerate(cells):
        peak = nt * nr * t[c]
        amp = np.sqrt(peak)
        # the weights are rounded to complex64: 2^-24 relative per element on top of the arithmetic's bound
        slack = bnd[k, k][c] + amp * 4 * 2.0**-24
        assert abs(np.sqrt(power[k, k][c]) - amp) <= slack, (c, power[k, k][c], peak)
        for br in range(4):
            for bt in range(4):
                assert np.sqrt(power[br, bt][c]) <= amp + slack * 4, (c, br, bt)
        assert power[k, k][c] > 0.5 * peak and peak > 0
    # and an unmatched pair is well below the peak somewhere
    assert power[0, 1][cells[0]] < 0.9 * nt * nr * t[cells[0]]


def test_recipe_from_the_walls_on_a_grid_of_its_own():
    walls, fixed, _, _ = _case("random7")
    X, Y = unit_grid(7, 5)
    kw = dict(min_order=0, max_order=2, approx=True, function="hard_sigmoid")
    etx, erx = SHAPES["3x4"]
    wtx, wrx = BOOKS["3x4"]
    br = BO.beam_response(walls, fixed, X, Y, INV_LIST[:3], AMP_SQRT, etx, erx, wtx, wrx, **kw)
    afr = AFO.array_frequency_response(walls, fixed, X, Y, INV_LIST[:3], AMP_SQRT, etx, erx, **kw)
    assert br.re.shape == br.im.shape == (3, 2, 3, 5, 7) and np.array_equal(_bits(br.total), _bits(afr.total))
    y = BO.contract(afr.re, afr.im, wtx, wrx)
    assert np.allclose(br.re + 1j * br.im, y, atol=1e-4) and np.abs(y).max() > 0.1


# ---- utils ---------------------------------------------------------------------------------------------------------------------------
def test_steering_weights_against_closed_forms():
    from differt2d_amd.utils import steering_weights, ula

    e = ula(4, 0.025)
    w = steering_weights(e, [0.0, np.pi / 2, np.pi / 3], 0.05)
    assert w.dtype == np.complex64 and w.shape == (3, 4)
    assert np.allclose(np.abs(w), 0.5, atol=1e-7)  # 1 / sqrt(n)
    # a half-wavelength ULA along x: broadside (pi / 2) has equal phases, end-fire (0) alternates by pi
    assert np.allclose(w[1], 0.5, atol=1e-6)
    assert np.allclose(w[0] / w[0, 0], [1, -1, 1, -1], atol=1e-5)
    q = e.astype(np.float64) @ np.array([np.cos(np.pi / 3), np.sin(np.pi / 3)])
    assert np.array_equal(w[2], (np.exp(2j * np.pi * q / 0.05) / 2).astype(np.complex64))  # float64, rounded once
    # matched: conj(w) . s = sqrt(n) for the steering vector of the same angle; angle + pi is its conjugate
    s = np.exp(2j * np.pi * q / 0.05)
    assert abs(np.vdot(w[2], s) - 2.0) < 1e-6
    assert np.allclose(steering_weights(e, [np.pi / 3 + np.pi], 0.05)[0], w[2].conj(), atol=1e-6)
    assert steering_weights(e[:1], 0.3, 0.05).shape == (1, 1) and steering_weights(e, [], 0.05).shape == (0, 4)


def test_beam_power_and_best_beam_on_hand_made_planes():
    from differt2d_amd.engine import BeamResponse
    from differt2d_amd.utils import beam_power, beam_response, best_beam

    rng = np.random.default_rng(7)
    nf, nbr, nbt, shape = 3, 2, 3, (2, 4)
    re = rng.normal(size=(nf, nbr, nbt) + shape).astype(F)
    im = rng.normal(size=(nf, nbr, nbt) + shape).astype(F)
    # cell (0, 0): a tie between flat indices 1 and 4 (both the largest); cell (0, 1): all zero; cell (1, 2): NaN; cell (1, 3): inf
    re[:, :, :, 0, 0], im[:, :, :, 0, 0] = 0.5, 0.0
    re[:, 0, 1, 0, 0] = re[:, 1, 1, 0, 0] = 3.0
    re[:, :, :, 0, 1] = im[:, :, :, 0, 1] = 0.0
    im[1, 1, 0, 1, 2] = np.nan
    re[2, 0, 2, 1, 3] = np.inf
    br = BeamResponse(re, im, np.zeros(shape, F))
    y = beam_response(br)
    assert y.dtype == np.complex64 and y.shape == re.shape and np.array_equal(y.real, re) and np.array_equal(y.imag[0], im[0])
    p = beam_power(br)
    assert p.dtype == np.float64 and p.shape == re.shape
    ok = np.isfinite(re) & np.isfinite(im)
    assert np.array_equal(p[ok], re[ok].astype(np.float64) ** 2 + im[ok].astype(np.float64) ** 2)
    rx, tx, power = best_beam(br)
    assert rx.shape == tx.shape == power.shape == shape and power.dtype == np.float64 and rx.dtype.kind == "i"
    assert (rx[0, 0], tx[0, 0], power[0, 0]) == (0, 1, 9.0)  # the tie goes to the lowest flat index
    assert (rx[0, 1], tx[0, 1], power[0, 1]) == (0, 0, 0.0)
    for cell in ((1, 2), (1, 3)):
        assert rx[cell] == -1 and tx[cell] == -1 and np.isnan(power[cell])
    assert np.isnan(power).sum() == 2
    mean = p.mean(axis=0)
    for cell in ((0, 2), (0, 3), (1, 0), (1, 1)):
        flat = int(np.argmax(mean[(slice(None), slice(None)) + cell].reshape(-1)))
        assert (rx[cell], tx[cell]) == (flat // nbt, flat % nbt) and power[cell] == mean[(flat // nbt, flat % nbt) + cell]


# ---- bindings --------------------------------------------------------------------------------------------------------------------------
def test_bindings_and_abi_version():
    from differt2d_amd import _lib as L
    from differt2d_amd import utils
    from differt2d_amd.engine import BeamResponse, Context
    from differt2d_amd.scene import Scene

    assert L.D2D_ABI_VERSION == 12 and L.D2D_BEAM_MAX == 8 and BO.BEAM_MAX == 8
    names = [s[0] for s in L.SYMBOLS]
    assert "d2d_beam_response_launch" in names and "d2d_get_beam_response" in names
    assert callable(Context.beam_response) and callable(Context.launch_beam_response) and callable(Context.get_beam_response)
    assert callable(Scene.beam_response_on_receivers_grid) and callable(Scene.beam_response_on_transmitters_grid)
    assert BeamResponse._fields == BO.BeamResponse._fields == ("re", "im", "total")
    assert all(callable(getattr(utils, n)) for n in ("steering_weights", "beam_response", "beam_power", "best_beam"))
    header = open(os.path.join(ROOT, "include", "d2d.h")).read()
    assert "#define D2D_ABI_VERSION 12" in header and "#define D2D_BEAM_MAX 8" in header
    assert "int d2d_beam_response_launch(" in header and "int d2d_get_beam_response(" in header
    lib = L.load()  # the library has both
    assert lib.d2d_beam_response_launch and lib.d2d_get_beam_response and lib.d2d_abi_version() == 12


def test_scene_refuses_a_fun_that_is_not_fused_and_names_both_routes():
    from differt2d_amd import _lib as L
    from differt2d_amd.scene import Scene
    from differt2d_amd.utils import steering_weights, ula

    scene = Scene.square_scene_with_obstacle()
    X, Y = unit_grid(4, 3)

    def step(tx, rx, path, objs):
        return (path.length() < 1.0).astype(F)

    e2 = ula(2, 0.025)
    w2 = steering_weights(e2, [0.0, 1.0], 0.05)
    common = dict(tx_elements=e2, rx_elements=e2, tx_weights=w2, rx_weights=w2[0])
    for method in (scene.beam_response_on_receivers_grid, scene.beam_response_on_transmitters_grid):
        with pytest.raises(L.D2DUnsupported, match="valid_paths") as e:
            next(iter(method(X, Y, step, wavelengths=[0.05, 0.06], **common)))
        assert "trace_paths" in str(e.value) and "beam response" in str(e.value)
        # exactly one of the two wavelength arguments
        with pytest.raises(ValueError, match="exactly one"):
            method(X, Y, step, **common)
        with pytest.raises(ValueError, match="exactly one"):
            method(X, Y, step, wavelengths=[0.05], inv_wavelengths=[20.0], **common)


def test_context_refuses_weight_tables_of_the_wrong_shape():
    from differt2d_amd import _lib as L
    from differt2d_amd.engine import _beam_weights

    assert _beam_weights("tx_weights", [1, 1j, -1], 3).shape == (1, 3) and _beam_weights("tx_weights", np.ones((2, 3)), 3).dtype == np.complex64
    assert _beam_weights("tx_weights", np.zeros((0, 3)), 3).shape == (0, 3)
    for bad in (np.ones((2, 4)), np.ones(4), np.ones((2, 3, 1)), 1.0):
        with pytest.raises(L.D2DError, match="rx_weights"):
            _beam_weights("rx_weights", bad, 3)
